"""Inputs and expected values for the three entry points of the MSE scale (a14, csrc/mse_scale.hip):

  mi355q_mse_scale_f32      mse_scale_balanced_kernel | mse_scale_leaves_kernel
  mi355q_mse_scale_nd_f32   outer == 1: the entry above; channels == 1: the entry above on one unit of outer * inner
                            elements; inner == 1: mse_scale_cols_kernel; else mse_scale_seg_kernel
  mi355q_mse_requant_f32    mse_scale_balanced_kernel with the fused quantize, or the scale entry and then
                            mi355q_quantize_f32 (length no multiple of 4, chunk tree not complete, x not 16-byte aligned,
                            q_out not 4-byte aligned, MI355Q_MSE_TWO_KERNELS)

No GPU and no torch are needed here. Every expected value has two restatements:

  * reference_*: the reference's own expression, `multiplier * np.sqrt(np.mean(x**2, axis=dims, keepdims=True))` in
    float32 (ref mse.py:100-109), and oracle.aeq_oracle.uniform_quantize with a zero zero point for the integers (a
    narrow bound below 8 bits, which the oracle's signature cannot ask for, is the same clip(rint(x / scale + zp))
    written out). This is what the GPU is held to, bit for bit.
  * model_*: the additions spelled out with no NumPy reduction: 8192-element chunks added in order, each by the pairwise
    recursion with splits rounded down to a multiple of 8, leaves of at most 128 elements as eight strided accumulators
    combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and then the leaf tail; a left-to-right loop over rows for the
    [outer, channels] view; one running total per channel that takes each segment's chunks in order for the
    [outer, channels, inner] view; and for a tensor of ONE channel, whose axes NumPy merges, the contiguous vector of
    outer * inner elements (chunks of 8192 run across the segments). Products are rounded to float32 before they are added, the mean is a float32 division
    by float32(count). The tree is walked once per case with arrays over the units.
    test_mse_route_cases_host.py asserts that both agree on every case; the model exists so that it can be MUTATED
    (MUTATIONS): each mutation is a way a kernel could be subtly wrong, and the host test proves that every case whose
    features a mutation attacks shows it in at least one expected scale or integer.

route() restates the host's choice of kernels (the three extern "C" functions, balanced_chunk of common.h) and names the
features of a call; REQUIRED lists the features the case list has to reach.

Five kinds of input, by unit:
  wide       normal * exp(4 normal) as float32, the last chunk of several and the tail of the last leaf made as heavy as
             what comes before them: the order of every addition shows.
  squares    magnitudes from float32 denormals up to 3e19: a square underflows or overflows float32 (scales 0 and inf).
  signs      -0.0, an all-zero unit (scale 0: x / 0), a unit of -0.0, one outlier that makes everything else round to 0.
  nonfinite  +inf, -inf and NaN in the first leaf, the last leaf, a leaf tail and the last chunk.
  ties       (the fused entry only) normal data in which x / scale is exactly k + 0.5 at planted elements, k even and
             odd, of either sign: rounding ties to even differs from rounding them away, and from x * (1 / scale)."""
import dataclasses
import functools

import numpy as np

from oracle import aeq_oracle as O

F = np.float32
CHUNK = 8192          # NumPy's reduction buffer: 8192-element chunks are added in order, each pairwise
LEAF = 128            # pairwise_sum's unrolled block
COLS_UNROLL = 8       # mse_scale_cols_kernel: rows per unrolled step
COLS_BLOCK = 256      # and its channels per block
MULS = (0.05408, 0.37755)        # mse.py's multipliers for 8 and for 4 bits
TIES_MUL = 0.4375                # the ties kind: any multiplier is as good, the entry takes it as an argument


# ------------------------------------------------------------------------------------------------ routes
def balanced_chunk(n):
  """common.h: (leaf, depth) when n = leaf << depth with leaf <= 128 a multiple of 8, else None."""
  d = 0
  while (n >> d) > LEAF:
    d += 1
  leaf = n >> d
  if (leaf << d) != n or leaf < 8 or leaf % 8:
    return None
  return leaf, d


def pairwise_leaves(lo, n, round8=True):
  """The leaves (lo, n) of pairwise_sum's recursion, in order."""
  if n <= LEAF:
    return [(lo, n)]
  n2 = n // 2
  if round8:
    n2 -= n2 % 8
  return pairwise_leaves(lo, n2, round8) + pairwise_leaves(lo + n2, n - n2, round8)


def _contiguous(units, n):
  """mi355q_mse_scale_f32: kernel and features of `units` contiguous units of n elements."""
  feats = {("units%4", units % 4)}
  if units == 1:
    feats.add(("units", 1))
  chunks = -(-n // CHUNK)
  last = n - (n - 1) // CHUNK * CHUNK
  bal = balanced_chunk(last)
  if bal:
    leaf, depth = bal
    feats |= {("bal", "depth", depth), ("bal", "leaf", leaf)}
    feats.add(("bal", "single chunk") if chunks == 1 else ("bal", f"two chunks, last of depth {depth}") if chunks == 2 else
              ("bal", "three or more chunks"))
    if depth in (1, 2):
      feats.add(("bal", "one step, fewer than 8 leaves"))
    return "mse_scale_balanced_kernel", feats
  count = len(pairwise_leaves(0, last))
  if chunks == 1:
    if n < 8:
      feats.add(("leaves", "length < 8"))
    elif count == 1:
      feats.add(("leaves", "one leaf with a tail"))
    elif count == 2:
      feats.add(("leaves", "two leaves"))
  else:
    feats.add(("leaves", "multi-chunk, unbalanced last chunk"))
    if chunks >= 3:
      feats.add(("leaves", "three chunks"))
  if count > 8 and count % 8:
    feats.add(("leaves", "leaf count no multiple of 8"))
  if count > 64:
    feats.add(("leaves", "more than 64 leaves"))
  return "mse_scale_leaves_kernel", feats


def route(entry, units, shape, x_offset_floats=0, q_offset_bytes=0, two_kernels_env=False):
  """(kernels, features) of one call.

  entry 'scale' / 'requant': `units` contiguous units of shape = unit_len elements; x_offset_floats and q_offset_bytes
  are the distances of x and q_out from 16-byte aligned addresses. entry 'scale_nd': units = channels and
  shape = (outer, inner)."""
  if entry == "scale_nd":
    outer, inner = shape
    if outer == 1:
      kernel, feats = _contiguous(units, inner)
      return (kernel,), feats | {("nd", "outer == 1")}
    if units == 1:      # one channel is one contiguous vector, to NumPy (it merges the axes) and to the library
      kernel, feats = _contiguous(1, outer * inner)
      return (kernel,), feats | {("nd", "one channel, inner = 1" if inner == 1 else "one channel, inner > 1")}
    if inner == 1:
      feats = {("cols", "outer < 8") if outer < COLS_UNROLL else ("cols", "outer = 8k") if outer % COLS_UNROLL == 0 else
               ("cols", "outer = 8k + t"),
               ("cols", "channels < 256") if units < COLS_BLOCK else ("cols", "channels = 256") if units == COLS_BLOCK else
               ("cols", "channels > 256")}
      return ("mse_scale_cols_kernel",), feats
    feats = {("seg", f"channels % 4 = {units % 4}")}
    if inner < 8:
      feats.add(("seg", "inner < 8"))
    elif inner <= LEAF and inner % 8:
      feats.add(("seg", "8 <= inner <= 128 with a tail"))
    elif inner > CHUNK:
      feats.add(("seg", "inner > 8192"))
    if outer == 2:
      feats.add(("seg", "outer = 2"))
    elif outer % 2:
      feats.add(("seg", "outer odd, above 2"))
    return ("mse_scale_seg_kernel",), feats
  kernel, feats = _contiguous(units, shape)
  if entry == "scale":
    return (kernel,), feats
  assert entry == "requant", entry
  reasons = []
  if shape % 4:
    reasons.append("length no multiple of 4")
  elif kernel != "mse_scale_balanced_kernel":
    reasons.append("unbalanced length")
  if (4 * x_offset_floats) % 16:
    reasons.append("x not 16-byte aligned")
  if q_offset_bytes % 4:
    reasons.append("q_out not 4-byte aligned")
  if two_kernels_env:
    reasons.append("MI355Q_MSE_TWO_KERNELS")
  if not reasons:
    return (kernel + " (fused quantize)",), feats | {("requant", "one kernel")}
  return (kernel, "mi355q_quantize_f32"), feats | {("requant", "two kernels: " + r) for r in reasons}


KERNELS = ("balanced", "leaves", "seg", "cols")
REQUIRED = frozenset(
    [("bal", "depth", d) for d in (0, 1, 2, 3, 6)] + [("bal", "leaf", l) for l in (8, 72, 120, 128)] +
    [("bal", f) for f in ("single chunk", "two chunks, last of depth 0", "two chunks, last of depth 3", "three or more chunks",
                          "one step, fewer than 8 leaves")] +
    [("leaves", f) for f in ("length < 8", "one leaf with a tail", "two leaves", "leaf count no multiple of 8",
                             "more than 64 leaves", "multi-chunk, unbalanced last chunk", "three chunks")] +
    [("seg", f) for f in ("inner < 8", "8 <= inner <= 128 with a tail", "inner > 8192", "outer = 2", "outer odd, above 2")] +
    [("seg", f"channels % 4 = {r}") for r in range(4)] +
    [("cols", f) for f in ("outer < 8", "outer = 8k", "outer = 8k + t", "channels < 256", "channels = 256", "channels > 256")] +
    [("requant", "one kernel")] +
    [("requant", "two kernels: " + r) for r in ("length no multiple of 4", "unbalanced length", "x not 16-byte aligned",
                                                "q_out not 4-byte aligned")] +
    [("units%4", r) for r in range(4)] + [("units", 1)] +
    [("nd", "one channel, inner = 1"), ("nd", "one channel, inner > 1")] +
    [("kind", k, kernel) for k in ("wide", "squares", "signs", "nonfinite") for kernel in KERNELS] +
    [("kind", k, "requant") for k in ("wide", "squares", "signs", "nonfinite", "ties")])


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class ScaleCase:
  """mi355q_mse_scale_f32, and mi355q_mse_scale_nd_f32 with outer == 1."""
  units: int
  n: int
  kind: str


@dataclasses.dataclass(frozen=True)
class NdCase:
  """mi355q_mse_scale_nd_f32 on [outer, channels, inner]; inner == 1 is the [outer, channels] view."""
  outer: int
  channels: int
  inner: int
  kind: str


@dataclasses.dataclass(frozen=True)
class RequantCase:
  """mi355q_mse_requant_f32; x_off in floats and q_off in bytes past aligned buffers (through the C ABI only)."""
  units: int
  n: int
  bits: int
  narrow: int
  kind: str
  x_off: int = 0
  q_off: int = 0


def multiplier(c):
  return TIES_MUL if c.kind == "ties" else MULS[0] if c.bits >= 8 else MULS[1]


def _short(kernel):
  return kernel.split(" ")[0].replace("mse_scale_", "").replace("_kernel", "")


def kernels(c):
  if isinstance(c, ScaleCase):
    return route("scale", c.units, c.n)[0]
  if isinstance(c, NdCase):
    return route("scale_nd", c.channels, (c.outer, c.inner))[0]
  return route("requant", c.units, c.n, c.x_off, c.q_off)[0]


def features(c):
  if isinstance(c, ScaleCase):
    ks, f = route("scale", c.units, c.n)
  elif isinstance(c, NdCase):
    ks, f = route("scale_nd", c.channels, (c.outer, c.inner))
  else:
    ks, f = route("requant", c.units, c.n, c.x_off, c.q_off)
    f = f | {("kind", c.kind, "requant")}
  return f | {("kind", c.kind, _short(ks[0]))}


def case_id(c):
  feats = sorted("/".join(str(v) for v in f).replace(" ", "_") for f in features(c) if f[0] not in ("kind", "units%4", "units"))
  if isinstance(c, ScaleCase):
    head = f"scale-{c.units}x{c.n}"
  elif isinstance(c, NdCase):
    head = f"nd-{c.outer}x{c.channels}x{c.inner}"
  else:
    head = f"requant-{c.units}x{c.n}-b{c.bits}n{c.narrow}" + (f"-x+{c.x_off}" if c.x_off else "") + (f"-q+{c.q_off}" if c.q_off else "")
  return f"{head}-{c.kind}[{','.join(feats)}]"


BALANCED_LENGTHS = (8, 120, 128, 144, 512, 576, 1024, 4608, 8192, 8200, 8768, 11008, 16672, 3 * 8192)
LEAVES_LENGTHS = (4, 7, 9, 100, 129, 136, 1000, 1032, 8191, 8292, 25576)

SCALE_CASES = (
    # the balanced kernel
    ScaleCase(9, 8, "wide"),
    ScaleCase(9, 120, "wide"),
    ScaleCase(1, 128, "wide"),
    ScaleCase(6, 144, "wide"),
    ScaleCase(7, 512, "wide"),
    ScaleCase(8, 576, "wide"),
    ScaleCase(8, 1024, "wide"),
    ScaleCase(9, 4608, "wide"),
    ScaleCase(6, 8192, "wide"),
    ScaleCase(9, 8200, "wide"),
    ScaleCase(6, 8768, "wide"),
    ScaleCase(9, 11008, "wide"),
    ScaleCase(7, 16672, "wide"),
    ScaleCase(6, 3 * 8192, "wide"),
    ScaleCase(9, 8, "squares"),
    ScaleCase(9, 512, "squares"),
    ScaleCase(9, 8768, "squares"),
    ScaleCase(7, 144, "signs"),
    ScaleCase(5, 8200, "signs"),
    ScaleCase(7, 120, "nonfinite"),
    ScaleCase(6, 576, "nonfinite"),
    ScaleCase(7, 16672, "nonfinite"),
    # the leaves kernel
    ScaleCase(8, 4, "wide"),
    ScaleCase(9, 7, "wide"),
    ScaleCase(5, 9, "wide"),
    ScaleCase(7, 100, "wide"),
    ScaleCase(8, 129, "wide"),
    ScaleCase(5, 136, "wide"),
    ScaleCase(7, 1000, "wide"),
    ScaleCase(6, 1032, "wide"),
    ScaleCase(9, 8191, "wide"),
    ScaleCase(6, 8292, "wide"),
    ScaleCase(7, 25576, "wide"),
    ScaleCase(9, 7, "squares"),
    ScaleCase(9, 1032, "squares"),
    ScaleCase(9, 8292, "squares"),
    ScaleCase(7, 100, "signs"),
    ScaleCase(5, 8191, "signs"),
    ScaleCase(7, 9, "nonfinite"),
    ScaleCase(6, 1000, "nonfinite"),
    ScaleCase(7, 8191, "nonfinite"),
    ScaleCase(6, 25576, "nonfinite"),
)

ND_CASES = (
    # the segment kernel: [outer, channels, inner]
    NdCase(2, 5, 3, "wide"),
    NdCase(3, 8, 7, "wide"),
    NdCase(2, 6, 100, "wide"),
    NdCase(5, 7, 9, "wide"),
    NdCase(7, 4, 136, "wide"),
    NdCase(3, 7, 1000, "wide"),
    NdCase(2, 6, 8292, "wide"),
    NdCase(3, 3, 8192 + 8192 + 100, "wide"),
    NdCase(2, 9, 512, "wide"),
    NdCase(3, 9, 100, "squares"),
    NdCase(2, 7, 9, "signs"),
    NdCase(3, 7, 8200, "nonfinite"),
    NdCase(5, 6, 9, "nonfinite"),
    # the column kernel: [outer, channels]
    NdCase(2, 40, 1, "wide"),
    NdCase(7, 256, 1, "wide"),
    NdCase(8, 257, 1, "wide"),
    NdCase(24, 300, 1, "wide"),
    NdCase(19, 256, 1, "wide"),
    NdCase(1001, 9, 1, "wide"),
    NdCase(19, 9, 1, "squares"),
    NdCase(24, 300, 1, "signs"),
    NdCase(19, 257, 1, "nonfinite"),
    # one channel: a contiguous vector of outer * inner elements
    NdCase(64, 1, 1, "wide"),
    NdCase(9000, 1, 1, "wide"),
    NdCase(5, 1, 9, "wide"),
    NdCase(3, 1, 8292, "wide"),
    NdCase(3, 1, 1000, "nonfinite"),
)

REQUANT_CASES = (
    # one kernel
    RequantCase(9, 8, 3, 0, "wide"),
    RequantCase(7, 8, 2, 1, "wide"),
    RequantCase(9, 120, 4, 0, "wide"),
    RequantCase(1, 128, 4, 0, "wide"),
    RequantCase(6, 144, 4, 1, "wide"),
    RequantCase(7, 512, 8, 1, "wide"),
    RequantCase(8, 576, 8, 0, "wide"),
    RequantCase(8, 1024, 4, 0, "wide"),
    RequantCase(9, 4608, 8, 1, "wide"),
    RequantCase(6, 8192, 4, 0, "wide"),
    RequantCase(9, 8200, 8, 1, "wide"),
    RequantCase(6, 8768, 4, 0, "wide"),
    RequantCase(9, 11008, 8, 1, "wide"),
    RequantCase(7, 16672, 4, 0, "wide"),
    RequantCase(6, 3 * 8192, 8, 1, "wide"),
    RequantCase(9, 8, 4, 0, "squares"),
    RequantCase(9, 1024, 8, 1, "squares"),
    RequantCase(7, 8, 4, 0, "signs"),
    RequantCase(7, 576, 8, 1, "signs"),
    RequantCase(5, 8200, 4, 0, "signs"),
    RequantCase(7, 144, 4, 0, "nonfinite"),
    RequantCase(6, 8768, 8, 1, "nonfinite"),
    RequantCase(5, 8, 4, 0, "ties"),
    RequantCase(7, 120, 3, 1, "ties"),
    RequantCase(6, 512, 8, 1, "ties"),
    RequantCase(3, 8200, 4, 0, "ties"),
    RequantCase(2, 11008, 8, 0, "ties"),
    # two kernels: the length
    RequantCase(9, 7, 4, 0, "wide"),
    RequantCase(5, 9, 3, 0, "wide"),
    RequantCase(7, 100, 4, 1, "wide"),
    RequantCase(8, 129, 4, 0, "wide"),
    RequantCase(5, 136, 4, 0, "wide"),
    RequantCase(7, 1000, 8, 1, "wide"),
    RequantCase(6, 1032, 4, 0, "wide"),
    RequantCase(9, 8191, 8, 1, "wide"),
    RequantCase(6, 8292, 4, 0, "wide"),
    RequantCase(7, 25576, 8, 1, "wide"),
    RequantCase(7, 100, 4, 0, "signs"),
    RequantCase(6, 1000, 8, 1, "nonfinite"),
    RequantCase(5, 1000, 4, 0, "ties"),
    RequantCase(7, 129, 5, 1, "ties"),
    RequantCase(9, 1032, 8, 1, "squares"),
    # two kernels: the addresses
    RequantCase(9, 8, 3, 0, "wide", x_off=1),
    RequantCase(8, 1024, 4, 0, "wide", x_off=1),
    RequantCase(3, 8200, 4, 0, "ties", x_off=1),
    RequantCase(9, 8, 3, 0, "wide", q_off=1),
    RequantCase(6, 512, 8, 1, "ties", q_off=1),
    RequantCase(6, 8768, 4, 0, "wide", q_off=1),
    RequantCase(8, 576, 8, 0, "wide", x_off=1, q_off=1),
)

# every width the entry accepts with either bound, at one single-chunk and one multi-chunk balanced length
BITS_LENGTHS = (576, 8768)
BITS_UNITS = {576: 8, 8768: 6}
BITS_CASES = tuple(RequantCase(BITS_UNITS[n], n, bits, narrow, "wide") for n in BITS_LENGTHS for bits in range(2, 9)
                   for narrow in (0, 1) if RequantCase(BITS_UNITS[n], n, bits, narrow, "wide") not in REQUANT_CASES)

CASES = SCALE_CASES + ND_CASES + REQUANT_CASES + BITS_CASES


# ------------------------------------------------------------------------------------------------ inputs
def input_key(c):
  """What a case's input depends on: cases that differ in the width, the bound or the addresses only share their data
  (the ties kind plants its ties for one width and bound)."""
  if isinstance(c, NdCase):
    return ("nd", c.kind, c.outer, c.channels, c.inner)
  if c.kind == "ties":
    return ("ties", c.units, c.n, c.bits, c.narrow)
  return (c.kind, c.units, c.n)


# A seed other than 0 is the first one at which every case that shares the input shows every mutation that attacks it
# (test_mse_route_cases_host.py): a re-ordered addition or a mean rounded another way moves a unit's sum by one place at
# most, and the root that follows keeps it about every other time, so a handful of units can miss it.
SEEDS = {
    ('wide', 1, 128): 24,
    ('wide', 6, 144): 9,
    ('wide', 8, 576): 6,
    ('wide', 8, 1024): 4,
    ('wide', 9, 4608): 28,
    ('wide', 6, 8768): 159,
    ('wide', 9, 11008): 15,
    ('wide', 7, 16672): 23,
    ('wide', 6, 24576): 2,
    ('squares', 9, 8768): 8,
    ('wide', 9, 7): 3,
    ('wide', 5, 9): 21,
    ('wide', 7, 100): 35,
    ('wide', 8, 129): 2,
    ('wide', 5, 136): 19,
    ('wide', 7, 1000): 6,
    ('wide', 6, 1032): 10,
    ('wide', 6, 8292): 177,
    ('wide', 7, 25576): 119,
    ('squares', 9, 1032): 6,
    ('nd', 'wide', 2, 5, 3): 24,
    ('nd', 'wide', 3, 8, 7): 2,
    ('nd', 'wide', 2, 6, 100): 52,
    ('nd', 'wide', 5, 7, 9): 27,
    ('nd', 'wide', 7, 4, 136): 76,
    ('nd', 'wide', 3, 7, 1000): 7,
    ('nd', 'wide', 2, 6, 8292): 38,
    ('nd', 'wide', 3, 3, 16484): 154,
    ('nd', 'wide', 2, 9, 512): 10,
    ('nd', 'squares', 19, 9, 1): 1,
    ('nd', 'wide', 9000, 1, 1): 262,
    ('nd', 'wide', 5, 1, 9): 7,
    ('nd', 'wide', 3, 1, 8292): 7,
    ('ties', 2, 11008, 8, 0): 2,
    ('wide', 9, 8200): 163,
}


def _rng(c):
  key = input_key(c)
  return np.random.default_rng([SEEDS.get(key, 0), sum(map(ord, key[0]))] + [v for v in key[1:] if isinstance(v, int)])


def _wide(rng, units, n, run=None):
  """normal * exp(4 normal). One element carries most of such a sum, and an addition re-ordered elsewhere is lost in it,
  so the places a kernel treats on their own are made as heavy as the rest of the run they belong to (the whole unit, or
  a segment of `run` elements): the last chunk of several, and the tail of the last leaf."""
  run = run or n
  x = (rng.standard_normal((units, n)) * np.exp(4.0 * rng.standard_normal((units, n)))).astype(F)
  v = x.reshape(units, n // run, run)                       # a view: x is written through it
  top = np.abs(v).max(axis=2, keepdims=True)
  last = (run - 1) // CHUNK * CHUNK
  if last:
    grow = top / np.abs(v[:, :, last:]).max(axis=2, keepdims=True) * rng.uniform(0.5, 2.0, top.shape)
    v[:, :, last:] = v[:, :, last:] * grow
  ln = pairwise_leaves(0, run - last)[-1][1]
  tail = ln % 8 if ln >= 8 else 0
  if tail:
    shape = (units, n // run, tail)
    v[:, :, run - tail:] = top * rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)
  return x


def _squares(rng, units, n):
  """Unit u holds magnitudes around 10^e(u), e from -44.5 (float32 denormals) to 19.4 (squares overflow); shuffled."""
  e = rng.permutation(np.linspace(-44.5, 19.4, units)) if units > 1 else np.array([19.4])
  mag = rng.uniform(0.5, 1.0, (units, n)) * 10.0 ** e[:, None]
  return (mag * rng.choice([-1.0, 1.0], (units, n))).astype(F)


def _signs(rng, units, n):
  x = (rng.standard_normal((units, n)) * 0.03).astype(F)
  x[rng.random((units, n)) < 0.1] = -0.0
  for u in range(units):
    what = u % 5
    if what == 1:
      x[u] = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)      # scale 0: x / 0
    elif what == 2:
      x[u, rng.integers(n)] = 250.0                          # everything else rounds to 0, the outlier clips
    elif what == 3:
      x[u] = -0.0
    elif what == 4:
      x[u, rng.integers(n)] = -250.0
  return x


def nonfinite_plants(n):
  """(index, value, where) planted in unit u % len: the first leaf, the last leaf and its tail, the last chunk."""
  last_chunk = (n - 1) // CHUNK * CHUNK
  lo, ln = pairwise_leaves(0, n - last_chunk)[-1]
  return ((3 % n, np.inf, "first leaf"),
          (last_chunk + lo + min(ln - 1, 9), -np.inf, "last leaf"),
          (n - 1, np.nan, "leaf tail" if ln % 8 or ln < 8 else "last element"),
          (last_chunk + min(5, n - last_chunk - 1), np.nan, "last chunk"),
          (n - 1, np.inf, "leaf tail" if ln % 8 or ln < 8 else "last element"),
          (None, None, "clean"),
          (0, -np.inf, "first element"))


def _nonfinite(rng, units, n):
  x = _wide(rng, units, n)
  plants = nonfinite_plants(n)
  for u in range(units):
    i, v, _ = plants[u % len(plants)]
    if i is not None:
      x[u, i] = v
  if units > 4:
    x[4, n // 2] = np.nan                                    # an inf and a NaN in one unit
  return x


_KINDS = {"wide": _wide, "squares": _squares, "signs": _signs, "nonfinite": _nonfinite}
TIE_TARGETS = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 0.5, 1.5, -0.5, -1.5)


def _ties(c, rng):
  """Normal data in which, once the scale has settled, x / scale is exactly a tie at up to a dozen elements of every
  unit. A planted element moves the unit's scale, so plant, take the scale again and repeat until nothing moves."""
  x = rng.standard_normal((c.units, c.n)).astype(F)
  hi = 2 ** (c.bits - 1) - 1
  lo = -2 ** (c.bits - 1) + c.narrow
  targets = [t for t in TIE_TARGETS if lo < t < hi][:max(1, min(len(TIE_TARGETS), c.n // 2))]
  where = np.stack([rng.choice(c.n, len(targets), replace=False) for _ in range(c.units)])
  rows = np.arange(c.units)[:, None]
  t = np.array(targets, F)[None, :]
  for _ in range(64):
    scale = reference_scale(x, multiplier(c))
    planted = (t * scale[:, None]).astype(F)
    if np.array_equal(planted, x[rows, where]):
      break
    x[rows, where] = planted
  return x


def contiguous_input(c):
  """x float32 [units, n] of a ScaleCase or RequantCase."""
  rng = _rng(c)
  if c.kind == "ties":
    return _ties(c, rng)
  return _KINDS[c.kind](rng, c.units, c.n)


def nd_input(c):
  """x float32 [outer, channels, inner], or [outer, channels] when inner == 1; the kinds go by channel."""
  run = dict(run=c.inner if c.channels > 1 else c.outer * c.inner) if c.kind == "wide" else {}
  by_channel = _KINDS[c.kind](_rng(c), c.channels, c.outer * c.inner, **run)
  x = np.ascontiguousarray(by_channel.reshape(c.channels, c.outer, c.inner).transpose(1, 0, 2))
  return x.reshape(c.outer, c.channels) if c.inner == 1 else x


# ------------------------------------------------------------------------------------------------ the reference's expressions
def reference_scale(x, mult):
  """[units]: contiguous units [units, n] (ref mse.py:100-109, CHANNELWISE with the quantized dimension first)."""
  with np.errstate(all="ignore"):
    return (mult * np.sqrt(np.mean(x**2, axis=1, keepdims=True))).reshape(-1)


def reference_scale_nd(x, mult):
  """[channels]: x [outer, channels, inner] or [outer, channels], the quantized dimension second."""
  dims = (0, 2) if x.ndim == 3 else (0,)
  with np.errstate(all="ignore"):
    return (mult * np.sqrt(np.mean(x**2, axis=dims, keepdims=True))).reshape(-1)


def reference_q(x, scale, bits, narrow):
  """int8 [units, n]: uniform_quantize with a zero zero point. The oracle ties the narrow bound to `symmetric and
  num_bits >= 8`; the combinations it cannot ask for are its last three lines written out (ref
  uniform_quantize_tensor.py:357-360)."""
  s = np.asarray(scale, F).reshape(-1, 1)
  zp = np.zeros(s.shape, np.int32)
  with np.errstate(all="ignore"):
    if narrow == int(bits >= 8):
      return O.uniform_quantize(x, s, zp, bits, True, quantized_dim=0)
    if not narrow:
      return O.uniform_quantize(x, s, zp, bits, False, quantized_dim=0)
    q = np.divide(x, s)
    q = np.add(q, zp, out=q)
    return np.clip(np.rint(q, out=q), -2.0 ** (bits - 1) + 1, 2.0 ** (bits - 1) - 1, out=q).astype(np.int8)


# ------------------------------------------------------------------------------------------------ the in-order models
MUTATIONS = (
    "no_chunking",            # one pairwise sum over the whole unit, no 8192-element chunks
    "split_not_rounded",      # the recursion splits at n / 2, not rounded down to a multiple of 8
    "leaf_left_to_right",     # a leaf summed left to right
    "acc_sequential",         # the eight accumulators folded (((r0+r1)+r2)+r3)+...
    "tail_before_combine",    # the leaf tail added into the accumulators, before they are combined
    "tail_dropped",           # the leaf tail left out
    "last_table_full",        # the last chunk summed with the full chunk's leaf table (leaves of 128 under the 64-leaf tree)
    "chunks_pairwise",        # the chunks' partial sums combined pairwise, not in order
    "steps_sequential",       # the 8-leaf steps of a balanced tree folded in order, not as a binary counter
    "square_add_fused",       # acc + x * x with one rounding
    "mean_reciprocal",        # the mean as acc * (1 / count)
    "mean_f64",               # the mean and its root taken in float64, rounded once
    "seg_one_run",            # the segments of a channel summed as one contiguous run across outer
    "cols_pairwise",          # a column summed pairwise
    "cols_eight_partials",    # a column summed as eight strided partial sums
    "one_channel_in_pieces",  # a tensor of one channel summed row by row, or segment by segment
    "quant_reciprocal",       # x * (1 / scale) for x / scale
    "ties_away",              # ties rounded away from zero
    "narrow_flipped",         # the narrow bound applied where it is not asked for, and omitted where it is
)


def _sq(v):
  with np.errstate(all="ignore"):
    return v * v                                            # float32 * float32: rounded to float32


def _add_sq(acc, v, mut):
  with np.errstate(all="ignore"):
    if mut == "square_add_fused":
      return (acc.astype(np.float64) + v.astype(np.float64) * v.astype(np.float64)).astype(F)
    return acc + v * v


def _add(a, b):
  with np.errstate(all="ignore"):
    return a + b


def _combine8(r, mut):
  if mut == "acc_sequential":
    res = r[:, 0]
    for k in range(1, 8):
      res = _add(res, r[:, k])
    return res
  return _add(_add(_add(r[:, 0], r[:, 1]), _add(r[:, 2], r[:, 3])), _add(_add(r[:, 4], r[:, 5]), _add(r[:, 6], r[:, 7])))


def _leaf_sum(a, mut):
  """Sum of squares of a [units, n <= 128]: NumPy's unrolled block, every unit at once."""
  n = a.shape[1]
  if n < 8 or mut == "leaf_left_to_right":
    res = np.zeros(a.shape[0], F)
    for i in range(n):
      res = _add_sq(res, a[:, i], mut)
    return res
  r = _sq(a[:, :8])
  i = 8
  while i + 8 <= n:
    r = _add_sq(r, a[:, i:i + 8], mut)
    i += 8
  if mut == "tail_before_combine":
    r = r.copy()
    for j in range(i, n):
      r[:, j - i] = _add_sq(r[:, j - i], a[:, j], mut)
    return _combine8(r, mut)
  res = _combine8(r, mut)
  if mut != "tail_dropped":
    for j in range(i, n):
      res = _add_sq(res, a[:, j], mut)
  return res


def _fold_complete(sums):
  """A complete binary tree over a list whose missing leaves are None."""
  while len(sums) > 1:
    sums = [l if r is None else _add(l, r) for l, r in zip(sums[0::2], sums[1::2])]
  return sums[0]


def _chunk_sum(a, mut, last_of_many):
  """Pairwise sum of squares of a [units, n <= 8192]: the leaves first, then the recursion over their sums."""
  n = a.shape[1]
  if mut == "last_table_full" and last_of_many and n < CHUNK:
    sums = [_leaf_sum(a[:, lo:lo + LEAF], mut) for lo in range(0, n, LEAF)]
    return _fold_complete(sums + [None] * (CHUNK // LEAF - len(sums)))
  round8 = mut != "split_not_rounded"
  sums = [_leaf_sum(a[:, lo:lo + ln], mut) for lo, ln in pairwise_leaves(0, n, round8)]
  bal = balanced_chunk(n)
  if mut == "steps_sequential" and bal and bal[1] >= 4:
    steps = [_fold_complete(sums[s:s + 8]) for s in range(0, len(sums), 8)]
    res = steps[0]
    for s in steps[1:]:
      res = _add(res, s)
    return res
  it = iter(sums)

  def combine(m):
    if m <= LEAF:
      return next(it)
    m2 = m // 2
    if round8:
      m2 -= m2 % 8
    left = combine(m2)
    return _add(left, combine(m - m2))

  return combine(n)


def _fold_pairwise(parts):
  if len(parts) == 1:
    return parts[0]
  h = len(parts) // 2
  return _add(_fold_pairwise(parts[:h]), _fold_pairwise(parts[h:]))


def model_sumsq(a, mut=None):
  """Sum of squares along axis 1 of contiguous float32 units a [units, n]: 8192-element chunks added in order."""
  n = a.shape[1]
  if mut == "no_chunking":
    assert n <= 4 * CHUNK
    leaves = pairwise_leaves(0, n)
    it = iter([_leaf_sum(a[:, lo:lo + ln], mut) for lo, ln in leaves])

    def combine(m):
      if m <= LEAF:
        return next(it)
      m2 = m // 2 - (m // 2) % 8
      left = combine(m2)
      return _add(left, combine(m - m2))

    return combine(n)
  parts = [_chunk_sum(a[:, lo:lo + CHUNK], mut, n > CHUNK and lo + CHUNK >= n) for lo in range(0, n, CHUNK)]
  if mut == "chunks_pairwise":
    return _fold_pairwise(parts)
  total = parts[0]
  for p in parts[1:]:
    total = _add(total, p)
  return total


def _finish(acc, count, mult, mut):
  with np.errstate(all="ignore"):
    if mut == "mean_f64":
      root = np.sqrt(acc.astype(np.float64) / count).astype(F)
    elif mut == "mean_reciprocal":
      root = np.sqrt(acc * (F(1.0) / F(count)))
    else:
      root = np.sqrt(acc / F(count))
    return F(mult) * root


def model_scale(x, mult, mut=None):
  return _finish(model_sumsq(x, mut), x.shape[1], mult, mut)


def model_scale_nd(x, mult, mut=None):
  if x.shape[1] == 1 and mut != "one_channel_in_pieces":    # one channel: NumPy merges the axes into one vector
    return model_scale(x.reshape(1, -1), mult, mut)
  if x.ndim == 2:                                           # [outer, channels]: row by row
    outer = x.shape[0]
    if mut == "cols_pairwise":
      acc = model_sumsq(np.ascontiguousarray(x.T))
    elif mut == "cols_eight_partials":
      full = outer - outer % 8
      acc = np.zeros(x.shape[1], F)
      if full:
        r = _sq(x[:8].T)
        for o in range(8, full, 8):
          r = _add_sq(r, x[o:o + 8].T, mut)
        acc = _combine8(r, None)
      for o in range(full, outer):
        acc = _add_sq(acc, x[o], mut)
    else:
      acc = np.zeros(x.shape[1], F)
      for o in range(outer):
        acc = _add_sq(acc, x[o], mut)
    return _finish(acc, outer, mult, mut)
  outer, channels, inner = x.shape
  if mut == "seg_one_run":
    acc = model_sumsq(np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(channels, outer * inner))
  else:
    acc = None
    for o in range(outer):
      seg = x[o]
      if mut == "no_chunking":
        parts = [model_sumsq(seg, mut)]
      else:
        parts = [_chunk_sum(seg[:, lo:lo + CHUNK], mut, False) for lo in range(0, inner, CHUNK)]
      for p in parts:
        acc = p if acc is None else _add(acc, p)
  return _finish(acc, outer * inner, mult, mut)


def model_q(x, scale, bits, narrow, mut=None):
  if mut == "narrow_flipped":
    narrow = 1 - narrow
  hi = F(2 ** (bits - 1) - 1)
  lo = F(-2 ** (bits - 1) + narrow)
  s = scale.reshape(-1, 1)
  with np.errstate(all="ignore"):
    v = x * (F(1.0) / s) if mut == "quant_reciprocal" else x / s
    if mut == "ties_away":
      r = (np.sign(v) * np.floor(np.abs(v.astype(np.float64)) + 0.5)).astype(F)
    else:
      r = np.rint(v)
    r = np.minimum(np.maximum(r, lo), hi)
    return np.where(np.isnan(v), F(0.0), r).astype(np.int8)  # NaN: clip keeps it, the cast to an 8-bit integer gives 0


def _leaf_lists(n, round8=True):
  return [pairwise_leaves(0, min(CHUNK, n - lo), round8) for lo in range(0, n, CHUNK)]


def _run_attacks(mut, n, kind):
  """Whether a contiguous run of n elements of this kind has to show a mutation of the run's sum."""
  chunks = -(-n // CHUNK)
  last = n - (n - 1) // CHUNK * CHUNK
  leaves = [l for chunk in _leaf_lists(n) for l in chunk]
  if mut == "square_add_fused":                             # a square has to be added to something: a leaf of 8 has none
    return kind in ("wide", "squares") and any(2 <= ln < 8 or ln > 8 for _, ln in leaves)
  if kind != "wide":
    return False
  if mut == "no_chunking":                                  # one pairwise sum of 2 * 8192 splits at 8192: the same additions
    return n > CHUNK and n != 2 * CHUNK
  if mut == "split_not_rounded":
    return _leaf_lists(n) != _leaf_lists(n, False)
  if mut in ("leaf_left_to_right", "acc_sequential"):
    return n >= 8
  if mut in ("tail_before_combine", "tail_dropped"):
    return any(ln >= 8 and ln % 8 for _, ln in leaves)
  if mut == "last_table_full":                              # leaves of 128 under a complete tree are the full chunk's table
    bal = balanced_chunk(last)
    return chunks > 1 and last > LEAF and not (bal and bal[0] == LEAF)
  if mut == "chunks_pairwise":
    return chunks >= 3
  if mut == "steps_sequential":                             # two steps fold the same way either way
    bal = balanced_chunk(last)
    return chunks > 1 or bool(bal and bal[1] >= 5)
  return False


def clips_low(c):
  """Whether some element of a wide unit can reach the lower bound: |x| <= sqrt(n) rms, with a margin of two."""
  reach = multiplier(c) * (2 ** (c.bits - 1) - 0.5)
  return c.n > 4 * reach * reach


def attacks(mut, c):
  """Whether case c has to show mutation `mut` (a condition on the case list, checked by the host test)."""
  if mut in ("mean_reciprocal", "mean_f64"):
    count = c.outer * c.inner if isinstance(c, NdCase) else c.n
    return c.kind == "wide" and count & (count - 1) != 0    # a power of two divides exactly, in any precision
  if mut == "one_channel_in_pieces":                        # fewer than 8 rows, or segments that are whole chunks,
    return (isinstance(c, NdCase) and c.channels == 1 and c.kind == "wide" and c.outer > 1 and c.outer * c.inner >= 8 and
            c.inner % CHUNK != 0)                           # add up the same way
  if isinstance(c, NdCase) and c.channels == 1:             # what the one unit goes through is the contiguous cases' to show
    return mut == "no_chunking" and _run_attacks(mut, c.outer * c.inner, c.kind)
  if isinstance(c, NdCase):
    if c.inner == 1:
      if mut in ("cols_pairwise", "cols_eight_partials"):
        return c.kind == "wide" and c.outer >= 8
      return mut == "square_add_fused" and c.kind in ("wide", "squares") and c.outer >= 2
    if mut == "seg_one_run":                                # 2^k complete trees under one chunk are one complete tree
      one_tree = c.outer & (c.outer - 1) == 0 and balanced_chunk(c.inner) is not None and c.outer * c.inner <= CHUNK
      return c.kind == "wide" and c.inner >= 2 and not one_tree
    if mut in ("last_table_full", "chunks_pairwise"):       # the segment kernel has no tables, and its chunks join the
      return False                                          # channel's running total one by one
    if mut == "steps_sequential":
      return False
    return _run_attacks(mut, c.inner, c.kind)
  if isinstance(c, RequantCase):
    if mut in ("quant_reciprocal", "ties_away"):
      return c.kind == "ties"
    if mut == "narrow_flipped":
      return c.kind == "wide" and clips_low(c)
  return _run_attacks(mut, c.n, c.kind)


# ------------------------------------------------------------------------------------------------ expected values
@functools.lru_cache(maxsize=None)
def expected(c):
  """(inputs, expected outputs) of a case: the reference's expressions. Cached and shared: treat as read-only."""
  if isinstance(c, NdCase):
    x = nd_input(c)
    out = {f"scale@{m}": reference_scale_nd(x, m) for m in MULS}
  else:
    x = contiguous_input(c)
    if isinstance(c, ScaleCase):
      out = {f"scale@{m}": reference_scale(x, m) for m in MULS}
    else:
      scale = reference_scale(x, multiplier(c))
      out = dict(scale=scale, q=reference_q(x, scale, c.bits, c.narrow))
  inputs = dict(x=x)
  for v in list(inputs.values()) + list(out.values()):
    v.setflags(write=False)
  return inputs, out


def model(c, mut=None):
  x = expected(c)[0]["x"]
  if isinstance(c, NdCase):
    return {f"scale@{m}": model_scale_nd(x, m, mut) for m in MULS}
  if isinstance(c, ScaleCase):
    return {f"scale@{m}": model_scale(x, m, mut) for m in MULS}
  scale = model_scale(x, multiplier(c), mut)
  return dict(scale=scale, q=model_q(x, scale, c.bits, c.narrow, mut))


def same_bits(got, want):
  """'' when two dicts of arrays agree bit for bit (float32 as uint32 patterns, any NaN for a NaN; integers as int8),
  else what differs."""
  bad = []
  for name, w in want.items():
    g = np.asarray(got[name])
    if g.shape != w.shape or g.dtype != w.dtype:
      bad.append(f"{name}: {g.dtype}{g.shape} for {w.dtype}{w.shape}")
      continue
    if w.dtype == np.float32:
      differ = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    else:
      differ = g != w
    if differ.any():
      where = np.argwhere(differ)
      first = tuple(where[0])
      bad.append(f"{name}: {len(where)} of {w.size} differ, first at {first}: {g[first]!r} for {w[first]!r}")
  return "; ".join(bad)
