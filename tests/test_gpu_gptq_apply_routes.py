"""Every route of the OBS sweep behind mi355q_gptq_apply_f32 / mi355q_gptq_apply_wide_f32 (csrc/gptq.hip,
gptq_apply_impl), bit for bit, on inputs on which every float32 operation of the sweep is exact.

Which kernels a call reaches is decided on the host from the zero points, the scale type, block_size % 32, d % 64,
rows >= 8192, the target width, the entry point and two environment switches; route() below restates that choice and
every case carries the route it is there for in its id.

The construction (make_case). Scales are powers of two, S[r, c]; weights are S[r, c] * k / 8 with integer k, so w / s
sits on a grid of eighths (exact .5 ties and values beyond both clip bounds included); Hinv has a power of two hd[i] on
its diagonal and R[i, j] * hd[i] above it with integer R in {-2 .. 2}. The error of column i is e = (w - dq) / hd[i] and
what it sends to column j is e * Hinv[i, j] = (w - dq) * R[i, j]: an integer number of grid units (grid = min(scale) /
8), as is every working weight. While the float64 reference runs it adds up, per element, |w| and the magnitude of
every product that ever reaches it; the largest of these sums stays below 2^23 grid units, so every partial sum in ANY
order of additions is an integer below 2^24 and exact in float32. The integers therefore have ONE correct bit pattern
whatever a kernel's order of additions, its grouping of the far update (one K = 256 product, four K = 64 ones, bf16
planes on the matrix cores) or its lane layout, and every route must return exactly the reference's. Below its diagonal
Hinv is NaN: the sweep reads the diagonal and the upper triangle only. R has several non-zeros per row inside the
row's own 64-column block and one in every later block, so that every catch-up tile and every far-update tile carries
a contribution that moves integers (checked without a GPU, pair of blocks by pair of blocks, for d <= 704).

What the host-only tests establish: the reference in float32 returns the float64 run's integers, the 2^23 bound, the
share of clipped integers, that every level and at least one exact tie occur, the sensitivity to every block of Hinv,
agreement with oracle.aeq_oracle.gptq_apply where the oracle can express the case, that the case list reaches every
route, and the argument checks of both entry points.

What this file does NOT cover: non-finite weights or scales; targets of 26 bits and more (the clip bound itself rounds
there); the Hessian and its inverse (every route of the inverse, bit for bit on exact Hessians:
test_gpu_hinv_routes.py); speed. Hinv on this data has two significant bits and the errors few (about 20
in the 4-bit 4096-column case, whose scales grow along the row), so the low planes of Hinv in the bf16x3 split are
empty: the test proves upd_bf16x3's tiling, indexing and accumulation, not that the split of a full-mantissa value is
exact -- the rate-based full-size tests of test_gpu_gptq.py stay for that.

Why some cases look the way they do. The sweep amplifies: column j of block b receives the errors of about b + 3
earlier columns, and a column pushed beyond a clip bound sends on an error as large as its excess. On a range of 16
steps (4 bits) that runs away on long rows -- everything behind one large error clips, with ever larger errors --, so
below 8 bits the body of the weights stays inside the range (BODY; noise and a few values beyond the bounds fill the
outer levels), and on 4096 columns the 4-bit case has scales that grow along the row (what early groups send shrinks in
the steps of late ones) while a 6-bit case carries per-row scales. A few small cases carry a seed chosen so that every
level occurs among their few values."""
import ctypes
import dataclasses
import functools
import os
import sys
import types

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 64                          # the sweep's block: NB of csrc/gptq.hip
GROUP = 4 * NB                   # kErrLd: the columns whose far update is applied together below 8 bits
GUARD = 64                       # elements in front of and behind q that no kernel may touch (keeps q 16-byte aligned)
WS_TAIL = 4096                   # sentinel bytes behind the workspace
SENTINEL = {np.dtype(np.int8): 0x5A, np.dtype(np.int32): 0x5A5A5A5A}
WS_FILL = 0xA5
SPREAD, FP32_UPD, FAR_PER_BLOCK = "MI355Q_GPTQ_SPREAD", "MI355Q_UPD_FP32_MFMA", "MI355Q_GPTQ_FAR_PER_BLOCK"
WRAP_MARGIN = 16                 # levels the body of a wrapping case stays away from the side on which q - zp wraps
WRAP_TAIL = 4                    # ... which only a row's last columns visit
IN_BLOCK = 3                     # non-zeros of a row of R inside the row's own block (where that many columns are left)
OUTLIERS = 0.02                  # share of the weights a little beyond a clip bound
# half-width in steps of the uniform body of w / s below 8 bits (None: the whole range and two levels more on each side)
BODY = lambda bits, d: None if bits >= 8 else ((1 << (bits - 1)) - 1) * (0.6 if d <= 704 else 0.4 if d <= 2048 else 0.2)


def env_is_default():
  """Read once per process by the library; route() restates its default (per block from 8 bits on)."""
  return FAR_PER_BLOCK not in os.environ


@functools.lru_cache(maxsize=None)
def library():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


@pytest.fixture(scope="module")
def lib():
  return library()


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  assert env_is_default(), f"{FAR_PER_BLOCK} changes the routes this file restates"
  L = library()
  from mi355q import runtime as rt
  return types.SimpleNamespace(torch=torch, rt=rt, L=L)


# ------------------------------------------------------------------------------------------------------- the routes ---
def route(rows, d, scale_mode, block_size, bits, zp, scale_dtype, env):
  """gptq_apply_impl() restated: (chain kernels in launch order, far-update kind, its K, on the bf16 matrix cores).
  zp: whether zero points are passed; scale_dtype: "f32" or "f64"; env: the names of the switches that are set."""
  wide = bits > 8
  per_step = scale_mode == 2 and block_size % 32 != 0
  f64 = scale_dtype == "f64"
  if not zp and not per_step and not f64 and d % NB == 0 and not wide and SPREAD not in env:
    chain = ("gptq_rows_kernel",)
  else:
    lanes = 16 if rows >= 8192 else 32
    chain = []
    for c0 in range(0, d, NB):
      plain = min(NB, d - c0) == NB and not zp and not per_step and not bits > 16
      name = f"gptq_block_kernel<{'double' if f64 else 'float'}, {lanes}, {'true' if plain else 'false'}>"
      if name not in chain:
        chain.append(name)
    chain = tuple(chain)
  if d <= GROUP:
    return chain, "none", 0, False
  kind, k = ("per_block", NB) if bits >= 8 else ("lazy", GROUP)
  split = rows % 128 == 0 and d % 128 == 0 and (d >= 4096 or (d >= 1024 and rows >= 8192)) and FP32_UPD not in env
  return chain, kind, k, split


ZP_DTYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32}


@dataclasses.dataclass(frozen=True)
class Case:
  rows: int
  d: int
  mode: int = 1          # 0: one scale; 1: per row; 2: per (row, bs columns)
  bs: int = 0
  bits: int = 4
  zp: str = ""           # "", or the reference's zero-point type: i8, i16, i32 (decides zp_via_f64 and diff_bits)
  f64: bool = False      # float64 scales
  narrow: bool = False
  wrap: bool = False     # q - zp wraps in its container (diff_bits == the container's width)
  spread: bool = False   # MI355Q_GPTQ_SPREAD=1
  fp32_upd: bool = False  # MI355Q_UPD_FP32_MFMA=1
  seed: int = 0
  want: tuple = ()       # the elements of ALL_ROUTES this case is there for

  @property
  def env(self):
    return frozenset(([SPREAD] if self.spread else []) + ([FP32_UPD] if self.fp32_upd else []))

  @property
  def container_bits(self):
    return 8 if self.bits <= 8 else 16 if self.bits <= 16 else 32

  @property
  def diff_bits(self):
    """Width of q - zp in the reference's dequantize: np.result_type(container, zero-point type), 32 at most."""
    return min(32, max(self.container_bits, np.dtype(ZP_DTYPES[self.zp]).itemsize * 8)) if self.zp else 8

  @property
  def zp_via_f64(self):
    return bool(self.zp) and np.dtype(ZP_DTYPES[self.zp]).itemsize >= 4

  @property
  def data_key(self):
    return (self.rows, self.d, self.mode, self.bs, self.bits, bool(self.zp), self.seed, self.narrow, self.wrap, self.f64)


def route_of(c):
  return route(c.rows, c.d, c.mode, c.bs, c.bits, bool(c.zp), "f64" if c.f64 else "f32", c.env)


SHORT = {"gptq_rows_kernel": "rows", "gptq_block_kernel<float, 32, true>": "f32x32plain",
         "gptq_block_kernel<float, 32, false>": "f32x32general", "gptq_block_kernel<double, 32, true>": "f64x32plain",
         "gptq_block_kernel<double, 32, false>": "f64x32general", "gptq_block_kernel<float, 16, true>": "f32x16plain",
         "gptq_block_kernel<float, 16, false>": "f32x16general", "gptq_block_kernel<double, 16, true>": "f64x16plain",
         "gptq_block_kernel<double, 16, false>": "f64x16general"}


def case_id(c):
  chain, kind, k, split = route_of(c)
  far = "far_none" if kind == "none" else f"far_{kind}_K{k}_{'bf16x3' if split else 'gemm'}"
  extra = "".join([f"-zp_{c.zp}" if c.zp else "", "-f64" if c.f64 else "", "-narrow" if c.narrow else "",
                   "-wrap" if c.wrap else "", "-spread" if c.spread else "", "-fp32_upd" if c.fp32_upd else ""])
  return f"{'+'.join(SHORT[n] for n in chain)}-{far}-{c.rows}x{c.d}-mode{c.mode}-bs{c.bs}-int{c.bits}{extra}"


def features(c):
  """The elements of ALL_ROUTES one case covers."""
  chain, kind, k, split = route_of(c)
  f = {("chain", n) for n in chain}
  if kind != "none":
    f.add(("far", kind, k, "bf16x3" if split else "gemm"))
    if not split:
      f.add(("far", kind, "launch_gemm", c.d))
  if chain == ("gptq_rows_kernel",):
    f |= {("rows", "blocks in the last group", (c.d - 1) % GROUP // NB + 1), ("rows", "rows", c.rows),
          ("rows", "scales", c.mode, c.bs)}
    if c.d > GROUP:
      f.add(("rows", "more than one group"))
    if -(-c.rows // 16) >= 512:
      f.add(("rows", "512 workgroups"))
    if c.bits == 8:
      f.add(("narrow", "rows", c.narrow))
  general32, plain32 = "gptq_block_kernel<float, 32, false>", "gptq_block_kernel<float, 32, true>"
  if plain32 in chain:
    if c.spread:
      f.add(("f32x32plain", "spread"))
    if c.d % NB:
      f.add(("f32x32plain", "full blocks of a ragged layer"))
    if c.bits > 8:
      f.add(("f32x32plain", "q32 store"))
  if general32 in chain:
    if c.zp:
      f |= {("f32x32general", "diff_bits", c.diff_bits), ("f32x32general", "zp_via_f64", c.zp_via_f64)}
      if c.wrap:
        f.add(("f32x32general", "q - zp wraps", c.diff_bits))
    if c.mode == 2 and c.bs % 32:
      f.add(("f32x32general", "per-step lookup", c.bs))
    if c.d % NB:
      f.add(("f32x32general", "ragged last block", c.d))
    if c.bits > 16:
      f.add(("f32x32general", "container32"))
    if c.bits == 8:
      f.add(("narrow", "general", c.narrow))
  if c.rows >= 8192 and chain != ("gptq_rows_kernel",):
    f.add(("16 lanes", "ragged" if c.d % NB else "packed 4-byte store" if not c.zp else "full block, zero points"))
  if split and c.rows >= 8192:
    f.add(("far", "bf16x3", "8192x1024"))
  if c.fp32_upd and not split and route(c.rows, c.d, c.mode, c.bs, c.bits, bool(c.zp), "f32", frozenset())[3]:
    f.add(("far", "fp32 fallback at a bf16x3 shape"))
  return f


ALL_ROUTES = (
    {("chain", n) for n in SHORT}
    | {("rows", "blocks in the last group", n) for n in (1, 2, 3, 4)} | {("rows", "more than one group")}
    | {("rows", "rows", r) for r in (1, 16, 17, 37)} | {("rows", "512 workgroups")}
    | {("rows", "scales", mode, bs) for mode, bs in ((0, 0), (1, 0), (2, 32), (2, 64), (2, 128))}
    | {("narrow", kernel, on) for kernel in ("rows", "general") for on in (False, True)}
    | {("f32x32plain", what) for what in ("spread", "full blocks of a ragged layer", "q32 store")}
    | {("f32x32general", "diff_bits", b) for b in (8, 16, 32)} | {("f32x32general", "zp_via_f64", v) for v in (False, True)}
    | {("f32x32general", "q - zp wraps", b) for b in (8, 16)}
    | {("f32x32general", "per-step lookup", bs) for bs in (8, 100)}
    | {("f32x32general", "ragged last block", d) for d in (33, 65, 200)} | {("f32x32general", "container32")}
    | {("16 lanes", what) for what in ("ragged", "packed 4-byte store")}
    | {("far", kind, k, how) for kind, k in (("lazy", GROUP), ("per_block", NB)) for how in ("gemm", "bf16x3")}
    | {("far", kind, "launch_gemm", d) for kind in ("lazy", "per_block") for d in (320, 704)}
    | {("far", "bf16x3", "8192x1024"), ("far", "fp32 fallback at a bf16x3 shape")})

ROWS, PLAIN32, GENERAL32 = "gptq_rows_kernel", "gptq_block_kernel<float, 32, true>", "gptq_block_kernel<float, 32, false>"

CASES = [
    # ---- gptq_rows_kernel: groups of 1 .. 4 blocks, several groups, idle quads, every scale layout it takes
    Case(1, 64, mode=1, bits=3, seed=1, want=(("rows", "rows", 1), ("rows", "blocks in the last group", 1))),
    Case(16, 128, mode=0, bits=4, seed=4, want=(("rows", "rows", 16), ("rows", "blocks in the last group", 2), ("rows", "scales", 0, 0))),
    Case(17, 192, mode=2, bs=32, bits=4, want=(("rows", "rows", 17), ("rows", "blocks in the last group", 3), ("rows", "scales", 2, 32))),
    Case(37, 256, mode=2, bs=64, bits=8, narrow=True, want=(("rows", "rows", 37), ("rows", "blocks in the last group", 4), ("rows", "scales", 2, 64), ("narrow", "rows", True))),
    Case(37, 320, mode=2, bs=32, bits=4, want=(("rows", "more than one group"), ("far", "lazy", "launch_gemm", 320))),
    Case(37, 704, mode=1, bits=4, want=(("rows", "scales", 1, 0), ("far", "lazy", "launch_gemm", 704), ("far", "lazy", GROUP, "gemm"))),
    Case(37, 704, mode=2, bs=32, bits=8, narrow=True, want=(("far", "per_block", "launch_gemm", 704), ("far", "per_block", NB, "gemm"))),
    Case(17, 384, mode=2, bs=128, bits=8, want=(("rows", "scales", 2, 128), ("narrow", "rows", False))),
    Case(16, 320, mode=0, bits=8, narrow=True, want=(("far", "per_block", "launch_gemm", 320),)),
    Case(17, 320, mode=1, bits=3, seed=1, want=(("chain", ROWS),)),
    # ---- gptq_block_kernel<float, 32, true>
    Case(17, 192, mode=2, bs=32, bits=4, spread=True, want=(("f32x32plain", "spread"),)),
    Case(37, 320, mode=1, bits=8, spread=True, want=(("f32x32plain", "spread"),)),
    Case(20, 320, mode=1, bits=12, want=(("f32x32plain", "q32 store"),)),
    Case(20, 128, mode=2, bs=64, bits=16, want=(("f32x32plain", "q32 store"),)),
    # ---- gptq_block_kernel<float, 32, false> (with the plain kernel on the full blocks of a ragged layer)
    Case(33, 330, mode=0, bits=4, zp="i32", want=(("f32x32general", "diff_bits", 32), ("f32x32general", "zp_via_f64", True))),
    Case(20, 200, mode=2, bs=8, bits=4, zp="i8", want=(("f32x32general", "per-step lookup", 8), ("f32x32general", "diff_bits", 8), ("f32x32general", "zp_via_f64", False))),
    Case(37, 200, mode=2, bs=100, bits=8, zp="i16", want=(("f32x32general", "per-step lookup", 100), ("f32x32general", "diff_bits", 16), ("narrow", "general", False))),
    Case(37, 320, mode=2, bs=32, bits=8, zp="i8", wrap=True, want=(("f32x32general", "q - zp wraps", 8),)),
    Case(20, 128, mode=0, bits=16, zp="i16", wrap=True, want=(("f32x32general", "q - zp wraps", 16),)),
    Case(20, 200, mode=2, bs=8, bits=8, narrow=True, want=(("narrow", "general", True), ("f32x32general", "ragged last block", 200))),
    Case(20, 200, mode=2, bs=100, bits=4, want=(("f32x32general", "per-step lookup", 100),)),
    Case(9, 65, mode=1, bits=3, want=(("f32x32general", "ragged last block", 65), ("f32x32plain", "full blocks of a ragged layer"))),
    Case(5, 33, mode=1, bits=3, zp="i32", want=(("f32x32general", "ragged last block", 33),)),
    Case(12, 136, mode=0, bits=20, want=(("f32x32general", "container32"),)),
    Case(12, 128, mode=0, bits=20, zp="i32", want=(("f32x32general", "container32"),)),
    # ---- float64 scales
    Case(17, 192, mode=2, bs=32, bits=4, f64=True, want=(("chain", "gptq_block_kernel<double, 32, true>"),)),
    Case(33, 330, mode=1, bits=8, zp="i32", f64=True, want=(("chain", "gptq_block_kernel<double, 32, false>"),)),
    Case(20, 320, mode=1, bits=12, f64=True, want=(("chain", "gptq_block_kernel<double, 32, true>"),)),
    # ---- 16 lanes per row
    Case(8200, 136, mode=1, bits=4, want=(("chain", "gptq_block_kernel<float, 16, true>"), ("chain", "gptq_block_kernel<float, 16, false>"), ("16 lanes", "ragged"))),
    Case(8200, 136, mode=1, bits=4, f64=True, want=(("chain", "gptq_block_kernel<double, 16, true>"), ("chain", "gptq_block_kernel<double, 16, false>"), ("16 lanes", "ragged"))),
    Case(8192, 128, mode=2, bs=32, bits=8, narrow=True, spread=True, want=(("chain", "gptq_block_kernel<float, 16, true>"), ("16 lanes", "packed 4-byte store"))),
    Case(8192, 128, mode=2, bs=64, bits=4, f64=True, want=(("chain", "gptq_block_kernel<double, 16, true>"), ("16 lanes", "packed 4-byte store"))),
    Case(8192, 128, mode=1, bits=4, zp="i32", want=(("chain", "gptq_block_kernel<float, 16, false>"),)),
    # ---- the far update on the bf16 matrix cores, and its float32 fallback at the same shape
    # (4 bits on 4096 columns: see make_case on graded scales; the 6-bit case has one scale per row)
    Case(128, 4096, mode=2, bs=128, bits=4, want=(("far", "lazy", GROUP, "bf16x3"),)),
    Case(128, 4096, mode=1, bits=6, want=(("far", "lazy", GROUP, "bf16x3"),)),
    Case(128, 4096, mode=2, bs=32, bits=8, narrow=True, want=(("far", "per_block", NB, "bf16x3"),)),
    Case(128, 4096, mode=2, bs=128, bits=4, fp32_upd=True, want=(("far", "fp32 fallback at a bf16x3 shape"),)),
    Case(8192, 1024, mode=1, bits=6, want=(("far", "bf16x3", "8192x1024"), ("rows", "512 workgroups"))),
]
SMALL = [c for c in CASES if c.d <= 704]          # the sensitivity loop runs on these


# --------------------------------------------------------------------------------------------------- exact inputs ---
def bounds(bits, narrow):
  return -(1 << (bits - 1)) + (1 if narrow else 0), (1 << (bits - 1)) - 1


def make_r(d, rng, gentle_tail):
  """R [d, d] int8, strictly upper: up to four non-zeros in {-2, -1, 1, 2} per row inside the row's own block and
  one in every later block (rows of the last `gentle_tail` columns: +-1 only)."""
  R = np.zeros((d, d), np.int8)
  nblocks = -(-d // NB)
  vals = np.array([-2, -1, 1, 2], np.int8)
  for i in range(d):
    b1 = min((i // NB + 1) * NB, d)
    n = min(IN_BLOCK, b1 - i - 1)
    if n:
      R[i, rng.choice(np.arange(i + 1, b1), n, replace=False)] = rng.choice(vals, n, p=(0.1, 0.4, 0.4, 0.1))
  rows = np.arange(d)
  for b in range(1, nblocks):
    width = min(NB, d - b * NB)
    above = rows[: b * NB]
    R[above, b * NB + rng.integers(0, width, above.size)] = rng.choice(vals[1:3], above.size)
  if gentle_tail:
    R[d - gentle_tail:] = np.sign(R[d - gentle_tail:])
  return R


def make_case(rows, d, scale_mode, block_size, bits, zero_points, seed, narrow=False, wrap=False, scale_dtype=np.float32):
  """(w [rows, d] float32, hinv [d, d] float32, scale [1] / [rows] / [rows * d / block_size], zp int32 like scale or None).
  wrap: q - zp wraps in the target's container wherever a level within |zp| of one clip bound occurs, and the error of
  such a column is 2^bits steps; those levels are kept to a row's last WRAP_TAIL columns (elsewhere they would push
  everything behind them to a clip bound) and the body stays WRAP_MARGIN levels away from that bound.
  Below 5 bits on more than 2048 columns under scale_mode 2 the scales grow along the row (see the file's docstring)."""
  rng = np.random.default_rng([rows, d, scale_mode, block_size, bits, int(zero_points), seed])
  r, c = np.arange(rows)[:, None], np.arange(d)[None, :]
  # scales 2^-3 .. 2^-6; fewer where the levels alone are 2^15 and more, and on long rows
  spread = (4 if bits <= 12 else 2 if bits <= 16 else 1) if d <= 2048 else 2
  graded = scale_mode == 2 and bits < 5 and d > 2048
  if scale_mode == 0:
    scale = np.array([2.0 ** -5])
    zp = np.array([-3], np.int32) if zero_points else None
    entry = np.zeros((rows, d), np.int64)
  else:
    nblk = d // block_size if scale_mode == 2 else 1
    blk = c // block_size if scale_mode == 2 else np.zeros((1, d), np.int64)
    j = np.arange(nblk)[None, :]
    scale = 2.0 ** (-3 - (r + j) % spread)
    if graded:                       # ... growing along the row: what earlier groups send shrinks in the steps of later ones
      scale = 2.0 ** (-3 - np.minimum((d - 1) // GROUP - j * block_size // GROUP, 13) - j % 2 - r % 2)
    scale = scale.reshape(-1)
    zp = (((3 * r + 5 * j + seed) % 9) - 4).astype(np.int32).reshape(-1) if zero_points else None
    entry = r * nblk + blk
  S = scale[entry]
  Z = zp[entry].astype(np.int64) if zero_points else np.zeros((rows, d), np.int64)
  lo, hi = bounds(bits, narrow)
  # v = w / s + zp in eighths. The body: from two levels below the range to two above it at 8 bits and more; narrower
  # below 8 bits (BODY) and on long rows, where a few values of their own visit the `margin` levels next to each bound.
  shape, long_row = (rows, d), d > 2048
  body = BODY(bits, d)
  if body is None:
    v8 = rng.integers(8 * (lo - 2), 8 * (hi + 2) + 1, shape)
  else:
    v8 = rng.integers(-int(8 * body), int(8 * body) + 1, shape)
  if bits >= 5 and long_row:
    margin = min(24, 3 << (bits - 3))
    v8 = rng.integers(8 * (lo + margin), 8 * (hi - margin) + 1, shape)
    inward = rng.integers(0, 8 * (margin + 2) + 1, shape)
    v8 = np.where(rng.random(shape) < 0.015, np.where(rng.random(shape) < 0.5, 8 * (hi + 2) - inward, 8 * (lo - 2) + inward), v8)
  # ... and everywhere some values half a step to a step and a half beyond either bound
  out = rng.random(shape) < (0.015 if graded else OUTLIERS)
  beyond = rng.integers(4, 9 if long_row else 13, shape)
  far_side = np.where(rng.random(shape) < 0.5, 8 * hi + beyond, 8 * lo - beyond)
  v8 = np.where(out, far_side, v8)
  if wrap:
    assert zero_points
    side = -np.sign(Z)                                            # +1: q - zp wraps at the upper bound; -1: at the lower
    top = np.where(side > 0, hi, -lo)                             # in u = side * v, the wrapping bound ...
    bottom = np.where(side > 0, -lo, hi)                          # ... and the harmless one
    u8 = -8 * (bottom + 2) + rng.integers(0, 1 << 62, shape) % (8 * (top - WRAP_MARGIN + bottom + 2) + 1)
    u8 = np.where(out, -8 * bottom - beyond, u8)
    tail = c >= d - WRAP_TAIL
    level = top - WRAP_MARGIN + (r * WRAP_TAIL + (c - (d - WRAP_TAIL))) % (WRAP_MARGIN + 3)
    u8 = np.where(tail, 8 * level + rng.integers(-3, 5, shape), u8)
    v8 = np.where(side == 0, v8, side * u8)
  w = (S * (v8 - 8 * Z) / 8.0).astype(np.float32)
  hd = 2.0 ** ((7 * np.arange(d) + seed) % 5 - 2)
  R = make_r(d, rng, WRAP_TAIL if wrap else 0)
  hinv = R.astype(np.float32) * hd[:, None].astype(np.float32)
  hinv[np.arange(d), np.arange(d)] = hd
  hinv[np.tri(d, d, -1, dtype=bool)] = np.nan
  return w, hinv, scale.astype(scale_dtype), zp


@functools.lru_cache(maxsize=3)
def data(key):
  rows, d, mode, bs, bits, zero_points, seed, narrow, wrap, f64 = key
  return make_case(rows, d, mode, bs, bits, zero_points, seed, narrow=narrow, wrap=wrap,
                   scale_dtype=np.float64 if f64 else np.float32)


# ------------------------------------------------------------------------------------------------------ reference ---
def wrap_to(x, bits):
  return x if bits >= 64 else ((x + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))


def reference(w, hinv, scale, zp, scale_mode, block_size, bits, narrow, diff_bits, dtype, record=False):
  """ref gptq.py:180-214 in `dtype`, vectorised over the rows: column-serial quantize, dequantize, divide and rank-1
  update inside 64-column blocks, one eb @ hinv[b0:b1, b1:] per block. Returns (q int64 [rows, d], stats): with
  record, stats holds the largest magnitude in grid units that any element can hold under any order of the additions
  (|w| plus the magnitudes of everything ever subtracted from it; errors, dequantized values and products included)
  and the number of exact .5 ties rounded inside the range."""
  rows, d = w.shape
  fw = w.astype(dtype)
  nblk = d // block_size if scale_mode == 2 else 1
  sc = scale.astype(dtype).reshape(-1, nblk) if scale_mode else scale.astype(dtype).reshape(1, 1)
  zz = None if zp is None else (zp.astype(np.int64).reshape(-1, nblk) if scale_mode else zp.astype(np.int64).reshape(1, 1))
  lo, hi = bounds(bits, narrow)
  grid = float(scale.min()) / 8
  q_all = np.zeros((rows, d), np.int64)
  reach = np.abs(fw).astype(np.float64) if record else None
  peak, ties = 0.0, 0
  for b0 in range(0, d, NB):
    b1 = min(b0 + NB, d)
    wb = fw[:, b0:b1]
    eb = np.zeros((rows, b1 - b0), dtype)
    hb = hinv[b0:b1, b0:b1].astype(dtype)
    for i in range(b1 - b0):
      col = wb[:, i]
      j = (b0 + i) // block_size if scale_mode == 2 else 0
      s = sc[:, j]
      z = 0 if zz is None else zz[:, j]
      v = col / s + (0 if zz is None else z.astype(dtype))
      q = np.clip(np.rint(v), lo, hi).astype(np.int64)
      dq = (q if zz is None else wrap_to(q - z, diff_bits)).astype(dtype) * s
      diff = col - dq
      e = diff / hb[i, i]
      eb[:, i] = e
      q_all[:, b0 + i] = q
      if record:
        ties += int(((v - np.floor(v) == 0.5) & (v > lo) & (v < hi)).sum())
        peak = max(peak, float(np.abs(diff).max()), float(np.abs(dq).max()), float(np.abs(e * hb[i, i]).max()))
      if i < b1 - b0 - 1:
        p = np.outer(e, hb[i, i + 1:])
        wb[:, i + 1:] -= p
        if record:
          reach[:, b0 + i + 1:b1] += np.abs(p)
    if b1 < d:
      hf = hinv[b0:b1, b1:].astype(dtype)
      fw[:, b1:] -= eb @ hf
      if record:
        reach[:, b1:] += np.abs(eb).astype(np.float64) @ np.abs(hf).astype(np.float64)
  stats = None
  if record:
    assert np.isfinite(fw).all()
    stats = types.SimpleNamespace(peak_units=max(peak, float(reach.max())) / grid, ties=ties, lo=lo, hi=hi)
  return q_all, stats


def per_element(c, a):
  """scale or zero points as stored -> [rows, d]."""
  return np.broadcast_to(a.reshape(c.rows if c.mode else 1, -1).repeat(c.bs if c.mode == 2 else c.d, axis=1), (c.rows, c.d))


def run_reference(c, dtype, record=False, hinv=None):
  w, h, scale, zp = data(c.data_key)
  return reference(w, h if hinv is None else hinv, scale, zp, c.mode, c.bs, c.bits, c.narrow, c.diff_bits, dtype, record)


@functools.lru_cache(maxsize=None)
def expected(key_and_diff):
  """(q, stats) of the float64 reference, once per data set."""
  c = next(c for c in CASES if (c.data_key, c.diff_bits) == key_and_diff)
  return run_reference(c, np.float64, record=True)


def expected_of(c):
  return expected((c.data_key, c.diff_bits))


def unique_data(cases):
  seen, out = set(), []
  for c in cases:
    if (c.data_key, c.diff_bits) not in seen:
      seen.add((c.data_key, c.diff_bits))
      out.append(c)
  return out


# ------------------------------------------------------------------------------------------------- tests without a GPU ---
def test_environment_leaves_the_routes_alone():
  assert env_is_default()


def test_every_route_has_a_case():
  reached = set()
  for c in CASES:
    reached |= features(c)
  assert ALL_ROUTES - reached == set(), sorted(map(str, ALL_ROUTES - reached))
  assert len(ALL_ROUTES) == 9 + 5 + 5 + 5 + 4 + 3 + 5 + 2 + 2 + 4 + 2 + 4 + 4 + 2
  assert len({case_id(c) for c in CASES}) == len(CASES)


def test_every_case_reaches_the_route_it_is_there_for():
  for c in CASES:
    assert c.want and set(c.want) <= features(c), (case_id(c), set(c.want) - features(c))
    assert set(c.want) <= ALL_ROUTES, case_id(c)
    assert not (c.spread and route_of(c)[0] == (ROWS,)) and c.bits <= 25
    assert c.mode != 2 or c.d % c.bs == 0


def test_route_restates_the_host_at_its_thresholds():
  none = frozenset()

  def chain(rows, d, mode=1, bs=0, bits=4, zp=False, st="f32", env=none):
    return route(rows, d, mode, bs, bits, zp, st, env)[0]

  assert chain(37, 256) == (ROWS,) and chain(37, 256, env={SPREAD}) == (PLAIN32,)
  assert chain(37, 200) == (PLAIN32, GENERAL32) and chain(37, 33) == (GENERAL32,)
  assert chain(37, 256, zp=True) == (GENERAL32,) and chain(37, 256, bits=9) == (PLAIN32,)
  assert chain(37, 256, bits=16) == (PLAIN32,) and chain(37, 256, bits=17) == (GENERAL32,)
  assert chain(37, 256, mode=2, bs=32) == (ROWS,) and chain(37, 256, mode=2, bs=16) == (GENERAL32,)
  assert chain(37, 256, mode=0, bs=16) == (ROWS,)                                  # block_size counts under mode 2 only
  assert chain(8191, 128, st="f64") == ("gptq_block_kernel<double, 32, true>",)
  assert chain(8192, 128, st="f64") == ("gptq_block_kernel<double, 16, true>",)
  assert chain(8192, 128) == (ROWS,)
  assert route(37, 256, 1, 0, 4, False, "f32", none)[1:] == ("none", 0, False)
  assert route(37, 257, 1, 0, 4, False, "f32", none)[1:] == ("lazy", 256, False)
  assert route(37, 320, 1, 0, 7, False, "f32", none)[1:] == ("lazy", 256, False)
  assert route(37, 320, 1, 0, 8, False, "f32", none)[1:] == ("per_block", 64, False)
  assert route(128, 4096, 1, 0, 4, False, "f32", none)[3] and not route(128, 4096, 1, 0, 4, False, "f32", {FP32_UPD})[3]
  assert not route(128, 3968, 1, 0, 4, False, "f32", none)[3] and not route(127, 4096, 1, 0, 4, False, "f32", none)[3]
  assert route(8192, 1024, 1, 0, 4, False, "f32", none)[3] and not route(8064, 1024, 1, 0, 4, False, "f32", none)[3]
  assert not route(8192, 896, 1, 0, 4, False, "f32", none)[3]


def test_workspace_query_follows_the_route(lib, monkeypatch):
  monkeypatch.delenv(FP32_UPD, raising=False)
  plain = lambda rows, d: (rows * d + rows * GROUP) * 4
  assert lib.mi355q_gptq_apply_workspace_bytes(0, 64) == 0 and lib.mi355q_gptq_apply_workspace_bytes(64, -1) == 0
  for rows, d in ((37, 704), (128, 3968), (8064, 1024)):
    assert lib.mi355q_gptq_apply_workspace_bytes(rows, d) == plain(rows, d)
  for rows, d in ((128, 4096), (8192, 1024)):
    assert lib.mi355q_gptq_apply_workspace_bytes(rows, d) > plain(rows, d)
  monkeypatch.setenv(FP32_UPD, "1")
  assert lib.mi355q_gptq_apply_workspace_bytes(128, 4096) == plain(128, 4096)


@pytest.mark.parametrize("c", unique_data(CASES), ids=case_id)
def test_inputs_are_exact_and_sharp(c):
  """The conditions on every data set that make one bit pattern correct and the comparison sharp."""
  w, hinv, scale, zp = data(c.data_key)
  rows, d = w.shape
  # -- the recipe
  assert w.dtype == np.float32 and hinv.dtype == np.float32 and scale.dtype == (np.float64 if c.f64 else np.float32)
  assert np.array_equal(np.frexp(scale)[0], np.full(scale.shape, 0.5)) and np.array_equal(np.frexp(np.diag(hinv))[0], np.full(d, 0.5))
  assert len(set(np.diag(hinv).tolist())) >= min(d, 5)
  if c.mode:
    sc = scale.reshape(rows, -1)
    assert rows == 1 or (sc[1:] != sc[:-1]).all()
    assert sc.shape[1] == 1 or (sc[:, 1:] != sc[:, :-1]).all()       # bs == 32: the two halves of a 64-column block differ
  if zp is not None:
    assert zp.dtype == np.int32 and zp.shape == scale.shape and zp.any() and np.abs(zp).max() <= 4
    assert scale.size == 1 or ((zp > 0).any() and (zp < 0).any())
  upper = np.triu(np.ones((d, d), bool), 1)
  assert np.isnan(hinv[np.tri(d, d, -1, dtype=bool)]).all() and not np.isnan(hinv[upper]).any()
  R = np.where(upper, np.nan_to_num(hinv) / np.diag(hinv)[:, None], 0.0)
  assert np.isin(R, (-2, -1, 0, 1, 2)).all() and np.abs(R).max() == 2
  blocks = -(-d // NB)
  for b in range(blocks):
    mine = R[b * NB:(b + 1) * NB]
    inside = (mine[:, b * NB:(b + 1) * NB] != 0).sum(axis=1)
    left = np.minimum(IN_BLOCK, min((b + 1) * NB, d) - 1 - np.arange(b * NB, min((b + 1) * NB, d)))
    assert np.array_equal(inside, left)                              # four per row inside its own block where four fit
    for later in range(b + 1, blocks):                               # and every row reaches every later block
      assert (mine[:, later * NB:(later + 1) * NB] != 0).any(axis=1).all(), (b, later)
  # -- exactness and magnitude
  q64, stats = expected_of(c)
  q32, _ = run_reference(c, np.float32)
  assert np.array_equal(q32, q64)
  print(f"{case_id(c)}: largest magnitude 2^{np.log2(stats.peak_units):.1f} grid units")
  assert stats.peak_units < 2.0 ** 23
  # -- clipping, levels, ties
  lo, hi = bounds(c.bits, c.narrow)
  share = float(((q64 == lo) | (q64 == hi)).mean())
  print(f"{case_id(c)}: {100 * share:.1f} % of the integers at a clip bound, {stats.ties} ties")
  assert 0.01 <= share <= 0.5
  v = w.astype(np.float64) / per_element(c, scale.astype(np.float64))
  if zp is not None:
    v = v + per_element(c, zp)
  assert np.array_equal(v * 8, np.rint(v * 8)) and (v > hi + 0.5).any() and (v < lo - 0.5).any()
  if c.bits <= 8:
    assert np.array_equal(np.unique(q64), np.arange(lo, hi + 1))
  assert stats.ties >= 1
  # -- the oracle the rest of the suite trusts, where it can express the case
  if (c.zp in ("", "i32")) and not c.f64 and c.narrow == (not c.zp and c.bits >= 8):
    from oracle import aeq_oracle as O
    gran = ("TENSORWISE", "CHANNELWISE", "BLOCKWISE")[c.mode]
    shape = ((1, 1), (rows, 1), (rows, d // c.bs if c.mode == 2 else 1))[c.mode]
    z = np.zeros(shape, np.int32) if zp is None else zp.reshape(shape)
    got = O.gptq_apply(w, scale.reshape(shape), z, c.bits, zp is None, None, gran, c.bs, hinv=hinv)
    assert got.dtype == (np.int8 if c.bits <= 8 else np.int16 if c.bits <= 16 else np.int32)
    assert np.array_equal(got.astype(np.int64), q64)


WRAPPING = [c for c in CASES if c.wrap]


@pytest.mark.parametrize("c", WRAPPING, ids=case_id)
def test_wrapping_cases_wrap(c):
  """q - zp leaves its container in some rows, on both sides where zero points of both signs occur, and the integers
  differ from those of a sweep that does not wrap."""
  w, hinv, scale, zp = data(c.data_key)
  q, _ = expected_of(c)
  rows, d = w.shape
  Z = per_element(c, zp).astype(np.int64)
  diff = q - Z
  half = 1 << (c.diff_bits - 1)
  assert c.diff_bits == c.container_bits
  assert (diff >= half).any() and ((diff < -half).any() or not (zp > 0).any())
  unwrapped, _ = reference(w, hinv, scale, zp, c.mode, c.bs, c.bits, c.narrow, 32, np.float64)
  assert (unwrapped != q).any()


@pytest.mark.parametrize("c", unique_data(SMALL), ids=case_id)
def test_every_block_of_hinv_moves_integers(c):
  """Zeroing Hinv[block b, block b'] alone (b < b') changes integers inside block b'; zeroing the strictly upper part
  of a diagonal block changes that block's integers: no catch-up tile, far-update tile or chain can be dropped unseen."""
  _, hinv, _, _ = data(c.data_key)
  q, _ = expected_of(c)
  d = c.d
  blocks = -(-d // NB)
  for b in range(blocks):
    r0, r1 = b * NB, min((b + 1) * NB, d)
    if r1 - r0 > 1:
      h = hinv.copy()
      h[r0:r1, r0:r1][np.triu(np.ones((r1 - r0, r1 - r0), bool), 1)] = 0.0
      assert (run_reference(c, np.float64, hinv=h)[0][:, r0:r1] != q[:, r0:r1]).any(), ("diagonal block", b)
    for later in range(b + 1, blocks):
      c0, c1 = later * NB, min((later + 1) * NB, d)
      h = hinv.copy()
      h[r0:r1, c0:c1] = 0.0
      assert (run_reference(c, np.float64, hinv=h)[0][:, c0:c1] != q[:, c0:c1]).any(), ("blocks", b, later)


def test_entries_refuse_bad_arguments_before_they_launch(lib, monkeypatch):
  monkeypatch.delenv(FP32_UPD, raising=False)
  err = lib.mi355q_last_error
  rows, d = 4, 64
  need = lib.mi355q_gptq_apply_workspace_bytes(rows, d)
  assert need == (rows * d + rows * GROUP) * 4
  buf = ctypes.create_string_buffer(need + 64)                 # host memory: every call here returns before it launches
  base = (ctypes.addressof(buf) + 15) & ~15
  q = ctypes.create_string_buffer(b"\x5a" * (rows * d * 4), rows * d * 4)

  def call(fn, bits, **kw):
    a = dict(w=base, rows=rows, d=d, hinv=base, scale=base, f64=0, zp=None, mode=1, bs=0, bits=bits, narrow=0, via=0,
             diff=8, q=ctypes.addressof(q), ws=base, ws_bytes=need)
    a.update(kw)
    return fn(a["w"], a["rows"], a["d"], a["hinv"], a["scale"], a["f64"], a["zp"], a["mode"], a["bs"], a["bits"],
              a["narrow"], a["via"], a["diff"], a["q"], a["ws"], a["ws_bytes"], None)

  for fn, good, bad in ((lib.mi355q_gptq_apply_f32, 4, (-1, 0, 1, 9, 16, 33)), (lib.mi355q_gptq_apply_wide_f32, 12, (1, 4, 8, 33, 64))):
    for bits in bad:
      assert call(fn, bits) == -3 and b"bits" in err()
    for mode in (-1, 3):
      assert call(fn, good, mode=mode) == -1 and b"scale_mode" in err()
    for bs in (0, -32, 48, 128):
      assert call(fn, good, mode=2, bs=bs) == -2 and b"not divisible by block size" in err()
    for name in ("w", "hinv", "scale", "q"):
      assert call(fn, good, **{name: None}) == -1 and b"null pointer" in err()
    assert call(fn, good, ws=None) == -1 and b"workspace too small" in err()
    assert call(fn, good, ws_bytes=need - 1) == -1 and f"need {need} bytes".encode() in err()
    assert call(fn, good, rows=-1) == -1 and call(fn, good, d=-1) == -1 and b"negative shape" in err()
    # an empty layer is a no-op, whatever the other arguments, and leaves no message behind
    for empty in (dict(rows=0), dict(d=0)):
      assert call(fn, good, w=None, hinv=None, scale=None, q=None, ws=None, ws_bytes=0, **empty) == 0 and err() == b""
      assert call(fn, 99, mode=7, **empty) == 0 and err() == b""
  assert q.raw == b"\x5a" * (rows * d * 4)


# ---------------------------------------------------------------------------------------------------- tests on a GPU ---
def same_bits(got, exp, what, locate=None):
  assert got.dtype == exp.dtype and got.shape == exp.shape, what
  a, b = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
  u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
  bad = np.flatnonzero(a.view(u) != b.view(u))
  if bad.size:
    first = [locate(int(f)) if locate else int(f) for f in bad[:4]]
    raise AssertionError(f"{what}: {bad.size} of {a.size} elements differ; first at {first}: {a[bad[:4]].tolist()} "
                         f"instead of {b[bad[:4]].tolist()}")


def run_exact(m, c, monkeypatch):
  for name, on in ((SPREAD, c.spread), (FP32_UPD, c.fp32_upd)):       # both are read on every call
    if on:
      monkeypatch.setenv(name, "1")
    else:
      monkeypatch.delenv(name, raising=False)
  torch, L = m.torch, m.L
  w, hinv, scale, zp = data(c.data_key)
  want, stats = expected_of(c)
  assert stats.peak_units < 2.0 ** 23
  rows, d = w.shape
  wide = c.bits > 8
  qdt = np.dtype(np.int32 if wide else np.int8)
  dev = lambda a: torch.from_numpy(a).cuda()
  w_d, h_d, s_d = dev(w), dev(hinv), dev(scale)
  z_d = None if zp is None else dev(zp)
  need = L.mi355q_gptq_apply_workspace_bytes(rows, d)
  plain = (rows * d + rows * GROUP) * 4
  assert (need > plain) == route_of(c)[3] and need >= plain
  ws_d = torch.full((need + WS_TAIL,), WS_FILL, dtype=torch.uint8, device="cuda")
  q_host = np.full(GUARD + rows * d + GUARD, SENTINEL[qdt], qdt)
  q_d = dev(q_host)
  for t in (w_d, h_d, s_d, q_d, ws_d):
    assert t.data_ptr() % 16 == 0
  fn = L.mi355q_gptq_apply_wide_f32 if wide else L.mi355q_gptq_apply_f32
  st = fn(m.rt.ptr(w_d), rows, d, m.rt.ptr(h_d), m.rt.ptr(s_d), 1 if c.f64 else 0, m.rt.ptr(z_d), c.mode, c.bs, c.bits,
          1 if c.narrow else 0, 1 if c.zp_via_f64 else 0, c.diff_bits, ctypes.c_void_p(q_d.data_ptr() + GUARD * qdt.itemsize),
          m.rt.ptr(ws_d), need, m.rt.stream_ptr())
  assert st == 0, (st, L.mi355q_last_error())
  torch.cuda.synchronize()
  exp = q_host.copy()
  exp[GUARD:GUARD + rows * d] = want.reshape(-1).astype(qdt)

  def locate(flat):
    e = flat - GUARD
    if e < 0 or e >= rows * d:
      return f"buffer[{flat}] (a guard)"
    r, col = divmod(e, d)
    return (f"(row {r}, column {col}: column {col % NB} of block {col // NB}, block {col % GROUP // NB} of group {col // GROUP}, "
            f"lane {col % 4} of the quad)")

  what = case_id(c)
  same_bits(q_d.cpu().numpy(), exp, f"{what}: q and its guards", locate)
  same_bits(ws_d[need:].cpu().numpy(), np.full(WS_TAIL, WS_FILL, np.uint8), f"{what}: bytes behind the workspace")
  same_bits(w_d.cpu().numpy(), w, f"{what}: w")
  same_bits(h_d.cpu().numpy(), hinv, f"{what}: hinv")
  same_bits(s_d.cpu().numpy(), scale, f"{what}: scale")
  if zp is not None:
    same_bits(z_d.cpu().numpy(), zp, f"{what}: zero points")


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_route_returns_the_reference_integers(m, c, monkeypatch):
  """q bit for bit the reference's (as int8, int32 through the wide entry point) inside a sentinel-filled buffer whose
  guards keep their bits, as do the bytes behind a workspace of exactly the size the query asks for and w, hinv, scale
  and the zero points."""
  run_exact(m, c, monkeypatch)
