"""Inputs, routes and expected values for the Hadamard rotation (a7, csrc/hadamard.hip):

  mi355q_hadamard_rotate_f32            fwht_kernel | fwht_tile_kernel<12 | 13 | 14>, float loads and stores
  mi355q_weight_delta_transformed_f32   the same networks with a dequantizing load and `reference - v` as the store

No GPU and no torch are needed here; test_hadamard_route_cases_host.py checks everything below on the CPU and
test_gpu_hadamard_routes.py holds the kernels to it, bit for bit.

route() / delta_route() restate the host's choice of kernel, stage_order() the order in which that kernel runs the
butterfly stages (index bits), read from the passes of the kernels:

  r2    fwht_kernel: stage s = 0 .. L-1 in turn.
  t12   pass 1 bits 0, 1 and then the two top bits of the 4096 tile, 10 and 11; pass 2 bits 2..5; pass 3 bits 6..9.
  t13   pass 1 bits 0, 1, 11, 12; passes 2 and 3 as above; pass 4 bit 10.
  t14   pass 1 bits 0, 1, 12, 13; passes 2 and 3; pass 4 bits 10, 11.

Bits at or above L = log2 h are skipped (in a tile they select the vector). So t12 is r2's order up to h = 1024 and
another one from 2048 on, where bit 10 runs third.

model() is the kernels' arithmetic in NumPy float32 (the build has -ffp-contract=off): every input times
r = float32(1) / sqrt(float32(h)), rounded, then per stage (u + v, u - v) over the pairs 2^b apart.

Three classes of input; the first two have answers that need no model and hold for every order:

  impulse   one +-2^j per vector at position p: output q is +-2^j r (-1)^popcount(p & q), one rounded product (here
            even that is exact) and additions of zeros.
  integer   h = 4^m, |x| < 2^(23 - L): r = 2^-m and every partial sum is an integer < 2^23 times 2^-m, exact in float32.
            The answer is an int64 Sylvester butterfly.
  float     normals times a log-uniform scale per vector (no float32 subnormals), with a dominant last element, -0.0,
            an all-zero vector, a vector with a NaN and one with +inf. Expected: model() under the route's order.

A case has `n_vec` vectors per call (the launch shape is what the routes differ in); a class that needs more vectors
than that is spread over several calls ("batches") of the same shape."""
import dataclasses
import functools

import numpy as np

F = np.float32
TILE_FROM = 256          # the tile kernels start here
TILE = 4096              # elements per workgroup of fwht_tile_kernel<12>
MAX_H = 16384
R2_BLOCK = 2048          # elements per workgroup of fwht_kernel (one vector above that)
ROUTES = ("r2", "t12", "t13", "t14")
SIZES = tuple(1 << k for k in range(15))


def log2(h):
  h = int(h)
  assert h >= 1 and h & (h - 1) == 0 and h <= MAX_H
  return h.bit_length() - 1


# ------------------------------------------------------------------------------------------------ routes
def delta_route(h):
  """mi355q_weight_delta_transformed_f32: the network follows h alone."""
  log2(h)
  if h < TILE_FROM:
    return "r2"
  return "t12" if h <= TILE else "t13" if h == 8192 else "t14"


def route(h, x_aligned, out_aligned):
  """mi355q_hadamard_rotate_f32: the tile kernels need h >= 256 and both pointers 16-byte aligned."""
  return delta_route(h) if x_aligned and out_aligned else "r2"


def stage_order(route_name, h):
  """The index bits in the order in which `route_name` runs their butterflies, for vectors of length h."""
  L = log2(h)
  if route_name == "r2":
    bits = list(range(L))
  else:
    top = {"t12": 12, "t13": 13, "t14": 14}[route_name]
    assert TILE_FROM <= h <= 1 << top
    bits = [0, 1, top - 2, top - 1] + list(range(2, 10)) + list(range(10, top - 2))
  return tuple(b for b in bits if b < L)


# ------------------------------------------------------------------------------------------------ arithmetic
def scale_factor(h):
  return F(1) / np.sqrt(F(h))


def _stage(y, b):
  n, h = y.shape
  s = 1 << b
  y = y.reshape(n, h // (2 * s), 2, s)
  u, v = y[:, :, 0, :], y[:, :, 1, :]
  return np.stack([u + v, u - v], axis=2).reshape(n, h)


def model(x, h, order, scale_after=False):
  """float32 [n, h]: the kernels' arithmetic under `order`. scale_after is a deliberate defect (the product after the
  butterflies) for the host test's proof that the cases tell it apart."""
  r = scale_factor(h)
  y = np.array(x, F).reshape(-1, h)
  with np.errstate(invalid="ignore", over="ignore"):
    if not scale_after:
      y = y * r
    for b in order:
      y = _stage(y, b)
      assert y.dtype == F
    if scale_after:
      y = y * r
  return y


def fwht64(x, h):
  """reshape(x, (-1, h)) @ (Sylvester H_h / sqrt(h)) in float64."""
  y = np.array(x, np.float64).reshape(-1, h)
  for b in range(log2(h)):
    y = _stage(y, b)
  return y / np.sqrt(np.float64(h))


def bound(x, h):
  """[n, 1]: (L + 4) 2^-24 ||x||_2 per vector. An output is a sum of h terms +-r x_i; each term passes L additions,
  one product and a twice-rounded r (sqrt, divide), i.e. at most L + 3 roundings of relative size 2^-24, and
  r sum|x_i| <= ||x||_2 by Cauchy-Schwarz (r^2 h = 1 up to 2^-23, which the spare unit covers with the second-order
  terms)."""
  x = np.array(x, np.float64).reshape(-1, h)
  return (log2(h) + 4) * 2.0 ** -24 * np.linalg.norm(x, axis=1, keepdims=True)


def sylvester_int(x, h):
  """int64 [n, h]: x @ H_h for integer x, by butterflies (H is symmetric and order-free in exact arithmetic)."""
  y = np.array(x).astype(np.int64).reshape(-1, h)
  for b in range(log2(h)):
    y = _stage(y, b)
  return y


def same_bits(got, want):
  """'' when two float32 arrays agree word for word (a NaN for a NaN), else what differs."""
  got, want = np.asarray(got), np.asarray(want)
  if got.shape != want.shape or got.dtype != F or want.dtype != F:
    return f"{got.dtype}{got.shape} for {want.dtype}{want.shape}"
  gn, wn = np.isnan(got), np.isnan(want)
  differ = (gn != wn) | ((got.view(np.uint32) != want.view(np.uint32)) & ~(gn & wn))
  if not differ.any():
    return ""
  first = tuple(np.argwhere(differ)[0])
  return f"{int(differ.sum())} of {want.size} words differ, first at {first}: {got[first]!r} for {want[first]!r}"


def has_subnormals(a):
  a = np.abs(np.asarray(a, F))
  return bool(((a > 0) & (a < np.finfo(F).tiny)).any())


# ------------------------------------------------------------------------------------------------ inputs
def _batches(pool, n_vec):
  """[total, h] -> [batches, n_vec, h]; total is a multiple of n_vec."""
  return pool.reshape(-1, n_vec, pool.shape[1])


def _pool_size(need, n_vec):
  return n_vec * max(1, -(-need // n_vec))


def impulse_positions(h, seed):
  fixed = {0, h - 1} | {1 << k for k in range(log2(h))}
  rng = np.random.default_rng(seed)
  extra = {int(p) for p in rng.integers(0, h, size=4)}
  return sorted(fixed | extra)


@functools.lru_cache(maxsize=None)
def impulses(h, n_vec, seed=0):
  """(x, want) as [batches, n_vec, h] float32: every position of impulse_positions at least once."""
  pos = impulse_positions(h, seed)
  total = _pool_size(len(pos), n_vec)
  rng = np.random.default_rng([seed, h, n_vec, 1])
  p = np.array([pos[i % len(pos)] for i in range(total)], np.int64)
  j = rng.integers(-20, 21, size=total)
  sign = rng.choice(np.array([-1, 1]), size=total)
  value = (sign * 2.0 ** j).astype(F)
  x = np.zeros((total, h), F)
  x[np.arange(total), p] = value
  # the answer, with integers: popcount(p & q) by folding the bits
  q = np.arange(h, dtype=np.int64)
  parity = p[:, None] & q[None, :]
  for shift in (8, 4, 2, 1):
    parity ^= parity >> shift
  want = np.where(parity & 1, -value[:, None], value[:, None]).astype(F) * scale_factor(h)
  assert want.dtype == F
  for a in (x, want):
    a.setflags(write=False)
  return _batches(x, n_vec), _batches(want, n_vec)


def is_power_of_four(h):
  return log2(h) % 2 == 0


@functools.lru_cache(maxsize=None)
def integers(h, n_vec, seed=0):
  """(x, want) as [1, n_vec, h] float32 for h = 4^m: |x| < 2^(23 - L), the answer from int64."""
  L = log2(h)
  assert is_power_of_four(h)
  lim = 1 << (23 - L)
  rng = np.random.default_rng([seed, h, n_vec, 2])
  xi = rng.integers(-lim + 1, lim, size=(n_vec, h))
  xi[0, :] = lim - 1                                    # the largest sum there is: h (lim - 1) at output 0
  if n_vec > 1:
    xi[1, :] = np.where(np.arange(h) & 1, -(lim - 1), lim - 1)
  s = sylvester_int(xi, h)
  assert np.abs(s).max() < 1 << 23
  want = (s.astype(np.float64) * 2.0 ** -(L // 2)).astype(F)
  x = xi.astype(F)
  assert np.array_equal(x.astype(np.int64), xi) and np.array_equal(want.astype(np.float64) * 2.0 ** (L // 2), s)
  for a in (x, want):
    a.setflags(write=False)
  return x[None], want[None]


FLOAT_PLANTS = ("dominant", "negzero", "zero", "nan", "inf", "plain")


@functools.lru_cache(maxsize=None)
def floats(h, n_vec, seed=0):
  """(x [batches, n_vec, h] float32, plant [batches, n_vec] of names): pool vector i < 6 carries FLOAT_PLANTS[i]."""
  total = _pool_size(len(FLOAT_PLANTS), n_vec)
  rng = np.random.default_rng([seed, h, n_vec, 3])
  scale = np.exp2(rng.uniform(-8, 8, size=(total, 1)))
  x = (rng.standard_normal((total, h)) * scale).astype(F)
  plant = np.array([FLOAT_PLANTS[i] if i < len(FLOAT_PLANTS) else "plain" for i in range(total)])
  x[0, h - 1] = F(np.abs(x[0]).max() * 4096.0)           # everything else is at its rounding error
  x[1, 0] = F(-0.0)
  x[1, h // 2] = F(-0.0)
  x[2, :] = 0
  x[3, int(rng.integers(0, h))] = np.nan
  x[4, int(rng.integers(0, h))] = np.inf
  assert not has_subnormals(x)
  x.setflags(write=False)
  return _batches(x, n_vec), plant.reshape(-1, n_vec)


def float_want(h, n_vec, order, seed=0):
  x, _ = floats(h, n_vec, seed)
  return model(x, h, order).reshape(x.shape)


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
  route: str
  h: int
  n_vec: int
  x_off: int = 0          # floats past a 16-byte aligned address
  out_off: int = 0
  note: str = ""

  @property
  def id(self):
    off = "" if not (self.x_off or self.out_off) else f"-x+{self.x_off}-out+{self.out_off}"
    return f"{self.route}-h{self.h}-n{self.n_vec}{off}"


def _cases():
  out = [Case("r2", 1, 5, note="identity"),
         Case("r2", 2, 1027, note="a full block of 1024 vectors, then 6 elements by scalar accesses"),
         Case("r2", 8, 259), Case("r2", 128, 19),
         Case("r2", 4, 515, note="4^m: integers"), Case("r2", 16, 131, note="4^m"), Case("r2", 64, 35, note="4^m")]
  for h in (256, 2048, 4096, 8192, 16384):
    offsets = ((1, 0), (0, 1), (1, 1)) if h in (256, 4096) else ((1, 1),)
    out += [Case("r2", h, 3, xo, oo, note="misaligned fallback") for xo, oo in offsets]
  out += [Case("t12", 256, 1, note="a lone partial tile"), Case("t12", 256, 19), Case("t12", 1024, 7),
          Case("t12", 2048, 3), Case("t12", 4096, 2), Case("t13", 8192, 2), Case("t14", 16384, 2)]
  for c in out:
    assert route(c.h, c.x_off == 0, c.out_off == 0) == c.route, c
  return tuple(out)


CASES = _cases()

# (h, rows, d) of the effective-weight delta: every network, several vectors per row at one size of each LDS kernel
DELTA_SHAPES = tuple((h, 3, h) for h in (8, 128, 256, 2048, 4096, 8192, 16384)) + ((128, 3, 384), (2048, 3, 6144))
DELTA_KINDS = ("f16", "i4")


@functools.lru_cache(maxsize=None)
def delta_case(kind, h, rows, d, seed=0):
  """dict: w [rows * d] float32, the stored target (float16 values, or int4 pairs packed low nibble first with one
  float32 scale per row), its dequantized float32 values, and want = w - rotate_h(dequant) under delta_route(h)."""
  rng = np.random.default_rng([seed, h, rows, d, DELTA_KINDS.index(kind)])
  n = rows * d
  w = (rng.standard_normal(n) * 0.02).astype(F)
  if kind == "f16":
    stored = (rng.standard_normal(n) * 0.02).astype(np.float16)
    dq = stored.astype(F)                                      # exact
    scale = None
  else:
    q = rng.integers(-8, 8, size=n)
    scale = (np.exp(rng.normal(size=rows)) * 0.01).astype(F)
    dq = q.astype(F) * np.repeat(scale, d)                     # float32: int4 times float32 is exact in float64, so
    assert dq.dtype == F                                       # one rounding either way
    stored = ((q[0::2] & 15) | ((q[1::2] & 15) << 4)).astype(np.uint8)
  want = w - model(dq, h, stage_order(delta_route(h), h)).reshape(-1)
  assert want.dtype == F and not has_subnormals(dq)
  return dict(w=w, stored=stored, scale=scale, dq=dq, want=want)
