"""Activations whose Hessian product X^T X has ONE correct bit pattern on every route, shared by test_xtx_routes_host.py
and test_gpu_xtx_routes.py.

The condition (units). For every output entry (i, j), every product any route adds is an integer multiple of a quantum
q, and the magnitudes of those products -- over all tokens of all calls of a case, plus the initial product where there
is one -- add up to less than 2^24 q. Then every partial sum in any order is an integer number of quanta below 2^24:
exact in float32. That covers split-K, the fold every 32 k tiles, the separate accumulators of the cross terms,
big + lo, old + v and the reduce kernels; no case relies on an order. The majorant used is max |X|^T |X| (the planes of
a value share its sign, so the kept products of an entry are bounded by |x_i| |x_j|), plus max |P0|.

Three kinds, all built from (n, d, seed, kind) alone so that a child process rebuilds a call from its numbers:

  dense    every token live, integers in [-3, 3] from a counter hash of (token, column, seed); SPECIALS entries carry
           the magnitude 257 (nine significant bits: the second bf16 plane; one float16 plane still holds it), at most
           one per column and in distinct tokens, so an entry's majorant is at most 9 (n - 1) + 257^2. q = 1 and the
           model is the exact integer product. Catches K ranges, tiles, slabs, partials and accumulation.
  planes3  (bf16x3) all tokens zero except at most LIVE3 = 15 on the boundaries the kernels have (boundary_tokens);
           live values s (a + 2^-9 + 2^-18), a in {1, 2}, s in {-1, +1} per (token, column). The three planes are
           exactly s a, s 2^-9, s 2^-18 (the residuals keep the value's sign: 1 - 2^-9 - 2^-18 would round its first
           plane down to 1 - 2^-8 and leave the grid), every kept product is a multiple of q = 2^-18, and
           15 (2 + 2^-9 + 2^-18)^2 = 60.1, plus an initial product of at most 3, stays below 64 = 2^24 q. 16 do not fit.
  planes2  (f16x2) the same layout with s (a + 2^-12) and up to LIVE2 = 40 live tokens; tokens of a second slab are
           scaled by 2^(column % 2), so that the per-slab column exponents differ between the slabs. q = 2^-12.

Where a call has more boundaries than live tokens (16 split-K slices have 30 boundary tokens), boundary_tokens keeps them
in the order of its list; the dense kind covers every slice of such a call.

The expected value is the kernel's DEFINITION, not the exact product: for bf16x3 the six kept products
x1y1 + x1y2 + x2y1 + x1y3 + x2y2 + x3y1, for f16x2 the three kept products of the scaled planes, scaled back by
2^-(e_i + e_j) per slab -- from NumPy restatements of bf16_rne_bits, column_exponent and the two splits. On planes3 data
the float32-rounded exact product differs from it in a few per cent of the entries, which is the point."""
import functools

import numpy as np

TILE = 128
BK = 16
FOLD = 32
SLAB = 16384
LIVE3 = 15
LIVE2 = 40
SPECIALS = 4
SPECIAL_MAGNITUDE = 257
DENSE_MAX = 3
INITIAL_MAX = 3
LIMIT = float(1 << 24)
QUANTUM = {"dense": 1.0, "planes3": 2.0 ** -18, "planes2": 2.0 ** -12}
BF16_PAIRS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))     # (plane of A, plane of B) of the six kept products
F16_PAIRS = ((0, 0), (0, 1), (1, 0))
_M32 = 0xFFFFFFFF


def mix(t, c, seed):
  """A 32-bit counter hash of (token, column, seed) in int64 arithmetic that numpy and torch evaluate alike (every
  intermediate stays below 2^63)."""
  h = (t * 0x1E3779B1 + c * 0x05EBCA77 + ((seed * 0x42B2AE3D + 0x27D4EB2F) & _M32)) & _M32
  h = h ^ (h >> 15)
  h = (h * 0x2C1B3C6D) & _M32
  h = h ^ (h >> 12)
  h = (h * 0x297A2D39) & _M32
  return h ^ (h >> 15)


# ------------------------------------------------------------------------------------------------ the kernels' K layout ---
def splits_of(d, kt):
  """xtx_splits / xtx2_splits (MI355Q_XTX_SPLIT_BELOW at its default 512)."""
  tiles = (d // TILE) * (d // TILE + 1) // 2
  if tiles >= 512:
    return 1
  s = min((768 + tiles - 1) // tiles, 16, kt // 64)
  return max(s, 1)


def slabs_of(n, d, kind):
  """Per slab of a split-kernel call: (first token, tokens, kt, splits, kt_per_split), as xtx_bf16x3 (dense, planes3) or
  xtx_f16x2 (planes2) lays it out."""
  out = []
  for k0 in range(0, n, SLAB):
    ks = min(SLAB, n - k0)
    if kind == "planes2":
      kt = (ks + 2 * BK - 1) // (2 * BK) * 2
      s = splits_of(d, kt)
      per = ((kt // 2 + s - 1) // s) * 2
    else:
      kt = (ks + BK - 1) // BK
      s = splits_of(d, kt)
      per = (kt + s - 1) // s
    out.append((k0, ks, kt, s, per))
  return out


def boundary_tokens(n, d, seed, kind):
  """The live tokens of a planes* call, sorted: the last token, both sides of the slab boundary, first and last token of
  a k tile, both sides of the first fold boundary, both sides of the split-K boundaries (slab by slab in turn), the rest
  seeded -- in this order until the kind's room is used up."""
  cap = LIVE3 if kind == "planes3" else LIVE2
  want = [n - 1]
  slabs = slabs_of(n, d, kind)
  if len(slabs) > 1:
    want += [SLAB - 1, SLAB]
  want += [0, BK - 1, BK, FOLD * BK - 1, FOLD * BK]
  per_slab = [[k0 + z * per * BK for z in range(1, s) if z * per * BK < ks] for k0, ks, _, s, per in slabs]
  for z in range(max(len(b) for b in per_slab)):
    for b in per_slab:
      if z < len(b):
        want += [b[z] - 1, b[z]]
  rng = np.random.default_rng([n, d, seed, 7])
  want += [int(t) for t in rng.integers(0, n, 2 * cap)]
  live = []
  for t in want:
    if 0 <= t < n and t not in live and len(live) < cap:
      live.append(t)
  return tuple(sorted(live))


# ------------------------------------------------------------------------------------------------------------- the data ---
def special_entries(n, d, seed):
  """((token, column, value), ...) of the dense kind: distinct tokens (first and last among them), distinct columns."""
  tokens = sorted({int(t) for t in np.linspace(0, n - 1, SPECIALS)})
  columns = [1 % d, (d // 2 + 3) % d, d - 2, (TILE + 2) % d]
  out = []
  for i, t in enumerate(tokens):
    sign = 1 if int(mix(t, columns[i], seed + 99)) & 1 else -1
    out.append((t, columns[i], sign * SPECIAL_MAGNITUDE))
  assert len({c for _, c, _ in out}) == len(out) and len({t for t, _, _ in out}) == len(out)
  return tuple(out)


def dense_x(n, d, seed, xp=np, device=None):
  """X [n, d] float32 of the dense kind, with numpy or (xp = torch, on `device`) with torch."""
  if xp is np:
    t, c = np.arange(n, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
    x = (mix(t, c, seed) % 7 - DENSE_MAX).astype(np.float32)
  else:
    t = xp.arange(n, dtype=xp.int64, device=device)[:, None]
    c = xp.arange(d, dtype=xp.int64, device=device)[None, :]
    x = (mix(t, c, seed) % 7 - DENSE_MAX).to(xp.float32)
  for tok, col, v in special_entries(n, d, seed):
    x[tok, col] = float(v)
  return x


@functools.lru_cache(maxsize=64)
def live_rows(n, d, seed, kind):
  """(tokens, values float32 [len(tokens), d]) of a planes* call; every other token is zero."""
  tokens = boundary_tokens(n, d, seed, kind)
  t, c = np.array(tokens, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
  h = mix(t, c, seed)
  a = (1 + (h & 1)).astype(np.float64)
  s = (1 - 2 * ((h >> 1) & 1)).astype(np.float64)
  if kind == "planes3":
    v = s * (a + 2.0 ** -9 + 2.0 ** -18)
  else:
    v = s * (a + 2.0 ** -12) * np.where(t >= SLAB, np.ldexp(1.0, (c % 2).astype(np.int64)), 1.0)
  v32 = v.astype(np.float32)
  assert np.array_equal(v32.astype(np.float64), v)
  v32.setflags(write=False)
  return tokens, v32


def planes_x(n, d, seed, kind, xp=np, device=None):
  """X [n, d] float32 of a planes* call: zeros plus the live rows."""
  tokens, values = live_rows(n, d, seed, kind)
  if xp is np:
    x = np.zeros((n, d), dtype=np.float32)
    x[list(tokens)] = values
  else:
    x = xp.zeros((n, d), dtype=xp.float32, device=device)
    x[xp.tensor(tokens, device=device)] = xp.from_numpy(values.copy()).to(device)
  return x


def call_x(n, d, seed, kind, xp=np, device=None):
  return dense_x(n, d, seed, xp, device) if kind == "dense" else planes_x(n, d, seed, kind, xp, device)


def initial_product(d, seed, xp=np, device=None):
  """A symmetric integer matrix with entries in [-INITIAL_MAX, INITIAL_MAX], float64: the product of earlier calls."""
  if xp is np:
    i, j = np.arange(d, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return (mix(hi, lo, seed + 31337) % (2 * INITIAL_MAX + 1) - INITIAL_MAX).astype(np.float64)
  i = xp.arange(d, dtype=xp.int64, device=device)[:, None]
  j = xp.arange(d, dtype=xp.int64, device=device)[None, :]
  lo, hi = xp.minimum(i, j), xp.maximum(i, j)
  return (mix(hi, lo, seed + 31337) % (2 * INITIAL_MAX + 1) - INITIAL_MAX).to(xp.float64)


# ------------------------------------------------------------------------------------------ the splits, restated ---
def bf16_rne_bits(x):
  """bf16_rne_bits of csrc/xtx_bf16x3.hip for finite float32 values that do not round to infinity."""
  b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
  r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
  assert np.all((r & 0x7F80) != 0x7F80)
  return r.astype(np.uint32)


def split_bf16x3(x):
  """The three bf16 planes of float32 x as float32 arrays (xtx_split_kernel): x == p1 + p2 + p3."""
  v = np.array(x, dtype=np.float32)
  planes = []
  for _ in range(3):
    p = (bf16_rne_bits(v) << np.uint32(16)).view(np.float32)
    planes.append(p)
    v = v - p
  return planes


def column_exponent(max_bits):
  """column_exponent of csrc/xtx_f16x2.hip for an array of bit patterns of column maxima."""
  biased = (max_bits >> 23).astype(np.int64)
  return np.where(max_bits == 0, 0, 14 - (np.maximum(biased, 1) - 127)).astype(np.int64)


def split_f16x2(x):
  """(e int64 [d], [h1, h2] float32) for the rows x of ONE slab (all of its non-zero rows): xtx2_colmax_kernel and
  xtx2_split_kernel. The planes are those of x 2^e, column by column."""
  x = np.asarray(x, dtype=np.float32)
  bits = (x.view(np.uint32) & np.uint32(0x7FFFFFFF))
  e = column_exponent(bits.max(axis=0) if len(x) else np.zeros(x.shape[1], np.uint32))
  v = np.ldexp(x, e[None, :].astype(np.int32)).astype(np.float32)
  planes = []
  for _ in range(2):
    h = v.astype(np.float16).astype(np.float32)
    planes.append(h)
    v = v - h
  return e, planes


# ----------------------------------------------------------------------------------------------------------- the models ---
def kept(pa, pb, pairs, xp=np):
  """sum over the kept (plane of A, plane of B) pairs of A_p^T B_q, float64."""
  total = None
  for p, q in pairs:
    term = pa[p].T @ pb[q]
    total = term if total is None else total + term
  return total


def _to(xp, a, device):
  a = np.ascontiguousarray(a, dtype=np.float64)
  return a if xp is np else xp.from_numpy(a).to(device)


def planes_model(n, d, seed, kind, xp=np, device=None, cols=None):
  """What the split kernel of `kind` must return for a planes* call, float64 [d, d] (or its leading cols x cols block):
  the kept products of the live rows, slab by slab."""
  tokens, values = live_rows(n, d, seed, kind)
  if cols is not None:
    values = values[:, :cols]
  tok = np.array(tokens)
  if kind == "planes3":
    planes = [_to(xp, p, device) for p in split_bf16x3(values)]
    return kept(planes, planes, BF16_PAIRS, xp)
  total = None
  for k0 in range(0, n, SLAB):
    rows = values[(tok >= k0) & (tok < k0 + SLAB)]
    if not len(rows):
      continue
    e, planes = split_f16x2(rows)
    planes = [_to(xp, p, device) for p in planes]
    back = _to(xp, np.ldexp(1.0, -(e[:, None] + e[None, :])), device)
    part = kept(planes, planes, F16_PAIRS, xp) * back
    total = part if total is None else total + part
  return total


def exact_product(n, d, seed, kind, cols=None):
  """float64 X^T X of a planes* call from its live rows (every product and every sum is exact in float64)."""
  _, values = live_rows(n, d, seed, kind)
  v = values.astype(np.float64)[:, :cols]
  return v.T @ v


def majorant_units(n, d, seed, kind, initial=False):
  """An upper bound of sum |products| of any entry, in quanta, for ONE call (callers add up the calls of a case)."""
  if kind == "dense":
    bound = float(DENSE_MAX ** 2 * (n - 1) + SPECIAL_MAGNITUDE ** 2)
  else:
    _, values = live_rows(n, d, seed, kind)
    bound = float((values.astype(np.float64) ** 2).sum(axis=0).max())     # (Cauchy-Schwarz: a diagonal entry is the largest)
  return (bound + (INITIAL_MAX if initial else 0)) / QUANTUM[kind]
