"""Hessians whose inverse has ONE correct bit pattern, shared by test_hinv_routes_host.py and test_gpu_hinv_routes.py.

The construction. Columns fall into classes c(i) = i % 3. S is strictly lower triangular and S[i, j] != 0 only where
c(j) < c(i), so a chain j -> i -> ... climbs a class with every link, S^3 = 0 and (I + S)^-1 = I - S + S^2 exactly. Row
i of S has IN_BLOCK non-zeros inside its own 64-column block (where that many admissible columns are left of i) and one
in every earlier 64-column block, with values from {-2, -1, 1, 2}; D is diagonal with D[j] = 2^k, k in {0, 1, 2}. Then

    L = (I + S) D,   H = L L^T,   L^-1 = D^-1 (I - S + S^2),   H^-1 = (L^-1)^T L^-1,

all from the closed form in float64 (never from a library inverse). The pivots of the factorization are D[j]^2 = 4^k
(exact square roots and reciprocals), every Cholesky intermediate is an integer, every intermediate of the merge levels
and of the final product a multiple of GRID = 1 / max(D)^2.

The condition (condition_units). With A = |S|, L+ = (I + A) D and Linv+ = D^-1 (I + A + A^2), the largest entries of
(Linv+)^T Linv+, of Linv+ L+ Linv+ and of L+ (L+)^T, in units of GRID, stay below 2^23. These majorants bound the sum
of magnitudes of every product any route adds up for one element (the factorization subtracts products of entries of
L from H; a merge level forms L22^-1 (L21 L11^-1); the product is Linv^T Linv), so every partial sum in any order is an
integer number of units below 2^24: exact in float64, in the float32 accumulators of the bf16x3 routes, and in the
float32 output.

Odd magnitudes. From d = ODD_MIN_D on, ODD further entries of S carry the magnitude 257: nine significant bits, so
that these entries of L and L^-1 need the second bf16 plane of the three-way split, and 257^2 in H and H^-1 the third.
They sit in rows spread over the matrix (at d = 4608: inside the lower left block of a pair of the 1024 level, of the
2048 level and of the ragged 4096 + 512 pair) and in columns of the first block. The room below 2^23 does not allow
them anywhere: 257^2 * max(D)^2 / GRID alone is 1.7e7. So the row has class 2 and the column class 0, which keeps
the entry out of S^2 (nothing links to the row, the column links to nothing), the column has D = 1, and no two
share a column. The condition above is checked with them in place. Stated limit: a third plane is needed only by sums
that hold 257^2; no single entry of L^-1 has more than nine significant bits.

Everything is built from (d, seed) alone, so that a child process rebuilds a case from its numbers."""
import functools

import numpy as np

NB = 64
IN_BLOCK = 3
VALUES = np.array([-2, -1, 1, 2], dtype=np.int64)
DMAX_LOG2 = 2
GRID = 1.0 / float(1 << (2 * DMAX_LOG2))      # every entry of H^-1 is a multiple of this
LIMIT = float(1 << 23)
ODD = 4                                       # entries of S with the odd magnitude below, for d >= ODD_MIN_D
ODD_MAGNITUDE = 257
ODD_MIN_D = 128


@functools.lru_cache(maxsize=64)
def factors(d, seed):
  """(S int64 [d, d], k int64 [d]) with D = 2^k; vectorised (one random admissible column per (row, block))."""
  rng = np.random.default_rng([d, seed])
  rows = np.arange(d)
  cls = rows % 3
  blk = rows // NB
  nblocks = (d + NB - 1) // NB
  s = np.zeros((d, d), dtype=np.int64)
  # one non-zero in every earlier block: a random class below the row's, a random column of the block moved onto it
  if nblocks > 1:
    bcol = np.arange(nblocks)
    target = (rng.random((d, nblocks)) * np.maximum(cls, 1)[:, None]).astype(np.int64)     # in [0, c(i))
    j = bcol[None, :] * NB + rng.integers(0, NB, (d, nblocks))
    j = j - (j - target) % 3
    j = np.where(j < bcol[None, :] * NB, j + 3, j)
    ok = (bcol[None, :] < blk[:, None]) & (cls[:, None] > 0)
    val = VALUES[rng.integers(0, 4, (d, nblocks))]
    ri = np.broadcast_to(rows[:, None], j.shape)
    s[ri[ok], j[ok]] = val[ok]
  # IN_BLOCK distinct admissible columns of the row's own block, by random keys
  cols = blk[:, None] * NB + np.arange(NB)[None, :]
  keys = rng.random((d, NB))
  admissible = (cols < rows[:, None]) & ((cols % 3) < cls[:, None])
  keys = np.where(admissible, keys, np.inf)
  order = np.argsort(keys, axis=1)[:, :IN_BLOCK]
  picked = np.take_along_axis(keys, order, axis=1) < np.inf
  val = VALUES[rng.integers(0, 4, (d, IN_BLOCK))]
  ri = np.broadcast_to(rows[:, None], order.shape)
  jc = np.take_along_axis(cols, order, axis=1)
  s[ri[picked], jc[picked]] = val[picked]
  k = rng.integers(0, DMAX_LOG2 + 1, d)
  if d >= ODD_MIN_D:
    # the odd magnitudes: row of class 2 (nothing links to it), column of class 0 in block 0 (it links to nothing), D = 1 there
    for n, r in enumerate(np.linspace(NB, d - 1, ODD).astype(np.int64)):
      i, j = int(r) - (int(r) - 2) % 3, 3 * (5 * n + 1)
      s[i, j] = ODD_MAGNITUDE * (1 if rng.random() < 0.5 else -1)
      k[j] = 0
  return s, k


def _eye(xp, d, like):
  if xp is np:
    return np.eye(d)
  return xp.eye(d, dtype=like.dtype, device=like.device)


def dense(d, seed, xp=np, device=None):
  """(L, Linv, H, Hinv) in float64, from the closed form, with numpy or (xp = torch, on `device`) with torch."""
  s_int, k = factors(d, seed)
  dv = np.ldexp(1.0, k)
  if xp is np:
    s, dd, di = s_int.astype(np.float64), dv, 1.0 / dv
  else:
    s = xp.from_numpy(s_int).to(device=device, dtype=xp.float64)
    dd = xp.from_numpy(dv).to(device=device)
    di = 1.0 / dd
  eye = _eye(xp, d, s)
  l = (eye + s) * dd[None, :]
  linv = di[:, None] * (eye - s + s @ s)
  return l, linv, l @ l.T, linv.T @ linv


def majorants(d, seed, xp=np, device=None):
  """(Linv+)^T Linv+, Linv+ L+ Linv+ and L+ (L+)^T of the module docstring."""
  s_int, k = factors(d, seed)
  dv = np.ldexp(1.0, k)
  if xp is np:
    a, dd, di = np.abs(s_int).astype(np.float64), dv, 1.0 / dv
  else:
    a = xp.from_numpy(np.abs(s_int)).to(device=device, dtype=xp.float64)
    dd = xp.from_numpy(dv).to(device=device)
    di = 1.0 / dd
  eye = _eye(xp, d, a)
  lp = (eye + a) * dd[None, :]
  lip = di[:, None] * (eye + a + a @ a)
  return lip.T @ lip, lip @ lp @ lip, lp @ lp.T


def condition_units(d, seed, xp=np, device=None):
  """The largest entry of each majorant, in units of GRID."""
  return tuple(float(m.max()) / GRID for m in majorants(d, seed, xp, device))


def zero_pivot(h, d, seed, j):
  """H with D[j]^2 taken off H[j, j] (in place): pivot j of the factorization is exactly 0, the ones before it unchanged."""
  _, k = factors(d, seed)
  h[j, j] -= float(4 ** int(k[j]))
  return h
