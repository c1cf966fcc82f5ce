"""Inputs and expected values for the three entry points of the OSCAR scale search (csrc/oscar.hip):

  mi355q_oscar_col_sumsq_f32      col_sumsq_kernel<64>, or group_sum_kernel<float> for a single column
  mi355q_oscar_group_terms_f32    group_top_row_kernel | group_top_block_kernel<8|16|32|64>, then
                                  group_sum_kernel | group_sum_balanced_kernel
  mi355q_oscar_winner_energy_f64  winner_energy_kernel

No GPU is needed here. Every output has two restatements:

  * reference_*: the reference's own NumPy expression in FP64 (ref oscar.py:173-251, restated in oracle/aeq_oracle.py,
    oscar_scale_objective / oscar_channel_scales) -- `(w64*w64).sum(0)`, `np.mean(.., axis=0)`, `.max(1)`, `np.argmax`,
    `(mx*mx).sum()`, `np.add.at`. This is what the GPU is held to, bit for bit.
  * model_*: the order of the additions spelled out, with no NumPy reduction: a row-by-row loop for the column sums
    (a matrix of ONE column is a contiguous vector to NumPy, which adds it as .sum() does: chunked pairwise),
    NumPy's pairwise recursion in 8192-element chunks for the vector sum, a first-maximum scan for the argmax, a row loop
    for add.at. Only elementwise operations on whole vectors are used, so that the many columns / groups of a case go
    through the loop at once. test_oscar_scale_cases_host.py asserts that both agree on every case; the model exists so
    that it can be MUTATED (MUTATIONS): each mutation is a way a kernel could be subtly wrong, and the host test proves
    that every case whose features a mutation attacks shows it in at least one expected value.

route() restates the host's choice of kernels (the extern "C" functions of oscar.hip, balanced_chunk of common.h) and
names the features of a shape; REQUIRED lists the features the case list has to reach.

Four kinds of input:
  wide     w = normal * exp(4 normal) as float32, s = exp(1.5 normal) clipped to [1e-4, 1e4]: the order of every
           addition shows.
  squares  magnitudes from float32 denormals to 3e19, by column: a square taken in float32 underflows or overflows.
  ties     s powers of two, every (row, group) maximum planted at two columns: inside one lane's four columns, in
           different lanes, and for the row kernel in different waves (either order) and in one thread at two strides.
  signs    -0.0, all-zero rows, +-inf weights (infinite ties resolve to the first index; top2, sums, eff are inf).

NaN in w or s is outside what group_terms and winner_energy are held to: beats() orders with `>`, np.max propagates NaN.
End to end the scales are NaN either way, because the column energies propagate it; only col_sumsq is pinned on
non-finite input (nonfinite_columns)."""
import dataclasses
import functools

import numpy as np

CHUNK = 8192          # NumPy's reduction buffer: .sum() adds 8192-element chunks in order, each pairwise
LEAF = 128            # pairwise_sum's unrolled block
COL_UNROLL = 64       # col_sumsq_kernel<64>: rows per unrolled step; also its columns per block
TOP_THREADS = 256     # both group_top kernels
STAGE_ROWS = 1024     # winner_energy_kernel's LDS staging
SLICE_COLS = 256      # winner_energy_kernel: columns per blockIdx.y
BLOCK_GROUPS = (32, 64, 128, 256)


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


def route(entry, n, d, g=0):
  """(kernels, features) of one call. entry: 'col_sumsq' (n = rows), 'group_terms', 'winner_energy'."""
  feats = set()
  if entry == "col_sumsq":
    feats.add(("col", "rows<64") if n < COL_UNROLL else ("col", "rows=64k") if n % COL_UNROLL == 0 else ("col", "rows=64k+t"))
    feats.add(("col", "d<64") if d < COL_UNROLL else ("col", "d=64k") if d % COL_UNROLL == 0 else ("col", "d=64k+t"))
    if d == 1:                                     # NumPy sums one column as a vector; so does the library
      feats.add(("col", "d=1"))
      if n > CHUNK:
        feats.add(("col", "d=1, rows>8192"))
      return ("group_sum_kernel<float>",), feats
    return ("col_sumsq_kernel<64>",), feats
  assert g > 0 and d % g == 0
  if entry == "winner_energy":
    if n < 8:
      feats.add(("we", "n<8"))
    if n in (STAGE_ROWS - 1, STAGE_ROWS, STAGE_ROWS + 1):
      feats.add(("we", f"n={n}"))
    if n > 2 * STAGE_ROWS and (n % STAGE_ROWS) % 8:
      feats.add(("we", "three stagings, ragged tail"))
    if g != d:
      feats.add(("we", f"block g={g}"))
    slices = -(-g // SLICE_COLS)
    if slices > 1 and g % SLICE_COLS:
      feats.add(("we", f"{slices} slices, last partial"))
    return ("winner_energy_kernel",), feats
  assert entry == "group_terms"
  if g == d:
    top = "group_top_row_kernel"
    if d == 1:
      feats.add(("row", "d=1"))
    elif d < 64:
      feats.add(("row", "d<64"))
    elif d < TOP_THREADS:
      feats.add(("row", "d<256"))
    elif d == TOP_THREADS:
      feats.add(("row", "d=256"))
    elif d % TOP_THREADS:
      feats.add(("row", "d>256 ragged"))
    if d == 32:
      feats.add(("row", "g=32=d takes the row route"))
  else:
    assert g in BLOCK_GROUPS, g
    lanes = g // 4
    top = f"group_top_block_kernel<{lanes}>"
    quads = n * d // 4
    # a partial last block ends in whole groups of dead lanes: quads is a multiple of the lanes of a group
    feats.add((top, "one partial block") if quads < TOP_THREADS else
              (top, "blocks>1") if quads > TOP_THREADS else (top, "one full block"))
    if quads > TOP_THREADS and quads % TOP_THREADS:
      feats.add((top, "blocks>1, last partial"))
  chunks = -(-n // CHUNK)
  last = n - (n - 1) // CHUNK * CHUNK
  bal = balanced_chunk(last)
  if bal:
    total = "group_sum_balanced_kernel"
    feats.add(("bal" if chunks == 1 else "bal-multi", bal[1], bal[0]))
  else:
    total = "group_sum_kernel"
    if chunks == 1:
      feats.add(("sum", "n<8") if n < 8 else ("sum", "8<n<=128 ragged") if n <= LEAF else ("sum", "one unbalanced chunk"))
    else:
      feats.add(("sum", "multi, last chunk of one") if last == 1 else ("sum", "multi, last chunk unbalanced"))
  return (top, total), feats


REQUIRED = frozenset(
    [("col", f) for f in ("rows<64", "rows=64k", "rows=64k+t", "d<64", "d=64k", "d=64k+t", "d=1", "d=1, rows>8192", "mean=0", "mean=1")] +
    [("row", f) for f in ("d=1", "d<64", "d<256", "d=256", "d>256 ragged", "g=32=d takes the row route")] +
    [(f"group_top_block_kernel<{lanes}>", f) for lanes in (8, 16, 32, 64) for f in ("one partial block", "blocks>1")] +
    [("sum", f) for f in ("n<8", "8<n<=128 ragged", "one unbalanced chunk", "multi, last chunk of one",
                          "multi, last chunk unbalanced")] +
    # depth, leaf: n = 8, 120, 128 | 144, 256 | 512 | 1024 | 2048 | 2816, 4096 | 6144, 8192
    [("bal", depth, leaf) for depth, leaf in ((0, 8), (0, 120), (0, 128), (1, 72), (1, 128), (2, 128), (3, 128), (4, 128),
                                              (5, 88), (5, 128), (6, 96), (6, 128))] +
    # n = 8200, 10240, 11008, 16384
    [("bal-multi", depth, leaf) for depth, leaf in ((0, 8), (4, 128), (5, 88), (6, 128))] +
    [("we", f) for f in ("n<8", "n=1023", "n=1024", "n=1025", "three stagings, ragged tail", "block g=32", "block g=256",
                         "2 slices, last partial", "4 slices, last partial")] +
    [("we-synthetic", f) for f in ("one column wins every row", "uniform winners")] +
    [("kind", k) for k in ("wide", "squares", "ties", "signs")])


# ------------------------------------------------------------------------------------------------ cases
# A seed other than 0 is the first one at which the case shows every mutation that attacks it (test_oscar_scale_cases_host.py):
# on one or two vectors whose largest term carries most of the sum, a single re-ordered addition changes the last bit of
# the result about every other time.
@dataclasses.dataclass(frozen=True)
class ColCase:
  rows: int
  d: int
  mean: int
  kind: str
  seed: int = 0


@dataclasses.dataclass(frozen=True)
class TermsCase:
  """group_terms, then winner_energy on its winner / wsq."""
  n: int
  d: int
  g: int
  kind: str
  seed: int = 0


@dataclasses.dataclass(frozen=True)
class WinnerCase:
  """winner_energy on winner / wsq that no weight produced."""
  n: int
  d: int
  g: int
  pattern: str      # 'one': one column of every group wins every row; 'uniform': uniform over the group but one column
  seed: int = 0


def features(c):
  if isinstance(c, ColCase):
    return route("col_sumsq", c.rows, c.d)[1] | {("col", f"mean={c.mean}"), ("kind", c.kind)}
  if isinstance(c, WinnerCase):
    f = route("winner_energy", c.n, c.d, c.g)[1]
    return f | {("we-synthetic", {"one": "one column wins every row", "uniform": "uniform winners"}[c.pattern])}
  return route("group_terms", c.n, c.d, c.g)[1] | route("winner_energy", c.n, c.d, c.g)[1] | {("kind", c.kind)}


def _show(f):
  return "/".join(str(v) for v in f[1:]) if f[0] in ("col", "row", "sum", "we", "we-synthetic") else \
      f"{f[0]}:d{f[1]}:leaf{f[2]}" if f[0] in ("bal", "bal-multi") else f[1]


def case_id(c):
  feats = sorted(_show(f).replace(" ", "_") for f in features(c) if f[0] != "kind")
  if isinstance(c, ColCase):
    return f"col-{c.rows}x{c.d}-{c.kind}[{','.join(feats)}]"
  if isinstance(c, WinnerCase):
    return f"we-{c.n}x{c.d}g{c.g}-{c.pattern}[{','.join(feats)}]"
  kernels = route("group_terms", c.n, c.d, c.g)[0]
  short = kernels[0].replace("group_top_", "").replace("_kernel", "") + "+" + kernels[1].replace("group_", "").replace("_kernel", "")
  return f"terms-{c.n}x{c.d}g{c.g}-{c.kind}-{short}[{','.join(feats)}]"


COL_CASES = (
    ColCase(1, 1, 0, "wide"),
    ColCase(1, 200, 1, "wide"),
    ColCase(63, 63, 1, "wide"),
    ColCase(63, 64, 0, "squares"),
    ColCase(64, 64, 0, "wide"),
    ColCase(64, 200, 1, "squares"),
    ColCase(65, 200, 1, "wide"),
    ColCase(65, 1, 0, "wide", seed=3),
    ColCase(130, 1, 1, "squares", seed=8),
    ColCase(9000, 1, 1, "wide", seed=16),
    ColCase(130, 64, 0, "wide"),
    ColCase(130, 63, 1, "squares"),
    ColCase(130, 200, 0, "squares"),
)

TERMS_CASES = (
    # the row kernel (g == d)
    TermsCase(1, 1, 1, "wide"),
    TermsCase(7, 40, 40, "signs"),
    TermsCase(7, 40, 40, "wide"),
    TermsCase(33, 32, 32, "ties"),
    TermsCase(129, 200, 200, "wide"),
    TermsCase(136, 256, 256, "ties"),
    TermsCase(1000, 300, 300, "wide", seed=1),
    TermsCase(1023, 1000, 1000, "ties"),
    TermsCase(1024, 300, 300, "squares", seed=24),
    TermsCase(1025, 1000, 1000, "wide", seed=15),
    TermsCase(2100, 300, 300, "wide", seed=2),
    # the block kernels, d = 3 g: one partial block, then more than one block
    TermsCase(5, 96, 32, "ties"),
    TermsCase(33, 96, 32, "wide"),
    TermsCase(9, 96, 32, "signs"),
    TermsCase(3, 192, 64, "ties"),
    TermsCase(8, 192, 64, "wide"),
    TermsCase(2, 384, 128, "ties"),
    TermsCase(120, 384, 128, "wide"),
    TermsCase(1, 768, 256, "wide"),
    TermsCase(3, 768, 256, "ties"),
    TermsCase(1023, 768, 256, "wide", seed=4),
    TermsCase(128, 96, 32, "squares"),
    TermsCase(12, 96, 32, "ties"),
    TermsCase(6, 192, 64, "ties"),
    TermsCase(3, 384, 128, "ties"),
    TermsCase(1, 768, 256, "ties"),
    # the routes of the sum: d = 64, g = 32 or g == d = 40
    TermsCase(144, 64, 32, "wide"),
    TermsCase(256, 40, 40, "wide"),
    TermsCase(512, 64, 32, "wide"),
    TermsCase(1024, 40, 40, "wide", seed=10),
    TermsCase(2048, 64, 32, "wide", seed=3),
    TermsCase(2100, 64, 32, "wide", seed=3),
    TermsCase(2816, 40, 40, "wide", seed=6),
    TermsCase(4096, 64, 32, "wide"),
    TermsCase(6144, 40, 40, "wide", seed=9),
    TermsCase(8192, 64, 32, "wide", seed=5),
    TermsCase(8193, 64, 32, "wide", seed=8),
    TermsCase(9000, 64, 32, "wide"),
    TermsCase(8192 + 136, 64, 32, "wide"),
    TermsCase(8200, 64, 32, "wide", seed=19),
    TermsCase(10240, 40, 40, "wide", seed=5),
    TermsCase(11008, 64, 32, "wide", seed=13),
    TermsCase(16384, 64, 32, "wide", seed=2),
    TermsCase(3 * 8192, 32, 32, "wide", seed=8),
)

WINNER_CASES = (
    WinnerCase(7, 32, 32, "one"),
    WinnerCase(1025, 64, 32, "one"),
    WinnerCase(2100, 300, 300, "one", seed=1),
    WinnerCase(2049, 768, 256, "uniform"),
    WinnerCase(2100, 1000, 1000, "uniform"),
)

CASES = COL_CASES + TERMS_CASES + WINNER_CASES

# the GPU file's end-to-end cross-check, one per granularity; n outside the seeded problems of test_gpu_oscar.py
SEEDED_N = frozenset((1, 5, 9, 12, 17, 20, 33, 40, 50, 64, 130, 300, 700, 9000))
OBJECTIVE_CASES = (TermsCase(2816, 40, 40, "wide", seed=6), TermsCase(11008, 64, 32, "wide", seed=13))


# ------------------------------------------------------------------------------------------------ inputs
def _rng(c, salt):
  fields = [v for v in dataclasses.astuple(c) if isinstance(v, int)]
  return np.random.default_rng([salt, sum(map(ord, getattr(c, "kind", getattr(c, "pattern", ""))))] + fields)


def _wide(rng, n, d):
  return (rng.standard_normal((n, d)) * np.exp(4.0 * rng.standard_normal((n, d)))).astype(np.float32)


def _squares(rng, n, d):
  """Column j holds magnitudes around 10^e(j), e from -44.5 (float32 denormals) to 19.4; columns shuffled."""
  e = rng.permutation(np.linspace(-44.5, 19.4, d)) if d > 1 else np.array([19.4])
  mag = rng.uniform(0.5, 1.0, (n, d)) * 10.0 ** e
  return (mag * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)


def _scales(rng, d):
  return np.clip(np.exp(1.5 * rng.standard_normal(d)), 1e-4, 1e4)


def col_input(c):
  rng = _rng(c, 1)
  return {"wide": _wide, "squares": _squares}[c.kind](rng, c.rows, c.d)


def tie_placements(d, g):
  """Pairs (j1 < j2, name) inside a group of g columns starting at 0 at which a tie is planted."""
  if g != d:                                       # block kernel: lane = column // 4
    lanes = g // 4
    return [(4 * (lanes // 2) + 1, 4 * (lanes // 2) + 3, "one lane"),
            (2, 4 * (lanes - 1) + 1, "lanes"),
            (4 * 1 + 3, 4 * 2 + 0, "neighbouring lanes"),
            (4 * (lanes // 2 - 1) + 3, 4 * (lanes // 2), "lanes across the last shuffle")]
  out = [(3, min(d, 64) - 2, "one wave")] if d >= 8 else []      # row kernel: thread = column % 256, wave = thread // 64
  if d > 100:
    out.append((10, 100, "wave 0 before wave 1"))
  if d >= 256:
    out.append((70, 255, "wave 1 before wave 3"))
  if d > 260:
    out.append((200, 260, "wave 3 before wave 0 of the next stride"))
  if d > 256 + 37:
    out.append((37, 256 + 37, "one thread, two strides"))
  if d > 768 + 5:
    out.append((256 + 5, 768 + 5, "one thread, strides 1 and 3"))
  return out


def _ties(rng, n, d, g):
  s = 2.0 ** rng.integers(-3, 4, d)
  w = (rng.uniform(-1.0, 1.0, (n, d)) * 2.0 ** -4 / s).astype(np.float32)       # |w| s <= 2^-4
  places = tie_placements(d, g)
  for r in range(n):
    for k in range(d // g):
      j1, j2, _ = places[(r + k) % len(places)]
      top = np.float32(rng.uniform(1.0, 2.0))                                   # |w| s = top at both, exactly
      for j in (k * g + j1, k * g + j2):
        w[r, j] = np.float32(rng.choice([-1.0, 1.0])) * top / np.float32(s[j])
      if (r + k) % 5 == 4:                                                      # a third column ties as well
        j3 = k * g + (j2 + 1) % g
        w[r, j3] = top / np.float32(s[j3])
  return w, s


def _signs(rng, n, d, g):
  w = rng.standard_normal((n, d)).astype(np.float32)
  w[rng.random((n, d)) < 0.1] = -0.0
  for r in range(n):
    what = r % 7
    if what == 1:
      w[r] = 0.0
    elif what == 2:
      w[r] = -0.0
    elif what == 3:
      w[r] = np.where(np.arange(d) % 2 == 0, -0.0, 0.0)
    elif what == 4:
      w[r, (5 + np.arange(d // g) * g)] = np.inf
    elif what == 5:
      for k in range(d // g):
        w[r, k * g + 9] = -np.inf           # the first of two infinities wins
        w[r, k * g + 22] = np.inf
  return w, _scales(rng, d)


def terms_input(c):
  """(w float32 [n, d], s float64 [d])"""
  rng = _rng(c, 2)
  if c.kind == "ties":
    return _ties(rng, c.n, c.d, c.g)
  if c.kind == "signs":
    return _signs(rng, c.n, c.d, c.g)
  w = {"wide": _wide, "squares": _squares}[c.kind](rng, c.n, c.d)
  return w, _scales(rng, c.d)


def masses(c):
  """mu2 for the objective of a terms case."""
  return np.exp(_rng(c, 3).standard_normal(c.d))


def winner_input(c):
  """(winner int32 [d/g, n], wsq float64 [d/g, n]); wsq = exp(4 normal)."""
  rng = _rng(c, 4)
  groups = c.d // c.g
  wsq = np.exp(4.0 * rng.standard_normal((groups, c.n)))
  if c.pattern == "one":
    local = np.repeat(rng.integers(0, c.g, (groups, 1)), c.n, axis=1)
  else:
    local = rng.integers(0, c.g - 1, (groups, c.n))
    local += local >= c.g // 3                      # uniform over the group but for one column, which no row picks
  return (local + np.arange(groups)[:, None] * c.g).astype(np.int32), wsq


def nonfinite_columns(rows=65, d=200):
  """x with a NaN in column 3, +inf in column 70, -inf in column 199 and a NaN and an inf in column 130; the expected
  class of every column ('nan', 'inf' or 'finite')."""
  x = _wide(np.random.default_rng(5), rows, d)
  x[64, 3] = np.nan
  x[10, 70] = np.inf
  x[0, 199] = -np.inf
  x[7, 130] = np.inf
  x[40, 130] = np.nan
  kinds = np.full(d, "finite", dtype=object)
  kinds[[3, 130]] = "nan"
  kinds[[70, 199]] = "inf"
  return x, kinds


# ------------------------------------------------------------------------------------------------ the reference's expressions
def reference_col(x, mean):
  x64 = x.astype(np.float64)
  return np.mean(x64 * x64, axis=0) if mean else (x64 * x64).sum(0)


def reference_terms(w, s, g):
  """top2, winner, wsq [d/g, n]; sums [d/g]; eff [d] -- ref oscar.py:175-194 and :236-246."""
  n, d = w.shape
  w64 = w.astype(np.float64)
  a = np.abs(w64) * s
  rows = np.arange(n)
  top2, winner, wsq, sums = [], [], [], []
  eff = np.zeros(d)
  for lo in range(0, d, g):
    mx = a[:, lo:lo + g].max(1)
    top2.append(mx * mx)
    sums.append(float((mx * mx).sum()))
    j_star = lo + np.argmax(a[:, lo:lo + g], 1)
    winner.append(j_star.astype(np.int32))
    wsq.append(w64[rows, j_star] ** 2)
    np.add.at(eff, j_star, w64[rows, j_star] ** 2)
  return dict(top2=np.array(top2), winner=np.array(winner), wsq=np.array(wsq), sums=np.array(sums), eff=eff)


def reference_winner_energy(winner, wsq, d):
  eff = np.zeros(d)
  for k in range(winner.shape[0]):
    np.add.at(eff, winner[k], wsq[k])
  return eff


# ------------------------------------------------------------------------------------------------ the in-order models
MUTATIONS = (
    "sq_f32",              # the square taken in float32
    "mag_f32",             # |w| * s taken in float32
    "colsum_pairwise",     # column sums added pairwise per column
    "mean_reciprocal",     # the mean as acc * (1 / rows)
    "tie_last",            # the last index wins ties
    "tie_across",          # ties resolved inside a lane (a wave) only: across lanes (waves) the later one wins
    "sum_unchunked",       # one pairwise sum over the whole vector
    "sum_left_to_right",   # the vector folded left to right
    "acc_linear",          # the eight accumulators folded ((((r0+r1)+r2)+r3)+...)
    "tree_misfold",        # the top two levels of a chunk's tree pair the wrong quarters: (A+C)+(B+D)
    "leaf_dropped",        # the last leaf of the last chunk left out
    "eff_masked_sum",      # winner energy as np.sum of the masked vector, per column
    "eff_partials_1024",   # winner energy as per-1024-row partial sums added afterwards
)


def _sq(v, mut):
  if mut == "sq_f32":
    with np.errstate(over="ignore", under="ignore"):
      return (v * v).astype(np.float64)                 # v float32: product rounded to float32
  v64 = v.astype(np.float64)
  return v64 * v64


def pairwise_leaves(lo, n):
  """The leaves (lo, n) of pairwise_sum's recursion, in order."""
  if n <= LEAF:
    return [(lo, n)]
  n2 = n // 2
  n2 -= n2 % 8
  return pairwise_leaves(lo, n2) + pairwise_leaves(lo + n2, n - n2)


def _leaf_sum(a, mut):
  """a [vectors, n <= 128]: NumPy's unrolled block, every vector at once."""
  n = a.shape[1]
  if n < 8:
    res = np.zeros(a.shape[0])
    for i in range(n):
      res = res + a[:, i]
    return res
  r = a[:, :8].copy()
  i = 8
  while i + 8 <= n:
    r = r + a[:, i:i + 8]
    i += 8
  if mut == "acc_linear":
    res = r[:, 0]
    for k in range(1, 8):
      res = res + r[:, k]
  else:
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
  while i < n:
    res = res + a[:, i]
    i += 1
  return res


def _chunk_sum(a, mut, last_chunk):
  """Pairwise sum of a [vectors, n <= 8192] along axis 1: leaves first, then the recursion over their sums."""
  leaves = pairwise_leaves(0, a.shape[1])
  sums = [_leaf_sum(a[:, lo:lo + ln], mut) for lo, ln in leaves]
  if mut == "leaf_dropped" and last_chunk:
    sums[-1] = np.zeros(a.shape[0])
  it = iter(sums)

  def halves(n):
    n2 = n // 2
    n2 -= n2 % 8
    return n2, n - n2

  def combine(n, top):
    if n <= LEAF:
      return next(it)
    left, right = halves(n)
    if top and mut == "tree_misfold" and left > LEAF and right > LEAF:
      (a_, b_), (c_, d_) = halves(left), halves(right)
      qa, qb, qc, qd = (combine(q, False) for q in (a_, b_, c_, d_))
      return (qa + qc) + (qb + qd)
    x = combine(left, False)
    return x + combine(right, False)

  return combine(a.shape[1], True)


def model_vector_sum(a, mut=None):
  """np.sum along axis 1 of contiguous FP64 vectors a [vectors, n]: 8192-element chunks added in order."""
  n = a.shape[1]
  if mut == "sum_left_to_right":
    res = a[:, 0].copy()
    for i in range(1, n):
      res = res + a[:, i]
    return res
  if mut == "sum_unchunked":
    return _chunk_sum(a, None, True)
  total = None
  for lo in range(0, n, CHUNK):
    part = _chunk_sum(a[:, lo:lo + CHUNK], mut, lo + CHUNK >= n)
    total = part if total is None else total + part
  return total


def model_col(x, mean, mut=None):
  rows = x.shape[0]
  sq = _sq(x, mut)
  if x.shape[1] == 1:
    # one column is a contiguous vector: NumPy drops the axis of length one and sums it as .sum() does
    acc = model_vector_sum(np.ascontiguousarray(sq.T), mut)
  elif mut == "colsum_pairwise":
    acc = _chunk_sum(np.ascontiguousarray(sq.T), None, True)
  else:
    acc = np.zeros(x.shape[1])
    for r in range(rows):
      acc = acc + sq[r]
  if not mean:
    return acc
  with np.errstate(over="ignore"):
    return acc * (1.0 / rows) if mut == "mean_reciprocal" else acc / float(rows)


def _first_max(a, part, mut):
  """(max, local index of the first maximum) along axis 1 of a [n, g]; `part` names the lane / wave of each column."""
  n, g = a.shape
  keep_later = (lambda new, old: new >= old) if mut == "tie_last" else (lambda new, old: new > old)

  def scan(cols):
    best, idx = a[:, cols[0]].copy(), np.full(n, cols[0])
    for j in cols[1:]:
      better = keep_later(a[:, j], best)
      best, idx = np.where(better, a[:, j], best), np.where(better, j, idx)
    return best, idx

  if mut != "tie_across":
    return scan(list(range(g)))
  best = idx = None
  for p in sorted(set(part)):
    b, i = scan([j for j in range(g) if part[j] == p])
    if best is None:
      best, idx = b, i
    else:
      better = b >= best
      best, idx = np.where(better, b, best), np.where(better, i, idx)
  return best, idx


def model_winner_energy(winner, wsq, d, mut=None):
  groups, n = winner.shape
  eff = np.zeros(d)
  if mut == "eff_masked_sum":
    for k in range(groups):
      for j in np.unique(winner[k]):
        eff[j] = np.sum(wsq[k][winner[k] == j])
    return eff
  if mut == "eff_partials_1024":
    for k in range(groups):
      for base in range(0, n, STAGE_ROWS):
        part = np.zeros(d)
        for r in range(base, min(n, base + STAGE_ROWS)):
          j = winner[k, r]
          part[j] = part[j] + wsq[k, r]
        eff = eff + part
    return eff
  for k in range(groups):
    for r in range(n):
      j = winner[k, r]
      eff[j] = eff[j] + wsq[k, r]
  return eff


def model_terms(w, s, g, mut=None):
  n, d = w.shape
  if mut == "mag_f32":
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
      a = (np.abs(w) * s.astype(np.float32)).astype(np.float64)
  else:
    a = np.abs(w.astype(np.float64)) * s
  local = np.arange(g)
  part = local // 4 if g != d else (local % TOP_THREADS) // 64
  rows = np.arange(n)
  top2, winner, wsq = [], [], []
  for lo in range(0, d, g):
    mx, idx = _first_max(a[:, lo:lo + g], part, mut)
    top2.append(mx * mx)
    winner.append((lo + idx).astype(np.int32))
    wsq.append(_sq(w[rows, lo + idx], mut))
  top2, winner, wsq = np.array(top2), np.array(winner), np.array(wsq)
  with np.errstate(invalid="ignore"):
    sums = model_vector_sum(top2, mut)
  return dict(top2=top2, winner=winner, wsq=wsq, sums=sums, eff=model_winner_energy(winner, wsq, d, mut))


def attacks(mut, c):
  """Whether case c has to show mutation `mut` (a condition on the case list, checked by the host test)."""
  if isinstance(c, ColCase):
    if mut == "sq_f32":
      return True
    if mut == "colsum_pairwise":
      return c.rows >= 63 and c.d > 1
    if c.d == 1:                                        # the vector sum's defects, on the one-column route
      if mut in ("sum_left_to_right", "acc_linear"):
        return c.rows >= 16
      if mut == "sum_unchunked":
        return c.rows > CHUNK
      if mut == "tree_misfold":
        return c.rows > CHUNK
      if mut == "leaf_dropped":
        return True
    if mut == "mean_reciprocal":
      return bool(c.mean) and c.rows & (c.rows - 1) != 0
    return False
  if isinstance(c, WinnerCase):
    if mut == "eff_masked_sum":                         # np.sum of fewer than 8 values is the in-order sum
      return c.pattern == "one" and c.n >= 16
    if mut == "eff_partials_1024":
      return c.n >= STAGE_ROWS + 2
    return False
  ordered = c.kind in ("wide", "squares")              # every addition rounds
  if mut in ("sq_f32", "mag_f32"):
    return ordered
  if mut == "tie_last":
    return c.kind in ("ties", "signs")
  if mut == "tie_across":
    return c.kind == "ties" and (c.g != c.d or c.d > 100)
  if mut == "sum_unchunked":                            # one pairwise sum of 2 * 8192 splits at 8192: the same additions
    return ordered and c.n > CHUNK and c.n != 2 * CHUNK
  if mut == "sum_left_to_right":
    return ordered and c.n >= 16
  if mut == "acc_linear":
    return ordered and c.n >= 8
  if mut == "tree_misfold":
    half = c.n // 2 - c.n // 2 % 8                      # both halves of a chunk split again
    return ordered and (c.n > CHUNK or (half > LEAF and c.n - half > LEAF))
  if mut == "leaf_dropped":
    return c.kind != "signs"
  if mut == "eff_masked_sum":
    return ordered and c.n >= 1023
  if mut == "eff_partials_1024":
    return ordered and c.n >= STAGE_ROWS + 2
  return False


# ------------------------------------------------------------------------------------------------ expected values
@functools.lru_cache(maxsize=None)
def expected(c):
  """(inputs, expected outputs) of a case: the reference's expressions. Cached and shared: treat as read-only."""
  if isinstance(c, ColCase):
    x = col_input(c)
    out = dict(out=reference_col(x, c.mean))
    inputs = dict(x=x)
  elif isinstance(c, WinnerCase):
    winner, wsq = winner_input(c)
    out = dict(eff=reference_winner_energy(winner, wsq, c.d))
    inputs = dict(winner=winner, wsq=wsq)
  else:
    w, s = terms_input(c)
    with np.errstate(invalid="ignore"):
      out = reference_terms(w, s, c.g)
    inputs = dict(w=w, s=s)
  for v in list(inputs.values()) + list(out.values()):
    v.setflags(write=False)
  return inputs, out


def model(c, mut=None):
  inputs, _ = expected(c)
  if isinstance(c, ColCase):
    return dict(out=model_col(inputs["x"], c.mean, mut))
  if isinstance(c, WinnerCase):
    return dict(eff=model_winner_energy(inputs["winner"], inputs["wsq"], c.d, mut))
  return model_terms(inputs["w"], inputs["s"], c.g, mut)


def same_bits(got, want):
  """'' when two dicts of arrays agree bit for bit (float64 as uint64 patterns, winner as int32), else what differs."""
  bad = []
  for name, w in want.items():
    g = got[name]
    if g.shape != w.shape or g.dtype != w.dtype:
      bad.append(f"{name}: {g.dtype}{g.shape} for {w.dtype}{w.shape}")
      continue
    gb, wb = (g.view(np.uint64), w.view(np.uint64)) if w.dtype == np.float64 else (g, w)
    if not np.array_equal(gb, wb):
      where = np.argwhere(gb != wb)
      first = tuple(where[0])
      bad.append(f"{name}: {len(where)} of {w.size} differ, first at {first}: {g[first]!r} for {w[first]!r}")
  return "; ".join(bad)
