"""What tests/test_gpu_oscar_scale_routes.py holds the OSCAR scale-search kernels to, proved without a GPU
(oscar_scale_cases.py):

  1. the reference's NumPy expressions equal the in-order models on every case, bit for bit -- so the orders oscar.hip
     reproduces (row by row, 8192-chunk pairwise, first maximum, add.at in order) are NumPy's;
  2. route() over the case list reaches every element of REQUIRED, the shapes the kernels' code singles out land where
     stated, and balanced_chunk agrees with a brute-force walk of the pairwise recursion;
  3. every mutation of the model changes at least one expected value of every case whose features it attacks: the
     inputs are such that a kernel with that defect cannot pass;
  4. the oracle's oscar_scale_objective is the sum over groups of the cases' expected sums times the group's mass."""
import numpy as np
import pytest

import oscar_scale_cases as S
from oracle import aeq_oracle as O

IDS = [S.case_id(c) for c in S.CASES]


# ---------------------------------------------------------------- 1. expressions == models
@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_numpy_expressions_equal_the_in_order_models(c):
  _, want = S.expected(c)
  assert S.same_bits(S.model(c), want) == ""


def test_vector_sum_is_chunked_pairwise_at_every_length_the_cases_use():
  rng = np.random.default_rng(11)
  lengths = sorted({c.n for c in S.TERMS_CASES} | {2, 8, 9, 127, 130, 8191, 20000})
  for n in lengths:
    a = np.exp(3.0 * rng.standard_normal((4, n)))
    want = np.array([float(row.sum()) for row in a])
    assert np.array_equal(S.model_vector_sum(a).view(np.uint64), want.view(np.uint64)), n


def test_expected_values_of_the_edges():
  for c in S.TERMS_CASES:
    (inputs, out) = S.expected(c)
    w, s = inputs["w"], inputs["s"]
    assert w.dtype == np.float32 and s.dtype == np.float64 and out["winner"].dtype == np.int32
    groups = np.arange(c.d // c.g)[:, None]
    assert ((out["winner"] >= groups * c.g) & (out["winner"] < (groups + 1) * c.g)).all()
    if c.kind == "signs":
      zero_rows = np.flatnonzero(~w.any(1))
      assert len(zero_rows) >= 3
      assert (out["winner"][:, zero_rows] == groups * c.g).all()                      # first column of the group
      assert (out["wsq"][:, zero_rows].view(np.uint64) == 0).all()                    # +0.0
      assert (out["top2"][:, zero_rows].view(np.uint64) == 0).all()
      assert np.signbit(w).any() and (w == -np.inf).any() and (w == np.inf).any()
      two = np.flatnonzero((np.isinf(w[:, :c.g])).sum(1) == 2)
      assert len(two) and (out["winner"][0, two] == 9).all()                          # the first of two infinities
      assert np.isinf(out["sums"]).all() and np.isinf(out["eff"]).any() and not np.isnan(out["eff"]).any()
    if c.kind == "ties":
      a = np.abs(w.astype(np.float64)) * s
      for k in range(c.d // c.g):
        block = a[:, k * c.g:(k + 1) * c.g]
        assert ((block == block.max(1, keepdims=True)).sum(1) >= 2).all()             # every maximum at >= 2 columns
      assert np.array_equal(np.log2(s), np.round(np.log2(s)))
    if c.kind == "squares":
      with np.errstate(over="ignore", under="ignore"):
        narrow = w * w
      assert np.isinf(narrow).any() and ((narrow == 0) & (w != 0)).any()              # float32 over- and underflow
      assert np.isfinite(out["sums"]).all()
    # a column that never wins is +0.0, bit for bit
    never = np.setdiff1d(np.arange(c.d), out["winner"].ravel())
    assert (out["eff"][never].view(np.uint64) == 0).all()
  for c in S.WINNER_CASES:
    inputs, out = S.expected(c)
    never = np.setdiff1d(np.arange(c.d), inputs["winner"].ravel())
    assert len(never) and (out["eff"][never].view(np.uint64) == 0).all()
    if c.pattern == "one":
      assert len(never) == c.d - c.d // c.g


def test_tie_placements_cover_lanes_waves_and_strides():
  for c in S.TERMS_CASES:
    if c.kind != "ties":
      continue
    places = S.tie_placements(c.d, c.g)
    assert c.n >= min(len(places), 3) or c.d // c.g >= 3, (c, "too few (row, group) pairs to meet the placements")
    assert all(0 <= j1 < j2 < c.g for j1, j2, _ in places)
    if c.g != c.d:
      assert any(j1 // 4 == j2 // 4 for j1, j2, _ in places)                          # inside one lane's four columns
      assert any(j1 // 4 != j2 // 4 for j1, j2, _ in places)                          # different lanes
    else:
      wave = lambda j: j % 256 // 64
      if c.d >= 256:
        assert any(wave(j1) < wave(j2) for j1, j2, _ in places)
      if c.d > 300:
        assert any(wave(j1) > wave(j2) for j1, j2, _ in places)                       # the first column in a later wave
        assert any(j1 % 256 == j2 % 256 for j1, j2, _ in places)                      # one thread, two strides
  row_ties = [c.d for c in S.TERMS_CASES if c.kind == "ties" and c.g == c.d]
  assert any(d > 300 for d in row_ties) and any(d == 256 for d in row_ties)
  assert {c.g for c in S.TERMS_CASES if c.kind == "ties" and c.g != c.d} == set(S.BLOCK_GROUPS)


def test_col_sumsq_nonfinite_classes():
  x, kinds = S.nonfinite_columns()
  for mean in (0, 1):
    with np.errstate(invalid="ignore"):
      want = S.reference_col(x, mean)
    assert np.array_equal(np.isnan(want), kinds == "nan") and np.array_equal(np.isposinf(want), kinds == "inf")


# ---------------------------------------------------------------- 2. routes
def test_case_list_reaches_every_required_feature():
  reached = set().union(*(S.features(c) for c in S.CASES))
  assert not S.REQUIRED - reached, sorted(S.REQUIRED - reached, key=str)


def test_ids_are_unique_and_name_the_features():
  assert len(set(IDS)) == len(IDS)
  for c in S.CASES:
    for f in S.features(c):
      if f[0] != "kind":
        assert S._show(f).replace(" ", "_") in S.case_id(c)


def test_routes_of_the_shapes_the_kernels_single_out():
  top = lambda n, d, g: S.route("group_terms", n, d, g)[0][0]
  total = lambda n: S.route("group_terms", n, 40, 40)[0][1]
  assert top(33, 32, 32) == "group_top_row_kernel"                 # g == d wins over g == 32
  assert [top(5, 3 * g, g) for g in S.BLOCK_GROUPS] == [f"group_top_block_kernel<{l}>" for l in (8, 16, 32, 64)]
  balanced = {8: (8, 0), 120: (120, 0), 128: (128, 0), 144: (72, 1), 256: (128, 1), 512: (128, 2), 1024: (128, 3),
              2048: (128, 4), 2816: (88, 5), 4096: (128, 5), 6144: (96, 6), 8192: (128, 6)}
  for n, want in balanced.items():
    assert S.balanced_chunk(n) == want and total(n) == "group_sum_balanced_kernel", n
  for n, last in {8200: (8, 0), 10240: (128, 4), 11008: (88, 5), 16384: (128, 6)}.items():
    assert S.balanced_chunk(n - (n - 1) // S.CHUNK * S.CHUNK) == last and total(n) == "group_sum_balanced_kernel", n
  for n in (1, 7, 33, 129, 136, 1000, 8193, 9000, 8192 + 136):
    assert total(n) == "group_sum_kernel", n
  assert {c.n for c in S.OBJECTIVE_CASES}.isdisjoint(S.SEEDED_N)
  assert {c.g == c.d for c in S.OBJECTIVE_CASES} == {True, False} and all(c.kind == "wide" for c in S.OBJECTIVE_CASES)
  assert all(c.n * c.d <= 1100000 for c in S.TERMS_CASES)


def test_balanced_chunk_is_exactly_the_complete_trees():
  def exact(n):
    """(leaf, depth) when every split of the pairwise recursion halves exactly, down to leaves the kernel's unrolled
    loop sums with no tail (a multiple of 8, at least 8)."""
    if n <= S.LEAF:
      return (n, 0) if n >= 8 and n % 8 == 0 else None
    n2 = n // 2
    n2 -= n2 % 8
    if 2 * n2 != n:
      return None
    below = exact(n2)
    return None if below is None else (below[0], below[1] + 1)

  for n in range(1, S.CHUNK + 1):
    assert S.balanced_chunk(n) == exact(n), n
    if exact(n):
      leaf, depth = exact(n)
      assert S.pairwise_leaves(0, n) == [(i * leaf, leaf) for i in range(1 << depth)]


# ---------------------------------------------------------------- 3. every mutation shows
ATTACKS = [(mut, c) for mut in S.MUTATIONS for c in S.CASES if S.attacks(mut, c)]


def test_every_mutation_attacks_cases_and_every_case_is_attacked():
  for mut in S.MUTATIONS:
    assert sum(1 for m, _ in ATTACKS if m == mut) >= 2, mut
  for c in S.CASES:
    if isinstance(c, S.WinnerCase) and c.n < 16:
      continue                                        # fewer than 8 additions per column: every order is the same
    assert any(k is c for _, k in ATTACKS), c
  # the features each mutation is there for
  by = lambda mut: {f for m, c in ATTACKS if m == mut for f in S.features(c)}
  assert {("bal", d, l) for d, l in ((2, 128), (3, 128), (4, 128), (5, 88), (5, 128), (6, 96), (6, 128))} <= by("tree_misfold")
  assert {f for f in S.REQUIRED if f[0] in ("bal", "bal-multi", "sum")} <= by("leaf_dropped")
  assert {f for f in S.REQUIRED if f[0] in ("bal", "bal-multi")} <= by("acc_linear")
  assert {f for f in S.REQUIRED if f[0] == "bal-multi"} | {("sum", "multi, last chunk of one"),
                                                           ("sum", "multi, last chunk unbalanced")} <= by("sum_unchunked")
  assert {("we", "three stagings, ragged tail"), ("we", "n=1023"), ("we", "n=1025"), ("we", "block g=256"),
          ("we", "2 slices, last partial"), ("we", "4 slices, last partial")} <= by("eff_masked_sum")
  assert {f for f in S.REQUIRED if f[0].startswith("group_top_block")} <= by("tie_across") | by("tie_last")
  assert {(f"group_top_block_kernel<{l}>", "one partial block") for l in (8, 16, 32)} <= by("tie_across")
  assert {("row", "d=256"), ("row", "d>256 ragged")} <= by("tie_across")
  assert {f for f in S.REQUIRED if f[0] == "col" and "mean" not in f[1]} <= by("sq_f32")


@pytest.mark.parametrize("mut,c", ATTACKS, ids=[f"{mut}-{S.case_id(c)}" for mut, c in ATTACKS])
def test_mutation_changes_an_expected_value(mut, c):
  _, want = S.expected(c)
  assert S.same_bits(S.model(c, mut), want) != "", "the case's inputs do not show this defect"


# ---------------------------------------------------------------- 4. tied to the oracle
@pytest.mark.parametrize("c", S.TERMS_CASES, ids=[S.case_id(c) for c in S.TERMS_CASES])
def test_oracle_objective_is_built_from_the_expected_sums(c):
  inputs, out = S.expected(c)
  w64, s, mu2 = inputs["w"].astype(np.float64), inputs["s"], S.masses(c)
  m = mu2 / (s * s)
  total = 0.0
  for k in range(c.d // c.g):
    total += float(out["sums"][k]) * float(m[k * c.g:(k + 1) * c.g].sum())
  block = c.g if c.g != c.d else 0
  with np.errstate(invalid="ignore"):
    assert O.oscar_scale_objective(w64, s, mu2, block) == total
