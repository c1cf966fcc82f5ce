"""What tests/test_gpu_mse_routes.py holds the MSE scale kernels to, proved without a GPU (mse_route_cases.py):

  1. the reference's NumPy expressions equal the in-order models on every case, bit for bit -- so the orders
     mse_scale.hip reproduces (8192-element chunks, pairwise with splits at multiples of 8, eight accumulators and a
     tail, row by row, segment by segment, one vector for one channel) are NumPy's;
  2. route() over the case list reaches every element of REQUIRED, agrees with balanced_chunk restated from common.h at
     every length up to three chunks and a leaf, and the lengths the kernels' code singles out land where stated;
  3. every mutation of the model changes at least one expected scale or integer of every case whose features it
     attacks: the inputs are such that a kernel with that defect cannot pass."""
import collections

import numpy as np
import pytest

import mse_route_cases as S
from oracle import aeq_oracle as O

IDS = [S.case_id(c) for c in S.CASES]


# ---------------------------------------------------------------- 1. expressions == models
@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_numpy_expressions_equal_the_in_order_models(c):
  _, want = S.expected(c)
  assert S.same_bits(S.model(c), want) == ""


def test_sum_of_squares_is_chunked_pairwise_at_every_length_the_issue_names():
  rng = np.random.default_rng(11)
  for n in S.BALANCED_LENGTHS + S.LEAVES_LENGTHS:
    x = rng.standard_normal((4, n)).astype(np.float32)
    want = np.mean(x**2, axis=1)
    got = S.model_sumsq(x) / np.float32(n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n


def test_restated_quantize_is_the_oracles_where_the_oracle_can_be_asked():
  x = S.expected(S.RequantCase(7, 1000, 8, 1, "wide"))[0]["x"]
  scale = S.reference_scale(x, S.MULS[0]).reshape(-1, 1)
  zp = np.zeros(scale.shape, np.int32)
  for bits in range(2, 9):
    narrow = int(bits >= 8)
    want = O.uniform_quantize(x, scale, zp, bits, True, quantized_dim=0)
    assert want.dtype == np.int8
    assert np.array_equal(S.model_q(x, scale, bits, narrow), want)
    assert np.array_equal(S.reference_q(x, scale, bits, narrow), want)
    for other in (0, 1):                                 # the written-out lines and the model agree on every bound
      assert np.array_equal(S.reference_q(x, scale, bits, other), S.model_q(x, scale, bits, other))


def test_expected_values_of_the_edges():
  seen = collections.Counter()
  for c in S.CASES:
    inputs, out = S.expected(c)
    x = inputs["x"]
    assert x.dtype == np.float32 and all(v.dtype == (np.int8 if k == "q" else np.float32) for k, v in out.items())
    scales = [v for k, v in out.items() if k != "q"]
    units = c.channels if isinstance(c, S.NdCase) else c.units
    assert all(s.shape == (units,) for s in scales)
    by_unit = x.reshape(units, -1) if not isinstance(c, S.NdCase) else \
        np.moveaxis(x.reshape(c.outer, c.channels, c.inner), 1, 0).reshape(units, -1)
    if c.kind == "squares":
      with np.errstate(all="ignore"):
        narrow = by_unit * by_unit
      if units > 1:
        assert ((narrow == 0) & (by_unit != 0)).any() and np.isinf(narrow).any()      # float32 under- and overflow
        assert (scales[0] == 0).any() and np.isposinf(scales[0]).any() and (np.isfinite(scales[0]) & (scales[0] > 0)).any()
      seen["squares"] += 1
    if c.kind == "signs":
      assert np.signbit(by_unit[by_unit == 0]).any()
      zero = np.flatnonzero(~by_unit.any(1))
      assert len(zero) >= 2 and all((s[zero].view(np.uint32) == 0).all() for s in scales)   # scale +0.0
      if "q" in out:                                     # 0 / 0 is NaN, which the cast makes 0
        assert (out["q"][zero] == 0).all()
        outlier = np.flatnonzero(np.abs(by_unit).max(1) == 250.0)
        hi, lo = 2 ** (c.bits - 1) - 1, -2 ** (c.bits - 1) + c.narrow
        assert len(outlier) >= 2 and ((out["q"][outlier] != 0).sum(1) == 1).all()        # everything else rounds to 0
        if c.n >= 100:                                   # and the outlier clips, at either bound
          assert set(np.unique(out["q"][outlier])) == {lo, 0, hi}
      seen["signs"] += 1
    if c.kind == "nonfinite":
      assert (np.isnan(scales[0]).any() and np.isposinf(scales[0]).any()) if units >= 3 else not np.isfinite(scales[0]).all()
      if units > 5:
        assert np.isfinite(scales[0]).any()
      n = by_unit.shape[1]
      where = {w for u in range(units) for _, _, w in [S.nonfinite_plants(n)[u % 7]]}
      assert {"first leaf", "last leaf", "last chunk"} <= where or units < 4
      seen["nonfinite"] += 1
    if c.kind == "ties":
      with np.errstate(all="ignore"):
        v = x / out["scale"][:, None]
      ties = (v - np.floor(v) == 0.5) & (np.abs(v) < 2 ** (c.bits - 1) - 1)
      assert (ties.sum(1) >= 2).all() and ties.sum() >= 3 * c.units, ties.sum(1)      # in every unit
      odd = ties & (np.floor(v) % 2 == 1)
      assert odd.any() and (ties & ~odd).any() and (ties & (v < 0)).any() and (ties & (v > 0)).any()
      seen["ties"] += 1
  assert min(seen[k] for k in ("squares", "signs", "nonfinite", "ties")) >= 5
  # the leaf tails, last leaves and last chunks that carry a non-finite value
  tails = {S.nonfinite_plants(c.n)[2][2] for c in S.SCALE_CASES if c.kind == "nonfinite"}
  assert tails == {"leaf tail", "last element"}


def test_cases_stay_small():
  for c in S.CASES:
    assert S.expected(c)[0]["x"].size <= 9 * 25576, c


# ---------------------------------------------------------------- 2. routes
def test_case_list_reaches_every_required_feature():
  reached = set().union(*(S.features(c) for c in S.CASES))
  assert not S.REQUIRED - reached, sorted(S.REQUIRED - reached, key=str)


def test_ids_are_unique():
  assert len(set(IDS)) == len(IDS)


def test_routes_of_the_lengths_the_kernels_single_out():
  kernel = lambda n: S.route("scale", 5, n)[0][0]
  for n in S.BALANCED_LENGTHS:
    assert kernel(n) == "mse_scale_balanced_kernel", n
    assert S.route("requant", 5, n)[0] == ("mse_scale_balanced_kernel (fused quantize)",), n
    assert S.route("requant", 5, n, two_kernels_env=True)[0] == ("mse_scale_balanced_kernel", "mi355q_quantize_f32"), n
  for n in S.LEAVES_LENGTHS:
    assert kernel(n) == "mse_scale_leaves_kernel", n
    assert S.route("requant", 5, n)[0] == ("mse_scale_leaves_kernel", "mi355q_quantize_f32"), n
  last = lambda n: S.balanced_chunk(n - (n - 1) // S.CHUNK * S.CHUNK)
  assert [last(n) for n in (8, 120, 128, 144, 512, 576, 1024, 4608, 8192)] == \
      [(8, 0), (120, 0), (128, 0), (72, 1), (128, 2), (72, 3), (128, 3), (72, 6), (128, 6)]
  assert [last(n) for n in (8200, 8768, 11008, 16672, 3 * 8192)] == [(8, 0), (72, 3), (88, 5), (72, 2), (128, 6)]
  leaves = lambda n: len(S.pairwise_leaves(0, n - (n - 1) // S.CHUNK * S.CHUNK))
  assert [leaves(n) for n in (1032, 8191, 8292, 25576)] == [9, 65, 1, 8]
  # the addresses: x by floats (16-byte alignment), q_out by bytes (4-byte alignment)
  for xo in range(8):
    for qo in range(8):
      one = S.route("requant", 3, 1024, xo, qo)[0] == ("mse_scale_balanced_kernel (fused quantize)",)
      assert one == (xo % 4 == 0 and qo % 4 == 0)
  # the nd entry
  nd = lambda outer, channels, inner: S.route("scale_nd", channels, (outer, inner))[0]
  assert nd(1, 5, 1024) == ("mse_scale_balanced_kernel",) and nd(1, 5, 1000) == ("mse_scale_leaves_kernel",)
  assert nd(1, 5, 1) == ("mse_scale_leaves_kernel",)                          # outer == 1 wins over inner == 1
  assert nd(3, 5, 1) == ("mse_scale_cols_kernel",) and nd(3, 5, 2) == ("mse_scale_seg_kernel",)
  assert nd(64, 1, 1) == ("mse_scale_balanced_kernel",) and nd(3, 1, 8292) == ("mse_scale_leaves_kernel",)


def test_route_agrees_with_balanced_chunk_at_every_length():
  def common_h(n):
    """balanced_chunk of csrc/common.h, statement by statement."""
    d = 0
    while (n >> d) > 128:
      d += 1
    l = n >> d
    if (l << d) != n or l < 8 or (l % 8) != 0:
      return None
    return l, d

  def exact(n):
    """(leaf, depth) when every split of the pairwise recursion halves exactly, down to leaves with no tail."""
    if n <= S.LEAF:
      return (n, 0) if n >= 8 and n % 8 == 0 else None
    n2 = n // 2
    n2 -= n2 % 8
    if 2 * n2 != n:
      return None
    below = exact(n2)
    return None if below is None else (below[0], below[1] + 1)

  for n in range(1, 3 * S.CHUNK + 129 + 1):
    last = n - (n - 1) // S.CHUNK * S.CHUNK
    want = common_h(last)
    assert 1 <= last <= S.CHUNK and (n - last) % S.CHUNK == 0
    (kernel,), feats = S.route("scale", 3, n)
    assert kernel == ("mse_scale_balanced_kernel" if want else "mse_scale_leaves_kernel"), n
    if want:
      assert {("bal", "leaf", want[0]), ("bal", "depth", want[1])} <= feats, n
    fused = S.route("requant", 3, n)[0]
    assert (len(fused) == 1) == (want is not None and n % 4 == 0), n
    if n <= S.CHUNK:
      assert want == exact(n), n
      if want:
        assert S.pairwise_leaves(0, n) == [(i * want[0], want[0]) for i in range(1 << want[1])]


# ---------------------------------------------------------------- 3. every mutation shows
ATTACKS = [(mut, c) for mut in S.MUTATIONS for c in S.CASES if S.attacks(mut, c)]


def test_every_mutation_attacks_cases_and_shows_in_each():
  """The list the issue asks for: every mutation with the number of cases that expose it."""
  lines = []
  for mut in S.MUTATIONS:
    cases = [c for m, c in ATTACKS if m == mut]
    shown = sum(1 for c in cases if S.same_bits(S.model(c, mut), S.expected(c)[1]) != "")
    lines.append(f"{mut}: attacks {len(cases)} cases, {shown} expose it")
    assert len(cases) >= 2 and shown == len(cases), lines[-1]
  print("\n".join(lines))


def test_every_ordered_case_is_attacked_and_the_features_each_mutation_is_there_for():
  for c in S.CASES:
    if c.kind in ("wide", "ties"):
      assert any(k is c for _, k in ATTACKS), c
  by = lambda mut: {f for m, c in ATTACKS if m == mut for f in S.features(c)}
  req = lambda *heads: {f for f in S.REQUIRED if f[0] in heads}
  assert req("bal", "leaves") - {("leaves", "length < 8")} <= by("acc_sequential") & by("leaf_left_to_right")
  assert req("bal", "leaves", "seg", "cols") <= by("square_add_fused") & by("mean_f64")
  assert {("leaves", f) for f in ("one leaf with a tail", "two leaves", "more than 64 leaves",
                                  "multi-chunk, unbalanced last chunk")} <= by("tail_dropped") & by("tail_before_combine")
  assert {("leaves", f) for f in ("two leaves", "leaf count no multiple of 8", "more than 64 leaves", "three chunks")} <= \
      by("split_not_rounded")
  assert {("bal", "two chunks, last of depth 0"), ("bal", "two chunks, last of depth 3"), ("bal", "three or more chunks"),
          ("leaves", "multi-chunk, unbalanced last chunk"), ("leaves", "three chunks"), ("seg", "inner > 8192"),
          ("nd", "one channel, inner = 1"), ("nd", "one channel, inner > 1")} <= by("no_chunking")
  assert {("bal", "two chunks, last of depth 3"), ("bal", "three or more chunks"), ("leaves", "three chunks")} <= by("last_table_full")
  assert {("bal", "three or more chunks"), ("leaves", "three chunks")} <= by("chunks_pairwise")
  assert {("bal", "depth", 6), ("bal", "leaf", 72), ("bal", "two chunks, last of depth 0")} <= by("steps_sequential")
  assert req("seg") <= by("seg_one_run")
  assert {("cols", f) for f in ("outer = 8k", "outer = 8k + t", "channels < 256", "channels = 256", "channels > 256")} <= \
      by("cols_pairwise") & by("cols_eight_partials")
  assert {("nd", "one channel, inner = 1"), ("nd", "one channel, inner > 1")} <= by("one_channel_in_pieces")
  assert req("requant") <= by("ties_away") & by("quant_reciprocal") & by("narrow_flipped")
  # every width the entry takes, with either bound, shows a bound on the wrong side
  flipped = {(c.bits, c.narrow) for m, c in ATTACKS if m == "narrow_flipped" and c.n in S.BITS_LENGTHS}
  assert flipped == {(b, nw) for b in range(2, 9) for nw in (0, 1)}


@pytest.mark.parametrize("mut,c", ATTACKS, ids=[f"{mut}-{S.case_id(c)}" for mut, c in ATTACKS])
def test_mutation_changes_an_expected_value(mut, c):
  _, want = S.expected(c)
  assert S.same_bits(S.model(c, mut), want) != "", "the case's inputs do not show this defect"
