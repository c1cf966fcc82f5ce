"""The case list of test_gpu_octav_routes.py, checked without a GPU: every route of the three OCTAV entry points and every
data-dependent path of the rows and tail kernels is reached by a case whose id says so; the NumPy restatement of the
iteration (octav_route_cases.trajectory / iterates) is the oracle's, iterate by iterate; the inputs named as
order-sensitive tell NumPy's summation order from a plain left-to-right one; the EXACT inputs have sums that no order can
change; and the entry points refuse bad arguments before they launch anything.

test_final_constant_hides_a_perturbed_iterate records why the GPU file compares every iterate and not the last one."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import numpy_sum_model as M
import octav_route_cases as C
from oracle import aeq_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ALL_CASES = C.CASES + C.ENV_CASES + C.EXACT


def same_bits(a, b):
  a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
  return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------------ coverage ---
def test_case_list_reaches_every_route_and_path():
  routes, paths = set(), set()
  for c in ALL_CASES:
    routes |= set(C.case_route(c))
    paths |= set(C.case_paths(c))
  assert routes <= set(C.ALL_ROUTES) and paths <= set(C.ALL_PATHS)
  assert [r for r in C.ALL_ROUTES if r not in routes] == []
  assert [p for p in C.ALL_PATHS if p not in paths] == []
  ids = [C.case_id(c) for c in ALL_CASES]
  assert len(set(ids)) == len(ids)
  for c in C.CASES + C.EXACT:
    assert not c.env
  for c in C.ENV_CASES:
    assert c.env and set(c.envd) <= set(C.SWITCHES)


def test_ids_are_what_route_and_trajectory_derive():
  """The id of a case ends in its route and its paths, derived here once more from the case's numbers alone."""
  for c in ALL_CASES:
    r = C.route(c.entry, c.units, c.shape, c.aligned, c.workspace, c.env)
    want = "+".join(r)
    if c.entry == "exact" and r[0].startswith("rows"):
      found = set()
      for u in C.data(c):
        found |= C.paths(C.trajectory(u, c.bits, c.max_iter, c.f64), u, C.tail_cap(c.unit_len, c.env), "tail" in r, c.max_iter)[0]
      if found:
        want += "-" + "+".join(p for p in C.ALL_PATHS if p in found)
    assert C.case_id(c).endswith("-" + want), (C.case_id(c), want)


def test_routes_of_the_shapes_the_issue_names():
  r = C.route
  assert r("exact", 70, 32)[0] == "lanes<32>" and r("exact", 257, 256) == ("lanes<256>", "pick-n")
  assert r("exact", 5, 128, aligned=False)[0] == "wave-lds-w4" and r("exact", 5, 256, aligned=False)[0] == "rows<1,64>"
  assert r("exact", 3, 127)[0] == "wave-lds-w4" and r("exact", 3, 129)[0] == "rows<1,64>"
  assert [r("exact", 3, n)[0] for n in (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385)] == [
      "rows<1,64>", "rows<1,128>", "rows<1,128>", "rows<1,256>", "rows<1,256>", "rows<1,512>", "rows<1,512>", "rows<1,1024>",
      "rows<1,1024>", "wave-global-w4"]
  assert r("exact", 3, 4096)[1] == "tail" and r("exact", 3, 4096, workspace="base")[1] == "no-tail"
  assert r("exact", 3, 4096, env={C.E_TAIL: "0"})[1] == "no-tail" and r("exact", 3, 4096, env={C.E_TAIL: "1"})[1] == "tail"
  narrow = {C.E_NARROW: "1"}
  assert [r("exact", 3, n, env=narrow)[:2] for n in (4096, 4097, 8192, 8193, 12288, 12289, 16384)] == [
      ("rows<1,256>", "tail")] + [(f"rows<{s},256>", "no-tail") for s in (2, 2, 3, 3, 4, 4)]
  wave = {C.E_WAVE: "1"}
  assert [r("exact", 3, n, env=wave)[0] for n in (64, 4096, 4097, 5460, 5461, 8192, 8193, 16384)] == [
      "wave-lds-w4", "wave-lds-w4", "wave-lds-w3", "wave-lds-w3", "wave-lds-w2", "wave-lds-w2", "wave-lds-w1", "wave-lds-w1"]
  off = {C.E_LANES: "0"}
  assert r("exact", 256, 32, env=off)[0] == "groups" and r("exact", 70, 32, env=off)[0] == "wave-lds-w4"
  assert r("exact", 32, 256, env=off)[0] == "rows<1,64>" and r("exact", 8, 512)[0] == "rows<1,64>"
  assert r("nd", 0, (2, 5, 1))[0] == "cols" and r("nd", 0, (2, 5, 9))[0] == "segs" and r("nd", 0, (1, 4, 1000))[0] == "rows<1,64>"
  for lo, hi, name in ((4, 16, "fast<1,4>"), (260, 512, "fast<32,4>"), (516, 1024, "fast<64,4>"), (4100, 8192, "fast<256,8>"),
                       (16388, 32768, "fast<1024,8>"), (32772, 65536, "fast<1024,16>")):
    assert r("fast", 3, lo)[0] == name and r("fast", 3, hi)[0] == name
  assert C.tail_cap(129) == 64 and C.tail_cap(4096) == 512 and C.tail_cap(16384) == 2048
  assert C.tail_cap(4096, {C.E_TAIL_DIV: "2"}) == 2048 and C.tail_cap(16384, {C.E_TAIL_DIV: "256"}) == 64
  assert C.tail_cap(4096, {C.E_TAIL_DIV: "1"}) == 512 and C.tail_cap(4096, {C.E_TAIL_DIV: "300"}) == 512


# -------------------------------------------------------------------------------------------- the restatements ---
def oracle_iterate(c, x, k):
  """The oracle's k-th iterate of every unit with the early stop off."""
  with np.errstate(all="ignore"):
    if c.entry == "nd":
      return O.octav_clip(x, c.bits, (0, 2), k, C.DIVISOR, early_stop=False).reshape(-1)
    if c.f64:
      return O.octav_clip(x, c.bits, (1,), k, C.DIVISOR, early_stop=False).reshape(-1)
    return np.array([O.octav_clip(u, c.bits, None, k, C.DIVISOR, early_stop=False).reshape(-1)[0] for u in x], F)


@pytest.mark.parametrize("c", ALL_CASES, ids=C.case_id)
def test_iterates_are_the_oracles(c):
  """iterates() -- what the GPU file compares with -- equals the oracle run for k iterations, for every k, and so does the
  unit-by-unit trajectory() the paths are derived from; octav_step's promotions (step_next) reproduce every iterate from
  the sums taken in NumPy's order."""
  x = C.data(c)
  its = C.case_iterates(c)
  assert its.shape == (c.max_iter, c.units) and its.dtype == F
  for k in range(1, c.max_iter + 1):
    assert same_bits(oracle_iterate(c, x, k), its[k - 1]), k
  if c.entry != "exact":
    return
  for u, steps in enumerate(C.case_trajectories(c)):
    assert same_bits([st.next for st in steps], its[:, u]), u
    for i, st in enumerate(steps):
      assert same_bits(st.guess, F(1.0) if i == 0 else steps[i - 1].next)
      assert st.count_pos == int(st.runs_pos[1].sum()) and st.count_neg == int(st.runs_neg[1].sum())
      assert (st.runs_pos[1] <= C.CHUNK).all() and (st.runs_neg[1] <= C.CHUNK).all()


def test_float32_count_cases_differ_from_the_float64_count():
  """count_is_f64 = 0: at lengths that are no power of two the cases are chosen so that s * N in float32 changes the bits
  of some iterate (at a power of two s * N is exact in both forms and no input can tell them apart)."""
  cases = [c for c in C.CASES if not c.f64]
  assert {c.units > 1 for c in cases} == {True, False}
  assert {C.case_route(c)[0].split("<")[0] for c in cases} >= {"rows", "wave-lds-w4", "lanes"}
  for c in cases:
    other = C.iterates(C.data(c), c.bits, c.max_iter, 1)
    differ = not same_bits(other, C.case_iterates(c))
    assert differ == (c.unit_len & (c.unit_len - 1) != 0), C.case_id(c)


def plain_next(x, st, c):
  """The iterate a kernel would return that added the selected elements left to right in float32."""
  pos = np.cumsum(x[st.mask_pos], dtype=F)[-1] if st.count_pos else F(0)
  neg = np.cumsum(x[st.mask_neg], dtype=F)[-1] if st.count_neg else F(0)
  return C.step_next(pos, neg, st.count_pos, st.count_neg, x.size, c.bits, c.f64)


ORDER_SENSITIVE = [c for c in ALL_CASES if c.order_sensitive]


@pytest.mark.parametrize("c", ORDER_SENSITIVE, ids=C.case_id)
def test_order_sensitive_inputs_tell_summation_orders_apart(c):
  """numpy_sum_model's order gives every iterate of the case's first iterations; a plain left-to-right float32 sum of the
  same selected elements changes the bits of at least one iterate of some unit."""
  assert c.entry == "exact"
  differs = 0
  for u, steps in zip(C.data(c), C.case_trajectories(c)):
    for i, st in enumerate(steps[:4]):
      if i < 3 and st.count_pos + st.count_neg <= 6000:       # (the model is a Python loop over the row)
        model = C.step_next(M.masked_sum(u, st.mask_pos), M.masked_sum(u, st.mask_neg), st.count_pos, st.count_neg, u.size, c.bits, c.f64)
        assert same_bits(model, st.next), (i, model, st.next)
    for st in steps:
      differs += not same_bits(plain_next(u, st, c), st.next)
  assert differs > 0


def test_there_are_order_sensitive_cases_on_every_kind_of_kernel():
  heads = {C.case_route(c)[0].split("<")[0].split("-")[0] for c in ORDER_SENSITIVE}
  assert {"rows", "wave", "lanes"} <= heads
  assert any(C.case_route(c)[0] in ("rows<2,256>", "rows<3,256>", "rows<4,256>") for c in ORDER_SENSITIVE)


# ------------------------------------------------------------------------------------------------- exact inputs ---
@pytest.mark.parametrize("c", C.EXACT, ids=C.case_id)
def test_exact_units_have_sums_no_order_can_change(c):
  x = C.data(c)
  assert [c.unit_len for c in C.EXACT] == list(C.EXACT_LENGTHS)
  granule = np.ldexp(1.0, -C.exact_granule_log2(c.unit_len))
  for u in x:
    v = np.abs(u[np.isfinite(u)]).astype(np.float64)
    units = v / granule
    assert np.array_equal(units, np.rint(units)) and units.sum() <= C.EXACT_LIMIT
    fwd = np.cumsum(v.astype(F), dtype=F)[-1]
    bwd = np.cumsum(v.astype(F)[::-1], dtype=F)[-1]
    assert float(fwd) == float(bwd) == v.sum()
  assert np.isnan(x).any() and (x == 0).any() and np.signbit(x[x == 0]).any()
  assert np.isinf(x).any() or c.seed % 2 == 0
  if c.units >= 5:
    assert not x[3].any() and np.isposinf(x[4]).any() and np.isneginf(x[4]).any()


def test_exact_cases_cover_both_ends_of_every_instantiation():
  seen = {}
  for c in C.EXACT:
    seen.setdefault(C.case_route(c)[0], []).append(c.unit_len)
  assert list(seen) == [name for _, name in C.FAST]
  for (limit, name), lo in zip(C.FAST, [4] + [4 * l + 4 for l, _ in C.FAST[:-1]]):
    assert seen[name] == [lo, 4 * limit]
  for c in C.EXACT:
    assert c.units == (5 if c.unit_len < 1028 else 3)


# --------------------------------------------------------------------------------- why every iterate is compared ---
def _clip_with_a_nudge(x, bits, nudge_at, factor, max_iter=10):
  """ref octav.py:30-112 on one row with the early stop on; the iterate of iteration `nudge_at` is multiplied by `factor`."""
  s = F(4.0 ** (-bits) / C.DIVISOR)
  guess = F(1.0)
  for it in range(max_iter):
    old = guess
    mp, mn = x >= old, x <= -old
    denom = F(F(np.count_nonzero(mp)) + np.count_nonzero(mn))
    denom = F(F(denom * (F(1.0) - s)) + np.float64(s) * np.int64(x.size))
    guess = F(F(np.sum(x, where=mp, dtype=F) - np.sum(x, where=mn, dtype=F)) / denom)
    if it == nudge_at:
      guess = F(guess * F(factor))
    elif np.allclose(old, guess):
      break
  return guess


def test_final_constant_hides_a_perturbed_iterate(capsys):
  """Gaussian rows (sigma 0.02) of 256 / 1024 / 4096 elements, bits 4 and 8, iterate 1, 2 or 3 off by 1e-6, 1e-3 or 3e-2:
  once the masks settle the final constant is determined by the last masks alone, so most runs end on the unperturbed
  bits and a comparison of final constants cannot see the wrong iterate. Measured: see the printed share."""
  same = total = 0
  for n in (256, 1024, 4096):
    for seed in range(20):
      x = (np.random.default_rng([n, seed]).standard_normal(n) * 0.02).astype(F)
      for bits in (4, 8):
        clean = _clip_with_a_nudge(x, bits, -1, 1.0)
        assert same_bits(clean, O.octav_clip(x[None], bits, (1,), 10, C.DIVISOR))
        for at in (1, 2, 3):
          for factor in (1 + 1e-6, 1 + 1e-3, 1 + 3e-2):
            total += 1
            same += same_bits(clean, _clip_with_a_nudge(x, bits, at, factor))
  with capsys.disabled():
    print(f"\n{same} of {total} perturbed runs end on the unperturbed constant ({100.0 * same / total:.1f} %)")
  assert total == 1080 and 2 * same >= total


# ----------------------------------------------------------------------- iterates that move after 32 iterations ---
def test_search_for_a_unit_that_still_moves_after_32_iterations():
  """100 000 units of 8 elements with a few distinct magnitudes: at bits = 1 thousands of them end in a 2-cycle wider than
  np.allclose (the first one alternates between 4 and 4.0976), at bits 2 / 4 / 8 none of this population does. The found
  units are cases: as they are (the one-wave kernel) and inside rows of zeros (the rows kernel and its tail)."""
  found = C.moving_search()
  assert len(found) == 19612 and found[0] == 8
  for bits in (2, 4, 8):
    assert len(C.moving_search(bits)) == 0
  moving_cases = [c for c in C.CASES if c.kind in ("moving", "moving-row")]
  assert len(moving_cases) == 3 and all(c.max_iter == 40 and c.bits == C.MOVING_BITS and c.f64 for c in moving_cases)
  for c in moving_cases:
    x, its = C.data(c), C.case_iterates(c)
    before = np.concatenate((np.ones((1, c.units), F), its[:-1]))
    moving = ~np.isclose(before, its)
    assert moving[C.MOVING_FROM:].any(axis=0).sum() >= 3
    with np.errstate(all="ignore"):
      _, iters = O.octav_clip(x, c.bits, (1,), c.max_iter, C.DIVISOR, early_stop=True, return_iters=True)
    assert iters == 40
  rows = [c for c in moving_cases if c.kind == "moving-row"]
  assert {C.case_route(c)[1] for c in rows} == {"tail", "no-tail"}
  assert "handover" in C.case_paths([c for c in rows if C.case_route(c)[1] == "tail"][0])


# ---------------------------------------------------------------------------------------------- argument checks ---
@functools.lru_cache(maxsize=None)
def library():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def test_workspace_queries_match_the_restatement(monkeypatch):
  for name in C.SWITCHES:
    monkeypatch.delenv(name, raising=False)
  lib = library()
  for units, max_iter in ((0, 10), (-1, 10), (5, 0), (5, -3)):
    assert lib.mi355q_octav_workspace_bytes(units, max_iter) == 0
    assert lib.mi355q_octav_rows_workspace_bytes(units, 4096, max_iter) == 0
  for units, max_iter in ((1, 1), (3, 10), (257, 40), (5, 64)):
    assert lib.mi355q_octav_workspace_bytes(units, max_iter) == C.workspace_bytes(units, max_iter)
    for n in (1, 128, 129, 1000, 4096, 8193, 16384, 16385):
      assert lib.mi355q_octav_rows_workspace_bytes(units, n, max_iter) == C.rows_workspace_bytes(units, n, max_iter), (units, n)
  assert C.rows_workspace_bytes(3, 128, 10) == C.workspace_bytes(3, 10) == C.rows_workspace_bytes(3, 16385, 10)
  assert C.rows_workspace_bytes(3, 129, 10) > C.workspace_bytes(3, 10)


def test_entries_refuse_bad_arguments_before_they_launch(monkeypatch):
  """Host memory stands in for every buffer: each of these calls returns before it touches a device."""
  for name in C.SWITCHES:
    monkeypatch.delenv(name, raising=False)
  lib = library()
  err = lib.mi355q_last_error
  buf = ctypes.create_string_buffer(b"\x5a" * 8192, 8192)
  base = (ctypes.addressof(buf) + 63) & ~63
  need = C.workspace_bytes(3, 10)

  def exact(**kw):
    a = dict(x=base, units=3, n=64, bits=4, it=10, f64=1, out=base, iters=base, ws=base, ws_bytes=need)
    a.update(kw)
    return lib.mi355q_octav_clip_f32(a["x"], a["units"], a["n"], a["bits"], a["it"], 3.0, 1, a["f64"], a["out"], a["iters"], a["ws"],
                                     a["ws_bytes"], None)

  def fast(**kw):
    a = dict(x=base, units=3, n=64, bits=4, it=10, out=base, iters=base, ws=base, ws_bytes=need)
    a.update(kw)
    return lib.mi355q_octav_clip_fast_f32(a["x"], a["units"], a["n"], a["bits"], a["it"], 3.0, 1, a["out"], a["iters"], a["ws"],
                                          a["ws_bytes"], None)

  def nd(**kw):
    a = dict(x=base, outer=2, units=3, n=64, bits=4, it=10, out=base, iters=base, ws=base, ws_bytes=need)
    a.update(kw)
    return lib.mi355q_octav_clip_nd_f32(a["x"], a["outer"], a["units"], a["n"], a["bits"], a["it"], 3.0, 1, a["out"], a["iters"],
                                        a["ws"], a["ws_bytes"], None)

  for fn in (exact, fast, nd, lambda **kw: nd(outer=1, **kw)):
    assert fn(units=-1) == -1 and b"negative shape" in err()
    assert fn(n=-1) == -1 and b"negative shape" in err()
    for it in (0, -1, 65):
      assert fn(it=it) == -1 and b"max_iter must be in [1, 64]" in err()
    for bits in (0, 17):
      assert fn(bits=bits) == -1 and b"bits must be in [1, 16]" in err()
    assert fn(n=0) == -2 and b"empty reduction unit" in err()
    assert fn(x=None) == -1 and b"null pointer" in err()
    assert fn(out=None) == -1 and b"null pointer" in err()
    assert fn(ws=None) == -1 and b"workspace too small" in err()
    assert fn(ws_bytes=need - 1) == -1 and f"need {need} bytes".encode() in err()
    assert fn(units=0, x=None, out=None, ws=None, ws_bytes=0) == 0 and err() == b""
  assert exact(n=0x7FFFFFFF - 63) == -3 and b"unit_len too large" in err()
  assert nd(outer=-1) == -1 and b"negative shape" in err()
  assert nd(outer=0) == -2 and b"empty reduction unit" in err()
  assert nd(outer=1 << 31) == -3 and b"reduction unit too large" in err()
  assert nd(outer=1 << 20, n=1 << 12) == -3 and b"reduction unit too large" in err()
  for n in (6, 65540):
    assert fast(n=n) == -3 and b"multiple of 4" in err()
  assert fast(units=1 << 31, ws_bytes=C.workspace_bytes(1 << 31, 10)) == -3 and b"too many units" in err()
  assert fast(x=base + 4) == -1 and b"16-byte aligned" in err()
  assert buf.raw == b"\x5a" * 8192
