"""hadamard_route_cases.py checked on the CPU: the model gives the exact answers of the impulse and integer classes
under every order, stays inside the derived float64 bound, tells one route's order from another's and a product after
the butterflies from one before them; route(), delta_route() and stage_order() at every boundary; the case list
reaches what the GPU suite promises. And the Python layer refuses a Hadamard size of 1 before it touches the GPU."""
import numpy as np
import pytest

import hadamard_route_cases as H
from oracle import aeq_oracle as O

from mi355q import qtyping as q
from mi355q.algorithms.uniform_quantize import hadamard_rotation

F = np.float32


def _orders(h):
  """Every order any route could run at h, plus the reverse of the plain one."""
  out = {H.stage_order("r2", h), tuple(reversed(H.stage_order("r2", h)))}
  for name in ("t12", "t13", "t14"):
    if H.TILE_FROM <= h <= 1 << int(name[1:]):
      out.add(H.stage_order(name, h))
  return sorted(out)


def _differ(a, b):
  return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# ------------------------------------------------------------------------------------------------ routes
def test_routes_at_every_boundary():
  for h, want in ((1, "r2"), (2, "r2"), (128, "r2"), (256, "t12"), (1024, "t12"), (2048, "t12"), (4096, "t12"),
                  (8192, "t13"), (16384, "t14")):
    assert H.route(h, True, True) == want and H.delta_route(h) == want
    for xa, oa in ((False, True), (True, False), (False, False)):
      assert H.route(h, xa, oa) == "r2"
  for bad in (0, 3, 32768):
    with pytest.raises(AssertionError):
      H.delta_route(bad)


def test_stage_orders_at_every_boundary():
  assert H.stage_order("r2", 1) == ()
  assert H.stage_order("r2", 2) == (0,)
  assert H.stage_order("r2", 128) == tuple(range(7))
  assert H.stage_order("r2", 16384) == tuple(range(14))
  assert H.stage_order("t12", 256) == tuple(range(8)) == H.stage_order("r2", 256)
  assert H.stage_order("t12", 1024) == tuple(range(10)) == H.stage_order("r2", 1024)
  assert H.stage_order("t12", 2048) == (0, 1, 10, 2, 3, 4, 5, 6, 7, 8, 9)
  assert H.stage_order("t12", 4096) == (0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9)
  assert H.stage_order("t13", 8192) == (0, 1, 11, 12, 2, 3, 4, 5, 6, 7, 8, 9, 10)
  assert H.stage_order("t14", 16384) == (0, 1, 12, 13, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
  for h in H.SIZES:
    for name in H.ROUTES:
      if name == "r2" or H.TILE_FROM <= h <= 1 << int(name[1:]):
        assert sorted(H.stage_order(name, h)) == list(range(H.log2(h)))      # every stage once


def test_scale_factor_is_a_power_of_two_exactly_for_powers_of_four():
  for h in H.SIZES:
    r = H.scale_factor(h)
    assert r.dtype == F
    assert (float(r) == 2.0 ** -(H.log2(h) // 2)) == H.is_power_of_four(h)


# ------------------------------------------------------------------------------------------------ the exact classes
@pytest.mark.parametrize("h", H.SIZES)
def test_model_gives_the_impulse_answers_under_every_order(h):
  x, want = H.impulses(h, 3)
  assert {int(np.flatnonzero(v)[0]) for v in x.reshape(-1, h)} == set(H.impulse_positions(h, 0))
  assert {0, h - 1, h // 2, 1 % h} <= set(H.impulse_positions(h, 0))
  assert (np.count_nonzero(x.reshape(-1, h), axis=1) == 1).all() and not H.has_subnormals(want)
  if h <= 1024:                                                  # the closed form is the matrix product
    dense = x.reshape(-1, h).astype(np.float64) @ (O.hadamard_matrix(h) if h > 1 else np.ones((1, 1))).astype(np.float64)
    assert np.array_equal(dense, want.reshape(-1, h).astype(np.float64))
  for order in _orders(h):
    assert H.same_bits(H.model(x, h, order).reshape(x.shape), want) == "", order


@pytest.mark.parametrize("h", [h for h in H.SIZES if H.is_power_of_four(h)])
def test_model_gives_the_integer_answers_under_every_order(h):
  x, want = H.integers(h, 3)
  lim = 1 << (23 - H.log2(h))
  assert np.abs(x).max() == lim - 1 and np.abs(want).max() == (lim - 1) * h * float(H.scale_factor(h))
  assert np.array_equal(H.fwht64(x, h).reshape(want.shape), want.astype(np.float64))
  if h <= 1024 and h > 1:
    assert np.array_equal(H.sylvester_int(x, h), x.reshape(-1, h).astype(np.int64) @ np.rint(O.hadamard_matrix(h) * np.sqrt(h)).astype(np.int64))
  for order in _orders(h):
    assert H.same_bits(H.model(x, h, order).reshape(x.shape), want) == "", order


# ------------------------------------------------------------------------------------------------ the float class
@pytest.mark.parametrize("h", H.SIZES)
def test_model_stays_inside_the_float64_bound(h):
  n_vec = 7
  x, plant = H.floats(h, n_vec)
  assert set(H.FLOAT_PLANTS) <= set(plant.ravel())
  finite = ~np.isin(plant, ("nan", "inf"))
  xs = x[finite]
  want64, tol = H.fwht64(xs, h), H.bound(xs, h)
  worst = 0.0
  for order in _orders(h):
    got = H.model(xs, h, order)
    err = np.abs(got.astype(np.float64) - want64)
    assert (err <= tol).all(), order
    nz = tol[:, 0] > 0
    worst = max(worst, float((err[nz] / tol[nz]).max()))
  print(f"h={h}: worst |model - float64| / bound = {worst:.3f}")
  assert (H.model(x[plant == "zero"], h, H.stage_order("r2", h)).view(np.uint32) == 0).all()


@pytest.mark.parametrize("h", H.SIZES)
def test_nan_and_inf_stay_in_their_vectors(h):
  x, plant = H.floats(h, 3)
  got = H.model(x, h, H.stage_order("r2", h)).reshape(x.shape)
  assert np.array_equal((~np.isfinite(got)).any(axis=-1), np.isin(plant, ("nan", "inf")))
  assert np.array_equal(np.isnan(got).any(axis=-1), plant == "nan")      # an output holds one term per input: no inf - inf
  assert np.isnan(got[plant == "nan"]).all() and np.isinf(got[plant == "inf"]).all()      # every output takes every input


def test_planted_values_are_where_the_docstring_says():
  x, plant = H.floats(256, 19)
  assert x.shape == (1, 19, 256) and list(plant[0, :6]) == list(H.FLOAT_PLANTS)
  v = x[0]
  assert abs(v[0, -1]) >= 4096 * np.abs(v[0, :-1]).max()
  assert np.signbit(v[1, 0]) and v[1, 0] == 0 and np.signbit(v[1, 128]) and v[1, 128] == 0
  assert not v[2].any() and np.isnan(v[3]).sum() == 1 and np.isposinf(v[4]).sum() == 1
  assert np.isfinite(np.delete(v, (3, 4), axis=0)).all()
  x1, plant1 = H.floats(256, 1)
  assert x1.shape == (6, 1, 256) and list(plant1[:, 0]) == list(H.FLOAT_PLANTS)
  xi, _ = H.impulses(16384, 3)
  assert xi.shape[1:] == (3, 16384) and xi.shape[0] * 3 >= len(H.impulse_positions(16384, 0))


# ------------------------------------------------------------------------------------------------ discrimination
@pytest.mark.parametrize("h", [2048, 4096, 8192, 16384])
def test_another_routes_order_changes_words_from_2048_on(h):
  x, plant = H.floats(h, 3)
  xs = x[plant == "plain"][:1]
  tile, plain = H.stage_order(H.delta_route(h), h), H.stage_order("r2", h)
  assert tile != plain
  a, b = H.model(xs, h, tile), H.model(xs, h, plain)
  assert _differ(a, b) > h // 4                                   # not a word here and there: most of the vector
  if h == 8192:                                                   # and the tile kernels among themselves
    wrong = tuple(v for v in H.stage_order("t14", 16384) if v < 13)
    assert _differ(a, H.model(xs, h, wrong)) > h // 4


@pytest.mark.parametrize("h", [256, 512, 1024])
def test_the_orders_coincide_below_2048(h):
  assert H.stage_order("t12", h) == H.stage_order("r2", h)


@pytest.mark.parametrize("h", [h for h in H.SIZES if not H.is_power_of_four(h)])
def test_scaling_after_the_butterflies_changes_words_for_odd_log2(h):
  x, plant = H.floats(h, 3)
  xs = x[plant == "plain"]
  order = H.stage_order(H.delta_route(h), h)
  assert _differ(H.model(xs, h, order), H.model(xs, h, order, scale_after=True)) > 0


def test_an_approximate_scale_changes_the_impulse_answers():
  for h in (2, 8, 128, 2048, 8192):
    x, _ = H.impulses(h, 3)
    near = np.nextafter(H.scale_factor(h), F(2))
    assert _differ((x * near).astype(F), (x * H.scale_factor(h)).astype(F)) > 0


def test_same_bits_reports_nan_moves_and_signed_zeros():
  a = np.array([1.0, np.nan, 0.0], F)
  assert H.same_bits(a, a.copy()) == ""
  assert H.same_bits(a, np.array([1.0, np.nan, -0.0], F)) != ""
  assert H.same_bits(a, np.array([np.nan, 1.0, 0.0], F)) != ""
  assert H.same_bits(a, a.astype(np.float64)) != "" and H.same_bits(a, a[:2]) != ""
  quiet = np.array([0x7FC00000, 0xFFC00001], np.uint32).view(F)
  assert H.same_bits(quiet[:1], quiet[1:]) == ""                   # any NaN for a NaN


# ------------------------------------------------------------------------------------------------ the case lists
def test_case_list_reaches_every_route_and_edge():
  by = {}
  for c in H.CASES:
    by.setdefault(c.route, []).append(c)
    assert H.route(c.h, c.x_off == 0, c.out_off == 0) == c.route
    assert c.n_vec * c.h * 4 <= 256 * 1024
  assert set(by) == set(H.ROUTES)
  assert len({c.id for c in H.CASES}) == len(H.CASES)
  fallback = {(c.h, c.x_off, c.out_off) for c in by["r2"] if c.h >= H.TILE_FROM}
  assert {(h, 1, 1) for h in (256, 2048, 4096, 8192, 16384)} <= fallback
  assert {(h, xo, oo) for h in (256, 4096) for xo, oo in ((1, 0), (0, 1))} <= fallback
  assert {(c.h, c.n_vec) for c in by["r2"] if c.h < H.TILE_FROM} >= {(1, 5), (2, 1027), (8, 259), (128, 19)}
  assert {(c.h, c.n_vec) for c in by["t12"]} == {(256, 1), (256, 19), (1024, 7), (2048, 3), (4096, 2)}
  assert [(c.h, c.n_vec) for c in by["t13"] + by["t14"]] == [(8192, 2), (16384, 2)]
  # what the shapes are for
  assert 1027 * 2 % H.R2_BLOCK == 6 and 6 % 4                      # h = 2: a scalar tail behind a full block
  assert 259 * 8 > H.R2_BLOCK and 19 * 128 > H.R2_BLOCK            # several blocks, the last one partial
  assert 1 * 256 < H.TILE and 19 * 256 > H.TILE and 19 * 256 % H.TILE and 7 * 1024 % H.TILE and 3 * 2048 % H.TILE
  assert {h for h in H.SIZES if H.is_power_of_four(h) and h > 1} <= {c.h for c in H.CASES}
  assert {s[0] for s in H.DELTA_SHAPES} == {8, 128, 256, 2048, 4096, 8192, 16384}
  assert {s for s in H.DELTA_SHAPES if s[2] != s[0]} == {(128, 3, 384), (2048, 3, 6144)}


@pytest.mark.parametrize("kind", H.DELTA_KINDS)
def test_delta_case_is_the_reference_minus_the_rotated_target(kind):
  h, rows, d = 128, 3, 384
  c = H.delta_case(kind, h, rows, d)
  assert c["w"].dtype == c["dq"].dtype == c["want"].dtype == F and c["w"].size == rows * d
  rot64 = H.fwht64(c["dq"], h).reshape(-1)
  err = np.abs(c["want"].astype(np.float64) - (c["w"].astype(np.float64) - rot64))
  tol = np.repeat(H.bound(c["dq"], h), h) + 2.0 ** -24 * np.abs(c["want"])
  assert (err <= tol).all()
  if kind == "i4":
    assert c["stored"].dtype == np.uint8 and c["stored"].size == rows * d // 2
    lo = ((c["stored"].astype(np.int32) & 15) ^ 8) - 8
    hi = (c["stored"].astype(np.int32) >> 4 ^ 8) - 8
    q4 = np.stack([lo, hi], axis=1).reshape(-1)
    assert q4.min() == -8 and q4.max() == 7
    in64 = (q4.astype(np.float64) * np.repeat(c["scale"], d).astype(np.float64)).astype(F)     # int32 * float32 in NumPy
    assert np.array_equal(in64, c["dq"])
  else:
    assert c["stored"].dtype == np.float16 and np.array_equal(c["stored"].astype(F), c["dq"])


# ------------------------------------------------------------------------------------------------ the Python layer
def _info(cfg):
  return q.OpInfo(op=q.OperatorT(), op_name=q.TFLOperationName.FULLY_CONNECTED, subgraph_op_index=0,
                  op_quant_config=q.OpQuantizationConfig(weight_tensor_config=cfg))


@pytest.mark.parametrize("shape,max_size", [((4, 7), None), ((2, 4, 9), None), ((4, 8), 1), ((6, 7), 64)])
def test_a_hadamard_size_of_one_is_refused_before_the_gpu(shape, max_size, monkeypatch):
  """An odd last dimension (or a cap of 1) leaves nothing to rotate: the reference fails in its matrix product
  (reshape(-1, 1) @ 2x2) and so does the oracle. Rotating the flattened tensor in pairs would mix rows."""
  from mi355q import ops
  from mi355q import runtime as rt

  def touched(*a, **k):
    raise AssertionError("the GPU was reached")
  monkeypatch.setattr(rt, "require_gpu", touched)
  monkeypatch.setattr(ops, "hadamard_rotate", touched)
  w = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
  axis = len(shape) - 1
  assert hadamard_rotation.hadamard_size_for(shape[-1], max_size) == 1
  with pytest.raises(ValueError, match="Hadamard size would be 1"):
    hadamard_rotation._rotate_with_diagonal_hadamard(w, axis, max_size)      # pylint: disable=protected-access
  with pytest.raises(ValueError, match="Hadamard size would be 1"):
    hadamard_rotation._rotate_in_hbm(w, axis, max_size)                      # pylint: disable=protected-access
  params = {"num_bits": 4, "granularity": q.QuantGranularity.CHANNELWISE}
  if max_size:
    params["max_hadamard_size"] = max_size
  cfg = q.TensorQuantizationConfig.from_dict(params)
  assert cfg.algorithm_params.get("max_hadamard_size") == max_size
  with pytest.raises(ValueError, match="Hadamard size would be 1"):
    hadamard_rotation.get_tensor_quant_params(_info(cfg), cfg, w)
  with pytest.raises(ValueError):
    O.hadamard_rotate(w, max_size)
  with pytest.raises(ValueError):
    O.hadamard_quant_params(w, 4, "CHANNELWISE", max_size=max_size)
