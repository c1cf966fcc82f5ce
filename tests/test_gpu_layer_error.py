"""Layer output error on the GPU (csrc/layer_error.hip, ops.weight_delta / ops.quadform_rows,
model_validator.compare_layer_outputs, Quantizer.validate_layer_outputs).

  1. dW = W - dequant(W^) bit for bit against NumPy for every target kind and scale view;
  2. the quadratic form on integer data, where every accumulation order is exact: equal to the int64 result (a dropped
     tile, a wrong mask on the diagonal tile or a missing factor of 2 shows here);
  3. the same with NaN above the diagonal: the upper triangle is never read;
  4. float data against the float64 evaluation, inside the derived first-order bound 8 d u S_r, equal bits in two runs;
  5. a planted scale error is seen in its row only;
  6. end to end on a one-layer decoder-shaped model: GPTQ against min/max, the float64 evaluation from the written
     model's own integers, the calibration_data route, the Hadamard skip and save().
"""
import json
import os
import sys

import numpy as np
import pytest

import layer_error_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available()
  import __graft_entry__ as g
  g.build()
  from mi355q import ops

  class M:
    pass
  M.torch, M.ops = torch, ops
  M.dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
  return M


# ---------------------------------------------------------------- 1. delta
def _views(rows, d):
  """(label, channels, inner) scale views that fit [rows, d]."""
  out = [("channelwise", rows, d), ("tensorwise", 1, 1)]
  for block in (32, 128):
    if d % block == 0:
      out.append((f"blockwise{block}", rows * d // block, block))
  return out


def _delta_cases():
  cases = []
  for kind, shapes in (("i8", ((1, 8), (5, 96), (33, 128), (7, 200))), ("i4", ((1, 8), (5, 96), (33, 128))),
                       ("i2", ((1, 8), (5, 96), (33, 128))), ("i16", ((1, 8), (5, 96), (33, 128)))):
    for rows, d in shapes:
      for label, channels, inner in _views(rows, d):
        for diff_bits in ((8, 16, 32) if kind in ("i8", "i4", "i2") else (16, 32)):
          cases.append(pytest.param(kind, rows, d, channels, inner, diff_bits, id=f"{kind}-{rows}x{d}-{label}-diff{diff_bits}"))
  return cases


@pytest.mark.parametrize("kind,rows,d,channels,inner,diff_bits", _delta_cases())
def test_delta_integer_kinds_bit_for_bit(m, kind, rows, d, channels, inner, diff_bits):
  rng = np.random.default_rng(rows * 1000 + d + channels + diff_bits)
  bits = {"i8": 8, "i4": 4, "i2": 2, "i16": 16}[kind]
  lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
  q = rng.integers(lo, hi, size=rows * d, endpoint=True)
  scale = np.exp(rng.normal(size=channels)).astype(np.float32) * np.float32(0.01)
  zp_span = 3 if bits < 8 else 100
  zp = rng.integers(-zp_span, zp_span, size=channels, endpoint=True).astype(np.int32)
  ref = rng.standard_normal(rows * d).astype(np.float32)
  stored = LC.pack(q, bits) if bits < 8 else q.astype(np.int8 if bits == 8 else np.int16)
  want = ref - LC.dequantize(q, scale, zp, channels, inner, diff_bits)
  target = m.ops.CompareTarget(m.dev(stored), rows * d, kind, m.dev(scale), m.dev(zp), channels, inner, diff_bits)
  got = m.ops.weight_delta(m.dev(ref), target).cpu().numpy()
  assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("rows,d", [(1, 8), (5, 96), (33, 128)])
def test_delta_float_kinds_bit_for_bit(m, kind, rows, d):
  torch = m.torch
  rng = np.random.default_rng(rows + d)
  ref = rng.standard_normal(rows * d).astype(np.float32)
  t32 = rng.standard_normal(rows * d).astype(np.float32)
  dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]
  stored = torch.from_numpy(t32).cuda().to(dtype)
  want = ref - stored.to(torch.float32).cpu().numpy()          # widening to float32 is exact
  got = m.ops.weight_delta(m.dev(ref), m.ops.CompareTarget(stored, rows * d, kind)).cpu().numpy()
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_delta_passes_non_finite_values_through(m):
  rng = np.random.default_rng(3)
  rows, d = 5, 96
  ref = rng.standard_normal(rows * d).astype(np.float32)
  ref[[0, 7, 100, 479]] = [np.inf, -np.inf, np.nan, np.inf]
  q = rng.integers(-128, 127, size=rows * d, endpoint=True).astype(np.int8)
  scale = (np.abs(rng.standard_normal(rows)) + 0.1).astype(np.float32)
  want = ref - LC.dequantize(q, scale, None, rows, d, 32)
  got = m.ops.weight_delta(m.dev(ref), m.ops.CompareTarget(m.dev(q), rows * d, "i8", m.dev(scale), None, rows, d, 32)).cpu().numpy()
  nan = np.isnan(want)
  assert nan.sum() == 1 and np.array_equal(np.isnan(got), nan)      # no nan_to_num: NaN stays NaN, inf stays inf
  assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
  assert np.isposinf(got[0]) and np.isneginf(got[7]) and np.isposinf(got[479])


# ---------------------------------------------------------------- 2. / 3. exact quadratic form
ROWS = (1, 5, 33, 65, 130)


def _integer_case(d):
  rng = np.random.default_rng(7000 + d)
  low = np.tril(rng.integers(-7, 7, size=(d, d), endpoint=True))
  psym = low + np.tril(low, -1).T
  a = rng.integers(-3, 3, size=(max(ROWS), d), endpoint=True)
  want = ((a @ psym) * a).sum(axis=1)               # int64, below d^2 * 63 <= 9.3 M < 2^24
  assert np.abs(want).max() < 1 << 24
  return a.astype(np.float32), psym.astype(np.float32), 0.5 * want.astype(np.float64)


@pytest.mark.parametrize("d", [1, 8, 33, 64, 96, 200, 256, 384])
def test_quadform_is_exact_on_integer_data(m, d):
  a, psym, want = _integer_case(d)
  p_dev = m.dev(psym)
  for rows in ROWS:
    got = m.ops.quadform_rows(m.dev(a[:rows]), p_dev, 0.5).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want[:rows]), (d, rows)


@pytest.mark.parametrize("d", [1, 8, 33, 64, 96, 200, 256, 384])
def test_quadform_never_reads_the_upper_triangle(m, d):
  a, psym, want = _integer_case(d)
  psym[np.triu_indices(d, 1)] = np.nan
  p_dev = m.dev(psym)
  before = p_dev.clone()
  for rows in ROWS:
    got = m.ops.quadform_rows(m.dev(a[:rows]), p_dev, 0.5).cpu().numpy()
    assert np.array_equal(got, want[:rows]), (d, rows)
  assert m.torch.equal(p_dev.view(m.torch.int32), before.view(m.torch.int32))      # nothing of product is written


# ---------------------------------------------------------------- 4. float data
@pytest.mark.parametrize("d", [64, 200, 256, 384])
def test_quadform_float_data_within_the_derived_bound(m, d):
  low = LC.product_of(d, 40 + d)
  psym = LC.symmetric(low)
  alpha = 0.5 * 2.0 / 4.0
  p_dev = m.dev(low)
  worst = 0.0
  for rows in (5, 33, 130):
    a = (np.random.default_rng(d + rows).standard_normal((rows, d)) * 0.02).astype(np.float32)
    exact, gate = LC.exact_rows(a, psym, alpha), LC.gate_rows(a, psym, alpha)
    a_dev = m.dev(a)
    got = m.ops.quadform_rows(a_dev, p_dev, alpha).cpu().numpy()
    again = m.ops.quadform_rows(a_dev, p_dev, alpha).cpu().numpy()
    frac = float(np.max(np.abs(got - exact) / gate))
    worst = max(worst, frac)
    print(f"quadform d={d} rows={rows}: worst |gpu - exact| / gate = {frac:.3e}")
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    assert np.all(np.abs(got - exact) <= gate), (d, rows, frac)
  print(f"quadform d={d}: worst fraction of the gate {worst:.3e}")


# ---------------------------------------------------------------- 5. planted error
def test_planted_scale_error_shows_in_its_row_only(m):
  rows, d, block = 9, 128, 32
  rng = np.random.default_rng(55)
  w = (rng.standard_normal((rows, d)) * 0.02).astype(np.float32)
  scale = (np.abs(w.reshape(-1, block)).max(axis=1) / 7.0).astype(np.float32)
  q = np.clip(np.rint(w.reshape(-1, block) / scale[:, None]), -8, 7).astype(np.int8).ravel()
  low = LC.product_of(d, 77)
  psym, alpha = LC.symmetric(low), 0.5 * 2.0 / 4.0
  planted_row, planted_block = 4, 2
  bad = scale.copy()
  bad[planted_row * (d // block) + planted_block] *= np.float32(2.0)
  deltas = [w.ravel() - LC.dequantize(q, s, None, rows * d // block, block, 32) for s in (scale, bad)]
  exact = [LC.exact_rows(dl.reshape(rows, d), psym, alpha) for dl in deltas]
  gate = np.maximum(*[LC.gate_rows(dl.reshape(rows, d), psym, alpha) for dl in deltas])
  assert abs(exact[1][planted_row] - exact[0][planted_row]) > 10 * gate[planted_row]      # float64 first
  got = []
  for s in (scale, bad):
    target = m.ops.CompareTarget(m.dev(LC.pack(q, 4)), rows * d, "i4", m.dev(s), None, rows * d // block, block, 32)
    delta = m.ops.weight_delta(m.dev(w), target)
    got.append(m.ops.quadform_rows(delta.view(rows, d), m.dev(low), alpha).cpu().numpy())
  others = np.arange(rows) != planted_row
  assert np.array_equal(got[0][others].view(np.uint64), got[1][others].view(np.uint64))
  assert abs(got[1][planted_row] - got[0][planted_row]) > 8 * gate[planted_row]


# ---------------------------------------------------------------- 6. end to end
D, DKV, DFF = 128, 32, 256


def _fc_recipe(C, key):
  return [C._fc(key, bits=4)]      # pylint: disable=protected-access


@pytest.fixture(scope="module")
def chain(m, tmp_path_factory):
  import c5_model as C
  from mi355q import algorithm_manager, quantizer
  from mi355q.utils import tfl_flatbuffer_utils
  projections = C.projections(D, DKV, DFF)
  model = C.build_model(1, d=D, dkv=DKV, dff=DFF)
  weights = {}
  for t in model.subgraphs[0].tensors:
    name = t.name.decode()
    if name.endswith("/w"):
      weights[name] = np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()
  samples = LC.calibration_samples(projections)
  out = dict(C=C, projections=projections, weights=weights, samples=samples)
  recipes = {"gptq": C.recipe("gptq"), "minmax": _fc_recipe(C, algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT.value),
             "mixed": C.recipe("mixed")}
  qsvs = None
  for key, rcp in recipes.items():
    qz = quantizer.Quantizer(model, rcp)
    calib = qz.calibrate({"serving_default": samples}) if qz.need_calibration else {}
    if key == "gptq":
      qsvs = calib
    res = qz.quantize(calib)
    out[key] = dict(qz=qz, model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)))
  out["qsvs"] = qsvs
  out["gptq"]["cmp"] = out["gptq"]["qz"].validate_layer_outputs(calibration_result=qsvs)
  out["minmax"]["cmp"] = out["minmax"]["qz"].validate_layer_outputs(calibration_result=qsvs)
  out["save_dir"] = str(tmp_path_factory.mktemp("layer_errors"))
  return out


def _unpack_int4(packed, n):
  b = np.asarray(packed, dtype=np.uint8)
  out = np.empty(b.size * 2, np.int8)
  out[0::2], out[1::2] = (b & 0xF).astype(np.int8), (b >> 4).astype(np.int8)
  return np.where(out > 7, out - 16, out).astype(np.int8)[:n]


def _float64_evaluation(chain, key, name, src):
  """(signal, error, gate of the signal, gate of the error) from the Hessian read back and the written integers."""
  w = chain["weights"][f"l0/{name}/w"]
  rows, d = w.shape
  qm = chain[key]["model"]
  t = next(t for t in qm.subgraphs[0].tensors if t.name.decode() == f"l0/{name}/w")
  q = _unpack_int4(np.asarray(qm.buffers[t.buffer].data), rows * d)
  scale = np.asarray(t.quantization.scale, np.float32)
  delta = (w.ravel() - LC.dequantize(q, scale, None, rows, d, 32)).reshape(rows, d)
  h = np.asarray(chain["qsvs"][f"l0/{src}"]["hessian"])
  assert h.dtype == np.float64 and h.shape == (d, d)
  return (LC.exact_rows(w, h, 0.5).sum(), LC.exact_rows(delta, h, 0.5).sum(),
          LC.gate_rows(w, h, 0.5).sum(), LC.gate_rows(delta, h, 0.5).sum())


def test_gptq_halves_the_output_error_of_min_max_on_every_projection(chain):
  g, n = chain["gptq"]["cmp"], chain["minmax"]["cmp"]
  assert not g.skipped and not n.skipped
  for name, rows, d, src in chain["projections"]:
    y = f"l0/{name}/y"
    assert g[y]["weight"] == f"l0/{name}/w" and g[y]["input"] == f"l0/{src}" and (g[y]["rows"], g[y]["d"]) == (rows, d)
    print(f"{y}: GPTQ error {g[y]['error']:.6e}, min/max error {n[y]['error']:.6e}, ratio {g[y]['error'] / n[y]['error']:.3f},"
          f" SNR {g[y]['output_snr']:.1f} against {n[y]['output_snr']:.1f}")
    assert g[y]["error"] < 0.5 * n[y]["error"], y
    assert g[y]["signal"] == n[y]["signal"]


@pytest.mark.parametrize("key", ["gptq", "minmax"])
def test_reported_figures_match_the_float64_evaluation(chain, key):
  cmp_ = chain[key]["cmp"]
  for name, rows, d, src in chain["projections"]:
    r = cmp_[f"l0/{name}/y"]
    signal, error, gate_s, gate_e = _float64_evaluation(chain, key, name, src)
    print(f"{key} l0/{name}: |signal - exact| / gate {abs(r['signal'] - signal) / gate_s:.3e},"
          f" |error - exact| / gate {abs(r['error'] - error) / gate_e:.3e}")
    assert abs(r["signal"] - signal) <= gate_s and abs(r["error"] - error) <= gate_e
    assert r["per_channel_error"].dtype == np.float64 and r["per_channel_error"].shape == (rows,)
    assert r["error"] == float(np.sum(r["per_channel_error"]))
    assert r["output_mse"] == r["error"] / rows
    assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)


def test_calibration_data_route_gives_the_same_figures(chain):
  qz = chain["minmax"]["qz"]
  got = qz.validate_layer_outputs(calibration_data={"serving_default": chain["samples"]})
  assert not got.skipped and len(got) == 7
  for name, rows, d, src in chain["projections"]:
    r, b = got[f"l0/{name}/y"], chain["minmax"]["cmp"][f"l0/{name}/y"]
    signal, error, gate_s, gate_e = _float64_evaluation(chain, "minmax", name, src)
    assert abs(r["signal"] - signal) <= gate_s and abs(r["error"] - error) <= gate_e
    # the same numbers as from the calibration result: the same accumulators over the same tokens, so the Hessians
    # differ by float32 summation order at the most (a wrong num_samples or alpha would be a factor, not 1e-6)
    print(f"l0/{name}: calibration_data against calibration_result, relative: signal"
          f" {abs(r['signal'] - b['signal']) / b['signal']:.3e}, error {abs(r['error'] - b['error']) / b['error']:.3e}")
    np.testing.assert_allclose([r["signal"], r["error"]], [b["signal"], b["error"]], rtol=1e-6)


def test_hadamard_rotated_projection_is_reported_as_skipped(chain):
  from mi355q import model_validator as mv
  got = chain["mixed"]["qz"].validate_layer_outputs(calibration_result=chain["qsvs"])
  assert got.skipped == {"l0/down/y": mv.SKIP_INPUT}
  assert sorted(got.results) == sorted(f"l0/{name}/y" for name, *_ in chain["projections"] if name != "down")


def test_save_writes_every_key(chain):
  cmp_ = chain["gptq"]["qz"].validate_layer_outputs(calibration_result=chain["qsvs"], save_folder=chain["save_dir"],
                                                    model_name="one_layer")
  with open(os.path.join(chain["save_dir"], "one_layer_layer_output_errors.json")) as fh:
    saved = json.load(fh)
  assert saved["skipped"] == {} and len(saved["layers"]) == 7
  for y, entry in saved["layers"].items():
    assert sorted(entry) == ["d", "error", "input", "output_mse", "output_snr", "rows", "signal", "weight"]
    for k, v in entry.items():
      assert v == cmp_[y][k]
