"""Model validation on the GPU: the five comparison metrics of csrc/validation.hip against NumPy, every stored
target form, the batched launch, and compare_model / Quantizer.validate end to end.

`_np_metrics` restates the reference's validation_utils in NumPy (ref: utils/validation_utils.py:63-255):
MSE, SNR and the median diff ratio must be bit-equal to it, the cosine within 4e-6, the KL divergence within
1e-5 * sum|terms| + 1e-30 (NumPy's SIMD log against the GPU's).
"""
import json
import os

import numpy as np
import pytest

from oracle import aeq_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")


@pytest.fixture(scope="module")
def v():
  import torch
  assert torch.cuda.is_available()
  import __graft_entry__ as g
  g.build()
  import types
  from mi355q import model_validator, ops, quantizer, recipe
  from mi355q.utils import validation_utils
  return types.SimpleNamespace(vu=validation_utils, mv=model_validator, ops=ops, quantizer=quantizer, recipe=recipe,
                               torch=torch)


def _prep(d1, d2):
  d1 = np.nan_to_num(np.ravel(np.asarray(d1, np.float32)), nan=1e-9, neginf=-1e9, posinf=1e9)
  d2 = np.nan_to_num(np.ravel(np.asarray(d2, np.float32)), nan=1e-9, neginf=-1e9, posinf=1e9)
  return d1, d2


def _np_metrics(d1, d2):
  """{name: (value, kl tolerance scale)} of target d1 against reference d2, as the reference computes them."""
  d1, d2 = _prep(d1, d2)
  if d1.size == 0:
    return {"mse": 0.0, "median_diff_ratio": 0.0, "cosine_similarity": 0.0, "kl_divergence": 0.0, "snr": 0.0}, 0.0
  mse = float(np.square(np.subtract(d1, d2)).mean())
  med = np.median(abs(d1 - d2) / (abs(d2) + 1e-6))
  n1, n2 = np.linalg.norm(d1), np.linalg.norm(d2)
  if n1 == 0 and n2 == 0:
    cos = 1.0
  elif n1 == 0 or n2 == 0:
    cos = 0.0
  else:
    cos = np.dot(d1, d2) / (n1 * n2)
  p, q = np.maximum(0, d2), np.maximum(0, d1)
  terms = p * np.log((p + 1e-9) / (q + 1e-9))
  kl = float(np.sum(terms))
  snr = float(np.square(d2).mean()) / (mse + 1e-9)
  return {"mse": mse, "median_diff_ratio": med, "cosine_similarity": cos, "kl_divergence": kl, "snr": snr}, \
      float(np.sum(np.abs(terms.astype(np.float64))))


def _check(got, want, kl_scale, cos_tol=4e-6):
  g = {k.value: val for k, val in got.items()}
  assert g["mse"] == want["mse"], (g["mse"], want["mse"])
  assert g["snr"] == want["snr"], (g["snr"], want["snr"])
  assert np.float32(g["median_diff_ratio"]) == np.float32(want["median_diff_ratio"]), \
      (g["median_diff_ratio"], want["median_diff_ratio"])
  assert abs(float(g["cosine_similarity"]) - float(want["cosine_similarity"])) <= cos_tol
  assert abs(g["kl_divergence"] - want["kl_divergence"]) <= 1e-5 * kl_scale + 1e-30


SIZES = [1, 2, 7, 8, 9, 127, 128, 129, 1000, 8191, 8192, 8193, 20000, 100003, (1 << 20) + 3]


def _pair(seed, n, corruption):
  rng = np.random.default_rng(seed)
  r = (rng.standard_normal(n) * rng.uniform(0.1, 10.0)).astype(np.float32)
  t = (r + rng.standard_normal(n).astype(np.float32) * np.float32(0.05)).astype(np.float32)
  if corruption == "nonfinite" and n >= 4:
    t[rng.integers(0, n, 3)] = [np.nan, np.inf, -np.inf]
    r[rng.integers(0, n, 3)] = [np.inf, np.nan, -np.inf]
  elif corruption == "zeros":
    t[:] = 0
    r[:] = 0
  elif corruption == "zero_target":
    t[:] = 0
  elif corruption == "negative":
    t, r = -np.abs(t), np.abs(r) - np.float32(1.0)
  elif corruption == "ties":
    t = np.round(t, 1).astype(np.float32)
    r = np.round(r, 1).astype(np.float32)
  return t, r


@pytest.mark.parametrize("n", SIZES)
def test_metrics_match_numpy(v, n):
  t, r = _pair(n, n, "noise")
  want, kls = _np_metrics(t, r)
  _check(v.vu.compare_all(v.torch.from_numpy(t).cuda(), v.torch.from_numpy(r).cuda()), want, kls)


@pytest.mark.parametrize("corruption", ["nonfinite", "zeros", "zero_target", "negative", "ties"])
@pytest.mark.parametrize("n", [8, 129, 8193, 65536])
def test_metrics_match_numpy_corrupted(v, corruption, n):
  t, r = _pair(1000 + n, n, corruption)
  want, kls = _np_metrics(t, r)
  _check(v.vu.compare_all(t, r), want, kls)


def test_large_tensor(v):
  t, r = _pair(7, 1 << 24, "noise")
  want, kls = _np_metrics(t, r)
  # at 2^24 elements NumPy's float32 sdot drifts from the float64 sums by 5.5e-6 in the cosine
  _check(v.vu.compare_all(t, r), want, kls, cos_tol=1e-5)


def test_empty_and_single_functions(v):
  vu = v.vu
  assert vu.mean_squared_difference(np.zeros(0), np.zeros(0)) == 0.0
  assert vu.median_diff_ratio([], []) == 0.0
  t, r = _pair(3, 1001, "noise")
  want, _ = _np_metrics(t, r)
  assert vu.mean_squared_difference(t, r) == want["mse"]
  assert type(vu.mean_squared_difference(t, r)) is float
  assert vu.signal_to_noise_ratio(t, r) == want["snr"]
  med = vu.median_diff_ratio(t, r)
  assert isinstance(med, np.float32) and med == want["median_diff_ratio"]
  assert isinstance(vu.cosine_similarity(t, r), np.float32)
  assert vu.cosine_similarity(np.zeros(5), np.zeros(5)) == 1.0
  assert vu.cosine_similarity(np.zeros(5), np.ones(5)) == 0.0
  with pytest.raises(ValueError, match="same size"):
    vu.mean_squared_difference(t, r[:-1])


def _uq(x, bits, axis=None, block=None, symmetric=True, seed=0):
  """int quantization of x in NumPy: (q, scale, zp) with the scale view of ops.CompareTarget."""
  qmax = 2 ** (bits - 1) - 1
  if block:
    rows, cols = x.shape
    xb = x.reshape(rows, cols // block, block)
    s = (np.max(np.abs(xb), axis=2) / qmax).astype(np.float32)
    s = s.astype(np.float16).astype(np.float32)
    s[s == 0] = 1
    q = np.clip(np.rint(xb / s[..., None]), -qmax - 1, qmax).astype(np.int8).reshape(rows, cols)
    return q, s.ravel(), np.zeros(s.size, np.int32)
  if axis is None:
    s = np.array([np.max(np.abs(x)) / qmax], np.float32)
  else:
    s = (np.max(np.abs(x), axis=tuple(i for i in range(x.ndim) if i != axis)) / qmax).astype(np.float32)
  rng = np.random.default_rng(seed)
  zp = np.zeros(s.size, np.int32) if symmetric else rng.integers(-3, 4, s.size).astype(np.int32)
  shape = [1] * x.ndim
  if axis is not None:
    shape[axis] = -1
  dt = {8: np.int8, 16: np.int16, 32: np.int32}[bits]
  q = np.clip(np.rint(x / s.reshape(shape)) + zp.reshape(shape), -qmax - 1, qmax).astype(dt)
  return q, s, zp


def _dequant_np(q, s, zp, axis, diff_dtype):
  """oracle.uniform_dequantize with the zero points in `diff_dtype` (int8 ones make q - zp wrap, as in NumPy)."""
  if axis is None:
    one = [1] * q.ndim
    return O.uniform_dequantize(q, s.reshape(one), zp.astype(diff_dtype).reshape(one))
  return O.uniform_dequantize(q, s, zp.astype(diff_dtype), quantized_dim=axis)


def _pack(q, bits):
  per = 8 // bits
  u = (q.ravel().astype(np.int32) & ((1 << bits) - 1)).astype(np.uint8)
  u = np.concatenate([u, np.zeros((-len(u)) % per, np.uint8)]).reshape(-1, per)
  out = np.zeros(len(u), np.uint8)
  for k in range(per):
    out |= (u[:, k] << (bits * k)).astype(np.uint8)
  return out


@pytest.mark.parametrize("form", ["i8_channel", "i8_channel_zp", "i8_wrap", "i16", "i32_bias", "i4_block128",
                                  "i4_channel", "i2_channel", "f16", "bf16"])
def test_target_forms(v, form):
  torch, ops = v.torch, v.ops
  rng = np.random.default_rng(sum(form.encode()))
  x = rng.standard_normal((96, 512)).astype(np.float32)
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  if form.startswith("i8") or form in ("i16", "i4_channel", "i2_channel"):
    bits = {"i16": 16, "i4_channel": 4, "i2_channel": 2}.get(form, 8)
    q, s, zp = _uq(x, max(bits, 8) if bits >= 8 else 8, axis=0, symmetric=form != "i8_channel_zp", seed=1)
    if bits < 8:
      qmax = 2 ** (bits - 1) - 1
      s = (np.max(np.abs(x), axis=1) / qmax).astype(np.float32)
      q = np.clip(np.rint(x / s[:, None]), -qmax - 1, qmax).astype(np.int8)
      zp = np.zeros(96, np.int32)
    diff_bits, diff_dtype = 32, np.int32
    if form == "i8_wrap":
      zp = rng.integers(-100, 100, 96).astype(np.int8)
      diff_bits, diff_dtype = 8, np.int8
    want_t = _dequant_np(q, s, zp, 0, diff_dtype)
    if bits < 8:
      tgt = ops.CompareTarget(dev(_pack(q, bits)), q.size, f"i{bits}", dev(s), dev(zp), 96, 512, diff_bits)
    else:
      tgt = ops.CompareTarget(dev(q), q.size, {8: "i8", 16: "i16"}[bits], dev(s), dev(zp.astype(np.int32)), 96, 512,
                              diff_bits)
  elif form == "i32_bias":
    b = (rng.standard_normal(4099) * 3).astype(np.float32)
    s = np.array([1.37e-5], np.float32)
    q = np.rint(b / s).astype(np.int32)
    x = b
    want_t = _dequant_np(q, s, np.zeros(1, np.int32), None, np.int32)
    tgt = ops.CompareTarget(dev(q), q.size, "i32", dev(s), dev(np.zeros(1, np.int32)), 1, 1, 32)
  elif form == "i4_block128":
    x4 = rng.standard_normal((64, 1024)).astype(np.float32)
    qmax = 7
    xb = x4.reshape(64, 8, 128)
    s = (np.max(np.abs(xb), axis=2) / qmax).astype(np.float16).astype(np.float32)
    q = np.clip(np.rint(xb / s[..., None]), -8, 7).astype(np.int8).reshape(64, 1024)
    x = x4
    want_t = (q.reshape(64, 8, 128).astype(np.int32) * s[..., None]).reshape(64, 1024)
    tgt = ops.CompareTarget(dev(_pack(q, 4)), q.size, "i4", dev(s.ravel()), None, s.size, 128, 32)
  elif form == "f16":
    h = x.astype(np.float16)
    want_t = h
    tgt = ops.CompareTarget(dev(h), h.size, "f16")
  else:
    tb = torch.from_numpy(x).to(torch.bfloat16)
    want_t = tb.to(torch.float32).numpy()
    tgt = ops.CompareTarget(tb.cuda(), x.size, "bf16")
  want, kls = _np_metrics(want_t, x)
  _check(v.vu.compare_all(tgt, x), want, kls)


def test_batched_equals_single(v):
  pairs = [_pair(50 + i, n, "noise") for i, n in enumerate([1, 5, 8, 129, 8192, 8193, 30001, 0, 77])]
  batched = v.vu.compare_all_batched(pairs)
  for (t, r), b in zip(pairs, batched):
    one = v.vu.compare_all(t, r)
    for k in one:
      assert (one[k] == b[k]) or (np.isnan(one[k]) and np.isnan(b[k])), (k, one[k], b[k])


# ----------------------------------------------------------------------------- compare_model end to end
# The expected constants are read from the flatbuffers here, independently of model_validator: the target tensor's own
# quantization record (scale / zeroPoint / quantizedDimension, or BlockwiseQuantization and its float16 scales tensor)
# goes through oracle.uniform_dequantize, with int32 zero points as the interpreter reports them.
def _tensors(model):
  from mi355q.utils import tfl_flatbuffer_utils as fu
  m = fu.read_model(model)
  return m, {t.name.decode() if isinstance(t.name, bytes) else t.name: t for t in m.subgraphs[0].tensors}


def _stored_values(m, t):
  from mi355q import schema
  raw = np.frombuffer(bytes(np.ravel(np.asarray(m.buffers[t.buffer].data)).view(np.uint8)), np.uint8)
  n = int(np.prod(t.shape)) if t.shape is not None else 1
  if t.type == schema.TensorType.INT4:
    lo, hi = (raw & 0xF).astype(np.int8), (raw >> 4).astype(np.int8)
    q = np.empty(raw.size * 2, np.int8)
    q[0::2], q[1::2] = lo, hi
    return np.where(q > 7, q - 16, q).astype(np.int8)[:n].reshape(t.shape)
  return raw.view(schema.NUMPY_DTYPE[schema.TensorType(t.type)])[:n].reshape(t.shape)


def _expected_constant(m, by_name, t):
  """(float32 target values as the reference's get_tensor_data sees them, largest scale or None)."""
  from mi355q import schema
  q = t.quantization
  vals = _stored_values(m, t)
  if t.type == schema.TensorType.FLOAT32 or q is None:
    return np.asarray(vals, np.float32), None
  details = getattr(q, "details", None)
  if details is not None and hasattr(details, "blockSize"):
    sc_t = m.subgraphs[0].tensors[int(details.scales)]
    scale = np.asarray(_stored_values(m, sc_t), np.float32)
    deq = O.uniform_dequantize(vals, scale, np.zeros(scale.shape, np.int32), quantized_dim=int(q.quantizedDimension),
                               block_size=int(details.blockSize))
    return np.asarray(deq, np.float32), float(scale.max())
  if q.scale is None or len(q.scale) == 0:
    return np.asarray(vals, np.float32), None
  scale = np.asarray(q.scale, np.float32)
  zp = np.asarray(q.zeroPoint if q.zeroPoint is not None and len(q.zeroPoint) else np.zeros(scale.size), np.int32)
  if scale.size == 1:
    one = [1] * vals.ndim
    deq = O.uniform_dequantize(vals, scale.reshape(one), zp.reshape(one))
  else:
    deq = O.uniform_dequantize(vals, scale, zp, quantized_dim=int(q.quantizedDimension))
  return np.asarray(deq, np.float32), float(scale.max())


def _expected_constants(ref_bytes, tgt_bytes):
  """{name: (target float values, reference float values, largest scale)} of the constants compare_model compares:
  reference tensors with data, at least one element, present by name (with data) in the target."""
  rm, rnames = _tensors(ref_bytes)
  tm, tnames = _tensors(tgt_bytes)
  out = {}
  for name, t in rnames.items():
    buf = rm.buffers[t.buffer].data
    if buf is None or len(buf) == 0 or name not in tnames:
      continue
    tt = tnames[name]
    if tm.buffers[tt.buffer].data is None or len(tm.buffers[tt.buffer].data) == 0:
      continue
    ref_vals = np.asarray(_stored_values(rm, t), np.float32)
    tgt_vals, smax = _expected_constant(tm, tnames, tt)
    out[name] = (tgt_vals, ref_vals, smax)
  return out


def _check_constants(v, got, ref_bytes, tgt_bytes, reps=1, mse_only=False):
  want = _expected_constants(ref_bytes, tgt_bytes)
  assert set(got) == set(want)
  quantized = 0
  for name, (t, r, smax) in want.items():
    m = {"mse": float(np.square(np.subtract(*_prep(t, r))).mean())} if mse_only else _np_metrics(t, r)[0]
    g = got[name]
    for k in ("mse", "snr", "median_diff_ratio"):
      if k in g:
        assert g[k] == float(np.mean([float(m[k])] * reps)), (name, k, g[k], m[k])
    if smax is not None:
      quantized += 1
      assert g["mse"] <= smax * smax / 4 * (1 + 1e-6), (name, g["mse"], smax)   # |error| <= scale / 2 per element
  return quantized


def _quantize(v, model_path, rec):
  qz = v.quantizer.Quantizer(model_path, rec)
  qz.quantize()
  return qz


RECIPES = {
    "dynamic_wi8_afp32": lambda v: v.recipe.dynamic_wi8_afp32(),
    "weight_only_wi4_afp32": lambda v: v.recipe.weight_only_wi4_afp32(),
    "dynamic_wi4b128_afp32": lambda v: v.recipe.dynamic_wi4b128_afp32(),
}
# the fixture models' weights are not divisible into blocks of 128: blockwise-128 runs on a 3-layer FC model
# of 384 x 640 weights (tools/file_bench.py builds it)
CASES = [(m, r) for m in ("single_fc_bias.tflite", "conv_fc_mnist.tflite") for r in RECIPES if "b128" not in r] + \
    [("fc3_384x640", "dynamic_wi4b128_afp32")]


def _model_path(model, tmp_path):
  if model.endswith(".tflite"):
    return os.path.join(MODELS, model)
  import sys
  sys.path.insert(0, os.path.join(ROOT, "tools"))
  import file_bench
  path = str(tmp_path / (model + ".tflite"))
  file_bench.build_model(path, 3, 384, 640)
  return path


@pytest.mark.parametrize("model,recipe_name", CASES)
def test_compare_model_constants(v, recipe_name, model, tmp_path):
  path = _model_path(model, tmp_path)
  qz = _quantize(v, path, RECIPES[recipe_name](v))
  metrics = list(v.vu.ValidationErrorMetric)
  res = qz.validate(error_metrics=metrics, save_folder=str(tmp_path), model_name="m")
  key = res.available_signature_keys()[0]
  sig = res.get_signature_comparison_result(key)
  ref_bytes, tgt_bytes = open(path, "rb").read(), bytes(qz._result.quantized_model)
  assert _check_constants(v, sig.constant_tensors, ref_bytes, tgt_bytes) >= 1
  if recipe_name == "dynamic_wi4b128_afp32":
    tm, tnames = _tensors(tgt_bytes)
    blockwise = [nm for nm, t in tnames.items() if t.quantization is not None
                 and hasattr(getattr(t.quantization, "details", None), "blockSize")]
    assert blockwise and set(blockwise) <= set(sig.constant_tensors)
  assert sig.input_tensors == {} and sig.output_tensors == {}
  assert os.path.exists(tmp_path / "m_comparison_result.json")
  for mt in metrics:
    assert os.path.exists(tmp_path / f"m_comparison_result_me_input_{mt.value}.json")


def test_test_data_without_a_runner_fills_the_constants(v):
  path = os.path.join(MODELS, "single_fc_bias.tflite")
  qz = _quantize(v, path, v.recipe.dynamic_wi8_afp32())
  key = v.mv.signature_keys(open(path, "rb").read())[0]
  res = qz.validate(test_data={key: [{}, {}]})
  sig = res.get_signature_comparison_result(key)
  assert sig.constant_tensors and not sig.output_tensors and not sig.input_tensors


def test_gemma_shaped_section_constants_in_one_call(v, monkeypatch):
  """A 2-layer Gemma-2B-shaped model (tools/c5_model.py, as test_gpu_c5_mixed.py builds it): its constants pass is one
  comparison call, and every MSE equals NumPy's on the CPU."""
  import sys
  import tempfile
  sys.path.insert(0, os.path.join(ROOT, "tools"))
  import c5_model as C
  from mi355q import model_modifier
  with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "gemma2.tflite")
    model_modifier.serialize_model(C.build_model(2), src)
    ref_bytes = open(src, "rb").read()
  qz = v.quantizer.Quantizer(ref_bytes, v.recipe.dynamic_wi4b128_afp32())
  tgt_bytes = bytes(qz.quantize().quantized_model)
  calls = []
  real = v.ops.compare
  monkeypatch.setattr(v.ops, "compare", lambda *a, **k: calls.append(1) or real(*a, **k))
  got = v.mv.compare_constants(ref_bytes, tgt_bytes, [v.vu.ValidationErrorMetric.MSE])
  assert len(calls) == 1 and len(got) >= 14
  got = {name: {mt.value: val for mt, val in d.items()} for name, d in got.items()}
  assert _check_constants(v, got, ref_bytes, tgt_bytes, mse_only=True) >= 14


def _fc_runner(model_bytes, signature_key, inputs):
  """A tiny NumPy interpreter for single_fc_bias: y = x W^T + b with the model's (dequantized) constants."""
  from mi355q import model_validator as mv
  from mi355q import schema
  from mi355q.utils import tfl_flatbuffer_utils as fu
  m = fu.read_model(model_bytes)
  sg = m.subgraphs[0]
  op = sg.operators[0]
  tens = sg.tensors
  x = np.asarray(next(iter(inputs.values())), np.float32)
  def const(i):
    return _expected_constant(m, None, tens[i])[0].reshape(tens[i].shape)
  w, b = const(op.inputs[1]), const(op.inputs[2])
  y = (x.reshape(-1, w.shape[1]) @ w.T + b).astype(np.float32)
  return {schema.tensor_name(tens[op.inputs[0]]): x, schema.tensor_name(tens[op.outputs[0]]): y}


def test_compare_model_with_runner(v):
  path = os.path.join(MODELS, "single_fc_bias.tflite")
  qz = _quantize(v, path, v.recipe.dynamic_wi8_afp32())
  ref_bytes = open(path, "rb").read()
  key = v.mv.signature_keys(ref_bytes)[0]
  in_name = v.mv.create_random_normal_input_data(ref_bytes, key)[0]
  shape = next(iter(in_name.values())).shape
  rng = np.random.default_rng(5)
  samples = [{k: rng.standard_normal(shape).astype(np.float32) for k in in_name} for _ in range(3)]
  metrics = [v.vu.ValidationErrorMetric.MSE, v.vu.ValidationErrorMetric.SNR]
  res = qz.validate(test_data={key: samples}, error_metrics=metrics, run_signature=_fc_runner)
  sig = res.get_signature_comparison_result(key)
  assert sig.output_tensors and sig.input_tensors and sig.constant_tensors
  out_name = next(iter(sig.output_tensors))
  tgt_bytes = bytes(qz._result.quantized_model)
  per = [_np_metrics(_fc_runner(tgt_bytes, key, s)[out_name], _fc_runner(ref_bytes, key, s)[out_name])[0]
         for s in samples]
  assert sig.output_tensors[out_name]["mse"] == float(np.mean([p["mse"] for p in per]))
  assert sig.output_tensors[out_name]["snr"] == float(np.mean([p["snr"] for p in per]))
  # outputs only
  res2 = qz.validate(test_data={key: samples}, validate_output_tensors_only=True, run_signature=_fc_runner)
  sig2 = res2.get_signature_comparison_result(key)
  assert set(sig2.output_tensors) == {out_name} and not sig2.constant_tensors and not sig2.input_tensors
  # no test data: one seeded random sample
  res3 = qz.validate(run_signature=_fc_runner)
  assert res3.get_signature_comparison_result(key).output_tensors


def test_fp16_model_constants(v):
  path = os.path.join(MODELS, "single_fc_bias.tflite")
  rm_recipe = [{"algorithm_key": "float_casting", "operation": "*", "regex": ".*",
                "op_config": {"compute_precision": "FLOAT", "explicit_dequantize": True, "min_weight_elements": 0,
                              "skip_checks": False,
                              "weight_tensor_config": {"dtype": "FLOAT", "granularity": "CHANNELWISE", "num_bits": 16,
                                                       "symmetric": True}}}]
  qz = _quantize(v, path, rm_recipe)
  res = qz.validate(error_metrics=list(v.vu.ValidationErrorMetric))
  key = res.available_signature_keys()[0]
  plans = v.mv.constant_plans(open(path, "rb").read(), bytes(qz._result.quantized_model), key)
  assert any(p.kind == "f16" and not p.dequantized for p in plans)
  got = res.get_signature_comparison_result(key).constant_tensors
  _check_constants(v, got, open(path, "rb").read(), bytes(qz._result.quantized_model))
