"""CPU checks of the layer output error (model_validator.compare_layer_outputs, Quantizer.validate_layer_outputs) with
a NumPy stand-in for the two kernels: how ops are matched by tensor names, every skip reason, shared weights, an
explicit-dequantize model, blockwise scales, float64 Hessians, the argument errors; and that csrc/layer_error.hip is
built and compiles for gfx950 without scratch."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import layer_error_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

D, DKV, DFF = 16, 8, 32


def _kernels():
  from mi355q import model_validator as mv

  class NumpyKernels(mv.LayerErrorKernels):
    """What csrc/layer_error.hip computes, in NumPy float64."""
    calls = []

    def weight(self, values):
      return np.asarray(values, np.float32)

    def delta(self, reference, plan):
      if plan.kind == "f32":
        return reference - np.asarray(plan.data, np.float32)
      q = np.asarray(plan.data)
      if plan.kind == "i4":
        b = q.view(np.uint8)
        q = np.stack([(b & 0xF), (b >> 4)], axis=1).ravel().astype(np.int8)
        q = np.where(q > 7, q - 16, q)[:reference.size]
      return reference - LC.dequantize(q, plan.scale, plan.zero_point, plan.channels, plan.inner, plan.diff_bits)

    def hessian(self, stat):
      form = stat.product_form() if hasattr(stat, "product_form") else None
      NumpyKernels.calls.append("product" if form is not None else "float64")
      return form if form is not None else (np.asarray(stat, np.float64).astype(np.float32), 1.0)

    def quadform(self, a, rows, d, product, alpha):
      return LC.exact_rows(np.asarray(a).reshape(rows, d), LC.symmetric(product), alpha)
  NumpyKernels.calls = []
  return NumpyKernels


def _float_and_target():
  import c5_model as C
  return C, C.build_model(1, d=D, dkv=DKV, dff=DFF), C.build_model(1, d=D, dkv=DKV, dff=DFF)


def _tensor(model, name):
  return next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)


def _weight(model, name):
  t = _tensor(model, name)
  return np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()


def _quantize_int8(model, name, zero_point=0):
  """Rewrites constant `name` of the tree as channelwise int8; returns its dequantized float32 values."""
  from mi355q import qtyping as q
  t = _tensor(model, name)
  w = _weight(model, name)
  scale = (np.abs(w).max(axis=1) / 100.0).astype(np.float32)
  ints = np.clip(np.rint(w / scale[:, None]) + zero_point, -128, 127).astype(np.int8)
  t.type = int(q.TensorType.INT8)
  t.quantization = q.QuantizationParametersT(scale=scale, zeroPoint=np.full(len(scale), zero_point, np.int64),
                                             quantizedDimension=0)
  model.buffers[t.buffer].data = ints.reshape(-1).view(np.uint8)
  zp = np.full(len(scale), zero_point, np.int32)
  return LC.dequantize(ints, scale, zp, w.shape[0], w.shape[1], 32).reshape(w.shape)


def _hessians(C, rng=None):
  rng = rng or np.random.default_rng(9)
  out = {}
  for _, _, cols, src in C.projections(D, DKV, DFF):
    if f"l0/{src}" not in out:
      x = rng.standard_normal((40, cols))
      out[f"l0/{src}"] = {"hessian": (2.0 / 4.0) * x.T @ x, "num_samples": np.array(4)}
  return out


def _want(w, deq, h):
  return LC.exact_rows(w, h, 0.5), LC.exact_rows(w - deq, h, 0.5)


def test_ops_are_matched_by_names_and_figures_follow_the_definition():
  from mi355q import model_validator as mv
  C, ref, tgt = _float_and_target()
  deq = {name: _quantize_int8(tgt, f"l0/{name}/w", zero_point=3 * i) for i, (name, *_) in enumerate(C.projections(D, DKV, DFF))}
  # (the quantized model may order its tensors and ops differently: matching is by name)
  tgt.subgraphs[0].operators.reverse()
  qsvs = _hessians(C)
  kernels = _kernels()
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=kernels())
  assert not got.skipped and len(got) == 7 and list(got) == [f"l0/{n}/y" for n, *_ in C.projections(D, DKV, DFF)]
  for name, rows, d, src in C.projections(D, DKV, DFF):
    r = got[f"l0/{name}/y"]
    w = _weight(ref, f"l0/{name}/w")
    signal, error = _want(w, deq[name], np.float32(qsvs[f"l0/{src}"]["hessian"]).astype(np.float64))
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
    np.testing.assert_allclose(r["per_channel_error"], error, rtol=1e-12)
    np.testing.assert_allclose([r["signal"], r["error"]], [signal.sum(), error.sum()], rtol=1e-12)
    assert r["error"] > 0 and r["output_mse"] == r["error"] / rows
    assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)
  assert kernels.calls == ["float64"] * 4           # one Hessian per distinct input: q / k / v and gate / up share


def test_every_skip_reason():
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  C, ref, tgt = _float_and_target()
  for name, *_ in C.projections(D, DKV, DFF):
    _quantize_int8(tgt, f"l0/{name}/w")
  qsvs = _hessians(C)
  # q: no Hessian for its input ... which k and v read too
  del qsvs["l0/attn_in"]
  # o: the Hessian has another order
  qsvs["l0/o_in"] = {"hessian": np.eye(D + 1), "num_samples": np.array(1)}
  # gate: the target constant is missing; up: it has another size
  _tensor(tgt, "l0/gate/w").name = b"l0/gate/renamed"
  _tensor(tgt, "l0/up/w").shape = [DFF, D // 2]
  # down: the quantized op reads a rotated activation
  sg = tgt.subgraphs[0]
  sg.tensors.append(q.TensorT(name=b"l0/down_in_rotated", shape=[1, DFF], buffer=0))
  down = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name == b"l0/down/y")
  down.inputs[0] = len(sg.tensors) - 1
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=_kernels()())
  assert not got.results
  assert got.skipped == {"l0/q/y": mv.SKIP_NO_HESSIAN, "l0/k/y": mv.SKIP_NO_HESSIAN, "l0/v/y": mv.SKIP_NO_HESSIAN,
                         "l0/o/y": mv.SKIP_ORDER, "l0/gate/y": mv.SKIP_TARGET, "l0/up/y": mv.SKIP_TARGET,
                         "l0/down/y": mv.SKIP_INPUT}
  # a weight that is no constant, or not 2-D, in the float model
  C, ref, tgt = _float_and_target()
  ref.buffers[_tensor(ref, "l0/q/w").buffer].data = None
  _tensor(ref, "l0/o/w").shape = [D, D // 2, 2]
  got = mv.compare_layer_outputs(ref, tgt, _hessians(C), kernels=_kernels()())
  assert got.skipped == {"l0/q/y": mv.SKIP_WEIGHT, "l0/o/y": mv.SKIP_WEIGHT} and len(got) == 5
  # no calibration result at all
  got = mv.compare_layer_outputs(ref, tgt, {}, kernels=_kernels()())
  assert not got.results and set(got.skipped.values()) == {mv.SKIP_WEIGHT, mv.SKIP_NO_HESSIAN}


def test_weight_shared_by_two_fully_connected_ops_gives_two_entries():
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  from mi355q.utils import tfl_flatbuffer_utils
  path = os.path.join(MODELS, "weight_sharing_fcs.tflite")
  ref, tgt = tfl_flatbuffer_utils.read_model(path), tfl_flatbuffer_utils.read_model(path)
  keys = mv.signature_keys(open(path, "rb").read())
  assert len(keys) == 2
  rng = np.random.default_rng(4)
  entries, buffers = {}, set()
  scale = ints = w = None
  for key in keys:
    sg_index, _ = mv._signature_subgraph(tgt, key)      # pylint: disable=protected-access
    (op, x_name, wt, y_name), = mv._fully_connected_ops(tgt, sg_index)      # pylint: disable=protected-access
    buffers.add(wt.buffer)
    if w is None:
      w = np.asarray(tgt.buffers[wt.buffer].data).view(np.float32).reshape(wt.shape).copy()
      scale = (np.abs(w).max(axis=1) / 7.0).astype(np.float32)
      ints = np.clip(np.rint(w / scale[:, None]), -8, 7).astype(np.int8)
      tgt.buffers[wt.buffer].data = ints.reshape(-1).view(np.uint8)
    wt.type = int(q.TensorType.INT8)
    wt.quantization = q.QuantizationParametersT(scale=scale, zeroPoint=np.zeros(len(scale), np.int64), quantizedDimension=0)
    x = rng.standard_normal((24, w.shape[1]))
    qsvs = {x_name: {"hessian": 0.5 * x.T @ x, "num_samples": np.array(4)}}
    got = mv.compare_layer_outputs(ref, tgt, qsvs, key, kernels=_kernels()())
    assert list(got) == [y_name] and not got.skipped and got[y_name]["input"] == x_name
    deq = LC.dequantize(ints, scale, None, w.shape[0], w.shape[1], 32).reshape(w.shape)
    _, error = _want(w, deq, np.float32(qsvs[x_name]["hessian"]).astype(np.float64))
    np.testing.assert_allclose(got[y_name]["per_channel_error"], error, rtol=1e-12)
    entries[(key, y_name)] = got[y_name]
  assert len(entries) == 2 and len(buffers) == 1
  assert len({(e["rows"], e["d"]) for e in entries.values()}) == 1


def test_weight_shared_by_two_ops_of_one_subgraph_is_uploaded_and_measured_once():
  """Two FULLY_CONNECTED ops of ONE subgraph read the same weight and the same input: two entries with the same
  figures, from one device copy of the weight and one signal."""
  from mi355q import model_validator as mv
  C, ref, tgt = _float_and_target()
  for model in (ref, tgt):
    sg = model.subgraphs[0]
    q_op = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name == b"l0/q/y")
    k_op = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name == b"l0/k/y")
    k_op.inputs[1] = q_op.inputs[1]
  _quantize_int8(tgt, "l0/q/w")
  counts = {"weight": 0, "quadform": 0}
  base = _kernels()

  class Counting(base):
    def weight(self, values):
      counts["weight"] += 1
      return super().weight(values)

    def quadform(self, *args):
      counts["quadform"] += 1
      return super().quadform(*args)
  qsvs = {"l0/attn_in": _hessians(C)["l0/attn_in"]}
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=Counting())
  assert sorted(got) == ["l0/k/y", "l0/q/y", "l0/v/y"] and len(got.skipped) == 4
  a, b = got["l0/q/y"], got["l0/k/y"]
  assert a["weight"] == b["weight"] == "l0/q/w" and a["error"] == b["error"] > 0 and a["signal"] == b["signal"]
  assert np.array_equal(a["per_channel_error"], b["per_channel_error"])
  assert counts == {"weight": 2, "quadform": 5}      # q's and v's weights; two signals and three errors


def test_explicit_dequantize_model_is_matched_through_the_constants_name():
  """Weight-only: the quantized constant keeps its name, a DEQUANTIZE op feeds the FULLY_CONNECTED op a new tensor."""
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  C, ref, tgt = _float_and_target()
  deq = _quantize_int8(tgt, "l0/o/w")
  sg = tgt.subgraphs[0]
  sg.tensors.append(q.TensorT(name=b"l0/o/w_dequant", shape=[D, D], buffer=0))
  tgt.operatorCodes.append(q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.DEQUANTIZE), deprecatedBuiltinCode=6))
  fc = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name == b"l0/o/y")
  weight_index = fc.inputs[1]
  fc.inputs[1] = len(sg.tensors) - 1
  sg.operators.insert(0, q.OperatorT(inputs=[weight_index], outputs=[len(sg.tensors) - 1], opcodeIndex=1))
  qsvs = _hessians(C)
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=_kernels()())
  assert not got.skipped and len(got) == 7
  w = _weight(ref, "l0/o/w")
  _, error = _want(w, deq, np.float32(qsvs["l0/o_in"]["hessian"]).astype(np.float64))
  np.testing.assert_allclose(got["l0/o/y"]["per_channel_error"], error, rtol=1e-12)
  assert got["l0/o/y"]["error"] > 0
  assert got["l0/q/y"]["error"] == 0.0 and got["l0/q/y"]["output_snr"] == (got["l0/q/y"]["signal"] / D) / 1e-9   # still float


def test_blockwise_int4_target_reads_its_scale_tensor():
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  C, ref, tgt = _float_and_target()
  block = 32
  t = _tensor(tgt, "l0/down/w")                     # [D, DFF]: one block per row
  w = _weight(tgt, "l0/down/w")
  scale = (np.abs(w.reshape(-1, block)).max(axis=1) / 7.0).astype(np.float16).astype(np.float32)
  ints = np.clip(np.rint(w.reshape(-1, block) / scale[:, None]), -8, 7).astype(np.int8).ravel()
  sg = tgt.subgraphs[0]
  tgt.buffers.append(q.BufferT(data=scale.astype(np.float16).view(np.uint8)))
  sg.tensors.append(q.TensorT(name=b"l0/down/w_scales", shape=[D, DFF // block], type=int(q.TensorType.FLOAT16),
                              buffer=len(tgt.buffers) - 1))
  t.type = int(q.TensorType.INT4)
  t.quantization = q.QuantizationParametersT(
      detailsType=2, details=q.BlockwiseQuantizationT(scales=len(sg.tensors) - 1, zeroPoints=-1, blockSize=block))
  tgt.buffers[t.buffer].data = LC.pack(ints, 4)
  qsvs = _hessians(C)
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=_kernels()())
  deq = LC.dequantize(ints, scale, None, w.size // block, block, 32).reshape(w.shape)
  _, error = _want(w, deq, np.float32(qsvs["l0/down_in"]["hessian"]).astype(np.float64))
  np.testing.assert_allclose(got["l0/down/y"]["per_channel_error"], error, rtol=1e-12)
  assert got["l0/down/y"]["error"] > 0


def test_product_form_is_used_when_the_statistic_has_one_and_float64_is_rounded_once():
  from mi355q import model_validator as mv
  C, ref, tgt = _float_and_target()
  _quantize_int8(tgt, "l0/o/w")
  x = np.random.default_rng(1).standard_normal((40, D)).astype(np.float32)
  low = np.tril(x.T @ x).astype(np.float32)

  class Accumulator:
    shape = (D, D)

    def product_form(self):
      return low, 2.0 / 4.0
  kernels = _kernels()
  a = mv.compare_layer_outputs(ref, tgt, {"l0/o_in": {"hessian": Accumulator()}}, kernels=kernels())
  b = mv.compare_layer_outputs(ref, tgt, {"l0/o_in": {"hessian": 0.5 * LC.symmetric(low)}}, kernels=kernels())
  assert kernels.calls == ["product", "float64"] and list(a) == list(b) == ["l0/o/y"]
  np.testing.assert_allclose(a["l0/o/y"]["per_channel_error"], b["l0/o/y"]["per_channel_error"], rtol=1e-12)
  # a non-finite Hessian gives non-finite figures, not an error
  c = mv.compare_layer_outputs(ref, tgt, {"l0/o_in": {"hessian": np.full((D, D), np.nan)}}, kernels=kernels())
  assert np.isnan(c["l0/o/y"]["error"]) and np.isnan(c["l0/o/y"]["output_snr"])


def test_save_leaves_the_per_channel_arrays_out(tmp_path):
  from mi355q import model_validator as mv
  C, ref, tgt = _float_and_target()
  _quantize_int8(tgt, "l0/o/w")
  qsvs = _hessians(C)
  del qsvs["l0/down_in"]
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=_kernels()())
  path = got.save(str(tmp_path / "out"), "m")
  assert path.endswith("m_layer_output_errors.json") and os.path.exists(path)
  saved = json.load(open(path))
  assert saved["skipped"] == {"l0/down/y": mv.SKIP_NO_HESSIAN} and len(saved["layers"]) == 6
  for y, entry in saved["layers"].items():
    assert sorted(entry) == ["d", "error", "input", "output_mse", "output_snr", "rows", "signal", "weight"]
    assert entry["error"] == got[y]["error"]


def test_validate_layer_outputs_arguments_and_route(monkeypatch):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  ref = open(os.path.join(MODELS, "single_fc_bias.tflite"), "rb").read()
  qz = quantizer.Quantizer(ref)
  with pytest.raises(ValueError, match="No quantized model available to validate"):
    qz.validate_layer_outputs(calibration_result={})
  qz._result = quantizer.QuantizationResult([{}], bytearray(ref))      # pylint: disable=protected-access
  with pytest.raises(ValueError, match="exactly one of calibration_result and calibration_data"):
    qz.validate_layer_outputs()
  with pytest.raises(ValueError, match="exactly one of calibration_result and calibration_data"):
    qz.validate_layer_outputs(calibration_result={}, calibration_data=[])
  with pytest.raises(ValueError, match="signature_key is required"):
    qz.validate_layer_outputs(calibration_data={"a": [], "b": []})
  with pytest.raises(ValueError, match="no samples for signature"):
    qz.validate_layer_outputs(calibration_data={"a": []}, signature_key="serving_default")
  # the whole route with the kernels replaced: a float "quantized" model has no error at all
  monkeypatch.setattr(mv, "LayerErrorKernels", _kernels())
  x = np.random.default_rng(2).standard_normal((12, 8))
  qsvs = {"serving_default_input_2:0": {"hessian": 0.5 * x.T @ x, "num_samples": np.array(4)}}
  got = qz.validate_layer_outputs(calibration_result=qsvs)
  assert list(got) == ["StatefulPartitionedCall:0"] and not got.skipped
  r = got["StatefulPartitionedCall:0"]
  assert (r["weight"], r["rows"], r["d"], r["error"]) == ("arith.constant", 4, 8, 0.0) and r["signal"] > 0


# ---------------------------------------------------------------- the kernels' build
def test_layer_error_is_built():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "layer_error.hip" in g.SOURCES


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_layer_error_kernels_use_no_scratch(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path / "layer_error.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "layer_error.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  names = " ".join(kernels)
  for k in ("weight_delta_kernel", "quadform_kernel", "quadform_sum_kernel"):
    assert k in names, k
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(kernels) == 3 and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
