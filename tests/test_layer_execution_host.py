"""CPU checks of the integer execution comparison (model_validator.compare_layer_execution,
Quantizer.validate_layer_execution) with the NumPy stand-in of tests/layer_execution_cases.py for the kernels, on the
small models the layer-error host tests build: mode detection, every skip reason, the transform route, how samples are
added, the saved JSON, the argument errors; that the new entry points are declared, exported and refuse bad arguments;
and that csrc/qfc.hip compiles for gfx950 without scratch onto the int8 matrix cores."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import layer_error_cases as LC
import layer_execution_cases as EC
import test_layer_error_host as H
import test_layer_error_transforms_host as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("mi355q_qfc_quantize_rows_f32", "mi355q_qfc_forward_workspace_bytes", "mi355q_qfc_forward_i8",
               "mi355q_sqdiff_cols_workspace_bytes", "mi355q_sqdiff_cols_f64")
D, DKV, DFF = H.D, H.DKV, H.DFF


# ---------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
  from mi355q import _ffi
  header = open(os.path.join(ROOT, "include", "mi355q.h")).read()
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  for name in NEW_SYMBOLS:
    assert re.search(r"\b%s\s*\(" % name, header), name
    assert name in _ffi.PROTOTYPES and hasattr(lib, name), name
  assert len(_ffi.PROTOTYPES["mi355q_qfc_forward_i8"][1]) == 17
  assert len(_ffi.PROTOTYPES["mi355q_sqdiff_cols_f64"][1]) == 10


def test_refusals_come_before_any_launch(lib):
  EC.check_forward_refusals(lib)
  err = lib.mi355q_last_error
  assert lib.mi355q_qfc_quantize_rows_f32(None, 0, 64, None, None, None) == 0
  assert lib.mi355q_qfc_quantize_rows_f32(None, 4, 0, None, None, None) == 0
  assert lib.mi355q_qfc_quantize_rows_f32(None, 4, 64, None, None, None) == -1 and b"null pointer" in err()
  assert lib.mi355q_qfc_quantize_rows_f32(None, -4, 64, None, None, None) == -1 and b"negative shape" in err()
  assert lib.mi355q_sqdiff_cols_f64(None, None, 4, 0, None, None, 0, None, 0, None) == 0
  assert lib.mi355q_sqdiff_cols_f64(None, None, 4, 8, None, None, 0, None, 0, None) == -1 and b"null pointer" in err()
  assert lib.mi355q_sqdiff_cols_f64(None, None, -1, 8, None, None, 0, None, 0, None) == -1 and b"negative shape" in err()
  assert lib.mi355q_sqdiff_cols_workspace_bytes(1000, 130) == 2 * 16 * 130 * 8 + (-(2 * 16 * 130 * 8)) % 256
  assert lib.mi355q_sqdiff_cols_workspace_bytes(0, 130) == 0


# ---------------------------------------------------------------- the NumPy statement itself
def test_numpy_rounding_is_half_away_from_zero_and_exact():
  x = np.array([[127.0, 0.5, -0.5, 1.5, -1.5, 126.5, -126.5, 0.49999997, -0.49999997, -0.0, 2.5]], np.float32)
  q, s = EC.quantize_rows(x)
  assert s.tolist() == [1.0] and q[0].tolist() == [127, 1, -1, 2, -2, 127, -127, 0, 0, 0, 3]
  q, s = EC.quantize_rows(np.array([[0.0, -0.0], [1.0, np.nan], [np.inf, 2.0], [0.25, -0.5]], np.float32))
  assert s[0] == 1.0 and np.isnan(s[1]) and np.isnan(s[2]) and s[3] == np.float32(0.5) / np.float32(127.0)
  assert q.tolist() == [[0, 0], [0, 0], [0, 0], [64, -127]]      # 0.25 * 254 = 63.5 -> 64
  # the accumulator and both rescales
  xq = np.array([[-128, 127, 5, 0]], np.int8)
  qw = np.array([[7, -8, 3, 1], [-1, 0, 2, -8]])
  acc, y = EC.forward(xq, np.float32(0.3), -128, qw, np.array([0.1, 0.7], np.float32))
  assert acc.tolist() == [[0 * 7 + 255 * -8 + 133 * 3 + 128, 0 + 0 + 133 * 2 + 128 * -8]]
  want = np.float32(acc[0]) * (np.float32(0.3) * np.array([0.1, 0.7], np.float32))
  assert np.array_equal(y[0], want)
  packed = LC.pack(qw.ravel(), 4)
  assert np.array_equal(EC.unpack(packed, "i4", 8).reshape(2, 4), qw)
  assert np.array_equal(EC.unpack(LC.pack(np.array([1, -2, -1, 0, 1]).repeat(4)[:20], 2), "i2", 20),
                        np.array([1, -2, -1, 0, 1]).repeat(4))


# ---------------------------------------------------------------- compare_layer_execution
def _samples(C, count=2, length=24, seed=3):
  rng = np.random.default_rng(seed)
  widths = {}
  for _, _, cols, src in C.projections(D, DKV, DFF):
    widths[f"l0/{src}"] = cols
  return [{name: (rng.standard_normal((1, length + 3 * k, cols)) * (1.0 + k)).astype(np.float32)
           for name, cols in widths.items()} for k in range(count)]


def _add_quantize(model, x_name, consumers, scale, zero_point, ttype=None):
  """x -> QUANTIZE -> `<x>_quantized` (INT8 unless `ttype`) for the FULLY_CONNECTED ops named `consumers`."""
  from mi355q import qtyping as q
  sg = model.subgraphs[0]
  src = TH._tensor_id(model, x_name)      # pylint: disable=protected-access
  sg.tensors.append(q.TensorT(name=x_name.encode() + b"_quantized", shape=list(sg.tensors[src].shape), buffer=0,
                              type=int(ttype if ttype is not None else q.TensorType.INT8),
                              quantization=q.QuantizationParametersT(scale=np.array([scale], np.float32),
                                                                     zeroPoint=np.array([zero_point], np.int64))))
  new = len(sg.tensors) - 1
  model.operatorCodes.append(q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.QUANTIZE), deprecatedBuiltinCode=114))
  for name in consumers:
    fc = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"l0/{name}/y")
    fc.inputs[0] = new
  sg.operators.insert(0, q.OperatorT(inputs=[src], outputs=[new], opcodeIndex=len(model.operatorCodes) - 1))


def _add_dequantize(model, name):
  """The FULLY_CONNECTED op `name` reads `<w>_dequant`, a DEQUANTIZE of its integer weight."""
  from mi355q import qtyping as q
  sg = model.subgraphs[0]
  fc = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"l0/{name}/y")
  wid = fc.inputs[1]
  sg.tensors.append(q.TensorT(name=f"l0/{name}/w_dequant".encode(), shape=list(sg.tensors[wid].shape), buffer=0))
  model.operatorCodes.append(q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.DEQUANTIZE), deprecatedBuiltinCode=6))
  fc.inputs[1] = len(sg.tensors) - 1
  sg.operators.insert(0, q.OperatorT(inputs=[wid], outputs=[len(sg.tensors) - 1], opcodeIndex=len(model.operatorCodes) - 1))


def _mixed_modes():
  """q / k / v static (one QUANTIZE of attn_in), o weight-only, gate / up / down dynamic. Returns the integer weights'
  dequantized values as well."""
  C, ref, tgt = H._float_and_target()      # pylint: disable=protected-access
  deq = {name: H._quantize_int8(tgt, f"l0/{name}/w") for name, *_ in C.projections(D, DKV, DFF)}      # pylint: disable=protected-access
  _add_quantize(tgt, "l0/attn_in", ["q", "k", "v"], 0.05, -3)
  _add_dequantize(tgt, "o")
  return C, ref, tgt, deq


def _reference(ref, tgt, samples, name, src, mode, x_quant=None, transform=None):
  """(signal, error, per-channel error) of one op, written out here from the helper's arithmetic."""
  w = H._weight(ref, f"l0/{name}/w")      # pylint: disable=protected-access
  rows, d = w.shape
  t = H._tensor(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
  qw = np.asarray(tgt.buffers[t.buffer].data).view(np.int8).reshape(rows, d)
  scale = np.asarray(t.quantization.scale, np.float32)
  sq_d, sq_b, tokens = np.zeros(rows), np.zeros(rows), 0
  for s in samples:
    x = s[f"l0/{src}"].reshape(-1, d)
    xt = x if transform is None else transform(x)
    y = (x @ w.T).astype(np.float64)
    if mode == "dynamic":
      xq, xs = EC.quantize_rows(xt)
      yq = EC.forward(xq, xs, 0, qw, scale)[1]
    elif mode == "static":
      yq = EC.forward(EC.quantize_static(xt, *x_quant), np.float32(x_quant[0]), x_quant[1], qw, scale)[1]
    else:
      yq = xt @ LC.dequantize(qw, scale, None, rows, d, 32).reshape(rows, d).T
    sq_d += ((yq.astype(np.float64) - y) ** 2).sum(axis=0)
    sq_b += (y ** 2).sum(axis=0)
    tokens += x.shape[0]
  return sq_b.sum() / tokens, sq_d.sum() / tokens, sq_d / tokens, tokens


def test_modes_are_read_from_the_graph_and_figures_follow_the_definition():
  from mi355q import model_validator as mv
  C, ref, tgt, _ = _mixed_modes()
  tgt.subgraphs[0].operators.reverse()      # (matching is by names, not by order)
  samples = _samples(C)
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()())
  assert isinstance(got, mv.LayerExecutionComparison) and not got.skipped
  assert list(got) == [f"l0/{n}/y" for n, *_ in C.projections(D, DKV, DFF)]
  modes = {"q": "static", "k": "static", "v": "static", "o": "weight_only", "gate": "dynamic", "up": "dynamic", "down": "dynamic"}
  for name, rows, d, src in C.projections(D, DKV, DFF):
    r = got[f"l0/{name}/y"]
    signal, error, per_channel, tokens = _reference(ref, tgt, samples, name, src, modes[name], (0.05, -3))
    assert (r["weight"], r["input"], r["rows"], r["d"], r["mode"]) == (f"l0/{name}/w", f"l0/{src}", rows, d, modes[name])
    assert r["tokens"] == tokens == 24 + 27 and "input_transform" not in r
    np.testing.assert_allclose(r["per_channel_error"], per_channel, rtol=1e-12)
    np.testing.assert_allclose([r["signal"], r["error"]], [signal, error], rtol=1e-12)
    assert r["error"] > 0 and r["output_mse"] == r["error"] / rows
    assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)
  # the static ops carry the activations' rounding: far more error than the weight alone leaves
  weight_only = _reference(ref, tgt, samples, "q", "attn_in", "weight_only")[1]
  assert got["l0/q/y"]["error"] > 2.0 * weight_only


def test_two_samples_give_the_sum_of_each_divided_by_the_total_tokens():
  from mi355q import model_validator as mv
  C, ref, tgt, _ = _mixed_modes()
  samples = _samples(C)
  kernels = EC.numpy_kernels()
  both = mv.compare_layer_execution(ref, tgt, samples, kernels=kernels())
  first = mv.compare_layer_execution(ref, tgt, samples[:1], kernels=kernels())
  second = mv.compare_layer_execution(ref, tgt, samples[1:], kernels=kernels())
  for y, r in both.results.items():
    a, b = first[y], second[y]
    assert (a["tokens"], b["tokens"], r["tokens"]) == (24, 27, 51)
    np.testing.assert_allclose(r["error"], (a["error"] * 24 + b["error"] * 27) / 51, rtol=1e-12)
    np.testing.assert_allclose(r["signal"], (a["signal"] * 24 + b["signal"] * 27) / 51, rtol=1e-12)
    np.testing.assert_allclose(r["per_channel_error"], (a["per_channel_error"] * 24 + b["per_channel_error"] * 27) / 51,
                               rtol=1e-12)


def test_samples_are_walked_in_chunks_of_at_most_4096_rows(monkeypatch):
  from mi355q import model_validator as mv
  C, ref, tgt, _ = _mixed_modes()
  samples = _samples(C, count=1, length=24)
  whole = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()())
  seen = []
  base = EC.numpy_kernels()

  class Counting(base):
    def gemm(self, x, w):
      seen.append(x.shape[0])
      return super().gemm(x, w)
  monkeypatch.setattr(mv, "EXECUTION_CHUNK_ROWS", 10)
  chunked = mv.compare_layer_execution(ref, tgt, samples, kernels=Counting())
  assert max(seen) == 10 and set(seen) == {10, 4}
  for y, r in whole.results.items():
    np.testing.assert_allclose(chunked[y]["per_channel_error"], r["per_channel_error"], rtol=1e-12)
    assert chunked[y]["tokens"] == r["tokens"] == 24
  assert mv.EXECUTION_CHUNK_ROWS == 10
  monkeypatch.undo()
  assert mv.EXECUTION_CHUNK_ROWS == 4096


def test_every_skip_reason():
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  C, ref, tgt = H._float_and_target()      # pylint: disable=protected-access
  for name in ("q", "k", "o", "gate", "down"):
    H._quantize_int8(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
  H._quantize_int8(tgt, "l0/v/w", zero_point=3)      # v: a weight zero point      # pylint: disable=protected-access
  # up: the target weight is still float. q / k / v read an INT16 activation ... v's zero point is met first? no: INT16 first
  _add_quantize(tgt, "l0/attn_in", ["q", "k"], 0.001, 0, ttype=q.TensorType.INT16)
  # down: behind an inserted multiply, not followed
  TH._insert(tgt, "multiply", "l0/down_in", ["down"], multiplier=np.full(DFF, 0.5, np.float32))      # pylint: disable=protected-access
  samples = _samples(C)
  for s in samples:
    del s["l0/o_in"]      # o: no sample
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()())
  assert got.skipped == {"l0/q/y": mv.SKIP_INT16, "l0/k/y": mv.SKIP_INT16, "l0/v/y": mv.SKIP_WEIGHT_ZERO_POINT,
                         "l0/o/y": mv.SKIP_NO_SAMPLE, "l0/up/y": mv.SKIP_FLOAT_TARGET, "l0/down/y": mv.SKIP_INPUT}
  assert list(got) == ["l0/gate/y"] and got["l0/gate/y"]["mode"] == "dynamic"
  # a weight that is no constant or not 2-D in the float model; a target constant that is missing; a sample of another width
  C, ref, tgt = H._float_and_target()      # pylint: disable=protected-access
  for name in ("q", "o", "gate", "up", "down"):
    H._quantize_int8(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
  ref.buffers[H._tensor(ref, "l0/q/w").buffer].data = None      # pylint: disable=protected-access
  H._tensor(ref, "l0/o/w").shape = [D, D // 2, 2]      # pylint: disable=protected-access
  H._tensor(tgt, "l0/gate/w").name = b"l0/gate/renamed"      # pylint: disable=protected-access
  samples = _samples(C)
  for s in samples:
    s["l0/down_in"] = s["l0/down_in"][..., :DFF - 1]
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()())
  assert got.skipped == {"l0/q/y": mv.SKIP_WEIGHT, "l0/o/y": mv.SKIP_WEIGHT, "l0/gate/y": mv.SKIP_TARGET,
                         "l0/k/y": mv.SKIP_FLOAT_TARGET, "l0/v/y": mv.SKIP_FLOAT_TARGET,
                         "l0/down/y": mv.SKIP_SAMPLE_SHAPE}
  assert list(got) == ["l0/up/y"]
  # no samples at all
  got = mv.compare_layer_execution(ref, tgt, [], kernels=EC.numpy_kernels()())
  assert not got.results and mv.SKIP_NO_SAMPLE in set(got.skipped.values())


def test_transformed_inputs_are_followed_through_the_inserted_constant():
  from mi355q import model_validator as mv
  C, ref, tgt, m, _ = TH._models()      # pylint: disable=protected-access
  d_, dkv_, dff_ = TH.D, TH.DKV, TH.DFF
  rng = np.random.default_rng(8)
  widths = {f"l0/{src}": cols for _, _, cols, src in C.projections(d_, dkv_, dff_)}
  samples = [{name: rng.standard_normal((1, 20, cols)).astype(np.float32) for name, cols in widths.items()} for _ in range(2)]
  off = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()())
  assert sorted(off.results) == ["l0/k/y", "l0/q/y", "l0/v/y"]
  assert off.skipped == {f"l0/{n}/y": mv.SKIP_INPUT for n in ("o", "gate", "up", "down")}
  assert all("input_transform" not in r for r in off.results.values())
  on = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()(), follow_input_transforms=True)
  assert not on.skipped and len(on) == 7
  for name, rows, d, src in C.projections(d_, dkv_, dff_):
    r = on[f"l0/{name}/y"]
    kind, h = TH.EXPECTED[name]
    assert (r["input_transform"], r["hadamard_size"], r["mode"]) == (kind, h, "dynamic")
    transform = {"none": None, "multiply": lambda x: x * m,
                 "hadamard": lambda x, h=h: TH._rotate(x, h).astype(np.float32)}[kind]      # pylint: disable=protected-access
    t = TH._tensor(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
    w = TH._weight(ref, f"l0/{name}/w")      # pylint: disable=protected-access
    qw = np.asarray(tgt.buffers[t.buffer].data).view(np.int8).reshape(rows, d)
    scale = np.asarray(t.quantization.scale, np.float32)
    sq = np.zeros(rows)
    for s in samples:
      x = s[f"l0/{src}"].reshape(-1, d)
      xq, xs = EC.quantize_rows(x if transform is None else transform(x))
      yq = EC.forward(xq, xs, 0, qw, scale)[1].astype(np.float64)
      sq += ((yq - (x @ w.T).astype(np.float64)) ** 2).sum(axis=0)
    np.testing.assert_allclose(r["per_channel_error"], sq / 40, rtol=1e-12)
    assert r["error"] < 0.05 * r["signal"]      # the weight is in the basis the op reads: the wrong X would lose the signal
    if name in ("q", "k", "v"):
      assert r["error"] == off[f"l0/{name}/y"]["error"]


def test_save_leaves_the_per_channel_arrays_out(tmp_path):
  from mi355q import model_validator as mv
  C, ref, tgt, _ = _mixed_modes()
  samples = _samples(C)
  for s in samples:
    del s["l0/down_in"]
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC.numpy_kernels()())
  path = got.save(str(tmp_path / "out"), "m")
  assert path.endswith("m_layer_execution_errors.json") and os.path.exists(path)
  saved = json.load(open(path))
  assert saved["skipped"] == {"l0/down/y": mv.SKIP_NO_SAMPLE} and len(saved["layers"]) == 6
  for y, entry in saved["layers"].items():
    assert sorted(entry) == ["d", "error", "input", "mode", "output_mse", "output_snr", "rows", "signal", "tokens", "weight"]
    assert entry["error"] == got[y]["error"] and entry["mode"] == got[y]["mode"]


def test_validate_layer_execution_arguments_and_route(monkeypatch, tmp_path):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  ref = open(os.path.join(MODELS, "single_fc_bias.tflite"), "rb").read()
  qz = quantizer.Quantizer(ref)
  with pytest.raises(ValueError, match="No quantized model available to validate"):
    qz.validate_layer_execution([])
  qz._result = quantizer.QuantizationResult([{}], bytearray(ref))      # pylint: disable=protected-access
  with pytest.raises(ValueError, match="signature_key is required"):
    qz.validate_layer_execution({"a": [], "b": []})
  with pytest.raises(ValueError, match="no samples for signature"):
    qz.validate_layer_execution({"a": []}, signature_key="serving_default")
  # the whole route with the kernels replaced: a float "quantized" model is reported as such
  monkeypatch.setattr(mv, "LayerExecutionKernels", EC.numpy_kernels())
  x = np.random.default_rng(2).standard_normal((12, 8)).astype(np.float32)
  for data in ([{"serving_default_input_2:0": x}], {"serving_default": [{"serving_default_input_2:0": x}]}):
    got = qz.validate_layer_execution(data, save_folder=str(tmp_path), model_name="single")
    assert got.skipped == {"StatefulPartitionedCall:0": mv.SKIP_FLOAT_TARGET} and not got.results
  assert json.load(open(tmp_path / "single_layer_execution_errors.json"))["layers"] == {}


# ---------------------------------------------------------------- the kernels' build
def test_qfc_is_built():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "qfc.hip" in g.SOURCES


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_qfc_kernels_use_no_scratch_and_the_int8_matrix_cores(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path / "qfc.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "qfc.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  names = " ".join(kernels)
  for k in ("quantize_rows_vec_kernel", "quantize_rows_scalar_kernel", "weight_sums_kernel", "qfc_mfma_kernel",
            "qfc_generic_kernel", "sqdiff_cols_partial_kernel", "sqdiff_cols_sum_kernel"):
    assert k in names, k
  assert sum("qfc_mfma_kernel" in k for k in kernels) == 9      # I8 / I4 / I2 x (K = 64, K = 64 blockwise, K = 32 blockwise)
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
  # every MFMA kernel's body holds its instruction: the K = 64 one, or the K = 32 one for block 32
  text = {}
  for k in kernels:
    found = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(k), asm, re.M | re.S)
    assert found, k
    text[k] = found.group(1)
  for k in kernels:
    if "qfc_mfma_kernel" not in k:
      assert "v_mfma" not in text[k], k
    elif "Li32E" in k:
      assert "v_mfma_i32_16x16x32_i8" in text[k] and "v_mfma_i32_16x16x64_i8" not in text[k], k
    else:
      assert "v_mfma_i32_16x16x64_i8" in text[k] and "v_mfma_i32_16x16x32_i8" not in text[k], k
  # waves per SIMD as the compiler reports them, per (K step, blockwise): what the kernels had when each held a copy
  # of the main loop that csrc/qfc_tile.h now holds once (profiles/qfc_unify_isa.txt)
  floor = {("64", "0"): 3, ("32", "1"): 2, ("64", "1"): 1}
  for k in kernels:
    if "qfc_mfma_kernel" in k:
      occ = re.search(r"^%s:.*?;\s*Occupancy:\s*(\d+)" % re.escape(k), asm, re.M | re.S)
      assert occ and int(occ.group(1)) >= floor[re.search(r"Li(\d+)ELb([01])E", k).groups()], (k, occ and occ.group(1))
