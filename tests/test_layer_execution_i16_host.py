"""CPU checks of the integer execution of INT16-activation FULLY_CONNECTED ops (a16w8): the two entry points are
declared, exported, bound and refuse bad arguments before any launch; the NumPy statement of
tests/layer_execution_i16_cases.py holds against Python integers at the extremes and for the byte split over every
int16 value; model_validator.compare_layer_execution and Quantizer.validate_layer_execution with `int16_activations`
on the small models of the layer-execution host tests, with the NumPy stand-in for the kernels; and csrc/qfc16.hip is
built and compiles for gfx950 without scratch onto the int8 matrix cores."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import test_layer_error_host as H
import test_layer_execution_host as XH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("mi355q_qfc_forward_i16_workspace_bytes", "mi355q_qfc_forward_i16")
D, DKV, DFF = H.D, H.DKV, H.DFF
S16 = 0.0004        # the INT16 activation's scale in the models below: +- 13.1, wider than every sample


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
  assert len(_ffi.PROTOTYPES["mi355q_qfc_forward_i16"][1]) == 16
  assert len(_ffi.PROTOTYPES["mi355q_qfc_forward_i16_workspace_bytes"][1]) == 3
  from mi355q import model_validator as mv
  from mi355q import ops
  assert callable(ops.qfc_forward_i16)
  assert callable(mv.LayerExecutionKernels.quantize_static16) and callable(mv.LayerExecutionKernels.forward16)


def test_refusals_come_before_any_launch(lib):
  EC16.check_forward16_refusals(lib)


# ---------------------------------------------------------------- the NumPy statement itself
def _python_forward(xq, xs, qw, sw):
  """acc in Python integers; y = float32(float(acc) * float(float32(xs * sw))): a Python float is float64."""
  acc = [[sum(int(a) * int(b) for a, b in zip(xrow, wrow)) for wrow in qw] for xrow in xq]
  y = [[np.float32(float(acc[t][r]) * float(np.float32(xs[t]) * np.float32(sw[r]))) for r in range(len(qw))]
       for t in range(len(xq))]
  return acc, np.array(y, np.float32)


def test_numpy_statement_at_the_extremes():
  d = 65536
  xs, sw = np.array([3.1e-5, 0.7], np.float32), np.array([0.0071, 1.3e-3], np.float32)
  xq = np.stack([np.full(d, -32768, np.int16), np.full(d, 32767, np.int16)])
  qw = np.stack([np.full(d, -128), np.full(d, 127)])
  acc, y = EC16.forward16(xq, xs, qw, sw)
  assert acc.dtype == np.int64 and y.dtype == np.float32
  assert acc.tolist() == [[d * 32768 * 128, -d * 32768 * 127], [-d * 32767 * 128, d * 32767 * 127]]
  assert acc[0, 0] == 2 ** 38 and abs(int(acc[1, 0])) > 2 ** 37
  for t in range(2):
    for r in range(2):
      want = np.float32(float(int(acc[t, r])) * float(xs[t] * sw[r]))
      assert y[t, r] == want and np.isfinite(want)
  # float64 carries the accumulator exactly; a float32 of it would not: 2^38 - 2^21 + 1 terms differ
  odd = np.array([[2 ** 38 - 2 ** 21 + 1]], np.int64)
  assert int(odd.astype(np.float64)[0, 0]) == int(odd[0, 0]) and int(odd.astype(np.float32)[0, 0]) != int(odd[0, 0])
  # a small case written out in Python integers, per channel and blockwise
  rng = np.random.default_rng(4)
  xq = rng.integers(-32768, 32767, size=(3, 64), endpoint=True).astype(np.int16)
  xq[0, :15] = EC16.PLANTED
  qw = rng.integers(-128, 127, size=(5, 64), endpoint=True)
  xs = (np.exp(rng.normal(size=3)) * 1e-4).astype(np.float32)
  sw = (np.exp(rng.normal(size=5)) * 0.0071).astype(np.float32)
  acc, y = EC16.forward16(xq, xs, qw, sw)
  want_acc, want_y = _python_forward(xq, xs, qw, sw)
  assert acc.tolist() == want_acc and EC.same_bits(y, want_y)
  swb = (np.exp(rng.normal(size=10)) * 0.0071).astype(np.float32)
  none, yb = EC16.forward16(xq, xs, qw, swb, 32)
  want = np.zeros((3, 5), np.float32)
  for b in range(2):
    p = _python_forward(xq[:, 32 * b:32 * b + 32], xs, qw[:, 32 * b:32 * b + 32], swb.reshape(5, 2)[:, b])[1]
    want = want + p
  assert none is None and EC.same_bits(yb, want)
  # one scale for all tokens; a NaN scale gives NaN in its row only
  acc1, y1 = EC16.forward16(xq, xs[:1], qw, sw[:1])
  assert EC.same_bits(y1, _python_forward(xq, np.repeat(xs[:1], 3), qw, np.repeat(sw[:1], 5))[1])
  xs_nan = xs.copy()
  xs_nan[1] = np.nan
  y_nan = EC16.forward16(xq, xs_nan, qw, sw)[1]
  assert np.isnan(y_nan[1]).all() and EC.same_bits(y_nan[[0, 2]], y[[0, 2]])


def test_split_identity_over_every_int16_value():
  x = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
  h, l_s = EC16.split(x)
  assert h.dtype == np.int8 and l_s.dtype == np.int8
  for v, a, b in zip(x.tolist(), h.tolist(), l_s.tolist()):
    assert -128 <= a <= 127 and -128 <= b <= 127 and 256 * a + b + 128 == v, v
  assert (int(h.min()), int(h.max()), int(l_s.min()), int(l_s.max())) == (-128, 127, -128, 127)
  # so acc = 256 Sum h w + Sum l_s w + 128 Sum w, each of the first two within 2^30 at d = 65536
  rng = np.random.default_rng(6)
  xq = rng.integers(-32768, 32767, size=(4, 192), endpoint=True).astype(np.int16)
  xq[:, :15] = EC16.PLANTED
  qw = rng.integers(-128, 127, size=(6, 192), endpoint=True)
  h, l_s = EC16.split(xq)
  planes = 256 * (h.astype(np.int64) @ qw.T) + l_s.astype(np.int64) @ qw.T + 128 * qw.sum(axis=1)[None, :]
  assert np.array_equal(planes, EC16.forward16(xq, np.float32(1), qw, np.float32(1))[0])
  assert 65536 * 128 * 128 == 2 ** 30


def test_static_int16_quantizer_clips_and_rounds_to_even():
  x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 32767.4, 32767.5, 40000.0, -32768.5, -40000.0, -0.0], np.float32)
  assert EC16.quantize_static16(x, 1.0).tolist() == [0, 2, 2, 0, -2, 32767, 32767, 32767, -32768, -32768, 0]
  q = EC16.quantize_static16(np.array([1.0, -1.0, 0.3], np.float32), 1.0 / 32767)
  assert q.dtype == np.int16 and q.tolist()[:2] == [32767, -32767]


# ---------------------------------------------------------------- compare_layer_execution
def _a16_model():
  """q / k / v read an INT16 QUANTIZE of attn_in, o an INT8 one of o_in, gate / up are dynamic, down is weight-only."""
  from mi355q import qtyping as q
  C, ref, tgt = H._float_and_target()      # pylint: disable=protected-access
  for name, *_ in C.projections(D, DKV, DFF):
    H._quantize_int8(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
  XH._add_quantize(tgt, "l0/attn_in", ["q", "k", "v"], S16, 0, ttype=q.TensorType.INT16)      # pylint: disable=protected-access
  XH._add_quantize(tgt, "l0/o_in", ["o"], 0.05, -3)      # pylint: disable=protected-access
  XH._add_dequantize(tgt, "down")      # pylint: disable=protected-access
  return C, ref, tgt


def _reference16(ref, tgt, samples, name, src):
  """(signal, error, per-channel error, tokens) of an a16 op, written out here from the helper's arithmetic."""
  w = H._weight(ref, f"l0/{name}/w")      # pylint: disable=protected-access
  rows, d = w.shape
  t = H._tensor(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
  qw = np.asarray(tgt.buffers[t.buffer].data).view(np.int8).reshape(rows, d)
  scale = np.asarray(t.quantization.scale, np.float32)
  sq_d, sq_b, tokens = np.zeros(rows), np.zeros(rows), 0
  for s in samples:
    x = s[f"l0/{src}"].reshape(-1, d)
    y = (x @ w.T).astype(np.float64)
    yq = EC16.forward16(EC16.quantize_static16(x, S16), np.float32(S16), qw, scale)[1]
    sq_d += ((yq.astype(np.float64) - y) ** 2).sum(axis=0)
    sq_b += (y ** 2).sum(axis=0)
    tokens += x.shape[0]
  return sq_b.sum() / tokens, sq_d.sum() / tokens, sq_d / tokens, tokens


MODES = {"q": ("static", 16), "k": ("static", 16), "v": ("static", 16), "o": ("static", 8), "gate": ("dynamic", None),
         "up": ("dynamic", None), "down": ("weight_only", None)}


def test_the_plain_call_still_skips_int16_and_the_keyword_executes_it():
  from mi355q import model_validator as mv
  C, ref, tgt = _a16_model()
  samples = XH._samples(C)      # pylint: disable=protected-access
  plain = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()())
  assert plain.skipped == {f"l0/{n}/y": mv.SKIP_INT16 for n in ("q", "k", "v")}
  assert list(plain) == [f"l0/{n}/y" for n in ("o", "gate", "up", "down")]
  assert all("activation_bits" not in r for r in plain.results.values())
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()(), int16_activations=True)
  assert not got.skipped and list(got) == [f"l0/{n}/y" for n, *_ in C.projections(D, DKV, DFF)]
  for name, rows, d, src in C.projections(D, DKV, DFF):
    r = got[f"l0/{name}/y"]
    assert (r["mode"], r["activation_bits"]) == MODES[name], name
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
    if MODES[name][1] == 16:
      signal, error, per_channel, tokens = _reference16(ref, tgt, samples, name, src)
      assert r["tokens"] == tokens == 24 + 27
      np.testing.assert_allclose(r["per_channel_error"], per_channel, rtol=1e-12)
      np.testing.assert_allclose([r["signal"], r["error"]], [signal, error], rtol=1e-12)
      assert r["error"] > 0 and r["output_mse"] == r["error"] / rows
      assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)
    else:      # the other modes are what the plain call gives
      for key, value in plain[f"l0/{name}/y"].items():
        assert np.array_equal(r[key], value), (name, key)
  # the int16 activation costs next to nothing: the a16 op's error is the weight's, within a percent
  weight_only = XH._reference(ref, tgt, samples, "q", "attn_in", "weight_only")[1]      # pylint: disable=protected-access
  assert abs(got["l0/q/y"]["error"] - weight_only) < 0.01 * weight_only


def test_int16_inputs_that_are_not_executed():
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  C, ref, tgt = H._float_and_target()      # pylint: disable=protected-access
  for name, *_ in C.projections(D, DKV, DFF):
    H._quantize_int8(tgt, f"l0/{name}/w")      # pylint: disable=protected-access
  # q / k / v: zero point 3; gate / up: two scales; o: another source; down: behind a DEQUANTIZE'd weight
  XH._add_quantize(tgt, "l0/attn_in", ["q", "k", "v"], S16, 3, ttype=q.TensorType.INT16)      # pylint: disable=protected-access
  XH._add_quantize(tgt, "l0/mlp_in", ["gate", "up"], S16, 0, ttype=q.TensorType.INT16)      # pylint: disable=protected-access
  H._tensor(tgt, "l0/mlp_in_quantized").quantization.scale = np.array([S16, S16], np.float32)      # pylint: disable=protected-access
  XH._add_quantize(tgt, "l0/down_in", ["o", "down"], S16, 0, ttype=q.TensorType.INT16)      # pylint: disable=protected-access
  XH._add_dequantize(tgt, "down")      # pylint: disable=protected-access
  samples = XH._samples(C)      # pylint: disable=protected-access
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()(), int16_activations=True)
  assert not got.results
  assert got.skipped == {f"l0/{n}/y": mv.SKIP_INPUT for n, *_ in C.projections(D, DKV, DFF)}
  plain = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()())
  assert plain.skipped == {f"l0/{n}/y": mv.SKIP_INT16 for n, *_ in C.projections(D, DKV, DFF)}
  # an absent zero point is 0, and the op may read the float model's input itself as INT16
  C, ref, tgt = _a16_model()
  H._tensor(tgt, "l0/attn_in_quantized").quantization.zeroPoint = None      # pylint: disable=protected-access
  t = H._tensor(tgt, "l0/mlp_in")      # pylint: disable=protected-access
  t.type = int(q.TensorType.INT16)
  t.quantization = q.QuantizationParametersT(scale=np.array([S16], np.float32), zeroPoint=np.array([0], np.int64))
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()(), int16_activations=True)
  assert not got.skipped
  assert [got[f"l0/{n}/y"]["activation_bits"] for n in ("q", "k", "v", "gate", "up")] == [16] * 5
  assert got["l0/gate/y"]["mode"] == "static"


def test_save_carries_activation_bits_only_with_the_keyword(tmp_path):
  from mi355q import model_validator as mv
  C, ref, tgt = _a16_model()
  samples = XH._samples(C)      # pylint: disable=protected-access
  keys = ["d", "error", "input", "mode", "output_mse", "output_snr", "rows", "signal", "tokens", "weight"]
  plain = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()())
  saved = json.load(open(plain.save(str(tmp_path / "plain"), "m")))
  assert len(saved["layers"]) == 4 and all(sorted(e) == keys for e in saved["layers"].values())
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()(), int16_activations=True)
  saved = json.load(open(got.save(str(tmp_path / "a16"), "m")))
  assert saved["skipped"] == {} and len(saved["layers"]) == 7
  for y, entry in saved["layers"].items():
    assert sorted(entry) == sorted(keys + ["activation_bits"])
    assert entry["activation_bits"] == got[y]["activation_bits"] == MODES[y.split("/")[1]][1]


def test_validate_layer_execution_passes_the_keyword_on_and_saves(monkeypatch, tmp_path):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  from mi355q.utils import tflite_flatbuffer
  C, ref, tgt = _a16_model()
  samples = XH._samples(C)      # pylint: disable=protected-access
  qz = quantizer.Quantizer(ref)
  qz._result = quantizer.QuantizationResult([{}], bytearray(tflite_flatbuffer.write_model(tgt)))      # pylint: disable=protected-access
  monkeypatch.setattr(mv, "LayerExecutionKernels", EC16.numpy_kernels())
  plain = qz.validate_layer_execution(samples)
  assert plain.skipped == {f"l0/{n}/y": mv.SKIP_INT16 for n in ("q", "k", "v")} and len(plain) == 4
  got = qz.validate_layer_execution({"serving_default": samples}, save_folder=str(tmp_path), model_name="a16",
                                    int16_activations=True)
  assert got.skipped == {} and len(got) == 7
  want = mv.compare_layer_execution(ref, tgt, samples, kernels=EC16.numpy_kernels()(), int16_activations=True)
  for y, r in want.results.items():
    assert got[y]["error"] == r["error"] and got[y]["activation_bits"] == r["activation_bits"] and got[y]["mode"] == r["mode"]
  saved = json.load(open(tmp_path / "a16_layer_execution_errors.json"))
  assert {y: e["activation_bits"] for y, e in saved["layers"].items()} == {f"l0/{n}/y": b for n, (_, b) in MODES.items()}


# ---------------------------------------------------------------- the kernels' build
def test_qfc16_is_built():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "qfc16.hip" in g.SOURCES and "qfc.hip" in g.SOURCES
  assert "qfc_frag.h" in g.HEADERS      # (what both files include is part of their fingerprints)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_qfc16_kernels_use_no_scratch_and_the_int8_matrix_cores(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path / "qfc16.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "qfc16.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  names = " ".join(kernels)
  for k in ("weight_sums_kernel", "qfc16_mfma_kernel", "qfc16_generic_kernel"):
    assert k in names, k
  assert sum("qfc16_mfma_kernel" in k for k in kernels) == 9      # I8 / I4 / I2 x (K = 64, K = 64 blockwise, K = 32 blockwise)
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
  text = {}
  for k in kernels:
    found = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(k), asm, re.M | re.S)
    assert found, k
    text[k] = found.group(1)
  for k in kernels:
    if "qfc16_mfma_kernel" not in k:
      assert "v_mfma" not in text[k], k
    elif "Li32E" in k:
      assert "v_mfma_i32_16x16x32_i8" in text[k] and "v_mfma_i32_16x16x64_i8" not in text[k], k
    else:
      assert "v_mfma_i32_16x16x64_i8" in text[k] and "v_mfma_i32_16x16x32_i8" not in text[k], k
    if "qfc16_mfma_kernel" in k:      # the split of the activation into its two int8 planes is done in registers
      assert "v_perm_b32" in text[k], k
  # waves per SIMD as the compiler reports them, per (K step, blockwise): what the kernels had before their policy,
  # constants and host side moved into csrc/qfc_tile.h (profiles/qfc_unify_isa.txt)
  floor = {("64", "0"): 3, ("32", "1"): 2, ("64", "1"): 2}
  for k in kernels:
    if "qfc16_mfma_kernel" in k:
      occ = re.search(r"^%s:.*?;\s*Occupancy:\s*(\d+)" % re.escape(k), asm, re.M | re.S)
      assert occ and int(occ.group(1)) >= floor[re.search(r"Li(\d+)ELb([01])E", k).groups()], (k, occ and occ.group(1))
