"""CPU checks of the integer execution of static FULLY_CONNECTED ops through to their stored output: the entry points
are declared, exported, bound and refuse bad arguments before any launch; hand-derived known answers of the statement
in tests/layer_output_cases.py (Python integers); ops.quantize_multiplier / ops.activation_range against it;
model_validator.compare_layer_execution and Quantizer.validate_layer_execution with `quantized_outputs` and NumPy
kernels, with the keyword off (nothing changes) and on (the new keys, every final_skipped reason); csrc/qfc_out.hip is
built and compiles for gfx950 without scratch, the MFMA route onto the int8 matrix cores."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("mi355q_qfc_output_workspace_bytes", "mi355q_qfc_output_i8", "mi355q_qfc_output_i16")


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
  assert len(_ffi.PROTOTYPES["mi355q_qfc_output_i8"][1]) == 18
  assert len(_ffi.PROTOTYPES["mi355q_qfc_output_i16"][1]) == 16
  assert len(_ffi.PROTOTYPES["mi355q_qfc_output_workspace_bytes"][1]) == 2
  from mi355q import model_validator as mv
  from mi355q import ops
  for fn in (ops.qfc_output, ops.qfc_output_i16, ops.quantize_multiplier, ops.activation_range):
    assert callable(fn)
  for method in ("bias", "output", "output16", "dequantize_output", "reference_output"):
    assert callable(getattr(mv.LayerExecutionKernels, method)), method


def test_refusals_come_before_any_launch(lib):
  OC.check_output_refusals(lib)


def test_the_wrapper_refuses_multipliers_and_shifts_outside_the_preconditions(lib):
  """ops._qfc_output_tables works on the host tables it is given, before anything touches the device."""
  from mi355q import ops
  check = ops._qfc_output_tables      # pylint: disable=protected-access
  for bits, hi in ((8, 30), (16, 14)):
    with pytest.raises(ValueError, match="multiplier is outside"):
      check("t", [-1], [0], 4, bits)
    with pytest.raises(ValueError, match="multiplier is outside"):
      check("t", [1 << 31], [0], 4, bits)
    with pytest.raises(ValueError, match=r"shift is outside \[-31, %d\]" % hi):
      check("t", [1 << 30], [hi + 1], 4, bits)
    with pytest.raises(ValueError, match="shift is outside"):
      check("t", [1 << 30] * 4, [0, 0, -32, 0], 4, bits)
    with pytest.raises(ValueError, match="1 or rows = 4 entries"):
      check("t", [1 << 30] * 3, [0] * 3, 4, bits)
    with pytest.raises(ValueError, match="1 or rows = 4 entries"):
      check("t", [1 << 30] * 4, [0], 4, bits)


# ---------------------------------------------------------------- known answers, derived by hand
def test_quantize_multiplier_known_answers():
  assert OC.quantize_multiplier(0.0) == (0, 0)
  assert OC.quantize_multiplier(0.5) == (1 << 30, 0)            # frexp(0.5) = (0.5, 0)
  assert OC.quantize_multiplier(1.0) == (1 << 30, 1)            # frexp(1.0) = (0.5, 1)
  assert OC.quantize_multiplier(0.75) == (1610612736, 0)        # 0.75 * 2^31
  assert OC.quantize_multiplier(0.25) == (1 << 30, -1)
  # a fraction within 2^-33 of 1 rounds up to 2^31, which becomes 2^30 with the exponent one higher
  almost_one = 1.0 - 2.0 ** -34
  assert almost_one < 1.0 and OC.quantize_multiplier(almost_one) == (1 << 30, 1)
  assert OC.quantize_multiplier(4.0 * almost_one) == (1 << 30, 3)
  assert OC.quantize_multiplier(1.0 - 2.0 ** -32) == (1 << 30, 1)            # 2^31 - 1/2: the half goes away from zero
  assert OC.quantize_multiplier(1.0 - 2.0 ** -31) == ((1 << 31) - 1, 0)      # the largest multiplier
  assert OC.quantize_multiplier(2.0 ** -33) == (0, 0)           # frexp = (0.5, -32): below the shift range
  assert OC.quantize_multiplier(2.0 ** -32) == (1 << 30, -31)   # the smallest exponent kept
  assert OC.quantize_multiplier(2.0 ** 29) == (1 << 30, 30)
  with pytest.raises(ValueError):
    OC.quantize_multiplier(2.0 ** 30)                           # frexp = (0.5, 31)
  # the half of the last place rounds away from zero: frac * 2^31 = 2^30 + 1/2
  assert OC.quantize_multiplier((2.0 ** 30 + 0.5) / 2.0 ** 31) == ((1 << 30) + 1, 0)


def test_mbqm32_known_answers():
  half = 1 << 30      # M = 2^30 is the real multiplier 1/2
  assert OC.mbqm32(100, half, 0) == 50
  # exact halves of the high multiplication: p + 2^30 carries a positive half up; a negative p gets 1 - 2^30 and the
  # division truncates, so -50.5 becomes -50 and -49.5 becomes -49 (halves go towards +infinity)
  assert OC.mbqm32(101, half, 0) == 51 and OC.mbqm32(-101, half, 0) == -50
  assert OC.mbqm32(99, half, 0) == 50 and OC.mbqm32(-99, half, 0) == -49
  assert OC.mbqm32(102, half, 0) == 51 and OC.mbqm32(-102, half, 0) == -51
  assert OC.mbqm32(0, half, 0) == 0 and OC.mbqm32(12345, 0, 0) == 0
  # ties after the right shift: h = +-(2^(R-1)) (+-0.5 after it) goes away from zero, one less in magnitude goes to 0
  for right in (1, 8, 31):
    tie = 1 << (right - 1)
    for h, want in ((tie, 1), (-tie, -1), (3 * tie, 2), (-3 * tie, -2)):
      if not OC.INT32_MIN <= 2 * h <= OC.INT32_MAX:
        continue
      assert OC.mbqm32(2 * h, half, -right) == want, (right, h)      # 2 h * 1/2 = h exactly
    if right > 1:
      assert OC.mbqm32(2 * (tie - 1), half, -right) == 0 and OC.mbqm32(-2 * (tie - 1), half, -right) == 0
  assert OC.mbqm32(1 << 30, half, -31) == 0            # h = 2^29: a quarter
  assert OC.mbqm32(OC.INT32_MAX, OC.INT32_MAX, -31) == 1 and OC.mbqm32(OC.INT32_MIN, OC.INT32_MAX, -31) == -1
  # sat32 of a * 2^L: without it 2^30 * 2^1 would wrap to -2^31
  assert OC.mbqm32(1 << 30, half, 1) == 1 << 30        # sat32(2^31) = 2^31 - 1, times 1/2 and rounded: 2^30
  assert OC.mbqm32(-(1 << 30) - 1, half, 1) == -(1 << 30)
  assert OC.mbqm32(3, half, 30) == 1 << 30 and OC.mbqm32(-3, half, 30) == -(1 << 30)
  assert OC.mbqm32(1, half, 30) == 1 << 29             # 2^30 fits: no saturation
  assert OC.mbqm32(5, OC.INT32_MAX, 7) == 640          # 640 (1 - 2^-31) rounds to 640
  assert OC.sat32(OC.INT32_MAX + 1) == OC.INT32_MAX and OC.sat32(OC.INT32_MIN - 1) == OC.INT32_MIN
  assert OC.sat32(-5) == -5
  # the division truncates towards zero where Python's // floors
  assert OC.trunc_div(-(1 << 31) - 1, 1 << 31) == -1 and OC.trunc_div(-1, 1 << 31) == 0 and (-1) // (1 << 31) == -1


def test_output_i8_saturates_the_bias_sum_and_clamps_to_the_activation_range():
  x = np.zeros((1, 64), np.int8)
  x[0, 0] = 1
  w = np.zeros((4, 64), np.int64)
  w[:, 0] = 1      # acc = 1 in every channel
  bias = np.array([OC.INT32_MAX, OC.INT32_MIN, 199, -201], np.int64)
  # a = sat32(1 + bias) = [2^31 - 1, -2^31 + 1, 200, -200]; M = 2^30, s = 0 halves them
  got = OC.output_i8(x, 0, w, bias, [1 << 30], [0], 3, -128, 127)
  assert got.tolist() == [[127, -128, 103, -97]]
  got = OC.output_i8(x, 0, w, bias, [1 << 30], [0], 3, -100, 100)
  assert got.tolist() == [[100, -100, 100, -97]]
  # a zero point on the input: acc = (1 - 5) * 1 + 63 * (0 - 5) * 0 = -4
  got = OC.output_i8(x, 5, w, None, [1 << 30], [1], 0, -128, 127)
  assert got.tolist() == [[-4] * 4]


def test_mbqm64_known_answers():
  assert OC.rounded_multiplier(0x7FFEFFFF) == 0x7FFF and OC.rounded_multiplier(0x7FFF0000) == 0x7FFF
  assert OC.rounded_multiplier(0x7FFE7FFF) == 0x7FFE and OC.rounded_multiplier(0x7FFE8000) == 0x7FFF
  assert OC.rounded_multiplier(0x7FFFFFFF) == 0x7FFF      # (the rounding would give 2^15: the threshold keeps 15 bits)
  assert OC.rounded_multiplier(1 << 30) == 1 << 14 and OC.rounded_multiplier(0) == 0
  assert OC.mbqm64(100, 1 << 30, 0) == 50                 # Mr = 2^14, T = 15: 100 * 2^14 / 2^15
  assert OC.mbqm64(101, 1 << 30, 0) == 51 and OC.mbqm64(-101, 1 << 30, 0) == -50      # halves go UP (floor of + 1/2)
  assert OC.mbqm64(1, 1 << 30, 14) == 1 << 13             # T = 1
  # at +-(2^47 - 1) with the largest Mr and T = 46: (2^47 - 1) 32767 / 2^46 = 65534 - 32767 / 2^46, plus the half
  assert OC.mbqm64(OC.A16_MAX, 0x7FFFFFFF, -31) == 65534 and OC.mbqm64(-OC.A16_MAX, 0x7FFFFFFF, -31) == -65534
  assert OC.mbqm64(OC.A16_MIN, 0x7FFFFFFF, -31) == -65534      # -65534 + 1/2 floors to -65534
  assert OC.mbqm64(OC.A16_MAX, 0x7FFFFFFF, 14) == (OC.A16_MAX * 0x7FFF + 1) >> 1
  assert (1 << 47) * 0x7FFF + (1 << 45) < 1 << 63         # the largest intermediate fits int64
  x = np.zeros((1, 64), np.int16)
  x[0, 0] = 1
  w = np.zeros((2, 64), np.int64)
  w[:, 0] = 1
  # bias +-2^50: a is clamped to [-2^47, 2^47 - 1] first; Mr = 2^13, T = 46: 2^14 + 1/2 - 2^-33 and -2^14 + 1/2
  got = OC.output_i16(x, w, np.array([1 << 50, -(1 << 50)], np.int64), [1 << 29], [-31], -32768, 32767)
  assert got.tolist() == [[16384, -16384]]
  got = OC.output_i16(x, w, np.array([1 << 50, -(1 << 50)], np.int64), [1 << 29], [-30], -32768, 32767)
  assert got.tolist() == [[32767, -32768]]                # twice that: 32768 is beyond the type
  got = OC.output_i16(x, w, np.array([1 << 50, -(1 << 50)], np.int64), [1 << 29], [-30], -5, 9)
  assert got.tolist() == [[9, -5]]


def test_activation_range_known_answers():
  assert OC.activation_range(OC.NONE, 0.1, 7, 8) == (-128, 127)
  assert OC.activation_range(OC.RELU, 0.1, 7, 8) == (7, 127) and OC.activation_range(OC.RELU, 0.1, -128, 8) == (-128, 127)
  assert OC.activation_range(OC.RELU6, 6.0 / 255.0, -128, 8) == (-128, 127)
  assert OC.activation_range(OC.RELU6, 0.1, -100, 8) == (-100, -40)
  assert OC.activation_range(OC.RELU6, 0.01, 0, 8) == (0, 127)           # 600 is beyond the type
  assert OC.activation_range(OC.RELU_N1_TO_1, 0.1, 3, 8) == (-7, 13)
  assert OC.activation_range(OC.RELU_N1_TO_1, 0.4, 0, 8) == (-3, 3)      # 2.5 goes away from zero
  assert OC.activation_range(OC.RELU6, 0.001, 0, 16) == (0, 6000) and OC.activation_range(OC.NONE, 1.0, 0, 16) == (-32768, 32767)
  with pytest.raises(ValueError):
    OC.activation_range(OC.TANH, 0.1, 0, 8)


def test_ops_host_functions_equal_the_statement_on_a_seeded_sweep():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import ops
  rng = np.random.default_rng(2024)
  reals = np.concatenate([np.exp(rng.uniform(np.log(2.0 ** -36), np.log(2.0 ** 32), size=9000)),
                          np.ldexp(1.0 - np.ldexp(rng.uniform(0, 4, size=500), -33), rng.integers(-33, 32, size=500)),
                          np.ldexp(0.5, rng.integers(-34, 34, size=500)).astype(np.float64)])
  assert reals.size == 10 ** 4
  raised = 0
  for real in reals.tolist():
    try:
      want = OC.quantize_multiplier(real)
    except ValueError:
      raised += 1
      with pytest.raises(ValueError):
        ops.quantize_multiplier(real)
      continue
    assert ops.quantize_multiplier(real) == want, real
    m, s = want
    assert (m, s) == (0, 0) or ((1 << 30) <= m < (1 << 31) and -31 <= s <= 30 and abs(m * 2.0 ** (s - 31) / real - 1) < 2.0 ** -30)
  assert 0 < raised < 1000
  assert ops.quantize_multiplier(0.0) == (0, 0) and ops.quantize_multiplier(0.75) == (1610612736, 0)
  for i, real in enumerate(reals.tolist()):
    s_y, zp, bits = min(max(real, 1e-6), 1e3), int(rng.integers(-128, 128)), (8, 16)[i % 2]
    zp = zp if bits == 8 else 0
    for fused in (OC.NONE, OC.RELU, OC.RELU_N1_TO_1, OC.RELU6):
      assert ops.activation_range(fused, s_y, zp, bits) == OC.activation_range(fused, s_y, zp, bits), (fused, s_y, zp, bits)
  with pytest.raises(ValueError, match="fused activation 4"):
    ops.activation_range(OC.TANH, 0.1, 0, 8)
  assert ops.FUSED_ACTIVATION_NAMES == OC.NAMES


# ---------------------------------------------------------------- compare_layer_execution
@pytest.fixture(scope="module")
def models():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  ref = OC.build_model()
  samples = OC.build_samples(ref)
  return ref, samples, OC.quantize_by_hand(ref, samples, 8), OC.quantize_by_hand(ref, samples, 16)


def _tensor(model, name):
  return next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)


def _op(model, name):
  sg = model.subgraphs[0]
  return next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"{name}/y")


def _final_reference(ref, tgt, samples, name, rows, fused, has_bias, bits):
  """(final_signal, final_error, per channel) written out here from the statement and the written tensors."""
  x_t, y_t, w_t = _tensor(tgt, f"{name}/x"), _tensor(tgt, f"{name}/y"), _tensor(tgt, f"{name}/w")
  s_x, zp_x = np.float32(x_t.quantization.scale[0]), int(x_t.quantization.zeroPoint[0])
  s_y, zp_y = np.float32(y_t.quantization.scale[0]), int(y_t.quantization.zeroPoint[0])
  s_w = np.asarray(w_t.quantization.scale, np.float32)
  qw = np.asarray(tgt.buffers[w_t.buffer].data).view(np.int8).reshape(rows, OC.D)
  bias = None
  if has_bias:
    b_t = _tensor(tgt, f"{name}/b")
    bias = np.asarray(tgt.buffers[b_t.buffer].data).view(np.int64 if bits == 16 else np.int32)
  ms = [OC.quantize_multiplier(float(s_x) * float(v) / float(s_y)) for v in s_w.tolist()]
  m, s = [v[0] for v in ms], [v[1] for v in ms]
  lo, hi = OC.activation_range(fused, float(s_y), zp_y, bits)
  sq_d, sq_b, tokens = np.zeros(rows), np.zeros(rows), 0
  for sample in samples:
    x = sample[f"{name}/x"].reshape(-1, OC.D)
    if bits == 16:
      q = OC.output_i16(OC.EC16.quantize_static16(x, s_x), qw, bias, m, s, lo, hi)
    else:
      q = OC.output_i8(OC.EC.quantize_static(x, s_x, zp_x), zp_x, qw, bias, m, s, zp_y, lo, hi)
    yq = ((q.astype(np.int32) - zp_y).astype(np.float32) * s_y).astype(np.float64)
    y = OC.float_output(ref, name, fused, has_bias, x).astype(np.float64)
    sq_d += ((yq - y) ** 2).sum(axis=0)
    sq_b += (y ** 2).sum(axis=0)
    tokens += x.shape[0]
  return sq_b.sum() / tokens, sq_d.sum() / tokens, sq_d / tokens, tokens


def test_with_the_keyword_off_results_and_saved_json_are_what_they_were(models, tmp_path):
  from mi355q import model_validator as mv
  ref, samples, tgt8, _ = models
  old = mv.compare_layer_execution(ref, tgt8, samples, kernels=OC.EC.numpy_kernels()(), int16_activations=True)
  new = mv.compare_layer_execution(ref, tgt8, samples, kernels=OC.numpy_kernels()(), int16_activations=True,
                                   quantized_outputs=False)
  plain = mv.compare_layer_execution(ref, tgt8, samples, kernels=OC.numpy_kernels()())
  keys = ["d", "error", "input", "mode", "output_mse", "output_snr", "per_channel_error", "rows", "signal", "tokens", "weight"]
  assert list(old) == list(new) == list(plain) == [f"{n}/y" for n, *_ in OC.OPS] and not new.skipped and not plain.skipped
  for y in old:
    assert sorted(plain[y]) == keys and sorted(new[y]) == sorted(keys + ["activation_bits"])
    for k, v in old[y].items():
      assert np.array_equal(new[y][k], v), (y, k)
  a, b = open(old.save(str(tmp_path / "old"), "m"), "rb").read(), open(new.save(str(tmp_path / "new"), "m"), "rb").read()
  assert a == b and b"final" not in a and b"output_bits" not in a
  on = mv.compare_layer_execution(ref, tgt8, samples, kernels=OC.numpy_kernels()(), quantized_outputs=True)
  for y in plain:      # the pre-bias figures do not move when the keyword is on
    for k, v in plain[y].items():
      assert np.array_equal(on[y][k], v), (y, k)


@pytest.mark.parametrize("bits", [8, 16])
def test_with_the_keyword_on_every_static_op_carries_its_final_figures(models, bits, tmp_path):
  from mi355q import model_validator as mv
  ref, samples, tgt8, tgt16 = models
  tgt = tgt16 if bits == 16 else tgt8
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=OC.numpy_kernels()(), int16_activations=True,
                                   quantized_outputs=True)
  assert not got.skipped and list(got) == [f"{n}/y" for n, *_ in OC.OPS]
  for name, rows, fused, has_bias in OC.OPS:
    r = got[f"{name}/y"]
    signal, error, per_channel, tokens = _final_reference(ref, tgt, samples, name, rows, fused, has_bias, bits)
    assert "final_skipped" not in r and r["output_bits"] == r["activation_bits"] == bits and r["mode"] == "static"
    assert r["fused_activation"] == OC.NAMES[fused] and r["tokens"] == tokens == sum(OC.TOKENS)
    np.testing.assert_allclose(r["final_per_channel_error"], per_channel, rtol=1e-12)
    np.testing.assert_allclose([r["final_signal"], r["final_error"]], [signal, error], rtol=1e-12)
    assert r["final_per_channel_error"].dtype == np.float64 and r["final_per_channel_error"].shape == (rows,)
    assert r["final_output_mse"] == r["final_error"] / rows
    assert r["final_output_snr"] == (r["final_signal"] / rows) / (r["final_output_mse"] + 1e-9)
    assert 0 < r["final_error"] < r["final_signal"]
  assert got["fc3/y"]["final_error"] > got["fc3/y"]["error"] or bits == 16      # no bias: the int8 output grid adds error
  saved = json.load(open(got.save(str(tmp_path), "m")))
  scalars = ["activation_bits", "d", "error", "final_error", "final_output_mse", "final_output_snr", "final_signal",
             "fused_activation", "input", "mode", "output_bits", "output_mse", "output_snr", "rows", "signal", "tokens", "weight"]
  for y, entry in saved["layers"].items():
    assert sorted(entry) == scalars and entry["final_error"] == got[y]["final_error"] and entry["output_bits"] == bits


def test_every_final_skipped_reason(models):
  import copy
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  ref, samples, tgt8, tgt16 = models

  def run(ref_model, tgt):
    return mv.compare_layer_execution(ref_model, tgt, samples, kernels=OC.numpy_kernels()(), int16_activations=True,
                                      quantized_outputs=True)

  def expect(got, reasons):
    assert not got.skipped
    for name, *_ in OC.OPS:
      r = got[f"{name}/y"]
      if name in reasons:
        assert r["final_skipped"] == reasons[name] and not [k for k in r if k.startswith("final_") and k != "final_skipped"]
        assert "fused_activation" not in r and r["output_bits"] in (8, 16) and r["error"] > 0
      else:
        assert "final_skipped" not in r and r["final_error"] > 0
  # the output tensor: per-channel scales; float; an INT16 output with a zero point; an INT8 output under a16
  t8, t16 = copy.deepcopy(tgt8), copy.deepcopy(tgt16)
  y = _tensor(t8, "fc0/y")
  y.quantization.scale = np.full(128, y.quantization.scale[0], np.float32)
  _tensor(t8, "fc1/y").type = int(q.TensorType.FLOAT32)
  _tensor(t8, "fc2/y").quantization = None
  expect(run(ref, t8), {"fc0": mv.FINAL_SKIP_OUTPUT, "fc1": mv.FINAL_SKIP_OUTPUT, "fc2": mv.FINAL_SKIP_OUTPUT})
  _tensor(t16, "fc0/y").quantization.zeroPoint = np.array([3], np.int64)
  _tensor(t16, "fc1/y").type = int(q.TensorType.INT8)
  _tensor(t16, "fc2/y").quantization.zeroPoint = None      # absent is 0
  expect(run(ref, t16), {"fc0": mv.FINAL_SKIP_OUTPUT, "fc1": mv.FINAL_SKIP_OUTPUT})
  # the target's bias: float, of another length, INT32 under a16, beyond 2^47
  t8, t16 = copy.deepcopy(tgt8), copy.deepcopy(tgt16)
  _tensor(t8, "fc0/b").type = int(q.TensorType.FLOAT32)
  b = _tensor(t8, "fc1/b")
  b.shape = [95]
  _op(t8, "fc2").inputs = [_op(t8, "fc2").inputs[0], _op(t8, "fc2").inputs[1]]      # two inputs: no bias at all
  r = run(ref, t8)
  expect(r, {"fc0": mv.FINAL_SKIP_BIAS, "fc1": mv.FINAL_SKIP_BIAS})
  b = _tensor(t16, "fc0/b")
  t16.buffers[b.buffer].data = np.asarray(t16.buffers[b.buffer].data).view(np.int64).astype(np.int32).view(np.uint8)
  b.type = int(q.TensorType.INT32)
  b = _tensor(t16, "fc1/b")
  big = np.asarray(t16.buffers[b.buffer].data).view(np.int64).copy()
  big[5] = (1 << 47) + 1
  t16.buffers[b.buffer].data = big.view(np.uint8)
  b = _tensor(t16, "fc2/b")
  edge = np.asarray(t16.buffers[b.buffer].data).view(np.int64).copy()
  edge[5] = -(1 << 47)      # at the bound: executed
  t16.buffers[b.buffer].data = edge.view(np.uint8)
  expect(run(ref, t16), {"fc0": mv.FINAL_SKIP_BIAS, "fc1": mv.FINAL_SKIP_BIAS_RANGE})
  # the float model's bias: not a constant; float16
  r2 = copy.deepcopy(ref)
  _tensor(r2, "fc0/b").buffer = 0
  _tensor(r2, "fc1/b").type = int(q.TensorType.FLOAT16)
  expect(run(r2, tgt8), {"fc0": mv.FINAL_SKIP_FLOAT_BIAS, "fc1": mv.FINAL_SKIP_FLOAT_BIAS})
  # fused TANH in the target or in the float model; another weightsFormat
  t8, r2 = copy.deepcopy(tgt8), copy.deepcopy(ref)
  _op(t8, "fc0").builtinOptions.fusedActivationFunction = OC.TANH
  _op(r2, "fc1").builtinOptions.fusedActivationFunction = OC.TANH
  _op(t8, "fc2").builtinOptions.weightsFormat = 1
  expect(run(r2, t8), {"fc0": mv.FINAL_SKIP_ACTIVATION, "fc1": mv.FINAL_SKIP_ACTIVATION, "fc2": mv.FINAL_SKIP_WEIGHTS_FORMAT})
  # an output scale so small that the multiplier needs a left shift beyond the op's range
  t8, t16 = copy.deepcopy(tgt8), copy.deepcopy(tgt16)
  _tensor(t8, "fc0/y").quantization.scale = np.array([1e-15], np.float32)
  _tensor(t16, "fc0/y").quantization.scale = np.array([1e-11], np.float32)      # a shift within [-31, 30], beyond 14
  expect(run(ref, t8), {"fc0": mv.FINAL_SKIP_MULTIPLIER})
  expect(run(ref, t16), {"fc0": mv.FINAL_SKIP_MULTIPLIER})


def test_dynamic_and_weight_only_ops_have_no_output_bits(models):
  import copy
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  ref, samples, tgt8, _ = models
  tgt = copy.deepcopy(tgt8)
  for name in ("fc0", "fc1"):      # float activations in and out: the op is dynamic-range
    for end in ("x", "y"):
      t = _tensor(tgt, f"{name}/{end}")
      t.type, t.quantization = int(q.TensorType.FLOAT32), None
  got = mv.compare_layer_execution(ref, tgt, samples, kernels=OC.numpy_kernels()(), quantized_outputs=True)
  for name in ("fc0", "fc1"):
    r = got[f"{name}/y"]
    assert r["mode"] == "dynamic" and r["output_bits"] is None and not [k for k in r if k.startswith("final") or k == "fused_activation"]
  assert got["fc2/y"]["output_bits"] == 8 and got["fc2/y"]["fused_activation"] == "RELU6"


def test_validate_layer_execution_passes_the_keyword_on_and_saves(models, monkeypatch, tmp_path):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  from mi355q.utils import tflite_flatbuffer
  ref, samples, tgt8, _ = models
  qz = quantizer.Quantizer(ref)
  qz._result = quantizer.QuantizationResult([{}], bytearray(tflite_flatbuffer.write_model(tgt8)))      # pylint: disable=protected-access
  monkeypatch.setattr(mv, "LayerExecutionKernels", OC.numpy_kernels())
  plain = qz.validate_layer_execution(samples)
  assert all("output_bits" not in r for r in plain.results.values()) and len(plain) == 4
  got = qz.validate_layer_execution({"serving_default": samples}, save_folder=str(tmp_path), model_name="out",
                                    quantized_outputs=True)
  want = mv.compare_layer_execution(ref, tgt8, samples, kernels=OC.numpy_kernels()(), quantized_outputs=True)
  assert got.skipped == {} and len(got) == 4
  for y, r in want.results.items():
    assert got[y]["final_error"] == r["final_error"] and got[y]["fused_activation"] == r["fused_activation"]
    assert got[y]["error"] == plain[y]["error"]
  saved = json.load(open(tmp_path / "out_layer_execution_errors.json"))
  assert {y: e["fused_activation"] for y, e in saved["layers"].items()} == {f"{n}/y": OC.NAMES[f] for n, _, f, _ in OC.OPS}
  assert all("final_per_channel_error" not in e and e["output_bits"] == 8 for e in saved["layers"].values())


# ---------------------------------------------------------------- the kernels' build
def test_qfc_out_is_built():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "qfc_out.hip" in g.SOURCES and "qfc_frag.h" in g.HEADERS


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_qfc_out_kernels_use_no_scratch_and_the_int8_matrix_cores(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path / "qfc_out.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "qfc_out.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  names = " ".join(kernels)
  for k in ("weight_sums_kernel", "qfc_out_mfma_kernel", "qfc_out16_mfma_kernel", "qfc_out_generic_kernel",
            "qfc_out16_generic_kernel"):
    assert k in names, k
  assert sum("qfc_out_mfma_kernel" in k for k in kernels) == 3 and sum("qfc_out16_mfma_kernel" in k for k in kernels) == 3
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
  text = {}
  for k in kernels:
    found = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(k), asm, re.M | re.S)
    assert found, k
    text[k] = found.group(1)
  for k in kernels:
    if "mfma_kernel" not in k:
      assert "v_mfma" not in text[k], k
    else:
      assert "v_mfma_i32_16x16x64_i8" in text[k] and "v_mfma_i32_16x16x32_i8" not in text[k], k
      # the epilogue stores the requantized tile only: bytes or shorts, never a dword of accumulator or a float
      stores = set(re.findall(r"\b(global_store_\w+|flat_store_\w+|buffer_store_\w+)", text[k]))
      assert stores and stores <= ({"global_store_byte"} if "out_mfma" in k else {"global_store_short"}), (k, stores)
    if "qfc_out16_mfma_kernel" in k:
      assert "v_perm_b32" in text[k], k
  # waves per SIMD as the compiler reports them: what the kernels had before csrc/qfc_tile.h
  # (profiles/qfc_unify_isa.txt)
  for k in kernels:
    if "mfma_kernel" in k:
      occ = re.search(r"^%s:.*?;\s*Occupancy:\s*(\d+)" % re.escape(k), asm, re.M | re.S)
      assert occ and int(occ.group(1)) >= 3, (k, occ and occ.group(1))
