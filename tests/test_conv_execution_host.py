"""CPU checks of the integer execution of quantized CONV_2D ops: mi355q_conv_patches_nhwc is declared, exported, bound
and refuses bad arguments before any launch; ops.conv_geometry against hand-derived values; the NumPy gather of
tests/conv_execution_cases.py followed by a matrix product equals an independent direct convolution exactly; the
Conv2DOptions reader on the golden models and on hand-made tables; model_validator.compare_layer_execution with
`conv_2d` and NumPy kernels, with the keyword off (nothing changes) and on (every mode, every new key, every new skip
reason); csrc/conv_patches.hip is built and compiles for gfx950 without scratch."""
import copy
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import conv_execution_cases as CC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
MODELS = os.path.join(ROOT, "tests", "golden", "models")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOL = "mi355q_conv_patches_nhwc"


@pytest.fixture(scope="module")
def lib():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


# ---------------------------------------------------------------- the ABI
def test_the_symbol_is_declared_exported_and_bound(lib):
  from mi355q import _ffi
  from mi355q import model_validator as mv
  from mi355q import ops
  header = open(os.path.join(ROOT, "include", "mi355q.h")).read()
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  assert re.search(r"\b%s\s*\(" % SYMBOL, header)
  assert SYMBOL in _ffi.PROTOTYPES and hasattr(lib, SYMBOL)
  declared = re.search(r"%s\s*\(([^)]*)\)" % SYMBOL, header).group(1)
  assert len(_ffi.PROTOTYPES[SYMBOL][1]) == len(declared.split(",")) == 21
  assert callable(ops.conv_geometry) and callable(ops.conv_patches)
  for method in ("sample4d", "patches", "quantize_dynamic_images"):
    assert callable(getattr(mv.LayerExecutionKernels, method)), method
  import __graft_entry__ as g
  assert "conv_patches.hip" in g.SOURCES


def test_refusals_come_before_any_launch(lib):
  CC.check_patch_refusals(lib)


# ---------------------------------------------------------------- geometry
def test_conv_geometry_hand_derived(lib):
  from mi355q import ops
  # SAME 3x3 stride 1 on 9 x 11: out = in, total pad 2 (even), 1 before
  assert ops.conv_geometry(9, 11, 3, 3, 1, 1, "SAME") == (9, 11, 1, 1)
  # SAME 3x3 stride 2 on 8 x 8: out 4, total = 3 * 2 + 3 - 8 = 1 (odd): 0 before, the extra row after
  assert ops.conv_geometry(8, 8, 3, 3, 2, 1, "SAME") == (4, 4, 0, 0)
  # SAME 2x5 stride 1 on 5 x 7: totals 1 and 4: 0 and 2 before
  assert ops.conv_geometry(5, 7, 2, 5, (1, 1), (1, 1), "SAME") == (5, 7, 0, 2)
  # SAME 4x4 stride (3, 2) on 10 x 9: out 4 and 5; totals 9 + 4 - 10 = 3 and 8 + 4 - 9 = 3: 1 before each (2 after)
  assert ops.conv_geometry(10, 9, 4, 4, (3, 2), 1, "SAME") == (4, 5, 1, 1)
  # dilation 2: eff = 5; SAME stride 1 on 9 x 11 pads 2 before; VALID gives 5 x 7
  assert ops.conv_geometry(9, 11, 3, 3, 1, 2, "SAME") == (9, 11, 2, 2)
  assert ops.conv_geometry(9, 11, 3, 3, 1, (2, 2), "VALID") == (5, 7, 0, 0)
  # VALID 5x5 stride 2 on 9 x 11: (9 + 2 - 5) // 2 = 3, (11 + 2 - 5) // 2 = 4
  assert ops.conv_geometry(9, 11, 5, 5, 2, 1, "VALID") == (3, 4, 0, 0)
  # a kernel larger than the image: SAME keeps it (7x7 on 1 x 1: total 6, 3 before), VALID has no output
  assert ops.conv_geometry(1, 1, 7, 7, 1, 1, "SAME") == (1, 1, 3, 3)
  assert ops.conv_geometry(28, 28, 3, 3, 1, 1, 0) == (28, 28, 1, 1) and ops.conv_geometry(28, 28, 3, 3, 1, 1, 1) == (26, 26, 0, 0)
  for bad in (dict(h=1, w=1, kh=7, kw=7, stride=1, dilation=1, padding="VALID"),
              dict(h=4, w=4, kh=3, kw=3, stride=1, dilation=2, padding="VALID"),
              dict(h=4, w=4, kh=3, kw=3, stride=0, dilation=1, padding="SAME"),
              dict(h=4, w=4, kh=3, kw=3, stride=1, dilation=(1, 0), padding="SAME"),
              dict(h=0, w=4, kh=3, kw=3, stride=1, dilation=1, padding="SAME"),
              dict(h=4, w=4, kh=3, kw=3, stride=1, dilation=1, padding="FULL"),
              dict(h=4, w=4, kh=3, kw=3, stride=1, dilation=1, padding=2)):
    with pytest.raises(ValueError):
      ops.conv_geometry(**bad)
  for n, h, w, k, s, dil, padding in CC.geometries():
    assert ops.conv_geometry(h, w, k[0], k[1], s, dil, padding) == CC.geometry(h, w, k[0], k[1], s, dil, padding)


# ---------------------------------------------------------------- the statement against the convolution itself
def test_gather_then_product_is_the_direct_convolution_for_every_case():
  """Full-range integers, the extremes planted in the corners (border patches), zero points at the ends of int8: the
  patch rows padded with the zero point, times the filter viewed [O, K], are exactly the direct convolution."""
  cases = CC.geometries()
  assert len(cases) > 300 and any(k[0] > h for _, h, _, k, *_ in cases)
  for i, (n, h, w, k, s, dil, padding) in enumerate(cases):
    rng = np.random.default_rng(i)
    c, o = (1, 3, 4)[i % 3], (1, 5)[i % 2]
    zp = (0, -128, 127, 5)[i % 4]
    for dtype, lo, hi, zero in ((np.int8, -128, 127, zp), (np.int16, -32768, 32767, 0)):
      x = rng.integers(lo, hi, size=(n, h, w, c), endpoint=True).astype(dtype)
      x[:, 0, 0, :], x[:, -1, -1, :] = lo, hi
      qw = rng.integers(-128, 127, size=(o, k[0], k[1], c), endpoint=True)
      qw[0, 0, 0, :], qw[-1, -1, -1, :] = -128, 127
      rows = CC.gather(x, k[0], k[1], s, dil, padding, zero)
      oh, ow, _, _ = CC.geometry(h, w, k[0], k[1], s, dil, padding)
      assert rows.shape == (n * oh * ow, k[0] * k[1] * c) and rows.dtype == dtype
      acc = (rows.astype(np.int64) - zero) @ qw.reshape(o, -1).astype(np.int64).T
      assert np.array_equal(acc, CC.direct_conv(x, zero, qw, s, dil, padding)), (i, dtype)
      for first, count in CC.windows(rows.shape[0], oh * ow):
        assert CC.same_bytes(CC.gather(x, k[0], k[1], s, dil, padding, zero, first, count), rows[first:first + count])


# ---------------------------------------------------------------- the options reader
def _conv_ops(model):
  from mi355q import model_validator as mv
  m = mv._as_model(model)      # pylint: disable=protected-access
  return [op for op, *_ in mv._conv_2d_ops(m, 0)], m      # pylint: disable=protected-access


@pytest.mark.parametrize("name,count", [("conv_fc_mnist.tflite", 1), ("conv_fc_mnist_srq_a8w8.tflite", 1),
                                        ("branching_conv_fc.tflite", None)])
def test_options_reader_on_the_golden_models(lib, name, count):
  from mi355q import model_validator as mv
  from mi355q.utils import tflite_flatbuffer as fb
  convs, m = _conv_ops(open(os.path.join(MODELS, name), "rb").read())
  assert convs and (count is None or len(convs) == count)
  for op in convs:
    assert isinstance(op.builtinOptions, fb.OpaqueTableT) and op.builtinOptionsType == 1
    got = mv.conv_2d_options(op)
    assert sorted(got) == ["dilation_h_factor", "dilation_w_factor", "fused_activation_function", "padding", "stride_h", "stride_w"]
    assert got["padding"] in (0, 1) and got["stride_h"] >= 1 and got["stride_w"] >= 1
    assert got["dilation_h_factor"] >= 1 and got["dilation_w_factor"] >= 1 and got["fused_activation_function"] in OC.NAMES
    # what _fc_option's getattr made of the opaque table: always 0
    assert mv._fc_option(op, "fusedActivationFunction") == 0      # pylint: disable=protected-access
    assert mv._conv_option(op, "fusedActivationFunction") == got["fused_activation_function"]      # pylint: disable=protected-access
    assert mv._conv_option(op, "weightsFormat") == 0      # pylint: disable=protected-access
  # all three were converted from Keras Conv2D(3x3, padding="same", activation="relu") layers
  assert mv.conv_2d_options(convs[0]) == dict(padding=0, stride_w=1, stride_h=1, fused_activation_function=OC.RELU,
                                              dilation_w_factor=1, dilation_h_factor=1)


def test_options_reader_on_hand_made_tables(lib):
  from mi355q import model_validator as mv
  from mi355q import qtyping as q

  def read(table, options_type=1):
    return mv.conv_2d_options(q.OperatorT(inputs=[0, 1], outputs=[2], opcodeIndex=0, builtinOptionsType=options_type,
                                          builtinOptions=table))
  full = CC.conv_options_table(1, 2, 3, OC.RELU6, 4, 5)
  assert read(full) == dict(padding=1, stride_w=2, stride_h=3, fused_activation_function=3, dilation_w_factor=4,
                            dilation_h_factor=5)
  # absent fields take the schema's defaults: 0, and 1 for the dilations
  assert read(CC.conv_options_table()) == dict(padding=0, stride_w=0, stride_h=0, fused_activation_function=0,
                                               dilation_w_factor=1, dilation_h_factor=1)
  assert read(CC.conv_options_table(stride_w=2, stride_h=2)) == dict(padding=0, stride_w=2, stride_h=2, fused_activation_function=0,
                                                                     dilation_w_factor=1, dilation_h_factor=1)
  assert read(CC.conv_options_table(padding=1, dilation_h=2))["dilation_h_factor"] == 2
  assert read(CC.conv_options_table(padding=1, dilation_h=2))["dilation_w_factor"] == 1
  assert read(CC.conv_options_table(fused=-3))["fused_activation_function"] == -3
  assert read(None, 0) == read(CC.conv_options_table())
  assert read(full, 8) is None                          # the options of another op type
  assert read(q.FullyConnectedOptionsT(), 8) is None

  class Decoded:      # the generated object API's names, should the reader ever decode the table
    padding, strideW, strideH, fusedActivationFunction, dilationWFactor, dilationHFactor = 1, 2, 3, 1, None, 2
  assert read(Decoded()) == dict(padding=1, stride_w=2, stride_h=3, fused_activation_function=1, dilation_w_factor=1,
                                 dilation_h_factor=2)
  # a table survives the writer and the reader
  from mi355q.utils import tflite_flatbuffer as fb
  model = CC.build_model()
  again = fb.read_model(bytes(fb.write_model(model)))
  for a, b in zip(model.subgraphs[0].operators[:3], again.subgraphs[0].operators[:3]):
    assert mv.conv_2d_options(a) == mv.conv_2d_options(b) and mv.conv_2d_options(a)["stride_w"] >= 1
  want = {c[0]: dict(padding=CC.PADDING_CODE[c[6]], stride_w=c[4][1], stride_h=c[4][0], fused_activation_function=c[8],
                     dilation_w_factor=c[5][1], dilation_h_factor=c[5][0]) for c in CC.CONVS}
  for conv, op in zip(CC.CONVS, model.subgraphs[0].operators):
    assert mv.conv_2d_options(op) == want[conv[0]]


# ---------------------------------------------------------------- compare_layer_execution
@pytest.fixture(scope="module")
def models(lib):
  ref = CC.build_model()
  samples = CC.build_samples(ref)
  return dict(ref=ref, samples=samples, static=CC.quantize_by_hand(ref, samples, "static", 8),
              static16=CC.quantize_by_hand(ref, samples, "static", 16), dynamic=CC.quantize_by_hand(ref, samples, "dynamic"),
              weight_only=CC.quantize_by_hand(ref, samples, "weight_only"))


def _tensor(model, name):
  return next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)


def _op(model, name):
  sg = model.subgraphs[0]
  return next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"{name}/y")


def _run(models, key, ref=None, tgt=None, samples=None, **kw):
  from mi355q import model_validator as mv
  kw.setdefault("conv_2d", True)
  return mv.compare_layer_execution(ref or models["ref"], tgt or models[key], models["samples"] if samples is None else samples,
                                    kernels=CC.numpy_kernels()(), **kw)


def _reference(models, key, conv, bits=8):
  """(error, signal, final_error or None, final_signal or None, tokens) of one conv, written out here with the direct
  convolution for the integer product: no patches on the quantized side."""
  name, c, o, k, s, dil, padding, has_bias, fused = conv
  ref, tgt = models["ref"], models[key]
  w_t = _tensor(tgt, f"{name}/w")
  s_w = np.asarray(w_t.quantization.scale, np.float32)
  qw = np.asarray(tgt.buffers[w_t.buffer].data).view(np.int8).reshape(o, k[0], k[1], c)
  sq_d = sq_y = f_d = f_y = 0.0
  tokens = 0
  for sample in models["samples"]:
    x = sample[f"{name}/x"]
    y32 = CC.float_conv(ref, conv, x, np.float32, pre_bias=True)
    n = y32.shape[0]
    if key == "weight_only":
      deq = (qw.reshape(o, -1).astype(np.float32) * s_w[:, None]).astype(np.float32)
      yq = CC.gather(x, k[0], k[1], s, dil, padding, 0.0) @ deq.T
    elif key == "dynamic":
      q, scale = EC.quantize_rows(x.reshape(CC.BATCH, -1))
      acc = CC.direct_conv(q.reshape(x.shape), 0, qw, s, dil, padding)
      sc = np.repeat(scale, n // CC.BATCH)[:, None] * s_w[None, :]
      yq = acc.astype(np.int32).astype(np.float32) * sc
    else:
      x_t, y_t = _tensor(tgt, f"{name}/x"), _tensor(tgt, f"{name}/y")
      s_x, zp_x = np.float32(x_t.quantization.scale[0]), int(x_t.quantization.zeroPoint[0])
      s_y, zp_y = np.float32(y_t.quantization.scale[0]), int(y_t.quantization.zeroPoint[0])
      xq = EC16.quantize_static16(x, s_x) if bits == 16 else EC.quantize_static(x, s_x, zp_x)
      acc = CC.direct_conv(xq, zp_x, qw, s, dil, padding)
      sc = (s_x * s_w)[None, :].astype(np.float32)
      yq = EC16.rescale(acc, np.broadcast_to(sc, acc.shape).copy()) if bits == 16 else acc.astype(np.int32).astype(np.float32) * sc
      # the epilogue of the statement, on the accumulators of the direct convolution (a one-hot product passes them on)
      bias = None
      if has_bias:
        b_t = _tensor(tgt, f"{name}/b")
        bias = np.asarray(tgt.buffers[b_t.buffer].data).view(np.int64 if bits == 16 else np.int32)
      ms = [OC.quantize_multiplier(float(s_x) * float(v) / float(s_y)) for v in s_w.tolist()]
      lo, hi = OC.activation_range(fused, float(s_y), zp_y, bits)
      b = [0] * o if bias is None else [int(v) for v in bias]
      if bits == 16:
        q_out = [[min(max(OC.mbqm64(min(max(a + b[r], OC.A16_MIN), OC.A16_MAX), ms[r][0], ms[r][1]), lo), hi)
                  for r, a in enumerate(row)] for row in acc.tolist()]
      else:
        q_out = [[min(max(OC.mbqm32(OC.sat32(a + b[r]), ms[r][0], ms[r][1]) + zp_y, lo), hi) for r, a in enumerate(row)]
                 for row in acc.tolist()]
      yf = ((np.array(q_out, np.int32) - zp_y).astype(np.float32) * s_y).astype(np.float64)
      y_act = CC.float_conv(ref, conv, x, np.float32).astype(np.float64)
      f_d += ((yf - y_act) ** 2).sum()
      f_y += (y_act ** 2).sum()
    sq_d += ((yq.astype(np.float64) - y32.astype(np.float64)) ** 2).sum()
    sq_y += (y32.astype(np.float64) ** 2).sum()
    tokens += n
  final = (f_d / tokens, f_y / tokens) if key.startswith("static") else (None, None)
  return sq_d / tokens, sq_y / tokens, final[0], final[1], tokens


def test_with_the_keyword_off_results_and_saved_json_are_what_they_were(models, tmp_path):
  from mi355q import model_validator as mv
  for key in ("static", "dynamic", "weight_only"):
    for kw in (dict(), dict(int16_activations=True, quantized_outputs=True), dict(follow_input_transforms=True)):
      old = mv.compare_layer_execution(models["ref"], models[key], models["samples"], kernels=OC.numpy_kernels()(), **kw)
      off = _run(models, key, conv_2d=False, **kw)
      assert list(old) == list(off) == ["fc/y"] and old.skipped == off.skipped == {}
      assert sorted(old["fc/y"]) == sorted(off["fc/y"]) and "op" not in off["fc/y"]
      for k, v in old["fc/y"].items():
        assert np.array_equal(off["fc/y"][k], v), (key, k)
      a = open(old.save(str(tmp_path / "old"), "m"), "rb").read()
      b = open(off.save(str(tmp_path / "off"), "m"), "rb").read()
      assert a == b and b"CONV_2D" not in a and b"kernel" not in a
      on = _run(models, key, **kw)      # the FC entry's other keys do not move when the keyword is on
      assert on["fc/y"]["op"] == "FULLY_CONNECTED" and sorted(on["fc/y"]) == sorted(list(old["fc/y"]) + ["op"])
      for k, v in old["fc/y"].items():
        assert np.array_equal(on["fc/y"][k], v), (key, k)


@pytest.mark.parametrize("key", ["static", "static16", "dynamic", "weight_only"])
def test_with_the_keyword_on_every_conv_is_reported_in_every_mode(models, key, tmp_path):
  bits = 16 if key == "static16" else 8
  got = _run(models, key, int16_activations=True, quantized_outputs=True)
  assert got.skipped == {} and list(got) == ["fc/y"] + [f"{c[0]}/y" for c in CC.CONVS]
  mode = {"static": "static", "static16": "static", "dynamic": "dynamic", "weight_only": "weight_only"}[key]
  for conv in CC.CONVS:
    name, c, o, k, s, dil, padding, has_bias, fused = conv
    r = got[f"{name}/y"]
    error, signal, f_error, f_signal, tokens = _reference(models, key, conv, bits)
    oh, ow, _, _ = CC.geometry(CC.HEIGHT, CC.WIDTH, k[0], k[1], s, dil, padding)
    assert (r["op"], r["weight"], r["input"], r["mode"]) == ("CONV_2D", f"{name}/w", f"{name}/x", mode)
    assert (r["rows"], r["d"], r["tokens"]) == (o, k[0] * k[1] * c, CC.SAMPLES * CC.BATCH * oh * ow) and tokens == r["tokens"]
    assert (r["kernel"], r["strides"], r["dilations"], r["padding"], r["output_hw"]) == (list(k), list(s), list(dil), padding, [oh, ow])
    np.testing.assert_allclose([r["error"], r["signal"]], [error, signal], rtol=1e-12)
    assert r["per_channel_error"].shape == (o,) and r["per_channel_error"].dtype == np.float64
    np.testing.assert_allclose(r["error"], r["per_channel_error"].sum(), rtol=1e-12)
    assert r["output_mse"] == r["error"] / o and r["output_snr"] == (r["signal"] / o) / (r["output_mse"] + 1e-9)
    assert 0 < r["error"] < 1e-2 * r["signal"]
    if mode == "static":
      assert r["activation_bits"] == r["output_bits"] == bits and r["fused_activation"] == OC.NAMES[fused]
      assert "final_skipped" not in r
      np.testing.assert_allclose([r["final_error"], r["final_signal"]], [f_error, f_signal], rtol=1e-12)
      assert r["final_per_channel_error"].shape == (o,) and 0 < r["final_error"] < r["final_signal"]
      assert r["final_output_mse"] == r["final_error"] / o
    else:
      assert r["activation_bits"] is None and r["output_bits"] is None
      assert not [x for x in r if x.startswith("final") or x == "fused_activation"]
  saved = json.load(open(got.save(str(tmp_path), "m")))
  entry = saved["layers"]["convC/y"]
  assert entry["op"] == "CONV_2D" and entry["kernel"] == [3, 3] and entry["dilations"] == [2, 2] and entry["padding"] == "SAME"
  assert entry["strides"] == [1, 1] and entry["output_hw"] == [9, 11] and "per_channel_error" not in entry
  assert saved["layers"]["fc/y"]["op"] == "FULLY_CONNECTED"
  plain = _run(models, key, int16_activations=True)      # without quantized_outputs: the pre-bias figures alone
  for y in got:
    assert not [x for x in plain[y] if x.startswith("final") or x in ("output_bits", "fused_activation")]
    assert plain[y]["error"] == got[y]["error"]
  if key == "static16":
    assert _run(models, key).skipped == {f"{n}/y": "the op reads an INT16 activation" for n in ("fc", "convA", "convB", "convC")}


def test_static_patches_of_the_integer_tensor_are_the_quantized_float_patches(models):
  """The pad identity the static mode rests on, in NumPy: q(0.0) = zp_x."""
  rng = np.random.default_rng(3)
  x = rng.standard_normal((2, 5, 7, 3)).astype(np.float32)
  for zp in (-128, 5, 127):
    a = CC.gather(EC.quantize_static(x, 0.05, zp), 3, 3, (2, 1), (1, 2), CC.SAME, zp)
    b = EC.quantize_static(CC.gather(x, 3, 3, (2, 1), (1, 2), CC.SAME, 0.0), 0.05, zp)
    assert CC.same_bytes(a, b) and (a == zp).sum() > 50
  a = CC.gather(EC16.quantize_static16(x, 0.0005), 3, 3, (2, 1), (1, 2), CC.SAME, 0)
  assert CC.same_bytes(a, EC16.quantize_static16(CC.gather(x, 3, 3, (2, 1), (1, 2), CC.SAME, 0.0), 0.0005))


def test_every_new_skip_reason(models):
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  ref, tgt, samples = models["ref"], models["static"], models["samples"]
  # the filter: rank 3; not a constant; float16
  r2 = copy.deepcopy(ref)
  _tensor(r2, "convA/w").shape = [24, 9, 16]
  _tensor(r2, "convB/w").buffer = 0
  _tensor(r2, "convC/w").type = int(q.TensorType.FLOAT16)
  got = _run(models, "static", ref=r2)
  assert got.skipped == {f"{n}/y": mv.SKIP_CONV_FILTER for n in ("convA", "convB", "convC")} and list(got) == ["fc/y"]
  # grouped: the sample has twice the filter's input channels; a sample that is not rank 4
  doubled = [dict(s, **{"convA/x": np.concatenate([s["convA/x"]] * 2, axis=3), "convB/x": s["convB/x"].reshape(2, 9, 33)})
             for s in samples]
  got = _run(models, "static", samples=doubled)
  assert got.skipped == {"convA/y": mv.SKIP_CONV_GROUPS, "convB/y": mv.SKIP_SAMPLE_SHAPE} and "convC/y" in got
  # options: a stride of 0, a dilation of 0, an unknown padding (each in both models, as a converter would write them)
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):
    _op(model, "convA").builtinOptions = CC.conv_options_table(None, 0, 1, 1)
    _op(model, "convB").builtinOptions = CC.conv_options_table(1, 2, 2, None, 1, 0)
    _op(model, "convC").builtinOptions = CC.conv_options_table(2, 1, 1, 3, 2, 2)
  got = _run(models, "static", ref=r2, tgt=t2)
  assert got.skipped == {f"{n}/y": mv.SKIP_CONV_OPTIONS for n in ("convA", "convB", "convC")}
  t2 = copy.deepcopy(tgt)      # the two models disagree about the geometry
  _op(t2, "convA").builtinOptions = CC.conv_options_table(None, 2, 2, 1)
  _op(t2, "convB").builtinOptionsType = 8      # (the options of another op type)
  got = _run(models, "static", tgt=t2)
  assert got.skipped == {"convA/y": mv.SKIP_CONV_OPTIONS, "convB/y": mv.SKIP_CONV_OPTIONS}
  # geometry: VALID 5x5 on a 4 x 4 image has no output; K above 65536
  small = [dict(s, **{"convB/x": s["convB/x"][:, :4, :4, :]}) for s in samples]
  got = _run(models, "static", samples=small)
  assert got.skipped == {"convB/y": mv.SKIP_CONV_GEOMETRY}
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model, dtype in ((r2, np.float32), (t2, np.int8)):
    w = _tensor(model, "convB/w")
    w.shape = [1, 5, 5, 2622]      # K = 65550
    model.buffers[w.buffer].data = np.zeros(65550, dtype).view(np.uint8)
  _tensor(t2, "convB/w").quantization.scale = np.ones(1, np.float32)
  _tensor(t2, "convB/w").quantization.zeroPoint = np.zeros(1, np.int64)
  wide = [dict(s, **{"convB/x": np.zeros((1, 9, 11, 2622), np.float32)}) for s in samples]
  got = _run(models, "static", ref=r2, tgt=t2, samples=wide)
  assert got.skipped == {"convB/y": mv.SKIP_CONV_GEOMETRY}
  # blockwise scales
  t2 = copy.deepcopy(models["dynamic"])
  w = _tensor(t2, "convA/w")
  sg = t2.subgraphs[0]
  t2.buffers.append(q.BufferT(data=np.ones(24 * 144 // 32, np.float16).view(np.uint8)))
  sg.tensors.append(q.TensorT(name=b"convA/w_scales", shape=[24, 144 // 32], buffer=len(t2.buffers) - 1,
                              type=int(q.TensorType.FLOAT16)))
  w.quantization = q.QuantizationParametersT(detailsType=2, details=q.BlockwiseQuantizationT(
      scales=len(sg.tensors) - 1, blockSize=32))
  got = _run(models, "dynamic", tgt=t2)
  assert got.skipped == {"convA/y": mv.SKIP_CONV_BLOCKWISE} and got["convB/y"]["mode"] == "dynamic"
  # the reasons FULLY_CONNECTED has hold for a conv too: a transformed input, per-channel scales along dimension 3
  t2 = copy.deepcopy(models["dynamic"])
  _tensor(t2, "convA/x").name = b"convA/x_rotated"
  _tensor(t2, "convB/w").quantization.quantizedDimension = 3
  _tensor(t2, "convB/w").quantization.scale = np.ones(3, np.float32)
  _tensor(t2, "convB/w").quantization.zeroPoint = np.zeros(3, np.int64)
  got = _run(models, "dynamic", tgt=t2, follow_input_transforms=True)
  assert got.skipped == {"convA/y": mv.SKIP_INPUT, "convB/y": mv.SKIP_TARGET}
  assert got["convC/y"]["input_transform"] == "none" and got["convC/y"]["hadamard_size"] == 0
  # and no sample at all
  got = _run(models, "static", samples=[{k: v for k, v in s.items() if k != "convC/x"} for s in samples])
  assert got.skipped == {"convC/y": mv.SKIP_NO_SAMPLE}


def test_validate_layer_execution_passes_the_keyword_on(models, monkeypatch, tmp_path):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  from mi355q.utils import tflite_flatbuffer
  qz = quantizer.Quantizer(models["ref"])
  qz._result = quantizer.QuantizationResult([{}], bytearray(tflite_flatbuffer.write_model(models["static"])))      # pylint: disable=protected-access
  monkeypatch.setattr(mv, "LayerExecutionKernels", CC.numpy_kernels())
  plain = qz.validate_layer_execution(models["samples"])
  assert list(plain) == ["fc/y"] and not plain.skipped and "op" not in plain["fc/y"]
  got = qz.validate_layer_execution({"serving_default": models["samples"]}, save_folder=str(tmp_path), model_name="out",
                                    quantized_outputs=True, conv_2d=True)
  want = _run(models, "static", quantized_outputs=True)
  assert got.skipped == {} and list(got) == list(want) and len(got) == 4
  for y, r in want.results.items():
    assert got[y]["final_error"] == r["final_error"] and got[y]["op"] == r["op"]
  saved = json.load(open(tmp_path / "out_layer_execution_errors.json"))
  assert {y: e["op"] for y, e in saved["layers"].items()} == {"fc/y": "FULLY_CONNECTED", "convA/y": "CONV_2D",
                                                             "convB/y": "CONV_2D", "convC/y": "CONV_2D"}


# ---------------------------------------------------------------- the kernel's build
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_conv_patches_kernels_use_no_scratch(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path / "conv_patches.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "conv_patches.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  # the vector route (16-byte units) and the generic one (1, 2 and 4 bytes), each with a 32-bit and a 64-bit unit index
  assert len(kernels) == 8 and all("conv_patches_kernel" in k for k in kernels), kernels
  assert sum("HIP_vector_type" in k for k in kernels) == 2
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == 8 and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
  assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)\S*\s.*\boffen\b", asm)
  vgprs = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", asm)]
  assert len(vgprs) == 8 and max(vgprs) <= 32, vgprs
  for k in kernels:      # one 16-byte load and one 16-byte store per lane on the vector route
    body = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(k), asm, re.M | re.S).group(1)
    if "HIP_vector_type" in k:
      assert len(re.findall(r"global_load_dwordx4", body)) == 1 and len(re.findall(r"global_store_dwordx4", body)) == 1, k
