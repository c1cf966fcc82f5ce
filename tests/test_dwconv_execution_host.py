"""CPU checks of the integer execution of quantized DEPTHWISE_CONV_2D ops: the five mi355q_dwconv_* entries are
declared, exported, bound and refuse bad arguments before any launch; the two NumPy statements of
tests/dwconv_execution_cases.py agree with each other and with the CONV_2D statements where a depthwise convolution
is one; the DepthwiseConv2DOptions reader on hand-made tables; model_validator.compare_layer_execution with
`depthwise_conv_2d` and NumPy kernels, with the keyword off (nothing changes) and on (every mode, both activation
widths, every new key, every new skip reason); csrc/dwconv.hip is built and compiles for gfx950 without scratch."""
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
import dwconv_execution_cases as DW
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def lib():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


# ---------------------------------------------------------------- the ABI
def test_the_symbols_are_declared_exported_and_bound(lib):
  from mi355q import _ffi
  from mi355q import model_validator as mv
  from mi355q import ops
  header = open(os.path.join(ROOT, "include", "mi355q.h")).read()
  assert "Direct depthwise convolution (csrc/dwconv.hip)" in header
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  for symbol in DW.ENTRIES:
    assert re.search(r"\b%s\s*\(" % symbol, header), symbol
    assert symbol in _ffi.PROTOTYPES and hasattr(lib, symbol), symbol
    declared = re.search(r"%s\s*\(([^)]*)\)" % symbol, header).group(1)
    assert len(_ffi.PROTOTYPES[symbol][1]) == len(declared.split(",")) == DW.ARGUMENT_COUNTS[symbol], symbol
  assert DW.I8 == ops.COMPARE_KINDS["i8"]
  assert callable(ops.dwconv_forward) and callable(ops.dwconv_output) and callable(ops.dwconv_output_i16)
  for method in ("depthwise_float", "depthwise_forward", "depthwise_forward16", "depthwise_output", "depthwise_output16"):
    assert callable(getattr(mv.LayerExecutionKernels, method)), method
  import __graft_entry__ as g
  assert "dwconv.hip" in g.SOURCES and "qfc_epilogue.h" in g.HEADERS      # (the shared epilogue is part of both fingerprints)
  for source in ("qfc_out.hip", "dwconv.hip"):      # one piece of epilogue code, included by both
    text = open(os.path.join(CSRC, source)).read()
    assert '#include "qfc_epilogue.h"' in text and "struct Chan8" not in text and "output16(long long acc" not in text, source


def test_refusals_come_before_any_launch(lib):
  DW.check_depthwise_refusals(lib)


# ---------------------------------------------------------------- the statements against each other
def test_the_two_statements_agree_where_both_are_exact():
  """Small integers make every float32 product and sum exact, so the float loop (array operations per tap) and the
  integer convolution (one pixel and one tap at a time) must give the same numbers; with M = 1 and one channel both
  are the CONV_2D statements of conv_execution_cases, and every window is a slice of the whole."""
  cases = CC.geometries()
  assert len(cases) > 300 and any(k[0] > h for _, h, _, k, *_ in cases)
  for i, (n, h, w, k, s, dil, padding) in enumerate(cases):
    rng = np.random.default_rng(i)
    c, mult = ((4, 1), (3, 2), (1, 1), (5, 3))[i % 4]
    o = c * mult
    x = rng.integers(-128, 127, size=(n, h, w, c), endpoint=True).astype(np.int8)
    x[:, 0, 0, :], x[:, -1, -1, :] = -128, 127
    qw = rng.integers(-128, 127, size=(k[0], k[1], o), endpoint=True)
    qw[0, 0, :], qw[-1, -1, :] = -128, 127
    zp = (0, -128, 127, 5)[i % 4]
    acc = DW.direct_depthwise(x, zp, qw, mult, s, dil, padding)
    oh, ow, _, _ = CC.geometry(h, w, k[0], k[1], s, dil, padding)
    assert acc.shape == (n * oh * ow, o) and acc.dtype == np.int64
    assert np.abs(acc).max() < 1 << 24      # (49 taps of at most 255 * 128: exact in float32)
    y = DW.float_depthwise(x.astype(np.float32) - np.float32(zp), qw.astype(np.float32), mult, s, dil, padding)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.int64), acc), i
    for first, count in CC.windows(acc.shape[0], oh * ow):
      part = DW.float_depthwise(x.astype(np.float32) - np.float32(zp), qw.astype(np.float32), mult, s, dil, padding, first, count)
      assert CC.same_bytes(part, y[first:first + count])
    if (c, mult) == (1, 1):      # a depthwise convolution of one channel is a CONV_2D with O = I = 1
      assert np.array_equal(acc, CC.direct_conv(x, zp, qw.reshape(1, k[0], k[1], 1), s, dil, padding))
    for ch in range(o):      # every output channel is the CONV_2D of its one input channel
      if i % 7 == 0:
        one = CC.direct_conv(x[..., ch // mult:ch // mult + 1], zp, qw[:, :, ch].reshape(1, k[0], k[1], 1), s, dil, padding)
        assert np.array_equal(acc[:, ch:ch + 1], one), (i, ch)


def test_the_float_statement_is_the_scalar_loop():
  """Element by element, in Python: y = ((0 + p_0) + p_1) ..., np.float32 scalars, taps outside skipped; -0.0, inf."""
  rng = np.random.default_rng(5)
  n, h, w, c, mult, k, s, dil, padding = 2, 4, 5, 3, 2, (3, 2), (2, 1), (1, 2), CC.SAME
  x = rng.standard_normal((n, h, w, c)).astype(np.float32)
  x[0, 0, 0, 0], x[1, 2, 3, 1], x[0, 3, 4, 2] = -0.0, np.inf, 0.0
  wt = rng.standard_normal((k[0], k[1], c * mult)).astype(np.float32)
  oh_n, ow_n, top, left = CC.geometry(h, w, k[0], k[1], s, dil, padding)
  want = np.zeros((n, oh_n, ow_n, c * mult), np.float32)
  with np.errstate(invalid="ignore"):
    for b in range(n):
      for oh in range(oh_n):
        for ow in range(ow_n):
          for oc in range(c * mult):
            acc = np.float32(0)
            for i in range(k[0]):
              for j in range(k[1]):
                ih, iw = oh * s[0] - top + i * dil[0], ow * s[1] - left + j * dil[1]
                if 0 <= ih < h and 0 <= iw < w:
                  acc = np.float32(acc + np.float32(x[b, ih, iw, oc // mult] * wt[i, j, oc]))
            want[b, oh, ow, oc] = acc
  got = DW.float_depthwise(x, wt, mult, s, dil, padding)
  assert np.isinf(want).any() and EC.same_bits(got, want.reshape(-1, c * mult))


# ---------------------------------------------------------------- the options reader
def test_options_reader_on_hand_made_tables(lib):
  from mi355q import model_validator as mv
  from mi355q import qtyping as q

  def read(table, options_type=2):
    return mv.depthwise_conv_2d_options(q.OperatorT(inputs=[0, 1], outputs=[2], opcodeIndex=0,
                                                    builtinOptionsType=options_type, builtinOptions=table))
  full = DW.depthwise_options_table(1, 2, 3, 4, OC.RELU6, 5, 6)
  assert read(full) == dict(padding=1, stride_w=2, stride_h=3, depth_multiplier=4, fused_activation_function=3,
                            dilation_w_factor=5, dilation_h_factor=6)
  # absent fields take the schema's defaults: 0, and 1 for the dilations
  defaults = dict(padding=0, stride_w=0, stride_h=0, depth_multiplier=0, fused_activation_function=0, dilation_w_factor=1,
                  dilation_h_factor=1)
  assert read(DW.depthwise_options_table()) == defaults
  assert read(DW.depthwise_options_table(stride_w=2, stride_h=2)) == dict(defaults, stride_w=2, stride_h=2)
  assert read(DW.depthwise_options_table(depth_multiplier=2)) == dict(defaults, depth_multiplier=2)
  assert read(DW.depthwise_options_table(padding=1, dilation_h=2)) == dict(defaults, padding=1, dilation_h_factor=2)
  assert read(DW.depthwise_options_table(fused=-3))["fused_activation_function"] == -3
  assert read(None, 0) == defaults
  # the options of another op type: Conv2DOptions (type 1, whose field 3 is the fused activation), FullyConnectedOptions
  assert read(CC.conv_options_table(1, 2, 3, OC.RELU6, 4, 5), 1) is None
  assert read(full, 1) is None and read(full, 8) is None
  assert read(q.FullyConnectedOptionsT(), 8) is None
  assert mv.conv_2d_options(q.OperatorT(inputs=[0, 1], outputs=[2], opcodeIndex=0, builtinOptionsType=2, builtinOptions=full)) is None

  class DecodedConv:      # a decoded Conv2DOptions has no depthMultiplier
    padding, strideW, strideH, fusedActivationFunction, dilationWFactor, dilationHFactor = 1, 2, 3, 1, None, 2
  assert read(DecodedConv()) is None

  class Decoded(DecodedConv):      # the generated object API's names
    depthMultiplier = 2
  assert read(Decoded()) == dict(padding=1, stride_w=2, stride_h=3, depth_multiplier=2, fused_activation_function=1,
                                 dilation_w_factor=1, dilation_h_factor=2)
  # a table survives the writer and the reader, and the model's ops read as built
  from mi355q.utils import tflite_flatbuffer as fb
  model = DW.build_model()
  again = fb.read_model(bytes(fb.write_model(model)))
  want = {d[0]: dict(padding=CC.PADDING_CODE[d[6]], stride_w=d[4][1], stride_h=d[4][0], depth_multiplier=0 if d[0] == "dwC" else d[2],
                     fused_activation_function=d[8], dilation_w_factor=d[5][1], dilation_h_factor=d[5][0]) for d in DW.DWS}
  for dw, a, b in zip(DW.DWS, model.subgraphs[0].operators, again.subgraphs[0].operators):
    assert isinstance(b.builtinOptions, fb.OpaqueTableT) and b.builtinOptionsType == 2
    assert mv.depthwise_conv_2d_options(a) == mv.depthwise_conv_2d_options(b) == want[dw[0]]
    assert mv._depthwise_option(a, "fusedActivationFunction") == dw[8]      # pylint: disable=protected-access
    assert mv._depthwise_option(a, "weightsFormat") == 0      # pylint: disable=protected-access
  assert [op is o for (op, *_), o in zip(mv._depthwise_conv_2d_ops(model, 0), model.subgraphs[0].operators)] == [True] * 3      # pylint: disable=protected-access


# ---------------------------------------------------------------- compare_layer_execution
@pytest.fixture(scope="module")
def models(lib):
  ref = DW.build_model()
  samples = DW.build_samples(ref)
  return dict(ref=ref, samples=samples, static=DW.quantize_by_hand(ref, samples, "static", 8),
              static16=DW.quantize_by_hand(ref, samples, "static", 16), dynamic=DW.quantize_by_hand(ref, samples, "dynamic"),
              weight_only=DW.quantize_by_hand(ref, samples, "weight_only"))


@pytest.fixture(scope="module")
def conv_models(lib):
  ref = CC.build_model()
  samples = CC.build_samples(ref)
  return dict(ref=ref, samples=samples, static=CC.quantize_by_hand(ref, samples, "static", 8),
              dynamic=CC.quantize_by_hand(ref, samples, "dynamic"), weight_only=CC.quantize_by_hand(ref, samples, "weight_only"))


def _tensor(model, name):
  return next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)


def _op(model, name):
  sg = model.subgraphs[0]
  return next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"{name}/y")


def _run(models, key, ref=None, tgt=None, samples=None, **kw):
  from mi355q import model_validator as mv
  kw.setdefault("depthwise_conv_2d", True)
  return mv.compare_layer_execution(ref or models["ref"], tgt or models[key], models["samples"] if samples is None else samples,
                                    kernels=DW.numpy_kernels()(), **kw)


def _reference(models, key, dw, bits=8):
  """(error, signal, final_error or None, final_signal or None, tokens) of one op, written out here from the model's own
  tensors: the float loop for Y, the direct integer convolution for the accumulators."""
  name, c, mult, k, s, dil, padding, has_bias, fused = dw
  o = c * mult
  ref, tgt = models["ref"], models[key]
  w_t = _tensor(tgt, f"{name}/w")
  s_w = np.asarray(w_t.quantization.scale, np.float32)
  assert s_w.shape == (o,) and w_t.quantization.quantizedDimension == 3
  qw = np.asarray(tgt.buffers[w_t.buffer].data).view(np.int8).reshape(k[0], k[1], o)
  sq_d = sq_y = f_d = f_y = 0.0
  tokens = 0
  for sample in models["samples"]:
    x = sample[f"{name}/x"]
    y32 = DW.float_op(ref, dw, x, pre_bias=True)
    n = y32.shape[0]
    if key == "weight_only":
      deq = (qw.astype(np.float32) * s_w[None, None, :]).astype(np.float32)
      yq = DW.float_depthwise(x, deq, mult, s, dil, padding)
    elif key == "dynamic":
      q, scale = EC.quantize_rows(x.reshape(DW.BATCH, -1))
      acc = DW.direct_depthwise(q.reshape(x.shape), 0, qw, mult, s, dil, padding)
      sc = np.repeat(scale, n // DW.BATCH)[:, None] * s_w[None, :]
      yq = acc.astype(np.int32).astype(np.float32) * sc
    else:
      x_t, y_t = _tensor(tgt, f"{name}/x"), _tensor(tgt, f"{name}/y")
      s_x, zp_x = np.float32(x_t.quantization.scale[0]), int(x_t.quantization.zeroPoint[0])
      s_y, zp_y = np.float32(y_t.quantization.scale[0]), int(y_t.quantization.zeroPoint[0])
      xq = EC16.quantize_static16(x, s_x) if bits == 16 else EC.quantize_static(x, s_x, zp_x)
      acc = DW.direct_depthwise(xq, zp_x, qw, mult, s, dil, padding)
      sc = np.broadcast_to((s_x * s_w)[None, :].astype(np.float32), acc.shape).copy()
      yq = EC16.rescale(acc, sc) if bits == 16 else acc.astype(np.int32).astype(np.float32) * sc
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
      y_act = DW.float_op(ref, dw, x).astype(np.float64)
      f_d += ((yf - y_act) ** 2).sum()
      f_y += (y_act ** 2).sum()
    sq_d += ((yq.astype(np.float64) - y32.astype(np.float64)) ** 2).sum()
    sq_y += (y32.astype(np.float64) ** 2).sum()
    tokens += n
  final = (f_d / tokens, f_y / tokens) if key.startswith("static") else (None, None)
  return sq_d / tokens, sq_y / tokens, final[0], final[1], tokens


CONV_KEYS = ["d", "dilations", "error", "input", "kernel", "mode", "op", "output_hw", "output_mse", "output_snr", "padding",
             "per_channel_error", "rows", "signal", "strides", "tokens", "weight"]


def test_with_the_keyword_off_results_and_saved_json_are_what_they_were(conv_models, tmp_path):
  """On the CONV_2D test model: not giving the keyword, and giving it as False, with `conv_2d` off and on; the key sets
  of the entries are pinned, so that a key added without the keyword shows."""
  from mi355q import model_validator as mv
  for key in ("static", "dynamic", "weight_only"):
    for conv_2d in (False, True):
      for kw in (dict(), dict(int16_activations=True, quantized_outputs=True), dict(follow_input_transforms=True)):
        args = (conv_models["ref"], conv_models[key], conv_models["samples"])
        old = mv.compare_layer_execution(*args, kernels=CC.numpy_kernels()(), conv_2d=conv_2d, **kw)
        off = mv.compare_layer_execution(*args, kernels=DW.numpy_kernels()(), conv_2d=conv_2d, depthwise_conv_2d=False, **kw)
        assert list(old) == list(off) == (["fc/y"] + [f"{c[0]}/y" for c in CC.CONVS] if conv_2d else ["fc/y"])
        assert old.skipped == off.skipped == {}
        for y in old:
          assert sorted(old[y]) == sorted(off[y]) and ("op" in off[y]) == conv_2d
          assert "depth_multiplier" not in off[y]
          for k, v in old[y].items():
            assert np.array_equal(off[y][k], v), (key, y, k)
        if conv_2d and not kw:
          assert sorted(off["convA/y"]) == CONV_KEYS
          assert sorted(off["fc/y"]) == sorted(set(CONV_KEYS) - {"kernel", "strides", "dilations", "padding", "output_hw"})
        a = open(old.save(str(tmp_path / "old"), "m"), "rb").read()
        b = open(off.save(str(tmp_path / "off"), "m"), "rb").read()
        assert a == b and b"DEPTHWISE" not in a and b"depth_multiplier" not in a
        # with the keyword on, a model without depthwise ops gains nothing but `op` on its entries
        on = mv.compare_layer_execution(*args, kernels=DW.numpy_kernels()(), conv_2d=conv_2d, depthwise_conv_2d=True, **kw)
        assert list(on) == list(old) and on.skipped == {}
        for y in old:
          assert sorted(on[y]) == sorted(set(old[y]) | {"op"})
          assert on[y]["op"] == ("FULLY_CONNECTED" if y == "fc/y" else "CONV_2D")
          for k, v in old[y].items():
            assert np.array_equal(on[y][k], v), (key, y, k)


def test_conv_2d_alone_leaves_the_depthwise_ops_out(models):
  got = _run(models, "static", depthwise_conv_2d=False, conv_2d=True)
  assert list(got) == ["fc/y"] and got.skipped == {} and got["fc/y"]["op"] == "FULLY_CONNECTED"
  plain = _run(models, "static", depthwise_conv_2d=False)
  assert list(plain) == ["fc/y"] and "op" not in plain["fc/y"]


@pytest.mark.parametrize("key", ["static", "static16", "dynamic", "weight_only"])
def test_with_the_keyword_on_every_depthwise_op_is_reported_in_every_mode(models, key, tmp_path):
  bits = 16 if key == "static16" else 8
  got = _run(models, key, int16_activations=True, quantized_outputs=True)
  assert got.skipped == {} and list(got) == ["fc/y"] + [f"{d[0]}/y" for d in DW.DWS]
  mode = {"static": "static", "static16": "static", "dynamic": "dynamic", "weight_only": "weight_only"}[key]
  for dw in DW.DWS:
    name, c, mult, k, s, dil, padding, has_bias, fused = dw
    o = c * mult
    r = got[f"{name}/y"]
    error, signal, f_error, f_signal, tokens = _reference(models, key, dw, bits)
    oh, ow, _, _ = CC.geometry(DW.HEIGHT, DW.WIDTH, k[0], k[1], s, dil, padding)
    assert (r["op"], r["weight"], r["input"], r["mode"]) == ("DEPTHWISE_CONV_2D", f"{name}/w", f"{name}/x", mode)
    assert (r["rows"], r["d"], r["tokens"]) == (o, k[0] * k[1], DW.SAMPLES * DW.BATCH * oh * ow) and tokens == r["tokens"]
    assert (r["kernel"], r["strides"], r["dilations"], r["padding"], r["output_hw"]) == (list(k), list(s), list(dil), padding, [oh, ow])
    assert r["depth_multiplier"] == mult
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
  if key != "static16":      # (the key set with no other keyword: a conv entry's and `depth_multiplier`)
    assert sorted(_run(models, key)["dwA/y"]) == sorted(CONV_KEYS + ["depth_multiplier"])
  saved = json.load(open(got.save(str(tmp_path), "m")))
  entry = saved["layers"]["dwC/y"]
  assert entry["op"] == "DEPTHWISE_CONV_2D" and entry["kernel"] == [3, 3] and entry["dilations"] == [2, 2]
  assert entry["padding"] == "SAME" and entry["strides"] == [1, 1] and entry["output_hw"] == [9, 11]
  assert entry["depth_multiplier"] == 1 and entry["d"] == 9 and "per_channel_error" not in entry
  assert saved["layers"]["dwB/y"]["depth_multiplier"] == 2 and saved["layers"]["dwB/y"]["rows"] == 6
  assert saved["layers"]["fc/y"]["op"] == "FULLY_CONNECTED"
  plain = _run(models, key, int16_activations=True)      # without quantized_outputs: the pre-bias figures alone
  for y in got:
    assert not [x for x in plain[y] if x.startswith("final") or x in ("output_bits", "fused_activation")]
    assert plain[y]["error"] == got[y]["error"]
  if key == "static16":
    assert _run(models, key).skipped == {f"{n}/y": "the op reads an INT16 activation" for n in ("fc", "dwA", "dwB", "dwC")}
  # per-tensor scales: the whole filter on one grid (dwA's channel gains differ by a decade: the weight's error grows)
  if key == "weight_only":
    t2 = copy.deepcopy(models[key])
    w = _tensor(t2, "dwA/w")
    flat = DW.constant(models["ref"], "dwA/w").reshape(-1)
    s_w = np.float32(np.abs(flat).max() / 127.0)
    w.quantization.scale, w.quantization.zeroPoint = np.array([s_w], np.float32), np.zeros(1, np.int64)
    t2.buffers[w.buffer].data = np.clip(np.rint(flat / s_w), -127, 127).astype(np.int8).view(np.uint8)
    one = _run(models, key, tgt=t2)
    assert one.skipped == {} and one["dwA/y"]["mode"] == "weight_only" and one["dwB/y"]["error"] == got["dwB/y"]["error"]
    assert one["dwA/y"]["error"] > 1.5 * got["dwA/y"]["error"]


def test_every_new_skip_reason(models):
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  ref, tgt, samples = models["ref"], models["static"], models["samples"]
  reasons = (mv.SKIP_DEPTHWISE_FILTER, mv.SKIP_DEPTHWISE_MULTIPLIER, mv.SKIP_DEPTHWISE_KIND, mv.SKIP_DEPTHWISE_BLOCKWISE,
             mv.SKIP_DEPTHWISE_SCALE_AXIS, mv.SKIP_DEPTHWISE_MISMATCH)
  known = [v for k, v in vars(mv).items() if k.startswith("SKIP_") and isinstance(v, str)]
  assert len(set(reasons)) == 6 and all(known.count(r) == 1 for r in reasons)      # each its own constant and text
  # the filter: a first dimension that is not 1; not a constant; float16; rank 3
  r2 = copy.deepcopy(ref)
  _tensor(r2, "dwA/w").shape = [16, 3, 3, 1]
  _tensor(r2, "dwB/w").buffer = 0
  _tensor(r2, "dwC/w").type = int(q.TensorType.FLOAT16)
  got = _run(models, "static", ref=r2)
  assert got.skipped == {f"{n}/y": mv.SKIP_DEPTHWISE_FILTER for n in ("dwA", "dwB", "dwC")} and list(got) == ["fc/y"]
  r2 = copy.deepcopy(ref)
  _tensor(r2, "dwA/w").shape = [9, 16, 1]
  assert _run(models, "static", ref=r2).skipped == {"dwA/y": mv.SKIP_DEPTHWISE_FILTER}
  # the multiplier: O = 16 is no multiple of C = 32; a depth_multiplier option (3, in both models) that is not O / C = 2;
  # a sample that is not rank 4 keeps its CONV_2D text
  doubled = [dict(s, **{"dwA/x": np.concatenate([s["dwA/x"]] * 2, axis=3), "dwC/x": s["dwC/x"].reshape(2, 9, 88)}) for s in samples]
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):
    _op(model, "dwB").builtinOptions = DW.depthwise_options_table(1, 2, 2, 3)
  got = _run(models, "static", ref=r2, tgt=t2, samples=doubled)
  assert got.skipped == {"dwA/y": mv.SKIP_DEPTHWISE_MULTIPLIER, "dwB/y": mv.SKIP_DEPTHWISE_MULTIPLIER, "dwC/y": mv.SKIP_SAMPLE_SHAPE}
  # a filter kind other than int8
  t2 = copy.deepcopy(models["dynamic"])
  _tensor(t2, "dwA/w").type = int(q.TensorType.INT4)
  _tensor(t2, "dwB/w").type = int(q.TensorType.INT16)
  got = _run(models, "dynamic", tgt=t2)
  assert got.skipped == {"dwA/y": mv.SKIP_DEPTHWISE_KIND, "dwB/y": mv.SKIP_DEPTHWISE_KIND} and got["dwC/y"]["mode"] == "dynamic"
  # blockwise scales
  t2 = copy.deepcopy(models["dynamic"])
  w = _tensor(t2, "dwA/w")
  sg = t2.subgraphs[0]
  t2.buffers.append(q.BufferT(data=np.ones(144 // 16, np.float16).view(np.uint8)))
  sg.tensors.append(q.TensorT(name=b"dwA/w_scales", shape=[9, 1], buffer=len(t2.buffers) - 1, type=int(q.TensorType.FLOAT16)))
  w.quantization = q.QuantizationParametersT(detailsType=2, details=q.BlockwiseQuantizationT(scales=len(sg.tensors) - 1, blockSize=16))
  got = _run(models, "dynamic", tgt=t2)
  assert got.skipped == {"dwA/y": mv.SKIP_DEPTHWISE_BLOCKWISE} and got["dwB/y"]["mode"] == "dynamic"
  # per-channel scales along another dimension: 2 (KW entries), and 0 (O entries along a dimension of size 1)
  t2 = copy.deepcopy(models["dynamic"])
  for name, axis, count in (("dwA", 2, 3), ("dwB", 0, 6), ("dwC", 1, 3)):
    w = _tensor(t2, f"{name}/w")
    w.quantization.quantizedDimension = axis
    w.quantization.scale, w.quantization.zeroPoint = np.ones(count, np.float32), np.zeros(count, np.int64)
  got = _run(models, "dynamic", tgt=t2)
  assert got.skipped == {f"{n}/y": mv.SKIP_DEPTHWISE_SCALE_AXIS for n in ("dwA", "dwB", "dwC")}
  # the float op and the target op disagree: strides; padding; depth multiplier written differently
  t2 = copy.deepcopy(tgt)
  _op(t2, "dwA").builtinOptions = DW.depthwise_options_table(None, 2, 2, 1, 1)
  _op(t2, "dwB").builtinOptions = DW.depthwise_options_table(None, 2, 2, 2)
  _op(t2, "dwC").builtinOptions = DW.depthwise_options_table(None, 1, 1, 1, 3, 2, 2)
  got = _run(models, "static", tgt=t2)
  assert got.skipped == {f"{n}/y": mv.SKIP_DEPTHWISE_MISMATCH for n in ("dwA", "dwB", "dwC")}
  # ---- the reasons CONV_2D has keep their texts
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):      # a stride of 0, a dilation of 0, an unknown padding
    _op(model, "dwA").builtinOptions = DW.depthwise_options_table(None, 0, 1, 1, 1)
    _op(model, "dwB").builtinOptions = DW.depthwise_options_table(1, 2, 2, 2, None, 1, 0)
    _op(model, "dwC").builtinOptions = DW.depthwise_options_table(2, 1, 1, None, 3, 2, 2)
  got = _run(models, "static", ref=r2, tgt=t2)
  assert got.skipped == {f"{n}/y": mv.SKIP_CONV_OPTIONS for n in ("dwA", "dwB", "dwC")}
  t2 = copy.deepcopy(tgt)
  _op(t2, "dwB").builtinOptionsType = 1      # (the options of another op type)
  assert _run(models, "static", tgt=t2).skipped == {"dwB/y": mv.SKIP_CONV_OPTIONS}
  small = [dict(s, **{"dwB/x": s["dwB/x"][:, :4, :4, :]}) for s in samples]      # VALID 5x5 on a 4 x 4 image
  assert _run(models, "static", samples=small).skipped == {"dwB/y": mv.SKIP_CONV_GEOMETRY}
  t2 = copy.deepcopy(models["dynamic"])
  _tensor(t2, "dwA/x").name = b"dwA/x_rotated"
  _tensor(t2, "dwB/w").quantization.zeroPoint = np.ones(6, np.int64)
  got = _run(models, "dynamic", tgt=t2, follow_input_transforms=True)
  assert got.skipped == {"dwA/y": mv.SKIP_INPUT, "dwB/y": mv.SKIP_WEIGHT_ZERO_POINT}
  assert got["dwC/y"]["input_transform"] == "none" and got["dwC/y"]["hadamard_size"] == 0
  t2 = copy.deepcopy(models["dynamic"])
  w = _tensor(t2, "dwA/w")
  w.type, w.quantization = int(q.TensorType.FLOAT32), None
  t2.buffers[w.buffer].data = DW.constant(ref, "dwA/w").reshape(-1).view(np.uint8)
  _op(t2, "dwC").opcodeIndex = 1
  got = _run(models, "dynamic", tgt=t2)
  assert got.skipped == {"dwA/y": mv.SKIP_FLOAT_TARGET, "dwC/y": mv.SKIP_TARGET}
  got = _run(models, "static", samples=[{k: v for k, v in s.items() if k != "dwC/x"} for s in samples])
  assert got.skipped == {"dwC/y": mv.SKIP_NO_SAMPLE}
  # a final_skipped reason reaches a depthwise entry as it reaches the others: a fused activation the epilogue has not
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):
    _op(model, "dwA").builtinOptions = DW.depthwise_options_table(None, 1, 1, 1, OC.TANH)
  got = _run(models, "static", ref=r2, tgt=t2, quantized_outputs=True)
  assert got.skipped == {} and got["dwA/y"]["final_skipped"] == mv.FINAL_SKIP_ACTIVATION and "final_error" not in got["dwA/y"]
  assert "final_error" in got["dwC/y"]


def test_validate_layer_execution_passes_the_keyword_on(models, monkeypatch, tmp_path):
  """(On the parent commit the keyword is a TypeError.)"""
  from mi355q import model_validator as mv
  from mi355q import quantizer
  from mi355q.utils import tflite_flatbuffer
  qz = quantizer.Quantizer(models["ref"])
  qz._result = quantizer.QuantizationResult([{}], bytearray(tflite_flatbuffer.write_model(models["static"])))      # pylint: disable=protected-access
  monkeypatch.setattr(mv, "LayerExecutionKernels", DW.numpy_kernels())
  plain = qz.validate_layer_execution(models["samples"])
  assert list(plain) == ["fc/y"] and not plain.skipped and "op" not in plain["fc/y"]
  got = qz.validate_layer_execution({"serving_default": models["samples"]}, save_folder=str(tmp_path), model_name="out",
                                    quantized_outputs=True, depthwise_conv_2d=True)
  want = _run(models, "static", quantized_outputs=True)
  assert got.skipped == {} and list(got) == list(want) and len(got) == 4
  for y, r in want.results.items():
    assert got[y]["final_error"] == r["final_error"] and got[y]["op"] == r["op"]
  saved = json.load(open(tmp_path / "out_layer_execution_errors.json"))
  assert {y: e["op"] for y, e in saved["layers"].items()} == {"fc/y": "FULLY_CONNECTED", "dwA/y": "DEPTHWISE_CONV_2D",
                                                             "dwB/y": "DEPTHWISE_CONV_2D", "dwC/y": "DEPTHWISE_CONV_2D"}
  both = qz.validate_layer_execution(models["samples"], conv_2d=True, depthwise_conv_2d=True)
  assert list(both) == list(want) and both["dwA/y"]["error"] == want["dwA/y"]["error"]


# ---------------------------------------------------------------- the kernels' build
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_dwconv_kernels_use_no_scratch(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path / "dwconv.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "dwconv.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  # five entries (float32 forward; int8 and int16, forward and output) x two routes x a 32-bit and a 64-bit unit index
  assert len(kernels) == 20 and all("dwconv_kernel" in k for k in kernels), kernels
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == 20 and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
  assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)\S*\s.*\boffen\b", asm)
  vgprs = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", asm)]
  assert len(vgprs) == 20, vgprs
  for k, v in zip(kernels, vgprs):      # 8 waves per SIMD with the 32-bit unit index, at least 6 in the strided form
    assert v <= (64 if k.split("ELb")[1][1:3] == "Ej" else 80), (k, v)
  # the float32 kernels multiply and add, and fuse nothing (with a 64-bit unit index the expansion of the 64-bit
  # division holds fused operations of its own, so the 32-bit kernels are the ones read); the vector route's tap loop
  # has one 16-byte load of the activation and one of the filter, and the kernel one 16-byte store
  seen = 0
  for k in kernels:
    body = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(k), asm, re.M | re.S).group(1)
    if "IfLi0ELb" in k and k.split("ELb")[1][1:3] == "Ej":      # <float, forward, either route, uint32_t>
      seen += 1
      assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac|madmk|madak)_f32", body), k
      assert re.search(r"\bv_(pk_)?mul_f32", body) and re.search(r"\bv_(pk_)?add_f32", body), k
    if "IfLi0ELb1Ej" in k:
      assert len(re.findall(r"global_load_dwordx4", body)) == len(re.findall(r"global_load_", body)) == 2, k
      assert len(re.findall(r"global_store_dwordx4", body)) == len(re.findall(r"global_store_", body)) == 1, k
  assert seen == 2
