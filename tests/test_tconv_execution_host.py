"""CPU checks of the integer execution of quantized TRANSPOSE_CONV ops: mi355q_tconv_patches_nhwc is declared,
exported, bound and refuses bad arguments before any launch; ops.tconv_geometry / ops.tconv_phases and the NumPy phase
gather of tests/tconv_execution_cases.py against an independent scatter-form transposed convolution on every listed
geometry; the TransposeConvOptions reader on the recorded model, on a decoded object and on an op without options;
model_validator.compare_layer_execution with `transpose_conv` and NumPy kernels, with the keyword off (nothing
changes) and on (every mode, every new key, every new skip reason, the saved JSON)."""
import copy
import json
import os
import re
import sys

import numpy as np
import pytest

import conv_execution_cases as CC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC
import tconv_execution_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
SYMBOL = "mi355q_tconv_patches_nhwc"


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
  assert "Patch gather for TRANSPOSE_CONV" in header
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  assert re.search(r"\b%s\s*\(" % SYMBOL, header)
  assert SYMBOL in _ffi.PROTOTYPES and hasattr(lib, SYMBOL)
  declared = re.search(r"%s\s*\(([^)]*)\)" % SYMBOL, header).group(1)
  assert len(_ffi.PROTOTYPES[SYMBOL][1]) == len(declared.split(",")) == 21
  for name in ("tconv_geometry", "tconv_phases", "tconv_patches", "tconv_forward", "tconv_output", "tconv_output_i16"):
    assert callable(getattr(ops, name)), name
  for method in ("tconv_patches", "image_scales"):
    assert callable(getattr(mv.LayerExecutionKernels, method)), method
  import __graft_entry__ as g
  assert "conv_patches.hip" in g.SOURCES      # (beside the CONV_2D gather: the source list did not change)


def test_refusals_come_before_any_launch(lib):
  TC.check_patch_refusals(lib)
  CC.check_patch_refusals(lib)      # the CONV_2D entry refuses what it refused, a dilation below 1 included


# ---------------------------------------------------------------- geometry and phases
def test_the_geometry_list():
  every, kept = TC.all_geometries(), TC.geometries()
  assert len(every) == 312 and 0 < len(kept) < len(every)
  assert all(max(s) > 1 for _, _, _, k, s, *_ in set(every) - set(kept))      # (an empty phase needs a stride above 1)
  assert any(g[6][0] % g[4][0] for g in kept) and any((g[1], g[2]) == (1, 1) for g in kept)
  assert any(len({(len(p[4]), len(p[5])) for p in TC.phases(*g[1:3], *g[3], *g[4:])}) > 1 for g in kept)      # unequal tap counts


def test_tconv_geometry_and_phases_against_the_cases(lib):
  from mi355q import ops
  # 4x4 stride 2 SAME 5 x 7 -> 10 x 14: the forward convolution pads (2 * 4 + 4 - 10) // 2 = 1; both taps' parities
  assert ops.tconv_geometry(5, 7, 4, 4, 2, "SAME", (10, 14)) == (1, 1)
  assert ops.tconv_phases(5, 7, 4, 4, 2, "SAME", (10, 14)) == [(0, 0, 5, 7, (1, 3), (1, 3)), (0, 1, 5, 7, (1, 3), (0, 2)),
                                                               (1, 0, 5, 7, (0, 2), (1, 3)), (1, 1, 5, 7, (0, 2), (0, 2))]
  # 3x3 stride 2 VALID 3 x 4 -> 7 x 10 (or 8 x 10): no padding, phase 0 has two taps and phase 1 one
  assert ops.tconv_geometry(3, 4, 3, 3, 2, 1, (8, 10)) == (0, 0)
  assert ops.tconv_phases(3, 4, 3, 3, (2, 2), "VALID", (7, 10))[0] == (0, 0, 4, 5, (0, 2), (0, 2))
  assert ops.tconv_phases(3, 4, 3, 3, (2, 2), "VALID", (7, 10))[3] == (1, 1, 3, 5, (1,), (1,))
  for bad in ((11, 14), (10, 12), (0, 14), (10, -1)):
    with pytest.raises(ValueError):
      ops.tconv_geometry(5, 7, 4, 4, 2, "SAME", bad)
  with pytest.raises(ValueError):
    ops.tconv_geometry(5, 7, 4, 4, 2, "FULL", (10, 14))
  for n, ih, iw, k, s, padding, out_hw in TC.all_geometries():
    assert ops.tconv_geometry(ih, iw, k[0], k[1], s, padding, out_hw) == TC.geometry(ih, iw, k[0], k[1], s, padding, out_hw)
    assert ops.conv_geometry(out_hw[0], out_hw[1], k[0], k[1], s, 1, padding)[:2] == (ih, iw)
    assert ops.tconv_phases(ih, iw, k[0], k[1], s, padding, out_hw) == TC.phases(ih, iw, k[0], k[1], s, padding, out_hw)


def test_phase_gather_then_product_is_the_scatter_form_for_every_geometry():
  """Full-range integers, the extremes planted in the corners, zero points at the ends of int8: the phase's patch rows
  padded with the zero point, times the filter slice, interleaved over the phases, are exactly the scatter form."""
  for i, (n, ih, iw, k, s, padding, out_hw) in enumerate(TC.geometries()):
    rng = np.random.default_rng(i)
    c, o = (1, 3, 4)[i % 3], (1, 5)[i % 2]
    zp = (0, -128, 127, 5)[i % 4]
    for dtype, lo, hi, zero in ((np.int8, -128, 127, zp), (np.int16, -32768, 32767, 0)):
      x = rng.integers(lo, hi, size=(n, ih, iw, c), endpoint=True).astype(dtype)
      x[:, 0, 0, :], x[:, -1, -1, :] = lo, hi
      qw = rng.integers(-128, 127, size=(o, k[0], k[1], c), endpoint=True)
      qw[0, 0, 0, :], qw[-1, -1, -1, :] = -128, 127
      parts, pixels = [], 0
      for py, px, qh, qw_n, kys, kxs in TC.phases(ih, iw, k[0], k[1], s, padding, out_hw):
        rows = TC.gather(x, k[0], k[1], s, padding, out_hw, (py, px), zero)
        assert rows.shape == (n * qh * qw_n, len(kys) * len(kxs) * c) and rows.dtype == dtype
        parts.append((py, px, (rows.astype(np.int64) - zero) @ TC.filter_slice(qw, kys, kxs).astype(np.int64).T))
        pixels += qh * qw_n
        for first, count in TC.windows(rows.shape[0], qh * qw_n):
          assert CC.same_bytes(TC.gather(x, k[0], k[1], s, padding, out_hw, (py, px), zero, first, count), rows[first:first + count])
      assert pixels == out_hw[0] * out_hw[1]
      assert np.array_equal(TC.interleave(parts, n, out_hw, s, o), TC.integer_tconv(x, zero, qw, s, padding, out_hw)), (i, dtype)


# ---------------------------------------------------------------- the options reader
def test_options_reader(lib):
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  from mi355q.utils import tflite_flatbuffer as fb
  m = mv._as_model(open(os.path.join(MODELS, "single_conv2d_transpose_bias.tflite"), "rb").read())      # pylint: disable=protected-access
  found = mv._transpose_conv_ops(m, 0)      # pylint: disable=protected-access
  assert len(found) == 1
  op, x_name, w, y_name = found[0]
  assert isinstance(op.builtinOptions, fb.OpaqueTableT) and op.builtinOptionsType == 49
  assert (x_name, list(w.shape), y_name) == ("serving_default_input_6:0", [1, 5, 5, 1], "StatefulPartitionedCall:0")
  assert mv.transpose_conv_options(op) == dict(padding=1, stride_w=1, stride_h=1, fused_activation_function=0)
  assert mv._transpose_conv_option(op, "fusedActivationFunction") == 0 and mv._transpose_conv_option(op, "weightsFormat") == 0      # pylint: disable=protected-access
  assert mv.conv_2d_options(op) is None      # (another op's options)

  def read(table, options_type=49):
    return mv.transpose_conv_options(q.OperatorT(inputs=[0, 1, 2], outputs=[3], opcodeIndex=0, builtinOptionsType=options_type,
                                                 builtinOptions=table))
  assert read(TC.tconv_options_table(1, 2, 3, OC.RELU6)) == dict(padding=1, stride_w=2, stride_h=3, fused_activation_function=3)
  assert read(TC.tconv_options_table()) == dict(padding=0, stride_w=0, stride_h=0, fused_activation_function=0)
  assert read(TC.tconv_options_table(stride_w=2, stride_h=1)) == dict(padding=0, stride_w=2, stride_h=1, fused_activation_function=0)
  assert read(None, 0) == read(TC.tconv_options_table())      # an op without options: every default
  assert read(TC.tconv_options_table(1, 2, 3, 1), 1) is None      # Conv2DOptions
  assert read(q.FullyConnectedOptionsT(), 8) is None

  class Decoded:      # the generated object API's names
    padding, strideW, strideH, fusedActivationFunction = 1, 2, None, 1

  class DecodedConv(Decoded):
    dilationWFactor, dilationHFactor = 1, 1
  assert read(Decoded()) == dict(padding=1, stride_w=2, stride_h=0, fused_activation_function=1)
  assert read(DecodedConv()) is None
  model = TC.build_model()      # a table survives the writer and the reader
  again = fb.read_model(bytes(fb.write_model(model)))
  for tconv, a, b in zip(TC.TCONVS, model.subgraphs[0].operators, again.subgraphs[0].operators):
    want = dict(padding=TC.PADDING_CODE[tconv[5]], stride_w=tconv[4][1], stride_h=tconv[4][0], fused_activation_function=tconv[7])
    assert mv.transpose_conv_options(a) == mv.transpose_conv_options(b) == want


# ---------------------------------------------------------------- compare_layer_execution
@pytest.fixture(scope="module")
def models(lib):
  ref = TC.build_model()
  samples = TC.build_samples(ref)
  return dict(ref=ref, samples=samples, static=TC.quantize_by_hand(ref, samples, "static", 8),
              static16=TC.quantize_by_hand(ref, samples, "static", 16), dynamic=TC.quantize_by_hand(ref, samples, "dynamic"),
              weight_only=TC.quantize_by_hand(ref, samples, "weight_only"))


def _tensor(model, name):
  return next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)


def _op(model, name):
  sg = model.subgraphs[0]
  return next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"{name}/y")


def _run(models, key, ref=None, tgt=None, samples=None, **kw):
  from mi355q import model_validator as mv
  kw.setdefault("transpose_conv", True)
  return mv.compare_layer_execution(ref or models["ref"], tgt or models[key], models["samples"] if samples is None else samples,
                                    kernels=TC.numpy_kernels()(), **kw)


def _reference(models, key, tconv, bits=8):
  """(error, signal, final_error or None, final_signal or None, tokens) of one op, written out here with the scatter
  form for the integer product: neither patches nor phases on the quantized side."""
  name, c, o, k, s, padding, has_bias, fused, out_hw = tconv
  ref, tgt = models["ref"], models[key]
  w_t = _tensor(tgt, f"{name}/w")
  s_w = np.asarray(w_t.quantization.scale, np.float32)
  qw = np.asarray(tgt.buffers[w_t.buffer].data).view(np.int8).reshape(o, k[0], k[1], c)
  sq_d = sq_y = f_d = f_y = 0.0
  tokens = 0
  for sample in models["samples"]:
    x = sample[f"{name}/x"]
    y32 = TC.float_tconv(ref, tconv, x, np.float32, pre_bias=True).reshape(-1, o)
    n = y32.shape[0]
    if key == "weight_only":
      deq = (qw.astype(np.float32) * s_w[:, None, None, None]).astype(np.float32)
      parts = [(py, px, TC.gather(x, k[0], k[1], s, padding, out_hw, (py, px), 0.0) @ TC.filter_slice(deq, kys, kxs).T)
               for py, px, _, _, kys, kxs in TC.phases(TC.HEIGHT, TC.WIDTH, k[0], k[1], s, padding, out_hw)]
      yq = TC.interleave(parts, TC.BATCH, out_hw, s, o).reshape(-1, o)
    elif key == "dynamic":
      q, scale = EC.quantize_rows(x.reshape(TC.BATCH, -1))
      acc = TC.integer_tconv(q.reshape(x.shape), 0, qw, s, padding, out_hw).reshape(-1, o)
      sc = np.repeat(scale, n // TC.BATCH)[:, None] * s_w[None, :]
      yq = acc.astype(np.int32).astype(np.float32) * sc
    else:
      x_t, y_t = _tensor(tgt, f"{name}/x"), _tensor(tgt, f"{name}/y")
      s_x, zp_x = np.float32(x_t.quantization.scale[0]), int(x_t.quantization.zeroPoint[0])
      s_y, zp_y = np.float32(y_t.quantization.scale[0]), int(y_t.quantization.zeroPoint[0])
      xq = EC16.quantize_static16(x, s_x) if bits == 16 else EC.quantize_static(x, s_x, zp_x)
      acc = TC.integer_tconv(xq, zp_x, qw, s, padding, out_hw).reshape(-1, o)
      sc = (s_x * s_w)[None, :].astype(np.float32)
      yq = EC16.rescale(acc, np.broadcast_to(sc, acc.shape).copy()) if bits == 16 else acc.astype(np.int32).astype(np.float32) * sc
      # the epilogue of the statement, on the accumulators of the scatter form
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
      y_act = TC.float_tconv(ref, tconv, x, np.float32).reshape(-1, o).astype(np.float64)
      f_d += ((yf - y_act) ** 2).sum()
      f_y += (y_act ** 2).sum()
    sq_d += ((yq.astype(np.float64) - y32.astype(np.float64)) ** 2).sum()
    sq_y += (y32.astype(np.float64) ** 2).sum()
    tokens += n
  final = (f_d / tokens, f_y / tokens) if key.startswith("static") else (None, None)
  return sq_d / tokens, sq_y / tokens, final[0], final[1], tokens


def test_the_float_phases_are_the_float64_scatter_form(models):
  """The float side of the report is formed by phases too; against the float64 scatter form it is a float32 product."""
  for tconv in TC.TCONVS:
    x = models["samples"][0][f"{tconv[0]}/x"]
    a = TC.float_tconv(models["ref"], tconv, x, np.float32)
    b = TC.float_tconv(models["ref"], tconv, x, np.float64)
    assert a.shape == b.shape == (TC.BATCH, *tconv[8], tconv[2]) and a.dtype == np.float32
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-5 * float(np.abs(b).max()))


def test_with_the_keyword_off_results_and_saved_json_are_what_they_were(models, tmp_path):
  from mi355q import model_validator as mv
  for key in ("static", "dynamic", "weight_only"):
    for kw in (dict(), dict(int16_activations=True, quantized_outputs=True), dict(follow_input_transforms=True),
               dict(conv_2d=True, depthwise_conv_2d=True, batch_matmul=True)):
      old = mv.compare_layer_execution(models["ref"], models[key], models["samples"], kernels=OC.numpy_kernels()(), **kw)
      off = _run(models, key, transpose_conv=False, **kw)
      assert list(old) == list(off) == ["fc/y"] and old.skipped == off.skipped == {}
      assert sorted(old["fc/y"]) == sorted(off["fc/y"]) and ("op" in off["fc/y"]) == ("conv_2d" in kw)
      for k, v in old["fc/y"].items():
        assert np.array_equal(off["fc/y"][k], v), (key, k)
      a = open(old.save(str(tmp_path / "old"), "m"), "rb").read()
      b = open(off.save(str(tmp_path / "off"), "m"), "rb").read()
      assert a == b and b"TRANSPOSE_CONV" not in a and b"phases" not in a
      on = _run(models, key, **kw)      # the FC entry's other keys do not move when the keyword is on
      assert on["fc/y"]["op"] == "FULLY_CONNECTED" and sorted(on["fc/y"]) == sorted(set(old["fc/y"]) | {"op"})
      for k, v in old["fc/y"].items():
        assert np.array_equal(on["fc/y"][k], v), (key, k)


@pytest.mark.parametrize("key", ["static", "static16", "dynamic", "weight_only"])
def test_with_the_keyword_on_every_op_is_reported_in_every_mode(models, key, tmp_path):
  bits = 16 if key == "static16" else 8
  got = _run(models, key, int16_activations=True, quantized_outputs=True)
  assert got.skipped == {} and list(got) == ["fc/y"] + [f"{c[0]}/y" for c in TC.TCONVS]
  mode = {"static": "static", "static16": "static", "dynamic": "dynamic", "weight_only": "weight_only"}[key]
  for tconv in TC.TCONVS:
    name, c, o, k, s, padding, has_bias, fused, out_hw = tconv
    r = got[f"{name}/y"]
    error, signal, f_error, f_signal, tokens = _reference(models, key, tconv, bits)
    assert (r["op"], r["weight"], r["input"], r["mode"]) == ("TRANSPOSE_CONV", f"{name}/w", f"{name}/x", mode)
    assert (r["rows"], r["d"], r["tokens"]) == (o, k[0] * k[1] * c, TC.SAMPLES * TC.BATCH * out_hw[0] * out_hw[1]) and tokens == r["tokens"]
    assert (r["kernel"], r["strides"], r["padding"], r["output_hw"]) == (list(k), list(s), padding, list(out_hw))
    assert "dilations" not in r and r["phases"] == s[0] * s[1]
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
  entry = saved["layers"]["tcC/y"]
  assert entry["op"] == "TRANSPOSE_CONV" and entry["kernel"] == [2, 5] and entry["strides"] == [2, 1] and entry["padding"] == "SAME"
  assert entry["output_hw"] == [9, 6] and entry["phases"] == 2 and "per_channel_error" not in entry and "dilations" not in entry
  assert saved["layers"]["fc/y"]["op"] == "FULLY_CONNECTED"
  plain = _run(models, key, int16_activations=True)      # without quantized_outputs: the pre-bias figures alone
  for y in got:
    assert not [x for x in plain[y] if x.startswith("final") or x in ("output_bits", "fused_activation")]
    assert plain[y]["error"] == got[y]["error"]
  if key == "static16":
    assert _run(models, key).skipped == {f"{n}/y": "the op reads an INT16 activation" for n in ("fc", "tcA", "tcB", "tcC")}


def test_chunks_do_not_change_the_figures(models, monkeypatch):
  """A chunk of 7 rows cuts every phase many times; the integer-derived error moves only by the order of float64 sums."""
  from mi355q import model_validator as mv
  whole = _run(models, "static", quantized_outputs=True)
  monkeypatch.setattr(mv, "EXECUTION_CHUNK_ROWS", 7)
  cut = _run(models, "static", quantized_outputs=True)
  for y in whole:
    assert cut[y]["tokens"] == whole[y]["tokens"]
    np.testing.assert_allclose([cut[y]["error"], cut[y]["final_error"]], [whole[y]["error"], whole[y]["final_error"]], rtol=1e-5)


def test_every_new_skip_reason(models):
  from mi355q import model_validator as mv
  from mi355q import qtyping as q
  ref, tgt, samples = models["ref"], models["static"], models["samples"]
  # output_shape: not a constant; FLOAT32; channels that disagree with the filter
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  _tensor(r2, "tcA/output_shape").buffer = 0
  _tensor(r2, "tcB/output_shape").type = int(q.TensorType.FLOAT32)
  for model in (r2, t2):
    model.buffers[_tensor(model, "tcC/output_shape").buffer].data = np.array([2, 9, 6, 17], np.int32).view(np.uint8)
  got = _run(models, "static", ref=r2, tgt=t2)
  assert got.skipped == {f"{n}/y": mv.SKIP_TCONV_OUTPUT_SHAPE for n in ("tcA", "tcB", "tcC")} and list(got) == ["fc/y"]
  # ... a batch that disagrees with the sample; the two models disagree about it
  t2 = copy.deepcopy(tgt)
  t2.buffers[_tensor(t2, "tcB/output_shape").buffer].data = np.array([2, 12, 14, 8], np.int32).view(np.uint8)
  got = _run(models, "static", tgt=t2, samples=[dict(s, **{"tcA/x": s["tcA/x"][:1]}) for s in samples])
  assert got.skipped == {"tcA/y": mv.SKIP_TCONV_OUTPUT_SHAPE, "tcB/y": mv.SKIP_TCONV_OUTPUT_SHAPE} and "tcC/y" in got
  # unreachable: 9 x 12 does not map back to a 4 x 6 sample; 10 x 12 does not map back under VALID
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):
    _op(model, "tcC").builtinOptions = TC.tconv_options_table(1, 1, 2, 3)
  got = _run(models, "static", ref=r2, tgt=t2, samples=[dict(s, **{"tcA/x": s["tcA/x"][:, :4]}) for s in samples])
  assert got.skipped == {"tcA/y": mv.SKIP_TCONV_UNREACHABLE, "tcC/y": mv.SKIP_TCONV_UNREACHABLE}
  # a stride above the kernel: 2x5 under strides (3, 1), 5 x 6 -> 15 x 6 (SAME)
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):
    _op(model, "tcC").builtinOptions = TC.tconv_options_table(None, 1, 3, 3)
    model.buffers[_tensor(model, "tcC/output_shape").buffer].data = np.array([2, 15, 6, 16], np.int32).view(np.uint8)
  got = _run(models, "static", ref=r2, tgt=t2)
  assert got.skipped == {"tcC/y": mv.SKIP_TCONV_STRIDE}
  # options: the two models differ; a stride of 0 and an unknown padding in both; another op's options
  t2 = copy.deepcopy(tgt)
  _op(t2, "tcA").builtinOptions = TC.tconv_options_table(1, 2, 2)
  _op(t2, "tcB").builtinOptions = TC.tconv_options_table(1, 2, 1, OC.RELU)
  _op(t2, "tcC").builtinOptionsType = 1
  got = _run(models, "static", tgt=t2)
  assert got.skipped == {"tcA/y": mv.SKIP_TCONV_MISMATCH, "tcB/y": mv.SKIP_TCONV_MISMATCH, "tcC/y": mv.SKIP_CONV_OPTIONS}
  r2, t2 = copy.deepcopy(ref), copy.deepcopy(tgt)
  for model in (r2, t2):
    _op(model, "tcA").builtinOptions = TC.tconv_options_table(None, 0, 2)
    _op(model, "tcB").builtinOptions = TC.tconv_options_table(2, 2, 2, OC.RELU)
  got = _run(models, "static", ref=r2, tgt=t2)
  assert got.skipped == {"tcA/y": mv.SKIP_CONV_OPTIONS, "tcB/y": mv.SKIP_CONV_OPTIONS}
  # the filter: blockwise; scales along dimension 3; INT16
  t2 = copy.deepcopy(models["dynamic"])
  sg = t2.subgraphs[0]
  t2.buffers.append(q.BufferT(data=np.ones(24 * 256 // 32, np.float16).view(np.uint8)))
  sg.tensors.append(q.TensorT(name=b"tcA/w_scales", shape=[24, 256 // 32], buffer=len(t2.buffers) - 1,
                              type=int(q.TensorType.FLOAT16)))
  _tensor(t2, "tcA/w").quantization = q.QuantizationParametersT(detailsType=2, details=q.BlockwiseQuantizationT(
      scales=len(sg.tensors) - 1, blockSize=32))
  _tensor(t2, "tcB/w").quantization.quantizedDimension = 3
  _tensor(t2, "tcB/w").quantization.scale = np.ones(3, np.float32)
  _tensor(t2, "tcB/w").quantization.zeroPoint = np.zeros(3, np.int64)
  w = _tensor(t2, "tcC/w")
  w.type = int(q.TensorType.INT16)
  t2.buffers[w.buffer].data = np.zeros(16 * 2 * 5 * 16, np.int16).view(np.uint8)
  got = _run(models, "dynamic", tgt=t2)
  assert got.skipped == {f"{n}/y": mv.SKIP_TCONV_FILTER_SCALES for n in ("tcA", "tcB", "tcC")}
  # the reasons of CONV_2D that apply keep their texts
  r2 = copy.deepcopy(ref)
  _tensor(r2, "tcA/w").shape = [24, 16, 16]
  doubled = [dict(s, **{"tcB/x": np.concatenate([s["tcB/x"]] * 2, axis=3), "tcC/x": s["tcC/x"].reshape(2, 5, 96)}) for s in samples]
  got = _run(models, "static", ref=r2, samples=doubled)
  assert got.skipped == {"tcA/y": mv.SKIP_CONV_FILTER, "tcB/y": mv.SKIP_CONV_GROUPS, "tcC/y": mv.SKIP_SAMPLE_SHAPE}
  t2 = copy.deepcopy(models["dynamic"])
  _tensor(t2, "tcA/x").name = b"tcA/x_rotated"
  got = _run(models, "dynamic", tgt=t2, follow_input_transforms=True)
  assert got.skipped == {"tcA/y": mv.SKIP_INPUT} and got["tcC/y"]["input_transform"] == "none"
  got = _run(models, "static", samples=[{k: v for k, v in s.items() if k != "tcC/x"} for s in samples])
  assert got.skipped == {"tcC/y": mv.SKIP_NO_SAMPLE}
  got = _run(models, "static", samples=[dict(s, **{"tcC/x": s["tcC/x"][:0]}) for s in samples])
  assert got.skipped == {"tcC/y": mv.SKIP_NO_SAMPLE}
  # a static op whose bias is not what the epilogue reads keeps its pre-bias figures (the bias is input 3)
  t2 = copy.deepcopy(tgt)
  _tensor(t2, "tcA/b").type = int(q.TensorType.FLOAT32)
  got = _run(models, "static", tgt=t2, quantized_outputs=True)
  assert got.skipped == {} and got["tcA/y"]["final_skipped"] == mv.FINAL_SKIP_BIAS and "final_error" in got["tcC/y"]


def test_validate_layer_execution_passes_the_keyword_on(models, monkeypatch, tmp_path):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  from mi355q.utils import tflite_flatbuffer
  qz = quantizer.Quantizer(models["ref"])
  qz._result = quantizer.QuantizationResult([{}], bytearray(tflite_flatbuffer.write_model(models["static"])))      # pylint: disable=protected-access
  monkeypatch.setattr(mv, "LayerExecutionKernels", TC.numpy_kernels())
  plain = qz.validate_layer_execution(models["samples"])
  assert list(plain) == ["fc/y"] and not plain.skipped and "op" not in plain["fc/y"]
  got = qz.validate_layer_execution({"serving_default": models["samples"]}, save_folder=str(tmp_path), model_name="out",
                                    quantized_outputs=True, transpose_conv=True)
  want = _run(models, "static", quantized_outputs=True)
  assert got.skipped == {} and list(got) == list(want) and len(got) == 4
  for y, r in want.results.items():
    assert got[y]["final_error"] == r["final_error"] and got[y]["op"] == r["op"]
  saved = json.load(open(tmp_path / "out_layer_execution_errors.json"))
  assert {y: e["op"] for y, e in saved["layers"].items()} == {"fc/y": "FULLY_CONNECTED", "tcA/y": "TRANSPOSE_CONV",
                                                             "tcB/y": "TRANSPOSE_CONV", "tcC/y": "TRANSPOSE_CONV"}
