"""Host checks of the integer BATCH_MATMUL execution (csrc/qbmm.hip): the NumPy statement of bmm_execution_cases against
a triple loop, the case list against the restated dispatch, the int32 bound, and the ABI in the header, the prototypes
and the wrappers. No GPU."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import bmm_execution_cases as BC
import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mi355q_qbmm_mfma_route", "mi355q_qbmm_workspace_bytes", "mi355q_qbmm_forward_i8", "mi355q_qbmm_output_i8")


@pytest.fixture(scope="module")
def lib():
  """The built library on the host: mi355q_qbmm_mfma_route reads nothing and needs no GPU."""
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def _library_route(lib, m, n, k, adj_x, adj_y, a_misaligned=False, b_misaligned=False) -> str:
  """What the library's own dispatch says for bases that are (not) 16-byte aligned; the addresses are never read."""
  a, b = 4096 + int(a_misaligned), 8192 + int(b_misaligned)
  return "mfma" if lib.mi355q_qbmm_mfma_route(a, m, k, int(adj_x), b, n, int(adj_y)) else "generic"


@pytest.mark.parametrize("adj_x,adj_y", BC.LAYOUTS)
def test_the_statement_is_the_triple_loop(adj_x, adj_y):
  for i, (batch, b_batch, m, n, k) in enumerate(((1, 1, 1, 1, 1), (2, 2, 3, 5, 7), (3, 1, 4, 2, 9))):
    c = BC.Case(batch, b_batch, m, n, k, adj_x, adj_y, *BC.ZERO_POINTS[(i + 1) % 4])
    rng = np.random.default_rng(i)
    sa, sb = c.shapes()
    a = rng.integers(-128, 127, size=sa, endpoint=True).astype(np.int8)
    b = rng.integers(-128, 127, size=sb, endpoint=True).astype(np.int8)
    want = BC.accumulators_loop(a, b, adj_x, adj_y, c.za, c.zb)
    assert np.array_equal(BC.accumulators(a, b, adj_x, adj_y, c.za, c.zb), want), c.id
    # leading dimensions of any rank are the batch
    a4, b4 = a.reshape((1,) + a.shape), b.reshape((1,) + b.shape)
    assert np.array_equal(BC.accumulators(a4, b4, adj_x, adj_y, c.za, c.zb), want)


def test_the_rescale_and_the_epilogue_of_the_statement():
  acc = np.array([[[3, -5], [1 << 24 | 1, -(1 << 30)]]], np.int64)
  y = BC.rescale(acc, [0.5, 0.25], [2.0, 3.0])
  assert y.dtype == np.float32 and y.shape == (1, 2, 2)
  assert y[0, 0].tolist() == [3.0, -7.5]
  # float(acc) rounds to float32 BEFORE the product: 2^24 + 1 -> 2^24
  assert y[0, 1, 0] == np.float32(1 << 24) * np.float32(0.5) and y[0, 1, 1] == -np.float32(1 << 30) * np.float32(0.75)
  sc = np.float32(np.float32(0.013) * np.float32(0.0071))
  assert BC.rescale(acc, [0.013], [0.0071])[0, 0, 0] == np.float32(3) * sc
  m, s = OC.quantize_multiplier(0.5)
  q = BC.output(np.array([[[53, -53], [255, -257]]], np.int64), [m], [s], 100)
  assert q.dtype == np.int8 and q.tolist() == [[[127, 74], [127, -28]]]      # 26.5 -> 27; -26.5 -> -26; clamp; -128.5 -> -128
  q = BC.output(np.array([[[4, 4]]], np.int64), [m, m], [s, s + 1], 0)
  assert q.tolist() == [[[2, 4]]]


def test_the_case_list_reaches_every_route_for_every_layout(lib):
  cases = BC.cases()
  for c in cases:      # the restated dispatch is the library's
    assert _library_route(lib, c.m, c.n, c.k, c.adj_x, c.adj_y, c.a_misaligned, c.b_misaligned) == c.route[0], c.id
  assert len({c.id for c in cases}) == len(cases)
  for adj_x, adj_y in BC.LAYOUTS:
    mine = [c for c in cases if (c.adj_x, c.adj_y) == (adj_x, adj_y)]
    routes = {c.route for c in mine}
    loads = ("a_transposed" if adj_x else "a_direct", "b_direct" if adj_y else "b_transposed")
    assert routes == {("generic",), ("mfma",) + loads + ("sums",), ("mfma",) + loads + ("nosums",)}, (adj_x, adj_y)
    for form in ((3, 3), (3, 1), (1, 1)):      # both batch forms (and a single batch) on every route and sum path
      for r in routes:
        assert any((c.batch, c.b_batch) == form and c.route == r for c in mine), (adj_x, adj_y, form, r)
    for zp in BC.ZERO_POINTS:
      assert any((c.za, c.zb) == zp and c.route[0] == "mfma" for c in mine), zp
    for edge in (1, 15, 16, 17, 64, 65, 129):
      assert any(c.m == edge for c in mine) and any(c.n == edge for c in mine), edge
    assert {c.k for c in mine if c.route[0] == "mfma"} == set(BC.MFMA_K)
    assert set(BC.GENERIC_K) <= {c.k for c in mine if c.route == ("generic",)}
    assert any(c.a_misaligned for c in mine) and any(c.b_misaligned for c in mine)
    assert all(c.route == ("generic",) for c in mine if c.a_misaligned or c.b_misaligned)
  seen = set()
  for c in cases:
    seen.update(c.route)
  assert seen == BC.ROUTE_ELEMENTS
  assert all(all(e in c.id for e in c.route) for c in cases)


def test_route_conditions(lib):
  for m, n, k in ((15, 17, 64), (16, 17, 64), (17, 16, 64), (16, 16, 64), (16, 16, 65), (16, 16, 1), (16, 16, 0), (32, 48, 32768)):
    for adj_x, adj_y in BC.LAYOUTS:
      for mis in ((False, False), (True, False), (False, True)):
        assert _library_route(lib, m, n, k, adj_x, adj_y, *mis) == BC.route(m, n, k, adj_x, adj_y, 0, 0, *mis)[0], (m, n, k)
  assert BC.route(16, 16, 0, False, True, 0, 0) == ("generic",)      # K = 0: the empty sum, no fragment to load
  assert BC.route(15, 17, 64, False, True, 0, 0) == ("mfma", "a_direct", "b_direct", "nosums")
  assert BC.route(16, 17, 64, False, False, 0, 0) == ("generic",)            # N % 16 with b transposed
  assert BC.route(17, 16, 64, True, True, 0, 0) == ("generic",)              # M % 16 with a transposed
  assert BC.route(16, 16, 64, True, False, 1, 0) == ("mfma", "a_transposed", "b_transposed", "sums")
  assert BC.route(16, 16, 65, False, True, 0, 0) == ("generic",) and BC.route(16, 16, 1, False, True, 0, 0) == ("generic",)
  assert BC.route(16, 16, 64, False, True, 0, 0, a_misaligned=True) == ("generic",)


def test_the_extremes_stay_inside_int32_and_the_limit_is_the_power_of_two_below_the_bound():
  term = 255 * 255
  assert BC.MAX_K * term == BC.EXTREME_ACC < 2 ** 31
  assert (BC.MAX_K + 1) * term > BC.EXTREME_ACC and 33025 * term < 2 ** 31 <= 33026 * term      # (the limit is the power of two below)
  c = BC.EXTREME
  assert (c.k, c.m, c.n, c.za, c.zb) == (BC.MAX_K, 16, 16, 127, 127) and c.route[0] == "mfma"
  a, b = np.full((1, 2, c.k), -128, np.int8), np.full((1, 2, c.k), -128, np.int8)
  assert (BC.accumulators(a, b, False, True, 127, 127) == BC.EXTREME_ACC).all()
  sys.path.insert(0, os.path.join(ROOT, "ai-edge-quantizer_amd"))
  from mi355q import ops
  assert ops.QBMM_MAX_K == BC.MAX_K      # K = 32769 is refused by the wrapper and by the library (the GPU test of refusals)
  # the four terms of the MFMA route's combination: each within int32, a partial sum of them not
  k, za, zb = BC.MAX_K, 127, 127
  dot, sum_a, sum_b = k * 128 * 128, -128 * k, -128 * k
  terms = (dot, -zb * sum_a, -za * sum_b, k * za * zb)
  assert all(abs(t) < 2 ** 31 for t in terms) and sum(terms) == BC.EXTREME_ACC
  assert terms[0] + terms[1] + terms[2] >= 2 ** 30 and abs(sum_a) <= 2 ** 22
  za, zb = -128, -128      # every term at its bound 2^29: three of them pass int32, the total does not
  a_v, b_v = 127, 127
  terms = (k * a_v * b_v, -zb * k * a_v, -za * k * b_v, k * za * zb)
  assert terms[0] + terms[1] + terms[2] + terms[3] == k * 255 * 255 and terms[1] + terms[2] + terms[3] < 2 ** 31
  assert max(abs(t) for t in terms) <= 2 ** 29


def test_abi_names_in_the_header_the_prototypes_and_the_wrappers():
  with open(os.path.join(ROOT, "include", "mi355q.h")) as f:
    header = f.read()
  sys.path.insert(0, os.path.join(ROOT, "ai-edge-quantizer_amd"))
  from mi355q import _ffi, ops
  for name in ENTRIES:
    decl = re.search(r"^(?:int32_t|int64_t|size_t)\s+" + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert decl, name
    assert len(_ffi.PROTOTYPES[name][1]) == decl.group(1).count(",") + 1, name
  fwd = re.search(r"mi355q_qbmm_forward_i8\(([^;]*)\);", header, re.S).group(1)
  order = [w for w in ("batch", "adj_x", "a_scale_count", "a_zero_point", "b_batch", "adj_y", "b_scale_count", "b_zero_point",
                       "y_out", "acc_out", "workspace_bytes", "stream")]
  assert [fwd.index(w) for w in order] == sorted(fwd.index(w) for w in order)
  assert "Integer batched matrix product" in header and "v_mfma_i32_16x16x64_i8" in header
  sig = inspect.signature(ops.qbmm_forward)
  assert list(sig.parameters) == ["a", "b", "adj_x", "adj_y", "a_scale", "a_zero_point", "b_scale", "b_zero_point", "want_acc"]
  assert all(p.kind == p.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("a", "b"))
  assert sig.parameters["want_acc"].default is False
  assert {"adj_x", "adj_y", "a_zero_point", "b_zero_point", "multiplier", "shift", "out_zero_point"} <= set(
      inspect.signature(ops.qbmm_output).parameters)
  assert ops.QBMM_MAX_K == BC.MAX_K
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "qbmm.hip" in g.SOURCES


# ---------------------------------------------------------------- compare_layer_execution(..., batch_matmul=True)
FC_KEYS = {"weight", "input", "rows", "d", "tokens", "mode", "signal", "error", "output_mse", "output_snr", "per_channel_error"}
BMM_KEYS = FC_KEYS | {"op", "operands", "adj_x", "adj_y", "batch", "activation_bits"}
MODELS = {"constant": (BC.build_constant_model, BC.CONSTANT_OPS), "attention": (BC.build_attention_model, BC.ATTENTION_OPS)}


@pytest.fixture(scope="module")
def mv():
  sys.path.insert(0, os.path.join(ROOT, "ai-edge-quantizer_amd"))
  from mi355q import model_validator
  return model_validator


@pytest.fixture(scope="module")
def built():
  sys.path.insert(0, os.path.join(ROOT, "ai-edge-quantizer_amd"))
  out = {}
  for key, (build, ops_list) in MODELS.items():
    model = build()
    out[key] = (model, BC.build_samples(model, ops_list), ops_list)
  return out


def _run(mv, float_model, target, samples, **kw):
  return mv.compare_layer_execution(float_model, target, samples, kernels=BC.numpy_kernels()(), **kw)


@pytest.mark.parametrize("which,mode,per_channel", [("constant", "static", True), ("constant", "static", False),
                                                    ("constant", "dynamic", True), ("constant", "weight_only", True),
                                                    ("attention", "static", True)])
def test_every_mode_gives_the_statements_figures(mv, built, which, mode, per_channel):
  model, samples, ops_list = built[which]
  tgt = BC.quantize_by_hand(model, samples, ops_list, mode, per_channel)
  rep = _run(mv, model, tgt, samples, batch_matmul=True, quantized_outputs=True)
  for op in ops_list:
    name, a_shape, b_shape, adj_x, adj_y, constant = op
    if mode == "dynamic" and adj_x:
      assert rep.skipped[f"{name}/y"] == mv.SKIP_BMM_DYNAMIC_ADJ_X
      continue
    r = rep.results[f"{name}/y"]
    want = BC.statement(model, tgt, samples, op, mode)
    assert (r["op"], r["operands"], r["mode"]) == ("BATCH_MATMUL", "constant" if constant else "activations", mode)
    assert (r["adj_x"], r["adj_y"], r["batch"]) == (adj_x, adj_y, int(np.prod(a_shape[:-2])))
    assert (r["rows"], r["d"], r["tokens"]) == (want["rows"], a_shape[-2] if adj_x else a_shape[-1], want["tokens"])
    assert r["input"] == f"{name}/a" and r["weight"] == (f"{name}/b" if constant else None)
    assert r["activation_bits"] == (8 if mode == "static" else None)
    for key in ("signal", "error"):
      np.testing.assert_allclose(r[key], want[key], rtol=1e-12)
    np.testing.assert_allclose(r["per_channel_error"], want["per_channel_error"], rtol=1e-12)
    np.testing.assert_allclose(r["output_mse"], want["error"] / want["rows"], rtol=1e-12)
    assert 0 < r["error"] < 1e-2 * r["signal"]
    if mode == "static":
      assert BMM_KEYS < set(r) and r["output_bits"] == 8 and r["fused_activation"] == "NONE" and "final_skipped" not in r
      np.testing.assert_allclose(r["final_error"], want["final_error"], rtol=1e-12)
      np.testing.assert_allclose(r["final_per_channel_error"], want["final_per_channel_error"], rtol=1e-12)
      assert r["final_error"] > 0
    else:
      assert r["output_bits"] is None and not [k for k in r if k.startswith("final") or k == "fused_activation"]
  assert rep.results["fc/y"]["op"] == "FULLY_CONNECTED"      # every entry carries `op` when the keyword is on


def test_without_the_keyword_nothing_changes(mv, built):
  for which in MODELS:
    model, samples, ops_list = built[which]
    tgt = BC.quantize_by_hand(model, samples, ops_list, "static")
    plain = _run(mv, model, tgt, samples)
    assert list(plain.results) == ["fc/y"] and plain.skipped == {} and set(plain.results["fc/y"]) == FC_KEYS
    on = _run(mv, model, tgt, samples, batch_matmul=True)
    assert set(on.results["fc/y"]) == FC_KEYS | {"op"}
    for key in FC_KEYS - {"per_channel_error"}:
      assert on.results["fc/y"][key] == plain.results["fc/y"][key], key
    assert np.array_equal(on.results["fc/y"]["per_channel_error"], plain.results["fc/y"]["per_channel_error"])
    assert set(on.results) == {"fc/y"} | {f"{op[0]}/y" for op in ops_list}
    assert set(on.results[f"{ops_list[0][0]}/y"]) == BMM_KEYS | ({"input_b"} if which == "attention" else set())
    other = _run(mv, model, tgt, samples, conv_2d=True, depthwise_conv_2d=True)      # the other keywords do not bring them in
    assert list(other.results) == ["fc/y"] and other.skipped == {}
    assert json_safe(on.as_dict())


def json_safe(d) -> bool:
  import json
  return bool(json.dumps(d))


def test_every_skip_reason_once(mv, built):
  import copy
  import types
  from mi355q import qtyping as q
  model, samples, ops_list = built["constant"]
  static = BC.quantize_by_hand(model, samples, ops_list, "static")

  def skipped(target, float_model=model, smp=samples, **kw):
    return _run(mv, float_model, target, smp, batch_matmul=True, **kw).skipped

  def mutated(fn, base=static):
    t = copy.deepcopy(base)
    fn(t, {x.name.decode(): x for x in t.subgraphs[0].tensors})
    return t
  # ---- the new reasons
  rank = [dict(s, **{"bmA/a": s["bmA/a"].reshape(-1)[:24]}) for s in samples]
  assert skipped(static, smp=rank)["bmA/y"] == mv.SKIP_BMM_RANK
  k_off = [dict(s, **{"bmA/a": s["bmA/a"][..., :23]}) for s in samples]
  assert skipped(static, smp=k_off)["bmA/y"] == mv.SKIP_BMM_RANK
  batch = [dict(s, **{"bmC/a": s["bmC/a"][:2]}) for s in samples]
  assert skipped(static, smp=batch)["bmC/y"] == mv.SKIP_BMM_BATCH

  def as_int16(t, by):
    w = by["bmA/b"]
    ints = np.asarray(t.buffers[w.buffer].data).view(np.int8).astype(np.int16)
    w.type = int(q.TensorType.INT16)
    t.buffers[w.buffer].data = ints.view(np.uint8)
  assert skipped(mutated(as_int16))["bmA/y"] == mv.SKIP_BMM_KIND

  def blockwise(t, by):
    by["bmA/b"].quantization.details = types.SimpleNamespace(blockSize=8, scales=0)
  assert skipped(mutated(blockwise))["bmA/y"] == mv.SKIP_BMM_BLOCKWISE

  def other_axis(t, by):
    by["bmA/b"].quantization = q.QuantizationParametersT(scale=np.full(24, 0.01, np.float32), zeroPoint=np.zeros(24, np.int64),
                                                         quantizedDimension=0)
  assert skipped(mutated(other_axis))["bmA/y"] == mv.SKIP_BMM_SCALE_AXIS
  dynamic = BC.quantize_by_hand(model, samples, ops_list, "dynamic")
  assert skipped(dynamic) == {"bmC/y": mv.SKIP_BMM_DYNAMIC_ADJ_X}

  def no_options(t, by):      # (an op without options has every default: both sides, and the entry is there)
    for o in t.subgraphs[0].operators:
      if by["bmA/y"] is t.subgraphs[0].tensors[o.outputs[0]]:
        o.builtinOptions, o.builtinOptionsType = None, 0
  bare = _run(mv, mutated(no_options, model), mutated(no_options), samples, batch_matmul=True)
  assert bare.results["bmA/y"]["adj_y"] is False and bare.skipped == {}

  def flipped(t, by):
    op = next(o for o in t.subgraphs[0].operators if by["bmB/y"] is t.subgraphs[0].tensors[o.outputs[0]])
    op.builtinOptions = q.BatchMatMulOptionsT(adjX=False, adjY=False)
  assert skipped(mutated(flipped))["bmB/y"] == mv.SKIP_BMM_MISMATCH

  def foreign_options(t, by):
    op = next(o for o in t.subgraphs[0].operators if by["bmB/y"] is t.subgraphs[0].tensors[o.outputs[0]])
    op.builtinOptions = q.FullyConnectedOptionsT(fusedActivationFunction=0)
  assert skipped(mutated(foreign_options))["bmB/y"] == mv.SKIP_BMM_MISMATCH
  long_ops = (("bmK", (1, 1, 32769), (32769, 1), False, False, True),)
  long_model = BC.build_model(long_ops, with_fc=False)
  long_samples = BC.build_samples(long_model, long_ops, with_fc=False)[:1]
  long_target = BC.quantize_by_hand(long_model, long_samples, long_ops, "static")
  assert skipped(long_target, float_model=long_model, smp=long_samples) == {"bmK/y": mv.SKIP_BMM_K}
  assert {k: v for k, v in skipped(copy.deepcopy(model)).items() if k != "fc/y"} == {f"{op[0]}/y": mv.SKIP_BMM_FLOAT for op in ops_list}
  a_model, a_samples, a_ops = built["attention"]
  float_skips = skipped(copy.deepcopy(a_model), float_model=a_model, smp=a_samples)
  assert (float_skips["qk/y"], float_skips["pv/y"]) == (mv.SKIP_BMM_FLOAT, mv.SKIP_BMM_FLOAT)
  # ---- the existing reasons that apply

  def int16_lhs(t, by):
    by["bmA/a"].type = int(q.TensorType.INT16)
  assert skipped(mutated(int16_lhs))["bmA/y"] == mv.SKIP_INT16

  def weight_zero_point(t, by):
    by["bmA/b"].quantization.zeroPoint = np.full(12, 3, np.int64)
  assert skipped(mutated(weight_zero_point))["bmA/y"] == mv.SKIP_WEIGHT_ZERO_POINT
  assert skipped(static, smp=[{k: v for k, v in s.items() if k != "bmA/a"} for s in samples])["bmA/y"] == mv.SKIP_NO_SAMPLE

  def two_scales(t, by):
    by["bmA/a"].quantization.scale = np.array([0.1, 0.2], np.float32)
  assert skipped(mutated(two_scales))["bmA/y"] == mv.SKIP_INPUT

  def renamed(t, by):
    by["bmA/y"].name = b"elsewhere"
  assert skipped(mutated(renamed))["bmA/y"] == mv.SKIP_TARGET
  a_static = BC.quantize_by_hand(a_model, a_samples, a_ops, "static")
  no_b = [{k: v for k, v in s.items() if k != "qk/b"} for s in a_samples]
  assert skipped(a_static, float_model=a_model, smp=no_b)["qk/y"] == mv.SKIP_NO_SAMPLE

  def int16_rhs(t, by):
    by["pv/b"].type = int(q.TensorType.INT16)
  assert skipped(mutated(int16_rhs, a_static), float_model=a_model, smp=a_samples)["pv/y"] == mv.SKIP_INT16
  # ---- the stored output: an output that is not INT8, and a grid with no multiplier in range

  def float_output(t, by):
    by["bmA/y"].type = int(q.TensorType.FLOAT32)
  rep = _run(mv, model, mutated(float_output), samples, batch_matmul=True, quantized_outputs=True)
  assert rep.results["bmA/y"]["final_skipped"] == mv.FINAL_SKIP_OUTPUT and "final_error" not in rep.results["bmA/y"]

  def tiny_output_scale(t, by):
    by["bmA/y"].quantization.scale = np.array([1e-30], np.float32)
  rep = _run(mv, model, mutated(tiny_output_scale), samples, batch_matmul=True, quantized_outputs=True)
  assert rep.results["bmA/y"]["final_skipped"] == mv.FINAL_SKIP_MULTIPLIER
  assert len({v for k, v in vars(mv).items() if k.startswith("SKIP_BMM_")}) == 9


def test_batch_matmul_options_and_the_quantizers_keyword(mv):
  import types
  from mi355q import qtyping as q
  from mi355q import quantizer
  assert mv.batch_matmul_options(types.SimpleNamespace(builtinOptions=None)) == {
      "adj_x": False, "adj_y": False, "asymmetric_quantize_inputs": False}
  op = types.SimpleNamespace(builtinOptions=q.BatchMatMulOptionsT(adjX=True, adjY=False))
  assert mv.batch_matmul_options(op) == {"adj_x": True, "adj_y": False, "asymmetric_quantize_inputs": False}
  assert mv.batch_matmul_options(types.SimpleNamespace(builtinOptions=q.FullyConnectedOptionsT())) is None
  for fn in (mv.compare_layer_execution, quantizer.Quantizer.validate_layer_execution):
    p = inspect.signature(fn).parameters["batch_matmul"]
    assert p.default is False
  for method in ("sample_nd", "bmm_constant", "bmm_float", "bmm_forward", "bmm_output"):
    assert hasattr(mv.LayerExecutionKernels, method)
