"""CPU checks of the sensitivity sweep: what mi355q_requant_delta_sweep_f32 refuses before a launch; the host walk
(model_validator.sweep_layer_sensitivity) with a NumPy stand-in for the kernels: routing, chunking, keys and derived
figures, the data-free mode, cheapest(), save(), the Quantizer methods' arguments and apply_layer_selection(); and that
csrc/sensitivity.hip is built and compiles for gfx950 without scratch."""
import ctypes
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
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

D, DKV, DFF = 64, 8, 96          # d = 64 for q / k / v / o / gate / up, 96 for down: BLOCKWISE_64 does not divide it
MIN_MAX = "min_max_uniform_quantize"


# ---------------------------------------------------------------- the entry point's refusals
@pytest.fixture(scope="module")
def lib():
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def test_entry_refuses_or_does_nothing_before_a_launch(lib):
  """Host buffers stand in for device pointers: every one of these calls returns before it launches."""
  buf = ctypes.create_string_buffer(4096)
  base = (ctypes.addressof(buf) + 15) & ~15
  p = ctypes.c_void_p(base)
  err = lib.mi355q_last_error

  def table(*values):
    return (ctypes.c_int32 * len(values))(*values)

  def call(rows=4, cols=128, bits=(4,), block=(0,), x=p, delta=p, stride=None, sq=None, count=None, tables=True):
    return lib.mi355q_requant_delta_sweep_f32(
        x, rows, cols, len(bits) if count is None else count, table(*bits) if tables else None,
        table(*block) if tables else None, delta, rows * cols if stride is None else stride, sq, None)

  for count in (0, -1, 9, 128):
    assert call(count=count) == -1 and b"count must be in [1, 8]" in err()
  assert call(bits=(4,) * 9, block=(0,) * 9) == -1 and b"count must be in [1, 8]" in err()
  assert call(tables=False, count=1) == -1 and b"candidate tables must not be null" in err()
  for bits in (0, 1, 3, 5, 16):
    assert call(bits=(8, bits), block=(0, 0)) == -1 and b"bits must be 8, 4 or 2" in err()
  for block in (-32, 1, 16, 48, 512):
    assert call(bits=(8, 4), block=(0, block)) == -1 and b"block must be 0, 32, 64, 128 or 256" in err()
  assert call(cols=96, bits=(4, 4), block=(32, 64)) == -1
  assert b"Quantized dimension 96 is not divisible by block size 64." in err()
  assert call(rows=-1) == -1 and b"negative shape" in err()
  assert call(cols=-4) == -1 and b"negative shape" in err()
  # an empty tensor enqueues nothing (also with null pointers), but a bad candidate is still refused
  assert call(rows=0, x=None, delta=None) == 0 and err() == b""
  assert call(cols=0, x=None, delta=None) == 0
  assert call(rows=0, bits=(3,)) == -1
  assert call(x=None) == -1 and b"x and delta_out must not be null" in err()
  assert call(delta=None) == -1 and b"x and delta_out must not be null" in err()
  assert call(stride=4 * 128 - 1) == -1 and b"smaller than rows * cols" in err()
  assert call(rows=1 << 31, cols=4, stride=1 << 40) == -3 and b"rows > 2^31-1" in err()
  assert call(rows=0) == 0 and err() == b""          # (and a call that succeeds clears the message)


def test_ops_wrapper_raises_the_reference_texts_without_a_device():
  import __graft_entry__ as g
  g.build()
  from mi355q import ops
  with pytest.raises(ValueError, match=r"Quantized dimension 96 in tensor shape \(4, 96\) is not divisible by block size 64\."):
    ops.check_sweep_candidates([(4, 0), (4, 64)], (4, 96))
  with pytest.raises(ValueError, match="bits must be 8, 4 or 2"):
    ops.check_sweep_candidates([(16, 0)], (4, 96))
  with pytest.raises(ValueError, match="block must be"):
    ops.check_sweep_candidates([(4, 8)], (4, 96))
  assert ops.check_sweep_candidates([(np.int64(4), np.int64(32))], (4, 96)) == [(4, 32)]


# ---------------------------------------------------------------- the host walk
def _oracle_params(w, candidate):
  from oracle import aeq_oracle as O
  gran = candidate.granularity_name
  key = candidate.algorithm_name
  if key == MIN_MAX:
    return O.min_max_quant_params(w, candidate.num_bits, candidate.symmetric, gran)
  if key == "MSE":
    return O.mse_quant_params(w, candidate.num_bits, gran, symmetric=candidate.symmetric)
  if key == "OCTAV":
    return O.octav_quant_params(w, candidate.num_bits, gran, symmetric=candidate.symmetric)
  raise AssertionError(key)


def _kernels():
  from mi355q import model_validator as mv
  from mi355q import qtyping
  from oracle import aeq_oracle as O

  class NumpySweepKernels(mv.SweepKernels):
    """What the device side computes, in NumPy: the fused candidates restated with the oracle's min/max and quantize
    functions, the generic ones with the oracle's algorithms."""
    calls = []

    def weight(self, values):
      return np.asarray(values, np.float32)

    def hessian(self, stat):
      return np.asarray(stat, np.float64).astype(np.float32), 1.0

    def quadform(self, a, rows, d, product, alpha):
      NumpySweepKernels.calls.append(("quadform", rows, d))
      return LC.exact_rows(np.asarray(a).reshape(rows, d), LC.symmetric(product), alpha)

    def stack(self, count, rows, d):
      NumpySweepKernels.calls.append(("stack", count))
      return np.zeros((count, rows * d), np.float32)

    def sweep_into(self, stack, first, reference, rows, d, pairs):
      NumpySweepKernels.calls.append(("sweep", tuple(pairs)))
      w = reference.reshape(rows, d)
      sq = np.zeros((len(pairs), rows))
      for i, (bits, block) in enumerate(pairs):
        p = O.min_max_quant_params(w, bits, True, f"BLOCKWISE_{block}" if block else "CHANNELWISE")
        channels, inner = (rows * d // block, block) if block else (rows, d)
        delta = reference - LC.dequantize(p["quantized_data"], np.ravel(p["scale"]), None, channels, inner, 8)
        stack[first + i] = delta
        sq[i] = np.sum(delta.reshape(rows, d).astype(np.float64) ** 2, axis=1)
      return sq

    def candidate_params(self, candidate, op_info, values, tensor_qsv):
      NumpySweepKernels.calls.append(("params", candidate.name))
      assert op_info.op_name == qtyping.TFLOperationName.FULLY_CONNECTED
      assert op_info.op_quant_config.weight_tensor_config == candidate.tensor_config()
      if candidate.algorithm_name == "GPTQ":        # (the update itself is the device's: a fixed perturbation here)
        assert "hessian" in tensor_qsv["activation_tensor_qsv"]
        p = O.min_max_quant_params(values, candidate.num_bits, True, candidate.granularity_name)
      else:
        assert tensor_qsv is None
        p = _oracle_params(values, candidate)
      return qtyping.UniformQuantParams(
          num_bits=p["num_bits"], quantized_dimension=p["quantized_dimension"], scale=p["scale"],
          zero_point=p["zero_point"], symmetric=p["symmetric"], quantized_data=p["quantized_data"],
          block_size=p["block_size"])

    def params_delta_into(self, stack, index, reference, rows, d, params):
      channels, inner = mv.scale_view(params, rows, d)
      zp = np.broadcast_to(np.ravel(params.zero_point).astype(np.int32), (channels,))
      delta = reference - LC.dequantize(params.quantized_data, np.ravel(params.scale), zp, channels, inner, 32)
      stack[index] = delta
      return np.sum(delta.reshape(1, rows, d).astype(np.float64) ** 2, axis=2)

    def energy(self, reference):
      return float(np.sum(np.asarray(reference, np.float64) ** 2))
  NumpySweepKernels.calls = []
  return NumpySweepKernels


def _model():
  import c5_model as C
  return C, C.build_model(1, d=D, dkv=DKV, dff=DFF)


def _weight(model, name):
  t = next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)
  return np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()


def _hessians(C):
  rng = np.random.default_rng(11)
  out = {}
  for _, _, cols, src in C.projections(D, DKV, DFF):
    if f"l0/{src}" not in out:
      x = rng.standard_normal((40, cols))
      out[f"l0/{src}"] = {"hessian": (2.0 / 4.0) * x.T @ x, "num_samples": np.array(4)}
  return out


def _candidates(mv):
  return [mv.SweepCandidate("w8", 8, "CHANNELWISE"), mv.SweepCandidate("w4", 4, "CHANNELWISE"),
          mv.SweepCandidate("w4b32", 4, "BLOCKWISE_32"), mv.SweepCandidate("w4b64", 4, "BLOCKWISE_64"),
          mv.SweepCandidate("w2", 2, "CHANNELWISE"),
          mv.SweepCandidate("asym4", 4, "CHANNELWISE", symmetric=False),
          mv.SweepCandidate("tensor8", 8, "TENSORWISE"),
          mv.SweepCandidate("octav4", 4, "CHANNELWISE", algorithm_key="OCTAV"),
          mv.SweepCandidate("mse4", 4, "CHANNELWISE", algorithm_key="MSE"),
          mv.SweepCandidate("mse4b32", 4, "BLOCKWISE_32", algorithm_key="MSE"),
          mv.SweepCandidate("gptq4", 4, "CHANNELWISE", algorithm_key="GPTQ"),
          mv.SweepCandidate("hadamard4", 4, "CHANNELWISE", algorithm_key="HADAMARD_ROTATION"),
          mv.SweepCandidate("oscar4", 4, "CHANNELWISE", algorithm_key="OSCAR")]


FUSED = ("w8", "w4", "w4b32", "w4b64", "w2")
GENERIC = ("asym4", "tensor8", "octav4", "mse4", "gptq4")


@pytest.fixture(scope="module")
def walked():
  from mi355q import model_validator as mv
  C, model = _model()
  qsvs = _hessians(C)
  kernels = _kernels()
  table = mv.sweep_layer_sensitivity(model, _candidates(mv), qsvs, kernels=kernels())
  return dict(C=C, mv=mv, model=model, qsvs=qsvs, table=table, calls=list(kernels.calls))


def test_every_candidate_takes_its_route_or_is_skipped_with_the_reason(walked):
  mv, table = walked["mv"], walked["table"]
  ys = [f"l0/{name}/y" for name, *_ in walked["C"].projections(D, DKV, DFF)]
  assert list(table) == ys and len(table) == 7
  for y in ys:
    down = y == "l0/down/y"                        # d = 96: blocks of 64 do not divide it
    assert sorted(table[y]) == sorted([c for c in FUSED + GENERIC if not (down and c == "w4b64")])
    for name, r in table[y].items():
      assert r["route"] == ("fused" if name in FUSED else "generic")
    assert table.skipped[(y, "hadamard4")] == mv.SKIP_BASIS and table.skipped[(y, "oscar4")] == mv.SKIP_BASIS
    assert "Blockwise quantization is not supported for MSE" in table.skipped[(y, "mse4b32")]
    if down:
      assert "Quantized dimension 96" in table.skipped[(y, "w4b64")] and "block size 64" in table.skipped[(y, "w4b64")]
  assert len(table.skipped) == 7 * 3 + 1
  # one sweep call per op with all its fused candidates, one stack and one quadratic form per op besides the signal
  sweeps = [c for c in walked["calls"] if c[0] == "sweep"]
  assert len(sweeps) == 7 and all(len(c[1]) == (4 if i == 6 else 5) for i, c in enumerate(sweeps))
  assert sweeps[0][1] == ((8, 0), (4, 0), (4, 32), (4, 64), (2, 0))
  assert sum(1 for c in walked["calls"] if c[0] == "stack") == 7
  # 7 signals (every weight is its own) + 7 stacked forms
  quads = [c for c in walked["calls"] if c[0] == "quadform"]
  assert len(quads) == 14 and quads[1] == ("quadform", 10 * D, D)


def test_keys_and_derived_figures(walked):
  from oracle import aeq_oracle as O
  table, mv = walked["table"], walked["mv"]
  cands = {c.name: c for c in _candidates(mv)}
  for name, rows, d, src in walked["C"].projections(D, DKV, DFF):
    y = f"l0/{name}/y"
    w = _weight(walked["model"], f"l0/{name}/w")
    h = np.float32(walked["qsvs"][f"l0/{src}"]["hessian"]).astype(np.float64)
    for cand, r in table[y].items():
      assert sorted(r) == sorted(["weight", "input", "rows", "d", "route", "weight_sq_error", "weight_snr",
                                  "bits_per_weight", "signal", "error", "output_mse", "output_snr", "per_channel_error"])
      assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
      c = cands[cand]
      p = _oracle_params(w, c) if cand != "gptq4" else O.min_max_quant_params(w, 4, True, "CHANNELWISE")
      deq = O.uniform_dequantize(p["quantized_data"], p["scale"], p["zero_point"], p["quantized_dimension"], p["block_size"])
      delta = w.astype(np.float64) - deq.astype(np.float64)
      np.testing.assert_allclose(r["weight_sq_error"], np.sum(delta ** 2), rtol=1e-5)
      np.testing.assert_allclose(r["per_channel_error"], LC.exact_rows(w - deq.astype(np.float32), h, 0.5), rtol=1e-4)
      assert r["error"] == float(np.sum(r["per_channel_error"])) and r["output_mse"] == r["error"] / rows
      np.testing.assert_allclose(r["signal"], LC.exact_rows(w, h, 0.5).sum(), rtol=1e-12)
      assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)
      assert r["weight_snr"] == float(np.sum(w.astype(np.float64) ** 2)) / (r["weight_sq_error"] + 1e-9 * rows * d)
    per = table[y]
    assert per["w8"]["bits_per_weight"] == 8 + 32.0 / d and per["w2"]["bits_per_weight"] == 2 + 32.0 / d
    assert per["w4b32"]["bits_per_weight"] == 4.5 and per["tensor8"]["bits_per_weight"] == 8 + 32.0 / (rows * d)
    if "w4b64" in per:
      assert per["w4b64"]["bits_per_weight"] == 4.25
    assert per["w8"]["error"] < per["w4"]["error"] < per["w2"]["error"]


def test_chunking_under_a_small_stack_gives_the_same_table(walked):
  mv = walked["mv"]
  kernels = _kernels()
  # room for three [DFF, D] deltas: the 11 candidates that reach the stack (mse4b32 is refused by its algorithm only
  # there) take four chunks of gate / up / down, three (4 + 4 + 3) of the [D, D] weights, and one of k / v (8 rows)
  small = mv.sweep_layer_sensitivity(walked["model"], _candidates(mv), walked["qsvs"], kernels=kernels(),
                                     max_stack_bytes=3 * DFF * D * 4)
  stacks = [c[1] for c in kernels.calls if c[0] == "stack"]
  assert stacks == [4, 4, 3, 11, 11, 4, 4, 3, 3, 3, 3, 2, 3, 3, 3, 2, 3, 3, 3, 1]      # (down: w4b64 never gets there)
  assert small.skipped == walked["table"].skipped
  for y in walked["table"]:
    assert list(small[y]) == list(walked["table"][y])
    for cand, r in walked["table"][y].items():
      for k, v in r.items():
        assert np.array_equal(small[y][cand][k], v), (y, cand, k)
  # one candidate per chunk when not even one delta fits
  kernels = _kernels()
  one = mv.sweep_layer_sensitivity(walked["model"], _candidates(mv)[:3], walked["qsvs"], kernels=kernels(), max_stack_bytes=1)
  assert {c[1] for c in kernels.calls if c[0] == "stack"} == {1}
  assert one["l0/q/y"]["w4b32"]["error"] == walked["table"]["l0/q/y"]["w4b32"]["error"]


def test_data_free_mode_reports_weight_figures_only(walked):
  mv = walked["mv"]
  kernels = _kernels()
  free = mv.sweep_layer_sensitivity(walked["model"], _candidates(mv), kernels=kernels())
  assert not [c for c in kernels.calls if c[0] == "quadform"]
  for y in walked["table"]:
    assert free.skipped[(y, "gptq4")] == mv.SKIP_NO_HESSIAN
    assert sorted(free[y]) == sorted(c for c in walked["table"][y] if c != "gptq4")
    for cand, r in free[y].items():
      assert sorted(r) == ["bits_per_weight", "d", "input", "route", "rows", "weight", "weight_snr", "weight_sq_error"]
      assert r["weight_sq_error"] == walked["table"][y][cand]["weight_sq_error"]
  pick = free.cheapest(min_weight_snr=100.0)
  assert set(pick) == set(free.results) and all(v is not None for v in pick.values())
  assert free.cheapest(min_output_snr=1.0) == {y: None for y in free.results}      # no output figures: nothing qualifies


def test_op_level_skips_are_those_of_compare_layer_outputs(walked):
  mv = walked["mv"]
  C, model = _model()
  qsvs = _hessians(C)
  del qsvs["l0/attn_in"]
  qsvs["l0/o_in"] = {"hessian": np.eye(D + 1), "num_samples": np.array(1)}
  t = next(t for t in model.subgraphs[0].tensors if t.name == b"l0/gate/w")
  model.buffers[t.buffer].data = None
  cands = _candidates(mv)[:2]
  got = mv.sweep_layer_sensitivity(model, cands, qsvs, kernels=_kernels()())
  assert sorted(got.results) == ["l0/down/y", "l0/up/y"]
  want = {"l0/q/y": mv.SKIP_NO_HESSIAN, "l0/k/y": mv.SKIP_NO_HESSIAN, "l0/v/y": mv.SKIP_NO_HESSIAN,
          "l0/o/y": mv.SKIP_ORDER, "l0/gate/y": mv.SKIP_WEIGHT}
  assert got.skipped == {(y, c.name): reason for y, reason in want.items() for c in cands}
  with pytest.raises(ValueError, match="candidate names must be unique"):
    mv.sweep_layer_sensitivity(model, [cands[0], cands[0]], qsvs, kernels=_kernels()())


def _table(mv, rows):
  """A LayerSensitivity from {op: {candidate: (bits per weight, output snr, weight snr)}}."""
  s = mv.LayerSensitivity("serving_default", [mv.SweepCandidate(c, 4, "CHANNELWISE") for c in ("a", "b", "c", "d")])
  for y, per in rows.items():
    s.results[y] = {c: {"bits_per_weight": b, "output_snr": o, "weight_snr": w} for c, (b, o, w) in per.items()}
  return s


def test_cheapest():
  from mi355q import model_validator as mv
  s = _table(mv, {"y0": {"a": (8.5, 1000.0, 900.0), "b": (4.5, 100.0, 90.0), "c": (4.5, 120.0, 80.0), "d": (2.5, 3.0, 2.0)},
                  "y1": {"a": (8.5, 50.0, 40.0), "b": (4.5, 5.0, 4.0)},
                  "y2": {"a": (8.5, float("nan"), 10.0)}})
  # the threshold on either side of a figure: at it the candidate qualifies, just above it no longer
  assert s.cheapest(min_output_snr=3.0) == {"y0": "d", "y1": "b", "y2": None}
  assert s.cheapest(min_output_snr=np.nextafter(3.0, 4.0)) == {"y0": "c", "y1": "b", "y2": None}      # a tie in bits: the larger SNR
  assert s.cheapest(min_output_snr=120.0) == {"y0": "c", "y1": None, "y2": None}
  assert s.cheapest(min_output_snr=121.0) == {"y0": "a", "y1": None, "y2": None}
  assert s.cheapest(min_output_snr=1001.0) == {"y0": None, "y1": None, "y2": None}
  # ... on the weight figure the tie goes the other way
  assert s.cheapest(min_weight_snr=10.0) == {"y0": "b", "y1": "a", "y2": "a"}
  for kwargs in ({}, {"min_output_snr": 1.0, "min_weight_snr": 1.0}):
    with pytest.raises(ValueError, match="exactly one of min_output_snr and min_weight_snr"):
      s.cheapest(**kwargs)


def test_save_leaves_the_per_channel_arrays_out(walked, tmp_path):
  table = walked["table"]
  path = table.save(str(tmp_path / "out"), "m")
  assert path.endswith("m_layer_sensitivity.json") and os.path.exists(path)
  saved = json.load(open(path))
  assert saved == json.loads(json.dumps(table.as_dict()))
  assert saved["candidates"] == [c.name for c in _candidates(walked["mv"])] and len(saved["layers"]) == 7
  assert saved["skipped"]["l0/down/y"]["hadamard4"] == walked["mv"].SKIP_BASIS
  for y, per in saved["layers"].items():
    for cand, entry in per.items():
      assert "per_channel_error" not in entry and entry["error"] == table[y][cand]["error"]
      assert entry["route"] == table[y][cand]["route"]


# ---------------------------------------------------------------- the Quantizer methods
def test_quantizer_sweep_arguments_and_route(monkeypatch):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  C, model = _model()
  qz = quantizer.Quantizer(model)              # no recipe, no quantize()
  cands = _candidates(mv)[:3]
  with pytest.raises(ValueError, match="at most one of calibration_result and calibration_data"):
    qz.sweep_layer_sensitivity(cands, calibration_result={}, calibration_data=[])
  with pytest.raises(ValueError, match="signature_key is required"):
    qz.sweep_layer_sensitivity(cands, calibration_data={"a": [], "b": []})
  with pytest.raises(ValueError, match="no samples for signature"):
    qz.sweep_layer_sensitivity(cands, calibration_data={"a": []}, signature_key="serving_default")
  monkeypatch.setattr(mv, "SweepKernels", _kernels())
  qsvs = _hessians(C)
  got = qz.sweep_layer_sensitivity(cands, calibration_result=qsvs)
  assert len(got) == 7 and not got.skipped and "output_snr" in got["l0/q/y"]["w4"]
  free = qz.sweep_layer_sensitivity(cands)
  assert len(free) == 7 and "output_snr" not in free["l0/q/y"]["w4"]
  assert free["l0/q/y"]["w4"]["weight_sq_error"] == got["l0/q/y"]["w4"]["weight_sq_error"]


@pytest.mark.parametrize("mode", ["weight_only", "dynamic"])
def test_apply_layer_selection_adds_one_anchored_entry_per_chosen_op(walked, mode):
  from mi355q import qtyping, quantizer, recipe_manager
  mv = walked["mv"]
  C, model = _model()
  # an op whose output name is a prefix of another's, and one with regex characters in it: neither may catch the other
  sg = model.subgraphs[0]
  next(t for t in sg.tensors if t.name == b"l0/k/y").name = b"l0/q/y2"
  next(t for t in sg.tensors if t.name == b"l0/v/y").name = b"l0/q.y"
  previous = C._fc("OCTAV", bits=8)      # pylint: disable=protected-access
  qz = quantizer.Quantizer(model, [previous])
  sens = mv.LayerSensitivity("serving_default", _candidates(mv))
  # (the config policy admits blockwise and 2-bit weights for dynamic-range ops only)
  first, third = ("w4b32", "w2") if mode == "dynamic" else ("w4", "w8")
  selection = {"l0/q/y": first, "l0/q/y2": None, "l0/o/y": "mse4", "l0/gate/y": third, "l0/down/y": None}
  before = qz.get_quantization_recipe()
  qz.apply_layer_selection(sens, selection, mode=mode)
  recipe = qz.get_quantization_recipe()
  assert recipe[:len(before)] == before and len(recipe) == len(before) + 3
  for entry in recipe[len(before):]:
    assert entry["regex"].startswith("^") and entry["regex"].endswith("$") and entry["operation"] == "FULLY_CONNECTED"
  manager = recipe_manager.RecipeManager()
  manager.load_quantization_recipe(recipe)
  fc = qtyping.TFLOperationName.FULLY_CONNECTED
  told_for = {"w4b32": (MIN_MAX, 4, "BLOCKWISE_32"), "w2": (MIN_MAX, 2, "CHANNELWISE"), "w4": (MIN_MAX, 4, "CHANNELWISE"),
              "w8": (MIN_MAX, 8, "CHANNELWISE")}
  want = {"l0/q/y": told_for[first], "l0/o/y": ("MSE", 4, "CHANNELWISE"), "l0/gate/y": told_for[third]}
  scopes = mv.fully_connected_scopes(model)
  assert scopes["l0/q/y"] == "l0/q/y;" and len(scopes) == 7
  def told(key, cfg):
    w = cfg.weight_tensor_config
    return str(getattr(key, "value", key)), w.num_bits, str(getattr(w.granularity, "value", w.granularity))

  for y, scope in scopes.items():
    key, cfg = manager.get_quantization_configs(fc, scope)
    w = cfg.weight_tensor_config
    if y in want:
      assert told(key, cfg) == want[y], y
      assert w.symmetric and cfg.explicit_dequantize == (mode == "weight_only")
      assert cfg.compute_precision == (qtyping.ComputePrecision.FLOAT if mode == "weight_only" else qtyping.ComputePrecision.INTEGER)
    else:                                        # the previous entry, untouched
      assert told(key, cfg) == ("OCTAV", 8, "CHANNELWISE"), y
      assert cfg.compute_precision == qtyping.ComputePrecision.INTEGER
  with pytest.raises(ValueError, match="mode must be"):
    qz.apply_layer_selection(sens, selection, mode="static")
  if mode == "weight_only":                       # what the policy refuses for the mode is refused here, by the policy
    with pytest.raises(ValueError, match="Unsupported op for"):
      qz.apply_layer_selection(sens, {"l0/q/y": "w4b32"}, mode=mode)
  with pytest.raises(ValueError, match="unknown candidate"):
    qz.apply_layer_selection(sens, {"l0/q/y": "w3"}, mode=mode)
  with pytest.raises(ValueError, match="no FULLY_CONNECTED op writes"):
    qz.apply_layer_selection(sens, {"l0/nothing/y": "w4"}, mode=mode)
  with pytest.raises(ValueError, match="asymmetric"):
    qz.apply_layer_selection(sens, {"l0/q/y": "asym4"}, mode=mode)


# ---------------------------------------------------------------- the kernels' build
def test_sensitivity_is_built():
  import __graft_entry__ as g
  assert "sensitivity.hip" in g.SOURCES


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_sensitivity_kernels_use_no_scratch(tmp_path):
  import __graft_entry__ as g
  out = str(tmp_path / "sensitivity.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "sensitivity.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  scratch = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  vgprs = re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", asm)
  lds = re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", asm)
  assert len(kernels) == 8 and len(scratch) == len(vgprs) == len(lds) == len(kernels)
  for name, s, v, l in zip(kernels, scratch, vgprs, lds):
    print(f"{name}: {v} VGPRs, {l} bytes of LDS, {s} bytes of scratch")
  assert sum("delta_sweep_rows_kernel" in k for k in kernels) == 7 and sum("delta_sweep_generic_kernel" in k for k in kernels) == 1
  assert all(int(s) == 0 for s in scratch), scratch
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
