"""Sensitivity sweep on the GPU (csrc/sensitivity.hip, ops.requant_delta_sweep, model_validator.sweep_layer_sensitivity,
Quantizer.sweep_layer_sensitivity / apply_layer_selection).

  1. ops.requant_delta_sweep bit for bit against the composition it replaces, ops.requant_sym -> ops.weight_delta, on
     every route of the kernel and every (bits, block) a shape admits, with zero rows, maxima in the last block, rint
     ties, NaN, inf and -0.0 planted; the float64 row sums against NumPy, and their bits in two runs;
  2. the stacked quadratic form [count * rows, d] on integer data against the int64 result;
  3. end to end on a one-layer decoder-shaped model: the fused candidates against quantize() + validate_layer_outputs
     with the matching recipe, the order of the bit widths, GPTQ against min/max, the data-free call, the
     calibration_data route, the Hadamard candidate in .skipped;
  4. cheapest() -> apply_layer_selection() -> quantize() -> validate_layer_outputs() gives back the sweep's figures.
"""
import os
import sys

import numpy as np
import pytest

import layer_error_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

BITS = (8, 4, 2)
BLOCKS = (32, 64, 128, 256)
QMAX = {8: 127, 4: 7, 2: 1}


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available()
  import __graft_entry__ as g
  g.build()
  from mi355q import ops

  class M:
    pass
  M.torch, M.ops = torch, ops
  M.dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
  return M


# ---------------------------------------------------------------- 1. bit for bit against the composition
# (rows, cols, misaligned): the smallest shapes that reach every route of the kernel
VECTOR = [(1, 4), (3, 32), (5, 96), (33, 128), (4, 256), (2, 4096), (1, 16384)]
ODD_COLS = [(7, 33), (3, 4098)]
LONG = [(2, 16388), (1, 32768)]
MISALIGNED = [(5, 96), (33, 128)]
PLANTS = ("none", "zero", "lastmax", "ties8", "ties4", "ties2", "nan", "inf", "negzero")


def _candidates(cols):
  return [(bits, block) for block in (0,) + tuple(b for b in BLOCKS if cols % b == 0) for bits in BITS]


def _plant(row, what):
  cols = row.size
  if what == "zero":                 # the 1e-9 floor of the scale
    row[:] = 0.0
  elif what == "lastmax":            # the maximum in the row's last block (and last piece)
    row[cols - 1] = 0.5
  elif what.startswith("ties"):      # x = (k + 1/2) s for a power-of-two s = max / qmax: exact rint ties up to both ends
    bits = int(what[4:])
    qmax, s = QMAX[bits], np.float32(2.0 ** -8)
    np.clip(row, -0.5 * qmax * s, 0.5 * qmax * s, out=row)
    values = [qmax * s, (qmax - 0.5) * s, -(qmax - 0.5) * s, 0.5 * s, -0.5 * s, 1.5 * s, -1.5 * s, 2.5 * s, -2.5 * s,
              -qmax * s]
    values = [v for v in values if abs(v) <= qmax * s][:cols]
    row[:len(values)] = values
  elif what == "nan":
    row[cols // 2] = np.nan
  elif what == "inf":
    row[min(1, cols - 1)] = np.inf
  elif what == "negzero":
    row[0] = -0.0
    row[cols - 1] = -0.0


def _inputs(rows, cols):
  """Arrays [rows, cols], normal * 0.02, that between them carry every plant (one plant per row)."""
  rng = np.random.default_rng(rows * 100003 + cols)
  out = []
  for first in range(0, len(PLANTS), rows):
    x = (rng.standard_normal((rows, cols)) * 0.02).astype(np.float32)
    for r, what in enumerate(PLANTS[first:first + rows]):
      _plant(x[r], what)
    out.append(x)
  return out


def _composition(m, x, bits, block):
  rows, cols = x.shape
  r = m.ops.requant_sym(x, block, bits, want_q=True)
  n = r["scale"].numel()
  target = m.ops.CompareTarget(r["q"], rows * cols, "i8", r["scale"].reshape(-1), None, n, block or cols, 8)
  return m.ops.weight_delta(x, target)


def _check_sweep(m, x_dev, cands):
  torch = m.torch
  rows, cols = x_dev.shape
  delta, sq = m.ops.requant_delta_sweep(x_dev, cands)
  assert delta.shape == (len(cands), rows, cols) and delta.dtype == torch.float32 and delta.is_contiguous()
  assert sq.shape == (len(cands), rows) and sq.dtype == torch.float64
  for k, (bits, block) in enumerate(cands):
    want = _composition(m, x_dev, bits, block)
    same = torch.equal(delta[k].reshape(-1).view(torch.int32), want.view(torch.int32))
    if not same:
      bad = (delta[k].reshape(-1).view(torch.int32) != want.view(torch.int32)).nonzero().reshape(-1)[:4].tolist()
      raise AssertionError(f"{rows}x{cols} bits {bits} block {block}: differs from requant_sym -> weight_delta at {bad}")
  # the float64 row sums: any summation order of non-negative terms stays within cols * 2^-52 of the sum
  host, got = delta.cpu().numpy().astype(np.float64), sq.cpu().numpy()
  with np.errstate(over="ignore", invalid="ignore"):
    ref = np.sum(host * host, axis=2)
  finite = np.isfinite(ref)
  assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
  assert np.all(np.abs(got[finite] - ref[finite]) <= cols * 2.0 ** -52 * ref[finite])
  _, again = m.ops.requant_delta_sweep(x_dev, cands)
  assert np.array_equal(again.cpu().numpy().view(np.uint64), got.view(np.uint64))
  assert m.ops.requant_delta_sweep(x_dev, cands[:1], want_sq=False)[1] is None


def _shape_cases():
  cases = [pytest.param(r, c, False, id=f"{r}x{c}") for r, c in VECTOR + ODD_COLS + LONG]
  return cases + [pytest.param(r, c, True, id=f"{r}x{c}-misaligned") for r, c in MISALIGNED]


@pytest.mark.parametrize("rows,cols,misaligned", _shape_cases())
def test_sweep_equals_requant_then_weight_delta_bit_for_bit(m, rows, cols, misaligned):
  cands = _candidates(cols)
  assert len(cands) == 3 * (1 + sum(cols % b == 0 for b in BLOCKS))
  for x in _inputs(rows, cols):
    if misaligned:                   # a view 4 bytes into its buffer
      base = m.torch.empty(rows * cols + 1, dtype=m.torch.float32, device="cuda")
      x_dev = base[1:].view(rows, cols)
      x_dev.copy_(m.dev(x))
      assert x_dev.data_ptr() % 16 == 4
    else:
      x_dev = m.dev(x)
    _check_sweep(m, x_dev, cands)                         # every candidate in one call (split when there are 9+)
  # ... a call of 9+ candidates (split into several launches) and one of at most 8 (a single launch) for every shape
  x_dev = m.dev(_inputs(rows, cols)[0])
  many = cands if len(cands) > 8 else cands * 3
  assert len(many) >= 9
  _check_sweep(m, x_dev, many)
  _check_sweep(m, x_dev, many[1:8])


def test_sweep_refuses_bad_candidates_before_touching_the_device(m):
  x = m.dev(np.zeros((4, 96), np.float32))
  with pytest.raises(ValueError, match="Quantized dimension 96 in tensor shape .* is not divisible by block size 64"):
    m.ops.requant_delta_sweep(x, [(4, 0), (4, 64)])
  with pytest.raises(ValueError, match="bits must be 8, 4 or 2"):
    m.ops.requant_delta_sweep(x, [(3, 0)])
  with pytest.raises(ValueError, match="block must be"):
    m.ops.requant_delta_sweep(x, [(4, 16)])
  with pytest.raises(ValueError, match="at least one candidate"):
    m.ops.requant_delta_sweep(x, [])
  delta, sq = m.ops.requant_delta_sweep(m.dev(np.zeros((0, 96), np.float32)), [(4, 0)])
  assert delta.shape == (1, 0, 96) and sq.shape == (1, 0)


# ---------------------------------------------------------------- 2. the stacked quadratic form
@pytest.mark.parametrize("d", [33, 64, 200])
@pytest.mark.parametrize("rows", [5, 130])
def test_stacked_quadform_is_exact_on_integer_data(m, d, rows):
  count = 3
  rng = np.random.default_rng(9000 + d + rows)
  low = np.tril(rng.integers(-7, 7, size=(d, d), endpoint=True))
  psym = low + np.tril(low, -1).T
  a = rng.integers(-3, 3, size=(count, rows, d), endpoint=True)
  want = ((a.reshape(-1, d) @ psym) * a.reshape(-1, d)).sum(axis=1)          # int64, below d^2 * 63 < 2^24
  assert np.abs(want).max() < 1 << 24
  stack, p_dev = m.dev(a.astype(np.float32)), m.dev(psym.astype(np.float32))
  got = m.ops.quadform_rows(stack.view(count * rows, d), p_dev, 0.5).cpu().numpy()
  assert got.dtype == np.float64 and np.array_equal(got, 0.5 * want.astype(np.float64))
  # a row's form does not depend on where the row sits in the stack
  for k in range(count):
    alone = m.ops.quadform_rows(stack[k], p_dev, 0.5).cpu().numpy()
    assert np.array_equal(alone.view(np.uint64), got[k * rows:(k + 1) * rows].view(np.uint64))


# ---------------------------------------------------------------- 3. end to end
D, DKV, DFF = 128, 32, 256          # the sizes of test_gpu_layer_error.py's one-layer model
FUSED = {"w8": (8, "CHANNELWISE"), "w4": (4, "CHANNELWISE"), "w4b32": (4, "BLOCKWISE_32"), "w2": (2, "CHANNELWISE")}
MIN_MAX = "min_max_uniform_quantize"


def _all_candidates(mv):
  c = [mv.SweepCandidate(name, bits, gran) for name, (bits, gran) in FUSED.items()]
  c += [mv.SweepCandidate("octav4", 4, "CHANNELWISE", algorithm_key="OCTAV"),
        mv.SweepCandidate("mse4", 4, "CHANNELWISE", algorithm_key="MSE"),
        mv.SweepCandidate("gptq4", 4, "CHANNELWISE", algorithm_key="GPTQ"),
        mv.SweepCandidate("asym4", 4, "CHANNELWISE", symmetric=False),
        mv.SweepCandidate("hadamard4", 4, "CHANNELWISE", algorithm_key="DECOMPOSED_HADAMARD_ROTATION")]
  return c


def _recipe(C, bits, granularity):
  entry = C._fc(MIN_MAX, bits=bits)      # pylint: disable=protected-access
  entry["op_config"]["weight_tensor_config"]["granularity"] = granularity
  return [entry]


@pytest.fixture(scope="module")
def sweep(m):
  import c5_model as C
  from mi355q import model_validator as mv, quantizer
  projections = C.projections(D, DKV, DFF)
  model = C.build_model(1, d=D, dkv=DKV, dff=DFF)
  weights = {}
  for t in model.subgraphs[0].tensors:
    name = t.name.decode()
    if name.endswith("/w"):
      weights[name] = np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()
  samples = LC.calibration_samples(projections)
  qsvs = quantizer.Quantizer(model, C.recipe("gptq")).calibrate({"serving_default": samples})
  cands = _all_candidates(mv)
  table = quantizer.Quantizer(model).sweep_layer_sensitivity(cands, calibration_result=qsvs)
  validated = {}
  for name, (bits, gran) in FUSED.items():
    qz = quantizer.Quantizer(model, _recipe(C, bits, gran))
    qz.quantize()
    validated[name] = qz.validate_layer_outputs(calibration_result=qsvs)
  return dict(C=C, mv=mv, quantizer=quantizer, projections=projections, model=model, weights=weights, samples=samples,
              qsvs=qsvs, cands=cands, table=table, validated=validated)


def _gates(sweep, name, src, cand):
  """(per-row gate of the signal, per-row gate of the error): 8 d u S_r of W and of the candidate's dW, the delta
  restated with the oracle's min/max parameters."""
  from oracle import aeq_oracle as O
  bits, gran = FUSED[cand]
  w = sweep["weights"][f"l0/{name}/w"]
  rows, d = w.shape
  p = O.min_max_quant_params(w, bits, True, gran)
  block = O.block_size_of(gran)
  channels, inner = (rows * d // block, block) if block else (rows, d)
  delta = (w.ravel() - LC.dequantize(p["quantized_data"], np.ravel(p["scale"]), None, channels, inner, 32)).reshape(rows, d)
  h = np.asarray(sweep["qsvs"][f"l0/{src}"]["hessian"])
  assert h.dtype == np.float64 and h.shape == (d, d)
  return LC.gate_rows(w, h, 0.5), LC.gate_rows(delta, h, 0.5)


def test_routes_and_skips(sweep):
  table, mv = sweep["table"], sweep["mv"]
  ys = [f"l0/{name}/y" for name, *_ in sweep["projections"]]
  assert list(table) == ys
  assert table.skipped == {(y, "hadamard4"): mv.SKIP_BASIS for y in ys}
  for y in ys:
    assert sorted(table[y]) == sorted(["w8", "w4", "w4b32", "w2", "octav4", "mse4", "gptq4", "asym4"])
    for cand, r in table[y].items():
      assert r["route"] == ("fused" if cand in FUSED else "generic"), (y, cand)
      assert r["error"] == float(np.sum(r["per_channel_error"])) and r["output_mse"] == r["error"] / r["rows"]
      assert r["output_snr"] == (r["signal"] / r["rows"]) / (r["output_mse"] + 1e-9)
      assert r["weight_sq_error"] > 0 and r["per_channel_error"].shape == (r["rows"],)


@pytest.mark.parametrize("cand", list(FUSED))
def test_fused_candidates_equal_quantize_then_validate_layer_outputs(sweep, cand):
  """The sweep's delta is x - fl(float(q) s) and validate_layer_outputs' is x - float(double(q) double(s)): the same
  exact product rounded once, so the same bits; and a row's quadratic form does not depend on where the row sits in
  the stack. Both within the derived gate, and equal."""
  table, val = sweep["table"], sweep["validated"][cand]
  assert not val.skipped
  for name, rows, d, src in sweep["projections"]:
    y = f"l0/{name}/y"
    a, b = table[y][cand], val[y]
    gate_s, gate_e = _gates(sweep, name, src, cand)
    print(f"{cand} {y}: |signal diff| / gate {abs(a['signal'] - b['signal']) / gate_s.sum():.3e},"
          f" |error diff| / gate {abs(a['error'] - b['error']) / gate_e.sum():.3e},"
          f" worst row {np.max(np.abs(a['per_channel_error'] - b['per_channel_error']) / gate_e):.3e}")
    assert (a["weight"], a["input"], a["rows"], a["d"]) == (b["weight"], b["input"], rows, d)
    assert abs(a["signal"] - b["signal"]) <= gate_s.sum() and abs(a["error"] - b["error"]) <= gate_e.sum()
    assert np.all(np.abs(a["per_channel_error"] - b["per_channel_error"]) <= gate_e)
    assert a["signal"] == b["signal"] and a["error"] == b["error"]
    assert np.array_equal(a["per_channel_error"].view(np.uint64), b["per_channel_error"].view(np.uint64))


def test_fewer_bits_more_error_and_gptq_halves_min_max(sweep):
  table = sweep["table"]
  for y in table:
    r = table[y]
    print(f"{y}: SNR w8 {r['w8']['output_snr']:.3e} w4 {r['w4']['output_snr']:.3e} w2 {r['w2']['output_snr']:.3e};"
          f" GPTQ-4 / w4 error {r['gptq4']['error'] / r['w4']['error']:.3f}")
    assert r["w8"]["error"] < r["w4"]["error"] < r["w2"]["error"], y
    assert r["gptq4"]["error"] < 0.5 * r["w4"]["error"], y
    assert r["w4"]["bits_per_weight"] == 4 + 32.0 / r["w4"]["d"] and r["w4b32"]["bits_per_weight"] == 4.5


def test_data_free_call_reports_the_same_weight_figures(sweep):
  mv = sweep["mv"]
  free = sweep["quantizer"].Quantizer(sweep["model"]).sweep_layer_sensitivity(sweep["cands"])
  ys = list(sweep["table"])
  assert list(free) == ys
  assert free.skipped == {**{(y, "hadamard4"): mv.SKIP_BASIS for y in ys}, **{(y, "gptq4"): mv.SKIP_NO_HESSIAN for y in ys}}
  for y in ys:
    for cand, r in free[y].items():
      assert sorted(r) == ["bits_per_weight", "d", "input", "route", "rows", "weight", "weight_snr", "weight_sq_error"]
      assert r["weight_sq_error"] == sweep["table"][y][cand]["weight_sq_error"], (y, cand)
      assert r["weight_snr"] == sweep["table"][y][cand]["weight_snr"]


def test_calibration_data_route_gives_the_same_figures(sweep):
  # (without GPTQ: its integers depend on the Hessian's last bits, and the two routes' Hessians differ by float32
  # summation order)
  cands = [c for c in sweep["cands"] if c.name != "gptq4"]
  got = sweep["quantizer"].Quantizer(sweep["model"]).sweep_layer_sensitivity(
      cands, calibration_data={"serving_default": sweep["samples"]})
  for y in sweep["table"]:
    for c in cands:
      if c.name == "hadamard4":
        continue
      a, b = got[y][c.name], sweep["table"][y][c.name]
      np.testing.assert_allclose([a["signal"], a["error"]], [b["signal"], b["error"]], rtol=1e-6)
      assert a["weight_sq_error"] == b["weight_sq_error"]


# ---------------------------------------------------------------- 4. selection round trip
def test_selection_round_trip(sweep):
  mv, table = sweep["mv"], sweep["table"]
  fused = mv.LayerSensitivity(table.signature_key, [c for c in sweep["cands"] if c.name in FUSED])
  fused.results = {y: {c: r for c, r in per.items() if c in FUSED} for y, per in table.results.items()}
  # a threshold between the int4 SNRs of the best and the worst projection: some ops stay at w4, the others go up
  snr4 = [per["w4"]["output_snr"] for per in fused.results.values()]
  threshold = float(np.sqrt(min(snr4) * max(snr4)))
  selection = fused.cheapest(min_output_snr=threshold)
  print("threshold", threshold, "selection", selection)
  assert None not in selection.values() and len(set(selection.values())) >= 2
  qz = sweep["quantizer"].Quantizer(sweep["model"])
  qz.apply_layer_selection(fused, selection, mode="dynamic")
  assert len(qz.get_quantization_recipe()) == len(selection)
  qz.quantize()
  val = qz.validate_layer_outputs(calibration_result=sweep["qsvs"])
  assert not val.skipped
  for name, rows, d, src in sweep["projections"]:
    y = f"l0/{name}/y"
    a, b = fused[y][selection[y]], val[y]
    _, gate_e = _gates(sweep, name, src, selection[y])
    assert a["output_snr"] >= threshold
    assert abs(a["error"] - b["error"]) <= gate_e.sum() and np.all(np.abs(a["per_channel_error"] - b["per_channel_error"]) <= gate_e)
    assert a["error"] == b["error"] and np.array_equal(a["per_channel_error"], b["per_channel_error"])
