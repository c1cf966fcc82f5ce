"""The effective-weight delta behind an inserted transformation on the GPU (mi355q_weight_delta_transformed_f32 in
csrc/hadamard.hip, ops.weight_delta_transformed, compare_layer_outputs(follow_input_transforms=True)).

  1. bit for bit against the three-launch composition (dequantize, rotate or multiply, subtract) on every route: the
     radix-2 kernel with several vectors per block and a partial last block, the 4096 tile with several vectors per tile
     and a partial last tile, the 8192 and 16384 tiles; every target kind; rows that are no multiple of 4; operands
     offset by one float; neither transformation = weight_delta;
  2. hadamard_rotate itself against a float64 Sylvester product, inside the bound of tests/test_gpu_ops.py;
  3. non-finite scales land where the composition puts them;
  4. end to end on a one-layer decoder-shaped model: the mixed recipe, a custom-op Hadamard recipe and an OSCAR recipe
     report all seven projections, each error inside a derived gate of a float64 evaluation from the written model.
"""
import os
import sys

import numpy as np
import pytest

import layer_error_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


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
KINDS = ("i4-channel", "i4-block32", "i8-zp", "i2", "f16")


def _packed(q, bits):
  per = 8 // bits
  q = np.concatenate([q, np.zeros(-q.size % per, q.dtype)])      # whole bytes
  return LC.pack(q, bits)


def _with_kinds(shapes):
  """Every target kind for every shape its scale view fits (blockwise-32 needs d % 32 == 0)."""
  return [pytest.param(kind, *shape, id=f"{kind}-" + "x".join(str(v) for v in shape))
          for shape in shapes for kind in KINDS if kind != "i4-block32" or shape[-1] % 32 == 0]


def _target(m, kind, rows, d, seed, scale_edit=None):
  """A CompareTarget of `kind` for a [rows, d] weight."""
  rng = np.random.default_rng(seed)
  n = rows * d
  if kind == "f16":
    return m.ops.CompareTarget(m.dev((rng.standard_normal(n) * 0.02).astype(np.float16)), n, "f16")
  bits = {"i4-channel": 4, "i4-block32": 4, "i8-zp": 8, "i2": 2}[kind]
  if kind == "i4-block32":
    channels, inner = n // 32, 32
  else:
    channels, inner = rows, d
  q = rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, size=n, endpoint=True)
  scale = (np.exp(rng.normal(size=channels)) * 0.01).astype(np.float32)
  if scale_edit is not None:
    scale_edit(scale)
  zp = rng.integers(-100, 100, size=channels, endpoint=True).astype(np.int32) if kind == "i8-zp" else None
  diff_bits = {"i4-channel": 32, "i4-block32": 32, "i8-zp": 16, "i2": 8}[kind]
  stored = q.astype(np.int8) if bits == 8 else _packed(q, bits)
  return m.ops.CompareTarget(m.dev(stored), n, kind[:2], m.dev(scale), None if zp is None else m.dev(zp), channels, inner,
                             diff_bits)


def _same_bits(m, got, want):
  torch = m.torch
  assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
  nan = torch.isnan(want)
  assert torch.equal(torch.isnan(got), nan)
  assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


def _reference(m, rows, d, seed):
  return m.dev((np.random.default_rng(seed).standard_normal(rows * d) * 0.02).astype(np.float32))


def _dequantized(m, target):
  return -m.ops.weight_delta(m.torch.zeros(target.n, dtype=m.torch.float32, device="cuda"), target)


def _hadamard_shapes():
  shapes = [(5, h, mult * h) for h in (2, 8, 128) for mult in (1, 3)]             # radix-2, partial last block
  shapes += [(3, h, mult * h) for h in (256, 1024, 4096) for mult in (1, 3)]      # 4096 tile, partial last tile
  shapes += [(3, h, h) for h in (8192, 16384)]
  return shapes


@pytest.mark.parametrize("kind,rows,h,d", _with_kinds(_hadamard_shapes()))
def test_hadamard_form_equals_dequantize_rotate_subtract(m, kind, rows, h, d):
  target = _target(m, kind, rows, d, seed=h + d + rows)
  w = _reference(m, rows, d, seed=7 * h + d)
  want = w - m.ops.hadamard_rotate(_dequantized(m, target), h)
  got = m.ops.weight_delta_transformed(w, target, d, hadamard_size=h)
  _same_bits(m, got, want)


@pytest.mark.parametrize("kind,rows,d", _with_kinds([(5, 37), (5, 96), (33, 128), (3, 4100)]))
def test_multiply_form_equals_dequantize_multiply_subtract(m, kind, rows, d):
  target = _target(m, kind, rows, d, seed=rows + d)
  w = _reference(m, rows, d, seed=rows * d)
  mult = m.dev(np.exp(np.random.default_rng(d).normal(size=d)).astype(np.float32))
  product = _dequantized(m, target).view(rows, d) * mult.view(1, d)      # rounded to float32 ...
  want = w - product.view(-1)                                            # ... then subtracted
  got = m.ops.weight_delta_transformed(w, target, d, multiplier=mult)
  _same_bits(m, got, want)


@pytest.mark.parametrize("kind,rows,d", _with_kinds([(5, 37), (5, 96)]))
def test_neither_transformation_is_weight_delta(m, kind, rows, d):
  target = _target(m, kind, rows, d, seed=rows + d)
  w = _reference(m, rows, d, seed=3)
  for h in (0, 1):
    _same_bits(m, m.ops.weight_delta_transformed(w, target, d, hadamard_size=h), m.ops.weight_delta(w, target))


@pytest.mark.parametrize("h,rows", [(128, 5), (1024, 3)])
@pytest.mark.parametrize("kind", ["i4-channel", "f16"])
def test_operands_offset_by_one_float_give_the_aligned_bits(m, kind, h, rows):
  """The network is chosen from h alone: a misaligned reference / delta_out only makes the accesses scalar."""
  from mi355q import _ffi, runtime as rt
  torch = m.torch
  d = 3 * h
  n = rows * d
  target = _target(m, kind, rows, d, seed=h)
  w = _reference(m, rows, d, seed=h + 1)
  aligned = m.ops.weight_delta_transformed(w, target, d, hadamard_size=h)
  w_off = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
  w_off[1:] = w
  out_off = torch.full((n + 2,), 123.0, dtype=torch.float32, device="cuda")
  ref_view, out_view = w_off[1:], out_off[1:n + 1]
  assert ref_view.data_ptr() % 16 == 4 and out_view.data_ptr() % 16 == 4
  _ffi.check(_ffi.lib().mi355q_weight_delta_transformed_f32(
      rt.ptr(ref_view), rt.ptr(target.data), n, m.ops.COMPARE_KINDS[target.kind], target.diff_bits, target.channels,
      target.inner, rt.ptr(target.scale), rt.ptr(target.zero_point), d, None, h, rt.ptr(out_view), rt.stream_ptr()))
  _same_bits(m, out_view.clone(), aligned)
  assert float(out_off[0]) == 123.0 and float(out_off[n + 1]) == 123.0      # nothing outside the n elements


def test_multiply_form_with_offset_operands(m):
  from mi355q import _ffi, runtime as rt
  torch = m.torch
  rows, d = 5, 96
  n = rows * d
  target = _target(m, "i4-channel", rows, d, seed=1)
  w = _reference(m, rows, d, seed=2)
  mult = m.dev(np.exp(np.random.default_rng(5).normal(size=d)).astype(np.float32))
  aligned = m.ops.weight_delta_transformed(w, target, d, multiplier=mult)
  w_off = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
  w_off[1:] = w
  out_off = torch.full((n + 2,), 123.0, dtype=torch.float32, device="cuda")
  ref_view, out_view = w_off[1:], out_off[1:n + 1]
  _ffi.check(_ffi.lib().mi355q_weight_delta_transformed_f32(
      rt.ptr(ref_view), rt.ptr(target.data), n, m.ops.COMPARE_KINDS[target.kind], target.diff_bits, target.channels,
      target.inner, rt.ptr(target.scale), rt.ptr(target.zero_point), d, rt.ptr(mult), 0, rt.ptr(out_view),
      rt.stream_ptr()))
  _same_bits(m, out_view.clone(), aligned)
  assert float(out_off[0]) == 123.0 and float(out_off[n + 1]) == 123.0


def test_ops_refuses_bad_arguments(m):
  target = _target(m, "i8-zp", 5, 96, seed=0)
  w = _reference(m, 5, 96, seed=0)
  mult = m.torch.ones(96, dtype=m.torch.float32, device="cuda")
  with pytest.raises(ValueError, match="not a multiple of the row length"):
    m.ops.weight_delta_transformed(w, target, 7)
  with pytest.raises(ValueError, match="power of 2"):
    m.ops.weight_delta_transformed(w, target, 96, hadamard_size=12)
  with pytest.raises(ValueError, match="must divide the row length"):
    m.ops.weight_delta_transformed(w, target, 96, hadamard_size=64)
  with pytest.raises(ValueError, match="at once"):
    m.ops.weight_delta_transformed(w, target, 96, multiplier=mult, hadamard_size=32)
  with pytest.raises(ValueError, match="multiplier has 48 elements"):
    m.ops.weight_delta_transformed(w, target, 96, multiplier=mult[:48])
  with pytest.raises(ValueError, match="same size"):
    m.ops.weight_delta_transformed(w[:-1], target, 96)


# ---------------------------------------------------------------- 2. hadamard_rotate is unchanged
def _fwht64(x, h):
  """reshape(x, (-1, h)) @ (Sylvester H_h / sqrt(h)) in float64, by butterflies (H_16384 is 2 GiB as a matrix)."""
  y = np.asarray(x, np.float64).reshape(-1, h)
  n = y.shape[0]
  step = 1
  while step < h:
    y = y.reshape(n, h // (2 * step), 2, step)
    y = np.stack([y[:, :, 0, :] + y[:, :, 1, :], y[:, :, 0, :] - y[:, :, 1, :]], axis=2)
    step *= 2
  return y.reshape(n, h) / np.sqrt(h)


@pytest.mark.parametrize("h", [2, 8, 128, 256, 1024, 4096, 8192, 16384])
def test_hadamard_rotate_stays_inside_its_bound(m, h):
  """The bound of test_hadamard_rotate_all_sizes_partial_tiles_and_in_place: 2e-6 max|x| sqrt(h) per vector."""
  from mi355q.transformations import graph_edits
  rng = np.random.default_rng(h)
  n_vec = 5 if h < 256 else 3
  x = rng.standard_normal((n_vec, h)).astype(np.float32)
  want = _fwht64(x, h)
  if h <= 1024:      # the butterflies are the Sylvester product
    dense = x.astype(np.float64) @ graph_edits._sylvester_hadamard(h)      # pylint: disable=protected-access
    assert np.allclose(want, dense, rtol=0, atol=1e-12 * np.sqrt(h))
  got = m.ops.hadamard_rotate(m.dev(x), h).cpu().numpy()
  tol = 2e-6 * np.abs(x).max(axis=1, keepdims=True) * np.sqrt(h)
  print(f"hadamard_rotate h={h}: worst |gpu - float64| / bound = {float(np.max(np.abs(got - want) / tol)):.3e}")
  assert got.dtype == np.float32 and np.all(np.abs(got - want) <= tol)


# ---------------------------------------------------------------- 3. non-finite scales
@pytest.mark.parametrize("form,rows,d,h", [("multiply", 5, 96, 0), ("hadamard", 5, 128, 128), ("hadamard", 5, 1024, 1024)])
def test_non_finite_scales_pass_through(m, form, rows, d, h):
  def edit(scale):
    scale[0], scale[-1] = np.inf, np.nan
    if scale.size > 2:
      scale[1] = -np.inf
  target = _target(m, "i8-zp", rows, d, seed=11, scale_edit=edit)
  w = _reference(m, rows, d, seed=12)
  dq = _dequantized(m, target)
  if form == "multiply":
    mult = m.dev(np.exp(np.random.default_rng(5).normal(size=d)).astype(np.float32))
    want = w - (dq.view(rows, d) * mult.view(1, d)).view(-1)
    got = m.ops.weight_delta_transformed(w, target, d, multiplier=mult)
  else:
    want = w - m.ops.hadamard_rotate(dq, h)
    got = m.ops.weight_delta_transformed(w, target, d, hadamard_size=h)
  assert int(m.torch.isnan(want).sum()) > 0 and int(m.torch.isfinite(want).sum()) > 0
  _same_bits(m, got, want)


# ---------------------------------------------------------------- 4. end to end
D, DKV, DFF = 128, 32, 256


@pytest.fixture(scope="module")
def chain(m):
  import c5_model as C
  from mi355q import model_validator as mv
  from mi355q import quantizer
  from mi355q.utils import tfl_flatbuffer_utils
  projections = C.projections(D, DKV, DFF)
  model = C.build_model(1, d=D, dkv=DKV, dff=DFF)
  weights = {}
  for t in model.subgraphs[0].tensors:
    name = t.name.decode()
    if name.endswith("/w"):
      weights[name] = np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()
  samples = LC.calibration_samples(projections)
  out = dict(C=C, projections=projections, weights=weights, samples=samples)
  fc = C._fc      # pylint: disable=protected-access
  recipes = {"mixed": C.recipe("mixed"), "custom": [fc("HADAMARD_ROTATION", bits=4)], "oscar": [fc("OSCAR", bits=4)]}
  # a GPTQ recipe on every projection keeps the Hessian of every input (the mixed one keeps none for down's)
  out["qsvs"] = quantizer.Quantizer(model, C.recipe("gptq")).calibrate({"serving_default": samples})
  for key, rcp in recipes.items():
    qz = quantizer.Quantizer(model, rcp)
    calib = qz.calibrate({"serving_default": samples}) if key != "custom" else {}
    res = qz.quantize(calib)
    out[key] = dict(qz=qz, model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)))
  for key in ("mixed", "custom"):
    out[key]["hessians"] = out["qsvs"]
    out[key]["cmp"] = out[key]["qz"].validate_layer_outputs(calibration_result=out["qsvs"], follow_input_transforms=True)
  # OSCAR's calibration keeps second moments, no Hessians: they are formed from the samples
  out["oscar"]["cmp"] = out["oscar"]["qz"].validate_layer_outputs(calibration_data={"serving_default": samples},
                                                                  follow_input_transforms=True)
  out["oscar"]["hessians"] = mv.layer_hessians(model, samples, "serving_default")
  return out


def _unpack_int4(packed, n):
  b = np.asarray(packed, dtype=np.uint8)
  out = np.empty(b.size * 2, np.int8)
  out[0::2], out[1::2] = (b & 0xF).astype(np.int8), (b >> 4).astype(np.int8)
  return np.where(out > 7, out - 16, out).astype(np.int8)[:n]


def _graph_transform(qm, y_name, d):
  """What the written graph does to the op's input, read here independently of the library:
  (kind, float64 [d] multiplier or float64 [h, h] matrix or None, h)."""
  from mi355q.transformations import graph_edits
  from mi355q.utils import flexbuffer, tfl_flatbuffer_utils
  sg = qm.subgraphs[0]
  producer = {int(o): op for op in sg.operators for o in op.outputs}
  code = lambda op: int(qm.operatorCodes[op.opcodeIndex].builtinCode)      # noqa: E731
  op = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == y_name)
  before = producer.get(int(op.inputs[0]))
  if before is None:
    return "none", None, 0
  if code(before) == 18:      # MUL
    const = tfl_flatbuffer_utils.get_tensor_data(sg.tensors[before.inputs[1]], qm.buffers)
    return "multiply", np.asarray(const, np.float64).reshape(d), 0
  if code(before) == 32:      # CUSTOM: its matrix is H_h / sqrt(h) itself
    h = int(flexbuffer.decode(bytes(bytearray(before.customOptions)))["hadamard_size"])
    return "hadamard", graph_edits._sylvester_hadamard(h), h      # pylint: disable=protected-access
  assert code(before) == 22      # RESHAPE <- FULLY_CONNECTED(., matrix) <- RESHAPE
  rotation = producer[int(before.inputs[0])]
  matrix = np.asarray(tfl_flatbuffer_utils.get_tensor_data(sg.tensors[rotation.inputs[1]], qm.buffers), np.float64)
  return "hadamard", matrix, int(matrix.shape[0])


def _float64_evaluation(chain, key, name, src):
  """(kind, h, error, gate) from the written integers and scales, the graph's own constant, the Hessian read back.
  The gate is gate_rows(dW) plus the first-order effect of the float32 rounding d of dW itself,
  2 alpha Sum_ij d_ri |P_ij| |dW_rj|: d <= u (|W_eff| + |dW|) for the multiply (one product, one subtraction),
  d <= (log2 h + 4) u ||dq_block||_1 / sqrt(h) + u |dW| for the rotation (log2 h butterfly stages, the scale r, the
  float32 matrix entries, the subtraction)."""
  w = chain["weights"][f"l0/{name}/w"].astype(np.float64)
  rows, d = w.shape
  qm = chain[key]["model"]
  t = next(t for t in qm.subgraphs[0].tensors if t.name.decode() == f"l0/{name}/w")
  q = _unpack_int4(np.asarray(qm.buffers[t.buffer].data), rows * d)
  scale = np.asarray(t.quantization.scale, np.float32)
  dq = LC.dequantize(q, scale, None, rows, d, 32).reshape(rows, d).astype(np.float64)
  kind, const, h = _graph_transform(qm, f"l0/{name}/y", d)
  hess = np.asarray(chain[key]["hessians"][f"l0/{src}"]["hessian"])
  assert hess.dtype == np.float64 and hess.shape == (d, d)
  if kind == "multiply":
    w_eff = dq * const.reshape(1, d)
    delta = w - w_eff
    rounding = LC.U * (np.abs(w_eff) + np.abs(delta))
  elif kind == "hadamard":
    w_eff = (dq.reshape(-1, h) @ const).reshape(rows, d)
    delta = w - w_eff
    block = np.abs(dq).reshape(-1, h).sum(axis=1, keepdims=True) / np.sqrt(h)
    rounding = (np.log2(h) + 4) * LC.U * np.broadcast_to(block, (rows * d // h, h)).reshape(rows, d) + LC.U * np.abs(delta)
  else:
    delta = w - dq
    rounding = np.zeros_like(delta)
  alpha = 0.5
  gate = LC.gate_rows(delta, hess, alpha).sum() + 2.0 * alpha * float(np.einsum("ri,ij,rj->", rounding, np.abs(hess), np.abs(delta)))
  return kind, h, LC.exact_rows(delta, hess, alpha).sum(), gate


def _expected_transforms(key):
  if key == "mixed":
    return {name: ("hadamard", DFF) if name == "down" else ("none", 0) for name in ("q", "k", "v", "o", "gate", "up", "down")}
  if key == "custom":
    return {name: ("hadamard", DFF if name == "down" else D) for name in ("q", "k", "v", "o", "gate", "up", "down")}
  return {name: ("multiply", 0) for name in ("q", "k", "v", "o", "gate", "up", "down")}


@pytest.mark.parametrize("key", ["mixed", "custom", "oscar"])
def test_every_projection_is_reported_inside_the_derived_gate(chain, key):
  cmp_ = chain[key]["cmp"]
  assert cmp_.skipped == {} and len(cmp_) == 7
  expected = _expected_transforms(key)
  for name, rows, d, src in chain["projections"]:
    r = cmp_[f"l0/{name}/y"]
    kind, h, error, gate = _float64_evaluation(chain, key, name, src)
    print(f"{key} l0/{name}: {r['input_transform']} h={r['hadamard_size']} error {r['error']:.6e} signal {r['signal']:.6e}"
          f" SNR {r['output_snr']:.1f}; |error - exact| / gate {abs(r['error'] - error) / gate:.3e}")
    assert (r["input_transform"], r["hadamard_size"]) == expected[name] == (kind, h)
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
    assert r["per_channel_error"].dtype == np.float64 and r["per_channel_error"].shape == (rows,)
    assert r["error"] == float(np.sum(r["per_channel_error"]))
    assert abs(r["error"] - error) <= gate
    assert 0 < r["error"] < r["signal"]      # int4 of a weight in the right basis; the wrong one loses the signal


def test_untransformed_projections_report_the_same_bits_with_the_flag_on_and_off(chain):
  from mi355q import model_validator as mv
  on = chain["mixed"]["cmp"]
  off = chain["mixed"]["qz"].validate_layer_outputs(calibration_result=chain["qsvs"])
  assert off.skipped == {"l0/down/y": mv.SKIP_INPUT} and len(off) == 6
  for y, r in off.results.items():
    assert "input_transform" not in r and "hadamard_size" not in r
    assert r["error"] == on[y]["error"] and r["signal"] == on[y]["signal"]
    assert np.array_equal(r["per_channel_error"].view(np.uint64), on[y]["per_channel_error"].view(np.uint64))
