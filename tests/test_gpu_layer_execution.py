"""Integer execution of quantized FULLY_CONNECTED ops on the GPU (csrc/qfc.hip, ops.qfc_quantize_rows / ops.qfc_forward /
ops.sqdiff_cols, model_validator.compare_layer_execution, Quantizer.validate_layer_execution).

  1. the dynamic row quantizer bit for bit (q and scale) on both routes, with planted rows;
  2. the integer product: acc_out and y_out bit for bit against tests/layer_execution_cases.py on the MFMA route (full
     tiles, partial tiles, several workgroups, every kind, scale granularity, zero point) and on the generic route,
     and every refusal. Integer MFMA is exact, so a wrong lane map or a row <-> column swap cannot pass;
  3. the per-column squared differences against NumPy float64, exact on integers, deterministic, accumulating;
  4. end to end on a one-layer decoder-shaped model for dynamic int8, dynamic int4 blockwise-32, static a8w8 and
     weight-only int8, against the NumPy chain with Y in float64 and the first-order bound of the FP32 GEMM.
"""
import json
import os
import sys

import numpy as np
import pytest

import layer_error_cases as LC
import layer_execution_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
KIND_CODE = {"i8": 3, "i4": 6, "i2": 7}


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available()
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi, ops
  from mi355q import runtime as rt

  class M:
    pass
  M.torch, M.ops, M.rt, M.ffi, M.lib = torch, ops, rt, _ffi, _ffi.lib()
  M.dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())

  def misaligned(a, offset=1):
    """A dense device copy of `a` whose base address is `offset` elements past an aligned allocation."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 != 0
    return view
  M.misaligned = staticmethod(misaligned)
  return M


# ---------------------------------------------------------------- 1. the row quantizer
ROW_D = (1, 7, 64, 100, 1024, 4096, 16384)
HALVES = (127.0, -127.0, 0.5, -0.5, 1.5, -1.5, 126.5, -126.5, 2.5, -2.5, 0.49999997, -0.49999997, -0.0, 0.0, 63.5, -64.5)


def _planted(kind: int, d: int, rng) -> np.ndarray:
  row = (rng.standard_normal(d) * np.exp(rng.normal())).astype(np.float32)
  if kind == 0:          # all zero
    row[:] = 0.0
  elif kind == 1:        # the maximum in the last element
    row = np.clip(row, -1.0, 1.0)
    row[-1] = -3.5
  elif kind == 2:        # range 127 exactly, so inv = 1: the halves, 0.49999997f and -0.0 are seen as they are
    row = np.resize(np.asarray(HALVES, np.float32), d)
  elif kind == 3:        # all -0.0: range 0
    row[:] = -0.0
  elif kind == 4:        # a NaN
    row[d // 2] = np.nan
  elif kind == 5:        # an infinity
    row[0] = -np.inf
  elif kind == 6:        # 0.49999997f next to the range, anywhere in the row
    row = np.clip(row, -100.0, 100.0)
    row[d // 3] = 127.0
    row[(d // 3 + 1) % d] = np.float32(0.49999997)
  return row.astype(np.float32)


def _row_case(n: int, d: int):
  rng = np.random.default_rng(1000 * n + d)
  shift = ROW_D.index(d)
  return np.stack([_planted((t + shift) % 9, d, rng) for t in range(n)])


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("d", ROW_D)
def test_row_quantizer_bit_for_bit(m, d, aligned):
  for n in (1, 3, 65):
    x = _row_case(n, d)
    want_q, want_s = EC.quantize_rows(x)
    q, s = m.ops.qfc_quantize_rows(m.dev(x) if aligned else m.misaligned(x))
    q, s = q.cpu().numpy(), s.cpu().numpy()
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert EC.same_bits(s, want_s), (n, d, s, want_s)
    assert np.array_equal(q, want_q), (n, d, np.argwhere(q != want_q)[:4])
  # the planted rows are what they claim (n = 65 holds every kind at every d)
  x = _row_case(65, d)
  q, s = EC.quantize_rows(x)
  kinds = [(t + ROW_D.index(d)) % 9 for t in range(65)]
  zero, nan, inf, half = kinds.index(0), kinds.index(4), kinds.index(5), kinds.index(2)
  assert s[zero] == 1.0 and not q[zero].any() and np.isnan(s[nan]) and np.isnan(s[inf]) and not q[nan].any()
  assert s[kinds.index(3)] == 1.0 and s[half] == 1.0
  assert q[half][:min(d, 16)].tolist() == [127, -127, 1, -1, 2, -2, 127, -127, 3, -3, 0, 0, 0, 0, 64, -65][:min(d, 16)]
  assert np.isfinite(s[[t for t in range(65) if kinds[t] not in (4, 5)]]).all()


def test_row_quantizer_empty_shapes_enqueue_nothing(m):
  assert m.lib.mi355q_qfc_quantize_rows_f32(None, 0, 64, None, None, None) == 0
  assert m.lib.mi355q_qfc_quantize_rows_f32(None, 5, 0, None, None, None) == 0
  assert m.lib.mi355q_qfc_quantize_rows_f32(None, 5, 64, None, None, None) == -1
  assert m.lib.mi355q_qfc_quantize_rows_f32(None, -1, 64, None, None, None) == -1


# ---------------------------------------------------------------- 2. the integer product
def _stored(qw: np.ndarray, kind: str) -> np.ndarray:
  if kind == "i8":
    return qw.astype(np.int8).ravel()
  per = 8 // EC.BITS[kind]
  flat = qw.ravel()
  pad = (-flat.size) % per
  return LC.pack(np.concatenate([flat, np.zeros(pad, flat.dtype)]), EC.BITS[kind])


def _forward(m, xq_dev, xs_dev, zp, w_dev, kind, rows, ws_dev, block, want_acc):
  n, d = xq_dev.shape
  y = m.torch.full((n, rows), float("nan"), dtype=m.torch.float32, device="cuda")
  acc = m.torch.full((n, rows), -7, dtype=m.torch.int32, device="cuda") if want_acc else None
  nbytes = m.lib.mi355q_qfc_forward_workspace_bytes(rows, d, block)
  ws = m.torch.empty(max(nbytes, 1), dtype=m.torch.uint8, device="cuda")
  m.ffi.check(m.lib.mi355q_qfc_forward_i8(m.rt.ptr(xq_dev), n, d, m.rt.ptr(xs_dev), xs_dev.numel(), zp, m.rt.ptr(w_dev),
                                          KIND_CODE[kind], rows, m.rt.ptr(ws_dev), ws_dev.numel(), block, m.rt.ptr(y),
                                          m.rt.ptr(acc), m.rt.ptr(ws), nbytes, m.rt.stream_ptr()))
  return y.cpu().numpy(), None if acc is None else acc.cpu().numpy()


def _case(m, n, rows, d, kind, w_mode, zp, x_per_row, seed, misalign_x=False, nan_row=False, extreme=False):
  """One call against the helper: `w_mode` "tensor", "channel" or a block size."""
  rng = np.random.default_rng(seed)
  bits = EC.BITS[kind]
  lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
  xq = rng.integers(-128, 127, size=(n, d), endpoint=True).astype(np.int8)
  qw = rng.integers(lo, hi, size=(rows, d), endpoint=True)
  if extreme:
    xq[:], qw[:] = -128, lo
  else:
    xq.ravel()[rng.integers(0, xq.size)] = -128
    qw.ravel()[rng.integers(0, qw.size)] = lo
  xs = (np.exp(rng.normal(size=n if x_per_row else 1)) * 0.013).astype(np.float32)      # no powers of two
  if nan_row:
    xs[min(1, xs.size - 1)] = np.nan
  block = w_mode if isinstance(w_mode, int) else 0
  count = 1 if w_mode == "tensor" else rows if w_mode == "channel" else rows * d // block
  wsc = (np.exp(rng.normal(size=count)) * 0.0071).astype(np.float32)
  want_acc, want_y = EC.forward(xq, xs, zp, qw, wsc, block)
  xq_dev = m.misaligned(xq) if misalign_x else m.dev(xq)
  got_y, got_acc = _forward(m, xq_dev, m.dev(xs), zp, m.dev(_stored(qw, kind)), kind, rows, m.dev(wsc), block, block == 0)
  tag = (n, rows, d, kind, w_mode, zp, x_per_row)
  if block == 0:
    assert np.array_equal(got_acc.astype(np.int64), want_acc), (tag, np.argwhere(got_acc != want_acc)[:4])
  assert EC.same_bits(got_y, want_y), (tag, np.argwhere(got_y.view(np.uint32) != want_y.view(np.uint32))[:4])
  return want_acc


ZPS = (0, -128, 5, 127)
MFMA_N, MFMA_ROWS = (1, 15, 16, 17, 33, 130), (1, 15, 16, 17, 130)


@pytest.mark.parametrize("d", [64, 128, 192, 1024])
@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_mfma_route_bit_for_bit(m, kind, d):
  """Every n x rows of the list; zero point, x_scale_count and the weight scale's count take turns, and every
  combination of the three is met for every kind and d (30 shapes, 16 combinations)."""
  i = 0
  for n in MFMA_N:
    for rows in MFMA_ROWS:
      _case(m, n, rows, d, kind, ("tensor", "channel")[(i // 8) % 2], ZPS[i % 4], bool((i // 4) % 2), 100 * d + i)
      i += 1


@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_every_zero_point_and_scale_count(m, kind):
  for zp in ZPS:
    for x_per_row in (False, True):
      for w_mode in ("tensor", "channel", 32, 64):
        _case(m, 33, 17, 128, kind, w_mode, zp, x_per_row, 7)


@pytest.mark.parametrize("d", [64, 128, 256, 512])
@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_blockwise_bit_for_bit(m, kind, d):
  i = 0
  for block in (32, 64, 128, 256):
    if d % block:
      continue
    for n, rows in ((1, 1), (17, 15), (130, 33), (16, 130)):
      _case(m, n, rows, d, kind, block, ZPS[i % 4], bool(i % 2), 31 * d + i)
      i += 1


def test_forward_long_rows(m):
  _case(m, 33, 17, 4096, "i8", "channel", 5, True, 1)
  _case(m, 17, 33, 4096, "i4", 128, -128, True, 2)
  # d = 65536 with every product at its extreme: (-128 - 127) * -128 = 32640, 65536 of them, just below 2^31
  acc = _case(m, 1, 1, 65536, "i8", "tensor", 127, False, 3, extreme=True)
  assert acc[0, 0] == 65536 * 255 * 128 and acc[0, 0] < 2 ** 31
  acc = _case(m, 1, 1, 65536, "i8", "tensor", 0, False, 4, extreme=True)
  assert acc[0, 0] == 65536 * 128 * 128


@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_generic_route_bit_for_bit(m, kind):
  """d that is no multiple of the MFMA step (with packed weights whose rows begin inside a byte when d is odd) and
  a misaligned xq at an MFMA shape."""
  i = 0
  for d in (1, 7, 33, 100):
    for n, rows in ((1, 1), (5, 6), (17, 3)):
      _case(m, n, rows, d, kind, ("tensor", "channel")[i % 2], ZPS[i % 4], bool((i // 2) % 2), 9000 + 10 * d + i)
      i += 1
  for w_mode in ("channel", 32, 64):
    _case(m, 17, 15, 128, kind, w_mode, 5, True, 9500, misalign_x=True)
  _case(m, 5, 6, 96, kind, 32, -128, True, 9600)      # block 32 with d % 64 != 0: the K = 32 instruction's own route


def test_forward_nan_x_scale_row_gives_nan_outputs(m):
  for d, kind, w_mode in ((128, "i8", "channel"), (128, "i4", 32), (33, "i8", "channel")):
    _case(m, 5, 17, d, kind, w_mode, 0, True, 12, nan_row=True)


def test_forward_refusals(m):
  EC.check_forward_refusals(m.lib)


def test_ops_qfc_forward_reads_the_compare_target(m):
  rng = np.random.default_rng(5)
  n, rows, d = 17, 33, 128
  xq = rng.integers(-128, 127, size=(n, d), endpoint=True).astype(np.int8)
  xs = (np.exp(rng.normal(size=n)) * 0.01).astype(np.float32)
  for kind, channels, inner, block in (("i8", 1, 1, 0), ("i8", rows, d, 0), ("i4", rows * d // 32, 32, 32), ("i2", rows * d // 64, 64, 64)):
    bits = EC.BITS[kind]
    qw = rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, size=(rows, d), endpoint=True)
    wsc = (np.exp(rng.normal(size=channels)) * 0.01).astype(np.float32)
    target = m.ops.CompareTarget(m.dev(_stored(qw, kind)), rows * d, kind, m.dev(wsc), None, channels, inner, 32)
    want_acc, want_y = EC.forward(xq, xs, 3, qw, wsc, block)
    if block == 0:
      y, acc = m.ops.qfc_forward(m.dev(xq), m.dev(xs), 3, target, rows, d, want_acc=True)
      assert np.array_equal(acc.cpu().numpy(), want_acc)
    else:
      y = m.ops.qfc_forward(m.dev(xq), m.dev(xs), 3, target, rows, d)
    assert EC.same_bits(y.cpu().numpy(), want_y)
  with pytest.raises(ValueError, match="neither per tensor, per channel nor blockwise"):
    m.ops.qfc_forward(m.dev(xq), m.dev(xs), 0, m.ops.CompareTarget(m.dev(_stored(qw, "i8")), rows * d, "i8", m.dev(wsc[:3]),
                                                                   None, 3, 5, 32), rows, d)


# ---------------------------------------------------------------- 3. per-column squared differences
@pytest.mark.parametrize("cols", [1, 17, 64, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_sqdiff_cols(m, n, cols):
  rng = np.random.default_rng(n * 1000 + cols)
  a = rng.standard_normal((n, cols)).astype(np.float32)
  b = (a + 0.01 * rng.standard_normal((n, cols))).astype(np.float32)
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  want_d, want_b = ((a64 - b64) ** 2).sum(axis=0), (b64 ** 2).sum(axis=0)
  got = [v.cpu().numpy() for v in m.ops.sqdiff_cols(m.dev(a), m.dev(b))]
  again = [v.cpu().numpy() for v in m.ops.sqdiff_cols(m.dev(a), m.dev(b))]
  assert got[0].dtype == np.float64 and got[0].shape == (cols,)
  # NumPy's own summation of n non-negative terms is within n 2^-53 of exact, as the kernel's is
  tol = n * 2.0 ** -52
  assert np.all(np.abs(got[0] - want_d) <= tol * want_d) and np.all(np.abs(got[1] - want_b) <= tol * want_b)
  assert np.array_equal(got[0].view(np.uint64), again[0].view(np.uint64))
  assert np.array_equal(got[1].view(np.uint64), again[1].view(np.uint64))
  # small integers: every order of addition is exact
  ai = rng.integers(-9, 9, size=(n, cols), endpoint=True).astype(np.float32)
  bi = rng.integers(-9, 9, size=(n, cols), endpoint=True).astype(np.float32)
  got = [v.cpu().numpy() for v in m.ops.sqdiff_cols(m.dev(ai), m.dev(bi))]
  assert np.array_equal(got[0], ((ai.astype(np.int64) - bi.astype(np.int64)) ** 2).sum(axis=0).astype(np.float64))
  assert np.array_equal(got[1], (bi.astype(np.int64) ** 2).sum(axis=0).astype(np.float64))
  # accumulate over two calls = one call over the stacked rows
  ci = rng.integers(-9, 9, size=(n + 3, cols), endpoint=True).astype(np.float32)
  di = rng.integers(-9, 9, size=(n + 3, cols), endpoint=True).astype(np.float32)
  sums = m.ops.sqdiff_cols(m.dev(ai), m.dev(bi))
  out = m.ops.sqdiff_cols(m.dev(ci), m.dev(di), out=sums)
  assert out[0] is sums[0] and out[1] is sums[1]
  whole = m.ops.sqdiff_cols(m.dev(np.concatenate([ai, ci])), m.dev(np.concatenate([bi, di])))
  assert np.array_equal(out[0].cpu().numpy(), whole[0].cpu().numpy())
  assert np.array_equal(out[1].cpu().numpy(), whole[1].cpu().numpy())


# ---------------------------------------------------------------- 4. end to end
D, DKV, DFF = 128, 32, 256


def _fc_entry(C, bits, granularity):
  from mi355q import algorithm_manager
  entry = C._fc(algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT.value, bits=bits)      # pylint: disable=protected-access
  entry["op_config"]["weight_tensor_config"]["granularity"] = granularity
  return entry


@pytest.fixture(scope="module")
def chain(m, tmp_path_factory):
  import c5_model as C
  from mi355q import quantizer, recipe
  from mi355q.utils import tfl_flatbuffer_utils
  projections = C.projections(D, DKV, DFF)
  model = C.build_model(1, d=D, dkv=DKV, dff=DFF)
  weights = {}
  for t in model.subgraphs[0].tensors:
    name = t.name.decode()
    if name.endswith("/w"):
      weights[name] = np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()
  samples = LC.calibration_samples(projections)
  out = dict(C=C, projections=projections, weights=weights, samples=samples, model=model)
  recipes = {"dynamic_i8": recipe.dynamic_wi8_afp32(), "dynamic_i4_b32": [_fc_entry(C, 4, "BLOCKWISE_32")],
             "static_a8w8": recipe.static_wi8_ai8(), "weight_only_i8": recipe.weight_only_wi8_afp32(),
             "mixed": C.recipe("mixed")}
  for key, rcp in recipes.items():
    qz = quantizer.Quantizer(model, rcp)
    calib = qz.calibrate({"serving_default": samples}) if qz.need_calibration else {}
    res = qz.quantize(calib)
    out[key] = dict(qz=qz, model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)))
    if key != "mixed":
      out[key]["cmp"] = qz.validate_layer_execution({"serving_default": samples})
  out["save_dir"] = str(tmp_path_factory.mktemp("layer_execution"))
  return out


MODES = {"dynamic_i8": "dynamic", "dynamic_i4_b32": "dynamic", "static_a8w8": "static", "weight_only_i8": "weight_only",
         "mixed": "dynamic"}


def _written_weight(qm, name, rows, d):
  """(integers [rows, d], float32 scales, block or 0) of the written constant, read here independently of the library."""
  from mi355q import schema
  from mi355q.utils import tfl_flatbuffer_utils
  sg = qm.subgraphs[0]
  t = next(t for t in sg.tensors if t.name.decode() == name)
  kind = {int(schema.TensorType.INT8): "i8", int(schema.TensorType.INT4): "i4", int(schema.TensorType.INT2): "i2"}[int(t.type)]
  q = EC.unpack(np.asarray(qm.buffers[t.buffer].data), kind, rows * d).reshape(rows, d)
  details = getattr(t.quantization, "details", None)
  if details is not None and hasattr(details, "blockSize"):
    scales = np.asarray(tfl_flatbuffer_utils.get_tensor_data(sg.tensors[int(details.scales)], qm.buffers))
    assert scales.dtype == np.float16
    return q, scales.astype(np.float32).ravel(), int(details.blockSize)
  assert t.quantization.zeroPoint is None or not np.any(np.asarray(t.quantization.zeroPoint))
  return q, np.asarray(t.quantization.scale, np.float32), 0


def _numpy_chain(chain, key, name, src, rotate_h=0):
  """(error, bound, per-channel error, per-channel bound, signal) from the written model and the samples, Y in float64.
  The only inexact device step is the FP32 GEMM, whose elements lie within eps[t, r] = (d + 2) 2^-24 Sum_k |x| |w| of
  exact to first order, so |error - error_ref| <= (1/n) Sum (2 |yq - y64| eps + eps^2)."""
  from oracle import aeq_oracle as O
  w = chain["weights"][f"l0/{name}/w"]
  rows, d = w.shape
  x = np.concatenate([s[f"l0/{src}"].reshape(-1, d) for s in chain["samples"]], axis=0).astype(np.float32)
  n = x.shape[0]
  qm = chain[key]["model"]
  qw, scales, block = _written_weight(qm, f"l0/{name}/w", rows, d)
  xt = x
  if rotate_h:
    xt, h = O.hadamard_rotate(x, max_size=rotate_h)
    assert h == rotate_h and xt.dtype == np.float32
  mode = MODES[key]
  if mode == "dynamic":
    xq, xs = EC.quantize_rows(xt)
    yq = EC.forward(xq, xs, 0, qw, scales, block)[1].astype(np.float64)
  elif mode == "static":
    sg = qm.subgraphs[0]
    fc = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"l0/{name}/y")
    t = sg.tensors[fc.inputs[0]]      # the int8 activation the op reads, with the calibrated (s_x, zp_x)
    assert int(t.type) == 9 and len(t.quantization.scale) == 1
    s_x, zp_x = np.float32(t.quantization.scale[0]), int(t.quantization.zeroPoint[0])
    yq = EC.forward(EC.quantize_static(xt, s_x, zp_x), np.array([s_x], np.float32), zp_x, qw, scales, block)[1].astype(np.float64)
  else:
    dq = LC.dequantize(qw.ravel(), scales, None, rows if scales.size > 1 else 1, d if scales.size > 1 else 1, 32)
    yq = xt.astype(np.float64) @ dq.reshape(rows, d).astype(np.float64).T
  y64 = x.astype(np.float64) @ w.astype(np.float64).T
  eps = (d + 2) * LC.U * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T)
  diff = yq - y64
  per_channel = (diff ** 2).sum(axis=0) / n
  per_channel_bound = (2.0 * np.abs(diff) * eps + eps ** 2).sum(axis=0) / n
  return per_channel.sum(), per_channel_bound.sum(), per_channel, per_channel_bound, (y64 ** 2).sum() / n


@pytest.mark.parametrize("key", ["dynamic_i8", "dynamic_i4_b32", "static_a8w8", "weight_only_i8"])
def test_every_projection_matches_the_numpy_chain(chain, key):
  """In weight-only mode Yq is a second FP32 GEMM; its rounding is of the size of Y's and lies inside the same
  first-order worst-case bound in practice, so the bound is asserted as it stands."""
  cmp_ = chain[key]["cmp"]
  assert cmp_.skipped == {} and len(cmp_) == 7
  for name, rows, d, src in chain["projections"]:
    r = cmp_[f"l0/{name}/y"]
    error, bound, per_channel, per_channel_bound, signal = _numpy_chain(chain, key, name, src)
    worst = float(np.max(np.abs(r["per_channel_error"] - per_channel) / per_channel_bound))
    print(f"{key} l0/{name}: error {r['error']:.6e} signal {r['signal']:.6e} SNR {r['output_snr']:.1f};"
          f" |error - ref| / bound {abs(r['error'] - error) / bound:.3e}, per channel worst {worst:.3e}")
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
    assert r["tokens"] == 1024 and r["mode"] == MODES[key]
    assert abs(r["error"] - error) <= bound
    assert np.all(np.abs(r["per_channel_error"] - per_channel) <= per_channel_bound)
    assert r["per_channel_error"].dtype == np.float64 and r["per_channel_error"].shape == (rows,)
    np.testing.assert_allclose(r["signal"], signal, rtol=1e-5)
    np.testing.assert_allclose(r["error"], float(np.sum(r["per_channel_error"])), rtol=1e-12)
    assert r["output_mse"] == r["error"] / rows
    assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)
    assert 0 < r["error"] < r["signal"]


def test_rotated_projection_is_followed_through_its_rotation(chain):
  from mi355q import model_validator as mv
  qz = chain["mixed"]["qz"]
  off = qz.validate_layer_execution(chain["samples"])
  assert off.skipped == {"l0/down/y": mv.SKIP_INPUT} and len(off) == 6
  on = qz.validate_layer_execution(chain["samples"], follow_input_transforms=True)
  assert on.skipped == {} and len(on) == 7
  for name, rows, d, src in chain["projections"]:
    r = on[f"l0/{name}/y"]
    want = ("hadamard", DFF) if name == "down" else ("none", 0)
    assert (r["input_transform"], r["hadamard_size"]) == want and r["mode"] == "dynamic"
    error, bound, per_channel, per_channel_bound, _ = _numpy_chain(chain, "mixed", name, src, DFF if name == "down" else 0)
    print(f"mixed l0/{name}: {r['input_transform']} error {r['error']:.6e} signal {r['signal']:.6e};"
          f" |error - ref| / bound {abs(r['error'] - error) / bound:.3e}")
    assert abs(r["error"] - error) <= bound
    assert np.all(np.abs(r["per_channel_error"] - per_channel) <= per_channel_bound)
    assert 0 < r["error"] < r["signal"]
    if name != "down":
      assert "input_transform" not in off[f"l0/{name}/y"] and off[f"l0/{name}/y"]["error"] == r["error"]


def test_device_resident_samples_give_identical_results(chain, m):
  qz = chain["dynamic_i8"]["qz"]
  resident = [{k: m.dev(v) for k, v in s.items()} for s in chain["samples"]]
  got = qz.validate_layer_execution(resident, signature_key="serving_default")
  want = chain["dynamic_i8"]["cmp"]
  assert got.skipped == {} and list(got) == list(want)
  for y, r in want.results.items():
    assert got[y]["error"] == r["error"] and got[y]["signal"] == r["signal"] and got[y]["tokens"] == r["tokens"]
    assert np.array_equal(got[y]["per_channel_error"].view(np.uint64), r["per_channel_error"].view(np.uint64))


def test_save_writes_every_key(chain):
  qz = chain["static_a8w8"]["qz"]
  cmp_ = qz.validate_layer_execution({"serving_default": chain["samples"]}, save_folder=chain["save_dir"], model_name="one_layer")
  with open(os.path.join(chain["save_dir"], "one_layer_layer_execution_errors.json")) as fh:
    saved = json.load(fh)
  assert saved["skipped"] == {} and len(saved["layers"]) == 7
  for y, entry in saved["layers"].items():
    assert sorted(entry) == ["d", "error", "input", "mode", "output_mse", "output_snr", "rows", "signal", "tokens", "weight"]
    for k, v in entry.items():
      assert v == cmp_[y][k]


def test_weight_only_on_exact_data_equals_the_hessian_route(m):
  """Integer X and power-of-two weight scales: every product and sum of both GEMMs is exact in float32, and so is the
  quadratic form of validate_layer_outputs. The two routes measure the same quantity."""
  import c5_model as C
  from mi355q import quantizer, recipe
  d, dkv, dff = 32, 16, 64

  def weights(layer, name, rows, cols):
    rng = np.random.default_rng(rows * 7 + cols + len(name))
    k = rng.integers(-120, 120, size=(rows, cols), endpoint=True).astype(np.float64) + 0.25
    k[np.arange(rows), rng.integers(0, cols, size=rows)] = 127.0      # max |w| = 127 * 2^-7: the scale is 2^-7
    return (k * 2.0 ** -7).astype(np.float32)
  model = C.build_model(1, d=d, dkv=dkv, dff=dff, weights=weights)
  rng = np.random.default_rng(77)
  widths = {src: cols for _, _, cols, src in C.projections(d, dkv, dff)}
  # (2-D samples: their leading dimension, which the Hessians count, is the token count)
  samples = [{f"l0/{src}": rng.integers(-3, 3, size=(48, cols), endpoint=True).astype(np.float32)
              for src, cols in widths.items()} for _ in range(3)]
  qz = quantizer.Quantizer(model, recipe.weight_only_wi8_afp32())
  res = qz.quantize({})
  assert res.quantized_model is not None
  execution = qz.validate_layer_execution(samples, signature_key="serving_default")
  hessian = qz.validate_layer_outputs(calibration_data=samples, signature_key="serving_default")
  assert execution.skipped == {} and hessian.skipped == {} and len(execution) == len(hessian) == 7
  for y, r in execution.results.items():
    assert r["mode"] == "weight_only" and r["tokens"] == 144 and r["error"] > 0
    np.testing.assert_allclose(r["error"], hessian[y]["error"], rtol=1e-12)
    np.testing.assert_allclose(r["signal"], hessian[y]["signal"], rtol=1e-12)
    np.testing.assert_allclose(r["per_channel_error"], hessian[y]["per_channel_error"], rtol=1e-12)
