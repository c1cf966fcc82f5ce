"""Integer execution of INT16-activation FULLY_CONNECTED ops on the GPU (csrc/qfc16.hip, ops.qfc_forward_i16,
model_validator.compare_layer_execution / Quantizer.validate_layer_execution with `int16_activations`).

  1. the integer product: acc_out (int64) and y_out bit for bit against tests/layer_execution_i16_cases.py on the
     MFMA route (full tiles, partial tiles, several workgroups, every kind and scale granularity, blockwise), with
     the int16 values where a byte split goes wrong planted in every row, at the extremes of d = 65536 where each
     int32 plane stands at +-2^30, and on the generic route; every refusal. Integer MFMA is exact, so a wrong lane
     map, a wrong byte selector or a row <-> column swap cannot pass;
  2. end to end on the one-layer decoder-shaped model of test_gpu_layer_execution.py under static_wi8_ai16, against
     the NumPy chain with Y in float64 and the first-order bound of the FP32 GEMM.
"""
import os
import sys

import numpy as np
import pytest

import layer_error_cases as LC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16

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


# ---------------------------------------------------------------- 1. the integer product
def _stored(qw: np.ndarray, kind: str) -> np.ndarray:
  if kind == "i8":
    return qw.astype(np.int8).ravel()
  per = 8 // EC.BITS[kind]
  flat = qw.ravel()
  pad = (-flat.size) % per
  return LC.pack(np.concatenate([flat, np.zeros(pad, flat.dtype)]), EC.BITS[kind])


def _forward(m, xq_dev, xs_dev, w_dev, kind, rows, ws_dev, block, want_acc):
  n, d = xq_dev.shape
  y = m.torch.full((n, rows), float("nan"), dtype=m.torch.float32, device="cuda")
  acc = m.torch.full((n, rows), -7, dtype=m.torch.int64, device="cuda") if want_acc else None
  nbytes = m.lib.mi355q_qfc_forward_i16_workspace_bytes(rows, d, block)
  ws = m.torch.empty(max(nbytes, 1), dtype=m.torch.uint8, device="cuda")
  m.ffi.check(m.lib.mi355q_qfc_forward_i16(m.rt.ptr(xq_dev), n, d, m.rt.ptr(xs_dev), xs_dev.numel(), m.rt.ptr(w_dev),
                                           KIND_CODE[kind], rows, m.rt.ptr(ws_dev), ws_dev.numel(), block, m.rt.ptr(y),
                                           m.rt.ptr(acc), m.rt.ptr(ws), nbytes, m.rt.stream_ptr()))
  return y.cpu().numpy(), None if acc is None else acc.cpu().numpy()


def _activations(n, d, rng) -> np.ndarray:
  """Random int16 over the full range, with the values where a byte split goes wrong planted in every row (at a
  place that moves with the row, so they meet every lane and both 16-byte halves of a fragment)."""
  xq = rng.integers(-32768, 32767, size=(n, d), endpoint=True).astype(np.int16)
  for t in range(n):
    for j, v in enumerate(EC16.PLANTED[:d]):
      xq[t, (3 * t + j) % d] = v
  return xq


def _case(m, n, rows, d, kind, w_mode, x_per_row, seed, misalign_x=False, nan_row=False, extreme=None):
  """One call against the helper: `w_mode` "tensor", "channel" or a block size."""
  rng = np.random.default_rng(seed)
  bits = EC.BITS[kind]
  lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
  xq = _activations(n, d, rng)
  qw = rng.integers(lo, hi, size=(rows, d), endpoint=True)
  if extreme is not None:
    xq[:], qw[:] = extreme
  else:
    qw.ravel()[rng.integers(0, qw.size)] = lo
  xs = (np.exp(rng.normal(size=n if x_per_row else 1)) * 3.1e-5).astype(np.float32)      # no powers of two
  if nan_row:
    xs[min(1, xs.size - 1)] = np.nan
  block = w_mode if isinstance(w_mode, int) else 0
  count = 1 if w_mode == "tensor" else rows if w_mode == "channel" else rows * d // block
  wsc = (np.exp(rng.normal(size=count)) * 0.0071).astype(np.float32)
  want_acc, want_y = EC16.forward16(xq, xs, qw, wsc, block)
  xq_dev = m.misaligned(xq) if misalign_x else m.dev(xq)
  got_y, got_acc = _forward(m, xq_dev, m.dev(xs), m.dev(_stored(qw, kind)), kind, rows, m.dev(wsc), block, block == 0)
  tag = (n, rows, d, kind, w_mode, x_per_row)
  if block == 0:
    assert got_acc.dtype == np.int64
    assert np.array_equal(got_acc, want_acc), (tag, np.argwhere(got_acc != want_acc)[:4])
  assert EC.same_bits(got_y, want_y), (tag, np.argwhere(got_y.view(np.uint32) != want_y.view(np.uint32))[:4])
  return want_acc


MFMA_N, MFMA_ROWS = (1, 15, 16, 17, 33, 130), (1, 15, 16, 17, 130)


@pytest.mark.parametrize("d", [64, 128, 192, 1024])
@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_mfma_route_bit_for_bit(m, kind, d):
  """Every n x rows of the list; x_scale_count and the weight scale's count take turns, and every combination of
  the two is met for every kind and d (30 shapes, 4 combinations)."""
  i = 0
  for n in MFMA_N:
    for rows in MFMA_ROWS:
      _case(m, n, rows, d, kind, ("tensor", "channel")[(i // 2) % 2], bool(i % 2), 100 * d + i)
      i += 1


@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_every_scale_count(m, kind):
  for x_per_row in (False, True):
    for w_mode in ("tensor", "channel", 32, 64, 128):
      _case(m, 33, 17, 128, kind, w_mode, x_per_row, 7)


@pytest.mark.parametrize("d", [64, 128, 256, 512])
@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_blockwise_bit_for_bit(m, kind, d):
  i = 0
  for block in (32, 64, 128, 256):
    if d % block:
      continue
    for n, rows in ((1, 1), (17, 15), (130, 33), (16, 130)):
      _case(m, n, rows, d, kind, block, bool(i % 2), 31 * d + i)
      i += 1


def test_forward_extremes_at_the_longest_row(m):
  """d = 65536, n = 17, rows = 16: every h = -128 (or 127) against w = -128 puts the high plane at +-2^30, every
  l_s against it the low plane near it, and the combined value is far beyond int32."""
  acc = _case(m, 17, 16, 65536, "i8", "channel", True, 3, extreme=(-32768, -128))
  assert (acc == 65536 * 32768 * 128).all() and acc[0, 0] == 2 ** 38
  h, l_s = EC16.split(np.int16(-32768))
  assert 65536 * int(h) * -128 == 2 ** 30 and 65536 * int(l_s) * -128 == 2 ** 30
  acc = _case(m, 17, 16, 65536, "i8", "tensor", False, 4, extreme=(32767, -128))
  assert (acc == -65536 * 32767 * 128).all() and acc[0, 0] < -2 ** 37
  h, l_s = EC16.split(np.int16(32767))
  assert 65536 * int(h) * -128 == -(2 ** 30 - 2 ** 23) and 65536 * int(l_s) * -128 == -(2 ** 30 - 2 ** 23)
  # and a long row of random values with packed weights, blockwise
  _case(m, 17, 33, 4096, "i4", 128, True, 2)


@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
def test_forward_generic_route_bit_for_bit(m, kind):
  """d that is no multiple of the MFMA step (with packed weights whose rows begin inside a byte when d is odd) and
  a 2-byte-misaligned xq at an MFMA shape."""
  i = 0
  for d in (1, 7, 33, 100):
    for n, rows in ((1, 1), (5, 6), (17, 3)):
      _case(m, n, rows, d, kind, ("tensor", "channel")[i % 2], bool((i // 2) % 2), 9000 + 10 * d + i)
      i += 1
  for w_mode in ("channel", 32, 64):
    _case(m, 17, 15, 128, kind, w_mode, True, 9500, misalign_x=True)
  _case(m, 5, 6, 96, kind, 32, True, 9600)      # block 32 with d % 64 != 0: the K = 32 instruction's own route


def test_forward_nan_x_scale_row_gives_nan_outputs_in_that_row_only(m):
  for d, kind, w_mode in ((128, "i8", "channel"), (128, "i4", 32), (33, "i8", "channel")):
    _case(m, 5, 17, d, kind, w_mode, True, 12, nan_row=True)
  rng = np.random.default_rng(13)
  xq, qw = _activations(5, 128, rng), rng.integers(-128, 127, size=(17, 128), endpoint=True)
  xs = np.array([1e-4, np.nan, 2e-4, 3e-4, 4e-4], np.float32)
  y, _ = _forward(m, m.dev(xq), m.dev(xs), m.dev(_stored(qw, "i8")), "i8", 17, m.dev(np.array([0.0071], np.float32)), 0, False)
  assert np.isnan(y[1]).all() and np.isfinite(y[[0, 2, 3, 4]]).all()


def test_forward_refusals(m):
  EC16.check_forward16_refusals(m.lib)


def test_ops_qfc_forward_i16_reads_the_compare_target(m):
  rng = np.random.default_rng(5)
  n, rows, d = 17, 33, 128
  xq = _activations(n, d, rng)
  xs = (np.exp(rng.normal(size=n)) * 1e-4).astype(np.float32)
  for kind, channels, inner, block in (("i8", 1, 1, 0), ("i8", rows, d, 0), ("i4", rows * d // 32, 32, 32), ("i2", rows * d // 64, 64, 64)):
    bits = EC.BITS[kind]
    qw = rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, size=(rows, d), endpoint=True)
    wsc = (np.exp(rng.normal(size=channels)) * 0.01).astype(np.float32)
    target = m.ops.CompareTarget(m.dev(_stored(qw, kind)), rows * d, kind, m.dev(wsc), None, channels, inner, 32)
    want_y, want_acc = _forward(m, m.dev(xq), m.dev(xs), target.data, kind, rows, target.scale, block, block == 0)
    ref_acc, ref_y = EC16.forward16(xq, xs, qw, wsc, block)
    if block == 0:
      y, acc = m.ops.qfc_forward_i16(m.dev(xq), m.dev(xs), target, rows, d, want_acc=True)
      assert acc.dtype == m.torch.int64 and np.array_equal(acc.cpu().numpy(), want_acc) and np.array_equal(want_acc, ref_acc)
    else:
      y = m.ops.qfc_forward_i16(m.dev(xq), m.dev(xs), target, rows, d)
    assert EC.same_bits(y.cpu().numpy(), want_y) and EC.same_bits(want_y, ref_y)
  with pytest.raises(ValueError, match="neither per tensor, per channel nor blockwise"):
    m.ops.qfc_forward_i16(m.dev(xq), m.dev(xs), m.ops.CompareTarget(m.dev(_stored(qw, "i8")), rows * d, "i8", m.dev(wsc[:3]),
                                                                    None, 3, 5, 32), rows, d)
  with pytest.raises(TypeError, match="expected an int16"):
    m.ops.qfc_forward_i16(m.dev(xq.astype(np.int8)), m.dev(xs), target, rows, d)
  zp = m.ops.CompareTarget(target.data, rows * d, kind, target.scale, m.dev(np.full(channels, 3, np.int32)), channels, inner, 32)
  with pytest.raises(ValueError, match="zero point must be 0"):
    m.ops.qfc_forward_i16(m.dev(xq), m.dev(xs), zp, rows, d)
  # the static int16 quantizer as it stands, against the helper's statement of it
  x = (rng.standard_normal((n, d)) * 3.0).astype(np.float32)
  x[0, :4] = (40.0, -40.0, 0.00005, -0.00015)      # beyond the range on both sides; halves of the step
  q, s = m.ops.quantize(m.dev(x), 1, 1, x.size, m.dev(np.array([1e-4], np.float32)), m.dev(np.array([0], np.int32)), 16, False), 1e-4
  assert q.dtype == m.torch.int16 and np.array_equal(q.cpu().numpy(), EC16.quantize_static16(x, s))
  assert q.cpu().numpy()[0, :2].tolist() == [32767, -32768]


# ---------------------------------------------------------------- 2. end to end
D, DKV, DFF = 128, 32, 256


@pytest.fixture(scope="module")
def chain(m):
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
  qz = quantizer.Quantizer(model, recipe.static_wi8_ai16())
  res = qz.quantize(qz.calibrate({"serving_default": samples}))
  return dict(projections=projections, weights=weights, samples=samples, qz=qz,
              model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)),
              cmp=qz.validate_layer_execution({"serving_default": samples}, int16_activations=True))


def _numpy_chain(chain, name, src):
  """(error, bound, per-channel error, per-channel bound, signal) from the written model and the samples, Y in float64:
  quantize_static16 with the written tensor's own scale -> forward16 on the written integers. The only inexact device
  step is the FP32 GEMM of Y, whose elements lie within eps[t, r] = (d + 2) 2^-24 Sum_k |x| |w| of exact to first
  order, so |error - error_ref| <= (1/n) Sum (2 |yq - y64| eps + eps^2) (derived, not measured)."""
  import test_gpu_layer_execution as G8
  w = chain["weights"][f"l0/{name}/w"]
  rows, d = w.shape
  x = np.concatenate([s[f"l0/{src}"].reshape(-1, d) for s in chain["samples"]], axis=0).astype(np.float32)
  n = x.shape[0]
  qm = chain["model"]
  qw, scales, block = G8._written_weight(qm, f"l0/{name}/w", rows, d)      # pylint: disable=protected-access
  sg = qm.subgraphs[0]
  fc = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"l0/{name}/y")
  t = sg.tensors[fc.inputs[0]]      # the int16 activation the op reads, with the calibrated s_x
  assert int(t.type) == 7 and len(t.quantization.scale) == 1      # TensorType.INT16
  assert t.quantization.zeroPoint is None or not np.any(np.asarray(t.quantization.zeroPoint))
  s_x = np.float32(t.quantization.scale[0])
  yq = EC16.forward16(EC16.quantize_static16(x, s_x), np.array([s_x], np.float32), qw, scales, block)[1].astype(np.float64)
  y64 = x.astype(np.float64) @ w.astype(np.float64).T
  eps = (d + 2) * LC.U * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T)
  diff = yq - y64
  per_channel = (diff ** 2).sum(axis=0) / n
  per_channel_bound = (2.0 * np.abs(diff) * eps + eps ** 2).sum(axis=0) / n
  return per_channel.sum(), per_channel_bound.sum(), per_channel, per_channel_bound, (y64 ** 2).sum() / n


def test_the_plain_call_lists_every_projection_under_skip_int16(chain):
  from mi355q import model_validator as mv
  plain = chain["qz"].validate_layer_execution({"serving_default": chain["samples"]})
  assert not plain.results
  assert plain.skipped == {f"l0/{name}/y": mv.SKIP_INT16 for name, *_ in chain["projections"]}


def test_every_a16_projection_matches_the_numpy_chain(chain):
  cmp_ = chain["cmp"]
  assert cmp_.skipped == {} and len(cmp_) == 7
  for name, rows, d, src in chain["projections"]:
    r = cmp_[f"l0/{name}/y"]
    error, bound, per_channel, per_channel_bound, signal = _numpy_chain(chain, name, src)
    worst = float(np.max(np.abs(r["per_channel_error"] - per_channel) / per_channel_bound))
    print(f"a16w8 l0/{name}: error {r['error']:.6e} signal {r['signal']:.6e} SNR {r['output_snr']:.1f};"
          f" |error - ref| / bound {abs(r['error'] - error) / bound:.3e}, per channel worst {worst:.3e}")
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
    assert r["tokens"] == 1024 and r["mode"] == "static" and r["activation_bits"] == 16
    assert abs(r["error"] - error) <= bound
    assert np.all(np.abs(r["per_channel_error"] - per_channel) <= per_channel_bound)
    assert r["per_channel_error"].dtype == np.float64 and r["per_channel_error"].shape == (rows,)
    np.testing.assert_allclose(r["signal"], signal, rtol=1e-5)
    np.testing.assert_allclose(r["error"], float(np.sum(r["per_channel_error"])), rtol=1e-12)
    assert r["output_mse"] == r["error"] / rows
    assert r["output_snr"] == (r["signal"] / rows) / (r["output_mse"] + 1e-9)
    assert 0 < r["error"] < r["signal"]


def test_device_resident_samples_give_identical_results(chain, m):
  resident = [{k: m.dev(v) for k, v in s.items()} for s in chain["samples"]]
  got = chain["qz"].validate_layer_execution(resident, signature_key="serving_default", int16_activations=True)
  want = chain["cmp"]
  assert got.skipped == {} and list(got) == list(want)
  for y, r in want.results.items():
    assert got[y]["error"] == r["error"] and got[y]["signal"] == r["signal"] and got[y]["tokens"] == r["tokens"]
    assert got[y]["activation_bits"] == 16
    assert np.array_equal(got[y]["per_channel_error"].view(np.uint64), r["per_channel_error"].view(np.uint64))
