"""Integer execution of quantized TRANSPOSE_CONV ops on the GPU (csrc/conv_patches.hip, ops.tconv_patches,
ops.tconv_forward / tconv_output / tconv_output_i16, compare_layer_execution / validate_layer_execution with
`transpose_conv`).

  1. the phase gather, byte for byte against the NumPy statement of tests/tconv_execution_cases.py: both routes at
     their smallest channel counts, every element width, every window form, guard bytes around every output; the
     crossed geometries at C = 3 and C = 16 with NaN payloads; phases with unequal tap counts, OH % sh != 0, an input
     of one pixel;
  2. the product: the accumulators of ops.tconv_forward (int32 and int64) against an independent scatter-form
     transposed convolution, and ops.tconv_output / tconv_output_i16 against the written epilogue on them;
  3. end to end: the hand-built model under four recipes, and the recorded single_conv2d_transpose_bias model
     quantized by this project's own Quantizer.
"""
import os
import sys

import numpy as np
import pytest

import conv_execution_cases as CC
import layer_error_cases as LC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC
import tconv_execution_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")

pytestmark = pytest.mark.gpu
GUARD = 64      # elements behind every output buffer
INT_VIEW = {1: "int8", 2: "int16", 4: "int32"}


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available()
  sys.path.insert(0, ROOT)
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


def _call(m, x_dev, k, s, padding, out_hw, phase, pad, first, count, out_offset=0):
  """One call of the C entry into a buffer pre-filled with a pattern, `GUARD` elements longer than the output (and
  `out_offset` elements in front); returns the rows [count, K] after checking the elements around them."""
  import ctypes
  torch = m.torch
  n, ih, iw, c = x_dev.shape
  top, left = TC.geometry(ih, iw, k[0], k[1], s, padding, out_hw)
  kys, kxs = next(p[4:] for p in TC.phases(ih, iw, k[0], k[1], s, padding, out_hw) if p[:2] == tuple(phase))
  kk = len(kys) * len(kxs) * c
  np_dtype = CC.DTYPES[x_dev.element_size()]
  fill = np.frombuffer(b"\x5a" * x_dev.element_size(), np_dtype)[0]
  buf = torch.from_numpy(np.full(out_offset + count * kk + GUARD, fill, np_dtype)).cuda()
  out = buf[out_offset:out_offset + count * kk]
  pad_host = np.asarray(pad, np_dtype).reshape(1).copy()
  st = m.lib.mi355q_tconv_patches_nhwc(m.rt.ptr(x_dev), x_dev.element_size(), n, ih, iw, c, k[0], k[1], s[0], s[1], top, left,
                                       out_hw[0], out_hw[1], phase[0], phase[1], first, count,
                                       ctypes.c_void_p(pad_host.ctypes.data), ctypes.c_void_p(out.data_ptr()), m.rt.stream_ptr())
  m.ffi.check(st)
  view = getattr(torch, INT_VIEW[x_dev.element_size()])
  around = torch.cat([buf[:out_offset], buf[out_offset + count * kk:]]).view(view)
  pattern = int.from_bytes(b"\x5a" * x_dev.element_size(), "little", signed=True)
  assert around.numel() == out_offset + GUARD and bool((around == pattern).all()), "the bytes around the output moved"
  return out.view(count, kk)


def _equal(m, got, want: np.ndarray) -> bool:
  """torch.equal on the bytes (an integer view: a NaN equals itself only as bits)."""
  view = getattr(m.torch, INT_VIEW[want.dtype.itemsize])
  return got.shape == want.shape and m.torch.equal(got.contiguous().view(view), m.dev(want).view(view))


# (N, IH, IW, kernel, strides, padding, out_hw): 4x4 stride 2 (equal tap counts); 3x3 stride 2 (phases of 2 and 1 taps)
# with OH % sh != 0; 2x5 under (2, 1) with an odd total padding; an input of one pixel; 3x3 under (3, 2)
GATHER_GEOMETRIES = [(3, 5, 7, (4, 4), (2, 2), TC.SAME, (10, 14)), (3, 3, 4, (3, 3), (2, 2), TC.VALID, (7, 10)),
                     (2, 5, 6, (2, 5), (2, 1), TC.SAME, (9, 6)), (3, 1, 1, (3, 3), (2, 2), TC.VALID, (3, 4)),
                     (2, 3, 4, (3, 3), (3, 2), TC.SAME, (8, 7)), (3, 5, 2, (3, 3), (1, 1), TC.SAME, (5, 2))]


# ---------------------------------------------------------------- 1. the gather
def test_every_route_every_window_and_both_entries(m):
  """Each (width, C, pad, alignment) of conv_execution_cases.ROUTES on six geometries, every phase and all four window
  forms; ops.tconv_patches gives the same rows. The vector route needs C elem_bytes % 16 == 0 and aligned pointers:
  int8 C = 16, int16 C = 8 and float32 C = 4 are its smallest; C = 1, 3, 20 and a misaligned base go the generic way."""
  assert all(TC.geometry(*g[1:3], *g[3], *g[4:]) is not None for g in GATHER_GEOMETRIES)
  tap_counts = set()
  for ri, route in enumerate(CC.ROUTES):
    elem_bytes, c, pad, mis = route
    for gi, (n, ih, iw, k, s, padding, out_hw) in enumerate(GATHER_GEOMETRIES):
      x = CC.random_tensor(np.random.default_rng(100 * ri + gi), (n, ih, iw, c), elem_bytes)
      x_dev = m.misaligned(x) if mis else m.dev(x)
      for py, px, qh, qw, kys, kxs in TC.phases(ih, iw, k[0], k[1], s, padding, out_hw):
        tap_counts.add((gi, len(kys), len(kxs)))
        whole = TC.gather(x, k[0], k[1], s, padding, out_hw, (py, px), pad)
        for first, count in TC.windows(n * qh * qw, qh * qw):
          want = whole[first:first + count]
          got = _call(m, x_dev, k, s, padding, out_hw, (py, px), pad, first, count)
          assert _equal(m, got, want), (route, gi, (py, px), first, count)
          got = m.ops.tconv_patches(x_dev, k[0], k[1], s, padding, out_hw, (py, px), pad, first, count)
          assert got.dtype == x_dev.dtype and _equal(m, got, want), (route, gi, (py, px), first, count)
        assert _equal(m, m.ops.tconv_patches(x_dev, k[0], k[1], s, padding, out_hw, (py, px), pad_value=pad), whole)
  assert {(1, 2, 2), (1, 2, 1), (1, 1, 2), (1, 1, 1)} <= tap_counts      # 3x3 stride 2: unequal tap counts
  # an output that begins off a 16-byte boundary takes the generic route too
  n, ih, iw, k, s, padding, out_hw = GATHER_GEOMETRIES[0]
  x = CC.random_tensor(np.random.default_rng(7), (n, ih, iw, 16), 1)
  want = TC.gather(x, k[0], k[1], s, padding, out_hw, (1, 0), 5)
  assert _equal(m, _call(m, m.dev(x), k, s, padding, out_hw, (1, 0), 5, 0, want.shape[0], out_offset=3), want)


def test_the_crossed_geometries(m):
  """Images x kernels x strides x SAME / VALID x every output size that maps back, without those that leave a phase
  no tap: every phase whole, at C = 3 (generic route, float32 of random bits: NaNs of many payloads, a NaN pad) and at
  C = 16 (vector route; int8 and float32 in turn), byte for byte."""
  cases = TC.geometries()
  assert len(cases) > 200
  for i, (n, ih, iw, k, s, padding, out_hw) in enumerate(cases):
    for c, elem_bytes, pad in ((3, 4, CC.NAN_PAYLOAD), (16, (1, 4)[i % 2], (-128, CC.NAN_PAYLOAD)[i % 2])):
      x = CC.random_tensor(np.random.default_rng(5000 + i), (n, ih, iw, c), elem_bytes)
      x_dev = m.dev(x)
      for py, px, qh, qw, kys, kxs in TC.phases(ih, iw, k[0], k[1], s, padding, out_hw):
        want = TC.gather(x, k[0], k[1], s, padding, out_hw, (py, px), pad)
        got = _call(m, x_dev, k, s, padding, out_hw, (py, px), pad, 0, n * qh * qw)
        assert _equal(m, got, want), (i, c, (py, px))


def test_ops_wrapper_checks(m):
  torch = m.torch
  x = m.dev(np.zeros((2, 5, 7, 4), np.int8))
  for bad, exc in ((dict(x=x.cpu()), TypeError), (dict(x=x.to(torch.int32)), TypeError), (dict(x=x[0]), ValueError),
                   (dict(stride=0), ValueError), (dict(padding="FULL"), ValueError), (dict(kh=0), ValueError),
                   (dict(out_hw=(11, 14)), ValueError), (dict(out_hw=(10, 12)), ValueError), (dict(phase=(2, 0)), ValueError),
                   (dict(phase=(0, -1)), ValueError), (dict(first=-1), ValueError), (dict(first=70, count=1), ValueError),
                   (dict(count=71), ValueError), (dict(pad_value=128), ValueError), (dict(pad_value=0.5), ValueError),
                   (dict(kh=1, kw=1, out_hw=(9, 13), padding="VALID", phase=(1, 0)), ValueError),      # a phase with no tap
                   (dict(x=m.dev(np.zeros((1, 5, 7, 16385), np.int8))), ValueError)):
    kw = dict(x=x, kh=4, kw=4, stride=2, padding="SAME", out_hw=(10, 14), phase=(0, 0))
    kw.update(bad)
    with pytest.raises(exc):
      m.ops.tconv_patches(**kw)
  empty = m.ops.tconv_patches(x, 4, 4, 2, "SAME", (10, 14), (1, 1), first=70, count=0)
  assert tuple(empty.shape) == (0, 16) and empty.dtype == torch.int8
  assert tuple(m.ops.tconv_patches(x, 3, 3, 2, 1, (11, 15), (1, 1)).shape) == (2 * 5 * 7, 4)      # (VALID as the schema's code)
  with pytest.raises(ValueError):
    m.ops.tconv_forward(x, m.dev(np.zeros((3, 1, 1, 4), np.float32)), 1, 1, 2, "VALID", (9, 13))      # float filter, int8 x
  with pytest.raises(ValueError):
    m.ops.tconv_forward(m.dev(np.zeros((2, 5, 7, 4), np.float32)), m.dev(np.zeros((3, 1, 1, 4), np.float32)), 1, 1, 2,
                        "VALID", (9, 13))      # a stride above the kernel
  TC.check_patch_refusals(m.lib)


# ---------------------------------------------------------------- 2. the product
PRODUCT_CASES = [  # (N, IH, IW, C, O, kernel, strides, padding, out_hw): vector and generic gathers, MFMA and generic products
    (2, 5, 6, 16, 24, (4, 4), (2, 2), TC.SAME, (9, 12)), (3, 3, 4, 3, 8, (3, 3), (2, 2), TC.VALID, (7, 10)),
    (2, 5, 6, 16, 5, (2, 5), (2, 1), TC.SAME, (9, 6)), (3, 1, 1, 20, 33, (3, 3), (2, 2), TC.VALID, (3, 4)),
    (1, 16, 16, 1, 1, (5, 5), (1, 1), TC.VALID, (20, 20)), (2, 3, 4, 64, 17, (3, 3), (3, 2), TC.SAME, (8, 7))]


def _one_hot(acc: np.ndarray) -> tuple:
  """(rows, filter) for layer_output_cases.output_i8 / output_i16: a one-hot product passes the accumulators on."""
  return acc.reshape(-1, acc.shape[-1]), np.eye(acc.shape[-1], dtype=np.int64)


def test_the_whole_op_by_phases_is_the_scatter_form(m):
  """acc of ops.tconv_forward (int32 of int8, int64 of int16) against the scatter form, y against the statement's
  rescaling, and ops.tconv_output / tconv_output_i16 against the written epilogue on those accumulators; full-range
  operands, the extremes planted in the corners of image and filter, zero points at the ends of int8."""
  torch, ops = m.torch, m.ops
  for i, (n, ih, iw, c, o, k, s, padding, out_hw) in enumerate(PRODUCT_CASES):
    rng = np.random.default_rng(300 + i)
    d = k[0] * k[1] * c
    qw = rng.integers(-128, 127, size=(o, k[0], k[1], c), endpoint=True)
    qw[0, 0, 0, :], qw[-1, -1, -1, :] = -128, 127
    per_channel = bool(i % 2)
    wsc = (np.exp(rng.normal(size=o if per_channel else 1)) * 0.01).astype(np.float32)
    target = ops.CompareTarget(m.dev(qw.astype(np.int8).ravel()), o * d, "i8", m.dev(wsc), None, o if per_channel else 1,
                               d if per_channel else 1, 32)
    sw = np.broadcast_to(wsc, (o,)).astype(np.float32)
    for zp in (0, -128, 127):
      x = rng.integers(-128, 127, size=(n, ih, iw, c), endpoint=True).astype(np.int8)
      x[:, 0, 0, :], x[:, -1, -1, :] = -128, 127
      want = TC.integer_tconv(x, zp, qw, s, padding, out_hw)
      xs = (np.exp(rng.normal(size=n if zp == 0 else 1)) * 0.02).astype(np.float32)      # one scale per image, or one
      y, acc = ops.tconv_forward(m.dev(x), target, k[0], k[1], s, padding, out_hw, x_scale=m.dev(xs), x_zero_point=zp,
                                 want_acc=True)
      assert acc.dtype == torch.int32 and tuple(acc.shape) == (n, *out_hw, o)
      assert np.array_equal(acc.cpu().numpy(), want), (i, zp)
      sc = (np.broadcast_to(xs, (n,)).astype(np.float32)[:, None] * sw[None, :])[:, None, None, :]
      assert EC.same_bits(y.cpu().numpy(), want.astype(np.int32).astype(np.float32) * sc), (i, zp)
      assert torch.equal(ops.tconv_forward(m.dev(x), target, k[0], k[1], s, padding, out_hw, x_scale=m.dev(xs), x_zero_point=zp), y)
      ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-1, 1))) * 40.0 / (np.sqrt(d) * 74.0 * 127.5)) for _ in wsc]
      mult, shift = [v[0] for v in ms], [v[1] for v in ms]
      bias = rng.integers(-3000, 3000, size=o).astype(np.int32) if i % 3 else None
      got = ops.tconv_output(m.dev(x), zp, target, k[0], k[1], s, padding, out_hw, bias, mult, shift, -3, -128, 127)
      assert got.dtype == torch.int8 and tuple(got.shape) == (n, *out_hw, o)
      rows, eye = _one_hot(want)
      assert np.array_equal(got.cpu().numpy().reshape(-1, o), OC.output_i8(rows, 0, eye, bias, mult, shift, -3, -128, 127)), (i, zp)
    x = rng.integers(-32768, 32767, size=(n, ih, iw, c), endpoint=True).astype(np.int16)
    x[:, 0, 0, :], x[:, -1, -1, :] = -32768, 32767
    want = TC.integer_tconv(x, 0, qw, s, padding, out_hw)
    xs = np.array([0.0003], np.float32)
    y, acc = ops.tconv_forward(m.dev(x), target, k[0], k[1], s, padding, out_hw, x_scale=m.dev(xs), want_acc=True)
    assert acc.dtype == torch.int64 and np.array_equal(acc.cpu().numpy(), want), (i, 16)
    sc = np.broadcast_to((xs[0] * sw)[None, :].astype(np.float32), (want.size // o, o)).copy()
    assert EC.same_bits(y.cpu().numpy().reshape(-1, o), EC16.rescale(want.reshape(-1, o), sc)), (i, 16)
    ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-1, 1))) * 9000.0 / (np.sqrt(d) * 18918.0 * 127.5)) for _ in wsc]
    mult, shift = [v[0] for v in ms], [v[1] for v in ms]
    bias = rng.integers(-(1 << 20), 1 << 20, size=o).astype(np.int64) if i % 3 else None
    got = ops.tconv_output_i16(m.dev(x), target, k[0], k[1], s, padding, out_hw, bias, mult, shift, -32768, 32767)
    assert got.dtype == torch.int16 and tuple(got.shape) == (n, *out_hw, o)
    rows, eye = _one_hot(want)
    assert np.array_equal(got.cpu().numpy().reshape(-1, o), OC.output_i16(rows, eye, bias, mult, shift, -32768, 32767)), (i, 16)


def test_the_float_op_by_phases(m):
  """ops.tconv_forward on float32 against the float64 scatter form, within the first-order bound of a K-term FP32
  product: |y - y64| <= (K + 3) 2^-24 Sum |x| |w| with K = KH KW C, which no phase exceeds."""
  ops = m.ops
  for i, (n, ih, iw, c, o, k, s, padding, out_hw) in enumerate(PRODUCT_CASES):
    rng = np.random.default_rng(400 + i)
    x = rng.standard_normal((n, ih, iw, c)).astype(np.float32)
    w = rng.standard_normal((o, k[0], k[1], c)).astype(np.float32)
    y = ops.tconv_forward(m.dev(x), m.dev(w), k[0], k[1], s, padding, out_hw).cpu().numpy()
    y64 = TC.scatter_tconv(x.astype(np.float64), w.astype(np.float64), s, padding, out_hw)
    mass = TC.scatter_tconv(np.abs(x).astype(np.float64), np.abs(w).astype(np.float64), s, padding, out_hw)
    assert y.shape == y64.shape and y.dtype == np.float32
    assert np.all(np.abs(y - y64) <= (k[0] * k[1] * c + 3) * LC.U * mass + 1e-300), i


# ---------------------------------------------------------------- 3. end to end
def _zero_point(t) -> int:
  return int(t.quantization.zeroPoint[0]) if t.quantization.zeroPoint is not None and len(t.quantization.zeroPoint) else 0


def _statement(float_model, qm, samples, x_name, y_name, k, strides, padding, out_hw, fused):
  """The statement of compare_layer_execution's TRANSPOSE_CONV evaluated in NumPy on the WRITTEN model: Y in float64 by
  the scatter form, the integer side by the scatter form on the quantized sample (neither patches nor phases), with
  the first-order bound of the device's FP32 products as test_gpu_conv_execution.py holds CONV_2D's: an element of a
  K-term FP32 product (plus one addition of the bias) lies within eps = (K + 3) 2^-24 (Sum |x| |w| + |b|) of the exact
  value, K = KH KW I bounding every phase's own K; the activations are 1-Lipschitz; so
  |error - ref| <= (1/n) Sum (2 |yq - y| eps + eps^2). Returns {error, bound, final_error, final_bound, signal,
  final_signal, mode, bits, tokens} (the final_* None unless the op is static)."""
  import test_gpu_layer_execution as G8
  from mi355q import schema
  fsg, sg = float_model.subgraphs[0], qm.subgraphs[0]
  op = next(op for op in sg.operators if schema.tensor_name(sg.tensors[op.outputs[0]]) == y_name)
  fop = next(op for op in fsg.operators if schema.tensor_name(fsg.tensors[op.outputs[0]]) == y_name)
  w_f = fsg.tensors[fop.inputs[1]]
  w64 = np.asarray(float_model.buffers[w_f.buffer].data).view(np.float32).reshape(w_f.shape).astype(np.float64)
  o, kh, kw, c = w64.shape
  d = kh * kw * c
  assert (kh, kw) == tuple(k)
  b64 = np.zeros(o)
  if len(fop.inputs) > 3 and fop.inputs[3] >= 0:
    b_f = fsg.tensors[fop.inputs[3]]
    b64 = np.asarray(float_model.buffers[b_f.buffer].data).view(np.float32).astype(np.float64)
  x_t, y_t = sg.tensors[op.inputs[2]], sg.tensors[op.outputs[0]]
  read = sg.tensors[op.inputs[1]]
  through_dequantize = read.buffer == 0 or qm.buffers[read.buffer].data is None or not len(qm.buffers[read.buffer].data)
  qw, s_w, block = G8._written_weight(qm, schema.tensor_name(w_f), o, d)      # pylint: disable=protected-access
  assert block == 0 and s_w.size in (1, o)
  qw = np.asarray(qw).reshape(o, kh, kw, c)
  s_w = np.broadcast_to(s_w, (o,)).astype(np.float32)
  int_types = {int(schema.TensorType.INT8): 8, int(schema.TensorType.INT16): 16}
  bits = int_types.get(int(x_t.type))
  mode = "static" if bits else ("weight_only" if through_dequantize else "dynamic")
  out = dict(mode=mode, bits=bits, tokens=0, signal=0.0, error=0.0, bound=0.0, final_error=None, final_bound=None, final_signal=None)
  if mode == "static":
    out.update(final_error=0.0, final_bound=0.0, final_signal=0.0)
    s_x, zp_x, s_y, zp_y = np.float32(x_t.quantization.scale[0]), _zero_point(x_t), np.float32(y_t.quantization.scale[0]), _zero_point(y_t)
    assert int(y_t.type) == int(x_t.type)
    bias = None
    if len(op.inputs) > 3 and op.inputs[3] >= 0:
      b_t = sg.tensors[op.inputs[3]]
      bias = np.asarray(qm.buffers[b_t.buffer].data).view(np.int64 if bits == 16 else np.int32)[:o]
    ms = [OC.quantize_multiplier(float(s_x) * float(v) / float(s_y)) for v in s_w.tolist()]
    mult, shift = [v[0] for v in ms], [v[1] for v in ms]
    lo, hi = OC.activation_range(fused, float(s_y), zp_y, bits)
  for sample in samples:
    x = np.asarray(sample[x_name], np.float32)
    n_img = x.shape[0]
    y64 = TC.scatter_tconv(x.astype(np.float64), w64, strides, padding, out_hw).reshape(-1, o)
    mass = TC.scatter_tconv(np.abs(x).astype(np.float64), np.abs(w64), strides, padding, out_hw).reshape(-1, o)
    n = y64.shape[0]
    eps = (d + 3) * LC.U * mass
    if mode == "weight_only":
      deq = (qw.astype(np.float32) * s_w[:, None, None, None]).astype(np.float32).astype(np.float64)
      yq = TC.scatter_tconv(x.astype(np.float64), deq, strides, padding, out_hw).reshape(-1, o)
      eps = eps + (d + 3) * LC.U * TC.scatter_tconv(np.abs(x).astype(np.float64), np.abs(deq), strides, padding, out_hw).reshape(-1, o)
    elif mode == "dynamic":
      q, scale = EC.quantize_rows(x.reshape(n_img, -1))
      acc = TC.integer_tconv(q.reshape(x.shape), 0, qw, strides, padding, out_hw).reshape(-1, o)
      sc = np.repeat(scale, n // n_img)[:, None] * s_w[None, :]
      yq = (acc.astype(np.int32).astype(np.float32) * sc).astype(np.float64)
    elif bits == 16:
      acc = TC.integer_tconv(EC16.quantize_static16(x, s_x), 0, qw, strides, padding, out_hw).reshape(-1, o)
      sc = np.broadcast_to((s_x * s_w)[None, :].astype(np.float32), acc.shape).copy()
      yq = EC16.rescale(acc, sc).astype(np.float64)
    else:
      acc = TC.integer_tconv(EC.quantize_static(x, s_x, zp_x), zp_x, qw, strides, padding, out_hw).reshape(-1, o)
      yq = (acc.astype(np.int32).astype(np.float32) * (s_x * s_w)[None, :].astype(np.float32)).astype(np.float64)
    diff = yq - y64
    out["error"] += (diff ** 2).sum()
    out["bound"] += (2.0 * np.abs(diff) * eps + eps ** 2).sum()
    out["signal"] += (y64 ** 2).sum()
    if mode == "static":
      rows, eye = _one_hot(acc)
      if bits == 16:
        q_out = OC.output_i16(rows, eye, bias, mult, shift, lo, hi)
      else:
        q_out = OC.output_i8(rows, 0, eye, bias, mult, shift, zp_y, lo, hi)
      yf = ((q_out.astype(np.int32) - zp_y).astype(np.float32) * s_y).astype(np.float64)
      ya = OC.float_activation(y64 + b64, fused)
      eps_f = (d + 3) * LC.U * (mass + np.abs(b64))
      out["final_error"] += ((yf - ya) ** 2).sum()
      out["final_bound"] += (2.0 * np.abs(yf - ya) * eps_f + eps_f ** 2).sum()
      out["final_signal"] += (ya ** 2).sum()
    out["tokens"] += n
  for key in ("error", "bound", "signal", "final_error", "final_bound", "final_signal"):
    if out[key] is not None:
      out[key] /= out["tokens"]
  return out


RECIPES = ("dynamic_wi8_afp32", "weight_only_wi8_afp32", "static_wi8_ai8", "static_wi8_ai16")
EXPECT = {"dynamic_wi8_afp32": ("dynamic", None), "weight_only_wi8_afp32": ("weight_only", None),
          "static_wi8_ai8": ("static", 8), "static_wi8_ai16": ("static", 16)}
KEYWORDS = dict(transpose_conv=True, int16_activations=True, quantized_outputs=True)


def _quantized(model, samples, name):
  from mi355q import quantizer, recipe
  from mi355q.utils import tfl_flatbuffer_utils
  qz = quantizer.Quantizer(model, getattr(recipe, name)())
  res = qz.quantize(qz.calibrate({"serving_default": samples})) if name.startswith("static") else qz.quantize()
  return qz, tfl_flatbuffer_utils.read_model(bytes(res.quantized_model))


@pytest.fixture(scope="module", params=RECIPES)
def chain(m, request):
  model = TC.build_model()
  samples = TC.build_samples(model)
  qz, qm = _quantized(model, samples, request.param)
  return dict(recipe=request.param, float=model, samples=samples, qz=qz, model=qm,
              cmp=qz.validate_layer_execution({"serving_default": samples}, **KEYWORDS))


def _hold(r, ref, o, mode, fused, line):
  """An entry's figures against the statement's, as test_gpu_conv_execution.py holds CONV_2D's."""
  line += f": error {r['error']:.6e} SNR {r['output_snr']:.1f} |error - ref| / bound {abs(r['error'] - ref['error']) / ref['bound']:.3e}"
  if mode == "static":
    line += (f"; final error {r['final_error']:.6e} SNR {r['final_output_snr']:.1f} |final_error - ref| / bound"
             f" {abs(r['final_error'] - ref['final_error']) / ref['final_bound']:.3e}")
  print(line)
  assert abs(r["error"] - ref["error"]) <= ref["bound"]
  np.testing.assert_allclose(r["signal"], ref["signal"], rtol=1e-5)
  np.testing.assert_allclose(r["error"], float(np.sum(r["per_channel_error"])), rtol=1e-12)
  assert r["per_channel_error"].shape == (o,) and 0 < r["error"] < 1e-2 * r["signal"]
  if mode == "static":
    assert "final_skipped" not in r and r["fused_activation"] == OC.NAMES[fused]
    assert abs(r["final_error"] - ref["final_error"]) <= ref["final_bound"]
    np.testing.assert_allclose(r["final_signal"], ref["final_signal"], rtol=1e-5)
    assert r["final_per_channel_error"].shape == (o,) and 0 < r["final_error"] < r["final_signal"]
  else:
    assert not [x for x in r if x.startswith("final") or x == "fused_activation"]


def test_every_op_of_the_hand_built_model_matches_the_statement(chain):
  cmp_ = chain["cmp"]
  mode, bits = EXPECT[chain["recipe"]]
  assert cmp_.skipped == {} and list(cmp_) == ["fc/y"] + [f"{c[0]}/y" for c in TC.TCONVS]
  assert cmp_["fc/y"]["op"] == "FULLY_CONNECTED" and cmp_["fc/y"]["mode"] == mode and cmp_["fc/y"]["tokens"] == 7 * TC.SAMPLES
  for tconv in TC.TCONVS:
    name, c, o, k, s, padding, has_bias, fused, out_hw = tconv
    r = cmp_[f"{name}/y"]
    ref = _statement(chain["float"], chain["model"], chain["samples"], f"{name}/x", f"{name}/y", k, s, padding, out_hw, fused)
    assert (r["op"], r["mode"], r["activation_bits"], r["output_bits"]) == ("TRANSPOSE_CONV", mode, bits, bits)
    assert (ref["mode"], ref["bits"]) == (mode, bits)
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"{name}/w", f"{name}/x", o, k[0] * k[1] * c)
    assert r["tokens"] == ref["tokens"] == TC.SAMPLES * TC.BATCH * out_hw[0] * out_hw[1]
    assert (r["kernel"], r["strides"], r["padding"], r["output_hw"], r["phases"]) == (list(k), list(s), padding, list(out_hw), s[0] * s[1])
    assert "dilations" not in r
    _hold(r, ref, o, mode, fused, f"{chain['recipe']} {name}")


def test_integer_derived_figures_equal_the_host_statement(chain):
  """With the float products in float64 on both sides (NumPy kernels, gemm_dtype float64, on the WRITTEN model), what is
  left is integer arithmetic and float32 rescaling: the device's integer-derived parts must then agree with the host
  run of the same validator to the FP32 bound of Y alone, and the token counts, modes and keys exactly."""
  from mi355q import model_validator as mv
  host = mv.compare_layer_execution(chain["float"], chain["model"], chain["samples"], kernels=TC.numpy_kernels(gemm_dtype=np.float64)(),
                                    **KEYWORDS)
  got = chain["cmp"]
  assert host.skipped == {} and list(host) == list(got)
  for tconv in TC.TCONVS:
    name, c, o, k, s, padding, has_bias, fused, out_hw = tconv
    h, r = host[f"{name}/y"], got[f"{name}/y"]
    assert sorted(h) == sorted(r)
    for key in ("op", "mode", "tokens", "rows", "d", "phases", "activation_bits", "output_bits", "kernel", "strides", "padding", "output_hw"):
      assert h[key] == r[key], (name, key)
    ref = _statement(chain["float"], chain["model"], chain["samples"], f"{name}/x", f"{name}/y", k, s, padding, out_hw, fused)
    assert abs(h["error"] - ref["error"]) <= ref["bound"] and abs(r["error"] - h["error"]) <= ref["bound"]
    if r["mode"] == "static":
      assert abs(h["final_error"] - ref["final_error"]) <= ref["final_bound"]
      assert abs(r["final_error"] - h["final_error"]) <= ref["final_bound"]


def test_device_resident_samples_give_identical_bits(chain, m):
  resident = [{k: m.dev(v) for k, v in s.items()} for s in chain["samples"]]
  got = chain["qz"].validate_layer_execution(resident, signature_key="serving_default", **KEYWORDS)
  want = chain["cmp"]
  assert got.skipped == {} and list(got) == list(want)
  for y, r in want.results.items():
    assert sorted(got[y]) == sorted(r)
    for key, v in r.items():
      if isinstance(v, np.ndarray):
        assert np.array_equal(got[y][key].view(np.uint64), v.view(np.uint64)), (y, key)
      else:
        assert got[y][key] == v, (y, key)


def test_without_the_keyword_only_the_fully_connected_entry_and_no_op_key(chain):
  plain = chain["qz"].validate_layer_execution({"serving_default": chain["samples"]}, int16_activations=True,
                                               quantized_outputs=True)
  assert list(plain) == ["fc/y"] and plain.skipped == {} and "op" not in plain["fc/y"]
  want = dict(chain["cmp"]["fc/y"])
  assert want.pop("op") == "FULLY_CONNECTED" and sorted(want) == sorted(plain["fc/y"])
  for k, v in want.items():
    assert np.array_equal(plain["fc/y"][k], v), k


@pytest.mark.parametrize("recipe_name", RECIPES)
def test_the_recorded_single_conv2d_transpose_bias(m, recipe_name):
  """1 x 16 x 16 x 1 -> 1 x 20 x 20 x 1, 5x5, VALID, stride 1 (one phase of 25 taps), quantized by this project's own
  Quantizer; the output sample for calibration is the scatter form in float64."""
  from mi355q import model_validator as mv
  from mi355q.utils import tfl_flatbuffer_utils
  float_bytes = open(os.path.join(MODELS, "single_conv2d_transpose_bias.tflite"), "rb").read()
  fm = tfl_flatbuffer_utils.read_model(float_bytes)
  x_name, y_name = "serving_default_input_6:0", "StatefulPartitionedCall:0"
  op = fm.subgraphs[0].operators[0]
  assert mv.transpose_conv_options(op) == dict(padding=1, stride_w=1, stride_h=1, fused_activation_function=0)
  w_t, b_t = (fm.subgraphs[0].tensors[op.inputs[i]] for i in (1, 3))
  w = np.asarray(fm.buffers[w_t.buffer].data).view(np.float32).reshape(1, 5, 5, 1)
  b = np.asarray(fm.buffers[b_t.buffer].data).view(np.float32)
  rng = np.random.default_rng(60)
  samples = []
  for _ in range(2):
    x = rng.standard_normal((1, 16, 16, 1), dtype=np.float32)
    y = TC.scatter_tconv(x.astype(np.float64), w.astype(np.float64), (1, 1), TC.VALID, (20, 20)) + b.astype(np.float64)
    samples.append({x_name: x, y_name: y.astype(np.float32)})
  qz, qm = _quantized(float_bytes, samples, recipe_name)
  got = qz.validate_layer_execution({"serving_default": samples}, **KEYWORDS)
  mode, bits = EXPECT[recipe_name]
  assert got.skipped == {} and list(got) == [y_name]
  r = got[y_name]
  assert (r["op"], r["mode"], r["activation_bits"], r["output_bits"]) == ("TRANSPOSE_CONV", mode, bits, bits)
  assert (r["rows"], r["d"], r["tokens"], r["phases"]) == (1, 25, 2 * 400, 1)
  assert (r["kernel"], r["strides"], r["padding"], r["output_hw"]) == ([5, 5], [1, 1], "VALID", [20, 20])
  ref = _statement(fm, qm, samples, x_name, y_name, (5, 5), (1, 1), TC.VALID, (20, 20), OC.NONE)
  assert (ref["mode"], ref["bits"], ref["tokens"]) == (mode, bits, r["tokens"])
  _hold(r, ref, 1, mode, OC.NONE, f"single_conv2d_transpose_bias {recipe_name}")
