"""Integer execution of quantized CONV_2D ops on the GPU (csrc/conv_patches.hip, ops.conv_patches,
compare_layer_execution / validate_layer_execution with `conv_2d`).

  1. the gather, byte for byte against the NumPy statement of tests/conv_execution_cases.py: both routes at their
     smallest channel counts, every element width, the crossed geometries, pad elements, row windows, guard bytes
     behind every output; an activation beyond 2^31 bytes and a launch beyond 2^32 units (the 64-bit unit index);
  2. the pad identity: patches of the quantized tensor padded with zp are the quantized patches padded with 0.0;
  3. the product: ops.qfc_forward / qfc_forward_i16 / qfc_output / qfc_output_i16 on the gathered rows against an
     independent direct integer convolution;
  4. end to end: the hand-built model under four recipes, and the reference's own recorded a8w8 model.
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


def _call(m, x_dev, k, s, dil, padding, pad, first, count, out_offset=0):
  """One call of the C entry into a buffer pre-filled with a pattern, `GUARD` elements longer than the output (and
  `out_offset` elements in front); returns (rows [count, K], the elements around them)."""
  import ctypes
  torch = m.torch
  n, h, w, c = x_dev.shape
  oh, ow, top, left = CC.geometry(h, w, k[0], k[1], s, dil, padding)
  kk = k[0] * k[1] * c
  np_dtype = CC.DTYPES[x_dev.element_size()]
  fill = np.frombuffer(b"\x5a" * x_dev.element_size(), np_dtype)[0]
  buf = torch.from_numpy(np.full(out_offset + count * kk + GUARD, fill, np_dtype)).cuda()
  out = buf[out_offset:out_offset + count * kk]
  pad_host = np.asarray(pad, np_dtype).reshape(1).copy()
  st = m.lib.mi355q_conv_patches_nhwc(m.rt.ptr(x_dev), x_dev.element_size(), n, h, w, c, k[0], k[1], s[0], s[1], dil[0],
                                      dil[1], top, left, oh, ow, first, count,
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


def _check(m, x, route, k, s, dil, padding, pad, window, tag):
  elem_bytes, c, _, mis = route
  x_dev = m.misaligned(x) if mis else m.dev(x)
  first, count = window
  want = CC.gather(x, k[0], k[1], s, dil, padding, pad, first, count)
  got = _call(m, x_dev, k, s, dil, padding, pad, first, count)
  assert _equal(m, got, want), tag
  return want


# ---------------------------------------------------------------- 1. the gather
def test_every_route_every_window_and_both_ops_entries(m):
  """Each (width, C, pad, alignment) of the route list on six geometries and all four windows; ops.conv_patches gives
  the same rows. The vector route needs C elem_bytes % 16 == 0 and aligned pointers: C = 16 / 8 / 4 are its smallest."""
  geoms = [(3, 5, 7, (3, 3), (1, 1), (1, 1), CC.SAME), (3, 5, 7, (2, 5), (2, 1), (1, 3), CC.SAME),
           (2, 4, 4, (7, 7), (1, 1), (1, 1), CC.SAME), (3, 5, 7, (3, 3), (1, 1), (1, 1), CC.VALID),
           (1, 1, 1, (1, 1), (1, 1), (1, 1), CC.VALID), (3, 5, 7, (3, 3), (3, 2), (2, 2), CC.SAME)]
  assert [CC.is_vector(*r[:2], r[3]) for r in CC.ROUTES] == [True] * 4 + [False] * 6 + [True] + [False] * 2
  for ri, route in enumerate(CC.ROUTES):
    elem_bytes, c, pad, mis = route
    for gi, (n, h, w, k, s, dil, padding) in enumerate(geoms):
      x = CC.random_tensor(np.random.default_rng(100 * ri + gi), (n, h, w, c), elem_bytes)
      oh, ow, _, _ = CC.geometry(h, w, k[0], k[1], s, dil, padding)
      for window in CC.windows(n * oh * ow, oh * ow):
        want = _check(m, x, route, k, s, dil, padding, pad, window, (route, gi, window))
        if not mis:
          got = m.ops.conv_patches(m.dev(x), k[0], k[1], s, dil, padding, pad, window[0], window[1])
          assert got.dtype == m.dev(x).dtype and _equal(m, got, want), (route, gi, window)
      whole = m.ops.conv_patches(m.misaligned(x) if mis else m.dev(x), k[0], k[1], s, dil, padding, pad_value=pad)
      assert _equal(m, whole, CC.gather(x, k[0], k[1], s, dil, padding, pad))
  # an output that begins off a 16-byte boundary takes the generic route too
  x = CC.random_tensor(np.random.default_rng(7), (3, 5, 7, 16), 1)
  want = CC.gather(x, 3, 3, (1, 1), (1, 1), CC.SAME, 5)
  assert _equal(m, _call(m, m.dev(x), (3, 3), (1, 1), (1, 1), CC.SAME, 5, 0, want.shape[0], out_offset=3), want)


def test_the_crossed_geometries(m):
  """(H, W) x kernels x strides x dilations x SAME / VALID x N, every combination with a positive output, kernels
  larger than the image among them; each on a vector and a generic route in turn, the whole output and one window."""
  cases = CC.geometries()
  assert len(cases) > 300
  vector = [r for r in CC.ROUTES if CC.is_vector(*r[:2], r[3])]
  generic = [r for r in CC.ROUTES if not CC.is_vector(*r[:2], r[3])]
  for i, (n, h, w, k, s, dil, padding) in enumerate(cases):
    oh, ow, _, _ = CC.geometry(h, w, k[0], k[1], s, dil, padding)
    wins = CC.windows(n * oh * ow, oh * ow)
    for j, route in enumerate((vector[i % len(vector)], generic[i % len(generic)])):
      x = CC.random_tensor(np.random.default_rng(5000 + i), (n, h, w, route[1]), route[0])
      for window in {wins[0], wins[(i // 2) % len(wins)]} if (i + j) % 2 else {wins[0]}:
        _check(m, x, route, k, s, dil, padding, route[2], window, (i, route, window))


@pytest.mark.parametrize("elem_bytes,pad", [(1, -128), (1, 5), (1, 127), (2, 0), (2, -32768), (4, 0.0), (4, -0.0),
                                            (4, CC.NAN_PAYLOAD)])
def test_pad_elements(m, elem_bytes, pad):
  """The pad element arrives as bytes on both routes: a NaN keeps its payload, -0.0 its sign."""
  for c in (16 // elem_bytes, 3):
    x = CC.random_tensor(np.random.default_rng(c), (2, 4, 4, c), elem_bytes)
    want = _check(m, x, (elem_bytes, c, pad, False), (3, 3), (1, 1), (2, 2), CC.SAME, pad, (0, 32), (elem_bytes, c))
    padded = np.frombuffer(np.asarray(pad, CC.DTYPES[elem_bytes]).tobytes(), np.uint8)
    taps = want.view(np.uint8).reshape(32, 9, -1)
    assert (taps[0, 0].reshape(-1, elem_bytes) == padded).all()      # the first row's first tap lies outside the image
    got = m.ops.conv_patches(m.dev(x), 3, 3, 1, 2, "same", pad)
    assert _equal(m, got, want)


def test_ops_wrapper_checks(m):
  torch = m.torch
  x = m.dev(np.zeros((2, 5, 7, 4), np.int8))
  for bad, exc in ((dict(x=x.cpu()), TypeError), (dict(x=x.to(torch.int32)), TypeError), (dict(x=x[0]), ValueError),
                   (dict(stride=0), ValueError), (dict(dilation=(1, 0)), ValueError), (dict(padding="FULL"), ValueError),
                   (dict(kh=0), ValueError), (dict(first=-1), ValueError), (dict(first=70, count=1), ValueError),
                   (dict(count=71), ValueError), (dict(pad_value=128), ValueError), (dict(pad_value=0.5), ValueError),
                   (dict(kh=9, kw=9, padding="VALID"), ValueError), (dict(x=m.dev(np.zeros((1, 2, 2, 16385), np.int8)), kh=2, kw=2), ValueError)):
    kw = dict(x=x, kh=3, kw=3, stride=1, dilation=1, padding="SAME")
    kw.update(bad)
    with pytest.raises(exc):
      m.ops.conv_patches(**kw)
  empty = m.ops.conv_patches(x, 3, 3, 1, 1, "SAME", first=70, count=0)
  assert tuple(empty.shape) == (0, 36) and empty.dtype == torch.int8
  assert tuple(m.ops.conv_patches(x, 3, 3, 2, 1, 1).shape) == (2 * 2 * 3, 36)      # (VALID as the schema's code)
  CC.check_patch_refusals(m.lib)


def test_an_activation_beyond_2_to_the_31_bytes(m):
  """N H W C = 3 x 2^30 bytes: the last image begins at byte 2^31. Only its last four rows hold data (the rest is
  zero and never read by the rows checked): the last 2 OW patch rows of a VALID 3x3 are the gather of that crop."""
  torch = m.torch
  h, w, c = 1 << 23, 8, 16
  x = torch.zeros((3, h, w, c), dtype=torch.int8, device="cuda")
  assert x.numel() > (1 << 31) + (1 << 30) - 1
  crop = CC.random_tensor(np.random.default_rng(31), (1, 4, w, c), 1)
  x[2, h - 4:] = m.dev(crop)[0]
  want = CC.gather(crop, 3, 3, (1, 1), (1, 1), CC.VALID, 9)
  oh, ow = h - 2, w - 2
  assert want.shape == (2 * ow, 9 * c)
  got = m.ops.conv_patches(x, 3, 3, 1, 1, "VALID", 9, first=3 * oh * ow - 2 * ow, count=2 * ow)      # vector route
  assert _equal(m, got, want)
  got = _call(m, x, (3, 3), (1, 1), (1, 1), CC.VALID, 9, 3 * oh * ow - 2 * ow, 2 * ow, out_offset=1)      # generic route
  assert _equal(m, got, want)
  del x
  torch.cuda.empty_cache()


def test_a_launch_beyond_2_to_the_32_units(m):
  """Generic route, int8, 2100 x 2100 x 20 under a 7x7 SAME: 4 410 000 rows of 980 elements are 4.32e9 units, more
  than a 32-bit unit index holds. Windows of the big output (its start, around unit 2^32, its end) equal the same
  windows gathered on their own (32-bit index), and those equal the NumPy statement."""
  torch = m.torch
  h = w = 2100
  c, k = 20, (7, 7)
  x = CC.random_tensor(np.random.default_rng(32), (1, h, w, c), 1)
  x_dev = m.dev(x)
  kk, rows = 49 * c, h * w
  assert rows * kk > (1 << 32) + (1 << 24)
  big = m.ops.conv_patches(x_dev, 7, 7, 1, 1, "SAME", -7)
  assert tuple(big.shape) == (rows, kk)
  cross = (1 << 32) // kk
  for first in (0, cross - 500, rows - 1000):
    part = m.ops.conv_patches(x_dev, 7, 7, 1, 1, "SAME", -7, first, 1000)
    assert torch.equal(big[first:first + 1000], part), first
    for sub in (0, 499, 936):
      want = CC.gather(x, 7, 7, (1, 1), (1, 1), CC.SAME, -7, first + sub, 64)
      assert _equal(m, part[sub:sub + 64], want), (first, sub)
  del big
  torch.cuda.empty_cache()


# ---------------------------------------------------------------- 2. the pad identity
def test_patches_of_the_quantized_tensor_are_the_quantized_patches(m):
  torch, ops = m.torch, m.ops
  rng = np.random.default_rng(40)
  x = m.dev(rng.standard_normal((3, 5, 7, 16)).astype(np.float32) * 3)

  def q(t, scale, zp, bits):
    s = torch.tensor([scale], dtype=torch.float32, device="cuda")
    z = torch.tensor([zp], dtype=torch.int32, device="cuda")
    return ops.quantize(t.contiguous(), 1, 1, t.numel(), s, z, bits, False)
  for k, s, dil, padding in (((3, 3), 1, 1, "SAME"), ((2, 5), (2, 1), (1, 3), "SAME"), ((7, 7), 1, 1, "SAME")):
    float_rows = ops.conv_patches(x, k[0], k[1], s, dil, padding, 0.0)
    for zp in (-128, 5, 127):
      a = ops.conv_patches(q(x, 0.05, zp, 8), k[0], k[1], s, dil, padding, zp)
      b = q(float_rows, 0.05, zp, 8)
      assert a.dtype == torch.int8 and torch.equal(a, b) and int((a == zp).sum()) > 1000
      if zp != 0:
        assert not torch.equal(ops.conv_patches(q(x, 0.05, zp, 8), k[0], k[1], s, dil, padding, 0), b)
    a = ops.conv_patches(q(x, 0.0004, 0, 16), k[0], k[1], s, dil, padding, 0)
    assert a.dtype == torch.int16 and torch.equal(a, q(float_rows, 0.0004, 0, 16))


# ---------------------------------------------------------------- 3. the product
def _stored(qw: np.ndarray, kind: str) -> np.ndarray:
  if kind == "i8":
    return qw.astype(np.int8).ravel()
  per = 8 // EC.BITS[kind]
  flat = qw.ravel()
  pad = (-flat.size) % per
  return LC.pack(np.concatenate([flat, np.zeros(pad, flat.dtype)]), EC.BITS[kind])


PRODUCT_CASES = [  # (C, O, kernel, strides, dilations, padding): a vector and a generic gather route, MFMA and generic products
    (16, 24, (3, 3), (1, 1), (1, 1), CC.SAME), (64, 17, (1, 1), (2, 2), (1, 1), CC.VALID), (16, 5, (2, 2), (1, 2), (2, 1), CC.SAME),
    (3, 8, (5, 5), (2, 2), (1, 1), CC.VALID), (20, 33, (3, 3), (1, 1), (2, 2), CC.SAME), (1, 4, (7, 7), (1, 1), (1, 1), CC.SAME)]


@pytest.mark.parametrize("kind", sorted(EC.BITS))
def test_the_integer_product_on_gathered_rows_is_the_direct_convolution(m, kind):
  """acc of ops.qfc_forward (int32) and ops.qfc_forward_i16 (int64) on the device's patch rows against the direct
  convolution; full-range operands, the extremes planted in the corners of image and filter (border patches)."""
  torch, ops = m.torch, m.ops
  wbits = EC.BITS[kind]
  wlo, whi = -(1 << (wbits - 1)), (1 << (wbits - 1)) - 1
  for i, (c, o, k, s, dil, padding) in enumerate(PRODUCT_CASES):
    rng = np.random.default_rng(300 + i)
    n, h, w = 3, 5, 7
    d = k[0] * k[1] * c
    qw = rng.integers(wlo, whi, size=(o, k[0], k[1], c), endpoint=True)
    qw[0, 0, 0, :], qw[-1, -1, -1, :] = wlo, whi
    per_channel = bool(i % 2)
    wsc = (np.exp(rng.normal(size=o if per_channel else 1)) * 0.01).astype(np.float32)
    target = ops.CompareTarget(m.dev(_stored(qw.reshape(o, d), kind)), o * d, kind, m.dev(wsc), None,
                               o if per_channel else 1, d if per_channel else 1, 32)
    for zp in (0, -128, 127):
      x = rng.integers(-128, 127, size=(n, h, w, c), endpoint=True).astype(np.int8)
      x[:, 0, 0, :], x[:, -1, -1, :], x[:, 0, -1, :] = -128, 127, -zp if zp > -128 else 127
      rows = ops.conv_patches(m.dev(x), k[0], k[1], s, dil, padding, zp)
      want = CC.direct_conv(x, zp, qw, s, dil, padding)
      xs = torch.tensor([0.02], dtype=torch.float32, device="cuda")
      y, acc = ops.qfc_forward(rows, xs, zp, target, o, d, want_acc=True)
      assert acc.dtype == torch.int32 and np.array_equal(acc.cpu().numpy(), want), (kind, i, zp)
      assert EC.same_bits(y.cpu().numpy(), EC.forward(rows.cpu().numpy(), [0.02], zp, qw.reshape(o, d), wsc)[1])
      # through to the stored output, on the same rows
      ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-1, 1))) * 40.0 / (np.sqrt(d) * 74.0 * (whi + 0.5))) for _ in wsc]
      mult, shift = [v[0] for v in ms], [v[1] for v in ms]
      bias = rng.integers(-3000, 3000, size=o).astype(np.int32) if i % 3 else None
      got = ops.qfc_output(rows, zp, target, o, d, bias, mult, shift, -3, -128, 127)
      assert np.array_equal(got.cpu().numpy(), OC.output_i8(rows.cpu().numpy(), zp, qw.reshape(o, d), bias, mult, shift, -3, -128, 127))
    x = rng.integers(-32768, 32767, size=(n, h, w, c), endpoint=True).astype(np.int16)
    x[:, 0, 0, :], x[:, -1, -1, :] = -32768, 32767
    rows = ops.conv_patches(m.dev(x), k[0], k[1], s, dil, padding, 0)
    want = CC.direct_conv(x, 0, qw, s, dil, padding)
    xs = torch.tensor([0.0003], dtype=torch.float32, device="cuda")
    y, acc = ops.qfc_forward_i16(rows, xs, target, o, d, want_acc=True)
    assert acc.dtype == torch.int64 and np.array_equal(acc.cpu().numpy(), want), (kind, i, 16)
    ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-1, 1))) * 9000.0 / (np.sqrt(d) * 18918.0 * (whi + 0.5))) for _ in wsc]
    mult, shift = [v[0] for v in ms], [v[1] for v in ms]
    bias = rng.integers(-(1 << 20), 1 << 20, size=o).astype(np.int64) if i % 3 else None
    got = ops.qfc_output_i16(rows, target, o, d, bias, mult, shift, -32768, 32767)
    assert np.array_equal(got.cpu().numpy(), OC.output_i16(rows.cpu().numpy(), qw.reshape(o, d), bias, mult, shift, -32768, 32767))


# ---------------------------------------------------------------- 4. end to end
def _zero_point(t) -> int:
  return int(t.quantization.zeroPoint[0]) if t.quantization.zeroPoint is not None and len(t.quantization.zeroPoint) else 0


def _statement(float_model, qm, samples, x_name, y_name, k, strides, dil, padding, fused):
  """The statement of compare_layer_execution's CONV_2D evaluated in NumPy on the WRITTEN model, Y in float64, with
  the first-order bound of the device's FP32 products: an element of a K-term FP32 product (plus one addition of the
  bias) lies within eps = (K + 3) 2^-24 (Sum |x| |w| + |b|) of the exact value; the activations are 1-Lipschitz; so
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
  if len(fop.inputs) > 2 and fop.inputs[2] >= 0:
    b_f = fsg.tensors[fop.inputs[2]]
    b64 = np.asarray(float_model.buffers[b_f.buffer].data).view(np.float32).astype(np.float64)
  x_t, y_t = sg.tensors[op.inputs[0]], sg.tensors[op.outputs[0]]
  read = sg.tensors[op.inputs[1]]
  through_dequantize = read.buffer == 0 or qm.buffers[read.buffer].data is None or not len(qm.buffers[read.buffer].data)
  qw, s_w, block = G8._written_weight(qm, schema.tensor_name(w_f), o, d)      # pylint: disable=protected-access
  assert block == 0 and s_w.size in (1, o)
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
    if len(op.inputs) > 2 and op.inputs[2] >= 0:
      b_t = sg.tensors[op.inputs[2]]
      bias = np.asarray(qm.buffers[b_t.buffer].data).view(np.int64 if bits == 16 else np.int32)[:o]
    ms = [OC.quantize_multiplier(float(s_x) * float(v) / float(s_y)) for v in s_w.tolist()]
    mult, shift = [v[0] for v in ms], [v[1] for v in ms]
    lo, hi = OC.activation_range(fused, float(s_y), zp_y, bits)
  for sample in samples:
    x = np.asarray(sample[x_name], np.float32)
    p = CC.gather(x, kh, kw, strides, dil, padding, 0.0)
    n = p.shape[0]
    y64 = p.astype(np.float64) @ w64.reshape(o, d).T
    mass = np.abs(p).astype(np.float64) @ np.abs(w64.reshape(o, d)).T
    eps = (d + 3) * LC.U * mass
    if mode == "weight_only":
      deq = (qw.astype(np.float32) * s_w[:, None]).astype(np.float32)
      yq = p.astype(np.float64) @ deq.astype(np.float64).T
      eps = eps + (d + 3) * LC.U * (np.abs(p).astype(np.float64) @ np.abs(deq).astype(np.float64).T)      # (two FP32 products)
    elif mode == "dynamic":
      q, scale = EC.quantize_rows(x.reshape(x.shape[0], -1))
      rows = CC.gather(q.reshape(x.shape), kh, kw, strides, dil, padding, 0)
      yq = EC.forward(rows, np.repeat(scale, n // x.shape[0]), 0, qw, s_w)[1].astype(np.float64)
    elif bits == 16:
      rows = CC.gather(EC16.quantize_static16(x, s_x), kh, kw, strides, dil, padding, 0)
      yq = EC16.forward16(rows, [s_x], qw, s_w)[1].astype(np.float64)
    else:
      rows = CC.gather(EC.quantize_static(x, s_x, zp_x), kh, kw, strides, dil, padding, zp_x)
      yq = EC.forward(rows, [s_x], zp_x, qw, s_w)[1].astype(np.float64)
    diff = yq - y64
    out["error"] += (diff ** 2).sum()
    out["bound"] += (2.0 * np.abs(diff) * eps + eps ** 2).sum()
    out["signal"] += (y64 ** 2).sum()
    if mode == "static":
      if bits == 16:
        q_out = OC.output_i16(rows, qw, bias, mult, shift, lo, hi)
      else:
        q_out = OC.output_i8(rows, zp_x, qw, bias, mult, shift, zp_y, lo, hi)
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


@pytest.fixture(scope="module", params=RECIPES)
def chain(m, request):
  from mi355q import quantizer, recipe
  from mi355q.utils import tfl_flatbuffer_utils
  model = CC.build_model()
  samples = CC.build_samples(model)
  qz = quantizer.Quantizer(model, getattr(recipe, request.param)())
  if request.param.startswith("static"):
    res = qz.quantize(qz.calibrate({"serving_default": samples}))
  else:
    res = qz.quantize()
  return dict(recipe=request.param, float=model, samples=samples, qz=qz,
              model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)),
              cmp=qz.validate_layer_execution({"serving_default": samples}, conv_2d=True, int16_activations=True,
                                              quantized_outputs=True))


def test_every_conv_of_the_hand_built_model_matches_the_statement(chain):
  cmp_ = chain["cmp"]
  mode, bits = EXPECT[chain["recipe"]]
  assert cmp_.skipped == {} and list(cmp_) == ["fc/y"] + [f"{c[0]}/y" for c in CC.CONVS]
  assert cmp_["fc/y"]["op"] == "FULLY_CONNECTED" and cmp_["fc/y"]["mode"] == mode and cmp_["fc/y"]["tokens"] == 7 * CC.SAMPLES
  for conv in CC.CONVS:
    name, c, o, k, s, dil, padding, has_bias, fused = conv
    r = cmp_[f"{name}/y"]
    ref = _statement(chain["float"], chain["model"], chain["samples"], f"{name}/x", f"{name}/y", k, s, dil, padding, fused)
    oh, ow, _, _ = CC.geometry(CC.HEIGHT, CC.WIDTH, k[0], k[1], s, dil, padding)
    line = f"{chain['recipe']} {name}: error {r['error']:.6e} SNR {r['output_snr']:.1f} |error - ref| / bound {abs(r['error'] - ref['error']) / ref['bound']:.3e}"
    assert (r["op"], r["mode"], r["activation_bits"], r["output_bits"]) == ("CONV_2D", mode, bits, bits)
    assert (ref["mode"], ref["bits"]) == (mode, bits)
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"{name}/w", f"{name}/x", o, k[0] * k[1] * c)
    assert r["tokens"] == ref["tokens"] == CC.SAMPLES * CC.BATCH * oh * ow
    assert (r["kernel"], r["strides"], r["dilations"], r["padding"], r["output_hw"]) == (list(k), list(s), list(dil), padding, [oh, ow])
    if mode == "static":
      line += f"; final error {r['final_error']:.6e} SNR {r['final_output_snr']:.1f} |final_error - ref| / bound {abs(r['final_error'] - ref['final_error']) / ref['final_bound']:.3e}"
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


def test_device_resident_samples_give_identical_bits(chain, m):
  resident = [{k: m.dev(v) for k, v in s.items()} for s in chain["samples"]]
  got = chain["qz"].validate_layer_execution(resident, signature_key="serving_default", conv_2d=True,
                                             int16_activations=True, quantized_outputs=True)
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


def test_the_recorded_a8w8_conv_fc_mnist(m):
  """compare_layer_execution on the reference's own recorded quantized file: the conv that reads the model's input."""
  from mi355q import model_validator as mv
  from mi355q.utils import tfl_flatbuffer_utils
  float_bytes = open(os.path.join(MODELS, "conv_fc_mnist.tflite"), "rb").read()
  quant_bytes = open(os.path.join(MODELS, "conv_fc_mnist_srq_a8w8.tflite"), "rb").read()
  x_name, fc1, fc2 = "serving_default_conv2d_input:0", "sequential/flatten/Reshape", "sequential/dense/MatMul;sequential/dense/Relu;sequential/dense/BiasAdd"
  y_name = "sequential/conv2d/Relu;sequential/conv2d/BiasAdd;sequential/conv2d/Conv2D;sequential/conv2d/BiasAdd/ReadVariableOp1"
  rng = np.random.default_rng(50)
  n = 3
  samples = [{x_name: rng.random((n, 28, 28, 1), dtype=np.float32), fc1: rng.random((n, 1568), dtype=np.float32),
              fc2: rng.random((n, 32), dtype=np.float32) * 4} for _ in range(2)]
  got = mv.compare_layer_execution(float_bytes, quant_bytes, samples, conv_2d=True, quantized_outputs=True)
  assert got.skipped == {} and len(got) == 3 and [r["op"] for r in got.results.values()] == ["FULLY_CONNECTED"] * 2 + ["CONV_2D"]
  r = got[y_name]
  assert (r["mode"], r["output_bits"], r["d"], r["rows"], r["tokens"]) == ("static", 8, 9, 8, 784 * n * 2)
  assert (r["kernel"], r["strides"], r["dilations"], r["padding"], r["output_hw"]) == ([3, 3], [1, 1], [1, 1], "SAME", [28, 28])
  assert r["fused_activation"] == "RELU" and "final_skipped" not in r
  assert all(np.isfinite(r[k]) for k in ("final_signal", "final_error", "final_output_mse", "final_output_snr"))
  assert np.all(np.isfinite(r["final_per_channel_error"])) and 0 < r["final_error"] < r["final_signal"]
  host = mv.compare_layer_execution(float_bytes, quant_bytes, samples, conv_2d=True, quantized_outputs=True,
                                    kernels=CC.numpy_kernels(gemm_dtype=np.float64)())
  ref = _statement(tfl_flatbuffer_utils.read_model(float_bytes), tfl_flatbuffer_utils.read_model(quant_bytes), samples,
                   x_name, y_name, (3, 3), (1, 1), (1, 1), CC.SAME, OC.RELU)
  h = host[y_name]
  print(f"conv_fc_mnist a8w8 conv: error {r['error']:.6e} (host {h['error']:.6e}) final {r['final_error']:.6e} (host"
        f" {h['final_error']:.6e}) SNR {r['final_output_snr']:.1f}; / bound {abs(r['error'] - h['error']) / ref['bound']:.3e}"
        f" {abs(r['final_error'] - h['final_error']) / ref['final_bound']:.3e}")
  # the host kernels form the products in float64 but round Y to float32 before the bias is added (one rounding of at
  # most 2^-24 |y| <= eps per element), so their figures lie within the same bound of the float64 statement
  assert abs(h["error"] - ref["error"]) <= ref["bound"] and abs(h["final_error"] - ref["final_error"]) <= ref["final_bound"]
  np.testing.assert_allclose([h["error"], h["final_error"]], [ref["error"], ref["final_error"]], rtol=1e-6)
  assert abs(r["error"] - h["error"]) <= ref["bound"] and abs(r["final_error"] - h["final_error"]) <= ref["final_bound"]
  assert (h["tokens"], h["mode"], h["fused_activation"]) == (r["tokens"], r["mode"], r["fused_activation"])
  for y in got:      # the two FULLY_CONNECTED entries are there as before, with the same figures as the host's to FP32
    np.testing.assert_allclose(got[y]["signal"], host[y]["signal"], rtol=1e-4)
