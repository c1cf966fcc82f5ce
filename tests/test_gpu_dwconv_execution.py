"""Integer execution of quantized DEPTHWISE_CONV_2D ops on the GPU (csrc/dwconv.hip, ops.dwconv_forward /
dwconv_output / dwconv_output_i16, compare_layer_execution / validate_layer_execution with `depthwise_conv_2d`).

  1. the accumulators of the int8 and int16 entries, bit for bit against the independent direct convolution of
     tests/dwconv_execution_cases.py, on every crossed geometry and both routes;
  2. all five entries on both routes, every window, both scale granularities and scale counts, bit for bit against
     the statement (the epilogue statement of layer_output_cases on the direct convolution's accumulators);
  3. the extremes of both integer types; 4. the float route, with signed zeros and infinities; 5. the wrappers' checks;
  6. end to end: the hand-built model through the Quantizer under four recipes.
"""
import os
import sys

import numpy as np
import pytest

import conv_execution_cases as CC
import dwconv_execution_cases as DW
import layer_error_cases as LC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


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

  def target(qw, scale):
    """The int8 filter [KH, KW, O] as the validators hand it over: per tensor (one scale), or per channel along the
    last dimension (O scales: channels = O, inner = 1)."""
    scale = np.asarray(scale, np.float32).reshape(-1)
    return ops.CompareTarget(M.dev(qw.astype(np.int8).ravel()), qw.size, "i8", M.dev(scale), None, scale.size, 1, 32)
  M.target = staticmethod(target)
  return M


def _tables(rng, o, per_channel, real):
  ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-1, 1))) * real) for _ in range(o if per_channel else 1)]
  return [v[0] for v in ms], [v[1] for v in ms]


# ---------------------------------------------------------------- 1. the accumulators
def test_accumulators_on_every_geometry_and_both_routes(m):
  """acc_out of the i8 (int32) and i16 (int64) entries against the direct convolution, on every geometry of the CONV_2D
  cross (kernels larger than the image among them) at (C, M) = (4, 1), the vector route, and (3, 2), the generic
  one; full-range operands with the extremes planted in the corners, zero points at the ends of int8."""
  torch, ops = m.torch, m.ops
  cases = CC.geometries()
  assert len(cases) > 300
  xs = torch.tensor([0.02], dtype=torch.float32, device="cuda")
  for i, (n, h, w, k, s, dil, padding) in enumerate(cases):
    rng = np.random.default_rng(7000 + i)
    for c, mult in ((4, 1), (3, 2)):
      o = c * mult
      qw = rng.integers(-128, 127, size=(k[0], k[1], o), endpoint=True)
      qw[0, 0, :], qw[-1, -1, :] = -128, 127
      tgt = m.target(qw, [0.01])
      zp = (0, -128, 127, 5)[i % 4]
      x = rng.integers(-128, 127, size=(n, h, w, c), endpoint=True).astype(np.int8)
      x[:, 0, 0, :], x[:, -1, -1, :] = -128, 127
      _, acc = ops.dwconv_forward(m.dev(x), tgt, k[0], k[1], s, dil, padding, mult, x_scale=xs, x_zero_point=zp, want_acc=True)
      assert acc.dtype == torch.int32 and np.array_equal(acc.cpu().numpy(), DW.direct_depthwise(x, zp, qw, mult, s, dil, padding)), (i, c, 8)
      x = rng.integers(-32768, 32767, size=(n, h, w, c), endpoint=True).astype(np.int16)
      x[:, 0, 0, :], x[:, -1, -1, :] = -32768, 32767
      _, acc = ops.dwconv_forward(m.dev(x), tgt, k[0], k[1], s, dil, padding, mult, x_scale=xs, want_acc=True)
      assert acc.dtype == torch.int64 and np.array_equal(acc.cpu().numpy(), DW.direct_depthwise(x, 0, qw, mult, s, dil, padding)), (i, c, 16)


# ---------------------------------------------------------------- 2. routes x entries
GEOMETRIES = [(3, 5, 7, (3, 3), (1, 1), (1, 1), CC.SAME), (3, 5, 7, (2, 5), (2, 1), (1, 3), CC.SAME),
              (2, 4, 4, (7, 7), (1, 1), (1, 1), CC.SAME), (3, 5, 7, (3, 3), (1, 1), (1, 1), CC.VALID),
              (1, 1, 1, (1, 1), (1, 1), (1, 1), CC.VALID), (3, 5, 7, (3, 3), (3, 2), (2, 2), CC.SAME)]
# (C, M, misaligned base): vector (68 channels: 17 groups, more than one wave's worth of lanes with the pixels, and a
# ragged last wave); generic by shape, and by a base one element off; a depth multiplier
CHANNELS = [(4, 1, False), (8, 1, False), (68, 1, False), (1, 1, False), (3, 1, False), (20, 1, True), (4, 2, False), (5, 3, False)]


@pytest.mark.parametrize("c,mult,mis", CHANNELS)
def test_all_five_entries_on_every_route_and_window(m, c, mult, mis):
  torch, ops = m.torch, m.ops
  put = m.misaligned if mis else m.dev
  o = c * mult
  for gi, (n, h, w, k, s, dil, padding) in enumerate(GEOMETRIES):
    rng = np.random.default_rng(100 * c + 10 * mult + gi)
    oh, ow, _, _ = CC.geometry(h, w, k[0], k[1], s, dil, padding)
    args = (k[0], k[1], s, dil, padding)
    qw = rng.integers(-128, 127, size=(k[0], k[1], o), endpoint=True)
    qw[0, 0, :], qw[-1, -1, :] = -128, 127
    zp = (-128, 5, 127, 0)[gi % 4]
    x8 = rng.integers(-128, 127, size=(n, h, w, c), endpoint=True).astype(np.int8)
    x16 = rng.integers(-32768, 32767, size=(n, h, w, c), endpoint=True).astype(np.int16)
    xf = rng.standard_normal((n, h, w, c)).astype(np.float32)
    wf = rng.standard_normal((k[0], k[1], o)).astype(np.float32)
    acc8, acc16 = DW.direct_depthwise(x8, zp, qw, mult, s, dil, padding), DW.direct_depthwise(x16, 0, qw, mult, s, dil, padding)
    yf = DW.float_depthwise(xf, wf, mult, s, dil, padding)
    bias8 = rng.integers(-3000, 3000, size=o).astype(np.int32) if gi % 3 else None
    bias16 = rng.integers(-(1 << 20), 1 << 20, size=o).astype(np.int64) if gi % 3 else None
    taps = k[0] * k[1]
    for wi, (first, count) in enumerate(CC.windows(n * oh * ow, oh * ow)):
      rows = slice(first, first + count)
      win = dict(first=first, count=count)
      got = ops.dwconv_forward(put(xf), put(wf), *args, mult, **win)
      assert EC.same_bits(got.cpu().numpy(), yf[rows]), (gi, "f32", first, count)
      for per_channel, per_image in ((False, False), (True, True)) if wi == 0 else (((gi + wi) % 2 == 0, (gi + wi) % 3 == 0),):
        wsc = (np.exp(rng.normal(size=o if per_channel else 1)) * 0.01).astype(np.float32)
        xsc = (np.exp(rng.normal(size=n if per_image else 1)) * 0.02).astype(np.float32)
        tgt = m.target(qw, wsc)
        y, acc = ops.dwconv_forward(put(x8), tgt, *args, mult, x_scale=m.dev(xsc), x_zero_point=zp, want_acc=True, **win)
        assert np.array_equal(acc.cpu().numpy(), acc8[rows]), (gi, "i8 acc", first, count)
        assert EC.same_bits(y.cpu().numpy(), DW.rescale_i8(acc8, xsc, wsc, n)[rows]), (gi, "i8", first, count, per_channel, per_image)
        y = ops.dwconv_forward(put(x8), tgt, *args, mult, x_scale=m.dev(xsc), x_zero_point=zp, **win)      # (no acc_out)
        assert EC.same_bits(y.cpu().numpy(), DW.rescale_i8(acc8, xsc, wsc, n)[rows])
        y, acc = ops.dwconv_forward(put(x16), tgt, *args, mult, x_scale=m.dev(xsc * np.float32(0.01)), want_acc=True, **win)
        assert acc.dtype == torch.int64 and np.array_equal(acc.cpu().numpy(), acc16[rows]), (gi, "i16 acc", first, count)
        assert EC.same_bits(y.cpu().numpy(), DW.rescale_i16(acc16, xsc * np.float32(0.01), wsc, n)[rows]), (gi, "i16", first, count)
        # through to the stored output: multipliers that bring the accumulators onto the output type's range
        mult8, shift8 = _tables(rng, o, per_channel, 40.0 / (np.sqrt(taps) * 74.0 * 127.5))
        got = ops.dwconv_output(put(x8), zp, tgt, *args, bias8, mult8, shift8, -3, -128, 127, mult, **win)
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), DW.epilogue_i8(acc8[rows], bias8, mult8, shift8, -3, -128, 127)), (gi, "out8", first, count)
        got = ops.dwconv_output(put(x8), zp, tgt, *args, bias8, mult8, shift8, 7, -20, 31, mult, **win)      # (a fused range)
        assert np.array_equal(got.cpu().numpy(), DW.epilogue_i8(acc8[rows], bias8, mult8, shift8, 7, -20, 31))
        mult16, shift16 = _tables(rng, o, per_channel, 9000.0 / (np.sqrt(taps) * 18918.0 * 127.5))
        got = ops.dwconv_output_i16(put(x16), tgt, *args, bias16, mult16, shift16, -32768, 32767, mult, **win)
        assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), DW.epilogue_i16(acc16[rows], bias16, mult16, shift16, -32768, 32767)), (gi, "out16", first, count)
        prepared = ops.qfc_multipliers(mult16, shift16, o, 16)      # the prepared tables qfc_output_i16 takes
        got = ops.dwconv_output_i16(put(x16), tgt, *args, bias16, prepared, None, 0, 9000, mult, **win)
        assert np.array_equal(got.cpu().numpy(), DW.epilogue_i16(acc16[rows], bias16, mult16, shift16, 0, 9000))


def test_outputs_off_a_16_byte_boundary_take_the_generic_route(m):
  """The C entry with y_out one element past an aligned address (C = 8, M = 1 would be the vector route), guard elements
  around the output: the same bits, and nothing written outside."""
  import ctypes
  torch = m.torch
  rng = np.random.default_rng(9)
  n, h, w, c, k, s, dil, padding = 2, 5, 7, 8, (3, 3), (1, 1), (1, 1), CC.SAME
  oh, ow, top, left = CC.geometry(h, w, k[0], k[1], s, dil, padding)
  xf, wf = rng.standard_normal((n, h, w, c)).astype(np.float32), rng.standard_normal((3, 3, c)).astype(np.float32)
  want = DW.float_depthwise(xf, wf, 1, s, dil, padding)
  x_dev, w_dev = m.dev(xf), m.dev(wf)
  for offset in (0, 1):
    buf = torch.full((offset + want.size + 64,), 12345.0, dtype=torch.float32, device="cuda")
    out = buf[offset:offset + want.size]
    st = m.lib.mi355q_dwconv_forward_f32(m.rt.ptr(x_dev), n, h, w, c, m.rt.ptr(w_dev), 3, 3, 1, 1, 1, 1, 1, top, left, oh, ow, 0,
                                         n * oh * ow, ctypes.c_void_p(out.data_ptr()), m.rt.stream_ptr())
    m.ffi.check(st)
    assert EC.same_bits(out.view(want.shape).cpu().numpy(), want), offset
    assert bool((buf[:offset] == 12345.0).all()) and bool((buf[offset + want.size:] == 12345.0).all()), offset


# ---------------------------------------------------------------- 3. the extremes
def test_int8_extremes_and_epilogue_ties(m):
  torch, ops = m.torch, m.ops
  xs = torch.tensor([1.0], dtype=torch.float32, device="cuda")
  # x = -128 with zp = 127 and w = -128, a 7x7 VALID kernel all inside: 49 * 255 * 128, on both routes
  for c in (4, 3):
    x = np.full((1, 7, 7, c), -128, np.int8)
    qw = np.full((7, 7, c), -128)
    y, acc = ops.dwconv_forward(m.dev(x), m.target(qw, [1.0]), 7, 7, 1, 1, "VALID", x_scale=xs, x_zero_point=127, want_acc=True)
    assert acc.cpu().numpy().tolist() == [[49 * 255 * 128] * c] and y.cpu().numpy().tolist() == [[float(49 * 255 * 128)] * c]
    assert np.array_equal(acc.cpu().numpy(), DW.direct_depthwise(x, 127, qw, 1, (1, 1), (1, 1), CC.VALID))
  # ties of the epilogue's two roundings: a 1x1 filter of 1 passes x - zp on as the accumulator, -255 .. 255; with
  # M = 2^30 and shift 0 the multiplier is 1/2 (every odd accumulator is a tie, rounded away from zero), with shift -1
  # and -2 the rounding right shift meets ties of its own; [act_min, act_max] cuts through the middle of the values
  clamped = 0
  for c in (4, 1):
    x = np.arange(-128, 128, dtype=np.int64).astype(np.int8).reshape(1, 16, 16, 1).repeat(c, axis=3)
    qw = np.ones((1, 1, c))
    for zp in (127, -128, 0):
      acc = DW.direct_depthwise(x, zp, qw, 1, (1, 1), (1, 1), CC.VALID)
      for mult, shift in ((1 << 30, 0), (1 << 30, -1), (1 << 30, -2), (3 << 29, -1), (1 << 30, 1)):
        for zp_y, lo, hi in ((0, -128, 127), (0, -31, 32), (-5, -5, 100)):
          got = ops.dwconv_output(m.dev(x), zp, m.target(qw, [1.0]), 1, 1, 1, 1, "VALID", None, [mult], [shift], zp_y, lo, hi)
          want = DW.epilogue_i8(acc, None, [mult], [shift], zp_y, lo, hi)
          assert np.array_equal(got.cpu().numpy(), want), (c, zp, mult, shift, zp_y)
          clamped += int(want.min() == lo) + int(want.max() == hi)
    got = ops.dwconv_output(m.dev(x), 0, m.target(qw, [1.0]), 1, 1, 1, 1, "VALID", None, [1 << 30], [0], 0, -128, 127).cpu().numpy()
    by_acc = dict(zip(x[0, :, :, 0].ravel().tolist(), got[:, 0].tolist()))
    # a / 2 by the statement's doubling high multiplication: h = trunc((a 2^30 + nudge) / 2^31), nudge 2^30 for a >= 0
    # and 1 - 2^30 below: 1/2 -> 1, 3/2 -> 2, 5/2 -> 3, and -1/2 -> 0, -3/2 -> -1 (worked out by hand)
    assert [by_acc[a] for a in (-3, -2, -1, 0, 1, 2, 3, 5)] == [-1, -1, 0, 0, 1, 1, 2, 3]
  assert clamped > 40      # (the ranges cut through the values: both ends are reached again and again)


def test_int16_extremes_an_accumulator_above_int32(m):
  """x = -32768, w = -128, a 23x23 VALID kernel on a 23x23 image: the one accumulator is 529 * 2^22 = 2 218 786 816,
  above 2^31 - 1; exact, in acc_out, in the rescale through float64 and through the int16 epilogue."""
  torch, ops = m.torch, m.ops
  for c in (4, 3):
    x = np.full((1, 23, 23, c), -32768, np.int16)
    qw = np.full((23, 23, c), -128)
    tgt = m.target(qw, [0.5])
    xs = torch.tensor([0.25], dtype=torch.float32, device="cuda")
    y, acc = ops.dwconv_forward(m.dev(x), tgt, 23, 23, 1, 1, "VALID", x_scale=xs, want_acc=True)
    assert 529 * (1 << 22) == 2218786816 > (1 << 31) - 1
    assert acc.dtype == torch.int64 and acc.cpu().numpy().tolist() == [[2218786816] * c]
    assert y.cpu().numpy().tolist() == [[2218786816 / 8.0] * c]      # (529 * 2^19 is a float32)
    want = DW.direct_depthwise(x, 0, qw, 1, (1, 1), (1, 1), CC.VALID)
    assert np.array_equal(acc.cpu().numpy(), want)
    for mult, shift, bias in ((1 << 30, -16, None), (0x7FFFFFFF, -17, np.full(c, -(1 << 31), np.int64)), (1 << 30, -15, None)):
      got = ops.dwconv_output_i16(m.dev(x), tgt, 23, 23, 1, 1, "VALID", bias, [mult], [shift], -32768, 32767)
      assert np.array_equal(got.cpu().numpy(), DW.epilogue_i16(want, bias, [mult], [shift], -32768, 32767)), (c, mult, shift)
    # Mr = 2^14, T = 31: (529 2^36 + 2^30) >> 31 = 16928, inside int16; with T = 30 it is 33856 and saturates
    assert ops.dwconv_output_i16(m.dev(x), tgt, 23, 23, 1, 1, "VALID", None, [1 << 30], [-16], -32768, 32767).cpu().numpy().tolist() == [[16928] * c]
    assert ops.dwconv_output_i16(m.dev(x), tgt, 23, 23, 1, 1, "VALID", None, [1 << 30], [-15], -32768, 32767).cpu().numpy().tolist() == [[32767] * c]


# ---------------------------------------------------------------- 4. the float route
@pytest.mark.parametrize("c,mult", [(4, 1), (68, 1), (3, 2)])
def test_float_route_signed_zeros_and_infinities(m, c, mult):
  ops = m.ops
  rng = np.random.default_rng(40 + c)
  n, h, w, k, s, dil, padding = 3, 9, 11, (3, 3), (1, 1), (1, 1), CC.SAME
  x = rng.standard_normal((n, h, w, c)).astype(np.float32)
  wt = rng.standard_normal((3, 3, c * mult)).astype(np.float32)
  x[rng.random(x.shape) < 0.05] = 0.0
  x[rng.random(x.shape) < 0.05] = -0.0
  wt[0, 0, 0], wt[2, 2, -1] = -0.0, 0.0
  x[:, 0, 0, :] = -0.0      # (a corner pixel whose every tap inside is -0.0 * w: the sum of signed zeros)
  want = DW.float_depthwise(x, wt, mult, s, dil, padding)
  assert np.isfinite(want).all() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
  got = ops.dwconv_forward(m.dev(x), m.dev(wt), 3, 3, s, dil, padding, mult).cpu().numpy()
  assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
  for stride, dilation, pad in (((2, 2), (1, 1), CC.SAME), ((1, 2), (2, 1), CC.VALID)):
    got = ops.dwconv_forward(m.dev(x), m.dev(wt), 3, 3, stride, dilation, pad, mult).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), DW.float_depthwise(x, wt, mult, stride, dilation, pad).view(np.uint32))
  # a planted +inf: inf, -inf or NaN (inf * 0, inf - inf) at the same positions, the finite values unchanged
  x[1, 4, 5, :] = np.inf
  want = DW.float_depthwise(x, wt, mult, s, dil, padding)
  got = ops.dwconv_forward(m.dev(x), m.dev(wt), 3, 3, s, dil, padding, mult).cpu().numpy()
  assert np.isinf(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
  assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


# ---------------------------------------------------------------- 5. the wrappers
def test_ops_wrapper_checks(m):
  torch, ops = m.torch, m.ops
  x8 = m.dev(np.zeros((2, 5, 7, 4), np.int8))
  x16, xf = x8.to(torch.int16), x8.to(torch.float32)
  qw = np.ones((3, 3, 4))
  tgt = m.target(qw, [0.5])
  xs = torch.tensor([0.1], dtype=torch.float32, device="cuda")
  wf = m.dev(qw.astype(np.float32))
  good = dict(x=x8, w=tgt, kh=3, kw=3, stride=1, dilation=1, padding="SAME", x_scale=xs)
  assert tuple(ops.dwconv_forward(**good).shape) == (70, 4)
  along_0 = ops.CompareTarget(tgt.data, 36, "i8", m.dev(np.ones(3, np.float32)), None, 3, 12, 32)
  with_zp = ops.CompareTarget(tgt.data, 36, "i8", tgt.scale, m.dev(np.ones(1, np.int32)), 1, 1, 32)
  for bad, exc in ((dict(x=x8.cpu()), TypeError), (dict(x=x8.to(torch.int32)), TypeError), (dict(x=x8[0]), ValueError),
                   (dict(stride=0), ValueError), (dict(dilation=(1, 0)), ValueError), (dict(padding="FULL"), ValueError),
                   (dict(kh=0), ValueError), (dict(first=-1), ValueError), (dict(first=70, count=1), ValueError),
                   (dict(count=71), ValueError), (dict(depth_multiplier=0), ValueError), (dict(depth_multiplier=2), ValueError),
                   (dict(kh=9, kw=9, padding="VALID"), ValueError), (dict(x_scale=None), ValueError),
                   (dict(x_scale=torch.ones(3, device="cuda")), ValueError), (dict(x_zero_point=128), ValueError),
                   (dict(w=wf), ValueError), (dict(w=along_0), ValueError), (dict(w=with_zp), ValueError),
                   (dict(w=m.target(np.ones((3, 3, 5)), [0.5])), ValueError), (dict(x=x16, x_zero_point=3), ValueError),
                   (dict(x=xf, w=wf), ValueError), (dict(x=xf, w=wf, x_scale=None, want_acc=True), ValueError),
                   (dict(x=xf, w=tgt, x_scale=None), TypeError), (dict(x=xf, w=wf[:2], x_scale=None), TypeError),
                   (dict(x=xf, w=wf.to(torch.float64), x_scale=None), TypeError)):
    kw = dict(good)
    kw.update(bad)
    with pytest.raises(exc):
      ops.dwconv_forward(**kw)
  assert tuple(ops.dwconv_forward(x=xf, w=wf, kh=3, kw=3, stride=2, dilation=1, padding=1).shape) == (2 * 2 * 3, 4)      # (VALID as the code)
  empty = ops.dwconv_forward(first=70, count=0, **good)
  assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.float32
  out = dict(x=x8, x_zero_point=0, target=tgt, kh=3, kw=3, stride=1, dilation=1, padding="SAME", bias=None, multiplier=[1 << 30],
             shift=[0], out_zero_point=0, act_min=-128, act_max=127)
  assert tuple(ops.dwconv_output(**out).shape) == (70, 4)
  for bad, exc in ((dict(x=x16), TypeError), (dict(bias=np.zeros(4, np.int64)), TypeError), (dict(bias=np.zeros(3, np.int32)), TypeError),
                   (dict(multiplier=[1, 2]), ValueError), (dict(multiplier=[-1]), ValueError), (dict(shift=[31]), ValueError),
                   (dict(act_min=5, act_max=4), ValueError), (dict(act_max=128), ValueError), (dict(out_zero_point=-129), ValueError),
                   (dict(x_zero_point=200), ValueError), (dict(target=along_0), ValueError), (dict(count=71), ValueError),
                   (dict(multiplier=ops.qfc_multipliers([1], [0], 4, 16), shift=None), ValueError)):
    kw = dict(out)
    kw.update(bad)
    with pytest.raises(exc):
      ops.dwconv_output(**kw)
  out16 = dict(x=x16, target=tgt, kh=3, kw=3, stride=1, dilation=1, padding="SAME", bias=np.zeros(4, np.int64), multiplier=[1 << 30],
               shift=[0], act_min=-32768, act_max=32767)
  assert tuple(ops.dwconv_output_i16(**out16).shape) == (70, 4) and ops.dwconv_output_i16(**out16).dtype == torch.int16
  for bad, exc in ((dict(x=x8), TypeError), (dict(bias=np.zeros(4, np.int32)), TypeError), (dict(shift=[15]), ValueError),
                   (dict(act_min=-32769), ValueError), (dict(act_min=2, act_max=1), ValueError), (dict(first=71), ValueError)):
    kw = dict(out16)
    kw.update(bad)
    with pytest.raises(exc):
      ops.dwconv_output_i16(**kw)
  DW.check_depthwise_refusals(m.lib)


# ---------------------------------------------------------------- 6. end to end
def _zero_point(t) -> int:
  return int(t.quantization.zeroPoint[0]) if t.quantization.zeroPoint is not None and len(t.quantization.zeroPoint) else 0


def _statement(float_model, qm, samples, dw):
  """The statement of compare_layer_execution's DEPTHWISE_CONV_2D evaluated in NumPy on the WRITTEN model's own
  integers, Y in float64, with the first-order bound of the device's FP32 loops (derived as
  test_gpu_conv_execution._statement derives it): an element of a KH KW-term FP32 sum of rounded products (plus one
  addition of the bias) lies within eps = (KH KW + 3) 2^-24 (Sum |x| |w| + |b|) of the exact value; the activations are
  1-Lipschitz; so |error - ref| <= (1/n) Sum (2 |yq - y| eps + eps^2). Returns {error, bound, final_error,
  final_bound, signal, final_signal, mode, bits, tokens} (the final_* None unless the op is static)."""
  from mi355q import schema
  name, c, mult, k, strides, dil, padding, has_bias, fused = dw
  o, taps = c * mult, k[0] * k[1]
  x_name, y_name = f"{name}/x", f"{name}/y"
  fsg, sg = float_model.subgraphs[0], qm.subgraphs[0]
  op = next(op for op in sg.operators if schema.tensor_name(sg.tensors[op.outputs[0]]) == y_name)
  w64 = DW.constant(float_model, f"{name}/w")[0].astype(np.float64)
  b64 = DW.constant(float_model, f"{name}/b").astype(np.float64) if has_bias else np.zeros(o)
  x_t, y_t = sg.tensors[op.inputs[0]], sg.tensors[op.outputs[0]]
  read = sg.tensors[op.inputs[1]]
  through_dequantize = read.buffer == 0 or qm.buffers[read.buffer].data is None or not len(qm.buffers[read.buffer].data)
  w_t = next(t for t in sg.tensors if schema.tensor_name(t) == f"{name}/w")
  # the expected form: int8, per-channel scales along dimension 3 (or one scale), zero points 0
  assert int(w_t.type) == int(schema.TensorType.INT8) and list(w_t.shape) == [1, k[0], k[1], o]
  s_w = np.asarray(w_t.quantization.scale, np.float32)
  assert s_w.size in (1, o) and (s_w.size == 1 or int(w_t.quantization.quantizedDimension) == 3)
  assert w_t.quantization.zeroPoint is None or not np.any(np.asarray(w_t.quantization.zeroPoint))
  s_w = np.broadcast_to(s_w, (o,)).astype(np.float32)
  qw = np.asarray(qm.buffers[w_t.buffer].data).view(np.int8).reshape(k[0], k[1], o)
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
      assert int(b_t.type) == int(schema.TensorType.INT64 if bits == 16 else schema.TensorType.INT32)
      bias = np.asarray(qm.buffers[b_t.buffer].data).view(np.int64 if bits == 16 else np.int32)[:o]
      # the bias on the grid s_x s_w: the integers are the float bias over that grid, to the rounding
      grid = float(s_x) * s_w.astype(np.float64)
      assert np.all(np.abs(bias.astype(np.float64) - b64 / grid) <= 0.5 + 1e-3 * np.abs(b64 / grid))
    ms = [OC.quantize_multiplier(float(s_x) * float(v) / float(s_y)) for v in s_w.tolist()]
    mult_q, shift_q = [v[0] for v in ms], [v[1] for v in ms]
    lo, hi = OC.activation_range(fused, float(s_y), zp_y, bits)
  source = np.arange(o) // mult

  def exact(x64, w_):
    """float64 [N OH OW, O]: the depthwise sum over the taps inside, one array operation per tap."""
    n_img, h, w, _ = x64.shape
    oh_n, ow_n, top, left = CC.geometry(h, w, k[0], k[1], strides, dil, padding)
    y = np.zeros((n_img, oh_n, ow_n, o))
    for i in range(k[0]):
      for j in range(k[1]):
        for oh in range(oh_n):
          ih = oh * strides[0] - top + i * dil[0]
          if not 0 <= ih < h:
            continue
          for ow in range(ow_n):
            iw = ow * strides[1] - left + j * dil[1]
            if 0 <= iw < w:
              y[:, oh, ow, :] += x64[:, ih, iw, :][:, source] * w_[i, j]
    return y.reshape(-1, o)
  for sample in samples:
    x = np.asarray(sample[x_name], np.float32)
    n_img = x.shape[0]
    y64 = exact(x.astype(np.float64), w64)
    n = y64.shape[0]
    mass = exact(np.abs(x).astype(np.float64), np.abs(w64))
    eps = (taps + 3) * LC.U * mass
    if mode == "weight_only":
      deq = (qw.astype(np.float32) * s_w[None, None, :]).astype(np.float32)
      yq = exact(x.astype(np.float64), deq.astype(np.float64))
      eps = eps + (taps + 3) * LC.U * exact(np.abs(x).astype(np.float64), np.abs(deq).astype(np.float64))      # (two FP32 loops)
    elif mode == "dynamic":
      q, scale = EC.quantize_rows(x.reshape(n_img, -1))
      xq = q.reshape(x.shape)
      yq = DW.rescale_i8(DW.direct_depthwise(xq, 0, qw, mult, strides, dil, padding), scale, s_w, n_img).astype(np.float64)
    elif bits == 16:
      xq = EC16.quantize_static16(x, s_x)
      yq = DW.rescale_i16(DW.direct_depthwise(xq, 0, qw, mult, strides, dil, padding), [s_x], s_w, n_img).astype(np.float64)
    else:
      xq = EC.quantize_static(x, s_x, zp_x)
      yq = DW.rescale_i8(DW.direct_depthwise(xq, zp_x, qw, mult, strides, dil, padding), [s_x], s_w, n_img).astype(np.float64)
    diff = yq - y64
    out["error"] += (diff ** 2).sum()
    out["bound"] += (2.0 * np.abs(diff) * eps + eps ** 2).sum()
    out["signal"] += (y64 ** 2).sum()
    if mode == "static":
      acc = DW.direct_depthwise(xq, zp_x if bits == 8 else 0, qw, mult, strides, dil, padding)
      if bits == 16:
        q_out = DW.epilogue_i16(acc, bias, mult_q, shift_q, lo, hi)
      else:
        q_out = DW.epilogue_i8(acc, bias, mult_q, shift_q, zp_y, lo, hi)
      yf = ((q_out.astype(np.int32) - zp_y).astype(np.float32) * s_y).astype(np.float64)
      ya = OC.float_activation(y64 + b64, fused)
      eps_f = (taps + 3) * LC.U * (mass + np.abs(b64))
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
KEYWORDS = dict(depthwise_conv_2d=True, int16_activations=True, quantized_outputs=True)


@pytest.fixture(scope="module", params=RECIPES)
def chain(m, request):
  from mi355q import quantizer, recipe
  from mi355q.utils import tfl_flatbuffer_utils
  model = DW.build_model()
  samples = DW.build_samples(model)
  qz = quantizer.Quantizer(model, getattr(recipe, request.param)())
  if request.param.startswith("static"):
    res = qz.quantize(qz.calibrate({"serving_default": samples}))
  else:
    res = qz.quantize()
  return dict(recipe=request.param, float=model, samples=samples, qz=qz,
              model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)),
              cmp=qz.validate_layer_execution({"serving_default": samples}, **KEYWORDS))


def test_every_depthwise_op_of_the_hand_built_model_matches_the_statement(chain):
  cmp_ = chain["cmp"]
  mode, bits = EXPECT[chain["recipe"]]
  assert cmp_.skipped == {} and list(cmp_) == ["fc/y"] + [f"{d[0]}/y" for d in DW.DWS]
  assert cmp_["fc/y"]["op"] == "FULLY_CONNECTED" and cmp_["fc/y"]["mode"] == mode and cmp_["fc/y"]["tokens"] == 7 * DW.SAMPLES
  for dw in DW.DWS:
    name, c, mult, k, s, dil, padding, has_bias, fused = dw
    o = c * mult
    r = cmp_[f"{name}/y"]
    ref = _statement(chain["float"], chain["model"], chain["samples"], dw)
    oh, ow, _, _ = CC.geometry(DW.HEIGHT, DW.WIDTH, k[0], k[1], s, dil, padding)
    line = f"{chain['recipe']} {name}: error {r['error']:.6e} SNR {r['output_snr']:.1f} |error - ref| / bound {abs(r['error'] - ref['error']) / ref['bound']:.3e}"
    assert (r["op"], r["mode"], r["activation_bits"], r["output_bits"]) == ("DEPTHWISE_CONV_2D", mode, bits, bits)
    assert (ref["mode"], ref["bits"]) == (mode, bits)
    assert (r["weight"], r["input"], r["rows"], r["d"], r["depth_multiplier"]) == (f"{name}/w", f"{name}/x", o, k[0] * k[1], mult)
    assert r["tokens"] == ref["tokens"] == DW.SAMPLES * DW.BATCH * oh * ow
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


def test_the_device_kernels_give_the_numpy_kernels_figures_on_the_hand_quantized_model(m):
  """compare_layer_execution on the hand-quantized models of the host tests, device kernels against NumPy kernels: the
  integer sides are bit-equal, so the figures differ by the float64 summation order alone."""
  from mi355q import model_validator as mv
  ref = DW.build_model()
  samples = DW.build_samples(ref)
  for mode, bits in (("static", 8), ("static", 16), ("dynamic", 8), ("weight_only", 8)):
    tgt = DW.quantize_by_hand(ref, samples, mode, bits)
    got = mv.compare_layer_execution(ref, tgt, samples, **KEYWORDS)
    want = mv.compare_layer_execution(ref, tgt, samples, kernels=DW.numpy_kernels()(), **KEYWORDS)
    assert got.skipped == want.skipped == {} and list(got) == list(want)
    for dw in DW.DWS:
      a, b = got[f"{dw[0]}/y"], want[f"{dw[0]}/y"]
      assert sorted(a) == sorted(b) and (a["mode"], a["tokens"], a["depth_multiplier"]) == (b["mode"], b["tokens"], b["depth_multiplier"])
      keys = ["error", "signal"] + (["final_error", "final_signal"] if mode == "static" else [])
      np.testing.assert_allclose([a[k] for k in keys], [b[k] for k in keys], rtol=1e-12)
      np.testing.assert_allclose(a["per_channel_error"], b["per_channel_error"], rtol=1e-12)
