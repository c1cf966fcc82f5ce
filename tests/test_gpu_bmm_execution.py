"""The integer BATCH_MATMUL product on the GPU (csrc/qbmm.hip, ops.qbmm_forward / qbmm_output). The validators do
not stand between the kernels and items 1 - 5; item 6 goes through compare_layer_execution and the Quantizer.

  1. acc_out bit for bit against the statement of tests/bmm_execution_cases.py on every case of its list (all four
     layouts, both batch forms, tile, wave and workgroup edges, both routes, both sum paths) and at K = 32768, and the
     library's own answer about the route of every case against the restated dispatch;
  2. y_out and q_out bit for bit: both scale counts, per-row a_scale, multipliers on both sides of shift 0, rint ties
     at the clamp bounds, 0 / inf / NaN scales;
  3. guards: sentinel bytes around every output and the workspace;
  4. every refusal and its status, nothing written;
  5. the transposing MFMA route and the generic route on the same inputs;
  6. end to end: the hand-built models through the Quantizer under three recipes, and the device kernels against the
     NumPy stand-in on the hand-quantized models.
"""
import os
import sys

import numpy as np
import pytest

import bmm_execution_cases as BC
import layer_execution_cases as EC
import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

OK, BAD_ARG, BAD_SHAPE, UNSUPPORTED = 0, -1, -2, -3


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


def _operands(m, case, a, b):
  return (m.misaligned(a) if case.a_misaligned else m.dev(a)), (m.misaligned(b) if case.b_misaligned else m.dev(b))


# ---------------------------------------------------------------- 1. the accumulators
@pytest.mark.parametrize("adj_x,adj_y", BC.LAYOUTS)
def test_accumulators_on_every_case_of_the_list(m, adj_x, adj_y):
  one = m.dev(np.ones(1, np.float32))
  cases = [c for c in BC.cases() if (c.adj_x, c.adj_y) == (adj_x, adj_y)]
  assert len(cases) > 40
  for i, c in enumerate(cases):
    a, b = c.build(100 + i)
    ad, bd = _operands(m, c, a, b)
    took = m.lib.mi355q_qbmm_mfma_route(m.rt.ptr(ad), c.m, c.k, int(adj_x), m.rt.ptr(bd), c.n, int(adj_y))
    assert took == int(c.route[0] == "mfma"), c.id
    _, acc = m.ops.qbmm_forward(ad, bd, adj_x=adj_x, adj_y=adj_y, a_scale=one, a_zero_point=c.za, b_scale=one,
                                b_zero_point=c.zb, want_acc=True)
    want = BC.accumulators(a, b, adj_x, adj_y, c.za, c.zb)
    got = acc.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, c.id
    assert np.array_equal(got, want), (c.id, np.argwhere(got != want)[:4])


def test_accumulator_at_the_bound_of_int32(m):
  """K = 32768 with every term 255 * 255: 2 130 739 200, on the MFMA route (sums in int32, the combination in wrapping uint32, three of whose terms pass 2^31)
  and, one base off, on the generic route."""
  c = BC.EXTREME
  sa, sb = c.shapes()
  a, b = np.full(sa, -128, np.int8), np.full(sb, -128, np.int8)
  one = m.dev(np.ones(1, np.float32))
  for ad in (m.dev(a), m.misaligned(a)):
    _, acc = m.ops.qbmm_forward(ad, m.dev(b), adj_x=c.adj_x, adj_y=c.adj_y, a_scale=one, a_zero_point=c.za, b_scale=one,
                                b_zero_point=c.zb, want_acc=True)
    got = acc.cpu().numpy()
    assert got.shape == (1, 16, 16) and (got == BC.EXTREME_ACC).all() and BC.EXTREME_ACC < 2 ** 31


# ---------------------------------------------------------------- 2. the rescale and the stored output
def _tables(rng, n, per_channel, real):
  ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-1, 1))) * real) for _ in range(n if per_channel else 1)]
  return [v[0] for v in ms], [v[1] for v in ms]


@pytest.mark.parametrize("adj_x,adj_y", BC.LAYOUTS)
def test_rescale_and_stored_output_bit_for_bit(m, adj_x, adj_y):
  """Both routes (K = 128 and 65), both scale counts on either side with per-row a_scale, multipliers above and
  below one (shifts on both sides of 0), per tensor and per channel."""
  i = 0
  for k in (128, 65):
    for batch, b_batch in ((1, 1), (3, 3), (3, 1)):
      for a_rows, b_chan, real in ((False, False, 3e-5), (True, True, 2.5), (True, False, 0.7), (False, True, 1.3e-3)):
        c = BC.Case(batch, b_batch, 32, 48, k, adj_x, adj_y, *BC.ZERO_POINTS[i % 4])
        rng = np.random.default_rng(500 + i)
        a, b = c.build(600 + i)
        sa = (np.exp(rng.normal(size=batch * c.m if a_rows else 1)) * 0.013).astype(np.float32)
        sb = (np.exp(rng.normal(size=c.n if b_chan else 1)) * 0.0071).astype(np.float32)
        acc = BC.accumulators(a, b, adj_x, adj_y, c.za, c.zb)
        y = m.ops.qbmm_forward(m.dev(a), m.dev(b), adj_x=adj_x, adj_y=adj_y, a_scale=m.dev(sa), a_zero_point=c.za,
                               b_scale=m.dev(sb), b_zero_point=c.zb)
        assert EC.same_bits(y.cpu().numpy(), BC.rescale(acc, sa, sb)), (c.id, a_rows, b_chan)
        # (full-range products reach 2^22 K: a real multiplier of `real` / 2^20 spreads them over and beyond int8)
        mult, shift = _tables(rng, c.n, b_chan, real / (1 << 14))
        zp_y = int(rng.integers(-128, 127, endpoint=True))
        q = m.ops.qbmm_output(m.dev(a), m.dev(b), adj_x=adj_x, adj_y=adj_y, a_zero_point=c.za, b_zero_point=c.zb,
                              multiplier=mult, shift=shift, out_zero_point=zp_y)
        assert q.dtype == m.torch.int8 and np.array_equal(q.cpu().numpy(), BC.output(acc, mult, shift, zp_y)), (c.id, real)
        mult, shift = _tables(rng, c.n, b_chan, real * 4.0)      # left shifts: sat32 before the multiplier
        assert max(shift) > 0 or real < 0.3
        q = m.ops.qbmm_output(m.dev(a), m.dev(b), adj_x=adj_x, adj_y=adj_y, a_zero_point=c.za, b_zero_point=c.zb,
                              multiplier=mult, shift=shift, out_zero_point=zp_y)
        assert np.array_equal(q.cpu().numpy(), BC.output(acc, mult, shift, zp_y)), (c.id, real, "left")
        i += 1


def test_ties_at_the_clamp_bounds_and_special_scales(m):
  """acc = a[m, 0] exactly (b's first row ones, everything else 0) under a multiplier of exactly 1/2: odd accumulators
  are rint ties, rounded away from zero, planted so that they land on and beyond both clamp bounds. Then scales of
  0, inf and NaN: the statement's bits (any NaN for a NaN)."""
  vals = np.array([53, 55, 57, -53, -55, -57, 1, -1, 3, -3, 127, -127, 0, 2, -2, -128], np.int8)
  for k, route in ((64, "mfma"), (65, "generic")):
    a = np.zeros((1, 16, k), np.int8)
    a[0, :, 0] = vals
    b = np.zeros((1, k, 16), np.int8)
    b[0, 0, :] = 1
    assert BC.route(16, 16, k, False, False, 0, 0)[0] == route
    acc = BC.accumulators(a, b, False, False, 0, 0)
    assert np.array_equal(acc[0, :, 0], vals.astype(np.int64))
    mult, shift = OC.quantize_multiplier(0.5)
    assert (mult, shift) == (1 << 30, 0)
    for zp_y in (100, 101, -100, -101, 0):
      q = m.ops.qbmm_output(m.dev(a), m.dev(b), adj_x=False, adj_y=False, a_zero_point=0, b_zero_point=0,
                            multiplier=[mult], shift=[shift], out_zero_point=zp_y).cpu().numpy()
      want = BC.output(acc, [mult], [shift], zp_y)
      assert np.array_equal(q, want), (k, zp_y)
    assert (BC.output(acc, [mult], [shift], 101) == 127).sum() >= 32       # 53 / 2 and 55 / 2 + 101: on and past 127
    assert (BC.output(acc, [mult], [shift], -101) == -128).sum() >= 32
    sa = np.array([0.0, np.inf, np.nan, -0.0, 1.0, 2.0, -np.inf, 1e-40] * 2, np.float32)
    sb = np.array([1.0, 0.0, np.inf, np.nan] * 4, np.float32)
    y = m.ops.qbmm_forward(m.dev(a), m.dev(b), adj_x=False, adj_y=False, a_scale=m.dev(sa), a_zero_point=0,
                           b_scale=m.dev(sb), b_zero_point=0).cpu().numpy()
    assert EC.same_bits(y, BC.rescale(acc, sa, sb)), k


# ---------------------------------------------------------------- 3. guards
PAD = 256


def _guarded(m, nbytes):
  """(buffer, pointer to its middle): `nbytes` of payload between two runs of PAD sentinel bytes."""
  buf = m.torch.full((nbytes + 2 * PAD,), 0xA5, dtype=m.torch.uint8, device="cuda")
  return buf, buf.data_ptr() + PAD


def _untouched(buf, nbytes):
  h = buf.cpu().numpy()
  return bool((h[:PAD] == 0xA5).all() and (h[PAD + nbytes:] == 0xA5).all())


@pytest.mark.parametrize("adj_x,adj_y", BC.LAYOUTS)
def test_nothing_is_written_outside_the_outputs_and_the_workspace(m, adj_x, adj_y):
  """Ragged tiles in M, N and the batch on the MFMA route, and the generic route: the bytes before and after y_out,
  acc_out, q_out and the workspace keep their sentinel, and the payload is the statement's."""
  for mm, nn, k in ((16, 16, 64), (144, 16, 64), (16, 144, 128), (17, 15, 65)):
    c = BC.Case(3, 3, mm, nn, k, adj_x, adj_y, 5, -3)
    a, b = c.build(900 + mm + nn)
    ad, bd = m.dev(a), m.dev(b)
    count = 3 * mm * nn
    one = m.dev(np.ones(1, np.float32))
    ws_bytes = m.lib.mi355q_qbmm_workspace_bytes(3, mm, k, int(adj_x), 3, nn, int(adj_y))
    assert ws_bytes >= 4 * 3 * (mm + nn) + 3 * k * (mm * int(adj_x) + nn * int(not adj_y))
    ybuf, yp = _guarded(m, 4 * count)
    abuf, ap = _guarded(m, 4 * count)
    qbuf, qp = _guarded(m, count)
    wbuf, wp = _guarded(m, ws_bytes)
    m.ffi.check(m.lib.mi355q_qbmm_forward_i8(m.rt.ptr(ad), 3, mm, k, int(adj_x), m.rt.ptr(one), 1, c.za, m.rt.ptr(bd), 3, nn,
                                             int(adj_y), m.rt.ptr(one), 1, c.zb, yp, ap, wp, ws_bytes, m.rt.stream_ptr()))
    mult, shift = OC.quantize_multiplier(1e-4)
    tab = m.dev(np.array([mult, shift], np.int32))
    m.ffi.check(m.lib.mi355q_qbmm_output_i8(m.rt.ptr(ad), 3, mm, k, int(adj_x), c.za, m.rt.ptr(bd), 3, nn, int(adj_y), c.zb,
                                            tab.data_ptr(), tab.data_ptr() + 4, 1, 7, qp, wp, ws_bytes, m.rt.stream_ptr()))
    m.torch.cuda.synchronize()
    for buf, nbytes in ((ybuf, 4 * count), (abuf, 4 * count), (qbuf, count), (wbuf, ws_bytes)):
      assert _untouched(buf, nbytes), (c.id, nbytes)
    want = BC.accumulators(a, b, adj_x, adj_y, c.za, c.zb)
    got = abuf.cpu().numpy()[PAD:PAD + 4 * count].view(np.int32).reshape(want.shape)
    assert np.array_equal(got, want), c.id
    gq = qbuf.cpu().numpy()[PAD:PAD + count].view(np.int8).reshape(want.shape)
    assert np.array_equal(gq, BC.output(want, [mult], [shift], 7)), c.id


# ---------------------------------------------------------------- 4. refusals
def test_every_refusal_and_its_status_writes_nothing(m):
  torch, lib, rt = m.torch, m.lib, m.rt
  batch, mm, k, nn = 2, 16, 64, 16
  a = torch.zeros((batch, mm, k), dtype=torch.int8, device="cuda")
  b = torch.zeros((batch, k, nn), dtype=torch.int8, device="cuda")
  s = torch.ones(batch * mm, dtype=torch.float32, device="cuda")
  tab = torch.ones(2 * nn, dtype=torch.int32, device="cuda")
  y = torch.full((batch, mm, nn), 7.0, dtype=torch.float32, device="cuda")
  acc = torch.full((batch, mm, nn), 7, dtype=torch.int32, device="cuda")
  q = torch.full((batch, mm, nn), 7, dtype=torch.int8, device="cuda")
  ws_bytes = lib.mi355q_qbmm_workspace_bytes(batch, mm, k, 0, batch, nn, 1)
  ws = torch.full((ws_bytes,), 7, dtype=torch.uint8, device="cuda")
  P = rt.ptr

  def fwd(**kw):
    g = dict(a=P(a), batch=batch, M=mm, K=k, adj_x=0, a_scale=P(s), a_count=1, za=0, b=P(b), b_batch=batch, N=nn, adj_y=0,
             b_scale=P(s), b_count=1, zb=0, y=P(y), acc=P(acc), ws=P(ws), ws_bytes=ws_bytes)
    g.update(kw)
    return lib.mi355q_qbmm_forward_i8(g["a"], g["batch"], g["M"], g["K"], g["adj_x"], g["a_scale"], g["a_count"], g["za"],
                                      g["b"], g["b_batch"], g["N"], g["adj_y"], g["b_scale"], g["b_count"], g["zb"], g["y"],
                                      g["acc"], g["ws"], g["ws_bytes"], rt.stream_ptr())

  def out(**kw):
    g = dict(a=P(a), batch=batch, M=mm, K=k, adj_x=0, za=0, b=P(b), b_batch=batch, N=nn, adj_y=0, zb=0, mult=P(tab),
             shift=tab.data_ptr() + 4 * nn, mcount=1, zp_y=0, q=P(q), ws=P(ws), ws_bytes=ws_bytes)
    g.update(kw)
    return lib.mi355q_qbmm_output_i8(g["a"], g["batch"], g["M"], g["K"], g["adj_x"], g["za"], g["b"], g["b_batch"], g["N"],
                                     g["adj_y"], g["zb"], g["mult"], g["shift"], g["mcount"], g["zp_y"], g["q"], g["ws"],
                                     g["ws_bytes"], rt.stream_ptr())

  both = [(dict(batch=-1), BAD_ARG), (dict(M=-1), BAD_ARG), (dict(K=-1), BAD_ARG), (dict(N=-1), BAD_ARG),
          (dict(b_batch=-1), BAD_ARG), (dict(a=None), BAD_ARG), (dict(b=None), BAD_ARG), (dict(za=128), BAD_ARG),
          (dict(za=-129), BAD_ARG), (dict(zb=128), BAD_ARG), (dict(zb=-129), BAD_ARG), (dict(b_batch=3), BAD_SHAPE),
          (dict(b_batch=0), BAD_SHAPE), (dict(K=32769), UNSUPPORTED), (dict(za=1, ws=None), BAD_ARG),
          (dict(zb=1, ws_bytes=ws_bytes - 1), BAD_ARG), (dict(za=1, ws=ws.data_ptr() + 2, ws_bytes=ws_bytes - 2), BAD_ARG)]
  only_fwd = [(dict(a_scale=None), BAD_ARG), (dict(b_scale=None), BAD_ARG), (dict(y=None), BAD_ARG),
              (dict(a_count=2), BAD_ARG), (dict(a_count=mm), BAD_ARG), (dict(b_count=2), BAD_ARG), (dict(b_count=0), BAD_ARG)]
  only_out = [(dict(mult=None), BAD_ARG), (dict(shift=None), BAD_ARG), (dict(q=None), BAD_ARG), (dict(mcount=2), BAD_ARG),
              (dict(mcount=0), BAD_ARG), (dict(zp_y=128), BAD_ARG), (dict(zp_y=-129), BAD_ARG)]
  for kw, status in both + only_fwd:
    assert fwd(**kw) == status, kw
    assert lib.mi355q_last_error(), kw
  for kw, status in both + only_out:
    assert out(**kw) == status, kw
  # after the refusals an empty request enqueues nothing, whatever K is; a null workspace is fine without zero points
  for kw in (dict(batch=0, b_batch=0), dict(M=0), dict(N=0), dict(M=0, K=0)):
    assert fwd(**kw) == OK and out(**kw) == OK, kw
  torch.cuda.synchronize()
  assert bool((y == 7.0).all()) and bool((acc == 7).all()) and bool((q == 7).all()) and bool((ws == 7).all())
  assert lib.mi355q_qbmm_workspace_bytes(0, mm, k, 0, 1, nn, 1) == 0
  # a K-strided operand on the MFMA route needs the workspace for its transposed copy, at a 16-byte aligned address
  full = lib.mi355q_qbmm_workspace_bytes(batch, mm, k, 0, batch, nn, 0)
  assert full >= ws_bytes + batch * k * nn
  big = torch.full((full + 16,), 7, dtype=torch.uint8, device="cuda")
  for kw in (dict(ws=None, ws_bytes=0), dict(ws_bytes=full - 1), dict(ws=big.data_ptr() + 1, ws_bytes=full)):
    assert fwd(**kw) == BAD_ARG and out(**kw) == BAD_ARG, kw
  assert fwd(za=1, adj_y=1, ws=big.data_ptr() + 2, ws_bytes=full) == BAD_ARG and b"4-byte aligned" in lib.mi355q_last_error()
  assert out(zb=1, adj_y=1, ws=big.data_ptr() + 2, ws_bytes=full) == BAD_ARG and b"4-byte aligned" in lib.mi355q_last_error()
  torch.cuda.synchronize()
  assert bool((y == 7.0).all()) and bool((acc == 7).all()) and bool((q == 7).all()) and bool((big == 7).all())
  # with both operands contiguous along K and no zero point the workspace may be NULL (b read as [batch, N, K])
  assert fwd(adj_y=1, ws=None, ws_bytes=0) == OK and out(adj_y=1, ws=None, ws_bytes=0) == OK
  torch.cuda.synchronize()
  assert bool((y == 0.0).all()) and bool((acc == 0).all()) and bool((q == 0).all()) and bool((ws == 7).all())
  # K = 0 is the empty sum: acc = 0 on the generic route, in every layout
  for layout in BC.LAYOUTS:
    y.fill_(7.0), acc.fill_(7), q.fill_(7)
    assert fwd(K=0, adj_x=int(layout[0]), adj_y=int(layout[1])) == OK and out(K=0, zp_y=-9, adj_x=int(layout[0]), adj_y=int(layout[1])) == OK
    torch.cuda.synchronize()
    assert bool((y == 0.0).all()) and bool((acc == 0).all()) and bool((q == -9).all())


def test_ops_wrapper_checks(m):
  torch, ops = m.torch, m.ops
  a = torch.zeros((2, 16, 64), dtype=torch.int8, device="cuda")
  b = torch.zeros((2, 64, 16), dtype=torch.int8, device="cuda")
  one = torch.ones(1, dtype=torch.float32, device="cuda")
  kw = dict(adj_x=False, adj_y=False, a_scale=one, a_zero_point=0, b_scale=one, b_zero_point=0)
  assert ops.qbmm_forward(a, b, **kw).shape == (2, 16, 16)
  assert ops.qbmm_forward(a.view(1, 2, 16, 64), b.view(1, 2, 64, 16), **kw).shape == (1, 2, 16, 16)
  assert ops.qbmm_forward(a, b[0], **kw).shape == (2, 16, 16)                      # a right-hand batch product of 1
  assert ops.qbmm_forward(a[0], b[0], **kw).shape == (16, 16)
  with pytest.raises(TypeError):
    ops.qbmm_forward(a.float(), b, **kw)
  with pytest.raises(TypeError):
    ops.qbmm_forward(a[0, 0], b, **kw)
  with pytest.raises(ValueError, match="disagree on K"):
    ops.qbmm_forward(a, b, **dict(kw, adj_y=True))
  with pytest.raises(ValueError, match="broadcasting"):
    ops.qbmm_forward(a, torch.zeros((3, 64, 16), dtype=torch.int8, device="cuda"), **kw)
  with pytest.raises(ValueError, match="exceeds"):
    ops.qbmm_forward(torch.zeros((1, 32769), dtype=torch.int8, device="cuda"),
                     torch.zeros((32769, 1), dtype=torch.int8, device="cuda"), **kw)
  with pytest.raises(ValueError, match="outside int8"):
    ops.qbmm_forward(a, b, **dict(kw, a_zero_point=128))
  with pytest.raises(ValueError, match="a_scale"):
    ops.qbmm_forward(a, b, **dict(kw, a_scale=torch.ones(16, dtype=torch.float32, device="cuda")))
  with pytest.raises(ValueError, match="b_scale"):
    ops.qbmm_forward(a, b, **dict(kw, b_scale=torch.ones(2, dtype=torch.float32, device="cuda")))
  okw = dict(adj_x=False, adj_y=False, a_zero_point=0, b_zero_point=0, multiplier=[1 << 30], shift=[0], out_zero_point=0)
  assert ops.qbmm_output(a, b, **okw).shape == (2, 16, 16)
  with pytest.raises(ValueError):
    ops.qbmm_output(a, b, **dict(okw, multiplier=[1, 2], shift=[0, 0]))
  with pytest.raises(ValueError, match="outside int8"):
    ops.qbmm_output(a, b, **dict(okw, out_zero_point=-129))


# ---------------------------------------------------------------- 5. the transposing route against the generic route
@pytest.mark.parametrize("adj_x,adj_y", [lay for lay in BC.LAYOUTS if lay != (False, True)])
def test_the_transposing_and_the_generic_route_agree_on_the_same_inputs(m, adj_x, adj_y):
  """The same values at an aligned base (MFMA route behind the transposing pre-pass) and one element off (generic route): equal bits in acc, y
  and q, over more than one workgroup and K step and with a ragged last tile."""
  c = BC.Case(3, 3, 144, 272, 320, adj_x, adj_y, -7, 9)
  assert c.route[0] == "mfma" and "transposed" in "".join(c.route)
  a, b = c.build(77)
  rng = np.random.default_rng(78)
  sa = m.dev((np.exp(rng.normal(size=3 * c.m)) * 0.01).astype(np.float32))
  sb = m.dev((np.exp(rng.normal(size=c.n)) * 0.01).astype(np.float32))
  mult, shift = _tables(rng, c.n, True, 1e-4)
  res = []
  for ad, bd in ((m.dev(a), m.dev(b)), (m.misaligned(a), m.dev(b)), (m.dev(a), m.misaligned(b))):
    y, acc = m.ops.qbmm_forward(ad, bd, adj_x=adj_x, adj_y=adj_y, a_scale=sa, a_zero_point=c.za, b_scale=sb,
                                b_zero_point=c.zb, want_acc=True)
    q = m.ops.qbmm_output(ad, bd, adj_x=adj_x, adj_y=adj_y, a_zero_point=c.za, b_zero_point=c.zb, multiplier=mult,
                          shift=shift, out_zero_point=-5)
    res.append((y.cpu().numpy(), acc.cpu().numpy(), q.cpu().numpy()))
  assert np.array_equal(res[0][1], BC.accumulators(a, b, adj_x, adj_y, c.za, c.zb))
  for other in res[1:]:
    assert np.array_equal(res[0][0].view(np.uint32), other[0].view(np.uint32))
    assert np.array_equal(res[0][1], other[1]) and np.array_equal(res[0][2], other[2])


# ---------------------------------------------------------------- 6. end to end: the hand-built models through the Quantizer
U = 2.0 ** -24


def _zero_point(t) -> int:
  return int(t.quantization.zeroPoint[0]) if t.quantization.zeroPoint is not None and len(t.quantization.zeroPoint) else 0


def _statement(float_model, qm, samples, op):
  """The statement of compare_layer_execution's BATCH_MATMUL evaluated in NumPy on the WRITTEN model's own integers, Y
  in float64, with the first-order bound tests/test_gpu_conv_execution.py derives for the same quantities: an element
  of a K-term FP32 sum of rounded products lies within eps = (K + 3) 2^-24 Sum |a| |b| of the exact value (there is no
  bias), so |error - ref| <= (1/n) Sum (2 |yq - y| eps + eps^2); the weight-only product is two such sums. Returns
  {mode, operands, tokens, signal, error, bound, final_error, final_bound} (the final_* None unless static)."""
  from mi355q import schema
  name, a_shape, b_shape, adj_x, adj_y, constant = op
  sg = qm.subgraphs[0]
  bmm = next(o for o in sg.operators if schema.tensor_name(sg.tensors[o.outputs[0]]) == f"{name}/y")
  a_t, y_t, read = sg.tensors[bmm.inputs[0]], sg.tensors[bmm.outputs[0]], sg.tensors[bmm.inputs[1]]
  k = a_shape[-2] if adj_x else a_shape[-1]
  n = BC.out_shape(a_shape, b_shape, adj_x, adj_y)[-1]
  static = int(a_t.type) == int(schema.TensorType.INT8)
  if constant:
    b_t = next(t for t in sg.tensors if schema.tensor_name(t) == f"{name}/b")
    through_dequantize = read is not b_t
    # the expected form: int8, one scale or one per output channel along the output axis, zero points 0
    assert int(b_t.type) == int(schema.TensorType.INT8) and list(b_t.shape) == list(b_shape)
    s_b = np.asarray(b_t.quantization.scale, np.float32)
    axis = len(b_shape) - 2 if adj_y else len(b_shape) - 1
    assert s_b.size in (1, n) and (s_b.size == 1 or int(b_t.quantization.quantizedDimension) == axis)
    assert b_t.quantization.zeroPoint is None or not np.any(np.asarray(b_t.quantization.zeroPoint))
    ints = np.asarray(qm.buffers[b_t.buffer].data).view(np.int8).reshape(b_shape)
    mode = "static" if static else ("weight_only" if through_dequantize else "dynamic")
    zb = 0
  else:
    b_t = read
    assert static and int(b_t.type) == int(schema.TensorType.INT8)
    s_b, zb, mode = np.asarray(b_t.quantization.scale, np.float32), _zero_point(b_t), "static"
  out = dict(mode=mode, operands="constant" if constant else "activations", tokens=0, signal=0.0, error=0.0, bound=0.0,
             final_error=None, final_bound=None)
  if mode == "static":
    out.update(final_error=0.0, final_bound=0.0)
    s_a, za, s_y, zp_y = np.float32(a_t.quantization.scale[0]), _zero_point(a_t), np.float32(y_t.quantization.scale[0]), _zero_point(y_t)
    assert int(y_t.type) == int(schema.TensorType.INT8)
    tables = [OC.quantize_multiplier(float(s_a) * float(v) / float(s_y)) for v in s_b.tolist()]

  def exact(a, b):
    a3, b3 = a.reshape((-1,) + a.shape[-2:]).astype(np.float64), b.reshape((-1,) + b.shape[-2:]).astype(np.float64)
    a3 = a3.swapaxes(1, 2) if adj_x else a3
    b3 = b3.swapaxes(1, 2) if adj_y else b3
    return np.einsum("bmk,bkn->bmn", a3, np.broadcast_to(b3, (a3.shape[0],) + b3.shape[1:]))
  for s in samples:
    a = np.asarray(s[f"{name}/a"], np.float32)
    b = BC.constant(float_model, f"{name}/b") if constant else np.asarray(s[f"{name}/b"], np.float32)
    y64 = exact(a, b)
    batch, m = y64.shape[0], y64.shape[1]
    eps = (k + 3) * U * exact(np.abs(a), np.abs(b))
    if mode == "weight_only":
      shape = [-1 if (i == axis and s_b.size > 1) else 1 for i in range(len(b_shape))]
      deq = (ints.astype(np.float32) * s_b.reshape(shape)).astype(np.float32)
      yq = exact(a, deq)
      eps = eps + (k + 3) * U * exact(np.abs(a), np.abs(deq))
    elif mode == "dynamic":
      q, scale = EC.quantize_rows(a.reshape(batch * m, -1))
      yq = BC.rescale(BC.accumulators(q.reshape(batch, m, -1), ints, adj_x, adj_y, 0, 0), scale, s_b).astype(np.float64)
    else:
      aq = EC.quantize_static(a, s_a, za)
      bq = ints if constant else EC.quantize_static(b, s_b[0], zb)
      acc = BC.accumulators(aq, bq, adj_x, adj_y, za, zb)
      yq = BC.rescale(acc, [s_a], s_b).astype(np.float64)
      q_out = BC.output(acc, [t[0] for t in tables], [t[1] for t in tables], zp_y)
      yf = ((q_out.astype(np.int32) - zp_y).astype(np.float32) * s_y).astype(np.float64)
      out["final_error"] += ((yf - y64) ** 2).sum()
      out["final_bound"] += (2.0 * np.abs(yf - y64) * eps + eps ** 2).sum()
    diff = yq - y64
    out["error"] += (diff ** 2).sum()
    out["bound"] += (2.0 * np.abs(diff) * eps + eps ** 2).sum()
    out["signal"] += (y64 ** 2).sum()
    out["tokens"] += batch * m
  for key in ("error", "bound", "signal", "final_error", "final_bound"):
    if out[key] is not None:
      out[key] /= out["tokens"]
  return out


RECIPES = ("static_wi8_ai8", "dynamic_wi8_afp32", "weight_only_wi8_afp32")
EXPECT = {"static_wi8_ai8": "static", "dynamic_wi8_afp32": "dynamic", "weight_only_wi8_afp32": "weight_only"}
KEYWORDS = dict(batch_matmul=True, quantized_outputs=True)
E2E_MODELS = {"constant": (BC.build_constant_model, BC.CONSTANT_OPS), "attention": (BC.build_attention_model, BC.ATTENTION_OPS)}


@pytest.fixture(scope="module", params=[(r, w) for r in RECIPES for w in E2E_MODELS])
def chain(m, request):
  from mi355q import quantizer, recipe
  from mi355q.utils import tfl_flatbuffer_utils
  recipe_name, which = request.param
  build, ops_list = E2E_MODELS[which]
  model = build()
  samples = BC.build_samples(model, ops_list)
  qz = quantizer.Quantizer(model, getattr(recipe, recipe_name)())
  if recipe_name.startswith("static"):
    res = qz.quantize(qz.calibrate({"serving_default": samples}))
  else:
    res = qz.quantize()
  return dict(recipe=recipe_name, which=which, ops=ops_list, float=model, samples=samples,
              model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)),
              cmp=qz.validate_layer_execution({"serving_default": samples}, **KEYWORDS),
              plain=qz.validate_layer_execution({"serving_default": samples}))


def test_the_hand_built_models_through_the_quantizer_match_the_statement(chain, m):
  """Modes and `operands` as the table of the docstring says; the figures within the bound derived in _statement. A
  product of two activations has no weight: under the dynamic and weight-only recipes it stays a float op and is
  skipped as one."""
  cmp_, mode = chain["cmp"], EXPECT[chain["recipe"]]
  print(chain["recipe"], chain["which"], "skipped:", cmp_.skipped)
  assert list(chain["plain"].results) == ["fc/y"] and "op" not in chain["plain"].results["fc/y"]
  assert not [k for k in chain["plain"].skipped if k != "fc/y"]
  assert cmp_.results["fc/y"]["op"] == "FULLY_CONNECTED"
  for op in chain["ops"]:
    name, a_shape, b_shape, adj_x, adj_y, constant = op
    y_name = f"{name}/y"
    if not constant and mode != "static":
      from mi355q import model_validator as mv
      assert cmp_.skipped[y_name] == mv.SKIP_BMM_FLOAT
      continue
    if mode == "dynamic" and adj_x:
      from mi355q import model_validator as mv
      assert cmp_.skipped[y_name] == mv.SKIP_BMM_DYNAMIC_ADJ_X
      continue
    assert y_name in cmp_.results, (y_name, cmp_.skipped)
    r = cmp_.results[y_name]
    ref = _statement(chain["float"], chain["model"], chain["samples"], op)
    line = (f"{chain['recipe']} {name}: error {r['error']:.6e} SNR {r['output_snr']:.1f} |error - ref| / bound "
            f"{abs(r['error'] - ref['error']) / ref['bound']:.3e}")
    assert (r["op"], r["operands"], r["mode"]) == ("BATCH_MATMUL", ref["operands"], mode) and ref["mode"] == mode
    assert (r["adj_x"], r["adj_y"], r["batch"]) == (adj_x, adj_y, int(np.prod(a_shape[:-2])))
    assert r["tokens"] == ref["tokens"] and r["rows"] == BC.out_shape(a_shape, b_shape, adj_x, adj_y)[-1]
    assert r["d"] == (a_shape[-2] if adj_x else a_shape[-1])
    if mode == "static":
      line += (f"; final error {r['final_error']:.6e} |final_error - ref| / bound "
               f"{abs(r['final_error'] - ref['final_error']) / ref['final_bound']:.3e}")
    print(line)
    assert abs(r["error"] - ref["error"]) <= ref["bound"]
    np.testing.assert_allclose(r["signal"], ref["signal"], rtol=1e-5)
    np.testing.assert_allclose(r["error"], float(np.sum(r["per_channel_error"])), rtol=1e-12)
    assert 0 < r["error"] < 1e-2 * r["signal"]
    if mode == "static":
      assert "final_skipped" not in r and r["activation_bits"] == 8 and r["output_bits"] == 8
      assert abs(r["final_error"] - ref["final_error"]) <= ref["final_bound"]
    else:
      assert not [x for x in r if x.startswith("final")]


def test_the_device_kernels_give_the_numpy_kernels_figures_on_the_hand_quantized_models(m):
  """compare_layer_execution with the device kernels against the NumPy stand-in on the hand-quantized models: the
  integer parts are bit-equal, so the figures differ only by the float32 products' rounding (the bound above)."""
  from mi355q import model_validator as mv
  for which, (build, ops_list) in E2E_MODELS.items():
    model = build()
    samples = BC.build_samples(model, ops_list)
    for mode in (("static", "dynamic", "weight_only") if which == "constant" else ("static",)):
      tgt = BC.quantize_by_hand(model, samples, ops_list, mode)
      got = mv.compare_layer_execution(model, tgt, samples, **KEYWORDS)
      want = mv.compare_layer_execution(model, tgt, samples, kernels=BC.numpy_kernels()(), **KEYWORDS)
      assert got.skipped == want.skipped and list(got.results) == list(want.results)
      for op in ops_list:
        y_name = f"{op[0]}/y"
        if y_name not in want.results:
          continue
        ref = _statement(model, tgt, samples, op)
        for key in ("error",) + (("final_error",) if mode == "static" else ()):
          assert abs(got.results[y_name][key] - want.results[y_name][key]) <= 2 * ref["bound" if key == "error" else "final_bound"], (which, mode, y_name, key)
        assert {k: v for k, v in got.results[y_name].items() if not isinstance(v, (float, np.ndarray))} == {
            k: v for k, v in want.results[y_name].items() if not isinstance(v, (float, np.ndarray))}
