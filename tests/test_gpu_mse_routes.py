"""Every route of the MSE scale kernels (mi355q_mse_scale_f32, mi355q_mse_scale_nd_f32, mi355q_mse_requant_f32;
csrc/mse_scale.hip), bit for bit against the reference's NumPy expressions.

The cases, their expected values, the restatement of the host's choice of kernels and the proof that each case shows
the defects its route could have are in mse_route_cases.py / test_mse_route_cases_host.py, which need no GPU. Here the
scale entries run through the wrappers of ops.py (nothing else calls ops.mse_scale) and the fused entry through the
wrapper and through the C ABI, where x and q_out can sit one float and one byte past aligned addresses and every output
lies between guard bytes that must come back untouched: the fused kernel stores whole 32-bit words of four int8.
float32 scales are compared by their 32-bit patterns (a NaN for a NaN), integers as int8. Nothing here tolerates a
difference."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest

import mse_route_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                       # bytes in front of and behind every output (a multiple of 16)
FILL = 0x5A                      # every byte of an output before the call: float32 1.5e16, int8 90
ENV = "MI355Q_MSE_TWO_KERNELS"


@functools.lru_cache(maxsize=None)
def modules():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), ffi=_ffi)


@pytest.fixture(scope="module")
def m():
  return modules()


def dev(a):
  return modules().torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cases are read-only


class Guarded:
  """`nbytes` bytes on the device, `offset` bytes past a 16-byte aligned address, between two runs of GUARD bytes;
  all of it pre-filled with FILL."""

  def __init__(self, nbytes, offset=0):
    torch = modules().torch
    self.nbytes, self.lo = nbytes, GUARD + offset
    self.buf = torch.full((self.lo + nbytes + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert self.buf.data_ptr() % 16 == 0
    self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.lo)

  def result(self, dtype, shape):
    host = self.buf.cpu().numpy()
    assert (host[:self.lo] == FILL).all() and (host[self.lo + self.nbytes:] == FILL).all(), "written outside the output"
    return host[self.lo:self.lo + self.nbytes].copy().view(dtype).reshape(shape)

  def untouched(self):
    return bool((self.buf.cpu().numpy() == FILL).all())


def placed(x, offset_floats=0):
  """x on the device `offset_floats` floats past a 16-byte aligned address: (keep-alive tensor, pointer)."""
  torch = modules().torch
  buf = torch.zeros((x.size + 8,), dtype=torch.float32, device="cuda")
  assert buf.data_ptr() % 16 == 0
  buf[offset_floats:offset_floats + x.size] = torch.from_numpy(np.array(x, order="C").reshape(-1)).cuda()
  return buf, ctypes.c_void_p(buf.data_ptr() + 4 * offset_floats)


def requant_abi(m, x, bits, narrow, mult, x_off=0, q_off=0):
  """mi355q_mse_requant_f32 through the C ABI: (scale [units], q [units, n]), the guards checked."""
  units, n = x.shape
  keep, xptr = placed(x, x_off)
  scale, q = Guarded(4 * units), Guarded(units * n, q_off)
  m.ffi.check(m.L.mi355q_mse_requant_f32(xptr, units, n, np.float32(mult), bits, narrow, scale.ptr, q.ptr, m.rt.stream_ptr()))
  got = dict(scale=scale.result(np.float32, (units,)), q=q.result(np.int8, (units, n)))
  back = keep.cpu().numpy()[x_off:x_off + x.size]
  assert np.array_equal(back.view(np.uint32), x.reshape(-1).view(np.uint32)), "the input was written to"
  return got


def requant_wrapper(m, x, bits, narrow, mult, two_kernels):
  if two_kernels:
    os.environ[ENV] = "1"
  try:
    scale, q = m.ops.mse_requant(dev(x).reshape(-1), x.shape[0], x.shape[1], mult, bits, bool(narrow))
    return dict(scale=scale.cpu().numpy(), q=q.cpu().numpy().reshape(x.shape))
  finally:
    os.environ.pop(ENV, None)


def scales_contiguous(m, x):
  """Both multipliers through ops.mse_scale, through ops.mse_scale_nd(outer=1) and through the guarded C ABI."""
  units, n = x.shape
  xd = dev(x).reshape(-1)
  direct = {f"scale@{k}": m.ops.mse_scale(xd, units, n, k).cpu().numpy() for k in S.MULS}
  nd = {f"scale@{k}": m.ops.mse_scale_nd(xd, 1, units, n, k).cpu().numpy() for k in S.MULS}
  abi = {}
  for k in S.MULS:
    out = Guarded(4 * units)
    m.ffi.check(m.L.mi355q_mse_scale_f32(m.rt.ptr(xd), units, n, np.float32(k), out.ptr, m.rt.stream_ptr()))
    abi[f"scale@{k}"] = out.result(np.float32, (units,))
  return direct, nd, abi


def scales_nd(m, c, x):
  xd = dev(x).reshape(-1)
  got = {}
  for k in S.MULS:
    out = Guarded(4 * c.channels)
    m.ffi.check(m.L.mi355q_mse_scale_nd_f32(m.rt.ptr(xd), c.outer, c.channels, c.inner, np.float32(k), out.ptr,
                                             m.rt.stream_ptr()))
    got[f"scale@{k}"] = out.result(np.float32, (c.channels,))
  wrapped = {f"scale@{k}": m.ops.mse_scale_nd(xd, c.outer, c.channels, c.inner, k).cpu().numpy() for k in S.MULS}
  return got, wrapped


# ---------------------------------------------------------------- 1. scales on every contiguous route
@pytest.mark.parametrize("c", S.SCALE_CASES, ids=[S.case_id(c) for c in S.SCALE_CASES])
def test_scale_equals_numpy_on_every_contiguous_route(m, c):
  inputs, want = S.expected(c)
  for got in scales_contiguous(m, inputs["x"]):
    assert S.same_bits(got, want) == ""


# ---------------------------------------------------------------- 2. scales on the nd routes
@pytest.mark.parametrize("c", S.ND_CASES, ids=[S.case_id(c) for c in S.ND_CASES])
def test_scale_nd_equals_numpy(m, c):
  inputs, want = S.expected(c)
  for got in scales_nd(m, c, inputs["x"]):
    assert S.same_bits(got, want) == ""


# ---------------------------------------------------------------- 3. - 5. the fused entry, its fallbacks, its guards
ALL_REQUANT = S.REQUANT_CASES + S.BITS_CASES


@pytest.mark.parametrize("c", ALL_REQUANT, ids=[S.case_id(c) for c in ALL_REQUANT])
def test_requant_equals_numpy_and_the_two_kernel_route(m, c):
  inputs, want = S.expected(c)
  x, mult = inputs["x"], S.multiplier(c)
  got = requant_abi(m, x, c.bits, c.narrow, mult, c.x_off, c.q_off)     # scale_out and q_out between guards
  assert S.same_bits(got, want) == ""
  if c.x_off or c.q_off:
    aligned = requant_abi(m, x, c.bits, c.narrow, mult)
    assert S.same_bits(got, aligned) == ""
    return
  one = requant_wrapper(m, x, c.bits, c.narrow, mult, two_kernels=False)
  two = requant_wrapper(m, x, c.bits, c.narrow, mult, two_kernels=True)
  assert S.same_bits(one, want) == "" and S.same_bits(two, want) == "" and S.same_bits(one, two) == ""


def test_every_width_and_either_bound_at_a_single_chunk_and_a_multi_chunk_length():
  ran = {(c.n, c.bits, c.narrow) for c in ALL_REQUANT if c.kind == "wide" and not (c.x_off or c.q_off) and
         S.route("requant", c.units, c.n)[0] == ("mse_scale_balanced_kernel (fused quantize)",)}
  assert {(n, b, nw) for n in S.BITS_LENGTHS for b in range(2, 9) for nw in (0, 1)} <= ran
  assert S.BITS_LENGTHS[0] <= S.CHUNK < S.BITS_LENGTHS[1]


# ---------------------------------------------------------------- 6. non-finite and extreme inputs, kernel by kernel
@pytest.mark.parametrize("kernel", S.KERNELS)
def test_nonfinite_and_extreme_inputs(m, kernel):
  classes = set()
  cases = [c for c in S.SCALE_CASES + S.ND_CASES if c.kind in ("squares", "signs", "nonfinite") and
           S._short(S.kernels(c)[0]) == kernel]                         # pylint: disable=protected-access
  assert {c.kind for c in cases} == {"squares", "signs", "nonfinite"}
  for c in cases:
    inputs, want = S.expected(c)
    if isinstance(c, S.NdCase):
      got = scales_nd(m, c, inputs["x"])[0]
    else:
      got = scales_contiguous(m, inputs["x"])[2]
    assert S.same_bits(got, want) == "", S.case_id(c)
    s = got[f"scale@{S.MULS[0]}"]
    classes |= {"nan"} if np.isnan(s).any() else set()
    classes |= {"inf"} if np.isposinf(s).any() else set()
    classes |= {"zero"} if (s.view(np.uint32) == 0).any() else set()
  assert classes == {"nan", "inf", "zero"}


# ---------------------------------------------------------------- 7. refusals
OK, BAD_ARG, BAD_SHAPE = 0, -1, -2
NEGATIVE, EMPTY, NULL, BITS = "negative shape", "empty reduction unit", "null pointer", "bits must be in [2, 8]"


def _refusal(m, call, status, message, outputs):
  assert call() == status
  assert m.L.mi355q_last_error().decode() == message
  assert all(o.untouched() for o in outputs), "a refused call wrote"


def test_refusals_return_the_status_and_message_and_write_nothing(m):
  L, st = m.L, m.rt.stream_ptr()
  keep, x = placed(np.ones((4, 8), np.float32))
  scale, q = Guarded(64), Guarded(64)
  outs = (scale, q)
  k = np.float32(S.MULS[0])
  for units, n, status, msg in ((-1, 8, BAD_ARG, NEGATIVE), (4, -8, BAD_ARG, NEGATIVE), (4, 0, BAD_SHAPE, EMPTY),
                                (0, 8, OK, ""), (0, 0, OK, "")):
    _refusal(m, lambda: L.mi355q_mse_scale_f32(x, units, n, k, scale.ptr, st), status, msg, outs)
    _refusal(m, lambda: L.mi355q_mse_requant_f32(x, units, n, k, 4, 0, scale.ptr, q.ptr, st), status, msg, outs)
    _refusal(m, lambda: L.mi355q_mse_scale_nd_f32(x, 1, units, n, k, scale.ptr, st), status, msg, outs)
  _refusal(m, lambda: L.mi355q_mse_scale_f32(None, 4, 8, k, scale.ptr, st), BAD_ARG, NULL, outs)
  _refusal(m, lambda: L.mi355q_mse_scale_f32(x, 4, 8, k, None, st), BAD_ARG, NULL, outs)
  for outer, channels, inner, status, msg in ((-2, 3, 4, BAD_ARG, NEGATIVE), (2, -3, 4, BAD_ARG, NEGATIVE), (2, 3, -4, BAD_ARG, NEGATIVE),
                                              (2, 0, 4, OK, ""), (2, 0, 0, OK, ""), (0, 3, 4, BAD_SHAPE, EMPTY),
                                              (2, 3, 0, BAD_SHAPE, EMPTY), (0, 3, 1, BAD_SHAPE, EMPTY), (0, 1, 4, BAD_SHAPE, EMPTY),
                                              (2, 1, 0, BAD_SHAPE, EMPTY)):
    _refusal(m, lambda: L.mi355q_mse_scale_nd_f32(x, outer, channels, inner, k, scale.ptr, st), status, msg, outs)
  for outer, channels, inner in ((2, 2, 4), (2, 4, 1), (2, 1, 4)):
    _refusal(m, lambda: L.mi355q_mse_scale_nd_f32(None, outer, channels, inner, k, scale.ptr, st), BAD_ARG, NULL, outs)
    _refusal(m, lambda: L.mi355q_mse_scale_nd_f32(x, outer, channels, inner, k, None, st), BAD_ARG, NULL, outs)
  for bits in (-1, 0, 1, 9, 16):
    _refusal(m, lambda: L.mi355q_mse_requant_f32(x, 4, 8, k, bits, 0, scale.ptr, q.ptr, st), BAD_ARG, BITS, outs)
  _refusal(m, lambda: L.mi355q_mse_requant_f32(x, 0, 8, k, 9, 0, scale.ptr, q.ptr, st), BAD_ARG, BITS, outs)   # before units == 0
  _refusal(m, lambda: L.mi355q_mse_requant_f32(None, 4, 8, k, 4, 0, scale.ptr, q.ptr, st), BAD_ARG, NULL, outs)
  _refusal(m, lambda: L.mi355q_mse_requant_f32(x, 4, 8, k, 4, 0, None, q.ptr, st), BAD_ARG, NULL, outs)
  _refusal(m, lambda: L.mi355q_mse_requant_f32(x, 4, 8, k, 4, 0, scale.ptr, None, st), BAD_ARG, NULL, outs)
  m.torch.cuda.synchronize()
  assert all(o.untouched() for o in outs) and (keep.cpu().numpy()[:32] == 1.0).all()
  # and the same arguments, accepted, do write
  m.ffi.check(L.mi355q_mse_requant_f32(x, 4, 8, k, 4, 0, scale.ptr, q.ptr, st))
  assert not scale.untouched() and not q.untouched()
