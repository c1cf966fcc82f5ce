"""Every route of the Hadamard rotation kernels (mi355q_hadamard_rotate_f32, mi355q_weight_delta_transformed_f32;
csrc/hadamard.hip), bit for bit.

The cases, the restatement of the host's choice of kernel, the order in which each kernel runs its butterfly stages and
the NumPy float32 model of that arithmetic are in hadamard_route_cases.py / test_hadamard_route_cases_host.py, which
need no GPU. Impulses and dense integers have exact answers that owe nothing to the model; dense floats are held to
the model under the order of the route the call takes. Everything runs through the C ABI, where x and out can sit one
float past an aligned address (the only way to the radix-2 kernel at h >= 256) and every output lies between guard
floats that must come back untouched. One assertion per case holds the floats to a float64 butterfly inside
(L + 4) 2^-24 ||x||_2 per vector, which does not depend on the model. Nothing else here tolerates a difference."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest

import hadamard_route_cases as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                        # floats in front of and behind every output (a multiple of 4)
FILL = np.float32(-7.25)          # every guard and every output word before the call
F = np.float32


@functools.lru_cache(maxsize=None)
def modules():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  from mi355q.algorithms.uniform_quantize import hadamard_rotation
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), ffi=_ffi, had=hadamard_rotation)


@pytest.fixture(scope="module")
def m():
  return modules()


class Guarded:
  """`n` floats on the device, `offset` floats past a 16-byte aligned address, between two runs of GUARD floats; all
  of it FILL, then `values` (if any) in the n floats."""

  def __init__(self, n, offset=0, values=None):
    torch = modules().torch
    self.n, self.lo = n, GUARD + offset
    self.buf = torch.full((self.lo + n + GUARD + 4,), float(FILL), dtype=torch.float32, device="cuda")
    assert self.buf.data_ptr() % 16 == 0
    if values is not None:
      self.buf[self.lo:self.lo + n] = torch.from_numpy(np.array(values, F).reshape(-1)).cuda()
    self.address = self.buf.data_ptr() + 4 * self.lo
    self.ptr = ctypes.c_void_p(self.address)
    assert self.address % 16 == 4 * (offset % 4)

  def result(self, shape):
    host = self.buf.cpu().numpy()
    assert (host[:self.lo] == FILL).all() and (host[self.lo + self.n:] == FILL).all(), "written outside the n floats"
    return host[self.lo:self.lo + self.n].copy().reshape(shape)

  def untouched(self):
    return bool((self.buf.cpu().numpy() == FILL).all())


def rotate(m, x, h, x_off=0, out_off=0, in_place=False):
  """mi355q_hadamard_rotate_f32 on x [n_vec, h] through the C ABI; the guards and (out of place) the input checked."""
  n_vec = x.shape[0]
  src = Guarded(x.size, x_off, x)
  dst = src if in_place else Guarded(x.size, out_off)
  m.ffi.check(m.L.mi355q_hadamard_rotate_f32(src.ptr, n_vec, h, dst.ptr, m.rt.stream_ptr()))
  got = dst.result(x.shape)
  if not in_place:
    assert H.same_bits(src.result(x.shape), np.array(x, F)) == "", "the input was written to"
  return got


def rotate_case(m, c, x):
  """One call of case c on x [n_vec, h]; where x and out share an offset also in place, which must give the same bits."""
  assert x.shape == (c.n_vec, c.h)
  assert H.route(c.h, c.x_off % 4 == 0, c.out_off % 4 == 0) == c.route          # a dispatch change fails here
  got = rotate(m, x, c.h, c.x_off, c.out_off)
  if c.x_off == c.out_off:
    assert H.same_bits(rotate(m, x, c.h, c.x_off, c.x_off, in_place=True), got) == "", "in place differs"
  return got


IDS = [c.id for c in H.CASES]


# ---------------------------------------------------------------- 1. the exact classes: no model involved
@pytest.mark.parametrize("c", H.CASES, ids=IDS)
def test_impulses_are_exact_on_every_route(m, c):
  x, want = H.impulses(c.h, c.n_vec)
  for xb, wb in zip(x, want):
    assert H.same_bits(rotate_case(m, c, xb), wb) == ""


INTEGER_CASES = [c for c in H.CASES if H.is_power_of_four(c.h)]


@pytest.mark.parametrize("c", INTEGER_CASES, ids=[c.id for c in INTEGER_CASES])
def test_dense_integers_are_exact_for_powers_of_four(m, c):
  x, want = H.integers(c.h, c.n_vec)
  assert H.same_bits(rotate_case(m, c, x[0]), want[0]) == ""


def test_integer_cases_reach_every_power_of_four_and_every_route_that_has_one():
  assert {c.h for c in INTEGER_CASES} == {1, 4, 16, 64, 256, 1024, 4096, 16384}
  assert {c.route for c in INTEGER_CASES} == {"r2", "t12", "t14"}                # 8192 is no power of four
  assert {c.h for c in INTEGER_CASES if c.route == "r2" and c.h >= H.TILE_FROM} == {256, 4096, 16384}


# ---------------------------------------------------------------- 2. dense floats: the stage-order model, and float64
@pytest.mark.parametrize("c", H.CASES, ids=IDS)
def test_floats_equal_the_stage_order_model_and_stay_inside_the_float64_bound(m, c):
  x, plant = H.floats(c.h, c.n_vec)
  want = H.float_want(c.h, c.n_vec, H.stage_order(c.route, c.h))
  assert set(H.FLOAT_PLANTS) <= set(plant.ravel())
  worst = 0.0
  for xb, pb, wb in zip(x, plant, want):
    got = rotate_case(m, c, xb)
    # vectors are independent (a tile or a block carries several): what is not finite stays where it was put
    assert np.array_equal((~np.isfinite(got)).any(axis=1), np.isin(pb, ("nan", "inf")))
    assert np.array_equal(np.isnan(got).any(axis=1), pb == "nan")
    assert H.same_bits(got, wb) == ""
    finite = ~np.isin(pb, ("nan", "inf"))
    err = np.abs(got[finite].astype(np.float64) - H.fwht64(xb[finite], c.h))
    tol = H.bound(xb[finite], c.h)
    assert (err <= tol).all()
    nz = tol[:, 0] > 0
    if nz.any():
      worst = max(worst, float((err[nz] / tol[nz]).max()))
    if not (c.x_off or c.out_off):                               # the wrapper takes the same route (torch aligns)
      wrapped = m.ops.hadamard_rotate(m.torch.from_numpy(np.array(xb)).cuda().reshape(-1), c.h)
      assert wrapped.data_ptr() % 16 == 0 and H.same_bits(wrapped.cpu().numpy().reshape(got.shape), got) == ""
  print(f"hadamard route {c.id}: worst |gpu - float64| / ((L + 4) 2^-24 ||x||_2) = {worst:.4f}")


@pytest.mark.parametrize("h", [2048, 4096, 8192, 16384])
def test_the_misaligned_fallback_differs_in_bits_from_the_tile_kernels_from_2048_on(m, h):
  """Documented, and pinned here: which order a call gets follows from h and the two alignments, nothing else."""
  x, plant = H.floats(h, 7)
  xb = x[0, 5:]
  assert xb.shape == (2, h) and (plant[0, 5:] == "plain").all()
  tile, fallback = rotate(m, xb, h), rotate(m, xb, h, 1, 1)
  assert H.same_bits(tile, H.model(xb, h, H.stage_order(H.route(h, True, True), h))) == ""
  assert H.same_bits(fallback, H.model(xb, h, H.stage_order("r2", h))) == ""
  assert (tile.view(np.uint32) != fallback.view(np.uint32)).sum() > h // 4


# ---------------------------------------------------------------- 3. refusals and empties
OK, BAD_ARG, UNSUPPORTED = 0, -1, -3
POWER, TOO_BIG = "Hadamard matrix size must be a power of 2. ", "hadamard size > 16384 does not fit one LDS tile"


def test_refusals_return_the_status_and_message_and_write_nothing(m):
  L, st = m.L, m.rt.stream_ptr()
  src, dst = Guarded(64, 0, np.ones(64, F)), Guarded(64)

  def refused(call, status, message):
    assert call() == status
    assert L.mi355q_last_error().decode() == message
    m.torch.cuda.synchronize()
    assert dst.untouched(), "a refused call wrote"

  refused(lambda: L.mi355q_hadamard_rotate_f32(src.ptr, 0, 8, dst.ptr, st), OK, "")
  refused(lambda: L.mi355q_hadamard_rotate_f32(None, 0, 8, None, st), OK, "")
  for h in (0, 3, -8):
    refused(lambda: L.mi355q_hadamard_rotate_f32(src.ptr, 64 // max(h, 1), h, dst.ptr, st), BAD_ARG, POWER)
  refused(lambda: L.mi355q_hadamard_rotate_f32(src.ptr, 1, 32768, dst.ptr, st), UNSUPPORTED, TOO_BIG)
  refused(lambda: L.mi355q_hadamard_rotate_f32(src.ptr, 0, 32768, dst.ptr, st), UNSUPPORTED, TOO_BIG)      # before n_vec == 0
  refused(lambda: L.mi355q_hadamard_rotate_f32(src.ptr, -1, 8, dst.ptr, st), BAD_ARG, "negative vector count")
  refused(lambda: L.mi355q_hadamard_rotate_f32(None, 8, 8, dst.ptr, st), BAD_ARG, "null pointer")
  refused(lambda: L.mi355q_hadamard_rotate_f32(src.ptr, 8, 8, None, st), BAD_ARG, "null pointer")
  x = m.torch.ones(32768, dtype=m.torch.float32, device="cuda")
  with pytest.raises(m.ffi.Mi355qError, match="UNSUPPORTED"):
    m.ops.hadamard_rotate(x, 32768)
  with pytest.raises(ValueError, match="power of 2"):
    m.ops.hadamard_rotate(x, 3)
  # and the same arguments, accepted, do write
  m.ffi.check(L.mi355q_hadamard_rotate_f32(src.ptr, 8, 8, dst.ptr, st))
  assert not dst.untouched()


# ---------------------------------------------------------------- 4. the effective-weight delta against the model
DELTA = [pytest.param(kind, h, rows, d, off, id=f"{kind}-h{h}-{rows}x{d}-{'offset' if off else 'aligned'}")
         for h, rows, d in H.DELTA_SHAPES for kind in H.DELTA_KINDS for off in (0, 1)]


@pytest.mark.parametrize("kind,h,rows,d,off", DELTA)
def test_weight_delta_transformed_equals_reference_minus_the_model(m, kind, h, rows, d, off):
  """Not against hadamard_rotate, whose networks it shares: against w - model(dequant) under delta_route(h), which
  follows h alone. A reference / delta_out one float off only make the accesses scalar."""
  c = H.delta_case(kind, h, rows, d)
  n = rows * d
  dev = lambda a: m.torch.from_numpy(np.array(a)).cuda()
  stored = dev(c["stored"])
  scale = None if c["scale"] is None else dev(c["scale"])
  assert stored.data_ptr() % 16 == 0
  ref, out = Guarded(n, off, c["w"]), Guarded(n, off)
  m.ffi.check(m.L.mi355q_weight_delta_transformed_f32(
      ref.ptr, m.rt.ptr(stored), n, m.ops.COMPARE_KINDS[kind], 32, rows if kind == "i4" else 1, d if kind == "i4" else 1,
      m.rt.ptr(scale), None, d, None, h, out.ptr, m.rt.stream_ptr()))
  assert H.same_bits(out.result((n,)), c["want"]) == ""
  assert H.same_bits(ref.result((n,)), c["w"]) == "", "the reference was written to"
  if not off:                                                    # and the wrapper, on torch's aligned allocations
    target = m.ops.CompareTarget(stored, n, kind, scale, None, rows if kind == "i4" else 1, d if kind == "i4" else 1, 32)
    got = m.ops.weight_delta_transformed(dev(c["w"]), target, d, hadamard_size=h)
    assert H.same_bits(got.cpu().numpy(), c["want"]) == ""


# ---------------------------------------------------------------- 5. the Python layer
def test_rotate_with_diagonal_hadamard_returns_the_bits_of_the_model(m):
  shape, h = (4, 6, 64), 64
  x, _ = H.floats(h, 24)
  w = np.array(x[0]).reshape(shape)
  w[~np.isfinite(w)] = 1.0                                       # a weight tensor
  rotated, size, vec = m.had._rotate_with_diagonal_hadamard(w, axis=2)      # pylint: disable=protected-access
  assert size == h and vec.dtype == np.int8 and np.array_equal(vec, np.ones(h, np.int8))
  assert isinstance(rotated, np.ndarray) and rotated.shape == shape
  want = H.model(w, h, H.stage_order(H.route(h, True, True), h)).reshape(shape)
  assert H.same_bits(rotated, want) == ""
  with pytest.raises(ValueError, match="Hadamard size would be 1"):
    m.had._rotate_with_diagonal_hadamard(w[..., :63], axis=2)               # pylint: disable=protected-access
