"""Every route of the OSCAR scale-search kernels (mi355q_oscar_col_sumsq_f32, mi355q_oscar_group_terms_f32,
mi355q_oscar_winner_energy_f64; csrc/oscar.hip), output by output and bit for bit against the reference's NumPy
expressions in FP64.

The cases, their expected values, the restatement of the host's choice of kernels and the proof that each case shows
the defects its route could have are in oscar_scale_cases.py / test_oscar_scale_cases_host.py, which need no GPU. Here
each case goes through the C ABI, so that the workspace of squared maxima (top2), which no wrapper returns, is compared
as well: float64 outputs by their 64-bit patterns, winners as int32. Every output sits between guard elements that
must come back untouched, and is pre-filled so that an element the kernel skips cannot pass. Nothing here tolerates a
difference.

What the seeded end-to-end problems of test_gpu_oscar.py cannot see, and this file does: the group sums (they feed two
comparisons of a loss), top2 (never read), winner / wsq (seen only after np.maximum(eff, 0.25 * a_base), two square roots
and a clamp) and the column sums (after sqrt(mu / sqrt(a_base)))."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest

import oscar_scale_cases as S
from oracle import aeq_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                       # elements in front of and behind every output
FILL = {np.float64: -12345.5, np.int32: -77}


@functools.lru_cache(maxsize=None)
def modules():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  from mi355q.algorithms.uniform_quantize import oscar
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), ffi=_ffi, oscar=oscar)


@pytest.fixture(scope="module")
def m():
  return modules()


def dev(a):
  return modules().torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cases are read-only


class Guarded:
  """`count` elements of `dtype` on the device between two runs of GUARD sentinels, pre-filled with the sentinel."""

  def __init__(self, count, dtype):
    torch = modules().torch
    self.count, self.dtype = count, dtype
    self.buf = torch.full((GUARD + count + GUARD,), FILL[dtype], dtype={np.float64: torch.float64, np.int32: torch.int32}[dtype],
                          device="cuda")
    self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

  def result(self, shape):
    host = self.buf.cpu().numpy()
    assert (host[:GUARD] == FILL[self.dtype]).all() and (host[GUARD + self.count:] == FILL[self.dtype]).all(), \
        "written outside the output"
    return host[GUARD:GUARD + self.count].reshape(shape).copy()


def col_sumsq(m, x, mean):
  rows, d = x.shape
  xd, out = dev(x), Guarded(d, np.float64)
  m.ffi.check(m.L.mi355q_oscar_col_sumsq_f32(m.rt.ptr(xd), rows, d, mean, out.ptr, m.rt.stream_ptr()))
  return out.result((d,))


def winner_energy(m, winner_ptr, wsq_ptr, n, d, g):
  eff = Guarded(d, np.float64)
  m.ffi.check(m.L.mi355q_oscar_winner_energy_f64(winner_ptr, wsq_ptr, n, d, g, eff.ptr, m.rt.stream_ptr()))
  return eff.result((d,))


def group_terms_then_energy(m, w, s, g):
  n, d = w.shape
  groups = d // g
  wd, sd = dev(w), dev(s)
  if g != d:            # the blockwise kernel reads w as float4 and s as double2 (include/mi355q.h)
    assert wd.data_ptr() % 16 == 0 and sd.data_ptr() % 16 == 0 and d % 4 == 0
  top2, winner, wsq = Guarded(groups * n, np.float64), Guarded(groups * n, np.int32), Guarded(groups * n, np.float64)
  sums = Guarded(groups, np.float64)
  m.ffi.check(m.L.mi355q_oscar_group_terms_f32(m.rt.ptr(wd), m.rt.ptr(sd), n, d, g, top2.ptr, winner.ptr, wsq.ptr, sums.ptr,
                                                m.rt.stream_ptr()))
  eff = winner_energy(m, winner.ptr, wsq.ptr, n, d, g)
  got = dict(top2=top2.result((groups, n)), winner=winner.result((groups, n)), wsq=wsq.result((groups, n)),
             sums=sums.result((groups,)), eff=eff)
  assert np.array_equal(wd.cpu().numpy().view(np.uint32), w.view(np.uint32)), "the weight was written to"
  # the wrappers the product calls return the same bits (all but top2, which they keep to themselves)
  o_sums, o_winner, o_wsq = m.ops.oscar_group_terms(wd, sd, g)
  o_eff = m.ops.oscar_winner_energy(o_winner, o_wsq, d, g)
  wrapped = dict(winner=o_winner.cpu().numpy(), wsq=o_wsq.cpu().numpy(), sums=o_sums.cpu().numpy(), eff=o_eff.cpu().numpy())
  assert S.same_bits(wrapped, {k: got[k] for k in wrapped}) == ""
  return got


@pytest.mark.parametrize("c", S.COL_CASES, ids=[S.case_id(c) for c in S.COL_CASES])
def test_col_sumsq_equals_numpy(m, c):
  inputs, want = S.expected(c)
  got = dict(out=col_sumsq(m, inputs["x"], c.mean))
  assert S.same_bits(got, want) == ""
  wrapped = m.ops.oscar_col_sumsq(dev(inputs["x"]), mean=bool(c.mean)).cpu().numpy()
  assert S.same_bits(dict(out=wrapped), want) == ""


@pytest.mark.parametrize("mean", (0, 1))
def test_col_sumsq_propagates_nan_and_inf(m, mean):
  x, kinds = S.nonfinite_columns()
  got = col_sumsq(m, x, mean)
  assert np.array_equal(np.isnan(got), kinds == "nan") and np.array_equal(np.isposinf(got), kinds == "inf")
  with np.errstate(invalid="ignore"):
    want = S.reference_col(x, mean)
  finite = kinds == "finite"
  assert np.array_equal(got[finite].view(np.uint64), want[finite].view(np.uint64))


@pytest.mark.parametrize("c", S.TERMS_CASES, ids=[S.case_id(c) for c in S.TERMS_CASES])
def test_group_terms_and_winner_energy_equal_numpy(m, c):
  inputs, want = S.expected(c)
  got = group_terms_then_energy(m, inputs["w"], inputs["s"], c.g)
  assert got["winner"].dtype == np.int32
  assert S.same_bits(got, want) == ""


@pytest.mark.parametrize("c", S.WINNER_CASES, ids=[S.case_id(c) for c in S.WINNER_CASES])
def test_winner_energy_on_synthetic_winners_equals_add_at(m, c):
  inputs, want = S.expected(c)
  wd, sd = dev(inputs["winner"]), dev(inputs["wsq"])
  got = dict(eff=winner_energy(m, m.rt.ptr(wd), m.rt.ptr(sd), c.n, c.d, c.g))
  assert S.same_bits(got, want) == ""
  never = np.setdiff1d(np.arange(c.d), inputs["winner"].ravel())
  assert len(never) and (got["eff"][never].view(np.uint64) == 0).all()          # +0.0, not the pre-fill and not -0.0


@pytest.mark.parametrize("c", S.OBJECTIVE_CASES, ids=[S.case_id(c) for c in S.OBJECTIVE_CASES])
def test_channel_scale_objective_equals_the_oracle(m, c):
  inputs, _ = S.expected(c)
  w, s, mu2 = inputs["w"], inputs["s"], S.masses(c)
  block = c.g if c.g != c.d else 0
  got = m.oscar._channel_scale_objective(w, s, mu2, block)                      # pylint: disable=protected-access
  want = O.oscar_scale_objective(w.astype(np.float64), s, mu2, block)
  assert isinstance(got, float) and got == want
