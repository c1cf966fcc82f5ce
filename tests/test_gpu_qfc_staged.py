"""The staged MFMA route of the integer FULLY_CONNECTED kernels (csrc/qfc_staged.h) on the GPU: ops.qfc_forward
(accumulator and float output) and ops.qfc_output (stored output) bit for bit against the NumPy statements of
layer_execution_cases / layer_output_cases, at every ragged reduction length around a 64-byte stage, every byte
alignment of both operands (slices of buffers whose other bytes are 127), partial tiles on both axes down to one wave
of four owning a tile, every zero point, the accumulator's extreme; the same calls on the generic kernel; and one
product of each consumer (CONV_2D patches, TRANSPOSE_CONV phases)."""
import os
import sys

import numpy as np
import pytest

import layer_execution_cases as EC
import layer_output_cases as OC
import tconv_execution_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
PLANTED = (-128, -127, -1, 0, 1, 127)
D_LIST = (1, 3, 27, 63, 64, 65, 100, 127, 129, 216)
SHAPES = ((1, 1), (17, 130), (129, 17), (130, 130))
OFFSETS = ((0, 0), (1, 2), (2, 3), (3, 1))      # bytes of xq and of w past an aligned allocation


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available()
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import ops

  class M:
    pass
  M.torch, M.ops = torch, ops
  M.dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())

  def inside(a, offset):
    """`a` on the device `offset` bytes into a buffer of 127s: a neighbour that is wrongly included changes the sum."""
    buf = torch.full((a.size + 8,), 127, dtype=torch.int8, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 4 == offset
    return view
  M.inside = staticmethod(inside)
  return M


def _operand(rng, rows, d, fill):
  if fill is not None:
    return np.full((rows, d), fill, np.int8)
  a = rng.integers(-128, 127, size=(rows, d), endpoint=True).astype(np.int8)
  for r in range(rows):      # the first and the last element of every row: what the edge words of the staging hold
    a[r, 0], a[r, -1] = PLANTED[r % 6], PLANTED[(r // 6 + r + 3) % 6]
  return a


def _case(m, n, rows, d, offsets, zp, per_channel, seed, fill=None):
  """The three outputs of one problem on the device (acc, y, q) and what the statements say."""
  rng = np.random.default_rng(seed)
  xq, qw = _operand(rng, n, d, fill), _operand(rng, rows, d, fill)
  xs = (np.exp(rng.normal(size=n if seed % 2 else 1)) * 0.02).astype(np.float32)
  ws = (np.exp(rng.normal(size=rows if per_channel else 1)) * 0.01).astype(np.float32)
  acc_rms = np.sqrt(d) * float(np.sqrt(5461.0 + zp * zp)) * 74.0
  ms = [OC.quantize_multiplier(50.0 / acc_rms * float(np.exp(rng.uniform(-1.5, 1.5)))) for _ in ws]
  mult, shift = [v[0] for v in ms], [v[1] for v in ms]
  bias = np.rint(rng.standard_normal(rows) * acc_rms).astype(np.int32) if seed % 3 else None
  x_dev, w_dev = m.inside(xq, offsets[0]), m.inside(qw, offsets[1])
  target = m.ops.CompareTarget(w_dev.view(-1), rows * d, "i8", m.dev(ws), None, ws.size, d if per_channel else 1, 32)

  def run():
    y, acc = m.ops.qfc_forward(x_dev, m.dev(xs), zp, target, rows, d, want_acc=True)
    q = m.ops.qfc_output(x_dev, zp, target, rows, d, bias, mult, shift, -3, -128, 127)
    return acc, y, q
  want_acc, want_y = EC.forward(xq, xs, zp, qw, ws)
  return run, (want_acc, want_y, OC.output_i8(xq, zp, qw, bias, mult, shift, -3, -128, 127)), (x_dev, w_dev)


def _check(m, n, rows, d, offsets, zp, per_channel, seed, fill=None, generic_too=False):
  run, (want_acc, want_y, want_q), (x_dev, w_dev) = _case(m, n, rows, d, offsets, zp, per_channel, seed, fill)
  assert m.ops.qfc_route(x_dev, w_dev, d) == "staged"
  acc, y, q = run()
  tag = (n, rows, d, offsets, zp, per_channel)
  assert np.array_equal(acc.cpu().numpy(), want_acc), tag
  assert EC.same_bits(y.cpu().numpy(), want_y), tag
  assert np.array_equal(q.cpu().numpy(), want_q), tag
  if generic_too:
    with m.ops.qfc_staged(False):
      assert m.ops.qfc_route(x_dev, w_dev, d) == "generic"
      for got, staged in zip(run(), (acc, y.view(m.torch.int32), q)):
        assert m.torch.equal(got.view(staged.dtype), staged), tag


def _cases():
  """(n, rows, d, offsets, zp, per_channel, seed, fill, generic_too) of every problem, each with its reason."""
  out = []
  # every reduction length: a stage that is all tail, a tail after one and after two whole stages, one byte short of
  # and beyond a stage, and whole stages reached only through misalignment (d = 64)
  for i, d in enumerate(D_LIST):
    out.append((17, 130, d, OFFSETS[1 + i % 3], (0, -128, 127)[i % 3], bool(i % 2), 100 + i, None, False))
  # one wave of four with a tile (1 x 1), partial tiles on either axis, two workgroups on both grid axes; every offset
  # of either base; and the generic kernel on the same operands
  for n, rows in SHAPES:
    for offsets in OFFSETS:
      for d in (27, 129):
        i = SHAPES.index((n, rows)) + OFFSETS.index(offsets)
        out.append((n, rows, d, offsets, (127, 0, -128)[i % 3], bool(i % 2), 200 + 10 * i + d, None, True))
  for zp in (0, -128, 127):
    for per_channel in (False, True):
      out.append((130, 130, 100, (3, 2), zp, per_channel, 300 + zp + int(per_channel), None, False))
  # d = 65535 (1023 whole stages and one of 63 bytes, every row at another alignment) with every operand -128 and
  # zp = 127: acc = 65535 * 255 * 128, the accumulator's extreme
  out.append((17, 3, 65535, (1, 3), 127, True, 400, -128, False))
  return out


def _a_convolutions_product_takes_the_route(m):
  """3 x 3 x 3 -> 8 on a 2 x 5 x 5 x 3 image, SAME: K = 27."""
  rng = np.random.default_rng(5)
  zp = -7
  x = rng.integers(-128, 127, size=(2, 5, 5, 3), endpoint=True).astype(np.int8)
  qw = rng.integers(-128, 127, size=(8, 3, 3, 3), endpoint=True).astype(np.int8)
  padded = np.full((2, 7, 7, 3), zp, np.int64)
  padded[:, 1:6, 1:6] = x
  want = np.zeros((2, 5, 5, 8), np.int64)
  for i in range(3):
    for j in range(3):
      want += np.einsum("nhwc,oc->nhwo", padded[:, i:i + 5, j:j + 5] - zp, qw[:, i, j].astype(np.int64))
  rows = m.ops.conv_patches(m.dev(x), 3, 3, 1, 1, "SAME", pad_value=zp)
  target = m.ops.CompareTarget(m.dev(qw.ravel()), qw.size, "i8", m.dev(np.array([0.01], np.float32)), None, 1, 1, 32)
  assert tuple(rows.shape) == (50, 27) and m.ops.qfc_route(rows, target.data, 27) == "staged"
  _, acc = m.ops.qfc_forward(rows, m.dev(np.array([0.02], np.float32)), zp, target, 8, 27, want_acc=True)
  assert np.array_equal(acc.cpu().numpy(), want.reshape(50, 8))


def _a_transposed_convolutions_phases_take_the_route(m):
  """4 x 4 at stride 2 over 24 channels on a 1 x 3 x 3 x 24 image, SAME: four phases of K = 2 x 2 x 24 = 96."""
  rng = np.random.default_rng(6)
  zp, k, s, out_hw = 127, (4, 4), (2, 2), (6, 6)
  x = rng.integers(-128, 127, size=(1, 3, 3, 24), endpoint=True).astype(np.int8)
  qw = rng.integers(-128, 127, size=(5, 4, 4, 24), endpoint=True).astype(np.int8)
  assert [len(p[4]) * len(p[5]) * 24 for p in TC.phases(3, 3, 4, 4, s, TC.SAME, out_hw)] == [96] * 4
  target = m.ops.CompareTarget(m.dev(qw.ravel()), qw.size, "i8", m.dev(np.array([0.01], np.float32)), None, 1, 1, 32)
  assert m.ops.qfc_route(m.dev(x), target.data, 96) == "staged"
  _, acc = m.ops.tconv_forward(m.dev(x), target, 4, 4, s, TC.SAME, out_hw, x_scale=m.dev(np.array([0.02], np.float32)),
                               x_zero_point=zp, want_acc=True)
  assert np.array_equal(acc.cpu().numpy(), TC.integer_tconv(x, zp, qw, s, TC.SAME, out_hw))


def test_the_staged_route_bit_for_bit(m):
  """Every case of _cases() and one product of each consumer, in ONE test (each assertion names its case): the cases
  are the parametrisation, kept inside a single test id so that the suite's number of GPU cases does not grow by 50."""
  for n, rows, d, offsets, zp, per_channel, seed, fill, generic_too in _cases():
    _check(m, n, rows, d, offsets, zp, per_channel, seed, fill, generic_too)
  _a_convolutions_product_takes_the_route(m)
  _a_transposed_convolutions_phases_take_the_route(m)
