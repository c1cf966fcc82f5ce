"""Integer execution of static FULLY_CONNECTED ops through to their stored output, on the GPU (csrc/qfc_out.hip,
ops.qfc_output / ops.qfc_output_i16, compare_layer_execution / validate_layer_execution with `quantized_outputs`).

  1. q_out bit for bit against the Python-integer statement of tests/layer_output_cases.py: the tile edges of the
     16 / 64 / 128 maps, every weight kind, one multiplier or one per channel, with and without a bias, zero points at
     the ends of int8; planted accumulators at every saturation, tie and range edge of the epilogue; d = 65536 with
     all-extreme operands; the generic route. The integers are exact, so one wrong bit anywhere is a failure.
  2. end to end: the four-op model of layer_output_cases under static_wi8_ai8 and static_wi8_ai16, against the
     statement run on the written model with Y in float64 and the first-order bound of the FP32 reference.
"""
import os
import sys

import numpy as np
import pytest

import layer_error_cases as LC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
KIND_CODE = {"i8": 3, "i4": 6, "i2": 7}


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


def _stored(qw: np.ndarray, kind: str) -> np.ndarray:
  if kind == "i8":
    return qw.astype(np.int8).ravel()
  per = 8 // EC.BITS[kind]
  flat = qw.ravel()
  pad = (-flat.size) % per
  return LC.pack(np.concatenate([flat, np.zeros(pad, flat.dtype)]), EC.BITS[kind])


def _run(m, bits, xq_dev, zp_x, qw, kind, bias, mult, shift, zp_y, lo, hi):
  """One call of the C entry; q_out is pre-filled so that an output the kernel skips shows."""
  n, d = xq_dev.shape
  rows = qw.shape[0]
  torch = m.torch
  q = torch.full((n, rows), 77, dtype=torch.int16 if bits == 16 else torch.int8, device="cuda")
  nbytes = m.lib.mi355q_qfc_output_workspace_bytes(rows, d)
  ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
  w_dev = m.dev(_stored(qw, kind))
  m_dev, s_dev = m.dev(np.asarray(mult, np.int32)), m.dev(np.asarray(shift, np.int32))
  if bits == 16:
    b_dev = None if bias is None else m.dev(np.asarray(bias, np.int64))
    st = m.lib.mi355q_qfc_output_i16(m.rt.ptr(xq_dev), n, d, m.rt.ptr(w_dev), KIND_CODE[kind], rows, m.rt.ptr(b_dev),
                                     m.rt.ptr(m_dev), m.rt.ptr(s_dev), m_dev.numel(), lo, hi, m.rt.ptr(q), m.rt.ptr(ws),
                                     nbytes, m.rt.stream_ptr())
  else:
    b_dev = None if bias is None else m.dev(np.asarray(bias, np.int32))
    st = m.lib.mi355q_qfc_output_i8(m.rt.ptr(xq_dev), n, d, zp_x, m.rt.ptr(w_dev), KIND_CODE[kind], rows, m.rt.ptr(b_dev),
                                    m.rt.ptr(m_dev), m.rt.ptr(s_dev), m_dev.numel(), zp_y, lo, hi, m.rt.ptr(q),
                                    m.rt.ptr(ws), nbytes, m.rt.stream_ptr())
  m.ffi.check(st)
  return q.cpu().numpy()


def _statement(bits, xq, zp_x, qw, bias, mult, shift, zp_y, lo, hi):
  if bits == 16:
    return OC.output_i16(xq, qw, bias, mult, shift, lo, hi)
  return OC.output_i8(xq, zp_x, qw, bias, mult, shift, zp_y, lo, hi)


def _check(m, bits, xq, zp_x, qw, kind, bias, mult, shift, zp_y, lo, hi, tag, misalign_x=False):
  want = _statement(bits, xq, zp_x, qw, bias, mult, shift, zp_y, lo, hi)
  got = _run(m, bits, m.misaligned(xq) if misalign_x else m.dev(xq), zp_x, qw, kind, bias, mult, shift, zp_y, lo, hi)
  assert got.dtype == want.dtype and got.shape == want.shape
  assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])
  return want


ZP_X, ZP_Y = (0, -128, 5, 127), (-128, 0, 127)
RANGES = {8: ((-128, 127), (-100, 90), (-128, 0), (3, 3)), 16: ((-32768, 32767), (-20000, 15000), (0, 32767), (-7, -7))}


def _random_case(m, bits, n, rows, d, kind, i, seed, misalign_x=False):
  """One random call; `i` picks the multiplier count, the bias, the zero points and the activation range in turn, so
  that a list of cases meets every value of each."""
  rng = np.random.default_rng(seed)
  wbits = EC.BITS[kind]
  wlo, whi = -(1 << (wbits - 1)), (1 << (wbits - 1)) - 1
  xlo, xhi = (-32768, 32767) if bits == 16 else (-128, 127)
  xq = rng.integers(xlo, xhi, size=(n, d), endpoint=True).astype(np.int16 if bits == 16 else np.int8)
  if bits == 16:
    for t in range(n):
      for j, v in enumerate(EC16.PLANTED[:d]):
        xq[t, (3 * t + j) % d] = v
  qw = rng.integers(wlo, whi, size=(rows, d), endpoint=True)
  qw.ravel()[rng.integers(0, qw.size)] = wlo
  # (in a list of 8 x 8 shapes with the second index fastest, neither choice is tied to a shape's place in its row)
  zp_x = 0 if bits == 16 else ZP_X[(i // 4 + i // 16) % 4]
  zp_y = 0 if bits == 16 else ZP_Y[(i // 5) % 3]
  per_channel, with_bias = bool((i + i // 8) % 2), bool((i // 2 + i // 16) % 2)
  lo, hi = RANGES[bits][(i // 3) % 4]
  # multipliers that spread the outputs over the type: acc is about sqrt(d) x_rms w_rms
  x_rms = 18918.0 if bits == 16 else float(np.sqrt(5461.0 + zp_x * zp_x))
  acc_rms = np.sqrt(d) * x_rms * (whi + 0.5) / np.sqrt(3.0)
  real = (9000.0 if bits == 16 else 50.0) / acc_rms
  ms = [OC.quantize_multiplier(real * float(np.exp(rng.uniform(-1.5, 1.5)))) for _ in range(rows if per_channel else 1)]
  mult, shift = [v[0] for v in ms], [v[1] for v in ms]
  bias = None
  if with_bias:
    bias = np.rint(rng.standard_normal(rows) * 2.0 * acc_rms).astype(np.int64)
  want = _check(m, bits, xq, zp_x, qw, kind, bias, mult, shift, zp_y, lo, hi, (bits, n, rows, d, kind, i), misalign_x)
  return want, (lo, hi)


EDGES = (1, 15, 16, 17, 63, 64, 65, 130)


@pytest.mark.parametrize("d", [64, 128, 1024])
@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
@pytest.mark.parametrize("bits", [8, 16])
def test_output_mfma_route_bit_for_bit(m, bits, kind, d):
  """Every n x rows of the tile edges. The case index walks through mcount in {1, rows}, with / without a bias, the
  four input and three output zero points and four activation ranges: 64 cases meet every value of each with every
  kind, d and entry, and some land inside the range while others clamp."""
  i, inside, clamped = 0, 0, 0
  for n in EDGES:
    for rows in EDGES:
      want, (lo, hi) = _random_case(m, bits, n, rows, d, kind, i, 1000 * d + 7 * i + bits)
      inside += int(((want > lo) & (want < hi)).sum())
      clamped += int(((want == lo) | (want == hi)).sum())
      i += 1
  assert inside > 10000 and clamped > 1000, (inside, clamped)


@pytest.mark.parametrize("kind", ["i8", "i4", "i2"])
@pytest.mark.parametrize("bits", [8, 16])
def test_output_generic_route_bit_for_bit(m, bits, kind):
  """d that is no multiple of 64 (packed rows that begin inside a byte when d is odd), and a misaligned xq at an MFMA
  shape."""
  i = 0
  for d in (1, 7, 33, 100):
    for n, rows in ((1, 1), (5, 6), (17, 3), (3, 65)):
      _random_case(m, bits, n, rows, d, kind, i, 9000 + 10 * d + i)
      i += 1
  for i in range(4):
    _random_case(m, bits, 17, 15, 128, kind, i + 1, 9500 + i, misalign_x=True)


# ---------------------------------------------------------------- planted accumulators
def _one_hot(rows, d=64):
  qw = np.zeros((rows, d), np.int64)
  qw[:, 0] = 1      # acc[t, r] = xq[t, 0] - zp_x
  return qw


I32 = (OC.INT32_MIN, OC.INT32_MAX)
PLANT_A8 = sorted(set(
    [I32[0], I32[0] + 1, I32[1] - 1, I32[1], 0, 1, -1, 2, -2, 3, -3, 99, -99, 100, -100, 101, -101, 102, -102,
     -104, -103, 87, 88, 89,                                                   # the edges of [-100, 90] with zp_y = 3
     (1 << 30) - 1, 1 << 30, (1 << 30) + 1, -(1 << 30) + 1, -(1 << 30), -(1 << 30) - 1,      # where a 2^1 saturates
     1 << 24, -(1 << 24), (1 << 24) + 1, (1 << 24) - 1, 3 << 23, -(3 << 23)]      # where a 2^7 saturates
    + [sgn * k * (1 << e) for sgn in (1, -1) for k in (1, 3) for e in (0, 7, 8, 29, 30)]))      # halves of >> 1, 8, 31
PLANT_M8 = (0, 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 1)
PLANT_S8 = (0, -1, -8, -31, 1, 7, 30)


def test_planted_accumulators_int8(m):
  """Every weight row is one-hot, so acc = xq[t, 0] - zp_x and the token with acc = 1 puts a = 1 + bias at a chosen
  value: INT32_MIN / INT32_MAX (both sat32), exact halves of the high multiplication in both signs (odd a with
  M = 2^30), exact halves of the rounding shift in both signs (a = +-k 2^(R-1) 2 with M = 2^30), R in {0, 1, 8, 31},
  L in {1, 7, 30} on both sides of where a 2^L saturates, M in {0, 1, 2^30, 2^30 + 1, 2^31 - 1}; one channel for
  every (a, M, s). The other tokens push a past both ends of int32. With M = 2^30 and s = 1 the op is the identity, so
  under zp_y = 3 and [-100, 90] the values -104, -103, 87, 88 land on act_min - 1, act_min, act_max, act_max + 1."""
  plan = [(a, mm, s) for a in PLANT_A8 for mm in PLANT_M8 for s in PLANT_S8]
  rows = len(plan)
  xq = np.zeros((6, 64), np.int8)
  xq[:, 0] = (1, 127, -128, 0, -1, 5)
  xq[:, 1:] = np.random.default_rng(1).integers(-128, 127, size=(6, 63), endpoint=True)      # (times weight 0)
  bias = np.clip(np.array([a - 1 for a, _, _ in plan], np.int64), *I32)
  mult, shift = [p[1] for p in plan], [p[2] for p in plan]
  # the statement's own values, checked here for what the docstring claims
  ident = {a: OC.mbqm32(a, 1 << 30, 1) for a in (-104, -103, 87, 88)}
  assert ident == {-104: -104, -103: -103, 87: 87, 88: 88}
  assert OC.sat32(127 + I32[1] - 1) == I32[1] and OC.sat32(-128 + I32[0]) == I32[0]
  for zp_y, (lo, hi) in ((3, (-100, 90)), (0, (-128, 127)), (-128, (-128, 127)), (127, (-128, 127))):
    for misalign in (False, True):      # the MFMA route and the generic route
      want = _check(m, 8, xq, 0, _one_hot(rows), "i8", bias, mult, shift, zp_y, lo, hi, ("planted", zp_y, misalign), misalign)
      if zp_y == 3:
        col = {p: r for r, p in enumerate(plan)}
        assert [int(want[0, col[(a, 1 << 30, 1)]]) for a in (-104, -103, 87, 88)] == [-100, -100, 90, 90]
        assert int(want[0, col[(-102, 1 << 30, 1)]]) == -99 and int(want[0, col[(89, 1 << 30, 1)]]) == 90
  # an input zero point moves acc: the same plan with zp_x = -128 (acc = xq + 128) and 127
  for zp_x in (-128, 127):
    _check(m, 8, xq, zp_x, _one_hot(rows), "i8", bias, mult, shift, 0, -128, 127, ("planted zp_x", zp_x))
  # one multiplier for the tensor, no bias: acc itself over all of int8 minus zp_x
  xs = np.zeros((256, 64), np.int8)
  xs[:, 0] = np.arange(-128, 128)
  for mm, s in ((1 << 30, 1), (1 << 30, 0), ((1 << 31) - 1, -1), (1 << 30, -8), (0, 5)):
    _check(m, 8, xs, 5, _one_hot(33), "i8", None, [mm], [s], -7, -128, 127, ("acc sweep", mm, s))


A16 = (OC.A16_MIN, OC.A16_MAX)
PLANT_A16 = sorted(set([A16[0] - (1 << 50), A16[0] - 5, A16[0] - 1, A16[0], A16[0] + 1, A16[1] - 1, A16[1], A16[1] + 1,
                        A16[1] + 5, 1 << 50, 0, 1, -1, 2, -2, 3, -3, 100, -100, 101, -101, 1 << 14, -(1 << 14), (1 << 14) + 1,
                        1 << 31, -(1 << 31), (1 << 31) + 1, (1 << 45), -(1 << 45), (1 << 45) + 1, 3 << 44, -(3 << 44)]))
PLANT_M16 = (0, 1 << 15, 1 << 30, 0x7FFE7FFF, 0x7FFE8000, 0x7FFEFFFF, 0x7FFF0000, 0x7FFFFFFF)
PLANT_S16 = (14, 13, 0, -1, -16, -30, -31)      # T = 1, 2, 15, 16, 31, 45, 46


def test_planted_accumulators_int16(m):
  """acc = xq[t, 0]; the token with acc = 1 puts acc + bias at a chosen value: beyond +-2^47 on both sides (clamped),
  the bounds themselves, halves of the rounding shift; T in {1, 2, 15, 16, 31, 45, 46}; M on both sides of each
  rounding step of Mr and of the 0x7FFF0000 threshold."""
  plan = [(a, mm, s) for a in PLANT_A16 for mm in PLANT_M16 for s in PLANT_S16]
  rows = len(plan)
  xq = np.zeros((5, 64), np.int16)
  xq[:, 0] = (1, 32767, -32768, 0, -1)
  xq[:, 1:] = np.random.default_rng(2).integers(-32768, 32767, size=(5, 63), endpoint=True)
  bias = np.array([a - 1 for a, _, _ in plan], np.int64)
  mult, shift = [p[1] for p in plan], [p[2] for p in plan]
  assert OC.rounded_multiplier(0x7FFE7FFF) + 1 == OC.rounded_multiplier(0x7FFE8000) == OC.rounded_multiplier(0x7FFFFFFF)
  for lo, hi in ((-32768, 32767), (-20000, 15000)):
    for misalign in (False, True):
      want = _check(m, 16, xq, 0, _one_hot(rows), "i8", bias, mult, shift, 0, lo, hi, ("planted16", lo, misalign), misalign)
      assert (want == lo).any() and (want == hi).any() and ((want > lo) & (want < hi)).sum() > rows
  xs = np.zeros((130, 64), np.int16)
  xs[:, 0] = np.arange(-65, 65) * 504
  xs[:15, 0] = EC16.PLANTED
  for mm, s in ((1 << 30, 1), (1 << 30, 0), (0x7FFFFFFF, -1), (0, 5)):
    _check(m, 16, xs, 0, _one_hot(33), "i8", None, [mm], [s], 0, -32768, 32767, ("acc sweep 16", mm, s))


# ---------------------------------------------------------------- the longest row
def test_extremes_at_the_longest_row(m):
  """d = 65536, n = 17, rows = 16, every operand at its extreme: the int8 accumulator stands at 65536 * 255 * 128 =
  2^31 - 2^23, each int16 plane at 2^30. A bias that keeps a in range, and one that saturates it."""
  d, n, rows = 65536, 17, 16
  xq = np.full((n, d), -128, np.int8)
  qw = np.full((rows, d), -128, np.int64)
  top = d * 255 * 128
  assert top == (1 << 31) - (1 << 23) and OC.accumulators(xq[:1], 127, qw[:1], top)[0][0] == top
  keep = np.array([(-top + 37 * r - 300) for r in range(rows)], np.int64)            # a = 37 r - 300
  saturate = np.array([(1 << 23) + r if r % 2 else -(1 << 30) for r in range(rows)], np.int64)      # a = 2^31 + r: sat32
  assert top + int(saturate[1]) > OC.INT32_MAX and 0 < top + int(saturate[0]) < OC.INT32_MAX
  ms = [OC.quantize_multiplier(0.11 * (1 + r % 5)) for r in range(rows)]      # |a| <= 300 stays inside int8
  mult, shift = [v[0] for v in ms], [v[1] for v in ms]
  want = _check(m, 8, xq, 127, qw, "i8", keep, mult, shift, -3, -128, 127, "extreme keep")
  assert len(set(want[0].tolist())) > 8 and (want == want[:1]).all()
  want = _check(m, 8, xq, 127, qw, "i8", saturate, [1 << 30] * rows, [-24] * rows, 0, -128, 127, "extreme saturate")
  assert want[0].tolist() == [32, 64] * 8      # (2^30 - 2^23) / 2^25 = 31.75 and (2^31 - 1) / 2^25 = 64 - 2^-25, rounded
  _check(m, 8, xq, 127, qw, "i8", saturate, [(1 << 31) - 1], [-31], 0, -128, 127, "extreme saturate one multiplier")
  _check(m, 8, np.full((n, d), 127, np.int8), -128, qw, "i8", -keep - 1, mult, shift, 5, -128, 127, "extreme negative")
  # int16: acc = 2^38 (and -65536 * 32767 * 128)
  x16 = np.full((n, d), -32768, np.int16)
  assert OC.accumulators(x16[:1], 0, qw[:1], 1 << 38)[0][0] == 1 << 38
  keep = np.array([-(1 << 38) + 1000 * r - 9000 for r in range(rows)], np.int64)
  saturate = np.array([(1 << 47) if r % 2 else -(1 << 47) - (1 << 39) for r in range(rows)], np.int64)
  want = _check(m, 16, x16, 0, qw, "i8", keep, mult, shift, 0, -32768, 32767, "extreme16 keep")
  assert len(set(want[0].tolist())) > 8
  want = _check(m, 16, x16, 0, qw, "i8", saturate, [1 << 26] * rows, [-31] * rows, 0, -32768, 32767, "extreme16 saturate")
  assert want[0].tolist() == [-2048, 2048] * 8      # a = -2^47 and 2^47 - 1 (both clamped), Mr = 2^10, T = 46
  keep = np.array([(1 << 38) - (1 << 23) + 1000 * r - 9000 for r in range(rows)], np.int64)      # acc = -2^38 + 2^23
  want = _check(m, 16, np.full((n, d), 32767, np.int16), 0, qw, "i8", keep, mult, shift, 0, -32768, 32767, "extreme16 negative")
  assert len(set(want[0].tolist())) > 8


def test_refusals_and_the_ops_wrappers(m):
  OC.check_output_refusals(m.lib)
  rng = np.random.default_rng(5)
  n, rows, d = 17, 33, 128
  for kind, channels, inner in (("i8", 1, 1), ("i8", rows, d), ("i4", rows, d), ("i2", 1, 1)):
    wbits = EC.BITS[kind]
    qw = rng.integers(-(1 << (wbits - 1)), (1 << (wbits - 1)) - 1, size=(rows, d), endpoint=True)
    wsc = (np.exp(rng.normal(size=channels)) * 0.01).astype(np.float32)
    target = m.ops.CompareTarget(m.dev(_stored(qw, kind)), rows * d, kind, m.dev(wsc), None, channels, inner, 32)
    ms = [OC.quantize_multiplier(float(np.exp(rng.uniform(-9, -7)))) for _ in range(channels)]
    mult, shift = [v[0] for v in ms], [v[1] for v in ms]
    x8 = rng.integers(-128, 127, size=(n, d), endpoint=True).astype(np.int8)
    b32 = rng.integers(-50000, 50000, size=rows).astype(np.int32)
    got = m.ops.qfc_output(m.dev(x8), 5, target, rows, d, b32, mult, shift, -3, -128, 127)
    assert got.dtype == m.torch.int8 and np.array_equal(got.cpu().numpy(), OC.output_i8(x8, 5, qw, b32, mult, shift, -3, -128, 127))
    tables = m.ops.qfc_multipliers(mult, shift, rows, 8)      # uploaded once, for several calls
    again = m.ops.qfc_output(m.dev(x8), 5, target, rows, d, m.dev(b32), tables, None, -3, -128, 127)
    assert np.array_equal(again.cpu().numpy(), got.cpu().numpy())
    with pytest.raises(ValueError, match="prepared multipliers are for 33 rows and 8-bit"):
      m.ops.qfc_output_i16(m.dev(x8.astype(np.int16)), target, rows, d, None, tables, None, -32768, 32767)
    got = m.ops.qfc_output(m.dev(x8), 0, target, rows, d, None, mult, shift, 0, -100, 90)
    assert np.array_equal(got.cpu().numpy(), OC.output_i8(x8, 0, qw, None, mult, shift, 0, -100, 90))
    x16 = rng.integers(-32768, 32767, size=(n, d), endpoint=True).astype(np.int16)
    b64 = rng.integers(-(1 << 24), 1 << 24, size=rows).astype(np.int64)
    ms16 = [OC.quantize_multiplier(v[0] * 2.0 ** (v[1] - 31)) for v in ms]
    got = m.ops.qfc_output_i16(m.dev(x16), target, rows, d, m.dev(b64), mult, shift, -32768, 32767)
    assert got.dtype == m.torch.int16 and ms16 == ms
    assert np.array_equal(got.cpu().numpy(), OC.output_i16(x16, qw, b64, mult, shift, -32768, 32767))
  with pytest.raises(ValueError, match="multiplier is outside"):
    m.ops.qfc_output(m.dev(x8), 0, target, rows, d, None, [-1], [0], 0, -128, 127)
  with pytest.raises(ValueError, match=r"shift is outside \[-31, 14\]"):
    m.ops.qfc_output_i16(m.dev(x16), target, rows, d, None, [1 << 30], [15], -32768, 32767)
  with pytest.raises(TypeError, match="bias must be int32"):
    m.ops.qfc_output(m.dev(x8), 0, target, rows, d, b64, mult, shift, 0, -128, 127)
  with pytest.raises(TypeError, match="expected an int8"):
    m.ops.qfc_output(m.dev(x16), 0, target, rows, d, None, mult, shift, 0, -128, 127)
  blockwise = m.ops.CompareTarget(target.data, rows * d, kind, m.dev(np.ones(rows * d // 32, np.float32)), None, rows * d // 32, 32, 32)
  with pytest.raises(ValueError, match="one accumulator per output"):
    m.ops.qfc_output(m.dev(x8), 0, blockwise, rows, d, None, mult, shift, 0, -128, 127)


# ---------------------------------------------------------------- 2. end to end
@pytest.fixture(scope="module", params=[8, 16])
def chain(m, request):
  from mi355q import quantizer, recipe
  from mi355q.utils import tfl_flatbuffer_utils
  bits = request.param
  model = OC.build_model()
  samples = OC.build_samples(model)
  qz = quantizer.Quantizer(model, recipe.static_wi8_ai16() if bits == 16 else recipe.static_wi8_ai8())
  res = qz.quantize(qz.calibrate({"serving_default": samples}))
  return dict(bits=bits, float=model, samples=samples, qz=qz, model=tfl_flatbuffer_utils.read_model(bytes(res.quantized_model)),
              cmp=qz.validate_layer_execution({"serving_default": samples}, int16_activations=True, quantized_outputs=True))


def _numpy_chain(chain, name, rows, fused, has_bias):
  """(error, bound, per-channel error, per-channel bound, signal, outputs at act_min / act_max) of one op from the
  written model and the samples. q_out of the device chain is exact, so the only inexact device step is the FP32 reference
  Y = act(fl(X W^T) + b): a product of d terms, one addition of the bias, within
  eps[t, r] = (d + 3) 2^-24 (Sum_k |x| |w| + |b|) of the float64 value to first order; the activations are
  1-Lipschitz, so the bound holds through them, and |error - ref| <= (1/n) Sum (2 |yq - y64| eps + eps^2)."""
  import test_gpu_layer_execution as G8
  bits, qm = chain["bits"], chain["model"]
  sg = qm.subgraphs[0]
  fc = next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == f"{name}/y")
  x_t, y_t = sg.tensors[fc.inputs[0]], sg.tensors[fc.outputs[0]]
  from mi355q import schema
  act_type = int(schema.TensorType.INT16 if bits == 16 else schema.TensorType.INT8)
  assert int(x_t.type) == act_type and int(y_t.type) == act_type
  assert len(x_t.quantization.scale) == 1 and len(y_t.quantization.scale) == 1
  assert int(fc.builtinOptions.fusedActivationFunction) == fused

  def zero_point(t):
    return int(t.quantization.zeroPoint[0]) if t.quantization.zeroPoint is not None and len(t.quantization.zeroPoint) else 0
  s_x, zp_x, s_y, zp_y = np.float32(x_t.quantization.scale[0]), zero_point(x_t), np.float32(y_t.quantization.scale[0]), zero_point(y_t)
  qw, s_w, block = G8._written_weight(qm, f"{name}/w", rows, OC.D)      # pylint: disable=protected-access
  assert block == 0 and s_w.size in (1, rows)
  bias = None
  if has_bias:
    b_t = sg.tensors[fc.inputs[2]]
    assert int(b_t.type) == int(schema.TensorType.INT64 if bits == 16 else schema.TensorType.INT32)
    bias = np.asarray(qm.buffers[b_t.buffer].data).view(np.int64 if bits == 16 else np.int32)[:rows]
  else:
    assert len(fc.inputs) < 3 or fc.inputs[2] < 0
  ms = [OC.quantize_multiplier(float(s_x) * float(v) / float(s_y)) for v in s_w.tolist()]
  mult, shift = [v[0] for v in ms], [v[1] for v in ms]
  lo, hi = OC.activation_range(fused, float(s_y), zp_y, bits)
  x = np.concatenate([s[f"{name}/x"].reshape(-1, OC.D) for s in chain["samples"]], axis=0).astype(np.float32)
  n = x.shape[0]
  if bits == 16:
    assert zp_x == 0 and zp_y == 0
    xq = EC16.quantize_static16(x, s_x)
    q = OC.output_i16(xq, qw, bias, mult, shift, lo, hi)
  else:
    xq = EC.quantize_static(x, s_x, zp_x)
    q = OC.output_i8(xq, zp_x, qw, bias, mult, shift, zp_y, lo, hi)
  yq = ((q.astype(np.int32) - zp_y).astype(np.float32) * s_y).astype(np.float64)
  w64 = OC.constant(chain["float"], f"{name}/w").astype(np.float64)
  b64 = OC.constant(chain["float"], f"{name}/b").astype(np.float64) if has_bias else np.zeros(rows)
  lin = x.astype(np.float64) @ w64.T
  y64 = OC.float_activation(lin + b64, fused)
  eps = (OC.D + 3) * LC.U * (np.abs(x).astype(np.float64) @ np.abs(w64).T + np.abs(b64))
  diff = yq - y64
  per_channel = (diff ** 2).sum(axis=0) / n
  per_channel_bound = (2.0 * np.abs(diff) * eps + eps ** 2).sum(axis=0) / n
  clamps = (int((q == lo).sum()), int((q == hi).sum()))
  return per_channel.sum(), per_channel_bound.sum(), per_channel, per_channel_bound, (y64 ** 2).sum() / n, clamps


def test_every_static_op_matches_the_statement_run_on_the_written_model(chain):
  cmp_, bits = chain["cmp"], chain["bits"]
  assert cmp_.skipped == {} and list(cmp_) == [f"{n}/y" for n, *_ in OC.OPS]
  for name, rows, fused, has_bias in OC.OPS:
    r = cmp_[f"{name}/y"]
    error, bound, per_channel, per_channel_bound, signal, clamps = _numpy_chain(chain, name, rows, fused, has_bias)
    worst = float(np.max(np.abs(r["final_per_channel_error"] - per_channel) / per_channel_bound))
    print(f"a{bits}w8 {name} ({OC.NAMES[fused]}{', bias' if has_bias else ''}): pre-bias error {r['error']:.6e} SNR"
          f" {r['output_snr']:.1f}; final error {r['final_error']:.6e} signal {r['final_signal']:.6e} SNR"
          f" {r['final_output_snr']:.1f}; |final_error - ref| / bound {abs(r['final_error'] - error) / bound:.3e}, per channel"
          f" worst {worst:.3e}; outputs at act_min / act_max {clamps}")
    assert "final_skipped" not in r and (r["weight"], r["input"], r["rows"], r["d"]) == (f"{name}/w", f"{name}/x", rows, OC.D)
    assert r["tokens"] == sum(OC.TOKENS) and r["mode"] == "static"
    assert r["output_bits"] == r["activation_bits"] == bits and r["fused_activation"] == OC.NAMES[fused]
    assert abs(r["final_error"] - error) <= bound
    assert np.all(np.abs(r["final_per_channel_error"] - per_channel) <= per_channel_bound)
    assert r["final_per_channel_error"].dtype == np.float64 and r["final_per_channel_error"].shape == (rows,)
    np.testing.assert_allclose(r["final_signal"], signal, rtol=1e-5)
    np.testing.assert_allclose(r["final_error"], float(np.sum(r["final_per_channel_error"])), rtol=1e-12)
    assert r["final_output_mse"] == r["final_error"] / rows
    assert r["final_output_snr"] == (r["final_signal"] / rows) / (r["final_output_mse"] + 1e-9)
    assert 0 < r["final_error"] < r["final_signal"]
    if fused == OC.RELU6 and bits == 8:
      assert clamps[0] > 10 and clamps[1] > 10      # the integer range clamps at both ends
  free = cmp_["fc3/y"]      # no bias, no activation: what the output grid adds is all that separates the two figures
  assert free["final_error"] > free["error"]


def test_device_resident_samples_give_identical_bits(chain, m):
  resident = [{k: m.dev(v) for k, v in s.items()} for s in chain["samples"]]
  got = chain["qz"].validate_layer_execution(resident, signature_key="serving_default", int16_activations=True,
                                             quantized_outputs=True)
  want = chain["cmp"]
  assert got.skipped == {} and list(got) == list(want)
  for y, r in want.results.items():
    for key in ("error", "signal", "tokens", "final_error", "final_signal", "output_bits", "fused_activation"):
      assert got[y][key] == r[key], (y, key)
    for key in ("per_channel_error", "final_per_channel_error"):
      assert np.array_equal(got[y][key].view(np.uint64), r[key].view(np.uint64)), (y, key)


def test_the_plain_call_is_unchanged_and_a_dynamic_recipe_has_no_output_bits(chain):
  from mi355q import quantizer, recipe
  plain = chain["qz"].validate_layer_execution({"serving_default": chain["samples"]}, int16_activations=True)
  for y, r in plain.results.items():
    assert "output_bits" not in r and not [k for k in r if k.startswith("final") or k == "fused_activation"]
    for k, v in r.items():
      assert np.array_equal(chain["cmp"][y][k], v), (y, k)
  if chain["bits"] == 8:
    qz = quantizer.Quantizer(chain["float"], recipe.dynamic_wi8_afp32())
    qz.quantize()
    got = qz.validate_layer_execution({"serving_default": chain["samples"]}, quantized_outputs=True)
    assert len(got) == 4 and not got.skipped
    for r in got.results.values():
      assert r["mode"] == "dynamic" and r["output_bits"] is None
      assert not [k for k in r if k.startswith("final") or k == "fused_activation"]
