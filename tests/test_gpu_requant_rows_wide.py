"""The row-wise fused requantization around its 16-byte stores (csrc/requant_kernels.h: requant_rows_wide_kernel with
its wave-contiguous runs and the LDS exchange, taken at the exact fits of rows<256, 4>, <256, 8> and <256, 16>, and
requant_rows_kernel everywhere else), bit for bit against the NumPy oracle: scale as uint32, q, packed bytes.

Every rows route <TPR, R> at the exact fit 4 TPR R, at 4 TPR R - 4 (rows no multiple of 16 bytes), at 4 TPR R - 16
(16-byte rows, four columns short of the wide kernel) and just above the route's narrowest row (most lanes hold
nothing). Three rows per buffer, so a store past a row's end lands in a row that is itself compared; outputs are
pre-filled and followed by guard bytes. Output pointers at +0 and +8 bytes of a 16-byte boundary (8 bytes is all
include/mi355q.h asks of a table form), and one device-table launch whose tensors sit at +0, +8, +0: each tensor takes
its own branch between 16-byte stores and a word per store. The row maxima sweep through the first and the last lane
of every wave's run and of every load step, negative in odd rows; the scales are powers of two, and a few quotients
lie exactly on k + 0.5."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_requant_routes import BITS, Out, device_input, m, qmax_of, reference, rows_shape, same  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = 3
ROUTES = [(64, 1), (64, 2), (64, 4), (256, 2), (256, 4), (256, 8), (256, 16)]
OUTPUTS = [("q", True, False), ("packed", False, True), ("q+packed", True, True)]
TENSORS = 9          # per case: 3 single-form launches and 3 host-table launches of 2 tensors, each on data of its own


def narrowest(tpr, r):
  """The smallest `cols` that launch_bits() hands to rows<tpr, r>."""
  below = {(64, 1): 0, (64, 2): 64, (64, 4): 128, (256, 2): 256, (256, 4): 512, (256, 8): 1024, (256, 16): 2048}
  return 4 * (below[(tpr, r)] + 1)


def widths(tpr, r):
  full = 4 * tpr * r
  low = narrowest(tpr, r) + 16
  out = [full, full - 4, full - 16, low, (low + 15) // 16 * 16]     # (the last: the same with 16-byte rows)
  return [c for c in dict.fromkeys(out) if c >= narrowest(tpr, r)]


CASES = [(tpr, r, cols, bits) for tpr, r in ROUTES for cols in widths(tpr, r) for bits in BITS]


def case_id(c):
  tpr, r, cols, bits = c
  return f"rows<{tpr},{r}>-{ROWS}x{cols}-int{bits}"


def test_cases_reach_their_routes():
  for tpr, r, cols, _ in CASES:
    assert rows_shape(cols) == (tpr, r), (tpr, r, cols)
  assert {(t, r) for t, r, _, _ in CASES} == set(ROUTES)
  for tpr, r in ROUTES:
    assert 4 * tpr * r in widths(tpr, r) and 4 * tpr * r - 4 in widths(tpr, r) and 4 * tpr * r - 16 in widths(tpr, r)


# --------------------------------------------------------------------------------------------------------- the data ---
def sweep_positions(tpr, r, cols):
  """float4 indices for the row maximum: first and last float4 of every wave's contiguous run (lane 0 of its first
  load step, lane 63 of its last) -- a run is ceil(cols4 / 256) load steps of 64 float4 long when four waves share a
  row, and the borders of runs of R steps are in the list as well --, the row's last float4, then lanes 0 and 63 of
  every other load step; only those inside the row."""
  cols4 = cols // 4
  waves = tpr // 64
  ends, steps = [], []
  for run in sorted({64 * r, 64 * -(-cols4 // tpr)} if waves > 1 else {64 * r}):
    for w in range(waves):
      ends += [w * run, min((w + 1) * run, cols4) - 1]
      for j in range(run // 64):
        steps += [w * run + j * 64 + 63, w * run + j * 64]
  return [p for p in dict.fromkeys(ends + [cols4 - 1] + steps) if 0 <= p < cols4]


@functools.lru_cache(maxsize=None)
def case_data(tpr, r, cols, bits):
  """TENSORS buffers of ROWS rows and their references. Row n (counted through all buffers) has its maximum
  +-qmax * s, s a power of two, in float4 sweep[n % len]; three more elements are (k + 0.5) * s."""
  pos = sweep_positions(tpr, r, cols)
  assert TENSORS * ROWS >= min(len(pos), 4 * (tpr // 64) + 1), "the sweep passes through every wave's first and last lane"
  rng = np.random.default_rng(1000 * cols + bits)
  qmax = qmax_of(bits)
  s0 = 2.0 ** np.ceil(np.log2(8.0 / qmax))      # qmax * s0 >= 8: above every normal value
  ws, refs = [], []
  for t in range(TENSORS):
    w = rng.standard_normal((ROWS, cols), dtype=np.float32)
    for i in range(ROWS):
      n = t * ROWS + i
      s = np.float32(s0 * (1 + n % 2))
      at = 4 * pos[n % len(pos)] + n % 4
      for k in range(3):     # quotients on rint ties: near the row's start, its middle and its end
        tie = (k * (cols - 1) // 2 + 4 * n + k) % cols
        if tie != at:
          w[i, tie] = np.float32((int(rng.integers(-qmax, qmax)) + 0.5) * s)
      w[i, at] = np.float32(qmax * s * (-1 if n % 2 else 1))
    ref = reference(w, 0, bits)
    expect = np.array([s0 * (1 + (t * ROWS + i) % 2) for i in range(ROWS)], np.float32)
    assert np.array_equal(ref["scale"], expect)     # the planted element is the row's maximum
    ws.append(w)
    refs.append(ref)
  return ws, refs


# --------------------------------------------------------------------------------------------------------- the call ---
def launch(m, form, ws, refs, bits, want_q, want_packed, offsets):
  """One call on the tensors `ws` (single: one of them), tensor i's q and packed `offsets[i]` bytes past a 16-byte
  boundary; every requested output against refs[i], guard bytes included."""
  rows, cols = ws[0].shape
  n = rows * cols
  count = len(ws)
  xs = [device_input(m, w) for w in ws]
  q = [Out(m, n, off) for off in offsets] if want_q else None
  p = [Out(m, n * bits // 8, off) for off in offsets] if want_packed else None
  sc = [Out(m, rows * 4) for _ in ws]
  stream = m.rt.stream_ptr()
  if form == "single":
    assert count == 1
    st = m.L.mi355q_requant_sym_f32(ctypes.c_void_p(xs[0][1]), rows, cols, 0, bits, None, q[0].ptr() if q else None,
                                    p[0].ptr() if p else None, sc[0].ptr(), None, stream)
  elif form == "hostptrs":
    arr = ctypes.c_void_p * count
    tab = lambda outs: arr(*[o.at for o in outs]) if outs else None     # noqa: E731
    st = m.L.mi355q_requant_sym_f32_batched_hostptrs(arr(*[xp for _, xp in xs]), count, rows, cols, 0, bits, tab(q),
                                                     tab(p), tab(sc), None, stream)
  else:
    dev = lambda v: m.torch.tensor(v, dtype=m.torch.int64).cuda()     # noqa: E731
    keep = [dev([xp for _, xp in xs]), dev([o.at for o in q]) if q else None, dev([o.at for o in p]) if p else None,
            dev([o.at for o in sc])]
    st = m.L.mi355q_requant_sym_f32_batched(m.rt.ptr(keep[0]), count, rows, cols, 0, bits, m.rt.ptr(keep[1]),
                                            m.rt.ptr(keep[2]), m.rt.ptr(keep[3]), None, stream)
  m.torch.cuda.synchronize()
  assert st == 0, (form, st, m.L.mi355q_last_error())
  for i, ref in enumerate(refs):
    what = f"{form} tensor {i} at +{offsets[i]}"
    same(sc[i].read(np.uint32), ref["scale"].view(np.uint32), f"{what}: scale bits")
    if want_q:
      same(q[i].read(np.int8).reshape(rows, cols), ref["q"], f"{what}: q")
    if want_packed:
      same(p[i].read(), ref["packed"], f"{what}: packed")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_route_width_output_and_offset(m, case):
  """The single form (RequantArgs, direct pointers) at +0 and the host-table form (RequantInlineArgs) with one tensor
  at +0 and one at +8, for q alone, packed alone and both."""
  tpr, r, cols, bits = case
  ws, refs = case_data(tpr, r, cols, bits)
  for k, (_, want_q, want_packed) in enumerate(OUTPUTS):
    launch(m, "single", ws[3 * k:3 * k + 1], refs[3 * k:3 * k + 1], bits, want_q, want_packed, [0])
    launch(m, "hostptrs", ws[3 * k + 1:3 * k + 3], refs[3 * k + 1:3 * k + 3], bits, want_q, want_packed, [0, 8])


TABLE_CASES = [(tpr, r, 4 * tpr * r - 16, bits) for tpr, r in ROUTES for bits in BITS if 4 * tpr * r - 16 >= narrowest(tpr, r)]
TABLE_CASES += [(tpr, r, 4 * tpr * r, bits) for tpr, r in ROUTES for bits in BITS]


@pytest.mark.parametrize("case", TABLE_CASES, ids=case_id)
def test_device_table_tensors_at_0_8_0(m, case):
  """One device-table launch (RequantArgs, batched) of three tensors whose outputs sit at +0, +8 and +0 bytes: the
  middle one cannot take 16-byte stores, its neighbours can, and each tensor decides for itself."""
  tpr, r, cols, bits = case
  ws, refs = case_data(tpr, r, cols, bits)
  for k, (_, want_q, want_packed) in enumerate(OUTPUTS):
    launch(m, "tables", ws[k:k + 3], refs[k:k + 3], bits, want_q, want_packed, [0, 8, 0])
