"""Every launch route of the fused symmetric requantization (csrc/requant.hip, csrc/requant_kernels.h) -- the rows
kernels, the groups kernels, the generic kernel, the single form, the device-table form and the host-table form --
against the NumPy oracle, bit for bit: scales as uint32 patterns, integers, packed bytes and f16 scale patterns.

Which kernel a call reaches is decided on the host (launch_bits()); route() below restates that choice and every case
carries the route it is there for in its id. The data are designed so that one wrong lane, tile border or rounding case
changes a scale or an integer: the maximum of every row / group is planted at a position that sweeps with its index
(negative in every other one), quotients sit on rint ties and past both clip bounds, and scales are driven to 0, inf
and NaN. Outputs are pre-filled and followed by guard bytes that must stay as they were."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from oracle import aeq_oracle as O

pytestmark = pytest.mark.gpu

BITS = [8, 4, 2]
FILL = 0xA5          # what every output byte holds before a call
GUARD = 64           # bytes behind every output that no kernel may touch
FLT_MAX = np.float32(3.4028235e38)
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]     # np.clip hands back -clip: the sign shows in the scale
NAN_PAYLOAD = np.array([0xFFC12345], np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  import __graft_entry__ as g
  g.build()
  import types
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib())


# ------------------------------------------------------------------------------------------------------- the routes ---
ROWS_SHAPES = [(64, "rows<64,1>"), (128, "rows<64,2>"), (256, "rows<64,4>"), (512, "rows<256,2>"),
               (1024, "rows<256,4>"), (2048, "rows<256,8>"), (4096, "rows<256,16>")]
ALL_ROUTES = {name for _, name in ROWS_SHAPES} | {f"groups<{g4}>" for g4 in (8, 16, 32, 64)} | {"generic_rows",
                                                                                               "generic_blocks"}


def route(rows, cols, block, bits, aligned=True):
  """launch_bits() of csrc/requant.hip, restated: the kernel one call reaches (the same for 8 / 4 / 2 bits)."""
  del rows, bits
  vec_ok = aligned and cols % 4 == 0
  if block > 0:
    return f"groups<{block // 4}>" if vec_ok and block in (32, 64, 128, 256) else "generic_blocks"
  if vec_ok:
    for limit, name in ROWS_SHAPES:
      if cols // 4 <= limit:
        return name
  return "generic_rows"


def rows_shape(cols):
  """(TPR, R) of the rows kernel that takes `cols` columns."""
  name = route(1, cols, 0, 8)
  tpr, r = name[5:-1].split(",")
  return int(tpr), int(r)


def case_id(rows, cols, block, bits, aligned=True, tag=""):
  return f"{route(rows, cols, block, bits, aligned)}-{rows}x{cols}-b{block}-int{bits}{tag}"


# ---------------------------------------------------------------------------------------------------- the reference ---
def qmax_of(bits):
  return 2 ** (bits - 1) - 1


def reference(w, block, bits, clip=None):
  """scale (float32, flat), q (int8 [rows, cols]), packed bytes and f16 scale patterns from the oracle."""
  rows, cols = w.shape
  with np.errstate(all="ignore"), warnings.catch_warnings():
    warnings.simplefilter("ignore")
    if block in (0, 32, 64, 128, 256):
      gran = "CHANNELWISE" if block == 0 else f"BLOCKWISE_{block}"
      if clip is None:
        ref = O.min_max_quant_params(w, bits, True, gran)
        scale, q = ref["scale"], ref["quantized_data"]
      else:
        qdim = O.weight_quantized_dim(gran)
        mm = O.init_tensor_min_max(w, gran, qdim)
        zp, scale = O.zp_scale_from_min_max(mm["min"], mm["max"], bits, True, gran,
                                            np.asarray(clip, np.float32).reshape(mm["min"].shape))
        q = O.uniform_quantize(w, scale, zp, bits, True, quantized_dim=qdim, block_size=block,
                               is_blockwise_quant=block > 0)
    else:   # not a granularity of the reference, but the ABI takes it: the reference's arithmetic on that block length
      assert clip is None
      bound = np.maximum(np.max(np.abs(w.reshape(rows, cols // block, block)), axis=2), np.float32(1e-9))
      scale = O.blockwise_scale_round(bound / np.float32(qmax_of(bits)))
      q = O.uniform_quantize(w, scale, np.zeros_like(scale, dtype=np.int8), bits, True, quantized_dim=1,
                             block_size=block, is_blockwise_quant=True)
    assert scale.dtype == np.float32 and q.dtype == np.int8
    out = {"scale": np.ascontiguousarray(scale).reshape(-1), "q": q.reshape(rows, cols)}
    flat = np.ravel(out["q"]).view(np.uint8)
    out["packed"] = O.pack_data(bits, flat) if bits < 8 else flat.copy()
    if block:
      out["s16"] = O.blockwise_scale_f16(scale).reshape(-1).view(np.uint16)
  return out


def same(got, want, what):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
  if not np.array_equal(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {bad[:6].tolist()}: "
                         f"{got.reshape(-1)[bad[:6]].tolist()} vs {want.reshape(-1)[bad[:6]].tolist()}")


def check(got, ref, what=""):
  """Every output the call was asked for, against the oracle's."""
  same(got["scale"].view(np.uint32), ref["scale"].view(np.uint32), f"{what} scale bits")
  for key in ("q", "packed", "s16"):
    if got.get(key) is not None:
      same(got[key], ref[key], f"{what} {key}")


# --------------------------------------------------------------------------------------------------------- the call ---
class Out:
  """An output buffer of `nbytes` at `offset` bytes into an allocation, pre-filled, with GUARD bytes behind it."""

  def __init__(self, m, nbytes, offset=0):
    self.m, self.nbytes, self.offset = m, nbytes, offset
    self.full = m.torch.full((offset + nbytes + GUARD,), FILL, dtype=m.torch.uint8, device="cuda")
    assert self.full.data_ptr() % 16 == 0
    self.at = self.full.data_ptr() + offset

  def ptr(self):
    return ctypes.c_void_p(self.at)

  def read(self, dtype=np.uint8):
    """The bytes of the buffer; what lies in front of it and behind it must be as it was."""
    h = self.full.cpu().numpy()
    assert (h[:self.offset] == FILL).all() and (h[self.offset + self.nbytes:] == FILL).all(), "write outside the output"
    return h[self.offset:self.offset + self.nbytes].view(dtype)

  def untouched(self):
    return bool((self.full.cpu().numpy() == FILL).all())


def device_input(m, w, offset=0):
  """x on the device in an allocation of exactly its size (plus `offset` bytes in front of it)."""
  raw = np.ascontiguousarray(w, dtype=np.float32).reshape(-1).view(np.uint8)
  t = m.torch.empty((offset + raw.size,), dtype=m.torch.uint8, device="cuda")
  t[offset:].copy_(m.torch.from_numpy(raw))
  assert t.data_ptr() % 16 == 0
  return t, t.data_ptr() + offset


def n_scales(rows, cols, block):
  return rows * (cols // block) if block else rows


def run_single(m, w, block, bits, clip=None, want_q=True, want_packed=False, alias=False, want_s16=False,
               x_off=0, q_off=0, p_off=0):
  """mi355q_requant_sym_f32 through the C ABI. alias: packed_out == q_out (8 bits). Returns (status, outputs, buffers)."""
  rows, cols = w.shape
  n, ns = rows * cols, n_scales(rows, cols, block)
  keep, xp = device_input(m, w, x_off)
  cd = None if clip is None else m.torch.from_numpy(np.ascontiguousarray(clip, dtype=np.float32).reshape(-1)).cuda()
  bufs = {"scale": Out(m, ns * 4)}
  if want_q:
    bufs["q"] = Out(m, n, q_off)
  if want_packed and not alias:
    bufs["packed"] = Out(m, n * bits // 8, p_off)
  if want_s16:
    bufs["s16"] = Out(m, ns * 2)
  qp = bufs["q"].ptr() if want_q else None
  pp = qp if alias else (bufs["packed"].ptr() if want_packed else None)
  st = m.L.mi355q_requant_sym_f32(ctypes.c_void_p(xp), rows, cols, block, bits, m.rt.ptr(cd), qp, pp,
                                  bufs["scale"].ptr(), bufs["s16"].ptr() if want_s16 else None, m.rt.stream_ptr())
  m.torch.cuda.synchronize()
  del keep
  if st != 0:
    return st, None, bufs
  got = {"scale": bufs["scale"].read(np.float32)}
  if want_q:
    got["q"] = bufs["q"].read(np.int8).reshape(rows, cols)
  if want_packed and not alias:
    got["packed"] = bufs["packed"].read()
  if want_s16:
    got["s16"] = bufs["s16"].read(np.uint16)
  return st, got, bufs


def run_modes(m, w, block, bits, ref, clip=None, packed_ok=True):
  """q alone, q and packed, packed alone (q_out = NULL), and for 8 bits packed_out == q_out, in turn."""
  s16 = block > 0
  modes = [("q", dict(want_q=True))]
  if packed_ok:
    modes += [("q+packed", dict(want_q=True, want_packed=True)), ("packed only", dict(want_q=False, want_packed=True))]
    if bits == 8:
      modes.append(("packed_out == q_out", dict(want_q=True, want_packed=True, alias=True)))
  for name, kw in modes:
    st, got, _ = run_single(m, w, block, bits, clip=clip, want_s16=s16, **kw)
    assert st == 0, (name, st, m.L.mi355q_last_error())
    check(got, ref, name)


# --------------------------------------------------------------------------------------------------------- the data ---
def normal(seed, rows, cols):
  return np.random.default_rng(seed).standard_normal((rows, cols), dtype=np.float32)


def row_positions(cols):
  """Columns for a planted row maximum: the first, the last, and for the rows kernel that takes this width one column
  in every R slot (lane's j-th float4 is float4 j * TPR + lane), walking through every wave of a 256-thread row."""
  tpr, r = rows_shape(cols) if cols % 4 == 0 and cols <= 16384 else (64, 1)
  cols4 = cols // 4
  pos = [0, cols - 1]
  for k in range(max(r, tpr // 64, 2)):
    j, wave = k % r, k % (tpr // 64)
    c4 = j * tpr + wave * 64 + (7 * k + 5) % 64
    if c4 < cols4:
      pos.append(4 * c4 + k % 4)
  pos += [min(cols - 1, 4 * (cols4 // 2) + 1)]
  return pos


def planted_rows(seed, rows, cols):
  """Normal data; row i has its extreme (+-(16 + i % 7), negative in odd rows) at row_positions(cols)[i % len]."""
  w = normal(seed, rows, cols)
  pos = row_positions(cols)
  for i in range(rows):
    w[i, pos[i % len(pos)]] = np.float32((16 + i % 7) * (-1 if i % 2 else 1))
  return w


def rows_for(cols):
  """A row count that is not a multiple of the rows per workgroup, spans several workgroups and reaches every
  planted position."""
  tpr, _ = rows_shape(cols)
  need = len(row_positions(cols))
  return max(67 if tpr == 64 else 5, need + 1 + need % 2)


def group_positions(block):
  """Offsets inside a group of `block` elements (block / 8 lanes of 8 elements share it): first and last element,
  last element of the first lane, first element of the last lane, and one that walks through the lanes."""
  return [0, block - 1, 7, block - 8]


def planted_groups(seed, rows, cols, block, big=None):
  """Normal data; flat group g has its extreme at an offset that sweeps with g, negative in odd groups."""
  w = normal(seed, rows, cols)
  flat = w.reshape(-1, block)
  pos = group_positions(block)
  lanes = block // 8
  for g in range(flat.shape[0]):
    at = pos[g % 5] if g % 5 < 4 else 8 * ((g // 5) % lanes) + (g // 5) % 8
    flat[g, at] = np.float32((16 + g % 7) * (-1 if g % 2 else 1))
    if big is not None and big[g]:
      flat[g, at] *= np.float32(2e6)     # 3.2e7 ... 4.4e7: above the f16 cap of every bit width
  return w


def row_clip(w):
  """A clip constant per row: below the maximum, above it, +inf, NaN, 0, in turn."""
  mx = np.max(np.abs(w), axis=1)
  kinds = [0.5, 2.0, np.inf, np.nan, 0.0, 0.25, 1.0, NEG_NAN]
  c = np.array([kinds[i % len(kinds)] for i in range(w.shape[0])], np.float32)
  with np.errstate(all="ignore"):
    c = np.where(np.isfinite(c) & (c > 0), c * mx, c).astype(np.float32)
  c[7::len(kinds)] = NEG_NAN     # (np.where may hand back another NaN than it was given)
  return c


# ----------------------------------------------------------------------------------------------------- rows kernels ---
ROWS_WIDTHS = [4, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196, 16384]
ROWS_CASES = [(rows, cols, 0, bits) for bits in BITS for cols in ROWS_WIDTHS for rows in (rows_for(cols), 1)]


@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: case_id(*c))
def test_rows_every_shape_both_edges(m, case):
  rows, cols, _, bits = case
  w = planted_rows(cols + bits, rows, cols)
  if rows == 1:
    w[0, 0], w[0, cols - 1] = np.float32(1.0), np.float32(-17.0)    # the extreme in the last float4 of the row
  run_modes(m, w, 0, bits, reference(w, 0, bits))


ROWS_CLIP_CASES = [(rows_for(cols), cols, 0, bits) for bits in BITS for cols in ROWS_WIDTHS]


@pytest.mark.parametrize("case", ROWS_CLIP_CASES, ids=lambda c: case_id(*c, tag="-clip"))
def test_rows_clip_per_row(m, case):
  rows, cols, _, bits = case
  w = planted_rows(3 * cols + bits, rows, cols)
  clip = row_clip(w)
  run_modes(m, w, 0, bits, reference(w, 0, bits, clip), clip=clip)


# --------------------------------------------------------------------------------------------------- groups kernels ---
BLOCKS = [32, 64, 128, 256]
# A tile is 256 lanes x U x CL x 4 elements: 4096 for int8 (U = 2), 2048 for 4 / 2 bits.
GROUP_SHAPES = [(3, 256),     # 768: less than one tile
                (1, 256),     # one row: a single group for block 256
                (13, 768),    # 9984: two (int8) / four tiles and 1792 elements of the next
                (5, 1024),    # 5120: int8's second workgroup has 1024 elements in its first tile and none in its second
                (6, 1024),    # 6144: int8's second workgroup has a full first tile and an empty second one
                (7, 1280)]    # 8960: int8's third workgroup holds 768 elements; 4 / 2 bits: 4 tiles + 768
GROUP_CASES = [(rows, cols, block, bits) for bits in BITS for block in BLOCKS for rows, cols in GROUP_SHAPES]


@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: case_id(*c))
def test_groups_every_g4_multi_block_and_partial_tiles(m, case):
  rows, cols, block, bits = case
  w = planted_groups(rows * cols + block + bits, rows, cols, block)
  run_modes(m, w, block, bits, reference(w, block, bits))


def f16_cap(bits):
  return 65280.0 * (2 ** bits - 1)


GROUP_CLIP_CASES = [(rows, cols, block, bits) for bits in BITS for block in BLOCKS for rows, cols in ((13, 768), (3, 256))]


@pytest.mark.parametrize("case", GROUP_CLIP_CASES, ids=lambda c: case_id(*c, tag="-clip"))
def test_groups_clip_per_block(m, case):
  """Clip constants NaN, +inf, 0, below and above the block maximum, and the f16 range cap reached: there both the
  clip and the block's own maximum lie above 65280 * (2^bits - 1), since the bound is clip(max|x|, -c, c)."""
  rows, cols, block, bits = case
  ng = rows * cols // block
  kinds = [np.nan, np.inf, 0.0, 0.5, 2.0, "cap_inf", "cap_1e8", "big_small_clip", NEG_NAN]
  kind = [kinds[(g + 5) % len(kinds)] for g in range(ng)]     # the capped ones first: 3 blocks reach them
  big = np.array([isinstance(k, str) for k in kind])
  w = planted_groups(7 * rows + block + bits, rows, cols, block, big=big)
  mx = np.max(np.abs(w.reshape(ng, block)), axis=1)
  assert (mx[big] > f16_cap(8)).all()
  clip = np.empty(ng, np.float32)
  for g, k in enumerate(kind):
    clip[g] = {"cap_inf": np.inf, "cap_1e8": 1e8, "big_small_clip": 3.0}[k] if isinstance(k, str) else (
        k * mx[g] if np.isfinite(k) and k > 0 else k)
  assert (clip.view(np.uint32) == 0xFFC00000).sum() == sum(1 for k in kind if not isinstance(k, str) and np.signbit(k))
  ref = reference(w, block, bits, clip)
  with np.errstate(all="ignore"):     # (8 bits: 65280 * 255 / 127 is itself beyond f16, the scale is inf)
    cap_scale = O.blockwise_scale_round(np.float32(f16_cap(bits)) / np.float32(qmax_of(bits)))
  capped = [g for g, k in enumerate(kind) if k in ("cap_inf", "cap_1e8")]
  assert capped and (ref["scale"][capped] == cap_scale).all()     # the cap is what these blocks' scales come from
  run_modes(m, w, block, bits, ref, clip=clip)


# ----------------------------------------------------------------------------------------------- fast-path rounding ---
def with_ulps(rng, x):
  return (x.view(np.int32) + rng.integers(-3, 4, size=x.shape).astype(np.int32)).view(np.float32)


def tie_fraction(w, scale_full, bits):
  """Share of the elements whose quotient lies within the kernel's guard distance of a half-integer, and share
  whose quotient lies beyond qmax + 2."""
  with np.errstate(all="ignore"):
    t = w.astype(np.float64) / scale_full.astype(np.float64)
  near = np.abs(np.abs(t - np.rint(t)) - 0.5) < 3.2e-5
  return float(near.mean()), float((np.abs(t) > qmax_of(bits) + 2).mean())


TIE_CASES = [(16, 4 * block, block, bits) for bits in BITS for block in BLOCKS]


@pytest.mark.parametrize("case", TIE_CASES, ids=lambda c: case_id(*c, tag="-ties"))
def test_half_integer_quotients_inside_the_range(m, case):
  """The 4 / 2-bit groups kernels divide once per block and multiply by the reciprocal, going back to the IEEE division
  near half-integer quotients (8 bits divides every element: the control). Quotients k + 0.5 with -3 ... +3 ulps,
  k in [-qmax, qmax - 1], everywhere except at the block maxima, which stay where they are."""
  rows, cols, block, bits = case
  rng = np.random.default_rng(block * bits)
  w = normal(block + bits, rows, cols)
  ref = reference(w, block, bits)
  scale_full = np.repeat(ref["scale"].reshape(rows, cols // block), block, axis=1)
  block_max = np.repeat(np.abs(w).reshape(rows, cols // block, block).max(axis=2), block, axis=1)
  k = rng.integers(-qmax_of(bits), qmax_of(bits), size=w.shape).astype(np.float32)
  planted = with_ulps(rng, ((k + np.float32(0.5)) * scale_full).astype(np.float32))
  keep = (np.abs(w) == block_max) | (np.abs(planted) >= block_max)
  w2 = np.where(keep, w, planted).astype(np.float32)
  ref2 = reference(w2, block, bits)
  assert np.array_equal(ref2["scale"], ref["scale"])     # maxima untouched
  near, _ = tie_fraction(w2, scale_full, bits)
  assert near > 0.9, near
  run_modes(m, w2, block, bits, ref2)


@pytest.mark.parametrize("case", TIE_CASES, ids=lambda c: case_id(*c, tag="-ties-clip"))
def test_half_integer_quotients_across_both_clip_bounds(m, case):
  """A clip constant per block in [0.5, 1.5), far below the block's maximum (one element of 1e3), makes the scale: the
  quotients k + 0.5 with -3 ... +3 ulps run from qmin - 3 to qmax + 3, across both clip bounds and across the
  |t| > qmax + 2 shortcut of the reciprocal path."""
  rows, cols, block, bits = case
  rng = np.random.default_rng(1000 + block * bits)
  ng = rows * cols // block
  clip = rng.uniform(0.5, 1.5, ng).astype(np.float32)
  w = (normal(block * bits, rows, cols) * np.float32(0.1)).astype(np.float32)
  flat = w.reshape(ng, block)
  at = (np.arange(ng) * 5) % block
  flat[np.arange(ng), at] = np.where(np.arange(ng) % 2 == 0, 1e3, -1e3).astype(np.float32)
  ref = reference(w, block, bits, clip)
  scale_full = np.repeat(ref["scale"].reshape(rows, cols // block), block, axis=1)
  lo = -qmax_of(bits) - 1
  k = rng.integers(lo - 3, qmax_of(bits) + 3, size=w.shape).astype(np.float32)     # k + 0.5 in [qmin - 2.5, qmax + 2.5]
  k = np.where(rng.integers(0, 8, size=w.shape) == 0, k + np.sign(k) * 2, k)       # ... and some farther out still
  planted = with_ulps(rng, ((k + np.float32(0.5)) * scale_full).astype(np.float32))
  is_big = np.abs(w) == np.float32(1e3)
  w2 = np.where(is_big, w, planted).astype(np.float32)
  ref2 = reference(w2, block, bits, clip)
  assert np.array_equal(ref2["scale"], ref["scale"])     # the clip makes the scale, before and after
  near, beyond = tie_fraction(w2, scale_full, bits)
  print(f"near a tie: {near:.3f}, beyond qmax + 2: {beyond:.3f}")
  assert near > 0.9 and beyond > (0.15 if bits < 8 else 0.01), (near, beyond)
  assert ref2["q"].min() == (-127 if bits == 8 else lo) and ref2["q"].max() == qmax_of(bits)
  run_modes(m, w2, block, bits, ref2, clip=clip)


SPARSE_TIE_CASES = [(128, 4096, block, bits) for bits in BITS for block in BLOCKS]


@pytest.mark.parametrize("case", SPARSE_TIE_CASES, ids=lambda c: case_id(*c, tag="-sparse-ties"))
def test_one_near_tie_per_wave(m, case):
  """The reciprocal path decides per wave: one lane near a tie sends all 64 to the division, so where ties are dense a
  kernel without a guard is right by accident. Here a wave (512 consecutive elements) holds ONE quotient k + 0.5 with
  -2 ... +2 ulps; the test first shows, in float32 NumPy, that rint(x * (1 / s)) gets several of them wrong."""
  rows, cols, block, bits = case
  rng = np.random.default_rng(77 + block * bits)
  w = normal(3 * block + bits, rows, cols)
  ref = reference(w, block, bits)
  scale_full = np.repeat(ref["scale"].reshape(rows, cols // block), block, axis=1).reshape(-1)
  block_max = np.repeat(np.abs(w).reshape(-1, block).max(axis=1), block)
  flat = w.reshape(-1).copy()
  at = np.arange(0, flat.size, 512) + (np.arange(flat.size // 512) * 37) % 512
  k = rng.integers(-qmax_of(bits), qmax_of(bits), size=at.size).astype(np.float32)
  planted = ((k + np.float32(0.5)) * scale_full[at]).astype(np.float32)
  planted = (planted.view(np.int32) + rng.integers(-2, 3, size=at.size).astype(np.int32)).view(np.float32)
  ok = (np.abs(flat[at]) != block_max[at]) & (np.abs(planted) < block_max[at])
  flat[at[ok]] = planted[ok]
  w2 = flat.reshape(rows, cols)
  ref2 = reference(w2, block, bits)
  assert np.array_equal(ref2["scale"], ref["scale"])     # maxima untouched
  lo = -127 if bits == 8 else -qmax_of(bits) - 1
  naive = np.clip(np.rint(flat * (np.float32(1) / scale_full)), lo, qmax_of(bits)).astype(np.int8)
  wrong = int((naive[at[ok]] != ref2["q"].reshape(-1)[at[ok]]).sum())
  print(f"{int(ok.sum())} planted, an unguarded reciprocal gets {wrong} of them wrong")
  assert wrong >= 8, wrong
  run_modes(m, w2, block, bits, ref2)


# --------------------------------------------------------------------------------------------------- scale extremes ---
def extreme_tensor(seed, cols, block):
  """Rows (and, blockwise, the blocks of a row) that are: zero with a -0.0; subnormal (the bound floors at 1e-9 and a
  blockwise scale rounds to zero in f16); holding +-FLT_MAX (a blockwise scale rounds to inf, 1 / s is 0); scaled by
  3e4, 1e6 (f16 overflow) and 1e-6 (f16-subnormal scales); holding one NaN, one +inf, one -inf; and ordinary."""
  w = normal(seed, 11, cols)
  g = max(block, 1)
  nb = cols // g if block else 1
  span = block if block else cols
  w[0, :] = 0
  w[0, 5 % cols] = np.float32(-0.0)
  w[1, :] = (w[1, :].astype(np.float64) * 1e-42).astype(np.float32)
  w[3, :] *= np.float32(3e4)
  w[4, :] *= np.float32(1e-6)
  w[5, :] *= np.float32(1e6)
  for b in range(nb):
    at = b * span + (3 * b + 1) % span
    w[2, at] = FLT_MAX if b % 2 == 0 else -FLT_MAX
    if b % 2 == 0 or nb == 1:
      w[6, at] = NAN_PAYLOAD if block and b % 4 == 2 else np.nan     # the bfloat16 step drops a NaN's sign and payload
    w[7, at] = np.inf if b % 3 != 1 else w[7, at]
    w[8, at] = -np.inf if b % 3 != 2 else w[8, at]
  w[9, cols - 1] = np.nan          # NaN in the last element, -inf in the first
  w[9, 0] = -np.inf
  return w


EXTREME_CASES = ([(11, cols, 0, bits) for bits in BITS for cols in (512, 2052, 16384, 33)] +
                 [(11, 512, block, bits) for bits in BITS for block in BLOCKS] +
                 [(11, 96, 48, bits) for bits in BITS])


@pytest.mark.parametrize("case", EXTREME_CASES, ids=lambda c: case_id(*c, tag="-extremes"))
def test_scale_extremes(m, case):
  rows, cols, block, bits = case
  w = extreme_tensor(cols + block + bits, cols, block)
  ref = reference(w, block, bits)
  s = ref["scale"]
  assert np.isnan(s).any() and np.isinf(s).any()                 # the oracle has an answer for each of them
  if block:
    assert (s == 0).any()
  run_modes(m, w, block, bits, ref, packed_ok=route(*case) not in ("generic_rows", "generic_blocks") or bits == 8)


# --------------------------------------------------------------------------------------------------- generic routes ---
GENERIC_CASES = ([(rows, cols, 0, bits) for bits in BITS for rows, cols in ((5, 3), (5, 33), (3, 4099), (2, 16388), (2, 20000))] +
                 [(6, cols, block, bits) for bits in BITS for cols, block in ((36, 12), (96, 48), (192, 96), (960, 96))])


@pytest.mark.parametrize("case", GENERIC_CASES, ids=lambda c: case_id(*c))
def test_generic_routes(m, case):
  """cols % 4 != 0, cols > 16384 and block sizes outside {32, 64, 128, 256}. Sub-byte packing is refused there before
  anything is launched; 8-bit `packed_out` is the same bytes as q_out on every route."""
  rows, cols, block, bits = case
  assert route(*case) in ("generic_rows", "generic_blocks")
  w = planted_groups(cols + bits, rows, cols, block) if block else planted_rows(cols + bits, rows, cols)
  ref = reference(w, block, bits)
  run_modes(m, w, block, bits, ref, packed_ok=bits == 8)
  if bits < 8 and (rows * cols) % (8 // bits) == 0:
    st, _, bufs = run_single(m, w, block, bits, want_q=True, want_packed=True, want_s16=block > 0)
    assert st == -3 and b"packed output needs" in m.L.mi355q_last_error()
    assert all(b.untouched() for b in bufs.values())


ALIGN_CASES = [(rows, cols, block, bits) for bits in BITS
               for rows, cols, block in ((67, 252, 0), (5, 2052, 0), (13, 768, 32), (13, 768, 256))]


@pytest.mark.parametrize("case", ALIGN_CASES, ids=lambda c: case_id(*c, aligned=False, tag="-offset4"))
def test_four_byte_offsets_take_the_generic_kernel(m, case):
  """The inputs of an aligned route again with x, then q_out, then (8 bits) packed_out 4 bytes past a 16-byte
  boundary: same results. A sub-byte packed_out cannot be produced there: UNSUPPORTED and nothing written."""
  rows, cols, block, bits = case
  w = planted_groups(cols + bits, rows, cols, block) if block else planted_rows(cols + bits, rows, cols)
  ref = reference(w, block, bits)
  s16 = block > 0
  st, aligned, _ = run_single(m, w, block, bits, want_s16=s16)
  assert st == 0
  check(aligned, ref, "aligned")
  offsets = [dict(x_off=4), dict(q_off=4), dict(x_off=4, q_off=4)]
  for off in offsets:
    st, got, _ = run_single(m, w, block, bits, want_s16=s16, **off)
    assert st == 0, (off, m.L.mi355q_last_error())
    check(got, ref, str(off))
    for key in aligned:
      same(got[key], aligned[key], f"{off} {key} against the aligned run")
  if bits == 8:
    for kw in (dict(want_q=True, p_off=4), dict(want_q=False, p_off=4), dict(want_q=True, x_off=4)):
      st, got, _ = run_single(m, w, block, bits, want_packed=True, want_s16=s16, **kw)
      assert st == 0, (kw, m.L.mi355q_last_error())
      check(got, ref, f"packed {kw}")
  else:
    for kw in (dict(x_off=4), dict(q_off=4), dict(p_off=4), dict(p_off=4, want_q=False)):
      kw = {"want_q": True, **kw}
      st, _, bufs = run_single(m, w, block, bits, want_packed=True, want_s16=s16, **kw)
      assert st == -3 and b"packed output needs" in m.L.mi355q_last_error(), (kw, st)
      assert all(b.untouched() for b in bufs.values()), kw


# ------------------------------------------------------------------------------------------------------ batched forms ---
FAMILIES = {                      # rows, cols, block
    "rows_tpr64": (3, 36, 0),     # slices of 108 (int8), 54 (int4) and 27 (int2) bytes: steps that are no multiple of 16
    "rows_tpr256": (2, 1028, 0),
    "groups": (5, 1024, 128),     # int8: two workgroups per tensor, the second one's second tile empty
    "groups_small": (3, 96, 32),  # less than a tile per tensor; packed slices of 144 / 72 bytes
    "generic_rows": (3, 33, 0),
    "generic_blocks": (3, 36, 12),
}
MAX_COUNT = 33
# ... and every other kernel shape once in each batched form, three tensors each
SHAPE_FAMILIES = {f"shape_{r}x{c}_b{b}": (r, c, b) for r, c, b in
                  [(3, 260, 0), (3, 516, 0), (2, 2052, 0), (2, 4100, 0), (2, 8196, 0), (13, 768, 64), (13, 768, 256)]}
FAMILIES.update(SHAPE_FAMILIES)


@functools.lru_cache(maxsize=None)
def batch_data(family, bits):
  """33 tensors of the family's shape (3 for a shape family), each with a seed and planted extremes of its own, and
  their references."""
  rows, cols, block = FAMILIES[family]
  ws, refs = [], []
  for i in range(3 if family in SHAPE_FAMILIES else MAX_COUNT):
    seed = 1000 * (i + 1) + bits
    w = planted_groups(seed, rows, cols, block) if block else planted_rows(seed, rows, cols)
    w[i % rows, (11 * i + 3) % cols] = np.float32((40 + i) * (-1 if i % 2 else 1))   # a scale only tensor i has
    ws.append(w)
    refs.append(reference(w, block, bits))
  return ws, refs


def run_batched(m, family, bits, count, form, want):
  """`count` tensors through one of the batched entry points, outputs laid out as requant_queue._launch lays them out:
  consecutive slices of one allocation per kind of output. want: "q" (packed table NULL) or "packed" (q table NULL)."""
  rows, cols, block = FAMILIES[family]
  ws, refs = batch_data(family, bits)
  n, ns = rows * cols, n_scales(rows, cols, block)
  out_bytes = n if want == "q" else n * bits // 8
  xs = [device_input(m, w) for w in ws[:count]]
  out = Out(m, count * out_bytes)
  scale = Out(m, count * ns * 4)
  s16 = Out(m, count * ns * 2) if block else None
  steps = np.arange(count, dtype=np.int64)
  tables = {"x": [p for _, p in xs], "out": (out.at + steps * out_bytes).tolist(),
            "scale": (scale.at + steps * ns * 4).tolist(),
            "s16": (s16.at + steps * ns * 2).tolist() if block else None}
  if form == "hostptrs":
    arr = ctypes.c_void_p * count
    t = {k: None if v is None else arr(*v) for k, v in tables.items()}
    st = m.L.mi355q_requant_sym_f32_batched_hostptrs(
        t["x"], count, rows, cols, block, bits, t["out"] if want == "q" else None,
        t["out"] if want == "packed" else None, t["scale"], t["s16"], m.rt.stream_ptr())
  else:
    dt = {k: None if v is None else m.torch.tensor(v, dtype=m.torch.int64).cuda() for k, v in tables.items()}
    st = m.L.mi355q_requant_sym_f32_batched(
        m.rt.ptr(dt["x"]), count, rows, cols, block, bits, m.rt.ptr(dt["out"]) if want == "q" else None,
        m.rt.ptr(dt["out"]) if want == "packed" else None, m.rt.ptr(dt["scale"]), m.rt.ptr(dt["s16"]),
        m.rt.stream_ptr())
  m.torch.cuda.synchronize()
  if st != 0:
    return st, (out, scale, s16)
  got_out = out.read(np.int8 if want == "q" else np.uint8).reshape(count, -1)
  got_scale = scale.read(np.uint32).reshape(count, ns)
  got_s16 = s16.read(np.uint16).reshape(count, ns) if block else None
  for i in range(count):
    same(got_scale[i], refs[i]["scale"].view(np.uint32), f"tensor {i} of {count}: scale bits")
    same(got_out[i], refs[i]["q"].reshape(-1) if want == "q" else refs[i]["packed"], f"tensor {i} of {count}: {want}")
    if block:
      same(got_s16[i], refs[i]["s16"], f"tensor {i} of {count}: f16 scale patterns")
  return st, None


BATCH_CASES = [(family, bits, form, count) for family in FAMILIES for bits in BITS
               for form, counts in (("hostptrs", (1, 5, 16, 17, 33)), ("tables", (1, 5, 33)))
               for count in ((3,) if family in SHAPE_FAMILIES else counts)]


def batch_id(c):
  family, bits, form, count = c
  return f"{route(*FAMILIES[family], bits)}-{family}-int{bits}-{form}-n{count}"


@pytest.mark.parametrize("case", BATCH_CASES, ids=batch_id)
def test_batched_forms(m, case):
  """Host tables (16 tensors per dispatch: counts 16, 17 and 33 cross the chunk border) and device tables. The q table
  alone, then the packed table alone; the generic kernel packs nothing below 8 bits and refuses before it launches."""
  family, bits, form, count = case
  generic = family.startswith("generic")
  st, _ = run_batched(m, family, bits, count, form, "q")
  assert st == 0, m.L.mi355q_last_error()
  rows, cols, _ = FAMILIES[family]
  if generic and bits < 8:
    if (rows * cols) % (8 // bits) == 0:
      st, bufs = run_batched(m, family, bits, count, form, "packed")
      assert st == -3 and b"packed output needs" in m.L.mi355q_last_error()
      assert all(b.untouched() for b in bufs if b is not None)
  else:
    st, _ = run_batched(m, family, bits, count, form, "packed")
    assert st == 0, m.L.mi355q_last_error()


@pytest.mark.parametrize("bits", BITS)
def test_requant_batch_object(m, bits):
  """ops.RequantBatch (what bench.py times): q, packed and f16 scales of every tensor in one device-table launch."""
  for family in ("rows_tpr256", "groups"):
    _, _, block = FAMILIES[family]
    ws, refs = batch_data(family, bits)
    b = m.ops.RequantBatch([m.torch.from_numpy(w).cuda() for w in ws[:5]], block, bits, want_q=True, want_packed=True,
                           want_scale_f16=True)
    b.run()
    for i in range(5):
      got = {"scale": b.scale[i].cpu().numpy().reshape(-1), "q": b.q[i].cpu().numpy(),
             "packed": b.packed[i].cpu().numpy().view(np.uint8),
             "s16": b.scale_f16[i].cpu().numpy().reshape(-1).view(np.uint16) if block else None}
      check(got, refs[i], f"{family} tensor {i}")


# ----------------------------------------------------------------------------------------------------- layer size ---
LAYER_CASES = ([(rows, cols, 0, bits) for rows, cols in ((4096, 4096), (2048, 16384)) for bits in BITS] +
               [(4096, cols, block, bits) for cols in (4096, 11008) for block in (32, 128) for bits in (8, 4)])


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: case_id(*c, tag="-layer"))
def test_layer_size_against_the_oracle_on_the_full_tensor(m, case):
  rows, cols, block, bits = case
  w = normal(rows + cols + block + bits, rows, cols)
  w[np.arange(rows), (np.arange(rows) * 37) % cols] *= np.float32(8)     # a row extreme whose column walks
  ref = reference(w, block, bits)
  st, got, _ = run_single(m, w, block, bits, want_q=True, want_packed=True, want_s16=block > 0)
  assert st == 0, m.L.mi355q_last_error()
  check(got, ref, "layer")


# --------------------------------------------------------------------------------------------------- route coverage ---
SINGLE_FORM_CASES = (ROWS_CASES + ROWS_CLIP_CASES + GROUP_CASES + GROUP_CLIP_CASES + TIE_CASES + SPARSE_TIE_CASES +
                     EXTREME_CASES +
                     GENERIC_CASES + LAYER_CASES)


def test_route_restates_launch_bits():
  assert [route(1, c, 0, 8) for c in (4, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196, 16384)] == [
      "rows<64,1>", "rows<64,1>", "rows<64,2>", "rows<64,2>", "rows<64,4>", "rows<64,4>", "rows<256,2>", "rows<256,2>",
      "rows<256,4>", "rows<256,4>", "rows<256,8>", "rows<256,8>", "rows<256,16>", "rows<256,16>"]
  assert route(1, 16388, 0, 4) == route(1, 6, 0, 4) == route(1, 512, 0, 4, aligned=False) == "generic_rows"
  assert [route(1, 768, b, 2) for b in (32, 64, 128, 256)] == ["groups<8>", "groups<16>", "groups<32>", "groups<64>"]
  assert route(1, 96, 48, 8) == route(1, 768, 128, 8, aligned=False) == "generic_blocks"
  assert len(ALL_ROUTES) == 13


@pytest.mark.parametrize("bits", BITS)
def test_every_single_form_route_is_reached(bits):
  """13 kernel shapes x 3 bit widths = 39 single-form routes; the alignment fall-backs reach the generic two again."""
  reached = {route(*c) for c in SINGLE_FORM_CASES if c[3] == bits}
  assert reached == ALL_ROUTES, sorted(ALL_ROUTES - reached)
  assert {route(*c, aligned=False) for c in ALIGN_CASES if c[3] == bits} == {"generic_rows", "generic_blocks"}
  assert {route(*FAMILIES[f], bits) for f in FAMILIES} == ALL_ROUTES     # each of them in both batched forms as well
