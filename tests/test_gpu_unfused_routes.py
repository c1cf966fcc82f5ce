"""Every launch route of the non-fused kernels of elementwise.hip -- given-parameter quantize (K3), dequantize, weight
min / max (K1) and unpacking -- and the public functions that take them, against the oracle or plain NumPy, bit for bit.

Which kernel a call reaches is decided on the host (mi355q_quantize_f32 / _dequantize_f32 / _minmax_f32 / _unpack_bits);
every case names the route it is there for. The data are designed so that a subtly wrong kernel changes integers: every
channel has its own scale and zero point, quotients land on rint ties, values lie past both clip bounds, and NaN / +-inf
sit at the first and last element of a row and inside it."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import aeq_oracle as O

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  import __graft_entry__ as g
  g.build()
  import types
  from mi355q import _ffi, ops, qtyping
  from mi355q import runtime as rt
  from mi355q.algorithms.uniform_quantize import naive_min_max_quantize, uniform_quantize_tensor
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), check=_ffi.check, qtyping=qtyping,
                               mm=naive_min_max_quantize, uqt=uniform_quantize_tensor)


def dev(a):
  import torch
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
  return t.cpu().numpy()


def same_bits(got, want):
  """Same dtype, shape and bit patterns (NaN payloads included)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
  if got.dtype.kind == "f":
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(u) != want.view(u))
  else:
    bad = np.flatnonzero(got != want)
  assert bad.size == 0, (f"{bad.size} of {got.size} differ, first at {bad[:5].tolist()}: "
                         f"{got.reshape(-1)[bad[:5]].tolist()} vs {want.reshape(-1)[bad[:5]].tolist()}")


# --------------------------------------------------------------------------------------------------------------- K3 ---
SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], np.float32)


def channel_params(rng, ch, bits, zp_kind, f64):
  """A scale and a zero point of its own for every channel. Two channels in three have a scale with four significant
  bits (x = (k + 1/2) * s is then exact and x / s a rint tie); the third a scale no float32 holds when f64."""
  j = np.arange(ch)
  simple = np.ldexp(1.0 + (j % 8) / 8.0, -(j % 5) - 1)
  scale = np.where(j % 3 == 2, rng.uniform(0.01, 0.3, ch), simple).astype(np.float64 if f64 else np.float32)
  if zp_kind is None:
    return scale, None
  qmin, qmax = -2 ** (bits - 1), 2 ** (bits - 1) - 1
  span = 100 if zp_kind == np.int8 else 5000
  zp = rng.integers(max(qmin, -span), min(qmax, span) + 1, ch).astype(zp_kind)
  return scale, zp


def designed_x(rng, outer, ch, inner, scale, zp, bits):
  """Quotients x / s + zp on integers and on rint ties, reaching past both clip bounds (for up to 18 bits), plus
  NaN / +-inf / +-1e30 / -0.0 at the first, middle and last element of every row and at random places."""
  reach = int(min(1.25 * 2 ** (bits - 1), 2 ** 18))
  z = np.zeros(ch, np.int64) if zp is None else zp.astype(np.int64)
  k = rng.integers(-reach, reach + 1, (outer, ch, inner)) - z[None, :, None]
  half = rng.integers(0, 2, (outer, ch, inner)) * 0.5
  x = ((k + half) * scale.astype(np.float64)[None, :, None]).astype(np.float32)
  c = np.arange(ch)
  for at, turn in ((0, 0), (inner // 2, 2), (inner - 1, 1)):
    x[:, :, at] = SPECIALS[(c + turn) % SPECIALS.size][None, :]
  flat = x.reshape(-1)
  flat[rng.integers(0, flat.size, 32)] = SPECIALS[rng.integers(0, SPECIALS.size, 32)]
  return x


def quantize_ref(x, scale, zp, bits, narrow):
  """The reference's arithmetic on the [outer, channels, inner] view (narrow == symmetric for bits >= 8)."""
  ch = scale.size
  z = np.zeros((1, ch, 1), np.int32) if zp is None else zp.reshape(1, ch, 1)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    return O.uniform_quantize(x.reshape(-1, ch, x.shape[-1]), scale.reshape(1, ch, 1), z, bits, narrow).reshape(x.shape)


def run_quantize(m, x, outer, ch, inner, scale, zp, bits, narrow, misalign=False):
  if misalign:   # the tensor one float past a 16-byte boundary
    full = dev(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]))
    xd = full[1:]
    assert xd.data_ptr() % 16 == 4
  else:
    xd = dev(x.reshape(-1))
    assert xd.data_ptr() % 16 == 0
  zd = None if zp is None else dev(zp.astype(np.int32))
  q = m.ops.quantize(xd, outer, ch, inner, dev(scale), zd, bits, narrow,
                     zp_via_f64=zp is not None and zp.dtype.itemsize >= 4)
  return host(q).reshape(x.shape)


INT8_CONFIGS = [(2, False), (4, False), (8, False), (8, True)]   # (bits, narrow): every one in an int8 container
ZP_KINDS = [None, np.int8, np.int32]

QUANT_ROUTES = [
    # id,                 outer, ch, inner, misalign
    ("rows_1024", 1, 3, 1024, False),            # quantize_rows_vec4_kernel: one full piece of 1024 float4 per run
    ("rows_1028_outer", 3, 4, 1028, False),      # quantize_rows_vec4_kernel: outer > 1, channel = run % channels
    ("rows_4096", 1, 2, 4096, False),            # quantize_rows_vec4_kernel: exactly one piece per run
    ("rows_4100", 2, 3, 4100, False),            # quantize_rows_vec4_kernel: the second piece holds one float4
    ("rows_16388", 1, 2, 16388, False),          # quantize_rows_vec4_kernel: five pieces, the last with one float4
    ("vec4_1020", 2, 3, 1020, False),            # quantize_vec4_kernel: inner < 1024
    ("vec4_36", 3, 5, 36, False),                # quantize_vec4_kernel: several channels per float4 grid stride
    ("generic_1027", 2, 3, 1027, False),         # quantize_kernel<float, int8_t>: inner % 4 != 0
    ("generic_misaligned", 2, 3, 1024, True),    # quantize_kernel<float, int8_t>: x not 16-byte aligned
]


@pytest.mark.parametrize("zp_kind", ZP_KINDS, ids=lambda k: "zp_none" if k is None else f"zp_{np.dtype(k).name}")
@pytest.mark.parametrize("route", QUANT_ROUTES, ids=lambda r: r[0])
def test_quantize_int8_container_routes(m, route, zp_kind):
  _, outer, ch, inner, misalign = route
  for bits, narrow in INT8_CONFIGS:
    rng = np.random.default_rng([outer, ch, inner, bits, int(narrow), 0 if zp_kind is None else 1 + zp_kind(0).itemsize])
    scale, zp = channel_params(rng, ch, bits, zp_kind, False)
    x = designed_x(rng, outer, ch, inner, scale, zp, bits)
    got = run_quantize(m, x, outer, ch, inner, scale, zp, bits, narrow, misalign)
    same_bits(got, quantize_ref(x, scale, zp, bits, narrow))


@pytest.mark.parametrize("f64", [False, True], ids=["scale_f32", "scale_f64"])
@pytest.mark.parametrize("bits,narrow", [(9, False), (16, True), (17, False), (31, True), (32, False), (32, True)])
def test_quantize_wide_containers(m, bits, narrow, f64):
  """quantize_kernel<float|double, int16_t|int32_t>. NaN must come out as NumPy's x86 cast makes it: 0 in int16,
  INT_MIN in int32 (cvttss2si / cvttsd2si 'integer indefinite'), for both scale types."""
  for zp_kind in ZP_KINDS:
    for outer, ch, inner in ((2, 3, 1024), (1, 4, 1027)):
      rng = np.random.default_rng([bits, int(narrow), int(f64), inner, 0 if zp_kind is None else zp_kind(0).itemsize])
      scale, zp = channel_params(rng, ch, bits, zp_kind, f64)
      x = designed_x(rng, outer, ch, inner, scale, zp, bits)
      got = run_quantize(m, x, outer, ch, inner, scale, zp, bits, narrow)
      same_bits(got, quantize_ref(x, scale, zp, bits, narrow))


@pytest.mark.parametrize("bits,narrow", INT8_CONFIGS)
def test_quantize_f64_scale_int8_container(m, bits, narrow):
  """quantize_kernel<double, int8_t>: a float64 scale never takes the float32 vector kernels, even where they fit."""
  for zp_kind in ZP_KINDS:
    rng = np.random.default_rng([bits, int(narrow), 64])
    outer, ch, inner = 2, 3, 4100
    scale, zp = channel_params(rng, ch, bits, zp_kind, True)
    x = designed_x(rng, outer, ch, inner, scale, zp, bits)
    got = run_quantize(m, x, outer, ch, inner, scale, zp, bits, narrow)
    same_bits(got, quantize_ref(x, scale, zp, bits, narrow))


def test_quantize_nan_into_int32_is_int_min(m):
  """The known answer behind the NaN rule: np.float32('nan').astype(np.int32) on x86."""
  x = np.array([np.nan, 1.0, -np.inf, np.inf], np.float32)
  # float32 chain: the bounds +-(2^31 - 1) round to +-2^31 and +2^31 is out of range (INT_MIN); float64 keeps them
  for scale, want in ((np.array([0.5], np.float32), [-2 ** 31, 2, -2 ** 31, -2 ** 31]),
                      (np.array([0.5], np.float64), [-2 ** 31, 2, -2 ** 31 + 1, 2 ** 31 - 1])):
    got = run_quantize(m, x.reshape(1, 1, 4), 1, 1, 4, scale, None, 32, True)
    assert got.dtype == np.int32 and got.reshape(-1).tolist() == want
    same_bits(got, quantize_ref(x.reshape(1, 1, 4), scale, None, 32, True))


def test_quantize_tensorwise_4096x4096_rows_route(m):
  """quantize_rows_vec4_kernel with channels == 1: 4096 pieces of one run, int8 zero point (float32 add)."""
  rng = np.random.default_rng(4096)
  scale, zp = np.array([0.046875], np.float32), np.array([-37], np.int8)
  x = designed_x(rng, 1, 1, 4096 * 4096, scale, zp, 8).reshape(4096, 4096)
  got = run_quantize(m, x, 1, 1, x.size, scale, zp, 8, False)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    want = O.uniform_quantize(x, scale.reshape(1, 1), zp.reshape(1, 1), 8, False)
  same_bits(got, want)


# ------------------------------------------------------------------------------------------------------- dequantize ---
def designed_q(rng, shape, dtype):
  """Integers over the whole container with its two extremes at the first, middle and last element of every row."""
  info = np.iinfo(dtype)
  q = rng.integers(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(dtype)
  q[..., 0], q[..., shape[-1] // 2], q[..., -1] = info.min, info.max, info.min
  return q


def dq_zero_points(rng, ch, zp_kind):
  """+-1 and the container's extremes (each makes some q - zp leave the difference type: NumPy wraps in int8 / int16 /
  int32, not in int64) and random values; int64 zero points stay in the int32 range the ABI carries."""
  info = np.iinfo(zp_kind if zp_kind != np.int64 else np.int32)
  fixed = np.array([1, -1, info.min, info.max], np.int64)
  z = rng.integers(info.min, int(info.max) + 1, ch, dtype=np.int64)
  z[:min(ch, 4)] = fixed[:min(ch, 4)]
  return z.astype(zp_kind)


def dequantize_ref(q, scale, zp):
  ch = scale.size
  return O.uniform_dequantize(q.reshape(-1, ch, q.shape[-1]), scale.reshape(1, ch, 1),
                              zp.reshape(1, ch, 1)).reshape(q.shape)


DQ_ROUTES = [
    # id,            outer, ch, inner, q dtype
    ("rows_1024", 1, 4, 1024, np.int8),          # dequantize_rows_vec4_kernel (int8 q, float32 out and scale)
    ("rows_1028_outer", 3, 4, 1028, np.int8),    # dequantize_rows_vec4_kernel: outer > 1, channel = run % channels
    ("rows_4100", 2, 5, 4100, np.int8),          # dequantize_rows_vec4_kernel: the second piece holds one dword
    ("generic_1020", 2, 4, 1020, np.int8),       # dequantize_kernel<int8_t, *>: inner < 1024
    ("generic_i16", 2, 4, 1028, np.int16),       # dequantize_kernel<int16_t, *>
    ("generic_i32", 2, 4, 1028, np.int32),       # dequantize_kernel<int32_t, double>
]


@pytest.mark.parametrize("f64", [False, True], ids=["scale_f32", "scale_f64"])
@pytest.mark.parametrize("zp_kind", [np.int8, np.int16, np.int32, np.int64], ids=lambda k: f"zp_{np.dtype(k).name}")
@pytest.mark.parametrize("route", DQ_ROUTES, ids=lambda r: r[0])
def test_dequantize_routes(m, route, zp_kind, f64):
  """diff_bits is the width of NumPy's promoted (q, zero point) type: 8 (an int8 difference that wraps), 16, 32 (wraps)
  or 64 (does not); the output has NumPy's result type, float64 for a float64 scale (the scale is not rounded to
  float32). Routes with a float32 output and an int8 q take the rows kernel, the others dequantize_kernel."""
  _, outer, ch, inner, qdt = route
  rng = np.random.default_rng([outer, ch, inner, np.dtype(qdt).itemsize, np.dtype(zp_kind).itemsize, int(f64)])
  q = designed_q(rng, (outer, ch, inner), qdt)
  zp = dq_zero_points(rng, ch, zp_kind)
  scale, _ = channel_params(rng, ch, 8, None, f64)
  diff_bits = np.result_type(qdt, zp_kind).itemsize * 8
  out = m.ops.dequantize(dev(q.reshape(-1)), outer, ch, inner, dev(scale), dev(zp.astype(np.int32)), diff_bits)
  same_bits(host(out).reshape(q.shape), dequantize_ref(q, scale, zp))


def test_dequantize_tensorwise_4096x4096_rows_route(m):
  """dequantize_rows_vec4_kernel with channels == 1 and 4096 pieces; int8 zero point, int8 difference that wraps."""
  rng = np.random.default_rng(44)
  q = designed_q(rng, (4096, 4096), np.int8)
  scale, zp = np.array([0.0123], np.float32), np.array([-100], np.int8)
  out = m.ops.dequantize(dev(q.reshape(-1)), 1, 1, q.size, dev(scale), dev(zp.astype(np.int32)), 8)
  same_bits(host(out).reshape(q.shape), O.uniform_dequantize(q, scale.reshape(1, 1), zp.reshape(1, 1)))


def test_dequantize_misaligned_buffers_take_the_generic_kernel(m):
  """dequantize_kernel<int8_t, float>: an output one float past a 16-byte boundary (through the C ABI) and a q one byte
  past a dword, where the rows kernel would otherwise fit. The float before the output stays untouched."""
  torch = m.torch
  outer, ch, inner = 2, 3, 1024
  rng = np.random.default_rng(7)
  q = designed_q(rng, (outer, ch, inner), np.int8)
  zp = dq_zero_points(rng, ch, np.int8)
  scale, _ = channel_params(rng, ch, 8, None, False)
  want = dequantize_ref(q, scale, zp)
  n = q.size
  qd, sd, zd = dev(q.reshape(-1)), dev(scale), dev(zp.astype(np.int32))
  out = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
  assert out.data_ptr() % 16 == 0
  m.check(m.L.mi355q_dequantize_f32(m.rt.ptr(qd), 8, outer, ch, inner, m.rt.ptr(sd), 0, m.rt.ptr(zd), 8, 0,
                                    ctypes.c_void_p(out.data_ptr() + 4), m.rt.stream_ptr()))
  got = host(out)
  same_bits(got[1:n + 1].reshape(q.shape), want)
  assert got[0] == -7.0 and np.all(got[n + 1:] == -7.0)
  qfull = dev(np.concatenate([np.zeros(1, np.int8), q.reshape(-1)]))
  assert qfull[1:].data_ptr() % 4 == 1
  out2 = m.ops.dequantize(qfull[1:], outer, ch, inner, sd, zd, 8)
  same_bits(host(out2).reshape(q.shape), want)


# ------------------------------------------------------------------------------------------------------- K1 min/max ---
def plan(outer, ch, inner):
  """elementwise.hip plan_minmax: (lastdim, splits, chunk or rows per split)."""
  if inner == 1 and outer > 1:
    splits = min(max(outer // 256, 1), 128)
    return True, splits, -(-outer // splits)
  n = outer * inner
  splits = min(max(8192 // ch, 1), max(-(-n // 4096), 1))
  chunk = -(-(-(-n // splits)) // 64) * 64
  return False, max(-(-n // chunk), 1), chunk


def finalize_of(splits, ch):
  return "wave" if splits >= 16 and ch <= 4096 else "kernel" if splits > 1 else "none"


MINMAX_VIEWS = [
    # id,                 outer, ch, inner, splits, finalize
    ("lastdim_1", 300, 70, 1, 1, "none"),               # minmax_lastdim_kernel, one split
    ("lastdim_16_wide", 4096, 4100, 1, 16, "kernel"),   # lastdim, 16 splits, channels > 4096: minmax_finalize_kernel
    ("lastdim_16_ragged", 4196, 9, 1, 16, "wave"),      # lastdim, 16 splits of 263 rows, the last of 251
    ("lastdim_128", 32768, 40, 1, 128, "wave"),         # lastdim, 128 splits
    ("runs_1", 1, 64, 1024, 1, "none"),                 # minmax_runs_kernel, outer == 1 aligned, one split
    ("runs_tail", 1, 5, 5001, 2, "kernel"),             # outer == 1, inner % 4 != 0: channels 0 / 4 aligned with a
                                                        #   one-float scalar tail, channels 1..3 on the unaligned path
    ("runs_10", 1, 1, 40000, 10, "kernel"),             # outer == 1, ten splits
    ("runs_outer", 7, 4, 3000, 6, "kernel"),            # outer > 1 (indexed path), splits across run boundaries
    ("runs_300", 1, 4, 4096 * 300, 300, "wave"),        # minmax_finalize_wave_kernel, tail loop only
    ("runs_782", 1, 4, 3200000, 782, "wave"),           # wave finalize, four-deep loop for threads 0..13
    ("tensorwise_4096", 1, 1, 4096 * 4096, 4096, "wave"),   # TENSORWISE 4096 x 4096: four-deep loop four times
]


def split_bounds(view):
  """[(begin, end)] of every split, in the channel's own element order (rows for lastdim)."""
  outer, ch, inner = view
  lastdim, splits, per = plan(outer, ch, inner)
  n = outer if lastdim else outer * inner
  return [(s * per, min((s + 1) * per, n)) for s in range(splits)]


def put(x, view, c, e, v):
  """Element e (in channel c's order) of the [outer, channels, inner] view."""
  outer, ch, inner = view
  o, i = divmod(e, inner)
  x[o, c, i] = v


def minmax_check(m, x, view):
  outer, ch, inner = view
  mn, mx = m.ops.minmax(dev(x.reshape(-1)), outer, ch, inner)
  # min / max of equal zeros of either sign is whichever the reduction order meets first, in NumPy as on the GPU; a
  # zero is compared by value (array_equal), every other value and NaN by value and bits
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    want_mn, want_mx = x.min(axis=(0, 2)), x.max(axis=(0, 2))
  for got, want in ((host(mn), want_mn), (host(mx), want_mx)):
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    nz = ~np.isnan(want) & (want != 0)
    assert np.array_equal(got[nz].view(np.uint32), want[nz].view(np.uint32))


@pytest.mark.parametrize("view", MINMAX_VIEWS, ids=lambda v: v[0])
def test_minmax_plans_extremes_at_split_edges(m, view):
  """Every channel's minimum sits at the first element of one split and its maximum at the last element of another
  (or at the channel's very last element, the scalar tail where there is one)."""
  name, outer, ch, inner, splits, fin = view
  v = (outer, ch, inner)
  lastdim, got_splits, _ = plan(*v)
  assert (got_splits, finalize_of(got_splits, ch)) == (splits, fin), name
  assert lastdim == (inner == 1)
  ws = m.L.mi355q_minmax_workspace_bytes(outer, ch, inner)
  assert ws == (splits * ch * 8 if splits > 1 else 0)
  rng = np.random.default_rng([outer, ch, inner])
  x = rng.uniform(-1, 1, (outer, ch, inner)).astype(np.float32)
  bounds = split_bounds(v)
  for c in range(ch):
    b0, _ = bounds[c % splits]
    _, e1 = bounds[(7 * c + 3) % splits]
    last = e1 - 1 if c % 2 == 0 else bounds[-1][1] - 1
    put(x, v, c, b0, np.float32(-2.0 - c / 8))
    put(x, v, c, last, np.float32(2.0 + c / 8))
  minmax_check(m, x, v)


@pytest.mark.parametrize("view", [mv for mv in MINMAX_VIEWS if mv[2] >= 4], ids=lambda v: v[0])
def test_minmax_plans_nan_inf_and_signed_zero(m, view):
  """Channel 0: one NaN in exactly one split (the others finite); channel 1: all NaN; channel 2: -inf at a split's
  first element and +inf at another's last; channel 3: only zeros of both signs."""
  name, outer, ch, inner, splits, _ = view
  v = (outer, ch, inner)
  rng = np.random.default_rng([outer, ch, inner, 1])
  x = rng.uniform(-1, 1, (outer, ch, inner)).astype(np.float32)
  bounds = split_bounds(v)
  b, e = bounds[len(bounds) // 2]
  put(x, v, 0, (b + e) // 2, np.float32(np.nan))
  x[:, 1, :] = np.nan
  put(x, v, 2, bounds[-1][0], np.float32(-np.inf))
  put(x, v, 2, bounds[0][1] - 1, np.float32(np.inf))
  x[:, 3, :] = np.where(rng.integers(0, 2, (outer, inner)) == 1, np.float32(-0.0), np.float32(0.0))
  minmax_check(m, x, v)


def test_minmax_tensorwise_nan_in_one_of_4096_splits(m):
  v = (1, 1, 4096 * 4096)
  x = np.random.default_rng(9).uniform(-1, 1, v).astype(np.float32)
  put(x, v, 0, 4096 * 2047 + 4095, np.float32(np.nan))   # the last element of split 2047
  minmax_check(m, x, v)


# ---------------------------------------------------------------------------------------------------------- unpack ---
UNPACK_NS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 33]


def run_unpack(m, packed, n, bits, p_off, o_off):
  """mi355q_unpack_bits with the packed bytes at byte offset p_off and the output at o_off of their buffers; the
  guard bytes around the output must stay untouched."""
  torch = m.torch
  pbuf = torch.zeros(packed.size + 8, dtype=torch.uint8, device="cuda")
  pbuf[p_off:p_off + packed.size] = dev(packed)
  obuf = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device="cuda")
  assert pbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
  m.check(m.L.mi355q_unpack_bits(ctypes.c_void_p(pbuf.data_ptr() + p_off), n, bits,
                                 ctypes.c_void_p(obuf.data_ptr() + o_off), m.rt.stream_ptr()))
  out = host(obuf)
  assert np.all(out[:o_off] == 0x5A) and np.all(out[o_off + n:] == 0x5A)
  return out[o_off:o_off + n].view(np.int8)


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_unpack_offsets_and_tails(m, bits):
  """unpack_kernel<2|4> (copy_bytes_kernel for 8): dword loads and stores only where both pointers are aligned and the
  group is whole, bytes elsewhere -- every length around a group edge at every byte offset of either pointer."""
  lo, hi = -(2 ** (bits - 1)), 2 ** (bits - 1)
  for n in UNPACK_NS:
    data = np.random.default_rng([bits, n]).integers(lo, hi, n).astype(np.int8)
    packed = O.pack_data(bits, data.view(np.uint8)).astype(np.uint8)
    assert packed.size == -(-n * bits // 8)
    for p_off in range(4):
      for o_off in range(4):
        same_bits(run_unpack(m, packed, n, bits, p_off, o_off), data)


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_unpack_large_round_trip(m, bits):
  n = (1 << 20) + 3
  lo, hi = -(2 ** (bits - 1)), 2 ** (bits - 1)
  data = np.random.default_rng(n + bits).integers(lo, hi, n).astype(np.int8)
  packed = O.pack_data(bits, data.view(np.uint8)).astype(np.uint8)
  for p_off, o_off in ((0, 0), (1, 3), (3, 2)):
    same_bits(run_unpack(m, packed, n, bits, p_off, o_off), data)
  if bits != 8:   # and through ops, from the packing kernel
    same_bits(host(m.ops.unpack_bits(m.ops.pack_bits(dev(data), bits), n, bits)), data)


# ------------------------------------------------------------------------------------------------------ public API ---
def op_info(m, op, cfg):
  q = m.qtyping
  return q.OpInfo(op=q.OperatorT(), op_name=q.TFLOperationName[op], subgraph_op_index=0,
                  op_quant_config=q.OpQuantizationConfig(weight_tensor_config=cfg))


def check_params(p, ref):
  for key in ("scale", "zero_point", "quantized_data"):
    same_bits(np.asarray(getattr(p, key)), np.asarray(ref[key]))
  assert p.quantized_dimension == ref["quantized_dimension"] and p.block_size == ref["block_size"]


def layer(rng, shape, qdim, nan=True):
  """Normal weights with an outlier channel, an all-zero channel and (optionally) a channel holding one NaN."""
  w = rng.standard_normal(shape, dtype=np.float32)
  wv = np.moveaxis(w, qdim, 0)   # a view: channel-first indexing of the same buffer
  wv[1] *= np.float32(300.0)
  wv[2] = 0.0
  if nan:
    wv[3][np.unravel_index(wv[3].size // 3, wv[3].shape)] = np.nan
  return w


def min_max_params(m, w, op, bits, symmetric, granularity):
  q = m.qtyping
  cfg = q.TensorQuantizationConfig(num_bits=bits, symmetric=symmetric, granularity=q.QuantGranularity[granularity])
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    p = m.mm.get_tensor_quant_params(op_info(m, op, cfg), cfg, w)
    ref = O.min_max_quant_params(w, bits, symmetric, granularity, op=op)
  return p, ref


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
def test_min_max_tensorwise_4096x4096(m, bits, symmetric):
  """TENSORWISE: K1 over 4096 splits with the wave finalize, then K3 on the rows route with channels == 1."""
  w = layer(np.random.default_rng([bits, int(symmetric)]), (4096, 4096), 0, nan=False)
  p, ref = min_max_params(m, w, "FULLY_CONNECTED", bits, symmetric, "TENSORWISE")
  check_params(p, ref)


def test_min_max_tensorwise_2048x16384_asymmetric(m):
  w = layer(np.random.default_rng(16384), (2048, 16384), 0, nan=False)
  p, ref = min_max_params(m, w, "FULLY_CONNECTED", 8, False, "TENSORWISE")
  check_params(p, ref)


def test_min_max_tensorwise_nan_weight(m):
  w = layer(np.random.default_rng(3), (256, 4096), 0)
  for symmetric in (True, False):
    p, ref = min_max_params(m, w, "FULLY_CONNECTED", 8, symmetric, "TENSORWISE")
    check_params(p, ref)


@pytest.mark.parametrize("op,shape,qdim", [
    ("FULLY_CONNECTED", (4096, 4096), 0),       # K1 runs, one split; K3 rows route, 4096 channels
    ("CONV_2D", (256, 3, 3, 512), 0),           # K1 runs, 2 splits (finalize kernel); K3 rows, two pieces per run
    ("DEPTHWISE_CONV_2D", (1, 48, 48, 512), 3), # K1 lastdim, 9 splits (finalize kernel); K3 quantize_kernel (inner 1)
], ids=["fc", "conv2d", "depthwise"])
def test_min_max_channelwise_asymmetric_layers(m, op, shape, qdim):
  w = layer(np.random.default_rng(list(shape)), shape, qdim)
  p, ref = min_max_params(m, w, op, 8, False, "CHANNELWISE")
  check_params(p, ref)


def uq_params(m, scale, zp, bits, symmetric, qdim):
  return m.qtyping.UniformQuantParams(scale=scale, zero_point=zp, num_bits=bits, symmetric=symmetric,
                                      quantized_dimension=qdim)


@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("zp_kind", [np.int8, np.int16, np.int32, np.int64], ids=lambda k: f"zp_{np.dtype(k).name}")
@pytest.mark.parametrize("f64", [False, True], ids=["scale_f32", "scale_f64"])
def test_uniform_quantize_dequantize_dtype_sweep(m, f64, zp_kind, bits):
  """uniform_quantize / uniform_dequantize against the oracle for every scale x zero-point x container type, on a
  [6, 1028] weight quantized along dimension 0 (int8 q on the rows kernels where the types allow)."""
  rng = np.random.default_rng([bits, np.dtype(zp_kind).itemsize, int(f64)])
  ch, inner = 6, 1028
  scale, zp = channel_params(rng, ch, bits, zp_kind, f64)
  x = designed_x(rng, 1, ch, inner, scale, zp, bits).reshape(ch, inner)
  s2, z2 = scale.reshape(ch, 1), zp.reshape(ch, 1)
  for symmetric in (True, False):
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")
      want = O.uniform_quantize(x, s2, z2, bits, symmetric, quantized_dim=0)
    got = m.uqt.uniform_quantize(x, uq_params(m, s2, z2, bits, symmetric, 0))
    same_bits(got, want)
  q = designed_q(rng, (ch, inner), O.int_dtype(bits))
  zq = dq_zero_points(rng, ch, zp_kind).reshape(ch, 1)
  got = m.uqt.uniform_dequantize(q, uq_params(m, s2, zq, bits, False, 0))
  same_bits(got, O.uniform_dequantize(q, s2, zq, quantized_dim=0))


def test_uniform_dequantize_known_answers_keep_the_float64_scale(m, known_answers):
  """The reference's own cases with their float64 scales: NumPy multiplies by the float64 value (-3.023622 for -24 *
  0.12598425), not by the scale rounded to float32."""
  for c in known_answers["uniform_dequantize"]["cases"]:
    q = np.array(c["quantized"], np.int8)
    scale, zp = np.array(c["scale"], np.float64), np.array(c["zero_point"], np.int64)
    want = O.uniform_dequantize(q, scale, zp)
    got = m.uqt.uniform_dequantize(q, uq_params(m, scale, zp, c["num_bits"], False, None))
    same_bits(got, want)
    np.testing.assert_allclose(got, c["expected"], rtol=0, atol=10.0 ** -known_answers["uniform_dequantize"]["places"])


def test_uniform_dequantize_int64_zero_point_does_not_wrap(m):
  """int32 q - int64 zero point is an int64 difference in NumPy: q = INT_MIN, zp = 1 gives -2^31 - 1."""
  q = np.array([[-2 ** 31, 2 ** 31 - 1, 5, -2 ** 31]], np.int32)
  for zdt in (np.int64, np.int32):
    zp = np.array([[1]], zdt)
    for sdt in (np.float32, np.float64):
      scale = np.array([[0.5]], sdt)
      want = O.uniform_dequantize(q, scale, zp)
      got = m.uqt.uniform_dequantize(q, uq_params(m, scale, zp, 32, False, None))
      same_bits(got, want)
  # int64 data (held as int32 on the device, so |q| < 2^31) subtracts in 64 bits too, whatever the zero point's type:
  # 2^31 - 1 - (-1) = 2^31
  q64 = np.array([[2 ** 31 - 1, -2 ** 31 + 1, 5, 2 ** 31 - 1]], np.int64)
  for zdt in (np.int8, np.int32):
    zp = np.array([[-1]], zdt)
    scale = np.array([[0.25]], np.float32)
    got = m.uqt.uniform_dequantize(q64, uq_params(m, scale, zp, 32, False, None))
    same_bits(got, O.uniform_dequantize(q64, scale, zp))


@pytest.mark.parametrize("in_bits", [8, 16])
@pytest.mark.parametrize("f64", [False, True], ids=["scale_f32", "scale_f64"])
def test_symmetric_quantize_bias_nan_inf_huge(m, f64, in_bits):
  """Bias quantization (out_bits 32): NaN -> INT_MIN, +-inf and +-1e30 past both bounds, rint ties, the largest value
  below the bound; int64 containers after a 16-bit input. The reference's expression: oracle.quantize_bias."""
  dt = np.float64 if f64 else np.float32
  ch = 9
  s_in = np.array([0.5], dt)
  s_w = np.ldexp(1.0, -np.arange(ch) - 1).astype(dt)
  eff = (s_in * s_w).astype(dt)
  bias = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.5, -3.5, 0.0, -0.0], np.float32)
  bias[5:7] *= eff[5:7].astype(np.float32)   # x / s = 2.5, -3.5: ties
  bias[7] = np.float32(2 ** 31 - 128) * np.float32(eff[7])
  mk = m.qtyping.UniformQuantParams
  pin = mk(scale=s_in, zero_point=np.zeros(1, np.int32), num_bits=in_bits, symmetric=True, quantized_dimension=None)
  pw = mk(scale=s_w, zero_point=np.zeros(ch, np.int32), num_bits=8, symmetric=True, quantized_dimension=0)
  got = m.uqt.symmetric_quantize_bias_tensor(bias, pin, pw)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    q, e, z, nbits, qdim = O.quantize_bias(bias, s_in, s_w, in_bits)
  same_bits(got.quantized_data, q)
  same_bits(got.scale, e)
  assert got.num_bits == nbits and got.quantized_dimension == qdim
  assert q.reshape(-1)[0] == -2 ** 31   # NaN, as NumPy casts it on x86
