"""Device-level operators: one function per libmi355q entry point.

Inputs and outputs are torch tensors resident in HBM (torch is only the
allocator / stream owner). Every function enqueues on the current HIP stream and
returns without synchronizing. Shapes follow the [outer, channels, inner] view of
include/mi355q.h.
"""
from __future__ import annotations

import contextlib as _contextlib
import ctypes
import math
import os
import threading

import numpy as np
import torch

from . import _ffi
from . import runtime as rt


def _f32(x: torch.Tensor) -> torch.Tensor:
  if x.dtype != torch.float32 or not x.is_cuda:
    raise TypeError(f"expected a float32 device tensor, got {x.dtype} on {x.device}")
  return x.contiguous()


def device_info() -> dict:
  import ctypes
  rt.require_gpu()
  cu, wave = ctypes.c_int32(0), ctypes.c_int32(0)
  name = ctypes.create_string_buffer(64)
  _ffi.check(_ffi.lib().mi355q_device_info(ctypes.byref(cu), ctypes.byref(wave), name, 64))
  return {"cu_count": cu.value, "wavefront": wave.value, "arch": name.value.decode()}


def minmax(x: torch.Tensor, outer: int, channels: int, inner: int):
  """K1. Returns (min, max) float32[channels]. ref: common_quantize.py:1311-1359."""
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != outer * channels * inner:
    raise ValueError("shape view does not match numel")
  if channels and (outer == 0 or inner == 0):
    raise ValueError("zero-size array to reduction operation minimum which has no identity")
  mn = rt.empty((channels,), torch.float32)
  mx = rt.empty((channels,), torch.float32)
  L = _ffi.lib()
  nbytes = L.mi355q_minmax_workspace_bytes(outer, channels, inner)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_minmax_f32(rt.ptr(x), outer, channels, inner, rt.ptr(mn), rt.ptr(mx),
                                 rt.ptr(ws), nbytes, rt.stream_ptr()))
  return mn, mx


def requant_sym(x: torch.Tensor, block: int, bits: int, clip: torch.Tensor | None = None,
                want_q: bool = True, want_packed: bool = False, want_scale_f16: bool = False):
  """Fused K1+K2+K3(+K4) for a [rows, cols] float32 weight buffer.

  Returns dict(q=int8[rows,cols]|None, packed=uint8[...]|None,
               scale=float32[rows] or [rows, cols/block], scale_f16=float16|None).
  ref: naive_min_max_quantize.py:34-110; transformation_utils.py:293-353.
  """
  rt.require_gpu()
  x = _f32(x)
  if x.dim() != 2:
    raise ValueError("requant_sym expects a 2-D [rows, cols] tensor")
  rows, cols = x.shape
  if block and cols % block != 0:
    raise ValueError(f"Quantized dimension {cols} in tensor shape {tuple(x.shape)} is not"
                     f" divisible by block size {block}.")
  nscale_shape = (rows, cols // block) if block else (rows,)
  scale = rt.empty(nscale_shape, torch.float32)
  q = rt.empty((rows, cols), torch.int8) if want_q else None
  packed = None
  if want_packed:
    per = 8 // bits
    if (rows * cols) % per:
      raise ValueError("packed output needs numel divisible by values-per-byte")
    packed = rt.empty((rows * cols // per,), torch.uint8)
  s16 = rt.empty(nscale_shape, torch.float16) if (want_scale_f16 and block) else None
  if clip is not None:
    clip = _f32(clip)
    if clip.numel() != scale.numel():
      raise ValueError("clip must have one entry per scale")
  _ffi.check(_ffi.lib().mi355q_requant_sym_f32(
      rt.ptr(x), rows, cols, block, bits, rt.ptr(clip), rt.ptr(q), rt.ptr(packed),
      rt.ptr(scale), rt.ptr(s16), rt.stream_ptr()))
  return {"q": q, "packed": packed, "scale": scale, "scale_f16": s16}


class RequantBatch:
  """Pre-staged pointer tables for mi355q_requant_sym_f32_batched.

  Holds `count` equally shaped weight buffers and their outputs in HBM so one
  launch requantizes all of them (used by bench.py and the model-level driver).
  """

  def __init__(self, xs, block: int, bits: int, want_q=True, want_packed=False,
               want_scale_f16=False):
    rt.require_gpu()
    self.xs = [_f32(x) for x in xs]
    self.rows, self.cols = self.xs[0].shape
    if any(x.shape != self.xs[0].shape for x in self.xs):
      raise ValueError("all tensors of a batch must share one shape")
    self.block, self.bits = block, bits
    n = len(self.xs)
    sshape = (self.rows, self.cols // block) if block else (self.rows,)
    per = 8 // bits
    self.q = [rt.empty((self.rows, self.cols), torch.int8) for _ in range(n)] if want_q else None
    self.packed = ([rt.empty((self.rows * self.cols // per,), torch.uint8) for _ in range(n)]
                   if want_packed else None)
    self.scale = [rt.empty(sshape, torch.float32) for _ in range(n)]
    self.scale_f16 = ([rt.empty(sshape, torch.float16) for _ in range(n)]
                      if (want_scale_f16 and block) else None)
    self._tx = rt.ptr_table(self.xs)
    self._tq = rt.ptr_table(self.q) if self.q else None
    self._tp = rt.ptr_table(self.packed) if self.packed else None
    self._ts = rt.ptr_table(self.scale)
    self._t16 = rt.ptr_table(self.scale_f16) if self.scale_f16 else None

  def run(self) -> None:
    _ffi.check(_ffi.lib().mi355q_requant_sym_f32_batched(
        rt.ptr(self._tx), len(self.xs), self.rows, self.cols, self.block, self.bits,
        rt.ptr(self._tq), rt.ptr(self._tp), rt.ptr(self._ts), rt.ptr(self._t16),
        rt.stream_ptr()))


_OUT_DTYPE = {8: torch.int8, 16: torch.int16, 32: torch.int32}


def quantize(x: torch.Tensor, outer: int, channels: int, inner: int, scale: torch.Tensor,
             zero_point: torch.Tensor | None, bits: int, narrow: bool,
             zp_via_f64: bool = False) -> torch.Tensor:
  """K3 with given parameters. scale is float32 or float64 [channels]; zero_point
  int32 [channels] or None. ref: uniform_quantize_tensor.py:273-362."""
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != outer * channels * inner:
    raise ValueError("shape view does not match numel")
  if scale.numel() != channels:
    raise ValueError("scale must have one entry per channel")
  if scale.dtype not in (torch.float32, torch.float64):
    raise TypeError("scale must be float32 or float64")
  out_bits = 8 if bits <= 8 else 16 if bits <= 16 else 32
  q = rt.empty(tuple(x.shape), _OUT_DTYPE[out_bits])
  if zero_point is not None:
    zero_point = zero_point.to(torch.int32).contiguous()
  _ffi.check(_ffi.lib().mi355q_quantize_f32(
      rt.ptr(x), outer, channels, inner, rt.ptr(scale.contiguous()),
      1 if scale.dtype == torch.float64 else 0, rt.ptr(zero_point), 1 if zp_via_f64 else 0,
      bits, 1 if narrow else 0, out_bits, rt.ptr(q), rt.stream_ptr()))
  return q


def dequantize(q: torch.Tensor, outer: int, channels: int, inner: int, scale: torch.Tensor,
               zero_point: torch.Tensor | None, diff_bits: int) -> torch.Tensor:
  """(q - zp) * scale. scale is float32 or float64 [channels]; diff_bits the width of NumPy's
  promoted (q, zero point) type (8 / 16 / 32 / 64). The output has NumPy's result type: float64
  for a float64 scale or a 32 / 64-bit difference, else float32. ref: uniform_quantize_tensor.py:365-409."""
  rt.require_gpu()
  in_bits = {torch.int8: 8, torch.int16: 16, torch.int32: 32}[q.dtype]
  if scale.dtype not in (torch.float32, torch.float64) or not scale.is_cuda:
    raise TypeError(f"scale must be a float32 or float64 device tensor, got {scale.dtype} on {scale.device}")
  scale_f64 = scale.dtype == torch.float64
  out_f64 = in_bits == 32 or diff_bits >= 32 or scale_f64
  out = rt.empty(tuple(q.shape), torch.float64 if out_f64 else torch.float32)
  if zero_point is not None:
    zero_point = zero_point.to(torch.int32).contiguous()
  _ffi.check(_ffi.lib().mi355q_dequantize_f32(
      rt.ptr(q.contiguous()), in_bits, outer, channels, inner, rt.ptr(scale.contiguous()),
      1 if scale_f64 else 0, rt.ptr(zero_point), diff_bits, 1 if out_f64 else 0, rt.ptr(out),
      rt.stream_ptr()))
  return out


def pack_bits(q: torch.Tensor, bits: int) -> torch.Tensor:
  """K4. int8 values -> packed bytes. ref: transformation_utils.py:293-353."""
  rt.require_gpu()
  if q.dtype not in (torch.int8, torch.uint8) or not q.is_cuda:
    raise TypeError("pack_bits expects an int8/uint8 device tensor")
  q = q.contiguous().view(-1)
  n = q.numel()
  n_out = n if bits not in (2, 4) else -(-n * bits // 8)
  out = rt.empty((n_out,), torch.uint8)
  if bits not in (2, 4):
    out.copy_(q.view(torch.uint8))
    return out
  _ffi.check(_ffi.lib().mi355q_pack_bits(rt.ptr(q), n, bits, rt.ptr(out), rt.stream_ptr()))
  return out


def unpack_bits(packed: torch.Tensor, n: int, bits: int) -> torch.Tensor:
  """Inverse of K4: n sign-extended int8 values from the packed bytes of one fused launch."""
  rt.require_gpu()
  if packed.dtype != torch.uint8 or not packed.is_cuda:
    raise TypeError("unpack_bits expects a uint8 device tensor")
  packed = packed.contiguous().view(-1)
  if packed.numel() != -(-n * bits // 8):
    raise ValueError("packed size does not match the element count")
  out = rt.empty((n,), torch.int8)
  _ffi.check(_ffi.lib().mi355q_unpack_bits(rt.ptr(packed), n, bits, rt.ptr(out), rt.stream_ptr()))
  return out


def cast_f16(x: torch.Tensor) -> torch.Tensor:
  """float32 -> float16 (RNE), same shape. ref: nonlinear_quantize/float_casting.py:157-160."""
  rt.require_gpu()
  x = _f32(x)
  out = rt.empty(tuple(x.shape), torch.float16)
  _ffi.check(_ffi.lib().mi355q_cast_f32_to_f16(rt.ptr(x), x.numel(), rt.ptr(out), rt.stream_ptr()))
  return out


# How far the host may run ahead of the GPU in tables (one per calibration sample): with 8 the op walk of an 18-layer GPTQ
# calibration stood still during every burst of Hessian products (one per 32 samples, 0.4 s each) and the GPU then waited for the
# walk of the next 24 samples (4 ms each); 64 x 128 KB of pinned memory let the walk finish while the products run.
_TABLE_SLOTS = int(os.environ.get("MI355Q_TABLE_SLOTS", 64))
_TABLE_CAPACITY = 8192          # entries per row of a slot (2 rows of int64: 128 KB of pinned memory)
_TABLE_RING: dict = {}          # device index -> {"slots": [(pinned int64 [2, capacity], event)], "next": 0}
_TABLE_LOCK = threading.Lock()


def _table_to_device(pointers, lengths) -> torch.Tensor:
  """int64 [2, n] on the device, copied asynchronously out of a ring of pinned slots."""
  n = len(pointers)
  dev = rt.device()
  if n > _TABLE_CAPACITY:
    return torch.tensor([pointers, lengths], dtype=torch.int64).to(dev)
  with _TABLE_LOCK:                         # (slot choice, fill and enqueue as one step: threads share the ring)
    ring = _TABLE_RING.setdefault(dev.index, {"slots": [], "next": 0})
    k = ring["next"] % _TABLE_SLOTS
    ring["next"] += 1
    if len(ring["slots"]) <= k:
      ring["slots"].append((torch.empty((2, _TABLE_CAPACITY), dtype=torch.int64, pin_memory=True), torch.cuda.Event()))
    pinned, event = ring["slots"][k]
    event.synchronize()                     # the copy that last read this slot (eight tables ago)
    pinned[0, :n] = torch.tensor(pointers, dtype=torch.int64)
    pinned[1, :n] = torch.tensor(lengths, dtype=torch.int64)
    out = torch.empty((2, n), dtype=torch.int64, device=dev)
    out.copy_(pinned[:, :n], non_blocking=True)
    event.record()
  return out


class ActMinMaxBatch:
  """Pre-staged K7 launch over a fixed list of float32 device tensors (<= 65535).

  Pointer / length tables, workspace and the [count, 2] output live in HBM, so
  `run()` is just the two kernel launches (used per calibration sample).
  """

  def __init__(self, tensors, lo: float | None = -3e38, hi: float | None = 3e38):
    rt.require_gpu()
    self.tensors = [_f32(t) for t in tensors]
    if len(self.tensors) > 65535:
      raise ValueError("at most 65535 tensors per batch")
    if any(t.numel() == 0 for t in self.tensors):
      raise ValueError("zero-size array to reduction operation minimum which has no identity")
    if (lo is None) != (hi is None):
      raise ValueError("lo and hi must both be given or both be None")
    self.use = lo is not None
    self.lo = np.float32(lo if self.use else 0.0)
    self.hi = np.float32(hi if self.use else 0.0)
    n = len(self.tensors)
    self.out = rt.empty((n, 2), torch.float32)
    if n:
      # pointer and length tables travel in one copy -- from a pinned slot, so that the copy is queued
      # like a kernel (a pageable copy holds the calling thread until everything queued before it on
      # the stream has run: one such wait per calibration sample was 0.5 s of an 18-layer GPTQ
      # calibration, the op walk and the Hessian products taking turns instead of overlapping)
      both = _table_to_device([t.data_ptr() for t in self.tensors], [t.numel() for t in self.tensors])
      self._tab, self._numel = both[0], both[1]
      self._nbytes = _ffi.lib().mi355q_act_minmax_workspace_bytes(n)
      self._ws = rt.empty((self._nbytes,), torch.uint8)

  def run(self) -> torch.Tensor:
    n = len(self.tensors)
    if n:
      _ffi.check(_ffi.lib().mi355q_act_minmax_f32(
          rt.ptr(self._tab), rt.ptr(self._numel), n, self.lo, self.hi, 1 if self.use else 0,
          rt.ptr(self.out), rt.ptr(self._ws), self._nbytes, rt.stream_ptr()))
    return self.out


def act_minmax(tensors, lo: float | None = -3e38, hi: float | None = 3e38) -> torch.Tensor:
  """K7 over a list of float32 device tensors -> float32[count, 2] (min, max).

  ref: common_quantize.py:1362-1413. lo/hi None disables the range masks.
  """
  ts = list(tensors)
  if len(ts) <= 65535:
    return ActMinMaxBatch(ts, lo, hi).run()
  return torch.cat([ActMinMaxBatch(ts[i:i + 65535], lo, hi).run() for i in range(0, len(ts), 65535)])


def act_minmax_entries(pointers, lengths, lo: float = -3e38, hi: float = 3e38) -> torch.Tensor:
  """K7 over (device pointer, float32 element count) pairs whose memory the caller keeps alive until the launch has
  run -> float32 [count, 2]. The calibrator's K-samples-per-launch path: K x T activations, one table, one launch."""
  rt.require_gpu()
  n = len(pointers)
  out = rt.empty((n, 2), torch.float32)
  L = _ffi.lib()
  for i in range(0, n, _TABLE_CAPACITY):
    m = min(_TABLE_CAPACITY, n - i)
    both = _table_to_device(pointers[i:i + m], lengths[i:i + m])
    nbytes = L.mi355q_act_minmax_workspace_bytes(m)
    ws = rt.empty((nbytes,), torch.uint8)
    _ffi.check(L.mi355q_act_minmax_f32(rt.ptr(both[0]), rt.ptr(both[1]), m, np.float32(lo), np.float32(hi), 1,
                                       rt.ptr(out[i:i + m]), rt.ptr(ws), nbytes, rt.stream_ptr()))
  return out


def _hist_tables(pointers, outers, channels, inners, i: int, m: int):
  """The entry tables of entries i .. i + m: three queued copies out of the pinned ring. -> (ptr, outer, channels, inner,
  slot0) device rows, the chunk's slot count and its largest element count."""
  ch = [int(c) for c in channels[i:i + m]]
  slot0, total = [], 0
  for c in ch:
    slot0.append(total)
    total += c
  a = _table_to_device(pointers[i:i + m], outers[i:i + m])
  b = _table_to_device(ch, inners[i:i + m])
  c = _table_to_device(slot0, slot0)
  numel = max(int(o) * int(k) * int(n) for o, k, n in zip(outers[i:i + m], ch, inners[i:i + m]))
  return (a[0], a[1], b[0], b[1], c[0]), total, numel


def hist_stats_entries(pointers, outers, channels, inners):
  """Finite min, finite max and finite count of every (entry, channel) of a table of float32 tensors whose memory the
  caller keeps alive until the launch has run; entry k is seen as [outers[k], channels[k], inners[k]] and owns channels[k]
  consecutive slots. -> (float32 [S], float32 [S], int64 [S]) on the device; +inf / -inf / 0 where nothing is finite.
  ref: utils/histogram_utils.py:145-146, 404-416."""
  rt.require_gpu()
  n = len(pointers)
  slots = sum(int(c) for c in channels)
  mn, mx = rt.empty((slots,), torch.float32), rt.empty((slots,), torch.float32)
  cnt = rt.empty((slots,), torch.int64)
  L = _ffi.lib()
  done = 0
  for i in range(0, n, _TABLE_CAPACITY):
    m = min(_TABLE_CAPACITY, n - i)
    tabs, s, numel = _hist_tables(pointers, outers, channels, inners, i, m)
    nbytes = L.mi355q_hist_stats_workspace_bytes(s)
    ws = rt.empty((max(nbytes, 1),), torch.uint8)
    _ffi.check(L.mi355q_hist_stats_f32(*[rt.ptr(t) for t in tabs], m, s, numel, rt.ptr(mn[done:done + s]),
                                       rt.ptr(mx[done:done + s]), rt.ptr(cnt[done:done + s]), rt.ptr(ws), nbytes,
                                       rt.stream_ptr()))
    done += s
  return mn, mx, cnt


def hist_bins_entries(pointers, outers, channels, inners, lower_bound, bin_width, n_bins, precision: int = 0):
  """Bin counts of the same kind of table: slot s (in table order) counts its finite elements into n_bins[s] bins from
  lower_bound[s] in steps of bin_width[s]; n_bins[s] == 0 skips the slot. precision: 0 float32 arithmetic, 1 float32
  subtraction and float64 division, 2 float64 (include/mi355q.h). -> (int64 [sum(n_bins)] on the device, the row offsets
  as an int64 ndarray). ref: utils/histogram_utils.py:157-164."""
  rt.require_gpu()
  n = len(pointers)
  nb = np.ascontiguousarray(n_bins, dtype=np.int64)
  slots = sum(int(c) for c in channels)
  if nb.shape != (slots,) or len(lower_bound) != slots or len(bin_width) != slots:
    raise ValueError("lower_bound, bin_width and n_bins need one entry per (entry, channel)")
  if nb.size and int(nb.min()) < 0:
    raise ValueError("n_bins must not be negative")
  offsets = np.zeros(slots, np.int64)
  if slots > 1:
    np.cumsum(nb[:-1], out=offsets[1:])
  total = int(nb.sum())
  out = torch.zeros((max(total, 1),), dtype=torch.int64, device=rt.device())
  if total == 0:
    return out[:0], offsets
  real = torch.from_numpy(np.stack([np.asarray(lower_bound, np.float64), np.asarray(bin_width, np.float64)])).to(rt.device())
  whole = torch.from_numpy(np.stack([nb, offsets])).to(rt.device())
  L = _ffi.lib()
  done = 0
  for i in range(0, n, _TABLE_CAPACITY):
    m = min(_TABLE_CAPACITY, n - i)
    tabs, s, numel = _hist_tables(pointers, outers, channels, inners, i, m)
    nbytes = L.mi355q_hist_bins_workspace_bytes(s)
    ws = rt.empty((max(nbytes, 1),), torch.uint8)
    _ffi.check(L.mi355q_hist_bins_f32(*[rt.ptr(t) for t in tabs], m, s, numel, rt.ptr(real[0, done:done + s]),
                                      rt.ptr(real[1, done:done + s]), rt.ptr(whole[0, done:done + s]),
                                      rt.ptr(whole[1, done:done + s]), int(nb[done:done + s].max()), int(precision),
                                      rt.ptr(out), total, rt.ptr(ws), nbytes, rt.stream_ptr()))
    done += s
  return out[:total], offsets


_OCTAV_MODE = [None]          # None: MI355Q_OCTAV_FAST decides; "exact" / "fast" inside octav_mode()


def _octav_fast() -> bool:
  if _OCTAV_MODE[0] is not None:
    return _OCTAV_MODE[0] == "fast"
  return os.environ.get("MI355Q_OCTAV_FAST", "") not in ("", "0")


@_contextlib.contextmanager
def octav_mode(mode: str = "exact"):
  """The kernel OCTAV's clip search (ref octav.py:30-112) runs on inside this block.

  "exact" (the default everywhere): the masked float32 sums in NumPy 2's summation order -- the clipping constants, and
  with them scales and integers, are the reference's bit for bit; 0.045 of one read of the tensor.
  "fast" (also MI355Q_OCTAV_FAST=1): one pass over HBM, a row / block stays in registers for all ten iterations, the
  sums as float32 partials combined by a tree -- tolerance class T2 (scales within 1e-6 relative, integers
  +-1 on <= 1e-5 of the elements; the reference pins neither NumPy nor its summation order). Units of 4 .. 65536
  elements (a multiple of 4) with an axis given; anything else runs on the exact kernels in either mode."""
  if mode not in ("exact", "fast"):
    raise ValueError("octav_mode must be 'exact' or 'fast'")
  before, _OCTAV_MODE[0] = _OCTAV_MODE[0], mode
  try:
    yield
  finally:
    _OCTAV_MODE[0] = before


def octav_clip(x: torch.Tensor, units: int, unit_len: int, bits: int, max_iter: int = 10,
               exponent_divisor: float = 3.0, early_stop: bool = True, axis_given: bool = True):
  """K5. Returns (clip float32[units], iterations int). ref: octav.py:30-112.

  `axis_given=False` is the TENSORWISE form (axis=None in the reference).
  """
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != units * unit_len:
    raise ValueError("shape view does not match numel")
  clip = rt.empty((units,), torch.float32)
  iters = rt.empty((1,), torch.int32)
  L = _ffi.lib()
  if axis_given and _octav_fast() and unit_len % 4 == 0 and 4 <= unit_len <= 65536 and x.data_ptr() % 16 == 0:
    # the opt-in one-read kernel (octav_mode("fast")): tolerance class T2 instead of NumPy's summation order
    nbytes = L.mi355q_octav_workspace_bytes(units, max_iter)
    ws = rt.empty((max(nbytes, 1),), torch.uint8)
    _ffi.check(L.mi355q_octav_clip_fast_f32(
        rt.ptr(x), units, unit_len, bits, max_iter, np.float32(exponent_divisor), 1 if early_stop else 0,
        rt.ptr(clip), rt.ptr(iters), rt.ptr(ws), nbytes, rt.stream_ptr()))
    return clip, iters
  nbytes = L.mi355q_octav_rows_workspace_bytes(units, unit_len, max_iter)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_octav_clip_f32(
      rt.ptr(x), units, unit_len, bits, max_iter, np.float32(exponent_divisor),
      1 if early_stop else 0, 1 if axis_given else 0, rt.ptr(clip), rt.ptr(iters), rt.ptr(ws),
      nbytes, rt.stream_ptr()))
  return clip, iters


def octav_clip_nd(x: torch.Tensor, outer: int, channels: int, inner: int, bits: int,
                  max_iter: int = 10, exponent_divisor: float = 3.0, early_stop: bool = True):
  """K5 over the [outer, channels, inner] view: one clipping constant per channel."""
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != outer * channels * inner:
    raise ValueError("shape view does not match numel")
  clip = rt.empty((channels,), torch.float32)
  iters = rt.empty((1,), torch.int32)
  L = _ffi.lib()
  nbytes = L.mi355q_octav_workspace_bytes(channels, max_iter)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_octav_clip_nd_f32(
      rt.ptr(x), outer, channels, inner, bits, max_iter, np.float32(exponent_divisor),
      1 if early_stop else 0, rt.ptr(clip), rt.ptr(iters), rt.ptr(ws), nbytes, rt.stream_ptr()))
  return clip, iters


def mse_scale_nd(x: torch.Tensor, outer: int, channels: int, inner: int,
                 multiplier: float) -> torch.Tensor:
  """a14 over the [outer, channels, inner] view: scale[c] = multiplier * sqrt(mean(x[:, c, :]**2))."""
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != outer * channels * inner:
    raise ValueError("shape view does not match numel")
  scale = rt.empty((channels,), torch.float32)
  _ffi.check(_ffi.lib().mi355q_mse_scale_nd_f32(rt.ptr(x), outer, channels, inner,
                                                np.float32(multiplier), rt.ptr(scale), rt.stream_ptr()))
  return scale


def mse_requant(x: torch.Tensor, units: int, unit_len: int, multiplier: float, bits: int,
                narrow: bool) -> tuple[torch.Tensor, torch.Tensor]:
  """a14 whole, contiguous units: (scale float32 [units], q int8 [units * unit_len]) -- the MSE scale in NumPy's order
  and clip(rint(x / scale)) with a zero zero point, one kernel where the unit length allows. ref: mse.py:100-128."""
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != units * unit_len:
    raise ValueError("shape view does not match numel")
  scale = rt.empty((units,), torch.float32)
  q = rt.empty(tuple(x.shape), torch.int8)
  _ffi.check(_ffi.lib().mi355q_mse_requant_f32(rt.ptr(x), units, unit_len, np.float32(multiplier), bits,
                                               1 if narrow else 0, rt.ptr(scale), rt.ptr(q), rt.stream_ptr()))
  return scale, q


def mse_scale(x: torch.Tensor, units: int, unit_len: int, multiplier: float) -> torch.Tensor:
  """a14. scale[u] = multiplier * sqrt(mean(x_u**2)). ref: mse.py:100-109."""
  rt.require_gpu()
  x = _f32(x)
  if x.numel() != units * unit_len:
    raise ValueError("shape view does not match numel")
  scale = rt.empty((units,), torch.float32)
  _ffi.check(_ffi.lib().mi355q_mse_scale_f32(rt.ptr(x), units, unit_len, np.float32(multiplier),
                                             rt.ptr(scale), rt.stream_ptr()))
  return scale


def hadamard_rotate(x: torch.Tensor, h: int) -> torch.Tensor:
  """K6. reshape(x, (-1, h)) @ (H_h / sqrt(h)), same shape as x. ref: hadamard_rotation.py:93-134."""
  rt.require_gpu()
  x = _f32(x)
  if h <= 0 or h & (h - 1):
    raise ValueError("Hadamard matrix size must be a power of 2. ")
  if x.numel() % h:
    raise ValueError("tensor size is not a multiple of the Hadamard size")
  out = torch.empty_like(x)
  _ffi.check(_ffi.lib().mi355q_hadamard_rotate_f32(rt.ptr(x), x.numel() // h, h, rt.ptr(out),
                                                   rt.stream_ptr()))
  return out


def gemm(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False,
         lower_only: bool = False) -> torch.Tensor:
  """MFMA GEMM on 2-D float32 / float64 device tensors: op(a) @ op(b)."""
  rt.require_gpu()
  if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.float64):
    raise TypeError("gemm expects matching float32 or float64 tensors")
  a, b = a.contiguous(), b.contiguous()
  m, k = (a.shape[1], a.shape[0]) if trans_a else a.shape
  k2, n = (b.shape[1], b.shape[0]) if trans_b else b.shape
  if k != k2:
    raise ValueError("inner dimensions do not match")
  c = torch.zeros((m, n), dtype=a.dtype, device=a.device)
  a_i, a_k = (1, a.shape[1]) if trans_a else (a.shape[1], 1)
  b_k, b_j = (1, b.shape[1]) if trans_b else (b.shape[1], 1)
  fn = _ffi.lib().mi355q_gemm_f32 if a.dtype == torch.float32 else _ffi.lib().mi355q_gemm_f64
  _ffi.check(fn(rt.ptr(a), a_i, a_k, rt.ptr(b), b_k, b_j, rt.ptr(c), n, 1, m, n, k, 1.0, 0.0,
                1 if lower_only else 0, rt.stream_ptr()))
  return c


def gptq_xtx(x: torch.Tensor, alpha: float) -> torch.Tensor:
  """K8. float64 [d, d] = alpha * (x^T x) for float32 x [n, d]. ref: gptq.py:100-107."""
  rt.require_gpu()
  x = _f32(x)
  n, d = x.shape
  h = rt.empty((d, d), torch.float64)
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_xtx_workspace_bytes(n, d)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_gptq_xtx_f32(rt.ptr(x), n, d, float(alpha), rt.ptr(h), rt.ptr(ws), nbytes,
                                   rt.stream_ptr()))
  return h


_XTX_SCRATCH: dict = {}      # (device index, d) -> uint8 scratch for products of <= 16384-token slabs


def gptq_xtx_accum(x: torch.Tensor, product: torch.Tensor | None) -> torch.Tensor:
  """product (float32 [d, d], lower-triangular part valid) (+)= x^T x for float32 x [n, d];
  None starts a new product. The scratch (bfloat16 planes of a slab / split-K partials, up to
  1.5 GiB at d = 16384) is kept per device and width: calibration calls this once per slab and
  Hessian, back to back on one stream."""
  rt.require_gpu()
  x = _f32(x)
  n, d = x.shape
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_xtx_accum_workspace_bytes(n, d)
  key = (x.device.index, d)
  ws = _XTX_SCRATCH.get(key)
  if ws is None or ws.numel() < nbytes:
    ws = _XTX_SCRATCH[key] = rt.empty((max(nbytes, L.mi355q_gptq_xtx_accum_workspace_bytes(16384, d), 1),), torch.uint8)
  fresh = product is None
  if fresh:
    product = rt.empty((d, d), torch.float32)
  _ffi.check(L.mi355q_gptq_xtx_accum_f32(rt.ptr(x), n, d, rt.ptr(product), 0 if fresh else 1, rt.ptr(ws),
                                         ws.numel(), rt.stream_ptr()))
  return product


def gptq_xtx_finish(product: torch.Tensor, alpha: float) -> torch.Tensor:
  """float64 [d, d] = alpha * product, both triangles (ref gptq.py:100-107's scaling)."""
  rt.require_gpu()
  d = product.shape[0]
  h = rt.empty((d, d), torch.float64)
  _ffi.check(_ffi.lib().mi355q_gptq_xtx_finish_f64(rt.ptr(product), d, float(alpha), rt.ptr(h), rt.stream_ptr()))
  return h


def release_scratch() -> None:
  """Gives the cached product scratch back (ParamsGenerator / Calibrator call this when done)."""
  _XTX_SCRATCH.clear()


def gptq_hessian_merge(h_cur: torch.Tensor, n_cur: float, h_new: torch.Tensor, n_new: float):
  """(h_cur*n_cur + h_new*n_new)/(n_cur+n_new), float64. ref: qsv_utils.py:71-88."""
  rt.require_gpu()
  out = torch.empty_like(h_cur)
  _ffi.check(_ffi.lib().mi355q_gptq_hessian_merge_f64(
      rt.ptr(h_cur.contiguous()), float(n_cur), rt.ptr(h_new.contiguous()), float(n_new),
      h_cur.shape[0], rt.ptr(out), rt.stream_ptr()))
  return out


def gptq_hinv(hessian: torch.Tensor, damp_factor: float = 0.01):
  """K9. Returns (hinv float32 [d,d], info int32[1]). ref: gptq.py:111-128."""
  rt.require_gpu()
  if hessian.dtype != torch.float64:
    hessian = hessian.to(torch.float64)
  hessian = hessian.contiguous()
  d = hessian.shape[0]
  hinv = rt.empty((d, d), torch.float32)
  info = rt.empty((1,), torch.int32)
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_hinv_workspace_bytes(d)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_gptq_hinv_f64(rt.ptr(hessian), d, float(damp_factor), rt.ptr(hinv),
                                    rt.ptr(info), rt.ptr(ws), nbytes, rt.stream_ptr()))
  return hinv, info


def gptq_hinv_from_product(product: torch.Tensor, alpha: float, damp_factor: float = 0.01):
  """K9 on hessian = alpha * product (float32 X^T X, lower triangle valid) without materializing the
  float64 Hessian; same (hinv, info) as gptq_hinv(gptq_xtx_finish(product, alpha))."""
  rt.require_gpu()
  d = product.shape[0]
  hinv = rt.empty((d, d), torch.float32)
  info = rt.empty((1,), torch.int32)
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_hinv_workspace_bytes(d)
  held = HinvWorkspace.current.pointer(nbytes) if HinvWorkspace.current is not None else None
  ws = None if held is not None else rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_gptq_hinv_from_product_f32(rt.ptr(_f32(product)), d, float(alpha), float(damp_factor), rt.ptr(hinv),
                                                 rt.ptr(info), held if held is not None else rt.ptr(ws), nbytes, rt.stream_ptr()))
  return hinv, info


class HinvWorkspace:
  """The workspace of the d >= 4096 inverses (5 GiB at d = 16384), allocated ahead of their first call on a helper
  thread: a fresh GiB of HBM costs its caller ~30 ms of hipMalloc, and whoever starts the first large inverse does so
  on a GPU that has just run dry (the end of calibration). mi355q_device_alloc runs without the interpreter lock and
  outside the framework's allocator (whose lock would stall every allocation of the feeding thread meanwhile).
  gptq_hinv_from_product() uses it while one is installed (`with`, or install() / release()); calls on one stream
  follow each other, so one workspace serves them all."""
  current = None

  def __init__(self, d: int, lanes: int = 1):
    """lanes = 2: room for the pair of large matrices gptq_hinv_from_product_batched keeps in flight."""
    import ctypes
    import threading
    rt.require_gpu()
    self.nbytes = int(_ffi.lib().mi355q_gptq_hinv_from_product_batched_workspace_bytes(lanes, d)) if lanes > 1 \
        else int(_ffi.lib().mi355q_gptq_hinv_workspace_bytes(d))
    self.d = d
    self._ptr = ctypes.c_void_p()
    self._status = 0
    self._device = torch.cuda.current_device()

    def work():
      torch.cuda.set_device(self._device)
      self._status = _ffi.lib().mi355q_device_alloc(self.nbytes, ctypes.byref(self._ptr))
    self._thread = threading.Thread(target=work, name="mi355q-hinv-workspace", daemon=True)
    self._thread.start()

  def pointer(self, nbytes: int):
    """Device pointer when the workspace is there and large enough, else None (the caller allocates its own)."""
    self._thread.join()
    return self._ptr if self._status == 0 and self._ptr.value and nbytes <= self.nbytes else None

  def install(self):
    HinvWorkspace.current = self
    return self

  def release(self) -> None:
    """Call with the stream that used it drained (hipFree waits for the device anyway)."""
    if HinvWorkspace.current is self:
      HinvWorkspace.current = None
    self._thread.join()
    if self._ptr.value:
      _ffi.lib().mi355q_device_free(self._ptr)
      self._ptr.value = None

  def __enter__(self):
    return self.install()

  def __exit__(self, *exc):
    self.release()


def gptq_hinv_batched(hessians, damp_factor: float = 0.01):
  """K9 for several Hessians of one order: [(hinv float32 [d, d], info int32[1]), ...], the same
  bits as gptq_hinv on each (for d < 4096 the independent chains interleave on a stream pool)."""
  import ctypes
  rt.require_gpu()
  hs = [h.contiguous() if h.dtype == torch.float64 else h.to(torch.float64).contiguous() for h in hessians]
  if not hs:
    return []
  d = hs[0].shape[0]
  if any(tuple(h.shape) != (d, d) for h in hs):
    raise ValueError("all Hessians of a batch must have one order")
  n = len(hs)
  hinv = rt.empty((n, d, d), torch.float32)
  info = rt.empty((n,), torch.int32)
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_hinv_batched_workspace_bytes(n, d)
  held = HinvWorkspace.current.pointer(nbytes) if HinvWorkspace.current is not None else None   # (calls on one stream follow each other)
  ws = None if held is not None else rt.empty((max(nbytes, 1),), torch.uint8)
  src = (ctypes.c_void_p * n)(*[h.data_ptr() for h in hs])
  dst = (ctypes.c_void_p * n)(*[hinv[i].data_ptr() for i in range(n)])
  _ffi.check(L.mi355q_gptq_hinv_f64_batched(src, n, d, float(damp_factor), dst, rt.ptr(info),
                                            held if held is not None else rt.ptr(ws), nbytes, rt.stream_ptr()))
  return [(hinv[i], info[i:i + 1]) for i in range(n)]




def gptq_hinv_from_product_batched(forms, damp_factor: float = 0.01):
  """K9 for several Hessians of one order handed over as (product float32 [d, d], alpha) pairs (what calibration leaves
  behind: gptq.HessianAccumulator.product_form): [(hinv float32 [d, d], info int32[1]), ...], the same bits as
  gptq_hinv_from_product on each (mi355q_gptq_hinv_from_product_f32_batched; MI355Q_HINV_PAIRS=1: two d >= 4096 matrices in flight)."""
  import ctypes
  rt.require_gpu()
  forms = [(_f32(p), float(a)) for p, a in forms]
  if not forms:
    return []
  d = forms[0][0].shape[0]
  if any(tuple(p.shape) != (d, d) for p, _ in forms):
    raise ValueError("all Hessians of a batch must have one order")
  n = len(forms)
  hinvs = [rt.empty((d, d), torch.float32) for _ in range(n)]      # (separate allocations: each is given back with its last reader)
  info = rt.empty((n,), torch.int32)
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_hinv_from_product_batched_workspace_bytes(n, d)
  held = HinvWorkspace.current.pointer(nbytes) if HinvWorkspace.current is not None else None
  ws = None if held is not None else rt.empty((max(nbytes, 1),), torch.uint8)
  src = (ctypes.c_void_p * n)(*[p.data_ptr() for p, _ in forms])
  alphas = (ctypes.c_double * n)(*[a for _, a in forms])
  dst = (ctypes.c_void_p * n)(*[h.data_ptr() for h in hinvs])
  _ffi.check(L.mi355q_gptq_hinv_from_product_f32_batched(src, alphas, n, d, float(damp_factor), dst, rt.ptr(info),
                                                         held if held is not None else rt.ptr(ws), nbytes, rt.stream_ptr()))
  return [(hinvs[i], info[i:i + 1]) for i in range(n)]


@_contextlib.contextmanager
def hessian_product(mode: str = "exact"):
  """The kernel GPTQ's Hessian products (mi355q_gptq_xtx_f32 / _accum_f32) run on inside this block.

  "exact" (the default everywhere): every float32 product from the exact three-way bfloat16 split, six
  bf16 MFMA products (xtx_bf16x3.hip) -- float32-sgemm-class like the reference's x.T.dot(x), and what the
  recorded parity rates are taken with (the d = 16384 chain reproduces the oracle's integers).
  "fast": the two-way float16 split, three f16 MFMA products, 22-23 of the 24 mantissa bits, 1.8 x faster;
  1.2e-3 of the d = 16384 integers then differ from the oracle's (profiles/r04_parity_rates.txt). The
  library reads MI355Q_XTX_F16X2 per call, which is what this sets."""
  import os
  if mode not in ("exact", "fast"):
    raise ValueError("hessian_product mode must be 'exact' or 'fast'")
  before = os.environ.get("MI355Q_XTX_F16X2")
  if mode == "fast":
    os.environ["MI355Q_XTX_F16X2"] = "1"
  else:
    os.environ.pop("MI355Q_XTX_F16X2", None)
  try:
    yield
  finally:
    if before is None:
      os.environ.pop("MI355Q_XTX_F16X2", None)
    else:
      os.environ["MI355Q_XTX_F16X2"] = before


def gptq_apply(w: torch.Tensor, hinv: torch.Tensor, scale: torch.Tensor,
               zero_point: torch.Tensor | None, scale_mode: int, block_size: int, bits: int,
               narrow: bool, zp_via_f64: bool, diff_bits: int) -> torch.Tensor:
  """K10. int8 [rows, d] (int32 for targets of 9..32 bits). ref: gptq.py:131-216."""
  rt.require_gpu()
  w = _f32(w)
  rows, d = w.shape
  wide = bits > 8         # int32 [rows, d] from mi355q_gptq_apply_wide_f32 (9..16 bits: the caller narrows the container; 17..32: int32 is the container)
  q = rt.empty((rows, d), torch.int32 if wide else torch.int8)
  if zero_point is not None:
    zero_point = zero_point.to(torch.int32).contiguous()
  L = _ffi.lib()
  nbytes = L.mi355q_gptq_apply_workspace_bytes(rows, d)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check((L.mi355q_gptq_apply_wide_f32 if wide else L.mi355q_gptq_apply_f32)(
      rt.ptr(w), rows, d, rt.ptr(_f32(hinv)), rt.ptr(scale.contiguous()),
      1 if scale.dtype == torch.float64 else 0, rt.ptr(zero_point), scale_mode, block_size, bits,
      1 if narrow else 0, 1 if zp_via_f64 else 0, diff_bits, rt.ptr(q), rt.ptr(ws), nbytes,
      rt.stream_ptr()))
  return q


# ------------------------------------------------------------------------ OSCAR (f4) ---
def _f64_dev(a) -> torch.Tensor:
  return rt.to_device(np.ascontiguousarray(a, dtype=np.float64))


def oscar_col_sumsq(x: torch.Tensor, mean: bool) -> torch.Tensor:
  """x float32 [rows, d] -> float64 [d]: sum_r x[r, j]^2, rows in order (/ rows when mean)."""
  rt.require_gpu()
  x = _f32(x)
  rows, d = x.shape
  out = rt.empty((d,), torch.float64)
  _ffi.check(_ffi.lib().mi355q_oscar_col_sumsq_f32(rt.ptr(x), rows, d, int(mean), rt.ptr(out),
                                                   rt.stream_ptr()))
  return out


def oscar_group_terms(w: torch.Tensor, s: torch.Tensor, g: int):
  """(sums float64 [d/g], winner int32 [d/g, n], wsq float64 [d/g, n]) for scales s float64 [d]."""
  rt.require_gpu()
  w = _f32(w)
  n, d = w.shape
  groups = d // g
  top2 = rt.empty((groups * n,), torch.float64)
  winner = rt.empty((groups, n), torch.int32)
  wsq = rt.empty((groups, n), torch.float64)
  sums = rt.empty((groups,), torch.float64)
  _ffi.check(_ffi.lib().mi355q_oscar_group_terms_f32(
      rt.ptr(w), rt.ptr(s), n, d, g, rt.ptr(top2), rt.ptr(winner), rt.ptr(wsq), rt.ptr(sums),
      rt.stream_ptr()))
  return sums, winner, wsq


def oscar_winner_energy(winner: torch.Tensor, wsq: torch.Tensor, d: int, g: int) -> torch.Tensor:
  rt.require_gpu()
  n = winner.shape[1]
  eff = rt.empty((d,), torch.float64)
  _ffi.check(_ffi.lib().mi355q_oscar_winner_energy_f64(rt.ptr(winner), rt.ptr(wsq), n, d, g,
                                                       rt.ptr(eff), rt.stream_ptr()))
  return eff


def oscar_clip_bounds(w: torch.Tensor, s: torch.Tensor, masses: torch.Tensor, g: int,
                      u: torch.Tensor, noise: torch.Tensor, qmax: int, blockwise_scale: bool = False,
                      want_bounds: bool = True, want_scale: bool = False, want_rows_left: bool = False):
  """Optimal clip bound (float64) of every g-element segment of the flattened weight and / or
  the symmetric scale derived from it (float64 values; float16-representable when blockwise).
  `want_rows_left`: also the per-segment flags of the rows the prefix kernel handed to the full sort + scan
  (uint8 [n * d / g]; None when the call took the full route for every segment) -- for the tests and the bench."""
  import ctypes
  import os
  rt.require_gpu()
  w = _f32(w)
  n, d = w.shape
  need = ctypes.c_size_t(0)
  _ffi.check(_ffi.lib().mi355q_oscar_clip_workspace_bytes(n, d, g, ctypes.byref(need)))
  ws = rt.empty((need.value,), torch.uint8)
  bounds = rt.empty((n * d // g,), torch.float64) if want_bounds else None
  scale = rt.empty((n * d // g,), torch.float64) if want_scale else None
  _ffi.check(_ffi.lib().mi355q_oscar_clip_bounds_f32(
      rt.ptr(w), rt.ptr(s), rt.ptr(masses), n, d, g, rt.ptr(u), rt.ptr(noise), int(qmax),
      int(blockwise_scale), rt.ptr(bounds), rt.ptr(scale), rt.ptr(ws), need.value, rt.stream_ptr()))
  if want_rows_left:
    took_prefix = (g == d and 384 <= g <= 16384 and qmax >= 7 and os.environ.get("MI355Q_OSCAR_PREFIX", "")[:1] != "0")
    slab = (n * d * 8 + 255) // 256 * 256
    return bounds, scale, (ws[4 * slab:4 * slab + n * d // g].clone() if took_prefix else None)
  return bounds, scale


def oscar_quantize(w: torch.Tensor, s: torch.Tensor, scale: torch.Tensor, g: int, qlo: int,
                   qhi: int) -> torch.Tensor:
  rt.require_gpu()
  w = _f32(w)
  n, d = w.shape
  out = rt.empty((n, d), torch.int8)
  _ffi.check(_ffi.lib().mi355q_oscar_quantize_f32(rt.ptr(w), rt.ptr(s), rt.ptr(scale), n, d, g, qlo,
                                                  qhi, rt.ptr(out), rt.stream_ptr()))
  return out


# ------------------------------------------------------- dequantized weight recovery ---
def dwr_scales(w: torch.Tensor, g: int, rounded: bool) -> torch.Tensor:
  """float64 [n*d/g]: smallest positive step of every g-element segment's sorted magnitudes."""
  import ctypes
  rt.require_gpu()
  w = _f32(w)
  n, d = w.shape
  need = ctypes.c_size_t(0)
  _ffi.check(_ffi.lib().mi355q_oscar_clip_workspace_bytes(n, d, g, ctypes.byref(need)))
  ws = rt.empty((need.value,), torch.uint8)
  out = rt.empty((n * d // g,), torch.float64)
  _ffi.check(_ffi.lib().mi355q_dwr_scales_f32(rt.ptr(w), n, d, g, int(rounded), rt.ptr(out), rt.ptr(ws),
                                              need.value, rt.stream_ptr()))
  return out


def dwr_max_error(w: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, g: int) -> float:
  """max |q * scale - w| over the tensor (float64; NaN if any element is NaN)."""
  rt.require_gpu()
  w = _f32(w)
  out = rt.empty((1,), torch.float64)
  _ffi.check(_ffi.lib().mi355q_dwr_max_error_f32(rt.ptr(w), rt.ptr(q), rt.ptr(scale), w.numel(), g,
                                                 rt.ptr(out), rt.stream_ptr()))
  return float(out.item())


# ------------------------------------------------------- tensor comparison (model validation) ---
# (include/mi355q.h, mi355q_compare_pair / mi355q_compare_result)
COMPARE_KINDS = {"f32": 0, "f16": 1, "bf16": 2, "i8": 3, "i16": 4, "i32": 5, "i4": 6, "i2": 7}
COMPARE_PAIR_DTYPE = np.dtype([("reference", "<u8"), ("target", "<u8"), ("n", "<i8"), ("kind", "<i4"),
                               ("diff_bits", "<i4"), ("channels", "<i8"), ("inner", "<i8"), ("scale", "<u8"),
                               ("zero_point", "<u8")])
COMPARE_RESULT_DTYPE = np.dtype([("sum_sq_diff", "<f4"), ("sum_ref_sq", "<f4"), ("sum_kl", "<f4"),
                                 ("median_lo", "<f4"), ("median_hi", "<f4"), ("reserved", "<f4"),
                                 ("dot_tr", "<f8"), ("dot_tt", "<f8"), ("dot_rr", "<f8")])
COMPARE_MEDIAN = 1
COMPARE_NO_KL = 2


class CompareTarget:
  """The target operand of a comparison in its stored form, on the device.

  `data`: float32 / float16 / bfloat16 / int8 / int16 / int32 tensor, or uint8 packed bytes with
  `packed_bits` 4 or 2. Integer targets carry `scale` (float32, `channels` entries) and optional `zero_point`
  (int32); element e uses entry (e // inner) % channels. `diff_bits` is the width in which q - zp is formed.
  """

  def __init__(self, data: torch.Tensor, n: int, kind: str, scale: torch.Tensor | None = None,
               zero_point: torch.Tensor | None = None, channels: int = 1, inner: int = 1, diff_bits: int = 32):
    if kind not in COMPARE_KINDS:
      raise ValueError(f"unknown target kind {kind!r}")
    if COMPARE_KINDS[kind] >= COMPARE_KINDS["i8"] and scale is None:
      raise ValueError("integer targets need scales")
    self.data, self.n, self.kind = data.contiguous(), int(n), kind
    self.scale = None if scale is None else _f32(scale)
    self.zero_point = None if zero_point is None else zero_point.to(torch.int32).contiguous()
    self.channels, self.inner, self.diff_bits = int(channels), int(inner), int(diff_bits)


def _pair_record(rec, reference: torch.Tensor, target: CompareTarget) -> None:
  rec["reference"], rec["target"], rec["n"] = reference.data_ptr(), target.data.data_ptr(), target.n
  rec["kind"], rec["diff_bits"] = COMPARE_KINDS[target.kind], target.diff_bits
  rec["channels"], rec["inner"] = target.channels, target.inner
  rec["scale"] = 0 if target.scale is None else target.scale.data_ptr()
  rec["zero_point"] = 0 if target.zero_point is None else target.zero_point.data_ptr()


def compare(pairs, median: bool = True, kl: bool = True) -> np.ndarray:
  """Comparison sums of (float32 reference, CompareTarget) pairs -> COMPARE_RESULT_DTYPE records (host).

  One pair goes through mi355q_compare_f32 (its descriptor in the kernel arguments), several through one
  mi355q_compare_f32_batched launch set. Synchronizes (the records are copied to the host).
  """
  rt.require_gpu()
  L = _ffi.lib()
  pairs = [(_f32(r).view(-1), t) for r, t in pairs]
  for r, t in pairs:
    if r.numel() != t.n:
      raise ValueError("data1 & data2 must be of the same size")
  out = np.zeros(len(pairs), COMPARE_RESULT_DTYPE)
  live = [(r, t) for r, t in pairs if t.n > 0]
  if not live:
    return out
  flags = (COMPARE_MEDIAN if median else 0) | (0 if kl else COMPARE_NO_KL)
  res = rt.empty((len(live) * COMPARE_RESULT_DTYPE.itemsize,), torch.uint8)
  chunks = sum(L.mi355q_compare_chunks(t.n) for _, t in live)
  nbytes = L.mi355q_compare_workspace_bytes(len(live), chunks)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  if len(live) == 1:
    r, t = live[0]
    _ffi.check(L.mi355q_compare_f32(
        rt.ptr(r), rt.ptr(t.data), t.n, COMPARE_KINDS[t.kind], t.diff_bits, t.channels, t.inner, rt.ptr(t.scale),
        rt.ptr(t.zero_point), flags, rt.ptr(res), rt.ptr(ws), nbytes, rt.stream_ptr()))
  else:
    table = np.zeros(len(live), COMPARE_PAIR_DTYPE)
    for i, (r, t) in enumerate(live):
      _pair_record(table[i], r, t)
    dev_table = torch.from_numpy(table.view(np.uint8).copy()).to(rt.device())
    _ffi.check(L.mi355q_compare_f32_batched(rt.ptr(dev_table), len(live), chunks, flags, rt.ptr(res), rt.ptr(ws),
                                            nbytes, rt.stream_ptr()))
  host = res.cpu().numpy().view(COMPARE_RESULT_DTYPE)     # (synchronizes: every operand above is still alive)
  out[[i for i, (_, t) in enumerate(pairs) if t.n > 0]] = host
  return out


def weight_delta(reference: torch.Tensor, target: CompareTarget) -> torch.Tensor:
  """float32 [n] = reference - dequant(target), the target dequantized in registers by the rule of `compare`
  (no nan_to_num: values pass through as they are). Does not synchronize."""
  rt.require_gpu()
  reference = _f32(reference).view(-1)
  if reference.numel() != target.n:
    raise ValueError("data1 & data2 must be of the same size")
  out = rt.empty((target.n,), torch.float32)
  _ffi.check(_ffi.lib().mi355q_weight_delta_f32(
      rt.ptr(reference), rt.ptr(target.data), target.n, COMPARE_KINDS[target.kind], target.diff_bits, target.channels,
      target.inner, rt.ptr(target.scale), rt.ptr(target.zero_point), rt.ptr(out), rt.stream_ptr()))
  return out


def weight_delta_transformed(reference: torch.Tensor, target: CompareTarget, d: int,
                             multiplier: torch.Tensor | None = None, hadamard_size: int = 0) -> torch.Tensor:
  """float32 [n]: the delta of a [n // d, d] weight whose quantized op reads a transformed activation
  (mi355q_weight_delta_transformed_f32). With `multiplier` (float32 [d]): reference - dequant(target) * multiplier
  per column, the product rounded to float32 before the subtraction. With `hadamard_size` h > 1 (a power of two
  <= 16384 that divides d): reference - hadamard_rotate(dequant(target), h), the butterfly network of
  `hadamard_rotate` fed from the stored target in one pass. With neither it equals `weight_delta`; both at once is
  refused. Does not synchronize."""
  rt.require_gpu()
  reference = _f32(reference).view(-1)
  if reference.numel() != target.n:
    raise ValueError("data1 & data2 must be of the same size")
  d, h = int(d), int(hadamard_size)
  if d < 1 or target.n % d:
    raise ValueError(f"tensor size {target.n} is not a multiple of the row length {d}")
  if h < 0 or h & (h - 1):
    raise ValueError("Hadamard matrix size must be a power of 2. ")
  if h > 1 and (h > 16384 or d % h):
    raise ValueError(f"Hadamard size {h} must divide the row length {d} and be at most 16384")
  if multiplier is not None:
    if h > 1:
      raise ValueError("a multiplier and a Hadamard rotation at once are not supported")
    multiplier = _f32(multiplier).view(-1)
    if multiplier.numel() != d:
      raise ValueError(f"multiplier has {multiplier.numel()} elements, the row length is {d}")
  out = rt.empty((target.n,), torch.float32)
  _ffi.check(_ffi.lib().mi355q_weight_delta_transformed_f32(
      rt.ptr(reference), rt.ptr(target.data), target.n, COMPARE_KINDS[target.kind], target.diff_bits, target.channels,
      target.inner, rt.ptr(target.scale), rt.ptr(target.zero_point), d, rt.ptr(multiplier), h, rt.ptr(out),
      rt.stream_ptr()))
  return out


def quadform_rows(a: torch.Tensor, product: torch.Tensor, alpha: float) -> torch.Tensor:
  """float64 [rows]: alpha * a_r Psym a_r^T for float32 a [rows, d] and the symmetric matrix whose LOWER triangle
  is `product` (float32 [d, d], e.g. HessianAccumulator.product_form(); the upper triangle is never read and
  `product` is not modified). Does not synchronize."""
  rt.require_gpu()
  a, product = _f32(a), _f32(product)
  if a.dim() != 2 or product.dim() != 2 or product.shape[0] != product.shape[1] or product.shape[0] != a.shape[1]:
    raise ValueError(f"expected a [rows, d] and product [d, d], got {tuple(a.shape)} and {tuple(product.shape)}")
  rows, d = a.shape
  out = rt.empty((rows,), torch.float64)
  L = _ffi.lib()
  nbytes = L.mi355q_quadform_rows_workspace_bytes(rows, d)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_quadform_rows_f32(rt.ptr(a), rows, d, rt.ptr(product), float(alpha), rt.ptr(out), rt.ptr(ws),
                                        nbytes, rt.stream_ptr()))
  return out


# ------------------------------------------------------- integer execution of FULLY_CONNECTED ---
# (include/mi355q.h, "Integer execution of a quantized FULLY_CONNECTED op")
QFC_BLOCKS = (32, 64, 128, 256)
QFC_MAX_D = 65536


def qfc_quantize_rows(x2d: torch.Tensor):
  """Dynamic-range activation rows: (q int8 [n, d], scale float32 [n]) of a float32 [n, d] device tensor, with
  scale = max|row| / 127 and q = clamp(round_half_away_from_zero(x * (127 / max|row|)), -127, 127); an all-zero row
  has scale 1, a row with a NaN or an infinity scale NaN and q = 0. Does not synchronize."""
  rt.require_gpu()
  x2d = _f32(x2d)
  if x2d.dim() != 2:
    raise ValueError(f"expected a [n, d] tensor, got {tuple(x2d.shape)}")
  n, d = x2d.shape
  q, scale = rt.empty((n, d), torch.int8), rt.empty((n,), torch.float32)
  _ffi.check(_ffi.lib().mi355q_qfc_quantize_rows_f32(rt.ptr(x2d), n, d, rt.ptr(q), rt.ptr(scale), rt.stream_ptr()))
  return q, scale


def _qfc_block(who: str, xq: torch.Tensor, dtype, target: CompareTarget, rows: int, d: int) -> int:
  """The argument checks qfc_forward and qfc_forward_i16 share; returns the block size the scale view means (0: per
  tensor or per channel)."""
  if target.kind not in ("i8", "i4", "i2"):
    raise ValueError(f"{who} needs an i8 / i4 / i2 weight, got {target.kind!r}")
  if xq.dtype != dtype or not xq.is_cuda or xq.dim() != 2 or xq.shape[1] != d:
    name = str(dtype).replace("torch.", "")
    raise TypeError(f"expected an {name} [n, {d}] device tensor, got {xq.dtype} {tuple(xq.shape)} on {xq.device}")
  if target.n != rows * d:
    raise ValueError(f"the weight has {target.n} elements, expected {rows} x {d}")
  if target.zero_point is not None and bool(torch.any(target.zero_point != 0)):
    raise ValueError("the weight's zero point must be 0")
  if target.channels == 1:
    block = 0
  elif target.channels == rows and target.inner == d:
    block = 0
  elif target.inner in QFC_BLOCKS and target.channels * target.inner == rows * d:
    block = target.inner
  else:
    raise ValueError(f"scale view ({target.channels} channels, inner {target.inner}) is neither per tensor, per channel"
                     f" nor blockwise over a [{rows}, {d}] weight")
  if target.scale.numel() != target.channels:
    raise ValueError("scale must have one entry per channel")
  return block


def qfc_forward(xq: torch.Tensor, x_scale: torch.Tensor, x_zero_point: int, target: CompareTarget, rows: int, d: int,
                want_acc: bool = False):
  """The integer FULLY_CONNECTED product of int8 activations xq [n, d] and the stored integer weight [rows, d] of
  `target` (kind i8 / i4 / i2, as the validators build it), rescaled to float32 [n, rows]:
  y = float(Sum_k (xq - x_zero_point) q_w) * (x_scale * w_scale), with one int32 accumulator per block under
  blockwise scales (added in float32 in ascending order). The pre-bias product: bias, fused activation and the
  requantization of the output do not enter. `x_scale` holds 1 or n float32 entries. The scale view of `target`
  decides the granularity: channels = 1 per tensor; channels = rows with inner = d per channel; inner = a block size
  blockwise. Returns y, or (y, acc int32 [n, rows]) with `want_acc` (not with blockwise scales). Does not
  synchronize."""
  rt.require_gpu()
  rows, d = int(rows), int(d)
  block = _qfc_block("qfc_forward", xq, torch.int8, target, rows, d)
  # (no .contiguous(): a misaligned view is still dense, and the library routes on the address)
  n = xq.shape[0]
  x_scale = _f32(x_scale).view(-1)
  y = rt.empty((n, rows), torch.float32)
  acc = rt.empty((n, rows), torch.int32) if want_acc else None
  L = _ffi.lib()
  nbytes = L.mi355q_qfc_forward_workspace_bytes(rows, d, block)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  if not xq.is_contiguous():
    xq = xq.contiguous()
  _ffi.check(L.mi355q_qfc_forward_i8(rt.ptr(xq), n, d, rt.ptr(x_scale), x_scale.numel(), int(x_zero_point),
                                     rt.ptr(target.data), COMPARE_KINDS[target.kind], rows, rt.ptr(target.scale),
                                     target.scale.numel(), block, rt.ptr(y), rt.ptr(acc), rt.ptr(ws), nbytes,
                                     rt.stream_ptr()))
  return (y, acc) if want_acc else y


def qfc_forward_i16(xq: torch.Tensor, x_scale: torch.Tensor, target: CompareTarget, rows: int, d: int,
                    want_acc: bool = False):
  """The integer FULLY_CONNECTED product of int16 activations xq [n, d] (symmetric: no zero point) and the stored
  integer weight [rows, d] of `target`, as qfc_forward reads it: acc = Sum_k xq q_w exact in int64 and
  y = float32(float64(acc) * float64(x_scale * w_scale)), the scale product in float32; with blockwise scales one
  exact accumulator per block, rescaled so and added in float32 in ascending order (include/mi355q.h, "Integer
  execution, int16 activations"). `x_scale` holds 1 or n float32 entries. Returns y float32 [n, rows], or
  (y, acc int64 [n, rows]) with `want_acc` (not with blockwise scales). Does not synchronize."""
  rt.require_gpu()
  rows, d = int(rows), int(d)
  block = _qfc_block("qfc_forward_i16", xq, torch.int16, target, rows, d)
  n = xq.shape[0]
  x_scale = _f32(x_scale).view(-1)
  y = rt.empty((n, rows), torch.float32)
  acc = rt.empty((n, rows), torch.int64) if want_acc else None
  L = _ffi.lib()
  nbytes = L.mi355q_qfc_forward_i16_workspace_bytes(rows, d, block)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  if not xq.is_contiguous():
    xq = xq.contiguous()
  _ffi.check(L.mi355q_qfc_forward_i16(rt.ptr(xq), n, d, rt.ptr(x_scale), x_scale.numel(), rt.ptr(target.data),
                                      COMPARE_KINDS[target.kind], rows, rt.ptr(target.scale), target.scale.numel(),
                                      block, rt.ptr(y), rt.ptr(acc), rt.ptr(ws), nbytes, rt.stream_ptr()))
  return (y, acc) if want_acc else y


# (include/mi355q.h, "Integer execution, through to the stored output")
FUSED_NONE, FUSED_RELU, FUSED_RELU_N1_TO_1, FUSED_RELU6 = 0, 1, 2, 3
FUSED_ACTIVATION_NAMES = {FUSED_NONE: "NONE", FUSED_RELU: "RELU", FUSED_RELU_N1_TO_1: "RELU_N1_TO_1", FUSED_RELU6: "RELU6"}
QFC_SHIFT_RANGE = {8: (-31, 30), 16: (-31, 14)}


def _round_half_away(v: float) -> int:
  return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def quantize_multiplier(real: float) -> tuple:
  """(M, shift) with real ~ M * 2^(shift - 31), host only: 0 -> (0, 0); otherwise real = frac * 2^exp (frexp,
  0.5 <= frac < 1), M = round_half_away(frac * 2^31), M == 2^31 becomes (2^30, exp + 1); exp < -31 gives (0, 0), and
  exp > 30 raises ValueError."""
  real = float(real)
  if not math.isfinite(real) or real < 0.0:
    raise ValueError(f"the real multiplier must be finite and not negative (got {real})")
  if real == 0.0:
    return 0, 0
  frac, exp = math.frexp(real)
  m = _round_half_away(frac * float(1 << 31))      # (frac * 2^31 is exact in float64)
  if m == 1 << 31:
    m, exp = 1 << 30, exp + 1
  if exp < -31:
    return 0, 0
  if exp > 30:
    raise ValueError(f"the real multiplier {real} needs a left shift of {exp} > 30")
  return m, exp


def activation_range(fused: int, s_y: float, zp_y: int, bits: int) -> tuple:
  """(act_min, act_max): the integer range of a fused activation on the output grid (s_y, zp_y) of `bits` (8 or 16).
  NONE: the type's range; RELU: (max(qmin, zp_y), qmax); RELU6 / RELU_N1_TO_1: zp_y + round_half_away(f / s_y) of
  their float bounds, clamped to the type. Any other code raises ValueError."""
  if bits not in (8, 16):
    raise ValueError(f"bits must be 8 or 16 (got {bits})")
  qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
  fused, zp_y = int(fused), int(zp_y)

  def grid(f: float) -> int:
    return min(max(zp_y + _round_half_away(f / float(s_y)), qmin), qmax)
  if fused == FUSED_NONE:
    return qmin, qmax
  if fused == FUSED_RELU:
    return max(qmin, zp_y), qmax
  if fused == FUSED_RELU6:
    return grid(0.0), grid(6.0)
  if fused == FUSED_RELU_N1_TO_1:
    return grid(-1.0), grid(1.0)
  raise ValueError(f"fused activation {fused} is neither NONE, RELU, RELU_N1_TO_1 nor RELU6")


class QfcMultipliers:
  """Checked multiplier and shift tables on the device (qfc_multipliers): what qfc_output / qfc_output_i16 take in
  place of host tables, so that repeated calls for one op upload them once."""

  def __init__(self, multiplier: torch.Tensor, shift: torch.Tensor, rows: int, bits: int):
    self.multiplier, self.shift, self.rows, self.bits = multiplier, shift, rows, bits


def qfc_multipliers(multiplier, shift, rows: int, bits: int) -> QfcMultipliers:
  """The host tables `multiplier` / `shift` (1 or rows entries each) of an op with `bits`-bit activations, checked
  as qfc_output (8) / qfc_output_i16 (16) check them, on the device."""
  if bits not in QFC_SHIFT_RANGE:
    raise ValueError(f"bits must be 8 or 16 (got {bits})")
  return _qfc_output_tables("qfc_multipliers", multiplier, shift, int(rows), bits)


def _qfc_output_tables(who: str, multiplier, shift, rows: int, bits: int) -> QfcMultipliers:
  """The host tables of multipliers and shifts, checked (M >= 0, shift within the entry's range), as device int32."""
  if isinstance(multiplier, QfcMultipliers):
    if shift is not None or multiplier.rows != rows or multiplier.bits != bits:
      raise ValueError(f"{who}: the prepared multipliers are for {multiplier.rows} rows and {multiplier.bits}-bit"
                       f" activations (and take no `shift` beside them), not for {rows} rows and {bits} bits")
    return multiplier
  m = np.asarray(multiplier, np.int64).reshape(-1)
  s = np.asarray(shift, np.int64).reshape(-1)
  if m.size != s.size or m.size not in (1, rows):
    raise ValueError(f"{who}: multiplier and shift need 1 or rows = {rows} entries each (got {m.size} and {s.size})")
  lo, hi = QFC_SHIFT_RANGE[bits]
  if np.any(m < 0) or np.any(m > 0x7FFFFFFF):
    raise ValueError(f"{who}: a multiplier is outside [0, 2^31 - 1]")
  if np.any(s < lo) or np.any(s > hi):
    raise ValueError(f"{who}: a shift is outside [{lo}, {hi}]")
  return QfcMultipliers(rt.to_device(m.astype(np.int32)), rt.to_device(s.astype(np.int32)), rows, bits)


def _qfc_output_common(who: str, xq, dtype, target: CompareTarget, rows: int, d: int, bias, bias_dtype):
  if _qfc_block(who, xq, dtype, target, rows, d) != 0:
    raise ValueError(f"{who}: a static op has one accumulator per output; blockwise scales are not available")
  if bias is not None:
    if not isinstance(bias, torch.Tensor):
      bias = rt.to_device(np.ascontiguousarray(np.asarray(bias).reshape(-1)))
    if bias.dtype != bias_dtype or not bias.is_cuda or bias.numel() != rows:
      name = str(bias_dtype).replace("torch.", "")
      raise TypeError(f"{who}: the bias must be {name} with {rows} entries, got {bias.dtype} with {bias.numel()}")
    bias = bias.contiguous().view(-1)
  return xq if xq.is_contiguous() else xq.contiguous(), bias


def qfc_output(xq: torch.Tensor, x_zero_point: int, target: CompareTarget, rows: int, d: int, bias, multiplier, shift,
               out_zero_point: int, act_min: int, act_max: int) -> torch.Tensor:
  """What a static int8 FULLY_CONNECTED op stores: int8 [n, rows] =
  clamp(mbqm32(sat32(Sum_k (xq - x_zero_point) q_w + bias), M, s) + out_zero_point, act_min, act_max) of int8
  activations xq [n, d] and the stored integer weight of `target` (per tensor or per channel, as ops.qfc_forward
  reads it); `bias` None or int32 [rows] (array or device tensor); `multiplier` / `shift` host tables of 1 or rows
  entries (quantize_multiplier), M >= 0 and shift in [-31, 30], or qfc_multipliers' result with `shift` None.
  include/mi355q.h, "Integer execution, through to the stored output". Does not synchronize."""
  rt.require_gpu()
  rows, d = int(rows), int(d)
  xq, bias = _qfc_output_common("qfc_output", xq, torch.int8, target, rows, d, bias, torch.int32)
  tables = _qfc_output_tables("qfc_output", multiplier, shift, rows, 8)
  m_dev, s_dev = tables.multiplier, tables.shift
  n = xq.shape[0]
  q = rt.empty((n, rows), torch.int8)
  L = _ffi.lib()
  nbytes = L.mi355q_qfc_output_workspace_bytes(rows, d)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_qfc_output_i8(rt.ptr(xq), n, d, int(x_zero_point), rt.ptr(target.data), COMPARE_KINDS[target.kind],
                                    rows, rt.ptr(bias), rt.ptr(m_dev), rt.ptr(s_dev), m_dev.numel(), int(out_zero_point),
                                    int(act_min), int(act_max), rt.ptr(q), rt.ptr(ws), nbytes, rt.stream_ptr()))
  return q


def qfc_output_i16(xq: torch.Tensor, target: CompareTarget, rows: int, d: int, bias, multiplier, shift, act_min: int,
                   act_max: int) -> torch.Tensor:
  """What a static int16-activation FULLY_CONNECTED op stores: int16 [n, rows] =
  clamp((clamp(Sum_k xq q_w + bias, -2^47, 2^47 - 1) * Mr + 2^(T - 1)) >> T, act_min, act_max) with Mr the multiplier
  rounded to 15 bits and T = 15 - shift; `bias` None or int64 [rows]; M >= 0 and shift in [-31, 14]; no zero points.
  Does not synchronize."""
  rt.require_gpu()
  rows, d = int(rows), int(d)
  xq, bias = _qfc_output_common("qfc_output_i16", xq, torch.int16, target, rows, d, bias, torch.int64)
  tables = _qfc_output_tables("qfc_output_i16", multiplier, shift, rows, 16)
  m_dev, s_dev = tables.multiplier, tables.shift
  n = xq.shape[0]
  q = rt.empty((n, rows), torch.int16)
  L = _ffi.lib()
  nbytes = L.mi355q_qfc_output_workspace_bytes(rows, d)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_qfc_output_i16(rt.ptr(xq), n, d, rt.ptr(target.data), COMPARE_KINDS[target.kind], rows, rt.ptr(bias),
                                     rt.ptr(m_dev), rt.ptr(s_dev), m_dev.numel(), int(act_min), int(act_max), rt.ptr(q),
                                     rt.ptr(ws), nbytes, rt.stream_ptr()))
  return q


# (include/mi355q.h, "Patch gather for CONV_2D")
CONV_PADDING_NAMES = {0: "SAME", 1: "VALID"}
_CONV_DTYPES = {torch.int8: np.int8, torch.int16: np.int16, torch.float32: np.float32}


def _pair(value, what: str) -> tuple:
  """An int, or (h, w), as two Python integers."""
  if isinstance(value, (tuple, list)):
    if len(value) != 2:
      raise ValueError(f"{what} must be an integer or an (h, w) pair (got {value!r})")
    return int(value[0]), int(value[1])
  return int(value), int(value)


def _padding_name(padding) -> str:
  name = CONV_PADDING_NAMES.get(padding, padding) if not isinstance(padding, str) else padding.upper()
  if name not in ("SAME", "VALID"):
    raise ValueError(f"padding must be 'SAME' (0) or 'VALID' (1), got {padding!r}")
  return name


def conv_geometry(h: int, w: int, kh: int, kw: int, stride, dilation, padding) -> tuple:
  """(oh, ow, pad_top, pad_left) of a CONV_2D over an h x w image, host arithmetic on Python integers by TFLite's
  rule: eff = (k - 1) dil + 1; SAME: out = ceil(in / stride); VALID: out = (in + stride - eff) // stride;
  total = max(0, (out - 1) stride + eff - in) and pad_before = total // 2 (an odd total puts the extra row after).
  `stride` and `dilation` are integers or (h, w) pairs, `padding` "SAME" / "VALID" (or the schema's 0 / 1). Raises
  ValueError when an output dimension is not positive."""
  (sh, sw), (dh, dw) = _pair(stride, "stride"), _pair(dilation, "dilation")
  name = _padding_name(padding)
  h, w, kh, kw = int(h), int(w), int(kh), int(kw)
  if min(h, w, kh, kw, sh, sw, dh, dw) < 1:
    raise ValueError(f"image {h} x {w}, kernel {kh} x {kw}, strides {sh}, {sw} and dilations {dh}, {dw} must be positive")

  def axis(size: int, k: int, stride_: int, dil: int) -> tuple:
    eff = (k - 1) * dil + 1
    out = -(-size // stride_) if name == "SAME" else (size + stride_ - eff) // stride_
    if out < 1:
      raise ValueError(f"no positive output size: {size} inputs, kernel {k}, stride {stride_}, dilation {dil}, {name}")
    return out, max(0, (out - 1) * stride_ + eff - size) // 2
  (oh, top), (ow, left) = axis(h, kh, sh, dh), axis(w, kw, sw, dw)
  return oh, ow, top, left


def _pad_element(pad_value, np_dtype):
  """One pad element of `np_dtype` as the host bytes the patch gathers read."""
  pad = np.asarray(pad_value)
  if pad.size != 1:
    raise ValueError("pad_value must be one element")
  if pad.dtype != np_dtype:
    if np_dtype != np.float32:
      if pad.dtype.kind not in "iub" or not np.iinfo(np_dtype).min <= int(pad.reshape(())) <= np.iinfo(np_dtype).max:
        raise ValueError(f"pad_value {pad_value!r} is no {np.dtype(np_dtype).name}")
    pad = pad.astype(np_dtype)
  return ctypes.create_string_buffer(pad.tobytes(), pad.itemsize)


def conv_patches(x: torch.Tensor, kh: int, kw: int, stride, dilation, padding, pad_value=0, first: int = 0,
                 count: int | None = None) -> torch.Tensor:
  """The patch rows of an NHWC activation: x [N, H, W, C] (int8, int16 or float32, on the device) ->
  [count, kh kw C] of the same dtype, rows first .. first + count - 1 of the N OH OW patch rows (default: all from
  `first` on), row t = (n, oh, ow) in that order and column (i kw + j) C + c the tap (i, j), channel c; a tap outside
  the image holds `pad_value` (the activation's zero point for an integer tensor). The geometry is conv_geometry's.
  A byte copy: a NaN pad keeps its payload. The rows are what qfc_forward / qfc_forward_i16 / qfc_output read
  against a filter [O, kh, kw, C] viewed as [O, kh kw C]. Does not synchronize."""
  rt.require_gpu()
  if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in _CONV_DTYPES:
    raise TypeError(f"expected an int8, int16 or float32 device tensor, got {getattr(x, 'dtype', type(x))}"
                    f" on {getattr(x, 'device', 'the host')}")
  if x.dim() != 4:
    raise ValueError(f"expected an [N, H, W, C] tensor, got {tuple(x.shape)}")
  n_img, h, w, c = (int(v) for v in x.shape)
  kh, kw = int(kh), int(kw)
  (sh, sw), (dh, dw) = _pair(stride, "stride"), _pair(dilation, "dilation")
  if min(n_img, h, w, c) < 1:
    raise ValueError(f"every dimension of x must be positive, got {tuple(x.shape)}")
  oh, ow, top, left = conv_geometry(h, w, kh, kw, (sh, sw), (dh, dw), padding)
  k = kh * kw * c
  if k > QFC_MAX_D:
    raise ValueError(f"K = {kh} x {kw} x {c} = {k} exceeds {QFC_MAX_D}, the forward entries' limit")
  rows_all = n_img * oh * ow
  if rows_all > 0x7FFFFFFF:
    raise ValueError(f"{rows_all} patch rows exceed INT32_MAX")
  first = int(first)
  count = rows_all - first if count is None else int(count)
  if first < 0 or count < 0 or first + count > rows_all:
    raise ValueError(f"rows [{first}, {first} + {count}) are outside the {rows_all} patch rows")
  pad_bytes = _pad_element(pad_value, _CONV_DTYPES[x.dtype])
  if not x.is_contiguous():
    x = x.contiguous()
  out = rt.empty((count, k), x.dtype)
  _ffi.check(_ffi.lib().mi355q_conv_patches_nhwc(rt.ptr(x), x.element_size(), n_img, h, w, c, kh, kw, sh, sw, dh, dw, top,
                                                 left, oh, ow, first, count, ctypes.cast(pad_bytes, ctypes.c_void_p),
                                                 rt.ptr(out), rt.stream_ptr()))
  return out


# (include/mi355q.h, "Patch gather for TRANSPOSE_CONV")
def tconv_geometry(ih: int, iw: int, kh: int, kw: int, stride, padding, out_hw) -> tuple:
  """(pad_top, pad_left) of a TRANSPOSE_CONV from an ih x iw image to `out_hw` = (OH, OW): the padding of the FORWARD
  convolution from the OUTPUT image back to the input (TFLite's rule, no dilation), host arithmetic:
  conv_geometry(OH, OW, kh, kw, stride, 1, padding) must return exactly (ih, iw, pad_top, pad_left). Raises ValueError
  when it does not: `out_hw` is not reachable from ih x iw under this padding and these strides."""
  oh, ow = _pair(out_hw, "out_hw")
  back = conv_geometry(oh, ow, kh, kw, stride, 1, padding)
  if back[:2] != (int(ih), int(iw)):
    raise ValueError(f"a {_padding_name(padding)} convolution ({int(kh)} x {int(kw)}, strides {_pair(stride, 'stride')}) maps the output"
                     f" {oh} x {ow} to {back[0]} x {back[1]}, not to the input {int(ih)} x {int(iw)}")
  return back[2], back[3]


def tconv_phases(ih: int, iw: int, kh: int, kw: int, stride, padding, out_hw) -> list:
  """The sub-pixel phases of a TRANSPOSE_CONV as a host list of (py, px, QH, QW, kys, kxs), py-major, for every phase
  that has output pixels: the pixels oy = qy sh + py < OH (QH of them) and ox = qx sw + px < OW all use the taps
  kys = (ky : (py + pad_top - ky) % sh == 0) and kxs likewise, in ascending order; tap ti of kys reads the input row
  a = qy + (py + pad_top - kys[ti]) / sh. A stride above the kernel leaves phases with no tap (kys or kxs empty).
  The geometry is tconv_geometry's."""
  (sh, sw), (oh, ow) = _pair(stride, "stride"), _pair(out_hw, "out_hw")
  top, left = tconv_geometry(ih, iw, kh, kw, (sh, sw), padding, (oh, ow))
  out = []
  for py in range(min(sh, oh)):
    kys = tuple(range((py + top) % sh, int(kh), sh))
    for px in range(min(sw, ow)):
      kxs = tuple(range((px + left) % sw, int(kw), sw))
      out.append((py, px, -(-(oh - py) // sh), -(-(ow - px) // sw), kys, kxs))
  return out


def _tconv_phase(x, kh: int, kw: int, stride, padding, out_hw, phase):
  """(QH, QW, kys, kxs) of `phase` = (py, px) for x [N, IH, IW, C]; ValueError when the phase is none of the op's."""
  py, px = _pair(phase, "phase")
  for p in tconv_phases(int(x.shape[1]), int(x.shape[2]), kh, kw, stride, padding, out_hw):
    if p[:2] == (py, px):
      return p[2:]
  raise ValueError(f"phase ({py}, {px}) is outside the strides {_pair(stride, 'stride')}, or has no output pixel in"
                   f" {_pair(out_hw, 'out_hw')}")


def tconv_patches(x: torch.Tensor, kh: int, kw: int, stride, padding, out_hw, phase, pad_value=0, first: int = 0,
                  count: int | None = None) -> torch.Tensor:
  """The patch rows of one phase of a TRANSPOSE_CONV: x [N, IH, IW, C] (int8, int16 or float32, on the device) ->
  [count, |kys| |kxs| C] of the same dtype, rows first .. first + count - 1 of the N QH QW rows of `phase` = (py, px)
  (default: all from `first` on), row t = (n, qy, qx) in that order and column (ti |kxs| + tj) C + c the tap
  (kys[ti], kxs[tj]), channel c, read at a = qy + (py + pad_top - ky) / sh and b likewise; a tap outside the image
  holds `pad_value`. The phases are tconv_phases', the geometry tconv_geometry's. A byte copy: a NaN pad keeps its
  payload. The rows are what qfc_forward / qfc_forward_i16 / qfc_output read against the filter slice
  W[:, kys][:, :, kxs] viewed as [O, |kys| |kxs| C]; the result is the output pixels (qy sh + py, qx sw + px).
  A phase without a tap raises ValueError. Does not synchronize."""
  rt.require_gpu()
  if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in _CONV_DTYPES:
    raise TypeError(f"expected an int8, int16 or float32 device tensor, got {getattr(x, 'dtype', type(x))}"
                    f" on {getattr(x, 'device', 'the host')}")
  if x.dim() != 4:
    raise ValueError(f"expected an [N, IH, IW, C] tensor, got {tuple(x.shape)}")
  n_img, h, w, c = (int(v) for v in x.shape)
  if min(n_img, h, w, c) < 1:
    raise ValueError(f"every dimension of x must be positive, got {tuple(x.shape)}")
  kh, kw = int(kh), int(kw)
  (sh, sw), (oh, ow), (py, px) = _pair(stride, "stride"), _pair(out_hw, "out_hw"), _pair(phase, "phase")
  top, left = tconv_geometry(h, w, kh, kw, (sh, sw), padding, (oh, ow))
  qh, qw, kys, kxs = _tconv_phase(x, kh, kw, (sh, sw), padding, (oh, ow), (py, px))
  if not kys or not kxs:
    raise ValueError(f"phase ({py}, {px}) has no tap: a stride of {sh}, {sw} exceeds the {kh} x {kw} kernel")
  k = len(kys) * len(kxs) * c
  if k > QFC_MAX_D:
    raise ValueError(f"K = {len(kys)} x {len(kxs)} x {c} = {k} exceeds {QFC_MAX_D}, the forward entries' limit")
  rows_all = n_img * qh * qw
  if rows_all > 0x7FFFFFFF:
    raise ValueError(f"{rows_all} patch rows exceed INT32_MAX")
  first = int(first)
  count = rows_all - first if count is None else int(count)
  if first < 0 or count < 0 or first + count > rows_all:
    raise ValueError(f"rows [{first}, {first} + {count}) are outside the {rows_all} patch rows of the phase")
  pad_bytes = _pad_element(pad_value, _CONV_DTYPES[x.dtype])
  if not x.is_contiguous():
    x = x.contiguous()
  out = rt.empty((count, k), x.dtype)
  _ffi.check(_ffi.lib().mi355q_tconv_patches_nhwc(rt.ptr(x), x.element_size(), n_img, h, w, c, kh, kw, sh, sw, top, left,
                                                  oh, ow, py, px, first, count, ctypes.cast(pad_bytes, ctypes.c_void_p),
                                                  rt.ptr(out), rt.stream_ptr()))
  return out


def _tconv_filter_slices(who: str, w, o: int, kh: int, kw: int, c: int, phases: list) -> list:
  """The filter slice W[:, kys][:, :, kxs] viewed [O, |kys| |kxs| C] of every phase: float32 tensors of a float32
  filter, CompareTargets (per tensor, or per channel along dimension 0: slicing leaves the scales as they are) of an
  int8 CompareTarget. Torch indexing: plumbing."""
  n = o * kh * kw * c
  if isinstance(w, CompareTarget):
    if w.kind != "i8" or w.n != n or w.data.dtype != torch.int8 or not w.data.is_cuda:
      raise ValueError(f"{who} needs an i8 filter of {o} x {kh} x {kw} x {c} elements on the device, got {w.kind!r} with {w.n}")
    if w.zero_point is not None and bool(torch.any(w.zero_point != 0)):
      raise ValueError("the weight's zero point must be 0")
    if not (w.channels == 1 or (w.channels == o and w.inner == kh * kw * c)) or w.scale.numel() != w.channels:
      raise ValueError(f"{who}: scale view ({w.channels} channels, inner {w.inner}) is neither per tensor nor per channel"
                       f" along dimension 0 of a [{o}, {kh}, {kw}, {c}] filter")
    data = w.data.view(o, kh, kw, c)
  else:
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or w.numel() != n:
      raise TypeError(f"{who}: expected a float32 device filter of {o} x {kh} x {kw} x {c} elements, got"
                      f" {getattr(w, 'dtype', type(w))} {tuple(getattr(w, 'shape', ()))}")
    data = w.contiguous().view(o, kh, kw, c)
  out = []
  for _, _, _, _, kys, kxs in phases:
    if not kys or not kxs:
      raise ValueError(f"{who}: a phase has no tap (a stride exceeds the {kh} x {kw} kernel)")
    part = data[:, list(kys)][:, :, list(kxs)].reshape(o, -1).contiguous()
    if isinstance(w, CompareTarget):
      part = CompareTarget(part, part.numel(), "i8", w.scale, None, w.channels, part.shape[1] if w.channels == o else 1)
    out.append(part)
  return out


def _tconv_run(who: str, x, dtypes, w, kh: int, kw: int, stride, padding, out_hw, pad_value, phase_fn, results: int):
  """The whole op by phases: `phase_fn(rows, filter slice, image index of every row)` returns `results` tensors
  [N QH QW, O] per phase, which are interleaved into `results` NHWC tensors [N, OH, OW, O] (out[:, py::sh, px::sw])."""
  if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in dtypes:
    names = " or ".join(str(t).replace("torch.", "") for t in dtypes)
    raise TypeError(f"{who}: expected an {names} device tensor, got {getattr(x, 'dtype', type(x))}"
                    f" on {getattr(x, 'device', 'the host')}")
  if x.dim() != 4 or min(int(v) for v in x.shape) < 1:
    raise ValueError(f"{who}: expected an [N, IH, IW, C] tensor with positive dimensions, got {tuple(x.shape)}")
  n_img, h, wd, c = (int(v) for v in x.shape)
  kh, kw = int(kh), int(kw)
  (sh, sw), (oh, ow) = _pair(stride, "stride"), _pair(out_hw, "out_hw")
  phases = tconv_phases(h, wd, kh, kw, (sh, sw), padding, (oh, ow))
  n_w = w.n if isinstance(w, CompareTarget) else int(getattr(w, "numel", lambda: 0)())
  if n_w < 1 or n_w % (kh * kw * c):
    raise ValueError(f"{who}: the filter's {n_w} elements are no multiple of {kh} x {kw} x {c}")
  o = n_w // (kh * kw * c)
  slices = _tconv_filter_slices(who, w, o, kh, kw, c, phases)
  outs = None
  for (py, px, qh, qw, _, _), part in zip(phases, slices):
    rows = tconv_patches(x, kh, kw, (sh, sw), padding, (oh, ow), (py, px), pad_value)
    image = torch.arange(n_img * qh * qw, device=x.device) // (qh * qw)
    got = phase_fn(rows, part, image)
    if outs is None:
      outs = [rt.empty((n_img, oh, ow, o), g.dtype) for g in got]
    for full, g in zip(outs, got):
      full[:, py::sh, px::sw, :] = g.view(n_img, qh, qw, o)
  return outs[0] if results == 1 else tuple(outs)


def tconv_forward(x: torch.Tensor, w, kh: int, kw: int, stride, padding, out_hw, x_scale: torch.Tensor | None = None,
                  x_zero_point: int = 0, want_acc: bool = False):
  """The TRANSPOSE_CONV product of an NHWC activation x [N, IH, IW, C] on the device and a filter [O, KH, KW, C], as
  float32 NHWC [N, OH, OW, O] with `out_hw` = (OH, OW):
    out[n, oy, ox, o] = Sum_{ky, kx, c} x[n, a, b, c] W[o, ky, kx, c]
  over the taps with (oy + pad_top - ky) % sh == 0 and a = (oy + pad_top - ky) / sh in [0, IH), likewise b; the
  geometry is tconv_geometry's (the forward convolution from OH x OW back to IH x IW; no dilation). Executed by
  sub-pixel phases (tconv_phases): the rows of tconv_patches against the filter slice W[:, kys][:, :, kxs], so that
  every multiply is a real one. By the dtype of x:
    float32  `w` a float32 device tensor of O KH KW C elements: every phase is gemm(rows, slice^T);
    int8     `w` a CompareTarget of kind i8 (per tensor, or per channel along dimension 0), `x_scale` float32 with 1
             or N entries (one per IMAGE), `x_zero_point` in int8, which is also the pad element: every phase is
             qfc_forward, y = float(Sum (x - zp_x) q_w) * (x_scale * w_scale), the accumulator exact in int32;
    int16    as int8 without a zero point: qfc_forward_i16, the accumulator exact in int64.
  Returns y, or (y, acc int32 / int64 [N, OH, OW, O]) with `want_acc` (integer activations only). The pre-bias
  product. A stride above the kernel (a phase without a tap) raises ValueError. This is the library's own definition,
  modelled on LiteRT's TRANSPOSE_CONV and unchecked against it. include/mi355q.h, "Patch gather for TRANSPOSE_CONV".
  Does not synchronize."""
  rt.require_gpu()
  who = "tconv_forward"
  is_float = isinstance(x, torch.Tensor) and x.dtype == torch.float32
  if is_float:
    if want_acc or x_scale is not None or int(x_zero_point) != 0:
      raise ValueError(f"{who}: a float32 activation takes no x_scale, x_zero_point or want_acc")
    return _tconv_run(who, x, (torch.float32,), w, kh, kw, stride, padding, out_hw, 0.0,
                      lambda rows, part, image: (gemm(rows, part, trans_b=True),), 1)
  if not isinstance(w, CompareTarget):
    raise ValueError(f"{who} needs an i8 filter (a CompareTarget) for an integer activation, got {type(w)}")
  if x_scale is None:
    raise ValueError(f"{who}: an integer activation needs x_scale")
  x_scale = _f32(x_scale).view(-1)
  if isinstance(x, torch.Tensor) and x.dim() == 4 and x_scale.numel() not in (1, int(x.shape[0])):
    raise ValueError(f"{who}: x_scale needs 1 or N = {int(x.shape[0])} entries (got {x_scale.numel()})")
  int16 = isinstance(x, torch.Tensor) and x.dtype == torch.int16
  zp = int(x_zero_point)
  if (int16 and zp != 0) or not -128 <= zp <= 127:
    raise ValueError(f"{who}: x_zero_point {x_zero_point} is outside int8, or given for an int16 activation")

  def phase(rows, part, image):
    scale = x_scale if x_scale.numel() == 1 else x_scale[image]
    o, k = part.data.shape
    if int16:
      got = qfc_forward_i16(rows, scale, part, o, k, want_acc=want_acc)
    else:
      got = qfc_forward(rows, scale, zp, part, o, k, want_acc=want_acc)
    return got if want_acc else (got,)
  return _tconv_run(who, x, (torch.int8, torch.int16), w, kh, kw, stride, padding, out_hw, zp, phase, 2 if want_acc else 1)


def tconv_output(x: torch.Tensor, x_zero_point: int, target: CompareTarget, kh: int, kw: int, stride, padding, out_hw,
                 bias, multiplier, shift, out_zero_point: int, act_min: int, act_max: int) -> torch.Tensor:
  """What a static int8 TRANSPOSE_CONV op stores: int8 NHWC [N, OH, OW, O] =
  clamp(mbqm32(sat32(acc + bias), M, s) + out_zero_point, act_min, act_max) of tconv_forward's int32 accumulator,
  out[n, oy, ox, o] = Sum_{ky, kx, c} (x[n, a, b, c] - x_zero_point) q_w[o, ky, kx, c] over the taps with
  (oy + pad_top - ky) % sh == 0 and a = (oy + pad_top - ky) / sh in [0, IH), likewise b; with the arithmetic and the
  argument forms of qfc_output (`bias` None or int32 [O]; `multiplier` / `shift` host tables of 1 or O entries, or
  qfc_multipliers' result with `shift` None), which runs unchanged on every phase's rows. This is the library's own
  definition, modelled on LiteRT's TRANSPOSE_CONV and unchecked against it. Does not synchronize."""
  rt.require_gpu()
  who = "tconv_output"
  if not isinstance(target, CompareTarget):
    raise ValueError(f"{who} needs an i8 filter (a CompareTarget), got {type(target)}")
  zp = int(x_zero_point)
  if not -128 <= zp <= 127:
    raise ValueError(f"{who}: x_zero_point {x_zero_point} is outside int8")
  tables = [None]

  def phase(rows, part, image):
    o, k = part.data.shape
    if tables[0] is None:      # (checked and uploaded once for all phases)
      tables[0] = (_qfc_output_tables(who, multiplier, shift, o, 8), _dwconv_bias(who, bias, o, torch.int32))
    return (qfc_output(rows, zp, part, o, k, tables[0][1], tables[0][0], None, out_zero_point, act_min, act_max),)
  return _tconv_run(who, x, (torch.int8,), target, kh, kw, stride, padding, out_hw, zp, phase, 1)


def tconv_output_i16(x: torch.Tensor, target: CompareTarget, kh: int, kw: int, stride, padding, out_hw, bias, multiplier,
                     shift, act_min: int, act_max: int) -> torch.Tensor:
  """What a static int16-activation TRANSPOSE_CONV op stores: int16 NHWC [N, OH, OW, O], qfc_output_i16's arithmetic
  on tconv_forward's int64 accumulator, out[n, oy, ox, o] = Sum_{ky, kx, c} x[n, a, b, c] q_w[o, ky, kx, c] over the
  taps with (oy + pad_top - ky) % sh == 0 and a = (oy + pad_top - ky) / sh in [0, IH), likewise b (`bias` None or int64
  [O]; shifts in [-31, 14]; no zero points). The library's own definition, modelled on LiteRT's TRANSPOSE_CONV and
  unchecked against it. Does not synchronize."""
  rt.require_gpu()
  who = "tconv_output_i16"
  if not isinstance(target, CompareTarget):
    raise ValueError(f"{who} needs an i8 filter (a CompareTarget), got {type(target)}")
  tables = [None]

  def phase(rows, part, image):
    o, k = part.data.shape
    if tables[0] is None:
      tables[0] = (_qfc_output_tables(who, multiplier, shift, o, 16), _dwconv_bias(who, bias, o, torch.int64))
    return (qfc_output_i16(rows, part, o, k, tables[0][1], tables[0][0], None, act_min, act_max),)
  return _tconv_run(who, x, (torch.int16,), target, kh, kw, stride, padding, out_hw, 0, phase, 1)


# (include/mi355q.h, "Direct depthwise convolution")
DWCONV_MAX_TAPS = 65536


def _dwconv_geometry(who: str, x, dtypes, kh: int, kw: int, depth_multiplier: int, stride, dilation, padding, first: int,
                     count):
  """The argument checks the depthwise entries share; returns the integers of the C call's geometry, in its order
  after (N, H, W, C): (n, h, w, c), (kh, kw, m), (sh, sw, dh, dw, top, left, oh, ow, first, count), and O = C M."""
  if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in dtypes:
    names = " or ".join(str(t).replace("torch.", "") for t in dtypes)
    raise TypeError(f"{who}: expected an {names} device tensor, got {getattr(x, 'dtype', type(x))}"
                    f" on {getattr(x, 'device', 'the host')}")
  if x.dim() != 4:
    raise ValueError(f"{who}: expected an [N, H, W, C] tensor, got {tuple(x.shape)}")
  n_img, h, w, c = (int(v) for v in x.shape)
  kh, kw, m = int(kh), int(kw), int(depth_multiplier)
  (sh, sw), (dh, dw) = _pair(stride, "stride"), _pair(dilation, "dilation")
  if min(n_img, h, w, c) < 1:
    raise ValueError(f"{who}: every dimension of x must be positive, got {tuple(x.shape)}")
  if m < 1:
    raise ValueError(f"{who}: the depth multiplier must be positive (got {m})")
  oh, ow, top, left = conv_geometry(h, w, kh, kw, (sh, sw), (dh, dw), padding)
  if kh * kw > DWCONV_MAX_TAPS:
    raise ValueError(f"{who}: {kh} x {kw} taps exceed {DWCONV_MAX_TAPS}")
  rows_all = n_img * oh * ow
  if rows_all > 0x7FFFFFFF or c * m > 0x7FFFFFFF:
    raise ValueError(f"{who}: {rows_all} output rows of {c * m} channels exceed INT32_MAX")
  first = int(first)
  count = rows_all - first if count is None else int(count)
  if first < 0 or count < 0 or first + count > rows_all:
    raise ValueError(f"{who}: rows [{first}, {first} + {count}) are outside the {rows_all} output rows")
  return (n_img, h, w, c), (kh, kw, m), (sh, sw, dh, dw, top, left, oh, ow, first, count), c * m


def _dwconv_filter(who: str, target: CompareTarget, taps: int, o: int) -> None:
  """An int8 filter [KH, KW, O] with per-tensor scales, or per-channel scales along its last dimension."""
  if not isinstance(target, CompareTarget) or target.kind != "i8":
    raise ValueError(f"{who} needs an i8 filter (a CompareTarget), got {getattr(target, 'kind', type(target))!r}")
  if target.n != taps * o or target.data.dtype != torch.int8 or not target.data.is_cuda:
    raise ValueError(f"{who}: the filter has {target.n} elements, expected {taps} x {o} int8 on the device")
  if target.zero_point is not None and bool(torch.any(target.zero_point != 0)):
    raise ValueError("the weight's zero point must be 0")
  if not (target.channels == 1 or (target.channels == o and target.inner == 1)):
    raise ValueError(f"{who}: scale view ({target.channels} channels, inner {target.inner}) is neither per tensor nor per"
                     f" channel along the last dimension of a [{taps}, {o}] filter")
  if target.scale.numel() != target.channels:
    raise ValueError("scale must have one entry per channel")


def dwconv_forward(x: torch.Tensor, w, kh: int, kw: int, stride, dilation, padding, depth_multiplier: int = 1,
                   x_scale: torch.Tensor | None = None, x_zero_point: int = 0, first: int = 0, count: int | None = None,
                   want_acc: bool = False):
  """The DEPTHWISE_CONV_2D product of an NHWC activation x [N, H, W, C] on the device and a filter [KH, KW, O]
  (O = C depth_multiplier, the stored bytes of TFLite's [1, KH, KW, O]; output channel oc reads input channel
  oc // depth_multiplier), as float32 [count, O]: rows first .. first + count - 1 of the N OH OW output rows (default:
  all from `first` on), the geometry conv_geometry's; a tap outside the image adds nothing. By the dtype of x:
    float32  `w` a float32 device tensor of KH KW O elements: y = (((0 + p_0) + p_1) ...), p = fl32(x w), taps in
             ascending (kh, kw) order, no FMA: the bits of a NumPy float32 loop in that order;
    int8     `w` a CompareTarget of kind i8 (per tensor, or per channel along the last dimension), `x_scale` float32
             with 1 or N entries (one per IMAGE), `x_zero_point` in int8:
             y = float(Sum (x - zp_x) q_w) * (x_scale * w_scale), the accumulator exact in int32;
    int16    as int8 without a zero point: the accumulator exact in int64 and
             y = float32(float64(acc) * float64(x_scale * w_scale)).
  Returns y, or (y, acc int32 / int64 [count, O]) with `want_acc` (integer activations only). The pre-bias product.
  include/mi355q.h, "Direct depthwise convolution". Does not synchronize."""
  rt.require_gpu()
  who = "dwconv_forward"
  (n_img, h, wd, c), (kh, kw, m), geo, o = _dwconv_geometry(who, x, (torch.float32, torch.int8, torch.int16), kh, kw,
                                                            depth_multiplier, stride, dilation, padding, first, count)
  count = geo[-1]
  if not x.is_contiguous():
    x = x.contiguous()
  L = _ffi.lib()
  y = rt.empty((count, o), torch.float32)
  if x.dtype == torch.float32:
    if want_acc or x_scale is not None or int(x_zero_point) != 0:
      raise ValueError(f"{who}: a float32 activation takes no x_scale, x_zero_point or want_acc")
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or w.numel() != kh * kw * o:
      raise TypeError(f"{who}: expected a float32 device filter of {kh} x {kw} x {o} elements, got"
                      f" {getattr(w, 'dtype', type(w))} {tuple(getattr(w, 'shape', ()))}")
    w = w if w.is_contiguous() else w.contiguous()
    _ffi.check(L.mi355q_dwconv_forward_f32(rt.ptr(x), n_img, h, wd, c, rt.ptr(w), kh, kw, m, *geo, rt.ptr(y),
                                           rt.stream_ptr()))
    return y
  _dwconv_filter(who, w, kh * kw, o)
  if x_scale is None:
    raise ValueError(f"{who}: an integer activation needs x_scale")
  x_scale = _f32(x_scale).view(-1)
  if x_scale.numel() not in (1, n_img):
    raise ValueError(f"{who}: x_scale needs 1 or N = {n_img} entries (got {x_scale.numel()})")
  if x.dtype == torch.int8:
    if not -128 <= int(x_zero_point) <= 127:
      raise ValueError(f"{who}: x_zero_point {x_zero_point} is outside int8")
    acc = rt.empty((count, o), torch.int32) if want_acc else None
    _ffi.check(L.mi355q_dwconv_forward_i8(rt.ptr(x), n_img, h, wd, c, rt.ptr(x_scale), x_scale.numel(), int(x_zero_point),
                                          rt.ptr(w.data), COMPARE_KINDS[w.kind], kh, kw, m, rt.ptr(w.scale),
                                          w.scale.numel(), *geo, rt.ptr(y), rt.ptr(acc), rt.stream_ptr()))
  else:
    if int(x_zero_point) != 0:
      raise ValueError(f"{who}: an int16 activation has no zero point")
    acc = rt.empty((count, o), torch.int64) if want_acc else None
    _ffi.check(L.mi355q_dwconv_forward_i16(rt.ptr(x), n_img, h, wd, c, rt.ptr(x_scale), x_scale.numel(), rt.ptr(w.data),
                                           COMPARE_KINDS[w.kind], kh, kw, m, rt.ptr(w.scale), w.scale.numel(), *geo,
                                           rt.ptr(y), rt.ptr(acc), rt.stream_ptr()))
  return (y, acc) if want_acc else y


def _dwconv_bias(who: str, bias, o: int, bias_dtype):
  if bias is None:
    return None
  if not isinstance(bias, torch.Tensor):
    bias = rt.to_device(np.ascontiguousarray(np.asarray(bias).reshape(-1)))
  if bias.dtype != bias_dtype or not bias.is_cuda or bias.numel() != o:
    name = str(bias_dtype).replace("torch.", "")
    raise TypeError(f"{who}: the bias must be {name} with {o} entries, got {bias.dtype} with {bias.numel()}")
  return bias.contiguous().view(-1)


def dwconv_output(x: torch.Tensor, x_zero_point: int, target: CompareTarget, kh: int, kw: int, stride, dilation, padding,
                  bias, multiplier, shift, out_zero_point: int, act_min: int, act_max: int, depth_multiplier: int = 1,
                  first: int = 0, count: int | None = None) -> torch.Tensor:
  """What a static int8 DEPTHWISE_CONV_2D op stores: int8 [count, O] =
  clamp(mbqm32(sat32(acc + bias), M, s) + out_zero_point, act_min, act_max) of dwconv_forward's int32 accumulator,
  with the arithmetic and the argument forms of qfc_output (`bias` None or int32 [O]; `multiplier` / `shift` host tables
  of 1 or O entries, or qfc_multipliers' result with `shift` None). Only the stored tensor is written. Does not
  synchronize."""
  rt.require_gpu()
  who = "dwconv_output"
  (n_img, h, wd, c), (kh, kw, m), geo, o = _dwconv_geometry(who, x, (torch.int8,), kh, kw, depth_multiplier, stride,
                                                            dilation, padding, first, count)
  _dwconv_filter(who, target, kh * kw, o)
  bias = _dwconv_bias(who, bias, o, torch.int32)
  tables = _qfc_output_tables(who, multiplier, shift, o, 8)
  for what, v in (("x_zero_point", x_zero_point), ("out_zero_point", out_zero_point)):
    if not -128 <= int(v) <= 127:
      raise ValueError(f"{who}: {what} {v} is outside int8")
  if not -128 <= int(act_min) <= int(act_max) <= 127:
    raise ValueError(f"{who}: [{act_min}, {act_max}] is no range within int8")
  if not x.is_contiguous():
    x = x.contiguous()
  q = rt.empty((geo[-1], o), torch.int8)
  _ffi.check(_ffi.lib().mi355q_dwconv_output_i8(rt.ptr(x), n_img, h, wd, c, int(x_zero_point), rt.ptr(target.data),
                                                COMPARE_KINDS[target.kind], kh, kw, m, rt.ptr(bias),
                                                rt.ptr(tables.multiplier), rt.ptr(tables.shift), tables.multiplier.numel(),
                                                int(out_zero_point), int(act_min), int(act_max), *geo, rt.ptr(q),
                                                rt.stream_ptr()))
  return q


def dwconv_output_i16(x: torch.Tensor, target: CompareTarget, kh: int, kw: int, stride, dilation, padding, bias,
                      multiplier, shift, act_min: int, act_max: int, depth_multiplier: int = 1, first: int = 0,
                      count: int | None = None) -> torch.Tensor:
  """What a static int16-activation DEPTHWISE_CONV_2D op stores: int16 [count, O], qfc_output_i16's arithmetic on
  dwconv_forward's int64 accumulator (`bias` None or int64 [O]; shifts in [-31, 14]; no zero points). Does not
  synchronize."""
  rt.require_gpu()
  who = "dwconv_output_i16"
  (n_img, h, wd, c), (kh, kw, m), geo, o = _dwconv_geometry(who, x, (torch.int16,), kh, kw, depth_multiplier, stride,
                                                            dilation, padding, first, count)
  _dwconv_filter(who, target, kh * kw, o)
  bias = _dwconv_bias(who, bias, o, torch.int64)
  tables = _qfc_output_tables(who, multiplier, shift, o, 16)
  if not -32768 <= int(act_min) <= int(act_max) <= 32767:
    raise ValueError(f"{who}: [{act_min}, {act_max}] is no range within int16")
  if not x.is_contiguous():
    x = x.contiguous()
  q = rt.empty((geo[-1], o), torch.int16)
  _ffi.check(_ffi.lib().mi355q_dwconv_output_i16(rt.ptr(x), n_img, h, wd, c, rt.ptr(target.data), COMPARE_KINDS[target.kind],
                                                 kh, kw, m, rt.ptr(bias), rt.ptr(tables.multiplier), rt.ptr(tables.shift),
                                                 tables.multiplier.numel(), int(act_min), int(act_max), *geo, rt.ptr(q),
                                                 rt.stream_ptr()))
  return q


QBMM_MAX_K = 32768      # K * 255 * 255 < 2^31 (include/mi355q.h, "Integer batched matrix product")


def _qbmm_shapes(who: str, a: torch.Tensor, b: torch.Tensor, adj_x: bool, adj_y: bool, a_zero_point: int,
                 b_zero_point: int) -> tuple:
  """The checks qbmm_forward and qbmm_output share: (a, b, lead, batch, b_batch, M, K, N), the operands dense."""
  for name, t in (("a", a), ("b", b)):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int8 or not t.is_cuda or t.dim() < 2:
      got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
      raise TypeError(f"{who}: `{name}` must be an int8 device tensor of rank >= 2, got {got}")
  lead = tuple(a.shape[:-2])
  batch, b_batch = int(np.prod(lead, dtype=np.int64)), int(np.prod(tuple(b.shape[:-2]), dtype=np.int64))
  k, m = (a.shape[-2], a.shape[-1]) if adj_x else (a.shape[-1], a.shape[-2])
  n, kb = (b.shape[-2], b.shape[-1]) if adj_y else (b.shape[-1], b.shape[-2])
  if k != kb:
    raise ValueError(f"{who}: the operands disagree on K ({k} of {tuple(a.shape)}, {kb} of {tuple(b.shape)};"
                     f" adj_x = {bool(adj_x)}, adj_y = {bool(adj_y)})")
  if tuple(b.shape[:-2]) != lead and b_batch != 1:
    raise ValueError(f"{who}: the batch dimensions of b {tuple(b.shape[:-2])} are neither those of a {lead} nor of"
                     " product 1 (general broadcasting is not built)")
  if k > QBMM_MAX_K:
    raise ValueError(f"{who}: K = {k} exceeds {QBMM_MAX_K} (the int32 accumulator)")
  for name, zp in (("a_zero_point", a_zero_point), ("b_zero_point", b_zero_point)):
    if not -128 <= int(zp) <= 127:
      raise ValueError(f"{who}: {name} = {zp} is outside int8")
  # (no copy of a dense operand: a misaligned view is still dense, and the library routes on the address)
  a = a if a.is_contiguous() else a.contiguous()
  b = b if b.is_contiguous() else b.contiguous()
  return a, b, lead, batch, (batch if tuple(b.shape[:-2]) == lead else 1), int(m), int(k), int(n)


def _qbmm_workspace(batch: int, m: int, k: int, adj_x: bool, b_batch: int, n: int, adj_y: bool, za: int, zb: int):
  """The operand sums and the transposed copy of every operand that is strided along K; nothing (a NULL workspace)
  when there is neither a zero point nor such an operand."""
  if za == 0 and zb == 0 and not adj_x and adj_y:
    return None, 0
  nbytes = _ffi.lib().mi355q_qbmm_workspace_bytes(batch, m, k, 1 if adj_x else 0, b_batch, n, 1 if adj_y else 0)
  return rt.empty((max(nbytes, 1),), torch.uint8), nbytes


def qbmm_forward(a: torch.Tensor, b: torch.Tensor, *, adj_x: bool, adj_y: bool, a_scale: torch.Tensor, a_zero_point: int,
                 b_scale: torch.Tensor, b_zero_point: int, want_acc: bool = False):
  """The integer BATCH_MATMUL product of two int8 device tensors of rank >= 2 that both carry a zero point:
  acc[.., m, n] = Sum_k (a - a_zero_point) (b - b_zero_point) exact in int32 and y = float(acc) * (a_scale * b_scale),
  float32 [.., M, N]. `a` is [.., M, K] ([.., K, M] with `adj_x`), `b` [.., K, N] ([.., N, K] with `adj_y`); the leading
  dimensions of `a` are the batch, and `b` has the same ones or a batch product of 1 (one matrix for every batch).
  `a_scale` holds 1 or batch * M float32 entries (per row: the dynamic mode), `b_scale` 1 or N. K <= 32768. Returns y,
  or (y, acc int32) with `want_acc` (include/mi355q.h, "Integer batched matrix product"). Does not synchronize."""
  rt.require_gpu()
  who = "qbmm_forward"
  za, zb = int(a_zero_point), int(b_zero_point)
  a, b, lead, batch, b_batch, m, k, n = _qbmm_shapes(who, a, b, adj_x, adj_y, za, zb)
  a_scale, b_scale = _f32(a_scale).view(-1), _f32(b_scale).view(-1)
  if a_scale.numel() not in (1, batch * m):
    raise ValueError(f"{who}: a_scale needs 1 or batch * M = {batch * m} entries (got {a_scale.numel()})")
  if b_scale.numel() not in (1, n):
    raise ValueError(f"{who}: b_scale needs 1 or N = {n} entries (got {b_scale.numel()})")
  y = rt.empty(lead + (m, n), torch.float32)
  acc = rt.empty(lead + (m, n), torch.int32) if want_acc else None
  ws, nbytes = _qbmm_workspace(batch, m, k, adj_x, b_batch, n, adj_y, za, zb)
  _ffi.check(_ffi.lib().mi355q_qbmm_forward_i8(rt.ptr(a), batch, m, k, 1 if adj_x else 0, rt.ptr(a_scale), a_scale.numel(),
                                               za, rt.ptr(b), b_batch, n, 1 if adj_y else 0, rt.ptr(b_scale),
                                               b_scale.numel(), zb, rt.ptr(y), rt.ptr(acc), rt.ptr(ws), nbytes,
                                               rt.stream_ptr()))
  return (y, acc) if want_acc else y


def qbmm_output(a: torch.Tensor, b: torch.Tensor, *, adj_x: bool, adj_y: bool, a_zero_point: int, b_zero_point: int,
                multiplier, shift, out_zero_point: int) -> torch.Tensor:
  """What a static int8 BATCH_MATMUL op stores: int8 [.., M, N] = clamp(mbqm32(acc, M, s) + out_zero_point, -128, 127)
  of qbmm_forward's accumulator, with qfc_output's fixed-point requantization; the op has neither a bias nor a fused
  activation. `multiplier` / `shift` are host tables of 1 or N entries (quantize_multiplier), or qfc_multipliers'
  result with `shift` None. Does not synchronize."""
  rt.require_gpu()
  who = "qbmm_output"
  za, zb = int(a_zero_point), int(b_zero_point)
  a, b, lead, batch, b_batch, m, k, n = _qbmm_shapes(who, a, b, adj_x, adj_y, za, zb)
  tables = _qfc_output_tables(who, multiplier, shift, n, 8)
  if not -128 <= int(out_zero_point) <= 127:
    raise ValueError(f"{who}: out_zero_point = {out_zero_point} is outside int8")
  q = rt.empty(lead + (m, n), torch.int8)
  ws, nbytes = _qbmm_workspace(batch, m, k, adj_x, b_batch, n, adj_y, za, zb)
  _ffi.check(_ffi.lib().mi355q_qbmm_output_i8(rt.ptr(a), batch, m, k, 1 if adj_x else 0, za, rt.ptr(b), b_batch, n,
                                              1 if adj_y else 0, zb, rt.ptr(tables.multiplier), rt.ptr(tables.shift),
                                              tables.multiplier.numel(), int(out_zero_point), rt.ptr(q), rt.ptr(ws), nbytes,
                                              rt.stream_ptr()))
  return q


def sqdiff_cols(a: torch.Tensor, b: torch.Tensor, out: tuple | None = None):
  """(Sum_t (a - b)^2, Sum_t b^2) per column of float32 [n, cols] device tensors, float64 [cols] each, added in a
  fixed order (the same bits in every run). With `out` = an earlier result the sums are added onto it in place and
  it is returned: the samples of a calibration set, in order. Does not synchronize."""
  rt.require_gpu()
  a, b = _f32(a), _f32(b)
  if a.dim() != 2 or a.shape != b.shape:
    raise ValueError(f"expected two [n, cols] tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
  n, cols = a.shape
  if out is None:
    sq_d, sq_b = rt.empty((cols,), torch.float64), rt.empty((cols,), torch.float64)
  else:
    sq_d, sq_b = out
    for v in (sq_d, sq_b):
      if v.dtype != torch.float64 or not v.is_cuda or v.numel() != cols or not v.is_contiguous():
        raise TypeError(f"`out` must hold two contiguous float64 device tensors of {cols} elements")
  L = _ffi.lib()
  nbytes = L.mi355q_sqdiff_cols_workspace_bytes(n, cols)
  ws = rt.empty((max(nbytes, 1),), torch.uint8)
  _ffi.check(L.mi355q_sqdiff_cols_f64(rt.ptr(a), rt.ptr(b), n, cols, rt.ptr(sq_d), rt.ptr(sq_b), 0 if out is None else 1,
                                      rt.ptr(ws), nbytes, rt.stream_ptr()))
  return sq_d, sq_b


SWEEP_BITS = (2, 4, 8)
SWEEP_BLOCKS = (0, 32, 64, 128, 256)
SWEEP_MAX_CANDIDATES = 8      # per launch (the candidate tables travel in the kernel arguments)


def check_sweep_candidates(candidates, shape) -> list:
  """[(bits, block)] as ints, or the ValueError `requant_sym` raises for them (no device is touched)."""
  out = []
  for bits, block in candidates:
    bits, block = int(bits), int(block)
    if bits not in SWEEP_BITS:
      raise ValueError(f"bits must be 8, 4 or 2 (got {bits})")
    if block not in SWEEP_BLOCKS:
      raise ValueError(f"block must be 0, 32, 64, 128 or 256 (got {block})")
    if block and shape[1] % block != 0:
      raise ValueError(f"Quantized dimension {shape[1]} in tensor shape {tuple(shape)} is not"
                       f" divisible by block size {block}.")
    out.append((bits, block))
  if not out:
    raise ValueError("requant_delta_sweep needs at least one candidate")
  return out


def requant_delta_sweep(x: torch.Tensor, candidates, want_sq: bool = True, out: torch.Tensor | None = None):
  """(delta float32 [count, rows, cols], sq float64 [count, rows] or None) for `candidates`, a sequence of
  (bits, block): delta[k] = x - dequant(requant_sym(x, block_k, bits_k)) bit for bit (the int8 / diff_bits 8 rule of
  `weight_delta`), from one read of x per launch of up to 8 candidates (mi355q_requant_delta_sweep_f32); sq[k][r] is
  the float64 sum of delta[k][r]^2 in a fixed order. More than 8 candidates are split into several launches that
  write into the one stacked output (`out`: a contiguous float32 [count, rows, cols] device tensor to write into
  instead of a fresh one). Does not synchronize."""
  import ctypes
  if x.dim() != 2:
    raise ValueError("requant_delta_sweep expects a 2-D [rows, cols] tensor")
  cands = check_sweep_candidates(candidates, x.shape)
  rt.require_gpu()
  x = _f32(x)
  rows, cols = x.shape
  count = len(cands)
  if out is None:
    delta = rt.empty((count, rows, cols), torch.float32)
  else:
    if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (count, rows, cols):
      raise ValueError(f"out must be a contiguous float32 device tensor of shape {(count, rows, cols)}")
    delta = out
  sq = rt.empty((count, rows), torch.float64) if want_sq else None
  L = _ffi.lib()
  for first in range(0, count, SWEEP_MAX_CANDIDATES):
    part = cands[first:first + SWEEP_MAX_CANDIDATES]
    bits = (ctypes.c_int32 * len(part))(*(b for b, _ in part))
    block = (ctypes.c_int32 * len(part))(*(b for _, b in part))
    _ffi.check(L.mi355q_requant_delta_sweep_f32(
        rt.ptr(x), rows, cols, len(part), bits, block, delta.data_ptr() + first * rows * cols * 4, rows * cols,
        (sq.data_ptr() + first * rows * 8) if want_sq else None, rt.stream_ptr()))
  return delta, sq
