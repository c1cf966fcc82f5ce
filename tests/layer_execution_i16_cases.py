"""Shared by test_gpu_layer_execution_i16.py and test_layer_execution_i16_host.py: the NumPy statement of the integer
FULLY_CONNECTED arithmetic with INT16 activations (include/mi355q.h, "Integer execution, int16 activations") and a
NumPy stand-in for model_validator.LayerExecutionKernels that has it."""
import numpy as np

import layer_execution_cases as EC

# the int16 values where a split into a high and a low byte goes wrong
PLANTED = (-32768, -32767, -257, -256, -255, -129, -128, -1, 0, 1, 127, 128, 255, 256, 32767)


# ---------------------------------------------------------------- the arithmetic
def quantize_static16(x: np.ndarray, scale) -> np.ndarray:
  """The static int16 activation quantizer as ops.quantize stands (16 bits, not narrow, zero point 0):
  q = clip(rint(fl(fl(x / s_x) + 0)), -32768, 32767), the quotient and the sum in float32."""
  v = (np.asarray(x, np.float32) / np.float32(scale)).astype(np.float32) + np.float32(0)
  return np.clip(np.rint(v.astype(np.float32)), -32768, 32767).astype(np.int16)


def rescale(acc: np.ndarray, sc: np.ndarray) -> np.ndarray:
  """fl32(double(acc) * double(sc)) of exact int64 accumulators and float32 scale products."""
  assert acc.dtype == np.int64 and sc.dtype == np.float32
  return (acc.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)


def forward16(xq: np.ndarray, x_scale, qw: np.ndarray, w_scale, block: int = 0):
  """(acc int64 [n, rows] or None when blockwise, y float32 [n, rows]) of int16 xq [n, d] and integers qw [rows, d].
  x_scale: 1 or n float32; w_scale: 1 or rows float32 (block = 0), or rows * d / block float32 (blockwise). There is
  no zero point. The integers go through int64, where every sum is exact (|acc| <= 65536 * 32768 * 128 = 2^38)."""
  xq, qw = np.asarray(xq), np.asarray(qw)
  assert xq.dtype == np.int16
  n, d = xq.shape
  rows = qw.shape[0]
  xi, wi = xq.astype(np.int64), qw.astype(np.int64)
  xs = np.broadcast_to(np.asarray(x_scale, np.float32).reshape(-1), (n,)).astype(np.float32)
  ws = np.asarray(w_scale, np.float32).reshape(-1)
  with np.errstate(invalid="ignore", over="ignore"):
    if block == 0:
      acc = xi @ wi.T
      sw = np.broadcast_to(ws, (rows,)).astype(np.float32)
      sc = xs[:, None] * sw[None, :]
      return acc, rescale(acc, sc)
    sw = ws.reshape(rows, d // block)
    y = np.zeros((n, rows), np.float32)
    for b in range(d // block):
      acc = xi[:, b * block:(b + 1) * block] @ wi[:, b * block:(b + 1) * block].T
      p = rescale(acc, xs[:, None] * sw[None, :, b])
      y = y + p
    return None, y


def split(x: np.ndarray):
  """(h, l_s) of int16 values as the MFMA route splits them: x = 256 h + l_s + 128, both int8."""
  x = np.asarray(x, np.int16)
  h = (x >> 8).astype(np.int8)
  l_s = ((x & 255) ^ 0x80).astype(np.uint8).view(np.int8)
  return h, l_s


def plan_forward16(xq, x_scale, plan, rows: int, d: int) -> np.ndarray:
  """forward16() with the granularity read from a ConstantPlan's scale view, as ops.qfc_forward_i16 reads it."""
  qw = EC.plan_integers(plan, rows, d)
  if plan.channels == 1 or (plan.channels == rows and plan.inner == d):
    return forward16(xq, x_scale, qw, plan.scale, 0)[1]
  assert plan.inner in (32, 64, 128, 256) and plan.channels * plan.inner == rows * d
  return forward16(xq, x_scale, qw, plan.scale, plan.inner)[1]


def numpy_kernels(**kwargs):
  """layer_execution_cases.numpy_kernels() with the two int16 methods."""
  class NumpyKernels16(EC.numpy_kernels(**kwargs)):
    def quantize_static16(self, x, scale):
      return quantize_static16(x, scale), np.array([scale], np.float32)

    def forward16(self, xq, x_scale, target, rows, d):
      return plan_forward16(xq, x_scale, target, rows, d)
  return NumpyKernels16


# ---------------------------------------------------------------- what mi355q_qfc_forward_i16 refuses before a launch
def check_forward16_refusals(lib) -> None:
  """Every refusal of include/mi355q.h with its status code. Host buffers stand in for device pointers: each call
  returns before it launches (the last two enqueue nothing)."""
  import ctypes
  buf = ctypes.create_string_buffer(4096)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error
  I8, I16 = 3, 4

  def call(xq=p, n=4, d=64, x_scale=p, x_count=1, w=p, kind=I8, rows=8, w_scale=p, w_count=1, block=0, y=p, acc=None,
           ws=p, ws_bytes=2048):
    return lib.mi355q_qfc_forward_i16(xq, n, d, x_scale, x_count, w, kind, rows, w_scale, w_count, block, y, acc, ws,
                                      ws_bytes, None)
  for null in ("xq", "x_scale", "w", "w_scale", "y"):
    assert call(**{null: None}) == -1 and b"null pointer" in err(), null
  for shape in ("n", "d", "rows"):
    assert call(**{shape: -1}) == -1 and b"negative shape" in err(), shape
  assert call(kind=I16) == -1 and b"weight kind 4" in err()
  assert call(kind=0) == -1 and b"weight kind 0" in err()
  for count in (0, 2, 3, 5):
    assert call(x_count=count) == -1 and b"x_scale_count must be 1 or n" in err(), count
  for count in (0, 2, 7, 9, 16):
    assert call(w_count=count) == -1 and b"w_scale_count must be 1, rows" in err(), count
  assert call(w_count=16, block=48) == -1 and b"block must be 0, 32, 64, 128 or 256 (got 48)" in err()
  assert call(d=48, block=32, w_count=12) == -2 and b"Quantized dimension 48 is not divisible by block size 32." in err()
  assert call(d=96, block=64, w_count=12) == -2 and b"Quantized dimension 96 is not divisible by block size 64." in err()
  assert call(w_count=16, block=32, acc=p) == -1 and b"acc_out is not available with blockwise scales" in err()
  assert call(w_count=8, block=64, acc=p) == -1 and b"acc_out is not available with blockwise scales" in err()
  assert call(d=65537) == -3 and b"exceeds 65536" in err()
  assert call(d=65600, block=32, w_count=8 * 2050) == -3 and b"exceeds 65536" in err()
  # the weight sums are a term of every accumulator: the workspace is always required
  assert call(ws=None, ws_bytes=0) == -1 and b"workspace" in err()
  assert call(ws=None, ws_bytes=2048) == -1 and b"workspace" in err()
  assert call(ws_bytes=16) == -1 and b"workspace of 16 bytes is smaller than the 256 needed" in err()
  assert call(rows=100, d=512, block=32, w_count=1600, ws_bytes=6399) == -1 and b"smaller than the 6400 needed" in err()
  # after those, an empty request enqueues nothing
  assert call(n=0, x_count=1) == 0 and err() == b""
  assert call(n=0, x_count=0) == 0 and err() == b""
  assert call(rows=0, w_count=1, ws=None, ws_bytes=0) == 0 and err() == b""
  assert lib.mi355q_qfc_forward_i16_workspace_bytes(8, 64, 0) == 256
  assert lib.mi355q_qfc_forward_i16_workspace_bytes(100, 512, 32) == ((100 * 16 * 4 + 255) // 256) * 256
  assert lib.mi355q_qfc_forward_i16_workspace_bytes(0, 64, 0) == 0
  assert lib.mi355q_qfc_forward_i16_workspace_bytes(8, 96, 64) == 0
