"""Shared by test_gpu_layer_execution.py and test_layer_execution_host.py: the NumPy statement of the integer
FULLY_CONNECTED arithmetic (include/mi355q.h, "Integer execution of a quantized FULLY_CONNECTED op") and a NumPy
stand-in for model_validator.LayerExecutionKernels built from it."""
import numpy as np

import layer_error_cases as LC

BITS = {"i8": 8, "i4": 4, "i2": 2}


# ---------------------------------------------------------------- the arithmetic
def quantize_rows(x: np.ndarray):
  """Dynamic activation rows: (q int8 [n, d], scale float32 [n]). The product x * inv is rounded to float32 once;
  the rounding half away from zero is done in float64 on that float32 value, where |v| + 0.5 is exact."""
  x = np.asarray(x, np.float32)
  n, d = x.shape
  q = np.zeros((n, d), np.int8)
  scale = np.ones(n, np.float32)
  for t in range(n):
    row = x[t]
    if d == 0:
      continue
    if not np.all(np.isfinite(row)):
      scale[t] = np.nan
      continue
    rng = np.float32(np.max(np.abs(row)))
    if rng == 0:
      continue
    scale[t] = rng / np.float32(127.0)
    inv = np.float32(127.0) / rng
    v = (row * inv).astype(np.float32).astype(np.float64)
    r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    q[t] = np.clip(r, -127, 127).astype(np.int8)
  return q, scale


def quantize_static(x: np.ndarray, scale, zero_point: int) -> np.ndarray:
  """The static activation quantizer as ops.quantize stands: q = clip(rint(fl(fl(x / s_x) + zp_x)), -128, 127), the
  quotient and the sum in float32 (the zero point is added before the rounding to an integer)."""
  v = (np.asarray(x, np.float32) / np.float32(scale)).astype(np.float32) + np.float32(zero_point)
  return np.clip(np.rint(v.astype(np.float32)), -128, 127).astype(np.int8)


def unpack(stored: np.ndarray, kind: str, n: int) -> np.ndarray:
  """The n integers of a stored weight: int8 as they are, int4 / int2 from packed bytes, element 0 in the low bits."""
  if kind == "i8":
    return np.asarray(stored).view(np.int8).ravel()[:n].astype(np.int64)
  bits = BITS[kind]
  per = 8 // bits
  b = np.asarray(stored).view(np.uint8).ravel().astype(np.int64)
  fields = np.stack([(b >> (bits * i)) & ((1 << bits) - 1) for i in range(per)], axis=1).ravel()[:n]
  return np.where(fields >= (1 << (bits - 1)), fields - (1 << bits), fields)


def forward(xq: np.ndarray, x_scale, x_zero_point: int, qw: np.ndarray, w_scale, block: int = 0):
  """(acc int64 [n, rows] or None when blockwise, y float32 [n, rows]) of int8 xq [n, d] and integers qw [rows, d].
  x_scale: 1 or n float32; w_scale: 1 or rows float32 (block = 0), or rows * d / block float32 (blockwise)."""
  xq, qw = np.asarray(xq), np.asarray(qw)
  n, d = xq.shape
  rows = qw.shape[0]
  xi = xq.astype(np.int64) - int(x_zero_point)
  wi = qw.astype(np.int64)
  xs = np.broadcast_to(np.asarray(x_scale, np.float32).reshape(-1), (n,)).astype(np.float32)
  ws = np.asarray(w_scale, np.float32).reshape(-1)
  with np.errstate(invalid="ignore", over="ignore"):
    if block == 0:
      acc = xi @ wi.T
      assert np.abs(acc).max(initial=0) < 2 ** 31
      sw = np.broadcast_to(ws, (rows,)).astype(np.float32)
      sc = xs[:, None] * sw[None, :]
      return acc, acc.astype(np.int32).astype(np.float32) * sc
    sw = ws.reshape(rows, d // block)
    y = np.zeros((n, rows), np.float32)
    for b in range(d // block):
      acc = xi[:, b * block:(b + 1) * block] @ wi[:, b * block:(b + 1) * block].T
      p = acc.astype(np.int32).astype(np.float32) * (xs[:, None] * sw[None, :, b])
      y = y + p
    return None, y


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
  """Equal float32 bit patterns, any NaN matching any NaN."""
  got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
  nan = np.isnan(want)
  return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
          and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


# ---------------------------------------------------------------- a model's weight as the validators describe it
def plan_integers(plan, rows: int, d: int) -> np.ndarray:
  return unpack(np.asarray(plan.data), plan.kind, rows * d).reshape(rows, d)


def plan_forward(xq, x_scale, x_zero_point, plan, rows: int, d: int) -> np.ndarray:
  """forward() with the granularity read from a ConstantPlan's scale view, as ops.qfc_forward reads it."""
  qw = plan_integers(plan, rows, d)
  if plan.channels == 1 or (plan.channels == rows and plan.inner == d):
    return forward(xq, x_scale, x_zero_point, qw, plan.scale, 0)[1]
  assert plan.inner in (32, 64, 128, 256) and plan.channels * plan.inner == rows * d
  return forward(xq, x_scale, x_zero_point, qw, plan.scale, plan.inner)[1]


def plan_dequantized(plan, rows: int, d: int) -> np.ndarray:
  q = unpack(np.asarray(plan.data), plan.kind, rows * d)
  return LC.dequantize(q, plan.scale, plan.zero_point, plan.channels, plan.inner, 32).reshape(rows, d)


def numpy_kernels(rotate=None, gemm_dtype=np.float32):
  """A LayerExecutionKernels whose every method is NumPy. `rotate(x, h)`: the rotation of rows (default: the float64
  product with the graph's own float32 Sylvester matrix, rounded to float32); `gemm_dtype`: the precision of the float products."""
  from mi355q import model_validator as mv
  from mi355q.transformations import graph_edits

  def default_rotate(x, h):
    m = np.asarray(graph_edits._sylvester_hadamard_f32(h), np.float64)      # pylint: disable=protected-access
    return (x.astype(np.float64).reshape(-1, h) @ m).reshape(x.shape).astype(np.float32)

  class NumpyKernels(mv.LayerExecutionKernels):
    def sample(self, value, d):
      value = value.cpu().numpy() if hasattr(value, "cpu") else np.asarray(value)
      return np.ascontiguousarray(value, np.float32).reshape(-1, d)

    def weight(self, values, rows, d):
      return np.asarray(values, np.float32).reshape(rows, d)

    def target(self, plan):
      return plan

    def dequantized(self, target, rows, d):
      return plan_dequantized(target, rows, d)

    def transform(self, x, kind, multiplier, hadamard_size):
      if kind == mv.TRANSFORM_MULTIPLY:
        return x * np.asarray(multiplier, np.float32)
      if kind == mv.TRANSFORM_HADAMARD:
        return (rotate or default_rotate)(x, hadamard_size)
      return x

    def gemm(self, x, w):
      return (np.asarray(x, gemm_dtype) @ np.asarray(w, gemm_dtype).T)

    def quantize_dynamic(self, x):
      return quantize_rows(x)

    def quantize_static(self, x, scale, zero_point):
      return quantize_static(x, scale, zero_point), np.array([scale], np.float32)

    def forward(self, xq, x_scale, x_zero_point, target, rows, d):
      return plan_forward(xq, x_scale, x_zero_point, target, rows, d)

    def sqdiff(self, yq, y, sums):
      a, b = np.asarray(yq, np.float64), np.asarray(y, np.float64)
      sq_d, sq_b = ((a - b) ** 2).sum(axis=0), (b ** 2).sum(axis=0)
      return (sq_d, sq_b) if sums is None else (sums[0] + sq_d, sums[1] + sq_b)

    def host(self, sums):
      return sums
  return NumpyKernels


# ---------------------------------------------------------------- what mi355q_qfc_forward_i8 refuses before a launch
def check_forward_refusals(lib) -> None:
  """Every refusal of include/mi355q.h with its status code. Host buffers stand in for device pointers: each call
  returns before it launches (the last two enqueue nothing)."""
  import ctypes
  buf = ctypes.create_string_buffer(4096)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error
  I8, I16 = 3, 4

  def call(xq=p, n=4, d=64, x_scale=p, x_count=1, zp=0, w=p, kind=I8, rows=8, w_scale=p, w_count=1, block=0, y=p,
           acc=None, ws=p, ws_bytes=2048):
    return lib.mi355q_qfc_forward_i8(xq, n, d, x_scale, x_count, zp, w, kind, rows, w_scale, w_count, block, y, acc, ws,
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
  assert call(zp=128) == -1 and call(zp=-129) == -1 and b"outside int8" in err()
  assert call(zp=5, ws=None, ws_bytes=0) == -1 and b"workspace" in err()
  assert call(zp=5, ws_bytes=16) == -1 and b"workspace of 16 bytes is smaller than the 256 needed" in err()
  # after those, an empty request enqueues nothing
  assert call(n=0, x_count=1) == 0 and err() == b""
  assert call(rows=0, w_count=1) == 0 and err() == b""
  assert lib.mi355q_qfc_forward_workspace_bytes(8, 64, 0) == 256
  assert lib.mi355q_qfc_forward_workspace_bytes(100, 512, 32) == ((100 * 16 * 4 + 255) // 256) * 256
