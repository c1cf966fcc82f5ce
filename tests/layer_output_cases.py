"""Shared by test_layer_output_host.py and test_gpu_layer_output.py: the statement of a static FULLY_CONNECTED op's
integer execution through to its stored output (include/mi355q.h, "Integer execution, through to the stored
output"), written on PYTHON INTEGERS, whose precision is arbitrary: no intermediate can wrap, so a saturation is in
the statement only where it is written. A small float model with biases and fused activations, its samples, a
hand-quantized static form of it for the host tests, and a NumPy stand-in for the new LayerExecutionKernels methods."""
import copy
import fractions
import math

import numpy as np

import layer_execution_cases as EC
import layer_execution_i16_cases as EC16

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
A16_MIN, A16_MAX = -(1 << 47), (1 << 47) - 1
NONE, RELU, RELU_N1_TO_1, RELU6 = 0, 1, 2, 3
TANH = 4
NAMES = {NONE: "NONE", RELU: "RELU", RELU_N1_TO_1: "RELU_N1_TO_1", RELU6: "RELU6"}


# ---------------------------------------------------------------- the arithmetic, on Python integers
def round_half_away(v) -> int:
  """Of a float or a Fraction, exactly (a float is a dyadic rational)."""
  f = fractions.Fraction(v)
  r = (abs(f) * 2 + 1) // 2      # floor(|v| + 1/2)
  return int(r) if f >= 0 else -int(r)


def quantize_multiplier(real: float):
  """(M, shift): real ~ M 2^(shift - 31)."""
  if real == 0.0:
    return 0, 0
  frac, exp = math.frexp(real)
  m = round_half_away(fractions.Fraction(frac) * (1 << 31))
  if m == 1 << 31:
    m, exp = 1 << 30, exp + 1
  if exp < -31:
    return 0, 0
  if exp > 30:
    raise ValueError("shift above 30")
  return m, exp


def sat32(v: int) -> int:
  return min(max(v, INT32_MIN), INT32_MAX)


def trunc_div(p: int, q: int) -> int:
  """C++ division of integers: towards zero."""
  return abs(p) // abs(q) * (1 if (p >= 0) == (q > 0) else -1)


def mbqm32(a: int, m: int, s: int) -> int:
  left, right = max(s, 0), max(-s, 0)
  v = sat32(a * (1 << left))
  p = v * m
  h = trunc_div(p + ((1 << 30) if p >= 0 else 1 - (1 << 30)), 1 << 31)
  mask = (1 << right) - 1
  return (h >> right) + (1 if (h & mask) > (mask >> 1) + (1 if h < 0 else 0) else 0)


def rounded_multiplier(m: int) -> int:
  return (m + (1 << 15)) >> 16 if m < 0x7FFF0000 else 0x7FFF


def mbqm64(a: int, m: int, s: int) -> int:
  """Of an `a` already clamped to [-2^47, 2^47 - 1]."""
  t = 15 - s
  return (a * rounded_multiplier(m) + (1 << (t - 1))) >> t      # (Python's >> of a negative integer is arithmetic)


def activation_range(fused: int, s_y: float, zp_y: int, bits: int):
  qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1

  def grid(f):
    return min(max(zp_y + round_half_away(f / float(s_y)), qmin), qmax)
  if fused == NONE:
    return qmin, qmax
  if fused == RELU:
    return max(qmin, zp_y), qmax
  if fused == RELU6:
    return grid(0.0), grid(6.0)
  if fused == RELU_N1_TO_1:
    return grid(-1.0), grid(1.0)
  raise ValueError(fused)


def accumulators(xq, x_zero_point: int, qw, limit: int):
  """[n][rows] Python integers Sum_k (xq - zp_x) q_w. The sum is formed in int64, which cannot wrap: |acc| <= `limit`
  < 2^63 is asserted, and from there on every value is a Python integer."""
  xi = np.asarray(xq).astype(np.int64) - int(x_zero_point)
  wi = np.asarray(qw).astype(np.int64)
  assert xi.shape[1] * int(np.abs(xi).max(initial=0)) * int(np.abs(wi).max(initial=0)) <= limit < 1 << 62
  return (xi @ wi.T).tolist()


def _tables(multiplier, shift, rows):
  m = [int(v) for v in np.asarray(multiplier).reshape(-1)]
  s = [int(v) for v in np.asarray(shift).reshape(-1)]
  assert len(m) == len(s) and len(m) in (1, rows)
  return (m * rows, s * rows) if len(m) == 1 and rows != 1 else (m, s)


def output_i8(xq, x_zero_point, qw, bias, multiplier, shift, out_zero_point, act_min, act_max) -> np.ndarray:
  """int8 [n, rows] = clamp(mbqm32(sat32(acc + bias), M, s) + zp_y, act_min, act_max)."""
  rows = np.asarray(qw).shape[0]
  acc = accumulators(xq, x_zero_point, qw, 65536 * 255 * 128)
  m, s = _tables(multiplier, shift, rows)
  b = [0] * rows if bias is None else [int(v) for v in np.asarray(bias).reshape(-1)]
  out = [[min(max(mbqm32(sat32(a + b[r]), m[r], s[r]) + int(out_zero_point), act_min), act_max)
          for r, a in enumerate(row)] for row in acc]
  return np.array(out, np.int64).reshape(len(acc), rows).astype(np.int8)


def output_i16(xq, qw, bias, multiplier, shift, act_min, act_max) -> np.ndarray:
  """int16 [n, rows] = clamp(mbqm64(clamp(acc + bias, -2^47, 2^47 - 1), M, s), act_min, act_max)."""
  rows = np.asarray(qw).shape[0]
  acc = accumulators(xq, 0, qw, 65536 * 32768 * 128)
  m, s = _tables(multiplier, shift, rows)
  b = [0] * rows if bias is None else [int(v) for v in np.asarray(bias).reshape(-1)]
  out = [[min(max(mbqm64(min(max(a + b[r], A16_MIN), A16_MAX), m[r], s[r]), act_min), act_max)
          for r, a in enumerate(row)] for row in acc]
  return np.array(out, np.int64).reshape(len(acc), rows).astype(np.int16)


def float_activation(y: np.ndarray, fused: int) -> np.ndarray:
  if fused == RELU:
    return np.maximum(y, y.dtype.type(0))
  if fused == RELU6:
    return np.clip(y, y.dtype.type(0), y.dtype.type(6))
  if fused == RELU_N1_TO_1:
    return np.clip(y, y.dtype.type(-1), y.dtype.type(1))
  assert fused == NONE
  return y


# ---------------------------------------------------------------- NumPy in place of the device
def numpy_kernels(**kwargs):
  """layer_execution_i16_cases.numpy_kernels() with the methods of `quantized_outputs`."""
  class NumpyOutputKernels(EC16.numpy_kernels(**kwargs)):
    def bias(self, values):
      return np.asarray(values)

    def output(self, xq, x_zero_point, target, rows, d, bias, multiplier, shift, out_zero_point, act_min, act_max):
      return output_i8(xq, x_zero_point, EC.plan_integers(target, rows, d), bias, multiplier, shift, out_zero_point,
                       act_min, act_max)

    def output16(self, xq, target, rows, d, bias, multiplier, shift, act_min, act_max):
      return output_i16(xq, EC.plan_integers(target, rows, d), bias, multiplier, shift, act_min, act_max)

    def dequantize_output(self, q, scale, zero_point):
      return (np.asarray(q).astype(np.int32) - int(zero_point)).astype(np.float32) * np.float32(scale)

    def reference_output(self, y, bias, fused):
      y = np.asarray(y, np.float32)
      if bias is not None:
        y = y + np.asarray(bias, np.float32)
      return float_activation(y, fused)
  return NumpyOutputKernels


# ---------------------------------------------------------------- the model
D = 128
OPS = (("fc0", 128, NONE, True), ("fc1", 96, RELU, True), ("fc2", 32, RELU6, True), ("fc3", 64, NONE, False))
TOKENS = (40, 33, 47)      # per sample


def build_model():
  """ModelT tree of four FULLY_CONNECTED ops `<op>/x` [1, 128] -> `<op>/y`, each with its own input: three with a
  bias and fused NONE / RELU / RELU6, a fourth without a bias."""
  from mi355q import qtyping as q
  model = q.ModelT(version=3, description=b"four FULLY_CONNECTED ops with bias and fused activations (synthetic)")
  model.buffers = [q.BufferT()]
  sg = q.SubGraphT(name=b"main", tensors=[], operators=[], inputs=[], outputs=[])
  rng = np.random.default_rng(77)

  def tensor(name, shape, data=None):
    buffer = 0
    if data is not None:
      model.buffers.append(q.BufferT(data=np.ascontiguousarray(data, np.float32).reshape(-1).view(np.uint8)))
      buffer = len(model.buffers) - 1
    sg.tensors.append(q.TensorT(name=name.encode(), shape=list(shape), buffer=buffer))
    return len(sg.tensors) - 1
  for name, rows, fused, has_bias in OPS:
    x = tensor(f"{name}/x", [1, D])
    w = tensor(f"{name}/w", [rows, D], rng.standard_normal((rows, D), dtype=np.float32) * np.float32(0.3))
    b = tensor(f"{name}/b", [rows], rng.standard_normal(rows, dtype=np.float32) * np.float32(1.5)) if has_bias else -1
    y = tensor(f"{name}/y", [1, rows])
    sg.inputs.append(x)
    sg.outputs.append(y)
    sg.operators.append(q.OperatorT(inputs=[x, w, b], outputs=[y], opcodeIndex=0, builtinOptionsType=8,
                                    builtinOptions=q.FullyConnectedOptionsT(fusedActivationFunction=fused)))
  model.operatorCodes = [q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.FULLY_CONNECTED), deprecatedBuiltinCode=9)]
  model.subgraphs = [sg]
  model.signatureDefs = [q.SignatureDefT(signatureKey=b"serving_default", subgraphIndex=0)]
  return model


def constant(model, name) -> np.ndarray:
  t = next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)
  return np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()


def float_output(model, name, fused, has_bias, x, dtype=np.float32) -> np.ndarray:
  """act(x W^T + b) of the float op `name` on rows x, in `dtype`."""
  y = np.asarray(x, dtype).reshape(-1, D) @ constant(model, f"{name}/w").astype(dtype).T
  if has_bias:
    y = y + constant(model, f"{name}/b").astype(dtype)
  return float_activation(y, fused)


def build_samples(model):
  """[{tensor name: float32 [1, tokens, width]}]: inputs ~ N(0, 1) and THE FLOAT MODEL'S OWN OUTPUTS (NumPy), so that
  calibration yields meaningful (s_y, zp_y). Checked here: under RELU6 some pre-activation values lie below 0 and some
  above 6, so the integer range clamps at both ends."""
  rng = np.random.default_rng(78)
  samples = []
  for tokens in TOKENS:
    s = {}
    for name, rows, fused, has_bias in OPS:
      x = rng.standard_normal((1, tokens, D), dtype=np.float32)
      s[f"{name}/x"] = x
      s[f"{name}/y"] = float_output(model, name, fused, has_bias, x).reshape(1, tokens, rows)
      if fused == RELU6:
        pre = float_output(model, name, NONE, has_bias, x)
        assert (pre < -0.5).sum() > 10 and (pre > 6.5).sum() > 10
        assert s[f"{name}/y"].min() == 0.0 and s[f"{name}/y"].max() == 6.0
    samples.append(s)
  return samples


def quantize_by_hand(model, samples, bits: int = 8):
  """A static form of build_model()'s tree written out in NumPy, for the host tests (no device): every `<op>/x`
  becomes INT8 / INT16 with (s_x, zp_x) from the samples' range, `<op>/w` per-channel symmetric int8, `<op>/b` INT32 /
  INT64 on the grid s_x s_w, `<op>/y` INT8 / INT16 with (s_y, zp_y) from the samples' range."""
  from mi355q import qtyping as q
  tgt = copy.deepcopy(model)
  sg = tgt.subgraphs[0]
  by_name = {t.name.decode(): t for t in sg.tensors}
  act_type = int(q.TensorType.INT16 if bits == 16 else q.TensorType.INT8)

  def grid(values):
    lo, hi = min(float(np.min(v)) for v in values), max(float(np.max(v)) for v in values)
    if bits == 16:
      return np.float32(max(abs(lo), abs(hi)) / 32767.0), 0
    lo, hi = min(lo, 0.0), max(hi, 0.0)
    scale = np.float32((hi - lo) / 255.0)
    return scale, int(np.clip(np.rint(-128 - lo / float(scale)), -128, 127))
  for name, rows, _, has_bias in OPS:
    for end in ("x", "y"):
      t = by_name[f"{name}/{end}"]
      scale, zp = grid([s[f"{name}/{end}"] for s in samples])
      t.type = act_type
      t.quantization = q.QuantizationParametersT(scale=np.array([scale], np.float32), zeroPoint=np.array([zp], np.int64))
    s_x = np.float32(by_name[f"{name}/x"].quantization.scale[0])
    w = constant(model, f"{name}/w")
    t = by_name[f"{name}/w"]
    s_w = (np.abs(w).max(axis=1) / 127.0).astype(np.float32)
    t.type = int(q.TensorType.INT8)
    t.quantization = q.QuantizationParametersT(scale=s_w, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=0)
    tgt.buffers[t.buffer].data = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8).reshape(-1).view(np.uint8)
    if has_bias:
      t = by_name[f"{name}/b"]
      s_b = (s_x * s_w).astype(np.float32)
      ints = np.rint(constant(model, f"{name}/b").astype(np.float64) / s_b.astype(np.float64))
      t.type = int(q.TensorType.INT64 if bits == 16 else q.TensorType.INT32)
      t.quantization = q.QuantizationParametersT(scale=s_b, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=0)
      tgt.buffers[t.buffer].data = ints.astype(np.int64 if bits == 16 else np.int32).view(np.uint8)
  return tgt


# ---------------------------------------------------------------- what the two entries refuse before a launch
def check_output_refusals(lib) -> None:
  """Every refusal of include/mi355q.h with its status code. Host buffers stand in for device pointers: each call
  returns before it launches (the last ones enqueue nothing)."""
  import ctypes
  buf = ctypes.create_string_buffer(4096)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error
  I8, I16 = 3, 4

  def call8(xq=p, n=4, d=64, zp=0, w=p, kind=I8, rows=8, bias=p, mult=p, shift=p, mcount=1, ozp=0, lo=-128, hi=127, q=p,
            ws=p, ws_bytes=2048):
    return lib.mi355q_qfc_output_i8(xq, n, d, zp, w, kind, rows, bias, mult, shift, mcount, ozp, lo, hi, q, ws, ws_bytes, None)

  def call16(xq=p, n=4, d=64, w=p, kind=I8, rows=8, bias=p, mult=p, shift=p, mcount=1, lo=-32768, hi=32767, q=p, ws=p,
             ws_bytes=2048):
    return lib.mi355q_qfc_output_i16(xq, n, d, w, kind, rows, bias, mult, shift, mcount, lo, hi, q, ws, ws_bytes, None)
  for call in (call8, call16):
    for null in ("xq", "w", "mult", "shift", "q"):
      assert call(**{null: None}) == -1 and b"null pointer" in err(), null
    for shape in ("n", "d", "rows"):
      assert call(**{shape: -1}) == -1 and b"negative shape" in err(), shape
    assert call(kind=I16) == -1 and b"weight kind 4 is not I8, I4 or I2" in err()
    assert call(kind=0) == -1 and b"weight kind 0" in err()
    for count in (0, 2, 7, 9):
      assert call(mcount=count) == -1 and b"mcount must be 1 or rows = 8" in err(), count
    assert call(lo=5, hi=4) == -1 and b"activation range [5, 4]" in err()
    assert call(d=65537) == -3 and b"exceeds 65536" in err()
    # after those, an empty request enqueues nothing; a bias may be absent
    assert call(n=0) == 0 and err() == b""
    assert call(rows=0, mcount=1, ws=None, ws_bytes=0) == 0 and err() == b""
    assert call(rows=0, mcount=0, ws=None, ws_bytes=0) == 0 and err() == b""
    assert call(n=0, bias=None, mcount=8) == 0 and err() == b""
  assert call8(zp=128) == -1 and b"activation zero point 128 is outside int8" in err()
  assert call8(zp=-129) == -1 and b"outside int8" in err()
  assert call8(ozp=128) == -1 and b"output zero point 128 is outside int8" in err()
  assert call8(ozp=-129) == -1 and b"output zero point -129" in err()
  assert call8(lo=-129) == -1 and call8(hi=128) == -1 and b"within int8" in err()
  assert call16(lo=-32769) == -1 and call16(hi=32768) == -1 and b"within int16" in err()
  # the workspace: under int8 only with a zero point, under int16 always
  assert call8(zp=5, ws=None, ws_bytes=0) == -1 and b"workspace" in err()
  assert call8(zp=5, ws_bytes=16) == -1 and b"workspace of 16 bytes is smaller than the 256 needed" in err()
  assert call8(n=0, zp=0, ws=None, ws_bytes=0) == 0 and err() == b""
  assert call16(ws=None, ws_bytes=0) == -1 and b"workspace" in err()
  assert call16(ws=None, ws_bytes=2048) == -1 and b"workspace" in err()
  assert call16(rows=100, mcount=100, ws_bytes=255) == -1 and b"smaller than the 512 needed" in err()
  assert call16(n=0) == 0 and err() == b""      # (and no message is left behind)
  assert lib.mi355q_qfc_output_workspace_bytes(8, 64) == 256
  assert lib.mi355q_qfc_output_workspace_bytes(100, 512) == 512
  assert lib.mi355q_qfc_output_workspace_bytes(0, 64) == 0 and lib.mi355q_qfc_output_workspace_bytes(8, 0) == 0
