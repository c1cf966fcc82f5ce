"""Shared by test_conv_execution_host.py and test_gpu_conv_execution.py: the NumPy statement of the CONV_2D patch
gather (include/mi355q.h, "Patch gather for CONV_2D"), an INDEPENDENT direct convolution on int64 / Python integers
that loops over taps and never builds patches, the gather's case list, a hand-built float model of three CONV_2D ops
and one FULLY_CONNECTED with its samples, a hand-quantized form of it for the host tests, and NumPy stand-ins for the
LayerExecutionKernels methods of `conv_2d`."""
import copy
import itertools
import struct

import numpy as np

import layer_execution_cases as EC
import layer_output_cases as OC

SAME, VALID = "SAME", "VALID"


# ---------------------------------------------------------------- geometry, written out once more (TFLite's rule)
def geometry(h, w, kh, kw, strides, dilations, padding):
  """(oh, ow, pad_top, pad_left), or None without a positive output size."""
  out = []
  for size, k, s, dil in ((h, kh, strides[0], dilations[0]), (w, kw, strides[1], dilations[1])):
    eff = (k - 1) * dil + 1
    o = (size + s - 1) // s if padding == SAME else (size + s - eff) // s
    if o < 1:
      return None
    out.append((o, max(0, (o - 1) * s + eff - size) // 2))
  return out[0][0], out[1][0], out[0][1], out[1][1]


# ---------------------------------------------------------------- the gather
def gather(x: np.ndarray, kh, kw, strides, dilations, padding, pad, first=0, count=None) -> np.ndarray:
  """The statement, element by element over (row, tap): rows first .. first + count - 1 of the [N OH OW, KH KW C]
  patch rows of x [N, H, W, C]; a tap outside the image holds `pad` (one element of x's dtype, copied as bytes)."""
  n_img, h, w, c = x.shape
  oh_n, ow_n, top, left = geometry(h, w, kh, kw, strides, dilations, padding)
  total = n_img * oh_n * ow_n
  count = total - first if count is None else count
  assert 0 <= first and first + count <= total
  pad = np.asarray(pad, x.dtype).reshape(())
  out = np.empty((count, kh * kw * c), x.dtype)
  out.view(np.uint8).reshape(-1)[:] = np.tile(np.frombuffer(pad.tobytes(), np.uint8), count * kh * kw * c)
  for r in range(count):
    t = first + r
    n, oh, ow = t // (oh_n * ow_n), (t // ow_n) % oh_n, t % ow_n
    for i in range(kh):
      ih = oh * strides[0] - top + i * dilations[0]
      if not 0 <= ih < h:
        continue
      for j in range(kw):
        iw = ow * strides[1] - left + j * dilations[1]
        if 0 <= iw < w:
          out[r, (i * kw + j) * c:(i * kw + j + 1) * c] = x[n, ih, iw]
  return out


def direct_conv(xq: np.ndarray, zero_point: int, qw: np.ndarray, strides, dilations, padding) -> np.ndarray:
  """int64 [N OH OW, O] = Sum over taps INSIDE the image and channels of (xq - zero_point) q_w, of integers
  xq [N, H, W, C] and qw [O, KH, KW, C]: the convolution itself, one output element at a time. A tap outside the image
  adds nothing (that is what a pad element equal to the zero point means), and no patch array is formed."""
  n_img, h, w, c = xq.shape
  o_n, kh, kw, _ = qw.shape
  oh_n, ow_n, top, left = geometry(h, w, kh, kw, strides, dilations, padding)
  xi, wi = xq.astype(np.int64) - int(zero_point), qw.astype(np.int64)
  assert kh * kw * c * int(np.abs(xi).max(initial=0)) * int(np.abs(wi).max(initial=0)) < 1 << 62
  out = np.zeros((n_img, oh_n, ow_n, o_n), np.int64)
  for i in range(kh):
    for j in range(kw):
      for oh in range(oh_n):
        ih = oh * strides[0] - top + i * dilations[0]
        if not 0 <= ih < h:
          continue
        for ow in range(ow_n):
          iw = ow * strides[1] - left + j * dilations[1]
          if 0 <= iw < w:
            out[:, oh, ow, :] += np.einsum("nc,oc->no", xi[:, ih, iw, :], wi[:, i, j, :])
  return out.reshape(-1, o_n)


# ---------------------------------------------------------------- the gather's cases
IMAGES = ((1, 1), (4, 4), (5, 7))
KERNELS = ((1, 1), (3, 3), (2, 5), (7, 7))
STRIDES = ((1, 1), (2, 2), (2, 1), (3, 2))
DILATIONS = ((1, 1), (2, 2), (1, 3))
BATCHES = (1, 3)


def geometries():
  """Every (N, H, W, kernel, strides, dilations, padding) of the cross with a positive output size; under SAME that
  includes kernels larger than the image."""
  out = []
  for (h, w), k, s, dil, padding, n in itertools.product(IMAGES, KERNELS, STRIDES, DILATIONS, (SAME, VALID), BATCHES):
    if geometry(h, w, k[0], k[1], s, dil, padding) is not None:
      out.append((n, h, w, k, s, dil, padding))
  return out


NAN_PAYLOAD = np.frombuffer(struct.pack("<I", 0x7FC12345), np.float32)[0]
DTYPES = {1: np.int8, 2: np.int16, 4: np.float32}
# (elem_bytes, C, pad, misaligned base): the vector route at its smallest C per width, the generic route
ROUTES = (
    (1, 16, -128, False), (2, 8, 0, False), (4, 4, 0.0, False), (1, 32, 127, False),           # vector
    (1, 1, 5, False), (1, 3, -128, False), (1, 20, 127, False), (1, 16, 5, True),              # generic
    (2, 3, 0, False), (4, 1, NAN_PAYLOAD, False), (4, 4, NAN_PAYLOAD, False), (2, 8, 0, True), (4, 3, 0.0, False))


def is_vector(elem_bytes, c, misaligned) -> bool:
  return (c * elem_bytes) % 16 == 0 and not misaligned


def random_tensor(rng, shape, elem_bytes) -> np.ndarray:
  """Full-range integers; floats with -0.0, infinities and NaNs of several payloads among them (a byte copy keeps all)."""
  if elem_bytes == 4:
    bits = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    return bits.view(np.float32)
  info = np.iinfo(DTYPES[elem_bytes])
  return rng.integers(info.min, info.max, size=shape, endpoint=True).astype(DTYPES[elem_bytes])


def same_bytes(a: np.ndarray, b: np.ndarray) -> bool:
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def windows(total: int, per_image: int):
  """(first, count): the whole output, (1, n - 2), two rows that straddle two images, the last row alone."""
  out = [(0, total), (total - 1, 1)]
  if total > 2:
    out.append((1, total - 2))
  if total > per_image:
    out.append((per_image - 1, 2))
  return out


# ---------------------------------------------------------------- Conv2DOptions as the flatbuffer layer keeps it
def conv_options_table(padding=None, stride_w=None, stride_h=None, fused=None, dilation_w=None, dilation_h=None):
  """An OpaqueTableT laid out as a flatbuffer writer lays Conv2DOptions out (fields ids 0 .. 5: padding i8, stride_w
  i32, stride_h i32, fused_activation_function i8, dilation_w_factor i32, dilation_h_factor i32). A field given as
  None is ABSENT, as a writer leaves out a field at its default."""
  from mi355q.utils import tflite_flatbuffer as fb
  inline = bytearray(4)      # (the vtable reference)
  fields = ((padding, "<b"), (stride_w, "<i"), (stride_h, "<i"), (fused, "<b"), (dilation_w, "<i"), (dilation_h, "<i"))
  offsets = [0] * 6
  for fmt in ("<i", "<b"):      # (the 4-byte scalars first, so that each is aligned without padding)
    for index, (value, field_fmt) in enumerate(fields):
      if value is not None and field_fmt == fmt:
        offsets[index] = len(inline)
        inline += struct.pack(fmt, int(value))
  while offsets and offsets[-1] == 0:
    offsets.pop()
  inline += bytes((-len(inline)) % 4)
  return fb.OpaqueTableT(offsets, bytes(inline), 0)


# ---------------------------------------------------------------- the model
# (name, input channels, output channels, kernel, strides, dilations, padding, has bias, fused)
CONVS = (("convA", 16, 24, (3, 3), (1, 1), (1, 1), SAME, True, OC.RELU),
         ("convB", 3, 8, (5, 5), (2, 2), (1, 1), VALID, False, OC.NONE),
         ("convC", 16, 16, (3, 3), (1, 1), (2, 2), SAME, True, OC.RELU6))
FC = ("fc", 32, 12)      # (name, d, rows): bias, no activation
BATCH, HEIGHT, WIDTH = 2, 9, 11
SAMPLES = 3
PADDING_CODE = {SAME: 0, VALID: 1}


def build_model():
  """ModelT tree: three CONV_2D ops `<op>/x` [2, 9, 11, C] -> `<op>/y` and one FULLY_CONNECTED, each with its own
  input. Conv2DOptions is an OpaqueTableT, what the reader makes of a file; convC's strides are explicit, its
  dilations too, and convA leaves the dilations absent (the schema's default 1)."""
  from mi355q import qtyping as q
  model = q.ModelT(version=3, description=b"three CONV_2D ops and one FULLY_CONNECTED (synthetic)")
  model.buffers = [q.BufferT()]
  sg = q.SubGraphT(name=b"main", tensors=[], operators=[], inputs=[], outputs=[])
  rng = np.random.default_rng(211)

  def tensor(name, shape, data=None):
    buffer = 0
    if data is not None:
      model.buffers.append(q.BufferT(data=np.ascontiguousarray(data, np.float32).reshape(-1).view(np.uint8)))
      buffer = len(model.buffers) - 1
    sg.tensors.append(q.TensorT(name=name.encode(), shape=list(shape), buffer=buffer))
    return len(sg.tensors) - 1
  for name, c, o, k, s, dil, padding, has_bias, fused in CONVS:
    oh, ow, _, _ = geometry(HEIGHT, WIDTH, k[0], k[1], s, dil, padding)
    x = tensor(f"{name}/x", [BATCH, HEIGHT, WIDTH, c])
    scale = np.float32(1.2 / np.sqrt(k[0] * k[1] * c))
    w = tensor(f"{name}/w", [o, k[0], k[1], c], rng.standard_normal((o, k[0], k[1], c), dtype=np.float32) * scale)
    b = tensor(f"{name}/b", [o], rng.standard_normal(o, dtype=np.float32) * np.float32(1.5)) if has_bias else -1
    y = tensor(f"{name}/y", [BATCH, oh, ow, o])
    sg.inputs.append(x)
    sg.outputs.append(y)
    table = conv_options_table(PADDING_CODE[padding] or None, s[1], s[0], fused or None,
                               None if dil == (1, 1) else dil[1], None if dil == (1, 1) else dil[0])
    sg.operators.append(q.OperatorT(inputs=[x, w, b] if has_bias else [x, w], outputs=[y], opcodeIndex=0,
                                    builtinOptionsType=1, builtinOptions=table))
  name, d, rows = FC
  x = tensor(f"{name}/x", [1, d])
  w = tensor(f"{name}/w", [rows, d], rng.standard_normal((rows, d), dtype=np.float32) * np.float32(0.3))
  b = tensor(f"{name}/b", [rows], rng.standard_normal(rows, dtype=np.float32))
  y = tensor(f"{name}/y", [1, rows])
  sg.inputs.append(x)
  sg.outputs.append(y)
  sg.operators.append(q.OperatorT(inputs=[x, w, b], outputs=[y], opcodeIndex=1, builtinOptionsType=8,
                                  builtinOptions=q.FullyConnectedOptionsT(fusedActivationFunction=OC.NONE)))
  model.operatorCodes = [q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.CONV_2D), deprecatedBuiltinCode=3),
                         q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.FULLY_CONNECTED), deprecatedBuiltinCode=9)]
  model.subgraphs = [sg]
  model.signatureDefs = [q.SignatureDefT(signatureKey=b"serving_default", subgraphIndex=0)]
  return model


def constant(model, name) -> np.ndarray:
  t = next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)
  return np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()


def float_conv(model, conv, x, dtype=np.float64, pre_bias=False) -> np.ndarray:
  """act(patches(x, pad 0) W^T + b) [N OH OW, O] of the float op in `dtype`; `pre_bias`: the product alone."""
  name, c, o, k, s, dil, padding, has_bias, fused = conv
  p = gather(np.asarray(x, np.float32), k[0], k[1], s, dil, padding, 0.0).astype(dtype)
  y = p @ constant(model, f"{name}/w").reshape(o, -1).astype(dtype).T
  if pre_bias:
    return y
  if has_bias:
    y = y + constant(model, f"{name}/b").astype(dtype)
  return OC.float_activation(y, fused)


def build_samples(model):
  """[{tensor name: float32 array}]: inputs ~ N(0, 1) and the float model's own outputs (NumPy), so that calibration
  yields meaningful (s_y, zp_y)."""
  rng = np.random.default_rng(212)
  samples = []
  for _ in range(SAMPLES):
    s = {}
    for conv in CONVS:
      name, c, o, k, st, dil, padding = conv[:7]
      oh, ow, _, _ = geometry(HEIGHT, WIDTH, k[0], k[1], st, dil, padding)
      x = rng.standard_normal((BATCH, HEIGHT, WIDTH, c), dtype=np.float32)
      s[f"{name}/x"] = x
      s[f"{name}/y"] = float_conv(model, conv, x, np.float32).reshape(BATCH, oh, ow, o)
    name, d, rows = FC
    x = rng.standard_normal((1, 7, d), dtype=np.float32)
    s[f"{name}/x"] = x
    s[f"{name}/y"] = (x.reshape(-1, d) @ constant(model, f"{name}/w").T + constant(model, f"{name}/b")).reshape(1, 7, rows)
    samples.append(s)
  return samples


def patch_rows(conv) -> int:
  k, st, dil, padding = conv[3:7]
  oh, ow, _, _ = geometry(HEIGHT, WIDTH, k[0], k[1], st, dil, padding)
  return BATCH * oh * ow


# ---------------------------------------------------------------- the model quantized by hand (host tests: no device)
def quantize_by_hand(model, samples, mode="static", bits=8):
  """`mode` "static": activations INT8 / INT16 with (s, zp) from the samples' range, filters per-channel symmetric int8
  along dimension 0, biases INT32 / INT64 on the grid s_x s_w. "dynamic": the integer filters alone, activations
  float. "weight_only": as dynamic, with a DEQUANTIZE op between every integer filter and its op."""
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
  ops_of = [(c[0], c[2], c[7]) for c in CONVS] + [(FC[0], FC[2], True)]
  for name, rows, has_bias in ops_of:
    w = constant(model, f"{name}/w")
    t = by_name[f"{name}/w"]
    flat = w.reshape(rows, -1)
    s_w = (np.abs(flat).max(axis=1) / 127.0).astype(np.float32)
    t.type = int(q.TensorType.INT8)
    t.quantization = q.QuantizationParametersT(scale=s_w, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=0)
    tgt.buffers[t.buffer].data = np.clip(np.rint(flat / s_w[:, None]), -127, 127).astype(np.int8).reshape(-1).view(np.uint8)
    if mode != "static":
      continue
    for end in ("x", "y"):
      a = by_name[f"{name}/{end}"]
      scale, zp = grid([s[f"{name}/{end}"] for s in samples])
      a.type = act_type
      a.quantization = q.QuantizationParametersT(scale=np.array([scale], np.float32), zeroPoint=np.array([zp], np.int64))
    if has_bias:
      s_x = np.float32(by_name[f"{name}/x"].quantization.scale[0])
      b = by_name[f"{name}/b"]
      s_b = (s_x * s_w).astype(np.float32)
      ints = np.rint(constant(model, f"{name}/b").astype(np.float64) / s_b.astype(np.float64))
      b.type = int(q.TensorType.INT64 if bits == 16 else q.TensorType.INT32)
      b.quantization = q.QuantizationParametersT(scale=s_b, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=0)
      tgt.buffers[b.buffer].data = ints.astype(np.int64 if bits == 16 else np.int32).view(np.uint8)
  if mode == "weight_only":
    tgt.operatorCodes.append(q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.DEQUANTIZE), deprecatedBuiltinCode=6))
    new_ops = []
    for op in sg.operators:
      w_index = op.inputs[1]
      w_t = sg.tensors[w_index]
      sg.tensors.append(q.TensorT(name=w_t.name + b"_dequant", shape=list(w_t.shape), buffer=0))
      new_ops.append(q.OperatorT(inputs=[w_index], outputs=[len(sg.tensors) - 1], opcodeIndex=len(tgt.operatorCodes) - 1))
      op.inputs = [op.inputs[0], len(sg.tensors) - 1] + list(op.inputs[2:])
      new_ops.append(op)
    sg.operators = new_ops
  return tgt


# ---------------------------------------------------------------- NumPy in place of the device
def numpy_kernels(**kwargs):
  """layer_output_cases.numpy_kernels() with the three methods of `conv_2d`."""
  class NumpyConvKernels(OC.numpy_kernels(**kwargs)):
    def sample4d(self, value):
      value = value.cpu().numpy() if hasattr(value, "cpu") else np.asarray(value)
      return np.ascontiguousarray(value, np.float32)

    def patches(self, x, kernel, strides, dilations, padding, pad_value, first, count):
      return gather(np.asarray(x), kernel[0], kernel[1], strides, dilations, padding, pad_value, first, count)

    def quantize_dynamic_images(self, x, patch_rows_per_image):
      q, scale = EC.quantize_rows(np.asarray(x, np.float32).reshape(x.shape[0], -1))
      return q.reshape(x.shape), np.repeat(scale, patch_rows_per_image)
  return NumpyConvKernels


# ---------------------------------------------------------------- what mi355q_conv_patches_nhwc refuses before a launch
def check_patch_refusals(lib) -> None:
  """Every refusal of include/mi355q.h with its status code. Host buffers stand in for device pointers: each call
  returns before it launches (the last ones enqueue nothing)."""
  import ctypes
  buf = ctypes.create_string_buffer(4096)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error

  def call(x=p, eb=1, N=2, H=5, W=7, C=16, KH=3, KW=3, sh=1, sw=1, dh=1, dw=1, top=1, left=1, OH=5, OW=7, first=0, count=1,
           pad=p, out=p):
    return lib.mi355q_conv_patches_nhwc(x, eb, N, H, W, C, KH, KW, sh, sw, dh, dw, top, left, OH, OW, first, count, pad, out, None)
  for null in ("x", "out", "pad"):
    assert call(**{null: None}) == -1 and b"null pointer" in err(), null
  for eb in (0, 3, 8, -1):
    assert call(eb=eb) == -1 and b"elem_bytes must be 1, 2 or 4" in err(), eb
  for dim in ("N", "H", "W", "C", "KH", "KW", "OH", "OW"):
    for bad in (0, -1):
      assert call(**{dim: bad}) == -1 and b"every dimension must be positive" in err(), dim
  for stride in ("sh", "sw"):
    for bad in (0, -2):
      assert call(**{stride: bad}) == -1 and b"strides must be positive" in err(), stride
  for dil in ("dh", "dw"):
    for bad in (0, -2):
      assert call(**{dil: bad}) == -1 and b"dilations must be positive" in err(), dil
  assert call(first=-1) == -1 and call(count=-1) == -1 and b"negative row window" in err()
  assert call(OH=1 << 16, OW=1 << 15, N=1) == -3 and b"exceeds INT32_MAX" in err()
  assert call(OH=1 << 15, OW=1 << 15, N=2) == -3 and b"exceeds INT32_MAX" in err()
  assert call(OH=1 << 40) == -3 and b"exceeds INT32_MAX" in err()
  assert call(first=70, count=1) == -1 and b"outside the 70 patch rows" in err()
  assert call(first=0, count=71) == -1 and b"outside the 70 patch rows" in err()
  assert call(first=69, count=2) == -1 and b"outside the 70 patch rows" in err()
  assert call(C=65537, KH=1, KW=1) == -3 and b"exceeds 65536" in err()
  assert call(C=4096, KH=4, KW=5) == -3 and b"exceeds 65536" in err()
  assert call(C=1, KH=1 << 20, KW=1 << 20) == -3 and b"exceeds 65536" in err()
  assert call(N=1 << 30, H=1 << 31, W=1 << 31, C=65536, KH=1, KW=1, OH=1, OW=1, count=0) == -3 and b"2^62 bytes" in err()
  # after those, an empty window enqueues nothing, whatever the pointers
  assert call(count=0) == 0 and err() == b""
  assert call(first=70, count=0, x=None, out=None, pad=None) == 0 and err() == b""
  assert call(C=65536, KH=1, KW=1, count=0) == 0 and err() == b""
