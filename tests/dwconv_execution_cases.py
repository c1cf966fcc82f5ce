"""Shared by test_dwconv_execution_host.py and test_gpu_dwconv_execution.py: the NumPy statement of the float
depthwise convolution (include/mi355q.h, "Direct depthwise convolution": the float32 loop in tap order), an
INDEPENDENT direct integer depthwise convolution on int64 that walks pixels and taps one at a time, the rescales and
epilogues of the integer entries applied to its accumulators, a hand-built float model of three DEPTHWISE_CONV_2D ops
and one FULLY_CONNECTED with its samples, a hand-quantized form of it (per-channel scales along dimension 3), NumPy
stand-ins for the LayerExecutionKernels methods of `depthwise_conv_2d`, and the refusals of the five C entries."""
import copy
import struct

import numpy as np

import conv_execution_cases as CC
import layer_execution_cases as EC
import layer_execution_i16_cases as EC16
import layer_output_cases as OC

SAME, VALID = CC.SAME, CC.VALID


# ---------------------------------------------------------------- the float statement
def float_depthwise(x, w, multiplier, strides, dilations, padding, first=0, count=None) -> np.ndarray:
  """float32 [count, O]: y = (((0 + p_0) + p_1) ...), p = fl32(x w), over the taps INSIDE the image in ascending
  (kh, kw) order, of x [N, H, W, C] and w [KH, KW, O = C multiplier]. One float32 multiplication and one float32
  addition per tap, each an array operation over the pixels the tap is inside for: NumPy rounds each separately."""
  x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
  n_img, h, wd, c = x.shape
  kh_n, kw_n, o = w.shape
  assert o == c * multiplier
  oh_n, ow_n, top, left = CC.geometry(h, wd, kh_n, kw_n, strides, dilations, padding)
  source = np.arange(o) // multiplier
  y = np.zeros((n_img, oh_n, ow_n, o), np.float32)
  with np.errstate(invalid="ignore", over="ignore"):
    for kh in range(kh_n):
      ohs = [oh for oh in range(oh_n) if 0 <= oh * strides[0] - top + kh * dilations[0] < h]
      for kw in range(kw_n):
        ows = [ow for ow in range(ow_n) if 0 <= ow * strides[1] - left + kw * dilations[1] < wd]
        if not ohs or not ows:
          continue
        ih = np.array(ohs) * strides[0] - top + kh * dilations[0]
        iw = np.array(ows) * strides[1] - left + kw * dilations[1]
        p = (x[:, ih[:, None], iw[None, :], :][..., source] * w[kh, kw]).astype(np.float32)
        sel = np.ix_(range(n_img), ohs, ows, range(o))
        y[sel] = (y[sel] + p).astype(np.float32)
  total = n_img * oh_n * ow_n
  count = total - first if count is None else count
  assert 0 <= first and first + count <= total
  return y.reshape(total, o)[first:first + count]


# ---------------------------------------------------------------- the integer convolution, written independently
def direct_depthwise(xq, zero_point: int, qw, multiplier, strides, dilations, padding) -> np.ndarray:
  """int64 [N OH OW, O] = Sum over the taps inside the image of (xq - zero_point) q_w, of integers xq [N, H, W, C] and
  qw [KH, KW, O]: one output pixel at a time, one tap at a time, the bounds tested per tap."""
  xq, qw = np.asarray(xq), np.asarray(qw)
  n_img, h, w, c = xq.shape
  kh_n, kw_n, o = qw.shape
  assert o == c * multiplier
  oh_n, ow_n, top, left = CC.geometry(h, w, kh_n, kw_n, strides, dilations, padding)
  xi, wi = xq.astype(np.int64) - int(zero_point), qw.astype(np.int64)
  assert kh_n * kw_n * int(np.abs(xi).max(initial=0)) * int(np.abs(wi).max(initial=0)) < 1 << 62
  reads = np.repeat(np.arange(c), multiplier)      # output channel -> its input channel
  out = np.zeros((n_img * oh_n * ow_n, o), np.int64)
  for n in range(n_img):
    for oh in range(oh_n):
      for ow in range(ow_n):
        row = (n * oh_n + oh) * ow_n + ow
        for i in range(kh_n):
          for j in range(kw_n):
            ih, iw = oh * strides[0] - top + i * dilations[0], ow * strides[1] - left + j * dilations[1]
            if ih < 0 or ih >= h or iw < 0 or iw >= w:
              continue
            out[row] += xi[n, ih, iw][reads] * wi[i, j]
  return out


def image_of_rows(n_img: int, rows: int) -> np.ndarray:
  return np.repeat(np.arange(n_img), rows // n_img)


def rescale_i8(acc, x_scale, w_scale, n_img: int) -> np.ndarray:
  """fl32(float(acc) fl32(x_scale[image] w_scale[oc])): x_scale 1 or N entries (per IMAGE), w_scale 1 or O."""
  xs = np.broadcast_to(np.asarray(x_scale, np.float32).reshape(-1), (n_img,))[image_of_rows(n_img, acc.shape[0])]
  ws = np.broadcast_to(np.asarray(w_scale, np.float32).reshape(-1), (acc.shape[1],))
  assert np.abs(acc).max(initial=0) < 2 ** 31
  with np.errstate(invalid="ignore", over="ignore"):
    return acc.astype(np.int32).astype(np.float32) * (xs[:, None] * ws[None, :]).astype(np.float32)


def rescale_i16(acc, x_scale, w_scale, n_img: int) -> np.ndarray:
  xs = np.broadcast_to(np.asarray(x_scale, np.float32).reshape(-1), (n_img,))[image_of_rows(n_img, acc.shape[0])]
  ws = np.broadcast_to(np.asarray(w_scale, np.float32).reshape(-1), (acc.shape[1],))
  with np.errstate(invalid="ignore", over="ignore"):
    return EC16.rescale(np.ascontiguousarray(acc, np.int64), (xs[:, None] * ws[None, :]).astype(np.float32))


def epilogue_i8(acc, bias, multiplier, shift, out_zero_point, act_min, act_max) -> np.ndarray:
  """layer_output_cases' statement of the int8 epilogue on given accumulators (Python integers)."""
  o = acc.shape[1]
  m, s = OC._tables(multiplier, shift, o)      # pylint: disable=protected-access
  b = [0] * o if bias is None else [int(v) for v in np.asarray(bias).reshape(-1)]
  out = [[min(max(OC.mbqm32(OC.sat32(a + b[r]), m[r], s[r]) + int(out_zero_point), act_min), act_max)
          for r, a in enumerate(row)] for row in acc.tolist()]
  return np.array(out, np.int64).reshape(acc.shape).astype(np.int8)


def epilogue_i16(acc, bias, multiplier, shift, act_min, act_max) -> np.ndarray:
  o = acc.shape[1]
  m, s = OC._tables(multiplier, shift, o)      # pylint: disable=protected-access
  b = [0] * o if bias is None else [int(v) for v in np.asarray(bias).reshape(-1)]
  out = [[min(max(OC.mbqm64(min(max(a + b[r], OC.A16_MIN), OC.A16_MAX), m[r], s[r]), act_min), act_max)
          for r, a in enumerate(row)] for row in acc.tolist()]
  return np.array(out, np.int64).reshape(acc.shape).astype(np.int16)


# ---------------------------------------------------------------- DepthwiseConv2DOptions as the flatbuffer layer keeps it
def depthwise_options_table(padding=None, stride_w=None, stride_h=None, depth_multiplier=None, fused=None, dilation_w=None,
                            dilation_h=None):
  """An OpaqueTableT laid out as a flatbuffer writer lays DepthwiseConv2DOptions out (field ids 0 .. 6: padding i8,
  stride_w i32, stride_h i32, depth_multiplier i32, fused_activation_function i8, dilation_w_factor i32,
  dilation_h_factor i32). A field given as None is ABSENT, as a writer leaves out a field at its default."""
  from mi355q.utils import tflite_flatbuffer as fb
  inline = bytearray(4)      # (the vtable reference)
  fields = ((padding, "<b"), (stride_w, "<i"), (stride_h, "<i"), (depth_multiplier, "<i"), (fused, "<b"), (dilation_w, "<i"),
            (dilation_h, "<i"))
  offsets = [0] * 7
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
# (name, input channels, depth multiplier, kernel, strides, dilations, padding, has bias, fused)
DWS = (("dwA", 16, 1, (3, 3), (1, 1), (1, 1), SAME, True, OC.RELU),
       ("dwB", 3, 2, (5, 5), (2, 2), (1, 1), VALID, False, OC.NONE),
       ("dwC", 8, 1, (3, 3), (1, 1), (2, 2), SAME, True, OC.RELU6))
FC = CC.FC
BATCH, HEIGHT, WIDTH = CC.BATCH, CC.HEIGHT, CC.WIDTH
SAMPLES = 3
DEPTHWISE_CONV_2D = 4


def build_model():
  """ModelT tree: three DEPTHWISE_CONV_2D ops `<op>/x` [2, 9, 11, C] -> `<op>/y` and one FULLY_CONNECTED, each with
  its own input. DepthwiseConv2DOptions is an OpaqueTableT, what the reader makes of a file, with absent defaults:
  dwA leaves padding (SAME = 0) and the dilations absent, dwB the fused activation and the dilations; dwA writes its
  depth_multiplier, dwC leaves it absent (0: the shapes say it)."""
  from mi355q import qtyping as q
  model = q.ModelT(version=3, description=b"three DEPTHWISE_CONV_2D ops and one FULLY_CONNECTED (synthetic)")
  model.buffers = [q.BufferT()]
  sg = q.SubGraphT(name=b"main", tensors=[], operators=[], inputs=[], outputs=[])
  rng = np.random.default_rng(311)

  def tensor(name, shape, data=None):
    buffer = 0
    if data is not None:
      model.buffers.append(q.BufferT(data=np.ascontiguousarray(data, np.float32).reshape(-1).view(np.uint8)))
      buffer = len(model.buffers) - 1
    sg.tensors.append(q.TensorT(name=name.encode(), shape=list(shape), buffer=buffer))
    return len(sg.tensors) - 1
  for name, c, mult, k, s, dil, padding, has_bias, fused in DWS:
    o = c * mult
    oh, ow, _, _ = CC.geometry(HEIGHT, WIDTH, k[0], k[1], s, dil, padding)
    x = tensor(f"{name}/x", [BATCH, HEIGHT, WIDTH, c])
    scale = np.float32(1.2 / np.sqrt(k[0] * k[1]))
    # (per-channel gains spread over a decade: what makes per-channel scales matter for a depthwise filter)
    gain = np.exp(rng.uniform(-1.2, 1.2, size=o)).astype(np.float32)
    w = tensor(f"{name}/w", [1, k[0], k[1], o], rng.standard_normal((1, k[0], k[1], o), dtype=np.float32) * scale * gain)
    b = tensor(f"{name}/b", [o], rng.standard_normal(o, dtype=np.float32) * np.float32(1.5)) if has_bias else -1
    y = tensor(f"{name}/y", [BATCH, oh, ow, o])
    sg.inputs.append(x)
    sg.outputs.append(y)
    table = depthwise_options_table(CC.PADDING_CODE[padding] or None, s[1], s[0], None if name == "dwC" else mult,
                                    fused or None, None if dil == (1, 1) else dil[1], None if dil == (1, 1) else dil[0])
    sg.operators.append(q.OperatorT(inputs=[x, w, b] if has_bias else [x, w], outputs=[y], opcodeIndex=0,
                                    builtinOptionsType=2, builtinOptions=table))
  name, d, rows = FC
  x = tensor(f"{name}/x", [1, d])
  w = tensor(f"{name}/w", [rows, d], rng.standard_normal((rows, d), dtype=np.float32) * np.float32(0.3))
  b = tensor(f"{name}/b", [rows], rng.standard_normal(rows, dtype=np.float32))
  y = tensor(f"{name}/y", [1, rows])
  sg.inputs.append(x)
  sg.outputs.append(y)
  sg.operators.append(q.OperatorT(inputs=[x, w, b], outputs=[y], opcodeIndex=1, builtinOptionsType=8,
                                  builtinOptions=q.FullyConnectedOptionsT(fusedActivationFunction=OC.NONE)))
  model.operatorCodes = [q.OperatorCodeT(builtinCode=DEPTHWISE_CONV_2D, deprecatedBuiltinCode=DEPTHWISE_CONV_2D),
                         q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.FULLY_CONNECTED), deprecatedBuiltinCode=9)]
  model.subgraphs = [sg]
  model.signatureDefs = [q.SignatureDefT(signatureKey=b"serving_default", subgraphIndex=0)]
  return model


constant = CC.constant


def float_op(model, dw, x, pre_bias=False) -> np.ndarray:
  """float32 [N OH OW, O]: act(depthwise(x) + b) of the float op, the product by the statement; `pre_bias`: it alone."""
  name, c, mult, k, s, dil, padding, has_bias, fused = dw
  y = float_depthwise(x, constant(model, f"{name}/w")[0], mult, s, dil, padding)
  if pre_bias:
    return y
  if has_bias:
    y = y + constant(model, f"{name}/b")
  return OC.float_activation(y, fused)


def build_samples(model):
  """[{tensor name: float32 array}]: inputs ~ N(0, 1) and the float model's own outputs (NumPy)."""
  rng = np.random.default_rng(312)
  samples = []
  for _ in range(SAMPLES):
    s = {}
    for dw in DWS:
      name, c, mult, k, st, dil, padding = dw[:7]
      oh, ow, _, _ = CC.geometry(HEIGHT, WIDTH, k[0], k[1], st, dil, padding)
      x = rng.standard_normal((BATCH, HEIGHT, WIDTH, c), dtype=np.float32)
      s[f"{name}/x"] = x
      s[f"{name}/y"] = float_op(model, dw, x).reshape(BATCH, oh, ow, c * mult)
    name, d, rows = FC
    x = rng.standard_normal((1, 7, d), dtype=np.float32)
    s[f"{name}/x"] = x
    s[f"{name}/y"] = (x.reshape(-1, d) @ constant(model, f"{name}/w").T + constant(model, f"{name}/b")).reshape(1, 7, rows)
    samples.append(s)
  return samples


def output_rows(dw) -> int:
  k, st, dil, padding = dw[3:7]
  oh, ow, _, _ = CC.geometry(HEIGHT, WIDTH, k[0], k[1], st, dil, padding)
  return BATCH * oh * ow


# ---------------------------------------------------------------- the model quantized by hand (no device)
def quantize_by_hand(model, samples, mode="static", bits=8):
  """`mode` "static": activations INT8 / INT16 with (s, zp) from the samples' range, depthwise filters per-channel
  symmetric int8 ALONG DIMENSION 3 (the FULLY_CONNECTED weight along 0), biases INT32 / INT64 on the grid s_x s_w.
  "dynamic": the integer filters alone. "weight_only": as dynamic, with a DEQUANTIZE op in front of every op."""
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
  ops_of = [(d[0], d[1] * d[2], d[7], 3) for d in DWS] + [(FC[0], FC[2], True, 0)]
  for name, rows, has_bias, axis in ops_of:
    w = constant(model, f"{name}/w")
    t = by_name[f"{name}/w"]
    flat = w.reshape(-1, rows) if axis == 3 else w.reshape(rows, -1).T      # [reduction, channel]
    s_w = (np.abs(flat).max(axis=0) / 127.0).astype(np.float32)
    ints = np.clip(np.rint(flat / s_w[None, :]), -127, 127).astype(np.int8)
    t.type = int(q.TensorType.INT8)
    t.quantization = q.QuantizationParametersT(scale=s_w, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=axis)
    tgt.buffers[t.buffer].data = np.ascontiguousarray(ints if axis == 3 else ints.T).reshape(-1).view(np.uint8)
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
      values = np.rint(constant(model, f"{name}/b").astype(np.float64) / s_b.astype(np.float64))
      b.type = int(q.TensorType.INT64 if bits == 16 else q.TensorType.INT32)
      b.quantization = q.QuantizationParametersT(scale=s_b, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=0)
      tgt.buffers[b.buffer].data = values.astype(np.int64 if bits == 16 else np.int32).view(np.uint8)
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
  """conv_execution_cases.numpy_kernels() with the five methods of `depthwise_conv_2d`: the float statement, and the
  direct integer convolution followed by the rescales and epilogues above."""
  class NumpyDepthwiseKernels(CC.numpy_kernels(**kwargs)):
    @staticmethod
    def _integers(target, kernel, x, multiplier):
      o = x.shape[3] * multiplier
      return EC.plan_integers(target, kernel[0] * kernel[1], o).reshape(kernel[0], kernel[1], o)

    def depthwise_float(self, x, w, kernel, depth_multiplier, strides, dilations, padding, first, count):
      w = np.asarray(w, np.float32).reshape(kernel[0], kernel[1], -1)
      return float_depthwise(x, w, depth_multiplier, strides, dilations, padding, first, count)

    def depthwise_forward(self, xq, x_scale, x_zero_point, target, kernel, depth_multiplier, strides, dilations, padding,
                          first, count):
      acc = direct_depthwise(xq, x_zero_point, self._integers(target, kernel, xq, depth_multiplier), depth_multiplier,
                             strides, dilations, padding)
      return rescale_i8(acc, x_scale, target.scale, xq.shape[0])[first:first + count]

    def depthwise_forward16(self, xq, x_scale, target, kernel, depth_multiplier, strides, dilations, padding, first, count):
      acc = direct_depthwise(xq, 0, self._integers(target, kernel, xq, depth_multiplier), depth_multiplier, strides,
                             dilations, padding)
      return rescale_i16(acc, x_scale, target.scale, xq.shape[0])[first:first + count]

    def depthwise_output(self, xq, x_zero_point, target, kernel, depth_multiplier, strides, dilations, padding, bias,
                         multiplier, shift, out_zero_point, act_min, act_max, first, count):
      acc = direct_depthwise(xq, x_zero_point, self._integers(target, kernel, xq, depth_multiplier), depth_multiplier,
                             strides, dilations, padding)[first:first + count]
      return epilogue_i8(acc, bias, multiplier, shift, out_zero_point, act_min, act_max)

    def depthwise_output16(self, xq, target, kernel, depth_multiplier, strides, dilations, padding, bias, multiplier, shift,
                           act_min, act_max, first, count):
      acc = direct_depthwise(xq, 0, self._integers(target, kernel, xq, depth_multiplier), depth_multiplier, strides,
                             dilations, padding)[first:first + count]
      return epilogue_i16(acc, bias, multiplier, shift, act_min, act_max)
  return NumpyDepthwiseKernels


# ---------------------------------------------------------------- what the five entries refuse before a launch
ENTRIES = ("mi355q_dwconv_forward_f32", "mi355q_dwconv_forward_i8", "mi355q_dwconv_forward_i16", "mi355q_dwconv_output_i8",
           "mi355q_dwconv_output_i16")
ARGUMENT_COUNTS = {"mi355q_dwconv_forward_f32": 21, "mi355q_dwconv_forward_i8": 28, "mi355q_dwconv_forward_i16": 27,
                   "mi355q_dwconv_output_i8": 30, "mi355q_dwconv_output_i16": 28}
I8 = 3      # MI355Q_CMP_I8 (checked against ops.COMPARE_KINDS by the host test)


def check_depthwise_refusals(lib) -> None:
  """Every refusal of include/mi355q.h with its status code and text, for each of the five entries. Host buffers stand
  in for device pointers: each call returns before it launches (the last ones enqueue nothing)."""
  import ctypes
  buf = ctypes.create_string_buffer(4096)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error
  geo = ("sh", "sw", "dh", "dw", "top", "left", "OH", "OW", "first", "count")

  def call(entry, **kw):
    a = dict(x=p, N=2, H=5, W=7, C=16, xs=p, xsc=1, zp=0, w=p, kind=I8, KH=3, KW=3, M=1, ws=p, wsc=1, bias=p, mult=p, shift=p,
             mcount=1, ozp=0, amin=-128, amax=127, sh=1, sw=1, dh=1, dw=1, top=1, left=1, OH=5, OW=7, first=0, count=1, y=p,
             acc=None, q=p)
    a.update(kw)
    order = {"mi355q_dwconv_forward_f32": ("x", "N", "H", "W", "C", "w", "KH", "KW", "M") + geo + ("y",),
             "mi355q_dwconv_forward_i8": ("x", "N", "H", "W", "C", "xs", "xsc", "zp", "w", "kind", "KH", "KW", "M", "ws", "wsc")
                                         + geo + ("y", "acc"),
             "mi355q_dwconv_forward_i16": ("x", "N", "H", "W", "C", "xs", "xsc", "w", "kind", "KH", "KW", "M", "ws", "wsc")
                                          + geo + ("y", "acc"),
             "mi355q_dwconv_output_i8": ("x", "N", "H", "W", "C", "zp", "w", "kind", "KH", "KW", "M", "bias", "mult", "shift",
                                         "mcount", "ozp", "amin", "amax") + geo + ("q",),
             "mi355q_dwconv_output_i16": ("x", "N", "H", "W", "C", "w", "kind", "KH", "KW", "M", "bias", "mult", "shift",
                                          "mcount", "amin", "amax") + geo + ("q",)}[entry]
    assert len(order) + 1 == ARGUMENT_COUNTS[entry]
    return getattr(lib, entry)(*[a[k] for k in order], None)

  for entry in ENTRIES:
    forward, integer, sixteen = "forward" in entry, "f32" not in entry, "i16" in entry
    nulls = {"mi355q_dwconv_forward_f32": ("x", "w", "y"), "mi355q_dwconv_forward_i8": ("x", "xs", "w", "ws", "y"),
             "mi355q_dwconv_forward_i16": ("x", "xs", "w", "ws", "y"), "mi355q_dwconv_output_i8": ("x", "w", "mult", "shift", "q"),
             "mi355q_dwconv_output_i16": ("x", "w", "mult", "shift", "q")}[entry]
    for null in nulls:
      assert call(entry, **{null: None}) == -1 and b"null pointer" in err(), (entry, null)
    for dim in ("N", "H", "W", "C", "KH", "KW", "OH", "OW"):
      for bad in (0, -1):
        assert call(entry, **{dim: bad}) == -1 and b"every dimension must be positive" in err(), (entry, dim)
    for bad in (0, -3):
      assert call(entry, M=bad) == -1 and b"depth multiplier must be positive" in err(), entry
    for stride in ("sh", "sw"):
      for bad in (0, -2):
        assert call(entry, **{stride: bad}) == -1 and b"strides must be positive" in err(), (entry, stride)
    for dil in ("dh", "dw"):
      for bad in (0, -2):
        assert call(entry, **{dil: bad}) == -1 and b"dilations must be positive" in err(), (entry, dil)
    assert call(entry, first=-1) == -1 and call(entry, count=-1) == -1 and b"negative row window" in err()
    assert call(entry, KH=257, KW=256) == -3 and b"exceeds 65536 taps" in err()
    assert call(entry, KH=1 << 20, KW=1 << 20) == -3 and b"exceeds 65536 taps" in err()
    assert call(entry, OH=1 << 16, OW=1 << 15, N=1) == -3 and b"exceeds INT32_MAX output rows" in err()
    assert call(entry, OH=1 << 15, OW=1 << 15, N=2) == -3 and b"exceeds INT32_MAX output rows" in err()
    assert call(entry, OH=1 << 40) == -3 and b"exceeds INT32_MAX output rows" in err()
    for first, count in ((70, 1), (0, 71), (69, 2)):
      assert call(entry, first=first, count=count) == -1 and b"outside the 70 output rows" in err(), entry
    assert call(entry, N=1 << 30, H=1 << 31, W=1 << 31, C=65536, OH=1, OW=1, count=0) == -3 and b"2^62 bytes" in err()
    assert call(entry, C=1 << 61, N=1, H=1, W=1, OH=1, OW=1, count=0) == -3 and b"2^62 bytes" in err()
    assert call(entry, C=1 << 20, M=1 << 12, count=0) == -3 and b"exceeds INT32_MAX output channels" in err()
    if integer:
      for kind in (0, 4, 6, 7, -1):      # (float32, int16, int4, int2, nothing: a depthwise filter is int8)
        assert call(entry, kind=kind) == -1 and b"is not I8" in err(), (entry, kind)
    if integer and forward:
      for bad in (0, 3, 16):
        assert call(entry, xsc=bad) == -1 and b"x_scale_count must be 1 or N = 2" in err(), (entry, bad)
      for bad in (0, 2, 15, 32):
        assert call(entry, wsc=bad) == -1 and b"w_scale_count must be 1 or O = 16" in err(), (entry, bad)
      assert call(entry, C=3, M=2, wsc=3) == -1 and b"w_scale_count must be 1 or O = 6" in err()
      assert call(entry, xsc=2, wsc=16, count=0) == 0 and err() == b""
    if integer and not forward:
      for bad in (0, 2, 15, 32):
        assert call(entry, mcount=bad) == -1 and b"mcount must be 1 or O = 16" in err(), (entry, bad)
      lo, hi, name = (-32768, 32767, b"int16") if sixteen else (-128, 127, b"int8")
      for amin, amax in ((1, 0), (lo - 1, 0), (0, hi + 1)):
        assert call(entry, amin=amin, amax=amax) == -1 and b"is no range within " + name in err(), (entry, amin, amax)
      assert call(entry, amin=lo, amax=hi, mcount=16, count=0) == 0 and call(entry, amin=3, amax=3, count=0) == 0
    if entry.endswith("_i8"):
      for bad in (-129, 128):
        assert call(entry, zp=bad) == -1 and b"activation zero point" in err() and b"outside int8" in err(), (entry, bad)
    if entry == "mi355q_dwconv_output_i8":
      for bad in (-129, 128):
        assert call(entry, ozp=bad) == -1 and b"output zero point" in err() and b"outside int8" in err(), bad
    # after those, an empty window enqueues nothing, whatever the pointers
    assert call(entry, count=0) == 0 and err() == b""
    everything = {k: None for k in ("x", "xs", "w", "ws", "bias", "mult", "shift", "y", "acc", "q")}
    assert call(entry, first=70, count=0, **everything) == 0 and err() == b""
    assert call(entry, KH=256, KW=256, count=0) == 0 and err() == b""
