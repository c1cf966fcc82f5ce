"""Shared by test_tconv_execution_host.py and test_gpu_tconv_execution.py: the NumPy statement of the TRANSPOSE_CONV
phase gather (include/mi355q.h, "Patch gather for TRANSPOSE_CONV"), element by element; an INDEPENDENT transposed
convolution in its scatter form (out[a sh - pad + ky] += x[a] w[ky]) that never forms patches or phases; the geometry
list; a hand-built float model of three TRANSPOSE_CONV ops and one FULLY_CONNECTED with its samples, a hand-quantized
form of it for the host tests; and NumPy stand-ins for the LayerExecutionKernels methods of `transpose_conv`."""
import copy
import itertools

import numpy as np

import conv_execution_cases as CC
import layer_output_cases as OC

SAME, VALID = CC.SAME, CC.VALID


# ---------------------------------------------------------------- geometry, written out once more
def geometry(ih, iw, kh, kw, strides, padding, out_hw):
  """(pad_top, pad_left) of the forward convolution from `out_hw` back to ih x iw (TFLite's rule, no dilation), or
  None when that convolution does not give ih x iw."""
  back = CC.geometry(out_hw[0], out_hw[1], kh, kw, strides, (1, 1), padding)
  if back is None or back[:2] != (ih, iw):
    return None
  return back[2], back[3]


def output_sizes(ih, iw, kernel, strides, padding):
  """Every (OH, OW) whose forward geometry gives the image back."""
  def axis(size, k, s):
    return [o for o in range(1, (size + 1) * s + k + 1)
            if (lambda g: g is not None and g[0] == size)(CC.geometry(o, 1, k, 1, (s, 1), (1, 1), padding))]
  return list(itertools.product(axis(ih, kernel[0], strides[0]), axis(iw, kernel[1], strides[1])))


def phases(ih, iw, kh, kw, strides, padding, out_hw):
  """[(py, px, QH, QW, kys, kxs)] of every phase with output pixels, from the definition: the taps of a pixel
  (oy, ox) are those with (oy + pad - k) % s == 0."""
  top, left = geometry(ih, iw, kh, kw, strides, padding, out_hw)
  out = []
  for py in range(strides[0]):
    for px in range(strides[1]):
      oys, oxs = range(py, out_hw[0], strides[0]), range(px, out_hw[1], strides[1])
      if len(oys) and len(oxs):
        out.append((py, px, len(oys), len(oxs), tuple(ky for ky in range(kh) if (py + top - ky) % strides[0] == 0),
                    tuple(kx for kx in range(kw) if (px + left - kx) % strides[1] == 0)))
  return out


def has_empty_phase(ih, iw, kernel, strides, padding, out_hw) -> bool:
  return any(not kys or not kxs for *_, kys, kxs in phases(ih, iw, kernel[0], kernel[1], strides, padding, out_hw))


# ---------------------------------------------------------------- the gather
def gather(x: np.ndarray, kh, kw, strides, padding, out_hw, phase, pad, first=0, count=None) -> np.ndarray:
  """The statement, element by element over (row, tap): rows first .. first + count - 1 of the
  [N QH QW, |kys| |kxs| C] patch rows of `phase` of x [N, IH, IW, C]; a tap outside the image holds `pad` (one element
  of x's dtype, copied as bytes)."""
  n_img, ih, iw, c = x.shape
  top, left = geometry(ih, iw, kh, kw, strides, padding, out_hw)
  py, px = phase
  qh_n, qw_n, kys, kxs = next(p[2:] for p in phases(ih, iw, kh, kw, strides, padding, out_hw) if p[:2] == (py, px))
  assert kys and kxs
  total = n_img * qh_n * qw_n
  count = total - first if count is None else count
  assert 0 <= first and first + count <= total
  k = len(kys) * len(kxs) * c
  pad = np.asarray(pad, x.dtype).reshape(())
  out = np.empty((count, k), x.dtype)
  out.view(np.uint8).reshape(-1)[:] = np.tile(np.frombuffer(pad.tobytes(), np.uint8), count * k)
  for r in range(count):
    t = first + r
    n, qy, qx = t // (qh_n * qw_n), (t // qw_n) % qh_n, t % qw_n
    for ti, ky in enumerate(kys):
      assert (qy * strides[0] + py + top - ky) % strides[0] == 0
      a = (qy * strides[0] + py + top - ky) // strides[0]
      if not 0 <= a < ih:
        continue
      for tj, kx in enumerate(kxs):
        b = (qx * strides[1] + px + left - kx) // strides[1]
        if 0 <= b < iw:
          out[r, (ti * len(kxs) + tj) * c:(ti * len(kxs) + tj + 1) * c] = x[n, a, b]
  return out


def scatter_tconv(x: np.ndarray, w: np.ndarray, strides, padding, out_hw) -> np.ndarray:
  """[N, OH, OW, O] in the dtype of `x` (int64 or float64): every input pixel (a, b) ADDS x[n, a, b, :] . w[o, ky, kx, :]
  to the output pixel (a sh - pad_top + ky, b sw - pad_left + kx) when that lies inside the output. The definition of
  a transposed convolution; no patches, no phases."""
  n_img, ih, iw, c = x.shape
  o_n, kh, kw, _ = w.shape
  top, left = geometry(ih, iw, kh, kw, strides, padding, out_hw)
  out = np.zeros((n_img, out_hw[0], out_hw[1], o_n), x.dtype)
  for a in range(ih):
    for ky in range(kh):
      oy = a * strides[0] - top + ky
      if not 0 <= oy < out_hw[0]:
        continue
      for b in range(iw):
        for kx in range(kw):
          ox = b * strides[1] - left + kx
          if 0 <= ox < out_hw[1]:
            out[:, oy, ox, :] += np.einsum("nc,oc->no", x[:, a, b, :], w[:, ky, kx, :].astype(x.dtype))
  return out


def integer_tconv(xq: np.ndarray, zero_point: int, qw: np.ndarray, strides, padding, out_hw) -> np.ndarray:
  """int64 [N, OH, OW, O]: the scatter form on (xq - zero_point) and the integer filter."""
  xi, wi = xq.astype(np.int64) - int(zero_point), qw.astype(np.int64)
  assert qw.shape[1] * qw.shape[2] * qw.shape[3] * int(np.abs(xi).max(initial=0)) * int(np.abs(wi).max(initial=0)) < 1 << 62
  return scatter_tconv(xi, wi, strides, padding, out_hw)


def interleave(parts, n_img, out_hw, strides, o) -> np.ndarray:
  """[N, OH, OW, O] of the per-phase results [(py, px, [N QH QW, O])]."""
  out = np.zeros((n_img, out_hw[0], out_hw[1], o), parts[0][2].dtype)
  for py, px, y in parts:
    view = out[:, py::strides[0], px::strides[1], :]
    view[...] = y.reshape(view.shape)
  return out


def filter_slice(w: np.ndarray, kys, kxs) -> np.ndarray:
  """W[:, kys][:, :, kxs] viewed [O, |kys| |kxs| C]."""
  return np.ascontiguousarray(w[:, list(kys)][:, :, list(kxs)]).reshape(w.shape[0], -1)


# ---------------------------------------------------------------- the geometries
IMAGES = ((1, 1), (3, 4), (5, 2))
KERNELS = ((1, 1), (3, 3), (2, 5), (4, 4))
STRIDES = ((1, 1), (2, 2), (2, 1), (3, 2))


def all_geometries():
  """(N, IH, IW, kernel, strides, padding, out_hw) over the cross, every output size that maps back to the image."""
  out = []
  for (ih, iw), k, s, padding in itertools.product(IMAGES, KERNELS, STRIDES, (SAME, VALID)):
    for out_hw in output_sizes(ih, iw, k, s, padding):
      out.append((1 + len(out) % 2, ih, iw, k, s, padding, out_hw))
  return out


def geometries():
  """all_geometries() without those that have a phase with no tap (a stride above the kernel): refusal cases."""
  return [g for g in all_geometries() if not has_empty_phase(*g[1:])]


def windows(total: int, per_image: int):
  return CC.windows(total, per_image)


# ---------------------------------------------------------------- the model
# (name, input channels, output channels, kernel, strides, padding, has bias, fused, output size)
HEIGHT, WIDTH, BATCH, SAMPLES = 5, 6, 2, 3
TCONVS = (("tcA", 16, 24, (4, 4), (2, 2), SAME, True, OC.NONE, (9, 12)),
          ("tcB", 3, 8, (3, 3), (2, 2), VALID, False, OC.RELU, (11, 14)),
          ("tcC", 16, 16, (2, 5), (2, 1), SAME, True, OC.RELU6, (9, 6)))      # rows: total padding 2 * 5 - 9 = 1, odd
FC = ("fc", 32, 12)      # (name, d, rows): bias, no activation
PADDING_CODE = CC.PADDING_CODE
TRANSPOSE_CONV, TRANSPOSE_CONV_OPTIONS = 67, 49


def tconv_options_table(padding=None, stride_w=None, stride_h=None, fused=None):
  """An OpaqueTableT laid out as a flatbuffer writer lays TransposeConvOptions out: field ids 0 .. 3 (padding i8,
  stride_w i32, stride_h i32, fused_activation_function i8), the first four of Conv2DOptions. None: ABSENT."""
  return CC.conv_options_table(padding, stride_w, stride_h, fused)


def build_model():
  """ModelT tree: three TRANSPOSE_CONV ops (output_shape, `<op>/w`, `<op>/x` [2, 5, 6, C], `<op>/b`) -> `<op>/y` and one
  FULLY_CONNECTED, each with its own input. TransposeConvOptions is an OpaqueTableT, what the reader makes of a file."""
  from mi355q import qtyping as q
  model = q.ModelT(version=3, description=b"three TRANSPOSE_CONV ops and one FULLY_CONNECTED (synthetic)")
  model.buffers = [q.BufferT()]
  sg = q.SubGraphT(name=b"main", tensors=[], operators=[], inputs=[], outputs=[])
  rng = np.random.default_rng(311)

  def tensor(name, shape, data=None, dtype=np.float32, ttype=None):
    buffer = 0
    if data is not None:
      model.buffers.append(q.BufferT(data=np.ascontiguousarray(data, dtype).reshape(-1).view(np.uint8)))
      buffer = len(model.buffers) - 1
    t = q.TensorT(name=name.encode(), shape=list(shape), buffer=buffer)
    if ttype is not None:
      t.type = int(ttype)
    sg.tensors.append(t)
    return len(sg.tensors) - 1
  for name, c, o, k, s, padding, has_bias, fused, out_hw in TCONVS:
    assert geometry(HEIGHT, WIDTH, k[0], k[1], s, padding, out_hw) is not None
    shape = tensor(f"{name}/output_shape", [4], [BATCH, out_hw[0], out_hw[1], o], np.int32, q.TensorType.INT32)
    x = tensor(f"{name}/x", [BATCH, HEIGHT, WIDTH, c])
    taps = -(-k[0] // s[0]) * -(-k[1] // s[1])
    scale = np.float32(1.2 / np.sqrt(taps * c))
    w = tensor(f"{name}/w", [o, k[0], k[1], c], rng.standard_normal((o, k[0], k[1], c), dtype=np.float32) * scale)
    b = tensor(f"{name}/b", [o], rng.standard_normal(o, dtype=np.float32) * np.float32(1.5)) if has_bias else -1
    y = tensor(f"{name}/y", [BATCH, out_hw[0], out_hw[1], o])
    sg.inputs.append(x)
    sg.outputs.append(y)
    table = tconv_options_table(PADDING_CODE[padding] or None, s[1], s[0], fused or None)
    sg.operators.append(q.OperatorT(inputs=[shape, w, x, b] if has_bias else [shape, w, x], outputs=[y], opcodeIndex=0,
                                    builtinOptionsType=TRANSPOSE_CONV_OPTIONS, builtinOptions=table))
  name, d, rows = FC
  x = tensor(f"{name}/x", [1, d])
  w = tensor(f"{name}/w", [rows, d], rng.standard_normal((rows, d), dtype=np.float32) * np.float32(0.3))
  b = tensor(f"{name}/b", [rows], rng.standard_normal(rows, dtype=np.float32))
  y = tensor(f"{name}/y", [1, rows])
  sg.inputs.append(x)
  sg.outputs.append(y)
  sg.operators.append(q.OperatorT(inputs=[x, w, b], outputs=[y], opcodeIndex=1, builtinOptionsType=8,
                                  builtinOptions=q.FullyConnectedOptionsT(fusedActivationFunction=OC.NONE)))
  model.operatorCodes = [q.OperatorCodeT(builtinCode=TRANSPOSE_CONV, deprecatedBuiltinCode=TRANSPOSE_CONV),
                         q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.FULLY_CONNECTED), deprecatedBuiltinCode=9)]
  model.subgraphs = [sg]
  model.signatureDefs = [q.SignatureDefT(signatureKey=b"serving_default", subgraphIndex=0)]
  return model


constant = CC.constant


def float_tconv(model, tconv, x, dtype=np.float64, pre_bias=False) -> np.ndarray:
  """act(tconv(x, W) + b) [N, OH, OW, O] of the float op. float64: the scatter form. float32: by phases, each the
  float32 product of its patch rows (pad 0.0) and its filter slice, which is how the validator forms Y."""
  name, c, o, k, s, padding, has_bias, fused, out_hw = tconv
  w = constant(model, f"{name}/w")
  x = np.asarray(x, np.float32)
  if dtype == np.float64:
    y = scatter_tconv(x.astype(np.float64), w.astype(np.float64), s, padding, out_hw)
  else:
    parts = [(py, px, gather(x, k[0], k[1], s, padding, out_hw, (py, px), 0.0) @ filter_slice(w, kys, kxs).T)
             for py, px, _, _, kys, kxs in phases(x.shape[1], x.shape[2], k[0], k[1], s, padding, out_hw)]
    y = interleave(parts, x.shape[0], out_hw, s, o)
  if pre_bias:
    return y
  if has_bias:
    y = y + constant(model, f"{name}/b").astype(dtype)
  return OC.float_activation(y, fused)


def build_samples(model):
  """[{tensor name: float32 array}]: inputs ~ N(0, 1) and the float model's own outputs (NumPy), so that calibration
  yields meaningful (s_y, zp_y)."""
  rng = np.random.default_rng(312)
  samples = []
  for _ in range(SAMPLES):
    s = {}
    for tconv in TCONVS:
      name, c = tconv[:2]
      x = rng.standard_normal((BATCH, HEIGHT, WIDTH, c), dtype=np.float32)
      s[f"{name}/x"] = x
      s[f"{name}/y"] = float_tconv(model, tconv, x, np.float32)
    name, d, rows = FC
    x = rng.standard_normal((1, 7, d), dtype=np.float32)
    s[f"{name}/x"] = x
    s[f"{name}/y"] = (x.reshape(-1, d) @ constant(model, f"{name}/w").T + constant(model, f"{name}/b")).reshape(1, 7, rows)
    samples.append(s)
  return samples


# ---------------------------------------------------------------- the model quantized by hand (host tests: no device)
def quantize_by_hand(model, samples, mode="static", bits=8):
  """conv_execution_cases.quantize_by_hand for this model: `mode` "static": activations INT8 / INT16 with (s, zp) from
  the samples' range, filters per-channel symmetric int8 along dimension 0, biases INT32 / INT64 on the grid s_x s_w.
  "dynamic": the integer filters alone. "weight_only": as dynamic, with a DEQUANTIZE op in front of every filter."""
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
  for name, rows, has_bias in [(c[0], c[2], c[6]) for c in TCONVS] + [(FC[0], FC[2], True)]:
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
    for op in sg.operators:      # (the filter is input 1 of both op kinds)
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
  """conv_execution_cases.numpy_kernels() with the two methods of `transpose_conv`."""
  class NumpyTconvKernels(CC.numpy_kernels(**kwargs)):
    def tconv_patches(self, x, kernel, strides, padding, out_hw, phase, pad_value, first, count):
      return gather(np.asarray(x), kernel[0], kernel[1], strides, padding, out_hw, phase, pad_value, first, count)

    def image_scales(self, scale, rows_per_image, first, count):
      return np.asarray(scale, np.float32)[np.arange(first, first + count) // rows_per_image]
  return NumpyTconvKernels


# ---------------------------------------------------------------- what mi355q_tconv_patches_nhwc refuses before a launch
def check_patch_refusals(lib) -> None:
  """Every refusal of include/mi355q.h with its status code. Host buffers stand in for device pointers: each call
  returns before it launches (the last ones enqueue nothing). The base call is 4x4 stride 2 SAME, 5 x 7 -> 10 x 14."""
  import ctypes
  buf = ctypes.create_string_buffer(4096)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error

  def call(x=p, eb=1, N=2, IH=5, IW=7, C=16, KH=4, KW=4, sh=2, sw=2, top=1, left=1, OH=10, OW=14, py=0, px=0, first=0,
           count=1, pad=p, out=p):
    return lib.mi355q_tconv_patches_nhwc(x, eb, N, IH, IW, C, KH, KW, sh, sw, top, left, OH, OW, py, px, first, count, pad,
                                         out, None)
  for null in ("x", "out", "pad"):
    assert call(**{null: None}) == -1 and b"null pointer" in err(), null
  for eb in (0, 3, 8, -1):
    assert call(eb=eb) == -1 and b"elem_bytes must be 1, 2 or 4" in err(), eb
  for dim in ("N", "IH", "IW", "C", "KH", "KW", "OH", "OW"):
    for bad in (0, -1):
      assert call(**{dim: bad}) == -1 and b"every dimension must be positive" in err(), dim
  for stride in ("sh", "sw"):
    for bad in (0, -2):
      assert call(**{stride: bad}) == -1 and b"strides must be positive" in err(), stride
  for phase in (dict(py=2), dict(px=2), dict(py=-1), dict(px=-1), dict(sh=1, OH=5, top=1, KH=3, py=1)):
    assert call(**phase) == -1 and b"outside the strides" in err(), phase
  assert call(first=-1) == -1 and call(count=-1) == -1 and b"negative row window" in err()
  assert call(OH=1 << 40) == -3 and b"exceeds INT32_MAX" in err()
  assert call(N=1 << 31) == -3 and b"exceeds INT32_MAX" in err()
  # a geometry whose forward convolution does not give the image back: the sizes, then each padding
  for geo in (dict(OH=11), dict(OW=12), dict(IH=6), dict(top=0), dict(left=2), dict(top=-1), dict(KH=6), dict(sw=3, px=0)):
    assert call(**geo) == -1 and b"does not map the output" in err(), geo
  # a stride above the kernel leaves phases without a tap: 1x1 stride 2 VALID, 5 x 7 -> 9 x 13 (or 10 x 14)
  assert call(KH=1, KW=1, top=0, left=0, OH=9, OW=13, py=1) == -3 and b"has no tap" in err()
  assert call(KH=1, KW=1, top=0, left=0, OH=9, OW=13, px=1) == -3 and b"has no tap" in err()
  assert call(KH=1, KW=1, top=0, left=0, OH=9, OW=13, count=0) == 0 and err() == b""      # (phase (0, 0) has its one tap)
  # the window: phase (0, 0) of the base call has 2 x 5 x 7 = 70 rows; of 5 x 7 -> 9 x 13 phase (1, 1) has 2 x 4 x 6 = 48
  assert call(first=70, count=1) == -1 and b"outside the 70 patch rows" in err()
  assert call(first=0, count=71) == -1 and b"outside the 70 patch rows" in err()
  assert call(first=69, count=2) == -1 and b"outside the 70 patch rows" in err()
  assert call(OH=9, OW=13, py=1, px=1, first=48, count=1) == -1 and b"outside the 48 patch rows" in err()
  assert call(OH=9, OW=13, py=1, px=1, first=47, count=1, x=None) == -1 and b"null pointer" in err()
  # the size limits of the CONV_2D entry, on the phase's own K = |kys| |kxs| C
  assert call(C=65537, KH=1, KW=1, sh=1, sw=1, top=0, left=0, OH=5, OW=7) == -3 and b"exceeds 65536" in err()
  assert call(C=16385) == -3 and b"exceeds 65536" in err()      # (2 x 2 taps per phase)
  assert call(C=16384, count=0) == 0 and err() == b""
  assert call(N=1 << 30, IH=1 << 15, IW=1 << 15, OH=1 << 16, OW=1 << 16, C=16384, count=0) == -3 and b"exceeds INT32_MAX patch rows" in err()
  assert call(N=1, IH=1 << 30, IW=1 << 30, OH=(1 << 30) + 2, OW=(1 << 30) + 2, KH=3, KW=3, sh=1, sw=1, top=0, left=0, C=8,
              eb=4, count=0) == -3 and b"patch rows" in err()
  # after those, an empty window enqueues nothing, whatever the pointers
  assert call(count=0) == 0 and err() == b""
  assert call(first=70, count=0, x=None, out=None, pad=None) == 0 and err() == b""
