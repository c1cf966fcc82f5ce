"""The statement of the integer BATCH_MATMUL execution (include/mi355q.h, "Integer batched matrix product") in NumPy,
the host dispatch restated, and the case list of the device tests.

  acc[b,m,n] = Sum_k (A[b,m,k] - za) (B[b',k,n] - zb)      int64 einsum, asserted to fit int32
  y          = float32(acc) * float32(a_scale[.] * b_scale[n])
  q          = clamp(mbqm32(acc, M[n], s[n]) + zp_y, -128, 127)      layer_output_cases' epilogue, no bias
"""
import numpy as np

import layer_output_cases as OC

MAX_K = 32768
INT32_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- the statement
def operands(a, b, adj_x: bool, adj_y: bool):
  """(A [batch, M, K], B [batch or 1, K, N]) as int64, leading dimensions flattened."""
  a, b = np.asarray(a), np.asarray(b)
  a3 = a.reshape((-1,) + a.shape[-2:]).astype(np.int64)
  b3 = b.reshape((-1,) + b.shape[-2:]).astype(np.int64)
  if adj_x:
    a3 = a3.swapaxes(1, 2)
  if adj_y:
    b3 = b3.swapaxes(1, 2)
  assert a3.shape[2] == b3.shape[1] and b3.shape[0] in (1, a3.shape[0])
  return a3, b3


def accumulators(a, b, adj_x: bool, adj_y: bool, za: int, zb: int) -> np.ndarray:
  """int64 [batch, M, N]; every value asserted to lie within int32."""
  a3, b3 = operands(a, b, adj_x, adj_y)
  acc = np.einsum("bmk,bkn->bmn", a3 - int(za), np.broadcast_to(b3 - int(zb), (a3.shape[0],) + b3.shape[1:]))
  assert np.abs(acc).max(initial=0) <= INT32_MAX
  return acc


def accumulators_loop(a, b, adj_x: bool, adj_y: bool, za: int, zb: int) -> np.ndarray:
  """The same by a triple loop over Python integers and the layouts' own indices (no transposed copy)."""
  a, b = np.asarray(a), np.asarray(b)
  a3, b3 = a.reshape((-1,) + a.shape[-2:]), b.reshape((-1,) + b.shape[-2:])
  batch = a3.shape[0]
  m, k = (a3.shape[2], a3.shape[1]) if adj_x else (a3.shape[1], a3.shape[2])
  n = b3.shape[1] if adj_y else b3.shape[2]
  out = np.zeros((batch, m, n), np.int64)
  for bz in range(batch):
    bb = b3[bz if b3.shape[0] != 1 else 0]
    for i in range(m):
      for j in range(n):
        s = 0
        for kk in range(k):
          av = int(a3[bz, kk, i]) if adj_x else int(a3[bz, i, kk])
          bv = int(bb[j, kk]) if adj_y else int(bb[kk, j])
          s += (av - za) * (bv - zb)
        out[bz, i, j] = s
  return out


def rescale(acc: np.ndarray, a_scale, b_scale) -> np.ndarray:
  """float32 [batch, M, N] = fl(float(acc) * fl(a_scale[.] * b_scale[n])); a_scale 1 or batch M entries, b_scale 1 or N."""
  batch, m, n = acc.shape
  sa = np.asarray(a_scale, np.float32).reshape(-1)
  sb = np.asarray(b_scale, np.float32).reshape(-1)
  assert sa.size in (1, batch * m) and sb.size in (1, n)
  sa = np.broadcast_to(sa.reshape(batch, m, 1) if sa.size == batch * m and sa.size != 1 else sa.reshape(1, 1, 1), acc.shape)
  sb = np.broadcast_to(sb.reshape(1, 1, -1), acc.shape)
  with np.errstate(all="ignore"):
    sc = (sa * sb).astype(np.float32)
    return (acc.astype(np.float32) * sc).astype(np.float32)


def output(acc: np.ndarray, multiplier, shift, out_zero_point: int) -> np.ndarray:
  """int8 [batch, M, N]: the epilogue statement of layer_output_cases without a bias, over the full int8 range."""
  batch, m, n = acc.shape
  mult = [int(v) for v in np.asarray(multiplier).reshape(-1)]
  sh = [int(v) for v in np.asarray(shift).reshape(-1)]
  assert len(mult) == len(sh) and len(mult) in (1, n)
  if len(mult) == 1:
    mult, sh = mult * n, sh * n
  flat = acc.reshape(-1, n).tolist()
  out = [[min(max(OC.mbqm32(OC.sat32(v), mult[j], sh[j]) + int(out_zero_point), -128), 127) for j, v in enumerate(row)]
         for row in flat]
  return np.array(out, np.int64).reshape(acc.shape).astype(np.int8)


# ---------------------------------------------------------------- the host dispatch, restated
def route(m: int, n: int, k: int, adj_x: bool, adj_y: bool, za: int, zb: int, a_misaligned=False, b_misaligned=False):
  """("generic",) or ("mfma", how a reaches the main loop, how b does, whether operand sums are taken): an operand
  that is contiguous along K is read directly, one that is strided along K is transposed by a pre-pass first."""
  mfma = (k > 0 and k % 64 == 0 and not a_misaligned and not b_misaligned and (not adj_x or m % 16 == 0)
          and (adj_y or n % 16 == 0))
  if not mfma:
    return ("generic",)
  return ("mfma", "a_transposed" if adj_x else "a_direct", "b_direct" if adj_y else "b_transposed",
          "sums" if (za != 0 or zb != 0) else "nosums")


ROUTE_ELEMENTS = {"generic", "mfma", "a_transposed", "a_direct", "b_transposed", "b_direct", "sums", "nosums"}
LAYOUTS = ((False, False), (False, True), (True, False), (True, True))
ZERO_POINTS = ((0, 0), (-128, 127), (127, -128), (5, -3))
BATCHES = ((1, 1), (3, 3), (3, 1))      # (batch, b_batch)
# every value of {1, 15, 16, 17, 64, 65, 129} as M and as N: tile (16), wave (64) and workgroup (128) edges
SHAPES = ((1, 1), (15, 17), (16, 16), (17, 15), (64, 65), (65, 64), (129, 129), (16, 129), (129, 16), (64, 64), (1, 64),
          (64, 1), (32, 48))      # (13 shapes: the zero points, taken in turn, meet every shape)
MFMA_K = (64, 128, 192)
GENERIC_K = (1, 63, 65)


class Case:
  def __init__(self, batch, b_batch, m, n, k, adj_x, adj_y, za, zb, a_misaligned=False, b_misaligned=False):
    self.batch, self.b_batch, self.m, self.n, self.k = batch, b_batch, m, n, k
    self.adj_x, self.adj_y, self.za, self.zb = adj_x, adj_y, za, zb
    self.a_misaligned, self.b_misaligned = a_misaligned, b_misaligned

  @property
  def route(self):
    return route(self.m, self.n, self.k, self.adj_x, self.adj_y, self.za, self.zb, self.a_misaligned, self.b_misaligned)

  @property
  def id(self):
    form = "own" if self.b_batch == self.batch else "shared"
    mis = ("-amis" if self.a_misaligned else "") + ("-bmis" if self.b_misaligned else "")
    return (f"{'-'.join(self.route)}-x{int(self.adj_x)}y{int(self.adj_y)}-b{self.batch}{form}-{self.m}x{self.n}x{self.k}"
            f"-za{self.za}zb{self.zb}{mis}")

  def shapes(self):
    a = (self.batch,) + ((self.k, self.m) if self.adj_x else (self.m, self.k))
    b = (self.b_batch,) + ((self.n, self.k) if self.adj_y else (self.k, self.n))
    return a, b

  def build(self, seed: int):
    """Full-range int8 operands with the extremes planted in the corners of every matrix."""
    rng = np.random.default_rng(seed)
    sa, sb = self.shapes()
    a = rng.integers(-128, 127, size=sa, endpoint=True).astype(np.int8)
    b = rng.integers(-128, 127, size=sb, endpoint=True).astype(np.int8)
    for t in (a, b):
      t[:, 0, 0], t[:, -1, -1], t[:, 0, -1], t[:, -1, 0] = -128, 127, 127, -128
    return a, b


def cases():
  out = []
  i = 0
  for adj_x, adj_y in LAYOUTS:
    for batch, b_batch in BATCHES:
      for m, n in SHAPES:
        za, zb = ZERO_POINTS[i % 4]
        out.append(Case(batch, b_batch, m, n, MFMA_K[(i // 4) % 3], adj_x, adj_y, za, zb))
        i += 1
    # the generic route by K, and by a base one element off at a shape the MFMA route would take
    for j, k in enumerate(GENERIC_K):
      za, zb = ZERO_POINTS[(i + j) % 4]
      out.append(Case(3, (3, 1)[j % 2], 17, 16, k, adj_x, adj_y, za, zb))
      out.append(Case(1, 1, 16, 33, k, adj_x, adj_y, zb, za))
    out.append(Case(3, 3, 32, 16, 64, adj_x, adj_y, 0, 0))        # no sums, with either batch form, whatever the turns gave
    out.append(Case(3, 1, 16, 32, 128, adj_x, adj_y, 0, 0))
    out.append(Case(3, 3, 16, 16, 64, adj_x, adj_y, 5, -3, a_misaligned=True))
    out.append(Case(3, 1, 16, 16, 128, adj_x, adj_y, -128, 127, b_misaligned=True))
  return out


EXTREME = Case(1, 1, 16, 16, MAX_K, False, True, 127, 127)      # all operands -128: every term 255 * 255
EXTREME_ACC = 2130739200


# ---------------------------------------------------------------- hand-built models
# (name, lhs shape, rhs shape, adj_x, adj_y, rhs constant): the lhs is `<name>/a`, the rhs `<name>/b`, the output `<name>/y`
CONSTANT_OPS = (("bmA", (2, 5, 24), (24, 12), False, False, True), ("bmB", (2, 5, 24), (12, 24), False, True, True),
                ("bmC", (3, 24, 5), (3, 24, 12), True, False, True))
ATTENTION_OPS = (("qk", (2, 3, 7, 16), (2, 3, 7, 16), False, True, False), ("pv", (2, 3, 7, 7), (2, 3, 7, 16), False, False, False))
FC = ("fc", 32, 12)      # (name, d, rows): bias, no activation
SAMPLES = 3
BATCH_MATMUL_CODE = 126


def out_shape(a_shape, b_shape, adj_x, adj_y):
  m = a_shape[-1] if adj_x else a_shape[-2]
  n = b_shape[-2] if adj_y else b_shape[-1]
  return tuple(a_shape[:-2]) + (m, n)


def build_model(ops_list, with_fc=True):
  """ModelT tree: one BATCH_MATMUL op per entry of `ops_list`, each with inputs of its own, and one FULLY_CONNECTED.
  Every op carries a BatchMatMulOptionsT (the Quantizer reads adjY from it)."""
  from mi355q import qtyping as q
  model = q.ModelT(version=3, description=b"BATCH_MATMUL ops and one FULLY_CONNECTED (synthetic)")
  model.buffers = [q.BufferT()]
  sg = q.SubGraphT(name=b"main", tensors=[], operators=[], inputs=[], outputs=[])
  rng = np.random.default_rng(411)

  def tensor(name, shape, data=None):
    buffer = 0
    if data is not None:
      model.buffers.append(q.BufferT(data=np.ascontiguousarray(data, np.float32).reshape(-1).view(np.uint8)))
      buffer = len(model.buffers) - 1
    sg.tensors.append(q.TensorT(name=name.encode(), shape=list(shape), buffer=buffer))
    return len(sg.tensors) - 1
  for name, a_shape, b_shape, adj_x, adj_y, constant in ops_list:
    a = tensor(f"{name}/a", a_shape)
    sg.inputs.append(a)
    if constant:
      axis = len(b_shape) - 2 if adj_y else len(b_shape) - 1
      gain = np.exp(rng.uniform(-1.0, 1.0, size=b_shape[axis])).astype(np.float32)      # (per-channel scales matter)
      gain = gain.reshape([-1 if i == axis else 1 for i in range(len(b_shape))])
      b = tensor(f"{name}/b", b_shape, rng.standard_normal(b_shape, dtype=np.float32) * np.float32(0.3) * gain)
    else:
      b = tensor(f"{name}/b", b_shape)
      sg.inputs.append(b)
    y = tensor(f"{name}/y", out_shape(a_shape, b_shape, adj_x, adj_y))
    sg.outputs.append(y)
    sg.operators.append(q.OperatorT(inputs=[a, b], outputs=[y], opcodeIndex=0, builtinOptionsType=101,
                                    builtinOptions=q.BatchMatMulOptionsT(adjX=adj_x, adjY=adj_y)))
  model.operatorCodes = [q.OperatorCodeT(builtinCode=BATCH_MATMUL_CODE, deprecatedBuiltinCode=BATCH_MATMUL_CODE)]
  if with_fc:
    name, d, rows = FC
    x = tensor(f"{name}/x", [1, d])
    w = tensor(f"{name}/w", [rows, d], rng.standard_normal((rows, d), dtype=np.float32) * np.float32(0.3))
    b = tensor(f"{name}/b", [rows], rng.standard_normal(rows, dtype=np.float32))
    y = tensor(f"{name}/y", [1, rows])
    sg.inputs.append(x)
    sg.outputs.append(y)
    sg.operators.append(q.OperatorT(inputs=[x, w, b], outputs=[y], opcodeIndex=1, builtinOptionsType=8,
                                    builtinOptions=q.FullyConnectedOptionsT(fusedActivationFunction=0)))
    model.operatorCodes.append(q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.FULLY_CONNECTED), deprecatedBuiltinCode=9))
  model.subgraphs = [sg]
  model.signatureDefs = [q.SignatureDefT(signatureKey=b"serving_default", subgraphIndex=0)]
  return model


def build_constant_model():
  return build_model(CONSTANT_OPS)


def build_attention_model():
  return build_model(ATTENTION_OPS)


def constant(model, name) -> np.ndarray:
  t = next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)
  return np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()


def float_product(a, b, adj_x, adj_y) -> np.ndarray:
  """float32 [batch, M, N]: one float32 matrix product per batch slice, b's batch 1 or a's."""
  a3, b3 = a.reshape((-1,) + a.shape[-2:]).astype(np.float32), b.reshape((-1,) + b.shape[-2:]).astype(np.float32)
  out = []
  for i in range(a3.shape[0]):
    x, w = a3[i], b3[i if b3.shape[0] != 1 else 0]
    out.append((x.T if adj_x else x) @ (w.T if adj_y else w))
  return np.stack(out).astype(np.float32)


def build_samples(model, ops_list, with_fc=True):
  """[{tensor name: float32 array}]: inputs (an offset makes the activations' zero points non-zero; `pv/a` is a row
  of probabilities, all positive) and the float model's own outputs."""
  rng = np.random.default_rng(412)
  samples = []
  for _ in range(SAMPLES):
    s = {}
    for name, a_shape, b_shape, adj_x, adj_y, is_constant in ops_list:
      a = rng.standard_normal(a_shape, dtype=np.float32) + np.float32(0.4)
      if name == "pv":
        a = np.exp(a)
        a = (a / a.sum(axis=-1, keepdims=True)).astype(np.float32)
      b = constant(model, f"{name}/b") if is_constant else rng.standard_normal(b_shape, dtype=np.float32) - np.float32(0.3)
      s[f"{name}/a"] = a
      if not is_constant:
        s[f"{name}/b"] = b
      s[f"{name}/y"] = float_product(a, b, adj_x, adj_y).reshape(out_shape(a_shape, b_shape, adj_x, adj_y))
    if with_fc:
      name, d, rows = FC
      x = rng.standard_normal((1, 7, d), dtype=np.float32)
      s[f"{name}/x"] = x
      s[f"{name}/y"] = (x.reshape(-1, d) @ constant(model, f"{name}/w").T + constant(model, f"{name}/b")).reshape(1, 7, rows)
    samples.append(s)
  return samples


def grid(values):
  """(scale, zero point) of the asymmetric int8 grid over the samples' range."""
  lo, hi = min(float(np.min(v)) for v in values), max(float(np.max(v)) for v in values)
  lo, hi = min(lo, 0.0), max(hi, 0.0)
  scale = np.float32((hi - lo) / 255.0)
  return scale, int(np.clip(np.rint(-128 - lo / float(scale)), -128, 127))


def quantize_by_hand(model, samples, ops_list, mode="static", per_channel=True):
  """`mode` "static": every activation INT8 with (s, zp) from the samples' range; a constant rhs int8, symmetric, per
  channel along its output axis (or per tensor). "dynamic": the integer constants alone. "weight_only": as dynamic,
  with a DEQUANTIZE in front of every constant. The FULLY_CONNECTED weight is int8 per channel in every mode."""
  import copy
  from mi355q import qtyping as q
  tgt = copy.deepcopy(model)
  sg = tgt.subgraphs[0]
  by_name = {t.name.decode(): t for t in sg.tensors}

  def activation(name):
    if name in by_name and name in samples[0]:
      scale, zp = grid([s[name] for s in samples])
      t = by_name[name]
      t.type = int(q.TensorType.INT8)
      t.quantization = q.QuantizationParametersT(scale=np.array([scale], np.float32), zeroPoint=np.array([zp], np.int64))
  for name, a_shape, b_shape, adj_x, adj_y, is_constant in ops_list:
    if is_constant:
      w = constant(model, f"{name}/b")
      t = by_name[f"{name}/b"]
      axis = len(b_shape) - 2 if adj_y else len(b_shape) - 1
      if per_channel:
        s_w = (np.abs(w).max(axis=tuple(i for i in range(w.ndim) if i != axis)) / 127.0).astype(np.float32)
        bshape = [-1 if i == axis else 1 for i in range(w.ndim)]
        ints = np.clip(np.rint(w / s_w.reshape(bshape)), -127, 127).astype(np.int8)
      else:
        s_w = np.array([np.abs(w).max() / 127.0], np.float32)
        ints = np.clip(np.rint(w / s_w[0]), -127, 127).astype(np.int8)
      t.type = int(q.TensorType.INT8)
      t.quantization = q.QuantizationParametersT(scale=s_w, zeroPoint=np.zeros(s_w.size, np.int64), quantizedDimension=axis)
      tgt.buffers[t.buffer].data = np.ascontiguousarray(ints).reshape(-1).view(np.uint8)
    if mode == "static":
      for end in ("a", "y") + (() if is_constant else ("b",)):
        activation(f"{name}/{end}")
  if f"{FC[0]}/w" in by_name:
    name, d, rows = FC
    w = constant(model, f"{name}/w")
    s_w = (np.abs(w).max(axis=1) / 127.0).astype(np.float32)
    t = by_name[f"{name}/w"]
    t.type = int(q.TensorType.INT8)
    t.quantization = q.QuantizationParametersT(scale=s_w, zeroPoint=np.zeros(rows, np.int64), quantizedDimension=0)
    tgt.buffers[t.buffer].data = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8).reshape(-1).view(np.uint8)
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


def tensor_of(model, name):
  return next(t for t in model.subgraphs[0].tensors if t.name.decode() == name)


def statement(float_model, target_model, samples, op, mode, quantized_outputs=True, dtype=np.float64) -> dict:
  """The figures of one op's entry, written out: the quantizers of layer_execution_cases, the integer statement above,
  sums in float64 over every row of every sample. `target_model`'s tensors give the grids and the stored integers."""
  import layer_execution_cases as EC
  name, a_shape, b_shape, adj_x, adj_y, is_constant = op
  b_t = tensor_of(target_model, f"{name}/b")
  n = out_shape(a_shape, b_shape, adj_x, adj_y)[-1]
  sq_d, sq_r, f_d, tokens = np.zeros(n), np.zeros(n), np.zeros(n), 0
  y_t = tensor_of(target_model, f"{name}/y")
  for s in samples:
    a = np.asarray(s[f"{name}/a"], np.float32)
    b = constant(float_model, f"{name}/b") if is_constant else np.asarray(s[f"{name}/b"], np.float32)
    y = float_product(a, b, adj_x, adj_y)
    batch, m = y.shape[0], y.shape[1]
    if is_constant:
      ints = np.asarray(target_model.buffers[b_t.buffer].data).view(np.int8).reshape(b_shape)
      s_b, zb = np.asarray(b_t.quantization.scale, np.float32), 0
    if mode == "static":
      a_t = tensor_of(target_model, f"{name}/a")
      s_a, za = np.float32(a_t.quantization.scale[0]), int(a_t.quantization.zeroPoint[0])
      aq = EC.quantize_static(a, s_a, za)
      if not is_constant:
        s_b, zb = np.asarray(b_t.quantization.scale, np.float32), int(b_t.quantization.zeroPoint[0])
        ints = EC.quantize_static(b, s_b[0], zb)
      acc = accumulators(aq, ints, adj_x, adj_y, za, zb)
      yq = rescale(acc, [s_a], s_b)
      if quantized_outputs:
        s_y, zp_y = float(np.float32(y_t.quantization.scale[0])), int(y_t.quantization.zeroPoint[0])
        tables = [OC.quantize_multiplier(float(s_a) * float(v) / s_y) for v in s_b.tolist()]
        q_out = output(acc, [t[0] for t in tables], [t[1] for t in tables], zp_y)
        y_f = (q_out.astype(np.int32) - zp_y).astype(np.float32) * np.float32(s_y)
        f_d += ((y_f.astype(np.float64) - y.astype(np.float64)) ** 2).reshape(-1, n).sum(axis=0)
    elif mode == "dynamic":
      aq, s_rows = EC.quantize_rows(a.reshape(batch * m, -1))
      yq = rescale(accumulators(aq.reshape(batch, m, -1), ints, adj_x, adj_y, 0, 0), s_rows, s_b)
    else:
      axis = len(b_shape) - 2 if adj_y else len(b_shape) - 1
      deq = (ints.astype(np.float64) * s_b.astype(np.float64).reshape(
          [-1 if (i == axis and s_b.size > 1) else 1 for i in range(len(b_shape))])).astype(np.float32)
      yq = float_product(a, deq, adj_x, adj_y)
    sq_d += ((yq.astype(np.float64) - y.astype(np.float64)) ** 2).reshape(-1, n).sum(axis=0)
    sq_r += (y.astype(np.float64) ** 2).reshape(-1, n).sum(axis=0)
    tokens += batch * m
  out = {"tokens": tokens, "rows": n, "signal": float(sq_r.sum() / tokens), "error": float(sq_d.sum() / tokens),
         "per_channel_error": sq_d / tokens}
  if mode == "static" and quantized_outputs:
    out.update(final_error=float(f_d.sum() / tokens), final_per_channel_error=f_d / tokens)
  return out


# ---------------------------------------------------------------- NumPy in place of the device
def numpy_kernels(**kwargs):
  """layer_output_cases.numpy_kernels() with the methods of `batch_matmul`: the statement above."""
  class NumpyBmmKernels(OC.numpy_kernels(**kwargs)):
    def sample_nd(self, value):
      value = value.cpu().numpy() if hasattr(value, "cpu") else np.asarray(value)
      return np.ascontiguousarray(value, np.float32)

    def bmm_constant(self, plan, shape):
      return np.asarray(plan.data).view(np.int8).reshape(shape), np.asarray(plan.scale, np.float32)

    def bmm_float(self, a, b, adj_x, adj_y):
      a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
      return ((a.T if adj_x else a) @ (b.T if adj_y else b)).astype(np.float32)

    def bmm_forward(self, aq, bq, adj_x, adj_y, a_scale, a_zero_point, b_scale, b_zero_point):
      return rescale(accumulators(aq, bq, adj_x, adj_y, a_zero_point, b_zero_point), a_scale, b_scale)

    def bmm_output(self, aq, bq, adj_x, adj_y, a_zero_point, b_zero_point, multiplier, shift, out_zero_point):
      return output(accumulators(aq, bq, adj_x, adj_y, a_zero_point, b_zero_point), multiplier, shift, out_zero_point)
  return NumpyBmmKernels
