"""Records WHAT model_validator.compare_layer_execution decides, with no float figure: for hand-built models in every
mode, and for models with two defects at once, under the keyword combinations the host tests use (all off, each on
alone, all on; see combinations()), the `skipped` map, every entry's key set and non-float values, and the ordered list of
LayerExecutionKernels methods the run called. It goes through the public API alone, so the same script records any
revision of the code; tests/test_layer_execution_structure_host.py compares a fresh record with
tests/golden/layer_execution_structure.json.

  python tools/record_layer_execution_structure.py [output.json]
"""
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ai-edge-quantizer_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "layer_execution_structure.json")
KEYWORDS = ("follow_input_transforms", "int16_activations", "quantized_outputs", "conv_2d", "depthwise_conv_2d",
            "batch_matmul")
COMBINATIONS = ((),) + tuple((k,) for k in KEYWORDS) + (KEYWORDS,)


def combinations(label: str) -> tuple:
  """All off, each keyword alone and all on; for the models of another op kind than FULLY_CONNECTED, whose runs
  without that kind's keyword would all repeat the one FULLY_CONNECTED entry: the kind's keyword alone, with each of
  the three keywords that are no op kind, and all on. A two-defect model ("+" in its label) leaves out
  `quantized_outputs` alone, which reads nothing before an op is executed."""
  kind = {"conv": "conv_2d", "dwconv": "depthwise_conv_2d", "bmm": "batch_matmul"}.get(label.split("/")[0])
  every = COMBINATIONS if kind is None else ((kind,),) + tuple((k, kind) for k in KEYWORDS[:3]) + (KEYWORDS,)
  return tuple(c for c in every if "+" not in label or c == KEYWORDS or "quantized_outputs" not in c)


# ---------------------------------------------------------------- the kernels, and the calls they receive
def _kernels():
  """One NumPy stand-in with the methods of every op kind."""
  import bmm_execution_cases as BC
  import dwconv_execution_cases as DC

  class AllKernels(DC.numpy_kernels(), BC.numpy_kernels()):
    pass
  return AllKernels()


class _Recorder:
  """Passes every method call on to `kernels` and keeps the methods' names in order."""

  def __init__(self, kernels):
    self._kernels, self.calls = kernels, []

  def __getattr__(self, name):
    method = getattr(self._kernels, name)

    def call(*args, **kwargs):
      self.calls.append(name)
      return method(*args, **kwargs)
    return call


def run_length(calls: list) -> list:
  """[[block of names, repeats], ...]: at every position the shortest block (up to 64 names) that repeats at once,
  with all its repeats; otherwise one name, once. Equal call lists give equal encodings and the reverse."""
  out, i = [], 0
  while i < len(calls):
    for size in range(1, min(64, (len(calls) - i) // 2) + 1):
      block = calls[i:i + size]
      if calls[i + size:i + 2 * size] == block:
        repeats = 2
        while calls[i + repeats * size:i + (repeats + 1) * size] == block:
          repeats += 1
        out.append([" ".join(block), repeats])
        i += repeats * size
        break
    else:
      if out and out[-1][1] == 1:
        out[-1][0] += " " + calls[i]
      else:
        out.append([calls[i], 1])
      i += 1
  return out


# ---------------------------------------------------------------- edits of a target model: one defect each
def _tensor_id(model, name: str) -> int:
  return next(i for i, t in enumerate(model.subgraphs[0].tensors) if t.name.decode() == name)


def _tensor(model, name: str):
  return model.subgraphs[0].tensors[_tensor_id(model, name)]


def _op(model, y_name: str):
  sg = model.subgraphs[0]
  return next(op for op in sg.operators if sg.tensors[op.outputs[0]].name.decode() == y_name)


def float_weight(tgt, ref, name: str) -> None:
  """The target constant `name` stays what it is in the float model."""
  t, r = _tensor(tgt, name), _tensor(ref, name)
  t.type, t.quantization = r.type, None
  tgt.buffers[t.buffer].data = ref.buffers[r.buffer].data


def int16_weight(tgt, name: str) -> None:
  """The int8 constant `name` stored as INT16, a kind no op kind executes."""
  from mi355q import qtyping as q
  t = _tensor(tgt, name)
  ints = np.asarray(tgt.buffers[t.buffer].data).view(np.int8).astype(np.int16)
  t.type = int(q.TensorType.INT16)
  tgt.buffers[t.buffer].data = ints.view(np.uint8)


def weight_zero_point(tgt, name: str, zero_point: int = 3) -> None:
  t = _tensor(tgt, name)
  t.quantization.zeroPoint = np.full(len(t.quantization.scale), zero_point, np.int64)


def activation(tgt, name: str, ttype: str, zero_point: int = 0) -> None:
  """The activation `name` as INT8 / INT16 with one scale and `zero_point`."""
  from mi355q import qtyping as q
  t = _tensor(tgt, name)
  t.type = int(getattr(q.TensorType, ttype))
  t.quantization = q.QuantizationParametersT(scale=np.array([0.02], np.float32), zeroPoint=np.array([zero_point], np.int64))


def insert_multiply(tgt, x_name: str, y_name: str, width: int) -> None:
  """The op that writes `y_name` reads MUL(x, constant float32 [width]) in place of `x_name` (an OSCAR multiply)."""
  from mi355q import qtyping as q
  sg = tgt.subgraphs[0]
  x = _tensor_id(tgt, x_name)
  tgt.buffers.append(q.BufferT(data=np.linspace(0.5, 2.0, width).astype(np.float32).view(np.uint8)))
  sg.tensors.append(q.TensorT(name=x_name.encode() + b"_multiplier", shape=[width], buffer=len(tgt.buffers) - 1))
  sg.tensors.append(q.TensorT(name=x_name.encode() + b"_scaled", shape=list(sg.tensors[x].shape), buffer=0,
                              type=sg.tensors[x].type, quantization=sg.tensors[x].quantization))
  tgt.operatorCodes.append(q.OperatorCodeT(builtinCode=int(q.BuiltinOperator.MUL), deprecatedBuiltinCode=18))
  op = _op(tgt, y_name)
  op.inputs = [len(sg.tensors) - 1] + list(op.inputs[1:])
  sg.operators.insert(0, q.OperatorT(inputs=[x, len(sg.tensors) - 2], outputs=[len(sg.tensors) - 1],
                                     opcodeIndex=len(tgt.operatorCodes) - 1))


def edited(tgt, *edits):
  """A copy of `tgt` with every (edit, *arguments) of `edits` applied."""
  tgt = copy.deepcopy(tgt)
  for edit, *args in edits:
    edit(tgt, *args)
  return tgt


def without(samples: list, name: str) -> list:
  return [{k: v for k, v in s.items() if k != name} for s in samples]


def sliced(samples: list, name: str, channels: int) -> list:
  """The first `channels` channels of sample `name`."""
  return [dict(s, **{name: np.ascontiguousarray(s[name][..., :channels])}) for s in samples]


def reshaped(samples: list, name: str, shape: tuple) -> list:
  return [dict(s, **{name: np.ascontiguousarray(s[name]).reshape(shape)}) for s in samples]


# ---------------------------------------------------------------- the models
def _fully_connected_models() -> list:
  import conv_execution_cases as CC
  import layer_output_cases as OC
  ref = OC.build_model()
  samples = OC.build_samples(ref)[:2]
  out = [("fc/static8", ref, OC.quantize_by_hand(ref, samples, 8), samples),
         ("fc/static16", ref, OC.quantize_by_hand(ref, samples, 16), samples)]
  # the FULLY_CONNECTED op of the CONV_2D model has a dynamic and a weight-only form as well
  cref = CC.build_model()
  csamples = CC.build_samples(cref)[:2]
  targets = {mode: CC.quantize_by_hand(cref, csamples, mode) for mode in ("static", "dynamic", "weight_only")}
  multiply = (insert_multiply, "fc/x", "fc/y", CC.FC[1])
  out += [
      ("fc/multiply", cref, edited(targets["dynamic"], multiply), csamples),
      ("fc/int16+float_weight", cref,
       edited(targets["static"], (activation, "fc/x", "INT16"), (float_weight, cref, "fc/w")), csamples),
      ("fc/multiply+int16_weight", cref, edited(targets["dynamic"], multiply, (int16_weight, "fc/w")), csamples),
      ("fc/weight_zero_point+no_sample", cref, edited(targets["static"], (weight_zero_point, "fc/w")),
       without(csamples, "fc/x")),
      ("fc/int16+dequantize", cref, edited(targets["weight_only"], (activation, "fc/x", "INT16")), csamples),
      ("fc/int16_zero_point+int16_weight", cref,
       edited(targets["static"], (activation, "fc/x", "INT16", 5), (int16_weight, "fc/w")), csamples),
      ("fc/int8_zero_point_200+bias_type", cref,
       edited(targets["static"], (activation, "fc/x", "INT8", 200), (activation, "fc/b", "INT8")), csamples),
      ("fc/sample_width+weight_zero_point", cref, edited(targets["dynamic"], (weight_zero_point, "fc/w")),
       sliced(csamples, "fc/x", CC.FC[1] - 1)),
  ]
  return out


def _conv_models(module, prefix: str, op_name: str, channels: int) -> list:
  """The models of conv_execution_cases or dwconv_execution_cases: every mode, and the defects on op `op_name`."""
  ref = module.build_model()
  samples = module.build_samples(ref)[:2]
  targets = {mode: module.quantize_by_hand(ref, samples, mode) for mode in ("static", "dynamic", "weight_only")}
  out = [(f"{prefix}/{mode}", ref, tgt, samples) for mode, tgt in targets.items()]
  out.append((f"{prefix}/static16", ref, module.quantize_by_hand(ref, samples, "static", 16), samples))
  x, w, y = f"{op_name}/x", f"{op_name}/w", f"{op_name}/y"
  n, hw = module.BATCH, module.HEIGHT * module.WIDTH
  out += [
      (f"{prefix}/int16+float_weight", ref,
       edited(targets["static"], (activation, x, "INT16"), (float_weight, ref, w)), samples),
      (f"{prefix}/multiply+int16_weight", ref,
       edited(targets["dynamic"], (insert_multiply, x, y, channels), (int16_weight, w)), samples),
      (f"{prefix}/weight_zero_point+no_sample", ref, edited(targets["static"], (weight_zero_point, w)), without(samples, x)),
      (f"{prefix}/rank3_sample+channels", ref, targets["dynamic"],
       reshaped(sliced(samples, x, channels - 1), x, (n, hw, channels - 1))),
      (f"{prefix}/channels+weight_zero_point", ref, edited(targets["dynamic"], (weight_zero_point, w)),
       sliced(samples, x, channels - 1)),
      (f"{prefix}/int16+dequantize", ref, edited(targets["weight_only"], (activation, x, "INT16")), samples),
      (f"{prefix}/int8_zero_point_200+int16_weight", ref,
       edited(targets["static"], (activation, x, "INT8", 200), (int16_weight, w)), samples),
  ]
  return out


def _batch_matmul_models() -> list:
  import bmm_execution_cases as BC
  out = []
  ref = BC.build_constant_model()
  samples = BC.build_samples(ref, BC.CONSTANT_OPS)[:2]
  targets = {mode: BC.quantize_by_hand(ref, samples, BC.CONSTANT_OPS, mode) for mode in ("static", "dynamic", "weight_only")}
  out += [(f"bmm/constant/{mode}", ref, tgt, samples) for mode, tgt in targets.items()]
  out.append(("bmm/constant/static_per_tensor", ref, BC.quantize_by_hand(ref, samples, BC.CONSTANT_OPS, "static", False),
              samples))
  aref = BC.build_attention_model()
  asamples = BC.build_samples(aref, BC.ATTENTION_OPS)[:2]
  attention = BC.quantize_by_hand(aref, asamples, BC.ATTENTION_OPS, "static")
  out.append(("bmm/attention/static", aref, attention, asamples))
  out.append(("bmm/attention/float", aref, copy.deepcopy(aref), asamples))

  def flip_adj_x(tgt, y_name):
    op = _op(tgt, y_name)
    op.builtinOptions.adjX = not op.builtinOptions.adjX

  def rename(tgt, name):
    _tensor(tgt, name).name = name.encode() + b"_renamed"
  out += [
      ("bmm/int16_lhs+dequantize", ref, edited(targets["weight_only"], (activation, "bmA/a", "INT16")), samples),
      ("bmm/adj_x+no_target", ref, edited(targets["static"], (flip_adj_x, "bmA/y"), (rename, "bmA/y")), samples),
      ("bmm/adj_x+float_constant", ref, edited(targets["static"], (flip_adj_x, "bmB/y"), (float_weight, ref, "bmB/b")),
       samples),
      ("bmm/weight_zero_point+no_sample", ref, edited(targets["static"], (weight_zero_point, "bmA/b")),
       without(samples, "bmA/a")),
      ("bmm/int16_lhs+float_constant", ref,
       edited(targets["static"], (activation, "bmA/a", "INT16"), (float_weight, ref, "bmA/b")), samples),
      ("bmm/int16_lhs+int16_constant", ref,
       edited(targets["static"], (activation, "bmB/a", "INT16"), (int16_weight, "bmB/b")), samples),
      ("bmm/dynamic_adj_x+weight_zero_point", ref, edited(targets["dynamic"], (weight_zero_point, "bmC/b")), samples),
      ("bmm/multiply+int16_constant", ref,
       edited(targets["dynamic"], (insert_multiply, "bmA/a", "bmA/y", 24), (int16_weight, "bmA/b")), samples),
      ("bmm/attention/int16_a+multiply_b", aref,
       edited(attention, (activation, "qk/a", "INT16"), (insert_multiply, "qk/b", "qk/y", 16)), asamples),
      ("bmm/attention/multiply_a+int16_b", aref,
       edited(attention, (insert_multiply, "pv/a", "pv/y", 7), (activation, "pv/b", "INT16")), asamples),
      ("bmm/attention/zero_point_200_a+no_sample_b", aref, edited(attention, (activation, "qk/a", "INT8", 200)),
       without(asamples, "qk/b")),
      ("bmm/attention/int16_b+output_type", aref,
       edited(attention, (activation, "pv/b", "INT16"), (activation, "pv/y", "INT16")), asamples),
  ]
  return out


def models() -> list:
  """[(label, float model, target model, samples)]."""
  import conv_execution_cases as CC
  import dwconv_execution_cases as DC
  return (_fully_connected_models() + _conv_models(CC, "conv", "convA", 16) + _conv_models(DC, "dwconv", "dwA", 16)
          + _batch_matmul_models())


# ---------------------------------------------------------------- the record
def _plain(value):
  if isinstance(value, (list, tuple)):
    return [_plain(v) for v in value]
  if isinstance(value, (np.integer, np.bool_)):
    return value.item()
  assert value is None or isinstance(value, (str, int, bool)), value
  return value


def record() -> dict:
  """{label: {keywords: {"skipped", "entries": {name: {"keys", "values"}}, "calls"}}}."""
  from mi355q import model_validator as mv
  out = {}
  for label, ref, tgt, samples in models():
    runs = out[label] = {}
    for combination in combinations(label):
      kernels = _Recorder(_kernels())
      got = mv.compare_layer_execution(ref, tgt, samples, kernels=kernels, **{k: True for k in combination})
      runs[",".join(combination) or "none"] = {
          "skipped": dict(got.skipped),
          "entries": {name: {"keys": " ".join(sorted(entry)),
                             "values": {k: _plain(entry[k]) for k in STRUCTURE_KEYS if k in entry}}
                      for name, entry in got.results.items()},
          "calls": run_length(kernels.calls)}
  return out


# an entry's values that are no float figures
STRUCTURE_KEYS = ("op", "mode", "rows", "d", "tokens", "weight", "input", "input_b", "operands", "adj_x", "adj_y", "batch",
                  "kernel", "strides", "dilations", "padding", "output_hw", "depth_multiplier", "activation_bits",
                  "output_bits", "fused_activation", "final_skipped", "input_transform", "hadamard_size")
# those that follow from the keywords; the others describe the op and its samples
KEYWORD_KEYS = ("op", "activation_bits", "output_bits", "fused_activation", "final_skipped", "input_transform",
                "hadamard_size")
TABLES = ("skipped", "block", "calls", "keys", "op_values", "keyword_values")


def compact(data: dict) -> dict:
  """record()'s result with everything that repeats kept once: {"tables": {name: [distinct values]}, "runs": {label:
  {keywords: [skipped, calls, {entry name: [keys, op values, keyword values]}]}}}, every value an index into its
  table, `calls` a list of indices into `block`. expand() gives record()'s form back."""
  tables = {name: [] for name in TABLES}

  def index(name: str, value) -> int:
    if value not in tables[name]:
      tables[name].append(value)
    return tables[name].index(value)
  runs = {}
  for label, by_keywords in data.items():
    runs[label] = {}
    for keywords, run in by_keywords.items():
      entries = {}
      for name, entry in run["entries"].items():
        values = entry["values"]
        entries[name] = [index("keys", entry["keys"]),
                         index("op_values", {k: v for k, v in values.items() if k not in KEYWORD_KEYS}),
                         index("keyword_values", {k: v for k, v in values.items() if k in KEYWORD_KEYS})]
      calls = index("calls", [index("block", block) for block in run["calls"]])
      runs[label][keywords] = [index("skipped", run["skipped"]), calls, entries]
  return {"tables": tables, "runs": runs}


def expand(stored: dict) -> dict:
  tables, out = stored["tables"], {}
  for label, by_keywords in stored["runs"].items():
    out[label] = {}
    for keywords, (skipped, calls, entries) in by_keywords.items():
      out[label][keywords] = {
          "skipped": tables["skipped"][skipped],
          "entries": {name: {"keys": tables["keys"][k], "values": {**tables["op_values"][o], **tables["keyword_values"][f]}}
                      for name, (k, o, f) in entries.items()},
          "calls": [tables["block"][b] for b in tables["calls"][calls]]}
  return out


def dumps(stored: dict) -> str:
  """compact()'s result, one table entry and one model per line."""
  one = lambda value: json.dumps(value, separators=(",", ":"))      # pylint: disable=unnecessary-lambda-assignment
  tables = ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(one(v) for v in values))
                      for name, values in stored["tables"].items())
  runs = ",\n".join("%s: %s" % (json.dumps(label), one(v)) for label, v in stored["runs"].items())
  return '{"tables": {\n%s\n},\n"runs": {\n%s\n}}\n' % (tables, runs)


if __name__ == "__main__":
  path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
  with open(path, "w") as fh:
    fh.write(dumps(compact(record())))
  print(path, os.path.getsize(path), "bytes")
