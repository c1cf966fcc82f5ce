"""Model validation: compare a float model with its quantized form tensor by tensor (ref: model_validator.py).

Constant tensors need no interpreter: they are read straight from the two flatbuffers, the quantized
constant is dequantized in registers by csrc/validation.hip, and all constants of a signature are
compared in one batched call. Input, output and intermediate tensors need a run of the model, which this
library does not do: the caller passes `run_signature(model_bytes, signature_key, inputs) ->
{tensor name: array}` (its own interpreter), the same boundary calibration draws.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
import pathlib
from collections.abc import Callable, Iterable, Sequence
from typing import Any, Optional, Union

import numpy as np

from . import schema
from .transformations import graph_edits
from .utils import flexbuffer
from .utils import tfl_flatbuffer_utils
from .utils import validation_utils

DEFAULT_SIGNATURE_KEY = "serving_default"
_DEFAULT_SIGNATURE_KEY = DEFAULT_SIGNATURE_KEY
RunSignature = Callable[[bytes, str, dict], dict]


# ----------------------------------------------------------------------------- flatbuffer views
def _model(model) -> Any:
  return tfl_flatbuffer_utils.read_model(model)


def _signature_subgraph(model, signature_key: Optional[str]) -> tuple[int, Any]:
  """(main subgraph index, SignatureDef or None) of a signature (ref: tfl_interpreter_utils.py:328-342)."""
  sigs = model.signatureDefs or []
  for sig in sigs:
    key = sig.signatureKey
    key = key.decode() if isinstance(key, (bytes, bytearray)) else key
    if signature_key is None or key == signature_key:
      return int(sig.subgraphIndex), sig
  if signature_key not in (None, DEFAULT_SIGNATURE_KEY) and sigs:
    raise ValueError(f"signature {signature_key!r} not found in the model")
  return 0, None


def signature_keys(model) -> list[str]:
  m = _model(model)
  keys = []
  for sig in m.signatureDefs or []:
    k = sig.signatureKey
    keys.append(k.decode() if isinstance(k, (bytes, bytearray)) else k)
  return keys or [DEFAULT_SIGNATURE_KEY]


def _io_tensor_names(model, signature_key: str, which: str) -> list[str]:
  m = _model(model)
  sg_index, sig = _signature_subgraph(m, signature_key)
  tensors = m.subgraphs[sg_index].tensors
  if sig is not None:
    return [schema.tensor_name(tensors[t.tensorIndex]) for t in (getattr(sig, which) or [])]
  ids = m.subgraphs[sg_index].inputs if which == "inputs" else m.subgraphs[sg_index].outputs
  return [schema.tensor_name(tensors[i]) for i in (ids if ids is not None else [])]


def get_input_tensor_names(model, signature_key: str = DEFAULT_SIGNATURE_KEY) -> list[str]:
  return _io_tensor_names(model, signature_key, "inputs")


def get_output_tensor_names(model, signature_key: str = DEFAULT_SIGNATURE_KEY) -> list[str]:
  return _io_tensor_names(model, signature_key, "outputs")


def _has_data(buffers, tensor) -> bool:
  buf = buffers[tensor.buffer] if tensor.buffer < len(buffers) else None
  return buf is not None and buf.data is not None and len(buf.data) > 0


def _numel(tensor) -> int:
  return int(np.prod(tensor.shape)) if tensor.shape is not None else 1


def get_constant_tensor_names(model, subgraph_index: int = 0, min_constant_size: int = 1) -> list[str]:
  """Names of the tensors with buffer data of at least `min_constant_size` elements (ref: tfl_interpreter_utils.py:292-325)."""
  m = _model(model)
  out = []
  for t in m.subgraphs[subgraph_index].tensors:
    if t.type == schema.TensorType.STRING or not _has_data(m.buffers, t):
      continue
    if _numel(t) >= min_constant_size:
      out.append(schema.tensor_name(t))
  return out


def _raw_bytes(buffers, tensor) -> np.ndarray:
  raw = buffers[tensor.buffer].data
  if hasattr(raw, "copy_into"):
    raw = np.ravel(np.asarray(raw)).view(np.uint8)
  return raw if isinstance(raw, np.ndarray) else np.frombuffer(raw, dtype=np.uint8)


@dataclasses.dataclass
class ConstantPlan:
  """How one constant of the target model is compared: `kind` and the scale view (ops.CompareTarget)."""
  name: str
  reference: np.ndarray          # float32 values of the reference constant (flat)
  data: np.ndarray               # stored bytes / values of the target constant (flat)
  kind: str
  dequantized: bool
  scale: Optional[np.ndarray] = None
  zero_point: Optional[np.ndarray] = None
  channels: int = 1
  inner: int = 1
  diff_bits: int = 32


_KIND = {schema.TensorType.FLOAT32: "f32", schema.TensorType.FLOAT16: "f16", schema.TensorType.BFLOAT16: "bf16",
         schema.TensorType.INT8: "i8", schema.TensorType.INT16: "i16", schema.TensorType.INT32: "i32",
         schema.TensorType.INT4: "i4", schema.TensorType.INT2: "i2"}


def _target_plan(name: str, ref_values: np.ndarray, m, tensor) -> Optional[ConstantPlan]:
  ttype = schema.TensorType(tensor.type)
  n = _numel(tensor)
  kind = _KIND.get(ttype)
  raw = _raw_bytes(m.buffers, tensor)
  q = tensor.quantization
  blockwise = q is not None and getattr(q, "details", None) is not None and hasattr(q.details, "blockSize")
  has_scale = q is not None and ((q.scale is not None and len(q.scale) > 0) or blockwise)
  if kind is None or ttype == schema.TensorType.FLOAT32 or not has_scale:
    # compared as stored: a raw cast to float32 (ref: tfl_interpreter_utils.py:176-182)
    if kind in ("i4", "i2"):
      return None
    if kind is None:
      values = np.asarray(tfl_flatbuffer_utils.get_tensor_data(tensor, m.buffers), np.float32).ravel()
      return ConstantPlan(name, ref_values, values, "f32", False)
    if kind in ("i8", "i16", "i32"):
      return ConstantPlan(name, ref_values, raw.view(schema.NUMPY_DTYPE[ttype])[:n], kind, False,
                          np.ones(1, np.float32), None, 1, 1, 32)
    dtype = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16}[kind]
    return ConstantPlan(name, ref_values, raw.view(dtype)[:n], kind, False)
  shape = list(tensor.shape) if tensor.shape is not None else []
  data = raw if kind in ("i4", "i2") else raw.view(schema.NUMPY_DTYPE[ttype])[:n]
  if blockwise:
    # one scale per block along the last axis (transformations/quantize_tensor.py stores them as float16)
    # (the scales are a tensor of their own, read by constant_plans)
    block = int(q.details.blockSize)
    return ConstantPlan(name, ref_values, data, kind, True, None, None, n // block, block, 32)
  scale = np.asarray(q.scale, np.float32)
  zp = np.asarray(q.zeroPoint if q.zeroPoint is not None and len(q.zeroPoint) else np.zeros(len(scale)), np.int64)
  zp = zp.astype(np.int32)
  if len(scale) == 1:
    channels, inner = 1, 1
  else:
    axis = int(q.quantizedDimension)
    channels, inner = int(shape[axis]), int(np.prod(shape[axis + 1:])) if axis + 1 < len(shape) else 1
  # the interpreter's zero points are int32: q - zp is formed in int32 and scaled in float64
  return ConstantPlan(name, ref_values, data, kind, True, scale, zp, channels, inner, 32)


def constant_plans(reference_model, target_model, signature_key: Optional[str] = DEFAULT_SIGNATURE_KEY
                   ) -> list[ConstantPlan]:
  """The constants that compare_model compares for a signature, and how (see the module docstring)."""
  ref, tgt = _model(reference_model), _model(target_model)
  sg_ref, _ = _signature_subgraph(ref, signature_key)
  sg_tgt, _ = _signature_subgraph(tgt, signature_key)
  tgt_tensors = tgt.subgraphs[sg_tgt].tensors
  by_name = {}
  for t in tgt_tensors:
    by_name.setdefault(schema.tensor_name(t), t)
  plans = []
  for t in ref.subgraphs[sg_ref].tensors:
    if t.type == schema.TensorType.STRING or not _has_data(ref.buffers, t) or _numel(t) < 1:
      continue
    name = schema.tensor_name(t)
    target = by_name.get(name)
    if target is None or not _has_data(tgt.buffers, target) or _numel(target) != _numel(t):
      continue
    if t.type in (schema.TensorType.INT4, schema.TensorType.INT2):
      continue
    values = tfl_flatbuffer_utils.get_tensor_data(t, ref.buffers)
    if values is None:
      continue
    plan = _target_plan(name, np.ravel(np.asarray(values, np.float32)), tgt, target)
    if plan is None:
      continue
    if plan.kind in ("i4", "i2", "i8", "i16", "i32") and plan.dequantized and plan.scale is None:
      _read_blockwise_scales(plan, tgt, tgt_tensors, target)
    plans.append(plan)
  return plans


def _read_blockwise_scales(plan: ConstantPlan, tgt, tgt_tensors, target) -> None:
  """The scales of a blockwise constant are a tensor of their own in the target model."""
  q = target.quantization
  sc = tgt_tensors[int(q.details.scales)]
  plan.scale = np.asarray(tfl_flatbuffer_utils.get_tensor_data(sc, tgt.buffers), np.float32).ravel()
  plan.zero_point = None
  if len(target.shape) != 2 or plan.channels != len(plan.scale):
    raise ValueError(
        f"blockwise constant {plan.name!r}: expected a 2-D weight with one scale per block of {plan.inner} along its"
        f" last axis, got shape {list(target.shape)} and {len(plan.scale)} scales")


def _device_target(plan: ConstantPlan):
  import torch
  from . import ops
  from . import runtime as rt
  data = rt.to_device(plan.data)
  if plan.kind == "bf16":
    data = data.view(torch.bfloat16)
  scale = None if plan.scale is None else rt.to_device(plan.scale)
  zp = None if plan.zero_point is None else rt.to_device(plan.zero_point)
  return ops.CompareTarget(data, plan.reference.size, plan.kind, scale, zp, plan.channels, plan.inner, plan.diff_bits)


def compare_constants(reference_model, target_model, error_metrics: Sequence[validation_utils.ValidationErrorMetric],
                      signature_key: Optional[str] = DEFAULT_SIGNATURE_KEY) -> dict[str, dict]:
  """{constant name: {metric: value}} of one signature's constants, from one batched comparison."""
  from . import runtime as rt
  plans = constant_plans(reference_model, target_model, signature_key)
  if not plans:
    return {}
  pairs = [(_device_target(p), rt.to_device(p.reference)) for p in plans]
  values = validation_utils.compare_all_batched(pairs, error_metrics)
  return {p.name: v for p, v in zip(plans, values)}


# ----------------------------------------------------------------------------- results
@dataclasses.dataclass(frozen=True)
class SingleSignatureComparisonResult:
  """Comparison result for a single signature."""
  error_metrics: Sequence[validation_utils.ValidationErrorMetric]
  input_tensors: dict[str, dict[str, float]]
  output_tensors: dict[str, dict[str, float]]
  constant_tensors: dict[str, dict[str, float]]
  intermediate_tensors: dict[str, dict[str, float]]


class ComparisonResult:
  """Comparison result for a model (ref: model_validator.py:55-234)."""

  def __init__(self, reference_model: bytes, target_model: bytes):
    self._reference_model = reference_model
    self._target_model = target_model
    self._comparison_results: dict[str, SingleSignatureComparisonResult] = {}

  def get_signature_comparison_result(self, signature_key: str = _DEFAULT_SIGNATURE_KEY
                                      ) -> SingleSignatureComparisonResult:
    if signature_key not in self._comparison_results:
      raise ValueError(
          f"{signature_key} is not in the comparison_results. Available"
          f" signature keys are: {self.available_signature_keys()}")
    return self._comparison_results[signature_key]

  def available_signature_keys(self) -> list[str]:
    return list(self._comparison_results.keys())

  def add_new_signature_results(self, error_metrics: Sequence[validation_utils.ValidationErrorMetric],
                                comparison_result: dict[str, dict[str, float]],
                                signature_key: str = _DEFAULT_SIGNATURE_KEY,
                                validate_output_tensors_only: bool = False) -> None:
    if signature_key in self._comparison_results:
      raise ValueError(f"{signature_key} is already in the comparison_results.")
    result = {key: {k: float(v) for k, v in value.items()} for key, value in comparison_result.items()}
    output_tensor_results = {}
    for name in get_output_tensor_names(self._reference_model, signature_key):
      if name in result:
        output_tensor_results[name] = result.pop(name)
    input_tensor_results = {}
    constant_tensor_results = {}
    if validate_output_tensors_only:
      result = {}
    else:
      for name in get_input_tensor_names(self._reference_model, signature_key):
        if name in result:
          input_tensor_results[name] = result.pop(name)
      sg, _ = _signature_subgraph(_model(self._reference_model), signature_key)
      for name in get_constant_tensor_names(self._reference_model, sg):
        if name in result:
          constant_tensor_results[name] = result.pop(name)
    self._comparison_results[signature_key] = SingleSignatureComparisonResult(
        error_metrics=error_metrics,
        input_tensors=input_tensor_results,
        output_tensors=output_tensor_results,
        constant_tensors=constant_tensor_results,
        intermediate_tensors=result,
    )

  def get_all_tensor_results(self) -> dict[str, Any]:
    result = {}
    for _, r in self._comparison_results.items():
      result.update(r.input_tensors)
      result.update(r.output_tensors)
      result.update(r.constant_tensors)
      result.update(r.intermediate_tensors)
    return result

  def get_model_size_reduction(self) -> tuple[int, float]:
    reduced_model_size = len(self._reference_model) - len(self._target_model)
    reduction_perc = reduced_model_size / len(self._reference_model) * 100
    return reduced_model_size, reduction_perc

  def save(self, save_folder: str, model_name: str) -> None:
    """`<model_name>_comparison_result.json` and one Model Explorer file per metric (ref: model_validator.py:184-234)."""
    reduced_model_size, reduction_ratio = self.get_model_size_reduction()
    result = {"reduced_size_bytes": reduced_model_size, "reduced_size_percentage": reduction_ratio}
    error_metrics_seen = []
    for signature, r in self._comparison_results.items():
      for metric in r.error_metrics:
        if metric not in error_metrics_seen:
          error_metrics_seen.append(metric)
      result[str(signature)] = {
          "input_tensors": r.input_tensors,
          "output_tensors": r.output_tensors,
          "constant_tensors": r.constant_tensors,
          "intermediate_tensors": r.intermediate_tensors,
      }
    save_path = pathlib.Path(save_folder)
    os.makedirs(str(save_path), exist_ok=True)
    with open(str(save_path / (model_name + "_comparison_result.json")), "w") as fh:
      fh.write(json.dumps(result))
    color_threshold = [0.05, 0.1, 0.2, 0.4, 1, 10, 100]
    for metric in error_metrics_seen:
      json_object = create_json_for_model_explorer(self, metric=metric, threshold=color_threshold)
      with open(str(save_path / f"{model_name}_comparison_result_me_input_{metric.value}.json"), "w") as fh:
        fh.write(json_object)


def create_json_for_model_explorer(data: ComparisonResult, metric: validation_utils.ValidationErrorMetric,
                                   threshold: list[Union[int, float]]) -> str:
  """The Model Explorer overlay of one metric (ref: model_validator.py:412-460)."""
  data_vals = data.get_all_tensor_results()
  color_scheme = []
  results = {}
  key = getattr(metric, "value", str(metric))
  for name, values in data_vals.items():
    if key in values:
      results[name] = {"value": float(values[key])}
  if threshold:
    green = 255
    gradient = math.floor(255 / len(threshold))
    for val in threshold:
      color_scheme.append({"value": val, "bgColor": f"rgb(200, {green}, 0)"})
      green = max(0, green - gradient)
  return json.dumps({"results": results, "thresholds": color_scheme})


# ----------------------------------------------------------------------------- compare_model
def create_random_normal_input_data(model, signature_key: str, num_samples: int = 1,
                                    random_seed: int = 666) -> list[dict[str, Any]]:
  """Seeded random inputs from a signature's input shapes and types (ref: tfl_interpreter_utils.py:345-475)."""
  m = _model(model)
  sg, sig = _signature_subgraph(m, signature_key)
  tensors = m.subgraphs[sg].tensors
  if sig is not None:
    items = [(t.name.decode() if isinstance(t.name, (bytes, bytearray)) else t.name, tensors[t.tensorIndex])
             for t in (sig.inputs or [])]
  else:
    items = [(schema.tensor_name(tensors[i]), tensors[i]) for i in (m.subgraphs[sg].inputs or [])]
  rng = np.random.default_rng(random_seed)
  dataset = []
  for _ in range(num_samples):
    sample = {}
    for arg, t in items:
      shape = tuple(int(d) for d in (t.shape if t.shape is not None else []))
      ttype = schema.TensorType(t.type)
      if ttype == schema.TensorType.BOOL:
        sample[arg] = rng.choice([True, False], size=shape, replace=True).astype(np.bool_)
      elif ttype in (schema.TensorType.FLOAT32, schema.TensorType.BFLOAT16):
        sample[arg] = rng.normal(size=shape).astype(np.float32)
      else:
        dtype = np.dtype(schema.NUMPY_DTYPE.get(ttype, ""))
        if not np.issubdtype(dtype, np.integer):
          raise ValueError(f"Unsupported dtype: {dtype}")
        sample[arg] = rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, size=shape, dtype=dtype, endpoint=True)
    dataset.append(sample)
  return dataset


def compare_model(reference_model: bytes, target_model: bytes,
                  test_data: Optional[dict[str, Iterable[dict[str, Any]]]] = None,
                  error_metrics: Optional[Sequence[validation_utils.ValidationErrorMetric]] = None,
                  compare_fns: Optional[Sequence[Callable[[Any, Any], float]]] = None,
                  use_xnnpack: bool = True, num_threads: int = 16, validate_output_tensors_only: bool = False,
                  *, run_signature: Optional[RunSignature] = None) -> ComparisonResult:
  """Compares the model's tensors over its signatures (ref: model_validator.py:282-409).

  Constants are compared straight from the flatbuffers (no run). Inputs, outputs and intermediates come
  from `run_signature(model_bytes, signature_key, inputs) -> {tensor name: array}`, called once per model
  and sample; without it only the constants are filled. `use_xnnpack` / `num_threads` belong to the
  caller's interpreter and are ignored here.
  """
  del use_xnnpack, num_threads
  # (a memoryview of a mapped model file stays one: its constants are views of the mapping, which runtime.to_device
  # reads from the file through the pinned upload ring when the file is large enough; bytes would copy the model)
  if not isinstance(reference_model, (bytes, memoryview)):
    reference_model = bytes(reference_model)
  if not isinstance(target_model, (bytes, memoryview)):
    target_model = bytes(target_model)
  if error_metrics is None:
    error_metrics = [validation_utils.ValidationErrorMetric.MSE]
  if compare_fns is None:
    compare_fns = [validation_utils.get_validation_func(metric) for metric in error_metrics]
  if len(error_metrics) != len(compare_fns):
    raise ValueError("The number of error metrics must match the number of compare functions.")
  default_fns = all(fn is validation_utils.get_validation_func(mt) for mt, fn in zip(error_metrics, compare_fns))
  if run_signature is None and validate_output_tensors_only:
    raise ValueError(
        "validate_output_tensors_only needs the model's output tensors, which only a run of the model gives:"
        " pass run_signature=(model_bytes, signature_key, inputs) -> {tensor name: array}.")
  if test_data is None:
    keys = signature_keys(reference_model)
    test_data = ({k: create_random_normal_input_data(reference_model, k) for k in keys} if run_signature
                 else {k: [] for k in keys})

  def _compare(pairs):
    if default_fns:
      vals = validation_utils.compare_all_batched(pairs, error_metrics)
      return [[v[mt] for mt in error_metrics] for v in vals]
    return [[fn(t, r) for fn in compare_fns] for t, r in pairs]

  result = ComparisonResult(reference_model, target_model)
  for signature_key, signature_inputs in test_data.items():
    samples = list(signature_inputs)
    per_tensor: dict[str, list[list[float]]] = {}
    constants = {}
    if not validate_output_tensors_only:
      plans = constant_plans(reference_model, target_model, signature_key)
      if plans:
        from . import runtime as rt
        vals = _compare([(_device_target(p), rt.to_device(p.reference)) for p in plans])
        constants = {p.name: v for p, v in zip(plans, vals)}
    out_names = set(get_output_tensor_names(reference_model, signature_key))
    # without a runner only the constants are filled (the samples need a run of both models)
    for sample in (samples if run_signature is not None else []):
      ref_run = run_signature(reference_model, signature_key, sample)
      tgt_run = run_signature(target_model, signature_key, sample)
      names = [nm for nm in ref_run if (nm in out_names or not validate_output_tensors_only)]
      pairs, keep = [], []
      for nm in names:
        if nm in constants or nm not in tgt_run:
          continue
        r = np.asarray(ref_run[nm])
        if r.dtype == np.object_ or r.size == 0:
          continue
        pairs.append((tgt_run[nm], r))
        keep.append(nm)
      for nm, v in zip(keep, _compare(pairs) if pairs else []):
        per_tensor.setdefault(nm, []).append(v)
    # constants are computed once and aggregated as len(samples) identical values (the same float64 rounding)
    reps = max(1, len(samples))
    for nm, v in constants.items():
      per_tensor.setdefault(nm, []).extend([v] * reps)
    aggregated = {}
    for nm, rows in per_tensor.items():
      aggregated[nm] = {mt.value: float(np.mean([row[i] for row in rows])) for i, mt in enumerate(error_metrics)}
    result.add_new_signature_results(error_metrics, aggregated, signature_key, validate_output_tensors_only)
  return result


# ----------------------------------------------------------------------------- layer output error
# For a FULLY_CONNECTED op y = x W^T, with H = (2/n) X^T X over the calibration inputs (the statistic GPTQ calibration
# keeps per FULLY_CONNECTED input) and dW = W - dequant(W^):
#   (1/n) ||X dW^T||_F^2 = 1/2 tr(dW H dW^T) = 1/2 Sum_r d_r H d_r^T
# the layer's output error over the whole calibration set, with no run of the model (csrc/layer_error.hip).
_FULLY_CONNECTED = 9
SKIP_NO_HESSIAN = "no Hessian for the input"
SKIP_WEIGHT = "weight is not a constant 2-D tensor"
SKIP_ORDER = "Hessian order differs from the weight's reduction dimension"
SKIP_TARGET = "target constant missing or of another size"
SKIP_INPUT = "the quantized op reads a transformed input"


def _as_model(model) -> Any:
  return model if hasattr(model, "subgraphs") else _model(model)


def _fully_connected_ops(m, sg_index: int):
  """(op, input 0 name, weight tensor, output name) of every FULLY_CONNECTED op of a subgraph."""
  sg = m.subgraphs[sg_index]
  out = []
  for op in sg.operators or []:
    if int(m.operatorCodes[op.opcodeIndex].builtinCode) != _FULLY_CONNECTED or len(op.inputs) < 2:
      continue
    out.append((op, schema.tensor_name(sg.tensors[op.inputs[0]]), sg.tensors[op.inputs[1]],
                schema.tensor_name(sg.tensors[op.outputs[0]])))
  return out


def layer_hessians(float_model, samples: Iterable[dict], signature_key: Optional[str] = None) -> dict[str, dict]:
  """{input tensor name: {"hessian": HessianAccumulator, "num_samples": n}} for every FULLY_CONNECTED op whose
  input 0 appears in `samples`, the {tensor name: array or device tensor} maps that `calibrate` takes. The same
  accumulators as GPTQ calibration: H = (2/n) X^T X, n = the samples' leading dimensions. For recipes whose
  calibration keeps no Hessians (min/max, OCTAV, MSE, ...)."""
  import torch
  from . import runtime as rt
  from .algorithms.uniform_quantize import gptq
  m = _as_model(float_model)
  sg_index, _ = _signature_subgraph(m, signature_key)
  names = {name for _, name, _, _ in _fully_connected_ops(m, sg_index)}
  out: dict[str, dict] = {}
  for sample in samples:
    for name in names:
      if name not in sample:
        continue
      x = rt.on_device(rt.resident_sample(sample[name]), torch.float32)
      n = int(x.shape[0]) if x.dim() > 0 else 1
      x2d = x.reshape(-1, x.shape[-1] if x.dim() > 0 else 1)
      entry = out.get(name)
      if entry is None:
        entry = out[name] = {"hessian": gptq.HessianAccumulator(x2d.shape[1]), "num_samples": 0}
      entry["hessian"].add(x2d, n)
      entry["num_samples"] += n
  for entry in out.values():
    entry["hessian"].finalize()
    entry["num_samples"] = np.array(entry["num_samples"])
  return out


_MUL, _RESHAPE, _CUSTOM = 18, 22, 32
_HADAMARD_CUSTOM_CODE = "aeq.hadamard_rotation"
_MAX_HADAMARD_SIZE = 16384
TRANSFORM_NONE, TRANSFORM_MULTIPLY, TRANSFORM_HADAMARD = "none", "multiply", "hadamard"


def _producers(sg) -> dict:
  """tensor index -> the op that writes it."""
  producers: dict[int, Any] = {}
  for op in sg.operators or []:
    for o in op.outputs:
      producers.setdefault(int(o), op)
  return producers


def _input_transform(m, sg, producers: dict, fc_op, x_name: str, d: int) -> Optional[tuple]:
  """(kind, multiplier or None, hadamard size) of the linear map between the float model's activation `x_name` and
  input 0 of the target FULLY_CONNECTED op `fc_op`, or None when its producer is none of the three inserted shapes:
  MUL(x, constant float32 [d]) (OSCAR), CUSTOM aeq.hadamard_rotation(x) with a vector of ones, and
  RESHAPE <- FULLY_CONNECTED(., H_h / sqrt(h)) <- RESHAPE(x) with exactly graph_edits' float32 matrix, the first
  RESHAPE to [-1, h] and the second back to x's shape. A fused activation or a bias on the MUL or on the rotation's
  FULLY_CONNECTED would make it another map: refused."""
  def plain(op) -> bool:
    """No fused activation function."""
    return int(getattr(op.builtinOptions, "fusedActivationFunction", 0) or 0) == 0

  def shape(index) -> Optional[list]:
    t = sg.tensors[index] if index >= 0 else None
    return None if t is None or t.shape is None else [int(v) for v in t.shape]

  def code(op) -> int:
    return int(m.operatorCodes[op.opcodeIndex].builtinCode)

  def name(index) -> Optional[str]:
    return schema.tensor_name(sg.tensors[index]) if index is not None and index >= 0 else None

  def constant_f32(index, count) -> Optional[np.ndarray]:
    if index < 0:
      return None
    t = sg.tensors[index]
    if t.type != schema.TensorType.FLOAT32 or not _has_data(m.buffers, t) or _numel(t) != count:
      return None
    return np.ascontiguousarray(_raw_bytes(m.buffers, t)).view(np.float32)[:count]

  def rotation(h: int) -> Optional[tuple]:
    if h < 1 or h & (h - 1) or h > _MAX_HADAMARD_SIZE or d % h:
      return None
    return (TRANSFORM_NONE, None, 0) if h == 1 else (TRANSFORM_HADAMARD, None, h)

  if code(fc_op) != _FULLY_CONNECTED or not len(fc_op.inputs) or fc_op.inputs[0] < 0:
    return None
  op = producers.get(int(fc_op.inputs[0]))
  if op is None:
    return None
  kind = code(op)
  if kind == _MUL and len(op.inputs) == 2 and plain(op):
    for a, b in ((0, 1), (1, 0)):
      if name(op.inputs[a]) == x_name:
        multiplier = constant_f32(int(op.inputs[b]), d)
        if multiplier is not None:
          return TRANSFORM_MULTIPLY, multiplier, 0
    return None
  if kind == _CUSTOM:
    custom = m.operatorCodes[op.opcodeIndex].customCode
    custom = custom.decode() if isinstance(custom, (bytes, bytearray)) else custom
    if custom != _HADAMARD_CUSTOM_CODE or not len(op.inputs) or name(op.inputs[0]) != x_name:
      return None
    try:
      options = flexbuffer.decode(bytes(bytearray(op.customOptions)))
      h = int(options["hadamard_size"])
      signs = list(options["random_binary_vector"])
    except (ValueError, KeyError, TypeError, IndexError):
      return None
    if len(signs) != h or any(v != 1 for v in signs):      # (the reference emits ones only: another vector, another map)
      return None
    return rotation(h)
  if kind == _RESHAPE and len(op.inputs):
    fc = producers.get(int(op.inputs[0]))
    if fc is None or code(fc) != _FULLY_CONNECTED or len(fc.inputs) < 2 or not plain(fc):
      return None
    if len(fc.inputs) > 2 and fc.inputs[2] >= 0:      # a bias
      return None
    pre = producers.get(int(fc.inputs[0]))
    if pre is None or code(pre) != _RESHAPE or not len(pre.inputs) or name(pre.inputs[0]) != x_name:
      return None
    matrix = sg.tensors[fc.inputs[1]] if fc.inputs[1] >= 0 else None
    if matrix is None or matrix.shape is None or len(matrix.shape) != 2 or matrix.shape[0] != matrix.shape[1]:
      return None
    h = int(matrix.shape[0])
    found = rotation(h)
    values = constant_f32(int(fc.inputs[1]), h * h)
    if found is None or values is None:
      return None
    x_shape, flat = shape(int(pre.inputs[0])), shape(int(fc.inputs[0]))
    if x_shape is None or flat is None or len(flat) != 2 or flat[1] != h or shape(int(fc.outputs[0])) != flat:
      return None
    if flat[0] * h != int(np.prod(x_shape)) or shape(int(op.outputs[0])) != x_shape or x_shape[-1] != d:
      return None
    want = graph_edits._sylvester_hadamard_f32(h)      # pylint: disable=protected-access
    if not np.array_equal(values.view(np.uint32), want.reshape(-1).view(np.uint32)):
      return None
    return found
  return None


class LayerErrorKernels:
  """The device side of compare_layer_outputs: where the operands live and the kernels."""

  def weight(self, values: np.ndarray):
    from . import runtime as rt
    return rt.to_device(values)

  def delta(self, reference, plan: ConstantPlan):
    from . import ops
    return ops.weight_delta(reference, _device_target(plan))

  def delta_transformed(self, reference, plan: ConstantPlan, d: int, multiplier, hadamard_size: int):
    """The delta of a weight stored in a transformed basis (ops.weight_delta_transformed): `multiplier` is the
    float32 [d] constant of an inserted MUL or None, `hadamard_size` the size of an inserted rotation or 0. Called
    only when compare_layer_outputs found such a transformation."""
    from . import ops
    from . import runtime as rt
    m = None if multiplier is None else rt.to_device(np.asarray(multiplier, np.float32))
    return ops.weight_delta_transformed(reference, _device_target(plan), d, m, hadamard_size)

  def hessian(self, stat):
    """(float32 [d, d] whose lower triangle is valid, alpha) with H = alpha * product."""
    import torch
    from . import runtime as rt
    form = stat.product_form() if hasattr(stat, "product_form") else None
    if form is not None:
      return form
    # a finished float64 Hessian (loaded, resumed): rounded to float32 once, on the device
    return rt.on_device(stat, torch.float64).to(torch.float32), 1.0

  def quadform(self, a, rows: int, d: int, product, alpha: float) -> np.ndarray:
    from . import ops
    return ops.quadform_rows(a.view(rows, d), product, alpha).cpu().numpy()


class LayerOutputComparison:
  """Per FULLY_CONNECTED op (keyed by its output tensor's name): how far the quantized weight moves the op's
  output over the calibration set. `results[name]` holds `weight`, `input`, `rows`, `d`, `signal`, `error`,
  `output_mse`, `output_snr` and `per_channel_error` (float64 [rows]), with `follow_input_transforms` also
  `input_transform` and `hadamard_size`; `skipped[name]` is the reason an op was not computed."""

  def __init__(self, signature_key: Optional[str] = None):
    self.signature_key = signature_key
    self.results: dict[str, dict] = {}
    self.skipped: dict[str, str] = {}

  def __getitem__(self, name: str) -> dict:
    return self.results[name]

  def __contains__(self, name: str) -> bool:
    return name in self.results

  def __iter__(self):
    return iter(self.results)

  def __len__(self) -> int:
    return len(self.results)

  def as_dict(self) -> dict:
    layers = {name: {k: v for k, v in r.items() if k != "per_channel_error"} for name, r in self.results.items()}
    return {"signature_key": self.signature_key, "layers": layers, "skipped": dict(self.skipped)}

  def save(self, save_folder: str, model_name: str) -> str:
    """`<model_name>_layer_output_errors.json`, without the per-channel arrays."""
    save_path = pathlib.Path(save_folder)
    os.makedirs(str(save_path), exist_ok=True)
    path = str(save_path / (model_name + "_layer_output_errors.json"))
    with open(path, "w") as fh:
      fh.write(json.dumps(self.as_dict()))
    return path


def compare_layer_outputs(reference_model, target_model, calibration_result: dict,
                          signature_key: Optional[str] = DEFAULT_SIGNATURE_KEY, *,
                          kernels: Optional[LayerErrorKernels] = None,
                          follow_input_transforms: bool = False) -> LayerOutputComparison:
  """Output error of every FULLY_CONNECTED op of the float model with a constant 2-D weight [rows, d].

  With H = calibration_result[input 0's name]["hessian"] = (2/n) X^T X and dW = W - dequant(W^), the target weight
  found BY NAME in the quantized model (so it does not matter whether a DEQUANTIZE op was inserted):
    error  = 1/2 Sum_r d_r H d_r^T = (1/n) ||X dW^T||_F^2        signal = the same form of W
    output_mse = error / rows     output_snr = (signal / rows) / (output_mse + 1e-9)
  (the convention of validation_utils.signal_to_noise_ratio). The cost does not depend on the number of calibration
  tokens, and a saved calibration result serves as well as a fresh one.

  This is the weight's contribution to the op's pre-activation output: bias and fused activation do not enter, and
  under static recipes the activations' own rounding is not included. Non-finite Hessians give non-finite results,
  which is no error.

  Ops whose quantized form reads a transformed activation (an inserted Hadamard rotation or OSCAR multiply) store
  their weight in the transformed basis and are reported in `.skipped` unless `follow_input_transforms` is set. Then
  the producer of the target op's input is looked at (_input_transform): both transformations are linear maps on the
  reduction dimension whose constants are in the quantized graph, y = (x * m) W^'T = x (W^ diag(m))^T and
  y = (x R) W^'T = x (W^ R)^T with R = blockdiag(H_h / sqrt(h)) symmetric, so the error is the same form against the
  same Hessian of the UNTRANSFORMED input with dW = W - dequant(W^) * m, or dW = W - rotate_h(dequant(W^))
  (kernels.delta_transformed). Every entry then also carries `input_transform` ("none", "multiply" or "hadamard")
  and `hadamard_size` (0 when none). A chain of two transformations, a rotation with another sign vector or matrix,
  or any other producer stays in `.skipped`.
  """
  kernels = kernels or LayerErrorKernels()
  ref, tgt = _as_model(reference_model), _as_model(target_model)
  sg_ref, _ = _signature_subgraph(ref, signature_key)
  sg_tgt, _ = _signature_subgraph(tgt, signature_key)
  tgt_sg = tgt.subgraphs[sg_tgt]
  by_name: dict[str, Any] = {}
  for t in tgt_sg.tensors:
    by_name.setdefault(schema.tensor_name(t), t)
  producer_input: dict[str, Optional[str]] = {}     # output tensor name -> name of its producer's input 0
  producer_op: dict[str, Any] = {}
  producers = _producers(tgt_sg) if follow_input_transforms else {}
  for op in tgt_sg.operators or []:
    first = schema.tensor_name(tgt_sg.tensors[op.inputs[0]]) if len(op.inputs) and op.inputs[0] >= 0 else None
    for o in op.outputs:
      producer_input.setdefault(schema.tensor_name(tgt_sg.tensors[o]), first)
      producer_op.setdefault(schema.tensor_name(tgt_sg.tensors[o]), op)
  out = LayerOutputComparison(signature_key)
  hessians: dict[str, tuple] = {}
  signals: dict[tuple, np.ndarray] = {}             # (weight name, input name) -> per-row signal
  resident: tuple = (None, None)                    # (weight name, its device copy): one float weight at a time
  for _, x_name, w, y_name in _fully_connected_ops(ref, sg_ref):
    w_name = schema.tensor_name(w)
    if (w.type != schema.TensorType.FLOAT32 or not _has_data(ref.buffers, w) or w.shape is None or len(w.shape) != 2):
      out.skipped[y_name] = SKIP_WEIGHT
      continue
    rows, d = int(w.shape[0]), int(w.shape[1])
    stat = (calibration_result.get(x_name) or {}).get("hessian") if calibration_result else None
    if stat is None:
      out.skipped[y_name] = SKIP_NO_HESSIAN
      continue
    if tuple(stat.shape) != (d, d):
      out.skipped[y_name] = SKIP_ORDER
      continue
    target = by_name.get(w_name)
    if target is None or not _has_data(tgt.buffers, target) or _numel(target) != rows * d:
      out.skipped[y_name] = SKIP_TARGET
      continue
    transform = (TRANSFORM_NONE, None, 0)
    if producer_input.get(y_name) != x_name:
      found = None
      if follow_input_transforms and y_name in producer_op:
        found = _input_transform(tgt, tgt_sg, producers, producer_op[y_name], x_name, d)
      if found is None:
        out.skipped[y_name] = SKIP_INPUT
        continue
      transform = found
    values = np.ravel(np.asarray(tfl_flatbuffer_utils.get_tensor_data(w, ref.buffers), np.float32))
    plan = _target_plan(w_name, values, tgt, target)
    if plan is None:
      out.skipped[y_name] = SKIP_TARGET
      continue
    if plan.kind in ("i4", "i2", "i8", "i16", "i32") and plan.dequantized and plan.scale is None:
      _read_blockwise_scales(plan, tgt, tgt_sg.tensors, target)
    if x_name not in hessians:
      hessians[x_name] = kernels.hessian(stat)
    product, alpha = hessians[x_name]
    if resident[0] != w_name:
      resident = (w_name, kernels.weight(values))
    w_dev = resident[1]
    if (w_name, x_name) not in signals:
      signals[(w_name, x_name)] = kernels.quadform(w_dev, rows, d, product, 0.5 * alpha)
    per_row_signal = signals[(w_name, x_name)]
    if transform[0] == TRANSFORM_NONE:
      delta = kernels.delta(w_dev, plan)
    else:
      delta = kernels.delta_transformed(w_dev, plan, d, transform[1], transform[2])
    per_channel = kernels.quadform(delta, rows, d, product, 0.5 * alpha)
    signal, error = float(np.sum(per_row_signal)), float(np.sum(per_channel))
    mse = error / rows
    out.results[y_name] = {"weight": w_name, "input": x_name, "rows": rows, "d": d, "signal": signal, "error": error,
                           "output_mse": mse, "output_snr": (signal / rows) / (mse + 1e-9),
                           "per_channel_error": per_channel}
    if follow_input_transforms:
      out.results[y_name].update(input_transform=transform[0], hadamard_size=transform[2])
  return out
