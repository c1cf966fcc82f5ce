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
from .utils import tflite_flatbuffer as tfl_flatbuffer
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


def _ops_of_kind(m, sg_index: int, builtin: int, present: tuple = (), activation: int = 0, constant: int = 1):
  """(op, input `activation` name, input `constant` tensor, output name) of every op of kind `builtin` of a subgraph that
  has those inputs, the ones numbered in `present` not absent (-1). The defaults are the positions of FULLY_CONNECTED,
  the two convolutions and BATCH_MATMUL; TRANSPOSE_CONV passes activation 2."""
  sg = m.subgraphs[sg_index]
  out = []
  for op in sg.operators or []:
    if (int(m.operatorCodes[op.opcodeIndex].builtinCode) != builtin or len(op.inputs) <= max(activation, constant, 1)
        or any(op.inputs[i] < 0 for i in present)):
      continue
    out.append((op, schema.tensor_name(sg.tensors[op.inputs[activation]]), sg.tensors[op.inputs[constant]],
                schema.tensor_name(sg.tensors[op.outputs[0]])))
  return out


def _fully_connected_ops(m, sg_index: int):
  """(op, input 0 name, weight tensor, output name) of every FULLY_CONNECTED op of a subgraph."""
  return _ops_of_kind(m, sg_index, _FULLY_CONNECTED)


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


# ----------------------------------------------------------------------------- integer execution
# compare_layer_outputs evaluates 1/2 tr(dW H dW^T): the weight's error alone. What a dynamic-range op adds by rounding
# every activation row to int8 at run time, what a static op adds by reading an int8 activation, and what a Hadamard
# rotation does to either cannot be written with the Hessian, because rounding X is no linear map of X. Here the
# quantized op is executed in integers on the calibration samples (csrc/qfc.hip) and compared with the float product.
_DEQUANTIZE, _QUANTIZE = 6, 114
MODE_STATIC, MODE_DYNAMIC, MODE_WEIGHT_ONLY = "static", "dynamic", "weight_only"
SKIP_INT16 = "the op reads an INT16 activation"
SKIP_WEIGHT_ZERO_POINT = "the weight has a non-zero zero point"
SKIP_FLOAT_TARGET = "the target weight is float"
SKIP_NO_SAMPLE = "no sample for the input"
SKIP_SAMPLE_SHAPE = "the sample's size is no multiple of the weight's reduction dimension"
SKIP_KIND = "the target weight is neither int8, int4 nor int2"
EXECUTION_CHUNK_ROWS = 4096
# `quantized_outputs`: why an executed static op has no final_* figures
FINAL_SKIP_OUTPUT = "the output tensor is not INT8 / INT16 (as the activation is) with one scale and no INT16 zero point"
FINAL_SKIP_BIAS = "the bias is no constant INT32 / INT64 vector of rows entries"
FINAL_SKIP_BIAS_RANGE = "the INT64 bias is beyond +-2^47"
FINAL_SKIP_FLOAT_BIAS = "the float model's bias is no constant float32 vector of rows entries"
FINAL_SKIP_ACTIVATION = "the fused activation is none of NONE, RELU, RELU_N1_TO_1 and RELU6"
FINAL_SKIP_WEIGHTS_FORMAT = "weightsFormat is not DEFAULT"
FINAL_SKIP_MULTIPLIER = "s_x s_w / s_y has no fixed-point multiplier within the op's shift range"


@dataclasses.dataclass
class OutputPlan:
  """What the integer epilogue of one static FULLY_CONNECTED op needs, read from the two models."""
  bits: int                          # 8 or 16
  bias: Optional[np.ndarray]         # int32 / int64 [rows] of the target op, or None
  float_bias: Optional[np.ndarray]   # float32 [rows] of the float op, or None
  multiplier: np.ndarray             # int32, 1 or rows entries
  shift: np.ndarray
  scale: float                       # s_y
  zero_point: int                    # zp_y
  act_min: int
  act_max: int
  fused: int                         # the target op's fused activation
  float_fused: int                   # the float op's


def _fc_option(op, field: str) -> int:
  return int(getattr(op.builtinOptions, field, 0) or 0) if op.builtinOptions is not None else 0


# `conv_2d`: CONV_2D ops beside the FULLY_CONNECTED ones
_CONV_2D = 3
_CONV_2D_OPTIONS_TYPE = 1      # Conv2DOptions in the BuiltinOptions union
SKIP_CONV_FILTER = "the filter is not a constant 4-D float32 tensor"
SKIP_CONV_GROUPS = "the filter's input channels differ from the sample's (grouped convolution)"
SKIP_CONV_OPTIONS = "a stride or dilation below 1, or an unknown padding"
SKIP_CONV_GEOMETRY = "no positive output size, or a reduction dimension above 65536"
SKIP_CONV_BLOCKWISE = "the filter has blockwise scales"
_CONV_OPTION_FIELDS = (("padding", "padding", "i8", 0), ("stride_w", "strideW", "i32", 0), ("stride_h", "strideH", "i32", 0),
                       ("fused_activation_function", "fusedActivationFunction", "i8", 0),
                       ("dilation_w_factor", "dilationWFactor", "i32", 1), ("dilation_h_factor", "dilationHFactor", "i32", 1))


def _table_options(op, fields: tuple, options_type: int, marker_attr: str) -> Optional[dict]:
  """The options table of an op as {name: int} over `fields`, (name, generated attribute, scalar code, default) in the
  schema's field order: from an OpaqueTableT (what the flatbuffer layer keeps) by field id, with the schema's defaults
  for absent fields, when the op's builtinOptionsType is `options_type`; from a decoded object that has `marker_attr`
  by the generated API's attribute names; every default for an op without options. None when the op carries the
  options of another op type."""
  o = op.builtinOptions
  if o is None:
    return {name: default for name, _, _, default in fields}
  if isinstance(o, tfl_flatbuffer.OpaqueTableT):
    if int(getattr(op, "builtinOptionsType", 0) or 0) != options_type:
      return None
    return {name: int(o.scalar(i, code, default)) for i, (name, _, code, default) in enumerate(fields)}
  if not hasattr(o, marker_attr):
    return None
  out = {}
  for name, attr, _, default in fields:
    v = getattr(o, attr, None)
    out[name] = default if v is None else int(v)
  return out


def _fused_option(options_reader):
  """An `option(op, field)` in _fc_option's form for an op kind whose options `options_reader` reads: its fused
  activation (-1 under another op's options); FC-only fields (weightsFormat) are default."""
  def option(op, field: str) -> int:
    if field != "fusedActivationFunction":
      return 0
    options = options_reader(op)
    return -1 if options is None else options["fused_activation_function"]
  return option


def conv_2d_options(op) -> Optional[dict]:
  """Conv2DOptions of a CONV_2D op as {padding (0 SAME, 1 VALID), stride_w, stride_h, fused_activation_function,
  dilation_w_factor, dilation_h_factor}, in the schema's field order (ids 0 to 5). The flatbuffer layer keeps the
  table as an OpaqueTableT, whose scalars are read by field id with the schema's defaults for absent fields (0, and 1
  for the dilations); a decoded object with the generated API's attribute names is read as well; an op without
  options has every default. None when the op carries the options of another op type."""
  return _table_options(op, _CONV_OPTION_FIELDS, _CONV_2D_OPTIONS_TYPE, "strideW")


_conv_option = _fused_option(conv_2d_options)      # (_fc_option for a CONV_2D)


def _conv_2d_ops(m, sg_index: int):
  """(op, input 0 name, filter tensor, output name) of every CONV_2D op of a subgraph."""
  return _ops_of_kind(m, sg_index, _CONV_2D, present=(1,))


# `depthwise_conv_2d`: DEPTHWISE_CONV_2D ops, executed by a direct convolution (csrc/dwconv.hip)
_DEPTHWISE_CONV_2D = 4
_DEPTHWISE_CONV_2D_OPTIONS_TYPE = 2      # DepthwiseConv2DOptions in the BuiltinOptions union
SKIP_DEPTHWISE_FILTER = "the filter is not a constant float32 [1, KH, KW, O] tensor"
SKIP_DEPTHWISE_MULTIPLIER = ("the filter's output channels are no multiple of the sample's channels, or the"
                             " depth_multiplier option is not their ratio")
SKIP_DEPTHWISE_KIND = "the target filter is not int8"
SKIP_DEPTHWISE_BLOCKWISE = "the depthwise filter has blockwise scales"
SKIP_DEPTHWISE_SCALE_AXIS = "the filter's per-channel scales are not along dimension 3"
SKIP_DEPTHWISE_MISMATCH = "the float op and the target op disagree about padding, strides, dilations or depth multiplier"
_DEPTHWISE_OPTION_FIELDS = (("padding", "padding", "i8", 0), ("stride_w", "strideW", "i32", 0),
                            ("stride_h", "strideH", "i32", 0), ("depth_multiplier", "depthMultiplier", "i32", 0),
                            ("fused_activation_function", "fusedActivationFunction", "i8", 0),
                            ("dilation_w_factor", "dilationWFactor", "i32", 1),
                            ("dilation_h_factor", "dilationHFactor", "i32", 1))


def depthwise_conv_2d_options(op) -> Optional[dict]:
  """DepthwiseConv2DOptions of a DEPTHWISE_CONV_2D op as {padding (0 SAME, 1 VALID), stride_w, stride_h,
  depth_multiplier, fused_activation_function, dilation_w_factor, dilation_h_factor}, in the schema's field order (ids
  0 to 6), read as conv_2d_options reads Conv2DOptions: from an OpaqueTableT by field id with the schema's defaults
  for absent fields (0, and 1 for the dilations; a depth_multiplier of 0 says nothing, converters leave it to the
  shapes), or from a decoded object with the generated API's attribute names; an op without options has every
  default. None when the op carries the options of another op type."""
  return _table_options(op, _DEPTHWISE_OPTION_FIELDS, _DEPTHWISE_CONV_2D_OPTIONS_TYPE, "depthMultiplier")


_depthwise_option = _fused_option(depthwise_conv_2d_options)      # (_conv_option for a DEPTHWISE_CONV_2D)


def _depthwise_conv_2d_ops(m, sg_index: int):
  """(op, input 0 name, filter tensor, output name) of every DEPTHWISE_CONV_2D op of a subgraph."""
  return _ops_of_kind(m, sg_index, _DEPTHWISE_CONV_2D, present=(0, 1))


# `transpose_conv`: TRANSPOSE_CONV ops, executed by sub-pixel phases on patch rows (csrc/conv_patches.hip). The op reads
# (output_shape, filter [O, KH, KW, I], activation, bias): the activation is input 2 and the bias input 3.
_TRANSPOSE_CONV = 67
_TRANSPOSE_CONV_OPTIONS_TYPE = 49      # TransposeConvOptions in the BuiltinOptions union
_TCONV_OUTPUT_SHAPE, _TCONV_FILTER, _TCONV_ACTIVATION, _TCONV_BIAS = 0, 1, 2, 3
SKIP_TCONV_OUTPUT_SHAPE = ("output_shape is not a constant INT32 [4] (the same in both models), or its batch / channels"
                           " disagree with the sample / filter")
SKIP_TCONV_UNREACHABLE = "output_shape is not reachable from the sample's H x W under the op's padding and strides"
SKIP_TCONV_STRIDE = "a stride exceeds the kernel: some output pixels have no tap"
SKIP_TCONV_MISMATCH = "the float op and the target op disagree about padding or strides"
SKIP_TCONV_FILTER_SCALES = "the target filter is not int8 with scales per tensor or per channel along dimension 0"
_TRANSPOSE_CONV_OPTION_FIELDS = (("padding", "padding", "i8", 0), ("stride_w", "strideW", "i32", 0),
                                 ("stride_h", "strideH", "i32", 0),
                                 ("fused_activation_function", "fusedActivationFunction", "i8", 0))


def transpose_conv_options(op) -> Optional[dict]:
  """TransposeConvOptions of a TRANSPOSE_CONV op as {padding (0 SAME, 1 VALID), stride_w, stride_h,
  fused_activation_function}, in the schema's field order (ids 0 to 3; the op has no dilation), read as
  conv_2d_options reads Conv2DOptions: from an OpaqueTableT by field id with the schema's defaults (0) for absent
  fields when the op's builtinOptionsType is 49, or from a decoded object with the generated API's attribute names
  (one that also has dilationWFactor is a convolution's); an op without options has every default. None when the op
  carries the options of another op type."""
  if op.builtinOptions is not None and hasattr(op.builtinOptions, "dilationWFactor"):
    return None
  return _table_options(op, _TRANSPOSE_CONV_OPTION_FIELDS, _TRANSPOSE_CONV_OPTIONS_TYPE, "strideW")


_transpose_conv_option = _fused_option(transpose_conv_options)      # (_conv_option for a TRANSPOSE_CONV)


def _transpose_conv_ops(m, sg_index: int):
  """(op, input 2 name, filter tensor, output name) of every TRANSPOSE_CONV op of a subgraph."""
  return _ops_of_kind(m, sg_index, _TRANSPOSE_CONV, present=(_TCONV_OUTPUT_SHAPE, _TCONV_FILTER, _TCONV_ACTIVATION),
                      activation=_TCONV_ACTIVATION)


# `batch_matmul`: BATCH_MATMUL ops, executed by the integer batched product (csrc/qbmm.hip)
_BATCH_MATMUL = 126
SKIP_BMM_RANK = "an operand has rank below 2, or the two operands disagree about K"
SKIP_BMM_BATCH = ("the batch dimensions are neither equal nor a right-hand batch product of 1 (general broadcasting is"
                  " not built)")
SKIP_BMM_KIND = "the target constant is not int8"
SKIP_BMM_BLOCKWISE = "the constant has blockwise scales"
SKIP_BMM_SCALE_AXIS = "the constant's per-channel scales are not along its output axis"
SKIP_BMM_DYNAMIC_ADJ_X = "a dynamic-range op with adjX: the per-row scales would lie along K"
SKIP_BMM_MISMATCH = "the float op and the target op disagree about adjX or adjY, or one carries another op's options"
SKIP_BMM_K = "K exceeds 32768 (the int32 accumulator)"
SKIP_BMM_FLOAT = "the target op is a float op (not quantized)"
OPERANDS_CONSTANT, OPERANDS_ACTIVATIONS = "constant", "activations"


def batch_matmul_options(op) -> Optional[dict]:
  """BatchMatMulOptions of a BATCH_MATMUL op as {adj_x, adj_y, asymmetric_quantize_inputs} (booleans; the schema's
  defaults, False, for absent fields and for an op without options). None when the op carries the options of another
  op type."""
  o = op.builtinOptions
  if o is None:
    return {"adj_x": False, "adj_y": False, "asymmetric_quantize_inputs": False}
  if not hasattr(o, "adjX") or not hasattr(o, "adjY"):
    return None
  return {"adj_x": bool(o.adjX), "adj_y": bool(o.adjY),
          "asymmetric_quantize_inputs": bool(getattr(o, "asymmetricQuantizeInputs", False))}


def _batch_matmul_ops(m, sg_index: int):
  """(op, lhs tensor, rhs tensor, output name) of every BATCH_MATMUL op of a subgraph."""
  sg = m.subgraphs[sg_index]
  return [(op, sg.tensors[op.inputs[0]], rhs, y_name)
          for op, _, rhs, y_name in _ops_of_kind(m, sg_index, _BATCH_MATMUL, present=(0, 1))]


def _bmm_geometry(a_shape, b_shape, adj_x: bool, adj_y: bool):
  """(batch, b_batch, M, K, N) of two operand shapes, or the SKIP_BMM_* reason they have none."""
  a_shape, b_shape = [int(v) for v in a_shape], [int(v) for v in b_shape]
  if len(a_shape) < 2 or len(b_shape) < 2:
    return SKIP_BMM_RANK
  k, m = (a_shape[-2], a_shape[-1]) if adj_x else (a_shape[-1], a_shape[-2])
  n, kb = (b_shape[-2], b_shape[-1]) if adj_y else (b_shape[-1], b_shape[-2])
  if k != kb:
    return SKIP_BMM_RANK
  batch, b_batch = int(np.prod(a_shape[:-2], dtype=np.int64)), int(np.prod(b_shape[:-2], dtype=np.int64))
  if a_shape[:-2] != b_shape[:-2] and b_batch != 1:
    return SKIP_BMM_BATCH
  if k > 32768:
    return SKIP_BMM_K
  return batch, (batch if a_shape[:-2] == b_shape[:-2] else 1), m, k, n


def _output_grid(y, bits: int):
  """(s_y, zp_y) of the output tensor `y` of a static op with `bits`-bit activations, or FINAL_SKIP_OUTPUT."""
  q = y.quantization
  want = schema.TensorType.INT16 if bits == 16 else schema.TensorType.INT8
  if y.type != want or q is None or q.scale is None or len(q.scale) != 1:
    return FINAL_SKIP_OUTPUT
  zp_y = int(q.zeroPoint[0]) if q.zeroPoint is not None and len(q.zeroPoint) else 0
  if (bits == 16 and zp_y != 0) or not -128 <= zp_y <= 127:
    return FINAL_SKIP_OUTPUT
  s_y = float(np.float32(q.scale[0]))
  if not (np.isfinite(s_y) and s_y > 0):
    return FINAL_SKIP_OUTPUT
  return s_y, zp_y


def _multiplier_table(s_x: float, w_scale: np.ndarray, s_y: float, bits: int):
  """(multiplier, shift), int32 with one entry per entry of `w_scale`: the fixed-point form of s_x s_w / s_y, in
  float64 from the float32 scales as they are stored; FINAL_SKIP_MULTIPLIER when one has none within the shift range
  of an op with `bits`-bit activations."""
  from . import ops
  lo, hi = ops.QFC_SHIFT_RANGE[bits]
  multiplier, shift = [], []
  for s_w in np.asarray(w_scale, np.float32).reshape(-1).tolist():
    try:
      m_r, e_r = ops.quantize_multiplier(float(np.float32(s_x)) * float(s_w) / s_y)
    except ValueError:
      return FINAL_SKIP_MULTIPLIER
    if not lo <= e_r <= hi:
      return FINAL_SKIP_MULTIPLIER
    multiplier.append(m_r)
    shift.append(e_r)
  return np.asarray(multiplier, np.int32), np.asarray(shift, np.int32)


def _output_plan(ref, ref_sg, ref_op, tgt, tgt_sg, fc, rows: int, bits: int, s_x: float, w_scale: np.ndarray,
                 option=_fc_option, bias_index: int = 2):
  """An OutputPlan, or the FINAL_SKIP_* reason there is none. `option(op, field)` reads an op's options
  (_conv_option for a CONV_2D and _depthwise_option for a DEPTHWISE_CONV_2D, whose FC-only fields are default).
  `bias_index`: the input that is the bias, 2 for every kind but TRANSPOSE_CONV (3)."""
  from . import ops
  if option(fc, "weightsFormat") != 0 or option(ref_op, "weightsFormat") != 0:
    return FINAL_SKIP_WEIGHTS_FORMAT
  fused, float_fused = option(fc, "fusedActivationFunction"), option(ref_op, "fusedActivationFunction")
  if fused not in ops.FUSED_ACTIVATION_NAMES or float_fused not in ops.FUSED_ACTIVATION_NAMES:
    return FINAL_SKIP_ACTIVATION
  grid = _output_grid(tgt_sg.tensors[fc.outputs[0]], bits)
  if isinstance(grid, str):
    return grid
  s_y, zp_y = grid
  # ---- the two biases
  def constant(m, sg, op, ttype) -> Any:
    """The op's bias input as a flat array of `ttype`, None when absent, False when it is something else."""
    if len(op.inputs) <= bias_index or op.inputs[bias_index] < 0:
      return None
    t = sg.tensors[op.inputs[bias_index]]
    if t.type != ttype or not _has_data(m.buffers, t) or _numel(t) != rows:
      return False
    return np.ascontiguousarray(_raw_bytes(m.buffers, t)).view(schema.NUMPY_DTYPE[ttype])[:rows].copy()
  bias = constant(tgt, tgt_sg, fc, schema.TensorType.INT64 if bits == 16 else schema.TensorType.INT32)
  if bias is False:
    return FINAL_SKIP_BIAS
  if bits == 16 and bias is not None and np.any((bias < -(1 << 47)) | (bias > (1 << 47))):
    return FINAL_SKIP_BIAS_RANGE
  float_bias = constant(ref, ref_sg, ref_op, schema.TensorType.FLOAT32)
  if float_bias is False:
    return FINAL_SKIP_FLOAT_BIAS
  if np.size(w_scale) not in (1, rows):
    return FINAL_SKIP_MULTIPLIER
  table = _multiplier_table(s_x, w_scale, s_y, bits)
  if isinstance(table, str):
    return table
  act_min, act_max = ops.activation_range(fused, s_y, zp_y, bits)
  return OutputPlan(bits, bias, float_bias, table[0], table[1], s_y, zp_y, act_min, act_max, fused, float_fused)


class LayerExecutionKernels:
  """The device side of compare_layer_execution: where the operands live and the kernels."""

  def sample(self, value, d: int):
    """A sample entry (array or device tensor of any rank) as float32 [n, d] rows."""
    import torch
    from . import runtime as rt
    x = rt.on_device(rt.resident_sample(value), torch.float32)
    return x.contiguous().view(-1, d)

  def weight(self, values: np.ndarray, rows: int, d: int):
    from . import runtime as rt
    return rt.to_device(values).view(rows, d)

  def target(self, plan: ConstantPlan):
    return _device_target(plan)

  def dequantized(self, target, rows: int, d: int):
    """float32 [rows, d]: the stored weight dequantized by the validators' rule (weight-only mode)."""
    import torch
    from . import ops
    from . import runtime as rt
    zeros = torch.zeros((rows * d,), dtype=torch.float32, device=rt.device())
    return torch.neg(ops.weight_delta(zeros, target)).view(rows, d)       # 0 - dq is exact

  def rows(self, x, first: int, count: int):
    return x[first:first + count]

  @staticmethod
  def _sample_as_it_is(value):
    """sample4d and sample_nd (two names, since stand-ins override them one by one)."""
    import torch
    from . import runtime as rt
    return rt.on_device(rt.resident_sample(value), torch.float32).contiguous()

  @staticmethod
  def _grid(scale: float, zero_point: int) -> tuple:
    """(float32 [1], int32 [1]) on the device: one scale and one zero point as ops.quantize / ops.dequantize read them."""
    import torch
    from . import runtime as rt
    return (torch.tensor([scale], dtype=torch.float32, device=rt.device()),
            torch.tensor([zero_point], dtype=torch.int32, device=rt.device()))

  def sample4d(self, value):
    """A rank-4 sample entry (array or device tensor) as a contiguous float32 [N, H, W, C] tensor (`conv_2d`)."""
    return self._sample_as_it_is(value)

  def patches(self, x, kernel: tuple, strides: tuple, dilations: tuple, padding: str, pad_value, first: int, count: int):
    """Rows first .. first + count - 1 of the [N OH OW, KH KW C] patch rows of x [N, H, W, C], in x's own type
    (float32, int8 or int16), padded taps holding `pad_value` (ops.conv_patches)."""
    from . import ops
    return ops.conv_patches(x, kernel[0], kernel[1], strides, dilations, padding, pad_value, first, count)

  def quantize_dynamic_images(self, x, patch_rows: int):
    """(q int8 [N, H, W, C], scale float32 [N patch_rows]): every image quantized as a whole, one scale per batch
    element (ops.qfc_quantize_rows on [N, H W C]), and the scale of every patch row, `patch_rows` per image in
    order: patch row t reads image t // patch_rows. The index is formed on the device."""
    import torch
    from . import ops
    n = int(x.shape[0])
    q, scale = ops.qfc_quantize_rows(x.view(n, -1))
    image = torch.arange(n * patch_rows, device=x.device) // patch_rows
    return q.view(x.shape), scale[image]

  # (`transpose_conv`: one sub-pixel phase (py, px) at a time; its rows are (n, qy, qx), QH QW per image)
  def tconv_patches(self, x, kernel: tuple, strides: tuple, padding: str, out_hw: tuple, phase: tuple, pad_value, first: int,
                    count: int):
    """Rows first .. first + count - 1 of the [N QH QW, |kys| |kxs| C] patch rows of `phase` of x [N, IH, IW, C], in
    x's own type, taps outside the image holding `pad_value` (ops.tconv_patches)."""
    from . import ops
    return ops.tconv_patches(x, kernel[0], kernel[1], strides, padding, out_hw, phase, pad_value, first, count)

  def image_scales(self, scale, rows_per_image: int, first: int, count: int):
    """float32 [count]: the scale of the image each of the rows first .. first + count - 1 belongs to, `rows_per_image`
    rows per image in order (`scale` has one entry per image). The index is formed on the device."""
    import torch
    return scale[torch.arange(first, first + count, device=scale.device) // rows_per_image]

  # (`depthwise_conv_2d`: x [N, H, W, C] float32 / int8 / int16; rows first .. first + count - 1 of the N OH OW output
  # rows as [count, O]; `kernel` (KH, KW); the filter is [KH KW, O], the stored bytes of TFLite's [1, KH, KW, O])
  def depthwise_float(self, x, w, kernel: tuple, depth_multiplier: int, strides: tuple, dilations: tuple, padding: str,
                      first: int, count: int):
    """float32 [count, O]: the float op's pre-bias product, every product and sum rounded, taps in order
    (ops.dwconv_forward on float32)."""
    from . import ops
    return ops.dwconv_forward(x, w, kernel[0], kernel[1], strides, dilations, padding, depth_multiplier, first=first,
                              count=count)

  def depthwise_forward(self, xq, x_scale, x_zero_point: int, target, kernel: tuple, depth_multiplier: int, strides: tuple,
                        dilations: tuple, padding: str, first: int, count: int):
    """float32 [count, O] of int8 activations, `x_scale` 1 or N entries (one per image) (ops.dwconv_forward)."""
    from . import ops
    return ops.dwconv_forward(xq, target, kernel[0], kernel[1], strides, dilations, padding, depth_multiplier,
                              x_scale=x_scale, x_zero_point=x_zero_point, first=first, count=count)

  def depthwise_forward16(self, xq, x_scale, target, kernel: tuple, depth_multiplier: int, strides: tuple, dilations: tuple,
                          padding: str, first: int, count: int):
    """float32 [count, O] of int16 activations (ops.dwconv_forward)."""
    from . import ops
    return ops.dwconv_forward(xq, target, kernel[0], kernel[1], strides, dilations, padding, depth_multiplier,
                              x_scale=x_scale, first=first, count=count)

  def depthwise_output(self, xq, x_zero_point: int, target, kernel: tuple, depth_multiplier: int, strides: tuple,
                       dilations: tuple, padding: str, bias, multiplier, shift, out_zero_point: int, act_min: int,
                       act_max: int, first: int, count: int):
    """int8 [count, O]: what the static int8 op stores (ops.dwconv_output)."""
    from . import ops
    return ops.dwconv_output(xq, x_zero_point, target, kernel[0], kernel[1], strides, dilations, padding, bias, multiplier,
                             shift, out_zero_point, act_min, act_max, depth_multiplier, first, count)

  def depthwise_output16(self, xq, target, kernel: tuple, depth_multiplier: int, strides: tuple, dilations: tuple,
                         padding: str, bias, multiplier, shift, act_min: int, act_max: int, first: int, count: int):
    """int16 [count, O]: what the static int16-activation op stores (ops.dwconv_output_i16)."""
    from . import ops
    return ops.dwconv_output_i16(xq, target, kernel[0], kernel[1], strides, dilations, padding, bias, multiplier, shift,
                                 act_min, act_max, depth_multiplier, first, count)

  # (`batch_matmul`: operands of rank 3, [batch, ., .], the right-hand one with a batch of 1 or the left's)
  def sample_nd(self, value):
    """A sample entry of any rank (array or device tensor) as a contiguous float32 tensor of its own shape."""
    return self._sample_as_it_is(value)

  def bmm_constant(self, plan: ConstantPlan, shape: tuple):
    """(int8 [b_batch, ., .], float32 scales): the stored integers and the scales of an int8 constant."""
    from . import runtime as rt
    return rt.to_device(np.ascontiguousarray(plan.data, np.int8)).view(shape), rt.to_device(np.asarray(plan.scale, np.float32))

  def bmm_float(self, a, b, adj_x: bool, adj_y: bool):
    """float32 [M, N] = op(a) op(b) of one batch slice (ops.gemm)."""
    from . import ops
    return ops.gemm(a, b, trans_a=adj_x, trans_b=adj_y)

  def bmm_forward(self, aq, bq, adj_x: bool, adj_y: bool, a_scale, a_zero_point: int, b_scale, b_zero_point: int):
    """float32 [batch, M, N] of two int8 operands with a zero point each (ops.qbmm_forward)."""
    from . import ops
    return ops.qbmm_forward(aq, bq, adj_x=adj_x, adj_y=adj_y, a_scale=a_scale, a_zero_point=a_zero_point, b_scale=b_scale,
                            b_zero_point=b_zero_point)

  def bmm_output(self, aq, bq, adj_x: bool, adj_y: bool, a_zero_point: int, b_zero_point: int, multiplier, shift,
                 out_zero_point: int):
    """int8 [batch, M, N]: what the static op stores (ops.qbmm_output)."""
    from . import ops
    return ops.qbmm_output(aq, bq, adj_x=adj_x, adj_y=adj_y, a_zero_point=a_zero_point, b_zero_point=b_zero_point,
                           multiplier=multiplier, shift=shift, out_zero_point=out_zero_point)

  def transform(self, x, kind: str, multiplier, hadamard_size: int):
    """The inserted op's own map on rows of length d: x * multiplier, or x R with R = blockdiag(H_h / sqrt(h))."""
    from . import ops
    from . import runtime as rt
    if kind == TRANSFORM_MULTIPLY:
      return x * rt.to_device(np.asarray(multiplier, np.float32))
    if kind == TRANSFORM_HADAMARD:
      return ops.hadamard_rotate(x.contiguous(), hadamard_size)
    return x

  def gemm(self, x, w):
    """float32 [n, rows] = x w^T."""
    from . import ops
    return ops.gemm(x, w, trans_b=True)

  def quantize_dynamic(self, x):
    from . import ops
    return ops.qfc_quantize_rows(x)

  def quantize_static(self, x, scale: float, zero_point: int):
    from . import ops
    s, zp = self._grid(scale, zero_point)
    return ops.quantize(x.contiguous(), 1, 1, x.numel(), s, zp, 8, False), s

  def forward(self, xq, x_scale, x_zero_point: int, target, rows: int, d: int):
    from . import ops
    return ops.qfc_forward(xq, x_scale, x_zero_point, target, rows, d)

  def quantize_static16(self, x, scale: float):
    """(q int16 [n, d], its one scale): q = clip(rint(x / s_x), -32768, 32767), symmetric, ops.quantize as it stands."""
    from . import ops
    s, zp = self._grid(scale, 0)
    return ops.quantize(x.contiguous(), 1, 1, x.numel(), s, zp, 16, False), s

  def forward16(self, xq, x_scale, target, rows: int, d: int):
    from . import ops
    return ops.qfc_forward_i16(xq, x_scale, target, rows, d)

  def bias(self, values: np.ndarray):
    """A bias vector (int32, int64 or float32 [rows]) where the kernels read it."""
    from . import runtime as rt
    return rt.to_device(np.ascontiguousarray(values))

  def output(self, xq, x_zero_point: int, target, rows: int, d: int, bias, multiplier, shift, out_zero_point: int,
             act_min: int, act_max: int):
    """int8 [n, rows]: what the static int8 op stores (ops.qfc_output)."""
    from . import ops
    return ops.qfc_output(xq, x_zero_point, target, rows, d, bias, multiplier, shift, out_zero_point, act_min, act_max)

  def output16(self, xq, target, rows: int, d: int, bias, multiplier, shift, act_min: int, act_max: int):
    """int16 [n, rows]: what the static int16-activation op stores (ops.qfc_output_i16)."""
    from . import ops
    return ops.qfc_output_i16(xq, target, rows, d, bias, multiplier, shift, act_min, act_max)

  def dequantize_output(self, q, scale: float, zero_point: int):
    """float32 [n, rows] = float32(q - zp_y) * s_y (ops.dequantize; the difference fits int16 for both types)."""
    from . import ops
    s, zp = self._grid(scale, zero_point)
    return ops.dequantize(q, 1, 1, q.numel(), s, zp, 16)

  def reference_output(self, y, bias, fused: int):
    """float32 [n, rows] = act(y + b) of the float op: one float32 addition, then the activation's clamp."""
    import torch
    from . import ops
    if bias is not None:
      y = y + bias
    if fused == ops.FUSED_RELU:
      return torch.clamp(y, min=0.0)
    if fused == ops.FUSED_RELU6:
      return torch.clamp(y, min=0.0, max=6.0)
    if fused == ops.FUSED_RELU_N1_TO_1:
      return torch.clamp(y, min=-1.0, max=1.0)
    return y

  def sqdiff(self, yq, y, sums):
    """(Sum_t (yq - y)^2, Sum_t y^2) per column, added onto `sums` (None: the first chunk)."""
    from . import ops
    return ops.sqdiff_cols(yq, y, out=sums)

  def host(self, sums) -> tuple:
    return sums[0].cpu().numpy(), sums[1].cpu().numpy()


class LayerExecutionComparison(LayerOutputComparison):
  """Per FULLY_CONNECTED op (keyed by its output tensor's name): how far the quantized op's integer execution is
  from the float product over the calibration samples. `results[name]` holds `weight`, `input`, `rows`, `d`,
  `tokens`, `mode` ("static", "dynamic" or "weight_only"), `signal`, `error`, `output_mse`, `output_snr` and
  `per_channel_error` (float64 [rows]), with `follow_input_transforms` also `input_transform` and `hadamard_size`,
  with `int16_activations` also `activation_bits` (8, 16, or None for dynamic and weight-only ops);
  with `quantized_outputs` also `output_bits` and, for a static op executed through to its stored output,
  `fused_activation`, `final_signal`, `final_error`, `final_output_mse`, `final_output_snr` and
  `final_per_channel_error`, or `final_skipped` with the reason there are none;
  with `conv_2d` also `op` ("FULLY_CONNECTED" or "CONV_2D"), and for a CONV_2D (rows = O, d = KH KW I, tokens = patch
  rows) `kernel`, `strides`, `dilations`, `padding` and `output_hw`;
  with `depthwise_conv_2d` also `op` (then also "DEPTHWISE_CONV_2D"), and for such an op the keys of a CONV_2D entry
  (rows = O, d = KH KW, tokens = output rows) and `depth_multiplier`;
  with `transpose_conv` also `op` (then also "TRANSPOSE_CONV"), and for such an op the keys of a CONV_2D entry without
  `dilations` (rows = O, d = KH KW I, tokens = output pixels) and `phases`;
  `skipped[name]` is the reason an op was not computed."""

  def as_dict(self) -> dict:
    out = super().as_dict()
    for entry in out["layers"].values():
      entry.pop("final_per_channel_error", None)
    return out

  def save(self, save_folder: str, model_name: str) -> str:
    """`<model_name>_layer_execution_errors.json`, without the per-channel arrays."""
    save_path = pathlib.Path(save_folder)
    os.makedirs(str(save_path), exist_ok=True)
    path = str(save_path / (model_name + "_layer_execution_errors.json"))
    with open(path, "w") as fh:
      fh.write(json.dumps(self.as_dict()))
    return path


def compare_layer_execution(reference_model, target_model, samples: Iterable[dict],
                            signature_key: Optional[str] = DEFAULT_SIGNATURE_KEY, *,
                            kernels: Optional[LayerExecutionKernels] = None,
                            follow_input_transforms: bool = False,
                            int16_activations: bool = False,
                            quantized_outputs: bool = False,
                            conv_2d: bool = False,
                            depthwise_conv_2d: bool = False,
                            batch_matmul: bool = False,
                            transpose_conv: bool = False) -> LayerExecutionComparison:
  """Executes every quantized FULLY_CONNECTED op in integers on the calibration samples and compares it with the
  float model's product, for every op of the float model with a constant 2-D float32 weight [rows, d] whose input 0
  is in `samples` (the {tensor name: array or device tensor} maps calibrate() takes; tensors of any rank are rows of
  length d). The target op is the producer of the same-named output in the quantized model, and its mode is read
  from the graph:
    "static"       input 0 is INT8 with quantization parameters: q = clip(rint(x / s_x + zp_x), -128, 127) with the
                   tensor's own (s_x, zp_x), ops.quantize as it stands;
    "dynamic"      input 0 is FLOAT32 and the op reads the integer weight itself: every row is quantized to int8 at
                   run time with s_x = max|row| / 127 (ops.qfc_quantize_rows);
    "weight_only"  the op reads a DEQUANTIZE of the integer weight: no activation rounding, Yq = X dequant(W^)^T in
                   float32, the direct measurement of what compare_layer_outputs derives from the Hessian.
  In the integer modes acc = Sum_k (q_x - zp_x) q_w is exact in int32 and Yq = float(acc) * (s_x * s_w), with one
  accumulator per block under blockwise scales (ops.qfc_forward). With Y = X W^T (ops.gemm) over n tokens in all:
    signal = (1/n) ||Y||^2     error = (1/n) ||Yq - Y||^2     per_channel_error[r] = (1/n) Sum_t (Yq - Y)[t, r]^2
    output_mse = error / rows     output_snr = (signal / rows) / (output_mse + 1e-9)
  the conventions of compare_layer_outputs. The sums are float64 and added in a fixed order, sample by sample and in
  chunks of at most 4096 rows: no [all tokens, rows] array exists.

  This is the pre-bias product: bias, fused activation and the requantization of the op's output do not enter, the
  boundary compare_layer_outputs draws. Skipped with a reason: an INT16 activation, a weight with a non-zero zero
  point, a float target weight, a missing sample, and an op behind an inserted Hadamard rotation or OSCAR multiply
  unless `follow_input_transforms` is set. Then X goes through the inserted op's own constant first
  (ops.hadamard_rotate, or the multiply; _input_transform) and the comparison is still against the float model's
  product of the untransformed input; every entry then also carries `input_transform` and `hadamard_size`.

  With `int16_activations` an op whose input 0 is INT16 (the a16w8 models of static_wi8_ai16) is executed as well,
  with mode "static": the tensor must have one scale, a zero point that is 0 or absent (INT16 activations are
  symmetric), and be a QUANTIZE of the float model's input or that input itself, in front of the integer weight
  itself; anything else about it is "the quantized op reads a transformed input". Then
  q = clip(rint(x / s_x), -32768, 32767) (ops.quantize, 16 bits), acc = Sum_k q q_w is exact in int64 and
  Yq = float32(float64(acc) * float64(s_x * s_w)) (ops.qfc_forward_i16), and every entry also carries
  `activation_bits`: 16, 8 for an INT8 activation, None for dynamic and weight-only ops.

  With `quantized_outputs` a static op is also executed THROUGH TO ITS STORED OUTPUT, the one tensor the next op
  reads: q_out = clamp(requantize(acc + bias) + zp_y, act_min, act_max) in integers (ops.qfc_output /
  ops.qfc_output_i16: the int32 / int64 bias constant of the op, the fixed-point multiplier of
  double(s_x) double(s_w[r]) / double(s_y) per channel from ops.quantize_multiplier, the output tensor's own
  (s_y, zp_y), the fused activation's integer range from ops.activation_range), Yq = s_y (q_out - zp_y)
  (ops.dequantize), and Y = act(X W^T + b) in float32 from the FLOAT model's own bias and fused activation. Every
  entry then carries `output_bits` (8, 16, or None for dynamic and weight-only ops), and an op executed so
  `fused_activation` (the name), `final_signal`, `final_error`, `final_output_mse`, `final_output_snr` and
  `final_per_channel_error`, formed from Yq and Y as the keys without the prefix are. It needs: an INT8 (INT16 under
  16-bit activations, zero point 0 or absent) output tensor with one scale; a bias that is absent or a constant
  INT32 (INT64, within +-2^47) vector of rows entries; a float bias that is absent or a constant float32 vector; a
  fused activation NONE, RELU, RELU_N1_TO_1 or RELU6; weightsFormat DEFAULT; multipliers within the op's shift range.
  Otherwise the pre-bias figures stay and the entry carries `final_skipped` (a FINAL_SKIP_* reason) and no final_*
  figure. Without the keyword nothing changes.

  With `conv_2d` every CONV_2D op of the float model is executed as well, whose filter is a constant float32
  [O, KH, KW, I] and whose input 0 has samples of rank 4, [N, H, W, I]. A TFLite filter's reduction dimension
  K = KH KW I is contiguous per output channel, so the filter is the [rows = O, d = K] weight above (per tensor or per
  channel along dimension 0; kinds i8 / i4 / i2) and the op is the same product on the [N OH OW, K] patch rows of the
  sample (ops.conv_patches, the geometry of ops.conv_geometry from the op's Conv2DOptions: conv_2d_options), gathered
  in chunks of at most 4096 rows, so that no [all patches, K] array exists. Y = patches(X, pad 0.0) W^T. The mode is
  read as for FULLY_CONNECTED. "static": the whole sample is quantized once with the tensor's (s_x, zp_x), 8 or 16
  bits, and the patches are gathered from the INTEGER tensor with pad element zp_x; since q(0.0) = zp_x these are the
  bits of quantizing float patches padded with 0.0, with one read of the sample instead of KH KW. "dynamic": one
  scale per batch element, every image quantized as a whole (ops.qfc_quantize_rows on [N, H W I]), int8 patches with
  pad 0, and patch row t takes the scale of image t // (OH OW). "weight_only": patches(X) dequant(W^)^T. With
  `quantized_outputs` the epilogue above runs on the patch rows, the fused activation read from Conv2DOptions; the
  output tensor [N, OH, OW, O] is the [n, O] rows as they stand. `follow_input_transforms` does not apply: a conv
  behind an inserted op is "the quantized op reads a transformed input". This is this library's definition, modelled
  on LiteRT's CONV_2D; agreement with LiteRT's kernels has not been checked. EVERY entry then carries `op`
  ("FULLY_CONNECTED" or "CONV_2D"), and a conv entry `rows` = O, `d` = K, `tokens` = the number of patch rows, and
  `kernel` [KH, KW], `strides` and `dilations` [h, w], `padding` ("SAME" / "VALID") and `output_hw` (of the first
  sample). Further skip reasons: SKIP_CONV_FILTER, SKIP_CONV_GROUPS (I differs from the sample's channels),
  SKIP_CONV_OPTIONS, SKIP_CONV_GEOMETRY, SKIP_CONV_BLOCKWISE, and SKIP_SAMPLE_SHAPE for a sample that is not rank 4.
  Without the keyword nothing changes.

  With `depthwise_conv_2d` every DEPTHWISE_CONV_2D op of the float model is executed as well, whose filter is a
  constant float32 [1, KH, KW, O] and whose input 0 has samples of rank 4, [N, H, W, C], with O a multiple of C: the
  depth multiplier is M = O / C and output channel oc reads input channel oc // M. Such a filter's reduction (its
  KH KW taps) is not contiguous per output channel and every output channel reads one input channel, so there are
  no patch rows and no shared product: the op is a direct convolution (ops.dwconv_forward, ops.dwconv_output,
  ops.dwconv_output_i16), in chunks of at most 4096 of its N OH OW output rows. The graph reading (the target filter,
  integer or behind a DEQUANTIZE; the activation's type and so the mode; the QUANTIZE producer) is CONV_2D's; the
  filter is int8 with scales per tensor or per channel along dimension 3. Y is the float32 loop
  (((0 + p_0) + p_1) ...) over the taps inside the image in ascending (kh, kw) order, p = fl32(x w), and under
  "weight_only" Yq is the same loop on the dequantized filter. "static": the sample is quantized once (8 or 16
  bits); a tap outside the image is skipped, which is what a pad element q(0.0) = zp_x adds. "dynamic": one scale per
  batch element, every image quantized as a whole. With `quantized_outputs` the epilogue above runs on the
  accumulator, the fused activation read from DepthwiseConv2DOptions (depthwise_conv_2d_options). An entry carries
  the keys of a conv entry with `op` = "DEPTHWISE_CONV_2D", `rows` = O, `d` = KH KW, `tokens` = the number of output
  rows, and `depth_multiplier`; EVERY entry carries `op` whenever either conv keyword is on. Further skip reasons:
  SKIP_DEPTHWISE_FILTER, SKIP_DEPTHWISE_MULTIPLIER (O is no multiple of C, or a non-zero depth_multiplier option
  that is not O / C), SKIP_DEPTHWISE_KIND, SKIP_DEPTHWISE_BLOCKWISE, SKIP_DEPTHWISE_SCALE_AXIS,
  SKIP_DEPTHWISE_MISMATCH (the two ops' options differ); the reasons of CONV_2D that apply keep their texts.
  Without the keyword nothing changes.

  With `batch_matmul` every BATCH_MATMUL op of the float model whose inputs are sampled is executed as well, by the
  integer batched product (ops.qbmm_forward, csrc/qbmm.hip); the target op is the producer of the same-named output,
  BatchMatMulOptions are read by batch_matmul_options and must agree. `operands` = "constant" (the float model's rhs is
  a constant float32 of rank >= 2): "static" (lhs INT8 with one scale and zero point, the int8 constant with scales per
  tensor or along its output axis, common_utils.get_bmm_weight_quantized_dim), "dynamic" (lhs FLOAT32, rows of
  [batch M, K] quantized by ops.qfc_quantize_rows; not with adjX) or "weight_only" (the constant behind a DEQUANTIZE:
  Yq is the float product with the dequantized constant). `operands` = "activations" (both inputs sampled): "static",
  both INT8 with one scale and a zero point of its own each, each the float input itself or a QUANTIZE of it: the place
  where two rounded activations multiply. Y is the float32 product of the float model's own operands (ops.gemm per
  batch slice), the errors go through ops.sqdiff_cols on [batch M, N] rows in chunks. An entry carries `op` =
  "BATCH_MATMUL", `operands`, `adj_x`, `adj_y`, `batch` (of the first sample), `rows` = N, `d` = K, `tokens` = Sum
  batch M, `mode`, `activation_bits`, and with `quantized_outputs` and an INT8 output with one scale `final_*` from
  ops.qbmm_output with ops.quantize_multiplier(s_a s_b[n] / s_y) (the op has neither bias nor fused activation), else
  `final_skipped`. Skipped with a SKIP_BMM_* reason: operands of rank < 2 or disagreeing about K; batch dimensions that
  are neither equal nor a right-hand product of 1; a constant that is not int8, has blockwise scales or scales off
  the output axis; a dynamic op with adjX; differing options; K > 32768; a float target op. INT16 inputs are
  SKIP_INT16, a constant with a zero point SKIP_WEIGHT_ZERO_POINT. The arithmetic is this library's own definition,
  modelled on LiteRT's BATCH_MATMUL; agreement with LiteRT's kernels is unchecked. Every entry carries `op` whenever
  this or a conv keyword is on.

  With `transpose_conv` every TRANSPOSE_CONV op of the float model is executed as well. The op reads (output_shape,
  filter, x, bias): its activation is input 2 and its bias input 3; the filter is a constant float32 [O, KH, KW, I],
  output_shape a constant INT32 [N, OH, OW, O] (the same in both models), and input 2 has samples of rank 4,
  [N, IH, IW, I]. With (pad_top, pad_left) the padding of the FORWARD convolution from the OUTPUT image back to the
  input (ops.tconv_geometry, from the op's TransposeConvOptions: transpose_conv_options; the op has no dilation),
    out[n, oy, ox, o] = Sum_{ky, kx, i} x[n, a, b, i] W[o, ky, kx, i]
  over the taps with (oy + pad_top - ky) % sh == 0 and a = (oy + pad_top - ky) / sh in [0, IH), likewise b. It is
  executed by SUB-PIXEL PHASES (ops.tconv_phases): the output pixels oy = qy sh + py, ox = qx sw + px of one phase all
  use the same taps kys x kxs, so the phase is the product above of its [N QH QW, |kys| |kxs| I] patch rows
  (ops.tconv_patches) with the filter slice W[:, kys][:, :, kxs], a [rows = O, |kys| |kxs| I] weight whose per-channel
  scales along dimension 0 are untouched by the slice; gathering full KH KW I rows over a zero-stuffed input instead
  would multiply sh sw - 1 of every sh sw taps by nothing. The float filter and the stored integers are sliced per
  phase on the host, once; the op then runs phase by phase, each in chunks of at most 4096 rows, and every chunk's
  sums are added into the op's one set of float64 sums in that fixed order. Y = patches(X, pad 0.0) slice^T. The mode
  is read as for CONV_2D. "static": the whole sample is quantized once with the tensor's (s_x, zp_x), 8 or 16 bits,
  and every phase gathers from the INTEGER tensor with pad element zp_x. "dynamic": one scale per batch element,
  every image quantized as a whole, and every row of every phase takes its image's scale. "weight_only":
  patches(X) dequant(slice)^T. With `quantized_outputs` the unchanged epilogue runs on each phase's rows (the bias is
  input 3, the fused activation read from TransposeConvOptions) and the final sums are added the same way; no
  interleaved output tensor is formed. The filter is int8, per tensor or per channel along dimension 0. This is the
  library's own definition, modelled on LiteRT's TRANSPOSE_CONV and unchecked against it. An entry carries the keys of
  a conv entry with `op` = "TRANSPOSE_CONV", `rows` = O, `d` = KH KW I, `tokens` = Sum N OH OW, `output_hw`, no
  `dilations`, and `phases` (the number executed); EVERY entry carries `op` whenever this keyword is on. Further skip
  reasons: SKIP_TCONV_OUTPUT_SHAPE (output_shape is no constant INT32 [4], or its batch / channels disagree with the
  sample / filter), SKIP_TCONV_UNREACHABLE (output_shape is not reachable from the sample's H x W under the op's
  padding and strides), SKIP_TCONV_STRIDE (a stride exceeds the kernel, so some output pixels have no tap),
  SKIP_TCONV_MISMATCH (the options differ between the two models), SKIP_TCONV_FILTER_SCALES (the filter is not int8,
  is blockwise, or has scales off dimension 0); the reasons of CONV_2D that apply keep their texts. Without the
  keyword nothing changes.
"""
  ref, tgt = _as_model(reference_model), _as_model(target_model)
  sg_ref, _ = _signature_subgraph(ref, signature_key)
  sg_tgt, _ = _signature_subgraph(tgt, signature_key)
  graph = _TargetGraph.of(tgt, tgt.subgraphs[sg_tgt])
  run = _ExecutionRun(ref, sg_ref, list(samples), kernels or LayerExecutionKernels(), follow_input_transforms,
                      int16_activations, quantized_outputs,
                      op_key=conv_2d or depthwise_conv_2d or batch_matmul or transpose_conv)
  out = LayerExecutionComparison(signature_key)
  _fully_connected_entries(out, graph, run)
  if conv_2d:
    _conv_2d_entries(out, graph, run)
  if depthwise_conv_2d:
    _depthwise_conv_2d_entries(out, graph, run)
  if batch_matmul:
    _batch_matmul_entries(out, graph, run)
  if transpose_conv:
    _transpose_conv_entries(out, graph, run)
  return out


@dataclasses.dataclass
class _TargetGraph:
  """The quantized model's subgraph as the readers below walk it."""
  tgt: Any
  tgt_sg: Any
  producers: dict        # tensor index -> the op that writes it
  producer_op: dict      # output tensor name -> the op that writes it

  @classmethod
  def of(cls, tgt, tgt_sg) -> "_TargetGraph":
    producer_op: dict[str, Any] = {}
    for op in tgt_sg.operators or []:
      for o in op.outputs:
        producer_op.setdefault(schema.tensor_name(tgt_sg.tensors[o]), op)
    return cls(tgt, tgt_sg, _producers(tgt_sg), producer_op)

  def code(self, op) -> int:
    return int(self.tgt.operatorCodes[op.opcodeIndex].builtinCode)

  def name(self, index) -> Optional[str]:
    return schema.tensor_name(self.tgt_sg.tensors[index]) if index is not None and index >= 0 else None


@dataclasses.dataclass(frozen=True)
class _ExecutionRun:
  """What one call of compare_layer_execution gives every op: the float model, the samples, the kernels, the keywords."""
  ref: Any
  sg_ref: int
  samples: list
  kernels: LayerExecutionKernels
  follow_input_transforms: bool
  int16_activations: bool
  quantized_outputs: bool
  op_key: bool           # every entry carries `op` (a keyword of another op kind is on)


_FLOAT_TYPES = (schema.TensorType.FLOAT32, schema.TensorType.FLOAT16, schema.TensorType.BFLOAT16)
_NO_TRANSFORM = (TRANSFORM_NONE, None, 0)


# ---- what the graph says about one op: each reader returns its value, or the SKIP_* reason there is none
def _record(out: LayerExecutionComparison, y_name: str, entry) -> None:
  if isinstance(entry, str):
    out.skipped[y_name] = entry
  else:
    out.results[y_name] = entry


def _target_op(graph: _TargetGraph, y_name: str, builtin: int, needed: tuple = (0, 1)):
  """The target op of kind `builtin` that writes `y_name` and has the inputs `needed` (0 and 1; TRANSPOSE_CONV passes
  0, 1 and 2), or None."""
  op = graph.producer_op.get(y_name)
  if op is None or graph.code(op) != builtin or len(op.inputs) <= max(needed) or any(op.inputs[i] < 0 for i in needed):
    return None
  return op


def _target_constant(graph: _TargetGraph, op, name: str, count: int, float_reason: str = SKIP_FLOAT_TARGET):
  """(tensor, through_dequantize) of the constant that input 1 of the target op reads: the integer constant itself, or
  a DEQUANTIZE of it. It bears the float constant's `name`, has data and `count` elements.
  `float_reason`: BATCH_MATMUL passes SKIP_BMM_FLOAT, the other kinds SKIP_FLOAT_TARGET."""
  tgt, tensors = graph.tgt, graph.tgt_sg.tensors
  target, through_dequantize = tensors[op.inputs[1]], False
  if not _has_data(tgt.buffers, target):
    deq = graph.producers.get(int(op.inputs[1]))
    if not (deq is not None and graph.code(deq) == _DEQUANTIZE and len(deq.inputs) and deq.inputs[0] >= 0):
      return SKIP_TARGET
    target, through_dequantize = tensors[deq.inputs[0]], True
  if schema.tensor_name(target) != name or not _has_data(tgt.buffers, target) or _numel(target) != count:
    return SKIP_TARGET
  if target.type in _FLOAT_TYPES:
    return float_reason
  return target, through_dequantize


def _quantized_activation(graph: _TargetGraph, index: int, want_name: str, *, int16: bool, zero_point_range: bool = True):
  """(scale, zero point, bits) of the target tensor `index`: INT8 or INT16 with one scale, `want_name` itself or a
  QUANTIZE of it, an INT16 zero point 0 or absent.
  `int16`: FULLY_CONNECTED and the two convolutions pass `int16_activations`; BATCH_MATMUL passes False (its kernels
  are int8), so that an INT16 input is SKIP_INT16 whatever the keyword.
  `zero_point_range`: whether an INT8 zero point outside [-128, 127] is refused; FULLY_CONNECTED passes False (it has
  never checked), the other three kinds True."""
  t = graph.tgt_sg.tensors[index]
  if t.type == schema.TensorType.INT16 and not int16:
    return SKIP_INT16
  if t.type not in (schema.TensorType.INT8, schema.TensorType.INT16):
    return SKIP_INPUT
  q = t.quantization
  source = graph.name(index)
  quantize = graph.producers.get(int(index))
  if quantize is not None and graph.code(quantize) == _QUANTIZE and len(quantize.inputs):
    source = graph.name(quantize.inputs[0])
  if q is None or q.scale is None or len(q.scale) != 1 or source != want_name:
    return SKIP_INPUT
  zero_point = int(q.zeroPoint[0]) if q.zeroPoint is not None and len(q.zeroPoint) else 0
  bits = 16 if t.type == schema.TensorType.INT16 else 8
  if (bits == 16 and zero_point != 0) or (zero_point_range and not -128 <= zero_point <= 127):
    return SKIP_INPUT
  return float(np.float32(q.scale[0])), zero_point, bits


def _execution_mode(graph: _TargetGraph, op, x_name: str, through_dequantize: bool, *, int16: bool,
                    zero_point_range: bool = True, transforms_d: Optional[int] = None, dequantize_first: bool = False,
                    activation: int = 0):
  """(mode, (scale, zero point, bits) or None, input transform) of a target op whose input `activation` (0 for every
  kind but TRANSPOSE_CONV, which passes 2) stands for the float
  model's `x_name` and whose constant is read `through_dequantize` or not: a FLOAT32 input is "weight_only" behind a
  DEQUANTIZE and "dynamic" otherwise, a quantized one (_quantized_activation, which takes `int16` and
  `zero_point_range`) is "static" and goes with the integer constant itself.
  `transforms_d`: the reduction dimension when an inserted op in front of a float input is followed
  (_input_transform), None when it is not; FULLY_CONNECTED passes d under `follow_input_transforms`, the convolutions
  and BATCH_MATMUL never follow.
  `dequantize_first`: BATCH_MATMUL passes True, a quantized input in front of a DEQUANTIZE'd constant is SKIP_INPUT
  before its type is looked at; for the other kinds an INT16 input without `int16_activations` is SKIP_INT16 first."""
  index = op.inputs[activation]
  if graph.tgt_sg.tensors[index].type == schema.TensorType.FLOAT32:
    mode = MODE_WEIGHT_ONLY if through_dequantize else MODE_DYNAMIC
    if graph.name(index) == x_name:
      return mode, None, _NO_TRANSFORM
    found = None
    if transforms_d is not None:
      found = _input_transform(graph.tgt, graph.tgt_sg, graph.producers, op, x_name, transforms_d)
    return SKIP_INPUT if found is None else (mode, None, found)
  if through_dequantize and dequantize_first:
    return SKIP_INPUT
  quant = _quantized_activation(graph, index, x_name, int16=int16, zero_point_range=zero_point_range)
  if isinstance(quant, str):
    return quant
  return SKIP_INPUT if through_dequantize else (MODE_STATIC, quant, _NO_TRANSFORM)


def _constant_plan(graph: _TargetGraph, ref, w, target, kinds: tuple, kind_reason: str, blockwise_reason: Optional[str],
                   axis: Optional[tuple] = None, axis_reason: str = SKIP_TARGET, scale_count: bool = False):
  """(the float constant's values, the ConstantPlan of the integer constant `target`) for a constant of one of
  `kinds`, dequantized by scales, with no zero point.
  `blockwise_reason`: None reads blockwise scales (FULLY_CONNECTED); the other kinds pass their SKIP_*_BLOCKWISE.
  `axis`: the (channels, inner) view per-channel scales must have, None for any (FULLY_CONNECTED); its failure is
  `axis_reason` (CONV_2D keeps SKIP_TARGET). `scale_count`: the depthwise and BATCH_MATMUL readers also want one
  scale per channel; CONV_2D has never checked."""
  values = np.ravel(np.asarray(tfl_flatbuffer_utils.get_tensor_data(w, ref.buffers), np.float32))
  plan = _target_plan(schema.tensor_name(w), values, graph.tgt, target)
  if plan is None or not plan.dequantized:
    return SKIP_TARGET
  if plan.kind not in kinds:
    return kind_reason
  if plan.scale is None:
    if blockwise_reason is not None:
      return blockwise_reason
    _read_blockwise_scales(plan, graph.tgt, graph.tgt_sg.tensors, target)
  if axis is not None and (not (plan.channels == 1 or (plan.channels, plan.inner) == axis)
                           or (scale_count and np.asarray(plan.scale).size != plan.channels)):
    return axis_reason
  if plan.zero_point is not None and np.any(np.asarray(plan.zero_point) != 0):
    return SKIP_WEIGHT_ZERO_POINT
  return values, plan


_CONV_GEOMETRY_OPTIONS = ("padding", "stride_h", "stride_w", "dilation_h_factor", "dilation_w_factor")


def _conv_options(reader, conv, ref_op, also: tuple = (), mismatch_reason: str = SKIP_CONV_OPTIONS,
                  geometry: tuple = _CONV_GEOMETRY_OPTIONS):
  """(options, strides, dilations, padding name) of a convolution whose float and target op agree about the geometry
  and the fields `also` (else `mismatch_reason`: the depthwise op has one of its own), by `reader`. `geometry`: the
  option fields that make the geometry, padding first; TRANSPOSE_CONV has no dilations (they read as 1)."""
  from . import ops
  options, float_options = reader(conv), reader(ref_op)
  if options is None or float_options is None:
    return SKIP_CONV_OPTIONS
  if any(options[k] != float_options[k] for k in geometry + also):
    return mismatch_reason
  if options["padding"] not in ops.CONV_PADDING_NAMES or min(options[k] for k in geometry[1:]) < 1:
    return SKIP_CONV_OPTIONS
  return (options, (options["stride_h"], options["stride_w"]),
          (options.get("dilation_h_factor", 1), options.get("dilation_w_factor", 1)), ops.CONV_PADDING_NAMES[options["padding"]])


def _output_shapes(present: list, kernel: tuple, strides: tuple, dilations: tuple, padding: str, d: int, max_d: int):
  """ops.conv_geometry of every sample that is not empty; SKIP_CONV_GEOMETRY when one has none or d exceeds `max_d`,
  SKIP_NO_SAMPLE when every sample is empty."""
  from . import ops
  try:
    if d > max_d:
      raise ValueError("d")
    shapes = [ops.conv_geometry(int(v.shape[1]), int(v.shape[2]), kernel[0], kernel[1], strides, dilations, padding)
              for v in present if int(v.shape[0]) > 0]
  except ValueError:
    return SKIP_CONV_GEOMETRY
  return shapes or SKIP_NO_SAMPLE


# ---- the device side the three constant-weight kinds share
def _device_operands(graph: _TargetGraph, run: _ExecutionRun, ref_op, op, values, plan, shape: tuple, rows: int, mode: str,
                     quant, option):
  """(float weight, integer target, dequantized weight or None, OutputPlan / FINAL_SKIP_* / None, bias, float bias) on
  the device; `shape` is the weight's 2-D view, `option` the op kind's options reader for _output_plan."""
  kernels = run.kernels
  w_dev = kernels.weight(values, *shape)
  t_dev = kernels.target(plan)
  dq_dev = kernels.dequantized(t_dev, *shape) if mode == MODE_WEIGHT_ONLY else None
  return (w_dev, t_dev, dq_dev) + _final_operands(graph, run, ref_op, op, plan, rows, mode, quant, option)


def _final_operands(graph: _TargetGraph, run: _ExecutionRun, ref_op, op, plan, rows: int, mode: str, quant, option,
                    bias_index: int = 2):
  """(OutputPlan / FINAL_SKIP_* / None, bias, float bias), the two biases on the device (_output_plan)."""
  kernels = run.kernels
  final, bias_dev, float_bias_dev = None, None, None
  if run.quantized_outputs and mode == MODE_STATIC:
    final = _output_plan(run.ref, run.ref.subgraphs[run.sg_ref], ref_op, graph.tgt, graph.tgt_sg, op, rows, quant[2],
                         quant[0], plan.scale, option=option, bias_index=bias_index)
  if isinstance(final, OutputPlan):
    bias_dev = None if final.bias is None else kernels.bias(final.bias)
    float_bias_dev = None if final.float_bias is None else kernels.bias(final.float_bias)
  return final, bias_dev, float_bias_dev


def _quantize_static(kernels, x, quant: tuple):
  """(q, its one scale) of `x` on the static grid `quant` = (scale, zero point, bits)."""
  if quant[2] == 16:
    return kernels.quantize_static16(x, quant[0])
  return kernels.quantize_static(x, quant[0], quant[1])


def _forward(kernels, xq, x_scale, quant: Optional[tuple], t_dev, rows: int, d: int):
  """The integer product of quantized rows: int16 or int8 with the grid's zero point; `quant` None: dynamic rows."""
  if quant is not None and quant[2] == 16:
    return kernels.forward16(xq, x_scale, t_dev, rows, d)
  return kernels.forward(xq, x_scale, 0 if quant is None else quant[1], t_dev, rows, d)


def _stored_output(kernels, final: OutputPlan, xq, x_zero_point: int, t_dev, rows: int, d: int, bias_dev):
  """What the static op stores for the rows `xq` (FULLY_CONNECTED, and CONV_2D on patch rows)."""
  if final.bits == 16:
    return kernels.output16(xq, t_dev, rows, d, bias_dev, final.multiplier, final.shift, final.act_min, final.act_max)
  return kernels.output(xq, x_zero_point, t_dev, rows, d, bias_dev, final.multiplier, final.shift, final.zero_point,
                        final.act_min, final.act_max)


def _final_sqdiff(kernels, final: OutputPlan, q_out, y, float_bias_dev, final_sums):
  """`final_sums` with the stored output `q_out`, dequantized, against the float op's act(y + b)."""
  return kernels.sqdiff(kernels.dequantize_output(q_out, final.scale, final.zero_point),
                        kernels.reference_output(y, float_bias_dev, final.float_fused), final_sums)


# ---- an entry's figures
def _error_figures(kernels, sums, tokens: int, rows: int, prefix: str = "") -> dict:
  """signal, error, output_mse, output_snr and per_channel_error (each with `prefix`) of the sums over `tokens` rows."""
  sq_diff, sq_ref = kernels.host(sums)
  per_channel = np.asarray(sq_diff, np.float64) / tokens
  signal, error = float(np.sum(np.asarray(sq_ref, np.float64)) / tokens), float(np.sum(sq_diff) / tokens)
  mse = error / rows
  return {prefix + "signal": signal, prefix + "error": error, prefix + "output_mse": mse,
          prefix + "output_snr": (signal / rows) / (mse + 1e-9), prefix + "per_channel_error": per_channel}


def _finish_entry(entry: dict, run: _ExecutionRun, mode: str, activation_bits: Optional[int], transform: tuple, final,
                  final_sums, tokens: int, rows: int) -> dict:
  """The keys an entry carries by the keywords: `input_transform` / `hadamard_size`, `activation_bits`, and
  `output_bits` with the final_* figures of an OutputPlan `final`, or `final_skipped` with the reason `final`."""
  if run.follow_input_transforms:
    entry.update(input_transform=transform[0], hadamard_size=transform[2])
  if run.int16_activations:
    entry["activation_bits"] = activation_bits
  if run.quantized_outputs:
    entry["output_bits"] = activation_bits if mode == MODE_STATIC else None
    if isinstance(final, OutputPlan):
      from . import ops
      entry["fused_activation"] = ops.FUSED_ACTIVATION_NAMES[final.fused]
      entry.update(_error_figures(run.kernels, final_sums, tokens, rows, "final_"))
    elif final is not None:
      entry["final_skipped"] = final
  return entry


# ---- the five op kinds: each *_entry returns the op's entry, or the reason it has none
def _fully_connected_entries(out, graph: _TargetGraph, run: _ExecutionRun) -> None:
  for ref_op, x_name, w, y_name in _fully_connected_ops(run.ref, run.sg_ref):
    _record(out, y_name, _fully_connected_entry(graph, run, ref_op, x_name, w, y_name))


def _fully_connected_entry(graph: _TargetGraph, run: _ExecutionRun, ref_op, x_name: str, w, y_name: str):
  kernels, ref = run.kernels, run.ref
  if w.type != schema.TensorType.FLOAT32 or not _has_data(ref.buffers, w) or w.shape is None or len(w.shape) != 2:
    return SKIP_WEIGHT
  rows, d = int(w.shape[0]), int(w.shape[1])
  fc = _target_op(graph, y_name, _FULLY_CONNECTED)
  if fc is None:
    return SKIP_TARGET
  found = _target_constant(graph, fc, schema.tensor_name(w), rows * d)
  if isinstance(found, str):
    return found
  target, through_dequantize = found
  found = _execution_mode(graph, fc, x_name, through_dequantize, int16=run.int16_activations, zero_point_range=False,
                          transforms_d=d if run.follow_input_transforms else None)
  if isinstance(found, str):
    return found
  mode, quant, transform = found
  found = _constant_plan(graph, ref, w, target, ("i8", "i4", "i2"), SKIP_KIND, None)
  if isinstance(found, str):
    return found
  values, plan = found
  present = [s[x_name] for s in run.samples if x_name in s]
  if not present:
    return SKIP_NO_SAMPLE
  if any(int(np.prod(v.shape)) % d for v in present):
    return SKIP_SAMPLE_SHAPE
  w_dev, t_dev, dq_dev, final, bias_dev, float_bias_dev = _device_operands(
      graph, run, ref_op, fc, values, plan, (rows, d), rows, mode, quant, _fc_option)
  sums, final_sums, tokens = None, None, 0
  for value in present:
    x = kernels.sample(value, d)
    n = int(x.shape[0])
    for first in range(0, n, EXECUTION_CHUNK_ROWS):
      xc = kernels.rows(x, first, min(EXECUTION_CHUNK_ROWS, n - first))
      y = kernels.gemm(xc, w_dev)
      xt = xc if transform[0] == TRANSFORM_NONE else kernels.transform(xc, *transform)
      if mode == MODE_WEIGHT_ONLY:
        yq = kernels.gemm(xt, dq_dev)
      else:
        xq, x_scale = kernels.quantize_dynamic(xt) if mode == MODE_DYNAMIC else _quantize_static(kernels, xt, quant)
        yq = _forward(kernels, xq, x_scale, quant, t_dev, rows, d)
      sums = kernels.sqdiff(yq, y, sums)
      if isinstance(final, OutputPlan):
        q_out = _stored_output(kernels, final, xq, quant[1], t_dev, rows, d, bias_dev)
        final_sums = _final_sqdiff(kernels, final, q_out, y, float_bias_dev, final_sums)
    tokens += n
  if sums is None:          # (every sample of the input was empty)
    return SKIP_NO_SAMPLE
  entry = {"weight": schema.tensor_name(w), "input": x_name, "rows": rows, "d": d, "tokens": tokens, "mode": mode,
           **_error_figures(kernels, sums, tokens, rows)}
  _finish_entry(entry, run, mode, quant and quant[2], transform, final, final_sums, tokens, rows)
  if run.op_key:
    entry["op"] = "FULLY_CONNECTED"
  return entry


def _conv_2d_entries(out, graph: _TargetGraph, run: _ExecutionRun) -> None:
  """CONV_2D: the same product on patch rows (compare_layer_execution's section on `conv_2d`)."""
  for ref_op, x_name, w, y_name in _conv_2d_ops(run.ref, run.sg_ref):
    _record(out, y_name, _conv_2d_entry(graph, run, ref_op, x_name, w, y_name))


def _conv_2d_entry(graph: _TargetGraph, run: _ExecutionRun, ref_op, x_name: str, w, y_name: str):
  from . import ops
  kernels, ref = run.kernels, run.ref
  if (w.type != schema.TensorType.FLOAT32 or not _has_data(ref.buffers, w) or w.shape is None or len(w.shape) != 4
      or min(int(v) for v in w.shape) < 1):
    return SKIP_CONV_FILTER
  rows, kh, kw, channels = (int(v) for v in w.shape)
  d = kh * kw * channels
  conv = _target_op(graph, y_name, _CONV_2D)
  if conv is None:
    return SKIP_TARGET
  found = _conv_options(conv_2d_options, conv, ref_op)
  if isinstance(found, str):
    return found
  _, strides, dilations, padding = found
  found = _target_constant(graph, conv, schema.tensor_name(w), rows * d)
  if isinstance(found, str):
    return found
  target, through_dequantize = found
  found = _execution_mode(graph, conv, x_name, through_dequantize, int16=run.int16_activations)
  if isinstance(found, str):
    return found
  mode, quant, transform = found
  # the filter as a [O, K] constant: K = KH KW I is contiguous per output channel (scales along dimension 0)
  found = _constant_plan(graph, ref, w, target, ("i8", "i4", "i2"), SKIP_KIND, SKIP_CONV_BLOCKWISE, axis=(rows, d))
  if isinstance(found, str):
    return found
  values, plan = found
  present = [s[x_name] for s in run.samples if x_name in s]
  if not present:
    return SKIP_NO_SAMPLE
  if any(len(v.shape) != 4 for v in present):
    return SKIP_SAMPLE_SHAPE
  if any(int(v.shape[3]) != channels for v in present):
    return SKIP_CONV_GROUPS
  shapes = _output_shapes(present, (kh, kw), strides, dilations, padding, d, ops.QFC_MAX_D)
  if isinstance(shapes, str):
    return shapes
  w_dev, t_dev, dq_dev, final, bias_dev, float_bias_dev = _device_operands(
      graph, run, ref_op, conv, values, plan, (rows, d), rows, mode, quant, _conv_option)
  sums, final_sums, tokens = None, None, 0
  gather = (kh, kw), strides, dilations, padding
  for value in present:
    if int(value.shape[0]) == 0:
      continue
    x = kernels.sample4d(value)
    oh, ow, _, _ = ops.conv_geometry(int(x.shape[1]), int(x.shape[2]), kh, kw, strides, dilations, padding)
    n = int(x.shape[0]) * oh * ow
    # the whole sample is quantized ONCE and the patches are gathered from the integer tensor, padded with the zero
    # point: q(0.0) = zp_x, so these are the bits of quantizing float patches padded with 0.0
    if mode == MODE_DYNAMIC:
      xq_all, scale_rows = kernels.quantize_dynamic_images(x, oh * ow)
    elif mode == MODE_STATIC:
      xq_all, x_scale = _quantize_static(kernels, x, quant)
    pad = quant[1] if mode == MODE_STATIC and quant[2] == 8 else 0
    for first in range(0, n, EXECUTION_CHUNK_ROWS):
      count = min(EXECUTION_CHUNK_ROWS, n - first)
      xc = kernels.patches(x, *gather, 0.0, first, count)
      y = kernels.gemm(xc, w_dev)
      if mode == MODE_WEIGHT_ONLY:
        yq = kernels.gemm(xc, dq_dev)
      else:
        xq = kernels.patches(xq_all, *gather, pad, first, count)
        yq = _forward(kernels, xq, kernels.rows(scale_rows, first, count) if mode == MODE_DYNAMIC else x_scale, quant,
                      t_dev, rows, d)
      sums = kernels.sqdiff(yq, y, sums)
      if isinstance(final, OutputPlan):
        q_out = _stored_output(kernels, final, xq, quant[1], t_dev, rows, d, bias_dev)
        final_sums = _final_sqdiff(kernels, final, q_out, y, float_bias_dev, final_sums)
    tokens += n
  entry = {"op": "CONV_2D", "weight": schema.tensor_name(w), "input": x_name, "rows": rows, "d": d, "tokens": tokens,
           "mode": mode, "kernel": [kh, kw], "strides": list(strides), "dilations": list(dilations), "padding": padding,
           "output_hw": [shapes[0][0], shapes[0][1]], **_error_figures(kernels, sums, tokens, rows)}
  return _finish_entry(entry, run, mode, quant and quant[2], transform, final, final_sums, tokens, rows)


def _transpose_conv_entries(out, graph: _TargetGraph, run: _ExecutionRun) -> None:
  """TRANSPOSE_CONV: the same product, one sub-pixel phase at a time (compare_layer_execution's section on
  `transpose_conv`)."""
  for ref_op, x_name, w, y_name in _transpose_conv_ops(run.ref, run.sg_ref):
    _record(out, y_name, _transpose_conv_entry(graph, run, ref_op, x_name, w, y_name))


def _constant_output_shape(m, sg, op):
  """The four INT32 values of a TRANSPOSE_CONV op's constant output_shape (input 0), or None."""
  t = sg.tensors[op.inputs[_TCONV_OUTPUT_SHAPE]]
  if t.type != schema.TensorType.INT32 or not _has_data(m.buffers, t) or t.shape is None or list(t.shape) != [4]:
    return None
  return [int(v) for v in np.ascontiguousarray(_raw_bytes(m.buffers, t)).view(np.int32)[:4]]


def _transpose_conv_entry(graph: _TargetGraph, run: _ExecutionRun, ref_op, x_name: str, w, y_name: str):
  from . import ops
  kernels, ref = run.kernels, run.ref
  if (w.type != schema.TensorType.FLOAT32 or not _has_data(ref.buffers, w) or w.shape is None or len(w.shape) != 4
      or min(int(v) for v in w.shape) < 1):
    return SKIP_CONV_FILTER
  rows, kh, kw, channels = (int(v) for v in w.shape)
  d = kh * kw * channels
  tconv = _target_op(graph, y_name, _TRANSPOSE_CONV, needed=(_TCONV_OUTPUT_SHAPE, _TCONV_FILTER, _TCONV_ACTIVATION))
  if tconv is None:
    return SKIP_TARGET
  found = _conv_options(transpose_conv_options, tconv, ref_op, mismatch_reason=SKIP_TCONV_MISMATCH,
                        geometry=("padding", "stride_h", "stride_w"))
  if isinstance(found, str):
    return found
  _, strides, _, padding = found
  out_shape = _constant_output_shape(ref, ref.subgraphs[run.sg_ref], ref_op)
  if out_shape is None or out_shape != _constant_output_shape(graph.tgt, graph.tgt_sg, tconv) or out_shape[3] != rows:
    return SKIP_TCONV_OUTPUT_SHAPE
  out_hw = (out_shape[1], out_shape[2])
  found = _target_constant(graph, tconv, schema.tensor_name(w), rows * d)
  if isinstance(found, str):
    return found
  target, through_dequantize = found
  found = _execution_mode(graph, tconv, x_name, through_dequantize, int16=run.int16_activations,
                          activation=_TCONV_ACTIVATION)
  if isinstance(found, str):
    return found
  mode, quant, transform = found
  # the filter as a [O, K] constant, K = KH KW I contiguous per output channel: per-channel scales along dimension 0
  # stay what they are under a slice of the taps
  found = _constant_plan(graph, ref, w, target, ("i8",), SKIP_TCONV_FILTER_SCALES, SKIP_TCONV_FILTER_SCALES, axis=(rows, d),
                         axis_reason=SKIP_TCONV_FILTER_SCALES, scale_count=True)
  if isinstance(found, str):
    return found
  values, plan = found
  present = [s[x_name] for s in run.samples if x_name in s]
  if not present:
    return SKIP_NO_SAMPLE
  if any(len(v.shape) != 4 for v in present):
    return SKIP_SAMPLE_SHAPE
  if any(int(v.shape[3]) != channels for v in present):
    return SKIP_CONV_GROUPS
  present = [v for v in present if int(v.shape[0]) > 0]
  if not present:
    return SKIP_NO_SAMPLE
  if any(int(v.shape[0]) != out_shape[0] for v in present):
    return SKIP_TCONV_OUTPUT_SHAPE
  if d > ops.QFC_MAX_D or min(out_hw) < 1:
    return SKIP_CONV_GEOMETRY
  try:
    for v in present:
      ops.tconv_geometry(int(v.shape[1]), int(v.shape[2]), kh, kw, strides, padding, out_hw)
  except ValueError:
    return SKIP_TCONV_UNREACHABLE
  # (the forward convolution maps out_hw to ONE input size, so every sample has the first one's phases)
  phases = ops.tconv_phases(int(present[0].shape[1]), int(present[0].shape[2]), kh, kw, strides, padding, out_hw)
  if any(not kys or not kxs for *_, kys, kxs in phases):
    return SKIP_TCONV_STRIDE
  # the float filter and the stored integers, sliced per phase on the host, once
  w4, q4 = values.reshape(rows, kh, kw, channels), np.asarray(plan.data).reshape(rows, kh, kw, channels)
  w_dev, t_dev, dq_dev = [], [], []
  for *_, kys, kxs in phases:
    k_p = len(kys) * len(kxs) * channels
    w_p = np.ascontiguousarray(w4[:, list(kys)][:, :, list(kxs)]).reshape(-1)
    q_p = np.ascontiguousarray(q4[:, list(kys)][:, :, list(kxs)]).reshape(-1)
    w_dev.append(kernels.weight(w_p, rows, k_p))
    t_dev.append(kernels.target(dataclasses.replace(plan, reference=w_p, data=q_p, inner=k_p if plan.channels == rows else 1)))
    dq_dev.append(kernels.dequantized(t_dev[-1], rows, k_p) if mode == MODE_WEIGHT_ONLY else None)
  final, bias_dev, float_bias_dev = _final_operands(graph, run, ref_op, tconv, plan, rows, mode, quant, _transpose_conv_option,
                                                    bias_index=_TCONV_BIAS)
  sums, final_sums, tokens = None, None, 0
  pad = quant[1] if mode == MODE_STATIC and quant[2] == 8 else 0
  for value in present:
    x = kernels.sample4d(value)
    n_img = int(x.shape[0])
    # as for CONV_2D the whole sample is quantized ONCE and every phase gathers from the integer tensor, padded with the
    # zero point; a dynamic op has one scale per image, which every row of every phase of that image takes
    if mode == MODE_DYNAMIC:
      xq_all, image_scale = kernels.quantize_dynamic_images(x, 1)
    elif mode == MODE_STATIC:
      xq_all, x_scale = _quantize_static(kernels, x, quant)
    for p, (py, px, qh, qw, kys, kxs) in enumerate(phases):
      n, k_p = n_img * qh * qw, len(kys) * len(kxs) * channels
      gather = (kh, kw), strides, padding, out_hw, (py, px)
      for first in range(0, n, EXECUTION_CHUNK_ROWS):
        count = min(EXECUTION_CHUNK_ROWS, n - first)
        xc = kernels.tconv_patches(x, *gather, 0.0, first, count)
        y = kernels.gemm(xc, w_dev[p])
        if mode == MODE_WEIGHT_ONLY:
          yq = kernels.gemm(xc, dq_dev[p])
        else:
          xq = kernels.tconv_patches(xq_all, *gather, pad, first, count)
          scale = kernels.image_scales(image_scale, qh * qw, first, count) if mode == MODE_DYNAMIC else x_scale
          yq = _forward(kernels, xq, scale, quant, t_dev[p], rows, k_p)
        sums = kernels.sqdiff(yq, y, sums)
        if isinstance(final, OutputPlan):
          q_out = _stored_output(kernels, final, xq, quant[1], t_dev[p], rows, k_p, bias_dev)
          final_sums = _final_sqdiff(kernels, final, q_out, y, float_bias_dev, final_sums)
    tokens += n_img * out_hw[0] * out_hw[1]
  entry = {"op": "TRANSPOSE_CONV", "weight": schema.tensor_name(w), "input": x_name, "rows": rows, "d": d, "tokens": tokens,
           "mode": mode, "kernel": [kh, kw], "strides": list(strides), "padding": padding, "output_hw": list(out_hw),
           "phases": len(phases), **_error_figures(kernels, sums, tokens, rows)}
  return _finish_entry(entry, run, mode, quant and quant[2], transform, final, final_sums, tokens, rows)


def _depthwise_conv_2d_entries(out, graph: _TargetGraph, run: _ExecutionRun) -> None:
  """DEPTHWISE_CONV_2D: a direct convolution, no patch rows (compare_layer_execution's section on
  `depthwise_conv_2d`)."""
  for ref_op, x_name, w, y_name in _depthwise_conv_2d_ops(run.ref, run.sg_ref):
    _record(out, y_name, _depthwise_conv_2d_entry(graph, run, ref_op, x_name, w, y_name))


def _depthwise_conv_2d_entry(graph: _TargetGraph, run: _ExecutionRun, ref_op, x_name: str, w, y_name: str):
  from . import ops
  kernels, ref = run.kernels, run.ref
  if (w.type != schema.TensorType.FLOAT32 or not _has_data(ref.buffers, w) or w.shape is None or len(w.shape) != 4
      or int(w.shape[0]) != 1 or min(int(v) for v in w.shape) < 1):
    return SKIP_DEPTHWISE_FILTER
  _, kh, kw, rows = (int(v) for v in w.shape)
  d = kh * kw
  conv = _target_op(graph, y_name, _DEPTHWISE_CONV_2D)
  if conv is None:
    return SKIP_TARGET
  found = _conv_options(depthwise_conv_2d_options, conv, ref_op, ("depth_multiplier",), SKIP_DEPTHWISE_MISMATCH)
  if isinstance(found, str):
    return found
  options, strides, dilations, padding = found
  found = _target_constant(graph, conv, schema.tensor_name(w), rows * d)
  if isinstance(found, str):
    return found
  target, through_dequantize = found
  found = _execution_mode(graph, conv, x_name, through_dequantize, int16=run.int16_activations)
  if isinstance(found, str):
    return found
  mode, quant, transform = found
  # the filter as a [KH KW, O] constant, the stored bytes of [1, KH, KW, O]: scales along dimension 3 (O scales along
  # dimension 0, of size 1, are read as one and refused by their count)
  found = _constant_plan(graph, ref, w, target, ("i8",), SKIP_DEPTHWISE_KIND, SKIP_DEPTHWISE_BLOCKWISE, axis=(rows, 1),
                         axis_reason=SKIP_DEPTHWISE_SCALE_AXIS, scale_count=True)
  if isinstance(found, str):
    return found
  values, plan = found
  present = [s[x_name] for s in run.samples if x_name in s]
  if not present:
    return SKIP_NO_SAMPLE
  if any(len(v.shape) != 4 for v in present):
    return SKIP_SAMPLE_SHAPE
  channels = int(present[0].shape[3])
  if (channels < 1 or any(int(v.shape[3]) != channels for v in present) or rows % channels
      or options["depth_multiplier"] not in (0, rows // channels)):
    return SKIP_DEPTHWISE_MULTIPLIER
  multiplier = rows // channels
  shapes = _output_shapes(present, (kh, kw), strides, dilations, padding, d, ops.DWCONV_MAX_TAPS)
  if isinstance(shapes, str):
    return shapes
  w_dev, t_dev, dq_dev, final, bias_dev, float_bias_dev = _device_operands(
      graph, run, ref_op, conv, values, plan, (d, rows), rows, mode, quant, _depthwise_option)
  sums, final_sums, tokens = None, None, 0
  where = (kh, kw), multiplier, strides, dilations, padding
  for value in present:
    if int(value.shape[0]) == 0:
      continue
    x = kernels.sample4d(value)
    oh, ow, _, _ = ops.conv_geometry(int(x.shape[1]), int(x.shape[2]), kh, kw, strides, dilations, padding)
    n = int(x.shape[0]) * oh * ow
    # the sample is quantized ONCE; a tap outside the image is skipped, which is what a pad element q(0.0) = zp_x adds
    if mode == MODE_DYNAMIC:
      xq_all, x_scale = kernels.quantize_dynamic_images(x, 1)      # (one scale per image)
    elif mode == MODE_STATIC:
      xq_all, x_scale = _quantize_static(kernels, x, quant)
    for first in range(0, n, EXECUTION_CHUNK_ROWS):
      count = min(EXECUTION_CHUNK_ROWS, n - first)
      y = kernels.depthwise_float(x, w_dev, *where, first, count)
      if mode == MODE_WEIGHT_ONLY:
        yq = kernels.depthwise_float(x, dq_dev, *where, first, count)
      elif mode == MODE_STATIC and quant[2] == 16:
        yq = kernels.depthwise_forward16(xq_all, x_scale, t_dev, *where, first, count)
      else:
        yq = kernels.depthwise_forward(xq_all, x_scale, 0 if mode == MODE_DYNAMIC else quant[1], t_dev, *where, first, count)
      sums = kernels.sqdiff(yq, y, sums)
      # (the four depthwise calls stay here: sharing _stored_output would take a table of callables)
      if isinstance(final, OutputPlan):
        if final.bits == 16:
          q_out = kernels.depthwise_output16(xq_all, t_dev, *where, bias_dev, final.multiplier, final.shift, final.act_min,
                                             final.act_max, first, count)
        else:
          q_out = kernels.depthwise_output(xq_all, quant[1], t_dev, *where, bias_dev, final.multiplier, final.shift,
                                           final.zero_point, final.act_min, final.act_max, first, count)
        final_sums = _final_sqdiff(kernels, final, q_out, y, float_bias_dev, final_sums)
    tokens += n
  entry = {"op": "DEPTHWISE_CONV_2D", "weight": schema.tensor_name(w), "input": x_name, "rows": rows, "d": d,
           "tokens": tokens, "mode": mode, "kernel": [kh, kw], "strides": list(strides), "dilations": list(dilations),
           "padding": padding, "output_hw": [shapes[0][0], shapes[0][1]], "depth_multiplier": multiplier,
           **_error_figures(kernels, sums, tokens, rows)}
  return _finish_entry(entry, run, mode, quant and quant[2], transform, final, final_sums, tokens, rows)


def _batch_matmul_entries(out, graph: _TargetGraph, run: _ExecutionRun) -> None:
  """BATCH_MATMUL: the integer batched product (compare_layer_execution's section on `batch_matmul`)."""
  for ref_op, lhs, rhs, y_name in _batch_matmul_ops(run.ref, run.sg_ref):
    _record(out, y_name, _batch_matmul_entry(graph, run, ref_op, lhs, rhs, y_name))


def _bmm_output_plan(y, s_a: float, s_b: np.ndarray):
  """The OutputPlan of a static BATCH_MATMUL with the output tensor `y` (the op has neither bias nor fused
  activation), or the FINAL_SKIP_* reason there is none."""
  from . import ops
  grid = _output_grid(y, 8)
  if isinstance(grid, str):
    return grid
  table = _multiplier_table(s_a, s_b, grid[0], 8)
  if isinstance(table, str):
    return table
  act_min, act_max = ops.activation_range(ops.FUSED_NONE, grid[0], grid[1], 8)
  return OutputPlan(8, None, None, table[0], table[1], grid[0], grid[1], act_min, act_max, ops.FUSED_NONE, ops.FUSED_NONE)


def _batch_matmul_entry(graph: _TargetGraph, run: _ExecutionRun, ref_op, lhs, rhs, y_name: str):
  from .algorithms.utils import common_utils
  kernels, ref, tensors = run.kernels, run.ref, graph.tgt_sg.tensors
  a_name, b_name = schema.tensor_name(lhs), schema.tensor_name(rhs)
  constant = _has_data(ref.buffers, rhs)
  if constant and (rhs.type != schema.TensorType.FLOAT32 or rhs.shape is None or len(rhs.shape) < 2):
    return SKIP_BMM_RANK
  bmm = _target_op(graph, y_name, _BATCH_MATMUL)
  if bmm is None:
    return SKIP_TARGET
  options, float_options = batch_matmul_options(bmm), batch_matmul_options(ref_op)
  if options is None or float_options is None or any(options[k] != float_options[k] for k in ("adj_x", "adj_y")):
    return SKIP_BMM_MISMATCH
  adj_x, adj_y = options["adj_x"], options["adj_y"]
  b_quant = None
  if constant:
    found = _target_constant(graph, bmm, b_name, _numel(rhs), float_reason=SKIP_BMM_FLOAT)
    if isinstance(found, str):
      return found
    target, through_dequantize = found
    found = _execution_mode(graph, bmm, a_name, through_dequantize, int16=False, dequantize_first=True)
    if isinstance(found, str):
      return found
    mode, a_quant, _ = found
    # an int8 constant with scales per tensor or along its output axis
    b_shape = [int(v) for v in rhs.shape]
    axis = common_utils.get_bmm_weight_quantized_dim(np.empty(b_shape, np.int8), adj_y)
    inner = int(np.prod(b_shape[axis + 1:])) if axis + 1 < len(b_shape) else 1
    found = _constant_plan(graph, ref, rhs, target, ("i8",), SKIP_BMM_KIND, SKIP_BMM_BLOCKWISE, axis=(b_shape[axis], inner),
                           axis_reason=SKIP_BMM_SCALE_AXIS, scale_count=True)
    if isinstance(found, str):
      return found
    values, plan = found
    if mode == MODE_DYNAMIC and adj_x:
      return SKIP_BMM_DYNAMIC_ADJ_X
  else:
    if tensors[bmm.inputs[0]].type in _FLOAT_TYPES and tensors[bmm.inputs[1]].type in _FLOAT_TYPES:
      return SKIP_BMM_FLOAT
    a_quant = _quantized_activation(graph, bmm.inputs[0], a_name, int16=False)
    b_quant = _quantized_activation(graph, bmm.inputs[1], b_name, int16=False)
    bad = a_quant if isinstance(a_quant, str) else b_quant if isinstance(b_quant, str) else None
    if bad is not None:
      return bad
    mode = MODE_STATIC
  # ---- the samples and their geometry
  present = [s for s in run.samples if a_name in s and (constant or b_name in s)]
  if not present:
    return SKIP_NO_SAMPLE
  geometries = [_bmm_geometry(s[a_name].shape, rhs.shape if constant else s[b_name].shape, adj_x, adj_y) for s in present]
  bad = next((g for g in geometries if isinstance(g, str)), None)
  if bad is not None:
    return bad
  d, rows = geometries[0][3], geometries[0][4]
  if any(g[3] != d or g[4] != rows for g in geometries):
    return SKIP_SAMPLE_SHAPE
  # ---- the output grid (static ops, `quantized_outputs`)
  final, final_sums = None, None
  if run.quantized_outputs and mode == MODE_STATIC:
    s_b = np.asarray(plan.scale, np.float32).reshape(-1) if constant else np.array([b_quant[0]], np.float32)
    final = _bmm_output_plan(tensors[bmm.outputs[0]], a_quant[0], s_b)
  if constant:
    b_shape3 = (int(np.prod(b_shape[:-2], dtype=np.int64)), b_shape[-2], b_shape[-1])
    b_float = kernels.weight(values, b_shape3[0] * b_shape3[1], b_shape3[2]).reshape(b_shape3)
    t_dev = kernels.target(plan)
    if mode == MODE_WEIGHT_ONLY:
      b_deq = kernels.dequantized(t_dev, b_shape3[0] * b_shape3[1], b_shape3[2]).reshape(b_shape3)
    else:
      bq, b_scale = kernels.bmm_constant(plan, b_shape3)
  sums, tokens = None, 0
  for s, (batch, b_batch, m, _, _) in zip(present, geometries):
    if batch * m == 0:
      continue
    a = kernels.sample_nd(s[a_name])
    a3 = a.reshape((batch,) + tuple(a.shape[-2:]))
    if not constant:
      b_act = kernels.sample_nd(s[b_name])
      b_float = b_act.reshape((b_batch,) + tuple(b_act.shape[-2:]))
    # the sample is quantized ONCE, as the op sees it
    if mode == MODE_STATIC:
      aq, a_scale = kernels.quantize_static(a3, a_quant[0], a_quant[1])
      if not constant:
        bq, b_scale = kernels.quantize_static(b_float, b_quant[0], b_quant[1])
      zps = (a_quant[1], 0 if constant else b_quant[1])
      yq = kernels.bmm_forward(aq, bq, adj_x, adj_y, a_scale, zps[0], b_scale, zps[1])
      if isinstance(final, OutputPlan):
        q_out = kernels.bmm_output(aq, bq, adj_x, adj_y, zps[0], zps[1], final.multiplier, final.shift, final.zero_point)
        y_final = kernels.dequantize_output(q_out, final.scale, final.zero_point)
    elif mode == MODE_DYNAMIC:
      aq, a_scale = kernels.quantize_dynamic(a3.reshape(batch * m, d))
      yq = kernels.bmm_forward(aq.reshape(batch, m, d), bq, adj_x, adj_y, a_scale, 0, b_scale, 0)
    for i in range(batch):
      j = i if b_batch != 1 else 0
      y = kernels.bmm_float(a3[i], b_float[j], adj_x, adj_y)
      yq_i = kernels.bmm_float(a3[i], b_deq[j], adj_x, adj_y) if mode == MODE_WEIGHT_ONLY else yq[i]
      for first in range(0, m, EXECUTION_CHUNK_ROWS):
        count = min(EXECUTION_CHUNK_ROWS, m - first)
        y_c = kernels.rows(y, first, count)
        sums = kernels.sqdiff(kernels.rows(yq_i, first, count), y_c, sums)
        if isinstance(final, OutputPlan):
          final_sums = kernels.sqdiff(kernels.rows(y_final[i], first, count), y_c, final_sums)
    tokens += batch * m
  if sums is None:          # (every sample was empty)
    return SKIP_NO_SAMPLE
  activation_bits = 8 if mode == MODE_STATIC else None
  entry = {"op": "BATCH_MATMUL", "operands": OPERANDS_CONSTANT if constant else OPERANDS_ACTIVATIONS, "adj_x": adj_x,
           "adj_y": adj_y, "batch": geometries[0][0], "weight": b_name if constant else None, "input": a_name, "rows": rows,
           "d": d, "tokens": tokens, "mode": mode, **_error_figures(kernels, sums, tokens, rows),
           "activation_bits": activation_bits}
  if not constant:
    entry["input_b"] = b_name
  return _finish_entry(entry, run, mode, activation_bits, _NO_TRANSFORM, final, final_sums, tokens, rows)


# ----------------------------------------------------------------------------- sensitivity sweep
# Which layers can go to int4 or int2, and which must stay at int8? One walk over the float model gives the layer
# output error of every FULLY_CONNECTED op under several candidate configurations at once: the float weight and the
# Hessian product are on the device once per op, the candidates that are plain symmetric min/max fake-quantization
# come out of ONE read of the weight (csrc/sensitivity.hip), and all candidates' deltas of an op go through one
# stacked quadratic form, whose rows are independent.
_MIN_MAX_KEY = "min_max_uniform_quantize"
ROUTE_FUSED, ROUTE_GENERIC = "fused", "generic"
SKIP_BASIS = "the candidate stores the weight in a transformed basis"
_FUSED_BLOCKS = {"CHANNELWISE": 0, "BLOCKWISE_32": 32, "BLOCKWISE_64": 64, "BLOCKWISE_128": 128, "BLOCKWISE_256": 256}
_GENERIC_ALGORITHMS = (_MIN_MAX_KEY, "OCTAV", "MSE", "GPTQ")       # weight-side, stored in the untransformed basis


@dataclasses.dataclass(frozen=True)
class SweepCandidate:
  """One configuration of a sensitivity sweep: what a recipe entry's weight_tensor_config and algorithm_key say."""
  name: str
  num_bits: int
  granularity: Any
  algorithm_key: str = _MIN_MAX_KEY
  symmetric: bool = True
  algorithm_params: Optional[dict] = None

  @property
  def granularity_name(self) -> str:
    return str(getattr(self.granularity, "value", self.granularity))

  @property
  def algorithm_name(self) -> str:
    return str(getattr(self.algorithm_key, "value", self.algorithm_key))

  @property
  def block_size(self) -> int:
    g = self.granularity_name
    return int(g.split("_")[1]) if g.startswith("BLOCKWISE_") else 0

  def fused_block(self, d: int) -> Optional[int]:
    """The block argument of the fused kernel (0 = one scale per row), or None when the candidate is none of its."""
    if (not self.symmetric or self.algorithm_name != _MIN_MAX_KEY or int(self.num_bits) not in (2, 4, 8)
        or self.algorithm_params or self.granularity_name not in _FUSED_BLOCKS):
      return None
    block = _FUSED_BLOCKS[self.granularity_name]
    return None if block and d % block else block

  def bits_per_weight(self, rows: int, d: int) -> float:
    """num_bits plus the scale's share: float32 per row or per tensor, float16 per block."""
    g = self.granularity_name
    if g == "CHANNELWISE":
      return self.num_bits + 32.0 / d
    if g == "TENSORWISE":
      return self.num_bits + 32.0 / (rows * d)
    return self.num_bits + 16.0 / self.block_size

  def tensor_config(self):
    from . import qtyping
    return qtyping.TensorQuantizationConfig(
        num_bits=int(self.num_bits), symmetric=bool(self.symmetric),
        granularity=qtyping.QuantGranularity(self.granularity_name), algorithm_params=dict(self.algorithm_params or {}))


class SweepKernels(LayerErrorKernels):
  """The device side of sweep_layer_sensitivity, on top of compare_layer_outputs' kernels."""

  def fused_ok(self, rows: int, d: int) -> bool:
    """Whether symmetric min/max candidates of a [rows, d] weight take the one-read kernel."""
    return True

  def stack(self, count: int, rows: int, d: int):
    import torch
    from . import runtime as rt
    return rt.empty((count, rows * d), torch.float32)

  def sweep_into(self, stack, first: int, reference, rows: int, d: int, pairs):
    """Deltas of the (bits, block) `pairs` into stack[first:first + len(pairs)]; returns their row sums of squares
    (float64 [len(pairs), rows], still on the device)."""
    from . import ops
    _, sq = ops.requant_delta_sweep(reference.view(rows, d), pairs, want_sq=True,
                                    out=stack[first:first + len(pairs)].view(len(pairs), rows, d))
    return sq

  def candidate_params(self, candidate: SweepCandidate, op_info, values: np.ndarray, tensor_qsv):
    """UniformQuantParams of the registered algorithm for this op's weight (its own get_tensor_quant_params)."""
    from .algorithms.uniform_quantize import gptq, mse, naive_min_max_quantize, octav
    module = {_MIN_MAX_KEY: naive_min_max_quantize, "OCTAV": octav, "MSE": mse, "GPTQ": gptq}[candidate.algorithm_name]
    return module.get_tensor_quant_params(op_info, candidate.tensor_config(), values, tensor_qsv)

  def params_delta_into(self, stack, index: int, reference, rows: int, d: int, params):
    """Delta of the integers and scales an algorithm returned into stack[index]; returns its row sums of squares
    (float64 [1, rows], on the device). q - zero_point is formed in int32 and scaled in float64 (diff_bits 32)."""
    import torch
    from . import ops
    from . import runtime as rt
    q = params.quantized_data
    q = q.device_tensor if isinstance(q, rt.HbmArray) else rt.to_device(np.ascontiguousarray(np.asarray(q)))
    kind = {torch.int8: "i8", torch.int16: "i16", torch.int32: "i32"}.get(q.dtype)
    if kind is None or q.numel() != rows * d:
      raise ValueError(f"quantized data of type {q.dtype} and {q.numel()} elements for a [{rows}, {d}] weight")
    channels, inner = scale_view(params, rows, d)
    scale = rt.on_device(params.scale, torch.float32).reshape(-1)
    zp = np.asarray(params.zero_point).reshape(-1).astype(np.int32)
    zp_dev = rt.to_device(np.ascontiguousarray(np.broadcast_to(zp, (channels,)))) if zp.any() else None
    target = ops.CompareTarget(q.reshape(-1), rows * d, kind, scale, zp_dev, channels, inner, 32)
    delta = ops.weight_delta(reference, target)
    stack[index].copy_(delta)
    return delta.view(rows, d).double().square_().sum(dim=1, keepdim=True).t()

  def energy(self, reference) -> float:
    """Sum of the weight's squares in float64."""
    return float(reference.double().square_().sum().item())

  def host(self, values) -> np.ndarray:
    return values if isinstance(values, np.ndarray) else values.cpu().numpy()


def scale_view(params, rows: int, d: int) -> tuple[int, int]:
  """(channels, inner) of ops.CompareTarget for the scale shape of a [rows, d] weight's UniformQuantParams."""
  n = int(np.prod(np.shape(params.scale)))
  if n == 1:
    return 1, 1
  if params.block_size:
    if n * params.block_size != rows * d:
      raise ValueError(f"{n} scales for blocks of {params.block_size} of a [{rows}, {d}] weight")
    return n, int(params.block_size)
  if params.quantized_dimension == 0 and n == rows:
    return rows, d
  if params.quantized_dimension == 1 and n == d:
    return d, 1
  raise ValueError(f"{n} scales along dimension {params.quantized_dimension} of a [{rows}, {d}] weight")


class LayerSensitivity:
  """results[output tensor name][candidate name] of sweep_layer_sensitivity: `weight`, `input`, `rows`, `d`, `route`
  ("fused" or "generic"), `weight_sq_error`, `weight_snr`, `bits_per_weight`, and with Hessians `signal`, `error`,
  `output_mse`, `output_snr`, `per_channel_error` as LayerOutputComparison defines them. skipped[(output tensor name,
  candidate name)] is the reason a pair was not computed."""

  def __init__(self, signature_key: Optional[str] = None, candidates: Sequence[SweepCandidate] = ()):
    self.signature_key = signature_key
    self.candidates = {c.name: c for c in candidates}
    self.results: dict[str, dict[str, dict]] = {}
    self.skipped: dict[tuple, str] = {}

  def __getitem__(self, name: str) -> dict:
    return self.results[name]

  def __contains__(self, name: str) -> bool:
    return name in self.results

  def __iter__(self):
    return iter(self.results)

  def __len__(self) -> int:
    return len(self.results)

  def as_dict(self) -> dict:
    layers = {y: {c: {k: v for k, v in r.items() if k != "per_channel_error"} for c, r in per.items()}
              for y, per in self.results.items()}
    skipped: dict[str, dict[str, str]] = {}
    for (y, c), reason in self.skipped.items():
      skipped.setdefault(y, {})[c] = reason
    return {"signature_key": self.signature_key, "candidates": list(self.candidates), "layers": layers,
            "skipped": skipped}

  def save(self, save_folder: str, model_name: str) -> str:
    """`<model_name>_layer_sensitivity.json`, without the per-channel arrays."""
    save_path = pathlib.Path(save_folder)
    os.makedirs(str(save_path), exist_ok=True)
    path = str(save_path / (model_name + "_layer_sensitivity.json"))
    with open(path, "w") as fh:
      fh.write(json.dumps(self.as_dict()))
    return path

  def cheapest(self, min_output_snr: Optional[float] = None, min_weight_snr: Optional[float] = None) -> dict:
    """{output tensor name: candidate name or None}: per op the candidate with the fewest bits per weight whose
    `output_snr` (or `weight_snr`) is at least the threshold; among equally cheap ones the larger SNR."""
    if (min_output_snr is None) == (min_weight_snr is None):
      raise ValueError("cheapest needs exactly one of min_output_snr and min_weight_snr.")
    key, least = ("output_snr", min_output_snr) if min_output_snr is not None else ("weight_snr", min_weight_snr)
    out: dict[str, Optional[str]] = {}
    for y, per in self.results.items():
      best = None
      for name, r in per.items():
        if key not in r or not r[key] >= least:
          continue
        rank = (r["bits_per_weight"], -r[key])
        if best is None or rank < best[0]:
          best = (rank, name)
      out[y] = None if best is None else best[1]
    return out


def fully_connected_scopes(float_model, signature_key: Optional[str] = DEFAULT_SIGNATURE_KEY) -> dict[str, str]:
  """{output tensor name: scope string} of a signature's FULLY_CONNECTED ops: the string params_generator hands
  recipe_manager for the op (tfl_flatbuffer_utils.get_op_scope)."""
  m = _as_model(float_model)
  sg_index, _ = _signature_subgraph(m, signature_key)
  tensors = m.subgraphs[sg_index].tensors
  return {y_name: tfl_flatbuffer_utils.get_op_scope(op, tensors) for op, _, _, y_name in _fully_connected_ops(m, sg_index)}


def sweep_layer_sensitivity(float_model, candidates: Sequence[SweepCandidate], calibration_result: Optional[dict] = None,
                            signature_key: Optional[str] = DEFAULT_SIGNATURE_KEY, *,
                            kernels: Optional[SweepKernels] = None, max_stack_bytes: int = 2 << 30) -> LayerSensitivity:
  """Layer output error of every FULLY_CONNECTED op of the float model with a constant 2-D float32 weight [rows, d]
  under every candidate configuration (the same ops, skip reasons and figures as compare_layer_outputs; no recipe, no
  quantize() and no quantized model are needed).

  Candidates that are symmetric min/max with 2, 4 or 8 bits, CHANNELWISE or BLOCKWISE_32 / 64 / 128 / 256 (the block
  dividing d) take the fused route: one ops.requant_delta_sweep call per op. The remaining weight-side algorithms that
  keep the weight in its own basis (asymmetric or TENSORWISE min/max, OCTAV, MSE, GPTQ) take the generic route: the
  registered algorithm's get_tensor_quant_params, then ops.weight_delta of its integers and scales. All deltas of an
  op are stacked as [count * rows, d] and go through one ops.quadform_rows launch per chunk of at most
  `max_stack_bytes`. Candidates stored in a transformed basis (Hadamard, OSCAR), or refused by the algorithm or the
  policy for an op, are listed in `.skipped` with the reason.

  Without `calibration_result` the sweep is data-free: weight-space figures only."""
  from . import algorithm_manager
  from . import qtyping
  kernels = kernels or SweepKernels()
  candidates = list(candidates)
  names = [c.name for c in candidates]
  if len(set(names)) != len(names):
    raise ValueError("candidate names must be unique")
  ref = _as_model(float_model)
  sg_ref, _ = _signature_subgraph(ref, signature_key)
  out = LayerSensitivity(signature_key, candidates)
  with_data = calibration_result is not None
  hessians: dict[str, tuple] = {}
  signals: dict[tuple, np.ndarray] = {}
  energies: dict[str, float] = {}
  resident: tuple = (None, None)
  operators = list(ref.subgraphs[sg_ref].operators or [])
  fc_key = qtyping.TFLOperationName.FULLY_CONNECTED
  for op, x_name, w, y_name in _fully_connected_ops(ref, sg_ref):
    def skip_all(reason):
      for c in candidates:
        out.skipped[(y_name, c.name)] = reason
    w_name = schema.tensor_name(w)
    if (w.type != schema.TensorType.FLOAT32 or not _has_data(ref.buffers, w) or w.shape is None or len(w.shape) != 2):
      skip_all(SKIP_WEIGHT)
      continue
    rows, d = int(w.shape[0]), int(w.shape[1])
    qsv = calibration_result.get(x_name) if with_data else None
    stat = (qsv or {}).get("hessian") if with_data else None
    if with_data:
      if stat is None:
        skip_all(SKIP_NO_HESSIAN)
        continue
      if tuple(stat.shape) != (d, d):
        skip_all(SKIP_ORDER)
        continue
    values = np.asarray(tfl_flatbuffer_utils.get_tensor_data(w, ref.buffers), np.float32).reshape(rows, d)
    # ---- which route every candidate takes for this op
    fused, generic = [], []
    for c in candidates:
      block = c.fused_block(d) if kernels.fused_ok(rows, d) else None
      if block is not None:
        fused.append((c, block))
        continue
      if c.algorithm_name not in _GENERIC_ALGORITHMS:
        out.skipped[(y_name, c.name)] = SKIP_BASIS
        continue
      if c.block_size and d % c.block_size:
        out.skipped[(y_name, c.name)] = (f"Quantized dimension {d} in tensor shape {(rows, d)} is not divisible by"
                                         f" block size {c.block_size}.")
        continue
      if c.algorithm_name == "GPTQ" and stat is None:
        out.skipped[(y_name, c.name)] = SKIP_NO_HESSIAN
        continue
      # the policy decides per mode (asymmetric weights pass as weight-only, not as dynamic): either one will do
      cfg, refusal = None, None
      for precision, explicit in ((qtyping.ComputePrecision.INTEGER, False), (qtyping.ComputePrecision.FLOAT, True)):
        try:
          trial = qtyping.OpQuantizationConfig(weight_tensor_config=c.tensor_config(), compute_precision=precision,
                                               explicit_dequantize=explicit)
          algorithm_manager.check_op_quantization_config(c.algorithm_name, fc_key, trial)
        except ValueError as e:
          refusal = refusal or str(e)
          continue
        cfg = trial
        break
      if cfg is None:
        out.skipped[(y_name, c.name)] = refusal
        continue
      generic.append((c, cfg))
    if not fused and not generic:
      continue
    if with_data and x_name not in hessians:
      hessians[x_name] = kernels.hessian(stat)
    if resident[0] != w_name:
      resident = (w_name, kernels.weight(values.reshape(-1)))
    w_dev = resident[1]
    if with_data and (w_name, x_name) not in signals:
      product, alpha = hessians[x_name]
      signals[(w_name, x_name)] = kernels.quadform(w_dev, rows, d, product, 0.5 * alpha)
    if w_name not in energies:
      energies[w_name] = kernels.energy(w_dev)
    # ---- chunks of at most max_stack_bytes: the fused candidates first (one sweep call per chunk), then the others
    todo = [(c, ROUTE_FUSED, block) for c, block in fused] + [(c, ROUTE_GENERIC, cfg) for c, cfg in generic]
    per_chunk = max(1, int(max_stack_bytes) // (rows * d * 4))
    for first in range(0, len(todo), per_chunk):
      chunk = todo[first:first + per_chunk]
      stack = kernels.stack(len(chunk), rows, d)
      n_fused = sum(1 for _, route, _ in chunk if route == ROUTE_FUSED)
      done, sq_parts = [], []
      if n_fused:
        sq_parts.append(kernels.sweep_into(stack, 0, w_dev, rows, d, [(int(c.num_bits), block) for c, _, block in chunk[:n_fused]]))
        done.extend((c, ROUTE_FUSED) for c, _, _ in chunk[:n_fused])
      for c, _, cfg in chunk[n_fused:]:
        try:
          op_info = qtyping.OpInfo(op, fc_key, operators.index(op), cfg)
          tensor_qsv = {"activation_tensor_qsv": qsv} if (c.algorithm_name == "GPTQ" and qsv is not None) else None
          params = kernels.candidate_params(c, op_info, values, tensor_qsv)
          if params.hadamard is not None or params.custom_algorithm_param:
            out.skipped[(y_name, c.name)] = SKIP_BASIS
            continue
          sq_parts.append(kernels.params_delta_into(stack, len(done), w_dev, rows, d, params))
        except (ValueError, KeyError, NotImplementedError) as e:       # what the algorithm refuses for this op
          out.skipped[(y_name, c.name)] = str(e) or type(e).__name__
          continue
        done.append((c, ROUTE_GENERIC))
      if not done:
        continue
      per_channel = None
      if with_data:
        product, alpha = hessians[x_name]
        filled = stack[:len(done)]
        per_channel = np.asarray(kernels.quadform(filled, len(done) * rows, d, product, 0.5 * alpha)).reshape(len(done), rows)
      sq = np.concatenate([np.asarray(kernels.host(p), np.float64).reshape(-1, rows) for p in sq_parts], axis=0)
      for i, (c, route) in enumerate(done):
        weight_sq = float(np.sum(sq[i]))
        entry = {"weight": w_name, "input": x_name, "rows": rows, "d": d, "route": route,
                 "weight_sq_error": weight_sq,
                 "weight_snr": energies[w_name] / (weight_sq + 1e-9 * rows * d),
                 "bits_per_weight": c.bits_per_weight(rows, d)}
        if with_data:
          signal, error = float(np.sum(signals[(w_name, x_name)])), float(np.sum(per_channel[i]))
          mse = error / rows
          entry.update(signal=signal, error=error, output_mse=mse, output_snr=(signal / rows) / (mse + 1e-9),
                       per_channel_error=per_channel[i].copy())
        out.results.setdefault(y_name, {})[c.name] = entry
  return out
