"""Quantizer facade: `.tflite` in, quantized `.tflite` out (ref: quantizer.py:59-620).

Covers the weight-requantization flow of the hot path: read the model (zero-copy views of the
mmap'd file), load a recipe, generate parameters through the registry (GPU kernels), apply the
QUANTIZE_TENSOR transformation (pack + store + metadata) and serialize. Running a model (the LiteRT
interpreter) is outside this build's scope: calibration results (QSVs) are passed in, and `validate()`
compares the constant tensors on the GPU and takes inputs, outputs and intermediates from a
caller-supplied `run_signature`; `validate_layer_outputs()` reports the output error of every FULLY_CONNECTED op
over the calibration set from the Hessians calibration keeps, without a run of the model; `sweep_layer_sensitivity()`
reports the same per op and candidate configuration from the float model alone, and `apply_layer_selection()` turns a
choice of candidates into recipe entries.
"""
from __future__ import annotations

import contextlib
import dataclasses
import json
import os
import pathlib
import re
from typing import Any, Optional, Union

from . import algorithm_manager
from . import calibrator
from . import default_policy
from . import model_modifier
from . import model_validator
from . import params_generator
from . import qtyping
from . import recipe_manager
from . import requant_queue
from .utils import tfl_flatbuffer_utils
from .utils import tflite_flatbuffer
from .utils import validation_utils

apply_quantize_tensor_transformations = model_modifier.apply_quantize_tensor_transformations

Path = Union[str, pathlib.Path]
ValidationErrorMetric = validation_utils.ValidationErrorMetric


class _Flag(int):
  """A bool-valued int that can also be called (`qt.need_calibration` / `qt.need_calibration()`)."""

  def __call__(self) -> bool:
    return bool(self)

  def __repr__(self) -> str:
    return repr(bool(self))


@dataclasses.dataclass(frozen=True)
class QuantizationResult:
  """recipe + the serialized quantized model (ref :59-128)."""
  recipe: qtyping.ModelQuantizationRecipe
  quantized_model: Optional[Any]

  def save(self, save_folder: Path, model_name: str, overwrite: bool = False) -> None:
    os.makedirs(save_folder, exist_ok=True)
    self.export_model(str(pathlib.Path(save_folder) / f"{model_name}.tflite"), overwrite)
    recipe_path = pathlib.Path(save_folder) / (model_name + "_recipe.json")
    tfl_flatbuffer_utils.set_file_contents(recipe_path, json.dumps(self.recipe).encode())

  def export_model(self, filepath: Path, overwrite: bool = False) -> None:
    if self.quantized_model is None:
      raise RuntimeError("No quantized model to save. Make sure .quantize() is called.")
    if os.path.exists(filepath) and not overwrite:
      raise ValueError(
          f"The model {filepath} already exists in the folder. Please consider change the model"
          " name or specify overwrite=True to overwrite the model if needed.")
    tfl_flatbuffer_utils.set_file_contents(filepath, self.quantized_model)


class Quantizer:
  """`float_model`: a `.tflite` path, model bytes, or an already parsed ModelT tree."""

  def __init__(self, float_model: Any,
               quantization_recipe: Optional[Union[Path, qtyping.ModelQuantizationRecipe]] = None):
    self._model_name: Optional[str] = None     # the float model's path, when it came from one (validate's file names)
    if isinstance(float_model, (str, pathlib.Path)):
      self._float_model_buffer = tfl_flatbuffer_utils.get_model_content(float_model)
      self._model_name = str(float_model)
      self.float_model = tfl_flatbuffer_utils.read_model(self._float_model_buffer)
    elif isinstance(float_model, (bytes, bytearray, memoryview)):
      self._float_model_buffer = memoryview(float_model)
      self.float_model = tfl_flatbuffer_utils.read_model(self._float_model_buffer)
    elif isinstance(float_model, tflite_flatbuffer.TableT):
      self._float_model_buffer = None
      self.float_model = float_model
    else:
      raise ValueError("Unsupported float_model type: %s" % type(float_model).__name__)
    self._recipe_manager = recipe_manager.RecipeManager()
    self._result = QuantizationResult([{}], None)
    self.quantized_model_object: Optional[Any] = None
    if quantization_recipe is not None:
      self.load_quantization_recipe(quantization_recipe)

  def load_quantization_recipe(self, recipe: Union[Path, qtyping.ModelQuantizationRecipe]) -> None:
    """A recipe list, or the path of a recipe .json (ref :195-205)."""
    if isinstance(recipe, (str, pathlib.Path)):
      with open(recipe, "r", encoding="utf-8") as f:
        recipe = json.load(f)
    self._recipe_manager.load_quantization_recipe(recipe)

  def get_quantization_recipe(self) -> qtyping.ModelQuantizationRecipe:
    return self._recipe_manager.get_quantization_recipe()

  @property
  def need_calibration(self) -> "_Flag":
    """A property in the reference (`qt.need_calibration`); also callable here."""
    return _Flag(self._recipe_manager.need_calibration())

  def load_config_policy(self, filename: Path) -> None:
    """A user policy .json replaces the min/max algorithm's config check policy (ref :207-222)."""
    with open(filename, "r", encoding="utf-8") as f:
      policy = default_policy.update_default_config_policy(f.read())
    algorithm_manager.register_config_check_policy_func(
        algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT, policy)

  def update_quantization_recipe(self, regex: str, operation_name, op_config=None,
                                 algorithm_key: str = algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT):
    """ref :233-262."""
    self._recipe_manager.add_quantization_config(regex, operation_name, op_config, algorithm_key)

  def add_dynamic_config(self, regex: str, operation_name, num_bits: int,
                         granularity=qtyping.QuantGranularity.CHANNELWISE,
                         algorithm_key: str = algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT):
    """ref :264-289."""
    self._recipe_manager.add_dynamic_config(regex, operation_name, num_bits, granularity, algorithm_key)

  def add_weight_only_config(self, regex: str, operation_name, num_bits: int,
                             granularity=qtyping.QuantGranularity.CHANNELWISE,
                             algorithm_key: str = algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT):
    """ref :291-316."""
    self._recipe_manager.add_weight_only_config(regex, operation_name, num_bits, granularity, algorithm_key)

  def add_static_config(self, regex: str, operation_name, activation_num_bits: int, weight_num_bits: int,
                        weight_granularity=qtyping.QuantGranularity.CHANNELWISE,
                        algorithm_key: str = algorithm_manager.AlgorithmName.MIN_MAX_UNIFORM_QUANT):
    """ref :318-352."""
    self._recipe_manager.add_static_config(regex, operation_name, activation_num_bits, weight_num_bits,
                                           weight_granularity, algorithm_key)

  def calibrate(self, calibration_data: dict, previous_calibration_result: Optional[dict] = None,
                tensor_provider: Optional[Any] = None, hessians: str = "consumed") -> dict[str, qtyping.QSV]:
    """Model QSVs from per-sample tensor contents (ref :369-413). The reference runs the float
    model in the LiteRT interpreter to obtain those tensors; here each sample is the
    {tensor name: ndarray} map itself, or `tensor_provider(signature_key, sample)` returns it.
    `hessians`: see Calibrator ("all" = a GPTQ Hessian for every runtime tensor, as the reference)."""
    if not self.need_calibration:
      return {}
    calib = calibrator.Calibrator(self.float_model, tensor_provider=tensor_provider, hessians=hessians)
    if previous_calibration_result is not None:
      calib.load_model_qsvs(previous_calibration_result)
    calib.calibrate(calibration_data, self._recipe_manager)
    return calib.get_model_qsvs()

  def quantize(self, calibration_result: Optional[dict[str, qtyping.QSV]] = None,
               serialize_to_path: Optional[Path] = None) -> QuantizationResult:
    """The float model is left untouched; the result holds the serialized quantized model
    (also written to `serialize_to_path` when given). `quantized_model_object` keeps the
    quantized ModelT tree for inspection."""
    if not self.get_quantization_recipe():
      raise RuntimeError("Can not quantize without a quantization recipe.")
    generator = params_generator.ParamsGenerator(self.float_model)
    modifier = model_modifier.ModelModifier(self.float_model)
    # One block around the op walk AND the writer when a file is written: the walk's own block joins it, so results
    # stay placeholders until somebody reads them; the writer lays the file out from their sizes, sends every quantized
    # buffer on its way behind its own producer and takes the values the flatbuffer stores (per-channel scales) last
    # (model_modifier.serialize_model, utils/tflite_flatbuffer.serialize_with_external_buffers).
    from . import runtime as rt
    rt.mark("quantize: call")
    try:
      with (requant_queue.batching() if serialize_to_path else contextlib.nullcontext()) as block:
        params = generator.generate_quantization_parameters(self._recipe_manager, calibration_result)
        rt.mark("quantize: parameters generated (host)")
        serialized = modifier.modify_model(params, serialize_to_path=serialize_to_path)
    finally:
      if serialize_to_path:
        rt.release_upload_files()      # (also when the call failed: announced uploads are waited for and dropped)
    rt.mark("quantize: model modified and serialized (host)")
    # launches / tensors of the batched path (with a file written, some launches left from inside the writer)
    self.batch_stats = dict(block.stats) if block is not None else getattr(generator, "batch_stats", None)
    self.quantized_model_object = modifier.quantized_model_object
    self._result = QuantizationResult(self.get_quantization_recipe(), serialized)
    return self._result

  def validate(self, test_data=None, error_metrics=None, use_xnnpack: bool = True, num_threads: int = 16,
               validate_output_tensors_only: bool = False, save_folder: Optional[str] = None,
               model_name: Optional[str] = None, *, run_signature=None) -> model_validator.ComparisonResult:
    """Numerical validation of the last quantize() result against the float model (ref :507-576).

    Constant tensors are compared on the GPU straight from the two flatbuffers. Input, output and intermediate
    tensors need a run of both models: `run_signature(model_bytes, signature_key, inputs) -> {tensor name: array}`
    is the caller's interpreter (without it only the constants are filled; with it and no `test_data`, one seeded
    random sample per signature is used). `use_xnnpack` and `num_threads` are accepted and ignored.
    """
    quantized_model = self._result.quantized_model
    if quantized_model is None:
      raise ValueError("No quantized model available to validate.")
    if self._float_model_buffer is not None:
      float_model = self._float_model_buffer    # (a mapped file stays mapped: see model_validator.compare_model)
    else:
      float_model = bytes(tflite_flatbuffer.write_model(self.float_model))
    results = model_validator.compare_model(
        float_model, bytes(quantized_model), test_data, error_metrics, compare_fns=None,
        use_xnnpack=use_xnnpack, num_threads=num_threads,
        validate_output_tensors_only=validate_output_tensors_only, run_signature=run_signature)
    if save_folder:
      if model_name is None:
        model_name = pathlib.Path(self._model_name).stem if self._model_name else "model"
      results.save(save_folder, model_name=model_name)
    return results

  def validate_layer_outputs(self, calibration_result: Optional[dict] = None, calibration_data: Optional[Any] = None,
                             signature_key: Optional[str] = None, save_folder: Optional[str] = None,
                             model_name: Optional[str] = None, follow_input_transforms: bool = False
                             ) -> model_validator.LayerOutputComparison:
    """Output error of every FULLY_CONNECTED op of the last quantize() result over the calibration set:
    error = 1/2 tr(dW H dW^T) = (1/n) ||X dW^T||_F^2 per op, with its signal, MSE, SNR and per-channel errors
    (model_validator.compare_layer_outputs; no run of the model is needed).

    Exactly one of `calibration_result` (what calibrate() returned for a recipe that keeps Hessians, or a loaded
    one) and `calibration_data` (the samples calibrate() takes: a list of {tensor name: array or device tensor}, or
    {signature key: such a list}; their Hessians are formed here) is required.

    Ops behind an inserted Hadamard rotation (custom op or decomposed) or OSCAR multiply are listed in `.skipped`
    unless `follow_input_transforms` is set: then their stored weight is mapped back through the inserted op's own
    constant (dW = W - rotate_h(dequant(W^)), or W - dequant(W^) * multiplier) and measured against the Hessian of the
    float model's untransformed input, and every entry also says which `input_transform` and `hadamard_size` it had.
    """
    quantized_model = self._result.quantized_model
    if quantized_model is None:
      raise ValueError("No quantized model available to validate.")
    if (calibration_result is None) == (calibration_data is None):
      raise ValueError("validate_layer_outputs needs exactly one of calibration_result and calibration_data.")
    if calibration_data is not None:
      calibration_result = self._layer_hessians(calibration_data, signature_key)
    results = model_validator.compare_layer_outputs(self.float_model, bytes(quantized_model), calibration_result,
                                                    signature_key, follow_input_transforms=follow_input_transforms)
    if save_folder:
      if model_name is None:
        model_name = pathlib.Path(self._model_name).stem if self._model_name else "model"
      results.save(save_folder, model_name=model_name)
    return results

  def validate_layer_execution(self, calibration_data: Any, signature_key: Optional[str] = None,
                               save_folder: Optional[str] = None, model_name: Optional[str] = None,
                               follow_input_transforms: bool = False,
                               int16_activations: bool = False,
                               quantized_outputs: bool = False,
                               conv_2d: bool = False,
                               depthwise_conv_2d: bool = False,
                               batch_matmul: bool = False,
                               transpose_conv: bool = False) -> model_validator.LayerExecutionComparison:
    """Executes every quantized FULLY_CONNECTED op of the last quantize() result in integers on the calibration
    samples and compares it with the float product: error = (1/n) ||Yq - Y||^2 per op with its signal, MSE, SNR,
    per-channel errors, token count and mode (model_validator.compare_layer_execution). Unlike
    validate_layer_outputs this includes the activations' own rounding: the per-row int8 quantization of
    dynamic-range ops and the calibrated int8 activations of static ops. The figure is the pre-bias product: bias,
    fused activation and the requantization of the op's output do not enter.

    `calibration_data`: the samples calibrate() takes, a list of {tensor name: array or device tensor}, or
    {signature key: such a list}. Ops behind an inserted Hadamard rotation or OSCAR multiply are listed in `.skipped`
    unless `follow_input_transforms` is set; then the samples go through the inserted op's own constant first. Ops
    that read an INT16 activation (static_wi8_ai16) are listed in `.skipped` unless `int16_activations` is set; then
    they are executed with an exact int64 accumulator and every entry also carries `activation_bits`. With
    `quantized_outputs` a static op is also executed through to the INT8 / INT16 tensor it stores (bias, fixed-point
    multiplier, output zero point, fused activation) and compared with the float op's own act(X W^T + b): every entry
    gains `output_bits`, and such an op `fused_activation` and the `final_*` figures, or `final_skipped` with the
    reason. With `conv_2d` every CONV_2D op is executed too, as the same integer product on the patch rows of its
    rank-4 samples (ops.conv_patches): every entry gains `op`, and a conv entry `kernel`, `strides`, `dilations`,
    `padding` and `output_hw`, with `rows` the output channels, `d` = KH KW I and `tokens` the patch rows. With
    `depthwise_conv_2d` every DEPTHWISE_CONV_2D op is executed too, by a direct convolution (ops.dwconv_forward): an
    entry has the keys of a conv entry with `op` = "DEPTHWISE_CONV_2D", `d` = KH KW, and `depth_multiplier`. With
    `batch_matmul` every BATCH_MATMUL op is executed too, by the integer batched product (ops.qbmm_forward): a constant
    right-hand side in the static, dynamic and weight-only modes, or two INT8 activations with a zero point each (the
    attention products); an entry has `op` = "BATCH_MATMUL", `operands`, `adj_x`, `adj_y` and `batch`, `rows` = N and
    `d` = K. With `transpose_conv` every TRANSPOSE_CONV op is executed too, by sub-pixel phases on patch rows
    (ops.tconv_patches), so that no multiply meets a stuffed zero: an entry has the keys of a conv entry without
    `dilations`, with `op` = "TRANSPOSE_CONV", `tokens` the output pixels and `phases`
    (model_validator.compare_layer_execution)."""
    quantized_model = self._result.quantized_model
    if quantized_model is None:
      raise ValueError("No quantized model available to validate.")
    samples = self._signature_samples(calibration_data, signature_key)
    results = model_validator.compare_layer_execution(self.float_model, bytes(quantized_model), samples, signature_key,
                                                      follow_input_transforms=follow_input_transforms,
                                                      int16_activations=int16_activations,
                                                      quantized_outputs=quantized_outputs, conv_2d=conv_2d,
                                                      depthwise_conv_2d=depthwise_conv_2d, batch_matmul=batch_matmul,
                                                      transpose_conv=transpose_conv)
    if save_folder:
      if model_name is None:
        model_name = pathlib.Path(self._model_name).stem if self._model_name else "model"
      results.save(save_folder, model_name=model_name)
    return results

  @staticmethod
  def _signature_samples(calibration_data: Any, signature_key: Optional[str]):
    """The sample list of one signature from the forms calibrate() takes (a list, or {signature key: list})."""
    samples = calibration_data
    if isinstance(calibration_data, dict):
      if signature_key is not None:
        if signature_key not in calibration_data:
          raise ValueError(f"calibration_data has no samples for signature {signature_key!r}")
        samples = calibration_data[signature_key]
      elif len(calibration_data) == 1:
        samples = next(iter(calibration_data.values()))
      else:
        raise ValueError("signature_key is required when calibration_data holds several signatures")
    return samples

  def _layer_hessians(self, calibration_data: Any, signature_key: Optional[str]) -> dict:
    """The Hessians of every FULLY_CONNECTED input from the samples calibrate() takes (a list, or {signature key: list})."""
    samples = self._signature_samples(calibration_data, signature_key)
    return model_validator.layer_hessians(self.float_model, samples, signature_key)

  def sweep_layer_sensitivity(self, candidates, calibration_result: Optional[dict] = None,
                              calibration_data: Optional[Any] = None, signature_key: Optional[str] = None,
                              save_folder: Optional[str] = None, model_name: Optional[str] = None
                              ) -> model_validator.LayerSensitivity:
    """Layer output error of every FULLY_CONNECTED op under every candidate configuration
    (model_validator.SweepCandidate), from the float model alone: no recipe and no quantize() are needed
    (model_validator.sweep_layer_sensitivity). At most one of `calibration_result` and `calibration_data` (as for
    validate_layer_outputs); with neither the sweep is data-free and reports the weight-space figures only.
    `result.cheapest(min_output_snr=...)` turns a threshold into a selection for apply_layer_selection()."""
    if calibration_result is not None and calibration_data is not None:
      raise ValueError("sweep_layer_sensitivity takes at most one of calibration_result and calibration_data.")
    if calibration_data is not None:
      calibration_result = self._layer_hessians(calibration_data, signature_key)
    results = model_validator.sweep_layer_sensitivity(self.float_model, candidates, calibration_result, signature_key)
    if save_folder:
      if model_name is None:
        model_name = pathlib.Path(self._model_name).stem if self._model_name else "model"
      results.save(save_folder, model_name=model_name)
    return results

  def apply_layer_selection(self, sensitivity: model_validator.LayerSensitivity, selection: dict,
                            mode: str = "weight_only") -> None:
    """One recipe entry per op of `selection` ({output tensor name: candidate name or None}, e.g. what
    `sensitivity.cheapest()` returned) with the candidate's algorithm key, bits and granularity, added through
    add_weight_only_config (`mode` "weight_only") or add_dynamic_config ("dynamic"). The entry's regex is the op's
    whole scope string, escaped and anchored, so it matches that op and no other; ops mapped to None are left to
    the entries already in the recipe."""
    if mode not in ("weight_only", "dynamic"):
      raise ValueError(f"mode must be 'weight_only' or 'dynamic', got {mode!r}")
    add = self.add_weight_only_config if mode == "weight_only" else self.add_dynamic_config
    scopes = model_validator.fully_connected_scopes(self.float_model, sensitivity.signature_key)
    for y_name, chosen in selection.items():
      if chosen is None:
        continue
      if y_name not in scopes:
        raise ValueError(f"no FULLY_CONNECTED op writes {y_name!r}")
      if chosen not in sensitivity.candidates:
        raise ValueError(f"unknown candidate {chosen!r}")
      c = sensitivity.candidates[chosen]
      if not c.symmetric or c.algorithm_params:
        raise ValueError(f"candidate {chosen!r} is asymmetric or carries algorithm parameters, which"
                         " add_weight_only_config / add_dynamic_config cannot express")
      add("^" + re.escape(scopes[y_name]) + "$", qtyping.TFLOperationName.FULLY_CONNECTED, int(c.num_bits),
          qtyping.QuantGranularity(c.granularity_name), c.algorithm_name)
