"""CPU checks of model validation: the metric enum and registry, size checks, which constants compare_model
takes from the two flatbuffers and how, the save() / Model Explorer layout, the missing-runner errors, the C ABI's
argument checks."""
import json
import os
import sys

import numpy as np
import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")


@pytest.fixture(scope="module")
def lib():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def test_metric_enum_and_registry():
  from mi355q.utils import validation_utils as vu
  from mi355q import quantizer
  assert [m.value for m in vu.ValidationErrorMetric] == [
      "mse", "median_diff_ratio", "cosine_similarity", "kl_divergence", "snr"]
  assert quantizer.ValidationErrorMetric is vu.ValidationErrorMetric
  assert vu.get_validation_func(vu.ValidationErrorMetric.MSE) is vu.mean_squared_difference
  assert vu.get_validation_func(vu.ValidationErrorMetric.SNR) is vu.signal_to_noise_ratio
  assert vu.get_validation_func(vu.ValidationErrorMetric.MEDIAN_DIFF_RATIO) is vu.median_diff_ratio
  assert vu.get_validation_func(vu.ValidationErrorMetric.COSINE_SIMILARITY) is vu.cosine_similarity
  assert vu.get_validation_func(vu.ValidationErrorMetric.KL_DIVERGENCE) is vu.kl_divergence
  with pytest.raises(ValueError, match="not supported"):
    vu.get_validation_func("mse")


@pytest.mark.parametrize("fn", ["mean_squared_difference", "median_diff_ratio", "cosine_similarity", "kl_divergence",
                                "signal_to_noise_ratio"])
def test_size_mismatch_raises_before_the_device(fn):
  from mi355q.utils import validation_utils as vu
  with pytest.raises(ValueError, match="data1 & data2 must be of the same size"):
    getattr(vu, fn)(np.zeros(3), np.zeros(4))


def test_empty_operands_need_no_device():
  from mi355q.utils import validation_utils as vu
  got = vu.compare_all(np.zeros((0, 3)), np.zeros(0))
  assert all(v == 0.0 and type(v) is float for v in got.values())


def _plans(ref, tgt):
  from mi355q import model_validator as mv
  return {p.name: p for p in mv.constant_plans(open(os.path.join(MODELS, ref), "rb").read(),
                                               open(os.path.join(MODELS, tgt), "rb").read())}


def test_constant_selection_srq_model():
  from mi355q import model_validator as mv
  ref = open(os.path.join(MODELS, "conv_fc_mnist.tflite"), "rb").read()
  plans = _plans("conv_fc_mnist.tflite", "conv_fc_mnist_srq_a8w8.tflite")
  names = set(mv.get_constant_tensor_names(ref))
  assert plans and set(plans) <= names
  quantized = [p for p in plans.values() if p.dequantized]
  assert quantized and all(p.kind in ("i8", "i32") and p.scale is not None for p in quantized)
  for p in quantized:
    assert p.channels == 1 or p.channels == len(p.scale)
    assert p.diff_bits == 32 and p.data.size == p.reference.size
  # a float model against itself: every constant compared as stored
  same = _plans("single_fc_bias.tflite", "single_fc_bias.tflite")
  assert same and all(p.kind == "f32" and not p.dequantized for p in same.values())


def test_constant_selection_needs_data_and_a_name_in_the_target():
  from mi355q import model_validator as mv
  plans = _plans("single_fc_bias.tflite", "single_fc.tflite")
  ref = open(os.path.join(MODELS, "single_fc_bias.tflite"), "rb").read()
  tgt = open(os.path.join(MODELS, "single_fc.tflite"), "rb").read()
  tgt_names = set(mv.get_constant_tensor_names(tgt))
  assert set(plans) <= tgt_names & set(mv.get_constant_tensor_names(ref))


def _hand_result():
  from mi355q import model_validator as mv
  from mi355q.utils import validation_utils as vu
  ref = open(os.path.join(MODELS, "single_fc_bias.tflite"), "rb").read()
  res = mv.ComparisonResult(ref, ref[: len(ref) // 2])
  key = mv.signature_keys(ref)[0]
  ins = mv.get_input_tensor_names(ref, key)
  outs = mv.get_output_tensor_names(ref, key)
  consts = mv.get_constant_tensor_names(ref)
  vals = {nm: {"mse": 0.5 + i, "snr": 2.0 * i} for i, nm in enumerate(ins + outs + consts + ["inner_tensor"])}
  res.add_new_signature_results([vu.ValidationErrorMetric.MSE, vu.ValidationErrorMetric.SNR], vals, key)
  return res, key, ins, outs, consts


def test_comparison_result_sections_and_save(tmp_path):
  from mi355q.utils import validation_utils as vu
  res, key, ins, outs, consts = _hand_result()
  sig = res.get_signature_comparison_result(key)
  assert set(sig.input_tensors) == set(ins) and set(sig.output_tensors) == set(outs)
  assert set(sig.constant_tensors) == set(consts) and set(sig.intermediate_tensors) == {"inner_tensor"}
  assert res.available_signature_keys() == [key]
  with pytest.raises(ValueError, match="is not in the comparison_results"):
    res.get_signature_comparison_result("nope")
  with pytest.raises(ValueError, match="already in the comparison_results"):
    res.add_new_signature_results([vu.ValidationErrorMetric.MSE], {}, key)
  size, perc = res.get_model_size_reduction()
  assert size > 0 and 49 < perc < 51
  res.save(str(tmp_path), "fc")
  files = sorted(os.listdir(tmp_path))
  assert files == ["fc_comparison_result.json", "fc_comparison_result_me_input_mse.json",
                   "fc_comparison_result_me_input_snr.json"]
  main = json.load(open(tmp_path / "fc_comparison_result.json"))
  assert list(main) == ["reduced_size_bytes", "reduced_size_percentage", key]
  assert list(main[key]) == ["input_tensors", "output_tensors", "constant_tensors", "intermediate_tensors"]
  me = json.load(open(tmp_path / "fc_comparison_result_me_input_mse.json"))
  assert me["thresholds"] == [
      {"value": 0.05, "bgColor": "rgb(200, 255, 0)"}, {"value": 0.1, "bgColor": "rgb(200, 219, 0)"},
      {"value": 0.2, "bgColor": "rgb(200, 183, 0)"}, {"value": 0.4, "bgColor": "rgb(200, 147, 0)"},
      {"value": 1, "bgColor": "rgb(200, 111, 0)"}, {"value": 10, "bgColor": "rgb(200, 75, 0)"},
      {"value": 100, "bgColor": "rgb(200, 39, 0)"}]
  assert me["results"]["inner_tensor"] == {"value": sig.intermediate_tensors["inner_tensor"]["mse"]}


def test_missing_runner_errors():
  from mi355q import model_validator as mv
  from mi355q import quantizer
  ref = open(os.path.join(MODELS, "single_fc_bias.tflite"), "rb").read()
  with pytest.raises(ValueError, match="run_signature"):
    mv.compare_model(ref, ref, None, validate_output_tensors_only=True)
  with pytest.raises(ValueError, match="No quantized model available to validate"):
    quantizer.Quantizer(ref).validate()
  with pytest.raises(ValueError, match="number of error metrics"):
    mv.compare_model(ref, ref, {}, error_metrics=[], compare_fns=[len])


def test_random_inputs_are_seeded():
  from mi355q import model_validator as mv
  ref = open(os.path.join(MODELS, "single_fc_bias.tflite"), "rb").read()
  key = mv.signature_keys(ref)[0]
  a, b = mv.create_random_normal_input_data(ref, key), mv.create_random_normal_input_data(ref, key)
  assert len(a) == 1 and a[0].keys() == b[0].keys()
  for k in a[0]:
    np.testing.assert_array_equal(a[0][k], b[0][k])
    assert a[0][k].dtype == np.float32


def test_abi_argument_checks(lib):
  from mi355q import _ffi
  assert lib.mi355q_compare_chunks(0) == 0 and lib.mi355q_compare_chunks(8193) == 2
  assert lib.mi355q_compare_workspace_bytes(1, 2) > 2 * 48
  assert lib.mi355q_compare_workspace_bytes(-1, 0) == 0
  # n = 0 enqueues nothing, whatever the pointers
  assert lib.mi355q_compare_f32(None, None, 0, 0, 32, 1, 1, None, None, 1, None, None, 0, None) == 0
  assert lib.mi355q_compare_f32(None, None, 5, 0, 32, 1, 1, None, None, 1, None, None, 0, None) == -1
  assert b"null operand" in lib.mi355q_last_error()
  assert lib.mi355q_compare_f32(None, None, -1, 0, 32, 1, 1, None, None, 1, None, None, 0, None) == -1
  with pytest.raises(_ffi.Mi355qError, match="BAD_ARG"):
    _ffi.check(lib.mi355q_compare_f32(1, 1, 5, 3, 32, 1, 1, None, None, 1, 1, None, 0, None))   # no scales
  assert b"without scales" in lib.mi355q_last_error()
  assert lib.mi355q_compare_f32(1, 1, 5, 9, 32, 1, 1, None, None, 1, 1, None, 0, None) == -1
  assert lib.mi355q_compare_f32(1, 1, 5, 3, 12, 1, 1, 1, None, 1, 1, None, 0, None) == -1
  assert lib.mi355q_compare_f32_batched(None, 0, 0, 1, None, None, 0, None) == 0
  assert lib.mi355q_compare_f32_batched(None, 2, 2, 1, None, None, 0, None) == -1
  assert lib.mi355q_compare_f32(None, None, 0, 0, 32, 1, 1, None, None, 1, None, None, 0, None) == 0
  assert lib.mi355q_last_error() == b""
