"""Comparator functions of model validation, computed on the GPU (ref: utils/validation_utils.py).

Same names, argument order and return types as the reference: `float` for MSE, KL divergence and SNR,
`np.float32` for the median diff ratio and the cosine similarity (Python floats for the special cases).
`data1` is the target (noisy) operand and `data2` the reference, as model_validator passes them.

Operands may be host arrays, torch tensors (device tensors are compared in place) or runtime.HbmArray;
the target may also be an ops.CompareTarget, a quantized tensor in its stored form that the kernel
dequantizes in registers. Every call is one set of launches of csrc/validation.hip; `compare_all`
returns all five metrics of a pair from one call, `compare_all_batched` those of many pairs.

Parity: MSE, SNR and the median diff ratio are bit-equal to NumPy (same float32 summation order, same
rounding of the means); the cosine similarity and the KL divergence agree within a tolerance
(BLAS sdot order, NumPy's SIMD log). DESIGN.md section 4.
"""
from __future__ import annotations

import enum
from typing import Any, Protocol, Sequence

import numpy as np


class ValidationFuncType(Protocol):
  """Type hint and documentation for validation functions."""

  def __call__(self, data1: Any, data2: Any) -> float:
    ...


class ValidationErrorMetric(enum.Enum):
  MSE = "mse"
  MEDIAN_DIFF_RATIO = "median_diff_ratio"
  COSINE_SIMILARITY = "cosine_similarity"
  KL_DIVERGENCE = "kl_divergence"
  SNR = "snr"


VALIDATION_FUNCS: dict[ValidationErrorMetric, ValidationFuncType] = {}


def _register_validation_func(metric_name: ValidationErrorMetric):
  def decorator(func: ValidationFuncType):
    VALIDATION_FUNCS[metric_name] = func
    return func

  return decorator


def get_validation_func(func_name: ValidationErrorMetric) -> ValidationFuncType:
  """Returns a validation function based on the metric type."""
  if func_name not in VALIDATION_FUNCS:
    raise ValueError(f"Validation function {func_name} not supported.")
  return VALIDATION_FUNCS[func_name]


# ----------------------------------------------------------------------------- operands
def _size(x) -> int:
  from .. import ops
  if isinstance(x, ops.CompareTarget):
    return x.n
  if hasattr(x, "device_tensor"):
    return int(x.device_tensor.numel())
  if hasattr(x, "numel") and hasattr(x, "is_cuda"):
    return int(x.numel())
  return int(np.size(x))


def _check_same_size(data1, data2) -> int:
  n1, n2 = _size(data1), _size(data2)
  if n1 != n2:
    raise ValueError("data1 & data2 must be of the same size")
  return n1


_TORCH_KINDS = {"torch.float32": "f32", "torch.float16": "f16", "torch.bfloat16": "bf16", "torch.int8": "i8",
                "torch.int16": "i16", "torch.int32": "i32"}


def _as_target(x):
  """data1 -> ops.CompareTarget (np.asarray(x, np.float32) semantics)."""
  import torch
  from .. import ops
  from .. import runtime as rt
  if isinstance(x, ops.CompareTarget):
    return x
  if hasattr(x, "device_tensor"):
    x = x.device_tensor
  if not (isinstance(x, torch.Tensor) and x.is_cuda):
    a = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
    a = a if a.dtype == np.float16 else np.asarray(a, np.float32)
    x = rt.to_device(np.ravel(a))
  kind = _TORCH_KINDS.get(str(x.dtype))
  if kind is None:
    x, kind = x.to(torch.float32), "f32"
  x = x.contiguous().view(-1)
  if kind in ("f32", "f16", "bf16"):
    return ops.CompareTarget(x, x.numel(), kind)
  one = torch.ones(1, dtype=torch.float32, device=x.device)   # a plain cast: (q - 0) * 1
  return ops.CompareTarget(x, x.numel(), kind, one, None, 1, 1, 32)


def _as_reference(x):
  """data2 -> contiguous float32 device tensor."""
  import torch
  from .. import runtime as rt
  if hasattr(x, "device_tensor"):
    x = x.device_tensor
  if isinstance(x, torch.Tensor) and x.is_cuda:
    return x.to(torch.float32).contiguous().view(-1)
  a = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
  return rt.to_device(np.ravel(np.asarray(a, np.float32)))


# ----------------------------------------------------------------------------- metrics from the sums
_ALL = tuple(ValidationErrorMetric)


def _metrics(rec, n: int) -> dict:
  """The five metrics of one pair from its comparison record, with NumPy's final roundings."""
  if n == 0:
    return {m: float(0) for m in _ALL}
  f32 = np.float32
  # .mean(): float32 sum / intp count is a float64 division, cast to float32
  mse = float(f32(np.float64(f32(rec["sum_sq_diff"])) / np.float64(n)))
  signal_power = float(f32(np.float64(f32(rec["sum_ref_sq"])) / np.float64(n)))
  snr = signal_power / (mse + 1e-9)
  lo, hi = f32(rec["median_lo"]), f32(rec["median_hi"])
  median = lo if n % 2 else f32(np.float64(f32(lo + hi)) / np.float64(2))
  norm1, norm2 = np.sqrt(f32(rec["dot_tt"])), np.sqrt(f32(rec["dot_rr"]))
  if norm1 == 0 and norm2 == 0:
    cosine = 1.0
  elif norm1 == 0 or norm2 == 0:
    cosine = 0.0
  else:
    cosine = f32(rec["dot_tr"]) / (norm1 * norm2)
  return {
      ValidationErrorMetric.MSE: mse,
      ValidationErrorMetric.MEDIAN_DIFF_RATIO: median,
      ValidationErrorMetric.COSINE_SIMILARITY: cosine,
      ValidationErrorMetric.KL_DIVERGENCE: float(f32(rec["sum_kl"])),
      ValidationErrorMetric.SNR: snr,
  }


def compare_all_batched(pairs: Sequence[tuple[Any, Any]],
                        error_metrics: Sequence[ValidationErrorMetric] | None = None) -> list[dict]:
  """[(data1, data2), ...] -> one {metric: value} per pair, all pairs in one set of launches."""
  from .. import ops
  metrics = tuple(error_metrics) if error_metrics is not None else _ALL
  sizes = [_check_same_size(d1, d2) for d1, d2 in pairs]
  if not any(sizes):
    return [{m: float(0) for m in metrics} for _ in pairs]
  dev = [(_as_reference(d2), _as_target(d1)) for d1, d2 in pairs]
  recs = ops.compare(dev, median=ValidationErrorMetric.MEDIAN_DIFF_RATIO in metrics,
                     kl=ValidationErrorMetric.KL_DIVERGENCE in metrics)
  out = []
  for rec, n in zip(recs, sizes):
    allm = _metrics(rec, n)
    out.append({m: allm[m] for m in metrics})
  return out


def compare_all(data1, data2, error_metrics: Sequence[ValidationErrorMetric] | None = None) -> dict:
  """All requested metrics (default: the five) of one pair from one call."""
  return compare_all_batched([(data1, data2)], error_metrics)[0]


# ----------------------------------------------------------------------------- the registered functions
@_register_validation_func(ValidationErrorMetric.MSE)
def mean_squared_difference(data1, data2) -> float:
  """mean((data1 - data2)^2) (ref: validation_utils.py:63-87)."""
  return compare_all(data1, data2, [ValidationErrorMetric.MSE])[ValidationErrorMetric.MSE]


@_register_validation_func(ValidationErrorMetric.MEDIAN_DIFF_RATIO)
def median_diff_ratio(data1, data2, tolerance_threshold=1e-6) -> float:
  """median(|data1 - data2| / (|data2| + 1e-6)) (ref: validation_utils.py:90-120)."""
  if tolerance_threshold != 1e-6:
    raise ValueError("the GPU kernel implements tolerance_threshold=1e-6 only")
  return compare_all(data1, data2, [ValidationErrorMetric.MEDIAN_DIFF_RATIO])[
      ValidationErrorMetric.MEDIAN_DIFF_RATIO]


@_register_validation_func(ValidationErrorMetric.COSINE_SIMILARITY)
def cosine_similarity(data1, data2) -> float:
  """dot(data1, data2) / (|data1| |data2|) (ref: validation_utils.py:123-152)."""
  return compare_all(data1, data2, [ValidationErrorMetric.COSINE_SIMILARITY])[
      ValidationErrorMetric.COSINE_SIMILARITY]


@_register_validation_func(ValidationErrorMetric.KL_DIVERGENCE)
def kl_divergence(data1, data2, epsilon: float = 1e-9) -> float:
  """sum(p log((p + eps) / (q + eps))), p = max(0, data2), q = max(0, data1) (ref: validation_utils.py:155-192)."""
  if epsilon != 1e-9:
    raise ValueError("the GPU kernel implements epsilon=1e-9 only")
  return compare_all(data1, data2, [ValidationErrorMetric.KL_DIVERGENCE])[ValidationErrorMetric.KL_DIVERGENCE]


@_register_validation_func(ValidationErrorMetric.SNR)
def signal_to_noise_ratio(noisy_signal, signal, epsilon: float = 1e-9) -> float:
  """mean(signal^2) / (mse + eps) (ref: validation_utils.py:195-228)."""
  if epsilon != 1e-9:
    raise ValueError("the GPU kernel implements epsilon=1e-9 only")
  return compare_all(noisy_signal, signal, [ValidationErrorMetric.SNR])[ValidationErrorMetric.SNR]
