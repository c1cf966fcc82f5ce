"""Shared by test_gpu_layer_error.py and test_layer_error_host.py: the calibration-token generator, the NumPy model of
mi355q_weight_delta_f32's dequantization and the float64 evaluation of the quadratic forms."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def tokens(width: int, seed: int, samples: int = 4, length: int = 256) -> list:
  """`samples` arrays [1, length, width] of correlated tokens: a rank max(4, width // 8) mixture plus 0.1 of white
  noise, the first three channels 20 times larger (activation outliers)."""
  rng = np.random.default_rng(seed)
  k = max(4, width // 8)
  mix = rng.standard_normal((k, width))
  out = []
  for _ in range(samples):
    x = rng.standard_normal((length, k)) @ mix + 0.1 * rng.standard_normal((length, width))
    x[:, :3] *= 20.0
    out.append(x.astype(np.float32)[None])
  return out


def product_of(width: int, seed: int) -> np.ndarray:
  """X^T X in float32 of the generator's tokens, lower triangle (zeros above the diagonal)."""
  x = np.concatenate([s[0] for s in tokens(width, seed)], axis=0)
  return np.tril(x.T @ x).astype(np.float32)


def symmetric(lower: np.ndarray) -> np.ndarray:
  """float64 symmetric matrix whose lower triangle is `lower`'s."""
  low = np.tril(np.asarray(lower, np.float64))
  return low + np.tril(low, -1).T


def exact_rows(a: np.ndarray, psym: np.ndarray, alpha: float) -> np.ndarray:
  """alpha * a_r Psym a_r^T in float64 of the inputs as given."""
  a = np.asarray(a, np.float64)
  return alpha * np.einsum("ri,ri->r", a @ psym, a)


def gate_rows(a: np.ndarray, psym: np.ndarray, alpha: float) -> np.ndarray:
  """8 d u S_r with S_r = alpha Sum_ij |a_ri| |P_ij| |a_rj|: the first-order worst case of any float32 accumulation
  order over the d^2 products ((2d + 3) u on terms whose magnitudes sum to at most 3 S for a 2*lower - diagonal form)."""
  d = a.shape[1]
  return 8.0 * d * U * exact_rows(np.abs(a), np.abs(psym), abs(alpha))


def pack(q: np.ndarray, bits: int) -> np.ndarray:
  """int values -> packed bytes, element 0 in the low bits."""
  per = 8 // bits
  v = (np.asarray(q).ravel().astype(np.int64) & ((1 << bits) - 1)).reshape(-1, per)
  out = np.zeros(v.shape[0], np.int64)
  for i in range(per):
    out |= v[:, i] << (bits * i)
  return out.astype(np.uint8)


def dequantize(q: np.ndarray, scale: np.ndarray, zero_point, channels: int, inner: int, diff_bits: int) -> np.ndarray:
  """NumPy model of the integer kinds: element e uses entry (e // inner) % channels."""
  q = np.asarray(q).ravel()
  c = (np.arange(q.size) // inner) % channels
  zp = np.zeros(channels, np.int32) if zero_point is None else np.asarray(zero_point, np.int32)
  diff = q.astype(np.int32) - zp[c]
  s = np.asarray(scale, np.float32)[c]
  if diff_bits == 32:
    return (diff.astype(np.float64) * s.astype(np.float64)).astype(np.float32)
  diff = diff.astype(np.int8 if diff_bits == 8 else np.int16)       # wraps, as NumPy's promoted type does
  return diff.astype(np.float32) * s


def calibration_samples(projections, seed0: int = 100) -> list:
  """Four samples {tensor name: [1, 256, width]} for the inputs of tools/c5_model.build_model(1, ...), seeds
  seed0 + index of the input; the outputs get one small shared zero buffer (their min / max is all calibration
  wants of them)."""
  per_input, outputs = {}, {}
  for name, rows, cols, src in projections:
    if src not in per_input:
      per_input[src] = tokens(cols, seed0 + len(per_input))
    outputs[f"l0/{name}/y"] = np.zeros((1, 8, rows), np.float32)
  samples = []
  for k in range(4):
    s = {f"l0/{src}": xs[k] for src, xs in per_input.items()}
    s.update(outputs)
    samples.append(s)
  return samples
