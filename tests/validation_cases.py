"""Seeded comparison cases of model validation, shared by tests/golden/gen/make_validation_golden.py (which records the
reference's five metrics for each) and tests/test_gpu_validation_golden.py (which regenerates the arrays from the
seeds and compares the GPU's metrics with the recorded ones). Quantized targets are built with the oracle's
uniform_quantize / pack_data and turned into floats with its uniform_dequantize (the reference's arithmetic).

make(case) -> (target_float, reference, stored) where `stored` describes the target in its stored form:
  {"kind": "f32" | "f16" | "i8" | "i16" | "i32" | "i4", "data": array, "scale": float32 | None, "zp": int32 | None,
   "channels": int, "inner": int}
"""
import numpy as np

from oracle import aeq_oracle as O

SIZES = [0, 1, 2, 7, 8, 127, 128, 129, 8191, 8193, (1 << 20) + 3, 1 << 24]


def cases() -> list:
  out = []
  for i, n in enumerate(SIZES):
    out.append({"name": f"noise_n{n}", "seed": 100 + i, "n": n, "corruption": "noise", "form": "f32"})
  for i, n in enumerate([1, 2, 8, 1000, 8193]):   # odd and even n for the median
    out.append({"name": f"ties_n{n}", "seed": 200 + i, "n": n, "corruption": "ties", "form": "f32"})
  for i, n in enumerate([7, 129, 8193, 70000]):
    out.append({"name": f"nonfinite_n{n}", "seed": 300 + i, "n": n, "corruption": "nonfinite", "form": "f32"})
  for i, n in enumerate([8, 8193]):
    out.append({"name": f"zeros_n{n}", "seed": 400 + i, "n": n, "corruption": "zeros", "form": "f32"})
    out.append({"name": f"zero_target_n{n}", "seed": 410 + i, "n": n, "corruption": "zero_target", "form": "f32"})
    out.append({"name": f"zero_reference_n{n}", "seed": 420 + i, "n": n, "corruption": "zero_reference",
                "form": "f32"})
  for i, n in enumerate([9, 4096, 65537]):
    out.append({"name": f"negative_n{n}", "seed": 500 + i, "n": n, "corruption": "negative", "form": "f32"})
  for form, shapes in (("int8_channelwise", [(64, 256), (257, 129)]), ("int4_blockwise128", [(32, 1024), (64, 384)]),
                       ("int16", [(96, 200), (1, 7)]), ("int32_bias", [(4099,), (1,)]), ("fp16", [(128, 300), (3,)])):
    for j, shape in enumerate(shapes):
      out.append({"name": f"{form}_{'x'.join(map(str, shape))}", "seed": 600 + 10 * len(out) + j,
                  "shape": list(shape), "n": int(np.prod(shape)), "corruption": "quantized", "form": form})
  return out


def _float_pair(case):
  rng = np.random.default_rng(case["seed"])
  n = case["n"]
  r = (rng.standard_normal(n) * rng.uniform(0.1, 10.0)).astype(np.float32)
  t = (r + rng.standard_normal(n).astype(np.float32) * np.float32(0.05)).astype(np.float32)
  c = case["corruption"]
  if c == "nonfinite":
    t[rng.integers(0, n, 3)] = [np.nan, np.inf, -np.inf]
    r[rng.integers(0, n, 3)] = [np.inf, np.nan, -np.inf]
  elif c == "zeros":
    t[:] = 0
    r[:] = 0
  elif c == "zero_target":
    t[:] = 0
  elif c == "zero_reference":
    r[:] = 0
  elif c == "negative":
    t, r = -np.abs(t), (np.abs(r) - np.float32(1.0)).astype(np.float32)
  elif c == "ties":
    t, r = np.round(t, 1).astype(np.float32), np.round(r, 1).astype(np.float32)
  return t, r, {"kind": "f32", "data": t, "scale": None, "zp": None, "channels": 1, "inner": 1}


def make(case):
  if case["form"] == "f32":
    return _float_pair(case)
  rng = np.random.default_rng(case["seed"])
  shape = tuple(case["shape"])
  form = case["form"]
  x = (rng.standard_normal(shape) * 0.05).astype(np.float32)
  if form == "fp16":
    h = x.astype(np.float16)
    return h.astype(np.float32).ravel(), x.ravel(), {"kind": "f16", "data": h.ravel(), "scale": None, "zp": None,
                                                     "channels": 1, "inner": 1}
  if form == "int8_channelwise":
    scale = (np.max(np.abs(x), axis=1) / 127).astype(np.float32)
    zp = rng.integers(-2, 3, shape[0]).astype(np.int32)
    q = O.uniform_quantize(x, scale[:, None], zp[:, None], 8, False, quantized_dim=0)
    deq = O.uniform_dequantize(q, scale[:, None], zp[:, None], quantized_dim=0)
    stored = {"kind": "i8", "data": q.ravel(), "scale": scale, "zp": zp, "channels": shape[0], "inner": shape[1]}
  elif form == "int16":
    scale = np.array([np.max(np.abs(x)) / 32767], np.float32)
    zp = np.zeros(1, np.int32)
    one = [1] * x.ndim
    q = O.uniform_quantize(x, scale.reshape(one), zp.reshape(one), 16, True)
    deq = O.uniform_dequantize(q, scale.reshape(one), zp.reshape(one))
    stored = {"kind": "i16", "data": q.ravel(), "scale": scale, "zp": zp, "channels": 1, "inner": 1}
  elif form == "int32_bias":
    scale = np.array([1.37e-6], np.float32)
    zp = np.zeros(1, np.int32)
    one = [1] * x.ndim
    q = O.uniform_quantize(x, scale.reshape(one), zp.reshape(one), 32, True)
    deq = O.uniform_dequantize(q, scale.reshape(one), zp.reshape(one))   # int32 * float32: float64
    stored = {"kind": "i32", "data": q.ravel(), "scale": scale, "zp": zp, "channels": 1, "inner": 1}
  elif form == "int4_blockwise128":
    rows, cols = shape
    xb = x.reshape(rows, cols // 128, 128)
    scale = (np.max(np.abs(xb), axis=2) / 7).astype(np.float16).astype(np.float32)
    zp = np.zeros(scale.shape, np.int32)
    q = O.uniform_quantize(x, scale, zp, 4, True, quantized_dim=1, block_size=128, is_blockwise_quant=True)
    deq = O.uniform_dequantize(q, scale, zp, quantized_dim=1, block_size=128)
    stored = {"kind": "i4", "data": O.pack_data(4, q), "scale": scale.ravel(), "zp": None,
              "channels": scale.size, "inner": 128}
  else:
    raise ValueError(form)
  return np.asarray(deq, np.float32).ravel(), x.ravel(), stored
