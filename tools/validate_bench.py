"""Tensor comparison (model validation) timings on one MI355X: prints one JSON line.

4096 x 4096 float32 reference against an int8 channelwise, an int4 blockwise-128 and an fp16 target:
  * us per call of the five-metric comparison and of MSE alone: wall clock per warm call from Python, host staging,
    allocation and the copy of the results included (the kernels alone: rocprofv3 --kernel-trace --stats);
  * the fraction of the HBM peak (8.0 TB/s) that one read of both operands in that time is;
  * the reference's NumPy functions over the same (dequantized) arrays: the median, the subtractions and the sums run
    on one core, the BLAS dot / norm with the process's OMP_NUM_THREADS (reported as `numpy_blas_threads`);
  * the constants pass of compare_model on the 32-layer C3-shaped model file (blockwise-128 int4 target).
Usage: python tools/validate_bench.py [--iters N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ai-edge-quantizer_amd"))

HBM_PEAK = 8.0e12


def _np_five(t, r):
  """The reference's five functions (utils/validation_utils.py) in NumPy, as compare_model calls them."""
  def prep(a):
    return np.nan_to_num(np.ravel(np.asarray(a, np.float32)), nan=1e-9, neginf=-1e9, posinf=1e9)
  d1, d2 = prep(t), prep(r)
  mse = float(np.square(np.subtract(d1, d2)).mean())
  np.median(abs(d1 - d2) / (abs(d2) + 1e-6))
  np.dot(d1, d2) / (np.linalg.norm(d1) * np.linalg.norm(d2))
  p, q = np.maximum(0, d2), np.maximum(0, d1)
  float(np.sum(p * np.log((p + 1e-9) / (q + 1e-9))))
  float(np.square(d2).mean()) / (mse + 1e-9)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--numpy-iters", type=int, default=2)
  ap.add_argument("--layers", type=int, default=32, help="layers of the model-file pass (0: skip it)")
  args = ap.parse_args()
  import torch
  import __graft_entry__ as g
  g.build()
  from mi355q import ops
  from mi355q.utils import validation_utils as vu

  rows = cols = 4096
  n = rows * cols
  rng = np.random.default_rng(0)
  x = rng.standard_normal((rows, cols)).astype(np.float32)
  ref = torch.from_numpy(x).cuda()
  s8 = (np.abs(x).max(axis=1) / 127).astype(np.float32)
  q8 = np.clip(np.rint(x / s8[:, None]), -128, 127).astype(np.int8)
  xb = x.reshape(rows, cols // 128, 128)
  s4 = (np.abs(xb).max(axis=2) / 7).astype(np.float16).astype(np.float32)
  q4 = np.clip(np.rint(xb / s4[..., None]), -8, 7).astype(np.int8).reshape(-1)
  packed = ((q4[0::2].astype(np.uint8) & 0xF) | ((q4[1::2].astype(np.uint8) & 0xF) << 4)).astype(np.uint8)
  h = x.astype(np.float16)
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  targets = {
      "int8_channelwise": (ops.CompareTarget(dev(q8), n, "i8", dev(s8), dev(np.zeros(rows, np.int32)), rows, cols, 32),
                           q8.size, (q8.astype(np.int32) * s8[:, None]).astype(np.float32)),
      "int4_blockwise128": (ops.CompareTarget(dev(packed), n, "i4", dev(s4.ravel()), None, s4.size, 128, 32),
                            packed.size, (q4.reshape(xb.shape).astype(np.int32) * s4[..., None]).astype(np.float32)),
      "fp16": (ops.CompareTarget(dev(h), n, "f16"), h.nbytes, h.astype(np.float32)),
  }
  out = {"shape": [rows, cols], "hbm_peak_tbs": HBM_PEAK / 1e12, "targets": {},
         "numpy_blas_threads": os.environ.get("OMP_NUM_THREADS", "default")}
  for name, (tgt, tbytes, deq) in targets.items():
    res = {}
    for label, metrics in (("five", None), ("mse_only", [vu.ValidationErrorMetric.MSE])):
      for _ in range(3):
        vu.compare_all(tgt, ref, metrics)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.iters):
        vu.compare_all(tgt, ref, metrics)
      torch.cuda.synchronize()
      us = (time.perf_counter() - t0) / args.iters * 1e6
      one_read = (n * 4 + tbytes) / HBM_PEAK * 1e6
      res[label] = {"us_per_call": round(us, 1), "one_read_us": round(one_read, 1),
                    "fraction_of_hbm_peak": round(one_read / us, 3)}
    t0 = time.perf_counter()
    for _ in range(args.numpy_iters):
      _np_five(deq, x)
    res["numpy_five_us"] = round((time.perf_counter() - t0) / args.numpy_iters * 1e6, 1)
    res["speedup_vs_numpy"] = round(res["numpy_five_us"] / res["five"]["us_per_call"], 1)
    out["targets"][name] = res

  # the constants pass of compare_model on the C3-shaped file that tests/test_gpu_batching.py builds
  # (32 FULLY_CONNECTED layers of 4096 x 11008 float32) against its blockwise-128 int4 form
  if args.layers:
    import tempfile
    from mi355q import model_validator as mv
    from mi355q import quantizer, recipe
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import file_bench
    with tempfile.TemporaryDirectory() as tmp:
      src = os.path.join(tmp, "c3.tflite")
      file_bench.build_model(src, args.layers, 4096, 11008)
      qz = quantizer.Quantizer(src, recipe.dynamic_wi4b128_afp32())
      qz.quantize()
      model, qbytes = open(src, "rb").read(), bytes(qz._result.quantized_model)
      del qz
      t0 = time.perf_counter()
      got = mv.compare_constants(model, qbytes, list(vu.ValidationErrorMetric))
      torch.cuda.synchronize()
      out["model_constants"] = {"layers": args.layers, "tensors": len(got),
                                "ms": round((time.perf_counter() - t0) * 1e3, 1)}
  print(json.dumps(out))


if __name__ == "__main__":
  main()
