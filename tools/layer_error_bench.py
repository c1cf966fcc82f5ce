#!/usr/bin/env python3
"""Times the layer-output-error quadratic form (ops.quadform_rows, csrc/layer_error.hip) against the composition the
library offered before it: ops.gemm(a, P mirrored to both triangles) followed by a float64 row dot in torch.

  python tools/layer_error_bench.py [--repeats 20] [--warmup 3] [--model-layers 2] [--out profiles/layer_error_bench.json]

Shapes: a [16384, 2048] against a d = 2048 product (gate / up of BASELINE config 5) and a [2048, 16384] against a
d = 16384 product (down). Medians of device-event times; the mirrored matrix is prepared outside the timing. The new
kernel reads half the products and writes no rows x d intermediate, so it must not be slower at either shape
(`not_slower`). With --model-layers N > 0 one Quantizer.validate_layer_outputs call on the N-layer full-shape model
of tests/test_gpu_c5_model.py (GPTQ int4) is timed too. One JSON line, also written to --out.

With --transforms the effective-weight delta behind an inserted transformation (ops.weight_delta_transformed, one
launch) is timed against the three launches the library offered before it -- ops.weight_delta against zeros (the one
route to a packed target's float32 values), then ops.hadamard_rotate or a torch multiply, then a torch add -- in one
process, the two alternating, medians of --repeats: [2048, 16384] int4 per channel with h = 2048 (down of BASELINE
config 5) and [16384, 2048] int4 per channel with a multiplier. The rows go to `transforms`; no ratio is required.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "ai-edge-quantizer_amd"), ROOT, os.path.join(ROOT, "tools")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

SHAPES = ((16384, 2048), (2048, 16384))


def _median_ms(torch, fn, warmup, repeats):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    times.append(start.elapsed_time(stop))
  return statistics.median(times), min(times), max(times)


def bench_shape(torch, ops, lib, rows, d, warmup, repeats):
  g = torch.Generator(device="cuda").manual_seed(rows + d)
  a = torch.randn((rows, d), generator=g, device="cuda") * 0.02
  x = torch.randn((4096, d), generator=g, device="cuda")
  product = torch.tril(ops.gemm(x, x, trans_a=True))            # lower triangle of X^T X, zeros above
  del x
  mirrored = product + torch.tril(product, -1).T
  alpha = 0.5 * 2.0 / 8.0

  def new():
    return ops.quadform_rows(a, product, alpha)

  def old():
    c = ops.gemm(a, mirrored)
    return alpha * (c.double() * a.double()).sum(dim=1)
  got, want = new(), old()
  torch.cuda.synchronize()
  rel = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
  new_ms, new_lo, new_hi = _median_ms(torch, new, warmup, repeats)
  old_ms, old_lo, old_hi = _median_ms(torch, old, warmup, repeats)
  flops_new = float(rows) * d * (d + 1)          # 2 flops for each of the rows * d (d + 1) / 2 products
  flops_old = 2.0 * rows * d * d
  return {"rows": rows, "d": d, "quadform_ms": new_ms, "quadform_ms_min_max": [new_lo, new_hi],
          "gemm_then_rowdot_ms": old_ms, "gemm_then_rowdot_ms_min_max": [old_lo, old_hi],
          "quadform_tflops": flops_new / (new_ms * 1e-3) / 1e12,
          "gemm_then_rowdot_tflops": flops_old / (old_ms * 1e-3) / 1e12,
          "speedup": old_ms / new_ms, "not_slower": new_ms <= old_ms,
          "workspace_bytes": int(lib.mi355q_quadform_rows_workspace_bytes(rows, d)),
          "intermediate_bytes_of_the_composition": rows * d * 4 + 2 * rows * d * 8,
          "max_rel_difference": rel}


TRANSFORM_SHAPES = ((2048, 16384, "hadamard", 2048), (16384, 2048, "multiply", 0))


def bench_transform(torch, ops, rows, d, form, h, warmup, repeats):
  g = torch.Generator(device="cuda").manual_seed(rows + d + h)
  n = rows * d
  w = torch.randn((n,), generator=g, device="cuda") * 0.02
  packed = torch.randint(0, 256, (n // 2,), generator=g, device="cuda", dtype=torch.uint8)
  scale = torch.rand((rows,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(packed, n, "i4", scale, None, rows, d, 32)
  mult = (torch.rand((d,), generator=g, device="cuda") + 0.5) if form == "multiply" else None
  zeros = torch.zeros((n,), dtype=torch.float32, device="cuda")

  def fused():
    return ops.weight_delta_transformed(w, target, d, multiplier=mult, hadamard_size=h)

  def composed():
    minus_dq = ops.weight_delta(zeros, target)                        # 0 - dequant(target)
    if form == "hadamard":
      return w + ops.hadamard_rotate(minus_dq, h)                      # (the rotation is linear: the sign is exact)
    return w + (minus_dq.view(rows, d) * mult.view(1, d)).view(-1)
  same = bool(torch.equal(fused().view(torch.int32), composed().view(torch.int32)))
  for _ in range(warmup):
    fused()
    composed()
  torch.cuda.synchronize()
  times = {"fused": [], "composed": []}
  for _ in range(repeats):                                            # alternating: both see the same clocks
    for key, fn in (("fused", fused), ("composed", composed)):
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      fn()
      stop.record()
      stop.synchronize()
      times[key].append(start.elapsed_time(stop))
  f_ms, c_ms = statistics.median(times["fused"]), statistics.median(times["composed"])
  bytes_fused = n * (0.5 + 4 + 4)
  bytes_composed = n * (0.5 + 4 + 4) + n * 8 + n * 12                  # delta against zeros, rotate / multiply, add
  return {"rows": rows, "d": d, "target": "int4 per channel", "form": form, "hadamard_size": h,
          "fused_ms": f_ms, "fused_ms_min_max": [min(times["fused"]), max(times["fused"])],
          "composed_ms": c_ms, "composed_ms_min_max": [min(times["composed"]), max(times["composed"])],
          "speedup": c_ms / f_ms, "fused_GBps": bytes_fused / (f_ms * 1e-3) / 1e9,
          "composed_GBps": bytes_composed / (c_ms * 1e-3) / 1e9, "bytes_per_element": [8.5, bytes_composed / n],
          "temporaries_of_the_composition_bytes": 2 * n * 4, "same_bits": same}


def bench_model(torch, layers, sequences, tokens):
  import c5_model as C
  from mi355q import quantizer
  model = C.build_model(layers)
  samples = C.calibration_set(torch, layers, sequences, tokens)
  qz = quantizer.Quantizer(model, C.recipe("gptq"))
  qsvs = qz.calibrate({"serving_default": samples})
  qz.quantize(qsvs)
  torch.cuda.synchronize()
  times = []
  for _ in range(2):                 # the second call has warm allocations
    t0 = time.perf_counter()
    res = qz.validate_layer_outputs(calibration_result=qsvs)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
  worst = min(res.results.items(), key=lambda kv: kv[1]["output_snr"])
  return {"layers": layers, "sequences": sequences, "tokens": tokens, "ops_reported": len(res.results),
          "ops_skipped": len(res.skipped), "validate_layer_outputs_s": times,
          "lowest_output_snr": [worst[0], worst[1]["output_snr"]]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--model-layers", type=int, default=2)
  ap.add_argument("--sequences", type=int, default=64)
  ap.add_argument("--tokens", type=int, default=512)
  ap.add_argument("--transforms", action="store_true", help="time the transformed weight delta against its composition")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_error_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import _ffi, ops
  if not torch.cuda.is_available():
    raise SystemExit("layer_error_bench needs a GPU")
  result = {"tool": "layer_error_bench", "device": ops.device_info(), "repeats": args.repeats, "warmup": args.warmup,
            "shapes": [bench_shape(torch, ops, _ffi.lib(), rows, d, args.warmup, args.repeats) for rows, d in SHAPES]}
  result["not_slower"] = all(s["not_slower"] for s in result["shapes"])
  if args.model_layers > 0:
    result["model"] = bench_model(torch, args.model_layers, args.sequences, args.tokens)
  if args.transforms:
    result["transforms"] = [bench_transform(torch, ops, rows, d, form, h, args.warmup, args.repeats)
                            for rows, d, form, h in TRANSFORM_SHAPES]
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
