#!/usr/bin/env python3
"""Times the int16-activation integer FULLY_CONNECTED kernel of csrc/qfc16.hip on 2048 tokens x the projection shapes
the other tools use (2048 -> 16384, 16384 -> 2048, 4096 -> 4096), int8 per channel and int4 blockwise-128, each beside
its two yardsticks on the same shape:

  python tools/qfc16_bench.py [--repeats 15] [--launches 8] [--warmup 3] [--out profiles/qfc16_bench.json]

  qfc_forward_i16   ops.qfc_forward_i16 on a static int16 activation (ops.quantize, 16 bits);
  qfc_forward_i8    ops.qfc_forward on the dynamic int8 rows of the same x (half the MFMAs and activation bytes over
                    the same weight bytes and unpacking: the i16 form should cost about twice this);
  dequantize_gemm   ops.dequantize (after ops.unpack_bits for int4) followed by ops.gemm in FP32: what a user would
                    otherwise do to execute the op without the activation's int8 rounding.

The three alternate within every repeat, in one process: a repeat times --launches back-to-back launches of each with
device events, and every figure is the median over --repeats of that time divided by the launches, after --warmup
untimed rounds. The i16 forward must be faster than the FP32 route on every row (exit status 1 otherwise); its ratio
to the i8 forward is recorded, not required. One JSON line, also written to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "ai-edge-quantizer_amd"), ROOT, os.path.join(ROOT, "tools")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

TOKENS = 2048
SHAPES = ((16384, 2048), (2048, 16384), (4096, 4096))      # (rows, d) of the weight


def _alternating_ms(torch, fns: dict, warmup, repeats, launches) -> dict:
  """{name: {"ms": median, "ms_min_max": [...]}}; within a repeat every fn is timed in turn."""
  for _ in range(warmup):
    for fn in fns.values():
      for _ in range(launches):
        fn()
  torch.cuda.synchronize()
  times = {name: [] for name in fns}
  for _ in range(repeats):
    for name, fn in fns.items():
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(launches):
        fn()
      stop.record()
      stop.synchronize()
      times[name].append(start.elapsed_time(stop) / launches)
  return {name: {"ms": statistics.median(t), "ms_min_max": [min(t), max(t)]} for name, t in times.items()}


def bench_row(torch, ops, rows, d, kind, args):
  g = torch.Generator(device="cuda").manual_seed(rows + d)
  x = torch.randn((TOKENS, d), generator=g, device="cuda")
  xq8, x_scale8 = ops.qfc_quantize_rows(x)
  s16 = (x.abs().max() / 32767.0).to(torch.float32).view(1)
  xq16 = ops.quantize(x, 1, 1, x.numel(), s16, torch.zeros(1, dtype=torch.int32, device="cuda"), 16, False)
  q = torch.randint(-127 if kind == "i8" else -8, 128 if kind == "i8" else 8, (rows, d), generator=g, device="cuda",
                    dtype=torch.int8)
  if kind == "i8":
    channels, inner, stored = rows, d, q
  else:
    channels, inner, stored = rows * d // 128, 128, ops.pack_bits(q, 4)
  scale = torch.rand((channels,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(stored, rows * d, kind, scale, None, channels, inner, 32)

  def i16():
    return ops.qfc_forward_i16(xq16, s16, target, rows, d)

  def i8():
    return ops.qfc_forward(xq8, x_scale8, 0, target, rows, d)

  def dequantize_then_gemm():
    ints = stored if kind == "i8" else ops.unpack_bits(stored, rows * d, 4)
    w = ops.dequantize(ints.view(-1), 1, channels, inner, scale, None, 8)
    return ops.gemm(x, w.view(rows, d), trans_b=True)
  a, b, c = i16(), i8(), dequantize_then_gemm()
  torch.cuda.synchronize()
  rel16, rel8 = float((a - c).norm() / c.norm()), float((b - c).norm() / c.norm())
  t = _alternating_ms(torch, {"i16": i16, "i8": i8, "f32": dequantize_then_gemm}, args.warmup, args.repeats, args.launches)
  macs = 2.0 * TOKENS * rows * d
  return {"rows": rows, "d": d, "tokens": TOKENS, "weight": "int8 per channel" if kind == "i8" else "int4 blockwise-128",
          "qfc_forward_i16_ms": t["i16"]["ms"], "qfc_forward_i16_ms_min_max": t["i16"]["ms_min_max"],
          "qfc_forward_i8_ms": t["i8"]["ms"], "qfc_forward_i8_ms_min_max": t["i8"]["ms_min_max"],
          "dequantize_gemm_f32_ms": t["f32"]["ms"], "dequantize_gemm_f32_ms_min_max": t["f32"]["ms_min_max"],
          "i16_over_i8": t["i16"]["ms"] / t["i8"]["ms"], "f32_route_over_i16": t["f32"]["ms"] / t["i16"]["ms"],
          "i16_faster_than_f32_route": t["i16"]["ms"] < t["f32"]["ms"],
          "i16_int8_mfma_tops": 2.0 * macs / (t["i16"]["ms"] * 1e-3) / 1e12,      # (two int8 planes)
          "f32_gemm_route_tflops": macs / (t["f32"]["ms"] * 1e-3) / 1e12,
          "relative_difference_i16_to_f32_route": rel16, "relative_difference_i8_to_f32_route": rel8}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=8)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qfc16_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("qfc16_bench needs a GPU")
  forward = [bench_row(torch, ops, rows, d, kind, args) for rows, d in SHAPES for kind in ("i8", "i4")]
  result = {"tool": "qfc16_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "forward": forward,
            "i16_faster_than_f32_route_on_every_row": all(r["i16_faster_than_f32_route"] for r in forward)}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)
  if not result["i16_faster_than_f32_route_on_every_row"]:
    raise SystemExit(1)


if __name__ == "__main__":
  main()
