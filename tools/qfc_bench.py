#!/usr/bin/env python3
"""Times the integer execution kernels of csrc/qfc.hip on 2048 tokens x the projection shapes the other tools use
(2048 -> 16384, 16384 -> 2048, 4096 -> 4096), each beside what a user would otherwise do on the same shape.

  python tools/qfc_bench.py [--repeats 15] [--launches 8] [--warmup 3] [--out profiles/qfc_bench.json]

  quantize_rows   ops.qfc_quantize_rows on x [2048, d]: 4 bytes read + 1 written per element;
  forward         ops.qfc_forward, int8 per channel and int4 blockwise-128, against ops.dequantize (after
                  ops.unpack_bits for int4) followed by ops.gemm in FP32 on the same shape;
  sqdiff_cols     ops.sqdiff_cols on two [2048, rows] outputs: 8 bytes read per element.

Every figure is the median over --repeats of the device-event time of --launches back-to-back launches, divided by the
launches, after --warmup untimed rounds. The memory-bound kernels rotate through enough input buffers to exceed the
256 MiB of last-level cache, so their bytes come from HBM. `forward` reports its rate in int8 TOPS (2 n rows d per
call) and the fraction of the 5 POPS dense int8 matrix peak. No ratio is required: the numbers are recorded.
One JSON line, also written to --out.
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
I8_PEAK_TOPS = 5000.0
CACHE_BYTES = 256 << 20


def _per_launch_ms(torch, fn, warmup, repeats, launches):
  """fn(i) enqueues launch i (i picks the buffer of a rotation)."""
  for w in range(warmup):
    for i in range(launches):
      fn(w * launches + i)
  torch.cuda.synchronize()
  times = []
  for r in range(repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(launches):
      fn(r * launches + i)
    stop.record()
    stop.synchronize()
    times.append(start.elapsed_time(stop) / launches)
  return {"ms": statistics.median(times), "ms_min_max": [min(times), max(times)]}


def _rotation(nbytes: int) -> int:
  return max(2, min(48, -(-2 * CACHE_BYTES // nbytes)))


def bench_quantize_rows(torch, ops, d, args):
  count = _rotation(TOKENS * d * 4)
  g = torch.Generator(device="cuda").manual_seed(d)
  xs = [torch.randn((TOKENS, d), generator=g, device="cuda") for _ in range(count)]
  t = _per_launch_ms(torch, lambda i: ops.qfc_quantize_rows(xs[i % count]), args.warmup, args.repeats, args.launches)
  t.update(d=d, tokens=TOKENS, buffers=count, GBps=TOKENS * d * 5 / (t["ms"] * 1e-3) / 1e9)
  return t


def bench_sqdiff(torch, ops, rows, args):
  count = _rotation(2 * TOKENS * rows * 4)
  g = torch.Generator(device="cuda").manual_seed(rows)
  pairs = [(torch.randn((TOKENS, rows), generator=g, device="cuda"), torch.randn((TOKENS, rows), generator=g, device="cuda"))
           for _ in range(count)]
  t = _per_launch_ms(torch, lambda i: ops.sqdiff_cols(*pairs[i % count]), args.warmup, args.repeats, args.launches)
  t.update(rows=rows, tokens=TOKENS, buffers=count, GBps=TOKENS * rows * 8 / (t["ms"] * 1e-3) / 1e9)
  return t


def bench_forward(torch, ops, rows, d, kind, args):
  g = torch.Generator(device="cuda").manual_seed(rows + d)
  x = torch.randn((TOKENS, d), generator=g, device="cuda")
  xq, x_scale = ops.qfc_quantize_rows(x)
  q = torch.randint(-127 if kind == "i8" else -8, 128 if kind == "i8" else 8, (rows, d), generator=g, device="cuda",
                    dtype=torch.int8)
  if kind == "i8":
    channels, inner, stored = rows, d, q
  else:
    channels, inner, stored = rows * d // 128, 128, ops.pack_bits(q, 4)
  scale = torch.rand((channels,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(stored, rows * d, kind, scale, None, channels, inner, 32)

  def integer(_):
    return ops.qfc_forward(xq, x_scale, 0, target, rows, d)

  def dequantize_then_gemm(_):
    ints = stored if kind == "i8" else ops.unpack_bits(stored, rows * d, 4)
    w = ops.dequantize(ints.view(-1), 1, channels, inner, scale, None, 8)
    return ops.gemm(x, w.view(rows, d), trans_b=True)
  a, b = integer(0), dequantize_then_gemm(0)
  torch.cuda.synchronize()
  rel = float((a - b).norm() / b.norm())      # (the integer route also rounds x to int8 rows: percent, not bits)
  ti = _per_launch_ms(torch, integer, args.warmup, args.repeats, args.launches)
  tf = _per_launch_ms(torch, dequantize_then_gemm, args.warmup, args.repeats, args.launches)
  tops = 2.0 * TOKENS * rows * d / (ti["ms"] * 1e-3) / 1e12
  return {"rows": rows, "d": d, "tokens": TOKENS, "weight": "int8 per channel" if kind == "i8" else "int4 blockwise-128",
          "qfc_forward_ms": ti["ms"], "qfc_forward_ms_min_max": ti["ms_min_max"],
          "dequantize_gemm_f32_ms": tf["ms"], "dequantize_gemm_f32_ms_min_max": tf["ms_min_max"],
          "ratio_to_dequantize_gemm": tf["ms"] / ti["ms"], "int8_tops": tops, "fraction_of_i8_peak": tops / I8_PEAK_TOPS,
          "f32_gemm_route_tflops": 2.0 * TOKENS * rows * d / (tf["ms"] * 1e-3) / 1e12,
          "relative_difference_of_the_outputs": rel}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=8)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qfc_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("qfc_bench needs a GPU")
  result = {"tool": "qfc_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "i8_peak_tops": I8_PEAK_TOPS,
            "quantize_rows": [bench_quantize_rows(torch, ops, d, args) for d in sorted({d for _, d in SHAPES})],
            "forward": [bench_forward(torch, ops, rows, d, kind, args) for rows, d in SHAPES for kind in ("i8", "i4")],
            "sqdiff_cols": [bench_sqdiff(torch, ops, rows, args) for rows in sorted({r for r, _ in SHAPES})]}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
