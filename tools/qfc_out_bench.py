#!/usr/bin/env python3
"""Times the stored-output kernels of csrc/qfc_out.hip on 2048 tokens x the projection shapes the other tools use
(2048 -> 16384, 16384 -> 2048, 4096 -> 4096), int8 per channel, each beside the forward entry it extends:

  python tools/qfc_out_bench.py [--repeats 15] [--launches 8] [--warmup 3] [--out profiles/qfc_out_bench.json]

  qfc_output        ops.qfc_output: int8 activations (zero point -3), int32 bias, one multiplier per channel, int8 out;
  qfc_forward       ops.qfc_forward on the same operands: the float32 rescale of the accumulator (the yardstick:
                    unchanged code);
  qfc_output_i16    ops.qfc_output_i16: int16 activations, int64 bias, one multiplier per channel, int16 out;
  qfc_forward_i16   ops.qfc_forward_i16 on the same operands (the yardstick).

The four alternate within every repeat, in one process: a repeat times --launches back-to-back launches of each with
device events, and every figure is the median over --repeats of that time divided by the launches, after --warmup
untimed rounds. The epilogue is O(n rows) beside an O(n rows d) product and stores 1 or 2 bytes per output instead of
4, so the ratios are expected near 1; they are recorded, not required. One JSON line, also written to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "ai-edge-quantizer_amd"), ROOT, os.path.join(ROOT, "tools")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

TOKENS = 2048
SHAPES = ((16384, 2048), (2048, 16384), (4096, 4096))      # (rows, d) of the weight
X_ZERO_POINT, OUT_ZERO_POINT = -3, 5


def bench_row(torch, ops, rows, d, args):
  from qfc16_bench import _alternating_ms
  g = torch.Generator(device="cuda").manual_seed(rows + d)
  x = torch.randn((TOKENS, d), generator=g, device="cuda")
  zero = torch.zeros(1, dtype=torch.int32, device="cuda")
  s8 = (x.abs().max() / 127.0).to(torch.float32).view(1)
  xq8 = ops.quantize(x, 1, 1, x.numel(), s8, zero + X_ZERO_POINT, 8, False)
  s16 = (x.abs().max() / 32767.0).to(torch.float32).view(1)
  xq16 = ops.quantize(x, 1, 1, x.numel(), s16, zero, 16, False)
  q = torch.randint(-127, 128, (rows, d), generator=g, device="cuda", dtype=torch.int8)
  scale = torch.rand((rows,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(q, rows * d, "i8", scale, None, rows, d, 32)
  # one multiplier per channel such that the outputs spread over the output type (acc is about sqrt(d) 37 73)
  spread = torch.rand((rows,), generator=g, device="cuda").cpu().numpy() + 0.5
  tables = {}
  for bits, x_rms, out in ((8, 37.0, 40.0), (16, 9400.0, 9000.0)):
    ms = [ops.quantize_multiplier(out * float(v) / (d ** 0.5 * x_rms * 73.0)) for v in spread]
    tables[bits] = ops.qfc_multipliers([v[0] for v in ms], [v[1] for v in ms], rows, bits)
  bias32 = torch.randint(-(1 << 16), 1 << 16, (rows,), generator=g, device="cuda", dtype=torch.int32)
  bias64 = torch.randint(-(1 << 24), 1 << 24, (rows,), generator=g, device="cuda", dtype=torch.int64)

  def out8():
    return ops.qfc_output(xq8, X_ZERO_POINT, target, rows, d, bias32, tables[8], None, OUT_ZERO_POINT, -128, 127)

  def fwd8():
    return ops.qfc_forward(xq8, s8, X_ZERO_POINT, target, rows, d)

  def out16():
    return ops.qfc_output_i16(xq16, target, rows, d, bias64, tables[16], None, -32768, 32767)

  def fwd16():
    return ops.qfc_forward_i16(xq16, s16, target, rows, d)
  a, b = out8(), out16()
  fwd8(), fwd16()
  torch.cuda.synchronize()
  # (that the outputs are spread, not all clamped: the epilogue's data-dependent selects see both sides)
  inside8 = float(((a > -128) & (a < 127)).float().mean())
  inside16 = float(((b > -32768) & (b < 32767)).float().mean())
  t = _alternating_ms(torch, {"out8": out8, "fwd8": fwd8, "out16": out16, "fwd16": fwd16}, args.warmup, args.repeats,
                      args.launches)
  macs = 2.0 * TOKENS * rows * d
  return {"rows": rows, "d": d, "tokens": TOKENS, "weight": "int8 per channel",
          "qfc_output_ms": t["out8"]["ms"], "qfc_output_ms_min_max": t["out8"]["ms_min_max"],
          "qfc_forward_ms": t["fwd8"]["ms"], "qfc_forward_ms_min_max": t["fwd8"]["ms_min_max"],
          "qfc_output_i16_ms": t["out16"]["ms"], "qfc_output_i16_ms_min_max": t["out16"]["ms_min_max"],
          "qfc_forward_i16_ms": t["fwd16"]["ms"], "qfc_forward_i16_ms_min_max": t["fwd16"]["ms_min_max"],
          "output_over_forward": t["out8"]["ms"] / t["fwd8"]["ms"],
          "output_i16_over_forward_i16": t["out16"]["ms"] / t["fwd16"]["ms"],
          "qfc_output_int8_mfma_tops": macs / (t["out8"]["ms"] * 1e-3) / 1e12,
          "qfc_output_i16_int8_mfma_tops": 2.0 * macs / (t["out16"]["ms"] * 1e-3) / 1e12,      # (two int8 planes)
          "fraction_of_outputs_inside_the_range": [inside8, inside16]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=8)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qfc_out_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("qfc_out_bench needs a GPU")
  rows_ = [bench_row(torch, ops, rows, d, args) for rows, d in SHAPES]
  result = {"tool": "qfc_out_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "shapes": rows_,
            "largest_output_over_forward": max(max(r["output_over_forward"], r["output_i16_over_forward_i16"]) for r in rows_)}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
