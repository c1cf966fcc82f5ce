#!/usr/bin/env python3
"""Times the integer BATCH_MATMUL of csrc/qbmm.hip on the two attention products of the config-5 geometry (8 heads,
head size 256) at 2048 tokens and on one product with a constant right-hand side:

  python tools/qbmm_bench.py [--repeats 15] [--launches 5] [--warmup 3] [--out profiles/qbmm_bench.json]

  qk      [8, 2048, 256] . [8, 2048, 256]^T    adj_y: both operands contiguous along K
  pv      [8, 2048, 2048] . [8, 2048, 256]     the default layout: b strided along K (the library transposes it first)
  const   [1, 2048, 2048] . [2048, 2048]       one constant matrix, the default layout

Per shape:
  qbmm        ops.qbmm_forward with both zero points non-zero (the operand sums included);
  fp32        (a) ops.dequantize of both operands + ops.gemm in float32 per batch: the only way to the number without
              this entry;
  qfc         (b) for batch = 1 and (adj_x, adj_y) = (False, True) (one head of qk): ops.qfc_forward on the identical
              problem, beside ops.qbmm_forward with b_zero_point = 0 (qfc_forward has no weight zero point). The
              library hands exactly this case (batch 1, adj_y, no b zero point) to the FULLY_CONNECTED entry, so the
              two sides run the same kernels;
  transposed  (c) for the K-strided layouts: an explicit int8 transpose of b (Tensor.transpose().contiguous()) followed
              by the direct route (adj_y), beside the library's own route on the same values. (A route that staged b
              through LDS inside the product lost this comparison 5.3 - 6.6 x, profiles/qbmm_staged_bench.json; the
              library's route is now a transposing pre-pass of its own, so the two sides differ in the transpose
              kernel and one allocation.)

Every timed segment is enqueued behind a long matrix product on the same stream (tools/dwconv_bench.py tells why), the
entries of a shape alternate within every repeat, and a figure is the median over --repeats of a segment's time
divided by its launches. The whole measurement runs TWICE in one process and both runs are recorded: the spread
between them is the yardstick for (b) and (c). There is no gate: the figures are recorded. One JSON line, also
written to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "ai-edge-quantizer_amd"), ROOT):
  if _p not in sys.path:
    sys.path.insert(0, _p)

SHAPES = (("qk", 8, 8, 2048, 2048, 256, True), ("pv", 8, 8, 2048, 256, 2048, False),
          ("const", 1, 1, 2048, 2048, 2048, False))      # (name, batch, b_batch, M, N, K, adj_y)
ZA, ZB = -3, 5
BLOCKER = 6144      # the matrix product in front of a timed segment: milliseconds of device time


def _behind_a_busy_device_ms(torch, fns: dict, warmup, repeats, launches) -> dict:
  a = torch.randn((BLOCKER, BLOCKER), device="cuda")
  for _ in range(warmup):
    torch.mm(a, a)
    for fn in fns.values():
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in fns}
  for _ in range(repeats):
    for name, fn in fns.items():
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.mm(a, a)
      start.record()
      for _ in range(launches):
        fn()
      stop.record()
      stop.synchronize()
      times[name].append(start.elapsed_time(stop) / launches)
  return {name: {"ms": statistics.median(t), "ms_min_max": [min(t), max(t)]} for name, t in times.items()}


def bench_shape(torch, ops, name, batch, b_batch, m, n, k, adj_y, args):
  g = torch.Generator(device="cuda").manual_seed(m + n + k)
  a = torch.randint(-128, 128, (batch, m, k), generator=g, device="cuda", dtype=torch.int8)
  b = torch.randint(-128, 128, (b_batch,) + ((n, k) if adj_y else (k, n)), generator=g, device="cuda", dtype=torch.int8)
  sa, sb = torch.full((1,), 0.02, device="cuda"), torch.full((1,), 0.01, device="cuda")
  za_t, zb_t = torch.tensor([ZA], device="cuda", dtype=torch.int32), torch.tensor([ZB], device="cuda", dtype=torch.int32)
  kw = dict(adj_x=False, a_scale=sa, a_zero_point=ZA, b_scale=sb)

  def fp32():
    af = ops.dequantize(a, 1, 1, a.numel(), sa, za_t, 8)
    bf = ops.dequantize(b, 1, 1, b.numel(), sb, zb_t, 8)
    return [ops.gemm(af[i], bf[i if b_batch != 1 else 0], trans_b=adj_y) for i in range(batch)]

  fns = {"qbmm": lambda: ops.qbmm_forward(a, b, adj_y=adj_y, b_zero_point=ZB, **kw), "fp32": fp32}
  if adj_y:      # (b): one head against the FULLY_CONNECTED entry
    a1, b1 = a[0].contiguous(), b[0].contiguous()
    target = ops.CompareTarget(b1.view(-1), b1.numel(), "i8", sb, None, 1, b1.numel(), 32)
    fns["qbmm_one_head"] = lambda: ops.qbmm_forward(a1, b1, adj_y=True, b_zero_point=0, **kw)
    fns["qfc_one_head"] = lambda: ops.qfc_forward(a1, sa, ZA, target, n, k)
  else:          # (c): transpose, then the direct route
    fns["transposed"] = lambda: ops.qbmm_forward(a, b.transpose(-1, -2).contiguous(), adj_y=True, b_zero_point=ZB, **kw)
  runs = [_behind_a_busy_device_ms(torch, fns, args.warmup, args.repeats, args.launches) for _ in range(2)]
  ops_count = 2.0 * batch * m * n * k
  out = {"name": name, "a": list(a.shape), "b": list(b.shape), "adj_y": adj_y, "zero_points": [ZA, ZB], "runs": runs,
         "qbmm_tops": [ops_count / (r["qbmm"]["ms"] * 1e-3) / 1e12 for r in runs],
         "fp32_over_qbmm": [r["fp32"]["ms"] / r["qbmm"]["ms"] for r in runs]}
  if adj_y:
    out["qbmm_over_qfc_one_head"] = [r["qbmm_one_head"]["ms"] / r["qfc_one_head"]["ms"] for r in runs]
  else:
    out["qbmm_over_transposed"] = [r["qbmm"]["ms"] / r["transposed"]["ms"] for r in runs]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qbmm_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("qbmm_bench needs a GPU")
  shapes = [bench_shape(torch, ops, *s, args) for s in SHAPES]
  result = {"tool": "qbmm_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "shapes": shapes}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
