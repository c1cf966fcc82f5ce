#!/usr/bin/env python3
"""Times the direct depthwise convolution of csrc/dwconv.hip beside a device-to-device copy of the same traffic, on
N = 8 images of 112x112x32, 56x56x128, 14x14x512 and 7x7x1024 under a 3x3 SAME filter at stride 1 and 2 (depth
multiplier 1: the vector route), per-channel int8 filters:

  python tools/dwconv_bench.py [--repeats 15] [--launches 10] [--warmup 3] [--out profiles/dwconv_bench.json]

  f32       ops.dwconv_forward of the float32 tensor (reads x, writes float32 [N OH OW, C]);
  i8        ops.dwconv_forward of the int8 tensor (reads x, writes float32);
  i8_out    ops.dwconv_output of the int8 tensor (reads x, writes int8);
  copy      per entry, Tensor.copy_ of (bytes of x + bytes of the output) / 2 bytes: a copy reads and writes what it
            moves, so its traffic is the bytes the entry must read and write. That copy is the floor of a kernel bound
            by memory (the filter, 9 C elements, and the per-channel vectors are not counted: they stay in cache).

A launch here moves 0.1 - 26 MB and lasts microseconds, less than a call takes to enqueue, so a plain event-timed loop
would time the host. Every timed segment is therefore enqueued BEHIND a long matrix product on the same stream: while
the device is busy with it the host enqueues `--launches` back-to-back calls between two events, and the events then
bracket the device's own time for them (kernel time plus the dispatch gap between dependent launches, which the copy
pays as well). The entries and their copies alternate within every repeat, in one process; every figure is the median
over --repeats of a segment's time divided by the launches, after --warmup untimed rounds. There is no gate: the
figures are recorded. One JSON line, also written to --out.
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

BATCH = 8
SHAPES = ((112, 112, 32), (56, 56, 128), (14, 14, 512), (7, 7, 1024))      # (H, W, C)
STRIDES = (1, 2)
ZERO_POINT = -3
BLOCKER = 6144      # the matrix product in front of a timed segment: milliseconds of device time


def _behind_a_busy_device_ms(torch, fns: dict, warmup, repeats, launches) -> dict:
  """{name: {"ms": median, "ms_min_max": [...]}} of the device's time per launch; within a repeat every fn in turn."""
  a = torch.randn((BLOCKER, BLOCKER), device="cuda")
  for _ in range(warmup):
    torch.mm(a, a)
    for fn in fns.values():
      for _ in range(launches):
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


def bench_shape(torch, ops, h, w, c, stride, args):
  g = torch.Generator(device="cuda").manual_seed(h * c + stride)
  xf = torch.randn((BATCH, h, w, c), generator=g, device="cuda")
  x8 = torch.randint(-128, 128, (BATCH, h, w, c), generator=g, device="cuda", dtype=torch.int8)
  oh, ow, _, _ = ops.conv_geometry(h, w, 3, 3, stride, 1, "SAME")
  rows = BATCH * oh * ow
  wf = torch.randn((3, 3, c), generator=g, device="cuda")
  q = torch.randint(-127, 128, (3, 3, c), generator=g, device="cuda", dtype=torch.int8)
  scale = torch.rand((c,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(q, 9 * c, "i8", scale, None, c, 1, 32)
  x_scale = torch.full((1,), 0.02, device="cuda")
  bias = torch.randint(-3000, 3000, (c,), generator=g, device="cuda", dtype=torch.int32)
  tables = ops.qfc_multipliers([ops.quantize_multiplier(0.003)[0]] * c, [ops.quantize_multiplier(0.003)[1]] * c, c, 8)
  traffic = {"f32": xf.numel() * 4 + rows * c * 4, "i8": x8.numel() + rows * c * 4, "i8_out": x8.numel() + rows * c}
  fns = {"f32": lambda: ops.dwconv_forward(xf, wf, 3, 3, stride, 1, "SAME"),
         "i8": lambda: ops.dwconv_forward(x8, target, 3, 3, stride, 1, "SAME", x_scale=x_scale, x_zero_point=ZERO_POINT),
         "i8_out": lambda: ops.dwconv_output(x8, ZERO_POINT, target, 3, 3, stride, 1, "SAME", bias, tables, None, -5, -128, 127)}
  for name, nbytes in traffic.items():
    src = torch.randint(-128, 128, (nbytes // 2,), generator=g, device="cuda", dtype=torch.int8)
    dst = torch.empty_like(src)
    fns[name + "_copy"] = (lambda d, s: lambda: d.copy_(s))(dst, src)
  t = _behind_a_busy_device_ms(torch, fns, args.warmup, args.repeats, args.launches)
  out = {"input": [BATCH, h, w, c], "filter": [3, 3, c], "stride": stride, "output_hw": [oh, ow], "rows": rows}
  for name, nbytes in traffic.items():
    out[name] = {"bytes_read_and_written": nbytes, "ms": t[name]["ms"], "ms_min_max": t[name]["ms_min_max"],
                 "copy_ms": t[name + "_copy"]["ms"], "copy_ms_min_max": t[name + "_copy"]["ms_min_max"],
                 "gb_per_s": nbytes / (t[name]["ms"] * 1e-3) / 1e9,
                 "copy_gb_per_s": nbytes / (t[name + "_copy"]["ms"] * 1e-3) / 1e9,
                 "over_copy": t[name]["ms"] / t[name + "_copy"]["ms"]}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwconv_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("dwconv_bench needs a GPU")
  layers = [bench_shape(torch, ops, h, w, c, stride, args) for h, w, c in SHAPES for stride in STRIDES]
  result = {"tool": "dwconv_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "batch": BATCH, "layers": layers,
            "largest_over_copy": {name: max(r[name]["over_copy"] for r in layers) for name in ("f32", "i8", "i8_out")},
            "over_copy_on_the_largest_shape": {name: layers[0][name]["over_copy"] for name in ("f32", "i8", "i8_out")}}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
