#!/usr/bin/env python3
"""Times the staged route of the integer FULLY_CONNECTED product (csrc/qfc_staged.h) against the generic kernel it
replaces, on the products that CONV_2D, TRANSPOSE_CONV phases and small FULLY_CONNECTED ops issue and that the aligned
MFMA route does not serve.

  python tools/qfc_staged_bench.py [--repeats 11] [--warmup 2] [--window-ms 40] [--out profiles/qfc_staged_bench.json]

Every row is ops.qfc_forward for static a8w8 (one activation scale, x_zero_point = 5, so the weight sums are part of
both sides; per-channel weight scales) in ONE process, three variants alternating within every repeat:
  generic_a, generic_b   inside ops.qfc_staged(False): the generic kernel, twice -- b / a is the tool's own spread;
  staged                 the default route.
A variant's figure is the median over --repeats of the device-event time of `launches` back-to-back calls divided by
the launches; `launches` is chosen per row so that a window of the generic kernel lasts about --window-ms. The ratios
are medians of the per-repeat ratios, with their smallest and largest. The last row (4096 x 4096 from an xq one byte
past an aligned base) also records the aligned MFMA route on the same problem from an aligned base, as context.
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

# (source, n = patch rows, rows, d, bytes xq lies past an aligned base)
SHAPES = (("stem 3x3x3 -> 32 at 112x112, N = 8", 100352, 32, 27, 0),
          ("1x1, 24 -> 144 at 56x56, N = 8", 25088, 144, 24, 0),
          ("3x3, 24 -> 24 at 56x56, N = 8", 25088, 24, 216, 0),
          ("1x1, 672 -> 112 at 14x14, N = 8", 1568, 112, 672, 0),
          ("TCONV phase 4x4 s2 over 24 ch, 28x28, N = 8", 6272, 64, 96, 0),
          ("FC, d = 1000", 2048, 4096, 1000, 0),
          ("4096 x 4096, xq one byte past an aligned base", 2048, 4096, 4096, 1))
ZERO_POINT = 5


def _window_ms(torch, fn, launches):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(launches):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) / launches


def _summary(times):
  return {"ms": statistics.median(times), "ms_min_max": [min(times), max(times)]}


def _ratio(num, den):
  r = [a / b for a, b in zip(num, den)]
  return {"median": statistics.median(r), "min_max": [min(r), max(r)]}


def bench(torch, ops, source, n, rows, d, offset, args):
  g = torch.Generator(device="cuda").manual_seed(n + rows + d)
  buf = torch.randint(-128, 128, (n * d + 16,), generator=g, device="cuda", dtype=torch.int8)
  xq = buf[offset:offset + n * d].view(n, d)
  q = torch.randint(-127, 128, (rows, d), generator=g, device="cuda", dtype=torch.int8)
  scale = torch.rand((rows,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(q, rows * d, "i8", scale, None, rows, d, 32)
  x_scale = torch.full((1,), 0.02, device="cuda")

  def forward(x=xq):
    return ops.qfc_forward(x, x_scale, ZERO_POINT, target, rows, d)

  def generic():
    with ops.qfc_staged(False):
      return forward()
  route = ops.qfc_route(xq, q, d)
  with ops.qfc_staged(False):
    assert ops.qfc_route(xq, q, d) == "generic"
  same = bool(torch.equal(forward().view(torch.int32), generic().view(torch.int32)))
  torch.cuda.synchronize()
  launches = max(1, min(64, round(args.window_ms / _window_ms(torch, generic, 1))))
  variants = {"generic_a": generic, "staged": forward, "generic_b": generic}
  aligned = None
  if offset:
    aligned = buf[16:16 + n * d].view(n, d)
    assert ops.qfc_route(aligned, q, d) == "mfma"
    variants["mfma_aligned"] = lambda: forward(aligned)
  times = {k: [] for k in variants}
  for r in range(args.warmup + args.repeats):
    for k, fn in variants.items():
      t = _window_ms(torch, fn, launches)
      if r >= args.warmup:
        times[k].append(t)
  out = {"source": source, "n": n, "rows": rows, "d": d, "xq_offset_bytes": offset, "route": route, "launches": launches,
         "same_bits_as_generic": same, "generic": _summary(times["generic_a"]), "staged": _summary(times["staged"]),
         "generic_again": _summary(times["generic_b"]), "speedup_staged_over_generic": _ratio(times["generic_a"], times["staged"]),
         "baseline_against_itself": _ratio(times["generic_a"], times["generic_b"]),
         "staged_int8_tops": 2.0 * n * rows * d / (statistics.median(times["staged"]) * 1e-3) / 1e12}
  if aligned is not None:
    out["mfma_from_an_aligned_base"] = _summary(times["mfma_aligned"])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=11)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--window-ms", type=float, default=40.0)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qfc_staged_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("qfc_staged_bench needs a GPU")
  result = {"tool": "qfc_staged_bench", "device": ops.device_info(), "repeats": args.repeats, "warmup": args.warmup,
            "window_ms": args.window_ms, "x_zero_point": ZERO_POINT,
            "rows": [bench(torch, ops, *shape, args) for shape in SHAPES]}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
