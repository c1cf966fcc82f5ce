#!/usr/bin/env python3
"""Times the CONV_2D patch gather of csrc/conv_patches.hip beside the integer product it feeds, on N = 8 images of
four 3x3 SAME layers (56x56x64 -> 64, 28x28x128 -> 128, 14x14x256 -> 256 at stride 1: the vector route; 112x112x3 -> 32
at stride 2: the generic route), int8 activations, int8 per-channel filters:

  python tools/qconv_bench.py [--repeats 15] [--launches 8] [--warmup 3] [--out profiles/qconv_bench.json]

  gather    ops.conv_patches of the int8 tensor, pad element = the zero point;
  forward   ops.qfc_forward on the rows the gather wrote;
  copy      a plain device copy (Tensor.copy_) of as many bytes as the gather writes.

Each is timed at two sizes: one chunk of model_validator.EXECUTION_CHUNK_ROWS patch rows (what
compare_layer_execution launches; a window from the middle of the sample) and all N OH OW rows of the sample in one
call. The three alternate within every repeat, in one process: a repeat times --launches back-to-back launches of
each with device events, and every figure is the median over --repeats of that time divided by the launches, after
--warmup untimed rounds (tools/qfc16_bench.py's method). Rates are the bytes the gather WRITES (rows x K) over its
time. There is no gate: the figures are recorded. One JSON line, also written to --out. At these sizes (0.1 - 14 MB
per launch) a call's kernel is shorter than its enqueue, so the event-timed figures are the host's time per call; the
kernels' own times come from a kernel trace of this tool in a run of its own (profiles/qconv_kernel_times.txt).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "ai-edge-quantizer_amd"), ROOT, os.path.join(ROOT, "tools")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

BATCH = 8
LAYERS = ((56, 56, 64, 64, 1), (28, 28, 128, 128, 1), (14, 14, 256, 256, 1), (112, 112, 3, 32, 2))      # (H, W, C, O, stride)
ZERO_POINT = -3


def bench_layer(torch, ops, chunk_rows, h, w, c, o, stride, args):
  from qfc16_bench import _alternating_ms
  g = torch.Generator(device="cuda").manual_seed(h * c + o)
  x = torch.randint(-128, 128, (BATCH, h, w, c), generator=g, device="cuda", dtype=torch.int8)
  oh, ow, _, _ = ops.conv_geometry(h, w, 3, 3, stride, 1, "SAME")
  rows_all, k = BATCH * oh * ow, 9 * c
  q = torch.randint(-127, 128, (o, k), generator=g, device="cuda", dtype=torch.int8)
  scale = torch.rand((o,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(q, o * k, "i8", scale, None, o, k, 32)
  x_scale = torch.full((1,), 0.02, device="cuda")
  out = {"input": [BATCH, h, w, c], "filter": [o, 3, 3, c], "stride": stride, "output_hw": [oh, ow], "rows": rows_all, "K": k,
         "route": "vector" if c % 16 == 0 else "generic"}
  for label, count in (("chunk", min(chunk_rows, rows_all)), ("sample", rows_all)):
    first = (rows_all - count) // 2
    rows = ops.conv_patches(x, 3, 3, stride, 1, "SAME", ZERO_POINT, first, count)
    src, dst = torch.randint(-128, 128, (count * k,), generator=g, device="cuda", dtype=torch.int8), torch.empty_like(rows).view(-1)

    def gather():
      return ops.conv_patches(x, 3, 3, stride, 1, "SAME", ZERO_POINT, first, count)

    def forward():
      return ops.qfc_forward(rows, x_scale, ZERO_POINT, target, o, k)

    def copy():
      return dst.copy_(src)
    t = _alternating_ms(torch, {"gather": gather, "forward": forward, "copy": copy}, args.warmup, args.repeats, args.launches)
    nbytes = count * k
    out[label] = {"rows": count, "bytes_written": nbytes,
                  "gather_ms": t["gather"]["ms"], "gather_ms_min_max": t["gather"]["ms_min_max"],
                  "forward_ms": t["forward"]["ms"], "forward_ms_min_max": t["forward"]["ms_min_max"],
                  "copy_ms": t["copy"]["ms"], "copy_ms_min_max": t["copy"]["ms_min_max"],
                  "gather_gb_per_s_written": nbytes / (t["gather"]["ms"] * 1e-3) / 1e9,
                  "copy_gb_per_s_written": nbytes / (t["copy"]["ms"] * 1e-3) / 1e9,
                  "gather_over_copy": t["gather"]["ms"] / t["copy"]["ms"],
                  "gather_over_forward": t["gather"]["ms"] / t["forward"]["ms"]}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=8)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qconv_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import model_validator, ops
  if not torch.cuda.is_available():
    raise SystemExit("qconv_bench needs a GPU")
  chunk_rows = model_validator.EXECUTION_CHUNK_ROWS
  layers = [bench_layer(torch, ops, chunk_rows, *layer, args) for layer in LAYERS]
  result = {"tool": "qconv_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "batch": BATCH, "chunk_rows": chunk_rows, "layers": layers,
            "largest_chunk_gather_over_forward_on_the_vector_route":
                max(r["chunk"]["gather_over_forward"] for r in layers if r["route"] == "vector")}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
