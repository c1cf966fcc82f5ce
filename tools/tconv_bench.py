#!/usr/bin/env python3
"""Times the integer execution of TRANSPOSE_CONV by sub-pixel phases (csrc/conv_patches.hip, ops.tconv_patches,
ops.tconv_forward) on N = 8 images of two upsampling layers, 28x28x128 -> 56x56x64 and 56x56x64 -> 112x112x32, each
under a 4x4 and a 3x3 filter at stride 2, SAME; static a8w8 (int8 activations with a zero point, int8 per-channel
filters):

  python tools/tconv_bench.py [--repeats 15] [--launches 4] [--warmup 3] [--out profiles/tconv_bench.json]

  (a) phase_gather     ops.tconv_patches of every phase (all its rows in one call), against
      copy             a plain device copy (Tensor.copy_) of as many bytes as those gathers write;
  (b) phase_whole      ops.tconv_forward: per phase the gather, ops.qfc_forward on its rows and the interleaving store,
      phase_product    ops.qfc_forward alone on every phase's rows (gathered beforehand), against the zero-stuffed route,
      which the library does not ship and this tool builds itself: the zero point inserted between the pixels, then
      stuffed_whole    the stuffing, ops.conv_patches at stride 1 (full KH KW C rows) and one full-K ops.qfc_forward
                       against the flipped filter,
      stuffed_gather / stuffed_product   its two kernels alone;
  (c) float_whole      ops.dequantize of the int8 activation plus ops.tconv_forward in float32 on the dequantized filter.

Before any timing the two integer routes must give the same float32 bits (the stuffed route multiplies zeros, the
accumulators are equal). All alternate within every repeat, in one process: a repeat times --launches back-to-back
calls of each with device events, and every figure is the median over --repeats of that time divided by the launches,
after --warmup untimed rounds (tools/qfc16_bench.py's method). The figures are times per call as a caller sees them,
host enqueue included; there is no gate, they are recorded. One JSON line, also written to --out.
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
LAYERS = ((28, 28, 128, 64), (56, 56, 64, 32))      # (IH, IW, C, O); the output is 2 IH x 2 IW
KERNELS = (4, 3)
STRIDE, PADDING = 2, "SAME"
ZERO_POINT = -3


def stuffed_input(torch, ops, x, k, out_hw):
  """[N, OH + K - 1, OW + K - 1, C] filled with the zero point, pixel (a, b) of x at (a s + K - 1 - pad_top,
  b s + K - 1 - pad_left): a VALID stride-1 convolution of it with the filter flipped in both axes is the op."""
  n, ih, iw, c = x.shape
  top, left = ops.tconv_geometry(ih, iw, k, k, STRIDE, PADDING, out_hw)
  out = torch.full((n, out_hw[0] + k - 1, out_hw[1] + k - 1, c), ZERO_POINT, dtype=x.dtype, device=x.device)
  out[:, k - 1 - top:k - 1 - top + (ih - 1) * STRIDE + 1:STRIDE, k - 1 - left:k - 1 - left + (iw - 1) * STRIDE + 1:STRIDE] = x
  return out


def bench_layer(torch, ops, ih, iw, c, o, k, args):
  from qfc16_bench import _alternating_ms
  g = torch.Generator(device="cuda").manual_seed(ih * c + o + k)
  out_hw = (ih * STRIDE, iw * STRIDE)
  x = torch.randint(-128, 128, (BATCH, ih, iw, c), generator=g, device="cuda", dtype=torch.int8)
  q = torch.randint(-127, 128, (o, k, k, c), generator=g, device="cuda", dtype=torch.int8)
  d = k * k * c
  scale = torch.rand((o,), generator=g, device="cuda") * 0.005 + 0.001
  target = ops.CompareTarget(q, o * d, "i8", scale, None, o, d, 32)
  flipped = ops.CompareTarget(torch.flip(q, dims=(1, 2)).contiguous(), o * d, "i8", scale, None, o, d, 32)
  x_scale = torch.full((1,), 0.02, device="cuda")
  zp_dev = torch.full((1,), ZERO_POINT, dtype=torch.int32, device="cuda")
  w_float = (q.to(torch.float32) * scale.view(o, 1, 1, 1)).contiguous()
  phases = ops.tconv_phases(ih, iw, k, k, STRIDE, PADDING, out_hw)
  slices = ops._tconv_filter_slices("tconv_bench", target, o, k, k, c, phases)      # pylint: disable=protected-access
  geometry = (k, k, STRIDE, PADDING, out_hw)

  def phase_gather():
    return [ops.tconv_patches(x, *geometry, p[:2], ZERO_POINT) for p in phases]
  rows = phase_gather()
  gathered = sum(r.numel() for r in rows)
  src, dst = torch.randint(-128, 128, (gathered,), generator=g, device="cuda", dtype=torch.int8), torch.empty(gathered, dtype=torch.int8, device="cuda")

  def copy():
    return dst.copy_(src)

  def phase_product():
    return [ops.qfc_forward(r, x_scale, ZERO_POINT, part, o, r.shape[1]) for r, part in zip(rows, slices)]

  def phase_whole():
    return ops.tconv_forward(x, target, *geometry, x_scale=x_scale, x_zero_point=ZERO_POINT)
  stuffed = stuffed_input(torch, ops, x, k, out_hw)

  def stuffed_gather():
    return ops.conv_patches(stuffed, k, k, 1, 1, "VALID", ZERO_POINT)
  stuffed_rows = stuffed_gather()

  def stuffed_product():
    return ops.qfc_forward(stuffed_rows, x_scale, ZERO_POINT, flipped, o, d)

  def stuffed_whole():
    return ops.qfc_forward(ops.conv_patches(stuffed_input(torch, ops, x, k, out_hw), k, k, 1, 1, "VALID", ZERO_POINT), x_scale,
                           ZERO_POINT, flipped, o, d)

  def float_whole():
    return ops.tconv_forward(ops.dequantize(x, 1, 1, x.numel(), x_scale, zp_dev, 16), w_float, *geometry)
  same = torch.equal(phase_whole().view(-1, o), stuffed_whole())
  if not same:
    raise SystemExit(f"the phase route and the zero-stuffed route disagree on {ih}x{iw}x{c} -> {o}, {k}x{k}")
  fns = {"phase_gather": phase_gather, "copy": copy, "phase_product": phase_product, "phase_whole": phase_whole,
         "stuffed_gather": stuffed_gather, "stuffed_product": stuffed_product, "stuffed_whole": stuffed_whole,
         "float_whole": float_whole}
  t = _alternating_ms(torch, fns, args.warmup, args.repeats, args.launches)
  out = {"input": [BATCH, ih, iw, c], "filter": [o, k, k, c], "stride": STRIDE, "padding": PADDING, "output_hw": list(out_hw),
         "phases": [{"phase": list(p[:2]), "rows": int(r.shape[0]), "K": int(r.shape[1])} for p, r in zip(phases, rows)],
         "full_K": d, "output_rows": BATCH * out_hw[0] * out_hw[1], "bytes_gathered_by_phases": gathered,
         "bytes_gathered_stuffed": int(stuffed_rows.numel()), "routes_agree_bit_for_bit": same}
  for name, v in t.items():
    out[name + "_ms"], out[name + "_ms_min_max"] = v["ms"], v["ms_min_max"]
  ms = {name: v["ms"] for name, v in t.items()}
  out.update(phase_gather_over_copy=ms["phase_gather"] / ms["copy"],
             phase_gather_gb_per_s_written=gathered / (ms["phase_gather"] * 1e-3) / 1e9,
             copy_gb_per_s_written=gathered / (ms["copy"] * 1e-3) / 1e9,
             stuffed_product_over_phase_product=ms["stuffed_product"] / ms["phase_product"],
             stuffed_gather_over_phase_gather=ms["stuffed_gather"] / ms["phase_gather"],
             stuffed_whole_over_phase_whole=ms["stuffed_whole"] / ms["phase_whole"],
             float_whole_over_phase_whole=ms["float_whole"] / ms["phase_whole"])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=15)
  ap.add_argument("--launches", type=int, default=4)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tconv_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("tconv_bench needs a GPU")
  layers = [bench_layer(torch, ops, *layer, k, args) for layer in LAYERS for k in KERNELS]
  result = {"tool": "tconv_bench", "device": ops.device_info(), "repeats": args.repeats, "launches": args.launches,
            "warmup": args.warmup, "batch": BATCH, "stride_product": STRIDE * STRIDE, "layers": layers}
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
