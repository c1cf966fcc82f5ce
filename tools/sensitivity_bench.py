#!/usr/bin/env python3
"""Times the sensitivity sweep against what it replaces.

  python tools/sensitivity_bench.py [--part kernel|model|all] [--repeats 20] [--warmup 3] [--model-layers 2]
                                    [--out profiles/sensitivity_bench.json]

kernel  ops.requant_delta_sweep (csrc/sensitivity.hip) with the six candidates int8 / int4 / int2 per channel and
        int4 in blocks of 32 / 128 / 256, against the composition: six times ops.requant_sym(want_q=True) then
        ops.weight_delta (int8 target, diff_bits 8), at [16384, 2048] and [2048, 16384]. The two alternate in one
        process; medians of --repeats device-event times after --warmup. Each route is reported in TB/s of the bytes IT
        moves: 4 + 4 * 6 = 28 per element for the sweep, 14 * 6 = 84 for the composition (requant reads 4 and writes 1,
        the delta reads 4 + 1 and writes 4), so the byte counts predict 3.0 x. The stacked quadratic form
        [6 * rows, d] is timed against six launches of [rows, d] in the same way.
model   one Quantizer.sweep_layer_sensitivity call with those six candidates on the N-layer full-shape model of
        tests/test_gpu_c5_model.py, against six times Quantizer(model, recipe).quantize() +
        validate_layer_outputs(calibration_result=...) on the same model and the same Hessians (host seconds, device
        drained). Nothing is derived for this ratio.

One JSON line; --out is read first when it exists, so the parts may run as separate processes (each under its own time
limit) and end up in one file.
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
CANDIDATES = (("w8", 8, 0), ("w4", 4, 0), ("w2", 2, 0), ("w4b32", 4, 32), ("w4b128", 4, 128), ("w4b256", 4, 256))
MIN_MAX = "min_max_uniform_quantize"


def _alternate_ms(torch, fns, warmup, repeats):
  """{name: (median, min, max) ms} of the callables, alternating so that all see the same clocks."""
  for _ in range(warmup):
    for fn in fns.values():
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in fns}
  for _ in range(repeats):
    for key, fn in fns.items():
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      fn()
      stop.record()
      stop.synchronize()
      times[key].append(start.elapsed_time(stop))
  return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def bench_kernel(torch, ops, rows, d, warmup, repeats):
  g = torch.Generator(device="cuda").manual_seed(rows + d)
  x = torch.randn((rows, d), generator=g, device="cuda") * 0.02
  pairs = [(bits, block) for _, bits, block in CANDIDATES]
  n = rows * d

  def sweep():
    return ops.requant_delta_sweep(x, pairs, want_sq=True)

  def composition():
    out = []
    for bits, block in pairs:
      r = ops.requant_sym(x, block, bits, want_q=True)
      target = ops.CompareTarget(r["q"], n, "i8", r["scale"].reshape(-1), None, r["scale"].numel(), block or d, 8)
      out.append(ops.weight_delta(x, target))
    return out
  got, want = sweep()[0], composition()
  same = all(bool(torch.equal(got[k].reshape(-1).view(torch.int32), want[k].view(torch.int32))) for k in range(len(pairs)))
  del got, want
  t = _alternate_ms(torch, {"sweep": sweep, "composition": composition}, warmup, repeats)
  count = len(pairs)
  bytes_sweep, bytes_comp = n * (4 + 4 * count), n * 14 * count
  out = {"rows": rows, "cols": d, "candidates": [c[0] for c in CANDIDATES], "same_bits": same,
         "sweep_ms": t["sweep"][0], "sweep_ms_min_max": list(t["sweep"][1:]),
         "composition_ms": t["composition"][0], "composition_ms_min_max": list(t["composition"][1:]),
         "sweep_TBps": bytes_sweep / (t["sweep"][0] * 1e-3) / 1e12,
         "composition_TBps": bytes_comp / (t["composition"][0] * 1e-3) / 1e12,
         "bytes_per_element": [4 + 4 * count, 14 * count], "speedup_predicted_by_bytes": bytes_comp / bytes_sweep,
         "speedup": t["composition"][0] / t["sweep"][0], "sweep_is_faster": t["sweep"][0] < t["composition"][0]}
  # the stacked quadratic form against one launch per candidate
  xs = torch.randn((2048, d), generator=g, device="cuda")
  product = torch.tril(ops.gemm(xs, xs, trans_a=True))
  del xs
  stack = sweep()[0]

  def stacked():
    return ops.quadform_rows(stack.view(count * rows, d), product, 0.25)

  def separate():
    return [ops.quadform_rows(stack[k], product, 0.25) for k in range(count)]
  same_rows = bool(torch.equal(stacked(), torch.cat(separate())))
  q = _alternate_ms(torch, {"stacked": stacked, "separate": separate}, warmup, repeats)
  out["quadform"] = {"stacked_ms": q["stacked"][0], "stacked_ms_min_max": list(q["stacked"][1:]),
                     "separate_ms": q["separate"][0], "separate_ms_min_max": list(q["separate"][1:]),
                     "stacked_us_per_row": q["stacked"][0] * 1e3 / (count * rows),
                     "separate_us_per_row": q["separate"][0] * 1e3 / (count * rows),
                     "stacked_is_not_slower": q["stacked"][0] <= q["separate"][0], "same_bits": same_rows}
  return out


def bench_model(torch, layers, sequences, tokens):
  import c5_model as C
  from mi355q import model_validator as mv, quantizer
  model = C.build_model(layers)
  samples = C.calibration_set(torch, layers, sequences, tokens)
  qsvs = quantizer.Quantizer(model, C.recipe("gptq")).calibrate({"serving_default": samples})
  del samples
  grans = {0: "CHANNELWISE", 32: "BLOCKWISE_32", 128: "BLOCKWISE_128", 256: "BLOCKWISE_256"}
  cands = [mv.SweepCandidate(name, bits, grans[block]) for name, bits, block in CANDIDATES]

  def recipe(bits, block):
    entry = C._fc(MIN_MAX, bits=bits)      # pylint: disable=protected-access
    entry["op_config"]["weight_tensor_config"]["granularity"] = grans[block]
    return [entry]
  torch.cuda.synchronize()
  sweep_s, loop_s = [], []
  table = results = None
  for _ in range(2):                 # the second round has warm allocations
    t0 = time.perf_counter()
    table = quantizer.Quantizer(model).sweep_layer_sensitivity(cands, calibration_result=qsvs)
    torch.cuda.synchronize()
    sweep_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    results = {}
    for name, bits, block in CANDIDATES:
      qz = quantizer.Quantizer(model, recipe(bits, block))
      qz.quantize()
      results[name] = qz.validate_layer_outputs(calibration_result=qsvs)
    torch.cuda.synchronize()
    loop_s.append(time.perf_counter() - t0)
  same = all(table[y][name]["error"] == results[name][y]["error"] for name in results for y in table)
  worst = {name: min(table[y][name]["output_snr"] for y in table) for name in results}
  return {"layers": layers, "sequences": sequences, "tokens": tokens, "ops": len(table), "candidates": list(results),
          "pairs_skipped": len(table.skipped), "sweep_layer_sensitivity_s": sweep_s,
          "six_quantize_plus_validate_s": loop_s, "speedup": loop_s[-1] / sweep_s[-1],
          "same_errors_as_validate_layer_outputs": same, "lowest_output_snr_by_candidate": worst}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--part", default="all", choices=("kernel", "model", "all"))
  ap.add_argument("--repeats", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--model-layers", type=int, default=2)
  ap.add_argument("--sequences", type=int, default=64)
  ap.add_argument("--tokens", type=int, default=512)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_bench.json"))
  args = ap.parse_args()
  import __graft_entry__ as g
  g.build()
  import torch
  from mi355q import ops
  if not torch.cuda.is_available():
    raise SystemExit("sensitivity_bench needs a GPU")
  result = {}
  if args.out and os.path.exists(args.out):
    with open(args.out) as fh:
      result = json.loads(fh.read() or "{}")
  result.update({"tool": "sensitivity_bench", "device": ops.device_info(), "repeats": args.repeats, "warmup": args.warmup})
  if args.part in ("kernel", "all"):
    result["shapes"] = [bench_kernel(torch, ops, rows, d, args.warmup, args.repeats) for rows, d in SHAPES]
    result["sweep_is_faster"] = all(s["sweep_is_faster"] for s in result["shapes"])
  if args.part in ("model", "all") and args.model_layers > 0:
    result["model"] = bench_model(torch, args.model_layers, args.sequences, args.tokens)
  line = json.dumps(result)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      fh.write(line + "\n")
  print(line)


if __name__ == "__main__":
  main()
