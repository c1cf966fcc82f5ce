#!/usr/bin/env python3
"""Timing of the activation-histogram launches against the activation min/max kernel on the same tensors.

    python tools/histogram_bench.py [--samples 16] [--iters 20] [--warmup 3] [--out profiles/histogram_bench.json]

Workload: BASELINE config 4's shape, 32 float32 activations of 4 MiB ([256, 4096]) per sample x --samples samples, all
resident in HBM, one table over all of them. Timed with device events after warm-up, the variants and the yardstick
alternating inside one process:

  minmax                  ops.act_minmax_entries over the same tensors (K7: the yardstick, not code under test);
  stats_*                 mi355q_hist_stats_f32 with prebuilt tables (finite min / max / count per slot);
  bins_*                  mi355q_hist_bins_f32 with prebuilt tables (pack kernel + bins kernel; the counts are added to);
  add_samples_*           ActivationHistograms.add_samples end to end, host clock around a synchronise: tables, both
                          launches, the copy of the counts to the host and the host state machine (twice).

Variants: per tensor with 2048 bins; per channel on the last axis of [8192, 128] (16 bins each) and of [256, 4096]
(1 bin each); per tensor with 65536 bins (the route that does not fit LDS). Every figure is also given as `hbm_frac`:
the time of one read of the bytes at 6.3 TB/s over the measured time. Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ai-edge-quantizer_amd")]
HBM_ACHIEVABLE = 6.3e12


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--samples", type=int, default=16)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()

  import __graft_entry__ as g
  g.build()
  import numpy as np
  import torch
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  from mi355q.utils import histogram_utils as hu
  rt.require_gpu()
  L = _ffi.lib()
  gen = torch.Generator(device="cuda").manual_seed(0)
  tensors = 32
  acts = [[torch.randn((256, 4096), generator=gen, device="cuda") * (1 + (i + 3 * k) / 8) for i in range(tensors)]
          for k in range(args.samples)]
  flat = [a for sample in acts for a in sample]
  count = len(flat)
  nbytes = sum(a.numel() for a in flat) * 4
  read_ms = nbytes / HBM_ACHIEVABLE * 1e3
  pointers = [a.data_ptr() for a in flat]

  variants = {"per_tensor_2048": ((1, 1, 1 << 20), 2048), "per_channel_128x16": ((8192, 128, 1), 16),
              "per_channel_4096x1": ((256, 4096, 1), 1), "per_tensor_65536": ((1, 1, 1 << 20), 65536)}
  runs = {"minmax": lambda: ops.act_minmax_entries(pointers, [a.numel() for a in flat])}
  keep = []
  for name, (view, n) in variants.items():
    outers, channels, inners = [view[0]] * count, [view[1]] * count, [view[2]] * count
    tabs, slots, numel = ops._hist_tables(pointers, outers, channels, inners, 0, count)
    mn, mx = rt.empty((slots,), torch.float32), rt.empty((slots,), torch.float32)
    cnt = rt.empty((slots,), torch.int64)
    sbytes = L.mi355q_hist_stats_workspace_bytes(slots)
    sws = rt.empty((sbytes,), torch.uint8)
    targs = [rt.ptr(t) for t in tabs]

    def stats(targs=targs, slots=slots, numel=numel, mn=mn, mx=mx, cnt=cnt, sws=sws, sbytes=sbytes):
      _ffi.check(L.mi355q_hist_stats_f32(*targs, count, slots, numel, rt.ptr(mn), rt.ptr(mx), rt.ptr(cnt), rt.ptr(sws),
                                         sbytes, rt.stream_ptr()))
    stats()
    torch.cuda.synchronize()
    lo, hi = mn.double(), mx.double()
    lower = (lo - 0.1 * (hi - lo)).float().double().contiguous()          # the first add's padded range
    width = ((1.2 * (hi - lo)).float() / n).double().contiguous()
    n_bins = torch.full((slots,), n, dtype=torch.int64, device="cuda")
    offsets = (torch.arange(slots, dtype=torch.int64, device="cuda") * n).contiguous()
    out = torch.zeros((slots * n,), dtype=torch.int64, device="cuda")
    bbytes = L.mi355q_hist_bins_workspace_bytes(slots)
    bws = rt.empty((bbytes,), torch.uint8)

    def bins(targs=targs, slots=slots, numel=numel, lower=lower, width=width, n_bins=n_bins, offsets=offsets, out=out,
             bws=bws, bbytes=bbytes, n=n):
      _ffi.check(L.mi355q_hist_bins_f32(*targs, count, slots, numel, rt.ptr(lower), rt.ptr(width), rt.ptr(n_bins),
                                        rt.ptr(offsets), n, 0, rt.ptr(out), out.numel(), rt.ptr(bws), bbytes,
                                        rt.stream_ptr()))
    bins()
    torch.cuda.synchronize()
    per_tensor = out.view(count, -1).sum(1)
    assert bool((per_tensor == (1 << 20)).all()), name               # every element is finite and counted once
    if name != "per_tensor_65536":
      runs["stats_" + name] = stats
    runs["bins_" + name] = bins
    keep.append((tabs, mn, mx, cnt, sws, lower, width, n_bins, offsets, out, bws))

  for _ in range(args.warmup):
    for fn in runs.values():
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in runs}
  for _ in range(args.iters):                                           # alternate: drift hits every variant alike
    for k, fn in runs.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      times[k].append((a, b))
  torch.cuda.synchronize()
  med = {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in times.items()}
  result = {"tool": "histogram_bench", "device": ops.device_info(), "samples": args.samples, "tensors_per_sample": tensors,
            "bytes": nbytes, "iters": args.iters, "one_hbm_read_ms_at_6.3TBps": round(read_ms, 4), "launches": {}}
  for k, ms in med.items():
    result["launches"][k] = {"ms": round(ms, 4), "vs_minmax": round(ms / med["minmax"], 3),
                             "hbm_frac": round(read_ms / ms, 3)}

  # end to end through the public collector
  e2e = {}
  for name, axis, shape in (("per_tensor_2048", None, (256, 4096)), ("per_channel_128x16", -1, (8192, 128))):
    samples = [{f"act{i}": a.view(shape) for i, a in enumerate(sample)} for sample in acts]
    best = None
    for _ in range(3):
      coll = hu.ActivationHistograms(axis=axis)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      coll.add_samples(samples)
      torch.cuda.synchronize()
      dt = (time.perf_counter() - t0) * 1e3
      best = dt if best is None else min(best, dt)
    total = sum(int(h.counts.sum()) for name_ in coll for h in coll[name_]._impls)
    assert total == count << 20, (name, total)
    e2e[name] = {"ms": round(best, 3), "vs_minmax": round(best / med["minmax"], 2), "hbm_frac": round(read_ms / best, 4)}
  result["add_samples"] = e2e
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
