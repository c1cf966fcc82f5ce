#!/usr/bin/env python3
"""Record the reference's DynamicHistogram end states on seeded cases.

Usage (build container only; /root/reference does not exist on the GPU box):
    python tests/golden/gen/make_histogram_golden.py [--time]

Imports the reference's utils/histogram_utils.py (NumPy and absl.logging only; the shim beside this file stands in for
absl) as a bare package module, the way make_validation_golden.py does, regenerates every case of
tests/histogram_cases.py from its seed and records, per case, the seed and parameters, a SHA-256 of the regenerated
samples and the reference's end state per channel (counts, bin_width, lower_bound, global_min, global_max, the type name
of every scalar), plus a digest of the state after every k-th add of the plain sequences -- no sample arrays -- into
tests/golden/ref_histogram_cases.json. To keep that file small, counts of more than a few bins are kept as the SHA-256
of their int64 bytes and states of several channels as the SHA-256 of the whole state (equality of either is exact).

--time: the reference's `add` of one 4 MiB float32 tensor on this CPU, per tensor with 2048 bins and per channel
(128 and 4096 channels), printed for scale only.
"""
import json
import os
import sys
sys.dont_write_bytecode = True  # never leave .pyc files in the read-only reference tree
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
TESTS = os.path.dirname(GOLDEN)
ROOT = os.path.dirname(TESTS)
REF = "/root/reference/ai_edge_quantizer"

pkg = types.ModuleType("ai_edge_quantizer")
pkg.__path__ = [REF]
sys.modules["ai_edge_quantizer"] = pkg
sys.path[:0] = [os.path.join(HERE, "shim"), TESTS, ROOT]
from ai_edge_quantizer.utils import histogram_utils as hu  # noqa: E402
import histogram_cases  # noqa: E402


def doublings(case, hist) -> int:
  """How often the first channel's width was doubled: log2 of final / initial width."""
  first = hu.DynamicHistogram(case["max_tensor_bins"], case["initial_bin_width"], case["axis"])
  first.add(histogram_cases.make(case)[0])
  a, b = first._impls[0].bin_width, hist._impls[0].bin_width   # pylint: disable=protected-access
  return int(round(np.log2(float(b) / float(a)))) if a and b else 0


def timing():
  rng = np.random.default_rng(0)
  x = rng.standard_normal((256, 4096)).astype(np.float32)
  for label, kw in (("per tensor, 2048 bins", {}), ("128 channels, 16 bins", {"axis": 0}), ("4096 channels, 1 bin", {"axis": 1})):
    data = x.reshape(128, 8192) if label.startswith("128") else x
    best = None
    for _ in range(3):
      h = hu.DynamicHistogram(**kw)
      t0 = time.perf_counter()
      h.add(data)
      dt = time.perf_counter() - t0
      best = dt if best is None else min(best, dt)
    print(f"reference add, one 4 MiB float32 tensor, {label}: {best * 1e3:.1f} ms")


def main():
  if "--time" in sys.argv:
    timing()
    return
  out = []
  for case in histogram_cases.cases():
    samples = histogram_cases.make(case)
    snaps = {}
    hist = histogram_cases.run(case, samples, hu.DynamicHistogram,
                               snapshot=lambda k, h: snaps.__setitem__(str(k), histogram_cases.state_digest(h)))
    rec = histogram_cases.compact(case)
    rec["input_sha256"] = histogram_cases.digest(samples)
    rec["finite"] = histogram_cases.recorded_finite(histogram_cases.finite_counts(case, samples))
    rec["state"] = histogram_cases.recorded_state(hist)
    rec["snapshots"] = snaps
    for ch in histogram_cases.state(hist):   # a range that overflows float32 is out of scope: no case may end there
      assert not ch["initialized"] or all(np.isfinite(ch[k]) for k in ("bin_width", "lower_bound", "global_min", "global_max")), case["name"]
    if case["op"] == "adds" and hist._impls and hist._impls[0].initialized:   # pylint: disable=protected-access
      rec["doublings"] = doublings(case, hist)
      assert rec["doublings"] >= case["min_doublings"], (case["name"], rec["doublings"])
    out.append(rec)
    print(case["name"], "channels", len(hist._impls), "n", len(hist._impls[0].counts), "doublings", rec.get("doublings"))  # pylint: disable=protected-access
  with open(os.path.join(GOLDEN, "ref_histogram_cases.json"), "w") as f:
    json.dump({"source": "reference utils/histogram_utils.py, NumPy " + np.__version__, "cases": out}, f, indent=None,
              separators=(",", ":"))


if __name__ == "__main__":
  main()
