#!/usr/bin/env python3
"""Record the reference's five validation metrics on seeded cases.

Usage (build container only; /root/reference does not exist on the GPU box):
    python tests/golden/gen/make_validation_golden.py

Imports the reference's utils/validation_utils.py (NumPy only) as a bare package module, the way make_golden.py does,
regenerates every case of tests/validation_cases.py from its seed and records, per case, the seed, the shape, the kind
of corruption / target form and the reference's results -- no arrays -- into tests/golden/ref_validation_cases.json.
The metrics are taken as model_validator.compare_model calls them: fn(target, reference).
"""
import json
import os
import sys
sys.dont_write_bytecode = True  # never leave .pyc files in the read-only reference tree
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
sys.path[:0] = [TESTS, ROOT]
from ai_edge_quantizer.utils import validation_utils as vu  # noqa: E402
import validation_cases  # noqa: E402


def main():
  out = []
  for case in validation_cases.cases():
    t, r, _ = validation_cases.make(case)
    res = {}
    for metric in vu.ValidationErrorMetric:
      val = vu.get_validation_func(metric)(t, r)
      res[metric.value] = {"value": float(val), "type": type(val).__name__}
    rec = {k: case[k] for k in ("name", "seed", "n", "corruption", "form")}
    if "shape" in case:
      rec["shape"] = case["shape"]
    rec["results"] = res
    out.append(rec)
    print(case["name"], {k: v["value"] for k, v in res.items()})
  with open(os.path.join(GOLDEN, "ref_validation_cases.json"), "w") as f:
    json.dump({"source": "reference utils/validation_utils.py, NumPy " + np.__version__, "cases": out}, f, indent=1)


if __name__ == "__main__":
  main()
