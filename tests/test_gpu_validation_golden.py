"""The GPU's comparison metrics against the reference's own, recorded by tests/golden/gen/make_validation_golden.py
(tests/golden/ref_validation_cases.json: seed, shape, corruption / target form and the reference's five results per
case; the arrays are regenerated here from the seeds by tests/validation_cases.py). Quantized targets are handed to
the kernel in their stored form (int8 channelwise with zero points, int16, int32 bias, packed int4 blockwise-128, fp16).

MSE, SNR and the median diff ratio are bit-equal; the cosine within 4e-6 (1e-5 at 2^24 elements, where NumPy's float32
sdot drifts from the float64 sums: DESIGN.md section 4); the KL divergence within 1e-5 * sum|terms| + 1e-30.
"""
import json
import os

import numpy as np
import pytest

import validation_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_validation_cases.json")) as _f:
  CASES = {c["name"]: c for c in json.load(_f)["cases"]}


@pytest.fixture(scope="module")
def v():
  import torch
  assert torch.cuda.is_available()
  import __graft_entry__ as g
  g.build()
  import types
  from mi355q import ops
  from mi355q.utils import validation_utils
  return types.SimpleNamespace(vu=validation_utils, ops=ops, torch=torch)


def _target(v, stored, n):
  torch = v.torch
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  if stored["kind"] in ("f32", "f16"):
    return v.ops.CompareTarget(dev(stored["data"]), n, stored["kind"])
  zp = None if stored["zp"] is None else dev(stored["zp"].astype(np.int32))
  return v.ops.CompareTarget(dev(stored["data"]), n, stored["kind"], dev(stored["scale"]), zp, stored["channels"],
                             stored["inner"], 32)


def _kl_scale(t, r):
  d1 = np.nan_to_num(t, nan=1e-9, neginf=-1e9, posinf=1e9).astype(np.float64)
  d2 = np.nan_to_num(r, nan=1e-9, neginf=-1e9, posinf=1e9).astype(np.float64)
  p, q = np.maximum(0, d2), np.maximum(0, d1)
  return float(np.sum(np.abs(p * np.log((p + 1e-9) / (q + 1e-9))))) if p.size else 0.0


def test_fixture_has_the_issue_cases():
  assert len(CASES) >= 40
  sizes = {c["n"] for c in CASES.values()}
  assert {0, 1, 2, 7, 8, 127, 128, 129, 8191, 8193, (1 << 20) + 3, 1 << 24} <= sizes
  assert {c["form"] for c in CASES.values()} >= {"int8_channelwise", "int4_blockwise128", "int16", "int32_bias", "fp16"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_metrics_equal_the_references_recorded_results(v, name):
  case = CASES[name]
  t, r, stored = validation_cases.make(case)
  got = {m.value: val for m, val in v.vu.compare_all(_target(v, stored, case["n"]), r).items()}
  want = {k: rec["value"] for k, rec in case["results"].items()}
  types = {k: rec["type"] for k, rec in case["results"].items()}
  assert got["mse"] == want["mse"] and type(got["mse"]).__name__ == types["mse"]
  assert got["snr"] == want["snr"] and type(got["snr"]).__name__ == types["snr"]
  assert float(got["median_diff_ratio"]) == want["median_diff_ratio"]
  assert type(got["median_diff_ratio"]).__name__ == types["median_diff_ratio"]
  cos_tol = 1e-5 if case["n"] >= 1 << 24 else 4e-6
  assert abs(float(got["cosine_similarity"]) - want["cosine_similarity"]) <= cos_tol
  assert abs(got["kl_divergence"] - want["kl_divergence"]) <= 1e-5 * _kl_scale(t, r) + 1e-30
  # the stored form and the float form of the same target give the same numbers
  if stored["kind"] != "f32":
    flat = {m.value: val for m, val in v.vu.compare_all(t, r).items()}
    for k in ("mse", "snr", "median_diff_ratio"):
      assert float(flat[k]) == float(got[k]), k


def test_batched_equals_single_over_the_fixture(v):
  names = [n for n in sorted(CASES) if CASES[n]["n"] < 1 << 20]
  built = [validation_cases.make(CASES[n]) for n in names]
  pairs = [(_target(v, s, CASES[n]["n"]), r) for n, (_, r, s) in zip(names, built)]
  batched = v.vu.compare_all_batched(pairs)
  for (tgt, r), b in zip(pairs, batched):
    one = v.vu.compare_all(tgt, r)
    assert {k: float(x) for k, x in one.items()} == {k: float(x) for k, x in b.items()}
