"""What model_validator.compare_layer_execution DECIDES, against a record made before its loops were merged
(tests/golden/layer_execution_structure.json, written by tools/record_layer_execution_structure.py): which skip reason
wins when two apply, every entry's key set and non-float values, and the ordered list of LayerExecutionKernels methods
each run calls, for every mode of every op kind and for models with two defects at once. The float figures are pinned
by the other host tests; none is in the record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_run_length_encoding_tells_call_lists_apart():
  import record_layer_execution_structure as R
  calls = ["weight", "target"] + ["sample", "gemm", "sqdiff"] * 3 + ["host", "host", "weight"]
  assert R.run_length(calls) == [["weight target", 1], ["sample gemm sqdiff", 3], ["host", 2], ["weight", 1]]
  assert R.run_length(calls) != R.run_length(calls[:-1]) and R.run_length([]) == []
  assert R.run_length(["a", "b", "a", "b", "a"]) == [["a b", 2], ["a", 1]]


def test_structure_is_what_was_recorded_before_the_loops_were_merged():
  import record_layer_execution_structure as R
  with open(R.GOLDEN) as fh:
    stored = json.load(fh)
  want, got = R.expand(stored), R.record()
  assert json.loads(R.dumps(R.compact(want))) == stored      # (the file is in the form the script writes)
  assert sorted(got) == sorted(want)
  # at least three two-defect models per op kind
  for kind in ("fc", "conv", "dwconv", "bmm"):
    assert sum(label.startswith(kind + "/") and "+" in label for label in want) >= 3, kind
  for label, runs in want.items():
    assert sorted(got[label]) == sorted(runs), label
    for keywords, run in runs.items():
      for part in ("skipped", "entries", "calls"):
        assert got[label][keywords][part] == run[part], (label, keywords, part)
      assert list(got[label][keywords]["entries"]) == list(run["entries"]), (label, keywords)      # (the order too)
