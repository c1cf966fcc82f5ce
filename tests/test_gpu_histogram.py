"""DynamicHistogram on the GPU against the reference's recorded end states (tests/golden/ref_histogram_cases.json, made by
tests/golden/gen/make_histogram_golden.py; the samples are regenerated from the seeds by tests/histogram_cases.py).

Every case runs through DynamicHistogram.add on device tensors; the plain sequences also through add_many and through
ActivationHistograms.add_samples with tensors of different shapes and axes in one call. Everything is exact: counts
array_equal as int64, bin_width and lower_bound equal as values and of the recorded type, global_min / global_max equal
by == (the sign of a zero minimum is not defined by np.min), counts.sum() equal to the number of finite elements. No
tolerance anywhere, no case left out."""
import json
import os

import numpy as np
import pytest

import histogram_cases as hc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_histogram_cases.json")) as _f:
  GOLDEN = {c["name"]: c for c in json.load(_f)["cases"]}
CASES = hc.cases()
SEQUENCES = [c for c in CASES if c["op"] == "adds"]


@pytest.fixture(scope="module")
def g():
  import torch
  assert torch.cuda.is_available()
  import __graft_entry__ as entry
  entry.build()
  import types
  from mi355q import ops, runtime
  from mi355q.utils import histogram_utils
  assert isinstance(histogram_utils._BACKEND, histogram_utils._GpuBackend)
  return types.SimpleNamespace(hu=histogram_utils, ops=ops, rt=runtime, torch=torch)


def _device(g, case, x):
  """The sample in HBM; with case['offset'] its first element sits one float behind a 16-byte boundary. float64 samples
  stay on the host (the module's NumPy route)."""
  if x.dtype != np.float32:
    return x
  if not case["offset"]:
    return g.torch.from_numpy(x).cuda()
  buf = g.torch.empty(x.size + case["offset"], dtype=g.torch.float32, device="cuda")
  view = buf[case["offset"]:]
  view.copy_(g.torch.from_numpy(x.reshape(-1)))
  assert view.data_ptr() % 16 == 4 * case["offset"]
  return view.view(x.shape)


def _samples(case):
  gold = GOLDEN[case["name"]]
  samples = hc.make(case)
  assert hc.digest(samples) == gold["input_sha256"], "input differs (random stream), not the kernels"
  return gold, samples


def _sums(hist):
  return [int(h.counts.sum()) if h.initialized else 0 for h in hist._impls]


def test_golden_file_covers_the_case_list():
  assert [c["name"] for c in CASES] == list(GOLDEN)
  assert {c["max_tensor_bins"] for c in CASES} >= {1, 37, 2048, 65536}
  assert max(int(np.prod(c["shape"])) for c in CASES) >= 1 << 20


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_add_on_device_tensors_matches_reference(g, case):
  gold, samples = _samples(case)
  snaps = {}
  kept = []

  def add(h, x):
    d = _device(g, case, x)
    before = d.clone() if isinstance(d, g.torch.Tensor) else None
    h.add(d)
    if before is not None:      # the device buffer is only read (bitwise: NaN payloads too)
      assert g.torch.equal(d.view(g.torch.int32), before.view(g.torch.int32))
    kept.append(d)

  hist = hc.run(case, samples, g.hu.DynamicHistogram, add=add,
                snapshot=lambda k, h: snaps.__setitem__(str(k), hc.state_digest(h)))
  hc.check(hist, gold["state"], case["name"])
  assert snaps == gold["snapshots"]
  if case["op"] != "merge":      # (merge resamples and rounds)
    hc.check_finite(_sums(hist), gold["finite"], case["name"])


@pytest.mark.parametrize("case", SEQUENCES, ids=[c["name"] for c in SEQUENCES])
def test_add_many_matches_reference(g, case):
  gold, samples = _samples(case)
  hist = g.hu.DynamicHistogram(case["max_tensor_bins"], case["initial_bin_width"], case["axis"])
  hist.add_many([_device(g, case, x) for x in samples])
  hc.check(hist, gold["state"], case["name"])
  hc.check_finite(_sums(hist), gold["finite"], case["name"])


@pytest.mark.parametrize("bins,width", sorted({(c["max_tensor_bins"], c["initial_bin_width"]) for c in SEQUENCES},
                                               key=str))
def test_add_samples_matches_reference(g, bins, width):
  """All plain sequences of one (max_tensor_bins, initial_bin_width) as the tensors of one calibration dataset: different
  shapes, axes, pointer offsets and numbers of samples in one add_samples call; device tensors and HbmArrays mixed."""
  group = [c for c in SEQUENCES if (c["max_tensor_bins"], c["initial_bin_width"]) == (bins, width)]
  data = {}
  for c in group:
    gold, samples = _samples(c)
    data[c["name"]] = [_device(g, c, x) for x in samples]
  steps = max(c["steps"] for c in group)
  samples = []
  for k in range(steps):
    sample = {}
    for i, c in enumerate(group):
      if k < c["steps"]:
        d = data[c["name"]][k]
        sample[c["name"]] = g.rt.HbmArray(d) if (i + k) % 2 and isinstance(d, g.torch.Tensor) else d
    samples.append(sample)
  acts = g.hu.ActivationHistograms(max_tensor_bins=bins, initial_bin_width=width, axis={c["name"]: c["axis"] for c in group})
  acts.add_samples(samples)
  assert sorted(acts) == sorted(c["name"] for c in group)
  for c in group:
    hc.check(acts[c["name"]], GOLDEN[c["name"]]["state"], c["name"])
    hc.check_finite(_sums(acts[c["name"]]), GOLDEN[c["name"]]["finite"], c["name"])


def test_host_float32_arrays_are_uploaded(g):
  case = next(c for c in CASES if c["name"] == "student_grow")
  gold, samples = _samples(case)
  hist = g.hu.DynamicHistogram(case["max_tensor_bins"], case["initial_bin_width"], case["axis"])
  for x in samples:
    hist.add(x)
  hc.check(hist, gold["state"], case["name"])


def test_float64_state_bins_float32_data_in_float64(g):
  """from_dict of float64 scalars: NumPy then subtracts and divides in float64 (precision 2), or divides in float64 only
  when just the width is float64 (precision 1)."""
  rng = np.random.default_rng(77)
  x = rng.standard_normal(50000).astype(np.float32)
  y = (rng.standard_normal(70001) * 0.9).astype(np.float32)
  base = g.hu.DynamicHistogram(max_tensor_bins=1000)
  base.add(g.torch.from_numpy(x).cuda())
  for widen in (("bin_width",), ("bin_width", "lower_bound")):
    st = base.to_dict()
    for ch in st["channels"]:
      for key in widen:
        ch[key] = np.float64(ch[key]) * (1 + 2.0 ** -40)      # not a float32 value any more
    hist = g.hu.DynamicHistogram.from_dict(st, max_tensor_bins=1000)
    lb, bw, n = hist.lower_bound, hist.bin_width, len(hist.counts)
    assert g.hu._precision(lb, bw) == len(widen)
    before = hist.counts.copy()
    hist.add(g.torch.from_numpy(y).cuda())
    assert (hist.lower_bound, hist.bin_width, len(hist.counts)) == (lb, bw, n)    # y lies inside x's padded range
    want = before + np.bincount(np.clip(np.floor((y - lb) / bw).astype(np.int32), 0, n - 1), minlength=n)
    assert np.array_equal(hist.counts, want)


def test_non_contiguous_and_non_float32_device_tensors(g):
  rng = np.random.default_rng(3)
  x = rng.standard_normal((300, 64)).astype(np.float32)
  t = g.torch.from_numpy(x).cuda().t()          # [64, 300], strides (1, 64)
  assert not t.is_contiguous()
  want = g.hu.DynamicHistogram(axis=0)
  want.add(g.torch.from_numpy(np.ascontiguousarray(x.T)).cuda())
  got = g.hu.DynamicHistogram(axis=0)
  got.add(t)
  for a, b in zip(got._impls, want._impls):
    assert np.array_equal(a.counts, b.counts) and a.bin_width == b.bin_width and a.lower_bound == b.lower_bound
  assert sum(_sums(got)) == x.size
  with pytest.raises(TypeError, match="float32 device tensors"):
    g.hu.DynamicHistogram().add(g.torch.from_numpy(x).cuda().half())
  with pytest.raises(ValueError, match="channels"):
    got.add(g.torch.zeros((63, 300), device="cuda"))


def test_ops_entries_against_numpy(g):
  """The two launches on a mixed table, against the NumPy stand-in of the host suite."""
  rng = np.random.default_rng(11)
  shapes = [((5000,), None), ((64, 300), 1), ((300, 100), 0), ((6, 3, 50), 1), ((2, 64, 128), 1), ((1,), None)]
  host, views = [], []
  for shape, axis in shapes:
    x = (rng.standard_t(3, shape) * 2).astype(np.float32)
    if x.size > 8:
      x.reshape(-1)[rng.choice(x.size, 4, replace=False)] = [np.nan, np.inf, -np.inf, -0.0]
    host.append(x)
    views.append(g.hu._view(shape, axis))
  dev = [g.torch.from_numpy(x).cuda() for x in host]
  ref = hc.NumpyKernels()
  mn, mx, cnt = g.hu._BACKEND.stats(dev, views)
  rmn, rmx, rcnt = ref.stats(host, views)
  assert np.array_equal(mn, rmn) and np.array_equal(mx, rmx) and np.array_equal(cnt, rcnt)
  assert cnt.dtype == np.int64 and mn.dtype == np.float32
  for nb in (1, 5, 8, 9, 300, 3000, 20000):
    lower = [float(v) - 0.25 for v in rmn]
    width = [float(np.float32((float(b) - float(a) + 0.5) / nb)) for a, b in zip(rmn, rmx)]
    n_bins = [nb if i % 7 else 0 for i in range(len(lower))]
    for precision in (0, 1, 2):
      got, off = g.hu._BACKEND.bins(dev, views, lower, width, n_bins, precision)
      want, woff = ref.bins(host, views, lower, width, n_bins, precision)
      assert np.array_equal(off, woff) and got.dtype == np.int64
      assert np.array_equal(got, want), (nb, precision)
