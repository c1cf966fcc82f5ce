"""DynamicHistogram without a GPU: the host state machine, merge, to_dict / from_dict, min_max_for_coverage and the error
texts against tests/golden/ref_histogram_cases.json (recorded from the reference's utils/histogram_utils.py), with the
per-element step supplied by histogram_cases.NumpyKernels through the module's seam (_BACKEND): the explicit float32
subtract / divide / floor / clip the kernels carry out, not a call into the reference. Plus the C ABI of the two entry
points and the ISA of csrc/histogram.hip."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ai-edge-quantizer_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
for p in (ROOT, PKG, os.path.dirname(os.path.abspath(__file__))):
  if p not in sys.path:
    sys.path.insert(0, p)

import histogram_cases as hc  # noqa: E402
from mi355q.utils import histogram_utils as hu  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "ref_histogram_cases.json")) as _f:
  GOLDEN = {c["name"]: c for c in json.load(_f)["cases"]}
CASES = hc.cases()


@pytest.fixture(autouse=True)
def numpy_kernels():
  saved = hu._BACKEND
  hu._BACKEND = hc.NumpyKernels()
  yield
  hu._BACKEND = saved


def test_golden_file_covers_the_case_list():
  assert [c["name"] for c in CASES] == list(GOLDEN)
  for c in CASES:
    assert {**hc.DEFAULTS, **{k: v for k, v in GOLDEN[c["name"]].items() if k in c}} == c, c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sequence_matches_reference(case):
  gold = GOLDEN[case["name"]]
  samples = hc.make(case)
  assert hc.digest(samples) == gold["input_sha256"], "input differs (random stream), not the histogram"
  snaps = {}
  hist = hc.run(case, samples, hu.DynamicHistogram, snapshot=lambda k, h: snaps.__setitem__(str(k), hc.state_digest(h)))
  hc.check(hist, gold["state"], case["name"])
  assert snaps == gold["snapshots"]
  sums = [int(h.counts.sum()) if h.initialized else 0 for h in hist._impls]
  if case["op"] != "merge":      # (merge resamples and rounds)
    hc.check_finite(sums, gold["finite"], case["name"])


@pytest.mark.parametrize("case", [c for c in CASES if c["op"] == "adds"], ids=lambda c: c["name"])
def test_add_many_is_the_sequence(case):
  gold = GOLDEN[case["name"]]
  hist = hu.DynamicHistogram(case["max_tensor_bins"], case["initial_bin_width"], case["axis"])
  hist.add_many(hc.make(case))
  hc.check(hist, gold["state"], case["name"])


def test_add_samples_takes_every_tensor_in_one_batch():
  group = [c for c in CASES if c["op"] == "adds" and c["max_tensor_bins"] == 2048 and c["initial_bin_width"] is None
           and c["dtype"] == "float32" and int(np.prod(c["shape"])) <= 1 << 17]
  assert len({str(c["axis"]) for c in group}) >= 3 and len(group) >= 10
  data = {c["name"]: hc.make(c) for c in group}
  steps = max(c["steps"] for c in group)
  samples = [{c["name"]: data[c["name"]][k] for c in group if k < c["steps"]} for k in range(steps)]
  calls = []
  backend = hu._BACKEND
  stats, bins = backend.stats, backend.bins
  backend.stats = lambda *a: calls.append("stats") or stats(*a)
  backend.bins = lambda *a: calls.append("bins") or bins(*a)
  acts = hu.ActivationHistograms(axis={c["name"]: c["axis"] for c in group})
  acts.add_samples(samples)
  assert calls == ["stats", "bins"]      # K x T float32 tensors: one launch each
  for c in group:
    hc.check(acts[c["name"]], GOLDEN[c["name"]]["state"], c["name"])
  # names= restricts; to_dict / from_dict / merge name by name
  some = hu.ActivationHistograms(axis={c["name"]: c["axis"] for c in group})
  some.add_samples(samples, names=[group[0]["name"]])
  assert list(some) == [group[0]["name"]]
  back = hu.ActivationHistograms.from_dict(acts.to_dict())
  assert sorted(back) == sorted(acts)
  for name in back:
    assert np.array_equal(back[name].global_min, acts[name].global_min)
  empty = hu.ActivationHistograms(axis={c["name"]: c["axis"] for c in group})
  empty.merge(acts)
  for c in group:
    hc.check(empty[c["name"]], GOLDEN[c["name"]]["state"], c["name"] + " (merged into empty)")


def test_state_types_follow_numpy_promotion():
  x = np.linspace(-1, 1, 101, dtype=np.float32)
  h = hu.DynamicHistogram()
  h.add(x)
  assert type(h.bin_width) is np.float32 and type(h.lower_bound) is np.float32
  g = hu.DynamicHistogram(initial_bin_width=0.01)
  g.add(x)
  g.add(x * 50)
  assert type(g.bin_width) is float and type(g.lower_bound) is np.float32
  d = hu.DynamicHistogram()
  d.add(x.astype(np.float64))
  assert type(d.bin_width) is np.float64
  # a float64 state (from_dict of float64 scalars) bins float32 data in float64
  st = h.to_dict()
  for ch in st["channels"]:
    ch["bin_width"], ch["lower_bound"] = np.float64(ch["bin_width"]), np.float64(ch["lower_bound"])
  back = hu.DynamicHistogram.from_dict(st)
  y = (x * np.float32(0.77)).astype(np.float32)
  back.add(y)
  lb, bw, n = np.float64(h.lower_bound), np.float64(h.bin_width), len(h.counts)
  want = h.counts + np.bincount(np.clip(np.floor((y - lb) / bw).astype(np.int32), 0, n - 1), minlength=n)
  assert np.array_equal(back.counts, want) and type(back.bin_width) is np.float64
  assert hu._precision(np.float32(1), np.float32(1)) == 0 and hu._precision(np.float32(1), 0.5) == 0
  assert hu._precision(np.float32(1), np.float64(1)) == 1 and hu._precision(np.float64(1), np.float64(1)) == 2


def test_properties_and_error_texts():
  h = hu.DynamicHistogram()
  assert not h.initialized and h.bin_width is None and h.lower_bound == 0.0
  assert np.array_equal(h.counts, np.zeros(1, np.int64)) and h.to_dict() == {}
  assert h.global_min[0] == np.inf and h.global_max[0] == -np.inf
  h.add(np.zeros((0,), np.float32))
  assert not h.initialized and h._impls is None
  h.add(np.full((4,), np.nan, np.float32))
  assert not h.initialized and h._impls is not None
  c = hu.DynamicHistogram(axis=0)
  assert c.global_min.size == 0
  c.add(np.arange(12, dtype=np.float32).reshape(3, 4))
  assert c.initialized and len(c._impls) == 3 and c._impls[0].max_bins == 2048 // 3
  for name in ("counts", "bin_width", "lower_bound"):
    with pytest.raises(AttributeError, match=f"{name} is not supported for per-channel histogram, use _impls\\[i\\].{name}"):
      getattr(c, name)
  with pytest.raises(ValueError, match="Cannot merge histograms with different axis: None vs 0"):
    h.merge(c)
  d = hu.DynamicHistogram(axis=0)
  d.add(np.arange(8, dtype=np.float32).reshape(2, 4))
  with pytest.raises(ValueError, match="Cannot merge: different number of channels: 3 vs 2"):
    c.merge(d)
  with pytest.raises(ValueError, match="channels"):
    c.add(np.zeros((2, 4), np.float32))
  with pytest.raises(ValueError, match="Invalid dictionary format for DynamicHistogram"):
    hu.DynamicHistogram.from_dict({"min": 0})
  assert not hu.DynamicHistogram.from_dict({}).initialized
  edges = c._impls[1].bin_edges
  assert len(edges) == len(c._impls[1].counts) + 1 and edges[0] == c._impls[1].lower_bound


def _coverage_by_definition(h, p):
  counts, edges = h.counts, h.bin_edges
  total = counts.sum()
  tail = (1 - p) / 2 * total
  low = max(j for j in range(len(counts) + 1) if counts[:j].sum() <= tail)
  high = min(j for j in range(len(counts) + 1) if counts[j:].sum() <= tail)
  clamp = lambda v: min(max(v, h.global_min), h.global_max)  # noqa: E731
  return np.float32(clamp(edges[low])), np.float32(clamp(edges[high]))


@pytest.mark.parametrize("axis,shape", [(None, (4000,)), (0, (3, 700)), (1, (50, 4, 9))])
def test_min_max_for_coverage(axis, shape):
  rng = np.random.default_rng(5)
  x = rng.standard_t(3, shape).astype(np.float32)
  h = hu.DynamicHistogram(max_tensor_bins=400, axis=axis)
  h.add(x)
  h.add(x * np.float32(3))
  want_shape = tuple(1 for _ in shape) if axis is None else tuple(d if k == axis else 1 for k, d in enumerate(shape))
  for p in (1.0, 0.999, 0.99, 0.9, 0.5, 1e-6):
    got = h.min_max_for_coverage(p)
    assert got["min"].dtype == np.float32 and got["max"].dtype == np.float32
    assert got["min"].shape == want_shape and got["max"].shape == want_shape
    for i, impl in enumerate(h._impls):
      lo, hi = _coverage_by_definition(impl, p)
      assert got["min"].ravel()[i] == lo and got["max"].ravel()[i] == hi, (p, i)
    if p < 1:
      assert np.all(got["min"] >= h.min_max_for_coverage(1.0)["min"]) and np.all(got["min"] <= got["max"])
  full = h.min_max_for_coverage(1.0)
  assert np.array_equal(full["min"].ravel(), h.global_min.astype(np.float32))
  assert np.array_equal(full["max"].ravel(), h.global_max.astype(np.float32))
  for bad in (0, -0.1, 1.5):
    with pytest.raises(ValueError, match="coverage"):
      h.min_max_for_coverage(bad)


def test_add_needs_a_gpu_without_the_stand_in():
  import torch
  if torch.cuda.is_available():
    pytest.skip("GPU present")
  hu._BACKEND = hu._GpuBackend()
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    hu.DynamicHistogram().add(np.ones(4, np.float32))
  # data that is not float32 takes the host route and needs none
  h = hu.DynamicHistogram()
  h.add(np.arange(10, dtype=np.float64))
  assert int(h.counts.sum()) == 10


# ---- C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def test_histogram_symbols_and_argument_checks(lib):
  for s in ("mi355q_hist_stats_workspace_bytes", "mi355q_hist_stats_f32", "mi355q_hist_bins_workspace_bytes",
            "mi355q_hist_bins_f32"):
    assert hasattr(lib, s), s
  assert lib.mi355q_hist_stats_workspace_bytes(3) == 3 * 16 and lib.mi355q_hist_stats_workspace_bytes(-1) == 0
  assert lib.mi355q_hist_bins_workspace_bytes(3) == 3 * 32 and lib.mi355q_hist_bins_workspace_bytes(0) == 0
  buf = ctypes.create_string_buffer(256)
  p = ctypes.c_void_p(ctypes.addressof(buf))
  err = lib.mi355q_last_error
  # host buffers stand in for device pointers: every one of these calls returns before it launches
  stats = lambda count=1, slots=1, numel=4, x=p, out=p, ws=p, nbytes=16: lib.mi355q_hist_stats_f32(  # noqa: E731
      x, p, p, p, p, count, slots, numel, out, p, p, ws, nbytes, None)
  assert stats(x=None) == -1 and b"null pointer" in err()
  assert stats(out=None) == -1 and b"null pointer" in err()
  assert stats(count=-1) == -1 and b"count" in err()
  assert stats(count=65536) == -1 and b"count must be in [0, 65535]" in err()
  assert stats(slots=-1) == -1 and b"negative size" in err()
  assert stats(numel=-1) == -1 and b"negative size" in err()
  assert stats(ws=None) == -1 and b"workspace too small" in err()
  assert stats(nbytes=8) == -1 and b"workspace too small: need 16 bytes" in err()
  assert stats(count=0, x=None, out=None, ws=None) == 0 and err() == b""
  bins = lambda count=1, slots=1, numel=4, x=p, lb=p, n_max=8, prec=0, out=p, out_len=8, ws=p, nbytes=32: (  # noqa: E731
      lib.mi355q_hist_bins_f32(x, p, p, p, p, count, slots, numel, lb, p, p, p, n_max, prec, out, out_len, ws, nbytes, None))
  assert bins(x=None) == -1 and b"null pointer" in err()
  assert bins(lb=None) == -1 and b"null pointer" in err()
  assert bins(out=None) == -1 and b"null pointer" in err()
  assert bins(count=-1) == -1 and b"count" in err()
  assert bins(slots=-1) == -1 and b"negative size" in err()
  assert bins(out_len=-1) == -1 and b"negative size" in err()
  assert bins(n_max=-1) == -1 and b"n_max" in err()
  assert bins(prec=3) == -1 and b"precision must be 0, 1 or 2" in err()
  assert bins(prec=-1) == -1 and b"precision" in err()
  assert bins(nbytes=16) == -1 and b"workspace too small: need 32 bytes" in err()
  assert bins(count=0, x=None, out=None, ws=None) == 0 and err() == b""
  assert bins(n_max=0, x=None, out=None, ws=None) == 0 and err() == b""


# ---- ISA -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
  if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
    pytest.skip("no hipcc")
  import __graft_entry__ as g
  out = str(tmp_path_factory.mktemp("isa") / "histogram.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "histogram.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    return f.read()


def test_histogram_is_built():
  import __graft_entry__ as g
  assert "histogram.hip" in g.SOURCES


def _kernel_bodies(asm):
  """kernel name -> its instructions (from its label to its s_endpgm section end)."""
  names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  bodies = {}
  for n in names:
    start = asm.index("\n" + n + ":")
    end = asm.index(".amdhsa_kernel " + n)
    bodies[n] = asm[start:end]
  return bodies


def test_histogram_kernels_isa(asm):
  bodies = _kernel_bodies(asm)
  stats = [n for n in bodies if "hist_stats_kernel" in n]
  bins = [n for n in bodies if "hist_bins_kernel" in n]
  assert len(stats) == 1 and len(bins) == 9, sorted(bodies)      # three arithmetics x three counting routes
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(bodies) and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
  assert "scratch_" not in asm
  lds_routes = [n for n in bins if "ds_add_u32" in bodies[n]]
  assert len(lds_routes) == 3, lds_routes                        # the LDS route of each arithmetic, and only it
  for n in bins:
    assert "ds_add_rtn" not in bodies[n], n
    assert "global_atomic_add_x2" in bodies[n], n
  # atomics: vector global ones without a return value, no compare-and-swap loop, nothing through the flat path
  assert "cmpswap" not in asm and "flat_atomic" not in asm
  atomics = set(re.findall(r"\b((?:global|flat|buffer|s|ds)_atomic_\w+|ds_add_\w+)", asm))
  assert atomics <= {"global_atomic_add_x2", "global_atomic_umax", "ds_add_u32"}, atomics
  # the quotient is the IEEE division sequence (v_div_scale .. v_div_fixup), not a bare reciprocal multiply; the one-bin
  # route needs no quotient at all
  for n in bins:
    if re.search(r"hist_bins_kernelILi\dELi(\d)E", n).group(1) != "0":
      assert re.search(r"v_div_fixup_f(32|64)", bodies[n]), n
