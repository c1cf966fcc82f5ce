"""Seeded DynamicHistogram cases, shared by tests/golden/gen/make_histogram_golden.py (which runs the reference's
utils/histogram_utils.py over them and records its end state) and the histogram tests (which regenerate the samples from
the seeds and compare this project's state with the recorded one, exactly).

A case is a sequence of samples of one tensor plus what is done with them:
  op "adds"       add every sample in order;
  op "merge"      A takes the first half, B (other scale, other range) the rest but the last; A.merge(B); A.add(last);
  op "roundtrip"  add the first half, to_dict -> from_dict, add the rest.
make(case) -> the list of samples. run(case, samples, cls, add) drives either implementation. state(hist) -> the
JSON-able end state; check(hist, recorded) asserts equality with a recorded one.
"""
import hashlib

import numpy as np

INLINE_COUNTS = 40       # cases with more integers than this record a SHA-256 of the int64 counts instead (as exact)
INLINE_CHANNELS = 1      # cases with more channels record a SHA-256 of the whole state and the first channels only
HEAD_CHANNELS = 1


DEFAULTS = {"dist": "normal", "scale": 1.0, "growth": 1.0, "drift": 0.0, "max_tensor_bins": 2048, "initial_bin_width": None,
            "axis": None, "dtype": "float32", "plant": False, "first": None, "offset": 0, "op": "adds", "every": 4,
            "min_doublings": 0}


def _case(name, seed, shape, steps, **kw):
  return {"name": name, "seed": seed, "shape": list(shape), "steps": steps, **DEFAULTS, **kw}


def compact(case) -> dict:
  """The case as the golden file records it: every parameter that differs from DEFAULTS."""
  return {k: v for k, v in case.items() if k not in DEFAULTS or v != DEFAULTS[k]}


def cases() -> list:
  out = [
      _case("normal_grow", 1, (4096,), 12, growth=2.0, drift=0.5, min_doublings=5),
      _case("student_grow", 2, (257, 33), 12, dist="student", growth=2.0, drift=-0.3, min_doublings=5),
      _case("student_bins37", 3, (1000,), 10, dist="student", growth=2.0, drift=0.2, max_tensor_bins=37, min_doublings=5),
      _case("zero_range_first", 4, (64,), 3, first="zero_range", growth=3.0),
      _case("width_given", 5, (3000,), 8, initial_bin_width=0.001, growth=2.0, drift=0.4, min_doublings=5),
      _case("width_given_bins37", 6, (999,), 8, initial_bin_width=0.01, growth=2.0, max_tensor_bins=37, min_doublings=5),
      _case("planted", 7, (5000,), 4, plant=True, growth=1.5),
      _case("all_nonfinite_first", 8, (777,), 3, first="all_nonfinite", growth=2.0),
      _case("all_nonfinite_first_channel", 9, (4, 600), 3, first="all_nonfinite_channel", axis=0, growth=2.0),
      _case("bins1", 10, (1000,), 4, max_tensor_bins=1, drift=3.0),
      _case("bins65536_4mib", 11, (1 << 20,), 3, max_tensor_bins=65536, growth=4.0, dist="student", plant=True),
      _case("bins65536_last_axis3", 12, (100, 3), 3, max_tensor_bins=65536, axis=1, growth=2.0),
      _case("axis0_c3", 13, (3, 5000), 5, axis=0, growth=2.0, drift=0.3, dist="student"),
      _case("axis0_c128_4mib", 14, (128, 8192), 3, axis=0, growth=3.0, plant=True),
      _case("axis0_c4096", 15, (4096, 70), 3, axis=0, drift=3.0, plant=True),
      _case("axis0_c300_bins6", 16, (300, 100), 4, axis=0, growth=2.0),
      _case("middle_c3_short_inner", 17, (6, 3, 50), 5, axis=1, growth=2.0, plant=True),
      _case("middle_c128", 18, (5, 128, 96), 4, axis=1, growth=2.0, dist="student"),
      _case("middle_c128_unaligned_rows", 19, (3, 128, 65), 4, axis=1, growth=2.0, plant=True, offset=1),
      _case("middle_c4096_inner8", 20, (2, 4096, 8), 3, axis=1, drift=3.0, plant=True),
      _case("last_c3", 21, (7001, 3), 5, axis=-1, growth=2.0, drift=0.2, plant=True),
      _case("last_c128_4mib", 22, (8192, 128), 3, axis=-1, growth=3.0, dist="student", plant=True),
      _case("last_c4096_4mib", 23, (256, 4096), 3, axis=1, drift=3.0, plant=True),
      _case("last_c300_bins6", 24, (64, 300), 4, axis=1, growth=2.0),
      _case("last_c128_offset", 25, (130, 128), 3, axis=1, growth=2.0, offset=1, plant=True),
      _case("merge_then_add", 30, (2000,), 7, op="merge", growth=1.7, drift=0.6, dist="student"),
      _case("merge_then_add_channels", 31, (3, 900), 7, op="merge", growth=1.7, drift=-0.4, axis=0),
      _case("roundtrip_then_add", 32, (2500,), 6, op="roundtrip", growth=2.0, drift=0.3),
      _case("roundtrip_width_given", 33, (2500,), 6, op="roundtrip", growth=2.0, initial_bin_width=0.002),
      _case("float64", 34, (3000,), 5, dtype="float64", growth=2.0, drift=0.3, plant=True),
  ]
  for i, n in enumerate([1, 2, 3, 5, 63, 1023, 4099, 65537, (1 << 20) + 3]):
    out.append(_case(f"size_{n}", 40 + i, (n,), 3, growth=2.0, plant=n >= 63))
    out.append(_case(f"size_{n}_offset", 60 + i, (n,), 3, growth=2.0, offset=1, dist="student"))
  return out   # (one bin cannot grow to the left -- the reference's width then overflows -- so those cases only drift upwards)


def make(case) -> list:
  rng = np.random.default_rng(case["seed"])
  shape = tuple(case["shape"])
  dt = np.dtype(case["dtype"])
  samples = []
  for k in range(case["steps"]):
    scale = case["scale"] * case["growth"] ** k
    if case["op"] == "merge" and case["steps"] // 2 <= k < case["steps"] - 1:
      scale *= 0.37          # B: another width, and a range shifted off A's
    base = rng.standard_t(3, shape) if case["dist"] == "student" else rng.standard_normal(shape)
    x = (base * scale + case["drift"] * k * scale).astype(dt)
    if case["plant"] and x.size >= 8:
      flat = x.reshape(-1)
      at = rng.choice(x.size, 8, replace=False)
      flat[at[:5]] = [np.nan, np.inf, -np.inf, 0.0, -0.0]
      flat[at[5:]] = [np.nan, np.inf, 0.0]
    if k == 0 and case["first"] == "zero_range":
      x[...] = 1.5
    if k == 0 and case["first"] == "all_nonfinite":
      x[...] = np.nan
      x.reshape(-1)[::3] = np.inf
      x.reshape(-1)[1::3] = -np.inf
    if k == 0 and case["first"] == "all_nonfinite_channel":
      np.moveaxis(x, case["axis"], 0)[1] = np.nan
    samples.append(x)
  return samples


def digest(samples) -> str:
  h = hashlib.sha256()
  for x in samples:
    h.update(np.ascontiguousarray(x).tobytes())
  return h.hexdigest()


def _kwargs(case) -> dict:
  return {"max_tensor_bins": case["max_tensor_bins"], "initial_bin_width": case["initial_bin_width"], "axis": case["axis"]}


def run(case, samples, cls, add=lambda h, x: h.add(x), snapshot=None):
  """Drives `cls` (a DynamicHistogram class) through the case. snapshot(step, hist) is called after every case['every']-th
  add of an "adds" case. -> the final histogram."""
  kw = _kwargs(case)
  if case["op"] == "adds":
    h = cls(**kw)
    for k, x in enumerate(samples):
      add(h, x)
      if snapshot is not None and (k + 1) % case["every"] == 0:
        snapshot(k + 1, h)
    return h
  half = len(samples) // 2
  if case["op"] == "merge":
    a, b = cls(**kw), cls(**kw)
    for x in samples[:half]:
      add(a, x)
    for x in samples[half:-1]:
      add(b, x)
    a.merge(b)
    add(a, samples[-1])
    return a
  if case["op"] == "roundtrip":
    h = cls(**kw)
    for x in samples[:half]:
      add(h, x)
    h = cls.from_dict(h.to_dict(), max_tensor_bins=case["max_tensor_bins"])
    for x in samples[half:]:
      add(h, x)
    return h
  raise ValueError(case["op"])


def finite_counts(case, samples) -> list:
  """Finite elements per channel over all samples."""
  total = None
  for x in samples:
    f = np.isfinite(x)
    per = np.array([f.sum()]) if case["axis"] is None else np.moveaxis(f, case["axis"], 0).reshape(x.shape[case["axis"]], -1).sum(1)
    total = per if total is None else total + per
  return [int(v) for v in total]


def recorded_finite(values):
  """The per-channel numbers of finite elements as the golden file keeps them: the list, or its total and SHA-256."""
  if len(values) <= INLINE_CHANNELS:
    return [int(v) for v in values]
  return {"channels": len(values), "total": int(sum(values)), "sha256": _counts_sha(values)}


def check_finite(sums, recorded, label="") -> None:
  assert recorded_finite(sums) == recorded, (label, sums[:8], recorded)


def _counts_sha(counts) -> str:
  return hashlib.sha256(np.ascontiguousarray(counts, dtype="<i8").tobytes()).hexdigest()


def state(hist) -> list:
  """Per channel: counts (or their SHA-256), the scalars as Python floats (exact for float32 / float64) and their types."""
  impls = hist._impls or []   # pylint: disable=protected-access
  inline = sum(len(h.counts) for h in impls) <= INLINE_COUNTS
  out = []
  for h in impls:
    rec = {"initialized": bool(h.initialized), "n": int(len(h.counts)), "sum": int(h.counts.sum()),
           "bin_width": None if h.bin_width is None else float(h.bin_width), "bin_width_type": type(h.bin_width).__name__,
           "lower_bound": float(h.lower_bound), "lower_bound_type": type(h.lower_bound).__name__,
           "global_min": float(h.global_min), "global_min_type": type(h.global_min).__name__,
           "global_max": float(h.global_max), "global_max_type": type(h.global_max).__name__}
    if inline:
      rec["counts"] = [int(v) for v in h.counts]
    else:
      rec["counts_sha256"] = _counts_sha(h.counts)
    out.append(rec)
  return out


def _sha_json(obj) -> str:
  import json
  return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def state_digest(hist) -> str:
  full = state(hist)
  for rec in full:              # -0.0 + 0.0 is +0.0: zeros print alike
    for key in ("global_min", "global_max", "lower_bound"):
      rec[key] = rec[key] + 0.0
  return _sha_json(full)


def recorded_state(hist):
  """What the golden file keeps of a state: all of it, or its digest and first channels when there are many."""
  full = state(hist)
  if len(full) <= INLINE_CHANNELS:
    return full
  return {"channels": len(full), "state_sha256": state_digest(hist), "head": full[:HEAD_CHANNELS]}


def check(hist, recorded, label="") -> None:
  """Exact equality with a recorded state: counts as int64 arrays, widths and bounds as values and types, extrema by ==
  (-0.0 == 0.0: the sign of a zero minimum is not defined by np.min)."""
  impls = hist._impls or []   # pylint: disable=protected-access
  if isinstance(recorded, dict):
    assert len(impls) == recorded["channels"], (label, len(impls), recorded["channels"])
    assert all(h.counts.dtype == np.int64 for h in impls), label
    check_channels(impls[:HEAD_CHANNELS], recorded["head"], label)
    assert state_digest(hist) == recorded["state_sha256"], f"{label}: state differs beyond the first {HEAD_CHANNELS} channels"
    return
  assert len(impls) == len(recorded), (label, len(impls), len(recorded))
  check_channels(impls, recorded, label)


def check_channels(impls, recorded, label) -> None:
  for i, (h, r) in enumerate(zip(impls, recorded)):
    where = f"{label} channel {i}"
    assert bool(h.initialized) == r["initialized"], where
    assert h.counts.dtype == np.int64, (where, h.counts.dtype)
    if "counts" in r:
      assert np.array_equal(h.counts, np.asarray(r["counts"], np.int64)), (where, h.counts.tolist(), r["counts"])
    else:
      assert len(h.counts) == r["n"] and int(h.counts.sum()) == r["sum"], (where, len(h.counts), int(h.counts.sum()), r)
      assert _counts_sha(h.counts) == r["counts_sha256"], where
    for key in ("bin_width", "lower_bound"):
      mine = getattr(h, key)
      assert type(mine).__name__ == r[key + "_type"], (where, key, type(mine).__name__, r[key + "_type"])
      assert (None if mine is None else float(mine)) == r[key], (where, key, mine, r[key])
    for key in ("global_min", "global_max"):
      mine = getattr(h, key)
      assert type(mine).__name__ == r[key + "_type"], (where, key, type(mine).__name__, r[key + "_type"])
      assert float(mine) == r[key], (where, key, mine, r[key])


class NumpyKernels:
  """A NumPy stand-in for the two kernels, for the seam mi355q.utils.histogram_utils._BACKEND: the explicit float32
  subtraction, division, floor and clip (float64 where the state calls for it), not a call into the reference."""

  def resident(self, data):
    arr = np.asarray(data)
    return np.ascontiguousarray(arr) if arr.dtype == np.float32 else None

  @staticmethod
  def shape(handle):
    return tuple(handle.shape)

  @staticmethod
  def _planes(handle, view):
    return np.moveaxis(handle.reshape(view), 1, 0).reshape(view[1], -1)

  def stats(self, handles, views):
    mn, mx, cnt = [], [], []
    for h, v in zip(handles, views):
      for plane in self._planes(h, v):
        f = plane[np.isfinite(plane)]
        mn.append(f.min() if f.size else np.float32(np.inf))
        mx.append(f.max() if f.size else np.float32(-np.inf))
        cnt.append(f.size)
    return np.asarray(mn, np.float32), np.asarray(mx, np.float32), np.asarray(cnt, np.int64)

  def bins(self, handles, views, lower, width, n_bins, precision):
    offsets = np.concatenate([[0], np.cumsum(n_bins)[:-1]]).astype(np.int64)
    out = np.zeros(int(np.sum(n_bins)), np.int64)
    slot = 0
    for h, v in zip(handles, views):
      for plane in self._planes(h, v):
        n = n_bins[slot]
        if n:
          x = plane[np.isfinite(plane)]
          if precision == 0:
            q = np.divide(np.subtract(x, np.float32(lower[slot]), dtype=np.float32), np.float32(width[slot]), dtype=np.float32)
          elif precision == 1:
            q = np.subtract(x, np.float32(lower[slot]), dtype=np.float32).astype(np.float64) / np.float64(width[slot])
          else:
            q = (x.astype(np.float64) - np.float64(lower[slot])) / np.float64(width[slot])
          idx = np.clip(np.floor(q), 0, n - 1).astype(np.int64)
          out[offsets[slot]:offsets[slot] + n] += np.bincount(idx, minlength=n)
        slot += 1
    return out, offsets
