"""Dynamic histograms of activations: the reference's second calibration statistic, collected on the GPU.

ref: utils/histogram_utils.py (_DynamicHistogram1D, DynamicHistogram). A histogram grows with the data, stays inside a bin
budget by doubling its bin width, can be merged and exports a {'min', 'max', 'axis', 'channels': [...]} map.

Where the work is. Only two steps of `add` touch the data: the finite min / max / count, and the binning
idx = clip(int32(floor((x - lower_bound) / bin_width)), 0, n - 1). Both run as HIP kernels over tensors that stay in HBM
(csrc/histogram.hip through ops.hist_stats_entries / ops.hist_bins_entries). Everything else -- initialisation, padding,
doubling, merge -- is scalar decisions plus pads and pair-sums of at most max_bins integers: a few thousand integer
operations per call on the host, not a hot path, and it works without a GPU. Those decisions read len(counts),
lower_bound and bin_width and never a count, so K samples need two launches, not 2 K: one for every sample's statistics,
the state machine run over them on a shadow of the state to learn the (lower_bound, bin_width, n) each sample is binned
with, one launch that bins every sample into a row of its own, and the state machine again on the real state, adding
row k where the sequential code adds it. Pads and pair-sums are linear in the counts, so the result is the sequential one.

Number types. The state holds NumPy scalars exactly as the reference's does under NEP 50 promotion: np.float32 throughout
for float32 data, a Python float bin_width when initial_bin_width is given, np.float64 after from_dict of float64 values.
The kernel is told which of the subtraction and the division NumPy would carry out in float64.

Data that is not float32 (the reference then works in float64) takes a host NumPy route. Inputs whose finite range
overflows float32 are out of scope: the reference then produces NaN indices.
"""
from __future__ import annotations

import copy
from typing import Any, Mapping, Sequence

import numpy as np


class _DynamicHistogram1D:
  """One growing histogram: counts (int64), bin_width, lower_bound, global_min / global_max.  ref :24-271."""

  def __init__(self, max_bins: int = 2048, initial_bin_width: float | None = None):
    self.bin_width = initial_bin_width
    self.max_bins = max_bins
    self.counts = np.zeros(1, dtype=np.int64)
    self.lower_bound = 0.0
    self.initialized = False
    self.global_min = float("inf")
    self.global_max = float("-inf")

  @classmethod
  def from_dict(cls, d: Mapping[str, Any], max_bins: int = 2048) -> "_DynamicHistogram1D":
    obj = cls(max_bins=max_bins)
    if "hist_counts" in d:
      obj.counts = np.array(d["hist_counts"], dtype=np.int64)
      obj.lower_bound = d["lower_bound"]
      obj.bin_width = d["bin_width"]
      obj.initialized = True
      first = lambda v: v[0] if isinstance(v, (np.ndarray, list, tuple)) else v  # noqa: E731  (scalar or one-element array)
      obj.global_min, obj.global_max = first(d["min"]), first(d["max"])
    return obj

  def to_dict(self) -> dict[str, Any]:
    if not self.initialized:
      return {}
    return {"hist_counts": self.counts, "bin_edges": self.bin_edges, "bin_width": self.bin_width,
            "lower_bound": self.lower_bound, "min": np.array([self.global_min]), "max": np.array([self.global_max])}

  @property
  def bin_edges(self) -> np.ndarray:
    if not self.initialized:
      return np.array([self.lower_bound])
    return self.lower_bound + np.arange(len(self.counts) + 1) * self.bin_width

  # ---- the state machine: scalar decisions, pads and pair-sums (host, no GPU) ----
  def _initialize(self, d_min, d_max) -> None:
    if self.bin_width is None:
      span = d_max - d_min
      pad = span * 0.1 if span > 0 else 1e-4          # 10 % on either side; +-1e-4 when all values are equal
      low, high = d_min - pad, d_max + pad
      self.lower_bound = low
      self.bin_width = max((high - low) / self.max_bins, 1e-5)
      n = self.max_bins
    else:
      self.lower_bound = d_min
      n = max(int(np.ceil((d_max - d_min) / self.bin_width)), 1)
    self.counts = np.zeros(n, dtype=np.int64)
    self.initialized = True

  def _double_bin_width_and_compact(self) -> None:
    c = self.counts
    if len(c) % 2:
      c = np.concatenate([c, np.zeros(1, dtype=c.dtype)])   # an odd length gets its zero at the END
    self.counts = c.reshape(-1, 2).sum(axis=1)
    self.bin_width *= 2.0                                   # lower_bound stays

  def _expand_to_fit(self, d_min, d_max) -> None:
    if d_min < self.lower_bound:
      missing = lambda: int(np.ceil((self.lower_bound - d_min) / self.bin_width))  # noqa: E731
      left = missing()
      while len(self.counts) + left > self.max_bins:
        self._double_bin_width_and_compact()
        left = missing()
      self.counts = np.concatenate([np.zeros(left, dtype=np.int64), self.counts])
      self.lower_bound -= left * self.bin_width
    upper = self.lower_bound + len(self.counts) * self.bin_width
    if d_max > upper:
      right = int(np.ceil((d_max - upper) / self.bin_width))
      while len(self.counts) + right > self.max_bins:
        self._double_bin_width_and_compact()
        upper = self.lower_bound + len(self.counts) * self.bin_width
        right = int(np.ceil((d_max - upper) / self.bin_width))
      self.counts = np.concatenate([self.counts, np.zeros(right, dtype=np.int64)])

  def _prepare(self, d_min, d_max):
    """Everything `add` does before it bins data whose finite extrema are d_min / d_max. -> the (lower_bound, bin_width, n)
    that data is binned with."""
    self.global_min = min(self.global_min, d_min)
    self.global_max = max(self.global_max, d_max)
    if not self.initialized:
      self._initialize(d_min, d_max)
    self._expand_to_fit(d_min, d_max)
    return self.lower_bound, self.bin_width, len(self.counts)

  def _shadow(self) -> "_DynamicHistogram1D":
    """A copy that takes the same decisions (they never read a count)."""
    s = copy.copy(self)
    s.counts = np.zeros(len(self.counts), dtype=np.int64)
    return s

  def add(self, data: np.ndarray) -> None:
    """Host route: finite values in a NumPy array, binned in the arithmetic NumPy gives their dtype."""
    data = np.asarray(data)
    if data.size == 0:
      return
    data = data.ravel()
    lower, width, n = self._prepare(np.min(data), np.max(data))
    idx = np.clip(np.floor((data - lower) / width).astype(np.int32), 0, n - 1)
    self.counts += np.bincount(idx, minlength=n)

  def _accumulate_resampled(self, other: "_DynamicHistogram1D") -> None:
    """Spreads every bin of `other` over the bins of this one it overlaps, by overlap length; rounds at the end."""
    acc = self.counts.astype(np.float64)
    for i, c in enumerate(other.counts):
      if c == 0:
        continue
      left = other.lower_bound + i * other.bin_width
      right = left + other.bin_width
      j0 = max(0, int(np.floor((left - self.lower_bound) / self.bin_width)))
      j1 = min(len(self.counts), int(np.ceil((right - self.lower_bound) / self.bin_width)))
      for j in range(j0, j1):
        mine = self.lower_bound + j * self.bin_width
        lo, hi = max(left, mine), min(right, mine + self.bin_width)
        if lo < hi:
          acc[j] += c * ((hi - lo) / other.bin_width)
    self.counts = np.round(acc).astype(np.int64)

  def merge(self, other: "_DynamicHistogram1D") -> None:
    self.global_min = min(self.global_min, other.global_min)
    self.global_max = max(self.global_max, other.global_max)
    if not other.initialized:
      return
    if not self.initialized:
      self.bin_width, self.counts, self.lower_bound = other.bin_width, np.copy(other.counts), other.lower_bound
      self.initialized = True
      return
    while self.bin_width < other.bin_width:
      self._double_bin_width_and_compact()
    self._expand_to_fit(other.lower_bound, other.lower_bound + len(other.counts) * other.bin_width)
    self._accumulate_resampled(other)


# ---- the per-element step -----------------------------------------------------------------------------------------------
_PRECISION: dict = {}   # (type of lower_bound, type of bin_width) -> 0 / 1 / 2: promotion depends on the types only


def _precision(lower_bound, bin_width) -> int:
  """Which of `(x - lower_bound) / bin_width` NumPy carries out in float64 for float32 x (ops.hist_bins_entries)."""
  key = (type(lower_bound), type(bin_width))
  if key not in _PRECISION:
    diff = np.zeros(1, np.float32) - lower_bound
    _PRECISION[key] = 2 if diff.dtype == np.float64 else 1 if (diff / bin_width).dtype == np.float64 else 0
  return _PRECISION[key]


class _GpuBackend:
  """The two kernels. A handle is a contiguous float32 device tensor."""

  def resident(self, data):
    """float32 data as this backend's handle, or None for data of another dtype (host route)."""
    import torch
    from mi355q import runtime as rt
    if isinstance(data, rt.HbmArray):
      data = data.device_tensor
    if isinstance(data, torch.Tensor):
      if data.dtype != torch.float32:
        raise TypeError(f"DynamicHistogram.add takes float32 device tensors, got {data.dtype}")
      rt.require_gpu()
      if not data.is_cuda:
        return data.to(rt.device())
      return data if data.is_contiguous() else data.contiguous()    # (a copy; the caller's buffer is only read)
    arr = np.asarray(data)
    if arr.dtype != np.float32:
      return None
    rt.require_gpu()
    return rt.to_device(arr)

  @staticmethod
  def shape(handle):
    return tuple(handle.shape)

  def stats(self, handles, views):
    from mi355q import ops
    mn, mx, cnt = ops.hist_stats_entries([h.data_ptr() for h in handles], [v[0] for v in views], [v[1] for v in views],
                                         [v[2] for v in views])
    return mn.cpu().numpy(), mx.cpu().numpy(), cnt.cpu().numpy()

  def bins(self, handles, views, lower, width, n_bins, precision):
    from mi355q import ops
    out, offsets = ops.hist_bins_entries([h.data_ptr() for h in handles], [v[0] for v in views], [v[1] for v in views],
                                         [v[2] for v in views], lower, width, n_bins, precision)
    return out.cpu().numpy(), offsets


_BACKEND = _GpuBackend()   # the seam of the per-element step: tests/test_histogram_host.py puts a NumPy stand-in here


def _view(shape, axis):
  """[outer, channels, inner] of a contiguous tensor; channels = 1 for axis None."""
  if axis is None:
    return 1, 1, int(np.prod(shape, dtype=np.int64))
  ax = axis + len(shape) if axis < 0 else axis
  return (int(np.prod(shape[:ax], dtype=np.int64)), int(shape[ax]), int(np.prod(shape[ax + 1:], dtype=np.int64)))


def _add_batch(items) -> None:
  """items: (DynamicHistogram, data) in the order the sequential code would add them. float32 data of the whole list goes
  through two launches; data of another dtype is added on the host at its place in the order."""
  run = []
  for hist, data in items:
    size = int(np.prod(tuple(data.shape), dtype=np.int64))
    if size == 0:
      continue
    handle = _BACKEND.resident(data)
    if handle is None:
      _run_resident(run)
      run = []
      hist._add_host(np.asarray(data))   # pylint: disable=protected-access
    else:
      run.append((hist, handle))
  _run_resident(run)


def _run_resident(run) -> None:
  if not run:
    return
  views, handles = [], []
  for hist, handle in run:
    shape = _BACKEND.shape(handle)
    hist._ensure_impls(shape)            # pylint: disable=protected-access
    view = _view(shape, hist.axis)
    if view[1] != len(hist._impls):      # pylint: disable=protected-access
      raise ValueError(f"Cannot add: data has {view[1]} channels on axis {hist.axis}, the histogram has"
                       f" {len(hist._impls)}")   # pylint: disable=protected-access
    views.append(view)
    handles.append(handle)
  mn, mx, cnt = _BACKEND.stats(handles, views)

  def walk(impls_of, rows):
    """The state machine over the run, in order. rows None: plan (-> per slot lower bound, width, n); else: add rows."""
    lower, width, n_bins, slot = [], [], [], 0
    for hist, _ in run:
      for impl in impls_of(hist):
        if cnt[slot] > 0:
          lb, bw, n = impl._prepare(mn[slot], mx[slot])   # pylint: disable=protected-access
          if rows is not None:
            impl.counts += rows[0][rows[1][slot]:rows[1][slot] + n]
        else:
          lb, bw, n = 0.0, 1.0, 0
        lower.append(lb)
        width.append(bw)
        n_bins.append(n)
        slot += 1
    return lower, width, n_bins

  shadows = {}

  def shadow_of(hist):
    if id(hist) not in shadows:
      shadows[id(hist)] = [impl._shadow() for impl in hist._impls]   # pylint: disable=protected-access
    return shadows[id(hist)]

  lower, width, n_bins = walk(shadow_of, None)
  # one launch per arithmetic: a table is almost always of one kind
  kinds = [(_precision(lb, bw) if n else -1) for lb, bw, n in zip(lower, width, n_bins)]
  counts = np.zeros(int(np.sum(n_bins, dtype=np.int64)), np.int64)
  offsets = np.zeros(len(n_bins), np.int64)
  if len(n_bins) > 1:
    np.cumsum(np.asarray(n_bins[:-1], np.int64), out=offsets[1:])
  for kind in sorted(set(kinds) - {-1}):
    masked = [n if k == kind else 0 for n, k in zip(n_bins, kinds)]
    part, part_offsets = _BACKEND.bins(handles, views, [float(v) for v in lower], [float(v) for v in width], masked, kind)
    for s, n in enumerate(masked):
      if n:
        counts[offsets[s]:offsets[s] + n] = part[part_offsets[s]:part_offsets[s] + n]
  walk(lambda hist: hist._impls, (counts, offsets))   # pylint: disable=protected-access


class DynamicHistogram:
  """Per-tensor (axis None) or per-channel histograms of one tensor; the bin budget is shared out among the channels.
  ref :274-480."""

  def __init__(self, max_tensor_bins: int = 2048, initial_bin_width: float | None = None, axis: int | None = None):
    self.initial_bin_width = initial_bin_width
    self.max_tensor_bins = max_tensor_bins
    self.axis = axis
    self._impls: Sequence[_DynamicHistogram1D] | None = None
    self._ndim: int | None = None     # of the data seen, for the shape of min_max_for_coverage

  @property
  def initialized(self) -> bool:
    if self._impls is None:
      return False
    return self._impls[0].initialized if self.axis is None else True

  @property
  def global_min(self) -> np.ndarray:
    if self._impls is None:
      return np.array([float("inf")]) if self.axis is None else np.array([])
    return np.array([h.global_min for h in self._impls])

  @property
  def global_max(self) -> np.ndarray:
    if self._impls is None:
      return np.array([float("-inf")]) if self.axis is None else np.array([])
    return np.array([h.global_max for h in self._impls])

  def _per_tensor(self, name: str, unset):
    if self.axis is not None:
      raise AttributeError(f"{name} is not supported for per-channel histogram, use _impls[i].{name}")
    return unset if self._impls is None else getattr(self._impls[0], name)

  @property
  def counts(self) -> np.ndarray:
    return self._per_tensor("counts", np.zeros(1, dtype=np.int64))

  @property
  def bin_width(self) -> float | None:
    return self._per_tensor("bin_width", None)

  @property
  def lower_bound(self) -> float:
    return self._per_tensor("lower_bound", 0.0)

  @property
  def bin_edges(self) -> np.ndarray:
    return self._per_tensor("bin_edges", np.array([0.0]))

  def _ensure_impls(self, shape) -> None:
    self._ndim = len(shape)
    if self._impls is not None:
      return
    channels = 1 if self.axis is None else int(shape[self.axis])
    per_channel = self.max_tensor_bins if self.axis is None else max(self.max_tensor_bins // channels, 1)
    self._impls = [_DynamicHistogram1D(max_bins=per_channel, initial_bin_width=self.initial_bin_width)
                   for _ in range(channels)]

  def _add_host(self, data: np.ndarray) -> None:
    """The host route of data that is not float32: NumPy, in the arithmetic of the data's dtype."""
    self._ensure_impls(data.shape)
    if self.axis is None:
      planes = [data.ravel()]
    else:
      moved = np.moveaxis(data, self.axis, 0)
      if moved.shape[0] != len(self._impls):
        raise ValueError(f"Cannot add: data has {moved.shape[0]} channels on axis {self.axis}, the histogram has"
                         f" {len(self._impls)}")
      planes = [moved[i].ravel() for i in range(len(self._impls))]
    for impl, plane in zip(self._impls, planes):
      finite = plane[np.isfinite(plane)]
      if finite.size:
        impl.add(finite)

  def add(self, data) -> None:
    """Adds a host ndarray, a torch device tensor or a runtime.HbmArray. Device data is read in place (a non-contiguous
    tensor through a contiguous copy); host float32 data is uploaded once; other dtypes are binned on the host."""
    _add_batch([(self, data)])

  def add_many(self, samples) -> None:
    """K samples of this tensor, in order, in two launches."""
    _add_batch([(self, s) for s in samples])

  def merge(self, other: "DynamicHistogram") -> None:
    if self.axis != other.axis:
      raise ValueError(f"Cannot merge histograms with different axis: {self.axis} vs {other.axis}")
    if self._impls is None and other._impls is not None:
      self._impls = [_DynamicHistogram1D(max_bins=other._impls[0].max_bins, initial_bin_width=self.initial_bin_width)
                     for _ in range(len(other._impls))]
      self._ndim = other._ndim
    if self._impls is None or other._impls is None:
      return
    if len(self._impls) != len(other._impls):
      raise ValueError(f"Cannot merge: different number of channels: {len(self._impls)} vs {len(other._impls)}")
    for mine, theirs in zip(self._impls, other._impls):
      mine.merge(theirs)

  def to_dict(self) -> dict[str, Any]:
    if not self.initialized:
      return {}
    return {"min": self.global_min, "max": self.global_max, "axis": self.axis,
            "channels": [h.to_dict() for h in self._impls]}

  @classmethod
  def from_dict(cls, d: Mapping[str, Any], max_tensor_bins: int = 2048) -> "DynamicHistogram":
    if not d:
      return cls(max_tensor_bins=max_tensor_bins)
    if "channels" not in d:
      raise ValueError(f"Invalid dictionary format for DynamicHistogram: {d}")
    obj = cls(max_tensor_bins=max_tensor_bins, axis=d["axis"])
    per_channel = max(max_tensor_bins // len(d["channels"]), 1)
    obj._impls = [_DynamicHistogram1D.from_dict(h, max_bins=per_channel) for h in d["channels"]]
    return obj

  def min_max_for_coverage(self, p: float) -> dict[str, np.ndarray]:
    """The range that keeps a fraction p of the mass, (1 - p) / 2 cut from either tail, per channel, from the bin edges.

    With T = counts.sum() and tail = (1 - p) / 2 * T: the lower value is bin_edges[j] for the largest j with
    counts[:j].sum() <= tail, the upper value bin_edges[j] for the smallest j with counts[j:].sum() <= tail, both clamped
    into [global_min, global_max]; p = 1 gives the global min and max. -> {'min', 'max'}: float32 arrays of the shape a
    min/max QSV of the tensor has ((1,) * ndim per tensor; the channel axis kept otherwise). Host only."""
    if not 0 < p <= 1:
      raise ValueError(f"coverage must be in (0, 1], got {p}")
    impls = self._impls or []
    lows, highs = [], []
    for h in impls:
      if not h.initialized:
        lows.append(h.global_min)
        highs.append(h.global_max)
        continue
      below = np.concatenate([[0], np.cumsum(h.counts)])      # below[j] = counts[:j].sum()
      total = below[-1]
      tail = (1 - p) / 2 * total
      edges = h.bin_edges
      low = edges[np.nonzero(below <= tail)[0][-1]]
      high = edges[np.nonzero(total - below <= tail)[0][0]]
      lows.append(min(max(low, h.global_min), h.global_max))
      highs.append(min(max(high, h.global_min), h.global_max))
    ndim = self._ndim if self._ndim else 1
    if self.axis is None:
      shape = (1,) * ndim
    else:
      ax = self.axis + ndim if self.axis < 0 else self.axis
      shape = tuple(len(impls) if k == ax else 1 for k in range(ndim)) if self._ndim else (len(impls),)
    return {"min": np.asarray(lows, np.float32).reshape(shape), "max": np.asarray(highs, np.float32).reshape(shape)}


class ActivationHistograms:
  """Histograms of named activations over a calibration dataset: one DynamicHistogram per tensor name, fed with the
  {tensor name: array} maps Quantizer.calibrate takes, every named float32 tensor of all K samples in two launches.
  axis: None (per tensor), one axis for every tensor, or a {tensor name: axis} map (tensors it does not name: per tensor)."""

  def __init__(self, max_tensor_bins: int = 2048, initial_bin_width: float | None = None, axis: int | None = None):
    self.max_tensor_bins = max_tensor_bins
    self.initial_bin_width = initial_bin_width
    self.axis = axis
    self._hists: dict[str, DynamicHistogram] = {}

  def _hist(self, name: str) -> DynamicHistogram:
    if name not in self._hists:
      axis = self.axis.get(name) if isinstance(self.axis, Mapping) else self.axis
      self._hists[name] = DynamicHistogram(self.max_tensor_bins, self.initial_bin_width, axis)
    return self._hists[name]

  def add_samples(self, samples, names=None) -> None:
    """samples: a list of {tensor name: host array, device tensor or HbmArray}; names: the tensors to take (default all)."""
    items = []
    for sample in samples:
      for name, data in sample.items():
        if names is None or name in names:
          items.append((self._hist(name), data))
    _add_batch(items)

  def __getitem__(self, name: str) -> DynamicHistogram:
    return self._hists[name]

  def __contains__(self, name: str) -> bool:
    return name in self._hists

  def __iter__(self):
    return iter(self._hists)

  def __len__(self) -> int:
    return len(self._hists)

  def merge(self, other: "ActivationHistograms") -> None:
    for name in other:
      self._hist(name).merge(other[name])

  def to_dict(self) -> dict[str, Any]:
    return {name: h.to_dict() for name, h in self._hists.items()}

  @classmethod
  def from_dict(cls, d: Mapping[str, Any], max_tensor_bins: int = 2048) -> "ActivationHistograms":
    obj = cls(max_tensor_bins=max_tensor_bins, axis={})
    for name, hd in d.items():
      obj._hists[name] = DynamicHistogram.from_dict(hd, max_tensor_bins=max_tensor_bins)
      obj.axis[name] = obj._hists[name].axis
    return obj
