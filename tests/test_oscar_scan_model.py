"""The FP64 model of the OSCAR clip search (oscar_scan_model.scan_clip_bounds) against the oracle's
breakpoint scan and against the bounds and scales the real reference recorded
(tests/golden/ref_oscar_cases.*). No GPU: this is what the GPU edge tests
(test_gpu_oscar_clip_edges.py) hold the kernels to."""
import json
import os

import numpy as np
import pytest

from oracle import aeq_oracle as O
from oscar_scan_model import product_u_noise, scan_clip_bounds

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_oscar_cases.json")) as _f:
  CASES = {c["name"]: c for c in json.load(_f)["cases"] if "granularity" in c}


def _same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _block(gran):
  return int(gran.split("_")[1]) if gran.startswith("BLOCKWISE") else 0


def _u_noise(m, n, d, g, qmax, gran):
  """Per-group u and noise from the masses, as algorithms/uniform_quantize/oscar.py forms them."""
  if gran == "TENSORWISE":
    return product_u_noise(np.tile(m, n), qmax)
  pairs = [product_u_noise(m[k * g:(k + 1) * g], qmax) for k in range(d // g)]
  return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def _segments(gran, n, d):
  if gran == "TENSORWISE":
    return n * d
  return _block(gran) or d


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_recorded_reference_bounds(name):
  """Every recorded OSCAR case (CHANNELWISE, BLOCKWISE_*, TENSORWISE): s from the case, masses floored from mu2 / s^2."""
  c = CASES[name]
  z = np.load(os.path.join(HERE, "golden", "ref_oscar_cases.npz"))
  w = z[f"{name}/w"]
  n, d = w.shape
  s = z[f"{name}/s"] if f"{name}/s" in z.files else np.ones(d)
  m = O.oscar_floor_masses(z[f"{name}/mu2"] / (s * s)) if c["has_mu2"] else np.ones(d)
  qmax = 2 ** (c["num_bits"] - 1) - 1
  gran = c["granularity"]
  g = _segments(gran, n, d)
  u, noise = _u_noise(m, n, d, g, qmax, gran)
  bounds, scales = scan_clip_bounds(w, s, m, g, u, noise, qmax, blockwise_scale=gran.startswith("BLOCKWISE"))
  want_b = z[f"{name}/bounds"]
  want_s = z[f"{name}/scale"]
  assert _same(bounds.reshape(want_b.shape), want_b)
  if gran.startswith("BLOCKWISE"):
    assert want_s.dtype == np.float32 and _same(scales.astype(np.float32).reshape(want_s.shape), want_s)
    assert _same(scales, scales.astype(np.float32).astype(np.float64))
  else:
    assert _same(scales.reshape(want_s.shape), want_s)


def _oracle_bounds(w, s, m, qmax, gran):
  mag = np.abs(w.astype(np.float64)) * s
  n, d = w.shape
  if gran == "TENSORWISE":
    return O.oscar_group_clip(mag.reshape(1, n * d), np.tile(m, n), qmax)
  b = _block(gran)
  if not b:
    return O.oscar_group_clip(mag, m, qmax)
  out = np.empty((n, d // b))
  for k in range(d // b):
    out[:, k] = O.oscar_group_clip(mag[:, k * b:(k + 1) * b], m[k * b:(k + 1) * b], qmax)
  return out.ravel()


@pytest.mark.parametrize("seed,n,d,bits,gran,kind", [
    (1, 40, 384, 4, "CHANNELWISE", "std"), (2, 9, 4097, 4, "CHANNELWISE", "std"), (3, 30, 1000, 8, "CHANNELWISE", "tail"),
    (4, 20, 640, 4, "CHANNELWISE", "sparse"), (5, 12, 256, 4, "BLOCKWISE_32", "std"), (6, 7, 512, 8, "BLOCKWISE_128", "tail"),
    (7, 5, 512, 2, "BLOCKWISE_256", "std"), (8, 11, 300, 4, "TENSORWISE", "std"), (9, 16, 2048, 4, "CHANNELWISE", "grid"),
    (10, 16, 256, 4, "BLOCKWISE_64", "grid"), (11, 3, 16384, 4, "CHANNELWISE", "masses"), (12, 64, 96, 3, "TENSORWISE", "grid"),
])
def test_model_equals_oracle_with_product_u_noise(seed, n, d, bits, gran, kind):
  """With u and noise formed from the masses as the product forms them, the model is the oracle's scan. Ties only
  among equal masses (grid: uniform masses), where the oracle's unstable argsort cannot change the sums."""
  rng = np.random.default_rng(seed)
  w = rng.standard_normal((n, d)) * 0.02
  s = np.exp(rng.normal(size=d) * 0.4)
  mu2 = np.exp(rng.normal(size=d) * 1.5)
  if kind == "tail":
    w = w * np.exp(rng.standard_normal((n, d)) * 1.2)
  elif kind == "sparse":
    w = np.where(rng.random((n, d)) < 0.05, w, 0.0)
  elif kind == "grid":
    w = np.round(w * 200) / 200
    s = np.ones(d)
    mu2 = np.ones(d)
  elif kind == "masses":
    mu2 = np.exp(rng.normal(size=d) * 9.0)
  w = w.astype(np.float32)
  m = O.oscar_floor_masses(mu2 / (s * s))
  qmax = 2 ** (bits - 1) - 1
  g = _segments(gran, n, d)
  u, noise = _u_noise(m, n, d, g, qmax, gran)
  bounds, scales = scan_clip_bounds(w, s, m, g, u, noise, qmax, blockwise_scale=gran.startswith("BLOCKWISE"))
  want = np.asarray(_oracle_bounds(w, s, m, qmax, gran)).ravel()
  assert _same(bounds, want)
  _, want_scale = O.zp_scale_from_min_max(-want, want, bits, True, gran if gran.startswith("BLOCKWISE") else "CHANNELWISE")
  assert _same(scales, np.asarray(want_scale, np.float64))


def test_model_uses_the_callers_u_and_noise():
  """u and noise are the caller's, per group: a segment's answer moves with its own group's pair only."""
  rng = np.random.default_rng(3)
  w = (rng.standard_normal((4, 256)) * 0.02).astype(np.float32)
  s, m = np.ones(256), np.exp(rng.normal(size=256))
  u = np.array([0.01, 0.01, 50.0, 0.01, 0.01, 0.01, 0.01, 0.01])
  noise = np.array([0.005, 0.005, 25.0, 0.005, 0.005, 0.005, 0.005, 0.005])
  b, _ = scan_clip_bounds(w, s, m, 32, u, noise, 7)
  b0, _ = scan_clip_bounds(w, s, m, 32, np.full(8, 0.01), np.full(8, 0.005), 7)
  moved = (b != b0).reshape(4, 8)
  assert moved[:, 2].all() and not moved[:, [0, 1, 3, 4, 5, 6, 7]].any()
  # heavier noise clips harder: every bound of group 2 went down
  assert (b.reshape(4, 8)[:, 2] < b0.reshape(4, 8)[:, 2]).all()


def test_model_tie_order_is_stable():
  """Equal keys with different masses: the stable order (lower position first) decides, as the ABI defines it."""
  w = np.array([[1.0, 0.5, 1.0, 0.25]], np.float32)
  m = np.array([1.0, 1.0, 1e-6, 1.0])
  u, noise = np.array([0.0]), np.array([1.0])
  b, _ = scan_clip_bounds(w, np.ones(4), m, 4, u, noise, 7)
  # by hand: sorted (1.0, m=1), (1.0, m=1e-6), (0.5, 1), (0.25, 1)
  a = np.array([1.0, 1.0, 0.5, 0.25])
  mm = np.array([1.0, 1e-6, 1.0, 1.0])
  rm, ram, ra2m = np.cumsum(mm), np.cumsum(a * mm), np.cumsum((a * a) * mm)
  c = np.clip((2.0 * ram) / (0.0 + 2.0 * rm), np.append(a[1:], 0.0), a)
  e = ((c * c * 1.0 + ra2m) - (2.0 * c) * ram) + (c * c) * rm
  want = np.concatenate([[1.0], c])[np.argmin(np.concatenate([[1.0], e]))]
  assert b[0] == want
