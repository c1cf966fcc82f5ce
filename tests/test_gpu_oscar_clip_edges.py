"""Edges of OSCAR's clip search (csrc/oscar.hip) through the C ABI mi355q_oscar_clip_bounds_f32, both routes:
every call runs once as is (CHANNELWISE rows of 384..16384 columns may be answered by clip_prefix_kernel) and once
with MI355Q_OSCAR_PREFIX=0 (full sort + scan for every row). Bounds and scales of both must be the bits of the FP64
model of the scan with the caller's own u and noise (oscar_scan_model.scan_clip_bounds, proven against the oracle
and the recorded reference in test_oscar_scan_model.py). Several kinds of rows share a tensor, so every workgroup
starts on LDS that another row has used."""
import numpy as np
import pytest

from oscar_scan_model import product_u_noise, scan_clip_bounds

pytestmark = pytest.mark.gpu


def _bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _target(g):
  """Elements the prefix kernel asks for by default (mi355q_oscar_clip_bounds_f32)."""
  if g <= 4096:
    return min(max(g // 16, 128), 256)
  return min(max(g // 32, 256), 512)


def _geometry(g):
  """(threads per row, elements per thread) of the prefix kernel's instantiation for g columns."""
  if g <= 1024:
    return 64, 16
  if g <= 2048:
    return 64, 32
  if g <= 4096:
    return 64, 64
  if g <= 8192:
    return 256, 32
  return 256, 64


def _clip(monkeypatch, w, s, m, g, u, noise, qmax, blockwise=False, rows=None):
  """Both routes against the model; returns the prefix route's rows-left flags (None: the call had no prefix route).
  rows: the segments whose bounds must equal the model's (default all; the others are compared route to route)."""
  import torch
  from mi355q import ops
  f64 = ops._f64_dev                                                    # pylint: disable=protected-access
  args = (torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda(), f64(s), f64(m), g, f64(u), f64(noise), qmax,
          blockwise)
  b1, s1, left = ops.oscar_clip_bounds(*args, want_bounds=True, want_scale=True, want_rows_left=True)
  monkeypatch.setenv("MI355Q_OSCAR_PREFIX", "0")
  b0, s0, none = ops.oscar_clip_bounds(*args, want_bounds=True, want_scale=True, want_rows_left=True)
  monkeypatch.delenv("MI355Q_OSCAR_PREFIX")
  assert none is None
  b1, s1, b0, s0 = (t.cpu().numpy() for t in (b1, s1, b0, s0))
  assert np.array_equal(_bits(b1), _bits(b0)) and np.array_equal(_bits(s1), _bits(s0))
  want_b, want_s = scan_clip_bounds(w, s, m, g, u, noise, qmax, blockwise)
  sel = slice(None) if rows is None else rows
  bad = np.flatnonzero(_bits(b0)[sel] != _bits(want_b)[sel])
  assert bad.size == 0, (bad[:8], b0[sel][bad[:8]], want_b[sel][bad[:8]])
  assert np.array_equal(_bits(s0)[sel], _bits(want_s)[sel])
  return None if left is None else left.cpu().numpy()


def _provable_without_next(a, mm, u, nk, g):
  """The prefix kernel's step 4 for a row whose unselected elements are all zero (a_next = 0), on the row's non-zero
  keys a (stable descending) and their masses: True / False when the proof holds / fails by a wide margin, None when
  it is too close to call."""
  s_m, s_am, s_a2m = np.cumsum(mm)[-1], np.cumsum(a * mm)[-1], np.cumsum((a * a) * mm)[-1]
  run_m, run_am, run_a2m = np.cumsum(mm), np.cumsum(a * mm), np.cumsum((a * a) * mm)
  c = np.clip((2.0 * run_am) / (u + 2.0 * run_m), np.append(a[1:], 0.0), a)
  e = ((c * c * nk + run_a2m) - (2.0 * c) * run_am) + (c * c) * run_m
  best = min((a[0] * a[0]) * nk, e.min())
  slack = 64.0 * g * 2.0 ** -53 * ((a[0] * a[0]) * nk + 4.0 * s_a2m)
  gap = s_a2m - best                                                    # e_next = E(0) = S_a2m
  assert 2.0 * s_am / (u + 2.0 * s_m) >= 0.0
  if gap > 40.0 * slack:
    return True
  if gap < 0.0:
    return False
  return None


# ---- every instantiation of the prefix kernel and its borders ---------------------------------------------------------
def _mixed_rows(rng, n, g):
  """n rows of different kinds: ordinary with loud columns, heavy tail, ties, sparse, a few leading non-zeros, zeros."""
  w = rng.standard_normal((n, g)) * 0.02
  w[0, : max(1, g // 64)] *= 12.0
  w[1] *= np.exp(rng.standard_normal(g) * 1.2)
  w[2] = np.round(w[2] * 300) / 300
  w[3] = np.where(rng.random(g) < 0.05, w[3], 0.0)
  w[4, 3:] = 0.0
  w[5] = 0.0
  w[6:, g - 1] = 0.5                                                    # the ragged last lane holds the maximum
  return w.astype(np.float32)


@pytest.mark.parametrize("g", [383, 384, 1024, 1025, 2048, 2049, 4096, 4097, 5000, 8192, 8193, 11008, 16384, 16385])
def test_every_width_border(g, monkeypatch):
  rng = np.random.default_rng(g)
  n = 9
  w = _mixed_rows(rng, n, g)
  s = np.exp(rng.normal(size=g) * 0.3)
  m = np.exp(rng.normal(size=g) * 1.5)
  u, noise = product_u_noise(m, 7)
  left = _clip(monkeypatch, w, s, m, g, u, noise, 7)
  if g < 384 or g > 16384:
    assert left is None
  else:
    assert left is not None
    assert left[5] == 1                                                 # all zeros: the full route


# ---- sparse rows: the multi-wave form's next-element count (all unselected elements zero) ----------------------------
def _sparse_positions(rng, g, k):
  threads, ept = _geometry(g)
  special = [0, g - 1]
  for first in (0, (ept - 1) * threads):
    for wv in range(threads // 64):
      special += [first + 64 * wv, first + 64 * wv + 63]
  special = [p for p in dict.fromkeys(special) if p < g]
  if k <= len(special):
    return np.array(special[:k])
  rest = rng.choice(np.setdiff1d(np.arange(g), special), k - len(special), replace=False)
  return np.concatenate([special, rest])


@pytest.mark.parametrize("g", [1024, 4096, 8192, 16384])
def test_sparse_rows_both_forms(g, monkeypatch):
  """k non-zeros within 2^7 of the row maximum, the rest exactly zero (below == 0 in the kernel: nothing is listed as
  the next element), and the same rows with one more element ten binades down (below != 0). Masses of one order of
  magnitude."""
  rng = np.random.default_rng(100 + g)
  t = _target(g)
  ks = sorted({1, 2, 3, 17, 255, 256, 257, t - 1, t, t + 1})
  n = 2 * len(ks)
  w = np.zeros((n, g), np.float32)
  for r, k in enumerate(ks):
    pos = _sparse_positions(rng, g, k)
    mag = 2.0 ** rng.uniform(-6.5, 0.0, k)
    w[r, pos] = (np.where(rng.random(k) < 0.5, -1.0, 1.0) * mag).astype(np.float32)
    w[len(ks) + r] = w[r]
    spare = np.setdiff1d(np.arange(g), pos)
    w[len(ks) + r, int(spare[rng.integers(spare.size)])] = np.float32(mag.max() * 2.0 ** -10.5)
  s = np.ones(g)
  m = rng.uniform(1.0, 10.0, g)
  u, noise = product_u_noise(m, 7)
  left = _clip(monkeypatch, w, s, m, g, u, noise, 7)
  assert left is not None
  for r, k in enumerate(ks):
    if k > t:
      continue                                                          # the bisection drops some non-zeros
    nz = np.flatnonzero(w[r])
    a = np.abs(w[r, nz].astype(np.float64))
    order = np.argsort(-a, kind="stable")
    verdict = _provable_without_next(a[order], m[nz][order], u[0], noise[0], g)
    assert verdict is True, (k, verdict)                                # (the rows are built for it)
    assert left[r] == 0, (g, k)


# ---- multi-wave forms of the kinds the full route must take ----------------------------------------------------------
@pytest.mark.parametrize("g", [8192, 16384])
def test_multi_wave_rows_for_the_full_route(g, monkeypatch):
  rng = np.random.default_rng(200 + g)
  n = 12
  w = (rng.standard_normal((n, g)) * 0.02).astype(np.float32)
  m = rng.uniform(1.0, 10.0, g)
  q = g // 4
  m[-q:] = 1e-30                                                        # weightless last quarter
  w[0] = 0.0                                                            # zeros
  w[1, 10] = np.nan                                                     # non-finite keys
  w[2, g - 1] = np.inf
  w[3, 0] = -np.inf
  w[4] = np.where(rng.random(g) < 0.5, -0.5, 0.5)                       # const: every key in one bin
  top = _target(g) + 100                                                # crowded: target + 100 keys on top, then 300 equal
  idx = rng.permutation(g)
  w[5] = (rng.standard_normal(g) * 1e-4).astype(np.float32)
  w[5, idx[:top]] = (1.0 + 0.04 * rng.random(top)).astype(np.float32)
  w[5, idx[top:top + 300]] = 0.5
  w[6, -q:] *= 100.0                                                    # weightless: loud where clipping is free
  w[7, -q:] = 0.0                                                       # an ordinary row next to them
  w[8, 0] = w[8, g - 1] = 0.7                                           # equal keys at 0 and g-1 (composite tie-break)
  w[9, 0] = w[9, g - 1] = -0.7
  w[9, 1] = 0.7
  w[10, :5] = [0.3, -0.2, 0.25, 0.1, 0.3]                               # a few leading non-zeros
  w[10, 5:] = 0.0
  w[11, :-q] *= np.exp(rng.standard_normal(g - q) * 1.2)
  s = np.ones(g)
  u, noise = product_u_noise(m, 7)
  finite = np.array([r for r in range(n) if r != 1])
  left = _clip(monkeypatch, w, s, m, g, u, noise, 7, rows=finite)
  assert left is not None
  assert left[[0, 1, 2, 3, 4, 5, 6]].all(), left
  a = np.abs(w[10, :5].astype(np.float64))
  order = np.argsort(-a, kind="stable")
  assert _provable_without_next(a[order], m[:5][order], u[0], noise[0], g) is True
  assert left[10] == 0, left


@pytest.mark.parametrize("g", [1024, 8192])
def test_keys_below_the_float32_pattern_floor(g, monkeypatch):
  """Positive keys below 2^-133 have a float32 pattern whose upper half is 0, like exact zeros. Row 0: twenty keys near
  2^-130 and fifty near 2^-136 whose columns carry most of the mass, so the optimum lies among the tiny ones: the
  prefix route must not take the tiny keys for zeros (a_next = 0 put its bound a hundred times too low). Row 2: only
  tiny keys."""
  rng = np.random.default_rng(900 + g)
  w = np.zeros((4, g), np.float32)
  cols = rng.permutation(g)
  big, tiny = cols[:20], cols[20:70]
  w[0, big] = (2.0 ** -130 * rng.uniform(1, 2, 20)).astype(np.float32)
  w[0, tiny] = (2.0 ** -136 * rng.uniform(1, 2, 50)).astype(np.float32)
  w[1] = (rng.standard_normal(g) * 0.02).astype(np.float32)
  w[2, tiny] = w[0, tiny]
  m = np.ones(g)
  m[tiny] = 1e6
  u, noise = product_u_noise(m, 7)
  left = _clip(monkeypatch, w, np.ones(g), m, g, u, noise, 7)
  assert left is not None and left[3] == 1


# ---- limits of the prefix search -------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,target", [(1024, 32), (1024, 512), (4096, 32), (4096, 512), (8192, 32), (8192, 1024),
                                      (16384, 32), (16384, 1024)])
def test_prefix_target_limits(g, target, monkeypatch):
  """MI355Q_OSCAR_PREFIX_TARGET at 32 and at its maximum: the selected count P on both sides of the LDS cap."""
  rng = np.random.default_rng(300 + g + target)
  w = _mixed_rows(rng, 8, g)
  w[7] = np.round(rng.standard_normal(g) * 4) / 64                      # coarse ties around the cap
  s = np.exp(rng.normal(size=g) * 0.3)
  m = np.exp(rng.normal(size=g) * 1.5)
  u, noise = product_u_noise(m, 7)
  monkeypatch.setenv("MI355Q_OSCAR_PREFIX_TARGET", str(target))
  left = _clip(monkeypatch, w, s, m, g, u, noise, 7)
  assert left is not None and left[5] == 1


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_qmax_limits(bits, monkeypatch):
  """qmax 3 is below the prefix route's floor (7); 7 and 127 take it."""
  rng = np.random.default_rng(400 + bits)
  g = 4096
  w = _mixed_rows(rng, 8, g)
  s = np.exp(rng.normal(size=g) * 0.3)
  m = np.exp(rng.normal(size=g) * 1.5)
  qmax = 2 ** (bits - 1) - 1
  u, noise = product_u_noise(m, qmax)
  left = _clip(monkeypatch, w, s, m, g, u, noise, qmax)
  assert (left is None) == (qmax < 7)


# ---- the caller's own u and noise --------------------------------------------------------------------------------------
@pytest.mark.parametrize("u,noise", [(0.01, 0.005), (1e3, 1e-3), (0.0, 0.5), (1e-9, 1e4), (5.0, 0.0), (2e4, 1e4)])
@pytest.mark.parametrize("g", [1024, 4096, 16384])
def test_caller_u_noise(g, u, noise, monkeypatch):
  """u / noise unrelated to sum(m) (bench.py's own pair among them), s != 1, masses over 10+ decades."""
  rng = np.random.default_rng(500 + g)
  w = _mixed_rows(rng, 8, g)
  s = np.exp(rng.normal(size=g) * 1.5)
  m = np.exp(rng.normal(size=g) * 5.0)
  m[:3] = [1e-7, 1e5, 1e-3]
  left = _clip(monkeypatch, w, s, m, g, np.array([u]), np.array([noise]), 7)
  assert left is not None and left[5] == 1


def test_negative_noise_or_mass_takes_the_full_route(monkeypatch):
  """The convexity the prefix route rests on needs noise >= 0 and masses >= 0: otherwise every row is flagged."""
  rng = np.random.default_rng(600)
  g = 8192
  w = _mixed_rows(rng, 8, g)
  w[:, 17] = 0.0
  s = np.ones(g)
  m = rng.uniform(1.0, 10.0, g)
  u, noise = product_u_noise(m, 7)
  left = _clip(monkeypatch, w, s, m, g, u, -noise, 7)
  assert left.all(), left
  m[17] = -1e-3                                                         # (a zero column: the running mass stays positive)
  left = _clip(monkeypatch, w, s, m, g, u, noise, 7)
  assert left.all(), left


# ---- layouts only the full route takes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [32, 128, 256])
def test_blockwise_full_route(g, monkeypatch):
  rng = np.random.default_rng(700 + g)
  n, d = 24, 1024
  w = _mixed_rows(rng, n, d)
  s = np.exp(rng.normal(size=d) * 1.0)
  m = np.exp(rng.normal(size=d) * 5.0)
  groups = d // g
  u = np.exp(rng.normal(size=groups) * 2.0)
  noise = np.exp(rng.normal(size=groups) * 2.0)
  assert _clip(monkeypatch, w, s, m, g, u, noise, 7, blockwise=True) is None


@pytest.mark.parametrize("n,d", [(3, 5000), (2, 8193), (5, 4097)])
def test_tensorwise_beyond_one_tile(n, d, monkeypatch):
  """TENSORWISE: one segment of n * d elements, sorted as 8192-element runs and merged."""
  rng = np.random.default_rng(800 + n * d)
  w = (rng.standard_normal((n, d)) * 0.02).astype(np.float32)
  w[0, :40] *= 30.0
  w[1, 5:] = 0.0
  s = np.exp(rng.normal(size=d) * 1.0)
  m = np.exp(rng.normal(size=d) * 5.0)
  assert _clip(monkeypatch, w, s, m, n * d, np.array([0.01]), np.array([0.005]), 7) is None
  assert _clip(monkeypatch, w, s, m, n * d, *product_u_noise(np.tile(m, n), 7), 7) is None
