"""FP64 model of the OSCAR clip search as the C ABI mi355q_oscar_clip_bounds_f32 defines it
(include/mi355q.h): upstream's breakpoint scan (oscar.py:62-108), restated segment by segment with
the caller's own u[k] and noise[k] instead of the ones upstream derives from the masses, and with a
stable sort, the only tie order the ABI defines. test_oscar_scan_model.py proves it against the
oracle and the recorded reference outputs; the GPU edge tests compare both routes of the kernel with it."""
import numpy as np

from oracle import aeq_oracle as O


def scan_clip_bounds(w, s, m, g, u, noise, qmax, blockwise_scale=False):
  """(bounds, scales), float64 [n * d / g], of every g-element segment of the flattened float32 [n, d] weight.

  Element e of the flattened weight has key |float64(w)| * s[e % d] and mass m[e % d]; segment k
  takes u[k % G] and noise[k % G] (G = d / g, or 1 when g == n * d). Per segment: keys in stable
  descending order, running sums by np.cumsum, candidate 2 S_am / (u + 2 S_m) clipped to [next key
  (0 after the last), key], energy ((c^2 noise + S_a2m) - (2c) S_am) + c^2 S_m, the "clip nothing"
  candidate a_0^2 noise first, np.argmin's first minimum. scale = max(c, 1e-9) / qmax, rounded
  float64 -> float32 -> bfloat16 -> float16 when blockwise_scale."""
  w = np.asarray(w, np.float32)
  n, d = w.shape
  total = n * d
  if g != total and d % g:
    raise ValueError(f"g={g} neither divides d={d} nor covers the tensor")
  groups = 1 if g == total else d // g
  s = np.asarray(s, np.float64).ravel()
  m = np.asarray(m, np.float64).ravel()
  u = np.asarray(u, np.float64).ravel()
  noise = np.asarray(noise, np.float64).ravel()
  col = np.arange(total) % d
  keys = (np.abs(w.ravel().astype(np.float64)) * s[col]).reshape(-1, g)
  mass = m[col].reshape(-1, g)
  segs = keys.shape[0]
  uk = u[np.arange(segs) % groups][:, None]
  nk = noise[np.arange(segs) % groups][:, None]
  order = np.argsort(-keys, axis=1, kind="stable")
  a = np.take_along_axis(keys, order, 1)
  mm = np.take_along_axis(mass, order, 1)
  run_m = np.cumsum(mm, 1)
  run_am = np.cumsum(a * mm, 1)
  run_a2m = np.cumsum((a * a) * mm, 1)
  cand = (2.0 * run_am) / (uk + 2.0 * run_m)
  lower = np.concatenate([a[:, 1:], np.zeros((segs, 1))], 1)
  cand = np.clip(cand, lower, a)
  c2 = cand * cand
  with np.errstate(invalid="ignore"):                                  # (inf - inf of an infinite key: NaN, as upstream)
    err = ((c2 * nk + run_a2m) - (2.0 * cand) * run_am) + c2 * run_m
  all_c = np.concatenate([a[:, :1], cand], 1)
  all_e = np.concatenate([(a[:, :1] * a[:, :1]) * nk, err], 1)
  bounds = all_c[np.arange(segs), np.argmin(all_e, 1)]
  scales = np.maximum(bounds, 1e-9) / float(qmax)
  if blockwise_scale:
    scales = O.blockwise_scale_round(scales.astype(np.float32)).astype(np.float64)
  return bounds, scales


def product_u_noise(masses, qmax):
  """u = M / (6 qmax^2), noise = M / (12 qmax^2) with M = sum(masses) + 1e-12, as the product forms them
  for one group of masses (algorithms/uniform_quantize/oscar.py)."""
  total = np.array([float(np.asarray(masses, np.float64).sum()) + 1e-12])
  return total / (6.0 * qmax * qmax), total / (12.0 * qmax * qmax)
