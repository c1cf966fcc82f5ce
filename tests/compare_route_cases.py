"""Designed inputs for every route of the tensor comparison kernels (csrc/validation.hip: mi355q_compare_f32 and
mi355q_compare_f32_batched), with host models of the routes. NumPy only. Shared by test_compare_route_cases_host.py
(which proves, without a GPU, that every named route has a case, that the references are self-consistent and that the
sum cases tell NumPy's order of addition from its neighbours) and test_gpu_compare_routes.py (which holds the kernels
to the references, case by case).

  chunk_shape(m)            what compare_sums_kernel does with a chunk of m elements: NumPy's pairwise leaves, whether
                            the kernel's own predicate calls the chunk balanced, the depth of the tree, the leaf forms
  median_route(bits, n)     the three-level radix select over the uint32 ratio patterns: the bins chosen, where the
                            upper middle value comes from, the chunk each middle lies in
  cases()                   every case; route_table(cases()) -> {route name: [case names]}
  reference_record(t, r)    the eight fields of mi355q_compare_result as NumPy forms them, with the bounds of the
                            fields that are not bit-exact

The sums use float32 data whose float32 sum depends on the order of addition (standard normal values times a
per-element power of two in 2^-6 .. 2^6). The median cases plant exact ratios: with r = 1 - 17 * 2^-24 the float32
sum |r| + 1e-6 is exactly 1, and t = r - k * 2^-24 is representable, so the ratio of an element is exactly k * 2^-24;
for k in [2^23, 2^24) the patterns are the consecutive integers 0x3F000000 + (k - 2^23), and the level-1, level-2 and
level-3 bins of an element are bit fields of k.
"""
import collections
import functools

import numpy as np

import layer_error_cases as LE

F = np.float32
CHUNK = 8192              # kChunk
LEAF = 128                # NumPy's pairwise block
WAVE = 64
COMBINE_TILE = 2048       # kCombineTile
MAX_LEAVES = 256          # kMaxLeaves: the LDS arrays of compare_sums_kernel
U24 = 2.0 ** -24
K0 = 1 << 23              # planted k = K0 + j has the ratio pattern 0x3F000000 + j
R0 = F(F(1) - F(17 * U24))
LARGE_N = (1 << 24) + CHUNK + 5     # 2050 chunks: the second tile of compare_combine_kernel


# ----------------------------------------------------------------------------- the pairwise tree of one chunk
def numpy_split(n: int) -> int:
  n2 = n // 2
  return n2 - n2 % 8


def plain_split(n: int) -> int:
  """Halving without the multiple-of-8 rule (alternative (b) of the host test)."""
  return n // 2


def leaves_of(m: int, split=numpy_split):
  """([(start, length)] of the pairwise leaves of [0, m) in order, depth of the tree)."""
  out = []

  def rec(s, n, d):
    if n <= LEAF:
      out.append((s, n))
      return d
    n2 = split(n)
    return max(rec(s, n2, d + 1), rec(s + n2, n - n2, d + 1))

  return out, rec(0, m, 0)


def leaf_form(n: int) -> str:
  return "short" if n < 8 else ("mult8" if n % 8 == 0 else "strided_tail")


def kernel_balanced(m: int):
  """(balanced, depth) by compare_sums_kernel's own predicate."""
  depth = 0
  while (m >> depth) > LEAF:
    depth += 1
  leaf = m >> depth
  return (leaf << depth) == m and leaf >= 8 and leaf % 8 == 0, depth


ChunkShape = collections.namedtuple("ChunkShape", "leaves balanced depth forms")


@functools.lru_cache(maxsize=None)
def chunk_shape(m: int) -> ChunkShape:
  leaves, depth = leaves_of(m)
  balanced, kdepth = kernel_balanced(m)
  if balanced:      # what the level-by-level tree assumes: 2^depth equal leaves
    assert depth == kdepth and len(leaves) == 1 << depth and len({n for _, n in leaves}) == 1
  return ChunkShape(tuple(n for _, n in leaves), balanced, depth, frozenset(leaf_form(n) for _, n in leaves))


def balanced_lengths() -> list:
  return [m for m in range(1, CHUNK + 1) if kernel_balanced(m)[0]]


# ----------------------------------------------------------------------------- models of the order of addition
def leaf_sum(a) -> np.float32:
  """NumPy's pairwise_sum of a run of <= 128 float32 values."""
  n = len(a)
  if n < 8:
    res = F(0.0)
    for v in a:
      res = F(res + v)
    return res
  full = n & ~7
  r = np.add.accumulate(a[:full].reshape(-1, 8), axis=0, dtype=F)[-1]     # eight accumulators, each in order
  res = F(F(F(r[0] + r[1]) + F(r[2] + r[3])) + F(F(r[4] + r[5]) + F(r[6] + r[7])))
  for v in a[full:]:
    res = F(res + v)
  return res


def chunk_sum(a, split=numpy_split) -> np.float32:
  n = len(a)
  balanced, depth = kernel_balanced(n)
  if balanced and depth:            # equal leaves under either split rule: all of them at once, then level by level
    x = a.reshape(1 << depth, -1, 8)
    r = np.add.accumulate(x, axis=1, dtype=F)[:, -1, :]
    v = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    while len(v) > 1:
      v = v[0::2] + v[1::2]
    return F(v[0])
  if n <= LEAF:
    return leaf_sum(a)
  n2 = split(n)
  return F(chunk_sum(a[:n2], split) + chunk_sum(a[n2:], split))


def _pairwise_scalars(v):
  if len(v) == 1:
    return v[0]
  h = len(v) // 2
  return F(_pairwise_scalars(v[:h]) + _pairwise_scalars(v[h:]))


def model_sum(x, split=numpy_split, combine="left") -> np.float32:
  """float32 sum of x: chunks of 8192, `split` inside, the chunk sums added left to right or ("pairwise") in a tree."""
  x = np.asarray(x, F)
  parts = [chunk_sum(x[i:i + CHUNK], split) for i in range(0, len(x), CHUNK)]
  if combine == "pairwise":
    return _pairwise_scalars(parts)
  acc = parts[0]
  for p in parts[1:]:
    acc = F(acc + p)
  return acc


def left_to_right_sum(x) -> np.float32:
  return F(np.add.accumulate(np.asarray(x, F), dtype=F)[-1])


ALTERNATIVES = {
    "left_to_right": left_to_right_sum,                                   # (a)
    "plain_halving": lambda x: model_sum(x, split=plain_split),           # (b)
    "pairwise_chunks": lambda x: model_sum(x, combine="pairwise"),        # (c)
}


def chunk_lengths(n: int) -> list:
  nc = -(-n // CHUNK)
  return [CHUNK] * (nc - 1) + [n - (nc - 1) * CHUNK]


def alternative_applies(n: int, alt: str) -> bool:
  """Is `alt` really another order of addition than NumPy's at length n?"""
  lens = chunk_lengths(n)
  if alt == "left_to_right":
    return n >= 8                                       # below 8 NumPy itself adds left to right
  if alt == "plain_halving":
    return any(leaves_of(m, plain_split)[0] != leaves_of(m)[0] for m in set(lens))
  if alt == "pairwise_chunks":
    return len(lens) >= 3                               # (a + b) + c against a + (b + c)
  raise ValueError(alt)


def sum_class(n: int) -> str:
  lens = chunk_lengths(n)
  if len(lens) > 1:
    return "two_chunks" if len(lens) == 2 else "three_or_more_chunks"
  s = chunk_shape(n)
  if n < 8:
    return "short"
  if n <= LEAF:
    return "one_leaf"
  return f"balanced_depth_{s.depth}" if s.balanced else "unbalanced"


# ----------------------------------------------------------------------------- the radix select of the median
MedianRoute = collections.namedtuple("MedianRoute", "bins lo hi source first_difference chunk_lo chunk_hi")


def median_route(ratio_bits, n: int) -> MedianRoute:
  """The select kernels' walk over the ratio patterns of one pair: bins at levels 1, 2 and 3 (bits 30..20, 19..9,
  8..0), the patterns of the two middles, the source of the upper one ("odd", "same_bin", "later_bin", "min_above"),
  for min_above the field in which the middles first differ ("19..9" or "30..20"), and element // 8192 of each middle
  (ties resolved as a stable sort does)."""
  u = np.asarray(ratio_bits, np.uint32)
  assert u.shape == (n,) and n >= 1 and not (u >> 31).any()

  def pick(values, bins, k):
    h = np.bincount(values, minlength=bins).astype(np.int64)
    c = np.cumsum(h)
    b = int(np.searchsorted(c, k, side="right"))
    return b, int(c[b] - h[b]), h

  k = (n - 1) // 2
  b1, below, _ = pick((u >> 20).astype(np.int64), 2048, k)
  k -= below
  sel = u[(u >> 20) == b1]
  b2, below, _ = pick(((sel >> 9) & 2047).astype(np.int64), 2048, k)
  k -= below
  prefix = (b1 << 11) | b2
  sel = u[(u >> 9) == prefix]
  b3, below, h3 = pick((sel & 511).astype(np.int64), 512, k)
  lo = (prefix << 9) | b3
  above = u[(u >> 9) > prefix]
  min_above = int(above.min()) if above.size else 0xFFFFFFFF
  first = None
  if n % 2:
    source, hi = "odd", lo
  else:
    r2 = k + 1
    cum = below + int(h3[b3])
    b = b3
    while cum <= r2 and b < 511:
      b += 1
      cum += int(h3[b])
    if cum > r2:
      source, hi = ("same_bin" if b == b3 else "later_bin"), (prefix << 9) | b
    else:
      source, hi = "min_above", min_above
      first = "19..9" if (hi >> 20) == (lo >> 20) else "30..20"
  order = np.argsort(u, kind="stable")
  return MedianRoute((b1, b2, b3), np.uint32(lo), np.uint32(hi), source, first,
                     int(order[(n - 1) // 2]) // CHUNK, int(order[n // 2]) // CHUNK)


# ----------------------------------------------------------------------------- references
def prep(x):
  return np.nan_to_num(np.asarray(x, F).ravel(), nan=1e-9, neginf=-1e9, posinf=1e9)


def ratios(t, r):
  """float32 |t - r| / (|r| + 1e-6) after nan_to_num, as validation_utils.median_diff_ratio forms it."""
  t, r = prep(t), prep(r)
  return np.abs(t - r) / (np.abs(r) + F(1e-6))


def reference_record(t, r, median: bool = True) -> dict:
  """What NumPy gives for the fields of mi355q_compare_result of target t against reference r (n >= 1).
  sum_sq_diff / sum_ref_sq / median_lo / median_hi are to be met bit for bit; dot_* within n * 2^-52 * Sum|terms| (any
  order of a float64 sum of the float32 products), sum_kl within 1e-5 * Sum|terms| + 1e-30 (logf against NumPy's log)."""
  t, r = prep(t), prep(r)
  n = t.size
  with np.errstate(all="ignore"):
    out = {"n": n, "sum_sq_diff": F(np.sum(np.square(t - r))), "sum_ref_sq": F(np.sum(np.square(r)))}
    p, q = np.maximum(F(0), r), np.maximum(F(0), t)
    terms = p * np.log((p + F(1e-9)) / (q + F(1e-9)))
    out["sum_kl"] = F(np.sum(terms))
    out["kl_bound"] = 1e-5 * float(np.sum(np.abs(terms.astype(np.float64)))) + 1e-30
    for name, a, b in (("dot_tr", t, r), ("dot_tt", t, t), ("dot_rr", r, r)):
      prod = (a * b).astype(np.float64)                  # the product rounded to float32 first
      out[name] = float(np.sum(prod))
      out[name + "_bound"] = n * 2.0 ** -52 * float(np.sum(np.abs(prod)))
    if median:
      s = np.sort(ratios(t, r))
      out["median_lo"], out["median_hi"] = s[(n - 1) // 2], s[n // 2]
  return out


# ----------------------------------------------------------------------------- the sums list
SumCase = collections.namedtuple("SumCase", "name group n seed kind")
MULTI_CHUNKS = (1, 2, 3, 63, 64, 65)
MULTI_TAILS = (0, 1, 7, 8, 129, 4096, 8191)
FIRST_LENGTHS = 264


def sum_lengths() -> list:
  ns = set(range(1, FIRST_LENGTHS + 1))
  for m in balanced_lengths():
    ns.add(m)
    if m > FIRST_LENGTHS:
      ns.update((m - 1, m + 1))
  ns.update(CHUNK * c + m for c in MULTI_CHUNKS for m in MULTI_TAILS)
  return sorted(ns)


def sum_cases() -> list:
  out = [SumCase(f"sum_n{n}", "sums", n, 10_000 + i, "noise") for i, n in enumerate(sum_lengths())]
  out.append(SumCase("integers_n8193", "sums", CHUNK + 1, 20_001, "integers"))
  for i, n in enumerate((100, CHUNK + 1)):
    out.append(SumCase(f"kl_zero_equal_positive_n{n}", "sums", n, 20_010 + i, "equal_positive"))
    out.append(SumCase(f"kl_zero_nonpositive_reference_n{n}", "sums", n, 20_020 + i, "nonpositive_reference"))
  return out


def order_sensitive(rng, n: int):
  """float32 values whose float32 sum depends on the order: N(0, 1) times a per-element power of two, 2^-6 .. 2^6."""
  return np.ldexp(rng.standard_normal(n, dtype=F), rng.integers(-6, 7, n).astype(np.int32)).astype(F)


def sum_pair(c):
  """(target, reference) float32 of a SumCase (or of the large case)."""
  rng = np.random.default_rng(c.seed)
  if c.kind == "integers":          # every product and every float64 sum of products is exact
    return rng.integers(-64, 65, c.n).astype(F), rng.integers(-64, 65, c.n).astype(F)
  r = order_sensitive(rng, c.n)
  if c.kind == "equal_positive":    # (p + e) / (q + e) = 1: every KL term is p * log(1) = 0
    r = np.abs(r) + F(2.0 ** -8)
    return r.copy(), r
  t = (r + order_sensitive(rng, c.n)).astype(F)
  if c.kind == "nonpositive_reference":   # p = max(0, r) = 0: every KL term is 0 * log(..) = 0
    r = -np.abs(r)
    r[::3] = F(0.0)
  return t, r


LargeCase = collections.namedtuple("LargeCase", "name group n seed kind")
LARGE = LargeCase("large_2050_chunks", "large", LARGE_N, 30_001, "noise")


# ----------------------------------------------------------------------------- the median list
MedianCase = collections.namedtuple("MedianCase", "name group n seed spec tags")
THREE_CHUNKS_EVEN = 2 * CHUNK + 100
BIN2_LAST = 2047 << 9      # j of level-2 bin 2047, level-3 bin 0, first level-1 bin


def _designed(name, n, lo, hi=None, where=None, seed=0, tags=()):
  return MedianCase(name, "median", n, 40_000 + seed, {"lo": lo, "hi": hi, "where": where}, tuple(tags))


def median_cases() -> list:
  out = [
      MedianCase("median_n1", "median", 1, 0, {"k": [K0 + 12345]}, ("median_n1",)),
      MedianCase("median_n2", "median", 2, 0, {"k": [K0 + 700, K0 + 5]}, ("median_n2",)),
      _designed("median_odd_n1001", 1001, 5 * 512 + 77, seed=1),
      _designed("median_odd_three_chunks", 2 * CHUNK + 101, (3 << 20) + 40 * 512 + 1, seed=2),
      _designed("median_tie_n1000", 1000, 9 * 512 + 300, 9 * 512 + 300, seed=3, tags=("median_tie",)),
      _designed("median_later_bin_n1000", 1000, 21 * 512 + 5, 21 * 512 + 300, seed=4),
      _designed("median_bins_510_511", 1000, 33 * 512 + 510, 33 * 512 + 511, seed=5),
      _designed("median_bins_0_511", 500, 34 * 512, 34 * 512 + 511, seed=6),
      _designed("median_bin3_0_odd", 999, (2 << 20) + 100 * 512, seed=7),
      _designed("median_bin3_0_next_pattern", 1000, (2 << 20) + 101 * 512, (2 << 20) + 101 * 512 + 1, seed=8),
      _designed("median_bin3_0_min_above", 1000, 50 * 512, 57 * 512 + 3, seed=9),
      MedianCase("median_identical_odd", "median", 1001, 0, {"k": [K0 + 77777] * 1001}, ("median_identical_odd",)),
      MedianCase("median_identical_even", "median", CHUNK + 8, 0, {"k": [K0 + 77777] * (CHUNK + 8)},
                 ("median_identical_even",)),
      MedianCase("median_all_zero_even", "median", 1000, 0, {"k": [0] * 1000}, ("median_all_zero",)),
      MedianCase("median_all_zero_odd", "median", 777, 0, {"k": [0] * 777}, ("median_all_zero",)),
      MedianCase("median_inf_pair_even", "median", 6, 0, {"k": [K0 + 9, -1, K0 + 1, -1, -1, K0 + 4], "special": "inf"},
                 ("median_inf_pair",)),
      MedianCase("median_inf_pair_odd", "median", 5, 0, {"k": [-1, K0 + 1, -1, -1, K0 + 4], "special": "inf"},
                 ("median_inf_pair",)),
      MedianCase("median_nan_reference", "median", 5, 0, {"k": [K0 + 3, -1, -1, 7, -1], "special": "nan"},
                 ("median_nan_reference",)),
      MedianCase("median_negative_zero", "median", 6, 0, {"k": [K0 + 3, -1, -1, K0 + 900, 2, -1], "special": "negzero"},
                 ("median_negative_zero",)),
  ]
  # the upper middle from outside the span: the next span of the same level-1 bin, a far span, another level-1 bin;
  # each with both middles in one chunk, the lower in chunk 0 and the upper in the last of three chunks, and reversed
  above = (("bits_19_9_next_span", 70 * 512 + 511, 71 * 512 + 2),
           ("bits_19_9_far_span", (1 << 20) + 300 * 512 + 7, (1 << 20) + 1200 * 512 + 400),
           ("bits_30_20_bin2_2047", (4 << 20) + BIN2_LAST + 511, (5 << 20) + 6),
           ("bits_30_20_bin2_2047_low_bin3", BIN2_LAST + 100, (2 << 20) + 3 * 512 + 9))
  for i, (nm, lo, hi) in enumerate(above):
    out.append(_designed(f"median_min_above_{nm}_n1000", 1000, lo, hi, seed=20 + 4 * i))
    for j, where in enumerate(((1, 1), (0, 2), (2, 0))):
      out.append(_designed(f"median_min_above_{nm}_chunks_{where[0]}_{where[1]}", THREE_CHUNKS_EVEN, lo, hi, where,
                           seed=21 + 4 * i + j))
  return out


def planted(k):
  """float32 target whose ratio against R0 is exactly k * 2^-24."""
  return (np.float64(R0) - np.asarray(k, np.float64) * U24).astype(F)


def median_pair(c):
  """(target, reference, k): k[i] >= 0 where element i carries the planted ratio k[i] * 2^-24, -1 elsewhere."""
  spec = c.spec
  if "k" in spec:
    k = np.asarray(spec["k"], np.int64)
  else:
    rng = np.random.default_rng(c.seed)
    n, lo = c.n, K0 + spec["lo"]
    hi = lo if spec["hi"] is None else K0 + spec["hi"]
    nb = (n - 1) // 2                         # strictly below the lower middle
    na = n - nb - (1 if n % 2 else 2)         # strictly above the upper middle: the middles are two known elements
    below = np.concatenate([lo - rng.integers(1, 4097, nb // 2), rng.integers(1, K0, nb - nb // 2)])
    above = np.concatenate([hi + rng.integers(1, 4097, na // 2), rng.integers(hi + 1, 1 << 24, na - na // 2)])
    others = rng.permutation(np.concatenate([below, above]))
    where = spec["where"]
    pos = []
    for ch in (where if where else (None, None)):
      while True:
        p = int(rng.integers(0, n)) if ch is None else ch * CHUNK + int(rng.integers(0, min(CHUNK, n - ch * CHUNK)))
        if p not in pos:
          pos.append(p)
          break
    k = np.empty(n, np.int64)
    mask = np.ones(n, bool)
    if n % 2:
      k[pos[0]] = lo
      mask[pos[0]] = False
    else:
      k[pos[0]], k[pos[1]] = lo, hi
      mask[pos] = False
    k[mask] = others
  assert k.shape == (c.n,) and (k < (1 << 24)).all()
  t = planted(np.maximum(k, 0))
  r = np.full(c.n, R0, F)
  special = spec.get("special")
  free = np.flatnonzero(k < 0)
  if special == "inf":                        # 1e9 against -1e9: the ratio is 2
    t[free], r[free] = np.inf, -np.inf
  elif special == "nan":                      # the denominator is 1e-9 + 1e-6
    r[free] = np.nan
    t[free] = np.asarray([0.5, 2e-6, 1e-7], F)[:free.size]
  elif special == "negzero":
    t[free], r[free] = F(-0.0), F(-0.0)
  else:
    assert free.size == 0
  return t, r, k


# ----------------------------------------------------------------------------- mixed target kinds in one table
MixedCase = collections.namedtuple("MixedCase", "name group kind n channels inner diff_bits zero_points seed tags")


def mixed_cases() -> list:
  M = lambda name, kind, n, channels=1, inner=1, diff_bits=32, zp=False, tags=(): MixedCase(
      name, "mixed", kind, n, channels, inner, diff_bits, zp, 50_000 + sum(name.encode()), (f"kind_{kind}",) + tuple(tags))
  return [
      M("mixed_f32", "f32", 777),
      M("mixed_f16", "f16", 1001),
      M("mixed_bf16", "bf16", 515),
      M("mixed_i8_channels_zero_points_wrap", "i8", 37 * 300, 37, 300, 8, True, ("kind_i8_zero_points_wrap_8",)),
      M("mixed_i8_per_tensor", "i8", 999, 1, 1, 32, False, ("kind_i8_per_tensor_no_zero_points",)),
      M("mixed_i16", "i16", 2 * 5 * 2000, 5, 2000, 16, True),
      M("mixed_i32_float64_product", "i32", 4099, 1, 1, 32, False, ("kind_i32_float64_product",)),
      M("mixed_i4_block32_odd_n", "i4", 37 * 32 + 1, 38, 32, 32, False, ("kind_i4_block32_odd_n",)),
      M("mixed_i2_n_mod4_3", "i2", 2103, 3, 701, 32, True, ("kind_i2_n_mod4_3",)),
      M("mixed_i8_inner_1", "i8", 1000, 7, 1, 32, True, ("kind_inner_1",)),
  ]


def _bf16(x):
  u = np.asarray(x, F).view(np.uint32)
  return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # round to nearest even


def mixed_entry(c):
  """(target as float32, reference, stored) with stored = {kind, data, scale, zero_point, channels, inner, diff_bits}:
  the integer kinds dequantized by layer_error_cases.dequantize, packed by layer_error_cases.pack."""
  rng = np.random.default_rng(c.seed)
  stored = {"kind": c.kind, "scale": None, "zero_point": None, "channels": c.channels, "inner": c.inner,
            "diff_bits": c.diff_bits}
  if c.kind in ("f32", "f16", "bf16"):
    x = rng.standard_normal(c.n).astype(F)
    if c.kind == "f32":
      data = t = x
    elif c.kind == "f16":
      data = x.astype(np.float16)
      t = data.astype(F)
    else:
      data = _bf16(x)
      t = (data.astype(np.uint32) << 16).view(F)
    stored["data"] = data
  else:
    bits = int(c.kind[1:])
    qmax = 2 ** (min(bits, 21) - 1) - 1
    q = rng.integers(-qmax - 1, qmax + 1, c.n)
    scale = (rng.uniform(0.5, 2.0, c.channels) * (1.37e-5 if bits == 32 else 4.0 / (qmax + 1))).astype(F)
    zlim = {8: 100, 16: 30_000}.get(c.diff_bits, 5)
    zp = rng.integers(-zlim, zlim + 1, c.channels).astype(np.int32) if c.zero_points else None
    t = LE.dequantize(q, scale, zp, c.channels, c.inner, c.diff_bits).astype(F)
    if bits >= 8:
      data = q.astype({8: np.int8, 16: np.int16, 32: np.int32}[bits])
    else:
      per = 8 // bits
      data = LE.pack(np.concatenate([q, np.zeros((-c.n) % per, q.dtype)]), bits)
    stored.update(data=data, scale=scale, zero_point=zp)
  r = (t + rng.standard_normal(c.n).astype(F) * F(0.03)).astype(F)
  return t, r, stored


# ----------------------------------------------------------------------------- device tables built by hand
TableCase = collections.namedtuple("TableCase", "name group lengths tags")
EMPTY_TABLES = [
    TableCase("table_empty_first", "empty_table", (0, 300, CHUNK + 1), ("table_empty_first",)),
    TableCase("table_empty_middle_pair", "empty_table", (300, 0, 0, CHUNK + 1, 77), ("table_empty_middle_pair",)),
    TableCase("table_empty_last", "empty_table", (CHUNK + 1, 300, 0), ("table_empty_last",)),
    TableCase("table_empty_around_full_chunks", "empty_table", (0, 2 * CHUNK, 0, 0, CHUNK, 5, 0),
              ("table_empty_first", "table_empty_middle_pair", "table_empty_last")),
    TableCase("table_all_empty", "empty_table", (0, 0, 0), ("table_all_empty_zero_chunks",)),
]
RefusalCase = collections.namedtuple("RefusalCase", "name group reason tags")
REFUSAL_REASONS = ("negative_n", "kind_9", "integer_kind_null_scale", "channels_0", "diff_bits_12",
                   "total_chunks_plus_1", "total_chunks_minus_1")
REFUSALS = [RefusalCase(f"refused_{r}", "refused", r, (f"refused_{r}",)) for r in REFUSAL_REASONS]


def table_pair(n: int, slot: int):
  """The pair at position `slot` of a hand-built table."""
  return sum_pair(SumCase("", "", n, 60_000 + 131 * slot + n, "noise"))


# ----------------------------------------------------------------------------- all cases and their routes
def cases() -> list:
  return sum_cases() + [LARGE] + median_cases() + mixed_cases() + EMPTY_TABLES + REFUSALS


def sum_routes(n: int) -> set:
  lens = chunk_lengths(n)
  out = set()
  for m in set(lens):
    s = chunk_shape(m)
    out |= {f"leaf_{f}" for f in s.forms}
    if s.balanced:
      out.add(f"tree_levels_depth_{s.depth}")
    else:
      out.add("tree_walk" if len(s.leaves) > 1 else "tree_walk_one_leaf")
  out.add("chunk_last_full" if lens[-1] == CHUNK else "chunk_last_partial")
  nc = len(lens)
  out.add("combine_one_chunk" if nc == 1 else "combine_chain")
  if nc > WAVE:
    out.add("combine_lane_loop_repeats")
  if nc > COMBINE_TILE:
    out.add("combine_second_tile")
  return out


def median_routes(c) -> set:
  t, r, _ = median_pair(c)
  m = median_route(ratios(t, r).view(np.uint32), c.n)
  out = set(c.tags) | {"median_" + m.source}
  if m.source == "min_above":
    out.add("median_min_above_first_difference_bits_" + m.first_difference.replace("..", "_"))
    nc = -(-c.n // CHUNK)
    if nc == 3 and m.chunk_lo == m.chunk_hi:
      out.add("median_min_above_both_in_one_chunk")
    if nc == 3 and (m.chunk_lo, m.chunk_hi) == (0, 2):
      out.add("median_min_above_lo_first_hi_last_chunk")
    if nc == 3 and (m.chunk_lo, m.chunk_hi) == (2, 0):
      out.add("median_min_above_hi_first_lo_last_chunk")
  b3_hi = int(m.hi) & 511
  if m.bins[2] == 0:
    out.add("median_lo_bin3_0")
  if m.bins[2] == 511:
    out.add("median_lo_bin3_511")
  if m.bins[1] == 2047:
    out.add("median_lo_bin2_2047")
  if m.source == "later_bin" and (m.bins[2], b3_hi) == (510, 511):
    out.add("median_later_bin_510_511")
  return out


def routes_of(c) -> set:
  if c.group in ("sums", "large"):
    out = sum_routes(c.n)
    out |= {"integers": {"dots_exact_integers"}, "equal_positive": {"kl_zero_equal_positive"},
            "nonpositive_reference": {"kl_zero_nonpositive_reference"}}.get(c.kind, set())
    return out
  if c.group == "median":
    return median_routes(c) | sum_routes(c.n)
  if c.group == "mixed":
    out = set(c.tags)
    if c.n > CHUNK and c.channels > 1:
      out.add("kind_scale_entry_across_chunk_boundary")
    return out
  return set(c.tags)


def route_table(all_cases) -> dict:
  """{route name: [names of the cases that reach it]}."""
  out = collections.defaultdict(list)
  for c in all_cases:
    for route in sorted(routes_of(c)):
      out[route].append(c.name)
  return dict(out)
