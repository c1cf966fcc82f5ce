"""Which kernels the damped Hessian inverse runs (csrc/gptq.hip: hinv_impl, hinv_lockstep, hinv_batched_impl), and that
the exact cases of hinv_exact_cases.py are what they claim to be. No GPU.

route() restates the host's choices: the batch mode (one call, lock step in groups of kHinvGroup, a pool of lanes, or
one after the other), the copy kernel, the kind of every 64-column Cholesky step, the update behind every outer block
(one GEMM, or strip + rest with the look-ahead stream), every level of the triangular merge (bf16x3, one batched FP64
launch pair, the per-pair loop, a ragged last pair) and the kernel of the final product. features() turns a route into
elements of ALL_ROUTES; the case list of the GPU file (CASES, here so that it can be checked without a GPU) reaches
every one of them, and every case carries its route in its id.

Per (d, seed) of the case list: np.linalg.cholesky(H) == L bit for bit, L Linv == I, the 2^23 condition, the float32
round trip of the expected inverse and of the product form, and a non-zero in every 64 x 64 tile on or below the
diagonal of L, L^-1 and lower(H^-1) that the class rule allows one in.

The argument checks of the four entry points return before anything is launched and are tested here on host memory."""
import ctypes
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

import hinv_exact_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 64                    # NB of csrc/gptq.hip
GROUP = 32                 # kHinvGroup
LANES = 8                  # kHinvLanes
NO_FUSED, ASU, OB, NO_LOOKAHEAD, NO_SPLIT_COPY, FUSED_MAX_M, FP64, SPLIT_MIN_S, SIDE_DELAY, USE_LANES, NO_LANES, PAIRS = (
    "MI355Q_NO_FUSED_STEP", "MI355Q_CHOL_ASU", "MI355Q_CHOL_OB", "MI355Q_NO_LOOKAHEAD", "MI355Q_NO_SPLIT_COPY",
    "MI355Q_FUSED_MAX_M", "MI355Q_HINV_FP64", "MI355Q_HINV_SPLIT_MIN_S", "MI355Q_DEBUG_SIDE_DELAY_US", "MI355Q_HINV_LANES",
    "MI355Q_HINV_NO_LANES", "MI355Q_HINV_PAIRS")
SWITCHES = (NO_FUSED, ASU, OB, NO_LOOKAHEAD, NO_SPLIT_COPY, FUSED_MAX_M, FP64, SPLIT_MIN_S, SIDE_DELAY, USE_LANES, NO_LANES, PAIRS)


def workspace_bytes(d):
  return (d * d * 2 + NB * NB + d * NB * 2 + 8) * 8 if d > 0 else 0


def lane_bytes(d):
  return (workspace_bytes(d) + 255) & ~255


def _outer_block(env):
  v = int(env.get(OB, 0) or 0)
  return v if v >= 64 and v % 64 == 0 else 8 * NB


def merge_levels(d, split, split_min_s):
  """Per level s = 64, 128, ...: (s, kinds) with kinds from bf16x3, batched, loop:full, loop:ragged, in launch order."""
  levels = []
  s = NB
  while s < d:
    kinds = []
    first = 0
    full = (d - s) // (2 * s) + (1 if (d - s) % (2 * s) >= s else 0)
    if split and s >= split_min_s and full >= 1:
      kinds.append("bf16x3")
      first = full * 2 * s
    elif full >= 2 and s <= 2048:
      kinds.append("batched")
      first = full * 2 * s
    p = first
    while p + s < d:
      kinds.append("loop:full" if d - (p + s) >= s else "loop:ragged")
      p += 2 * s
    levels.append((s, tuple(kinds)))
    s *= 2
  return tuple(levels)


def single_route(d, form="f64", env=None):
  """hinv_impl() restated for one matrix: copy kernel, step kinds in launch order, outer updates, merge levels, product."""
  env = env or {}
  ob_max = _outer_block(env)
  side = d >= 4096 and NO_LOOKAHEAD not in env
  copy = "cols:caller+side" if side and d > 2 * ob_max and NO_SPLIT_COPY not in env else "full"
  fused_on = NO_FUSED not in env
  fused_max_m = int(env[FUSED_MAX_M]) if FUSED_MAX_M in env else 2048
  asu_on = ASU not in env or int(env[ASU]) != 0
  steps, outer = [], []
  for k0 in range(0, d, ob_max):
    ob = min(ob_max, d - k0)
    ready = False
    for k in range(k0, k0 + ob, NB):
      nb = min(NB, k0 + ob - k)
      m = d - k - nb
      w = k0 + ob - k - nb
      if (m > 0 and nb == NB and m % NB == 0 and w % NB == 0 and fused_on and (not side or m <= fused_max_m)
          and (w > 0 or ready)):
        steps.append(f"fused:{'w>0' if w > 0 else 'w=0'}:{'panel ready' if ready else 'copy_panel'}")
        ready = True
      elif asu_on and nb == NB and m % NB == 0 and w % NB == 0:
        steps.append(f"asu:{'m=0' if m == 0 else 'w=0' if w == 0 else 'update'}")
        ready = False
      else:
        steps.append(f"generic:{'m=0' if m == 0 else 'w=0' if w == 0 else 'gemm'}:{'nb=64' if nb == NB else 'nb<64'}")
    m2 = d - k0 - ob
    if m2 > 0:
      nxt = min(m2, ob_max)
      if not side:
        outer.append("one gemm")
      elif m2 - nxt < 2048:
        outer.append("one gemm behind the side stream")
      else:
        outer.append("strip+rest")
  split_min_s = int(env.get(SPLIT_MIN_S, 0) or 0)
  split_min_s = split_min_s if split_min_s >= 128 else 1024
  split = FP64 not in env and d >= 4096 and d % 128 == 0 and d <= 16384
  return dict(copy=f"{form}:{copy}", steps=tuple(steps), outer=tuple(outer), side=side,
              delay=side and int(env.get(SIDE_DELAY, 0) or 0) > 0 and "strip+rest" in outer,
              merge=merge_levels(d, split, split_min_s), product="ltl_bf16x3" if split else "gemm", mirror="mirror_lower_f32")


def lockstep_route(d, env=None):
  """hinv_lockstep() restated: whole 64-column steps only, FP64 throughout, every launch over the whole group."""
  ob_max = _outer_block(env or {})
  steps, outer = [], []
  for k0 in range(0, d, ob_max):
    ob = min(ob_max, d - k0)
    for k in range(k0, k0 + ob, NB):
      m, w = d - k - NB, k0 + ob - k - NB
      steps.append(f"lockstep:{'m=0' if m == 0 else 'w=0' if w == 0 else 'update'}")
    if d - k0 - ob > 0:
      outer.append("one gemm over the group")
  return dict(copy="f64:batched", steps=tuple(steps), outer=tuple(outer), side=False, delay=False,
              merge=merge_levels(d, False, 1024), product="gemm over the group", mirror="mirror_out_batched")


def route(d, count=1, form="f64", env=None):
  """(batch mode, [route of every kind of call the batch makes]). count = 0: the single entry point."""
  env = env or {}
  if count == 0:
    return ("single",), [single_route(d, form, env)]
  if form == "f64" and USE_LANES not in env and count >= 2 and 2 * NB <= d < 4096 and d % NB == 0:
    group = max(1, min(count, GROUP, (4 << 30) // lane_bytes(d)))
    sizes = tuple(min(group, count - i) for i in range(0, count, group))
    routes = [lockstep_route(d, env)] if any(g > 1 for g in sizes) else []
    if 1 in sizes:
      routes.append(single_route(d, form, env))
    return ("lockstep", sizes), routes
  if count < 2:
    lanes = 1
  elif d >= 4096:
    lanes = 2 if int(env.get(PAIRS, 0) or 0) != 0 else 1
  else:
    lanes = min(count, LANES)
  if lanes > 1 and NO_LANES in env:
    lanes = 1
  return (("lanes", lanes) if lanes > 1 else ("serial",)), [single_route(d, form, env)]


@dataclasses.dataclass(frozen=True)
class Case:
  d: int
  count: int = 0            # 0: the single entry point; n: the batched one with n matrices (seeds seed .. seed + n - 1)
  form: str = "f64"         # or "product": alpha * float32 product, upper triangle NaN
  env: tuple = ()           # ((switch, value), ...): runs in a child process
  seed: int = 0
  bad: tuple = ()           # (matrix, pivot): that pivot of that matrix is exactly 0

  @property
  def envd(self):
    return dict(self.env)

  @property
  def seeds(self):
    return tuple(self.seed + i for i in range(max(self.count, 1)))


def route_of(c):
  return route(c.d, c.count, c.form, c.envd)


def _runs(seq):
  """a a b a -> a*3 b (kinds in the order of their first launch)"""
  count = {}
  for s in seq:
    count[s] = count.get(s, 0) + 1
  return " ".join(f"{s}*{n}" if n > 1 else s for s, n in count.items())


def describe(r):
  merge = " ".join(f"{s}:{'+'.join(k) or 'none'}" for s, k in r["merge"])
  return (f"copy({r['copy']}) steps({_runs(r['steps'])}) outer({_runs(r['outer']) or 'none'}{' delayed' if r['delay'] else ''}) "
          f"merge({merge or 'none'}) product({r['product']})")


def case_id(c):
  mode, routes = route_of(c)
  env = "".join(f"-{k[len('MI355Q_'):]}={v}" for k, v in c.env)
  bad = "".join(f"-zero_pivot{j}of{z}" for z, j in c.bad)
  head = f"d{c.d}-{c.form}-{'x'.join(str(x) for x in mode)}" + (f"-count{c.count}" if c.count else "") + env + bad
  return head + " = " + " | ".join(describe(r) for r in routes)


def features(c):
  """The elements of ALL_ROUTES one case covers."""
  mode, routes = route_of(c)
  f = {("batch",) + tuple(mode[:1])}
  if mode[0] == "lockstep":
    sizes = mode[1]
    f.add(("batch", "lockstep", "groups", len(sizes)))
    if 1 in sizes:
      f.add(("batch", "lockstep", "a last group of one takes the single route"))
  if mode[0] == "lanes":
    f.add(("batch", "lanes", "two large matrices in flight" if c.d >= 4096 else "pool"))
    if c.count > mode[1]:
      f.add(("batch", "lanes", "several matrices on one lane"))
  if mode[0] == "serial" and c.count >= 2:
    f.add(("batch", "serial", "large" if c.d >= 4096 else "pool switched off"))
  for r in routes:
    f.add(("copy", r["copy"]))
    f |= {("step", s) for s in r["steps"]}
    f |= {("outer", o) for o in r["outer"]}
    if r["delay"]:
      f.add(("outer", "strip+rest", "side stream delayed"))
    if r["side"] and any(s.startswith("generic") for s in r["steps"]):
      f.add(("step", "generic beside the look-ahead"))
    for s, kinds in r["merge"]:
      for kind in kinds:
        f.add(("merge", kind) if kind != "bf16x3" else ("merge", "bf16x3", "s>=1024" if s >= 1024 else "s<1024"))
      if len(kinds) > 1:
        f.add(("merge", "+".join(kinds[:1] + kinds[-1:])))
      if r["product"] == "ltl_bf16x3" and kinds and kinds[0] != "bf16x3":
        f.add(("merge", "FP64 level in a bf16x3 inverse", kinds[0]))
    f.add(("product", r["product"]))
    f.add(("mirror", r["mirror"]))
    if r["side"] and r["product"] == "gemm":
      f.add(("product", "gemm", "behind a look-ahead factorization"))
  for z, j in c.bad:
    r = routes[0]
    f.add(("info", r["steps"][j // NB].split(":")[0], "first column" if j % NB == 0 else "last column" if j % NB == NB - 1 or j == c.d - 1 else "inside"))
    if c.d % NB and j // NB == c.d // NB:
      f.add(("info", "ragged last block"))
    if j >= _outer_block(c.envd):
      f.add(("info", "second outer block"))
    if c.count >= 2:
      f.add(("info", "one failing matrix among exact ones"))
  return f


ALL_ROUTES = (
    {("batch", m) for m in ("single", "lockstep", "lanes", "serial")}
    | {("batch", "lockstep", "groups", n) for n in (1, 2)} | {("batch", "lockstep", "a last group of one takes the single route")}
    | {("batch", "lanes", w) for w in ("pool", "two large matrices in flight", "several matrices on one lane")}
    | {("batch", "serial", w) for w in ("large", "pool switched off")}
    | {("copy", c) for c in ("f64:full", "product:full", "f64:cols:caller+side", "product:cols:caller+side", "f64:batched")}
    | {("step", s) for s in ("fused:w>0:copy_panel", "fused:w>0:panel ready", "fused:w=0:panel ready", "asu:update", "asu:w=0",
                             "asu:m=0", "generic:gemm:nb=64", "generic:w=0:nb=64", "generic:m=0:nb=64", "generic:m=0:nb<64",
                             "lockstep:update", "lockstep:w=0", "lockstep:m=0", "generic beside the look-ahead")}
    | {("outer", o) for o in ("one gemm", "one gemm behind the side stream", "strip+rest", "one gemm over the group")}
    | {("outer", "strip+rest", "side stream delayed")}
    | {("merge", k) for k in ("batched", "loop:full", "loop:ragged", "batched+loop:ragged", "loop:full+loop:ragged")}
    | {("merge", "bf16x3", w) for w in ("s>=1024", "s<1024")}
    | {("merge", "FP64 level in a bf16x3 inverse", k) for k in ("batched", "loop:ragged")}
    | {("product", p) for p in ("ltl_bf16x3", "gemm", "gemm over the group")} | {("product", "gemm", "behind a look-ahead factorization")}
    | {("mirror", k) for k in ("mirror_lower_f32", "mirror_out_batched")}
    | {("info", k, w) for k, w in (("generic", "first column"), ("generic", "last column"), ("generic", "inside"),
                                   ("fused", "first column"), ("fused", "last column"), ("asu", "first column"),
                                   ("asu", "last column"), ("asu", "inside"), ("lockstep", "inside"))}
    | {("info", w) for w in ("ragged last block", "second outer block", "one failing matrix among exact ones")})

SIZES = (1, 7, 63, 64, 65, 100, 127, 128, 192, 448, 512, 576, 1000, 1024, 1088, 1100, 4096, 4160, 4200, 4608)


def _env(**kw):
  return tuple(("MI355Q_" + k, str(v)) for k, v in kw.items())


# (environment, single sizes, (d, count) batches, form of the batches)
ENV_TABLE = (
    (_env(NO_FUSED_STEP=1), (128, 576, 4608), (), "f64"),
    (_env(NO_FUSED_STEP=1, CHOL_ASU=0), (128, 576, 1088), (), "f64"),
    (_env(CHOL_OB=64), (256, 576), (), "f64"),
    (_env(CHOL_OB=128), (256, 576), (), "f64"),
    (_env(NO_LOOKAHEAD=1), (4608,), (), "f64"),
    (_env(NO_SPLIT_COPY=1), (4608,), (), "f64"),
    (_env(FUSED_MAX_M=0), (4608,), (), "f64"),
    (_env(FUSED_MAX_M=1000000), (4608,), (), "f64"),
    (_env(HINV_FP64=1), (4096, 4608), (), "f64"),
    (_env(HINV_SPLIT_MIN_S=128), (4608,), (), "f64"),
    (_env(DEBUG_SIDE_DELAY_US=3000), (4608,), (), "f64"),
    (_env(HINV_LANES=1), (), ((576, 3),), "f64"),
    (_env(HINV_NO_LANES=1), (), ((576, 3),), "f64"),
    (_env(HINV_PAIRS=1), (), ((4096, 3),), "f64"),
)

DEFAULT_CASES = (
    [Case(d, form=form) for d in SIZES for form in ("f64", "product")]
    # ---- batches, every matrix with a seed and a truth of its own
    + [Case(128, count=n) for n in (1, 2, 8, 33)] + [Case(576, count=3), Case(1088, count=2), Case(100, count=3), Case(4096, count=3)]
    + [Case(128, count=9, form="product"), Case(576, count=3, form="product"), Case(100, count=3, form="product"),
       Case(4096, count=3, form="product")]
    # ---- pivots that are exactly 0: info = j + 1
    # (a column of class 0 has nothing but its diagonal in L: its pivot IS H[j, j], and a zero there is the diag == 0 -> 1
    # substitution of the copy kernels, which the tolerance tests keep. So j % 3 != 0: never column 0, never column 63.)
    + [Case(100, bad=((0, 62),)), Case(100, bad=((0, 64),)), Case(200, bad=((0, 127),)), Case(200, bad=((0, 199),)),   # potf2_kernel
       Case(576, bad=((0, 64),)), Case(576, bad=((0, 191),)), Case(576, bad=((0, 512),)),                              # chol_step_kernel; asu m = 0
       Case(64, bad=((0, 62),)), Case(128, bad=((0, 127),)),                                                            # potf2_batched_kernel, one matrix
       Case(1100, bad=((0, 1099),)), Case(1100, bad=((0, 512),)),                                                       # ragged block, second outer block
       Case(576, count=3, bad=((1, 530),))])                                                                            # lock step
ENV_CASES = [Case(d, env=env) for env, sizes, _, _ in ENV_TABLE for d in sizes] + \
            [Case(d, count=n, form=form, env=env) for env, _, batches, form in ENV_TABLE for d, n in batches] + \
            [Case(d, count=3, form="product", env=_env(**{k: 1})) for k, d in (("HINV_LANES", 576), ("HINV_NO_LANES", 576), ("HINV_PAIRS", 4096))]
CASES = DEFAULT_CASES + ENV_CASES
DATA = sorted({(c.d, s) for c in CASES for s in c.seeds})


def test_case_list_reaches_every_route():
  reached = set()
  for c in CASES:
    reached |= features(c)
  assert not ALL_ROUTES - reached, sorted(ALL_ROUTES - reached, key=str)
  assert not reached - ALL_ROUTES, sorted(reached - ALL_ROUTES, key=str)      # the list above names everything route() can tell apart here
  assert len({case_id(c) for c in CASES}) == len(CASES)


def test_routes_of_the_sizes_the_issue_names():
  """The restatement against what csrc/gptq.hip says in words about a few sizes."""
  r = single_route(576)
  assert r["steps"] == ("fused:w>0:copy_panel",) + ("fused:w>0:panel ready",) * 6 + ("fused:w=0:panel ready", "asu:m=0")
  assert r["outer"] == ("one gemm",) and r["product"] == "gemm" and r["copy"] == "f64:full"
  assert r["merge"] == ((64, ("batched",)), (128, ("batched",)), (256, ("loop:full",)), (512, ("loop:ragged",)))
  r = single_route(100)
  assert r["steps"] == ("generic:gemm:nb=64", "generic:m=0:nb<64") and r["merge"] == ((64, ("loop:ragged",)),)
  r = single_route(4608)
  assert r["copy"] == "f64:cols:caller+side" and r["product"] == "ltl_bf16x3"
  assert r["outer"] == ("strip+rest",) * 4 + ("one gemm behind the side stream",) * 4
  assert r["steps"][:40] == (("asu:update",) * 7 + ("asu:w=0",)) * 5          # 2048 rows and more below the step
  assert r["steps"][40:48] == ("fused:w>0:copy_panel",) + ("fused:w>0:panel ready",) * 6 + ("fused:w=0:panel ready",)
  assert r["steps"][-1] == "asu:m=0"
  assert dict(r["merge"])[1024] == ("bf16x3",) and dict(r["merge"])[2048] == ("bf16x3",) and dict(r["merge"])[4096] == ("loop:ragged",)
  assert dict(r["merge"])[512] == ("batched",)
  r = single_route(4160)
  assert r["product"] == "gemm" and r["side"] and all(k != ("bf16x3",) for _, k in r["merge"])
  assert all(s.startswith("generic") for s in single_route(4200)["steps"]) and single_route(4200)["side"]
  assert set(single_route(256, env=dict(_env(CHOL_OB=64)))["steps"]) == {"asu:w=0", "asu:m=0"}
  assert single_route(256, env=dict(_env(CHOL_OB=128)))["steps"] == ("fused:w>0:copy_panel", "fused:w=0:panel ready", "fused:w>0:copy_panel", "asu:m=0")
  assert route(128, 33)[0] == ("lockstep", (32, 1)) and route(100, 3)[0] == ("lanes", 3) and route(4096, 3)[0] == ("serial",)
  assert route(576, 3, "product")[0] == ("lanes", 3) and route(4096, 3, "product", dict(_env(HINV_PAIRS=1)))[0] == ("lanes", 2)
  assert route(128, 1)[0] == ("serial",)


def _tiles(mask):
  d = mask.shape[0]
  n = -(-d // NB)
  pad = np.zeros((n * NB, n * NB), bool)
  pad[:d, :d] = mask
  return pad.reshape(n, NB, n, NB).any(axis=(1, 3))


@pytest.mark.parametrize("d,seed", DATA, ids=[f"d{d}-seed{s}" for d, s in DATA])
def test_case_is_exact(d, seed):
  s, k = X.factors(d, seed)
  l, linv, h, hinv = X.dense(d, seed)
  rows, cols = np.arange(d)[:, None], np.arange(d)[None, :]
  allowed = (cols < rows) & (cols % 3 < rows % 3)
  assert not s[~allowed].any() and set(np.unique(np.abs(s))) <= {0, 1, 2, X.ODD_MAGNITUDE}
  sf = s.astype(np.float64)
  assert not ((np.eye(d) - sf - linv * np.ldexp(1.0, k)[:, None]) @ sf).any()       # -S^2 S: S^3 = 0
  assert np.array_equal(np.linalg.cholesky(h), l)
  assert np.array_equal(l @ linv, np.eye(d))
  major = X.majorants(d, seed)
  units = [float(mj.max()) / X.GRID for mj in major]
  assert max(units) < X.LIMIT, units
  assert np.array_equal(hinv / X.GRID, np.rint(hinv / X.GRID)) and np.array_equal(h, np.rint(h))
  assert np.array_equal(hinv.astype(np.float32).astype(np.float64), hinv) and np.array_equal(hinv, hinv.T)
  for alpha in (4.0, 0.25):
    assert np.array_equal((h / alpha).astype(np.float32).astype(np.float64) * alpha, h)
  # every tile the class rule allows a non-zero in holds one
  lower = cols <= rows
  may = _tiles(allowed | (rows == cols))
  assert np.array_equal(_tiles(l != 0), may) and np.array_equal(_tiles(linv != 0), may)
  assert np.array_equal(_tiles((hinv != 0) & lower), _tiles((major[0] != 0) & lower))       # (where no product exists, none can)
  full = d // NB
  assert _tiles((hinv != 0) & lower)[:full, :full][np.tril_indices(full)].all()
  if d >= X.ODD_MIN_D:
    assert (np.abs(s) == X.ODD_MAGNITUDE).sum() == X.ODD and (np.abs(linv) * np.ldexp(1.0, k)[:, None] >= X.ODD_MAGNITUDE - 16).sum() == X.ODD  # (S^2 may add a few units there)
  if d == 4608:
    # the odd magnitudes reach the bf16x3 merges: below the diagonal blocks of the 1024 and the 2048 level
    odd = np.argwhere(np.abs(s) == X.ODD_MAGNITUDE)
    assert any(1024 <= i < 2048 and j < 1024 for i, j in odd) and any(2048 <= i < 4096 and j < 2048 for i, j in odd)
    assert any(i >= 4096 for i, _ in odd)


def test_zero_pivot_cases_fail_where_they_say():
  for c in CASES:
    for z, j in c.bad:
      _, _, h, _ = X.dense(c.d, c.seeds[z])
      h = X.zero_pivot(h.copy(), c.d, c.seeds[z], j)
      l = X.dense(c.d, c.seeds[z])[0]
      assert j % 3 and h[j, j] != 0.0            # else the copy kernels put a 1 there
      if j:
        assert np.array_equal(np.linalg.cholesky(h[:j, :j]), l[:j, :j])
      assert h[j, j] - (l[j, :j] ** 2).sum() == 0.0


# ---------------------------------------------------------------------------------------------- argument checks ---
@functools.lru_cache(maxsize=None)
def library():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


def test_workspace_query_matches_the_restatement():
  lib = library()
  for d in (-1, 0):
    assert lib.mi355q_gptq_hinv_workspace_bytes(d) == 0
  for d in (1, 64, 100, 576, 4608):
    assert lib.mi355q_gptq_hinv_workspace_bytes(d) == workspace_bytes(d)
    assert lib.mi355q_gptq_hinv_batched_workspace_bytes(1, d) == lane_bytes(d)
    assert lib.mi355q_gptq_hinv_from_product_batched_workspace_bytes(1, d) == lane_bytes(d)
  assert lib.mi355q_gptq_hinv_batched_workspace_bytes(0, 64) == 0 and lib.mi355q_gptq_hinv_batched_workspace_bytes(3, 0) == 0


def test_entries_refuse_bad_arguments_before_they_launch(monkeypatch):
  """Host memory stands in for every buffer: each of these calls returns before it touches a device."""
  for name in SWITCHES:
    monkeypatch.delenv(name, raising=False)
  lib = library()
  err = lib.mi355q_last_error
  d = 64
  need = workspace_bytes(d)
  buf = ctypes.create_string_buffer(b"\x5a" * 4096, 4096)
  base = ctypes.addressof(buf)
  P = ctypes.c_void_p

  def single(fn, product, **kw):
    a = dict(h=base, d=d, out=base, info=base, ws=base, ws_bytes=need)
    a.update(kw)
    head = (a["h"], a["d"], 1.0, 0.0) if product else (a["h"], a["d"], 0.0)
    return fn(*head, a["out"], a["info"], a["ws"], a["ws_bytes"], None)

  def batched(fn, product, **kw):
    a = dict(table=[base], count=1, d=d, outs=[base], info=base, ws=base, ws_bytes=lane_bytes(d), alphas=True)
    a.update(kw)
    n = max(a["count"], 1)
    table = None if a["table"] is None else (P * n)(*a["table"])
    outs = None if a["outs"] is None else (P * n)(*a["outs"])
    alphas = (ctypes.c_double * n)(*([1.0] * n)) if a["alphas"] else None
    head = (table, alphas, a["count"], a["d"], 0.0) if product else (table, a["count"], a["d"], 0.0)
    return fn(*head, outs, a["info"], a["ws"], a["ws_bytes"], None)

  for fn, product in ((lib.mi355q_gptq_hinv_f64, False), (lib.mi355q_gptq_hinv_from_product_f32, True)):
    assert single(fn, product, d=-1) == -1 and b"negative shape" in err()
    assert single(fn, product, h=None, d=-1) == -1 and b"negative shape" in err()
    for name in ("h", "out", "info"):
      assert single(fn, product, **{name: None}) == -1 and b"null pointer" in err()
    assert single(fn, product, d=46001, ws_bytes=workspace_bytes(46001)) == -3 and b"d too large" in err()
    assert single(fn, product, ws=None) == -1 and b"workspace too small" in err()
    assert single(fn, product, ws_bytes=need - 1) == -1 and f"need {need} bytes".encode() in err()
    assert single(fn, product, d=0, h=None, out=None, info=None, ws=None, ws_bytes=0) == 0 and err() == b""
  for fn, product in ((lib.mi355q_gptq_hinv_f64_batched, False), (lib.mi355q_gptq_hinv_from_product_f32_batched, True)):
    assert batched(fn, product, count=-1) == -1 and b"negative shape" in err()
    assert batched(fn, product, d=-1) == -1 and b"negative shape" in err()
    for kw in (dict(table=None), dict(outs=None), dict(info=None), dict(table=[None]), dict(outs=[None])):
      assert batched(fn, product, **kw) == -1 and b"null pointer" in err(), kw
    if product:
      assert batched(fn, product, alphas=False) == -1 and b"null pointer" in err()
    assert batched(fn, product, d=46001, ws_bytes=lane_bytes(46001)) == -3 and b"d too large" in err()
    assert batched(fn, product, ws=None) == -1 and b"workspace too small" in err()
    assert batched(fn, product, ws_bytes=lane_bytes(d) - 1) == -1 and f"need {lane_bytes(d)} bytes".encode() in err()
    # three matrices in lock step (float64) or on three lanes (products): three slices
    three = dict(table=[base] * 3, outs=[base] * 3, count=3, d=128)
    assert batched(fn, product, ws_bytes=3 * lane_bytes(128) - 1, **three) == -1 and f"need {3 * lane_bytes(128)} bytes".encode() in err()
    for empty in (dict(count=0), dict(d=0)):
      assert batched(fn, product, table=None, outs=None, info=None, ws=None, ws_bytes=0, alphas=False, **empty) == 0 and err() == b""
  assert buf.raw == b"\x5a" * 4096
