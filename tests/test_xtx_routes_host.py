"""Which kernels the Hessian product X^T X runs (csrc/gptq.hip: xtx_product; csrc/xtx_bf16x3.hip: xtx_bf16x3, xtx_splits,
xtx_bf16x3_usable; csrc/xtx_f16x2.hip: xtx_f16x2, xtx2_splits, xtx_f16x2_usable), and that the exact cases of
xtx_exact_cases.py are what they claim to be. No GPU.

route() restates the host's choices: the family (FP32 GEMM, bf16x3, f16x2) and, per slab of 16384 tokens, kt, splits,
kt_per_split, plain tile list or 8 x 8 XCD patches with the side of the patch grid, the kernel (narrow, wide, deep<0|1|2>,
f16x2<2|3|4>, f16x2_wide) and whether the slab goes through the reduce kernel (with its accumulate flag) or writes
direct (with `accumulate`). features() turns the routes of a case into elements of REQUIRED; the case list of the GPU file
(CASES, here so that it can be checked without a GPU) reaches every one of them, and every case carries its route in its id.

A case is a sequence of calls of mi355q_gptq_xtx_accum_f32 (call i has calls[i] tokens and the seed seed + i), onto an
initial integer product where `initial`. Per case: the 2^24-unit bound over the whole sequence; per planes* call: the
planes of every live element are exactly s a, s 2^-9, s 2^-18 (or a 2^k and 2^(k - 12) after the column scaling), all
columns are distinct, the model is a whole number of quanta, converts to float32 and back unchanged and differs from the
exact product; and one mutation of the model at a time -- planes 2 and 3 of operand B swapped, a cross term left out, a k
tile with a live token left out, a split's partial left out, the second slab not accumulated, the initial product not added, a
128 x 128 tile taken from (tj, ti) of the non-symmetric product of operand A shifted by one tile -- changes an entry.

Out of scope: MI355Q_XTX_PROBE gives wrong results by design (timing probes), and MI355Q_XTX_SPLIT_BELOW is a compile-time
macro; neither has a case."""
import dataclasses
import functools

import numpy as np
import pytest

import xtx_exact_cases as X

F16X2, BF16X3, FP32_MFMA, NARROW, DEEP, ALT, DEPTH = (
    "MI355Q_XTX_F16X2", "MI355Q_XTX_BF16X3", "MI355Q_XTX_FP32_MFMA", "MI355Q_XTX_NARROW", "MI355Q_XTX_DEEP", "MI355Q_XTX_ALT",
    "MI355Q_XTX_DEPTH")
SWITCHES = (F16X2, BF16X3, FP32_MFMA, NARROW, DEEP, ALT, DEPTH, "MI355Q_XTX_PROBE")
TILE, BK, SLAB, SUPER = 128, 16, 16384, 8


def _atoi(s):
  digits = ""
  for ch in s.strip():
    if ch.isdigit() or (ch in "+-" and not digits):
      digits += ch
    else:
      break
  try:
    return int(digits)
  except ValueError:
    return 0


def family(n, d, env):
  """xtx_product: f16x2 where usable, else bf16x3 where usable, else the FP32 GEMM."""
  eligible = d % TILE == 0 and d >= 256 and n >= 1024 and FP32_MFMA not in env
  fast = env.get(F16X2)
  if eligible and fast is not None and fast != "" and fast[0] != "0" and BF16X3 not in env:
    return "f16x2"
  return "bf16x3" if eligible else "fp32"


def route(n, d, env=None, accumulate=False):
  """dict(family, slabs); a slab: k0, ks, kt, splits, kt_per_split, patches, side, kernel, out ('reduce' or 'direct'), accumulate."""
  env = env or {}
  fam = family(n, d, env)
  if fam == "fp32":
    return dict(family=fam, accumulate=accumulate, slabs=())
  tiles = d // TILE
  slabs = []
  for k0 in range(0, n, SLAB):
    ks = min(SLAB, n - k0)
    if fam == "f16x2":
      kt = (ks + 2 * BK - 1) // (2 * BK) * 2
      splits = X.splits_of(d, kt)
      per = ((kt // 2 + splits - 1) // splits) * 2
    else:
      kt = (ks + BK - 1) // BK
      splits = X.splits_of(d, kt)
      per = (kt + splits - 1) // splits
    patches = tiles >= 4 * SUPER
    wide = env.get(NARROW, "") == "" and patches and d % (2 * TILE) == 0 and splits == 1
    if fam == "f16x2":
      depth = min(4, max(2, _atoi(env[DEPTH]))) if DEPTH in env else 2
      kernel = "f16x2_wide" if wide else f"f16x2<{depth}>"
    elif not wide:
      kernel = "narrow"
    elif DEEP in env and _atoi(env[DEEP]) == 0:
      kernel = "wide"
    else:
      alt = _atoi(env[ALT]) if ALT in env else 1
      kernel = f"deep<{alt if alt in (1, 2) else 0}>"
    slabs.append(dict(k0=k0, ks=ks, kt=kt, splits=splits, kt_per_split=per, patches=patches,
                      side=(tiles + SUPER - 1) // SUPER if patches else 0, kernel=kernel,
                      out="reduce" if splits > 1 else "direct", accumulate=k0 > 0 or accumulate))
  return dict(family=fam, accumulate=accumulate, slabs=tuple(slabs))


@dataclasses.dataclass(frozen=True)
class Case:
  d: int
  calls: tuple              # tokens of every call of mi355q_gptq_xtx_accum_f32, in order
  kind: str                 # dense, planes3 or planes2
  env: tuple = ()           # ((switch, value), ...); anything but () and F16X2 = 1 alone runs in a child process
  initial: bool = False     # the first call accumulates onto X.initial_product(d, seed)
  seed: int = 0

  @property
  def envd(self):
    return dict(self.env)

  @property
  def tokens(self):
    return sum(self.calls)

  @property
  def in_process(self):
    return self.env in ((), ((F16X2, "1"),))


def routes_of(c):
  return [route(n, c.d, c.envd, c.initial or i > 0) for i, n in enumerate(c.calls)]


def describe(r):
  if r["family"] == "fp32":
    return "fp32 gemm" + (" accumulate" if r["accumulate"] else "")
  out = []
  for s in r["slabs"]:
    grid = f"patches {s['side']}x{s['side']}" if s["patches"] else "plain"
    out.append(f"{s['kernel']} kt{s['kt']} splits{s['splits']}x{s['kt_per_split']} {grid} {s['out']}{' accumulate' if s['accumulate'] else ''}")
  return r["family"] + "(" + "; ".join(out) + ")"


def case_id(c):
  env = "".join(f"-{k[len('MI355Q_XTX_'):]}={v}" for k, v in c.env)
  head = f"d{c.d}-n{'+'.join(str(n) for n in c.calls)}-{c.kind}{'-initial' if c.initial else ''}{env}"
  return head + " = " + " | ".join(describe(r) for r in routes_of(c))


def features(c):
  """The elements of REQUIRED one case covers."""
  f = set()
  routes = routes_of(c)
  env = c.envd
  for n, r in zip(c.calls, routes):
    fam = r["family"]
    if fam == "fp32":
      f.add(("fp32", "d % 128" if c.d % TILE else "d < 256" if c.d < 256 else "n < 1024" if n < 1024 else "FP32_MFMA"))
      continue
    if F16X2 in env and BF16X3 in env and fam == "bf16x3":
      f.add(("bf16x3", "BF16X3 = 1 beside F16X2 = 1"))
    slabs = r["slabs"]
    for s in slabs:
      k, grid = s["kernel"], "patches" if s["patches"] else "plain"
      f.add((fam, k, grid, c.kind.rstrip("23")))
      if s["patches"]:
        f.add((fam, k, "patch grid side", s["side"]))
        if (c.d // TILE) % SUPER:
          f.add((fam, k, "ragged last patch"))
        if k != "f16x2_wide" and k.startswith("f16x2"):
          f.add((fam, k, "patches", "depth"))
      if grid == "plain" and s["k0"] == 0:
        if s["splits"] == 1:
          f.add((fam, k, "splits = 1"))
        else:
          last = s["kt"] - (s["splits"] - 1) * s["kt_per_split"]
          f.add((fam, k, "equal splits" if last == s["kt_per_split"] else "ragged last split"))
          if s["splits"] == 16:
            f.add((fam, k, "16 splits"))
        if s["ks"] % BK:
          f.add((fam, k, "ragged last k tile"))
      if k in ("wide", "deep<0>", "deep<1>", "deep<2>") and len(slabs) == 1:
        f.add((fam, k, "even kt" if s["kt"] % 2 == 0 else "odd kt"))
      if k == "f16x2_wide" and len(slabs) == 1:
        f.add((fam, k, "even pairs" if (s["kt"] // 2) % 2 == 0 else "odd pairs"))
      if s["k0"] == 0 and r["accumulate"] and len(c.calls) == 1:
        f.add((fam, "onto an initial product", s["out"]))
    if len(slabs) == 2:
      first, second = slabs
      f.add((fam, second["kernel"], "second slab", f"{first['out']} then {second['out']} accumulate"))
      if c.kind == "planes2":
        f.add((fam, second["kernel"], "second slab with other column maxima"))
  fams = [r["family"] for r in routes]
  if len(fams) == 3 and fams[1] == "fp32" and fams[0] == fams[2] != "fp32" and routes[2]["slabs"][0]["splits"] > 1:
    f.add((fams[0], "split kernel, fp32 gemm, split kernel with splits > 1"))
  return f


_WIDE = ("wide", "deep<0>", "deep<1>", "deep<2>")
REQUIRED = (
    {("fp32", w) for w in ("d % 128", "d < 256", "n < 1024", "FP32_MFMA")}
    # ---- narrow kernels on the plain list, both families
    | {(fam, k, w) for fam, k in (("bf16x3", "narrow"), ("f16x2", "f16x2<2>"))
       for w in ("splits = 1", "equal splits", "ragged last split", "ragged last k tile", "16 splits")}
    | {(fam, k, "second slab", w) for fam, k in (("bf16x3", "narrow"), ("f16x2", "f16x2<2>"))
       for w in ("reduce then direct accumulate", "reduce then reduce accumulate")}
    # ---- narrow kernels on patches: 33 tiles (a ragged last patch) and d = 4096 under MI355Q_XTX_NARROW
    | {(fam, k, "ragged last patch") for fam, k in (("bf16x3", "narrow"), ("f16x2", "f16x2<2>"))}
    | {(fam, k, "patch grid side", side) for fam, k in (("bf16x3", "narrow"), ("f16x2", "f16x2<2>")) for side in (4, 5)}
    # ---- 128 x 256 tiles
    | {("bf16x3", k, w) for k in _WIDE for w in ("even kt", "odd kt")}
    | {("bf16x3", k, "second slab", "direct then direct accumulate") for k in _WIDE}
    | {("bf16x3", k, "patch grid side", 4) for k in _WIDE} | {("bf16x3", "deep<1>", "patch grid side", 5)}
    | {("bf16x3", "deep<1>", "ragged last patch")}
    | {("f16x2", "f16x2_wide", w) for w in ("even pairs", "odd pairs")}
    | {("f16x2", "f16x2_wide", "second slab", "direct then direct accumulate")}
    # ---- the deeper rings of the narrow f16x2 kernel: one split-K shape, one patch shape
    | {("f16x2", k, w) for k in ("f16x2<3>", "f16x2<4>") for w in ("ragged last split", "ragged last patch")}
    | {("f16x2", "f16x2<2>", "second slab with other column maxima")}
    | {("bf16x3", "BF16X3 = 1 beside F16X2 = 1")}
    # ---- accumulating calls
    | {(fam, "onto an initial product", out) for fam in ("bf16x3", "f16x2") for out in ("direct", "reduce")}
    | {(fam, "split kernel, fp32 gemm, split kernel with splits > 1") for fam in ("bf16x3", "f16x2")}
    # ---- every split kernel on both kinds of data
    | {("bf16x3", "narrow", grid, kind) for grid in ("plain", "patches") for kind in ("dense", "planes")}
    | {("bf16x3", k, "patches", kind) for k in _WIDE for kind in ("dense", "planes")}
    | {("f16x2", "f16x2<2>", grid, kind) for grid in ("plain", "patches") for kind in ("dense", "planes")}
    | {("f16x2", k, grid, kind) for k in ("f16x2<3>", "f16x2<4>") for grid in ("plain", "patches") for kind in ("dense", "planes")}
    | {("f16x2", "f16x2_wide", "patches", kind) for kind in ("dense", "planes")})


def _env(**kw):
  return tuple(("MI355Q_XTX_" + k, str(v)) for k, v in kw.items())


def _both(d, n, env=(), initial=False):
  """A split-kernel shape on the dense kind and on the planes kind of its family."""
  planes = "planes2" if family(n, d, dict(env)) == "f16x2" else "planes3"
  return [Case(d, (n,), "dense", env, initial), Case(d, (n,), planes, env, initial)]


FAST = _env(F16X2=1)
# the shapes of the narrow kernels: splits = 1, equal splits, a ragged last split and k tile, 16 splits, two slabs (reduce then
# direct, reduce then reduce), 33 tiles on patches with an odd, ragged k-tile count
NARROW_SHAPES = ((256, 1024), (256, 4096), (256, 4100), (512, 16384), (256, SLAB + 1040), (256, SLAB + 4096), (4224, 1030))
WIDE_SHAPES = ((4096, 1024), (4096, 1040), (4096, SLAB + 48))

DEFAULT_CASES = (
    # ---- the FP32 GEMM: thresholds and plumbing (dense: the model is the exact integer product)
    [Case(320, (1100,), "dense"), Case(128, (1100,), "dense"), Case(256, (1023,), "dense")]
    + [c for d, n in NARROW_SHAPES for c in _both(d, n)]
    + [c for d, n in WIDE_SHAPES + ((4608, 1024), (4608, 1040)) for c in _both(d, n)]
    + [c for d, n in ((256, 1024), (256, 4096)) for c in _both(d, n, initial=True)]
    + [Case(256, (1024, 500, 4096), "dense")]
    # ---- MI355Q_XTX_F16X2 = 1 is read per call
    + [c for d, n in NARROW_SHAPES for c in _both(d, n, FAST)]
    + [c for d, n in WIDE_SHAPES for c in _both(d, n, FAST)]
    + [c for d, n in ((256, 1024), (256, 4096)) for c in _both(d, n, FAST, initial=True)]
    + [Case(256, (1024, 500, 4096), "dense", FAST)])
ENV_CASES = (
    [Case(256, (1024,), "dense", _env(FP32_MFMA=1))]
    + _both(4096, 1040, _env(NARROW=1)) + _both(4096, 1024, _env(NARROW=1))
    + [c for env in (_env(DEEP=0), _env(ALT=0), _env(ALT=2)) for d, n in WIDE_SHAPES for c in _both(d, n, env)]
    + _both(4096, 1040, _env(F16X2=1, NARROW=1))
    + [c for depth in (3, 4) for d, n in ((256, 4100), (4224, 1030)) for c in _both(d, n, _env(F16X2=1, DEPTH=depth))]
    + _both(256, 4096, _env(F16X2=1, BF16X3=1)))
CASES = DEFAULT_CASES + ENV_CASES
# where the source states that routes add the same products in the same order (xtx_bf16x3.hip: narrow, wide, deep<0|1|2>
# at d = 4096): equal bits on one dense full-mantissa tensor, every environment against the default one
SAME_BITS_SHAPE = (4096, 1040)
SAME_BITS_ENVS = (_env(NARROW=1), _env(DEEP=0), _env(ALT=0), _env(ALT=2))
PLANES_CALLS = sorted({(c.calls[0], c.d, c.seed, c.kind, c.initial) for c in CASES if c.kind != "dense"})


def test_case_list_reaches_every_route():
  reached = set()
  for c in CASES:
    assert all(c.in_process for c in DEFAULT_CASES) and not any(c.in_process for c in ENV_CASES)
    reached |= features(c)
  assert not REQUIRED - reached, sorted(REQUIRED - reached, key=str)
  assert len({case_id(c) for c in CASES}) == len(CASES)
  for env in SAME_BITS_ENVS:
    assert any(c.env == env for c in ENV_CASES)
  kernels = {route(SAME_BITS_SHAPE[1], SAME_BITS_SHAPE[0], dict(env))["slabs"][0]["kernel"] for env in ((),) + SAME_BITS_ENVS}
  assert kernels == {"narrow", "wide", "deep<0>", "deep<1>", "deep<2>"}
  assert {route(SAME_BITS_SHAPE[1], SAME_BITS_SHAPE[0], dict(env))["slabs"][0]["splits"] for env in ((),) + SAME_BITS_ENVS} == {1}


def test_routes_of_the_shapes_the_issue_names():
  """The restatement against what the sources say in words about a few shapes."""
  r = route(1024, 256)
  assert r["family"] == "bf16x3" and describe(r) == "bf16x3(narrow kt64 splits1x64 plain direct)"
  assert describe(route(4096, 256)) == "bf16x3(narrow kt256 splits4x64 plain reduce)"
  assert describe(route(4100, 256)) == "bf16x3(narrow kt257 splits4x65 plain reduce)"
  assert describe(route(4100, 256, dict(FAST))) == "f16x2(f16x2<2> kt258 splits4x66 plain reduce)"
  assert describe(route(16384, 512)) == "bf16x3(narrow kt1024 splits16x64 plain reduce)"
  assert describe(route(SLAB + 1040, 256)) == "bf16x3(narrow kt1024 splits16x64 plain reduce; narrow kt65 splits1x65 plain direct accumulate)"
  assert describe(route(SLAB + 4096, 256, accumulate=True)).count("reduce accumulate") == 2
  assert describe(route(1030, 4224)) == "bf16x3(narrow kt65 splits1x65 patches 5x5 direct)"
  assert describe(route(1040, 4096)) == "bf16x3(deep<1> kt65 splits1x65 patches 4x4 direct)"
  assert describe(route(1040, 4608)) == "bf16x3(deep<1> kt65 splits1x65 patches 5x5 direct)"
  assert route(1040, 4096, dict(_env(NARROW=1)))["slabs"][0]["kernel"] == "narrow"
  assert route(1040, 4096, dict(_env(DEEP=0)))["slabs"][0]["kernel"] == "wide"
  assert route(1040, 4096, dict(_env(ALT=0)))["slabs"][0]["kernel"] == "deep<0>"
  assert route(1040, 4096, dict(_env(ALT=2)))["slabs"][0]["kernel"] == "deep<2>"
  assert route(1040, 4096, dict(_env(ALT=7)))["slabs"][0]["kernel"] == "deep<0>"
  assert route(1040, 4096, dict(FAST))["slabs"][0]["kernel"] == "f16x2_wide" and route(1040, 4096, dict(FAST))["slabs"][0]["kt"] == 66
  assert route(4100, 256, dict(_env(F16X2=1, DEPTH=9)))["slabs"][0]["kernel"] == "f16x2<4>"
  assert route(4096, 256, dict(_env(F16X2=1, BF16X3=1)))["family"] == "bf16x3" and route(4096, 256, dict(_env(F16X2=0)))["family"] == "bf16x3"
  for n, d, env in ((1100, 320, {}), (1100, 128, {}), (1023, 256, {}), (1024, 256, dict(_env(FP32_MFMA=1))), (500, 256, dict(FAST))):
    assert route(n, d, env)["family"] == "fp32"
  # the layout xtx_exact_cases.py puts its live tokens by is the route's
  for c in CASES:
    for n, r in zip(c.calls, routes_of(c)):
      if r["family"] != "fp32":
        kind = "planes2" if r["family"] == "f16x2" else "planes3"
        assert c.kind in ("dense", kind)
        assert X.slabs_of(n, c.d, kind) == [(s["k0"], s["ks"], s["kt"], s["splits"], s["kt_per_split"]) for s in r["slabs"]]
      else:
        assert c.kind == "dense"       # the FP32 GEMM multiplies the values themselves: only integers are exact there


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_meets_the_bound(c):
  """sum of |products| over all tokens of all calls, plus the initial product, in quanta: below 2^24."""
  units = sum(X.majorant_units(n, c.d, c.seed + i, c.kind, c.initial and i == 0) for i, n in enumerate(c.calls))
  assert units < X.LIMIT, units
  if c.kind == "planes3":
    assert len(X.boundary_tokens(c.calls[0], c.d, c.seed, c.kind)) <= X.LIVE3 == 15 and len(c.calls) == 1
    assert 15 * (2 + 2.0 ** -9 + 2.0 ** -18) ** 2 + X.INITIAL_MAX < 64 < 16 * (2 + 2.0 ** -9 + 2.0 ** -18) ** 2


def test_dense_data_is_what_the_bound_assumes():
  """Integers in [-3, 3] but for the special entries (distinct tokens, distinct columns); 257 needs the second bf16 plane
  and no third, and fits one float16 plane; the analytic majorant holds against |X|^T |X|."""
  for n, d, seed in ((1024, 256, 0), (1100, 320, 0), (4100, 256, 1), (500, 256, 1)):
    x = X.dense_x(n, d, seed)
    special = X.special_entries(n, d, seed)
    mask = np.zeros(x.shape, bool)
    for t, col, v in special:
      assert x[t, col] == v and abs(v) == X.SPECIAL_MAGNITUDE
      mask[t, col] = True
    assert len(special) == X.SPECIALS and np.abs(x[~mask]).max() == X.DENSE_MAX and np.array_equal(x, np.rint(x))
    assert {int(v) for v in np.unique(x[~mask])} == set(range(-3, 4))
    a = np.abs(x.astype(np.float64))
    assert (a.T @ a).max() <= X.majorant_units(n, d, seed, "dense")
    p1, p2, p3 = X.split_bf16x3(x)
    assert not p3.any() and np.array_equal(p2 != 0, mask) and np.array_equal(p1 + p2, x)
    _, (h1, h2) = X.split_f16x2(x)
    assert not h2.any()
    prod = x.astype(np.float64).T @ x.astype(np.float64)
    assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)
  p0 = X.initial_product(256, 0)
  assert np.array_equal(p0, p0.T) and np.abs(p0).max() == X.INITIAL_MAX and np.array_equal(p0, np.rint(p0))


def _live_layout(n, d, seed, kind):
  """Per live token: (slab, k tile within the slab, split)."""
  tokens, _ = X.live_rows(n, d, seed, kind)
  slabs = X.slabs_of(n, d, kind)
  out = []
  for t in tokens:
    z = t // SLAB
    kt = (t - slabs[z][0]) // BK
    out.append((z, kt, kt // slabs[z][4]))
  return out


def structured_model(n, d, seed, kind, initial, cols, mutation=None, shift_a=False):
  """The model of a planes* call on its leading cols x cols block, built the way the kernels work -- slab by slab, split by
  split, k tile by k tile -- so that single steps can be left out or changed."""
  tokens, values = X.live_rows(n, d, seed, kind)
  layout = _live_layout(n, d, seed, kind)
  pairs = list(X.BF16_PAIRS if kind == "planes3" else X.F16_PAIRS)
  if mutation == "a cross term left out":
    pairs.remove((1, 0))
  middle = layout[len(layout) // 2]
  with_splits = [l for l in layout if X.slabs_of(n, d, kind)[l[0]][3] > 1]
  total = np.zeros((cols, cols))
  if initial and mutation != "the initial product not added":
    total += X.initial_product(d, seed)[:cols, :cols]
  tok = np.array(tokens)
  for z, (k0, _, _, _, _) in enumerate(X.slabs_of(n, d, kind)):
    if z == 1 and mutation == "the second slab not accumulated":
      continue
    sel = np.nonzero((tok >= k0) & (tok < k0 + SLAB))[0]
    if not len(sel):
      continue
    rows = values[sel]
    if kind == "planes3":
      planes, back = X.split_bf16x3(rows), 1.0
    else:
      e, planes = X.split_f16x2(rows)
      back = np.ldexp(1.0, -(e[:cols, None] + e[None, :cols]))
    pa = [np.roll(p, -TILE, axis=1)[:, :cols].astype(np.float64) for p in planes] if shift_a else [p[:, :cols].astype(np.float64) for p in planes]
    if shift_a and kind == "planes2":
      back = np.ldexp(1.0, -(np.roll(e, -TILE)[:cols, None] + e[None, :cols]))
    pb = [p[:, :cols].astype(np.float64) for p in planes]
    if mutation == "planes 2 and 3 of operand B swapped":
      pb = [pb[0], pb[2], pb[1]] if kind == "planes3" else [pb[1], pb[0]]
    for r, i in enumerate(sel):
      if mutation == "a k tile left out" and layout[i][:2] == middle[:2]:
        continue
      if mutation == "a split's partial left out" and (layout[i][0], layout[i][2]) == (with_splits[0][0], with_splits[0][2]):
        continue
      total += sum(np.outer(pa[p][r], pb[q][r]) for p, q in pairs) * back
  return total


MUTATIONS = ("planes 2 and 3 of operand B swapped", "a cross term left out", "a k tile left out", "a split's partial left out",
             "the second slab not accumulated", "the initial product not added", "a tile taken from (tj, ti)")


@pytest.mark.parametrize("n,d,seed,kind,initial", PLANES_CALLS, ids=[f"n{n}-d{d}-seed{s}-{k}{'-initial' if i else ''}" for n, d, s, k, i in PLANES_CALLS])
def test_planes_call_is_exact_and_sensitive(n, d, seed, kind, initial):
  q = X.QUANTUM[kind]
  tokens, values = X.live_rows(n, d, seed, kind)
  cap = X.LIVE3 if kind == "planes3" else X.LIVE2
  assert 0 < len(tokens) <= cap and n - 1 in tokens and 0 in tokens and (n <= SLAB or {SLAB - 1, SLAB} <= set(tokens))
  assert d >= 256 and len({values[:, c].tobytes() for c in range(d)}) == d        # all columns distinct
  # ---- the planes of every live element
  sign = np.sign(values)
  if kind == "planes3":
    p1, p2, p3 = X.split_bf16x3(values)
    assert np.isin(np.abs(p1), (1.0, 2.0)).all() and np.array_equal(np.sign(p1), sign)
    assert np.array_equal(p2, sign * np.float32(2.0 ** -9)) and np.array_equal(p3, sign * np.float32(2.0 ** -18))
    assert np.array_equal(p1.astype(np.float64) + p2 + p3, values.astype(np.float64))
  else:
    tok = np.array(tokens)
    for k0 in range(0, n, SLAB):
      rows = values[(tok >= k0) & (tok < k0 + SLAB)]
      e, (h1, h2) = X.split_f16x2(rows)
      u1, u2 = np.ldexp(h1.astype(np.float64), -e[None, :]), np.ldexp(h2.astype(np.float64), -e[None, :])
      scale = np.ldexp(1.0, (np.arange(d) % 2)[None, :]) if k0 else 1.0
      assert np.isin(np.abs(u1) / scale, (1.0, 2.0)).all() and np.array_equal(u2, np.sign(rows) * 2.0 ** -12 * scale)
      assert np.array_equal(u1 + u2, rows.astype(np.float64)) and np.abs(np.ldexp(rows, e[None, :])).max() < 2.0 ** 15
      assert e.min() >= 11 and e.max() <= 14
      if k0:
        first = X.split_f16x2(values[tok < SLAB])[0]
        assert (first != e).any() and (first == e).any()       # the exponents are per slab
  # ---- the model
  model = X.planes_model(n, d, seed, kind)
  assert np.array_equal(model, model.T)
  assert np.array_equal(model / q, np.rint(model / q)) and np.abs(model).max() < X.LIMIT * q
  assert np.array_equal(model.astype(np.float32).astype(np.float64), model)
  exact = X.exact_product(n, d, seed, kind)
  assert (exact != model).any()
  if kind == "planes3":
    differ = (exact.astype(np.float32) != model.astype(np.float32)).mean()
    assert 0.002 < differ < 0.2, differ       # what the kernel drops shows in float32 (4 to 5 % at d = 256 with 16 live tokens)
  # ---- sensitivity, on the leading block
  cols = min(d, 3 * TILE)
  base = structured_model(n, d, seed, kind, initial, cols)
  want = model[:cols, :cols] + (X.initial_product(d, seed)[:cols, :cols] if initial else 0.0)
  assert np.array_equal(base, want)
  lower = np.tril(np.ones((cols, cols), bool))
  slabs = X.slabs_of(n, d, kind)
  for mutation in MUTATIONS:
    if mutation == "a split's partial left out" and all(s[3] == 1 for s in slabs):
      continue
    if mutation == "the second slab not accumulated" and len(slabs) == 1:
      continue
    if mutation == "the initial product not added" and not initial:
      continue
    if mutation == "a tile taken from (tj, ti)":
      other = structured_model(n, d, seed, kind, initial, cols, shift_a=True)
      assert (other != other.T).any()
      mutated = base.copy()
      mutated[TILE:2 * TILE, :TILE] = other[:TILE, TILE:2 * TILE]
    else:
      mutated = structured_model(n, d, seed, kind, initial, cols, mutation)
    assert (mutated != base)[lower].any(), mutation
