"""Cases for every route of the OCTAV clip search (csrc/octav.hip: mi355q_octav_clip_f32, _fast_f32, _nd_f32),
shared by test_octav_route_cases_host.py (no GPU) and test_gpu_octav_routes.py.

Three restatements, none of which needs a GPU:

  route()       the host's choice of kernels for a call: which kernel, which instantiation, with or without the tail
                kernel, whether the rows kernel asks for more than 64 KB of dynamic LDS, how many blocks the pick kernel has;
  trajectory()  the reference iteration (ref octav.py:30-112) of ONE contiguous unit in NumPy, iteration by iteration: guess,
                next, both counts, the run lengths of both masks cut at NumPy's 8192-element chunk, whether the masks changed;
  paths()       what the rows kernel and its tail do with such a trajectory: the data-dependent branches of
                octav_rows_kernel / octav_tail_kernel / sparse_mask_sum, by name.

A case is a handful of numbers (entry, shape, kind of content, seed, parameters, environment): a child process rebuilds
it from the list index. Its id spells out its route and, for the rows kernel, the paths its data takes.

EXACT holds inputs for the one-read kernel: integer multiples of a power of two whose magnitudes add up to at most 2^24
granules per unit, so that every float32 partial sum in any order is exact and the one-read kernel (which shares
octav_step with the exact ones) must return NumPy's bits too."""
import dataclasses
import functools

import numpy as np

F = np.float32
CHUNK = 8192
PIECE = 16
WAVE = 64
GROUP_LEN = 4096
ROWS_MIN, ROWS_MAX = 129, 2 * CHUNK
DIVISOR = 3.0

E_WAVE, E_LANES, E_NARROW, E_TAIL, E_TAIL_DIV = ("MI355Q_OCTAV_WAVE_KERNEL", "MI355Q_OCTAV_UNIT_LANES", "MI355Q_OCTAV_NARROW_ROWS",
                                                 "MI355Q_OCTAV_TAIL", "MI355Q_OCTAV_TAIL_DIV")
SWITCHES = (E_WAVE, E_LANES, E_NARROW, E_TAIL, E_TAIL_DIV)


# ------------------------------------------------------------------------------------------- the host's choices ---
def _atoi(v):
  """C's atoi on the strings the cases use."""
  try:
    return int(v)
  except ValueError:
    return 0


def tail_cap(unit_len, env=None):
  env = dict(env or ())
  v = _atoi(env[E_TAIL_DIV]) if E_TAIL_DIV in env else 0
  div = v if 2 <= v <= 256 else 8
  return max(64, ((unit_len // div) + 63) & ~63)


def rows_threads(unit_len, env=None):
  npieces = (unit_len + PIECE - 1) // PIECE
  if npieces > 256 and E_NARROW not in dict(env or ()):
    return 512 if npieces <= 512 else 1024
  return 64 if npieces <= 64 else (128 if npieces <= 128 else 256)


def rows_slots(unit_len, env=None):
  threads = rows_threads(unit_len, env)
  return ((unit_len + PIECE - 1) // PIECE + threads - 1) // threads


def rows_smem(unit_len, env=None):
  """octav_rows_smem: two exchange areas, a dummy slot per thread, the padded row, two run lists, two mask-word arrays."""
  threads = rows_threads(unit_len, env)
  npieces = (unit_len + PIECE - 1) // PIECE
  xchg = 64 if threads <= 256 else 256
  row_floats = (unit_len + (unit_len >> 4) + 4) & ~3
  cap = ((unit_len // 2 + 2 + 63) & ~63) + 64
  return 2 * xchg * 4 + threads * 4 + row_floats * 4 + cap * 2 * 4 + ((npieces + 1) & ~1) * 2 * 2


def workspace_bytes(units, max_iter):
  return 0 if units <= 0 or max_iter <= 0 else units * max_iter * 4 + 64 * 4


TAIL_STATE_BYTES = 32


def rows_workspace_bytes(units, unit_len, max_iter, env=None):
  base = workspace_bytes(units, max_iter)
  if base == 0 or unit_len < ROWS_MIN or unit_len > ROWS_MAX:
    return base
  return ((base + 63) & ~63) + units * (TAIL_STATE_BYTES + 2 * tail_cap(unit_len, env) * (4 + 2))


def wave_plan(unit_len):
  """plan_units: (staged in LDS, waves per block)."""
  stride = (unit_len + 3) // 4 * 4
  waves = min(4, (64 * 1024) // (stride * 4))
  return (True, waves) if waves >= 1 else (False, 4)


FAST = ((4, "fast<1,4>"), (8, "fast<2,4>"), (16, "fast<4,4>"), (32, "fast<8,4>"), (64, "fast<16,4>"), (128, "fast<32,4>"),
        (256, "fast<64,4>"), (512, "fast<64,8>"), (1024, "fast<64,16>"), (2048, "fast<256,8>"), (4096, "fast<256,16>"),
        (8192, "fast<1024,8>"), (16384, "fast<1024,16>"))

ALL_ROUTES = tuple(
    [f"lanes<{n}>" for n in (32, 64, 128, 256)] +
    [f"rows<1,{t}>" for t in (64, 128, 256, 512, 1024)] + [f"rows<{s},256>" for s in (2, 3, 4)] +
    ["tail", "no-tail", "lds>64K", "lds<=64K", "groups"] +
    [f"wave-lds-w{w}" for w in (4, 3, 2, 1)] + ["wave-global-w4", "cols", "segs"] +
    [name for _, name in FAST] + ["pick-1", "pick-n"])


def route(entry, units, shape, aligned=True, workspace="rows", env=None):
  """The kernels a call launches, as a tuple of elements of ALL_ROUTES. `shape` is unit_len, or (outer, channels, inner)
  for the nd entry (`units` is ignored there); `workspace` says which of the two size queries the caller used."""
  env = dict(env or ())
  if entry == "nd":
    outer, channels, inner = shape
    if outer == 1:
      return route("exact", channels, inner, aligned, workspace, env)
    return ("cols" if inner == 1 else "segs",) + _pick(channels)
  unit_len = shape
  if entry == "fast":
    assert aligned and unit_len % 4 == 0 and 4 <= unit_len <= 65536
    return (next(name for limit, name in FAST if unit_len // 4 <= limit),) + _pick(units)
  assert entry == "exact"
  forced_wave = E_WAVE in env
  lanes_on = E_LANES not in env or _atoi(env[E_LANES]) != 0
  if unit_len in (32, 64, 128, 256) and aligned and lanes_on and not forced_wave:
    return (f"lanes<{unit_len}>",) + _pick(units)
  if ROWS_MIN <= unit_len <= ROWS_MAX and not forced_wave:
    threads, slots = rows_threads(unit_len, env), rows_slots(unit_len, env)
    tail_on = E_TAIL not in env or _atoi(env[E_TAIL]) != 0
    tail = tail_on and slots == 1 and workspace == "rows"
    return (f"rows<{slots},{threads}>", "tail" if tail else "no-tail",
            "lds>64K" if rows_smem(unit_len, env) > 64 * 1024 else "lds<=64K") + _pick(units)
  if (2 * PIECE <= unit_len <= 512 and unit_len & (unit_len - 1) == 0 and (units * unit_len) % GROUP_LEN == 0 and aligned
      and not forced_wave):
    return ("groups",) + _pick(units)
  lds, waves = wave_plan(unit_len)
  return (f"wave-lds-w{waves}" if lds else f"wave-global-w{waves}",) + _pick(units)


def _pick(units):
  return ("pick-1" if units <= 256 else "pick-n",)


def has_tail(r):
  return "tail" in r


# ------------------------------------------------------------------------------------------------ the iteration ---
@dataclasses.dataclass(frozen=True)
class Step:
  guess: np.float32
  next: np.float32
  count_pos: int
  count_neg: int
  runs_pos: tuple          # (starts, lengths) of the runs of x >= guess, cut at the 8192-element chunk
  runs_neg: tuple
  changed: bool            # the masks differ from the previous iteration's (from empty ones in iteration 0)
  mask_pos: np.ndarray = dataclasses.field(repr=False, compare=False, default=None)
  mask_neg: np.ndarray = dataclasses.field(repr=False, compare=False, default=None)


def runs_of(mask):
  """(starts, lengths) of the stretches of True inside one 8192-element chunk each."""
  n = len(mask)
  idx = np.arange(n)
  prev = np.concatenate(([False], mask[:-1]))
  prev[idx % CHUNK == 0] = False
  nxt = np.concatenate((mask[1:], [False]))
  nxt[(idx + 1) % CHUNK == 0] = False
  starts = np.flatnonzero(mask & ~prev)
  ends = np.flatnonzero(mask & ~nxt)
  return starts, ends - starts + 1


def trajectory(x_unit, bits, max_iter, count_is_f64):
  """The reference iteration of one unit, every iteration (no early stop): a list of max_iter Steps. With count_is_f64 the
  unit is a row of a [1, len] array reduced over axis 1 (N is np.int64, s * N float64); without, the whole tensor with
  axis=None (N a Python int, s * N float32)."""
  x = np.ascontiguousarray(x_unit, F).reshape(-1)
  if count_is_f64:
    x, axis = x.reshape(1, -1), (1,)
    count = np.prod([x.shape[1]])
    guess = np.ones((1, 1), F)
  else:
    axis = None
    count = x.size
    guess = np.ones((1,), F)
  s = np.asarray(4.0 ** (-bits) / DIVISOR, dtype=F)
  steps = []
  last_p = np.zeros(x.size, bool)
  last_n = np.zeros(x.size, bool)
  with np.errstate(all="ignore"):
    for _ in range(max_iter):
      old = guess
      mp = np.greater_equal(x, old)
      denom = np.count_nonzero(mp, axis=axis, keepdims=True).astype(F)
      guess = np.sum(x, axis=axis, where=mp, keepdims=True, dtype=F)
      mn = np.less_equal(x, -old)
      denom = np.add(denom, np.count_nonzero(mn, axis=axis, keepdims=True), out=denom)
      guess = np.subtract(guess, np.sum(x, axis=axis, where=mn, keepdims=True), out=guess)
      denom = np.multiply(denom, 1.0 - s, out=denom)
      denom = np.add(denom, s * count, out=denom)
      guess = np.divide(guess, denom, out=guess)
      fp, fn = mp.reshape(-1), mn.reshape(-1)
      steps.append(Step(F(old.reshape(-1)[0]), F(guess.reshape(-1)[0]), int(fp.sum()), int(fn.sum()), runs_of(fp), runs_of(fn),
                        bool((fp != last_p).any() or (fn != last_n).any()), fp, fn))
      last_p, last_n = fp, fn
  return steps


def iterates(x, bits, max_iter, count_is_f64=1, axes=(1,)):
  """Every iterate of every unit, [max_iter, units], all units in one NumPy call per step as the reference does it (x is
  [units, len] with axes (1,), or [outer, channels, inner] with axes (0, 2)); count_is_f64 = 0: axis=None unit by unit."""
  if not count_is_f64:
    return np.stack([np.array([st.next for st in trajectory(u, bits, max_iter, 0)], F) for u in x], axis=1)
  count = np.prod([x.shape[d] for d in axes])
  guess = np.ones(tuple(1 if k in axes else d for k, d in enumerate(x.shape)), F)
  s = np.asarray(4.0 ** (-bits) / DIVISOR, dtype=F)
  mask = np.zeros(x.shape, bool)
  out = []
  with np.errstate(all="ignore"):
    for _ in range(max_iter):
      old = guess
      mask = np.greater_equal(x, old, out=mask)
      denom = np.count_nonzero(mask, axis=axes, keepdims=True).astype(F)
      guess = np.sum(x, axis=axes, where=mask, keepdims=True, dtype=F)
      mask = np.less_equal(x, -old, out=mask)
      denom = np.add(denom, np.count_nonzero(mask, axis=axes, keepdims=True), out=denom)
      guess = np.subtract(guess, np.sum(x, axis=axes, where=mask, keepdims=True), out=guess)
      denom = np.multiply(denom, 1.0 - s, out=denom)
      denom = np.add(denom, s * count, out=denom)
      guess = np.divide(guess, denom, out=guess)
      out.append(guess.reshape(-1).copy())
  return np.stack(out)


def step_next(pos_sum, neg_sum, count_pos, count_neg, n, bits, count_is_f64):
  """octav_step of octav_common.h in NumPy scalars: the next iterate from the two masked sums and their counts."""
  s = F(4.0 ** (-bits) / DIVISOR)
  with np.errstate(all="ignore"):
    num = F(F(pos_sum) - F(neg_sum))
    den = F(count_pos)
    den = F(np.float64(den) + np.float64(count_neg))
    den = F(den * F(F(1.0) - s))
    if count_is_f64:
      den = F(np.float64(den) + np.float64(s) * np.float64(n))
    else:
      den = F(den + F(s * F(n)))
    return F(num / den)


# --------------------------------------------------------------------- what the rows kernel and its tail do with it ---
ALL_PATHS = ("empty", "reused", "dense", "sparse", "run>128", "run-x-piece", "run-x-chunk", "handover", "list>64", "carry64", "run7",
             "run8+", "below-cand", "margin")
KEEP = F(0.998046875)      # 1 - 2^-9


def _piece_events(mask, runs, out):
  starts, lengths = runs
  if len(starts) == 0:
    out.add("sparse")       # (no piece has more than 3 run starts)
    return
  npieces = (len(mask) + PIECE - 1) // PIECE
  per_piece = np.bincount(starts // PIECE, minlength=npieces)
  nw = (npieces + WAVE - 1) // WAVE
  per_wave = np.zeros(nw * WAVE, np.int64)
  per_wave[:npieces] = per_piece
  busy = (per_wave.reshape(nw, WAVE) > 3).any(axis=1)      # the choice is one per wave (and mask, and slot)
  if busy.any():
    out.add("dense")
  if (~busy).any():
    out.add("sparse")
  if (lengths > 128).any():
    out.add("run>128")
  if ((starts // PIECE) != ((starts + lengths - 1) // PIECE)).any():
    out.add("run-x-piece")


def _tail_mask(x, neg, guess, cand, out):
  """One sparse_mask_sum call: `cand` are the listed positions (ascending). False: the caller falls back."""
  v = x[cand]
  thr = -guess if neg else guess
  keep = -(guess * KEEP) if neg else guess * KEEP
  sel = (v <= thr) if neg else (v >= thr)
  stay = (v <= keep) if neg else (v >= keep)
  if len(cand) > WAVE:
    out.add("list>64")
  link = sel[:-1] & sel[1:] & (cand[1:] == cand[:-1] + 1) & (cand[1:] % CHUNK != 0)     # link[i]: i + 1 continues i's run
  length = np.zeros(len(cand), np.int64)
  n = 0
  for i in range(len(cand)):
    n = n + 1 if (i > 0 and link[i - 1]) else (1 if sel[i] else 0)
    length[i] = n
  if (length >= 8).any():
    out.add("run8+")
    return None
  ends = np.ones(len(cand), bool)
  ends[:-1] = ~link
  if ((length == 7) & ends).any():
    out.add("run7")
  if any(link[i - 1] for i in range(WAVE, len(cand), WAVE)):
    out.add("carry64")
  if (stay & ~sel).any():
    out.add("margin")
  return cand[stay]


def paths(steps, x_unit, cap, tail, max_iter):
  """The names (ALL_PATHS) of what octav_rows_kernel and, after a hand-over, octav_tail_kernel do on this unit.
  `tail`: the call has the tail workspace; `cap`: tail_cap of the row length."""
  x = np.ascontiguousarray(x_unit, F).reshape(-1)
  finite = x[~np.isnan(x)]
  amax = F(np.abs(finite).max()) if finite.size else F(0)
  out = set()
  force = True
  handover = None
  for it, st in enumerate(steps):
    empty = bool(st.guess > amax)
    if empty:
      out.add("empty")
      force = True
    else:
      if st.changed or force:
        force = False
        _piece_events(st.mask_pos, st.runs_pos, out)
        _piece_events(st.mask_neg, st.runs_neg, out)
        for m in (st.mask_pos, st.mask_neg):
          if len(m) > CHUNK and m[CHUNK - 1] and m[CHUNK]:
            out.add("run-x-chunk")
      else:
        out.add("reused")
    if st.next == st.guess:
      return out, handover
    if (tail and not empty and it + 2 < max_iter and st.guess > 0 and st.next >= st.guess and st.count_pos <= cap
        and st.count_neg <= cap):
      handover = it
      out.add("handover")
      break
  if handover is None:
    return out, None
  cand = [np.flatnonzero(steps[handover].mask_pos), np.flatnonzero(steps[handover].mask_neg)]
  cand_guess = steps[handover].guess
  lists_ok = True
  for it in range(handover + 1, max_iter):
    st = steps[it]
    if lists_ok and st.guess >= cand_guess:
      kept_p = _tail_mask(x, False, st.guess, cand[0], out)
      kept_n = _tail_mask(x, True, st.guess, cand[1], out) if kept_p is not None else None
      if kept_n is None:
        lists_ok = False
      else:
        cand = [kept_p, kept_n]
        cand_guess = st.guess * KEEP
    elif lists_ok:
      out.add("below-cand")
      lists_ok = False
    if st.next == st.guess:
      break
  return out, handover


# ------------------------------------------------------------------------------------------------------ contents ---
KINDS = ("gauss", "stretch", "same-sign", "outliers", "zeros-nan", "special")


def _stretch_spec(seed):
  return (7, 8, 9)[seed % 3], ("start", "end", "mid", "cross", "two")[(seed // 3) % 5]


def unit_of(kind, n, rng, seed):
  """One unit of `n` elements."""
  x = (rng.standard_normal(n) * 0.02).astype(F)
  if kind == "gauss":
    return x
  if kind == "stretch":
    k, where = _stretch_spec(seed)
    k = min(k, n)
    at = {"start": 0, "end": n - k, "mid": (n - k) // 2, "cross": CHUNK - 3 if n >= CHUNK + k else (n - k) // 3,
          "two": (n - k) // 2}[where]
    x[at:at + k] = (0.4 + 0.2 * rng.random(k)).astype(F)       # (full mantissas: the order of the additions shows)
    if where == "two" and at + 2 * k + 1 <= n:
      x[at + k] = 0.001                                   # one element between two stretches
      x[at + k + 1:at + 2 * k + 1] = (0.4 + 0.2 * rng.random(k)).astype(F)
    if seed % 2:
      x = -x
    return x
  if kind == "same-sign":
    x = np.abs(x) * F(2.5)
    return -x if seed % 2 else x
  if kind == "outliers":
    x = (x * F(0.05)).astype(F)
    pick = rng.random(n) < 0.03
    x[pick] *= F(3e3)
    return x
  if kind == "zeros-nan":
    x[rng.random(n) < 0.3] = 0.0
    x[rng.random(n) < 0.05] = -0.0
    x[n // 3] = np.nan
    return x
  if kind == "special":
    which = seed % 4
    if which == 0:
      return np.zeros(n, F)
    x[(2 * n) // 3] = (np.inf, -np.inf, np.inf)[which - 1]
    if which == 3:
      x[0] = -np.inf
    return x
  if kind == "unit-normal":
    return rng.standard_normal(n).astype(F)
  raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def content(kind, units, n, seed):
  """[units, n] float32. kind "mix": unit u has kind KINDS[(u + seed) % 6], so the units of a case converge in different
  iterations and the global early stop is decided by the slowest; any other kind: every unit of that kind."""
  rng = np.random.default_rng([units, n, seed])
  rows = [unit_of(KINDS[(u + seed) % len(KINDS)] if kind == "mix" else kind, n, rng, seed + u) for u in range(units)]
  x = np.stack(rows).astype(F)
  x.setflags(write=False)
  return x


# --- a unit that still moves after 32 iterations (a 2-cycle wider than np.allclose) ---
MOVING_SEARCH_UNITS = 100000
MOVING_SEARCH_LEN = 8
MOVING_SEARCH_SEED = 2025
MOVING_FROM = 32


@functools.lru_cache(maxsize=None)
def moving_search_units():
  """The search's population: [100000, 8], few distinct magnitudes per unit."""
  rng = np.random.default_rng(MOVING_SEARCH_SEED)
  levels = rng.integers(1, 6, size=(MOVING_SEARCH_UNITS, MOVING_SEARCH_LEN)).astype(F)
  x = (levels * rng.choice(np.array([0.125, 0.3, 1.0], F), size=(MOVING_SEARCH_UNITS, 1))).astype(F)
  x *= np.where(rng.random(x.shape) < 0.5, F(-1), F(1))
  x[rng.random(x.shape) < 0.2] = 0.0
  x.setflags(write=False)
  return x


MOVING_BITS = 1
MOVING_ROW_UNITS = (60, 115, 251)      # units of the population that still move when they sit in a row of zeros
MOVING_ROW_LEN = 136


def moving_rows():
  """The population's units MOVING_ROW_UNITS, each inside a row of MOVING_ROW_LEN zeros: rows-kernel units whose `moved` mask
  needs its high word."""
  x = np.zeros((len(MOVING_ROW_UNITS), MOVING_ROW_LEN), F)
  x[:, 3:3 + MOVING_SEARCH_LEN] = moving_search_units()[list(MOVING_ROW_UNITS)]
  return x


def moving_search(bits=MOVING_BITS, max_iter=40):
  """Indices of the population's units whose iterate still moves (not np.isclose to the one before) in some iteration
  >= MOVING_FROM."""
  x = moving_search_units()
  it = iterates(x, bits, max_iter)
  before = np.concatenate((np.ones((1, x.shape[0]), F), it[:-1]))
  moving = ~np.isclose(before, it)
  return np.flatnonzero(moving[MOVING_FROM:].any(axis=0))


# ---------------------------------------------------------------------------------------------------- the cases ---
@dataclasses.dataclass(frozen=True)
class Case:
  entry: str                 # "exact" | "nd" | "fast"
  units: int                 # (nd: channels)
  unit_len: int              # (nd: inner)
  kind: str = "mix"
  seed: int = 0
  bits: int = 4
  max_iter: int = 10
  f64: int = 1
  aligned: bool = True
  workspace: str = "rows"    # "rows": mi355q_octav_rows_workspace_bytes; "base": mi355q_octav_workspace_bytes
  outer: int = 1             # nd only
  env: tuple = ()
  order_sensitive: bool = False

  @property
  def envd(self):
    return dict(self.env)

  @property
  def shape(self):
    return (self.outer, self.units, self.unit_len) if self.entry == "nd" else self.unit_len


def data(c):
  """The case's tensor: [units, unit_len], or [outer, channels, inner] for the nd entry."""
  if c.kind == "moving":
    return moving_search_units()[c.seed:c.seed + c.units]
  if c.kind == "moving-row":
    return moving_rows()
  if c.kind == "exact":
    return exact_content(c.units, c.unit_len, c.seed)
  if c.entry == "nd":
    return content(c.kind, c.outer * c.units, c.unit_len, c.seed).reshape(c.outer, c.units, c.unit_len)
  return content(c.kind, c.units, c.unit_len, c.seed)


def case_route(c):
  return route(c.entry, c.units, c.shape, c.aligned, c.workspace, c.env)


@functools.lru_cache(maxsize=None)
def case_trajectories(c):
  assert c.entry == "exact"
  return tuple(tuple(trajectory(u, c.bits, c.max_iter, c.f64)) for u in data(c))


@functools.lru_cache(maxsize=None)
def case_paths(c):
  """The union of the units' paths (rows kernel only: the other kernels have no such branches to name)."""
  r = case_route(c)
  if c.entry != "exact" or not r[0].startswith("rows"):
    return ()
  cap = tail_cap(c.unit_len, c.env)
  found = set()
  for u, steps in zip(data(c), case_trajectories(c)):
    found |= paths(steps, u, cap, has_tail(r), c.max_iter)[0]
  return tuple(p for p in ALL_PATHS if p in found)


@functools.lru_cache(maxsize=None)
def case_iterates(c):
  x = data(c)
  if c.entry == "nd":
    return iterates(x, c.bits, c.max_iter, 1, (0, 2))
  return iterates(x, c.bits, c.max_iter, c.f64)


def case_id(c):
  shape = f"{c.outer}x{c.units}x{c.unit_len}" if c.entry == "nd" else f"{c.units}x{c.unit_len}"
  parts = [c.entry, shape, f"{c.kind}{c.seed}", f"b{c.bits}", f"i{c.max_iter}"]
  if not c.f64:
    parts.append("f32count")
  if not c.aligned:
    parts.append("offset4")
  if c.workspace == "base":
    parts.append("basews")
  parts += [f"{k.replace('MI355Q_OCTAV_', '')}={v}" for k, v in c.env]
  return "-".join(parts) + "-" + "+".join(case_route(c)) + ("-" + "+".join(case_paths(c)) if case_paths(c) else "")


BITS = (4, 8, 2, 1, 16)
ITERS = (10, 3, 10, 2, 10, 1, 10)


def _build_cases():
  cases = []
  n = [0]

  def add(entry, units, unit_len, **kw):
    i = n[0]
    n[0] += 1
    j = 7 * units + unit_len + kw.get("outer", 1)       # (parameters from the shape: adding a case does not change the others)
    kw.setdefault("seed", i)
    kw.setdefault("bits", BITS[j % len(BITS)])
    kw.setdefault("max_iter", ITERS[j % len(ITERS)])
    cases.append(Case(entry, units, unit_len, **kw))

  # the rows kernel: both workspaces, and x four bytes off a 16-byte boundary
  for k, unit_len in enumerate((129, 1000, 1024, 1025, 2048, 2049, 4096, 4097, 4100, 8191, 8192, 8193, 8192 + 71, 16383, 16384)):
    units = 3 + k % 4
    seed = 100 + k
    bits, max_iter = BITS[k % len(BITS)], (10, 10, 5, 10, 4)[k % 5]
    for variant in (dict(), dict(workspace="base"), dict(aligned=False)):
      add("exact", units, unit_len, seed=seed, bits=bits, max_iter=max_iter, order_sensitive=not variant, **variant)
  # contents aimed at the tail's branches (the stretches of 7 / 8 / 9, at the start, the end, across element 8192, two one apart)
  for unit_len in (1024, 4096, 16384):
    for seed in range(15):
      add("exact", 1, unit_len, kind="stretch", seed=seed, bits=4, max_iter=10)
  add("exact", 4, 4096, kind="same-sign", bits=4, max_iter=10, order_sensitive=True)
  add("exact", 3, 16384, kind="same-sign", bits=8, max_iter=10, order_sensitive=True)
  add("exact", 5, 2048, kind="outliers", bits=4, max_iter=10)
  add("exact", 5, 1000, kind="outliers", bits=2, max_iter=40)
  add("exact", 4, 3000, kind="unit-normal", bits=4, max_iter=10, order_sensitive=True)
  add("exact", 6, 640, kind="zeros-nan", bits=4, max_iter=10)
  add("exact", 4, 512, kind="special", bits=8, max_iter=10)
  add("exact", 3, 4096, kind="gauss", bits=4, max_iter=40)
  add("exact", 3, 1024, kind="gauss", bits=16, max_iter=10)
  add("exact", 3, 1024, kind="gauss", bits=1, max_iter=10)
  # iterates that still move after 32 iterations (moving_search): bit 32 and up of the `moved` masks
  add("exact", 40, MOVING_SEARCH_LEN, kind="moving", seed=0, bits=MOVING_BITS, max_iter=40)
  add("exact", len(MOVING_ROW_UNITS), MOVING_ROW_LEN, kind="moving-row", seed=0, bits=MOVING_BITS, max_iter=40)
  add("exact", len(MOVING_ROW_UNITS), MOVING_ROW_LEN, kind="moving-row", seed=0, bits=MOVING_BITS, max_iter=40, workspace="base")
  # count_is_f64 = 0 (TENSORWISE: s * N in float32): one unit and several
  # (seeds at which s * N in float32 changes bits of some iterate; at a power-of-two length s * N is exact either way)
  add("exact", 1, 4096, kind="gauss", f64=0, bits=4, max_iter=10)
  add("exact", 1, 3001, kind="unit-normal", seed=100, f64=0, bits=1, max_iter=10)
  add("exact", 1, 100, kind="gauss", seed=103, f64=0, bits=2, max_iter=10)
  add("exact", 4, 1000, seed=108, f64=0, bits=2, max_iter=10)
  add("exact", 5, 100, seed=101, f64=0, bits=2, max_iter=10)
  add("exact", 70, 64, f64=0, bits=2, max_iter=10)
  # the one-wave kernel: short units, units too long for the rows kernel, short power-of-two units off alignment
  for k, unit_len in enumerate((1, 2, 7, 31, 33, 63, 65, 100, 127, 16385, 20000)):
    add("exact", (1, 3, 5)[k % 3], unit_len, order_sensitive=unit_len >= 100, **(dict(max_iter=10) if unit_len > ROWS_MAX else {}))
  for unit_len in (32, 64, 128):
    add("exact", 5, unit_len, aligned=False)
  # a lane per unit: lanes of the last wave without a unit, and a second block of the pick kernel
  for k, unit_len in enumerate((32, 64, 128, 256)):
    add("exact", 70, unit_len, max_iter=(3, 10, 2, 10)[k], order_sensitive=unit_len == 256)
    add("exact", 257, unit_len, max_iter=10)
  add("exact", 64, 64, kind="unit-normal", bits=4, max_iter=40)
  # the nd entry
  for k, (outer, channels) in enumerate(((2, 1), (9, 255), (300, 257), (2, 257), (300, 1), (9, 1))):
    add("nd", channels, 1, outer=outer, kind=("mix", "unit-normal")[k % 2], max_iter=(10, 10, 3, 10, 10, 1)[k])
  for k, (outer, inner) in enumerate(((2, 2), (3, 7), (2, 8), (3, 9), (2, 129), (3, 8200), (3, 2), (2, 8200))):
    add("nd", (5, 3, 6)[k % 3], inner, outer=outer, kind=("mix", "unit-normal")[k % 2], max_iter=(10, 2, 10, 10, 10, 3, 10, 10)[k])
  add("nd", 4, 1000, outer=1)
  return tuple(cases)


def _build_env_cases():
  cases = []
  n = [0]

  def add(env, units, unit_len, **kw):
    i = n[0]
    n[0] += 1
    kw.setdefault("seed", 500 + i)
    kw.setdefault("bits", BITS[i % len(BITS)])
    kw.setdefault("max_iter", 10)
    cases.append(Case("exact", units, unit_len, env=tuple(sorted(env.items())), **kw))

  for k, unit_len in enumerate((4096, 4097, 5460, 5461, 8192, 8193, 16384)):
    add({E_WAVE: "1"}, (3, 5, 2)[k % 3], unit_len, order_sensitive=k == 0)
  add({E_WAVE: "1"}, 70, 64)
  for unit_len in (32, 64, 128):
    add({E_LANES: "0"}, GROUP_LEN // unit_len * 2, unit_len)
    add({E_LANES: "0"}, 70, unit_len)           # not a whole number of groups: the one-wave kernel
  add({E_LANES: "0"}, 32, 256)                   # (the rows kernel)
  for k, unit_len in enumerate((4097, 8192, 8193, 12288, 12289, 16384)):
    add({E_NARROW: "1"}, 3 + k % 2, unit_len, order_sensitive=unit_len in (8192, 12289, 16384))
    add({E_NARROW: "1"}, 2, unit_len, aligned=False)
  add({E_NARROW: "1"}, 3, 16384, kind="same-sign")
  add({E_NARROW: "1"}, 4, 1000)
  for k, unit_len in enumerate((129, 1024, 4100, 8192 + 71, 16384)):
    add({E_TAIL: "0"}, 3 + k % 3, unit_len)
  for k, unit_len in enumerate((129, 1000, 2048, 4096, 8193)):
    add({E_TAIL_DIV: "2"}, 3 + k % 3, unit_len)
  add({E_TAIL_DIV: "2"}, 4, 3000, kind="unit-normal")
  add({E_TAIL_DIV: "2"}, 3, 4096, kind="gauss", max_iter=40)
  for seed in range(6):
    add({E_TAIL_DIV: "2"}, 1, 4096, kind="stretch", seed=seed, bits=4)
  for k, unit_len in enumerate((1000, 4096, 16384)):
    add({E_TAIL_DIV: "256"}, 3 + k % 3, unit_len)
  for seed in range(3):
    add({E_TAIL_DIV: "256"}, 1, 16384, kind="stretch", seed=3 + seed, bits=4)
  return tuple(cases)


# ------------------------------------------------------------------------ exact inputs for the one-read kernel ---
EXACT_LIMIT = 1 << 24
EXACT_LENGTHS = (4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196, 16384,
                 16388, 32768, 32772, 65536)


def exact_granule_log2(unit_len):
  """e of the granule 2^-e: the integers' spread is chosen from the budget, the granule makes the values weight-sized."""
  return int(round(np.log2(exact_sigma(unit_len) / 0.03)))


def exact_sigma(unit_len):
  return min(4096.0, 0.9 * EXACT_LIMIT / unit_len)


@functools.lru_cache(maxsize=None)
def exact_integers(units, unit_len, seed):
  """[units, unit_len] int64: Gaussian-like integers; unit 1 mostly zeros, the last unit's sign pattern reversed."""
  rng = np.random.default_rng([7, units, unit_len, seed])
  k = np.rint(rng.standard_normal((units, unit_len)) * exact_sigma(unit_len)).astype(np.int64)
  if units > 1:
    k[1, rng.random(unit_len) < 0.7] = 0
  return k


@functools.lru_cache(maxsize=None)
def exact_content(units, unit_len, seed):
  k = exact_integers(units, unit_len, seed)
  x = np.ldexp(k.astype(np.float64), -exact_granule_log2(unit_len)).astype(F)
  x[1, unit_len - 1] = np.nan          # (unit 1: mostly zeros, and a NaN)
  x[2, unit_len // 2] = -0.0
  if seed % 2:
    x[2, 0] = np.inf if seed % 4 == 1 else -np.inf
  if units >= 5:                       # the short lengths: an all-zero unit, a unit with both infinities
    x[3] = 0.0
    x[4, 0], x[4, unit_len - 1] = np.inf, -np.inf
  x.setflags(write=False)
  return x


def _build_exact():
  out = []
  for i, unit_len in enumerate(EXACT_LENGTHS):
    units = 5 if unit_len < 1028 else 3
    out.append(Case("fast", units, unit_len, kind="exact", seed=i, bits=BITS[i % len(BITS)], max_iter=40 if i % 6 == 0 else (10, 6)[i % 2]))
  return tuple(out)


CASES = _build_cases()
ENV_CASES = _build_env_cases()
EXACT = _build_exact()
