"""Every route of the tensor comparison kernels (mi355q_compare_f32, mi355q_compare_f32_batched; csrc/validation.hip)
on designed inputs, field by field against NumPy.

The cases, the host models of the routes and the proof that the case list reaches every named route are in
compare_route_cases.py / test_compare_route_cases_host.py, which need no GPU. Here the whole sums list is one batched
call, the median list another and the mixed-kind table a third; the records are fetched once and asserted case by case,
so a failure names the case and the routes it runs.

  sum_sq_diff, sum_ref_sq     the bits of NumPy's float32 np.sum(np.square(t - r)) and np.sum(np.square(r))
  median_lo, median_hi        the bits of the two sorted middles of the host's float32 ratios
  dot_tr, dot_tt, dot_rr      within n * 2^-52 * Sum|terms| of np.sum of the float32 products in float64 (no order of a
                              float64 sum leaves that bound); equal where the sums are exact
  sum_kl                      within 1e-5 * Sum|terms| + 1e-30 (logf against NumPy's log); == 0.0 where every term is 0

The hand-built tables (empty entries, refused tables) go through the C ABI: ops.compare filters empty pairs out and
checks its arguments on the host. Every pointer of a refused table points at a live buffer of the right size, except
the null scale that one case is about, and the workspace is sized for the larger of the claimed and the true chunk
count: the point is the refusal, not what would happen without it."""
import functools
import os
import sys
import types

import numpy as np
import pytest

import compare_route_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN, NO_KL = 1, 2
F32_FIELDS = ("sum_sq_diff", "sum_ref_sq", "sum_kl", "median_lo", "median_hi")
F64_FIELDS = ("dot_tr", "dot_tt", "dot_rr")
FILL = 0x5A                       # every byte of the results before a call


@functools.lru_cache(maxsize=None)
def modules():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  assert ops.COMPARE_MEDIAN == MEDIAN and ops.COMPARE_NO_KL == NO_KL
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), ffi=_ffi)


@pytest.fixture(scope="module")
def m():
  return modules()


def f32_stored(t):
  return {"kind": "f32", "data": np.asarray(t, np.float32), "scale": None, "zero_point": None, "channels": 1,
          "inner": 1, "diff_bits": 32}


class Operands:
  """Host arrays packed into one device buffer (one upload), each at a 16-byte aligned offset."""

  def __init__(self):
    self.blobs, self.size, self.dev = [], 0, None

  def add(self, a):
    if a is None:
      return None
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    off = self.size
    self.blobs.append((off, b))
    self.size = (off + b.size + 15) & ~15
    return off

  def upload(self):
    host = np.zeros(self.size + 16, np.uint8)
    for off, b in self.blobs:
      host[off:off + b.size] = b
    self.dev = modules().torch.from_numpy(host).cuda()
    self.blobs = []
    return self.dev.data_ptr()


class Table:
  """A device table of mi355q_compare_pair built by hand from [(reference, stored)]; (None, None) is an empty entry."""

  def __init__(self, entries):
    m = modules()
    self.operands = Operands()
    offs = []
    for r, st in entries:
      if r is None:
        offs.append(None)
        continue
      zp = None if st["zero_point"] is None else np.asarray(st["zero_point"], np.int32)
      scale = None if st["scale"] is None else np.asarray(st["scale"], np.float32)
      offs.append((self.operands.add(np.asarray(r, np.float32)), self.operands.add(st["data"]),
                   self.operands.add(scale), self.operands.add(zp)))
    base = self.operands.upload()
    self.table = np.zeros(len(entries), m.ops.COMPARE_PAIR_DTYPE)
    for rec, (r, st), off in zip(self.table, entries, offs):
      if off is None:
        continue
      rec["reference"], rec["target"], rec["n"] = base + off[0], base + off[1], len(r)
      rec["kind"], rec["diff_bits"] = m.ops.COMPARE_KINDS[st["kind"]], st["diff_bits"]
      rec["channels"], rec["inner"] = st["channels"], st["inner"]
      rec["scale"] = 0 if off[2] is None else base + off[2]
      rec["zero_point"] = 0 if off[3] is None else base + off[3]
    self.chunks = int(sum(-(-int(n) // S.CHUNK) for n in self.table["n"]))
    assert self.chunks == sum(m.L.mi355q_compare_chunks(int(n)) for n in self.table["n"])


def workspace(m, count, chunks, fill=None):
  nbytes = max(int(m.L.mi355q_compare_workspace_bytes(count, chunks)), 1)
  if fill is None:
    return m.torch.empty((nbytes,), dtype=m.torch.uint8, device="cuda")
  return m.torch.full((nbytes,), fill, dtype=m.torch.uint8, device="cuda")


def run_batched(m, table, chunks, flags, ws=None):
  """mi355q_compare_f32_batched over a host copy of the table -> the records (host). Synchronizes."""
  count = len(table)
  dev_table = m.torch.from_numpy(table.view(np.uint8).copy()).cuda()
  res = m.torch.full((count * m.ops.COMPARE_RESULT_DTYPE.itemsize,), FILL, dtype=m.torch.uint8, device="cuda")
  if ws is None:
    ws = workspace(m, count, chunks)
  assert ws.numel() >= m.L.mi355q_compare_workspace_bytes(count, chunks)
  m.ffi.check(m.L.mi355q_compare_f32_batched(m.rt.ptr(dev_table), count, chunks, flags, m.rt.ptr(res), m.rt.ptr(ws),
                                             ws.numel(), m.rt.stream_ptr()))
  return res.cpu().numpy().view(m.ops.COMPARE_RESULT_DTYPE)


def run_single(m, r, st, flags):
  """One pair through mi355q_compare_f32 -> its record."""
  t = Table([(r, st)])
  rec = t.table[0]
  res = m.torch.full((m.ops.COMPARE_RESULT_DTYPE.itemsize,), FILL, dtype=m.torch.uint8, device="cuda")
  ws = workspace(m, 1, t.chunks)
  m.ffi.check(m.L.mi355q_compare_f32(
      int(rec["reference"]), int(rec["target"]), int(rec["n"]), int(rec["kind"]), int(rec["diff_bits"]),
      int(rec["channels"]), int(rec["inner"]), int(rec["scale"]) or None, int(rec["zero_point"]) or None, flags,
      m.rt.ptr(res), m.rt.ptr(ws), ws.numel(), m.rt.stream_ptr()))
  return res.cpu().numpy().view(m.ops.COMPARE_RESULT_DTYPE)[0]


def u32(x):
  return int(np.asarray(x, np.float32).view(np.uint32))


def record_bytes(rec):
  return np.asarray(rec).tobytes()


def mismatches(name, routes, rec, ref, exact_dots=False, kl_zero=False):
  """The fields of `rec` that miss the reference `ref` (compare_route_cases.reference_record), as messages."""
  out = []
  tag = f"{name} {sorted(routes)}"
  for f in ("sum_sq_diff", "sum_ref_sq", "median_lo", "median_hi"):
    if u32(rec[f]) != u32(ref[f]):
      out.append(f"{tag}: {f} {float(rec[f])!r} ({u32(rec[f]):#010x}) != {float(ref[f])!r} ({u32(ref[f]):#010x})")
  if ref["n"] % 2 and u32(rec["median_hi"]) != u32(rec["median_lo"]):
    out.append(f"{tag}: odd n with median_hi != median_lo")
  for f in F64_FIELDS:
    got, want, bound = float(rec[f]), ref[f], (0.0 if exact_dots else ref[f + "_bound"])
    if not abs(got - want) <= bound:
      out.append(f"{tag}: {f} {got!r} != {want!r} by {abs(got - want):.3e} > {bound:.3e}")
  got, want = float(rec["sum_kl"]), float(ref["sum_kl"])
  if kl_zero:
    if not got == 0.0:
      out.append(f"{tag}: sum_kl {got!r} != 0")
  elif not abs(got - want) <= ref["kl_bound"]:
    out.append(f"{tag}: sum_kl {got!r} != {want!r} by {abs(got - want):.3e} > {ref['kl_bound']:.3e}")
  return out


def report(failures):
  assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures[:40])


# ---------------------------------------------------------------- the three batched lists, run once per module
@pytest.fixture(scope="module")
def sums(m):
  cases = S.sum_cases()
  pairs = [S.sum_pair(c) for c in cases]
  table = Table([(r, f32_stored(t)) for t, r in pairs])
  recs = run_batched(m, table.table, table.chunks, MEDIAN)
  refs = [S.reference_record(t, r) for t, r in pairs]
  return {c.name: (c, rec, ref) for c, rec, ref in zip(cases, recs, refs)}


@pytest.fixture(scope="module")
def medians(m):
  cases = S.median_cases()
  pairs = [S.median_pair(c)[:2] for c in cases]
  table = Table([(r, f32_stored(t)) for t, r in pairs])
  recs = run_batched(m, table.table, table.chunks, MEDIAN)
  refs = [S.reference_record(t, r) for t, r in pairs]
  return types.SimpleNamespace(table=table, records=recs,
                               by_name={c.name: (c, rec, ref) for c, rec, ref in zip(cases, recs, refs)})


@pytest.fixture(scope="module")
def mixed(m):
  cases = S.mixed_cases()
  entries = [S.mixed_entry(c) for c in cases]
  table = Table([(r, st) for _, r, st in entries])
  recs = run_batched(m, table.table, table.chunks, MEDIAN)
  refs = [S.reference_record(t, r) for t, r, _ in entries]
  return {c.name: (c, rec, ref) for c, rec, ref in zip(cases, recs, refs)}


# ---------------------------------------------------------------- 1. the sums list and the median list
def test_sums_list_in_one_batched_call(sums):
  failures = []
  for name, (c, rec, ref) in sums.items():
    failures += mismatches(name, S.routes_of(c), rec, ref, exact_dots=c.kind == "integers",
                           kl_zero=c.kind in ("equal_positive", "nonpositive_reference"))
  report(failures)


def test_median_list_in_one_batched_call(medians):
  failures = []
  for name, (c, rec, ref) in medians.by_name.items():
    failures += mismatches(name, S.routes_of(c), rec, ref)
  report(failures)


# ---------------------------------------------------------------- 2. single equals batched
def test_single_entry_gives_the_bits_of_the_batched_record(m, sums, medians, mixed):
  by_name = {**sums, **medians.by_name, **mixed}
  chosen = {}
  for route, names in sorted(S.route_table([c for c, _, _ in by_name.values()]).items()):
    chosen.setdefault(names[0], []).append(route)
  failures = []
  for name, routes in chosen.items():
    c, batched, _ = by_name[name]
    if c.group == "sums":
      t, r = S.sum_pair(c)
      st = f32_stored(t)
    elif c.group == "median":
      t, r, _ = S.median_pair(c)
      st = f32_stored(t)
    else:
      _, r, st = S.mixed_entry(c)
    one = run_single(m, r, st, MEDIAN)
    if record_bytes(one) != record_bytes(batched):          # bytes: a NaN equals the same NaN
      failures.append(f"{name} {routes}: single {one} != batched {batched}")
  report(failures)


# ---------------------------------------------------------------- 3. the four flag combinations
@pytest.mark.parametrize("entry", ["single", "batched"])
def test_flag_combinations(m, sums, entry):
  torch, ops = m.torch, m.ops
  names = ["sum_n24705", "sum_n100"]                        # three chunks and a leaf; one leaf
  assert S.CHUNK * 3 + 129 == 24705
  dev = []
  for name in names:
    t, r = S.sum_pair(sums[name][0])
    dev.append((torch.from_numpy(r).cuda(), ops.CompareTarget(torch.from_numpy(t).cuda(), t.size, "f32")))
  got = {}
  for median in (False, True):
    for kl in (False, True):
      if entry == "batched":
        got[median, kl] = list(ops.compare(dev, median=median, kl=kl))
      else:
        got[median, kl] = [ops.compare([p], median=median, kl=kl)[0] for p in dev]
  for i, name in enumerate(names):
    _, full, ref = sums[name]
    for (median, kl), recs in got.items():
      rec = recs[i]
      for f in ("sum_sq_diff", "sum_ref_sq"):
        assert u32(rec[f]) == u32(full[f]) == u32(ref[f]), (name, median, kl, f)
      for f in F64_FIELDS:
        assert float(rec[f]).hex() == float(full[f]).hex(), (name, median, kl, f)
      if median:
        assert u32(rec["median_lo"]) == u32(ref["median_lo"]) and u32(rec["median_hi"]) == u32(ref["median_hi"])
      else:
        assert u32(rec["median_lo"]) == 0 and u32(rec["median_hi"]) == 0, (name, kl)
      if kl:
        assert u32(rec["sum_kl"]) == u32(full["sum_kl"]) and ref["kl_bound"] > 0, (name, median)
      else:
        assert float(rec["sum_kl"]) == 0.0, (name, median)


# ---------------------------------------------------------------- 4. workspace reuse
def test_a_workspace_is_reused_without_clearing(m, medians):
  """The select kernels leave the histograms clean and reset SelectState: the same batch twice in one workspace, which
  held other bytes before the first call, gives the records of a fresh workspace."""
  table = medians.table
  ws = workspace(m, len(table.table), table.chunks, fill=0xA5)
  first = run_batched(m, table.table, table.chunks, MEDIAN, ws)
  second = run_batched(m, table.table, table.chunks, MEDIAN, ws)
  assert record_bytes(first) == record_bytes(second) == record_bytes(medians.records)
  # and a smaller batch after a larger one, in the same workspace
  sub = table.table[::3].copy()
  chunks = int(sum(-(-int(n) // S.CHUNK) for n in sub["n"]))
  third = run_batched(m, sub, chunks, MEDIAN, ws)
  assert record_bytes(third) == record_bytes(medians.records[::3])


# ---------------------------------------------------------------- 5. the pair that reaches the second combine tile
def test_pair_of_2050_chunks(m):
  c = S.LARGE
  assert "combine_second_tile" in S.routes_of(c)
  t, r = S.sum_pair(c)
  rec = run_single(m, r, f32_stored(t), MEDIAN)
  report(mismatches(c.name, S.routes_of(c), rec, S.reference_record(t, r)))


# ---------------------------------------------------------------- 6. empty entries inside a device table
@pytest.mark.parametrize("c", S.EMPTY_TABLES, ids=[c.name for c in S.EMPTY_TABLES])
def test_empty_entries(m, c):
  entries, refs = [], []
  for slot, n in enumerate(c.lengths):
    if n == 0:
      entries.append((None, None))
      refs.append(None)
    else:
      t, r = S.table_pair(n, slot)
      entries.append((r, f32_stored(t)))
      refs.append(S.reference_record(t, r))
  table = Table(entries)
  assert table.chunks == sum(-(-n // S.CHUNK) for n in c.lengths)
  got = run_batched(m, table.table, table.chunks, MEDIAN)
  live = [i for i, n in enumerate(c.lengths) if n]
  if live:
    dense = run_batched(m, table.table[live].copy(), table.chunks, MEDIAN)
    for j, i in enumerate(live):
      assert record_bytes(got[i]) == record_bytes(dense[j]), (c.name, i)
      report(mismatches(f"{c.name}[{i}]", c.tags, got[i], refs[i]))
  else:
    assert table.chunks == 0
  zero = bytes(m.ops.COMPARE_RESULT_DTYPE.itemsize)
  for i, n in enumerate(c.lengths):
    if n == 0:
      assert record_bytes(got[i]) == zero, (c.name, i, got[i])
  # without the median the empty entries give the same zeros
  plain = run_batched(m, table.table, table.chunks, 0)
  for i, n in enumerate(c.lengths):
    if n == 0:
      assert record_bytes(plain[i]) == zero, (c.name, i, plain[i])
    else:
      assert u32(plain[i]["sum_sq_diff"]) == u32(refs[i]["sum_sq_diff"]), (c.name, i)


# ---------------------------------------------------------------- 7. refused tables
@pytest.fixture(scope="module")
def valid_table(m):
  rng = np.random.default_rng(70_001)
  q = rng.integers(-128, 128, 9000).astype(np.int8)
  scale = rng.uniform(0.01, 0.02, 3).astype(np.float32)
  zp = rng.integers(-5, 6, 3).astype(np.int32)
  tq = S.LE.dequantize(q, scale, zp, 3, 100, 32)
  entries = []
  for slot, n in enumerate((300, S.CHUNK + 1)):
    t, r = S.table_pair(n, 10 + slot)
    entries.append((t, r, f32_stored(t)))
  entries.insert(1, (tq, (tq + rng.standard_normal(9000).astype(np.float32) * np.float32(0.01)).astype(np.float32),
                     {"kind": "i8", "data": q, "scale": scale, "zero_point": zp, "channels": 3, "inner": 100,
                      "diff_bits": 32}))
  table = Table([(r, st) for _, r, st in entries])
  ws = workspace(m, len(entries), table.chunks + 1)          # the larger of every claimed and the true chunk count
  base = run_batched(m, table.table, table.chunks, MEDIAN, ws)
  for i, (t, r, _) in enumerate(entries):
    report(mismatches(f"valid[{i}]", (), base[i], S.reference_record(t, r)))
  return types.SimpleNamespace(table=table, ws=ws, base=base)


@pytest.mark.parametrize("c", S.REFUSALS, ids=[c.name for c in S.REFUSALS])
@pytest.mark.parametrize("flags", [MEDIAN, NO_KL], ids=["median", "sums_only"])
def test_refused_table_gives_nan_and_the_workspace_stays_usable(m, valid_table, c, flags):
  v = valid_table
  table, chunks = v.table.table.copy(), v.table.chunks
  if c.reason == "negative_n":
    table[0]["n"] = -5
    chunks -= 1
  elif c.reason == "kind_9":
    table[0]["kind"] = 9
  elif c.reason == "integer_kind_null_scale":
    table[1]["scale"] = 0
  elif c.reason == "channels_0":
    table[1]["channels"] = 0
  elif c.reason == "diff_bits_12":
    table[1]["diff_bits"] = 12
  elif c.reason == "total_chunks_plus_1":
    chunks += 1
  elif c.reason == "total_chunks_minus_1":
    chunks -= 1
  else:
    raise ValueError(c.reason)
  assert record_bytes(table) != record_bytes(v.table.table) or chunks != v.table.chunks
  got = run_batched(m, table, chunks, flags, v.ws)
  for i, rec in enumerate(got):
    for f in F32_FIELDS + F64_FIELDS:
      assert np.isnan(rec[f]), (c.name, i, f, rec)
  again = run_batched(m, v.table.table, v.table.chunks, MEDIAN, v.ws)
  assert record_bytes(again) == record_bytes(v.base)


# ---------------------------------------------------------------- 8. mixed target kinds in one table
def test_mixed_target_kinds_in_one_table(mixed):
  failures = []
  for name, (c, rec, ref) in mixed.items():
    failures += mismatches(name, S.routes_of(c), rec, ref)
  report(failures)
