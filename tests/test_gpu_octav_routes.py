"""Every route of the OCTAV clip search (csrc/octav.hip: mi355q_octav_clip_f32, mi355q_octav_clip_fast_f32,
mi355q_octav_clip_nd_f32), iterate by iterate and bit for bit against NumPy.

OCTAV is a fixed-point iteration: once the masks settle, the last masks alone determine the result, and an early iterate
that is off by up to 3 % leaves the final constant unchanged in 99 % of the runs
(test_octav_route_cases_host.py::test_final_constant_hides_a_perturbed_iterate). The iterations in which the kernels work
hardest -- guess 0 with every element selected, the dense / sparse choice per piece, the hand-over to the tail -- are the
early ones. So every case is called with early_stop = 0 and max_iter = k for every k up to its max_iter and must return
the reference's k-th iterate: the public contract and nothing else, and since the rows kernel hands over only while
it + 2 < max_iter, the hand-over point moves with k.

The cases, the restatement of the host's choices (route) and of the kernels' data-dependent branches (paths), and the
proof that the list reaches all of them are in octav_route_cases.py and test_octav_route_cases_host.py, which need no
GPU. Calls go through the C ABI, so that the test decides the workspace size (the rows kernel with and without the room
for its tail) and the alignment of x (16 bytes, or 4 bytes off). Around every call: guard floats on both sides of
clip_out, an int on each side of iters_out, a workspace of exactly the size asked for followed by sentinel bytes, the
input compared afterwards. There are no tolerances here: every comparison is on bits (NaN equal to NaN).

The library reads its switches once per process: every other environment runs its cases in one fresh child process that
rebuilds them from their numbers, compares them itself and prints one line per case. Children run one after another;
after one that ended on a signal, with status 134 / 139 or at its time limit, no further child is started."""
import ctypes
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import octav_route_cases as C
from oracle import aeq_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 64                 # float32 elements in front of and behind clip_out
GUARD_VALUE = -12345.5
WS_FILL = 0xA5
WS_TAIL = 4096
WS_TAIL_FILL = 0x3C
X_PAD = 8                  # floats in front of and behind x
X_PAD_VALUE = 7.0e3        # (selected by every guess: a kernel that read outside the unit would show it)
CHILD_TIMEOUT = 300        # seconds; a child takes a few


@functools.lru_cache(maxsize=None)
def modules():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  from mi355q import runtime as rt
  rt.require_gpu()
  return types.SimpleNamespace(torch=torch, rt=rt, L=_ffi.lib(), ffi=_ffi)


@pytest.fixture(scope="module")
def m():
  set_here = [s for s in C.SWITCHES if s in os.environ]
  assert not set_here, f"{set_here} change the routes this file restates for its in-process cases"
  return modules()


def same_bits(a, b):
  a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
  return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def where_different(got, want):
  got, want = np.asarray(got, F).reshape(-1), np.asarray(want, F).reshape(-1)
  bad = np.flatnonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
  return f"{len(bad)} of {len(want)} units differ; first (unit, got, expected): {[(int(u), float(got[u]), float(want[u])) for u in bad[:4]]}"


class Input:
  """A case's tensor on the device inside a padded buffer, 16-byte aligned or four bytes off."""

  def __init__(self, x, aligned):
    torch = modules().torch
    flat = np.ascontiguousarray(x, F).reshape(-1)
    lead = X_PAD if aligned else X_PAD + 1
    host = np.full(lead + flat.size + X_PAD, X_PAD_VALUE, F)
    host[lead:lead + flat.size] = flat
    self.host = host
    self.buffer = torch.from_numpy(host).cuda()
    self.address = self.buffer.data_ptr() + 4 * lead
    assert self.buffer.data_ptr() % 16 == 0 and (self.address % 16 == 0) == aligned

  def unchanged(self):
    return bool((self.buffer.cpu().numpy().view(np.uint32) == self.host.view(np.uint32)).all())


def call(c, inp, entry, max_iter, early_stop):
  """One raw call inside guards and sentinels: (clip, iterations, what else is wrong)."""
  mm = modules()
  torch, L, rt = mm.torch, mm.L, mm.rt
  base = L.mi355q_octav_workspace_bytes(c.units, max_iter)
  assert base == C.workspace_bytes(c.units, max_iter)
  need = base
  if entry != "fast" and c.workspace == "rows" and c.outer == 1:
    need = L.mi355q_octav_rows_workspace_bytes(c.units, c.unit_len, max_iter)
    assert need == C.rows_workspace_bytes(c.units, c.unit_len, max_iter, c.env)
  ws = torch.full((need + WS_TAIL,), WS_FILL, dtype=torch.uint8, device="cuda")
  ws[need:] = WS_TAIL_FILL
  out = torch.full((GUARD + c.units + GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
  iters = torch.full((3,), -7, dtype=torch.int32, device="cuda")
  x_ptr = ctypes.c_void_p(inp.address)
  out_ptr = ctypes.c_void_p(out.data_ptr() + GUARD * 4)
  iters_ptr = ctypes.c_void_p(iters.data_ptr() + 4)
  tail = (out_ptr, iters_ptr, rt.ptr(ws), need, rt.stream_ptr())
  if entry == "nd":
    st = L.mi355q_octav_clip_nd_f32(x_ptr, c.outer, c.units, c.unit_len, c.bits, max_iter, F(C.DIVISOR), early_stop, *tail)
  elif entry == "fast":
    st = L.mi355q_octav_clip_fast_f32(x_ptr, c.units, c.unit_len, c.bits, max_iter, F(C.DIVISOR), early_stop, *tail)
  else:
    st = L.mi355q_octav_clip_f32(x_ptr, c.units, c.unit_len, c.bits, max_iter, F(C.DIVISOR), early_stop, c.f64, *tail)
  mm.ffi.check(st)
  torch.cuda.synchronize()
  problems = []
  if not (torch.all(out[:GUARD] == GUARD_VALUE) and torch.all(out[GUARD + c.units:] == GUARD_VALUE)):
    problems.append("a guard element beside clip_out was written")
  if iters[0].item() != -7 or iters[2].item() != -7:
    problems.append("an element beside iters_out was written")
  if not torch.all(ws[need:] == WS_TAIL_FILL):
    problems.append("bytes behind the workspace were written")
  return out[GUARD:GUARD + c.units].cpu().numpy(), int(iters[1].item()), problems


def early_stop_oracle(c):
  """(clip, iterations) of the reference with its early stop, or None where there is no such oracle (several units with
  axis=None semantics: the reference has one tensor there)."""
  x = C.data(c)
  with np.errstate(all="ignore"):
    if c.entry == "nd" and c.outer > 1:
      clip, iters = O.octav_clip(x, c.bits, (0, 2), c.max_iter, C.DIVISOR, early_stop=True, return_iters=True)
    elif c.f64:
      clip, iters = O.octav_clip(x.reshape(c.units, c.unit_len), c.bits, (1,), c.max_iter, C.DIVISOR, early_stop=True, return_iters=True)
    elif c.units == 1:
      clip, iters = O.octav_clip(x.reshape(-1), c.bits, None, c.max_iter, C.DIVISOR, early_stop=True, return_iters=True)
    else:
      return None
  return np.asarray(clip, F).reshape(-1), iters


def run_case(c, entries=None):
  """Every iterate, the early stop, the guards, the input: '' or what is wrong."""
  want = C.case_iterates(c)
  inp = Input(C.data(c), c.aligned)
  problems = []
  for entry in entries or (c.entry,):
    for k in range(1, c.max_iter + 1):
      got, iters, wrong = call(c, inp, entry, k, 0)
      problems += [f"{entry} max_iter {k}: {w}" for w in wrong]
      if iters != k:
        problems.append(f"{entry} max_iter {k}: iters_out {iters}")
      if not same_bits(got, want[k - 1]):
        problems.append(f"{entry} iterate {k} of {c.max_iter}: {where_different(got, want[k - 1])}")
    ref = early_stop_oracle(c)
    if ref is not None:
      got, iters, wrong = call(c, inp, entry, c.max_iter, 1)
      problems += [f"{entry} early stop: {w}" for w in wrong]
      if iters != ref[1]:
        problems.append(f"{entry} early stop: {iters} iterations instead of {ref[1]}")
      if not same_bits(got, ref[0]):
        problems.append(f"{entry} early stop: {where_different(got, ref[0])}")
  if not inp.unchanged():
    problems.append("the input or its surroundings were written")
  return "; ".join(problems[:6])


# ------------------------------------------------------------------------------------- the default environment ---
@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_route_returns_every_iterate(m, c):
  """max_iter = 1 .. the case's, early stop off: the reference's k-th iterate of every unit and iters_out == k; then the
  early stop: the reference's constant and iteration count."""
  assert not c.env
  problems = run_case(c)
  assert not problems, f"{C.case_id(c)}: {problems}"


@pytest.mark.parametrize("c", C.EXACT, ids=C.case_id)
def test_one_read_kernel_returns_numpys_bits_on_exact_inputs(m, c):
  """Inputs whose float32 partial sums are exact in any order: the one-read kernel and the exact entry (whatever route it
  takes at this length) both return every iterate of the reference, and the same iteration count."""
  problems = run_case(c, ("fast", "exact"))
  assert not problems, f"{C.case_id(c)} / {'+'.join(C.route('exact', c.units, c.unit_len))}: {problems}"


def variants():
  """The rows-kernel cases that share their data: rows workspace, base workspace, x four bytes off."""
  groups = {}
  for c in C.CASES:
    if c.entry == "exact" and C.case_route(c)[0].startswith("rows") and c.kind == "mix":
      groups.setdefault((c.units, c.unit_len, c.seed, c.bits, c.max_iter, c.f64), []).append(c)
  return [g for g in groups.values() if len(g) == 3]


@pytest.mark.parametrize("group", variants(), ids=lambda g: f"{g[0].units}x{g[0].unit_len}")
def test_rows_kernel_returns_the_same_bits_with_and_without_tail_and_alignment(m, group):
  assert {(c.workspace, c.aligned) for c in group} == {("rows", True), ("base", True), ("rows", False)}
  assert {C.case_route(c)[1] for c in group} == {"tail", "no-tail"}
  results = []
  for c in group:
    inp = Input(C.data(c), c.aligned)
    for early in (0, 1):
      got, iters, wrong = call(c, inp, "exact", c.max_iter, early)
      assert not wrong, (C.case_id(c), wrong)
      results.append((early, got, iters))
  for early, got, iters in results:
    first = next(r for r in results if r[0] == early)
    assert same_bits(got, first[1]) and iters == first[2]


# ----------------------------------------------------------------------------------------- the other environments ---
_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/ai-edge-quantizer_amd"); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_octav_routes as G
G.child_main(json.loads(sys.argv[2]))
"""


def child_main(indices):
  """Runs ENV_CASES[i] for every i (all of one environment, which must be this process's) and prints one line each. A
  failed HIP call raises: the process ends there, with a status that is not 0."""
  for i in indices:
    c = C.ENV_CASES[i]
    for k in C.SWITCHES:
      assert os.environ.get(k) == c.envd.get(k), (k, os.environ.get(k), c.envd.get(k))
    problems = run_case(c)
    print(f"CASE {i} {'equal' if not problems else 'DIFFERENT: ' + problems}", flush=True)


ENVIRONMENTS = []
for _c in C.ENV_CASES:
  if _c.env not in ENVIRONMENTS:
    ENVIRONMENTS.append(_c.env)
_child_trouble = []      # a child that ended on a signal, aborted or ran into its time limit: nothing more is started


@pytest.mark.parametrize("env", ENVIRONMENTS, ids=lambda e: " ".join(f"{k}={v}" for k, v in e))
def test_switch_route_returns_every_iterate(m, env):
  """One child process per environment; its cases (ENV_CASES of octav_route_cases.py) carry their routes in their ids."""
  assert not _child_trouble, f"not started: an earlier child ended badly ({_child_trouble[0]})"
  indices = [i for i, c in enumerate(C.ENV_CASES) if c.env == env]
  child_env = {k: v for k, v in os.environ.items() if k not in C.SWITCHES}
  child_env.update(dict(env))
  try:
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(indices)], env=child_env, capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT)
  except subprocess.TimeoutExpired as e:
    _child_trouble.append(f"{dict(env)}: time limit")
    raise AssertionError(f"the child ran into its time limit of {CHILD_TIMEOUT} s: {(e.stdout or b'')[-2000:]}")
  if out.returncode < 0 or out.returncode in (134, 139):
    _child_trouble.append(f"{dict(env)}: status {out.returncode}")
  assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
  lines = [ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")]
  assert len(lines) == len(indices), out.stdout[-2000:]
  for i, ln in zip(indices, lines):
    assert ln == f"CASE {i} equal", f"{C.case_id(C.ENV_CASES[i])}: {ln}"
