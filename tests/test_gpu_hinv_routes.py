"""Every route of the damped Hessian inverse (mi355q_gptq_hinv_f64, mi355q_gptq_hinv_from_product_f32 and their batched
forms; csrc/gptq.hip: hinv_impl, hinv_lockstep, hinv_batched_impl), bit for bit, on Hessians whose inverse has one
correct bit pattern.

The data is hinv_exact_cases.py's: H = L L^T with L = (I + S) D, S nilpotent with small integers, D powers of two, so that
the pivots are powers of four, every Cholesky intermediate an integer and every intermediate of the triangular merge and
of L^-T L^-1 a multiple of 1/16 whose magnitudes add up to less than 2^23 units. No order of additions, no tiling, no
split into bf16 planes can change a bit of such a result, so every route -- the fused step kernel, the three step kernels
of the lock-step batch, the generic potf2 / trsm / GEMM chain, the look-ahead over two streams, FP64 and bf16x3 merge
levels, both product kernels, lock step, lanes -- must return exactly the closed form (L^-1)^T L^-1, in both triangles,
with info == 0. damp_factor is 0 throughout: the damping term is 0 * mean = 0 exactly. What the existing tolerance tests
of test_gpu_gptq.py keep for themselves: non-zero damping, the diag == 0 -> 1 substitution, full-mantissa data, d > 4608.

The case list, the restatement of the host's choices (route) and the proof that the list reaches every route are in
test_hinv_routes_host.py, which needs no GPU. Cases of the default environment run in this process; the library reads
its switches once per process, so every other environment runs its cases in one fresh child process that rebuilds them
from their numbers, compares them itself and prints one line per case.

Pivots that are exactly 0: D[j]^2 taken off H[j, j] makes pivot j of the factorization 0 and leaves the earlier ones
alone, so info must be j + 1 -- through potf2_kernel, chol_step_kernel, potf2_batched_kernel alone and in lock step,
where the other matrices of the batch must still be exact. A column of class 0 has only its diagonal in L, so its pivot
is H[j, j] itself and a zero there is the substitution case above: these cases take columns with j % 3 != 0, which
rules out column 0 and column 63 (first and last columns of later blocks are taken instead).

Single calls go through the raw entry points: 64 guard elements in front of and behind the output, a workspace of
exactly the size the query asks for, pre-filled with 0xA5 and followed by 4096 sentinel bytes, the input untouched."""
import ctypes
import functools
import json
import os
import subprocess
import sys
import types

import pytest

import hinv_exact_cases as X
import test_hinv_routes_host as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                 # float32 elements in front of and behind hinv_out
GUARD_VALUE = -12345.5
WS_FILL = 0xA5
WS_TAIL = 4096
WS_TAIL_FILL = 0x3C
CHILD_TIMEOUT = 300        # seconds; a child takes a few


@functools.lru_cache(maxsize=None)
def modules():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi, ops
  from mi355q import runtime as rt
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), ffi=_ffi)


@pytest.fixture(scope="module")
def m():
  set_here = [s for s in R.SWITCHES if s in os.environ]
  assert not set_here, f"{set_here} change the routes this file restates for its in-process cases"
  return modules()


@functools.lru_cache(maxsize=None)
def truth(d, seed):
  """(H float64, expected H^-1 float32) on the device, from the closed form (float64 torch products of exact integers)."""
  torch = modules().torch
  _, _, h, hinv = X.dense(d, seed, xp=torch, device="cuda")
  want = hinv.to(torch.float32)
  assert torch.equal(want.double(), hinv) and torch.equal(h, h.T)
  return h.contiguous(), want.contiguous()


def alpha_of(seed):
  return 4.0 if seed % 2 == 0 else 0.25


def input_of(c, z):
  """The z-th matrix of a case in the case's form: (tensor, alpha)."""
  torch = modules().torch
  seed = c.seeds[z]
  h = truth(c.d, seed)[0].clone()
  for zz, j in c.bad:
    if zz == z:
      X.zero_pivot(h, c.d, seed, j)
  if c.form == "f64":
    return h, 1.0
  alpha = alpha_of(seed)
  p = (h / alpha).to(torch.float32)
  assert torch.equal(p.double() * alpha, h)
  p[torch.triu(torch.ones((c.d, c.d), dtype=torch.bool, device="cuda"), 1)] = float("nan")   # only the lower triangle is read
  return p.contiguous(), alpha


def difference(got, want, d):
  """'' when the bits agree, else where they do not."""
  torch = modules().torch
  if got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want):
    return ""
  bad = torch.nonzero(~((got == want) | (torch.isnan(got) & torch.isnan(want))))
  tiles = sorted({(int(i) // R.NB, int(j) // R.NB) for i, j in bad[:: max(1, len(bad) // 512)].tolist()})
  first = [(int(i), int(j), float(got[i, j]), float(want[i, j])) for i, j in bad[:4].tolist()]
  return (f"{len(bad)} of {d * d} elements differ, in 64 x 64 tiles {tiles[:12]}{' ...' if len(tiles) > 12 else ''}; "
          f"first (row, column, got, expected): {first}")


def run_single(c):
  """One raw call inside guards and sentinels: '' or what is wrong."""
  mm = modules()
  torch, L, rt = mm.torch, mm.L, mm.rt
  d = c.d
  src, alpha = input_of(c, 0)
  before = src.clone()
  want = truth(d, c.seeds[0])[1]
  need = L.mi355q_gptq_hinv_workspace_bytes(d)
  assert need == R.workspace_bytes(d)
  ws = torch.full((need + WS_TAIL,), WS_FILL, dtype=torch.uint8, device="cuda")
  ws[need:] = WS_TAIL_FILL
  out = torch.full((GUARD + d * d + GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
  info = torch.full((3,), -7, dtype=torch.int32, device="cuda")
  out_ptr = ctypes.c_void_p(out.data_ptr() + GUARD * 4)
  info_ptr = ctypes.c_void_p(info.data_ptr() + 4)
  if c.form == "f64":
    st = L.mi355q_gptq_hinv_f64(rt.ptr(src), d, 0.0, out_ptr, info_ptr, rt.ptr(ws), need, rt.stream_ptr())
  else:
    st = L.mi355q_gptq_hinv_from_product_f32(rt.ptr(src), d, alpha, 0.0, out_ptr, info_ptr, rt.ptr(ws), need, rt.stream_ptr())
  mm.ffi.check(st)
  torch.cuda.synchronize()
  problems = []
  if not (torch.all(out[:GUARD] == GUARD_VALUE) and torch.all(out[GUARD + d * d:] == GUARD_VALUE)):
    problems.append("a guard element beside hinv_out was written")
  if not torch.all(ws[need:] == WS_TAIL_FILL):
    problems.append("bytes behind the workspace were written")
  if info[0].item() != -7 or info[2].item() != -7:
    problems.append("an element beside info_out was written")
  if not torch.equal(before.view(torch.int64 if c.form == "f64" else torch.int32), src.view(torch.int64 if c.form == "f64" else torch.int32)):
    problems.append("the input was written")
  expect_info = c.bad[0][1] + 1 if c.bad else 0
  if info[1].item() != expect_info:
    problems.append(f"info {info[1].item()} instead of {expect_info}")
  if not c.bad:
    diff = difference(out[GUARD:GUARD + d * d].view(d, d), want, d)
    if diff:
      problems.append(diff)
  return "; ".join(problems)


def run_batched(c):
  """ops.gptq_hinv_batched / ops.gptq_hinv_from_product_batched, every matrix against its own truth."""
  mm = modules()
  torch = mm.torch
  inputs = [input_of(c, z) for z in range(c.count)]
  before = [t.clone() for t, _ in inputs]
  if c.form == "f64":
    got = mm.ops.gptq_hinv_batched([t for t, _ in inputs], 0.0)
  else:
    got = mm.ops.gptq_hinv_from_product_batched(inputs, 0.0)
  torch.cuda.synchronize()
  bad = dict(c.bad)
  problems = []
  assert len(got) == c.count
  for z, (hinv, info) in enumerate(got):
    expect_info = bad[z] + 1 if z in bad else 0
    if int(info.item()) != expect_info:
      problems.append(f"matrix {z}: info {int(info.item())} instead of {expect_info}")
    if z not in bad:
      diff = difference(hinv, truth(c.d, c.seeds[z])[1], c.d)
      if diff:
        problems.append(f"matrix {z}: {diff}")
    kind = torch.int64 if c.form == "f64" else torch.int32
    if not torch.equal(before[z].view(kind), inputs[z][0].view(kind)):
      problems.append(f"matrix {z}: the input was written")
  return "; ".join(problems)


def run_case(c):
  return run_batched(c) if c.count else run_single(c)


# ------------------------------------------------------------------------------------- the default environment ---
@pytest.mark.parametrize("c", R.DEFAULT_CASES, ids=R.case_id)
def test_route_returns_the_closed_form(m, c):
  """Both triangles torch.equal to (L^-1)^T L^-1, info == 0 (or j + 1 for a pivot that is exactly 0, the other matrices
  of the batch still exact), guards, sentinels and inputs intact."""
  assert not c.env
  problems = run_case(c)
  assert not problems, f"{R.case_id(c)}: {problems}"


# ----------------------------------------------------------------------------------------- the other environments ---
_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/ai-edge-quantizer_amd"); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_hinv_routes as G
G.child_main(json.loads(sys.argv[2]))
"""


def child_main(indices):
  """Runs ENV_CASES[i] for every i (all of one environment, which must be this process's) and prints one line each. A
  failed HIP call raises: the process ends there, with a status that is not 0."""
  for i in indices:
    c = R.ENV_CASES[i]
    for k in R.SWITCHES:
      assert os.environ.get(k) == c.envd.get(k), (k, os.environ.get(k), c.envd.get(k))
    problems = run_case(c)
    print(f"CASE {i} {'equal' if not problems else 'DIFFERENT: ' + problems}", flush=True)


ENVIRONMENTS = []
for _c in R.ENV_CASES:
  if _c.env not in ENVIRONMENTS:
    ENVIRONMENTS.append(_c.env)


@pytest.mark.parametrize("env", ENVIRONMENTS, ids=lambda e: " ".join(f"{k}={v}" for k, v in e))
def test_switch_route_returns_the_closed_form(m, env):
  """One child process per environment; its cases (ENV_CASES of test_hinv_routes_host.py) carry their routes in their ids."""
  indices = [i for i, c in enumerate(R.ENV_CASES) if c.env == env]
  child_env = {k: v for k, v in os.environ.items() if k not in R.SWITCHES}
  child_env.update(dict(env))
  out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(indices)], env=child_env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
  assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
  lines = [ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")]
  assert len(lines) == len(indices), out.stdout[-2000:]
  for i, ln in zip(indices, lines):
    assert ln == f"CASE {i} equal", f"{R.case_id(R.ENV_CASES[i])}: {ln}"
