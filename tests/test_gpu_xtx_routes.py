"""Every route of the Hessian product X^T X (mi355q_gptq_xtx_accum_f32, mi355q_gptq_xtx_f32, mi355q_gptq_xtx_finish_f64;
csrc/gptq.hip: xtx_product, mirror_scale_to_f64_kernel; csrc/xtx_bf16x3.hip; csrc/xtx_f16x2.hip), bit for bit, on
activations whose product has one correct bit pattern.

The data is xtx_exact_cases.py's: every product any route adds is a whole number of quanta and the magnitudes of all of
them stay below 2^24 quanta, so no K range, split-K slice, fold, accumulator, slab, reduce kernel or accumulating call
can change a bit of the result. `dense` cases (small integers, a few entries of magnitude 257) must return the exact
integer product; `planes3` / `planes2` cases (a few live tokens on the boundaries the kernels have, values that fill all
three bf16 / both f16 planes) must return the kernel's DEFINITION -- the six / three kept products -- which differs from
the float32-rounded exact product in a few per cent of the entries. What the tolerance tests of test_gpu_gptq.py keep for
themselves: full-mantissa accuracy, 30 to 80 binades, non-finite activations, d = 8192.

The case list, the restatement of the host's choices (route) and the proofs about the data are in
test_xtx_routes_host.py, which needs no GPU. Cases of the default environment and of MI355Q_XTX_F16X2 = 1 (read per
call) run in this process; the library reads its other switches once per process, so every other environment runs its
cases in one fresh child process that rebuilds them from their numbers, compares them itself and prints one line per case.

A case goes through the raw entry points: 64 guard elements in front of and behind the product, which is pre-filled with
NaN (an initial product: its lower triangle, NaN above the diagonal -- only the lower triangle is read), a workspace of
exactly the size the query asks for, pre-filled with 0xA5 and followed by 4096 sentinel bytes, X untouched. The lower
triangle must equal the model bit for bit; an entry above the diagonal holds either the pre-fill or the correct symmetric
value (the 128 x 128 tiles on the diagonal are written whole, the 128 x 256 kernels write 128 columns more). Only a
sequence that changes between the FP32 GEMM and a split kernel is held to less there: the two cover different parts of
the diagonal tiles' upper halves, so such an entry holds the correct values of the first call and of any of the later
ones -- still nothing but whole, correct contributions. Single calls
then go through mi355q_gptq_xtx_f32, and through mi355q_gptq_xtx_finish_f64 on the model with NaN above the diagonal:
both must be alpha * float64(model) in both triangles -- one IEEE multiply, exact for any alpha."""
import contextlib
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys
import types

import pytest

import test_xtx_routes_host as R
import xtx_exact_cases as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                 # elements in front of and behind an output
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
  from mi355q.algorithms.uniform_quantize import gptq
  return types.SimpleNamespace(torch=torch, ops=ops, rt=rt, L=_ffi.lib(), ffi=_ffi, gptq=gptq)


@pytest.fixture(scope="module")
def m():
  set_here = [s for s in R.SWITCHES if s in os.environ]
  assert not set_here, f"{set_here} change the routes this file restates for its in-process cases"
  return modules()


@contextlib.contextmanager
def per_call_switches(c):
  """MI355Q_XTX_F16X2 of an in-process case, for the length of its calls (a child's environment already holds its switches)."""
  if c.in_process and c.env:
    with modules().ops.hessian_product("fast"):
      yield
  else:
    yield


def alpha_of(n):
  return 2.0 / (n if n & (n - 1) else n + 1)       # never a power of two


def inputs_of(c):
  torch = modules().torch
  return [X.call_x(n, c.d, c.seed + i, c.kind, xp=torch, device="cuda").contiguous() for i, n in enumerate(c.calls)]


def model_of(c, xs):
  """(float64 model of the whole sequence, the same in float32, the float64 models of the single calls) on the device."""
  torch = modules().torch
  total = X.initial_product(c.d, c.seed, xp=torch, device="cuda") if c.initial else torch.zeros((c.d, c.d), dtype=torch.float64, device="cuda")
  parts = []
  for i, (n, x) in enumerate(zip(c.calls, xs)):
    if c.kind == "dense":
      x64 = x.double()
      parts.append(x64.T @ x64)                   # exact: integers far below 2^53
    else:
      parts.append(X.planes_model(n, c.d, c.seed + i, c.kind, xp=torch, device="cuda"))
    total = total + parts[-1]
  want = total.to(torch.float32)
  assert torch.equal(want.double(), total) and torch.equal(total, total.T)
  return total, want, parts


def difference(got, want, d, where=None):
  """'' when the bits agree (inside `where`), else where they do not."""
  torch = modules().torch
  same = got.view(torch.int32 if got.dtype == torch.float32 else torch.int64) == want.view(torch.int32 if want.dtype == torch.float32 else torch.int64)
  if where is not None:
    same = same | ~where
  if bool(same.all()):
    return ""
  bad = torch.nonzero(~same)
  tiles = sorted({(int(i) // R.TILE, int(j) // R.TILE) for i, j in bad[:: max(1, len(bad) // 512)].tolist()})
  first = [(int(i), int(j), float(got[i, j]), float(want[i, j])) for i, j in bad[:4].tolist()]
  return (f"{len(bad)} of {d * d} elements differ, in 128 x 128 tiles {tiles[:12]}{' ...' if len(tiles) > 12 else ''}; "
          f"first (row, column, got, expected): {first}")


def guarded(count, dtype):
  torch = modules().torch
  buf = torch.full((GUARD + count + GUARD,), GUARD_VALUE, dtype=dtype, device="cuda")
  return buf, ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def guards_intact(buf, count):
  torch = modules().torch
  return bool(torch.all(buf[:GUARD] == GUARD_VALUE) and torch.all(buf[GUARD + count:] == GUARD_VALUE))


def workspace(need):
  torch = modules().torch
  ws = torch.full((need + WS_TAIL,), WS_FILL, dtype=torch.uint8, device="cuda")
  ws[need:] = WS_TAIL_FILL
  return ws


def run_case(c):
  """The calls of a case inside guards and sentinels, then (single calls) the two Hessian entry points: '' or what is wrong."""
  mm = modules()
  torch, L, rt = mm.torch, mm.L, mm.rt
  d = c.d
  problems = []
  with per_call_switches(c):
    xs = inputs_of(c)
    total, want, parts = model_of(c, xs)
    lower = torch.tril(torch.ones((d, d), dtype=torch.bool, device="cuda"))
    out, out_ptr = guarded(d * d, torch.float32)
    prod = out[GUARD:GUARD + d * d].view(d, d)
    prod.fill_(float("nan"))
    if c.initial:
      prod[lower] = X.initial_product(d, c.seed, xp=torch, device="cuda").to(torch.float32)[lower]
    for i, (n, x) in enumerate(zip(c.calls, xs)):
      before = x.clone()
      need = L.mi355q_gptq_xtx_accum_workspace_bytes(n, d)
      ws = workspace(need)
      mm.ffi.check(L.mi355q_gptq_xtx_accum_f32(rt.ptr(x), n, d, out_ptr, 1 if (c.initial or i > 0) else 0, rt.ptr(ws), need, rt.stream_ptr()))
      torch.cuda.synchronize()
      if not torch.all(ws[need:] == WS_TAIL_FILL):
        problems.append(f"call {i}: bytes behind the workspace were written")
      if not torch.equal(before.view(torch.int32), x.view(torch.int32)):
        problems.append(f"call {i}: X was written")
      del ws, before
    if not guards_intact(out, d * d):
      problems.append("a guard element beside the product was written")
    diff = difference(prod, want, d, lower)
    if diff:
      problems.append("product, lower triangle: " + diff)
    allowed = torch.isnan(prod) | (prod.view(torch.int32) == want.view(torch.int32))
    if len({r["family"] for r in R.routes_of(c)}) > 1:
      # the FP32 GEMM and the split kernels cover different parts of the diagonal tiles' upper halves: an entry there holds
      # the first call's value plus those of any of the later calls (NaN once a call has accumulated onto the pre-fill)
      assert not c.initial
      for subset in range(1 << (len(parts) - 1)):
        some = parts[0] + sum((p for i, p in enumerate(parts[1:]) if subset >> i & 1), torch.zeros_like(parts[0]))
        allowed |= prod.view(torch.int32) == some.to(torch.float32).view(torch.int32)
    stray = ~lower & ~allowed
    if bool(stray.any()):
      problems.append("product above the diagonal, neither the pre-fill nor the symmetric value: " + difference(prod, want, d, stray))
    if len(c.calls) == 1 and not c.initial:
      n, x = c.calls[0], xs[0]
      alpha = alpha_of(n)
      expect = alpha * total                        # one IEEE multiply per entry
      need = L.mi355q_gptq_xtx_workspace_bytes(n, d)
      ws = workspace(need)
      h, h_ptr = guarded(d * d, torch.float64)
      mm.ffi.check(L.mi355q_gptq_xtx_f32(rt.ptr(x), n, d, alpha, h_ptr, rt.ptr(ws), need, rt.stream_ptr()))
      torch.cuda.synchronize()
      if not (guards_intact(h, d * d) and torch.all(ws[need:] == WS_TAIL_FILL)):
        problems.append("xtx_f32: a guard element or bytes behind the workspace were written")
      diff = difference(h[GUARD:GUARD + d * d].view(d, d), expect, d)
      if diff:
        problems.append("xtx_f32: " + diff)
      del ws
      src = want.clone()
      src[~lower] = float("nan")                    # only the lower triangle is read
      h.fill_(GUARD_VALUE)
      mm.ffi.check(L.mi355q_gptq_xtx_finish_f64(rt.ptr(src), d, alpha, h_ptr, rt.stream_ptr()))
      torch.cuda.synchronize()
      if not guards_intact(h, d * d):
        problems.append("xtx_finish_f64: a guard element was written")
      diff = difference(h[GUARD:GUARD + d * d].view(d, d), expect, d)
      if diff:
        problems.append("xtx_finish_f64: " + diff)
  return "; ".join(problems)


# ------------------------------------------------------------------------------------- the in-process environments ---
@pytest.mark.parametrize("c", R.DEFAULT_CASES, ids=R.case_id)
def test_route_returns_the_model(m, c):
  """Lower triangle bit-equal to the model, above the diagonal the pre-fill or the symmetric value, guards, sentinels and
  X intact; the Hessian entry points alpha * float64(model) in both triangles."""
  assert c.in_process
  problems = run_case(c)
  assert not problems, f"{R.case_id(c)}: {problems}"


# ----------------------------------------------------------------------------------------- the other environments ---
def full_mantissa_digest():
  """sha256 of the lower triangle of the product of one dense full-mantissa tensor (R.SAME_BITS_SHAPE) on this process's route."""
  mm = modules()
  torch = mm.torch
  d, n = R.SAME_BITS_SHAPE
  gen = torch.Generator(device="cuda").manual_seed(4096)
  x = torch.randn((n, d), generator=gen, device="cuda", dtype=torch.float32)
  prod = torch.tril(mm.ops.gptq_xtx_accum(x, None))
  assert bool(torch.isfinite(prod).all()) and float(prod.diagonal().min()) > 0
  return hashlib.sha256(prod.cpu().numpy().tobytes()).hexdigest()


_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/ai-edge-quantizer_amd"); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_xtx_routes as G
G.child_main(json.loads(sys.argv[2]), sys.argv[3] == "1")
"""


def child_main(indices, digest):
  """Runs ENV_CASES[i] for every i (all of one environment, which must be this process's) and prints one line each. A
  failed HIP call raises: the process ends there, with a status that is not 0."""
  for i in indices:
    c = R.ENV_CASES[i]
    for k in R.SWITCHES:
      assert os.environ.get(k) == c.envd.get(k), (k, os.environ.get(k), c.envd.get(k))
    problems = run_case(c)
    print(f"CASE {i} {'equal' if not problems else 'DIFFERENT: ' + problems}", flush=True)
  if digest:
    print(f"FULL {full_mantissa_digest()}", flush=True)


ENVIRONMENTS = []
for _c in R.ENV_CASES:
  if _c.env not in ENVIRONMENTS:
    ENVIRONMENTS.append(_c.env)


@pytest.mark.parametrize("env", ENVIRONMENTS, ids=lambda e: " ".join(f"{k}={v}" for k, v in e))
def test_switch_route_returns_the_model(m, env):
  """One child process per environment; its cases (ENV_CASES of test_xtx_routes_host.py) carry their routes in their ids.
  Where xtx_bf16x3.hip states that a kernel adds the same products in the same order as the default one (narrow, wide,
  deep<0>, deep<2> at d = 4096; splits = 1 throughout), the child's product of one dense full-mantissa tensor has the bits
  of this process's (deep<1>)."""
  indices = [i for i, c in enumerate(R.ENV_CASES) if c.env == env]
  same_bits = env in R.SAME_BITS_ENVS
  child_env = {k: v for k, v in os.environ.items() if k not in R.SWITCHES}
  child_env.update(dict(env))
  out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(indices), "1" if same_bits else "0"], env=child_env,
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
  assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
  lines = [ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")]
  assert len(lines) == len(indices), out.stdout[-2000:]
  for i, ln in zip(indices, lines):
    assert ln == f"CASE {i} equal", f"{R.case_id(R.ENV_CASES[i])}: {ln}"
  if same_bits:
    full = [ln for ln in out.stdout.splitlines() if ln.startswith("FULL ")]
    assert full == [f"FULL {full_mantissa_digest()}"], "a dense full-mantissa product differs from the default route's"


# --------------------------------------------------------------------------------------------------- the Python path ---
def test_ops_accumulate_and_finish(m):
  """ops.gptq_xtx_accum / ops.gptq_xtx_finish over a split kernel, the FP32 GEMM (a short batch) and a split kernel with
  splits > 1, for both split kernels, against the model of the whole sequence."""
  torch = m.torch
  for env in ((), R.FAST):
    c = R.Case(256, (1024, 500, 4096), "dense", env, seed=5)
    with per_call_switches(c):
      xs = inputs_of(c)
      total, want, _ = model_of(c, xs)
      prod = None
      for x in xs:
        prod = m.ops.gptq_xtx_accum(x, prod)
      alpha = alpha_of(c.tokens)
      h = m.ops.gptq_xtx_finish(prod, alpha)
      torch.cuda.synchronize()
    lower = torch.tril(torch.ones((c.d, c.d), dtype=torch.bool, device="cuda"))
    assert not difference(prod, want, c.d, lower), difference(prod, want, c.d, lower)
    assert not difference(h, alpha * total, c.d), difference(h, alpha * total, c.d)


def test_hessian_accumulator_with_a_short_last_batch(m):
  """HessianAccumulator: a batch of a slab's size is multiplied where it lies (split kernel, two ... 16 partials through the
  reduce kernel), the short last one waits in the slab and joins through the FP32 GEMM with accumulate."""
  torch = m.torch
  c = R.Case(256, (X.SLAB, 500), "dense", seed=9)
  assert [r["family"] for r in R.routes_of(c)] == ["bf16x3", "fp32"]
  xs = inputs_of(c)
  total, _, _ = model_of(c, xs)
  acc = m.gptq.HessianAccumulator(c.d)
  assert acc.SLAB_TOKENS == X.SLAB
  acc.add(xs[0], 2.0)
  acc.add(xs[1], 1.0)
  h = acc.device_tensor
  torch.cuda.synchronize()
  expect = (2.0 / 3.0) * total
  assert not difference(h, expect, c.d), difference(h, expect, c.d)
