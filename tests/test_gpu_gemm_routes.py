"""Every launch route of the strided MFMA GEMM (csrc/gemm.hip) through mi355q_gemm_ex_f32 / _f64, against exact integer
products: the six tile configurations with each pair of 16-byte load modes, the generic kernel, the four k_modes with
every form of lower_only, split-K on both kernels, batch / outer / c32.

Which kernel a call reaches is decided on the host (launch_gemm(), launch_with(), pick_mode()); route() below restates
that choice and every case carries the route it is there for in its id. Operands are integers in [-8, 8], so every
partial sum is an integer below 2^24 and the result has ONE correct bit pattern whatever the order of the additions:
a tile that is not computed, computed twice, computed from the wrong K range or written to the wrong place differs from
beta*C0 + alpha*(A @ B) in at least one element. Operands sit in NaN-filled buffers (a read outside the operand shows
in the result), C is a view with gaps into a pre-filled buffer with guard elements around it, and the whole buffer is
compared bit for bit: what the call must not write has to keep its bits.

The tests that need a GPU are marked one by one; the route table, the argument checks of the entry points and the 2^24
bound of the data are checked without one."""
import ctypes
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                      # elements in front of and behind C that no kernel may touch
ALPHAS = (1.0, -1.0, 0.5, 3.0)
BETAS = (0.0, 1.0, -2.0)
NP = {"f32": np.float32, "f64": np.float64}
BITS = {"f32": np.uint32, "f64": np.uint64}
FILL = {"f32": np.array([0xFFC12345], np.uint32).view(np.float32)[0],         # a NaN with a payload: what C, its gaps
        "f64": np.array([0xFFF8000000012345], np.uint64).view(np.float64)[0]}  # and guards hold before a call
VEC = {"f32": 4, "f64": 2}      # elements per 16-byte load
UNIT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}


def env_is_default():
  """The launcher reads these once per process; route() restates their defaults."""
  return "MI355Q_K32_MAX_TILES" not in os.environ and "MI355Q_NO_F32_K64" not in os.environ


@functools.lru_cache(maxsize=None)
def library():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  return _ffi.lib()


@pytest.fixture(scope="module")
def lib():
  return library()


@pytest.fixture(scope="module")
def m():
  import torch
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  assert env_is_default(), "MI355Q_K32_MAX_TILES / MI355Q_NO_F32_K64 change the routes this file restates"
  import types
  L = library()
  from mi355q import _ffi
  from mi355q import runtime as rt
  return types.SimpleNamespace(torch=torch, rt=rt, L=L, ffi=_ffi)


# ------------------------------------------------------------------------------------------------------- the routes ---
TILES = {"Tile<float>": (128, 16), "TileF32Small": (64, 64), "TileF32K64": (128, 64),       # name -> (BM, BK)
         "Tile<double>": (64, 16), "TileF64K32": (64, 32), "TileF64Big": (128, 16)}
TILES_OF = {"f32": ("Tile<float>", "TileF32Small", "TileF32K64"), "f64": ("Tile<double>", "TileF64K32", "TileF64Big")}


@functools.lru_cache(maxsize=None)
def slices(dtype, M, N, K, lower_only):
  """K slices of a split product, from the library's own workspace query (1 = never split)."""
  L = library()
  fn = L.mi355q_gemm_splitk_workspace_bytes_f32 if dtype == "f32" else L.mi355q_gemm_splitk_workspace_bytes_f64
  nbytes = fn(M, N, K, lower_only)
  per_slice = M * N * np.dtype(NP[dtype]).itemsize
  assert nbytes % per_slice == 0
  return nbytes // per_slice if nbytes else 1


def pick_mode(dtype, s_m, s_k, aligned):
  """pick_mode() of csrc/gemm.hip: M = 16-byte loads along the non-k index, K = along k, G = scalar loads."""
  if aligned and s_m == 1 and s_k % VEC[dtype] == 0:
    return "M"
  if aligned and s_k == 1 and s_m % VEC[dtype] == 0:
    return "K"
  return "G"


def route(dtype, M, N, K, a_strides, b_strides, a_aligned, b_aligned, lower_only, k_mode, batch, have_ws, outer=0,
          c32=False, ws_enough=True, count=slices):
  """launch_gemm() and launch_with() restated: (tile, kernel, a_mode, b_mode, grid_kind, slices > 1).
  a_strides = (a_i, a_k), b_strides = (b_k, b_j); have_ws: a split-K workspace pointer is passed (ws_enough: of the
  size the query asks for); count: where the number of slices comes from (the library's query)."""
  a_mode = pick_mode(dtype, a_strides[0], a_strides[1], a_aligned)
  b_mode = pick_mode(dtype, b_strides[1], b_strides[0], b_aligned)
  fast_modes = a_mode != "G" and b_mode != "G"
  nb = max(batch, 1)

  def up(x, b):
    return -(-x // b)

  def with_tile(tile, ws):
    bm, bk = TILES[tile]
    if batch > 1 or outer > 1 or c32:
      ws = False
    nsl = count(dtype, M, N, K, lower_only) if (ws and ws_enough and k_mode == 0) else 1
    if not (M % bm == 0 and N % bm == 0 and K % bk == 0 and fast_modes):
      return (tile, "generic", a_mode, b_mode, "square", nsl > 1)
    if lower_only == 1 and M == N:
      grid = "triangular"
    elif k_mode == 3 and lower_only == 0:
      grid = "columns"
    elif k_mode == 1:
      grid = "rows_reversed"
    else:
      grid = "square"
    return (tile, "big" if tile == "TileF64Big" else "fast", a_mode, b_mode, grid, nsl > 1)

  if dtype == "f64":
    tiles128 = up(M, 128) * up(N, 128)
    splitk = have_ws and k_mode == 0 and not c32 and count(dtype, M, N, K, lower_only) > 1
    whole128 = M % 128 == 0 and N % 128 == 0 and K % 16 == 0 and fast_modes
    if tiles128 >= 256 and not splitk and whole128 and K >= 256 and (not lower_only or tiles128 >= 1024):
      return with_tile("TileF64Big", False)
    tiles64 = up(M, 64) * up(N, 64) * nb
    if ((k_mode in (1, 3) or (k_mode == 0 and lower_only)) and tiles64 <= 512 and M % 64 == 0 and N % 64 == 0 and
        K % 32 == 0 and K >= 128 and fast_modes):
      return with_tile("TileF64K32", False)
    return with_tile("Tile<double>", have_ws)
  tiles128 = up(M, 128) * up(N, 128) * nb
  short_k = k_mode == 0 and not lower_only and K % 64 == 0 and 128 <= K <= 1024 and fast_modes
  if short_k and tiles128 <= 256 and M % 64 == 0 and N % 64 == 0:
    return with_tile("TileF32Small", False)
  if short_k and tiles128 <= 512 and M % 128 == 0 and N % 128 == 0:
    return with_tile("TileF32K64", False)
  return with_tile("Tile<float>", have_ws)


# -------------------------------------------------------------------------------------------------------- the cases ---
@dataclasses.dataclass(frozen=True)
class Case:
  dtype: str
  M: int
  N: int
  K: int
  a: str = "K"          # which index of A(i,k) is contiguous: K (row-major), M (column-major), G (neither)
  b: str = "M"          # of B(k,j): M = j contiguous (row-major), K = k contiguous (column-major), G (neither)
  a_off: int = 0        # elements the base of A is moved off its 16-byte alignment
  b_off: int = 0
  lower: int = 0
  k_mode: int = 0
  batch: int = 0
  outer: int = 0
  ws: str = "none"      # split-K workspace: none, full (what the query asks for), short (one byte less)
  alpha: float = 1.0
  beta: float = 0.0
  c: str = "row"        # C(i,j): row (c_j = 1), col (c_i = 1), gen (neither)
  c32: bool = False
  want: str = ""        # tile/kernel this case is there for; test_every_case_reaches_the_route_it_is_there_for
  splits: bool = False  # the workspace query reports more than one slice for this shape (checked in the same test)
  tag: str = ""

  @property
  def problems(self):
    return max(self.batch, 1) * max(self.outer, 1)


def ld(n):
  """A leading dimension with a gap behind every row that keeps the rows 16-byte aligned."""
  return (n + 3) // 4 * 4 + 4


def operand_strides(layout, m, k):
  """(s_m, s_k) of an m x k operand."""
  return {"K": (ld(k), 1), "M": (1, ld(m)), "G": (2 * k + 3, 2)}[layout]


def a_strides(c):
  return operand_strides(c.a, c.M, c.K)                  # (a_i, a_k)


def b_strides(c):
  s_m, s_k = operand_strides(c.b, c.N, c.K)
  return (s_k, s_m)                                      # (b_k, b_j)


def c_strides(c):
  return {"row": (c.N + 5, 1), "col": (1, c.M + 3), "gen": (2 * c.N + 6, 2)}[c.c]      # (c_i, c_j)


def span(rows, cols, s_r, s_c):
  return (rows - 1) * s_r + (cols - 1) * s_c + 1


def batch_strides(c):
  """Batch and outer strides of A, B and C: multiples of four elements (the load mode is chosen from problem 0 alone),
  with a gap behind every problem."""
  nb = max(c.batch, 1)
  out = {}
  for name, sp in (("a", span(c.M, c.K, *a_strides(c))), ("b", span(c.K, c.N, *b_strides(c))),
                   ("c", span(c.M, c.N, *c_strides(c)))):
    inner = (sp + 3) // 4 * 4 + 16
    out[name] = (inner, nb * inner + 32)
  return out


def route_of(c, count=slices):
  return route(c.dtype, c.M, c.N, c.K, a_strides(c), b_strides(c), c.a_off % VEC[c.dtype] == 0,
               c.b_off % VEC[c.dtype] == 0, c.lower, c.k_mode, c.batch, c.ws != "none", outer=c.outer, c32=c.c32,
               ws_enough=c.ws == "full", count=count)


def declared_route(c):
  """route_of() with the slice count the case declares in place of the library's: ids are made when the file is
  collected, and collecting must not build or load the library. test_every_case_reaches_the_route_it_is_there_for
  holds the two together."""
  return route_of(c, count=lambda *shape: 2 if c.splits else 1)


def case_id(c):
  tile, kernel, am, bm, grid, split = declared_route(c)
  extra = "".join([f"-batch{c.batch}" if c.batch else "", f"-outer{c.outer}" if c.outer else "",
                   "-c32" if c.c32 else "", f"-ws_{c.ws}" if c.ws != "none" else "", f"-c_{c.c}" if c.c != "row" else "",
                   f"-{c.tag}" if c.tag else ""])
  return (f"{tile}-{kernel}-{am}{bm}-{grid}-{'split' if split else 'unsplit'}-{c.dtype}-{c.M}x{c.N}x{c.K}"
          f"-lower{c.lower}-k_mode{c.k_mode}-alpha{c.alpha:g}-beta{c.beta:g}{extra}")


def lower_kind(c):
  if c.lower == 0:
    return "full"
  if c.lower == 3:
    return "early_exit"
  return "triangle" if c.M == c.N else "strip"


LOWER_KINDS = ("full", "triangle", "strip", "early_exit")
PAIRS = [("M", "M"), ("M", "K"), ("K", "M"), ("K", "K")]
ALL_ROUTES = (
    {("tile", t, am, bm) for t in TILES for am, bm in PAIRS}
    | {("generic", d) for d in NP}
    | {("generic", d, which, mode) for d in NP for which in "ab" for mode in "GMK"}
    | {("k_mode x lower_only", kern, d, k, lk) for kern in ("fast", "generic") for d in NP for k in range(4)
       for lk in LOWER_KINDS}
    | {("TileF64K32", k, lk) for k, lk in ((1, "full"), (3, "full"), (0, "triangle"), (0, "strip"), (1, "early_exit"))}
    | {("TileF64Big", k, lk) for k, lk in ((0, "full"), (1, "full"), (3, "full"), (0, "triangle"), (2, "triangle"))}
    | {("grid", g) for g in ("square", "triangular", "columns", "rows_reversed")}
    | {("split-K", kern, d) for kern in ("fast", "generic") for d in NP}
    | {("split-K", "lower_only"), ("split-K", "workspace one byte short"), ("split-K", "uneven last slice")}
    | {("batch",), ("outer",), ("batch+outer",), ("c32",), ("c32", "batch"), ("c32", "outer"), ("c32", "batch+outer"),
       ("c32", "lower_only")}
    | {("c32", d) for d in NP}
    | {("c32", "split-K workspace", kern) for kern in ("fast", "generic")}
    | {("c_j != 1", kern) for kern in ("generic", "fast", "big", "split-K")}
    | {("misaligned base", d) for d in NP})


def features(c):
  """The elements of ALL_ROUTES one case covers."""
  tile, kernel, am, bm, grid, split = route_of(c)
  f = set()
  if kernel == "generic":
    f |= {("generic", c.dtype), ("generic", c.dtype, "a", am), ("generic", c.dtype, "b", bm)}
    if c.a_off % VEC[c.dtype] or c.b_off % VEC[c.dtype]:
      f.add(("misaligned base", c.dtype))
  else:
    f |= {("tile", tile, am, bm), ("grid", grid)}
  if tile in ("Tile<float>", "Tile<double>") and not c.batch and not c.outer:
    f.add(("k_mode x lower_only", "generic" if kernel == "generic" else "fast", c.dtype, c.k_mode, lower_kind(c)))
  if tile in ("TileF64K32", "TileF64Big"):
    f.add((tile, c.k_mode, lower_kind(c)))
  if split:
    f.add(("split-K", "generic" if kernel == "generic" else "fast", c.dtype))
    if c.lower:
      f.add(("split-K", "lower_only"))
    n = slices(c.dtype, c.M, c.N, c.K, c.lower)
    bk = TILES[tile][1]
    chunk = (-(-c.K // n) + bk - 1) // bk * bk          # K / n rounded up, then up to whole K steps
    if c.K - (n - 1) * chunk != chunk:
      f.add(("split-K", "uneven last slice"))
  if c.ws == "short" and slices(c.dtype, c.M, c.N, c.K, c.lower) > 1:
    f.add(("split-K", "workspace one byte short"))
  many = "batch+outer" if c.batch > 1 and c.outer > 1 else "batch" if c.batch > 1 else "outer" if c.outer > 1 else None
  if many:
    f.add((many,))
  if c.c32:
    f.add(("c32",))
    if many:
      f.add(("c32", many))
    if c.lower:
      f.add(("c32", "lower_only"))
    f.add(("c32", c.dtype))
    if c.ws == "full" and c.k_mode == 0 and not many and slices(c.dtype, c.M, c.N, c.K, c.lower) > 1:
      f.add(("c32", "split-K workspace", "generic" if kernel == "generic" else "fast"))   # must run unsplit
  if c.c != "row":
    f.add(("c_j != 1", "split-K" if split else kernel))
  return f


def build_cases():
  cases = []
  n = [0]

  def add(dtype, M, N, K, **kw):
    if "alpha" not in kw:            # every (alpha, beta) pair comes round
      kw["alpha"], kw["beta"] = ALPHAS[n[0] % 4], BETAS[(n[0] // 4 + n[0]) % 3]
      if kw.get("c32"):
        kw["beta"] = 0.0
    n[0] += 1
    kw.setdefault("splits", kw.get("ws", "none") != "none")
    cases.append(Case(dtype, M, N, K, **kw))

  # ---- float32
  for shape in ((1, 1, 1), (5, 7, 3), (130, 70, 33), (129, 257, 17)):
    add("f32", *shape, want="Tile<float>/generic")
    add("f32", *shape, a="M", b="K", c="col", want="Tile<float>/generic")
  add("f32", 130, 70, 33, a="G", b="G", c="gen", want="Tile<float>/generic")
  add("f32", 128, 128, 32, a_off=1, want="Tile<float>/generic", tag="a_off1")
  add("f32", 128, 128, 32, b_off=1, a="M", want="Tile<float>/generic", tag="b_off1")
  add("f32", 128, 128, 32, b="G", want="Tile<float>/generic")
  for a, b in PAIRS:
    add("f32", 256, 128, 48, a=a, b=b, want="Tile<float>/fast")
    add("f32", 128, 256, 1040, a=a, b=b, want="Tile<float>/fast", c="gen" if a == b else "row")
    add("f32", 192, 64, 128, a=a, b=b, want="TileF32Small/fast")
    add("f32", 64, 192, 1024, a=a, b=b, want="TileF32Small/fast", c="col" if a == "M" else "row")
    add("f32", 2304, 2048, 128, a=a, b=b, want="TileF32K64/fast")
  add("f32", 640, 512, 4096, ws="full", want="Tile<float>/fast/split")
  add("f32", 640, 512, 4096, ws="full", a="M", b="K", c="gen", alpha=3.0, beta=-2.0, want="Tile<float>/fast/split")
  add("f32", 640, 512, 4096, ws="short", alpha=-1.0, beta=1.0, want="Tile<float>/fast")
  add("f32", 640, 512, 8192, ws="full", alpha=0.5, beta=1.0, want="Tile<float>/fast/split")
  add("f32", 641, 512, 4096, ws="full", want="Tile<float>/generic/split")
  add("f32", 641, 512, 4096, ws="short", alpha=3.0, beta=-2.0, want="Tile<float>/generic")
  for beta in (0.0, -2.0):
    add("f32", 768, 768, 4096, ws="full", lower=1, alpha=-1.0, beta=beta, want="Tile<float>/fast/split")
  add("f32", 768, 768, 4096, ws="short", lower=1, alpha=0.5, beta=-2.0, want="Tile<float>/fast")
  # ---- float64
  for shape in ((5, 7, 3), (130, 70, 33)):
    add("f64", *shape, want="Tile<double>/generic")
    add("f64", *shape, a="M", b="K", c="col", want="Tile<double>/generic")
  add("f64", 130, 70, 33, a="G", b="G", c="gen", want="Tile<double>/generic")
  add("f64", 64, 64, 16, a_off=1, want="Tile<double>/generic", tag="a_off1")
  add("f64", 64, 64, 16, b_off=1, a="M", want="Tile<double>/generic", tag="b_off1")
  for a, b in PAIRS:
    add("f64", 128, 64, 48, a=a, b=b, want="Tile<double>/fast", c="gen" if a == b else "row")
  for k_mode in (1, 3):
    add("f64", 128, 128, 144, k_mode=k_mode, want="Tile<double>/fast")
  for a, b in PAIRS:
    add("f64", 128, 192, 128, k_mode=1, a=a, b=b, want="TileF64K32/fast")
  for M, N, K in ((128, 192, 128), (192, 192, 160)):
    add("f64", M, N, K, k_mode=1, want="TileF64K32/fast", c="col")
    add("f64", M, N, K, k_mode=3, want="TileF64K32/fast")
    add("f64", M, N, K, lower=1, alpha=-1.0, beta=1.0, want="TileF64K32/fast")     # the Cholesky trailing updates
    add("f64", M, N, K, lower=1, k_mode=2, a="M", b="M", c32=True, want="Tile<double>/fast")   # gp of gptq.hip
  add("f64", 192, 128, 160, lower=1, alpha=-1.0, beta=1.0, want="TileF64K32/fast")  # `strip` of the Cholesky
  for a, b in PAIRS:
    add("f64", 2048, 2048, 256, a=a, b=b, want="TileF64Big/big", c="gen" if a == b == "K" else "row")
  for k_mode in (1, 3):
    add("f64", 2048, 2048, 256, k_mode=k_mode, want="TileF64Big/big")
  add("f64", 4096, 4096, 256, lower=1, alpha=-1.0, beta=1.0, want="TileF64Big/big")
  add("f64", 4096, 4096, 256, lower=1, k_mode=2, a="M", b="M", alpha=1.0, beta=0.0, want="TileF64Big/big")
  # the tile walk: lower_only on a square grid under k_mode 1 (rows reversed), three tiles a side
  for lower, M, N in ((3, 192, 192), (1, 192, 128), (3, 192, 128), (1, 128, 192)):
    add("f64", M, N, 192, lower=lower, k_mode=1, want="TileF64K32/fast")
    add("f64", M, N, 176, lower=lower, k_mode=1, alpha=3.0, beta=-2.0, want="Tile<double>/fast")
  add("f32", 384, 384, 384, lower=3, k_mode=1, want="Tile<float>/fast")
  add("f32", 384, 256, 384, lower=1, k_mode=1, alpha=-1.0, beta=1.0, want="Tile<float>/fast")
  add("f64", 320, 256, 4096, ws="full", want="Tile<double>/fast/split")
  add("f64", 320, 256, 4096, ws="full", a="M", b="K", c="col", alpha=0.5, beta=1.0, want="Tile<double>/fast/split")
  add("f64", 320, 256, 4096, ws="short", alpha=3.0, beta=-2.0, want="Tile<double>/fast")
  add("f64", 320, 256, 8192, ws="full", alpha=-1.0, beta=-2.0, want="Tile<double>/fast/split")
  add("f64", 321, 256, 4096, ws="full", want="Tile<double>/generic/split")
  add("f64", 321, 256, 4096, ws="full", c="gen", alpha=-1.0, beta=1.0, want="Tile<double>/generic/split")
  add("f64", 321, 256, 4096, ws="short", want="Tile<double>/generic")
  add("f64", 320, 320, 4096, ws="full", lower=1, alpha=3.0, beta=1.0, splits=False, want="TileF64K32/fast")  # no workspace
  # c32 with a workspace that would split: the reducer knows no c32, so the product runs unsplit into c32
  add("f64", 320, 256, 4096, ws="full", c32=True, want="Tile<double>/fast")
  add("f64", 321, 256, 4096, ws="full", c32=True, c="gen", want="Tile<double>/generic")
  add("f32", 640, 512, 4096, ws="full", c32=True, want="Tile<float>/fast")
  add("f32", 641, 512, 4096, ws="full", c32=True, want="Tile<float>/generic")
  add("f64", 384, 384, 4112, ws="full", lower=1, alpha=3.0, beta=1.0, want="Tile<double>/fast/split")
  # ---- every k_mode with every form of lower_only, on the fast and on the generic kernel of the default tiles
  for dtype, bm in (("f32", 128), ("f64", 64)):
    for kernel in ("fast", "generic"):
      for k_mode in range(4):
        for lower, square in ((0, False), (1, True), (1, False), (3, True), (3, False)):
          if kernel == "fast":      # K % 32 != 0 keeps float64 off TileF64K32
            M, N, K = 3 * bm, (3 if square else 2) * bm, 3 * bm - 16
          else:
            M, N, K = 3 * bm - 5, (3 * bm - 5) if square else 2 * bm + 3, 3 * bm - 9
          add(dtype, M, N, K, lower=lower, k_mode=k_mode,
              want=("Tile<float>/" if dtype == "f32" else "Tile<double>/") + kernel)
  # ---- batches: g1 (k_mode 3) and g2 (k_mode 1) of the batched triangular inverse
  for k_mode in (1, 3):
    for batch, outer in ((3, 0), (0, 2), (3, 2)):
      for c32 in (False, True):
        add("f64", 128, 128, 128, k_mode=k_mode, batch=batch, outer=outer, c32=c32, want="TileF64K32/fast")
  add("f64", 130, 70, 33, batch=3, outer=2, want="Tile<double>/generic")
  add("f64", 130, 70, 33, batch=3, outer=2, c32=True, lower=1, want="Tile<double>/generic")
  add("f32", 192, 64, 128, batch=3, outer=2, want="TileF32Small/fast")
  add("f32", 192, 64, 128, batch=3, outer=2, c32=True, want="TileF32Small/fast")
  add("f32", 256, 128, 48, c32=True, c="col", want="Tile<float>/fast")
  add("f32", 130, 70, 33, c32=True, lower=3, want="Tile<float>/generic")
  add("f32", 130, 70, 33, batch=2, outer=3, want="Tile<float>/generic")
  return cases


def want_of(c):
  tile, kernel, _, _, _, split = route_of(c)
  return f"{tile}/{kernel}" + ("/split" if split else "")


# ---------------------------------------------------------------------------------------------------- the reference ---
def masked(A, B, k_mode):
  """The operands a k_mode promises: zeros where the kernel may skip."""
  if k_mode == 1:
    A = np.tril(A)                   # A(i,k) == 0 for k > i
  if k_mode == 2:
    A = np.triu(A)                   # A(i,k) == 0 for k < i
  if k_mode in (2, 3):
    B = np.tril(B)                   # B(k,j) == 0 for k < j
  return A, B


@functools.lru_cache(maxsize=2)
def host_data(dtype, M, N, K, k_mode, problems, kind):
  """A [P,M,K], B [P,K,N], C0 [P,M,N] in the case's type, and A @ B, |A| @ |B| in float64 -- made once per shape and
  left unchanged. kind int: integers in [-8, 8]; normal: standard-normal values."""
  rng = np.random.default_rng([M, N, K, k_mode, problems, 32 if dtype == "f32" else 64])
  if kind == "int":
    draw = lambda *s: rng.integers(-8, 9, size=s).astype(NP[dtype])  # noqa: E731
  else:
    draw = lambda *s: rng.standard_normal(s).astype(NP[dtype])  # noqa: E731
  A, B, C0 = draw(problems, M, K), draw(problems, K, N), draw(problems, M, N)
  A, B = masked(A, B, k_mode)
  A64, B64 = A.astype(np.float64), B.astype(np.float64)
  prod = np.matmul(A64, B64) + 0.0            # (+ 0.0: an exact zero is +0, as an accumulator that started at +0 is)
  mag = np.matmul(np.abs(A64), np.abs(B64))
  for x in (A, B, C0, prod, mag):
    x.setflags(write=False)
  return A, B, C0, prod, mag


def reference(c, kind="int"):
  """(C0, expected values [P,M,N] in the case's type or float32 for c32, |alpha| |A||B| + |beta C0|)."""
  _, _, C0, prod, mag = host_data(c.dtype, c.M, c.N, c.K, c.k_mode, c.problems, kind)
  size = c.alpha * prod                                      # beta == 0 never reads C: no term for it
  want = size if c.beta == 0.0 else c.beta * C0.astype(np.float64) + size
  scale = abs(c.alpha) * mag + np.abs(c.beta * C0.astype(np.float64))
  if kind == "int":
    # every partial sum, in any order and however it is split, is an integer below 2^24: exact in float32 and float64
    assert c.K <= 8192 and float(scale.max(initial=0.0)) < 2.0 ** 24
  return C0, want.astype(np.float32 if c.c32 else NP[c.dtype]), scale


# --------------------------------------------------------------------------------------------------------- the call ---
def positions(c, rows, cols, s_r, s_c, strides, base):
  """Buffer index of element (p, r, q) of every problem: [P, rows, cols]."""
  nb = max(c.batch, 1)
  p = np.arange(c.problems, dtype=np.int64)
  start = base + (p // nb) * strides[1] + (p % nb) * strides[0]
  return (start[:, None, None] + np.arange(rows, dtype=np.int64)[None, :, None] * s_r
          + np.arange(cols, dtype=np.int64)[None, None, :] * s_c)


def poison(c, A, B):
  """NaN wherever no tile of any kernel may look under the case's k_mode (128 is the largest tile edge)."""
  A, B = A.copy(), B.copy()
  i = np.arange(c.M)[:, None]
  k_a = np.arange(c.K)[None, :]
  k_b = np.arange(c.K)[:, None]
  j = np.arange(c.N)[None, :]
  if c.k_mode == 1:
    A[:, k_a >= -(-(i + 1) // 128) * 128] = np.nan
  if c.k_mode == 2:
    A[:, k_a < i // 128 * 128] = np.nan
  if c.k_mode in (2, 3):
    B[:, k_b < j // 128 * 128] = np.nan
  return A, B


class Run:
  """The buffers of one case on the host, the launch, and the comparison of everything the call could have written."""

  def __init__(self, m, c, kind="int", poisoned=False):
    self.m, self.c = m, c
    t = NP[c.dtype]
    A, B, C0, _, _ = host_data(c.dtype, c.M, c.N, c.K, c.k_mode, c.problems, kind)
    if poisoned:
      A, B = poison(c, A, B)
    bs = batch_strides(c)
    self.bs = bs
    nb, no = max(c.batch, 1), max(c.outer, 1)
    # operands: NaN everywhere but in the elements of the operand
    self.a_idx = positions(c, c.M, c.K, *a_strides(c), bs["a"], 4 + c.a_off)
    self.b_idx = positions(c, c.K, c.N, *b_strides(c), bs["b"], 4 + c.b_off)
    a_host = np.full(int(self.a_idx.max()) + 1 + 4, np.nan, t)
    b_host = np.full(int(self.b_idx.max()) + 1 + 4, np.nan, t)
    a_host[self.a_idx] = A
    b_host[self.b_idx] = B
    self.c_idx = positions(c, c.M, c.N, *c_strides(c), bs["c"], GUARD)
    total = GUARD + (no - 1) * bs["c"][1] + (nb - 1) * bs["c"][0] + span(c.M, c.N, *c_strides(c)) + GUARD
    assert total > int(self.c_idx.max()) + GUARD
    self.c_host = np.full(total, FILL[c.dtype], t)
    if c.beta != 0.0:                   # beta == 0: C holds NaN, and must never be read (c32 needs beta == 0)
      self.c_host[self.c_idx] = C0
    self.c32_idx = self.c32_host = None
    if c.c32:                           # C's strides and batch stride, an outer stride of its own (gp: 2 * oc)
      self.oc32 = bs["c"][1] + 48
      self.c32_idx = positions(c, c.M, c.N, *c_strides(c), (bs["c"][0], self.oc32), GUARD)
      self.c32_host = np.full(total + (no - 1) * 48, FILL["f32"], np.float32)
      assert self.c32_host.size > int(self.c32_idx.max()) + GUARD
    self.a_dev = m.torch.from_numpy(a_host).cuda()
    self.b_dev = m.torch.from_numpy(b_host).cuda()
    self.ws = None
    self.ws_bytes = 0
    if c.ws != "none":
      fn = m.L.mi355q_gemm_splitk_workspace_bytes_f32 if c.dtype == "f32" else m.L.mi355q_gemm_splitk_workspace_bytes_f64
      full = fn(c.M, c.N, c.K, c.lower)
      assert full > 0 or c.ws == "full"      # (0: never split; the pointer alone must change nothing then)
      self.ws = m.torch.empty(max(full, 16), dtype=m.torch.uint8, device="cuda")
      self.ws_bytes = full if c.ws == "full" else full - 1

  def launch(self, single=None, into=None):
    """One call (or, single = p: problem p alone, as a launch of its own, into the buffers of `into`). Returns
    (C buffer, c32 buffer or None) as they are afterwards."""
    m, c = self.m, self.c
    size = np.dtype(NP[c.dtype]).itemsize
    if into is None:
      c_dev = m.torch.from_numpy(self.c_host).cuda()
      c32_dev = m.torch.from_numpy(self.c32_host).cuda() if c.c32 else None
    else:
      c_dev, c32_dev = into
    for t in (self.a_dev, self.b_dev, c_dev):
      assert t.data_ptr() % 16 == 0
    d = m.ffi.GemmDesc()
    (d.a_i, d.a_k), (d.b_k, d.b_j), (d.c_i, d.c_j) = a_strides(c), b_strides(c), c_strides(c)
    d.M, d.N, d.K, d.alpha, d.beta, d.lower_only, d.k_mode = c.M, c.N, c.K, c.alpha, c.beta, c.lower, c.k_mode
    p = 0 if single is None else single
    d.A = self.a_dev.data_ptr() + int(self.a_idx[p, 0, 0]) * size
    d.B = self.b_dev.data_ptr() + int(self.b_idx[p, 0, 0]) * size
    d.C = c_dev.data_ptr() + int(self.c_idx[p, 0, 0]) * size
    d.c32 = c32_dev.data_ptr() + int(self.c32_idx[p, 0, 0]) * 4 if c.c32 else None
    if single is None:
      d.batch, d.outer = c.batch, c.outer
      (d.sa, d.oa), (d.sb, d.ob), (d.sc, d.oc) = self.bs["a"], self.bs["b"], self.bs["c"]
      d.oc32 = self.oc32 if c.c32 else 0
    fn = m.L.mi355q_gemm_ex_f32 if c.dtype == "f32" else m.L.mi355q_gemm_ex_f64
    st = fn(ctypes.c_void_p(ctypes.addressof(d)), m.rt.ptr(self.ws), self.ws_bytes, m.rt.stream_ptr())
    assert st == 0, (st, m.L.mi355q_last_error())
    if into is not None:
      return into
    m.torch.cuda.synchronize()
    return c_dev.cpu().numpy(), (c32_dev.cpu().numpy() if c.c32 else None)

  def written(self):
    """[M, N] mask of the elements a call writes."""
    i, j = np.arange(self.c.M)[:, None], np.arange(self.c.N)[None, :]
    return (j <= i) if self.c.lower else np.ones((self.c.M, self.c.N), bool)

  def expected(self, want):
    """(C buffer, c32 buffer) after the call, given the values [P,M,N] it has to write."""
    w = self.written()
    c_exp = self.c_host.copy()
    c32_exp = None
    if self.c.c32:
      c32_exp = self.c32_host.copy()
      c32_exp[self.c32_idx[:, w]] = want[:, w]
    else:
      c_exp[self.c_idx[:, w]] = want[:, w]
    return c_exp, c32_exp

  def where(self, flat, size):
    """(problem, i, j) and the 64-wide tiles of buffer elements, for a message."""
    idx = self.c_idx if size == self.c_host.size else self.c32_idx
    owner = np.full(size, -1, np.int64)
    owner[idx.reshape(-1)] = np.arange(idx.size)
    out = []
    for f in flat:
      o = int(owner[f])
      if o < 0:
        out.append(f"buffer[{int(f)}] (a gap or a guard)")
      else:
        p, r = divmod(o, self.c.M * self.c.N)
        i, j = divmod(r, self.c.N)
        out.append(f"(p{p}, {i}, {j})")
    inside = owner[flat][owner[flat] >= 0] % (self.c.M * self.c.N)
    tiles = sorted({(int(e // self.c.N // 64), int(e % self.c.N // 64)) for e in inside})
    return out, tiles

  def same_bits(self, got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.flatnonzero(got.view(u) != exp.view(u))
    if bad.size:
      names, _ = self.where(bad[:6], got.size)
      _, tiles = self.where(bad[::max(1, bad.size // 4096)], got.size)
      raise AssertionError(f"{what}: {bad.size} elements differ; first {names}: {got[bad[:6]].tolist()} instead of "
                           f"{exp[bad[:6]].tolist()}; 64 x 64 tiles (row, column) touched: {tiles[:24]}")


def run_exact(m, c, poisoned=False, repeat=True):
  _, want, _ = reference(c)
  r = Run(m, c, poisoned=poisoned)
  c_exp, c32_exp = r.expected(want)
  got = r.launch()
  what = case_id(c) + (" (skipped K range poisoned)" if poisoned else "")
  r.same_bits(got[0], c_exp, f"{what} C")
  if c.c32:
    r.same_bits(got[1], c32_exp, f"{what} c32")
  if repeat:
    again = r.launch()
    r.same_bits(again[0], got[0], f"{what} C, second call")
    if c.c32:
      r.same_bits(again[1], got[1], f"{what} c32, second call")


CASES = build_cases()


# ------------------------------------------------------------------------------------------------- tests without a GPU ---
def test_environment_leaves_the_routes_alone():
  assert env_is_default()


def test_every_route_has_a_case():
  reached = set()
  for c in CASES:
    reached |= features(c)
  assert ALL_ROUTES - reached == set(), sorted(map(str, ALL_ROUTES - reached))
  assert len(ALL_ROUTES) == 24 + 2 + 12 + 64 + 5 + 5 + 4 + 4 + 3 + 8 + 2 + 2 + 4 + 2
  assert {(c.alpha, c.beta) for c in CASES if not c.c32} == {(a, b) for a in ALPHAS for b in BETAS}
  assert len({case_id(c) for c in CASES}) == len(CASES)


def test_every_case_reaches_the_route_it_is_there_for():
  for c in CASES + FLOAT_CASES:
    assert want_of(c) == c.want, (case_id(c), c.want)
    assert declared_route(c) == route_of(c), case_id(c)
    assert c.splits == (c.ws != "none" and slices(c.dtype, c.M, c.N, c.K, c.lower) > 1), case_id(c)
    if "split" in c.want or c.ws == "short" or (c.c32 and c.ws == "full"):
      assert c.splits, case_id(c)


def test_route_restates_the_launcher_at_its_thresholds():
  def r(dtype, M, N, K, lower=0, k_mode=0, batch=0, ws=False, a="K", b="M"):
    c = Case(dtype, M, N, K, a=a, b=b, lower=lower, k_mode=k_mode, batch=batch, ws="full" if ws else "none")
    return want_of(c)

  assert r("f32", 2304, 2048, 128) == "TileF32K64/fast" and r("f32", 2048, 2048, 128) == "TileF32Small/fast"
  assert r("f32", 2304, 2048, 1024) == "TileF32K64/fast" and r("f32", 2304, 2048, 1088) == "Tile<float>/fast"
  assert r("f32", 2304, 2048, 64) == "Tile<float>/fast" and r("f32", 192, 64, 128, lower=3) == "Tile<float>/generic"
  assert r("f32", 4224, 4096, 128) == "Tile<float>/fast"                       # 33 x 32 tiles: more than 512
  assert r("f32", 192, 64, 128, batch=3) == "TileF32Small/fast"
  assert r("f64", 2048, 2048, 256) == "TileF64Big/big" and r("f64", 2048, 2048, 240) == "Tile<double>/fast"
  assert r("f64", 2048, 1920, 256) == "Tile<double>/fast"                      # 240 tiles of 128 x 128
  assert r("f64", 2048, 2048, 256, lower=1) == "Tile<double>/fast"             # 1024 tiles of 64 x 64: not K32 either
  assert r("f64", 4096, 4096, 256, lower=1) == "TileF64Big/big"
  assert r("f64", 1408, 1472, 128, k_mode=1) == "TileF64K32/fast"              # 22 x 23 = 506 tiles
  assert r("f64", 1472, 1472, 128, k_mode=1) == "Tile<double>/fast"            # 529 tiles
  assert r("f64", 192, 192, 160, k_mode=2, lower=1) == "Tile<double>/fast"
  assert r("f64", 192, 192, 96, k_mode=1) == "Tile<double>/fast"               # K < 128
  assert r("f64", 320, 256, 4096, ws=True) == "Tile<double>/fast/split" and r("f64", 320, 256, 4096) == "Tile<double>/fast"
  assert r("f64", 320, 256, 4080, ws=True) == "Tile<double>/fast"
  assert r("f64", 320, 256, 4096, ws=True, k_mode=1) == "TileF64K32/fast"
  assert route_of(Case("f64", 192, 128, 176, k_mode=1, lower=1))[4] == "rows_reversed"
  assert route_of(Case("f64", 192, 192, 176, k_mode=1, lower=1))[4] == "triangular"
  assert route_of(Case("f64", 192, 128, 176, k_mode=3))[4] == "columns"
  assert route_of(Case("f64", 192, 128, 176, k_mode=3, lower=3))[4] == "square"
  assert pick_mode("f32", 1, 4, True) == "M" and pick_mode("f32", 1, 1, True) == "G" and pick_mode("f64", 1, 3, True) == "G" and pick_mode("f64", 6, 1, True) == "K"
  assert pick_mode("f32", 6, 1, True) == "G" and pick_mode("f32", 8, 1, False) == "G"


@pytest.mark.parametrize("c", [c for c in CASES if c.problems * c.M * c.N * c.K <= 1 << 24], ids=case_id)
def test_partial_sums_stay_below_2_to_24(c):
  """The assertion on |alpha| (|A| @ |B|) + |beta C0| inside reference(), here without a GPU for the small cases; every
  case passes through it again when it runs. For all of them: 64 K |alpha| + 8 |beta| < 2^24."""
  _, want, scale = reference(c)
  assert np.array_equal(want.astype(np.float64), np.rint(want.astype(np.float64) * 2) / 2)
  assert float(scale.max()) < 2.0 ** 24


def test_every_case_is_bounded_by_its_shape():
  for c in CASES:
    assert c.K <= 8192 and 64 * c.K * abs(c.alpha) + 8 * abs(c.beta) < 2.0 ** 24
    assert c.alpha in ALPHAS and c.beta in BETAS


def host_desc(ffi, **kw):
  """A descriptor whose operands are host memory: for the calls that return before they launch."""
  buf = ctypes.create_string_buffer(256)
  base = (ctypes.addressof(buf) + 15) & ~15
  d = ffi.GemmDesc(A=base, a_i=4, a_k=1, B=base, b_k=4, b_j=1, C=base, c_i=4, c_j=1, M=4, N=4, K=4, alpha=1.0, beta=0.0)
  for key, value in kw.items():
    setattr(d, key, value)
  d.keep = buf
  return d


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_entry_refuses_bad_arguments_before_it_launches(lib, dtype):
  from mi355q import _ffi
  fn = lib.mi355q_gemm_ex_f32 if dtype == "f32" else lib.mi355q_gemm_ex_f64
  err = lib.mi355q_last_error

  def call(**kw):
    d = host_desc(_ffi, **kw)
    return fn(ctypes.c_void_p(ctypes.addressof(d)), None, 0, None)

  assert fn(None, None, 0, None) == -1 and b"null descriptor" in err()
  for operand in "ABC":
    assert call(**{operand: None}) == -1 and b"null pointer" in err()
  for dim in "MNK":
    assert call(**{dim: -1}) == -1 and b"negative shape" in err()
    assert call(**{dim: 1 << 31}) == -3 and b"too large" in err()
  # an empty product is a no-op, whatever the pointers
  assert call(M=0, A=None, B=None, C=None) == 0 and err() == b""
  assert call(N=0, A=None, B=None, C=None) == 0 and err() == b""
  for k_mode in (-1, 4, 7):
    assert call(k_mode=k_mode) == -1 and b"k_mode must be 0, 1, 2 or 3" in err()
  for lower in (-1, 2, 4):           # 2 is the launcher's own name for the triangular grid
    assert call(lower_only=lower) == -1 and b"lower_only must be 0, 1 or 3" in err()
  other = host_desc(_ffi)
  for beta in (1.0, -2.0):
    assert call(c32=other.A, beta=beta) == -1 and b"needs beta == 0" in err()
  assert call(batch=-1) == -1 and b"negative batch count" in err()
  assert call(outer=-1) == -1 and b"negative batch count" in err()
  assert call(batch=256, outer=256) == -3 and b"65535" in err()
  # refusals come before the empty-product shortcut, as in the other entry points
  assert call(M=0, k_mode=4) == -1 and call(N=0, lower_only=2) == -1
  assert call(M=0) == 0 and err() == b""          # (and leaves no message behind for whoever asks next)


def test_descriptor_matches_the_header():
  """GemmDesc of _ffi.py against mi355q_gemm_desc of include/mi355q.h: the same fields in the same order with the same
  sizes, no padding between them, 192 bytes."""
  import re
  from mi355q import _ffi
  text = open(os.path.join(ROOT, "include", "mi355q.h")).read()
  body = re.search(r"typedef struct mi355q_gemm_desc \{(.*?)\} mi355q_gemm_desc;", text, re.S).group(1)
  sizes = {"const void*": 8, "void*": 8, "float*": 8, "int64_t": 8, "double": 8, "int32_t": 4}
  header = []
  for decl in body.split(";"):
    decl = decl.strip()
    if decl:
      ctype, names = re.fullmatch(r"(.*[\w*])\s+(\w+(?:,\s*\w+)*)", decl).groups()
      header += [(name.strip(), sizes[ctype]) for name in names.split(",")]
  ours = [(name, ctypes.sizeof(t)) for name, t in _ffi.GemmDesc._fields_]
  assert ours == header
  offset = 0
  for name, size in ours:
    assert getattr(_ffi.GemmDesc, name).offset == offset, name
    offset += size
  assert ctypes.sizeof(_ffi.GemmDesc) == offset == 192


def test_workspace_query_without_gpu(lib):
  for dtype, fn in (("f32", lib.mi355q_gemm_splitk_workspace_bytes_f32), ("f64", lib.mi355q_gemm_splitk_workspace_bytes_f64)):
    size = np.dtype(NP[dtype]).itemsize
    assert fn(640, 512, 4095, 0) == 0 and fn(128, 128, 128, 0) == 0       # K < 4096: never split
    assert fn(-1, 512, 4096, 0) == 0 and fn(640, 0, 4096, 0) == 0 and fn(1 << 31, 512, 4096, 0) == 0
    assert fn(8192, 8192, 4096, 0) == 0                                   # enough tiles without a split
    n = fn(640, 512, 4096, 0)
    assert n > 0 and n % (640 * 512 * size) == 0 and 2 <= n // (640 * 512 * size) <= 16
    assert fn(768, 768, 4096, 1) % (768 * 768 * size) == 0 and fn(768, 768, 4096, 1) > 0


# ---------------------------------------------------------------------------------------------------- tests on a GPU ---
@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_route_is_exact_on_integers(m, c):
  """Bit for bit beta*C0 + alpha*(A @ B) where the call writes, the prefill everywhere else (gaps, guards, above the
  diagonal under lower_only, all of C under c32), NaN-prefilled C under beta == 0 (so under c32), the same bits from a
  second call of every case;
  under a k_mode again with NaN in the K range the mode lets every tile skip."""
  run_exact(m, c)
  if c.k_mode:
    run_exact(m, c, poisoned=True, repeat=False)


BATCHED = [c for c in CASES if c.batch > 1 or c.outer > 1]


@gpu
@pytest.mark.parametrize("c", BATCHED, ids=case_id)
def test_batched_launch_has_the_bits_of_single_launches(m, c):
  """Standard-normal data, where the order of the additions shows: one launch of batch * outer problems against one
  launch per problem."""
  single = dataclasses.replace(c, batch=0, outer=0)
  assert route_of(single)[:5] == route_of(c)[:5]
  r = Run(m, c, kind="normal")
  got = r.launch()
  c_dev = m.torch.from_numpy(r.c_host).cuda()
  c32_dev = m.torch.from_numpy(r.c32_host).cuda() if c.c32 else None
  for p in range(c.problems):
    r.launch(single=p, into=(c_dev, c32_dev))
  m.torch.cuda.synchronize()
  r.same_bits(got[0], c_dev.cpu().numpy(), "C, batched against single launches")
  if c.c32:
    r.same_bits(got[1], c32_dev.cpu().numpy(), "c32, batched against single launches")
    assert not np.isnan(got[1][r.c32_idx[:, r.written()]]).any()
  else:
    assert not np.isnan(got[0][r.c_idx[:, r.written()]]).any()


FLOAT_CASES = [
    Case("f32", 130, 70, 33, alpha=3.0, beta=-2.0, want="Tile<float>/generic"),
    Case("f32", 256, 128, 48, alpha=0.5, beta=1.0, want="Tile<float>/fast"),
    Case("f32", 192, 64, 128, alpha=-1.0, beta=-2.0, want="TileF32Small/fast"),
    Case("f32", 640, 512, 4096, ws="full", splits=True, alpha=3.0, beta=1.0, want="Tile<float>/fast/split"),
    Case("f32", 641, 512, 4096, ws="full", splits=True, alpha=0.5, beta=-2.0, want="Tile<float>/generic/split"),
    Case("f64", 130, 70, 33, alpha=3.0, beta=-2.0, want="Tile<double>/generic"),
    Case("f64", 128, 64, 48, alpha=0.5, beta=1.0, want="Tile<double>/fast"),
    Case("f64", 2048, 2048, 256, alpha=3.0, beta=-2.0, want="TileF64Big/big"),
    Case("f64", 320, 256, 4096, ws="full", splits=True, alpha=-1.0, beta=1.0, want="Tile<double>/fast/split"),
    Case("f64", 321, 256, 4096, ws="full", splits=True, alpha=3.0, beta=-2.0, want="Tile<double>/generic/split"),
]


def test_float_cases_reach_every_kernel_family():
  assert [want_of(c) for c in FLOAT_CASES] == [c.want for c in FLOAT_CASES]
  for dtype, families in (("f32", {"generic", "fast", "split"}), ("f64", {"generic", "fast", "big", "split"})):
    assert {c.want.split("/")[-1] for c in FLOAT_CASES if c.dtype == dtype} == families


@gpu
@pytest.mark.parametrize("c", FLOAT_CASES, ids=case_id)
def test_standard_normal_data_within_the_dot_product_bound(m, c):
  """|c - ref| <= 2 (K + 2) u (|alpha| |A||B| + |beta C0|) elementwise against the float64 product: the textbook bound
  of a length-K dot product in any order (K - 1 additions, K products, alpha, beta and their sum: gamma_(K+2)), doubled."""
  _, want, scale = reference(c, kind="normal")
  C0 = host_data(c.dtype, c.M, c.N, c.K, c.k_mode, c.problems, "normal")[2]
  prod = host_data(c.dtype, c.M, c.N, c.K, c.k_mode, c.problems, "normal")[3]
  ref = c.beta * C0.astype(np.float64) + c.alpha * prod
  r = Run(m, c, kind="normal")
  got = r.launch()[0]
  val = got[r.c_idx].astype(np.float64)
  assert not np.isnan(val).any()
  err = np.abs(val - ref)
  bound = 2.0 * (c.K + 2) * UNIT[c.dtype] * scale
  worst = float((err / bound).max())
  print(f"{case_id(c)}: largest error / bound = {worst:.3g}")
  assert (err <= bound).all(), worst
  exp = r.c_host.copy()
  exp[r.c_idx] = got[r.c_idx]
  r.same_bits(got, exp, "gaps and guards of C")
