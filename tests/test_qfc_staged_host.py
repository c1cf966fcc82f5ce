"""Host checks of the staged route of the integer FULLY_CONNECTED kernels (csrc/qfc_staged.h): what ops.qfc_route says
for every class of operands, the switch ops.qfc_staged, and the two new symbols in the header, the library and the
prototypes. The addresses are never read. No GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 4096, 8192      # 16-byte aligned "addresses"


@pytest.fixture(scope="module")
def ops():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import ops
  return ops


@pytest.mark.parametrize("want,args", [
    ("mfma", (A, B, 64)), ("mfma", (A, B, 4096)), ("mfma", (A, B, 4096, "i4")), ("mfma", (A, B, 96, "i8", 32, True)),
    ("staged", (A, B, 1)), ("staged", (A, B, 27)), ("staged", (A, B, 96)), ("staged", (A, B, 1000)),
    ("staged", (A, B, 65535)), ("staged", (A + 1, B, 4096)), ("staged", (A, B + 1, 4096)), ("staged", (A + 8, B, 64)),
    ("generic", (A, B, 100, "i4")), ("generic", (A, B, 100, "i2")), ("generic", (A + 1, B, 4096, "i4")),
    ("generic", (A + 1, B, 4096, "i8", 128, True)), ("generic", (A, B + 1, 96, "i8", 32, True)), ("generic", (A, B, 0)),
])
def test_route(ops, want, args):
  assert ops.qfc_route(*args) == want
  with ops.qfc_staged(False):      # the switch takes the staged route away and nothing else
    assert ops.qfc_route(*args) == ("generic" if want == "staged" else want)
    with ops.qfc_staged(True):
      assert ops.qfc_route(*args) == want
    assert ops.qfc_route(*args) != "staged"
  assert ops.qfc_route(*args) == want


def test_abi_of_the_two_entries(ops):
  from mi355q import _ffi
  with open(os.path.join(ROOT, "include", "mi355q.h")) as f:
    header = f.read()
  for name, nargs in (("mi355q_qfc_route", 6), ("mi355q_qfc_set_staged", 1)):
    decl = re.search(r"^int64_t\s+" + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert decl and decl.group(1).count(",") + 1 == nargs == len(_ffi.PROTOTYPES[name][1]), name
    assert _ffi.PROTOTYPES[name][0] is _ffi.c_i64 and hasattr(_ffi.lib(), name)
  codes = {k: int(v) for k, v in re.findall(r"#define MI355Q_QFC_ROUTE_(\w+) (\d)", header)}
  assert [codes[r.upper()] for r in ops.QFC_ROUTES] == [0, 1, 2]
  import __graft_entry__ as g
  assert "qfc_staged.hip" in g.SOURCES and {"qfc_staged.h", "qfc_tile_out.h"} <= set(g.HEADERS)
