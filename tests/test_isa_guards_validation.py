"""The comparison kernels of csrc/validation.hip compile for gfx950 without scratch: the pairwise-tree walks keep
their stacks in LDS (no recursion, no stack arrays), the per-element dequantization stays in registers."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  out = str(tmp_path_factory.mktemp("isa") / "validation.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "validation.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    return f.read()


def test_validation_is_built():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "validation.hip" in g.SOURCES


def test_comparison_kernels_use_no_scratch(asm):
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  names = " ".join(kernels)
  for k in ("compare_sums_kernel", "compare_combine_kernel", "compare_hist_kernel", "compare_select_kernel"):
    assert k in names, k
  assert len(kernels) >= 8
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
