"""The integer BATCH_MATMUL kernels of csrc/qbmm.hip compile for gfx950 without scratch (the accumulators, the
fragments and the transposed tile's words all stay in registers or LDS), and every MFMA kernel contains v_mfma_i32_16x16x64_i8."""
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
  out = str(tmp_path_factory.mktemp("isa") / "qbmm.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "qbmm.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    return f.read()


def test_qbmm_is_built():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "qbmm.hip" in g.SOURCES


def test_no_kernel_uses_scratch(asm):
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  names = " ".join(kernels)
  for k in ("qbmm_mfma_kernel", "qbmm_generic_kernel", "transpose_kernel"):
    assert k in names, k
  assert sum("qbmm_mfma_kernel" in k for k in kernels) == 2      # the float rescale and the stored output
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)


def test_every_mfma_kernel_contains_the_int8_matrix_instruction(asm):
  bodies = re.split(r"^\s*\.globl\s+", asm, flags=re.M)
  found = 0
  for body in bodies:
    name = body.split(None, 1)[0] if body.strip() else ""
    if "qbmm_mfma_kernel" in name:
      assert "v_mfma_i32_16x16x64_i8" in body, name
      found += 1
  assert found == 2
