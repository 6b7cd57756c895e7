"""Compile-time guard on k_pp_raw_image (the raw image of a client's public parameters, pp_raw_image.hpp in elementwise.hip), by the
method of tests/test_db_digest_kernel_resources.py: hipcc cross-compiles elementwise.hip for gfx950, no GPU needed, and the numbers are
read from the code object's metadata.  The kernel uses no scratch, spills nothing and has the workgroup size it declares.  Register
bound, from what a thread holds and not from what the compiler happened to give: 16 working words of the ChaCha state, the 16 input
words (the key, the constants and the counter: mostly uniform), 8 output words and addresses -- 64 registers, eight waves per SIMD.
Static LDS: none -- the key is read with uniform loads and the table entry is the workgroup's, so nothing is staged."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
KERNEL, SOURCE, WORKGROUP, LDS_BYTES, VGPRS = "k_pp_raw_image", "elementwise.hip", 256, 0, 64


@pytest.fixture(scope="module")
def kernel():
    if shutil.which(HIPCC) is None:
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(CSRC, SOURCE)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = []
    for block in r.stdout.split("  - .agpr_count:")[1:]:
        if KERNEL in re.search(r"\.name:\s+(\S+)", block).group(1):
            found.append({key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                          for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "group_segment_fixed_size", "max_flat_workgroup_size")})
    assert len(found) == 1, "%d kernels named %s in %s" % (len(found), KERNEL, SOURCE)
    return found[0]


def test_raw_image_kernel_resources(kernel):
    assert kernel["private_segment_fixed_size"] == 0, "scratch"
    assert kernel["vgpr_spill_count"] + kernel["sgpr_spill_count"] == 0, "spilled registers"
    assert kernel["max_flat_workgroup_size"] == WORKGROUP
    assert kernel["group_segment_fixed_size"] <= LDS_BYTES, "%d bytes of static LDS" % kernel["group_segment_fixed_size"]
    assert kernel["vgpr_count"] <= VGPRS, "%d VGPRs, bound %d" % (kernel["vgpr_count"], VGPRS)


def test_raw_image_kernel_adds_no_path_bit():
    """the kernel reports through launched(0, name) from one place, as the other kernels of elementwise.hip without a flow of their own
    do: sp_path_name has no bit for it, and the host part launches nothing itself"""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".cpp")))
    assert text.count('launched(0, "%s")' % KERNEL) == 1
    assert "launched(" not in open(os.path.join(CSRC, "capi_compact.hpp")).read()
    assert "hipLaunchKernelGGL" not in open(os.path.join(CSRC, "capi_compact.hpp")).read()


def test_path_names_are_those_of_before():
    """sp_path_name gained no bit: the last defined one is bit 36 (sweep_narrow_group)"""
    import ctypes as C
    import sdk_amd
    L = C.CDLL(sdk_amd.library_path())
    L.sp_path_name.restype = C.c_char_p
    assert L.sp_path_name(36) == b"sweep_narrow_group" and L.sp_path_name(37) is None
    hdr = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert len(re.findall(r"^\s*PATH_[A-Z0-9_]+ = 1ull << \d+", hdr, flags=re.M)) == 37
