"""Compile-time guard on the kernels of the item read-back (sp_db_read_items), by the method of
tests/test_planar_shards_kernel_resources.py: hipcc cross-compiles db.hip (item_readback.hpp: the two gathers and the decode) and
sweep_planar.hip (planar_resident.hpp: k_planar_gather) for gfx950, no GPU needed, and the numbers are read from the code objects'
metadata.  Every new kernel uses no scratch, spills nothing, has the workgroup size it declares, and its static LDS is what its tile
needs: a 32 x 33 tile of words, a 256 x 17 tile, and the two transform buffers plus the coefficient array of the decode.
Register bounds, from what a thread holds and not from what the compiler happened to give: the two PACKED / 8-byte gathers keep a
handful of words and addresses -- 64 registers, eight waves per SIMD; the planar gather keeps the 8 sixteen-byte operands it has
loaded and the 32 limbs it builds from them, the decode two sets of 8 residues beside the transform's temporaries -- 128 registers,
four waves per SIMD, the class of k_db_encode."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
N = 2048
LDS_WORDS = N + N // 8
# kernel -> (source file, workgroup size, static LDS bytes at most, VGPRs at most)
KERNELS = {"k_items_gather_words8": ("db.hip", 256, 32 * 33 * 8, 64),
           "k_items_gather_packed": ("db.hip", 256, 256 * 17 * 8, 64),
           "k_items_decode": ("db.hip", 256, 2 * LDS_WORDS * 4 + N * 4 + 16, 128),
           "k_planar_gather": ("sweep_planar.hip", 256, 256 * 17 * 8, 128)}


@pytest.fixture(scope="module")
def kernels():
    if shutil.which(HIPCC) is None:
        pytest.skip("no hipcc")
    out = {}
    for src in sorted({v[0] for v in KERNELS.values()}):
        r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                            os.path.join(CSRC, src)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for block in r.stdout.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            out[(src, name)] = {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                                for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                            "group_segment_fixed_size", "max_flat_workgroup_size")}
    return out


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_read_back_kernel_resources(kernels, kernel):
    src, wg, lds, vgprs = KERNELS[kernel]
    found = [k for (s, name), k in kernels.items() if s == src and kernel in name]
    assert len(found) == 1, "%s: %d kernels of that name in %s" % (kernel, len(found), src)
    k = found[0]
    assert k["private_segment_fixed_size"] == 0, "%s: scratch" % kernel
    assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % kernel
    assert k["max_flat_workgroup_size"] == wg, kernel
    assert 0 < k["group_segment_fixed_size"] <= lds, "%s: %d bytes of static LDS" % (kernel, k["group_segment_fixed_size"])
    assert k["vgpr_count"] <= vgprs, "%s: %d VGPRs, bound %d" % (kernel, k["vgpr_count"], vgprs)


def test_read_back_adds_no_path_bit():
    """the kernels report through launched(0, name), as the other kernels of db.hip do: sp_path_name has no bit for them, so no flow
    of tests/test_gpu_hardened_buffers.py is owed"""
    text = open(os.path.join(CSRC, "item_readback.hpp")).read() + open(os.path.join(CSRC, "sweep_planar.hip")).read()
    for name in KERNELS:
        assert text.count('launched(0, "%s")' % name) == 1, name
