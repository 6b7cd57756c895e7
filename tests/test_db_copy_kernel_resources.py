"""Compile-time guard on the writers of the item copy (sp_db_copy_items), by the method of
tests/test_item_readback_kernel_resources.py: hipcc cross-compiles db.hip (db_copy.hpp: the 8-byte and PACKED scatters),
sweep_planar.hip (db_copy_planar.hpp: k_planar_scatter_items) and sparse.hip (db_copy_sparse.hpp: k_items_copy_slots) for gfx950, no
GPU needed, and the numbers are read from the code objects' metadata.  Every kernel uses no scratch, spills nothing and has the
workgroup size it declares; its static LDS is no larger than the tile of the gather it inverts -- a 32 x 33 tile of words for the
8-byte scatter, a 256 x 17 tile for the PACKED and the planar one -- and the slot copy has none.
Register bounds, by the gathers' argument -- from what a thread holds, not from what the compiler happened to give: the 8-byte scatter
holds four words and their addresses, the PACKED one a quad's record (6 values), its four words (8 registers), the seven dwords of
the lane group it merges and one unit address: 64 registers, eight waves per SIMD.  The planar scatter holds a cell's 16 limbs of one
modulus, the four-dword entry it merges and the cell's mask and addresses: 128 registers, the class of k_planar_gather.  The slot copy
holds one 16-byte piece and two addresses: 64."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
# kernel -> (source file, the header that launches it, workgroup size, static LDS bytes at most, VGPRs at most)
KERNELS = {"k_items_scatter_words8": ("db.hip", "db_copy.hpp", 256, 32 * 33 * 8, 64),
           "k_items_scatter_packed": ("db.hip", "db_copy.hpp", 256, 256 * 17 * 8, 64),
           "k_planar_scatter_items": ("sweep_planar.hip", "sweep_planar.hip", 256, 256 * 17 * 8, 128),
           "k_items_copy_slots": ("sparse.hip", "db_copy_sparse.hpp", 256, 0, 64)}


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
def test_copy_kernel_resources(kernels, kernel):
    src, _, wg, lds, vgprs = KERNELS[kernel]
    found = [k for (s, name), k in kernels.items() if s == src and kernel in name]
    assert len(found) == 1, "%s: %d kernels of that name in %s" % (kernel, len(found), src)
    k = found[0]
    assert k["private_segment_fixed_size"] == 0, "%s: scratch" % kernel
    assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % kernel
    assert k["max_flat_workgroup_size"] == wg, kernel
    assert k["group_segment_fixed_size"] <= lds, "%s: %d bytes of static LDS" % (kernel, k["group_segment_fixed_size"])
    assert (k["group_segment_fixed_size"] > 0) == (lds > 0), kernel
    assert k["vgpr_count"] <= vgprs, "%s: %d VGPRs, bound %d" % (kernel, k["vgpr_count"], vgprs)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_copy_adds_no_path_bit(kernel):
    """the kernels report through launched(0, name), as the read-back kernels do: sp_path_name has no bit for them, so no flow of
    tests/test_gpu_hardened_buffers.py is owed"""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip", ".cpp")))
    assert text.count('launched(0, "%s")' % kernel) == 1, kernel
    assert open(os.path.join(CSRC, KERNELS[kernel][1])).read().count('launched(0, "%s")' % kernel) == 1, kernel
