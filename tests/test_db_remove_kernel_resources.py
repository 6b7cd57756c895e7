"""Compile-time guard on the kernels of the item removal (sp_db_remove_items), by the method of
tests/test_db_copy_kernel_resources.py: hipcc cross-compiles db.hip (db_remove.hpp: the 8-byte and PACKED clears), sweep_planar.hip
(db_remove_planar.hpp: k_planar_clear_items) and sparse.hip (db_remove_sparse.hpp: k_sparse_move_slots) for gfx950, no GPU needed, and
the numbers are read from the code objects' metadata.  Every kernel uses no scratch, spills nothing, has the workgroup size it
declares and no LDS at all: nothing is staged, a thread goes from its record straight to the resident bytes it owns.
The register counts are pinned to what the code objects report as built -- the 8-byte clear 34 (a record's index and eight store
addresses), the PACKED clear 33 (a quad's record, seven keep masks, the seven dwords of a lane group and a unit address), the planar
clear 33 (a cell's record, four byte masks, one four-dword entry and its index), the slot move 6 (one 16-byte piece and two offsets):
all far inside 64, eight waves per SIMD.  More than the pin is a regression to look at; fewer is fine."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
# kernel -> (source file, the file that launches it, workgroup size, VGPRs as built)
KERNELS = {"k_items_clear_words8": ("db.hip", "db_remove.hpp", 256, 34),
           "k_items_clear_packed": ("db.hip", "db_remove.hpp", 256, 33),
           "k_planar_clear_items": ("sweep_planar.hip", "sweep_planar.hip", 256, 33),
           "k_sparse_move_slots": ("sparse.hip", "db_remove_sparse.hpp", 256, 6)}


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
def test_remove_kernel_resources(kernels, kernel):
    src, _, wg, vgprs = KERNELS[kernel]
    found = [k for (s, name), k in kernels.items() if s == src and kernel in name]
    assert len(found) == 1, "%s: %d kernels of that name in %s" % (kernel, len(found), src)
    k = found[0]
    assert k["private_segment_fixed_size"] == 0, "%s: scratch" % kernel
    assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % kernel
    assert k["max_flat_workgroup_size"] == wg, kernel
    assert k["group_segment_fixed_size"] == 0, "%s: %d bytes of static LDS" % (kernel, k["group_segment_fixed_size"])
    assert k["vgpr_count"] <= vgprs, "%s: %d VGPRs, pinned at %d" % (kernel, k["vgpr_count"], vgprs)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_removal_adds_no_path_bit(kernel):
    """the kernels report through launched(0, name), as the copy's do: sp_path_name has no bit for them, so no flow of
    tests/test_gpu_hardened_buffers.py is owed"""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip", ".cpp")))
    assert text.count('launched(0, "%s")' % kernel) == 1, kernel
    assert open(os.path.join(CSRC, KERNELS[kernel][1])).read().count('launched(0, "%s")' % kernel) == 1, kernel
