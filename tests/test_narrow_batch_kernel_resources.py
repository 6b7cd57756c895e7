"""Compile-time guard on k_sweep_narrow_batch (the method of tests/test_sparse_batch_kernel_resources.py: hipcc cross-compiles
sweep_planar.hip for gfx950, no GPU needed): the three instantiations keep their B x 8 u64 sums in vector registers -- no scratch,
no spilled register -- within the VGPR bounds that sweep_narrow_batch.hpp states, and all their LDS is the launcher's dynamic
B * 8 KiB + 8 KiB, which stays within 80 KiB so that two workgroups fit a CU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
VGPR_BOUND = {"k_sweep_narrow_batchILi2E": 88, "k_sweep_narrow_batchILi4E": 128, "k_sweep_narrow_batchILi8E": 208}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")
def test_narrow_group_pass_resources():
    r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(CSRC, "sweep_planar.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for block in r.stdout.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        for frag, bound in VGPR_BOUND.items():
            if frag in name:
                seen.add(frag)
                field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))   # noqa: E731
                assert field("private_segment_fixed_size") == 0, "%s: scratch" % name
                assert field("vgpr_spill_count") + field("sgpr_spill_count") == 0, "%s: spilled registers" % name
                assert field("vgpr_count") <= bound, "%s: %d VGPRs, bound %d" % (name, field("vgpr_count"), bound)
                assert field("group_segment_fixed_size") == 0, "%s: static LDS" % name
    assert seen == set(VGPR_BOUND), "instantiations not found: %s" % sorted(set(VGPR_BOUND) - seen)


def test_narrow_group_pass_lds_budget():
    """the launcher's dynamic LDS, from the header's constants: [B][slab rows] 16-byte limb quads + one [256][8] u32 area"""
    text = open(os.path.join(CSRC, "sweep_narrow_batch.hpp")).read()
    rows = int(re.search(r"NARROW_SLAB_ROWS = (\d+);", text).group(1))
    assert "(size_t)B * NARROW_SLAB_ROWS * 16 + 256 * 8 * sizeof(u32)" in text
    assert rows == 512
    assert [b * rows * 16 + 256 * 8 * 4 for b in (2, 4, 8)] == [24 << 10, 40 << 10, 72 << 10]
    assert 8 * rows * 16 + 256 * 8 * 4 <= 80 << 10
