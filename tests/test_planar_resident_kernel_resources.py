"""Compile-time guard on the kernels of planar-resident databases (the method of tests/test_narrow_batch_kernel_resources.py: hipcc
cross-compiles sweep_planar.hip for gfx950, no GPU needed): the four one-tile instantiations of k_sweep_planar that
launch_sweep_planar_resident launches, and the writers and the read-back of planar_resident.hpp, use no scratch and spill nothing.

Registers of the one-tile pass: within the 256 of its launch bound (two waves per SIMD) in every form, and within what the launcher's
comment and DESIGN section 3 say about occupancy -- at most 160 with the ring of 4 units (three waves per SIMD of 512 registers), at
most 128 with the ring of 2 (four waves per SIMD: two eight-wave workgroups per CU).  All their LDS is the launcher's dynamic
nj * 128 bytes.  The two-tile instantiations keep the limits of tests/test_kernel_resources.py, which checks them itself."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
# k_sweep_planar<NBUF, QT = 1, DIAG = 0, MINWG = 2, WAVES>: mangled template arguments -> VGPR bound
ONE_TILE = {"k_sweep_planarILi4ELi1ELi0ELi2ELi8EE": 160, "k_sweep_planarILi2ELi1ELi0ELi2ELi8EE": 128,
            "k_sweep_planarILi4ELi1ELi0ELi2ELi4EE": 160, "k_sweep_planarILi2ELi1ELi0ELi2ELi4EE": 128}
WRITERS = {"k_planar_from_ref": 128, "k_planar_synth": 128, "k_planar_from_stage": 128, "k_planar_put_items": 64, "k_planar_read": 64}


@pytest.fixture(scope="module")
def kernels():
    if shutil.which(HIPCC) is None:
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(CSRC, "sweep_planar.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for block in r.stdout.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = dict({key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                          for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "group_segment_fixed_size", "max_flat_workgroup_size")}, agpr_count=int(block.split()[0]))
    return out


def _check(kernels, frags):
    seen = set()
    for name, k in kernels.items():
        for frag, bound in frags.items():
            if frag in name:
                seen.add(frag)
                assert k["private_segment_fixed_size"] == 0, "%s: scratch" % name
                assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % name
                assert k["vgpr_count"] <= 256, "%s: %d VGPRs" % (name, k["vgpr_count"])
                assert k["vgpr_count"] <= bound, "%s: %d VGPRs, bound %d" % (name, k["vgpr_count"], bound)
                assert k["group_segment_fixed_size"] == 0, "%s: static LDS" % name
    assert seen == set(frags), "instantiations not found: %s" % sorted(set(frags) - seen)


def test_one_tile_planar_pass_resources(kernels):
    _check(kernels, ONE_TILE)
    for name, k in kernels.items():
        if any(frag in name for frag in ONE_TILE):
            assert k["max_flat_workgroup_size"] == (512 if "Li8EE" in name else 256), name
            assert k["agpr_count"] == 0, "%s: accumulators parked in AGPRs" % name


def test_planar_writers_and_read_back_resources(kernels):
    _check(kernels, WRITERS)


def test_one_tile_lds_is_the_default_limit_at_512_rows():
    """the launcher's dynamic LDS: nj * 128 bytes, 64 KiB at the largest row count the layout takes"""
    text = open(os.path.join(CSRC, "sweep_planar.hip")).read()
    assert "const size_t lds = (size_t)d.nj * 128;   // one tile's query planes of one z-row" in text
    assert 512 * 128 == 65536
