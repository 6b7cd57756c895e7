"""Compile-time guard on the scatter form of k_sweep_planar (the pass over a planar row shard, sp_db_create_planar_shard), by the method
of tests/test_planar_resident_kernel_resources.py: hipcc cross-compiles sweep_planar.hip for gfx950, no GPU needed, and the numbers are
read from the code object's metadata.

The eight instantiations launch_sweep_planar_scatter launches -- k_sweep_planar_scatter<NBUF, QT, MINWG, WAVES>, ring of 2 or 4
units, one query tile or two, four or eight waves -- use no scratch, spill nothing and have no static LDS.  Registers: the scatter form
differs from the plain form in the addresses of its epilogue only, so it keeps the plain form's occupancy rules --
  one tile   (launch bound: two waves per SIMD, 256 registers): at most 160 with the ring of 4 (three waves per SIMD of 512 registers),
             at most 128 with the ring of 2 (four), accumulators never parked in AGPRs;
  two tiles  eight waves (two per SIMD): at most 256; four waves (one per SIMD, the unified file of 512): at most 512."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
# mangled template arguments <NBUF, QT, MINWG, WAVES> -> (VGPR bound incl. AGPRs, workgroup size)
SCATTER = {"k_sweep_planar_scatterILi4ELi1ELi2ELi8EE": (160, 512), "k_sweep_planar_scatterILi2ELi1ELi2ELi8EE": (128, 512),
           "k_sweep_planar_scatterILi4ELi1ELi2ELi4EE": (160, 256), "k_sweep_planar_scatterILi2ELi1ELi2ELi4EE": (128, 256),
           "k_sweep_planar_scatterILi4ELi2ELi1ELi8EE": (256, 512), "k_sweep_planar_scatterILi2ELi2ELi1ELi8EE": (256, 512),
           "k_sweep_planar_scatterILi4ELi2ELi1ELi4EE": (512, 256), "k_sweep_planar_scatterILi2ELi2ELi1ELi4EE": (512, 256)}


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


def test_scatter_form_resources(kernels):
    seen = set()
    for name, k in kernels.items():
        for frag, (bound, wg) in SCATTER.items():
            if frag in name:
                seen.add(frag)
                assert k["private_segment_fixed_size"] == 0, "%s: scratch" % name
                assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % name
                assert k["vgpr_count"] <= bound, "%s: %d VGPRs, bound %d" % (name, k["vgpr_count"], bound)
                assert k["group_segment_fixed_size"] == 0, "%s: static LDS" % name
                assert k["max_flat_workgroup_size"] == wg, name
                if "ELi1ELi2E" in frag:
                    assert k["agpr_count"] == 0, "%s: accumulators parked in AGPRs" % name
    assert seen == set(SCATTER), "instantiations not found: %s" % sorted(set(SCATTER) - seen)


def test_scatter_form_is_the_plain_forms_body():
    """one body, two kernels: the flag is a template parameter of sweep_planar_body, not a copy"""
    text = open(os.path.join(CSRC, "sweep_planar.hpp")).read()
    assert text.count("__builtin_amdgcn_mfma_i32_16x16x64_i8(") == 1
    assert "sweep_planar_body<NBUF, QT, DIAG, WAVES, false>(T, d);" in text and "sweep_planar_body<NBUF, QT, 0, WAVES, true>(T, d);" in text
