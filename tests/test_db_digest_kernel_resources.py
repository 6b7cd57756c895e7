"""Compile-time guard on the kernels of the database digest (sp_db_digest), by the method of
tests/test_item_readback_kernel_resources.py: hipcc cross-compiles db.hip (db_digest.hpp: the row keys, the 8-byte, PACKED and sparse
kernels) and sweep_planar.hip (db_digest_planar.hpp: k_digest_planar) for gfx950, no GPU needed, and the numbers are read from the code
objects' metadata.  Every new kernel uses no scratch, spills nothing, has the workgroup size it declares, and its static LDS is no more
than the row keys of 1024 rows for both lanes (16 KiB; the PACKED kernel reads them with scalar loads and the sparse kernel's row key
is one per workgroup, so these two keep the reduction area only; none at all in the kernel that writes the keys) plus the reduction area of one pair per thread (4 KiB).
Register bounds, from what a thread holds and not from what the compiler happened to give: a digest thread keeps a few words, two pairs
of sums and addresses -- 64 registers, eight waves per SIMD, for the 8-byte, PACKED and sparse kernels; the planar kernel keeps the
8 sixteen-byte entries it has loaded and the 32 limbs it builds from them -- 128 registers, four waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
R_TABLE = 2 * 1024 * 8
REDUCTION = 2 * 256 * 8
# kernel -> (source file, workgroup size, static LDS bytes at most, VGPRs at most)
KERNELS = {"k_digest_keys": ("db.hip", 256, 0, 64),
           "k_digest_words8": ("db.hip", 256, R_TABLE + REDUCTION, 64),
           "k_digest_packed": ("db.hip", 256, REDUCTION, 64),
           "k_digest_sparse": ("db.hip", 256, REDUCTION, 64),
           "k_digest_planar": ("sweep_planar.hip", 256, R_TABLE + REDUCTION, 128)}
LAUNCHED_IN = ("db_digest.hpp", "db_digest_planar.hpp", "sweep_planar.hip", "db.hip")


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
def test_digest_kernel_resources(kernels, kernel):
    src, wg, lds, vgprs = KERNELS[kernel]
    found = [k for (s, name), k in kernels.items() if s == src and kernel in name]
    assert len(found) == 1, "%s: %d kernels of that name in %s" % (kernel, len(found), src)
    k = found[0]
    assert k["private_segment_fixed_size"] == 0, "%s: scratch" % kernel
    assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % kernel
    assert k["max_flat_workgroup_size"] == wg, kernel
    assert k["group_segment_fixed_size"] <= lds, "%s: %d bytes of static LDS" % (kernel, k["group_segment_fixed_size"])
    assert (k["group_segment_fixed_size"] > 0) == (lds > 0), kernel
    assert k["vgpr_count"] <= vgprs, "%s: %d VGPRs, bound %d" % (kernel, k["vgpr_count"], vgprs)


def test_digest_adds_no_path_bit():
    """the kernels report through launched(0, name), as the other kernels of db.hip do: sp_path_name has no bit for them, so no flow
    of tests/test_gpu_hardened_buffers.py is owed.  Each name is launched from exactly one place."""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in LAUNCHED_IN)
    for name in KERNELS:
        assert text.count('launched(0, "%s")' % name) == 1, name
    assert "launched(" not in open(os.path.join(CSRC, "capi_digest.hpp")).read()
