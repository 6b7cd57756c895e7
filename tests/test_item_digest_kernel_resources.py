"""Compile-time guard on the kernels of the per-item digests (sp_db_item_digests), by the method of
tests/test_db_digest_kernel_resources.py: hipcc cross-compiles db.hip (db_item_digest.hpp: the 8-byte, PACKED and sparse kernels) and
sweep_planar.hip (db_item_digest_planar.hpp: k_item_digest_planar) for gfx950, no GPU needed, and the numbers are read from the code
objects' metadata.  Every new kernel uses no scratch, spills nothing and has the workgroup size it declares.

Static LDS: the dense kernels keep their sums in registers and read each row key once, from the table in the read buffer, when a sum
is finished -- no LDS at all.  The sparse kernel reduces a workgroup to its item's one pair: the reduction area of one pair per thread
(4 KiB) and no row-key table (an item has one row; its two keys are computed in place).

Register bounds, from what a thread holds and not from what the compiler happened to give (64-bit values take two registers):
  * k_item_digest_words8: 8 rows x 2 lanes of sums (32), the 8 words of a z in flight (16), two column keys and the mix's temporaries
    (12), the column's address, strides and indices (12): 72 -> bound 96, five waves per SIMD.
  * k_item_digest_packed: 4 row pairs x 4 words x 2 lanes of sums (64), the 4 units' 7 dwords in flight (28), four column keys (8), the
    four words being unpacked (8), the unit address and indices (10): 118 -> bound 128, four waves per SIMD.
  * k_item_digest_planar: 8 rows x 2 lanes of sums (32), the 8 eight-byte pieces in flight (16), their 8 addresses (16), two column keys
    and the mix's temporaries (12), the word being assembled and indices (12): 88 -> bound 112.
  * k_item_digest_sparse: a few words in flight, one pair of sums, the per-word column keys: the 64 of k_digest_sparse.
In no case is the bound above 128 (four waves per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "sdk_amd", "csrc")
REDUCTION = 2 * 256 * 8
# kernel -> (source file, workgroup size, static LDS bytes at most, VGPRs at most)
KERNELS = {"k_item_digest_words8": ("db.hip", 256, 0, 96),
           "k_item_digest_packed": ("db.hip", 256, 0, 128),
           "k_item_digest_sparse": ("db.hip", 256, REDUCTION, 64),
           "k_item_digest_planar": ("sweep_planar.hip", 256, 0, 112)}
LAUNCHED_IN = ("db_item_digest.hpp", "db_item_digest_planar.hpp", "db_digest.hpp", "db_digest_planar.hpp", "sweep_planar.hip", "db.hip")


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
def test_item_digest_kernel_resources(kernels, kernel):
    src, wg, lds, vgprs = KERNELS[kernel]
    assert vgprs <= 128
    found = [k for (s, name), k in kernels.items() if s == src and kernel in name]
    assert len(found) == 1, "%s: %d kernels of that name in %s" % (kernel, len(found), src)
    k = found[0]
    print(kernel, k)
    assert k["private_segment_fixed_size"] == 0, "%s: scratch" % kernel
    assert k["vgpr_spill_count"] + k["sgpr_spill_count"] == 0, "%s: spilled registers" % kernel
    assert k["max_flat_workgroup_size"] == wg, kernel
    assert k["group_segment_fixed_size"] <= lds, "%s: %d bytes of static LDS" % (kernel, k["group_segment_fixed_size"])
    assert (k["group_segment_fixed_size"] > 0) == (lds > 0), kernel
    assert k["vgpr_count"] <= vgprs, "%s: %d VGPRs, bound %d" % (kernel, k["vgpr_count"], vgprs)


def test_item_digests_add_no_path_bit():
    """the kernels report through launched(0, name), as the other kernels of db.hip do: sp_path_name has no bit for them, so no flow
    of tests/test_gpu_hardened_buffers.py is owed.  Each name is launched from exactly one place -- k_digest_keys, which a call's
    first launch reuses through launch_digest_keys, among them -- and the host side launches nothing itself."""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in LAUNCHED_IN)
    for name in list(KERNELS) + ["k_digest_keys"]:
        assert text.count('launched(0, "%s")' % name) == 1, name
    assert text.count("hipLaunchKernelGGL(k_digest_keys") == 1
    assert "launched(" not in open(os.path.join(CSRC, "capi_item_digest.hpp")).read()
