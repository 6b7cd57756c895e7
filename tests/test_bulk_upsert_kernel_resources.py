"""Compile-time guard on the bulk-upsert kernels (the method of tests/test_sparse_batch_kernel_resources.py: hipcc cross-compiles for
gfx950, no GPU needed; resource metadata only): k_sparse_items_encode, k_db_encode_quads and k_planar_patch_items use no scratch and
spill no register -- k_db_encode_quads keeps the quad's 32 words in registers by indexing them statically."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = {"sparse.hip": "k_sparse_items_encode", "db.hip": "k_db_encode_quads", "sweep_planar.hip": "k_planar_patch_items"}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")
@pytest.mark.parametrize("src", list(KERNELS))
def test_bulk_upsert_kernel_uses_no_scratch(src):
    r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(ROOT, "sdk_amd", "csrc", src)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = 0
    for block in r.stdout.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if KERNELS[src] not in name:
            continue
        seen += 1
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spilled = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) + int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        assert scratch == 0, "%s: %d bytes of scratch per lane" % (name, scratch)
        assert spilled == 0, "%s: %d spilled registers" % (name, spilled)
        assert vgprs <= 256, "%s: %d VGPRs" % (name, vgprs)
    assert seen == 1, "%s: %d kernels named %s" % (src, seen, KERNELS[src])
