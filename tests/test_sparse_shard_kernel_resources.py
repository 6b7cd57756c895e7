"""Compile-time guard on the scatter-form sparse sweeps (sweep_sparse_scatter.hpp, instantiated from sparse.hip; the method of
tests/test_sparse_batch_kernel_resources.py: hipcc cross-compiles for gfx950, no GPU needed): the single-query kernel and every
instantiation of the group kernel keep their u64 sums in vector registers -- no scratch, no spilled register, at most 256 VGPRs."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
INSTANCES = ("k_sweep_sparse_scatterEN", "k_sweep_sparse_scatter_batchILi2E", "k_sweep_sparse_scatter_batchILi4E",
             "k_sweep_sparse_scatter_batchILi8E")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")
def test_sparse_scatter_sweeps_do_not_spill():
    r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(ROOT, "sdk_amd", "csrc", "sparse.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for block in r.stdout.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        for frag in INSTANCES:
            if frag in name:
                seen.add(frag)
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
                spilled = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) + int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
                vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
                print(name, "vgprs", vgprs, "scratch", scratch, "spilled", spilled)
                assert scratch == 0, "%s: %d bytes of scratch per lane" % (name, scratch)
                assert spilled == 0, "%s: %d spilled registers" % (name, spilled)
                assert vgprs <= 256, "%s: %d VGPRs" % (name, vgprs)
    assert seen == set(INSTANCES), "instantiations not found: %s" % sorted(set(INSTANCES) - seen)
