"""CPU checks of the batched pass over row shards (tests/test_gpu_sharded_batch.py is the GPU suite):
  * the kernel-level tests of that file on the emulated device (tests/emu: the kernels' source compiled for the host), under an
    adversarial stream order -- nothing runs until the host waits, and then everything before stream 1 last -- so that the event
    ordering between the group's pass (first query's stream) and the per-query streams is what makes the bytes right;
  * the list call over PROCESS ranks with the shared-memory stand-in for RCCL (the loopback world of the GPU suite hands device
    pointers to torch, which the emulated device cannot serve: this is the flow-level check without a GPU);
  * the compile-time resource guard of the new kernel (no scratch; registers), in the style of tests/test_kernel_resources.py."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

LONG = os.environ.get("SPIRAL_EMU_LONG") == "1"
long_only = pytest.mark.skipif(not LONG, reason="SPIRAL_EMU_LONG=1 (keeps the CPU suite to a few minutes)")
FILE = "test_gpu_sharded_batch.py"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_group_pass_on_the_emulated_device(emulated):
    """64 x 128, G = 2, groups of 4, 5 and 8, both shards; the fallbacks and the error paths of the stage call"""
    assert _run(emulated, "(test_group_pass_leaves and 64x128-G2 and not planes) or test_group_pass_fallbacks_and_errors",
                {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=4, test_file=FILE) >= 4


def test_group_pass_store_from_registers_on_the_emulated_device(emulated):
    """the other store shape of the kernel (switch batch_scatter_store = 1) writes the same words"""
    assert _run(emulated, "test_group_pass_leaves and 64x128-G2-5", {"SPIRAL_EMU_STREAMS": "starve:1", "SPIRAL_BATCH_SCATTER_STORE": "1"},
                at_least=1, test_file=FILE) >= 1


@long_only
def test_group_pass_larger_shapes_on_the_emulated_device(emulated):
    assert _run(emulated, "test_group_pass_leaves and (128x128-G4 or 256x256-G8-5 or 8planes-8)", {"SPIRAL_EMU_STREAMS": "starve:1"},
                at_least=5, test_file=FILE, timeout=3000) >= 5


@pytest.mark.parametrize("world,streams", [(2, "starve:1")] + ([(4, "starve:2"), (8, "eager")] if LONG else []))
def test_batched_list_over_process_ranks(emulated, tmp_path, world, streams):
    """sp_process_queries_sharded_batched with the ranks as processes: group = 0, 4 and 1, lists of two clients, against the oracle
    and the existing list call; sp_comm_describe's collective counts"""
    id_file = str(tmp_path / "comm_id")
    env = dict(os.environ, SPIRAL_HIP_LIB=emulated, SPIRAL_EMU_THREADS="2" if world <= 4 else "1", SPIRAL_EMU_STREAMS=streams)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_emu_sharded_batch_rank.py"), str(r), str(world), id_file],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=1500)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, (pr, out) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0, "rank %d:\n%s" % (r, out[-3000:])
    assert "sharded-batch-ok" in outs[0]


# kernel name fragment -> (max scratch bytes per lane, max VGPRs): both store shapes of k_sweep_mfma_scatter<2, 2, STORE> run two
# workgroups per CU (256 registers per lane) and keep nothing in scratch
LIMITS = {"k_sweep_mfma_scatterILi2ELi2ELi1E": (0, 256), "k_sweep_mfma_scatterILi2ELi2ELi2E": (0, 256)}


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")
def test_scatter_pass_kernel_does_not_spill():
    r = subprocess.run([HIPCC, "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(ROOT, "sdk_amd", "csrc", "sweep_planar.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for block in r.stdout.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        vgpr = re.search(r"\.vgpr_count:\s+(\d+)", block)
        for frag, (max_scratch, max_vgprs) in LIMITS.items():
            if name and scratch and vgpr and "spiral" in name.group(1) and frag in name.group(1):
                seen.add(frag)
                assert int(scratch.group(1)) <= max_scratch, "%s: %s bytes of scratch per lane" % (name.group(1), scratch.group(1))
                assert int(vgpr.group(1)) <= max_vgprs, "%s: %s VGPRs" % (name.group(1), vgpr.group(1))
    assert seen == set(LIMITS), "kernels not found: %s" % sorted(set(LIMITS) - seen)
