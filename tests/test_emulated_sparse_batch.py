"""The sparse bucket's group flow (k_sweep_sparse_batch and the sparse flow of sp_process_query_batch) on the emulated device:
subsets of tests/test_gpu_sparse_batch.py, byte comparisons with the oracle, run in a child process against
tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB), as tests/test_emulated_library.py runs the other GPU files.  Stream orders as
unkind as the flow's own events allow: the pass is handed from every member's stream to the leader's and back."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run, long_only  # noqa: E402

FILE = "test_gpu_sparse_batch.py"
# lists of 2 (the B = 2 body) and 3 (the B = 4 body with a dead slot); columns of 256 and 3 items (one fold of the u64 sums) at B = 2
DEFAULT_SUBSET = "(test_group_sizes_and_slots and (2 or 3)) or (test_accumulator_range and nu1_8-256-3)"
ASAN_SUBSET = "test_group_sizes_and_slots and 3"
# cases 2 - 5 at nu_1 <= 8: two column shapes, two plane / gadget configurations, three shortcut buckets, the snapshots (8 tests)
LONG_SUBSET = ("(test_accumulator_range and nu1_8) or test_planes_and_gadgets or test_shortcuts or test_snapshots_follow_upserts")


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_sparse_group_flow_on_the_emulated_device(emulated):
    assert _run(emulated, DEFAULT_SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=3, test_file=FILE) >= 3


def test_sparse_group_pass_stays_inside_its_buffers(emulated):
    """the list of 3 once more under AddressSanitizer: the dead slot's reads and the members' stores stay inside their buffers"""
    if not emu_build.ASAN_RUNTIME:
        pytest.skip("no AddressSanitizer runtime")
    so = emu_build.build(asan=True)
    log = os.path.join(emu_build.BUILD, "asan_sparse_batch_report")
    for f in os.listdir(emu_build.BUILD):
        if f.startswith("asan_sparse_batch_report"):
            os.remove(os.path.join(emu_build.BUILD, f))
    env = {"LD_PRELOAD": emu_build.ASAN_RUNTIME, "SPIRAL_EMU_SCHEDULE": "random:20260926",
           "ASAN_OPTIONS": "detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1:log_path=" + log}
    try:
        _run(so, ASAN_SUBSET, env, at_least=1, test_file=FILE)
    finally:
        reports = [f for f in os.listdir(emu_build.BUILD) if f.startswith("asan_sparse_batch_report")]
        if reports:
            text = open(os.path.join(emu_build.BUILD, reports[0])).read()
            pytest.fail("AddressSanitizer report from the emulated library:\n" + text[:6000])


@long_only
@pytest.mark.parametrize("policy", ["random:5", "random:11"])
def test_sparse_group_flow_cases_on_the_emulated_device(emulated, policy):
    assert _run(emulated, LONG_SUBSET, {"SPIRAL_EMU_STREAMS": policy}, at_least=8, timeout=6000, test_file=FILE) >= 8
