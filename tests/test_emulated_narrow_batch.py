"""The narrow database's group flow (k_sweep_narrow_batch and GroupedFlow of sp_process_query_batch on an 8-byte database) on the
emulated device: a named subset of tests/test_gpu_narrow_batch.py, byte and word comparisons, run in a child process against
tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB), as tests/test_emulated_sparse_batch.py runs the sparse file.  Plain build.
Stream orders as unkind as the flow's own events allow: the pass is handed from every member's stream to the leader's and back."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_narrow_batch.py"
# the shapes with nu_1 <= 6 at B = 8 and B = 2: (4, 1) mostly idle threads, (6, 6) num_per = 64, (6, 0) not the group pass's;
# the switch-off case (lists of 5: the B = 8 body with dead slots)
FLOW_SUBSET = "(test_shapes and (nu4_1 or nu6_6 or nu6_0)) or test_switch_off_gives_the_same_bytes"
# the pass alone at (6, 6), B = 2 .. 8, largest words and random ones, a fold after every product / every second / the default
PASS_SUBSET = "test_pass_alone_accumulator_edges and nu6_6"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_narrow_group_flow_on_the_emulated_device(emulated):
    assert _run(emulated, FLOW_SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=4, test_file=FILE) >= 4


def test_narrow_group_pass_alone_on_the_emulated_device(emulated):
    assert _run(emulated, PASS_SUBSET, at_least=6, test_file=FILE) >= 6
