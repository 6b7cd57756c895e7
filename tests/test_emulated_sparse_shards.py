"""Row shards of a sparse bucket on the emulated device: the small shapes of tests/test_gpu_sparse_shards.py -- every scatter-form
kernel body against k_sweep_sparse on an unsharded bucket, word for word, and the flow by hand (scatter sweeps, the test's own sum,
local folds, gathered finish) against the oracle -- run in a child process against tests/emu/_build/libspiral_emu.so
(SPIRAL_HIP_LIB), as tests/test_emulated_sparse_batch.py runs the group flow.  Stream orders as unkind as the flow's own events allow."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_sparse_shards.py"
# case 2 at nu_1 <= 8: the single-query kernel in both exchange forms and the group kernel's B = 2 / 4 / 8 bodies, dead slots included,
# on every shard of four buckets (4 + 20 tests); case 3: the bucket with an empty residue class of columns at G = 2 (1 test)
SUBSET = "test_single_query_sweeps or test_group_sweep or (test_flow_by_hand and 2-class-1-empty)"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_sparse_shards_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=25, test_file=FILE) >= 25
