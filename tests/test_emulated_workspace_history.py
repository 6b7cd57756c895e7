"""Flows on workspaces that other flows have used (tests/test_gpu_workspace_history.py) on the emulated device: a named subset of the
walks, byte comparisons with the oracle, run in a child process against tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB), as
tests/test_emulated_hardened_buffers.py runs its file.  Plain build: the walks need no instrument, only one Params handle that lives
through them."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_workspace_history.py"
# What the emulated device runs is cut so that this file takes less time than tests/test_emulated_hardened_buffers.py does in the same
# run (35 s beside 42 s); the GPU runs every step.
# Walk 1 of family S over five steps that a leaked zero_shortcuts, sparse index or layout changes: single queries on the sparse bucket
# and on the dense handle with all-zero columns, the /update-row body, a swept and abandoned bucket query, a bucket query refused on
# the dense handle.  (The whole walk 1 of S, 14 steps, takes 31 s here; left to the GPU: bench_sweep before a normal finish and the
# other eight refused and abandoned steps.)
WALK_1_SPARSE = "test_walk_emulated_famS"
# The reduced walk 1 of family P, cut to four steps: the single query on PACKED words, the sharded flow by hand at G = 2 (two
# workspaces), fold_ciphertexts and fold_ciphertexts_fused one level deeper than nu_2 (fold_mats and fold_mats_w are regrown).
# (test_walk_reduced_famP, the fourteen steps the GPU runs, takes 71 s here: the 8-byte single query, both fold exports at nu_2 and
# the abandoned and refused steps are left to the GPU.)
WALK_1_PACKED = "test_walk_emulated_famP"
# Family S's walk 2 around the sparse group list of five (five workspaces) with the single queries on the bucket and on the dense
# handle between the lists.  (All 22 steps of test_walk_many_workspaces[famS-bucket-list5-group] take 38 s here.)
WALK_2_SPARSE_GROUP = "test_walk_many_workspaces_emulated_famS"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_walks_of_the_sparse_family_on_the_emulated_device(emulated):
    assert _run(emulated, "%s or %s" % (WALK_1_SPARSE, WALK_2_SPARSE_GROUP), at_least=2, test_file=FILE) >= 2


def test_reduced_walk_1_of_the_packed_family_on_the_emulated_device(emulated):
    assert _run(emulated, WALK_1_PACKED, at_least=1, test_file=FILE) >= 1
