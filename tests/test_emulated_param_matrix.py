"""The shipped parameter sets (tests/param_matrix.py: 9, 12 and 16 planes, n = 3 and 4, p = 512, packing version 1) on the emulated
device: a subset of tests/test_gpu_param_matrix.py, byte comparisons with the oracle, run in a child process against
tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB) as tests/test_emulated_planar_resident.py runs its GPU file.  Streams in `starve:1`
order: the order under which a missing wait between a group's expansions, its pass and its folds fails.
  * cells a (8-byte narrow handle, the narrow group pass) and b (sparse bucket, a list of 3, read_items) on all four sets;
  * cell d on N3 -- a planar-resident database of nine planes: read_ref, lists of 1, 8 and 9, the edit body, the digest; no longer
    than the longest case of tests/test_emulated_planar_resident.py, the oracle's 18 queries included, so it is in the default suite;
  * cell e's sparse shards on N3 with the ranks as processes and the shared-memory stand-in for RCCL (the loopback world of the GPU
    suite hands device pointers to torch, which the emulated device cannot serve)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_param_matrix.py"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_param_matrix_narrow_and_sparse_cells_on_the_emulated_device(emulated):
    assert _run(emulated, "test_a_narrow_handle or test_b_sparse_bucket", {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=8, test_file=FILE) >= 8


def test_param_matrix_planar_resident_n3_on_the_emulated_device(emulated):
    assert _run(emulated, "test_d_planar_resident and N3", {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=1, test_file=FILE, timeout=3000) >= 1


def test_sparse_shards_over_process_ranks(emulated, tmp_path):
    """N3 at (6, 3), two ranks: comm.cpp's per-plane reduce-scatter and gather loops at an odd plane count"""
    world, id_file = 2, str(tmp_path / "comm_id")
    env = dict(os.environ, SPIRAL_HIP_LIB=emulated, SPIRAL_EMU_THREADS="2", SPIRAL_EMU_STREAMS="starve:1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_emu_param_matrix_rank.py"), str(r), str(world), id_file, "N3"],
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
    assert "param-matrix-shards-ok" in outs[0]
