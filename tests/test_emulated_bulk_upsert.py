"""Bulk upserts (sp_db_update_items / sp_db_update_rows: k_sparse_items_encode, k_db_encode_quads, k_planar_patch_items) on the
emulated device: subsets of tests/test_gpu_bulk_upsert.py, comparisons with the oracle, run in a child process against
tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB), as tests/test_emulated_sparse_batch.py runs the sparse group flow."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402
from test_gpu_bulk_upsert import _body, _dense_case  # noqa: E402

FILE = "test_gpu_bulk_upsert.py"
# the mixed sparse body (duplicates, zero-length and short records, an overwrite, a new row), the five faulty bodies, the PACKED dense
# body by quads
DEFAULT_SUBSET = "(test_sparse_mixed_body and inst1) or (test_faulty_third_record and inst1) or (test_dense_body_by_quads and packed)"
PLANAR_SUBSET = "test_planar_copy_follows_one_body"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_bulk_upsert_on_the_emulated_device(emulated):
    assert _run(emulated, DEFAULT_SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=7, test_file=FILE) >= 7


def test_planar_copy_follows_a_body_on_the_emulated_device(emulated):
    """the 64 x 128 database with a standing digit-planar copy: one body, then a list of eleven queries over the patched copy"""
    assert _run(emulated, PLANAR_SUBSET, at_least=1, test_file=FILE) >= 1


def test_quad_descriptors_and_window_offsets_stay_inside_their_buffers(emulated, tmp_path, oracle_mod):
    """the PACKED dense body once more from a C++ program of its own (tests/emu/bulk_upsert_driver.cpp, no Python in the process)
    linked against the AddressSanitizer build where there is one, with a shuffled work-item order: the quad table, the window
    offsets and the lane groups written are where an out-of-bounds access would hide.  Once through one upload window and once
    through windows of 1 KiB (a quad or two each), every word read back == the oracle's load_db_from_bytes of the edited file."""
    import json
    cfg, blob, recs, exp = _dense_case(oracle_mod, "packed")
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    files = {"params.json": json.dumps(cfg).encode(), "items.bin": blob.tobytes(), "body.bin": _body(recs),
             "expected.bin": np.ascontiguousarray(exp[:, (0, 9, 2047)], dtype=np.uint64).tobytes()}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    exe = str(tmp_path / "bulk_upsert_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "bulk_upsert_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20260926")
    r = subprocess.run([exe] + [str(tmp_path / f) for f in files] + [str(len(recs)), str(512 << 20), "1024"], capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "2 runs" in r.stdout and "all words equal to the oracle's" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
