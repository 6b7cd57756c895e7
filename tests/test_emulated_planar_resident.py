"""Planar-resident databases (sp_db_create_planar: the writers of planar_resident.hpp, k_sweep_planar with one and with two query
tiles) on the emulated device: a subset of tests/test_gpu_planar_resident.py at 64 x 128, byte comparisons with the oracle, run in a
child process against tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB), as tests/test_emulated_bulk_upsert.py runs the bulk
upserts.  Streams in `starve:1` order: the order under which a missing wait between a group's expansions, its pass and its folds
fails.  The writers and the read-back once more from a C++ program of its own under AddressSanitizer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_planar_resident.py"
# load_items / read_ref; lists of 1, 3, 8 and 11 (each with a single query); upserts one by one and as one body; the faulty third
# record; the switches after creation, refused creations and the entry points that refuse the handle
SUBSET = ("(test_load_items_reads_back and 64x128) or (test_every_group_size and 64x128 and (B01 or B03 or B08 or B11)) "
          "or (test_upserts_in_place and 64x128) or test_faulty_third_record_applies_the_prefix "
          "or test_switches_after_creation_change_nothing or test_creation_is_refused_where_the_format_does_not_exist "
          "or test_entry_points_that_refuse_a_planar_handle")


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_planar_resident_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=10, test_file=FILE) >= 10


def test_planar_writers_stay_inside_their_buffers(emulated, tmp_path, oracle_mod):
    """an item file into a planar-resident handle, then the edit list as one body, from a C++ program of its own
    (tests/emu/planar_resident_driver.cpp, no Python in the process) linked against the AddressSanitizer build where there is one, with
    a shuffled work-item order: the staged words, the quad and cell tables and the planar entries written are where an out-of-bounds
    access would hide.  Once through one upload window and once through windows of 1 KiB, every word read back == the oracle's
    load_db_from_bytes of the edited file."""
    import json
    import types
    from test_gpu_planar_resident import _body, _cfg, _edits
    cfg = _cfg(6, 7)
    o = oracle_mod.Params(cfg)
    blob = np.random.default_rng(13).integers(0, 256, o.num_items * o.db_item_size, dtype=np.uint8)
    c = types.SimpleNamespace(o=o, npr=o.num_per, d0=o.dim0, isz=o.db_item_size, blob=blob)
    _, recs, after = _edits(c)
    exp = o.load_db_from_bytes(after.tobytes()).reshape(4, 2048, c.npr, c.d0)
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    files = {"params.json": json.dumps(cfg).encode(), "items.bin": blob.tobytes(), "body.bin": _body(recs),
             "expected.bin": np.ascontiguousarray(exp[:, (0, 9, 2047)], dtype=np.uint64).tobytes()}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    exe = str(tmp_path / "planar_resident_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "planar_resident_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20260926")
    r = subprocess.run([exe] + [str(tmp_path / f) for f in files] + [str(len(recs)), str(512 << 20), "1024"], capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "2 runs" in r.stdout and "all words equal to the oracle's" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
