"""CPU checks of the item removal (sp_db_remove_items / _range, sp_db_sparse_trim, sp_server_remove_items;
tests/test_gpu_db_remove.py is the GPU suite):
  * a subset of that file on the emulated device (tests/emu: the kernels' source compiled for the host), streams in `starve:1` order:
    one case per kernel (PACKED, 8-byte words, planar-resident and planar shards, sparse and sparse shards, nine planes), the sparse
    slot cases, the record lists across small windows -- the batch copy's second launch among them --, trim and the errors that
    write nothing;
  * the removal once more from a C++ program of its own (tests/emu/db_remove_driver.cpp) under AddressSanitizer where the compiler has
    its shared runtime -- the program is linked against the sanitized library, nothing is preloaded."""
import json
import os
import subprocess
import sys

import pytest

from conftest import FAST, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_db_remove.py"
SUBSET = ("(test_every_form and (A-packed] or B-words8] or A-planar] or C-planar-shards] or A-sparse] or A-sparse-shards] or "
          "A-column-shards] or N9-packed] or N9-sparse])) or test_sparse_slot_cases or test_sparse_absent_keys_and_upserts_after or "
          "test_sparse_remove_every_key or test_record_lists_across_windows or test_trim or test_errors_write_nothing")


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_db_remove_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=24, test_file=FILE, timeout=3000) >= 24


# (configuration, chain of the driver): a 16 x 128 shape that is PACKED, sparse-capable and has an 8-byte form; planar shards of 64 rows
DRIVER = {"packed-words8-sparse": dict(FAST, nu_1=4, nu_2=7, db_item_size=256),
          "planar-shards": {"n": 2, "nu_1": 7, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8,
                            "t_exp_right": 56, "instances": 1, "db_item_size": 256}}


@pytest.fixture(scope="module")
def driver(emulated, tmp_path_factory):
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    exe = str(tmp_path_factory.mktemp("db_remove") / "db_remove_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "db_remove_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    return exe


@pytest.mark.parametrize("chain", list(DRIVER))
def test_removal_stays_inside_its_buffers(driver, tmp_path, chain):
    """a PACKED, an 8-byte and a sparse handle of one shape, and a pair of planar row shards, lose one list -- single positions of a
    quad, a whole quad, rows of one 16-row cell, the corners of the shape, a run across a row end -- through one window and through
    one-record windows (db_load_window = 1), with a shuffled work-item order; the bucket then loses a range and is trimmed twice.
    The last record of a list, a workgroup's unused lanes and the tail of a shrunk store are where an out-of-bounds access would hide.
    Every word of every handle == the words that went in, zero where removed."""
    windows = [512 << 20, 1]
    (tmp_path / "params.json").write_bytes(json.dumps(DRIVER[chain]).encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20261021")
    r = subprocess.run([driver, str(tmp_path / "params.json"), chain] + [str(w) for w in windows],
                       capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0 and "%d runs" % len(windows) in r.stdout and "every word equal to the expected words" in r.stdout, (
        r.stdout[-1500:], r.stderr[-4000:])
