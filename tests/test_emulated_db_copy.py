"""CPU checks of the item copy (sp_db_copy_items, sp_server_replace_db; tests/test_gpu_db_copy.py is the GPU suite):
  * a subset of that file on the emulated device (tests/emu: the kernels' source compiled for the host), streams in `starve:1` order --
    the order under which a missing wait between a window's gather, its scatter and the patch of a batch copy fails: one pair per
    destination form (PACKED, planar-resident, sparse, 8-byte words, planar shards, sparse shards, column shards), the ranges across
    small windows, and the errors that write nothing;
  * the copy once more from a C++ program of its own (tests/emu/db_copy_driver.cpp) under AddressSanitizer where the compiler has its
    shared runtime -- the program is linked against the sanitized library, nothing is preloaded."""
import json
import os
import subprocess
import sys

import pytest

from conftest import FAST, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_db_copy.py"
SUBSET = ("(test_every_pair_of_forms and (A-sparse-to-packed] or A-packed-to-planar] or A-planar-to-sparse] or B-sparse-to-words8] "
          "or C-packed-to-planar-shards] or A-row-shards-to-sparse-shards] or A-packed-to-column-shards] or S-row-shards-to-packed])) "
          "or test_ranges_across_small_windows or test_errors_write_nothing")


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_db_copy_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=12, test_file=FILE, timeout=3000) >= 12


# (configuration, chain of the driver): a 16 x 128 shape that is PACKED, sparse-capable and has an 8-byte form; planar shards of 64 rows
DRIVER = {"packed-sparse-words8": dict(FAST, nu_1=4, nu_2=7, db_item_size=256),
          "planar-shards-packed": {"n": 2, "nu_1": 7, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8,
                                   "t_exp_right": 56, "instances": 1, "db_item_size": 256}}


@pytest.fixture(scope="module")
def driver(emulated, tmp_path_factory):
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    exe = str(tmp_path_factory.mktemp("db_copy") / "db_copy_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "db_copy_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    return exe


@pytest.mark.parametrize("chain", list(DRIVER))
def test_copy_stays_inside_its_buffers(driver, tmp_path, chain):
    """PACKED -> sparse -> 8-byte words and planar shards -> PACKED, the whole range through one window and a range that crosses two
    row ends through one-item windows (1 KiB: the library's smallest), with a shuffled work-item order: the LDS tiles' edges, a quad or
    a 16-row cell of which one entry is written, and the last window are where an out-of-bounds access would hide.  Every word of the
    destination == the words that went in."""
    windows = [512 << 20, 1024]
    (tmp_path / "params.json").write_bytes(json.dumps(DRIVER[chain]).encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20261021")
    r = subprocess.run([driver, str(tmp_path / "params.json"), chain] + [str(w) for w in windows],
                       capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0 and "%d runs" % len(windows) in r.stdout and "every word equal to the words that went in" in r.stdout, (
        r.stdout[-1500:], r.stderr[-4000:])
