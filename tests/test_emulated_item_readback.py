"""CPU checks of the item read-back (sp_db_read_items, sp_db_export_rows; tests/test_gpu_item_readback.py is the GPU suite):
  * a subset of that file on the emulated device (tests/emu: the kernels' source compiled for the host), streams in `starve:1` order --
    the order under which a missing wait between a window's gather, its decode and the copy out fails: the independent pin on 8-byte and
    PACKED words, every-format read-back on PACKED, planar shards and a sparse bucket, the ranges across small windows with the errors
    that write nothing, and the undecodable words;
  * the read-back once more from a C++ program of its own (tests/emu/item_readback_driver.cpp) under AddressSanitizer where the compiler
    has its shared runtime -- the program is linked against the sanitized library, nothing is preloaded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FAST, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_item_readback.py"
SUBSET = ("(test_oracle_words_read_back_as_the_file and (narrow or packed-ragged-chunk)) "
          "or (test_every_format_reads_back_what_was_written and (packed] or planar-shards-A or sparse])) "
          "or test_ranges_across_small_windows or test_bad_ranges_write_nothing "
          "or test_undecodable_words_are_counted_and_never_exported")


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_item_readback_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=10, test_file=FILE, timeout=3000) >= 10


# a PACKED shape whose 1000-byte items leave ragged chunks and a file 3000 bytes short; 5-byte items in four chunks (the last chunk
# starts past the item, the third holds one byte); planar shards of shape A; a sparse bucket
# (config, bytes the file is short, the driver's format, items per window of the last run: no divisor of the item count, so the last
# window is a shorter one.  Windows of 1 KiB hold one item each; on the planar shards, where a window's gather walks every column of
# its 16-row groups on the emulated device, the one-item windows are left to the ranges of 7.)
DRIVER = {"packed-ragged-short": (dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=1000), 3000, "dense", (1, 5)),
          "words8-5B-spill": (dict(FAST, nu_1=4, nu_2=1, db_item_size=5), 0, "dense", (1, 5)),
          "planar-shards-A": ({"n": 2, "nu_1": 7, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8,
                               "t_exp_right": 56, "instances": 1, "db_item_size": 256}, 0, "planar-shards", (300,)),
          "sparse": (dict(FAST, nu_1=6, nu_2=3, db_item_size=256), 0, "sparse", (1, 5))}


@pytest.fixture(scope="module")
def driver(emulated, tmp_path_factory):
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    exe = str(tmp_path_factory.mktemp("item_readback") / "item_readback_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "item_readback_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    return exe


@pytest.mark.parametrize("name", list(DRIVER))
def test_read_back_stays_inside_its_buffers(driver, tmp_path, name):
    """an item file in, every item back out through one window and through windows of 1 KiB (one item each: the library's smallest),
    in one call and in ranges of 7, with a shuffled work-item order: the LDS tiles' edges, the bit-packing tail of a chunk and the last
    window are where an out-of-bounds access would hide.  Every item == the file's, the export's records too."""
    cfg, short, fmt, per_window = DRIVER[name]
    num_items = 1 << (cfg["nu_1"] + cfg["nu_2"])
    per_item = 8 + cfg["db_item_size"] + (0 if fmt == "sparse" else 4 * 2048 * 8)     # list entry, bytes, gathered words
    windows = [512 << 20] + [1024 if k == 1 else 64 + k * per_item for k in per_window]
    blob = np.random.default_rng(17).integers(0, 256, num_items * cfg["db_item_size"] - short, dtype=np.uint8)
    (tmp_path / "params.json").write_bytes(json.dumps(cfg).encode())
    (tmp_path / "items.bin").write_bytes(blob.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20261019")
    r = subprocess.run([driver, str(tmp_path / "params.json"), str(tmp_path / "items.bin"), fmt] + [str(w) for w in windows],
                       capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0 and "%d runs" % len(windows) in r.stdout and "every item equal to the file's" in r.stdout, (
        r.stdout[-1500:], r.stderr[-4000:])
