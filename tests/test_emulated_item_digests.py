"""CPU checks of the per-item digests (sp_db_item_digests; tests/test_gpu_item_digests.py is the GPU suite):
  * a subset of that file on the emulated device (tests/emu: the kernels' source compiled for the host), streams in `starve:1` order --
    the order under which a missing wait between the zeroed table, the row keys, the kernels' atomic adds and the copy out fails: the
    synthetic words without the two-chunk shape, the one body on PACKED, a sparse bucket, two planar shards and four sparse shards,
    the corner words and the sparse corner items, the ranges on PACKED (windows of one row among them) and the errors that write
    nothing;
  * the table once more from a C++ program of its own (tests/emu/item_digest_driver.cpp) under AddressSanitizer where the compiler has
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

FILE = "test_gpu_item_digests.py"
SUBSET = ("(test_synthetic_words and not 4pairs-2chunks) "
          "or (test_one_body_every_format and (packed] or sparse] or planar-shards-2 or sparse-shards-4)) "
          "or test_corner_words or test_corner_items_sparse or (test_ranges and packed) or test_errors_write_nothing")
SUBSET_CASES = 6 + 4 + 5 + 1 + 1 + 1


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_item_digests_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=SUBSET_CASES, test_file=FILE, timeout=3000) >= SUBSET_CASES


_PLANAR = {"n": 2, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56, "instances": 1, "db_item_size": 256}
# (config, the driver's format): PACKED words of two chunks, 8-byte words, a planar-resident handle, two planar shards, a sparse bucket
DRIVER = {"packed-8x256": (dict(FAST, nu_1=3, nu_2=8, t_gsw=2, db_item_size=256), "dense"),
          "words8-16x2": (dict(FAST, nu_1=4, nu_2=1, db_item_size=256), "dense"),
          "planar-64x128": (dict(_PLANAR, nu_1=6, nu_2=7), "planar"),
          "planar-shards-128x128": (dict(_PLANAR, nu_1=7, nu_2=7), "planar-shards"),
          "sparse": (dict(FAST, nu_1=6, nu_2=3, db_item_size=256), "sparse")}


@pytest.fixture(scope="module")
def driver(emulated, tmp_path_factory):
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    exe = str(tmp_path_factory.mktemp("item_digest") / "item_digest_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "item_digest_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    return exe


@pytest.mark.parametrize("name", list(DRIVER))
def test_item_digests_stay_inside_their_buffers(driver, tmp_path, name):
    """a database filled, its table taken whole, range by range and plane by plane into blocks of exactly the size a call may write,
    with a shuffled work-item order: the window's table, the row keys, the flags, the slot list and the reduction area are where an
    out-of-bounds access would hide, and the atomic adds must not care for the order.  Every pair == the program's own scalar loop."""
    cfg, fmt = DRIVER[name]
    (tmp_path / "params.json").write_bytes(json.dumps(cfg).encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20261020")
    r = subprocess.run([driver, str(tmp_path / "params.json"), fmt], capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0 and "equal to the scalar loop" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
