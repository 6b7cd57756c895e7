"""CPU checks of the compact client registry (tests/test_gpu_compact_clients.py is the GPU suite):
  * a subset of that file on the emulated device (tests/emu: the kernels' source compiled for the host), streams in `starve:1` order --
    the order under which a missing wait between the raw image, the transform, the derived layouts and the first query that reads a
    slot fails: the keystream, expansion == deserialization on FAST and on packing version 1, slot reuse, the registry with two slots
    and the registry under threads;
  * the expansion once more from a C++ program of its own (tests/emu/compact_clients_driver.cpp) under AddressSanitizer where the
    compiler has its shared runtime -- the program is linked against the sanitized library, nothing is preloaded."""
import json
import os
import subprocess
import sys

import pytest

from conftest import FAST, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_compact_clients.py"
SUBSET = ("test_device_keystream or (test_expansion_equals_deserialization and (fast] or v1)) or test_slot_reuse "
          "or test_registry_with_two_slots or test_registry_default or test_registry_json or test_registry_under_threads")
SUBSET_CASES = 5 + 2 + 1 + 3 + 1


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_compact_clients_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=SUBSET_CASES, test_file=FILE, timeout=3000) >= SUBSET_CASES


# the wire layouts: expansion right on the wire, none (packing version 1), four-row packing matrices, no expansion matrices at all
DRIVER = {"fast": FAST,
          "v1": dict(FAST, version=1),
          "n3": {"n": 3, "nu_1": 4, "nu_2": 2, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
                 "instances": 1, "db_item_size": 18432},
          "direct": {"n": 2, "nu_1": 4, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 8, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
                     "instances": 1, "db_item_size": 256, "direct_upload": 1}}


@pytest.fixture(scope="module")
def driver(emulated, tmp_path_factory):
    asan = bool(emu_build.ASAN_RUNTIME)
    lib = emu_build.build(asan=True) if asan else emulated
    exe = str(tmp_path_factory.mktemp("compact_clients") / "compact_clients_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "compact_clients_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    return exe


@pytest.mark.parametrize("name", list(DRIVER))
def test_expansion_stays_inside_its_buffers(driver, tmp_path, name):
    """three clients expanded into a fresh handle and into two slots, the device keystream read into blocks of exactly `count` words,
    with a shuffled work-item order: the staging buffer, the table, the wire image and the slot's three layouts are where an
    out-of-bounds access would hide.  Every expansion == the program's own scalar restatement of the image."""
    (tmp_path / "params.json").write_bytes(json.dumps(DRIVER[name]).encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20261019")
    r = subprocess.run([driver, str(tmp_path / "params.json")], capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0 and "equal to the scalar restatement" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
