"""CPU checks of planar row shards (sp_db_create_planar_shard; tests/test_gpu_planar_shards.py is the GPU suite):
  * shape A of that file (64 local rows, G = 2) on the emulated device (tests/emu: the kernels' source compiled for the host), streams
    in `starve:1` order -- the order under which a missing wait between a group's expansions, its pass and the members' folds fails:
    loaders and read-back, the group pass with one query tile and two (B = 1, 8, 11) against the PACKED shards' partial buffers, the
    /update-row body on every rank, and the errors that enqueue nothing;
  * the list over PROCESS ranks with the shared-memory stand-in for RCCL (the loopback world of the GPU suite hands device pointers to
    torch, which the emulated device cannot serve); worlds of 4 and 8 only under SPIRAL_EMU_LONG=1;
  * the writers once more from a C++ program of its own (tests/emu/planar_shard_driver.cpp) under AddressSanitizer where the compiler
    has its shared runtime -- the program is linked against the sanitized library, nothing is preloaded."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

LONG = os.environ.get("SPIRAL_EMU_LONG") == "1"
FILE = "test_gpu_planar_shards.py"
SUBSET = ("(test_loaders_read_back_on_every_shard and shapeA) or test_limbs_above_q_are_reduced_as_on_packed "
          "or (test_group_pass_leaves_the_packed_shards_partials and shapeA and (B01 or B08 or B11)) "
          "or test_the_same_update_row_body_on_every_rank or test_creation_is_refused_where_the_format_does_not_exist "
          "or test_errors_enqueue_nothing_and_enter_no_collective")


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_planar_shards_on_the_emulated_device(emulated):
    assert _run(emulated, SUBSET, {"SPIRAL_EMU_STREAMS": "starve:1"}, at_least=8, test_file=FILE, timeout=3000) >= 8


@pytest.mark.parametrize("world,streams", [(2, "starve:1")] + ([(4, "starve:2"), (8, "eager")] if LONG else []))
def test_list_over_process_ranks(emulated, tmp_path, world, streams):
    """sp_process_queries_sharded_batched on planar shards with the ranks as processes: a list of 9 of two clients with group = 0 (16: two
    query tiles), its first two with group = 8 (one tile) and through the per-query list call, against the oracle; sp_comm_describe's collective counts"""
    id_file = str(tmp_path / "comm_id")
    env = dict(os.environ, SPIRAL_HIP_LIB=emulated, SPIRAL_EMU_THREADS="2" if world <= 4 else "1", SPIRAL_EMU_STREAMS=streams)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_emu_planar_shards_rank.py"), str(r), str(world), id_file],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=3000)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, (pr, out) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0, "rank %d:\n%s" % (r, out[-3000:])
    assert "planar-shards-ok" in outs[0]


def test_planar_shard_writers_stay_inside_their_buffers(emulated, tmp_path, oracle_mod):
    """an item file into both planar shards of A, then the edit list as one body handed to each, from a C++ program of its own linked
    against the AddressSanitizer build where there is one, with a shuffled work-item order: the staged words, the quad and cell
    tables and the planar entries -- at permuted columns, inside a row window -- are where an out-of-bounds access would hide.  Once
    through one upload window and once through windows of 1 KiB, every word read back == the oracle's load_db_from_bytes of the
    edited file."""
    from test_gpu_planar_resident import _body, _edits
    from test_gpu_planar_shards import _cfg
    cfg = _cfg(7, 7)
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
    exe = str(tmp_path / "planar_shard_driver")
    so_dir = os.path.dirname(lib)
    subprocess.check_call([emu_build.CLANG, "-std=c++17", "-O1"] + (["-fsanitize=address", "-shared-libasan"] if asan else []) +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "planar_shard_driver.cpp"),
                           "-L", so_dir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + so_dir,
                           "-Wl,-rpath," + os.path.dirname(emu_build.ASAN_RUNTIME or so_dir), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1",
               SPIRAL_EMU_SCHEDULE="random:20260926")
    r = subprocess.run([exe] + [str(tmp_path / f) for f in files] + [str(len(recs)), "2", str(512 << 20), "1024"], capture_output=True,
                       text=True, timeout=1800, env=env)
    assert r.returncode == 0 and "2 runs" in r.stdout and "all words equal to the oracle's" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
