"""One rank of tests/test_emulated_planar_shards.py::test_list_over_process_ranks (TEST INFRASTRUCTURE).

Run as N processes with SPIRAL_HIP_LIB = the emulated build: each loads its PLANAR row shard (sp_db_create_planar_shard), joins the
library's own communicator (the shared-memory stand-in for RCCL, tests/emu/emu_rccl.cpp) and answers the same list of 9 queries of
two clients through sp_process_queries_sharded_batched (group = 0 -- 16 here: one two-tile pass), its first two with group = 8 (a
one-tile pass) and through the per-query list call (the emulated device is several thousand times slower than a CU); rank 0 compares with the oracle and prints 'planar-shards-ok'.  64 rows per shard: shape A of tests/test_gpu_planar_shards.py at world 2.
usage: _emu_planar_shards_rank.py RANK WORLD ID_FILE"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle as oracle_mod  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import FAST  # noqa: E402
from sdk_amd.sharding import Comm  # noqa: E402

TWO_TILES = {"scatter_out", "sweep_batch", "sweep_batch_mfma", "sweep_batch_planar", "sweep_batch_mfma_two_tiles"}


def main():
    rank, world, id_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    assert hasattr(sp.lib(), "sp_emulated_device_marker"), "this helper is for the emulated build only"
    cfg = dict(FAST, nu_1=6 + world.bit_length() - 1, nu_2=7, db_item_size=256)      # 64 rows per shard: one block, ring of 2
    o = oracle_mod.Params(cfg)
    cls = [oracle_mod.Client(o), oracle_mod.Client(o)]
    pps = [cls[0].generate_keys(11), cls[1].generate_keys(12)]
    n = int(os.environ.get("SPIRAL_EMU_LIST", "9"))
    qs = [(k % 2, cls[k % 2].generate_query((311 * k + 9) % o.num_items, 20 + k)) for k in range(n)]
    item, db = o.generate_random_db_and_get_item(9)
    p = sp.Params(cfg)
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    shard = sp.Database.planar_shard(p, rank, world).load(db)
    assert shard.format() == "planar"
    if rank == 0:
        ident = Comm.unique_id()
        with open(id_file + ".tmp", "wb") as f:
            f.write(ident)
        os.rename(id_file + ".tmp", id_file)
    else:
        t0 = time.time()
        while not os.path.exists(id_file):
            assert time.time() - t0 < 120, "rank 0 never published the communicator id"
            time.sleep(0.01)
        ident = open(id_file, "rb").read()
    comm = Comm.rccl(rank, world, ident)
    comm.reserve_batch_for(p, shard, 0)
    pp_list, q_list = [gpps[c] for (c, _) in qs], [q for (_, q) in qs]
    planes = o.instances * o.n * o.n
    got = {}
    for group, size, m in ((0, 16, n), (8, 8, 2)):      # one two-tile pass over the whole list; a one-tile pass over its first two
        sp.paths_taken()
        got[group] = comm.process_queries_batched(p, pp_list[:m], q_list[:m], shard, group=group)
        taken = sp.paths_taken()
        assert "rccl_in_library" in taken and "expand_pruned" in taken and "sweep_batch_scatter" not in taken, taken
        assert TWO_TILES - {"sweep_batch_mfma_two_tiles"} <= taken, taken
        assert ("sweep_batch_mfma_two_tiles" in taken) == (m > 8), (group, taken)
        info = comm.describe()
        assert info["last_list"] == {"group": size, "reduce_scatters": m * planes, "all_gathers": m}, info
    listed = comm.process_queries(p, pp_list[:2], q_list[:2], shard)
    assert comm.process_queries_batched(p, [], [], shard) == []
    comm.barrier()
    comm.free()
    if rank == 0:
        want = [o.process_query(pps[c], q, db) for (c, q) in qs]
        for group in got:
            assert got[group] == want[:len(got[group])], "sp_process_queries_sharded_batched (group %d) on planar shards differs from the oracle" % group
        assert len(got[0]) == n and len(got[8]) == 2
        assert listed == want[:2]
        assert cls[0].decode_response(want[0]) == o.item_to_vec(item)
        print("planar-shards-ok")
    else:
        assert all(v == [] for v in got.values()) and listed == []


if __name__ == "__main__":
    main()
