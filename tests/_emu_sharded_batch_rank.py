"""One rank of tests/test_emulated_sharded_batch.py::test_batched_list_over_process_ranks (TEST INFRASTRUCTURE).

Run as N processes with SPIRAL_HIP_LIB = the emulated build: each loads its row shard, joins the library's own communicator (the
shared-memory stand-in for RCCL, tests/emu/emu_rccl.cpp) and answers the same list through sp_process_queries_sharded_batched
(group = 0, 4 and 1) and through the existing list call; rank 0 compares with the oracle and prints 'sharded-batch-ok'.
usage: _emu_sharded_batch_rank.py RANK WORLD ID_FILE"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle as oracle_mod  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import FAST  # noqa: E402
from sdk_amd.sharding import Comm  # noqa: E402


def main():
    rank, world, id_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    assert hasattr(sp.lib(), "sp_emulated_device_marker"), "this helper is for the emulated build only"
    cfg = dict(FAST, nu_1=5 + world.bit_length() - 1, nu_2=7, db_item_size=256)      # 32 rows per shard: one ring of the pass
    o = oracle_mod.Params(cfg)
    cls = [oracle_mod.Client(o), oracle_mod.Client(o)]
    pps = [cls[0].generate_keys(11), cls[1].generate_keys(12)]
    n = int(os.environ.get("SPIRAL_EMU_LIST", "6"))
    qs = [(k % 2, cls[k % 2].generate_query((311 * k + 9) % o.num_items, 20 + k)) for k in range(n)]
    item, db = o.generate_random_db_and_get_item(9)
    p = sp.Params(cfg)
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    shard = sp.Database(p, rank, world).load(db)
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
    comm.reserve_batch(p, 0)
    pp_list, q_list = [gpps[c] for (c, _) in qs], [q for (_, q) in qs]
    planes = o.instances * o.n * o.n
    got = {}
    for group, size in ((0, 8), (4, 4), (1, 1)):
        sp.paths_taken()
        got[group] = comm.process_queries_batched(p, pp_list, q_list, shard, group=group)
        taken = sp.paths_taken()
        assert "rccl_in_library" in taken and "expand_pruned" in taken, taken
        assert ("sweep_batch_scatter" in taken) == (group != 1), (group, taken)
        info = comm.describe()
        assert info["last_list"] == {"group": size, "reduce_scatters": n * planes, "all_gathers": n}, info
    listed = comm.process_queries(p, pp_list, q_list, shard)
    assert comm.process_queries_batched(p, [], [], shard) == []
    comm.barrier()
    comm.free()
    if rank == 0:
        want = [o.process_query(pps[c], q, db) for (c, q) in qs]
        for group in got:
            assert got[group] == want, "sp_process_queries_sharded_batched (group %d) differs from the oracle" % group
        assert listed == want
        assert cls[0].decode_response(want[0]) == o.item_to_vec(item)
        print("sharded-batch-ok")
    else:
        assert all(v == [] for v in got.values()) and listed == []


if __name__ == "__main__":
    main()
