"""One rank of tests/test_emulated_param_matrix.py::test_sparse_shards_over_process_ranks (TEST INFRASTRUCTURE).

Cell e's sparse shards of tests/test_gpu_param_matrix.py with the ranks as PROCESSES (the loopback world of the GPU suite hands device
pointers to torch, which the emulated device cannot serve).  Run as N processes with SPIRAL_HIP_LIB = the emulated build: each fills
its row shard of a sparse bucket of one of tests/param_matrix.py's sets at (6, 3) from the same /update-row body, joins the library's
own communicator (the shared-memory stand-in for RCCL, tests/emu/emu_rccl.cpp) and answers one query through
sp_process_query_sharded and a list of 3 through sp_process_queries_sharded_batched; rank 0 compares with oracle.SparseDb over the
whole bucket and prints 'param-matrix-shards-ok'.
usage: _emu_param_matrix_rank.py RANK WORLD ID_FILE SET"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle as oracle_mod  # noqa: E402
import sdk_amd as sp  # noqa: E402
from param_matrix import body, cfg, planes_of, sparse_records  # noqa: E402
from sdk_amd.sharding import Comm  # noqa: E402


def main():
    rank, world, id_file, name = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    assert hasattr(sp.lib(), "sp_emulated_device_marker"), "this helper is for the emulated build only"
    c = cfg(name, 6, 3)
    planes = planes_of(c)
    o, p = oracle_mod.Params(c), sp.Params(c)
    cls = [oracle_mod.Client(o), oracle_mod.Client(o)]
    pps = [cls[0].generate_keys(11), cls[1].generate_keys(12)]
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    recs, _ = sparse_records(o)
    held = {i for i, _ in recs}
    absent = next(i for i in range(o.num_items) if i not in held)
    idxs = [recs[9][0], absent, recs[5][0]]                       # a full record, an absent item, the short record
    qs = [cls[k % 2].generate_query(idx, 1100 + k) for k, idx in enumerate(idxs)]
    shard = sp.Database.sparse(p, rank, world)
    assert shard.update_rows(body(recs)) == (len(recs), 4 + o.db_item_size)      # (the other ranks' records count as applied)
    mine = sum(1 for i in held if (i // o.num_per) // (o.dim0 // world) == rank)
    assert shard.sparse_items() == mine and 0 < mine < len(recs)
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
    sp.paths_taken()
    one = comm.process_query(p, gpps[0], qs[0], shard)
    taken = sp.paths_taken()
    assert {"rccl_in_library", "sweep_sparse", "scatter_out", "expand_pruned"} <= taken and "sparse_group_pass" not in taken, taken
    listed = comm.process_queries_batched(p, [gpps[k % 2] for k in range(3)], qs, shard)
    taken = sp.paths_taken()
    assert {"rccl_in_library", "sweep_sparse", "scatter_out", "sparse_group_pass"} <= taken, taken
    assert not any(t.startswith("sweep_batch") for t in taken), taken
    assert ("pack_v1" in taken) == (name == "V1"), taken
    info = comm.describe()["last_list"]
    assert info["reduce_scatters"] == 3 * planes and info["all_gathers"] == 3, info
    comm.barrier()
    comm.free()
    if rank == 0:
        bucket = oracle_mod.SparseDb(o)
        for i, d in recs:
            bucket.update_item_raw(i, d)
        want = [bucket.process_query(pps[k % 2], q) for k, q in enumerate(qs)]
        assert one == want[0], "sp_process_query_sharded differs from the oracle"
        assert listed == want, "sp_process_queries_sharded_batched differs from the oracle"
        print("param-matrix-shards-ok")
    else:
        assert one == b"" and listed == []


if __name__ == "__main__":
    main()
