"""One rank's work for a LIST of queries on a C2 row shard, alone on one GPU with a null transport (the collectives return at
once and move no data): what one rank computes, NOT a multi-GPU measurement.  ms per query of
  batched   : Comm.process_queries_batched (group = 8: one pass over the shard per 8 queries)
  pipelined : Comm.process_queries (one sweep of the shard per query, query k + 1 expanding under query k's sweeps)
alternated in one process on one shard handle.  With SPIRAL_HIP_LIB pointing at a build of the parent commit only `pipelined`
runs (that library has no batched call): the baseline that is not the code under test.
Usage: python scripts/sharded_batch/list_ab.py [G ...] (default 8 4 2); one JSON line per (G, list length, variant, round)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import C2  # noqa: E402
from sdk_amd.sharding import NullTransport  # noqa: E402

ROUNDS = 3


def main():
    import torch
    Gs = [int(a) for a in sys.argv[1:] if a.isdigit()] or [8, 4, 2]
    have_batched = hasattr(sp.lib(), "sp_process_queries_sharded_batched")
    o = oracle.Params(C2)
    cl = oracle.Client(o)
    pp = cl.generate_keys(7)
    qs = [cl.generate_query((7919 * k + 1) % o.num_items, 100 + k) for k in range(32)]
    p = sp.Params(C2)
    gpp = sp.PublicParameters.deserialize(p, pp)
    for G in Gs:
        shard = sp.Database(p, 0, G).fill_synthetic(0x123456789)
        comm = NullTransport(0, G).comm
        if have_batched:
            comm.reserve_batch(p, 8)
        else:
            comm.reserve(p)
        variants = [("pipelined", lambda lst: comm.process_queries(p, gpp, lst, shard))]
        if have_batched:
            variants.insert(0, ("batched", lambda lst: comm.process_queries_batched(p, gpp, lst, shard, group=8)))
        for _, f in variants:
            f(qs[:8])   # warm: workspaces, buffers
        for n in (8, 32):
            for rnd in range(ROUNDS):
                for name, f in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f(qs[:n])
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3 / n
                    print(json.dumps({"G": G, "list": n, "round": rnd, "variant": name, "ms_per_query": round(ms, 4),
                                      "library": "parent" if not have_batched else "this",
                                      "note": "one rank alone, null transport: not a multi-GPU measurement"}), flush=True)
        comm.free()
        del shard


if __name__ == "__main__":
    main()
