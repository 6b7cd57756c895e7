"""Row shards of a sparse bucket (sp_db_create_sparse_shard): what the scatter-form sweeps cost against the plain-layout kernels over
the same items, and what ONE rank of G = 2, 4, 8 spends per query -- alone on one GPU with a NULL transport (collectives that return
at once), not a multi-GPU run -- beside the unsharded bucket's existing flows.

nu = (9, 7) buckets of 256-byte items (2^16 items, 4 planes) at 16 % and at 100 % occupancy, the shape of profiles/sparse_batch_pass.md.
Kernel level, per G on rank 0's handle (one allocation, one process): sp_bench_sweep_scatter_group with layout 0 (k_sweep_sparse for one
query, k_sweep_sparse_batch for 2 .. 8: the plain layout) and layout 1 (k_sweep_sparse_scatter / k_sweep_sparse_scatter_batch: the
per-plane exchange layout), alternated; device events.  Flow level: sp_process_query_sharded one query at a time and
sp_process_queries_sharded_batched(group = 0) on a list of 8 (host clock around the call, which ends synchronised), beside
sp_process_query and sp_process_query_batch of 8 on the unsharded bucket; each rank once with sharding.NullTransport and once with
LocalCopyTransport below.

Usage: python scripts/sparse_shards_ab.py [--out FILE.md] [--rounds R].  Writes the tables to --out (default profiles/sparse_shards.md)
between the file's heading and its "## Reading" section, which is kept as it stands."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import FAST  # noqa: E402
from sdk_amd.sharding import NullTransport  # noqa: E402

CFG = dict(FAST, nu_1=9, nu_2=7, db_item_size=256)
SHARDS = (2, 4, 8)
GROUPS = (1, 2, 4, 8)


def rng_of(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def ms_per_query(call, n, reps):
    call()      # warm: workspaces, exchange buffers, code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


class LocalCopyTransport:
    """Collectives of ONE rank alone that move its own data: the reduce-scatter copies the rank's own chunk of the send buffer into the
    receive buffer, the all-gather its own ciphertexts into its slot (device copies on the exchange stream, issued from Python).  The
    null transport leaves the receive buffer as allocated -- zeros, on which every fold step takes its all-zero shortcut; here the
    local fold works on the rank's own partial sums, as it would on reduced ones.  The other ranks' slots of the gather stay unwritten."""

    def __init__(self, rank, world):
        import torch
        from sdk_amd.sharding import Comm, _DevArray, _DevArray64

        def rs(send, recv, count, stream):
            with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                torch.as_tensor(_DevArray(recv, count), device="cuda").copy_(torch.as_tensor(_DevArray(send + 4 * count * rank, count), device="cuda"))
            return 0

        def ag(send, recv, count, stream):
            with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                torch.as_tensor(_DevArray64(recv + 8 * count * rank, count), device="cuda").copy_(torch.as_tensor(_DevArray64(send, count), device="cuda"))
            return 0
        self.comm = Comm.custom(rank, world, rs, ag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_shards.md"))
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    p = sp.Params(CFG)
    gpp = sp.PublicParameters.deserialize(p, bench.synthetic_wire_bytes(p.setup_bytes(), 1))
    qs = [bench.synthetic_wire_bytes(p.query_bytes(), 100 + k) for k in range(8)]
    order = np.random.default_rng(3).permutation(1 << 16)
    whole = sp.Database.sparse(p)
    rank0 = {G: sp.Database.sparse(p, 0, G) for G in SHARDS}
    comms = {(G, kind): T(0, G).comm for G in SHARDS for kind, T in (("null transport", NullTransport), ("local-copy transport", LocalCopyTransport))}
    for c in comms.values():
        c.reserve_batch(p, 0)
    klines = ["| occupancy | G | items on rank 0 | queries | plain layout, ms per pass | scatter layout, ms per pass | scatter / plain (medians) | gap larger than the plain kernel's spread |",
              "|---|---|---|---|---|---|---|---|"]
    flines = ["| occupancy | handle | one at a time, ms per query | list of 8, ms per query | group pass taken |", "|---|---|---|---|---|"]
    filled = 0
    for pct, target in ((16, 10485), (100, 1 << 16)):
        pairs = [(int(idx), b"\x01\x02\x03") for idx in order[filled:target]]
        for db in [whole] + [rank0[G] for G in SHARDS]:      # every handle is handed every write; a shard keeps its rows' items
            db.update_items(pairs)
        filled = target
        for G in SHARDS:
            db = rank0[G]
            for B in GROUPS:
                runs = [sp.QueryRun(p, gpp, q, db=db) for q in qs[:B]]
                try:
                    plain, scatter = [], []
                    sp.bench_sweep_scatter_group(runs, db, G, 2, layout=0)
                    sp.bench_sweep_scatter_group(runs, db, G, 2, layout=1)
                    for _ in range(args.rounds):
                        plain.append(sp.bench_sweep_scatter_group(runs, db, G, 5, layout=0))
                        scatter.append(sp.bench_sweep_scatter_group(runs, db, G, 5, layout=1))
                finally:
                    for r in runs:
                        r.free()
                gap = abs(statistics.median(scatter) - statistics.median(plain))
                klines.append("| %d %% | %d | %d | %d | %s | %s | %.2f | %s |" % (pct, G, db.sparse_items(), B, rng_of(plain), rng_of(scatter),
                                                                           statistics.median(scatter) / statistics.median(plain),
                                                                           "yes" if gap > max(plain) - min(plain) else "no"))
        one = ms_per_query(lambda: [sp.process_query(p, gpp, q, whole) for q in qs], 8, args.rounds)
        sp.paths_taken()
        lst = ms_per_query(lambda: sp.process_query_batch(p, gpp, qs, whole), 8, args.rounds)
        flines.append("| %d %% | unsharded bucket (sp_process_query, sp_process_query_batch) | %s | %s | %s |" %
                      (pct, rng_of(one), rng_of(lst), "yes" if "sparse_group_pass" in sp.paths_taken() else "no"))
        for G, kind in comms:
            c, db = comms[G, kind], rank0[G]
            one = ms_per_query(lambda: [c.process_query(p, gpp, q, db) for q in qs], 8, args.rounds)
            sp.paths_taken()
            lst = ms_per_query(lambda: c.process_queries_batched(p, gpp, qs, db, group=0), 8, args.rounds)
            taken = sp.paths_taken()
            assert {"sweep_sparse", "scatter_out"} <= taken, taken
            flines.append("| %d %% | rank 0 of %d alone, %s (sp_process_query_sharded, sp_process_queries_sharded_batched) | %s | %s | %s |" %
                          (pct, G, kind, rng_of(one), rng_of(lst), "yes" if "sparse_group_pass" in taken else "no"))
    text = "\n".join(["the kernels alone on rank 0's handle: median (min .. max) ms per pass over %d alternations of the two layouts, 5 passes per timing, device events" % args.rounds,
                      ""] + klines +
                     ["", "one rank ALONE on one GPU, not a multi-GPU run -- with a null transport (collectives return at once, the reduced chunk stays as "
                      "allocated, results meaningless) and with a local-copy transport (the rank's own chunk stands in for the reduced one) -- beside the "
                      "unsharded bucket's flows: median (min .. max) ms per query over %d timings of 8 queries, host clock" % args.rounds, ""] + flines + [""])
    print(text)
    head, reading = "# Row shards of a sparse bucket: the scatter-form sweeps and one rank's flows (`sp_db_create_sparse_shard`)\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
        if "\nthe kernels alone on rank 0" in old:
            head = old[:old.index("\nthe kernels alone on rank 0") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
