"""The batched pass over a C2 row shard, timed alone with HIP events (profiles/sharded_batch_pass.md): in ONE process, on ONE
shard handle, with the variants alternated --
  scatter-regs  : k_sweep_mfma_scatter, dword stores from the registers          (switch batch_scatter_store = 1)
  scatter-lds   : k_sweep_mfma_scatter, epilogue staged through LDS              (batch_scatter_store = 2)
  plain         : k_sweep_mfma_batch over the same rows, plain [z][ii] output    (the scatter form's lower bound)
  ring x B      : the per-query ring sweep of the shard (sp_bench_sweep_ex, one launch per plane) times the group size:
                  what a list costs without the shared pass
Usage: python scripts/sharded_batch/pass_ab.py [G ...] (default 8 2); one JSON line per (G, variant, round)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import C2  # noqa: E402

B, ITERS, ROUNDS = 8, 5, 3
HBM_TBPS = 8.0


def main():
    Gs = [int(a) for a in sys.argv[1:] if a.isdigit()] or [8, 2]
    o = oracle.Params(C2)
    cl = oracle.Client(o)
    pp = cl.generate_keys(7)
    qs = [cl.generate_query((7919 * k + 1) % o.num_items, 100 + k) for k in range(B)]
    p = sp.Params(C2)
    gpp = sp.PublicParameters.deserialize(p, pp)
    planes = o.instances * o.n * o.n
    for G in Gs:
        shard = sp.Database(p, 0, G).fill_synthetic(0x123456789)
        runs = [sp.QueryRun(p, gpp, q, db=shard) for q in qs]
        read = shard.device_bytes()
        written = B * planes * 4 * 2048 * o.num_per * 4
        variants = [("scatter-regs", 1, 1), ("scatter-lds", 2, 1), ("plain", 2, 0)]
        for rnd in range(ROUNDS):
            for name, store, layout in variants:
                sp.lib().sp_debug_set(b"batch_scatter_store", C.c_long(store))
                ms = sp.bench_sweep_scatter_group(runs, shard, G, ITERS, layout=layout)
                moved = read + written
                print(json.dumps({"G": G, "round": rnd, "variant": name, "ms_per_pass": round(ms, 4), "bytes_read": read,
                                  "bytes_written": written, "fraction_of_8TBps": round(moved / (ms * 1e-3) / (HBM_TBPS * 1e12), 4)}),
                      flush=True)
            ms = runs[0].bench_sweep(shard, ITERS, per_plane=1) * planes
            moved = B * (read + written // B)
            print(json.dumps({"G": G, "round": rnd, "variant": "ring x %d" % B, "ms_per_pass": round(ms * B, 4), "ms_per_query_sweep": round(ms, 4),
                              "bytes_read": B * read, "bytes_written": written,
                              "fraction_of_8TBps": round(moved / (ms * B * 1e-3) / (HBM_TBPS * 1e12), 4)}), flush=True)
        for r in runs:
            r.free()
        del shard, runs


if __name__ == "__main__":
    main()
