"""Lists of queries on a sparse bucket: the group flow (one pass over the bucket per group of up to 8, k_sweep_sparse_batch) against the
per-query flow (one k_sweep_sparse per query, `batch_in_flight` queries in flight), alternated in ONE process on ONE bucket handle
by the switch sparse_batch_min (0 = the per-query flow, 2 = every group of >= 2 shares a pass).

nu = (9, 7) buckets of 256-byte items (2^16 items, 4 planes) at 16 % and at 100 % occupancy; lists of 2, 3, 4, 5, 8 and 64 through
sp_process_query_batch (host clock around the call, which ends synchronised); the pass alone through sp_bench_sweep_batch and the
single-query kernel through QueryRun.timings()[1] (device events).  Bytes of a pass = items x planes x (16 + 32 B) KiB.

Usage: python scripts/sparse_batch_ab.py [--out FILE.md] [--rounds R].  Writes the tables to --out (default
profiles/sparse_batch_pass.md) between the file's heading and its "## Reading" section, which is kept as it stands: the numbers
are the script's, what they mean is written by whoever ran it."""
import argparse
import ctypes as C
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

CFG = dict(FAST, nu_1=9, nu_2=7, db_item_size=256)
LISTS = (2, 3, 4, 5, 8, 64)
PEAK = 8e12   # bytes/s


def set_min(v):
    sp.lib().sp_debug_set(b"sparse_batch_min", C.c_long(v))


def time_list(p, gpp, qs, gdb, queries_per_timing=64):
    reps = max(1, queries_per_timing // len(qs))
    t0 = time.perf_counter()
    for _ in range(reps):
        sp.process_query_batch(p, gpp, qs, gdb)
    return len(qs) * reps / (time.perf_counter() - t0)      # queries/s (process_query_batch returns synchronised)


def spread(xs):
    return "%.0f (%.0f .. %.0f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_batch_pass.md"))
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    p = sp.Params(CFG)
    gpp = sp.PublicParameters.deserialize(p, bench.synthetic_wire_bytes(p.setup_bytes(), 1))
    qs = [bench.synthetic_wire_bytes(p.query_bytes(), 100 + k) for k in range(64)]
    planes = 4
    order = np.random.default_rng(3).permutation(1 << 16)
    gdb = sp.Database.sparse(p)
    filled = 0
    lines = ["| occupancy | list | per-query flow, queries/s | group flow, queries/s | group / per-query (medians) | group wins by more than the spread |",
             "|---|---|---|---|---|---|"]
    klines = ["| occupancy | kernel | ms per pass | ms per query | bytes of the pass | share of 8 TB/s |", "|---|---|---|---|---|---|"]
    wins = {n: True for n in LISTS}
    try:
        for pct, target in ((16, 10485), (100, 1 << 16)):
            gdb.update_items([(int(idx), b"\x01\x02\x03") for idx in order[filled:target]])   # one call (sp_db_update_items)
            filled = target
            for m in (0, 2):                                  # warm both flows: workspaces, code objects
                set_min(m)
                sp.process_query_batch(p, gpp, qs[:11], gdb)
            qps = {(m, n): [] for m in (0, 2) for n in LISTS}
            for _ in range(args.rounds):
                for m in (0, 2):
                    set_min(m)
                    for n in LISTS:
                        qps[(m, n)].append(time_list(p, gpp, qs[:n], gdb))
            for n in LISTS:
                a, b = qps[(0, n)], qps[(2, n)]
                win = min(b) > max(a)
                wins[n] = wins[n] and win
                lines.append("| %d %% | %d | %s | %s | %.2f | %s |" % (pct, n, spread(a), spread(b), statistics.median(b) / statistics.median(a),
                                                                  "yes" if win else "no"))
            # the kernels alone
            single = []
            for _ in range(4):
                run = sp.QueryRun(p, gpp, qs[0], db=gdb).sweep(gdb)
                run.finish()
                single.append(run.timings()[1])
                run.free()
            by = filled * planes * 48 * 1024
            klines.append("| %d %% | k_sweep_sparse | %.3f | %.3f | %.2f GB | %.0f %% |" % (pct, min(single), min(single), by / 1e9,
                                                                                     100 * by / (min(single) * 1e-3) / PEAK))
            for B in (2, 3, 4, 5, 8):
                runs = [sp.QueryRun(p, gpp, q, db=gdb) for q in qs[:B]]
                try:
                    ms = min(sp.bench_sweep_batch(runs, gdb, 5) for _ in range(3))
                finally:
                    for r in runs:
                        r.free()
                by = filled * planes * (16 + 32 * B) * 1024
                klines.append("| %d %% | k_sweep_sparse_batch, %d queries | %.3f | %.3f | %.2f GB | %.0f %% |" % (pct, B, ms, ms / B, by / 1e9,
                                                                                                        100 * by / (ms * 1e-3) / PEAK))
    finally:
        set_min(int(os.environ.get("SPIRAL_SPARSE_BATCH_MIN", -1)))   # negative: the shipped default
    best = next((n for n in LISTS[:-1] if all(wins[k] for k in LISTS if k >= n)), 0)   # (a list of 64 is eight groups of 8: it has to win too)
    text = "\n".join(["queries/s: median (min .. max) over %d alternations of sparse_batch_min = 0 / 2, 64 queries per timing" % args.rounds, ""] +
                     lines + ["", "the kernels alone (device events; best of 4 / of 3 x 5 passes)", ""] + klines +
                     ["", "smallest measured group size from which the group flow wins on both buckets by more than the spread: %d (0 = none)" % best, ""])
    print(text)
    head, reading = "# One pass over a sparse bucket for a group of queries (`k_sweep_sparse_batch`)\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
        if "\nqueries/s: median" in old:
            head = old[:old.index("\nqueries/s: median") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
