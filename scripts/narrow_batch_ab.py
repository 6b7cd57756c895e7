"""Lists of queries on a narrow database (8-byte words, num_per <= 64): the group flow (one pass over the database per group of up
to 8, k_sweep_narrow_batch, shared expansion launches) against the per-query flow (one k_sweep_narrow2 per query, `batch_in_flight`
queries in flight), alternated in ONE process on ONE database handle per configuration by the switch narrow_batch_min (0 = the
per-query flow, 2 = every group of >= 2 shares a pass).

C1, P2 (CFG_20_256) and SERVER_DEFAULT of tests/conftest.py, synthetic database and wire bytes; lists of 2, 3, 4, 5, 8 and 64 through
sp_process_query_batch (host clock around the call, which ends synchronised); the pass alone through sp_bench_sweep_batch and the
single-query kernel through QueryRun.bench_sweep (device events).  Nominal bytes of a pass = the database once + per member its
query slice (planes x N x dim0 x 16 B) and its output (planes x 4 x N x num_per x 4 B).

Usage: python scripts/narrow_batch_ab.py [--out FILE.md] [--rounds R]
       python scripts/narrow_batch_ab.py --baseline LABEL      (the same lists at C1 and P2 in a process of their own with the loaded
                                                               library and no switch touched -- run it with SPIRAL_HIP_LIB = the parent
                                                               commit's build, or with SPIRAL_NARROW_BATCH_MIN set)
Writes the tables to --out (default profiles/narrow_batch_pass.md) between the file's heading and its "## Own process: LABEL" /
"## Reading" sections, which are kept as they stand (--baseline replaces the section of the same label): the numbers are the
script's, what they mean is written by whoever ran it."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import C1, P2, SERVER_DEFAULT  # noqa: E402

CONFIGS = (("C1", C1), ("P2", P2), ("SERVER_DEFAULT", SERVER_DEFAULT))
LISTS = (2, 3, 4, 5, 8, 64)
PEAK = 8e12   # bytes/s
N = 2048
HEAD = "# One pass over a narrow database for a group of queries (`k_sweep_narrow_batch`)\n\n"


def set_min(v):
    sp.lib().sp_debug_set(b"narrow_batch_min", C.c_long(v))


def time_list(p, gpp, qs, gdb, queries_per_timing=64):
    reps = max(1, queries_per_timing // len(qs))
    t0 = time.perf_counter()
    for _ in range(reps):
        sp.process_query_batch(p, gpp, qs, gdb)
    return len(qs) * reps / (time.perf_counter() - t0)      # queries/s (process_query_batch returns synchronised)


def spread(xs):
    return "%.0f (%.0f .. %.0f)" % (statistics.median(xs), min(xs), max(xs))


def setup(cfg):
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, bench.synthetic_wire_bytes(p.setup_bytes(), 1))
    qs = [bench.synthetic_wire_bytes(p.query_bytes(), 100 + k) for k in range(64)]
    return p, gpp, qs, sp.Database(p).fill_synthetic(7)


def split(old):
    """(heading, the "## Own process: ..." sections, "## Reading" section, tables) of an earlier file"""
    head, parent, reading = HEAD, "", ""
    if "\n## Reading" in old:
        reading = old[old.index("\n## Reading"):]
        old = old[:old.index("\n## Reading")]
    if "\n## Own process" in old:
        parent = old[old.index("\n## Own process"):]
        old = old[:old.index("\n## Own process")]
    if "\nqueries/s: median" in old:
        head = old[:old.index("\nqueries/s: median") + 1]
    return head, parent, reading, old[len(head):] if old.startswith(head) else ""


def baseline(args, others):
    """the section of this label; the sections of other labels are kept"""
    title = "## Own process: %s" % args.baseline
    kept = "".join("\n## " + sec for sec in others.split("\n## ")[1:] if not sec.startswith(title[3:] + "\n"))
    lines = ["", title, "", "no switch touched, queries/s: median (min .. max) over %d timings of 64 queries" % args.rounds, "",
             "| config | list | queries/s |", "|---|---|---|"]
    for name, cfg in CONFIGS[:2]:
        p, gpp, qs, gdb = setup(cfg)
        sp.process_query_batch(p, gpp, qs[:11], gdb)
        qps = {n: [] for n in LISTS}
        for _ in range(args.rounds):
            for n in LISTS:
                qps[n].append(time_list(p, gpp, qs[:n], gdb))
        lines += ["| %s | %d | %s |" % (name, n, spread(qps[n])) for n in LISTS]
    return kept + "\n".join(lines) + "\n"


def measure(args):
    lines = ["| config | list | per-query flow, queries/s | group flow, queries/s | group / per-query (medians) | group wins by more than the spread |",
             "|---|---|---|---|---|---|"]
    klines = ["| config | kernel | ms per pass | ms per query | bytes of the pass | share of 8 TB/s |", "|---|---|---|---|---|---|"]
    wins = {n: True for n in LISTS}
    try:
        for name, cfg in CONFIGS:
            p, gpp, qs, gdb = setup(cfg)
            planes, num_per, dim0 = cfg["instances"] * cfg["n"] ** 2, 1 << cfg["nu_2"], 1 << cfg["nu_1"]
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
                lines.append("| %s | %d | %s | %s | %.2f | %s |" % (name, n, spread(a), spread(b), statistics.median(b) / statistics.median(a),
                                                                  "yes" if win else "no"))
            # the kernels alone
            db_bytes = planes * N * num_per * dim0 * 8
            per_member = planes * N * dim0 * 16 + planes * 4 * N * num_per * 4
            run = sp.QueryRun(p, gpp, qs[0], db=gdb)
            try:
                single = min(run.bench_sweep(gdb, 5) for _ in range(3))
            finally:
                run.free()
            by = db_bytes + per_member
            klines.append("| %s | k_sweep_narrow2 | %.3f | %.3f | %.2f GB | %.0f %% |" % (name, single, single, by / 1e9, 100 * by / (single * 1e-3) / PEAK))
            for B in (2, 3, 4, 5, 8):
                runs = [sp.QueryRun(p, gpp, q, db=gdb) for q in qs[:B]]
                try:
                    ms = min(sp.bench_sweep_batch(runs, gdb, 5) for _ in range(3))
                finally:
                    for r in runs:
                        r.free()
                by = db_bytes + B * per_member
                klines.append("| %s | k_sweep_narrow_batch, %d queries | %.3f | %.3f | %.2f GB | %.0f %% |" % (name, B, ms, ms / B, by / 1e9,
                                                                                                       100 * by / (ms * 1e-3) / PEAK))
            del gdb
    finally:
        set_min(int(os.environ.get("SPIRAL_NARROW_BATCH_MIN", -1)))   # negative: the shipped default
    best = next((n for n in LISTS[:-1] if all(wins[k] for k in LISTS if k >= n)), 0)   # (a list of 64 is eight groups of 8: it has to win too)
    return "\n".join(["queries/s: median (min .. max) over %d alternations of narrow_batch_min = 0 / 2, 64 queries per timing" % args.rounds, ""] +
                     lines + ["", "the kernels alone (device events; best of 3 x 5 passes)", ""] + klines +
                     ["", "smallest measured list length m such that for every measured length >= m, on all three configurations, the group flow's "
                      "minimum exceeds the per-query flow's maximum: %d (0 = none)" % best, ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrow_batch_pass.md"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--baseline", default="")
    args = ap.parse_args()
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    head, parent, reading, tables = split(open(args.out).read() if os.path.exists(args.out) else "")
    if args.baseline:
        parent = baseline(args, parent)
        print(parent)
    else:
        tables = measure(args)
        print(tables)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + tables + parent + reading)


if __name__ == "__main__":
    main()
