"""A planar-resident database (sp_db_create_planar) against the two forms a PACKED database offers to lists of queries, at C2, in ONE
process, all three filled by sp_db_fill_synthetic with one seed:

  (a) PACKED, switch batch_planar = 0 at list time: the PACKED two-tile fallback k_sweep_mfma_batch<8, 1, 0, 2> for 9 .. 16 queries
      (what a database too large for a second copy gets);
  (b) PACKED with sp_db_prepare_batch: the digit-planar COPY beside the PACKED words (56 + 64 GiB at C2);
  (c) planar-resident: the digit-planar words alone (64 GiB).

(a) and (b) are one handle: (a) is measured first, then the copy is built and (b) is measured; (c) is created while that handle
lives, so at most (b) + (c) are resident.  Before anything is timed, every response of (c) -- single queries and lists of 8 and 16 --
is compared byte for byte with (a)'s.

Measured: queries/s for single queries and for lists of 8 and 16 through sp_process_query / sp_process_query_batch (host clock
around calls that end synchronised), the handles alternated inside every round; the pass alone through sp_bench_sweep_batch (device
events) with its share of 8 TB/s over the bytes it has to read (the database once + per member its query slice and its output);
resident bytes.  Synthetic wire bytes (bench.synthetic_wire_bytes): the answer path's arithmetic is data-independent.

Usage: python scripts/planar_resident_ab.py [--out FILE.md] [--rounds R] [--config C2|C1]
Writes the tables to --out (default profiles/planar_resident.md) with the box fingerprint of scripts/box_fingerprint.sh; a
"## Reading" section of an earlier file is kept as it stands: the numbers are the script's, what they mean is written by whoever
ran it."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
import sdk_amd as sp  # noqa: E402
from conftest import C1, C2  # noqa: E402

PEAK = 8e12   # bytes/s
N = 2048
SEED = 7
HEAD = "# A planar-resident database against PACKED with and without the digit-planar copy (`scripts/planar_resident_ab.py`)\n\n"


def set_planar(v):
    sp.lib().sp_debug_set(b"batch_planar", C.c_long(v))


def answer(p, gpp, qs, db):
    return [sp.process_query(p, gpp, qs[0], db)] if len(qs) == 1 else sp.process_query_batch(p, gpp, qs, db)


def time_list(p, gpp, qs, db, queries_per_timing=32):
    reps = max(1, queries_per_timing // len(qs))
    t0 = time.perf_counter()
    for _ in range(reps):
        answer(p, gpp, qs, db)
    return len(qs) * reps / (time.perf_counter() - t0)


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def pass_ms(p, gpp, qs, db):
    runs = [sp.QueryRun(p, gpp, q) for q in qs]
    try:
        return min(sp.bench_sweep_batch(runs, db, 5) for _ in range(3))
    finally:
        for r in runs:
            r.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planar_resident.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="C2", choices=("C2", "C1"))
    args = ap.parse_args()
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    cfg = {"C2": C2, "C1": C1}[args.config]
    planes, num_per, dim0 = cfg["instances"] * cfg["n"] ** 2, 1 << cfg["nu_2"], 1 << cfg["nu_1"]
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, bench.synthetic_wire_bytes(p.setup_bytes(), 1))
    qs = [bench.synthetic_wire_bytes(p.query_bytes(), 100 + k) for k in range(16)]
    lists = (1, 8, 16)
    forms = ("a", "b", "c")
    label = {"a": "(a) PACKED, batch_planar = 0", "b": "(b) PACKED + planar copy", "c": "(c) planar-resident"}
    packed = sp.Database(p).fill_synthetic(SEED)
    # ---- (a): responses for the byte check, then the pass alone
    set_planar(0)
    try:
        want = {n: answer(p, gpp, qs[:n], packed) for n in lists}
        ms = {("a", n): pass_ms(p, gpp, qs[:n], packed) for n in (8, 16)}
        resident = {"a": packed.device_bytes() + packed.batch_copy_bytes()}
    finally:
        set_planar(1)
    assert packed.prepare_batch() is True, "no room for the digit-planar copy: (b) cannot be measured on this device"
    resident["b"] = packed.device_bytes() + packed.batch_copy_bytes()
    planar = sp.Database.planar(p).fill_synthetic(SEED)
    resident["c"] = planar.device_bytes() + planar.batch_copy_bytes()
    for n in lists:   # before timing: (c) == (a), and (b) == (a), byte for byte, every query
        assert answer(p, gpp, qs[:n], planar) == want[n], "planar-resident responses differ from PACKED (list of %d)" % n
        assert answer(p, gpp, qs[:n], packed) == want[n], "planar-copy responses differ from PACKED (list of %d)" % n
    for n in (8, 16):
        ms[("b", n)] = pass_ms(p, gpp, qs[:n], packed)
        ms[("c", n)] = pass_ms(p, gpp, qs[:n], planar)
    ms[("c", 1)] = pass_ms(p, gpp, qs[:1], planar)
    # ---- queries/s, the three forms alternated inside every round
    qps = {(f, n): [] for f in forms for n in lists}
    try:
        for _ in range(args.rounds):
            for f in forms:
                set_planar(0 if f == "a" else 1)
                if f == "b":
                    assert packed.prepare_batch() is True      # (a)'s switch released the copy: built again, outside the timing
                db = planar if f == "c" else packed
                for n in lists:
                    qps[(f, n)].append(time_list(p, gpp, qs[:n], db))
    finally:
        set_planar(1)
    words = planes * N * num_per * dim0
    per_member = planes * N * dim0 * 16 + planes * 4 * N * num_per * 4
    out = ["config %s (%d x %d, %d planes), synthetic database seed %d; responses of (b) and (c) byte-equal to (a)'s for the single query and "
           "the lists of 8 and 16" % (args.config, dim0, num_per, planes, SEED), "",
           "queries/s: median (min .. max) over %d rounds, the three forms alternated inside every round, 32 queries per timing" % args.rounds, "",
           "| form | resident GiB | single queries | lists of 8 | lists of 16 |", "|---|---|---|---|---|"]
    out += ["| %s | %.1f | %s | %s | %s |" % (label[f], resident[f] / 2**30, spread(qps[(f, 1)]), spread(qps[(f, 8)]), spread(qps[(f, 16)]))
            for f in forms]
    out += ["", "the pass alone (sp_bench_sweep_batch, device events; best of 3 x 5 passes, query tables included)", "",
            "| form | queries | ms per pass | ms per query | bytes of the pass | share of 8 TB/s |", "|---|---|---|---|---|---|"]
    for (f, n), t in sorted(ms.items()):
        word_bytes = 8 if f == "c" or (f == "b" and n > 8) else 7
        by = words * word_bytes + n * per_member
        out.append("| %s | %d | %.3f | %.3f | %.2f GB | %.2f |" % (label[f], n, t, t / n, by / 1e9, by / (t * 1e-3) / PEAK))
    fp = subprocess.run(["bash", os.path.join(ROOT, "scripts", "box_fingerprint.sh")], capture_output=True, text=True).stdout
    out += ["", "box fingerprint (`scripts/box_fingerprint.sh`):", "", "```", fp.rstrip(), "```", ""]
    text = "\n".join(out)
    print(text)
    reading = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(HEAD + text + reading)


if __name__ == "__main__":
    main()
