"""Bulk upserts against the loop they replace: one /update-row body (sp_db_update_rows: one copy, one encode launch, one patch launch
and one synchronisation per upload window) against a loop of sp_db_update_item (a copy, a launch of `planes` workgroups, a patch
launch and a synchronisation per item), alternated in ONE process on one handle shape.

* sparse bucket, nu = (9, 7), 256-byte items: an empty bucket filled to 16 % (10,485 items) and on to 100 % (65,536), each way;
* dense PACKED database, nu = (6, 7), 256-byte items, with a standing digit-planar copy: 1, 16, 256 and 4096 items upserted each way
  on the same handle (the same items and bytes both ways, so the handle's content does not change between runs).

Host clock around the calls (both end synchronised); the body is built before the clock starts.

Usage: python scripts/bulk_upsert_ab.py [--out FILE.md] [--rounds R].  Writes the tables to --out (default profiles/bulk_upsert.md)
and keeps the file's "## Reading" section as it stands: the numbers are the script's, what they mean is written by whoever ran it."""
import argparse
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import sdk_amd as sp  # noqa: E402
from conftest import FAST  # noqa: E402

SPARSE = dict(FAST, nu_1=9, nu_2=7, db_item_size=256)
DENSE = {"n": 2, "nu_1": 6, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
         "instances": 1, "db_item_size": 256}


def body_of(records):
    return b"".join(struct.pack(">II", 4 + len(d), i) + d for i, d in records)


def clock(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def loop(db, records):
    for i, d in records:
        db.update_item(i, d)


def med(xs):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bulk_upsert.md"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    rng = np.random.default_rng(7)
    lines = ["seconds: median (min .. max) over %d alternations of the two ways in one process" % args.rounds, "",
             "### sparse bucket, nu = (9, 7), 256-byte items, filled from empty", "",
             "| step | items | loop of sp_db_update_item, s | items/s | one body, s | items/s | loop / body (medians) | body faster than every loop run |",
             "|---|---|---|---|---|---|---|---|"]
    p = sp.Params(SPARSE)
    order = [int(i) for i in rng.permutation(1 << 16)]
    data = rng.integers(0, 256, (1 << 16, 256), dtype=np.uint8)
    steps = [("empty -> 16 %", [(i, data[i].tobytes()) for i in order[:10485]]), ("16 % -> 100 %", [(i, data[i].tobytes()) for i in order[10485:]])]
    bodies = [body_of(r) for _, r in steps]
    sp.Database.sparse(p).update_rows(bodies[0][:264 * 8])          # warm: code objects, tables
    t = {(w, k): [] for w in ("loop", "body") for k in range(2)}
    for _ in range(args.rounds):
        for way in ("loop", "body"):
            db = sp.Database.sparse(p)
            for k, (_, recs) in enumerate(steps):
                t[(way, k)].append(clock((lambda: loop(db, recs)) if way == "loop" else (lambda: db.update_rows(bodies[k]))))
            assert db.sparse_items() == 1 << 16
            del db
    for k, (name, recs) in enumerate(steps):
        a, b, n = t[("loop", k)], t[("body", k)], len(recs)
        lines.append("| %s | %d | %s | %.0f | %s | %.0f | %.1f | %s |" % (name, n, med(a), n / statistics.median(a), med(b), n / statistics.median(b),
                                                                      statistics.median(a) / statistics.median(b), "yes" if max(b) < min(a) else "no"))
    lines += ["", "### dense PACKED database, nu = (6, 7), 256-byte items, digit-planar copy standing", "",
              "| items | loop of sp_db_update_item, s | items/s | one body, s | items/s | loop / body (medians) | body faster than every loop run |",
              "|---|---|---|---|---|---|---|"]
    p = sp.Params(DENSE)
    n_items = p.num_items()
    db = sp.Database(p).load_items(rng.integers(0, 256, n_items * 256, dtype=np.uint8))
    assert db.prepare_batch() is True
    copy = db.batch_copy_bytes()
    one = {}
    for n in (1, 16, 256, 4096):
        recs = [(int(i), data[k].tobytes()) for k, i in enumerate(rng.choice(n_items, n, replace=False))]
        body = body_of(recs)
        loop(db, recs[:2]), db.update_rows(body)                    # warm
        reps = args.rounds * (8 if n == 1 else 1)                    # (a single call: more samples for its spread)
        a, b = [], []
        for _ in range(reps):
            a.append(clock(lambda: loop(db, recs)))
            b.append(clock(lambda: db.update_rows(body)))
        if n == 1:
            one = {"loop": a, "body": b}
        lines.append("| %d | %s | %.0f | %s | %.0f | %.2f | %s |" % (n, med(a), n / statistics.median(a), med(b), n / statistics.median(b),
                                                                 statistics.median(a) / statistics.median(b), "yes" if max(b) < min(a) else "no"))
    assert db.batch_copy_bytes() == copy
    a, b = one["loop"], one["body"]
    lines += ["", "one record: the body's median is %+.1f us against one sp_db_update_item call's; that call's own run-to-run spread (max - min over "
              "%d runs in this process) is %.1f us" % ((statistics.median(b) - statistics.median(a)) * 1e6, len(a), (max(a) - min(a)) * 1e6), ""]
    text = "\n".join(lines)
    print(text)
    head, reading = "# Bulk upserts: one `/update-row` body against a loop of `sp_db_update_item`\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
