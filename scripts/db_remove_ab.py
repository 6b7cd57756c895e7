"""Item removal (sp_db_remove_items / sp_db_remove_range) beside the only routes the library offered before it, at nu = (9, 9) with
256-byte items: 2^18 items, about 14 GiB of PACKED words.  Speed is not a gate for the removal; this reports where it stands.
Per format -- PACKED, planar-resident, sparse (100 % full) -- and in ONE process per format, three removals:

    1 % of the items (scattered),  50 % of the items (scattered),  an eighth of the rows (whole rows, remove_range)

ms per removal (host clock around the whole call, which ends synchronised) beside
  * dense forms: update_items of the same list with zero-length data -- the upload window, the encode launch and a forward NTT of zeros;
  * sparse: a fresh bucket filled by copy_from of the surviving runs of the full one (what an operator had to do, short of replace_db);
  * sp_db_digest of the same handle, the yardstick for one pass.
Three runs each, median (min .. max).  A dense removal is repeatable as it stands (the same bytes are cleared again); a sparse bucket is
refilled between runs by copy_from of a second full bucket, outside the timed region.  After the timed runs the handle's per-item
digests must be those of the empty item exactly on the removed indices (dense), or present must be 0 exactly there (sparse).

Every format is a process of its own under its own time limit (`timeout -k 10 <seconds>`), and the formats are chained: the first one
that fails, faults or runs into its limit ends the run and nothing further is started on the device.

Usage: python scripts/db_remove_ab.py [--out FILE.md] [--rounds R] [--nu1 9 --nu2 9]
Writes the table to --out (default profiles/db_remove.md) and keeps the file's "## Reading" section as it stands."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMATS = ("packed", "planar", "sparse")
STEP_LIMIT = 420      # seconds per format
SEED = 0xDE1


def cfg_of(nu1, nu2):
    from conftest import FAST
    return dict(FAST, nu_1=nu1, nu_2=nu2, db_item_size=256)


def file_of(n_items):
    import numpy as np
    return np.random.default_rng(9).integers(0, 256, n_items * 256, dtype=np.uint8)


def empty(sp, p, fmt):
    return {"packed": sp.Database, "planar": sp.Database.planar, "sparse": sp.Database.sparse}[fmt](p)


def loaded(sp, p, fmt, blob):
    """a handle of the format holding the file (a sparse bucket: every item, through one /update-row body)"""
    n = p.num_items()
    db = empty(sp, p, fmt)
    if fmt == "sparse":
        rows = blob.reshape(n, 256)
        db.update_rows(b"".join(struct.pack(">II", 260, i) + rows[i].tobytes() for i in range(n)))
    else:
        db.load_items(blob)
    return db


def lists_of(p):
    """(name, indices or None, range or None) of the three removals"""
    import numpy as np
    n, npr = p.num_items(), p.num_per
    rng = np.random.default_rng(31)
    rows = (p.dim0 // 8) * npr
    return [("1 %", np.sort(rng.choice(n, n // 100, replace=False)), None),
            ("50 %", np.sort(rng.choice(n, n // 2, replace=False)), None),
            ("an eighth of the rows", np.arange(3 * npr, 3 * npr + rows), (3 * npr, rows))]


def runs_of(keep):
    """the runs of consecutive True in a bool array -> [(first, count)]"""
    import numpy as np
    edges = np.flatnonzero(np.diff(np.concatenate(([0], keep.astype(np.int8), [0]))))
    return [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]


def step(args):
    """one format in this process: prints one JSON line"""
    import numpy as np
    import sdk_amd as sp
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    fmt = args.format
    small = sp.Params(cfg_of(6, 7))      # warm: code objects, tables
    warm = loaded(sp, small, fmt, file_of(1 << 13))
    warm.remove_items([1, 2, 130])
    warm.update_items([(5, b"")])
    p = sp.Params(cfg_of(args.nu1, args.nu2))
    n = p.num_items()
    db = loaded(sp, p, fmt, file_of(n))
    assert db.format() == fmt
    full = loaded(sp, p, fmt, file_of(n)) if fmt == "sparse" else None
    out = {"format": fmt, "items": n, "bytes": db.device_bytes(), "digest": [], "cases": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        db.digest(SEED)
        out["digest"].append(time.perf_counter() - t0)
    db.remove_items([0])                 # warm: the upload buffer
    zero = empty(sp, p, "packed").item_digests(SEED, 0, 1)[0][0] if fmt != "sparse" else None
    for name, idx, rng in lists_of(p):
        case = {"name": name, "items": int(idx.size), "remove": [], "before": []}
        for _ in range(args.rounds):
            if fmt == "sparse":
                full_n = db.copy_from(full)          # refill: outside the timed region
                assert full_n == n and db.sparse_items() == n
            t0 = time.perf_counter()
            removed = db.remove_range(*rng) if rng else db.remove_items(idx)
            case["remove"].append(time.perf_counter() - t0)
            assert removed == idx.size
        table, present = db.item_digests(SEED)
        if fmt == "sparse":
            gone = np.ones(n, dtype=bool)
            gone[np.flatnonzero(present)] = False
            assert np.array_equal(np.flatnonzero(gone), idx), "present does not match the removed list"
            keep = ~gone
            for _ in range(args.rounds):             # the route before: a fresh bucket from the surviving runs
                t0 = time.perf_counter()
                fresh = empty(sp, p, "sparse")
                for a, cnt in runs_of(keep):
                    fresh.copy_from(full, a, cnt)
                case["before"].append(time.perf_counter() - t0)
                assert fresh.sparse_items() == int(keep.sum())
                del fresh
        else:
            assert (table[idx] == zero).all(), "a removed item is not the empty item"
            pairs = [(int(i), b"") for i in idx]
            for _ in range(args.rounds):             # the route before: an upsert of zero bytes
                t0 = time.perf_counter()
                db.update_items(pairs)
                case["before"].append(time.perf_counter() - t0)
            assert (db.item_digests(SEED)[0] == table).all(), "the zero-length upsert and the removal differ"
        out["cases"].append(case)
    print(json.dumps(out))


def run_steps(args):
    me = os.path.abspath(__file__)
    results = []
    for fmt in FORMATS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, me, "--format", fmt, "--rounds", str(args.rounds),
               "--nu1", str(args.nu1), "--nu2", str(args.nu2)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:      # chained: nothing further is started after a step that failed or ran into its limit
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("format %s ended with status %d: stopping here" % (fmt, r.returncode))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_remove.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nu1", type=int, default=9)
    ap.add_argument("--nu2", type=int, default=9)
    ap.add_argument("--format", default="")
    args = ap.parse_args()
    if args.format:
        return step(args)
    res = run_steps(args)
    ms = lambda xs: "%.1f (%.1f .. %.1f)" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)   # noqa: E731
    lines = ["nu = (%d, %d), 256-byte items; host clock around the whole call (each ends synchronised), median (min .. max) over %d "
             "runs; every format a process of its own.  \"the route before\": update_items with zero-length data on the dense forms, a "
             "fresh bucket filled by copy_from of the surviving runs on the sparse one" % (args.nu1, args.nu2, args.rounds),
             "",
             "| format | resident bytes | removed | items | removal, ms | the route before, ms | digest of the handle, ms | before / removal | removal / digest |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        d = statistics.median(r["digest"])
        for c in r["cases"]:
            rm, before = statistics.median(c["remove"]), statistics.median(c["before"])
            lines.append("| %s | %d | %s | %d | %s | %s | %s | %.1f | %.2f |" % (r["format"], r["bytes"], c["name"], c["items"], ms(c["remove"]),
                                                                               ms(c["before"]), ms(r["digest"]), before / rm, rm / d))
    text = "\n".join(lines) + "\n"
    print(text)
    head, reading = "# Item removal: `sp_db_remove_items` beside the routes before it and one digest pass\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
