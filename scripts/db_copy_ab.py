"""Item copy between resident databases (sp_db_copy_items) beside the path it replaces, at nu = (9, 9) with 256-byte items: 2^18
items, about 14 GiB of PACKED words.  Speed is not a gate for the copy; this reports where it stands.  Per pair of forms

    sparse (100 % full) -> PACKED,  PACKED -> planar-resident,  planar-resident -> PACKED,  PACKED -> sparse,  sparse -> sparse

and in ONE process per pair: ms per dst.copy_from(src) of the whole range (host clock around the whole call, which ends
synchronised), ms per dst.update_rows(src.export_rows()) of the same pair -- the host path through item bytes -- and ms per
sp_db_digest of src, the yardstick for one pass over the source.  Three runs each, median (min .. max).  After the timed copies the
destination's digest must equal the source's.

Every pair is a process of its own under its own time limit (`timeout -k 10 <seconds>`), and the pairs are chained: the first one
that fails, faults or runs into its limit ends the run and nothing further is started on the device.

Usage: python scripts/db_copy_ab.py [--out FILE.md] [--rounds R] [--nu1 9 --nu2 9]
Writes the table to --out (default profiles/db_copy.md) and keeps the file's "## Reading" section as it stands."""
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

PAIRS = (("sparse", "packed"), ("packed", "planar"), ("planar", "packed"), ("packed", "sparse"), ("sparse", "sparse"))
STEP_LIMIT = 420      # seconds per pair: two loads, three copies, three export / update-row round trips of 14 GiB
SEED = 0xC0B1


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


def step(args):
    """one pair in this process: prints one JSON line"""
    import sdk_amd as sp
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    src_fmt, dst_fmt = args.pair.split(":")
    small = sp.Params(cfg_of(6, 7))      # warm: code objects, tables
    empty(sp, small, dst_fmt).copy_from(loaded(sp, small, src_fmt, file_of(1 << 13)))
    p = sp.Params(cfg_of(args.nu1, args.nu2))
    src = loaded(sp, p, src_fmt, file_of(p.num_items()))
    assert src.format() == src_fmt
    want = src.digest(SEED).copy()
    out = {"pair": args.pair, "items": p.num_items(), "src_bytes": src.device_bytes(), "copy": [], "export_update": [], "digest": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        src.digest(SEED)
        out["digest"].append(time.perf_counter() - t0)
    dst = empty(sp, p, dst_fmt)
    dst.copy_from(src, 0, 64)            # warm: the read buffer
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        copied = dst.copy_from(src)
        out["copy"].append(time.perf_counter() - t0)
        assert copied == p.num_items()
    assert (dst.digest(SEED) == want).all(), "the copy differs from its source"
    out["dst_bytes"] = dst.device_bytes()
    del dst
    dst = empty(sp, p, dst_fmt)
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        dst.update_rows(src.export_rows())
        out["export_update"].append(time.perf_counter() - t0)
    assert (dst.digest(SEED) == want).all(), "the re-import differs from its source"
    print(json.dumps(out))


def run_steps(args):
    me = os.path.abspath(__file__)
    results = []
    for a, b in PAIRS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, me, "--pair", a + ":" + b, "--rounds", str(args.rounds),
               "--nu1", str(args.nu1), "--nu2", str(args.nu2)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:      # chained: nothing further is started after a step that failed or ran into its limit
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("pair %s -> %s ended with status %d: stopping here" % (a, b, r.returncode))
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_copy.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nu1", type=int, default=9)
    ap.add_argument("--nu2", type=int, default=9)
    ap.add_argument("--pair", default="")
    args = ap.parse_args()
    if args.pair:
        return step(args)
    res = run_steps(args)
    ms = lambda xs: "%.1f (%.1f .. %.1f)" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)   # noqa: E731
    lines = ["nu = (%d, %d), 256-byte items; host clock around the whole call (each ends synchronised), median (min .. max) over %d "
             "runs; every pair a process of its own, the three measurements of a pair in that one process" % (args.nu1, args.nu2, args.rounds),
             "",
             "| source -> destination | source bytes | destination bytes | copy_from, ms | update_rows(export_rows()), ms | digest of the source, ms | copy / digest | export + update / copy |",
             "|---|---|---|---|---|---|---|---|"]
    for r in res:
        c, e, d = (statistics.median(r[k]) for k in ("copy", "export_update", "digest"))
        lines.append("| %s | %d | %d | %s | %s | %s | %.1f | %.1f |" % (r["pair"].replace(":", " -> "), r["src_bytes"], r["dst_bytes"], ms(r["copy"]),
                                                                     ms(r["export_update"]), ms(r["digest"]), c / d, e / c))
    text = "\n".join(lines) + "\n"
    print(text)
    head, reading = "# Item copy: `sp_db_copy_items` beside `update_rows(export_rows())` and one digest pass\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
