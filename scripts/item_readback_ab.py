"""Item read-back (sp_db_read_items) against the loaders it inverts, at nu = (9, 9) with 256-byte items: 2^18 items, about 14 GiB of
PACKED words.  Speed is not a gate for the read-back -- there is no earlier path to compare with -- so this reports where it stands:

* per format (PACKED, planar-resident, a sparse bucket 100 % full): ms per full read-back (every item, one call, the shipped
  db_load_window) and GB/s of RESIDENT bytes consumed (sp_db_device_bytes / time);
* beside it the opposite direction as the yardstick: sp_db_load_items of the same file (a sparse bucket: one /update-row body of
  every item), from the library given with --parent-lib -- a build of the commit before the read-back -- or, without it, from this
  build, whose loaders are that commit's.

Every step is a process of its own under its own time limit (`timeout -k 10 <seconds>`), and the steps are chained: the first one
that fails, faults or runs into its limit ends the run and nothing further is started on the device.

Usage: python scripts/item_readback_ab.py [--out FILE.md] [--rounds R] [--parent-lib libspiral_hip.so] [--nu1 9 --nu2 9]
Writes the table to --out (default profiles/item_readback.md) and keeps the file's "## Reading" section as it stands."""
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
STEP_LIMIT = {"load": 300, "read": 300}      # seconds per step: a load or three read-backs of 14 GiB take a few seconds each


def cfg_of(nu1, nu2):
    from conftest import FAST
    return dict(FAST, nu_1=nu1, nu_2=nu2, db_item_size=256)


def file_of(n_items):
    import numpy as np
    return np.random.default_rng(9).integers(0, 256, n_items * 256, dtype=np.uint8)


def make(sp, p, fmt, blob):
    """a handle of the format holding the file -> (handle, seconds the load took)"""
    n = p.num_items()
    db = {"packed": sp.Database, "planar": sp.Database.planar, "sparse": sp.Database.sparse}[fmt](p)
    if fmt == "sparse":
        rows = blob.reshape(n, 256)
        body = b"".join(struct.pack(">II", 260, i) + rows[i].tobytes() for i in range(n))
        t0 = time.perf_counter()
        db.update_rows(body)
    else:
        t0 = time.perf_counter()
        db.load_items(blob)
    return db, time.perf_counter() - t0


def step(args):
    """one step in this process: prints one JSON line"""
    import sdk_amd as sp
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    p = sp.Params(cfg_of(args.nu1, args.nu2))
    blob = file_of(p.num_items())
    make(sp, sp.Params(cfg_of(6, 7)), args.format, file_of(1 << 13))      # warm: code objects, tables
    times = []
    if args.step == "load":
        for _ in range(args.rounds):
            db, t = make(sp, p, args.format, blob)
            times.append(t)
            resident = db.device_bytes()
            del db
    else:
        db, _ = make(sp, p, args.format, blob)
        assert db.format() == args.format
        resident = db.device_bytes()
        db.read_items(0, 64)                                                # warm: the read buffer
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            got, present, undecodable = db.read_items(0, p.num_items())
            times.append(time.perf_counter() - t0)
            assert got == blob.tobytes() and present.all() and undecodable == 0
    print(json.dumps({"step": args.step, "format": args.format, "seconds": times, "resident_bytes": resident, "items": p.num_items()}))


def run_steps(args):
    me = os.path.abspath(__file__)
    results = {}
    for fmt in FORMATS:
        for what in ("load", "read"):
            env = dict(os.environ)
            if what == "load" and args.parent_lib:
                env["SPIRAL_HIP_LIB"] = os.path.abspath(args.parent_lib)
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT[what]), sys.executable, me, "--step", what, "--format", fmt,
                   "--rounds", str(args.rounds), "--nu1", str(args.nu1), "--nu2", str(args.nu2)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:      # chained: nothing further is started after a step that failed or ran into its limit
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("step %s / %s ended with status %d: stopping here" % (what, fmt, r.returncode))
            results[(fmt, what)] = json.loads(r.stdout.strip().splitlines()[-1])
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_readback.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--nu1", type=int, default=9)
    ap.add_argument("--nu2", type=int, default=9)
    ap.add_argument("--step", choices=("load", "read"))
    ap.add_argument("--format", choices=FORMATS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    res = run_steps(args)
    yard = "the library given with --parent-lib" if args.parent_lib else "this build (its loaders are the previous commit's)"
    lines = ["nu = (%d, %d), 256-byte items; host clock around the calls (both end synchronised), median (min .. max) over %d runs; every "
             "step a process of its own; the loaders' figures are from %s" % (args.nu1, args.nu2, args.rounds, yard), "",
             "| format | resident bytes | full read-back, ms | GB/s of resident bytes | opposite direction (sp_db_load_items; sparse: one /update-row body), ms | GB/s of resident bytes | read-back / load (medians) |",
             "|---|---|---|---|---|---|---|"]
    for fmt in FORMATS:
        rd, ld = res[(fmt, "read")], res[(fmt, "load")]
        a, b = rd["seconds"], ld["seconds"]
        ms = lambda xs: "%.1f (%.1f .. %.1f)" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)   # noqa: E731
        lines.append("| %s | %d | %s | %.1f | %s | %.1f | %.2f |" % (fmt, rd["resident_bytes"], ms(a), rd["resident_bytes"] / statistics.median(a) / 1e9,
                                                                 ms(b), ld["resident_bytes"] / statistics.median(b) / 1e9,
                                                                 statistics.median(a) / statistics.median(b)))
    text = "\n".join(lines) + "\n"
    print(text)
    head, reading = "# Item read-back: `sp_db_read_items` beside the loaders it inverts\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
