"""The database digest (sp_db_digest) beside the sweep that streams the same words, at nu = (9, 9) with 256-byte items: 2^18 items, about
14 GiB of PACKED words.  Speed is not a gate for the digest; this writes down where it stands:

* per configuration (PACKED, planar-resident, a sparse bucket 100 % full, the digit-planar batch copy beside the PACKED words): ms per
  sp_db_digest of all planes, host clock around the whole call, and TB/s of the resident bytes it reads;
* the yardstick, on the same handle and in the same process: planes x the stand-alone per-plane sweep (sp_bench_sweep_ex with one
  launch per plane; the sweep kernel is unchanged by this feature and streams the same words), three measurements, so its own
  run-to-run spread stands beside the ratio.  A planar-resident handle has no per-plane sweep: its yardstick is the one-query group
  pass over all planes (sp_bench_sweep_batch).  A sparse bucket has neither: no yardstick;
* for context, one full sp_db_read_items of the bucket.

Every step is a process of its own under its own time limit (`timeout -k 10 <seconds>`), and the steps are chained: the first one
that fails, faults or runs into its limit ends the run and nothing further is started on the device.  Host thread pools: at most 16.

Usage: python scripts/db_digest_ab.py [--out FILE.md] [--rounds R] [--nu1 9 --nu2 9]
Writes the table to --out (default profiles/db_digest.md) and keeps the file's "## Reading" section as it stands."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import time

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_k] = str(min(16, int(os.environ.get(_k, "16") or 16)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = ("packed", "planar", "sparse", "batch_copy")
STEP_LIMIT = 420      # seconds per step: keys, a load of 14 GiB, a handful of passes over it and one read-back take well under a minute
SEED = 0x5EED


def cfg_of(nu1, nu2):
    from conftest import FAST
    return dict(FAST, nu_1=nu1, nu_2=nu2, db_item_size=256)


def make(sp, p, config, blob):
    n = p.num_items()
    db = {"packed": sp.Database, "batch_copy": sp.Database, "planar": sp.Database.planar, "sparse": sp.Database.sparse}[config](p)
    if config == "sparse":
        rows = blob.reshape(n, 256)
        db.update_rows(b"".join(struct.pack(">II", 260, i) + rows[i].tobytes() for i in range(n)))
    else:
        db.load_items(blob)
    if config == "batch_copy":
        assert db.prepare_batch() is True, "no room for the digit-planar copy on this device"
    return db


def step(args):
    """one configuration in this process: prints one JSON line"""
    import numpy as np
    import oracle
    import sdk_amd as sp
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    cfg = cfg_of(args.nu1, args.nu2)
    p = sp.Params(cfg)
    planes = p.instances * p.n * p.n
    blob = np.random.default_rng(9).integers(0, 256, p.num_items() * 256, dtype=np.uint8)
    db = make(sp, p, args.config, blob)
    which = "batch_copy" if args.config == "batch_copy" else "resident"
    resident = db.batch_copy_bytes() if args.config == "batch_copy" else db.device_bytes()
    first = db.digest(SEED, which=which).copy()                       # warm: code objects, the read buffer
    digest = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        got = db.digest(SEED, which=which)
        digest.append(time.perf_counter() - t0)
        assert (got == first).all() and got.all()
    if args.config == "batch_copy":
        assert (db.digest(SEED) == first).all(), "the copy and the PACKED words digest differently"
    sweep, how = [], ""
    if args.config != "sparse":
        oracle.build()
        o = oracle.Params(cfg)
        cl = oracle.Client(o)
        gpp = sp.PublicParameters.deserialize(p, cl.generate_keys(71))
        run = sp.QueryRun(p, gpp, cl.generate_query(5, 500), db)
        if args.config == "planar":
            how = "one-query group pass over all planes (sp_bench_sweep_batch)"
            sweep = [sp.bench_sweep_batch([run], db, 3) * 1e-3 for _ in range(args.rounds)]
        else:
            how = "planes x stand-alone per-plane sweep (sp_bench_sweep_ex, one launch per plane)"
            sweep = [planes * run.bench_sweep(db, 3, per_plane=1) * 1e-3 for _ in range(args.rounds)]
        run.free()
    t0 = time.perf_counter()
    got, present, undecodable = db.read_items(0, p.num_items())
    read = time.perf_counter() - t0
    assert got == blob.tobytes() and present.all() and undecodable == 0
    print(json.dumps({"config": args.config, "digest": digest, "sweep": sweep, "sweep_how": how, "read_items": read,
                      "resident_bytes": resident, "planes": planes}))


def run_steps(args):
    me = os.path.abspath(__file__)
    results = {}
    for config in CONFIGS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, me, "--step", "--config", config, "--rounds", str(args.rounds),
               "--nu1", str(args.nu1), "--nu2", str(args.nu2)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:      # chained: nothing further is started after a step that failed or ran into its limit
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("step %s ended with status %d: stopping here" % (config, r.returncode))
        results[config] = json.loads(r.stdout.strip().splitlines()[-1])
        sys.stderr.write("%s done\n" % config)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_digest.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nu1", type=int, default=9)
    ap.add_argument("--nu2", type=int, default=9)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--config", choices=CONFIGS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    res = run_steps(args)
    ms = lambda xs: "%.2f (%.2f .. %.2f)" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)   # noqa: E731
    lines = ["nu = (%d, %d), 256-byte items; one box; host clock around the whole sp_db_digest call (it ends synchronised), median "
             "(min .. max) over %d runs; every configuration a process of its own, its yardstick on the same handle in the same process"
             % (args.nu1, args.nu2, args.rounds), "",
             "| configuration | resident bytes read | sp_db_digest of all planes, ms | TB/s of resident bytes | yardstick, ms | what the yardstick is | digest / yardstick (medians) | yardstick spread (max / min) | full read_items, ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    for config in CONFIGS:
        r = res[config]
        d, s = r["digest"], r["sweep"]
        lines.append("| %s | %d | %s | %.2f | %s | %s | %s | %s | %.1f |" % (
            config, r["resident_bytes"], ms(d), r["resident_bytes"] / statistics.median(d) / 1e12, ms(s) if s else "n/a",
            r["sweep_how"] or "a sparse bucket has no stand-alone sweep benchmark", "%.2f" % (statistics.median(d) / statistics.median(s)) if s else "n/a",
            "%.3f" % (max(s) / min(s)) if s else "n/a", r["read_items"] * 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    head, reading = "# Database digest: `sp_db_digest` beside the sweep that streams the same words\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
