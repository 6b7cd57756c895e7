"""The per-item digests (sp_db_item_digests) beside the plane digest that reads the same bytes, at nu = (9, 9) with 256-byte items (the
shape of profiles/db_digest.md): 2^18 items, about 14 GiB of PACKED words.  Speed is not a gate; this writes down where it stands:

* per configuration (PACKED, planar-resident, the digit-planar batch copy beside the PACKED words, a sparse bucket 100 % full) and per
  range (all items; 1/8 of the rows, starting at row dim0 / 2): ms per sp_db_item_digests over all planes, host clock around the whole
  call (it ends synchronised), three runs;
* beside each figure, on the same handle in the same process: sp_db_digest of all planes -- THE YARDSTICK: the dense kernels read the
  same bytes with about the same arithmetic per word plus accumulators and atomics -- the stand-alone sweep (planes x the per-plane
  sweep; the one-query group pass on a planar-resident handle; none on a sparse bucket), and read_items of the same range, which is what
  the table replaces.

Every step is a process of its own under its own time limit (`timeout -k 10 <seconds>`), and the steps are chained: the first one
that fails, faults or runs into its limit ends the run and nothing further is started on the device.  Host thread pools: at most 16.

Usage: python scripts/item_digests_ab.py [--out FILE.md] [--rounds R] [--nu1 9 --nu2 9]
Writes the table to --out (default profiles/item_digests.md) and keeps the file's "## Reading" section as it stands."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_k] = str(min(16, int(os.environ.get(_k, "16") or 16)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CONFIGS = ("packed", "planar", "batch_copy", "sparse")
STEP_LIMIT = 420      # seconds per step, as scripts/db_digest_ab.py
SEED = 0x5EED


def step(args):
    """one configuration in this process: prints one JSON line"""
    import numpy as np
    import oracle
    import sdk_amd as sp
    from db_digest_ab import cfg_of, make
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    cfg = cfg_of(args.nu1, args.nu2)
    p = sp.Params(cfg)
    planes = p.instances * p.n * p.n
    n_items = p.num_items()
    blob = np.random.default_rng(9).integers(0, 256, n_items * 256, dtype=np.uint8)
    db = make(sp, p, args.config, blob)
    which = "batch_copy" if args.config == "batch_copy" else "resident"
    resident = db.batch_copy_bytes() if args.config == "batch_copy" else db.device_bytes()

    def clock(fn):
        out = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t0)
        return out

    whole, pres = db.item_digests(SEED, which=which)           # warm: code objects, the read buffer
    assert pres.all() and whole.all()
    with np.errstate(over="ignore"):
        sums = whole.sum(axis=0, dtype=np.uint64)
        planes_sum = db.digest(SEED, which=which).sum(axis=0, dtype=np.uint64)
    assert (sums == planes_sum).all(), "the table does not add up to the plane digests"
    ranges = {"all": (0, n_items), "eighth": ((p.dim0 // 2) * p.num_per, (p.dim0 // 8) * p.num_per)}
    res = {"config": args.config, "resident_bytes": resident, "planes": planes, "ranges": {}}
    res["digest"] = clock(lambda: db.digest(SEED, which=which))
    for name, (item0, count) in ranges.items():
        got = db.item_digests(SEED, item0, count, which=which)[0]
        assert (got == whole[item0:item0 + count]).all()
        r = {"items": count, "item_digests": clock(lambda: db.item_digests(SEED, item0, count, which=which))}
        t0 = time.perf_counter()
        data, present, undecodable = db.read_items(item0, count)
        r["read_items"] = time.perf_counter() - t0
        assert data == blob[item0 * 256:(item0 + count) * 256].tobytes() and present.all() and undecodable == 0
        res["ranges"][name] = r
    sweep, how = [], ""
    if args.config != "sparse":
        oracle.build()
        o = oracle.Params(cfg)
        cl = oracle.Client(o)
        gpp = sp.PublicParameters.deserialize(p, cl.generate_keys(71))
        run = sp.QueryRun(p, gpp, cl.generate_query(5, 500), db)
        if args.config == "planar":
            how = "one-query group pass over all planes"
            sweep = [sp.bench_sweep_batch([run], db, 3) * 1e-3 for _ in range(args.rounds)]
        else:
            how = "planes x stand-alone per-plane PACKED sweep"
            sweep = [planes * run.bench_sweep(db, 3, per_plane=1) * 1e-3 for _ in range(args.rounds)]
        run.free()
    res.update(sweep=sweep, sweep_how=how)
    print(json.dumps(res))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_digests.md"))
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
    lines = ["nu = (%d, %d), 256-byte items; one box; host clock around the whole call (each ends synchronised), median (min .. max) "
             "over %d runs; every configuration a process of its own, every figure of a row on the same handle in the same process"
             % (args.nu1, args.nu2, args.rounds), "",
             "| configuration | range | items | sp_db_item_digests, ms | sp_db_digest of all planes (the yardstick), ms | item digests / "
             "digest x share of the rows | stand-alone sweep of all planes, ms | read_items of the range, ms |",
             "|---|---|---|---|---|---|---|---|"]
    for config in CONFIGS:
        r = res[config]
        for name, rr in r["ranges"].items():
            share = rr["items"] / float(r["ranges"]["all"]["items"])
            lines.append("| %s | %s | %d | %s | %s | %.2f | %s | %.1f |" % (
                config, name, rr["items"], ms(rr["item_digests"]), ms(r["digest"]),
                statistics.median(rr["item_digests"]) / (statistics.median(r["digest"]) * share),
                (ms(r["sweep"]) + " (" + r["sweep_how"] + ")") if r["sweep"] else "n/a", rr["read_items"] * 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    head, reading = "# Per-item digests: `sp_db_item_digests` beside `sp_db_digest` of the same handle\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
