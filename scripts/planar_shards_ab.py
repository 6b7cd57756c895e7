"""Planar row shards (sp_db_create_planar_shard) against PACKED row shards at C2, shard 0 of G = 2, 4, 8, synthetic fill, ONE process,
the variants alternated inside every round (three rounds), everything timed against the PACKED-shard flow of the same build:

the pass alone (sp_bench_sweep_scatter_group / sp_bench_sweep_batch: HIP events on the pass's stream, query tables included)
  planar-scatter 8 / 16 : k_sweep_planar_scatter over the planar shard, one query tile / two
  packed-scatter 8      : k_sweep_mfma_scatter over a PACKED shard of the same rows
  planar-plain 8 / 16   : k_sweep_planar, plain layout, over an UNSHARDED planar database of the shard's row count (nu_1 = 6 .. 8): the
                          same loads and stores in runs of the same length, other addresses -- the scatter form's expected cost

the list (sp_process_queries_sharded_batched on a NULL transport: one rank alone, NOT a multi-GPU run -- the collectives return at
once and move nothing, so this is one rank's critical path without the exchange; host clock around calls that end synchronised)
  lists of 16 and 32 on the planar shard with group 16 and group 8, on the PACKED shard with group 8

Synthetic wire bytes (bench.synthetic_wire_bytes): the answer path's arithmetic is data-independent.
Usage: python scripts/planar_shards_ab.py [--out FILE.md] [--rounds R] [--gs 2,4,8]
Writes the tables to --out (default profiles/planar_shards.md) with the box fingerprint of scripts/box_fingerprint.sh; a "## Reading"
section of an earlier file is kept as it stands."""
import argparse
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
from conftest import C2  # noqa: E402
from sdk_amd.sharding import NullTransport  # noqa: E402

SEED, ITERS = 7, 5
HEAD = "# Planar row shards against PACKED row shards: the pass and the list (`scripts/planar_shards_ab.py`)\n\n"


def spread(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def wire(p, n):
    gpp = sp.PublicParameters.deserialize(p, bench.synthetic_wire_bytes(p.setup_bytes(), 1))
    return gpp, [bench.synthetic_wire_bytes(p.query_bytes(), 100 + k) for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planar_shards.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gs", default="2,4,8")
    args = ap.parse_args()
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    p = sp.Params(C2)
    gpp, qs = wire(p, 32)
    out = ["config C2 (512 x 2048, 4 planes), shard 0 of G, synthetic fill seed %d; median (min .. max) over %d rounds, the variants "
           "alternated inside every round" % (SEED, args.rounds), ""]
    pass_rows, list_rows, ratios = [], [], []
    for G in [int(g) for g in args.gs.split(",")]:
        nj = (1 << C2["nu_1"]) // G
        planar, packed = sp.Database.planar_shard(p, 0, G).fill_synthetic(SEED), sp.Database(p, 0, G).fill_synthetic(SEED)
        p_plain = sp.Params(dict(C2, nu_1=nj.bit_length() - 1))
        gpp_plain, qs_plain = wire(p_plain, 16)
        plain = sp.Database.planar(p_plain).fill_synthetic(SEED)
        runs = {"planar": [sp.QueryRun(p, gpp, q, db=planar) for q in qs[:16]], "packed": [sp.QueryRun(p, gpp, q, db=packed) for q in qs[:8]],
                "plain": [sp.QueryRun(p_plain, gpp_plain, q) for q in qs_plain]}
        variants = {"planar-scatter 8": lambda: sp.bench_sweep_scatter_group(runs["planar"][:8], planar, G, ITERS, layout=1),
                    "planar-scatter 16": lambda: sp.bench_sweep_scatter_group(runs["planar"], planar, G, ITERS, layout=1),
                    "packed-scatter 8": lambda: sp.bench_sweep_scatter_group(runs["packed"], packed, G, ITERS, layout=1),
                    "planar-plain 8": lambda: sp.bench_sweep_batch(runs["plain"][:8], plain, ITERS),
                    "planar-plain 16": lambda: sp.bench_sweep_batch(runs["plain"], plain, ITERS)}
        ms = {k: [] for k in variants}
        for k, f in variants.items():      # one untimed pass each: code objects loaded, LDS limits raised
            f()
        for _ in range(args.rounds):
            for k, f in variants.items():
                ms[k].append(f())
        for k in variants:
            n = int(k.split()[-1])
            pass_rows.append("| %d | %d | %s | %s | %.3f |" % (G, nj, k, spread(ms[k]), statistics.median(ms[k]) / n))
        for n in (8, 16):
            a, b = ms["planar-scatter %d" % n], ms["planar-plain %d" % n]
            ratios.append("| %d | %d | %.3f | %.3f .. %.3f | %.3f .. %.3f |" % (G, n, statistics.median(a) / statistics.median(b),
                                                                               min(a) / statistics.median(a), max(a) / statistics.median(a),
                                                                               min(b) / statistics.median(b), max(b) / statistics.median(b)))
        for v in runs.values():
            for r in v:
                r.free()
        del plain, runs, variants
        # ---- the list, one rank alone
        comm = NullTransport(0, G).comm
        comm.reserve_batch_for(p, planar, 16)
        flows = {"planar, group 16": (planar, 16), "planar, group 8": (planar, 8), "PACKED, group 8": (packed, 8)}
        t = {(k, n): [] for k in flows for n in (16, 32)}
        for k, (db, group) in flows.items():
            comm.process_queries_batched(p, gpp, qs[:16], db, group=group)      # untimed: workspaces, exchange buffers
        for _ in range(args.rounds):
            for k, (db, group) in flows.items():
                for n in (16, 32):
                    t0 = time.perf_counter()
                    comm.process_queries_batched(p, gpp, qs[:n], db, group=group)
                    t[(k, n)].append((time.perf_counter() - t0) * 1e3 / n)
        for k in flows:
            list_rows.append("| %d | %s | %s | %s |" % (G, k, spread(t[(k, 16)]), spread(t[(k, 32)])))
        comm.free()
        del planar, packed
    out += ["## The pass alone (HIP events; %d passes per timing, query tables included)" % ITERS, "",
            "| G | rows of the shard | variant | ms per pass | ms per query |", "|---|---|---|---|---|"] + pass_rows
    out += ["", "scatter form against plain form (median / median), beside each variant's own spread (min / median .. max / median)", "",
            "| G | queries | scatter / plain | spread of the scatter form | spread of the plain form |", "|---|---|---|---|---|"] + ratios
    out += ["", "## The list: one rank alone, NOT a multi-GPU run (null transport; ms per query, host clock)", "",
            "| G | flow | list of 16 | list of 32 |", "|---|---|---|---|"] + list_rows
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
