"""The compact client registry (sp_pp_compact / sp_pp_expand_into, sp_server_set_expanded_clients) beside today's registry, in one
process on one box, the arms alternating round by round.  Not a gate; this writes down where it stands:

* resident bytes per client, compact (sp_ppc_device_bytes) and expanded (sp_pp_device_bytes), at CFG_20_256 (P2) and C2 params;
* /setup latency, host clock around the whole sp_server_setup call: k = 0 (sp_pp_deserialize: keystream, raw image and upload from the
  host) against k > 0 (the wire image uploaded, nothing else), C1 params;
* one /private-read of one query, a HIT (the client's slot stands) against a MISS (k = 1, two clients in turn: every read evicts and
  expands), against k = 0, on C1 (the narrow database: the shortest query, where a miss shows most) and on C2 (synthetic words);
* direct-upload requests per second (two elements per request, the set of tests/test_request_layer.py), k = 0 against k = 2.

The measuring runs in ONE child process under its own time limit (`timeout -k 10 <seconds>`); if it fails, faults or runs into the limit
nothing further is started on the device.  Host thread pools: at most 16.

Usage: python scripts/compact_clients_ab.py [--out FILE.md] [--rounds R] [--skip-c2]
Writes the tables to --out (default profiles/compact_clients.md) and keeps the file's "## Reading" section as it stands."""
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

STEP_LIMIT = 540
DIRECT = {"n": 2, "nu_1": 4, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 8, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
          "instances": 1, "db_item_size": 256, "direct_upload": 1}


def clock(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def step(args):
    import oracle
    import sdk_amd as sp
    from conftest import C1, C2, P2
    assert not hasattr(sp.lib(), "sp_emulated_device_marker"), "a measurement needs the gfx950 library"
    oracle.build()
    out = {"bytes": {}, "setup": {}, "read": {}, "direct": {}}

    def session(cfg, clients):
        o = oracle.Params(cfg)
        cls = [oracle.Client(o) for _ in range(clients)]
        pps = [cl.generate_keys(60 + k) for k, cl in enumerate(cls)]
        qs = [cl.generate_query(5 + k, 600 + k) for k, cl in enumerate(cls)]
        return pps, qs

    # resident bytes per client
    for name, cfg in (("P2", P2), ("C2", C2)):
        p = sp.Params(cfg)
        pp = session(cfg, 1)[0][0]
        c = sp.PublicParameters.compact(p, pp)
        out["bytes"][name] = {"setup_bytes": p.setup_bytes(), "compact": c.device_bytes(), "expanded": c.expand().device_bytes()}

    # /setup and /private-read
    for name, cfg in (("C1", C1),) + (() if args.skip_c2 else (("C2", C2),)):
        p = sp.Params(cfg)
        db = sp.Database(p).fill_synthetic(77)
        pps, qs = session(cfg, 2)
        s0, s_hit, s_miss = sp.Server(p, db), sp.Server(p, db), sp.Server(p, db)
        s_hit.set_expanded_clients(2)
        s_miss.set_expanded_clients(1)
        u0 = [s0.setup(pp) for pp in pps]
        uh = [s_hit.setup(pp) for pp in pps]
        um = [s_miss.setup(pp) for pp in pps]
        req = lambda u, k: [u[k].encode() + qs[k]]       # noqa: E731
        for k in (0, 1, 0, 1):                            # warm: workspaces, slots, code objects
            s0.private_read(req(u0, k)), s_hit.private_read(req(uh, k)), s_miss.private_read(req(um, k))
        r = {"k0": [], "hit": [], "miss": []}
        for i in range(args.rounds):
            k = i % 2
            r["k0"].append(clock(lambda: s0.private_read(req(u0, k))))
            r["hit"].append(clock(lambda: s_hit.private_read(req(uh, k))))
            r["miss"].append(clock(lambda: s_miss.private_read(req(um, k))))
        st = s_miss.client_stats()
        assert st["misses"] >= args.rounds and s_hit.client_stats()["misses"] == 2, (st, s_hit.client_stats())
        out["read"][name] = r
        if name == "C1":
            su = {"k0": [], "compact": []}
            for i in range(args.rounds):
                su["k0"].append(clock(lambda: s0.setup(pps[i % 2])))
                su["compact"].append(clock(lambda: s_hit.setup(pps[i % 2])))
            out["setup"][name] = su
        del s0, s_hit, s_miss, db, p

    # direct upload: requests of two elements per second
    p = sp.Params(DIRECT)
    db = sp.Database(p).fill_synthetic(78)
    pps, qs = session(DIRECT, 2)
    body = [pps[0] + qs[0], pps[1] + qs[1]]
    s0, s2 = sp.Server(p, db), sp.Server(p, db)
    s2.set_expanded_clients(2)
    assert s0.private_read(body) == s2.private_read(body)
    d = {"k0": [], "k2": []}
    for i in range(args.rounds):
        d["k0"].append(clock(lambda: s0.private_read(body)))
        d["k2"].append(clock(lambda: s2.private_read(body)))
    out["direct"] = d
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_clients.md"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--skip-c2", action="store_true")
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if args.step:
        return step(args)
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", "--rounds", str(args.rounds)]
    r = subprocess.run(cmd + (["--skip-c2"] if args.skip_c2 else []), capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("the measuring process ended with status %d" % r.returncode)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    ms = lambda xs: "%.3f (%.3f .. %.3f)" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)   # noqa: E731
    lines = ["One box, one process, the arms alternating round by round; host clock around the whole call; median (min .. max) over %d "
             "rounds." % args.rounds, "",
             "| params | setup_bytes | compact handle, bytes | expanded handle, bytes | expanded / compact |", "|---|---|---|---|---|"]
    for name, b in res["bytes"].items():
        lines.append("| %s | %d | %d | %d | %.2f |" % (name, b["setup_bytes"], b["compact"], b["expanded"], b["expanded"] / b["compact"]))
    lines += ["", "| /setup, ms | k = 0 (expanded on the host path) | k > 0 (compact) |", "|---|---|---|"]
    for name, s in res["setup"].items():
        lines.append("| %s | %s | %s |" % (name, ms(s["k0"]), ms(s["compact"])))
    lines += ["", "| /private-read of one query, ms | k = 0 | hit | miss (evict + sp_pp_expand_into) | miss - hit (medians) | spread of a hit (max - min) |",
              "|---|---|---|---|---|---|"]
    for name, s in res["read"].items():
        lines.append("| %s | %s | %s | %s | %.3f | %.3f |" % (
            name, ms(s["k0"]), ms(s["hit"]), ms(s["miss"]), (statistics.median(s["miss"]) - statistics.median(s["hit"])) * 1e3,
            (max(s["hit"]) - min(s["hit"])) * 1e3))
    d = res["direct"]
    lines += ["", "| direct upload, two elements per request | k = 0 | k = 2 |", "|---|---|---|",
              "| ms per request | %s | %s |" % (ms(d["k0"]), ms(d["k2"])),
              "| requests per second (medians) | %.1f | %.1f |" % (1 / statistics.median(d["k0"]), 1 / statistics.median(d["k2"]))]
    text = "\n".join(lines) + "\n"
    print(text)
    head, reading = "# Compact client registry: resident bytes, /setup, hit against miss, direct upload\n\n", ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## Reading" in old:
            reading = old[old.index("\n## Reading"):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + text + reading)


if __name__ == "__main__":
    main()
