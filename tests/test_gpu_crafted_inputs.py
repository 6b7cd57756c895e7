"""Client-facing entry points on words no honest client sends.

The wire formats are bare u64 arrays that the reference never validates (client.rs:68-80, 303-329): a client may send any
64-bit word, and the server has to answer with exactly the bytes spiral-rs would.  Every case here takes honest bytes from
oracle.Client, overwrites wire words by a named family (`_FAMILIES`), and compares the library with the CPU oracle ON THE SAME
CRAFTED BYTES.  Nothing is decrypted: crafted inputs decode to garbage; the claim is "byte-identical to the reference for every
input of the right length".

Operand contract of the stage exports (include/spiral_hip.h): operands in NTT form are canonical (< q) -- the reference's own
pointwise code wraps a u64 beyond that (poly.rs:310-345 multiply_add_poly sums products of unreduced words in u64), so such
input has no defined answer and is out of contract; raw, wire and database words are unrestricted wherever the reference is
exact for them (to_ntt's Barrett step, arith.rs:122-134; the u128 sums of multiply_reg_by_database, server.rs:186-217).  No
family is left out of a byte comparison.

Sections: 1 crafted wire words (public parameters, queries, lists, direct upload); 2 the matrix-core pass with BOTH operands
at their digit extremes; 3 stage exports at the corners of their accumulators.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FAST, FAST56

pytestmark = pytest.mark.gpu

N = 2048
Q0, Q1 = 268369921, 249561089
Q = Q0 * Q1
U64 = (1 << 64) - 1
KQ = (U64 // Q) * Q          # the largest multiple of Q below 2^64
assert KQ + 1 <= U64

# the two configurations of tests/test_gpu_parity.py's _FUZZ list that the issue names: [11] 28-bit digits everywhere (digits can
# exceed q), [1] odd t_gsw
FUZZ11 = dict(n=2, nu_1=5, nu_2=4, p=256, q2_bits=20, t_gsw=4, t_conv=2, t_exp_left=2, t_exp_right=2, instances=1, db_item_size=8192)
FUZZ1 = dict(n=2, nu_1=6, nu_2=5, p=256, q2_bits=22, t_gsw=5, t_conv=3, t_exp_left=5, t_exp_right=28, instances=1, db_item_size=5000)
NO_EXPANSION = {"direct_upload": 1, "n": 5, "nu_1": 6, "nu_2": 3, "p": 65536, "q2_bits": 27, "t_gsw": 3, "t_conv": 56,
                "t_exp_left": 56, "t_exp_right": 56}   # get_no_expansion_testing_params, util.rs:139-153
DIRECT_WIDE = {"n": 2, "nu_1": 4, "nu_2": 10, "p": 256, "q2_bits": 20, "t_gsw": 2, "t_conv": 4, "t_exp_left": 8,
               "t_exp_right": 56, "instances": 1, "db_item_size": 8192, "direct_upload": 1}
# 512 x 32: k_sweep_narrow with two reductions of its u64 sums per output -- with 16 or 64 rows, or 4 columns, unreduced limbs are harmless
DIRECT_ROWS512 = dict(FAST, direct_upload=1, nu_1=9, nu_2=5, t_gsw=4, db_item_size=256)


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


# ------------------------------------------------------------------------------------------------------------ families
def _const(v):
    return lambda n, rng: np.full(n, v, dtype=np.uint64)


def _const_max(n, rng):
    w = np.zeros(n, dtype=np.uint64)
    w[::N] = Q - 1            # coefficient 0 of every polynomial: its NTT is q - 1 in every slot of both moduli
    return w


def _limbs(lo, hi):
    return lambda n, rng: np.full(n, lo | (hi << 32), dtype=np.uint64)


def _limbs_high(n, rng):
    return rng.integers(1 << 28, 1 << 32, n, dtype=np.uint64) | (rng.integers(1 << 28, 1 << 32, n, dtype=np.uint64) << np.uint64(32))


_FAMILIES = {
    "zero": _const(0), "ones": _const(U64),
    "Q": _const(Q), "Q-1": _const(Q - 1), "Q+1": _const(Q + 1), "2Q": _const(2 * Q),
    "kQ": _const(KQ), "kQ-1": _const(KQ - 1), "kQ+1": _const(KQ + 1),
    "q0": _const(Q0), "q1": _const(Q1), "q0-1": _const(Q0 - 1), "q1-1": _const(Q1 - 1),
    "2^28-1": _const((1 << 28) - 1), "2^28": _const(1 << 28), "2^32-1": _const((1 << 32) - 1), "2^32": _const(1 << 32),
    "2^56-1": _const((1 << 56) - 1), "2^63": _const(1 << 63), "2^63-1": _const((1 << 63) - 1), "2^63+1": _const((1 << 63) + 1),
    "full": lambda n, rng: rng.integers(0, 1 << 64, n, dtype=np.uint64),
    "const_max": _const_max,
    "digits_max": _const((1 << 55) - 1),      # < Q: every gadget digit of the wire half is all ones
}
# limb families of a direct-upload query's v_buf words (lo | hi << 32; the reference multiplies the limbs as they come)
_LIMB_FAMILIES = {
    "limbs-2^32-1": _limbs((1 << 32) - 1, (1 << 32) - 1), "limbs-q": _limbs(Q0, Q1), "limbs-q-1": _limbs(Q0 - 1, Q1 - 1),
    "limbs-high": _limbs_high,
}
ALL = list(_FAMILIES)
CORE = ["ones", "full", "const_max", "digits_max"]       # the families every flow beyond the single query sees


def craft(data, family, part="whole", seed=0, lo=0, hi=None):
    """`data` (public parameters or a query) with its 32-byte seed kept and the wire words [lo, hi) of its body overwritten by
    `family`: all of them (`whole`) or a random quarter (`quarter`: extreme and ordinary values meet in one polynomial)."""
    body = np.frombuffer(data[32:], dtype=np.uint64).copy()
    hi = body.size if hi is None else hi
    rng = np.random.default_rng([seed, sum(family.encode()), len(data) & 0xFFFF])
    gen = _FAMILIES.get(family) or _LIMB_FAMILIES[family]
    new = gen(hi - lo, rng)
    if part == "whole":
        body[lo:hi] = new
    else:
        assert part == "quarter"
        mask = rng.random(hi - lo) < 0.25
        body[lo:hi][mask] = new[mask]
    return bytes(data[:32]) + body.tobytes()


_BASE = {}


def _base(oracle_mod, cfg, idx=None, key_seed=7, with_db=True):
    """honest session + database of a configuration, kept for the parametrisations that follow (one at a time)"""
    import json
    key = (json.dumps(cfg, sort_keys=True), with_db)
    if key not in _BASE:
        _BASE.clear()
        o = oracle_mod.Params(cfg)
        cl = oracle_mod.Client(o)
        idx = (977 % o.num_items) if idx is None else idx
        c = {"o": o, "cl": cl, "pp": cl.generate_keys(key_seed), "q": cl.generate_query(idx, key_seed + 1)}
        if with_db:
            c["db"] = o.generate_random_db_and_get_item(idx)[1]
        _BASE[key] = c
    return _BASE[key]


# ------------------------------------------------------------------------------------------- 1. crafted wire words
@pytest.mark.parametrize("family", ALL)
@pytest.mark.parametrize("cfg", [FAST, FAST56], ids=["fast", "fast56"])
def test_pp_deserialize_crafted(sp, oracle_mod, cfg, family):
    """sp_pp_deserialize (ntt_fwd_body's plain path reduce64(word, q) on every wire word) == client.rs:212-259"""
    c = _base(oracle_mod, cfg, with_db=False)
    p = sp.Params(cfg)
    for part in ("whole", "quarter"):
        pp2 = craft(c["pp"], family, part)
        assert (sp.PublicParameters.deserialize(p, pp2).export() == c["o"].pp_deserialize_flat(pp2)).all(), part


@pytest.mark.parametrize("family", ALL)
@pytest.mark.parametrize("cfg", [FAST, FAST56, FUZZ11, FUZZ1], ids=["fast", "fast56", "fuzz11-28bit", "fuzz1-odd"])
def test_single_query_crafted(sp, oracle_mod, cfg, family):
    """expand_query and process_query bytes: crafted query with honest public parameters (whole body and a random quarter),
    honest query with crafted public parameters, both crafted."""
    c = _base(oracle_mod, cfg)
    o, pp, q, db = c["o"], c["pp"], c["q"], c["db"]
    p = sp.Params(cfg)
    gdb = sp.Database(p).load(db)
    cases = [(pp, craft(q, family, "whole")), (pp, craft(q, family, "quarter")), (craft(pp, family, "quarter"), q),
             (craft(pp, family, "whole"), q), (craft(pp, family, "whole"), craft(q, family, "quarter", seed=1))]
    for k, (pp2, q2) in enumerate(cases):
        gpp = sp.PublicParameters.deserialize(p, pp2)
        v_reg, v_fold = sp.expand_query(p, gpp, q2)
        e_reg, e_fold = o.expand_query(pp2, q2)
        assert (v_reg == e_reg).all() and (v_fold == e_fold).all(), k
        assert sp.process_query(p, gpp, q2, gdb) == o.process_query(pp2, q2, db), k


@pytest.mark.parametrize("name,cfg,B,bits", [
    ("narrow-5", FAST56, 5, set()),
    ("packed-8", {"n": 2, "nu_1": 6, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
                  "instances": 1, "db_item_size": 256}, 8, {"sweep_batch_mfma", "expand_group"}),
    ("packed-16", {"n": 2, "nu_1": 6, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
                   "instances": 1, "db_item_size": 256}, 16, {"sweep_batch_mfma_two_tiles", "sweep_batch_planar", "expand_group"})])
def test_query_lists_crafted_members(sp, oracle_mod, name, cfg, B, bits):
    """Lists (one pass per query on a narrow database; a PACKED group of 8 on k_sweep_mfma_batch; a two-tile group of 16 on the
    digit-planar copy -- k_ntt_fwd3_group is the group's begin) in which crafted and honest queries, and crafted and honest
    public parameters, sit in the SAME group: every response equals the oracle's for its (pp, q), and the honest members'
    responses equal what they are when the group holds honest queries only (nothing of a crafted neighbour leaks into shared
    tables)."""
    c = _base(oracle_mod, cfg)
    o, cl, pp, db = c["o"], c["cl"], c["pp"], c["db"]
    p = sp.Params(cfg)
    gdb = sp.Database(p).load(db)
    qs = [cl.generate_query((389 * i + 1) % o.num_items, 170 + i) for i in range(B)]
    pps = [pp] * B
    # members 1, 2, 5, 6 (and 9, 12 of the second tile): crafted query / crafted public parameters / both
    plan = {1: ("ones", "q"), 2: ("full", "q"), 5: ("const_max", "pp"), 6: ("digits_max", "both"), 9: ("ones", "both"), 12: ("full", "pp")}
    crafted_q, crafted_pp = list(qs), list(pps)
    for i, (family, what) in plan.items():
        if i >= B:
            continue
        if what in ("q", "both"):
            crafted_q[i] = craft(qs[i], family, "whole" if i % 2 else "quarter", seed=i)
        if what in ("pp", "both"):
            crafted_pp[i] = craft(pp, family, "quarter", seed=i)
    handles = {}
    for x in crafted_pp:
        if x not in handles:
            handles[x] = sp.PublicParameters.deserialize(p, x)
    gpps = [handles[x] for x in crafted_pp]
    honest = sp.process_query_batch(p, [handles[pp]] * B, qs, gdb)
    sp.paths_taken()
    got = sp.process_query_batch(p, gpps, crafted_q, gdb)
    assert bits <= sp.paths_taken()
    check = sorted(set(i for i in plan if i < B) | {0, B - 1})
    for i in check:
        assert got[i] == o.process_query(crafted_pp[i], crafted_q[i], db), i
    for i in range(B):
        if i not in plan:
            assert got[i] == honest[i], i
        assert got[i] == sp.process_query(p, gpps[i], crafted_q[i], gdb), i      # (tied to the oracle by the cases above)


@pytest.mark.parametrize("family", CORE)
@pytest.mark.parametrize("G", [2, 4])
def test_row_sharded_loopback_crafted(sp, oracle_mod, G, family):
    """sp_process_query_sharded with the pruned expansion on every rank's row shard (as test_process_query_sharded_c_abi_loopback)
    on a crafted query, then on an honest query under crafted public parameters."""
    from sdk_amd.sharding import LoopbackWorld
    cfg = dict(FAST56, nu_2=4)
    c = _base(oracle_mod, cfg)
    o, pp, q, db = c["o"], c["pp"], c["q"], c["db"]
    p = sp.Params(cfg)
    pp2, q2 = craft(pp, family, "quarter"), craft(q, family, "whole")
    gpp, gpp2 = sp.PublicParameters.deserialize(p, pp), sp.PublicParameters.deserialize(p, pp2)
    expect = [o.process_query(pp, q2, db), o.process_query(pp2, q, db)]
    shards = [sp.Database(p, s, G).load(db) for s in range(G)]
    world = LoopbackWorld(G)

    def rank_main(r):
        sp.lib().sp_set_device(0)
        sp.paths_taken()
        out = [world.comm(r).process_query(p, gpp, q2, shards[r]), world.comm(r).process_query(p, gpp2, q, shards[r])]
        return out, sp.paths_taken()
    res = world.run(rank_main)
    assert res[0][0] == expect                  # sp_process_query_sharded leaves the response on rank 0 ...
    for r in range(G):
        assert r == 0 or res[r][0] == [b"", b""]          # ... and nothing on the others
        assert "expand_pruned" in res[r][1], res[r][1]


@pytest.mark.parametrize("family", CORE)
def test_sparse_bucket_crafted(sp, oracle_mod, family):
    """a sparse bucket (pruned begin, k_sweep_sparse, fold shortcuts) against oracle.SparseDb.process_query"""
    cfg = dict(FAST, nu_1=4, nu_2=3, db_item_size=256)
    o = oracle_mod.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(11)
    q = cl.generate_query(5, 12)
    rng = np.random.default_rng(9)
    sdb = oracle_mod.SparseDb(o)
    p = sp.Params(cfg)
    gdb = sp.Database.sparse(p)
    for idx in rng.choice(o.num_items, 40, replace=False):
        data = rng.integers(0, 256, 256, dtype=np.uint8).tobytes()
        sdb.update_item_raw(int(idx), data)
        gdb.update_item(int(idx), data)
    for pp2, q2 in ((pp, craft(q, family, "whole")), (craft(pp, family, "quarter"), craft(q, family, "quarter"))):
        gpp = sp.PublicParameters.deserialize(p, pp2)
        sp.paths_taken()
        assert sp.process_query(p, gpp, q2, gdb) == sdb.process_query(pp2, q2)
        assert "sweep_sparse" in sp.paths_taken()


def test_private_read_one_crafted_request(sp, oracle_mod):
    """the request layer: one crafted request per family in a list of honest ones"""
    cfg = dict(FAST, nu_2=7, db_item_size=256)
    c = _base(oracle_mod, cfg)
    o, cl, pp, db = c["o"], c["cl"], c["pp"], c["db"]
    p = sp.Params(cfg)
    srv = sp.Server(p, sp.Database(p).load(db))
    uuid = srv.setup(pp).encode()
    qs = [cl.generate_query((911 * i + 7) % o.num_items, 500 + i) for i in range(5)]
    honest = [o.process_query(pp, x, db) for x in qs]
    for k, family in enumerate(CORE):
        bad = craft(qs[k], family, "whole" if k % 2 else "quarter")
        reqs = list(qs)
        reqs[k] = bad
        out = srv.private_read([uuid + x for x in reqs])
        assert out[k] == o.process_query(pp, bad, db), family
        assert [x for i, x in enumerate(out) if i != k] == [x for i, x in enumerate(honest) if i != k], family


@pytest.mark.parametrize("family", ALL + list(_LIMB_FAMILIES))
@pytest.mark.parametrize("cfg", [NO_EXPANSION, dict(FAST, direct_upload=1), DIRECT_WIDE, DIRECT_ROWS512],
                         ids=["no-expansion", "fast-direct", "wide", "rows512"])
def test_direct_upload_crafted(sp, oracle_mod, cfg, family):
    """Direct-upload queries (server.rs:666-679; run_begin_direct): the families on the v_buf words (k_interleave_query has to
    reduce both limbs: the sweeps' u64 sums and the digit split need them < 2^28) and on the GSW rows."""
    c = _base(oracle_mod, cfg)
    o, pp, q, db = c["o"], c["pp"], c["q"], c["db"]
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    gdb = sp.Database(p).load(db)
    nbuf = o.dim0 * N                                    # v_buf words (client.rs:315-327), then the GSW rows
    assert (len(q) - 32) // 8 > nbuf
    cases = [craft(q, family, "whole", hi=nbuf)]
    if family in _FAMILIES:
        cases += [craft(q, family, "whole", lo=nbuf), craft(q, family, "quarter")]
    else:
        cases += [craft(q, family, "quarter", hi=nbuf)]
    if cfg is DIRECT_WIDE or cfg is DIRECT_ROWS512:   # (the oracle is slow at these sizes: v_buf whole, and a quarter of everything)
        cases = [cases[0], cases[-1]]
    for k, q2 in enumerate(cases):
        assert sp.process_query(p, gpp, q2, gdb) == o.process_query(pp, q2, db), k


# ------------------------------------------------------- 2. both operands of the matrix-core pass at their digit extremes
def _signed_digits(x):
    """the query side's carry-propagated signed base-256 digits (sweep_mfma.hpp signed_digits): bytes 0-2 in [-128, 127], byte 3 >= 0"""
    v = ((x + 0x808080) ^ 0x808080) & 0xFFFFFFFF
    d = [(v >> (8 * i)) & 0xFF for i in range(4)]
    return [b - 256 if (b >= 128 and i < 3) else b for i, b in enumerate(d)]


def _offset_digits(x):
    """the database side's offset digits (byte a of x) - 128"""
    return [((x >> (8 * i)) & 0xFF) - 128 for i in range(4)]


def _digit_sums(x, y, nj):
    """D_s of nj equal rows with database residue x and query residue y"""
    dx, dy = _offset_digits(x), _signed_digits(y)
    return [nj * sum(dx[a] * dy[s - a] for a in range(4) if 0 <= s - a < 4) for s in range(7)]



# residues at the edges of both digit forms: every byte 0x80 / 0x7f, the largest top digit, q - 1, 0, 1; 0 and 0x..FFFF are the
# offset form's -128 and +127
_X_LO = [0x00808080, 0x007F7F7F, Q0 - 1, 0, 0x0F7F7F7F, 0x0F808080, 0x0080807F, 1, 0x0FFEFFFF, 0x0000FFFF]
_X_HI = [0x00808080, 0x007F7F7F, Q1 - 1, 0, 0x0E7F7F7F, 0x0E808080, 0x0E80807F, 1, 0x0EDFFFFF, 0x0000FFFF]


def _recombined(D, q):
    """what combine_digit_sums adds its bias to: D_0 + 2^8 D_1 + 2^16 D_2 + 2^24 D_3 + c4 D_4 + c5 D_5 + c6 D_6 with
    c_s = 256^s mod q -- a signed integer, congruent to sum_j x_j y_j minus the offset term"""
    return sum(D[s] << (8 * s) for s in range(4)) + sum(D[s] * pow(256, s, q) for s in range(4, 7))


def _worst_pairs(xs, q, nj):
    """of the extreme set: the (database, query) residue pair with the largest |D_s| and the one with the most negative
    recombined value, for nj equal rows"""
    by_d = max(((x, y) for x in xs for y in xs), key=lambda xy: max(abs(d) for d in _digit_sums(xy[0], xy[1], nj)))
    by_v = min(((x, y) for x in xs for y in xs), key=lambda xy: _recombined(_digit_sums(xy[0], xy[1], nj), q))
    return by_d, by_v


def _extreme_case(sp, oracle_mod, nu_1, B, nj):
    """Database and direct-upload queries of section 2: per (plane, z, column) one database residue pair and per (query, z) one
    query residue pair from the extreme set, the same in every row, so that the digit sums do not cancel (same sign in every
    row where the digits agree in sign, opposite where they differ).  z = 0 and z = 1 of every column and of query 0 hold the
    pairs _worst_pairs names: the magnitudes below are those of planted inputs.  `nj` = rows one pass sees (a shard's)."""
    cfg = {"n": 2, "nu_1": nu_1, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8,
           "t_exp_right": 56, "instances": 1, "db_item_size": 256 << max(0, 9 - nu_1), "direct_upload": 1}
    o = oracle_mod.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(51)
    dim0, num_per = o.dim0, o.num_per
    (d_lo, v_lo), (d_hi, v_hi) = _worst_pairs(_X_LO, Q0, nj), _worst_pairs(_X_HI, Q1, nj)
    reached = max(max(abs(d) for d in _digit_sums(*d_lo, nj)), max(abs(d) for d in _digit_sums(*d_hi, nj)))
    v_min = {q: _recombined(_digit_sums(*pair, nj), q) for q, pair in ((Q0, v_lo), (Q1, v_hi))}
    bound = 4 * nj * (1 << 14)
    print("nj %d: largest |D_s| planted %d, claimed bound %d (4 nj 2^14), combine_digit_sums assumes < %d; most negative recombined "
          "value %d (mod q0), %d (mod q1); bias q 2^29 = %d, %d" % (nj, reached, bound, 1 << 26, v_min[Q0], v_min[Q1], Q0 << 29, Q1 << 29))
    assert 0.7 * bound <= reached <= bound <= (1 << 25)
    for q in (Q0, Q1):
        assert v_min[q] + (q << 29) > 0                  # the kernel's bias covers the most negative value these inputs give
    if nj == 512:
        # at the largest row count the passes take, a bias of q 2^23 or less would leave the planted sum negative (with the true
        # constants 2^32, 2^40, 2^48 mod q no residue pair below q reaches -q 2^25: that takes 1352 equal rows mod q1, 9778 mod q0)
        assert v_min[Q1] + (Q1 << 23) < 0 < v_min[Q1] + (Q1 << 25)
    rng = np.random.default_rng(5)
    lo, hi = np.array(_X_LO, dtype=np.uint64), np.array(_X_HI, dtype=np.uint64)
    pick = rng.integers(0, len(_X_LO), (4, N, num_per, 1))
    col = lo[pick] | (hi[(pick + 3) % len(_X_HI)] << np.uint64(32))
    col[:, 0] = v_lo[0] | (v_hi[0] << 32)
    col[:, 1] = d_lo[0] | (d_hi[0] << 32)
    db = np.ascontiguousarray(np.broadcast_to(col, (4, N, num_per, dim0))).reshape(-1)    # [plane][z][ii][j]: every row equal
    qs = []
    for b in range(B):
        q = cl.generate_query((977 * b + 1) % o.num_items, 600 + b)
        body = np.frombuffer(q[32:], dtype=np.uint64).copy()
        pq = rng.integers(0, len(_X_LO), (N, 1))
        # (every third query with limbs above q, which the interleave kernel reduces to the same extreme residues)
        w = (lo[pq] + np.uint64(Q0 * (b % 3 == 2))) | ((hi[(pq + b) % len(_X_HI)] + np.uint64(Q1 * (b % 3 == 2))) << np.uint64(32))
        if b == 0:
            w[0] = v_lo[1] | (v_hi[1] << 32)
            w[1] = d_lo[1] | (d_hi[1] << 32)
        body[:N * dim0] = np.broadcast_to(w, (N, dim0)).reshape(-1)                        # v_buf [z][j]
        qs.append(bytes(q[:32]) + body.tobytes())
    return cfg, o, pp, db, qs


@pytest.mark.parametrize("name,nu_1,B,planar,bits", [
    ("one-tile-64", 6, 8, 1, {"sweep_batch_mfma"}),
    ("one-tile-512", 9, 8, 1, {"sweep_batch_mfma"}),
    ("two-tiles-packed-512", 9, 16, 0, {"sweep_batch_mfma_two_tiles"}),
    ("planar-512", 9, 16, 1, {"sweep_batch_mfma_two_tiles", "sweep_batch_planar"})])
def test_matrix_core_pass_both_operands_extreme(sp, oracle_mod, name, nu_1, B, planar, bits):
    """k_sweep_mfma_batch (one and two query tiles) and k_sweep_planar with database AND query residues from the extreme set
    (_extreme_case), at the largest row count their launch conditions take (nj <= 512: mfma_shape_ok, sweep_planar_ok).
    Computed from the planted inputs: the largest |D_s| is 0.77 of the bound 4 nj 2^14 the kernel comments give (25952256 of
    2^25 at 512 rows), below the 2^26 combine_digit_sums assumes; the most negative recombined value is -3173343055446016
    (mod q1, 512 rows) against a bias of q1 2^29 = 1.3e17.  Expected bytes: the oracle's exact u128 sums."""
    cfg, o, pp, db, qs = _extreme_case(sp, oracle_mod, nu_1, B, 1 << nu_1)
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    gdb = sp.Database(p).load(db)
    sp.lib().sp_debug_set(b"batch_planar", C.c_long(planar))
    try:
        sp.paths_taken()
        resp = sp.process_query_batch(p, [gpp] * B, qs, gdb)
        taken = sp.paths_taken()
    finally:
        sp.lib().sp_debug_set(b"batch_planar", C.c_long(1))
    assert bits <= taken and ("sweep_batch_planar" in taken) == ("sweep_batch_planar" in bits), taken
    for i in sorted({0, 2, 7, B - 1}):
        assert resp[i] == o.process_query(pp, qs[i], db), i
    for i in range(B):
        assert resp[i] == sp.process_query(p, gpp, qs[i], gdb), i


@pytest.mark.parametrize("nu_1,G", [(6, 2), (10, 2)], ids=["64-rows-G2", "1024-rows-G2"])
def test_scatter_form_pass_both_operands_extreme(sp, oracle_mod, nu_1, G):
    """k_sweep_mfma_scatter (the batched pass over a row shard, sp_process_queries_sharded_batched over the loopback world) on the
    same extreme database and direct-upload queries; 1024 rows over two ranks = 512 rows per pass, the most
    sweep_batch_scatter_ok takes.  Rank 0 holds the responses (the other ranks return []): the oracle's bytes over the unsharded
    database; every rank's pass was the scatter kernel."""
    from sdk_amd.sharding import LoopbackWorld
    B = 8
    cfg, o, pp, db, qs = _extreme_case(sp, oracle_mod, nu_1, B, (1 << nu_1) // G)
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    shards = [sp.Database(p, s, G).load(db) for s in range(G)]
    world = LoopbackWorld(G)

    def rank_main(r):
        sp.lib().sp_set_device(0)
        sp.paths_taken()
        return world.comm(r).process_queries_batched(p, [gpp] * B, qs, shards[r]), sp.paths_taken()
    res = world.run(rank_main)
    for r in range(G):
        assert {"sweep_batch_scatter", "scatter_out"} <= res[r][1], res[r][1]
        assert r == 0 or res[r][0] == []
    got = res[0][0]
    for i in (0, 2, 7):
        assert got[i] == o.process_query(pp, qs[i], db), i
    gdb = sp.Database(p).load(db)
    for i in range(B):
        assert got[i] == sp.process_query(p, gpp, qs[i], gdb), i          # (the unsharded single query, tied to the oracle above)


# --------------------------------------------------------------- 3. stage exports at the corners of their accumulators
def _limb_words(rng, n, kind):
    if kind == "ones":
        return np.full(n, U64, dtype=np.uint64)
    if kind == "full":
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if kind == "top":            # q - 1 in both limbs: 256 products fill the sweeps' u64 sums to 0.9995 of 2^64
        return np.full(n, (Q0 - 1) | ((Q1 - 1) << 32), dtype=np.uint64)
    assert kind == "canonical"
    return rng.integers(0, Q0, n, dtype=np.uint64) | (rng.integers(0, Q1, n, dtype=np.uint64) << np.uint64(32))


@pytest.mark.parametrize("kinds", [("canonical", "ones"), ("canonical", "full"), ("ones", "canonical"), ("full", "full"), ("ones", "ones"), ("top", "top")],
                         ids=lambda k: "db_%s-q_%s" % k)
@pytest.mark.parametrize("dim0,num_per", [(64, 4), (512, 32), (16, 64), (300, 128), (64, 256), (512, 1), (700, 2),
                                          (1024, 2), (1024, 64), (1024, 128), (2048, 4),
                                          pytest.param(257, 128, id="odd-257-128"), pytest.param(3, 256, id="odd-3-256")])
def test_multiply_reg_by_database_any_limbs(sp, oracle_mod, dim0, num_per, kinds):
    """sp_multiply_reg_by_database with limbs >= q up to 2^32 - 1 in `db` and in `v_firstdim`, at every shape of
    test_multiply_reg_by_database_shapes (k_sweep_narrow, the PACKED kernels) and at two wide shapes with an odd row count
    (k_sweep_wide).  The reference sums in u128 and is exact for any limbs (server.rs:186-217), the kernels sum up to 256 products
    in u64: the export reduces both operands' limbs on upload.  `top`: both operands q - 1 in every limb of every row, so that every reduction of a full block of 256 rows sees
    256 (q - 1)^2 = 0.9995 * 2^64 (reduce64's quotient estimate at its worst: an estimate two short leaves 2q <= r < 3q, which
    one conditional subtraction does not bring below q) and, at 1024 rows, the last block's result is stored as it comes."""
    p, o = sp.Params(FAST), oracle_mod.Params(FAST)
    rng = np.random.default_rng(dim0 * 1000 + num_per)
    db = _limb_words(rng, N * num_per * dim0, kinds[0])
    qv = _limb_words(rng, N * dim0 * 2, kinds[1])
    sp.paths_taken()
    got = sp.multiply_reg_by_database(p, db, qv, dim0, num_per)
    taken = sp.paths_taken()
    assert (got == o.multiply_reg_by_database(db, qv, dim0, num_per)).all()
    if num_per >= 128:     # an odd row count cannot be PACKED: the 8-byte words and k_sweep_wide
        assert ("sweep_wide" if dim0 % 2 else "sweep_packed_persist") in taken and len({"sweep_wide", "sweep_packed_persist"} & taken) == 1, taken


@pytest.mark.parametrize("num_per_log,dim0_log", [(7, 3), (5, 4)], ids=["packed", "narrow"])
def test_db_load_any_limbs(sp, oracle_mod, num_per_log, dim0_log):
    """sp_db_load + sp_db_read_ref on words with limbs up to 2^32 - 1: the resident database holds the canonical residues
    (canon_word in both re-layout kernels; 8-byte and PACKED formats), and a query over it answers as the oracle does over the
    words as they came."""
    cfg = dict(FAST, nu_1=dim0_log, nu_2=num_per_log, t_gsw=2)
    p, o = sp.Params(cfg), oracle_mod.Params(cfg)
    dim0, num_per = 1 << dim0_log, 1 << num_per_log
    rng = np.random.default_rng(num_per_log)
    words = rng.integers(0, 1 << 64, 4 * N * num_per * dim0, dtype=np.uint64)
    words[::5] = U64
    words[1::7] = Q0 | (Q1 << 32)
    canon = (words & np.uint64(0xFFFFFFFF)) % np.uint64(Q0) | (((words >> np.uint64(32)) % np.uint64(Q1)) << np.uint64(32))
    ref = canon.reshape(4, N, num_per, dim0)
    gdb = sp.Database(p).load(words)
    for _ in range(60):
        pl, z, ii = int(rng.integers(4)), int(rng.integers(N)), int(rng.integers(num_per))
        assert (gdb.read_ref(pl, z, ii, 0, dim0) == ref[pl, z, ii]).all()
    cl = oracle_mod.Client(o)
    pp, q = cl.generate_keys(3), cl.generate_query(5, 4)
    gpp = sp.PublicParameters.deserialize(p, pp)
    assert sp.process_query(p, gpp, q, gdb) == o.process_query(pp, q, words)


@pytest.mark.parametrize("variant", ["0", "3", "5"])
@pytest.mark.parametrize("t_gsw", [2, 3, 8, 28])
def test_fold_exports_at_accumulator_corners(sp, oracle_mod, monkeypatch, t_gsw, variant):
    """sp_fold_ciphertexts and sp_fold_ciphertexts_fused (every level fused / library default; SPIRAL_FOLD_VARIANT 0, 3, 5) on raw
    ciphertexts all Q - 1, all 0, 2^55 - 1 and alternating 0 / Q - 1 between the halves of every fold pair (the largest digit
    differences of the delta form, both signs), with v_folding all q - 1 (canonical NTT form), all 0 and honest: the lazy sums
    of 2 t_gsw products at their largest.  t_gsw = 2 has 28-bit digits (>= q possible)."""
    monkeypatch.setenv("SPIRAL_FOLD_VARIANT", variant)
    cfg = dict(FAST56, nu_2=4, t_gsw=t_gsw)
    o = oracle_mod.Params(cfg)
    p = sp.Params(cfg)
    cl = oracle_mod.Client(o)
    pp, q = cl.generate_keys(33), cl.generate_query(7, 34)
    honest = o.expand_query(pp, q)[1]
    top = np.tile(np.concatenate([np.full(N, Q0 - 1, dtype=np.uint64), np.full(N, Q1 - 1, dtype=np.uint64)]), honest.size // (2 * N))
    num_per = o.num_per
    shape = (num_per, 2 * N)
    alt = np.zeros(shape, dtype=np.uint64)
    alt[[i for i in range(num_per) if bin(i).count("1") % 2]] = Q - 1          # the two halves of every pair differ at every level
    cts_set = {"Q-1": np.full(shape, Q - 1, dtype=np.uint64), "zero": np.zeros(shape, dtype=np.uint64),
               "2^55-1": np.full(shape, (1 << 55) - 1, dtype=np.uint64), "alt": alt, "alt-inv": np.uint64(Q - 1) - alt}
    for vname, v_fold in (("top", top), ("zero", np.zeros_like(honest)), ("honest", honest)):
        v_neg = o.get_v_folding_neg(v_fold)
        for cname, cts in cts_set.items():
            raw = cts.reshape(-1)
            expect = o.fold_ciphertexts(raw, v_fold, v_neg)[:2 * N]
            assert (sp.fold_ciphertexts(p, raw, v_fold, v_neg)[:2 * N] == expect).all(), (vname, cname)
            for thr in (1, 0):
                assert (sp.fold_ciphertexts_fused(p, raw, v_fold, fused_min_pairs=thr)[:2 * N] == expect).all(), (vname, cname, thr)


def test_no_gadget_width_has_digits_between_q_and_2_28(sp, oracle_mod):
    """ntt_fwd_body takes gadget digits of at most 28 bits as they come and sends wider ones through reduce64.  get_bits_per
    (gadget.rs:3-9: floor(56 / t) + 1) gives 57, 29, 19, 15, ... bits for t = 1, 2, 3, 4, ...: never 20 to 28.  So every digit
    taken as it comes is below 2^19 < q, and t = 2 (29 bits) is reduced: no digit >= q can reach the subtraction of the delta
    form for any parameter set, and its `val >= m.q` step has no input that needs it.  A change of the gadget widths that
    makes 28-bit digits possible fails here first (and then needs fold cases with digits 2^28 - 1)."""
    o = oracle_mod.Params(FAST)
    p = sp.Params(FAST)
    for t in range(1, 57):
        bits = o.get_bits_per(t)
        assert bits <= 19 or bits >= 29, (t, bits)
        assert (1 << min(bits, 19)) < min(Q0, Q1)
    for t in (2, 3):
        cfg = dict(FAST, t_gsw=t)
        assert sp.Params(cfg).get("modulus") == Q and oracle_mod.Params(cfg).get_bits_per(t) == {2: 29, 3: 19}[t]
    del p


def test_multiply_export_all_top(sp, oracle_mod):
    """sp_multiply at 2 x 2 t_gsw . 2 t_gsw x 1 with both operands q - 1 in every slot"""
    for t in (8, 28):
        cfg = dict(FAST, t_gsw=t)
        p, o = sp.Params(cfg), oracle_mod.Params(cfg)
        poly = np.concatenate([np.full(N, Q0 - 1, dtype=np.uint64), np.full(N, Q1 - 1, dtype=np.uint64)])
        a, b = np.tile(poly, 2 * 2 * t), np.tile(poly, 2 * t)
        assert (sp.multiply(p, a, 2, 2 * t, b, 1) == o.multiply(a, 2, 2 * t, b, 1)).all()


@pytest.mark.parametrize("cfg", [FAST56, FUZZ11], ids=["fast56", "fuzz11-28bit"])
def test_expansion_conversion_pack_exports_const_max_keys(sp, oracle_mod, cfg):
    """sp_coefficient_expansion, sp_regev_to_gsw and sp_pack against a public-parameter handle made from `const_max` wire rows
    (key rows q - 1 in every NTT slot), inputs q - 1 in every slot (NTT form) and the NTT of `const_max` / `digits_max` raw
    polynomials: the lazy sums of t and 2 t products at their largest."""
    o = oracle_mod.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = craft(cl.generate_keys(60), "const_max")
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    flat = o.pp_deserialize_flat(pp)
    assert (gpp.export() == flat).all()
    w = 2 * o.ntt_words
    top_ct = np.tile(np.concatenate([np.full(N, Q0 - 1, dtype=np.uint64), np.full(N, Q1 - 1, dtype=np.uint64)]), 2)
    g, sr, mb = o.g, o.stop_round, o.t_gsw * o.db_dim_2
    for name, ct in (("top", top_ct), ("const_max", o.to_ntt(_const_max(2 * N, None))), ("digits_max", o.to_ntt(np.full(2 * N, (1 << 55) - 1, dtype=np.uint64)))):
        v = np.zeros((1 << g) * w, dtype=np.uint64)
        v[:w] = ct
        v_cpu = o.coefficient_expansion(pp, v, g, sr, mb)
        assert (sp.coefficient_expansion(p, gpp, v, g, sr, mb) == v_cpu).all(), name
        v_inp = np.tile(ct, mb)
        v_conv = flat[-2 * 2 * o.t_conv * o.ntt_words:]
        assert (sp.regev_to_gsw(p, gpp, v_inp, o.db_dim_2) == o.regev_to_gsw(v_inp, v_conv, o.db_dim_2)).all(), name
        v_ct = np.tile(o.from_ntt(ct), o.n * o.n)
        v_w = flat[:o.n * (o.n + 1) * o.t_conv * o.ntt_words]
        assert (sp.pack(p, gpp, v_ct) == o.pack(v_ct, v_w)).all(), name


def _rescale_boundaries(lo_mod, hi_mod):
    """inputs a in [0, hi_mod) either side of every place where rescale(a, hi_mod, lo_mod) (arith.rs:429-444: recentre, multiply
    by lo_mod, add hi_mod / 2 towards the sign, divide truncating, reduce) steps to its next value, for the first and last
    few output values"""
    out = set()
    ks = list(range(0, 4)) + list(range(lo_mod - 4, lo_mod + 1)) + [lo_mod // 2 - 1, lo_mod // 2, lo_mod // 2 + 1]
    for k in ks:
        # |a| lo_mod + hi_mod / 2 crosses k hi_mod at |a| = ceil((k hi_mod - hi_mod / 2) / lo_mod), on both signs
        edge = -(-(k * hi_mod - hi_mod // 2) // lo_mod)
        for e in (edge - 1, edge, edge + 1):
            out.add(e % hi_mod)
            out.add((-e) % hi_mod)
    out |= {hi_mod // 2 - 1, hi_mod // 2, hi_mod // 2 + 1}
    return sorted(out)


@pytest.mark.parametrize("p_mod", [4, 256, 65536])
@pytest.mark.parametrize("q2_bits", [14, 20, 27])
def test_encode_rounding_boundaries(sp, oracle_mod, q2_bits, p_mod):
    """sp_encode (server.rs:470-503): 0, 1, Q - 1, Q / 2, Q / 2 +- 1 and the values either side of the rounding boundaries of both
    rescale calls (Q -> q2 on the first row, Q -> q1 = 4 p on the rest), first and last few output values."""
    cfg = dict(FAST, p=p_mod, q2_bits=q2_bits)
    if 8192 * 8 > 4 * N * int(np.log2(p_mod)):
        cfg["db_item_size"] = 4 * N * int(np.log2(p_mod)) // 8
    o = oracle_mod.Params(cfg)
    p = sp.Params(cfg)
    vals = [0, 1, Q - 1, Q // 2, Q // 2 - 1, Q // 2 + 1] + _rescale_boundaries(1 << q2_bits, Q) + _rescale_boundaries(4 * p_mod, Q)
    words = (o.n + 1) * o.n * N
    rng = np.random.default_rng(q2_bits * 7 + p_mod)
    v = np.array([vals[i] for i in rng.integers(0, len(vals), words)], dtype=np.uint64)
    v[:len(vals)] = np.array(vals, dtype=np.uint64)               # each at least once in the first (q2) row ...
    v[-len(vals):] = np.array(vals, dtype=np.uint64)              # ... and in the last (q1) row
    assert len(vals) <= N
    assert sp.encode(p, v) == o.encode(v)
