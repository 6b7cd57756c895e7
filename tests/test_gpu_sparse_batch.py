"""A list of queries on a sparse bucket with one pass over the bucket per group of up to 8 (k_sweep_sparse_batch, the sparse flow
of sp_process_query_batch): every response byte for byte equal to oracle.SparseDb.process_query on the same bytes, present items
decoded.  Every case forces the group flow with sp_debug_set("sparse_batch_min", 2) and restores the switch afterwards, so nothing
here depends on the shipped default.  tests/test_emulated_sparse_batch.py runs subsets of this file on the emulated device."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import FAST

GROUP = "sparse_group_pass"


@contextlib.contextmanager
def batch_min(sp, value):
    sp.lib().sp_debug_set(b"sparse_batch_min", C.c_long(value))
    try:
        yield
    finally:
        sp.lib().sp_debug_set(b"sparse_batch_min", C.c_long(int(os.environ.get("SPIRAL_SPARSE_BATCH_MIN", -1))))   # negative: the shipped default


def _random_item(rng, size):
    return rng.integers(0, 256, size, dtype=np.uint8).tobytes()


class Bucket:
    """one sparse bucket on both sides (the GPU library's and the oracle's restatement of lib/server), `n_clients` clients' keys"""

    def __init__(self, oracle_mod, cfg, n_clients=1):
        import sdk_amd as sp
        self.sp, self.cfg = sp, cfg
        self.o, self.p = oracle_mod.Params(cfg), sp.Params(cfg)
        self.clients = []
        for k in range(n_clients):
            cl = oracle_mod.Client(self.o)
            pp = cl.generate_keys(11 + k)
            self.clients.append((cl, pp, sp.PublicParameters.deserialize(self.p, pp)))
        self.sdb, self.gdb = oracle_mod.SparseDb(self.o), sp.Database.sparse(self.p)
        self.num_per, self.dim0, self.size = 1 << cfg["nu_2"], 1 << cfg["nu_1"], cfg["db_item_size"]
        self.items = {}

    def put(self, idx, data):
        self.gdb.update_item(idx, data)
        self.sdb.update_item_raw(idx, data)
        self.items[idx] = bytes(data)

    def fill_columns(self, lens, rng):
        """column ii gets lens[ii] random items in random rows"""
        assert len(lens) == self.num_per
        cols = []
        for ii, n in enumerate(lens):
            cols.append([int(j) for j in np.sort(rng.choice(self.dim0, n, replace=False))])
            for j in cols[-1]:
                self.put(j * self.num_per + ii, _random_item(rng, self.size))
        return cols

    def queries(self, idxs, seed):
        """[(client number, item index, query bytes)]: the clients alternate, every query has its own seed"""
        return [(k % len(self.clients), idx, self.clients[k % len(self.clients)][0].generate_query(idx, seed + k)) for k, idx in enumerate(idxs)]

    def want(self, qs):
        return [self.sdb.process_query(self.clients[c][1], q) for c, _, q in qs]

    def ask(self, qs):
        """the list through sp_process_query_batch -> (responses, paths taken)"""
        self.sp.paths_taken()
        got = self.sp.process_query_batch(self.p, [self.clients[c][2] for c, _, _ in qs], [q for _, _, q in qs], self.gdb)
        return got, self.sp.paths_taken()

    def check(self, qs, want, decodes=None, grouped=True):
        """the group flow's responses == `want`, present items decode (t_gsw = 8; the first `decodes` bytes, default all)"""
        with batch_min(self.sp, 2):
            got, taken = self.ask(qs)
        if grouped:
            assert {GROUP, "sweep_sparse", "fold_fused"} <= taken, taken
        assert not any(t.startswith("sweep_batch") for t in taken), taken
        assert [g == w for g, w in zip(got, want)] == [True] * len(qs) and len(got) == len(want)
        if self.cfg.get("t_gsw", 8) == 8:
            n = self.size if decodes is None else decodes
            for (c, idx, _), resp in zip(qs, got):
                if idx in self.items:
                    assert self.clients[c][0].decode_response(resp)[:n] == self.items[idx].ljust(self.size, b"\0")[:n], idx
        return got


# ---- 1. group sizes and slots -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_bucket(oracle_mod):
    """nu = (6, 3), 256-byte items, 150 random items, two clients' keys alternating; eleven distinct queries -- one for an absent
    item, one item asked for twice -- with the oracle's answers, computed once"""
    b = Bucket(oracle_mod, dict(FAST, nu_1=6, nu_2=3, db_item_size=256), n_clients=2)
    rng = np.random.default_rng(31)
    for idx in rng.choice(b.dim0 * b.num_per, 150, replace=False):
        b.put(int(idx), _random_item(rng, b.size))
    present = list(b.items)
    absent = next(i for i in range(b.dim0 * b.num_per) if i not in b.items)
    idxs = present[:11]
    idxs[1] = absent
    idxs[2] = idxs[0]              # the same item again, same client (k = 0, 2), another query seed
    qs = b.queries(idxs, 300)
    assert len({q for _, _, q in qs}) == 11
    return b, qs, b.want(qs)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 8, 9, 11])
def test_group_sizes_and_slots(small_bucket, n):
    """2: the B = 2 body; 3: the B = 4 body with a dead slot; 8: the B = 8 body; 9: 8 + one query of the per-query flow;
    11: 8 + 3.  The path bit is what fails without the group flow."""
    b, qs, want = small_bucket
    b.check(qs[:n], want[:n])


# ---- 2. accumulator range -----------------------------------------------------------------------------------------------
# the pass folds its u64 sums after every 255 items of a column: columns one item either side of a fold (255, 256 / 257), two
# folds (512), one item, an empty column beside deep ones.  The nu_1 = 8 shapes are the emulated device's (tests/test_emulated_sparse_batch.py)
@pytest.mark.gpu
@pytest.mark.parametrize("nu,lens", [((9, 2), (512, 255, 256, 0)), ((9, 2), (257, 1, 0, 300)), ((8, 2), (256, 255, 0, 1)), ((8, 1), (256, 3))],
                         ids=["nu1_9-512-255-256-0", "nu1_9-257-1-0-300", "nu1_8-256-255-0-1", "nu1_8-256-3"])
def test_accumulator_range(oracle_mod, nu, lens):
    b = Bucket(oracle_mod, dict(FAST, nu_1=nu[0], nu_2=nu[1], db_item_size=256), n_clients=2)
    cols = b.fill_columns(lens, np.random.default_rng(sum(lens)))
    assert b.gdb.sparse_items() == sum(lens)
    idxs = []
    for ii, rows in enumerate(cols):        # first, middle and last present row of every column, an absent item of an empty one
        idxs += [j * b.num_per + ii for j in sorted({rows[0], rows[len(rows) // 2], rows[-1]})] if rows else [ii]
    idxs = (idxs * 8)[:8]
    qs = b.queries(idxs, 400)
    assert len({q for _, _, q in qs}) == 8
    want = b.want(qs)
    b.check(qs, want)              # B = 8, eight distinct queries
    b.check(qs[:2], want[:2])      # B = 2


# ---- 3. planes and gadgets ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n_items", [(dict(FAST, nu_1=6, nu_2=4, db_item_size=16384, instances=2, version=1), 40),
                                         (dict(FAST, nu_1=3, nu_2=2, db_item_size=256, t_gsw=7, t_conv=3, t_exp_left=5, t_exp_right=5, q2_bits=22), 32)],
                         ids=["two-instances-pack-v1", "full-bucket-server-gadgets"])
def test_planes_and_gadgets(oracle_mod, cfg, n_items):
    b = Bucket(oracle_mod, cfg, n_clients=2)
    rng = np.random.default_rng(5)
    for idx in rng.choice(b.o.num_items, n_items, replace=False):
        b.put(int(idx), _random_item(rng, b.size))
    assert b.gdb.sparse_items() == n_items
    qs = b.queries(list(b.items)[:5], 500)
    b.check(qs, b.want(qs))


# ---- 4. shortcuts -------------------------------------------------------------------------------------------------------
_SHORTCUT_CFG = dict(FAST, nu_1=3, nu_2=4, db_item_size=256)


@pytest.mark.gpu
def test_shortcuts_empty_bucket(oracle_mod):
    b = Bucket(oracle_mod, _SHORTCUT_CFG, n_clients=2)
    qs = b.queries([0, 17, b.dim0 * b.num_per - 1], 600)
    b.check(qs, b.want(qs))


@pytest.mark.gpu
def test_shortcuts_right_half_empty(oracle_mod):
    b = Bucket(oracle_mod, _SHORTCUT_CFG, n_clients=2)
    rng = np.random.default_rng(14)
    cols = b.fill_columns([2 if ii < b.num_per // 2 else 0 for ii in range(b.num_per)], rng)
    idxs = [cols[0][0] * b.num_per, cols[7][1] * b.num_per + 7, cols[3][0] * b.num_per + 3, b.num_per + 12]   # the last one absent
    qs = b.queries(idxs, 610)
    want = b.want(qs)
    dense = [b.o.process_query(b.clients[c][1], q, b.sdb.to_dense()) for c, _, q in qs]
    assert all(w != d for w, d in zip(want, dense))     # a fold shortcut fired in every answer
    b.check(qs, want)


@pytest.mark.gpu
def test_shortcuts_zero_and_short_items(oracle_mod):
    """a zero-length record and a 3-byte item (every plane but the first zero) beside ordinary columns: under the shortcuts a plane
    that is zero in the selected column comes back as its sibling's, as in lib/server, so the short item decodes in its first chunk"""
    b = Bucket(oracle_mod, _SHORTCUT_CFG, n_clients=2)
    rng = np.random.default_rng(17)
    for ii in range(6, b.num_per):
        for j in rng.choice(b.dim0, 3, replace=False):
            b.put(int(j) * b.num_per + ii, _random_item(rng, b.size))
    b.put(2 * b.num_per + 0, b"")
    b.put(7 * b.num_per + 5, bytes(rng.integers(1, 256, 3, dtype=np.uint8)))
    chunk = b.size // 4
    qs = b.queries([2 * b.num_per, 7 * b.num_per + 5], 620)
    want = b.want(qs)
    got = b.check(qs, want, decodes=0)
    assert b.clients[1][0].decode_response(got[1])[:chunk] == b.items[7 * b.num_per + 5].ljust(chunk, b"\0")


# ---- 5. snapshots -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_snapshots_follow_upserts(oracle_mod):
    b = Bucket(oracle_mod, dict(FAST, nu_1=6, nu_2=3, db_item_size=256), n_clients=2)
    rng = np.random.default_rng(23)
    for idx in rng.choice(b.dim0 * b.num_per, 40, replace=False):
        b.put(int(idx), _random_item(rng, b.size))
    present = list(b.items)
    new = next(i for i in range(b.dim0 * b.num_per) if i not in b.items)
    qs = b.queries([present[0], new, present[1], present[2]], 700)
    before = b.want(qs)
    b.check(qs, before)
    b.put(present[0], bytes(reversed(b.items[present[0]])))      # a present item overwritten
    b.put(new, _random_item(rng, b.size))                        # a new item
    assert b.gdb.sparse_items() == 41
    after = b.want(qs)
    assert after[0] != before[0] and after[1] != before[1]
    b.check(qs, after)                                           # (decodes the overwritten and the new item)


# ---- 6. switch ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_switch_off_gives_the_same_bytes(small_bucket):
    b, qs, want = small_bucket
    with batch_min(b.sp, 0):
        got, taken = b.ask(qs[:5])
    assert got == want[:5]
    assert GROUP not in taken and "sweep_sparse" in taken, taken
    b.check(qs[:5], want[:5])


# ---- 7. request layer ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_private_read_on_a_sparse_bucket(small_bucket):
    b, qs, want = small_bucket
    srv = b.sp.Server(b.p, b.gdb)
    uuids = [srv.setup(pp) for _, pp, _ in b.clients]
    assert srv.clients() == 2
    with batch_min(b.sp, 2):
        b.sp.paths_taken()
        out = srv.private_read([uuids[c].encode() + q for c, _, q in qs[:5]])
        taken = b.sp.paths_taken()
    assert out == want[:5]
    assert GROUP in taken, taken


# ---- 8. errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_member_then_a_good_list(small_bucket):
    b, qs, want = small_bucket
    bad = list(qs[:4])
    bad[2] = (bad[2][0], bad[2][1], bad[2][2][:-1])
    with batch_min(b.sp, 2):
        with pytest.raises(b.sp.SpiralError):
            b.ask(bad)
    b.check(qs[:4], want[:4])


# ---- 9. the pass alone ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bench_sweep_batch_takes_a_sparse_bucket(small_bucket, oracle_mod):
    b, qs, _ = small_bucket
    sp = b.sp
    for n in (8, 3):
        runs = [sp.QueryRun(b.p, b.clients[c][2], q, db=b.gdb) for c, _, q in qs[:n]]
        try:
            sp.paths_taken()
            ms = sp.bench_sweep_batch(runs, b.gdb, 2)
            assert ms > 0 and GROUP in sp.paths_taken()
        finally:
            for r in runs:
                r.free()
    # a dense 8-byte database is still refused
    cfg = dict(FAST, nu_2=2, db_item_size=256)
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    cl = oracle_mod.Client(o)
    gpp = sp.PublicParameters.deserialize(p, cl.generate_keys(3))
    dense = sp.Database(p).fill_synthetic(1)
    run = sp.QueryRun(p, gpp, cl.generate_query(1, 4))
    try:
        with pytest.raises(sp.SpiralError, match="the batched pass needs an unsharded PACKED database"):
            sp.bench_sweep_batch([run], dense, 1)
    finally:
        run.free()
