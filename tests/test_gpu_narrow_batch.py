"""A list of queries on a narrow database (8-byte words, 2 <= num_per <= 64) with one pass over the database per group of up to 8
(k_sweep_narrow_batch, GroupedFlow of sp_process_query_batch): every response byte for byte equal to oracle.Params.process_query on
the same bytes, planted items decoded.  Every case forces the flow with sp_debug_set("narrow_batch_min", 2) and restores the switch
afterwards, so nothing here depends on the shipped default.  Two clients' keys alternate within a list.
tests/test_emulated_narrow_batch.py runs a subset of this file on the emulated device."""
import base64
import contextlib
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from conftest import FAST, FAST56, SMALL_INST2

GROUP, SINGLE = "sweep_narrow_group", "sweep_narrow"
Q0, Q1 = 268369921, 249561089
SERVER_GADGETS = dict(FAST, nu_1=3, nu_2=2, db_item_size=256, t_gsw=7, t_conv=3, t_exp_left=5, t_exp_right=5, q2_bits=22)
NO_EXPANSION = {"direct_upload": 1, "n": 5, "nu_1": 6, "nu_2": 3, "p": 65536, "q2_bits": 27, "t_gsw": 3, "t_conv": 56,
                "t_exp_left": 56, "t_exp_right": 56}   # the set of tests/test_gpu_parity.py (get_no_expansion_testing_params)


@contextlib.contextmanager
def switch(sp, name, value, default=-1):
    sp.lib().sp_debug_set(name.encode(), C.c_long(value))
    try:
        yield
    finally:
        sp.lib().sp_debug_set(name.encode(), C.c_long(int(os.environ.get("SPIRAL_" + name.upper(), default))))


def batch_min(sp, value):
    return switch(sp, "narrow_batch_min", value)   # negative: the shipped default


class Dense:
    """one dense database on both sides (the GPU library's and the oracle's), `n_clients` clients' keys, one planted item"""

    def __init__(self, oracle_mod, cfg, n_clients=2, planted=5):
        import sdk_amd as sp
        self.sp, self.cfg = sp, cfg
        self.o, self.p = oracle_mod.Params(cfg), sp.Params(cfg)
        self.clients = []
        for k in range(n_clients):
            cl = oracle_mod.Client(self.o)
            pp = cl.generate_keys(21 + k)
            self.clients.append((cl, pp, sp.PublicParameters.deserialize(self.p, pp)))
        self.planted = planted % self.o.num_items
        self.item, self.words = self.o.generate_random_db_and_get_item(self.planted)
        self.gdb = sp.Database(self.p).load(self.words)

    def queries(self, n, seed):
        """[(client number, item index, query bytes)]: the clients alternate, every query its own seed; the first asks for the planted item"""
        idxs = [(self.planted + 37 * k) % self.o.num_items for k in range(n)]
        return [(k % len(self.clients), idx, self.clients[k % len(self.clients)][0].generate_query(idx, seed + k)) for k, idx in enumerate(idxs)]

    def want(self, qs):
        return [self.o.process_query(self.clients[c][1], q, self.words) for c, _, q in qs]

    def ask(self, qs):
        """the list through sp_process_query_batch -> (responses, paths taken)"""
        self.sp.paths_taken()
        got = self.sp.process_query_batch(self.p, [self.clients[c][2] for c, _, _ in qs], [q for _, _, q in qs], self.gdb)
        return got, self.sp.paths_taken()

    def check(self, qs, want, grouped=True, single=False):
        """the forced group flow's responses == `want`; the planted item decodes; which sweeps ran"""
        with batch_min(self.sp, 2):
            got, taken = self.ask(qs)
        assert (GROUP in taken) == grouped, taken
        assert (SINGLE in taken) == single, taken
        assert not any(t.startswith("sweep_batch") for t in taken), taken
        assert [g == w for g, w in zip(got, want)] == [True] * len(qs) and len(got) == len(want)
        for (c, idx, _), resp in zip(qs, got):
            if idx == self.planted:
                assert self.clients[c][0].decode_response(resp) == self.o.item_to_vec(self.item)
        return got, taken


# ---- 1. group sizes and slots -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_db(oracle_mod):
    """FAST56, nu = (6, 3): eleven distinct queries of two clients with the oracle's answers, computed once"""
    d = Dense(oracle_mod, FAST56)
    qs = d.queries(11, 300)
    assert len({q for _, _, q in qs}) == 11
    return d, qs, d.want(qs)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 11])
def test_group_sizes_and_slots(small_db, n):
    """2: the B = 2 body; 3: B = 4 with a dead slot; 4; 5: B = 8 with three dead slots; 8; 9: 8 + one query of the per-query flow;
    11: 8 + 3.  The path bit is what fails without the group flow."""
    d, qs, want = small_db
    d.check(qs[:n], want[:n], single=(n == 9))


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------
# (4, 1): 32 words per row block, most threads idle; (6, 6): num_per = 64; (9, 2): exactly one full slab of 512 rows;
# (10, 1): two slabs, num_per = 2; (6, 0): num_per = 1 is not the group pass's -- same bytes, the group bit absent
@pytest.mark.gpu
@pytest.mark.parametrize("nu", [(4, 1), (6, 6), (9, 2), (10, 1), (6, 0)], ids=lambda nu: "nu%d_%d" % nu)
def test_shapes(oracle_mod, nu):
    d = Dense(oracle_mod, dict(FAST, nu_1=nu[0], nu_2=nu[1], db_item_size=256), planted=3)
    qs = d.queries(8, 400)
    want = d.want(qs)
    grouped = nu[1] > 0
    d.check(qs, want, grouped=grouped, single=not grouped)            # B = 8
    d.check(qs[:2], want[:2], grouped=grouped, single=not grouped)    # B = 2


# ---- 3. planes, packing, gadgets, direct upload -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n", [(dict(SMALL_INST2, version=1), 5), (SERVER_GADGETS, 5), (NO_EXPANSION, 3)],
                         ids=["two-instances-pack-v1", "server-gadgets", "direct-upload"])
def test_planes_packing_gadgets_direct_upload(oracle_mod, cfg, n):
    d = Dense(oracle_mod, cfg)
    qs = d.queries(n, 500)
    _, taken = d.check(qs, d.want(qs))
    if cfg.get("direct_upload"):
        assert "expand_group" not in taken and "direct_upload" in taken, taken   # members begun one by one


# ---- 4. the pass alone: accumulator edges -------------------------------------------------------------------------------
def _partial(sp, run):
    """host copy of a run's partial buffer (uint32)"""
    run.sync()
    n = run.partial_words()
    if hasattr(sp.lib(), "sp_emulated_device_marker"):     # the CPU suite's emulated device: device memory is host memory
        return np.ctypeslib.as_array(C.cast(run.partial_ptr(), C.POINTER(C.c_uint32)), shape=(n,)).copy()
    from sdk_amd.sharding import partial_tensor
    return partial_tensor(run).cpu().numpy().view(np.uint32).copy()


def _clear_partial(sp, run):
    run.sync()
    if hasattr(sp.lib(), "sp_emulated_device_marker"):
        C.memset(run.partial_ptr(), 0xA5, run.partial_words() * 4)
    else:
        import torch
        from sdk_amd.sharding import partial_tensor
        partial_tensor(run).fill_(-1)
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("fold_every", [1, 2, 255], ids=["fold1", "fold2", "fold-default"])
@pytest.mark.parametrize("kind", ["max", "random"])
@pytest.mark.parametrize("nu", [(9, 2), (6, 6)], ids=lambda nu: "nu%d_%d" % nu)
def test_pass_alone_accumulator_edges(oracle_mod, nu, kind, fold_every):
    """sp_bench_sweep_batch(..., iters = 1) on B = 2 .. 8 begun queries leaves in every member's partial buffer, word for word,
    what the same query's own sp_query_sweep leaves.  Every database word (q0 - 1) | (q1 - 1) << 32 -- the largest products the
    sums can meet -- or random; a fold after every product, every second one, and the default.  (A single query is no group:
    sp_bench_sweep_batch refuses it on an 8-byte database, as tests/test_gpu_sparse_batch.py pins.)"""
    import sdk_amd as sp
    cfg = dict(FAST, nu_1=nu[0], nu_2=nu[1], db_item_size=256)
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    n_words = 4 * 2048 * o.num_per * o.dim0
    if kind == "max":
        words = np.full(n_words, (Q0 - 1) | ((Q1 - 1) << 32), dtype=np.uint64)
    else:
        rng = np.random.default_rng(nu[0])
        words = rng.integers(0, Q0, n_words, dtype=np.uint64) | (rng.integers(0, Q1, n_words, dtype=np.uint64) << np.uint64(32))
    gdb = sp.Database(p).load(words)
    clients = []
    for k in range(2):
        cl = oracle_mod.Client(o)
        clients.append((cl, sp.PublicParameters.deserialize(p, cl.generate_keys(31 + k))))
    runs = [sp.QueryRun(p, clients[k % 2][1], clients[k % 2][0].generate_query((11 * k + 1) % o.num_items, 600 + k), db=gdb) for k in range(8)]
    try:
        got = {}
        with switch(sp, "narrow_batch_fold_every", fold_every, default=255):
            with pytest.raises(sp.SpiralError, match="the batched pass needs an unsharded PACKED database"):
                sp.bench_sweep_batch(runs[:1], gdb, 1)
            for B in range(2, 9):
                for r in runs[:B]:
                    _clear_partial(sp, r)
                sp.paths_taken()
                assert sp.bench_sweep_batch(runs[:B], gdb, 1) > 0
                assert GROUP in sp.paths_taken()
                got[B] = [_partial(sp, r) for r in runs[:B]]
        ref = [_partial(sp, r.sweep(gdb)) for r in runs]
        assert max(int(x.max()) for x in ref) < Q0 and any(int(x.max()) > 0 for x in ref)
        for B in range(2, 9):
            for k in range(B):
                assert np.array_equal(got[B][k], ref[k]), (B, k, int((got[B][k] != ref[k]).sum()))
    finally:
        for r in runs:
            r.free()


# ---- 5. switch ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_switch_off_gives_the_same_bytes(small_db):
    d, qs, want = small_db
    with batch_min(d.sp, 0):
        got, taken = d.ask(qs[:5])
    assert got == want[:5]
    assert GROUP not in taken and SINGLE in taken, taken
    d.check(qs[:5], want[:5])


# ---- 6. upsert between lists --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_upsert_between_lists(oracle_mod):
    import sdk_amd as sp
    cfg = dict(FAST, nu_1=6, nu_2=3, db_item_size=256)
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    rng = np.random.default_rng(41)
    blob = rng.integers(0, 256, o.num_items * 256, dtype=np.uint8)
    gdb = sp.Database(p).load_items(blob)
    clients = []
    for k in range(2):
        cl = oracle_mod.Client(o)
        pp = cl.generate_keys(51 + k)
        clients.append((cl, pp, sp.PublicParameters.deserialize(p, pp)))
    idxs = [77, 200, 78, 3]
    qs = [(k % 2, idx, clients[k % 2][0].generate_query(idx, 700 + k)) for k, idx in enumerate(idxs)]

    def ask_and_check(blob_now):
        words = o.load_db_from_bytes(blob_now.tobytes())
        with batch_min(sp, 2):
            sp.paths_taken()
            got = sp.process_query_batch(p, [clients[c][2] for c, _, _ in qs], [q for _, _, q in qs], gdb)
            assert GROUP in sp.paths_taken()
        assert got == [o.process_query(clients[c][1], q, words) for c, _, q in qs]
        for (c, idx, _), resp in zip(qs, got):
            assert clients[c][0].decode_response(resp)[:256] == blob_now[idx * 256:(idx + 1) * 256].tobytes(), idx
        return got

    before = ask_and_check(blob)
    new = rng.integers(0, 256, 256, dtype=np.uint8)
    gdb.update_item(77, new.tobytes())
    blob[77 * 256:78 * 256] = new
    after = ask_and_check(blob)     # (decodes the new item)
    assert after[0] != before[0]


# ---- 7. errors and threads ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_member_then_a_good_list(small_db):
    d, qs, want = small_db
    bad = list(qs[:5])
    bad[2] = (bad[2][0], bad[2][1], bad[2][2][:-8])     # wrong length in the middle of a group
    with batch_min(d.sp, 2):
        with pytest.raises(d.sp.SpiralError):
            d.ask(bad)
    d.check(qs[:5], want[:5])


@pytest.mark.gpu
def test_two_threads_submit_lists(small_db):
    d, qs, want = small_db
    got, errs = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                sub = qs[t:7 + t]
                got[t] = d.sp.process_query_batch(d.p, [d.clients[c][2] for c, _, _ in sub], [q for _, _, q in sub], d.gdb)
        except Exception as e:  # pragma: no cover
            errs.append(e)
    with batch_min(d.sp, 2):
        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        [t.start() for t in th]
        [t.join() for t in th]
    assert not errs
    assert got[0] == want[0:7] and got[1] == want[1:8]


# ---- 8. request layer ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_private_read_on_a_narrow_database(small_db):
    d, qs, want = small_db
    srv = d.sp.Server(d.p, d.gdb)
    uuids = [srv.setup(pp) for _, pp, _ in d.clients]
    body = json.dumps([base64.b64encode(uuids[c].encode() + q).decode() for c, _, q in qs[:5]])
    with batch_min(d.sp, 2):
        d.sp.paths_taken()
        out = json.loads(srv.private_read_json(body))
        taken = d.sp.paths_taken()
    assert [base64.b64decode(x) for x in out] == want[:5]
    assert GROUP in taken, taken
