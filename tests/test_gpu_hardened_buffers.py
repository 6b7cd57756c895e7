"""Every flow of the library on device buffers that do not start at zero, and between guard regions.

devbuf_alloc (sdk_amd/csrc/server.cpp) zero-fills every fresh device buffer and says that no kernel ever reads a word it did not
write.  Zero is the one fill that hides such a read -- an accumulator, an atomicOr-packed output word, an addend that aliases its
output all come out right when they start at 0 -- so every flow runs here in two modes, on handles of its own:

  poison   sp_debug_set("poison_ws", 0xA5): every fresh DevBuf is filled with the byte (the single-query flows and the list of 16
           once more with 0xFF: the result must not depend on the fill)
  guard    sp_debug_set("guard_ws", 1 MiB): guard regions on both sides of every buffer, checked when it is released (the report goes
           to stderr: "[spiral] OUT-OF-BOUNDS WRITE around alloc ..."); under guards a buffer is neither poisoned nor zeroed, so
           this mode also runs on raw memory

Both act at allocation time only: a case computes (or takes from the module's cache) the oracle's answers, sets its switch, creates
its own Params, public parameters, database and query runs, compares every response or exported array byte for byte with the
oracle's, checks the path names the flow is meant to take, releases every handle it made -- the workspace pool goes with the Params
handle; a case that leaves a handle alive has checked nothing -- and only then, in guard mode, reads the captured stderr.  The switch
goes back to 0 in a `finally`.  Two cases show that the instruments work, and the last test compares the union of the path names the
poisoned cases took with everything sp_path_name knows.  tests/test_emulated_hardened_buffers.py runs a subset on the emulated device."""
import base64
import contextlib
import ctypes as C
import gc
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import FAST, FAST56, SMALL_INST2
from test_gpu_bulk_upsert import _body
from test_gpu_narrow_batch import NO_EXPANSION, SERVER_GADGETS, switch

pytestmark = pytest.mark.gpu

Q0, Q1 = 268369921, 249561089
Q = Q0 * Q1
N = 2048
TOP = (Q0 - 1) | ((Q1 - 1) << 32)
POISON = 0xA5                    # the fills of the stale-read hunt on record (profiles/r02_stale_reads.md): 0xA5, 0xFF
GUARD_BYTES = 1 << 20            # the value INTEGRATION.md documents
RETIRED_BITS = (1, 16, 21, 23, 26, 30)     # kernels.hpp: path bits whose kernels are gone
PACKED = dict(FAST, nu_1=6, nu_2=7, db_item_size=256)                  # 64 x 128: PACKED words, matrix cores, the planar copy
RING = {"n": 2, "nu_1": 5, "nu_2": 10, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
        "instances": 1, "db_item_size": 8192}                          # test_ring_sweep_and_batched_tails_parity's pipelined shape
LDS_STAGED = dict(RING, nu_1=4, nu_2=9, t_gsw=2)                       # test_process_query_batch_lds_staged's
SPARSE = dict(FAST, nu_1=6, nu_2=3, db_item_size=256)
_POISONED_PATHS = set()          # union of the path names the poisoned cases took (test_poisoned_cases_cover_every_path)
_POISONED_CASES = []


# ---- the oracle's side: computed before any switch is set, cached per (config, seeds) -------------------------------------------
def _many(fn, args):
    """[fn(a) for a in args] on up to 8 host threads (the oracle's calls release the interpreter lock)"""
    args = list(args)
    if len(args) < 2:
        return [fn(a) for a in args]
    with ThreadPoolExecutor(min(8, len(args))) as ex:
        return list(ex.map(fn, args))


class Case:
    """one configuration on the oracle's side: clients' keys, a database in reference layout, queries and the oracle's responses"""

    def __init__(self, oracle_mod, cfg, words=None, planted=5, key_seed=21, n_clients=2):
        self.cfg, self.o = cfg, oracle_mod.Params(cfg)
        self.clients = []
        for k in range(n_clients):
            cl = oracle_mod.Client(self.o)
            self.clients.append((cl, cl.generate_keys(key_seed + k)))
        self.planted = planted % self.o.num_items
        self.item, self.words = self.o.generate_random_db_and_get_item(self.planted) if words is None else (None, words(self.o))
        self._q, self._want = {}, {}

    def queries(self, n, seed=300):
        """[(client number, item index, query bytes)]: the clients alternate, every query its own seed"""
        for k in range(n):
            if (seed, k) not in self._q:
                c, idx = k % len(self.clients), (self.planted + 37 * k) % self.o.num_items
                self._q[(seed, k)] = (c, idx, self.clients[c][0].generate_query(idx, seed + k))
        return [self._q[(seed, k)] for k in range(n)]

    def want(self, qs, words=None, tag=""):
        """the oracle's responses to `qs` over `words` (default: the case's database); `tag` names an edited database"""
        words = self.words if words is None else words
        todo = [(c, q) for c, _, q in qs if (tag, q) not in self._want]
        for (c, q), resp in zip(todo, _many(lambda cq: self.o.process_query(self.clients[cq[0]][1], cq[1], words), todo)):
            self._want[(tag, q)] = resp
        return [self._want[(tag, q)] for _, _, q in qs]


_CASES = {}


_SMALL = {}       # the sparse bucket and the stage exports' references


def _case(oracle_mod, cfg, words_key="", **kw):
    """the cached Case of (config, seeds); the three used last are kept (the databases are up to 2 GiB: the flows of one shape are
    neighbours in FLOWS)"""
    key = json.dumps([cfg, words_key, sorted((k, v) for k, v in kw.items() if k != "words")], sort_keys=True)
    case = _CASES.pop(key, None) or Case(oracle_mod, cfg, **kw)
    _CASES[key] = case
    while len(_CASES) > 3:
        _CASES.pop(next(iter(_CASES)))
    return case


def _blob_case(oracle_mod, cfg, seed):
    """a database preprocessed from `num_items` records of random bytes -> (case, blob as a uint8 array)"""
    o = oracle_mod.Params(cfg)
    blob = np.random.default_rng(seed).integers(0, 256, o.num_items * o.db_item_size, dtype=np.uint8)
    case = _case(oracle_mod, cfg, words=lambda o_: o_.load_db_from_bytes(blob.tobytes()), words_key="blob%d" % seed, key_seed=31)
    return case, blob


# ---- the library's side: handles made after the switch is set, released before stderr is read -----------------------------------
class Side:
    def __init__(self, sp):
        self.sp, self.objs = sp, []

    def own(self, obj):
        self.objs.append(obj)
        return obj

    def params(self, cfg):
        return self.own(self.sp.Params(cfg))

    def pps(self, p, case):
        return [self.own(self.sp.PublicParameters.deserialize(p, pp)) for _, pp in case.clients]

    def db(self, p, *a, **kw):
        return self.own(self.sp.Database(p, *a, **kw))

    def run(self, *a, **kw):
        return self.own(self.sp.QueryRun(*a, **kw))

    def close(self):
        """query runs and communicators freed, servers, databases, public parameters and Params deleted, newest first"""
        for o in reversed(self.objs):
            (o.free if hasattr(o, "free") else o.__del__)()
        del self.objs[:]
        gc.collect()


def _hardened(flow, mode, fill, oracle_mod, capfd, record=False):
    """`flow(sp, oracle_mod, S, arm)` computes the oracle's side, calls arm() -- the switch -- and only then makes handles through S;
    it returns the path names it took"""
    import sdk_amd as sp
    assert sp.lib().sp_device_count() >= 1, "no HIP device visible"
    name, value = ("guard_ws", GUARD_BYTES) if mode == "guard" else ("poison_ws", fill)
    S, armed = Side(sp), []

    def arm():
        sp.lib().sp_debug_set(name.encode(), C.c_long(value))
        armed.append(value)
        return value
    capfd.readouterr()
    try:
        taken = flow(sp, oracle_mod, S, arm)
        assert armed, "the flow made its handles without the switch"
    finally:
        try:
            S.close()
        finally:
            sp.lib().sp_debug_set(name.encode(), C.c_long(0))
    err = capfd.readouterr().err
    assert "OUT-OF-BOUNDS" not in err, err[-2000:]
    if record and mode == "poison":
        _POISONED_PATHS.update(taken)
        _POISONED_CASES.append(flow.__name__)
    return taken


@contextlib.contextmanager
def env_switch(name, value):
    """SPIRAL_<NAME> in the environment for the calls inside (the library reads it again at every public entry point) and nothing
    left behind: a value set with sp_debug_set stays in the process and shadows the environment of every later test, so switches
    that other tests set through the environment (fold_variant, pipe_ring, ...) are set that way here too"""
    key = "SPIRAL_" + name.upper()
    old = os.environ.get(key)
    os.environ[key] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


def _ask(sp, p, gpps, qs, gdb):
    """the list through sp_process_query_batch -> (responses, paths taken)"""
    sp.paths_taken()
    got = sp.process_query_batch(p, [gpps[c] for c, _, _ in qs], [q for _, _, q in qs], gdb)
    return got, sp.paths_taken()


def _same(got, want):
    assert len(got) == len(want) and [g == w for g, w in zip(got, want)] == [True] * len(want)


def _named(name):
    def deco(f):
        f.__name__ = name
        return f
    return deco


# ---- flows: single queries ------------------------------------------------------------------------------------------------------
def _single(name, cfg, paths, absent=()):
    @_named(name)
    def flow(sp, oracle_mod, S, arm):
        case = _case(oracle_mod, cfg)
        qs = case.queries(2)
        want = case.want(qs)
        arm()
        p = S.params(cfg)
        gpps, gdb = S.pps(p, case), S.db(p).load(case.words)
        sp.paths_taken()
        got = [sp.process_query(p, gpps[c], q, gdb) for c, _, q in qs]     # (the second on the first one's pooled workspace)
        taken = sp.paths_taken()
        _same(got, want)
        if cfg.get("t_gsw", 8) == 8:     # (fewer gadget digits: too noisy to decode, the bytes still have to agree)
            assert case.clients[0][0].decode_response(got[0]) == case.o.item_to_vec(case.item)
        assert set(paths) <= taken and not (set(absent) & taken), taken
        return taken
    return flow


SINGLE_FLOWS = [
    _single("single-fast56", FAST56, {"sweep_narrow", "from_sweep4", "fold_tail_delta"}),
    _single("single-nu2_0", dict(FAST, nu_2=0, db_item_size=8192), {"sweep_narrow", "from_sweep1"}),
    _single("single-nu2_1", dict(FAST, nu_2=1), {"sweep_narrow", "from_sweep1", "fold_tail_delta"}),
    _single("single-packed", PACKED, {"sweep_packed_persist", "sweep_ring", "from_sweep4_xcd_order", "fold_fused", "fold_wave", "fold_tail_delta"}),
    _single("single-ring-pipelined", RING, {"pipelined_fold_overlap", "sweep_ring", "fold_tail_batched", "expand_split"}),
    _single("single-direct-upload-n5", NO_EXPANSION, {"direct_upload", "sweep_narrow"}),
    _single("single-inst2-pack-v1", dict(SMALL_INST2, version=1), {"pack_v1", "sweep_narrow"}),
    _single("single-server-gadgets", SERVER_GADGETS, {"sweep_narrow"}),
]


@_named("single-db-unpacked")
def _single_unpacked(sp, oracle_mod, S, arm):
    """the 8-byte wide database: k_sweep_wide where the shape would have been PACKED (tests/test_gpu_parity.py has the handle flows)"""
    case = _case(oracle_mod, PACKED)
    qs = case.queries(1)
    want = case.want(qs)
    arm()
    with switch(sp, "db_unpacked", 1, default=0):
        p = S.params(PACKED)
        gpps, gdb = S.pps(p, case), S.db(p).load(case.words)
    sp.paths_taken()
    got = [sp.process_query(p, gpps[c], q, gdb) for c, _, q in qs]
    taken = sp.paths_taken()
    _same(got, want)
    assert "sweep_wide" in taken and not ({"sweep_packed_persist", "sweep_ring"} & taken), taken
    return taken


# ---- flows: lists through sp_process_query_batch --------------------------------------------------------------------------------
def _list(name, cfg, n, paths, absent=(), switches=()):
    @_named(name)
    def flow(sp, oracle_mod, S, arm):
        case = _case(oracle_mod, cfg)
        qs = case.queries(n)
        want = case.want(qs)
        arm()
        p = S.params(cfg)
        gpps, gdb = S.pps(p, case), S.db(p).load(case.words)
        ctx = [switch(sp, nm, v, default=d) for nm, v, d in switches]
        for c in ctx:
            c.__enter__()
        try:
            got, taken = _ask(sp, p, gpps, qs, gdb)
        finally:
            for c in reversed(ctx):
                c.__exit__(None, None, None)
        _same(got, want)
        assert set(paths) <= taken and not (set(absent) & taken), taken
        return taken
    return flow


LIST_FLOWS = [
    _list("list3-fast56-in-flight", FAST56, 3, {"sweep_narrow"}, absent={"sweep_narrow_group"}),
    _list("list5-fast56-narrow-group", FAST56, 5, {"sweep_narrow_group"}, absent={"sweep_narrow"}, switches=[("narrow_batch_min", 2, -1)]),
    _list("list3-packed-valu", PACKED, 3, {"sweep_batch", "expand_group"}, absent={"sweep_batch_mfma"}),
    _list("list8-packed-matrix-cores", PACKED, 8, {"sweep_batch_mfma", "expand_group", "expand_round_one_launch"},
          absent={"sweep_batch_mfma_two_tiles"}),
    _list("list16-packed-planar", PACKED, 16, {"sweep_batch_mfma_two_tiles", "sweep_batch_planar", "expand_group"}),
    _list("list16-packed-two-tiles", PACKED, 16, {"sweep_batch_mfma_two_tiles"}, absent={"sweep_batch_planar"}, switches=[("batch_planar", 0, 1)]),
    # (56 one-bit digits on the expansion's right-hand side: the group's large rounds run on k_expand_wave)
    _list("list11-lds-staged", LDS_STAGED, 11, {"sweep_batch", "expand_group", "expand_wave"}, absent={"sweep_batch_mfma"}),
]


class SparseCase:
    """a small sparse bucket on the oracle's side: 150 random items of nu = (6, 3), two clients, queries for present items, an
    absent one and the same item twice"""

    def __init__(self, oracle_mod, cfg=SPARSE, seed=31):
        self.cfg, self.o = cfg, oracle_mod.Params(cfg)
        self.clients = []
        for k in range(2):
            cl = oracle_mod.Client(self.o)
            self.clients.append((cl, cl.generate_keys(11 + k)))
        rng = np.random.default_rng(seed)
        self.sdb, self.items = oracle_mod.SparseDb(self.o), {}
        for idx in rng.choice(self.o.num_items, 150, replace=False):
            self.items[int(idx)] = rng.integers(0, 256, cfg["db_item_size"], dtype=np.uint8).tobytes()
            self.sdb.update_item_raw(int(idx), self.items[int(idx)])
        idxs = list(self.items)[:5]
        idxs[1] = next(i for i in range(self.o.num_items) if i not in self.items)
        idxs[2] = idxs[0]
        self.qs = [(k % 2, idx, self.clients[k % 2][0].generate_query(idx, 300 + k)) for k, idx in enumerate(idxs)]
        self.want = [self.sdb.process_query(self.clients[c][1], q) for c, _, q in self.qs]
        # an /update-row body on top: an overwrite (shorter: the padding clears the old bytes), a new key in an occupied row, a new row's
        free_row = next(j for j in range(64) if not any(i // 8 == j for i in self.items))
        self.records = [(idxs[0], rng.integers(1, 256, 200, dtype=np.uint8).tobytes()),
                        ((idxs[3] // 8) * 8 + (idxs[3] + 1) % 8, rng.integers(0, 256, 256, dtype=np.uint8).tobytes()),
                        (free_row * 8 + 3, rng.integers(0, 256, 255, dtype=np.uint8).tobytes())]
        for i, d in self.records:
            self.sdb.update_item_raw(i, d)
        self.qs_after = [(k % 2, i, self.clients[k % 2][0].generate_query(i, 400 + k)) for k, (i, _) in enumerate(self.records)] + self.qs[3:]
        self.want_after = [self.sdb.process_query(self.clients[c][1], q) for c, _, q in self.qs_after]

    def bucket(self, S, p):
        gdb = S.own(S.sp.Database.sparse(p))
        for idx, data in self.items.items():
            gdb.update_item(idx, data)
        return gdb


def _sparse_case(oracle_mod):
    if "sparse" not in _SMALL:
        _SMALL["sparse"] = SparseCase(oracle_mod)
    return _SMALL["sparse"]


@_named("list5-and-1-sparse-bucket")
def _sparse_lists(sp, oracle_mod, S, arm):
    case = _sparse_case(oracle_mod)
    arm()
    p = S.params(case.cfg)
    gpps, gdb = S.pps(p, case), case.bucket(S, p)
    with switch(sp, "sparse_batch_min", 2):
        got, taken = _ask(sp, p, gpps, case.qs, gdb)
        one, taken1 = _ask(sp, p, gpps, case.qs[:1], gdb)
    _same(got + one, case.want + case.want[:1])
    assert {"sparse_group_pass", "sweep_sparse", "fold_fused"} <= taken and "sweep_sparse" in taken1 and "sparse_group_pass" not in taken1, (taken, taken1)
    return taken | taken1


# ---- flows: writers, then queries -----------------------------------------------------------------------------------------------
@_named("writer-load-items-windows")
def _load_items_windows(sp, oracle_mod, S, arm):
    """sp_db_load_items through upload windows of two row pairs each, items that spill into the next window (1001 bytes in 4 chunks)"""
    cfg = dict(FAST, nu_1=4, nu_2=1, db_item_size=1001)
    case, blob = _blob_case(oracle_mod, cfg, 5)
    qs = case.queries(2)
    want = case.want(qs)
    arm()
    p = S.params(cfg)
    gpps = S.pps(p, case)
    with switch(sp, "db_load_window", 4 * case.o.num_per * case.o.db_item_size, default=512 << 20):
        gdb = S.db(p).load_items(blob)
    ref = case.words.reshape(4, N, case.o.num_per, case.o.dim0)
    for pl, z, ii in ((0, 0, 0), (1, 500, 1), (3, 2047, 1)):
        assert (gdb.read_ref(pl, z, ii, 0, case.o.dim0) == ref[pl, z, ii]).all(), (pl, z, ii)
    sp.paths_taken()
    got = [sp.process_query(p, gpps[c], q, gdb) for c, _, q in qs]
    taken = sp.paths_taken()
    _same(got, want)
    assert "sweep_narrow" in taken, taken
    return taken


@_named("writer-update-item")
def _update_item(sp, oracle_mod, S, arm):
    cfg = dict(FAST, db_item_size=256)
    case, blob = _blob_case(oracle_mod, cfg, 41)
    qs = case.queries(2)            # item 5, item 42
    new = np.random.default_rng(42).integers(0, 256, 250, dtype=np.uint8)
    edited = blob.copy()
    edited[5 * 256:6 * 256] = 0
    edited[5 * 256:5 * 256 + 250] = new
    want = case.want(qs, case.o.load_db_from_bytes(edited.tobytes()), tag="edited")
    arm()
    p = S.params(cfg)
    gpps, gdb = S.pps(p, case), S.db(p).load_items(blob)
    gdb.update_item(5, new.tobytes())
    sp.paths_taken()
    got = [sp.process_query(p, gpps[c], q, gdb) for c, _, q in qs]
    taken = sp.paths_taken()
    _same(got, want)
    assert case.clients[0][0].decode_response(got[0])[:256] == edited[5 * 256:6 * 256].tobytes()
    assert "sweep_narrow" in taken, taken
    return taken


@_named("writer-update-rows-packed-planar")
def _update_rows_packed(sp, oracle_mod, S, arm):
    """an /update-row body on a PACKED database whose digit-planar copy stands: the copy is patched, not dropped; a single query reads
    the PACKED words, a list of 9 the copy"""
    case, blob = _blob_case(oracle_mod, PACKED, 13)
    rng = np.random.default_rng(14)
    npr = case.o.num_per
    records = [(0, rng.integers(0, 256, 256, dtype=np.uint8).tobytes()), (63 * npr + 127, rng.integers(0, 256, 255, dtype=np.uint8).tobytes()),
               (5 + 37, rng.integers(0, 256, 3, dtype=np.uint8).tobytes())]
    edited = blob.copy()
    for i, d in records:
        edited[i * 256:(i + 1) * 256] = 0
        edited[i * 256:i * 256 + len(d)] = np.frombuffer(d, dtype=np.uint8)
    qs = case.queries(9)            # (query 1 asks for item 42, an edited one)
    want = case.want(qs, case.o.load_db_from_bytes(edited.tobytes()), tag="edited")
    arm()
    p = S.params(PACKED)
    gpps, gdb = S.pps(p, case), S.db(p).load_items(blob)
    assert gdb.prepare_batch() is True
    copy = gdb.batch_copy_bytes()
    assert gdb.update_rows(_body(records)) == (3, 4 + 256)
    assert gdb.batch_copy_bytes() == copy > 0
    sp.paths_taken()
    one = sp.process_query(p, gpps[qs[1][0]], qs[1][2], gdb)
    taken = sp.paths_taken()
    got, taken_list = _ask(sp, p, gpps, qs, gdb)
    taken |= taken_list
    _same([one] + got, [want[1]] + want)
    assert {"sweep_batch_planar", "sweep_packed_persist"} <= taken, taken
    return taken


@_named("writer-update-rows-sparse")
def _update_rows_sparse(sp, oracle_mod, S, arm):
    case = _sparse_case(oracle_mod)
    arm()
    p = S.params(case.cfg)
    gpps, gdb = S.pps(p, case), case.bucket(S, p)
    sp.paths_taken()
    assert sp.process_query(p, gpps[0], case.qs[0][2], gdb) == case.want[0]       # an index snapshot exists before the body
    assert gdb.update_rows(_body(case.records)) == (3, 4 + 256)
    assert gdb.sparse_items() == 152
    got = [sp.process_query(p, gpps[c], q, gdb) for c, _, q in case.qs_after]
    taken = sp.paths_taken()
    _same(got, case.want_after)
    assert "sweep_sparse" in taken, taken
    return taken


# ---- flows: shards ----------------------------------------------------------------------------------------------------------------
def _row_sharded(name, cfg, G, batched=0):
    @_named(name)
    def flow(sp, oracle_mod, S, arm):
        """the whole sharded answer path inside the library, G ranks as host threads over the loopback transport; `batched`: that many
        queries through the batched list call (one pass over a rank's shard for the group, k_sweep_mfma_scatter)"""
        from sdk_amd.sharding import LoopbackWorld
        case = _case(oracle_mod, cfg)
        qs = case.queries(batched or 2)
        want = case.want(qs)
        arm()
        p = S.params(cfg)
        gpps = S.pps(p, case)
        shards = [S.db(p, s, G).load(case.words) for s in range(G)]
        world = LoopbackWorld(G)
        for r in range(G):
            S.own(world.comm(r))

        def rank_main(r):
            sp.lib().sp_set_device(0)
            sp.paths_taken()
            if batched:
                out = world.comm(r).process_queries_batched(p, [gpps[c] for c, _, _ in qs], [q for _, _, q in qs], shards[r])
            else:
                out = [world.comm(r).process_query(p, gpps[c], q, shards[r]) for c, _, q in qs]
            return out, sp.paths_taken()
        res = world.run(rank_main)
        _same(res[0][0], want)
        taken = set()
        for r in range(G):
            assert {"scatter_out", "custom_transport", "expand_pruned"} <= res[r][1], res[r][1]
            assert ("sweep_batch_scatter" in res[r][1]) == bool(batched), res[r][1]
            taken |= res[r][1]
        return taken
    return flow


@_named("column-shards-G2")
def _column_shards(sp, oracle_mod, S, arm):
    import torch
    from sdk_amd.sharding import local_cts_tensor
    cfg, G = dict(FAST56, nu_2=4), 2
    case = _case(oracle_mod, cfg)
    qs = case.queries(1)
    want = case.want(qs)
    arm()
    p = S.params(cfg)
    gpps = S.pps(p, case)
    shards = [S.db(p, g, G, by_columns=True).load(case.words) for g in range(G)]
    sp.paths_taken()
    runs = [S.run(p, gpps[0], qs[0][2]).sweep(shards[g]) for g in range(G)]
    locals_ = []
    for r in runs:
        r.fold_local(r.partial_ptr(), G)
        r.sync()
        locals_.append(local_cts_tensor(r).clone())
    gathered = torch.cat(locals_).contiguous()
    torch.cuda.synchronize()
    got = runs[0].finish_gathered(gathered.data_ptr(), G)
    taken = sp.paths_taken()
    del gathered, locals_
    assert got == want[0]
    assert "sweep_narrow" in taken, taken
    return taken


SHARD_FLOWS = [
    _row_sharded("row-shards-G2", dict(FAST56, nu_2=4), 2),
    _row_sharded("row-shards-G4-packed", PACKED, 4),
    _row_sharded("row-shards-G2-group-pass-5", PACKED, 2, batched=5),
    _column_shards,
]


# ---- flow: the stage exports, in one case ---------------------------------------------------------------------------------------
def _limbs(rng, n):
    return rng.integers(0, Q0, n, dtype=np.uint64) | (rng.integers(0, Q1, n, dtype=np.uint64) << np.uint64(32))


def _ntt_polys(rng, n):
    out = np.zeros((n, 2, N), dtype=np.uint64)
    out[:, 0] = rng.integers(0, Q0, (n, N), dtype=np.uint64)
    out[:, 1] = rng.integers(0, Q1, (n, N), dtype=np.uint64)
    out[0, 0], out[0, 1] = Q0 - 1, Q1 - 1
    return out.reshape(-1)


def _export_refs(oracle_mod):
    """inputs and the oracle's outputs of every stage export, computed once"""
    if "exports" in _SMALL:
        return _SMALL["exports"]
    cfg = dict(FAST56, nu_2=4)
    case = _case(oracle_mod, cfg)
    o, (cl, pp), (_, _, q) = case.o, case.clients[0], case.queries(1)[0]
    rng = np.random.default_rng(7)
    R = {"cfg": cfg, "pp": pp, "o": o}
    x = _ntt_polys(rng, 5)
    R["ntt"] = (x, o.ntt_forward(x), o.ntt_inverse(x))
    raw = rng.integers(0, Q, 6 * N, dtype=np.uint64)
    raw[:N], raw[N:2 * N], raw[2 * N] = 0, Q, (1 << 64) - 1
    ntt = o.to_ntt(raw)
    R["to_ntt"] = (raw, ntt, o.from_ntt(ntt))
    a, b = _ntt_polys(rng, 2 * 16), _ntt_polys(rng, 16 * 3)
    R["multiply"] = (a, b, o.multiply(a, 2, 16, b, 3))
    am = rng.integers(0, Q, 3 * N, dtype=np.uint64)
    R["automorph"] = (am, {t: o.automorph(am, t) for t in (2049, 5)})
    gi = rng.integers(0, Q, 2 * N, dtype=np.uint64)
    gi[5] = Q
    R["gadget"] = (gi, {ro: o.gadget_invert_rdim(gi, 2, 1, ro, rd) for ro, rd in ((16, 2), (56, 1))})
    v = _ntt_polys(rng, o.dim0 * 2)
    R["reorient"] = (v, o.reorient_reg_ciphertexts(v))
    R["sweep"] = {}
    for dim0, num_per in ((64, 4), (300, 128), (5, 128)):        # narrow, PACKED, k_sweep_wide
        db, qv = _limbs(rng, N * num_per * dim0), _limbs(rng, N * dim0 * 2)
        db[:num_per * dim0], qv[:dim0 * 2] = np.uint64(TOP), np.uint64(TOP)
        R["sweep"][(dim0, num_per)] = (db, qv, o.multiply_reg_by_database(db, qv, dim0, num_per))
    g, sr, mb = o.g, o.stop_round, o.t_gsw * o.db_dim_2
    v0 = np.zeros((1 << g) * 2 * o.ntt_words, dtype=np.uint64)
    v0[:2 * o.ntt_words] = o.to_ntt(o.query_deserialize_ct(q))
    v_cpu = o.coefficient_expansion(pp, v0, g, sr, mb)
    R["expansion"] = (v0, g, sr, mb, v_cpu)
    w = 2 * o.ntt_words
    gsw_inp = np.concatenate([v_cpu[(2 * i + 1) * w:(2 * i + 2) * w] for i in range(mb)])
    flat = o.pp_deserialize_flat(pp)
    R["gsw"] = (gsw_inp, o.regev_to_gsw(gsw_inp, flat[-2 * 2 * o.t_conv * o.ntt_words:], o.db_dim_2))
    v_reg, v_fold = o.expand_query(pp, q)
    v_neg = o.get_v_folding_neg(v_fold)
    sw = o.dim0 * o.num_per * N
    cts = []
    for trial in range(4):
        raw_ct = o.from_ntt(o.multiply_reg_by_database(case.words[trial * sw:(trial + 1) * sw], v_reg))
        cts.append((raw_ct, o.fold_ciphertexts(raw_ct, v_fold, v_neg)[:2 * N]))
    R["fold"] = (v_fold, v_neg, cts)
    v_ct = np.concatenate([f for _, f in cts])
    packed = o.pack(v_ct, flat[:o.n * (o.n + 1) * o.t_conv * o.ntt_words])
    praw = o.from_ntt(packed)
    R["pack"] = (v_ct, packed, praw, o.encode(praw))
    _SMALL["exports"] = R
    return R


@_named("stage-exports")
def _stage_exports(sp, oracle_mod, S, arm):
    import sdk_amd.spiral as L
    R = _export_refs(oracle_mod)
    arm()
    p = S.params(R["cfg"])
    gpp = S.own(sp.PublicParameters.deserialize(p, R["pp"]))
    sp.paths_taken()
    x, fwd, inv = R["ntt"]
    assert (L.ntt_forward(p, x) == fwd).all() and (L.ntt_inverse(p, x) == inv).all()
    raw, ntt, back = R["to_ntt"]
    assert (L.to_ntt(p, raw) == ntt).all() and (L.from_ntt(p, ntt) == back).all()
    a, b, ab = R["multiply"]
    assert (L.multiply(p, a, 2, 16, b, 3) == ab).all()
    am, autos = R["automorph"]
    for t, want in autos.items():
        assert (L.automorph(p, am, t) == want).all(), t
    gi, gadgets = R["gadget"]
    for (ro, rd) in ((16, 2), (56, 1)):
        assert (L.gadget_invert_rdim(p, gi, 2, 1, ro, rd) == gadgets[ro]).all(), ro
    v, reo = R["reorient"]
    assert (L.reorient_reg_ciphertexts(p, v) == reo).all()
    taken = sp.paths_taken()
    for (dim0, num_per), (db, qv, want) in R["sweep"].items():
        assert (L.multiply_reg_by_database(p, db, qv, dim0, num_per) == want).all(), (dim0, num_per)
        t = sp.paths_taken()
        assert {(64, 4): "sweep_narrow", (300, 128): "sweep_packed_persist", (5, 128): "sweep_wide"}[(dim0, num_per)] in t, t
        taken |= t
    v0, g, sr, mb, v_cpu = R["expansion"]
    assert (L.coefficient_expansion(p, gpp, v0, g, sr, mb) == v_cpu).all()
    gsw_inp, gsw = R["gsw"]
    assert (L.regev_to_gsw(p, gpp, gsw_inp, R["o"].db_dim_2) == gsw).all()
    v_fold, v_neg, cts = R["fold"]
    taken |= sp.paths_taken()
    for variant in (0, 3, 5):
        with env_switch("fold_variant", variant):
            for raw_ct, folded in cts[:2] if variant else cts:
                assert (L.fold_ciphertexts(p, raw_ct, v_fold, v_neg)[:2 * N] == folded).all(), variant
            t = sp.paths_taken()
            assert "fold_tail_literal" in t and "fold_fused" not in t, t
            assert (L.fold_ciphertexts_fused(p, cts[0][0], v_fold, fused_min_pairs=1)[:2 * N] == cts[0][1]).all(), variant
            t2 = sp.paths_taken()
            assert "fold_fused" in t2 and ("fold_wave" in t2) == (variant == 5), (variant, t2)
            taken |= t | t2
    assert (L.fold_ciphertexts_fused(p, cts[1][0], v_fold, fused_min_pairs=4)[:2 * N] == cts[1][1]).all()     # fused levels, then the delta tail
    v_ct, packed, praw, resp = R["pack"]
    assert (L.pack(p, gpp, v_ct) == packed).all()
    assert L.encode(p, praw) == resp
    return taken | sp.paths_taken()


# ---- flow: the request layer ----------------------------------------------------------------------------------------------------
@_named("request-layer-private-read")
def _private_read(sp, oracle_mod, S, arm):
    case = _case(oracle_mod, FAST56)
    qs = case.queries(5)
    want = case.want(qs)
    arm()
    p = S.params(FAST56)
    gdb = S.db(p).load(case.words)
    srv = S.own(sp.Server(p, gdb))
    uuids = [srv.setup(pp) for _, pp in case.clients]
    body = json.dumps([base64.b64encode(uuids[c].encode() + q).decode() for c, _, q in qs])
    sp.paths_taken()
    out = json.loads(srv.private_read_json(body))
    taken = sp.paths_taken()
    _same([base64.b64decode(x) for x in out], want)
    assert "sweep_narrow" in taken, taken
    return taken


# (neighbours share a cached database: FAST56, then the 64 x 128 shape, then the rest)
FLOWS = ([SINGLE_FLOWS[0], LIST_FLOWS[0], LIST_FLOWS[1], _private_read] + SINGLE_FLOWS[1:3] +
         [SINGLE_FLOWS[3], _single_unpacked] + LIST_FLOWS[2:6] + [SHARD_FLOWS[1], SHARD_FLOWS[2], _update_rows_packed] +
         [SINGLE_FLOWS[4], LIST_FLOWS[6]] + SINGLE_FLOWS[5:] + [_sparse_lists, _update_rows_sparse, _load_items_windows, _update_item,
                                                                SHARD_FLOWS[0], _column_shards, _stage_exports])
SECOND_FILL = {f.__name__ for f in SINGLE_FLOWS} | {"single-db-unpacked", "list16-packed-planar"}
CASES = []
for _f in FLOWS:
    CASES.append(pytest.param(_f, "poison", POISON, id=_f.__name__ + "-poison-a5"))
    if _f.__name__ in SECOND_FILL:
        CASES.append(pytest.param(_f, "poison", 0xFF, id=_f.__name__ + "-poison-ff"))
    CASES.append(pytest.param(_f, "guard", 0, id=_f.__name__ + "-guard"))
assert len({f.__name__ for f in FLOWS}) == len(FLOWS) == 27


@pytest.mark.parametrize("flow,mode,fill", CASES)
def test_flow_on_hardened_buffers(oracle_mod, capfd, flow, mode, fill):
    _hardened(flow, mode, fill, oracle_mod, capfd, record=True)


# ---- the instruments work ---------------------------------------------------------------------------------------------------------
def _emulated(sp):
    return hasattr(sp.lib(), "sp_emulated_device_marker")     # the CPU suite's emulated device: device memory is host memory


@_named("instrument-poison")
def _fresh_partial_buffer(sp, oracle_mod, S, arm):
    case = _case(oracle_mod, FAST56)
    q = case.queries(1)[0][2]
    arm()
    p = S.params(FAST56)
    run = S.run(p, S.pps(p, case)[0], q)
    run.sync()
    n = run.partial_words()
    if _emulated(sp):
        words = np.ctypeslib.as_array(C.cast(run.partial_ptr(), C.POINTER(C.c_uint32)), shape=(n,)).copy()
    else:
        from sdk_amd.sharding import partial_tensor
        words = partial_tensor(run).cpu().numpy().view(np.uint32).copy()
    assert n == 4 * 4 * N * 8 and (words == 0xA5A5A5A5).all(), "poison_ws does not reach a fresh workspace: %08x" % int(words[0])
    return set()


def test_poison_reaches_a_fresh_partial_buffer(oracle_mod, capfd):
    """a freshly begun QueryRun's partial buffer reads 0xA5A5A5A5 in every word before any sweep: without this a green poisoned run
    could mean that the switch never reached the allocator"""
    _hardened(_fresh_partial_buffer, "poison", POISON, oracle_mod, capfd)


def test_guard_reports_a_write_before_the_partial_buffer(oracle_mod, capfd):
    """one byte written at partial_ptr() - 1 -- the last byte of the front guard, inside the library's own allocation: a legal write,
    no fault -- must be reported when the workspace is released.  (sp_query_partial_ptr returns Workspace::sweep_out.p, the base of
    a DevBuf of its own: Workspace::ensure_sweep, sdk_amd/csrc/server.cpp.)"""
    @_named("instrument-guard")
    def flow(sp, oracle_mod, S, arm):
        case = _case(oracle_mod, FAST56)
        q = case.queries(1)[0][2]
        guard = arm()
        p = S.params(FAST56)
        run = S.run(p, S.pps(p, case)[0], q)
        run.sync()
        if guard <= 0:
            pass       # (no guard region, no write: the byte before the buffer would be somebody else's)
        elif _emulated(sp):
            C.memset(run.partial_ptr() - 1, 0x5A, 1)
        else:
            import torch
            from sdk_amd.sharding import _DevArray
            byte = _DevArray(run.partial_ptr() - 1, 1)
            byte.__cuda_array_interface__["typestr"] = "|u1"
            torch.as_tensor(byte, device="cuda").fill_(0x5A)
            torch.cuda.synchronize()
        return set()
    with pytest.raises(AssertionError, match="OUT-OF-BOUNDS WRITE around alloc .* reaches 1 bytes before / -1 bytes after"):
        _hardened(flow, "guard", 0, oracle_mod, capfd)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
def test_poisoned_cases_cover_every_path():
    """the union of the path names the poisoned cases took holds every name sp_path_name returns, except the retired bits and the
    library's own RCCL collectives (a 1-GPU suite cannot host two ranks): a path bit added later without a poisoned case fails here"""
    import sdk_amd as sp
    if len(set(_POISONED_CASES)) < len(FLOWS):
        pytest.skip("%d of the %d flows ran poisoned in this session" % (len(set(_POISONED_CASES)), len(FLOWS)))
    sp.lib().sp_path_name.restype = C.c_char_p
    names, bit = [], 0
    while sp.lib().sp_path_name(C.c_int(bit)) is not None:
        names.append(sp.lib().sp_path_name(C.c_int(bit)).decode())
        bit += 1
    assert len(names) >= 37
    live = {nm for b, nm in enumerate(names) if b not in RETIRED_BITS and nm != "rccl_in_library"}
    assert sorted(live - _POISONED_PATHS) == []
