"""Row shards of a sparse bucket (sp_db_create_sparse_shard) in the multi-GPU flows: the scatter-form sweeps (k_sweep_sparse_scatter,
k_sweep_sparse_scatter_batch) and every entry point that takes such a shard.  The yardstick is never the code under test: partial
buffers are compared word for word with k_sweep_sparse's output on an UNSHARDED bucket that holds the shard's items, re-indexed by
sharding.scatter_layout_index / scatter_plane_layout_index; responses byte for byte with oracle.SparseDb.process_query over the WHOLE
bucket.  tests/test_emulated_sparse_shards.py runs subsets of this file on the emulated device."""
import ctypes as C
import functools
import struct
import threading

import numpy as np
import pytest

from conftest import FAST
from test_gpu_sharded_batch import _partial
from test_gpu_sparse_batch import Bucket, _random_item, batch_min

pytestmark = pytest.mark.gpu

N = 2048
GROUP, SPARSE, SCATTER = "sparse_group_pass", "sweep_sparse", "scatter_out"


def _cfg(nu_1, nu_2, **kw):
    return dict(FAST, nu_1=nu_1, nu_2=nu_2, db_item_size=256, **kw)


def _emulated(sp):
    return hasattr(sp.lib(), "sp_emulated_device_marker")     # the CPU suite's emulated device: device memory is host memory


def _to_device(sp, arr):
    """a host array as a device buffer -> (owner to keep alive, device pointer)"""
    arr = np.ascontiguousarray(arr)
    if _emulated(sp):
        return arr, arr.ctypes.data
    import torch
    t = torch.from_numpy(arr.view(np.int32 if arr.dtype == np.uint32 else np.int64)).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def _local_cts(sp, run):
    """host copy of a run's locally folded ciphertexts [plane][2][N] (uint64)"""
    run.sync()
    n = run.local_cts_words()
    if _emulated(sp):
        return np.ctypeslib.as_array(C.cast(run.local_cts_ptr(), C.POINTER(C.c_uint64)), shape=(n,)).copy()
    from sdk_amd.sharding import local_cts_tensor
    return local_cts_tensor(run).cpu().numpy().view(np.uint64).copy()


def _body(pairs):
    """an /update-row body: be32 chunk_len | be32 item index | item bytes per record"""
    return b"".join(struct.pack(">II", 4 + len(d), i) + bytes(d) for i, d in pairs)


class Sharded(Bucket):
    """Bucket with its GPU side as G row shards: every write is handed to every shard (each keeps the items of its rows), the oracle's
    SparseDb holds the whole bucket"""

    def __init__(self, oracle_mod, cfg, G, n_clients=2):
        super().__init__(oracle_mod, cfg, n_clients)
        self.G, self.planes = G, cfg.get("instances", 1) * cfg["n"] ** 2
        self.shards = [self.sp.Database.sparse(self.p, s, G) for s in range(G)]

    def shard_of(self, idx):
        return (idx // self.num_per) // (self.dim0 // self.G)

    def put(self, idx, data):
        for sh in self.shards:
            sh.update_item(idx, data)
        self.sdb.update_item_raw(idx, data)
        self.items[idx] = bytes(data)

    def put_many(self, pairs):
        for sh in self.shards:
            sh.update_items(pairs)
        for idx, data in pairs:
            self.sdb.update_item_raw(idx, data)
            self.items[idx] = bytes(data)

    def run(self, s, query):
        c, _, q = query
        return self.sp.QueryRun(self.p, self.clients[c][2], q, db=self.shards[s])

    def reference(self, s, qs):
        """k_sweep_sparse on an UNSHARDED bucket that holds only shard s's items: the plain partial buffer of every query"""
        sp = self.sp
        ref = sp.Database.sparse(self.p)
        own = [(i, d) for i, d in self.items.items() if self.shard_of(i) == s]
        ref.update_items(own)
        assert ref.sparse_items() == len(own)
        out = []
        for c, _, q in qs:
            run = sp.QueryRun(self.p, self.clients[c][2], q, db=ref).sweep(ref)
            out.append(_partial(sp, run))
            run.free()
        return out


@functools.lru_cache(maxsize=None)
def _layouts(num_per, planes, G):
    """flat positions of the plain buffer's words [plane][r][crt][z][ii] in the chunk-major and in the per-plane scatter layout"""
    from sdk_amd.sharding import scatter_layout_index, scatter_plane_layout_index
    pl, r, crt, z, ii = (a.ravel() for a in np.indices((planes, 2, 2, N, num_per)))
    chunk_major = scatter_layout_index(num_per, planes, G, pl, r, crt, z, ii)
    per_plane = scatter_plane_layout_index(num_per, G, pl, r, crt, z, ii)
    for idx in (chunk_major, per_plane):      # both are permutations of the buffer
        assert np.array_equal(np.sort(idx), np.arange(idx.size))
    return chunk_major, per_plane


def _expected(plain, num_per, planes, G):
    chunk_major, per_plane = _layouts(num_per, planes, G)
    a, b = np.empty_like(plain), np.empty_like(plain)
    a[chunk_major] = plain
    b[per_plane] = plain
    return a, b


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got, want), (what, int((got != want).sum()))


# ---- 1. a shard keeps its rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4, 8])
def test_shard_keeps_its_rows(oracle_mod, G):
    import sdk_amd as sp
    cfg = _cfg(6, 3)
    p = sp.Params(cfg)
    num_per, dim0 = 8, 64
    shards = [sp.Database.sparse(p, s, G) for s in range(G)]
    rng = np.random.default_rng(100 + G)
    idxs = [int(i) for i in rng.choice(dim0 * num_per, 150, replace=False)]
    pairs = [(i, _random_item(rng, 256)) for i in idxs]
    for sh in shards:
        for i, d in pairs[:50]:
            sh.update_item(i, d)
        sh.update_items(pairs[50:100])
        assert sh.update_rows(_body(pairs[100:]))[0] == 50      # records a shard skips count as applied
    held = [sum(1 for i in idxs if (i // num_per) // (dim0 // G) == s) for s in range(G)]
    assert sum(held) == 150
    assert [sh.sparse_items() for sh in shards] == held
    for s, sh in enumerate(shards):
        assert sh.format() == "sparse"
        bad = dim0 * num_per
        with pytest.raises(sp.SpiralError):
            sh.update_item(bad, b"x")
        with pytest.raises(sp.SpiralError):
            sh.update_items([(idxs[0], b"x"), (bad, b"x")])
        with pytest.raises(sp.SpiralError):
            sh.update_rows(_body([(bad, b"x")]))
        assert sh.sparse_items() == held[s]
    for args in ((G, G), (-1, G), (0, 3), (0, 16)):      # bad shard, dim0 % 3 != 0, more than SP_MAX_ROW_SHARDS
        with pytest.raises(sp.SpiralError):
            sp.Database.sparse(p, *args)


# ---- 2. scatter sweeps leave the reference words ------------------------------------------------------------------------------
def _fill_small(b, shape):
    """the buckets of the small shapes: an empty shard, an empty column beside full ones, a residue class of columns (ii % G) that is
    empty on every shard"""
    rng = np.random.default_rng(len(shape) + b.G)
    nj = b.dim0 // b.G
    empty_shard, empty_class, empty_col = {"nu6-G2": (1, 1, 2), "nu6-G4": (2, 3, 1), "nu6-G8": (5, 6, 1), "nu8-G2-8planes": (None, None, 3)}[shape]
    rows = [j for j in range(b.dim0) if j // nj != empty_shard]
    pairs = []
    for ii in range(b.num_per):
        if ii == empty_col or (empty_class is not None and ii % b.G == empty_class):
            continue
        col_rows = rows if ii == 0 else [int(j) for j in rng.choice(rows, 9 + ii, replace=False)]      # column 0 is full
        pairs += [(j * b.num_per + ii, _random_item(rng, b.size)) for j in col_rows]
    b.put_many(pairs)
    held = [sh.sparse_items() for sh in b.shards]
    assert sum(held) == len(pairs) and all((n == 0) == (s == empty_shard) for s, n in enumerate(held)), held


SMALL = {"nu6-G2": (_cfg(6, 3), 2), "nu6-G4": (_cfg(6, 3), 4), "nu6-G8": (_cfg(6, 3), 8), "nu8-G2-8planes": (_cfg(8, 3, instances=2), 2)}
_small_cache = {}


@pytest.fixture
def small(request, oracle_mod):
    """(bucket, eight queries of two clients, per shard the reference partial buffers): built once per shape and never changed"""
    shape = request.param
    if shape not in _small_cache:
        cfg, G = SMALL[shape]
        b = Sharded(oracle_mod, cfg, G)
        _fill_small(b, shape)
        present = list(b.items)
        absent = next(i for i in range(b.dim0 * b.num_per) if i not in b.items)
        qs = b.queries([present[0], absent] + present[1:7], 900)
        _small_cache[shape] = (b, qs, [b.reference(s, qs) for s in range(G)])
    return _small_cache[shape]


@pytest.mark.parametrize("small", list(SMALL), indirect=True)
def test_single_query_sweeps_leave_the_reference_words(small):
    """on every shard: sweep == the reference, sweep_scatter and the chain of sweep_scatter_plane == the reference re-indexed"""
    b, qs, refs = small
    sp = b.sp
    for s in range(b.G):
        for k in (0, 1):      # one query of each client
            chunk_major, per_plane = _expected(refs[s][k], b.num_per, b.planes, b.G)
            sp.paths_taken()
            run = b.run(s, qs[k]).sweep(b.shards[s])
            _same(_partial(sp, run), refs[s][k], ("sweep", s, k))
            run.free()
            taken = sp.paths_taken()
            assert SPARSE in taken and SCATTER not in taken and GROUP not in taken, taken
            run = b.run(s, qs[k]).sweep_scatter(b.shards[s], b.G)
            _same(_partial(sp, run), chunk_major, ("sweep_scatter", s, k))
            run.free()
            run = b.run(s, qs[k])
            for pl in range(b.planes):
                run.sweep_scatter_plane(b.shards[s], b.G, pl)
            _same(_partial(sp, run), per_plane, ("sweep_scatter_plane", s, k))
            run.free()
            taken = sp.paths_taken()
            assert {SPARSE, SCATTER} <= taken and GROUP not in taken, taken
            assert not any(t.startswith("sweep_batch") for t in taken), taken


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("small", list(SMALL), indirect=True)
def test_group_sweep_leaves_the_reference_words(small, B):
    """sweep_scatter_group of B queries of two clients on every shard: every member's buffer == its reference re-indexed; B = 1 is
    the single-query kernel, 2 the B = 2 body, 3 and 5 the B = 4 and 8 bodies with dead slots, 8 the full B = 8 body"""
    b, qs, refs = small
    sp = b.sp
    for s in range(b.G):
        runs = [b.run(s, q) for q in qs[:B]]
        sp.paths_taken()
        sp.QueryRun.sweep_scatter_group(runs, b.shards[s], b.G)
        got = [_partial(sp, r) for r in runs]
        taken = sp.paths_taken()
        assert {SPARSE, SCATTER} <= taken and (GROUP in taken) == (B >= 2), taken
        assert not any(t.startswith("sweep_batch") for t in taken), taken
        for k in range(B):
            _same(got[k], _expected(refs[s][k], b.num_per, b.planes, b.G)[1], ("group", s, B, k))
        with pytest.raises(sp.SpiralError):
            sp.QueryRun.sweep_scatter_group(runs, b.shards[s], b.G)      # already swept
        for r in runs:
            r.free()


def test_accumulator_range(oracle_mod):
    """nu = (10, 3), shard 1 of 2 (512 rows): columns of 255, 256, 257, 512, 1 and 0 items of that shard -- one item either side of the
    Barrett fold after 255 items, and two folds -- through every kernel body; the other shard's items are handed over and skipped"""
    b = Sharded(oracle_mod, _cfg(10, 3), 2)
    sp, rng, s = b.sp, np.random.default_rng(77), 1
    lens = (255, 256, 257, 512, 1, 0, 300, 3)
    pairs = []
    for ii, n in enumerate(lens):
        pairs += [(int(j) * b.num_per + ii, _random_item(rng, b.size)) for j in 512 + np.sort(rng.choice(512, n, replace=False))]
    theirs = [(int(i), _random_item(rng, b.size)) for i in rng.choice(512 * b.num_per, 40, replace=False)]      # shard 0's rows
    for i, d in pairs:
        b.items[i] = d
    both = pairs + theirs
    order = rng.permutation(len(both))
    b.shards[s].update_items([both[k] for k in order])
    assert b.shards[s].sparse_items() == sum(lens)
    present = [pairs[0][0], pairs[254][0], pairs[255][0], pairs[255 + 256][0], pairs[-1][0], 5, pairs[600][0], pairs[900][0]]
    qs = b.queries(present, 950)
    refs = b.reference(s, qs)
    shard = b.shards[s]
    chunk_major, per_plane = _expected(refs[0], b.num_per, b.planes, 2)
    run = b.run(s, qs[0]).sweep(shard)
    _same(_partial(sp, run), refs[0], "sweep")
    run.free()
    run = b.run(s, qs[0]).sweep_scatter(shard, 2)
    _same(_partial(sp, run), chunk_major, "sweep_scatter")
    run.free()
    run = b.run(s, qs[0])
    for pl in range(b.planes):
        run.sweep_scatter_plane(shard, 2, pl)
    _same(_partial(sp, run), per_plane, "sweep_scatter_plane")
    run.free()
    for B in (2, 3, 8):
        runs = [b.run(s, q) for q in qs[:B]]
        sp.QueryRun.sweep_scatter_group(runs, shard, 2)
        for k, r in enumerate(runs):
            _same(_partial(sp, r), _expected(refs[k], b.num_per, b.planes, 2)[1], ("group", B, k))
            r.free()


# ---- 3. the flow by hand equals the oracle ------------------------------------------------------------------------------------
def _fold_and_finish(b, runs, reduced, per_plane):
    """runs[g] = rank g's swept query, reduced[g] = its summed chunk [plane][r][crt][z][ii / G] (uint32) -> the response of rank 0"""
    sp, G = b.sp, b.G
    keep, local = [], []
    chunk_pl = reduced[0].size // b.planes
    for g in range(G):
        if per_plane:
            for pl in range(b.planes):
                owner, ptr = _to_device(sp, reduced[g][pl * chunk_pl:(pl + 1) * chunk_pl])
                keep.append(owner)
                runs[g].fold_local_plane(ptr, G, pl)
            runs[g].fold_local_join()
        else:
            owner, ptr = _to_device(sp, reduced[g])
            keep.append(owner)
            runs[g].fold_local(ptr, G)
        local.append(_local_cts(sp, runs[g]))
    owner, ptr = _to_device(sp, np.concatenate(local))      # [g][plane][2][N]
    resp = runs[0].finish_gathered(ptr, G)
    for r in runs:
        r.sync()
    del keep, owner
    return resp


def _by_hand(b, query, per_plane):
    """per shard begin_for_db + scatter sweep, the test's own u32 sum of chunk g over the shards, fold_local on rank g's query, the
    local results gathered as [g][plane][2][N], finish_gathered on rank 0's query"""
    sp, G = b.sp, b.G
    runs = [b.run(s, query) for s in range(G)]
    parts = []
    for s, run in enumerate(runs):
        if per_plane:
            for pl in range(b.planes):
                run.sweep_scatter_plane(b.shards[s], G, pl)
        else:
            run.sweep_scatter(b.shards[s], G)
        parts.append(_partial(sp, run))
    reduced = _reduce(b, parts, per_plane)
    resp = _fold_and_finish(b, runs, reduced, per_plane)
    for r in runs:
        r.free()
    return resp


def _reduce(b, parts, per_plane):
    """the reduce-scatter: rank g's chunk [plane][r][crt][z][ii / G] summed over the shards' buffers as u32"""
    G = b.G
    total = np.zeros_like(parts[0])
    for part in parts:
        total += part      # uint32, as the exchange sums
    if per_plane:          # [plane][g][...]
        return [np.ascontiguousarray(total.reshape(b.planes, G, -1)[:, g, :]).ravel() for g in range(G)]
    return [total.reshape(G, -1)[g].copy() for g in range(G)]


def _fill_flow(b, kind):
    rng = np.random.default_rng(41)
    total = b.dim0 * b.num_per
    if kind == "random-150":
        idxs = [int(i) for i in rng.choice(total, 150, replace=False)]
    elif kind == "shard-0-only":
        idxs = [int(i) for i in rng.choice(b.dim0 // b.G * b.num_per, 60, replace=False)]
    elif kind == "class-1-empty":      # columns ii % G == 1 hold nothing: rank 1's local result is all zero and reaches the gathered levels
        idxs = [int(i) for i in rng.choice(total, 200, replace=False) if (i % b.num_per) % b.G != 1]
    else:
        idxs = []
    b.put_many([(i, _random_item(rng, b.size)) for i in idxs])
    assert sum(sh.sparse_items() for sh in b.shards) == len(idxs)


@pytest.mark.parametrize("kind", ["random-150", "shard-0-only", "class-1-empty", "empty"])
@pytest.mark.parametrize("G", [2, 4])
def test_flow_by_hand_equals_the_oracle(oracle_mod, G, kind):
    b = Sharded(oracle_mod, _cfg(6, 3), G)
    _fill_flow(b, kind)
    absent = next(i for i in range(b.dim0 * b.num_per) if i not in b.items and (kind != "class-1-empty" or (i % b.num_per) % G == 1))
    idxs = ([next(iter(b.items))] if b.items else [3]) + [absent]
    qs = b.queries(idxs, 1000)
    want = b.want(qs)
    for per_plane in (False, True):
        for query, w in zip(qs, want):
            got = _by_hand(b, query, per_plane)
            assert got == w, (per_plane, query[1])
            c, idx, _ = query
            if idx in b.items:
                assert b.clients[c][0].decode_response(got)[:b.size] == b.items[idx].ljust(b.size, b"\0")


# ---- 4. the library's flows over LoopbackWorld --------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [(6, 3), (6, 7)], ids=["nu6-3", "nu6-7"])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_flows_over_the_loopback_world(oracle_mod, G, nu):
    from sdk_amd.sharding import LoopbackWorld
    b = Sharded(oracle_mod, _cfg(*nu), G)
    sp = b.sp
    rng = np.random.default_rng(G + nu[1])
    b.put_many([(int(i), _random_item(rng, b.size)) for i in rng.choice(b.dim0 * b.num_per, 150 if nu[1] == 3 else 400, replace=False)])
    present = list(b.items)
    absent = next(i for i in range(b.dim0 * b.num_per) if i not in b.items)
    qs = b.queries([present[0], absent] + present[1:10], 1100)
    want = b.want(qs)
    pps, q_list = [b.clients[c][2] for c, _, _ in qs], [q for _, _, q in qs]
    world, gate, taken = LoopbackWorld(G), threading.Barrier(G, timeout=300), {}

    def measured(r, name, call):
        """call() twice (buffer reuse); the path bits of the two calls of all ranks together, read while no rank runs"""
        gate.wait()
        if r == 0:
            sp.paths_taken()
        gate.wait()
        out = (call(), call())
        gate.wait()
        if r == 0:
            taken[name] = sp.paths_taken()
        gate.wait()
        return out

    def rank_main(r):
        sp.lib().sp_set_device(0)
        comm, sh, res = world.comm(r), b.shards[r], {}
        res["one"] = measured(r, "one", lambda: comm.process_query(b.p, pps[0], q_list[0], sh))
        res["list"] = measured(r, "list", lambda: comm.process_queries(b.p, pps[:5], q_list[:5], sh))
        res["list-info"] = comm.describe()["last_list"]
        for group in (0, 4, 1):
            res[group] = measured(r, group, lambda: comm.process_queries_batched(b.p, pps, q_list, sh, group=group))
            res[group, "info"] = comm.describe()["last_list"]
        return res
    try:
        res = world.run(rank_main)
    except Exception:
        gate.abort()
        raise
    for r in range(G):
        assert res[r]["one"] == ((want[0], want[0]) if r == 0 else (b"", b"")), r
        assert res[r]["list"] == ((want[:5], want[:5]) if r == 0 else ([], [])), r
        assert res[r]["list-info"] == {"group": 1, "reduce_scatters": 5 * b.planes, "all_gathers": 5}
        for group, size in ((0, 8), (4, 4), (1, 1)):
            assert res[r][group] == ((want, want) if r == 0 else ([], [])), (r, group)
            assert res[r][group, "info"] == {"group": size, "reduce_scatters": 11 * b.planes, "all_gathers": 11}, res[r][group, "info"]
    for name, bits in taken.items():
        assert {SPARSE, SCATTER, "custom_transport", "expand_pruned"} <= bits and "rccl_in_library" not in bits, (name, bits)
        assert (GROUP in bits) == (name in (0, 4)), (name, bits)
        assert not any(t.startswith("sweep_batch") for t in bits), (name, bits)
    c, idx, _ = qs[0]
    assert b.clients[c][0].decode_response(want[0])[:b.size] == b.items[idx].ljust(b.size, b"\0")


# ---- 5. upserts between queries -----------------------------------------------------------------------------------------------
def test_upserts_between_queries(oracle_mod):
    G = 2
    b = Sharded(oracle_mod, _cfg(6, 3), G)
    sp, rng = b.sp, np.random.default_rng(59)
    b.put_many([(int(i), _random_item(rng, b.size)) for i in rng.choice(b.dim0 * b.num_per, 40, replace=False)])
    present = list(b.items)
    new = next(i for i in range(b.dim0 * b.num_per - 1, 0, -1) if i not in b.items)      # in the last shard's rows
    assert b.shard_of(new) == G - 1
    qs = b.queries([present[0], new], 1200)
    before = b.want(qs)
    assert [_by_hand(b, q, False) for q in qs] == before
    b.put(new, _random_item(rng, b.size))                              # a new key: part of the next query
    b.put(present[0], bytes(reversed(b.items[present[0]])))            # an overwrite
    assert sum(sh.sparse_items() for sh in b.shards) == 41
    after = b.want(qs)
    assert after[0] != before[0] and after[1] != before[1]
    got = [_by_hand(b, q, True) for q in qs]
    assert got == after
    for (c, idx, _), resp in zip(qs, got):
        assert b.clients[c][0].decode_response(resp)[:b.size] == b.items[idx].ljust(b.size, b"\0")
    # a group whose members were begun either side of an upsert (a new key): each member is answered on its own snapshot
    newer = next(i for i in range(b.dim0 * b.num_per) if i not in b.items)
    q_old, q_new = b.queries([newer, newer], 1300)
    want_old = b.want([q_old])[0]
    old_runs = [b.run(s, q_old) for s in range(G)]
    b.put(newer, _random_item(rng, b.size))
    want_new = b.want([q_new])[0]
    assert want_old != want_new
    new_runs = [b.run(s, q_new) for s in range(G)]
    parts_old, parts_new = [], []
    sp.paths_taken()
    for s in range(G):
        sp.QueryRun.sweep_scatter_group([old_runs[s], new_runs[s]], b.shards[s], G)
        parts_old.append(_partial(sp, old_runs[s]))
        parts_new.append(_partial(sp, new_runs[s]))
    taken = sp.paths_taken()
    assert b.shard_of(newer) == 0 and {SPARSE, SCATTER, GROUP} <= taken, taken      # shard 1's index did not change: one pass there
    assert _fold_and_finish(b, old_runs, _reduce(b, parts_old, True), False) == want_old
    assert _fold_and_finish(b, new_runs, _reduce(b, parts_new, True), False) == want_new
    c, idx, _ = q_new
    assert b.clients[c][0].decode_response(want_new)[:b.size] == b.items[newer].ljust(b.size, b"\0")
    for r in old_runs + new_runs:
        r.free()


# ---- 6. errors are status codes and enqueue nothing ---------------------------------------------------------------------------
@pytest.mark.parametrize("small", ["nu6-G2"], indirect=True)
def test_errors_enqueue_nothing(small, oracle_mod):
    b, qs, refs = small
    sp, G, s = b.sp, b.G, 0
    shard, other = b.shards[0], b.shards[1]
    c0, _, q0 = qs[0]
    gpp = b.clients[c0][2]
    # calls that need an unsharded database
    with pytest.raises(sp.SpiralError):
        sp.process_query(b.p, gpp, q0, shard)
    with pytest.raises(sp.SpiralError):
        sp.process_query_batch(b.p, [gpp, gpp], [q0, q0], shard)
    with pytest.raises(sp.SpiralError):
        srv = sp.Server(b.p, shard)
        uuid = srv.setup(b.clients[c0][1])
        srv.private_read([uuid.encode() + q0])
    runs = [b.run(s, q) for q in qs[:4]]
    for_other = b.run(1, qs[0])
    four = sp.Database.sparse(b.p, 0, 4)
    unsharded = sp.Database.sparse(b.p)
    for call in (lambda: for_other.sweep_scatter(shard, G),                          # begun for shard 1, swept over shard 0
                 lambda: for_other.sweep_scatter_plane(shard, G, 0),
                 lambda: for_other.sweep(shard),
                 lambda: sp.QueryRun.sweep_scatter_group([for_other], shard, G),
                 lambda: runs[0].sweep_scatter(shard, 4),                            # G unequal to num_shards
                 lambda: runs[0].sweep_scatter_plane(shard, 4, 0),
                 lambda: sp.QueryRun.sweep_scatter_group(runs, shard, 4),
                 lambda: sp.QueryRun.sweep_scatter_group(runs, four, 2),
                 lambda: sp.QueryRun.sweep_scatter_group(runs, unsharded, 2),
                 lambda: sp.QueryRun.sweep_scatter_group(runs, other, G),
                 lambda: sp.QueryRun.sweep_scatter_group(runs + runs + [runs[0]], shard, G),      # nine
                 lambda: sp.QueryRun.sweep_scatter_group([runs[0], runs[1], runs[0]], shard, G),  # the same member twice
                 lambda: sp.QueryRun.sweep_scatter_group([], shard, G)):
        with pytest.raises(sp.SpiralError):
            call()
    cfg2 = _cfg(6, 4)
    p2, o2 = sp.Params(cfg2), oracle_mod.Params(cfg2)
    cl2 = oracle_mod.Client(o2)
    alien = sp.QueryRun(p2, sp.PublicParameters.deserialize(p2, cl2.generate_keys(3)), cl2.generate_query(1, 4))
    with pytest.raises(sp.SpiralError):
        sp.QueryRun.sweep_scatter_group(runs[:3] + [alien], shard, G)               # a member of other params
    alien.free()
    with pytest.raises(sp.SpiralError):
        sp.Database.planar(b.p, 0, 2)                                               # planar-resident handles have no shards ...
    cfg3 = dict(FAST, nu_1=6, nu_2=7, db_item_size=256)
    p3, o3 = sp.Params(cfg3), oracle_mod.Params(cfg3)
    cl3 = oracle_mod.Client(o3)
    planar = sp.Database.planar(p3)
    run3 = sp.QueryRun(p3, sp.PublicParameters.deserialize(p3, cl3.generate_keys(5)), cl3.generate_query(1, 6))
    for call in (lambda: run3.sweep_scatter(planar, 1), lambda: run3.sweep_scatter_plane(planar, 1, 0),
                 lambda: sp.QueryRun.sweep_scatter_group([run3], planar, 1)):       # ... and stay refused by the scatter family
        with pytest.raises(sp.SpiralError, match="planar-resident"):
            call()
    run3.free()
    # the failed calls enqueued nothing and changed no state: the correct call leaves the words of case 2
    sp.QueryRun.sweep_scatter_group(runs, shard, G)
    for k, r in enumerate(runs):
        _same(_partial(sp, r), _expected(refs[s][k], b.num_per, b.planes, G)[1], ("after errors", k))
        r.free()
    for_other.sweep_scatter(other, G)
    _same(_partial(sp, for_other), _expected(refs[1][0], b.num_per, b.planes, G)[0], "after errors, shard 1")
    for_other.free()
    with batch_min(sp, 0):      # the switch at 0: every member sweeps alone inside the same entry point, the same words
        runs = [b.run(s, q) for q in qs[:3]]
        sp.paths_taken()
        sp.QueryRun.sweep_scatter_group(runs, shard, G)
        got = [_partial(sp, r) for r in runs]
        taken = sp.paths_taken()
    assert {SPARSE, SCATTER} <= taken and GROUP not in taken, taken
    for k, r in enumerate(runs):
        _same(got[k], _expected(refs[s][k], b.num_per, b.planes, G)[1], ("switch off", k))
        r.free()
