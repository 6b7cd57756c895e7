"""The reference's shipped parameter sets -- n = 3 and 4, p = 512, packing version 1: 9, 12 and 16 planes -- through every database
format and list flow (tests/param_matrix.py holds the sets, the pools and the helpers).  The plane count planes = instances * n * n is
a kernel dimension of all of them (zps = planes * N, grid.z = planes, n_items * planes grids, the per-plane exchange loops, the
per-plane digest pairs), and every other test of these features runs at 4 or 8 planes.

Every comparison is byte equality with the oracle on the same bytes: oracle.Params.process_query over load_db_from_bytes words,
oracle.SparseDb.process_query for buckets, the item file itself for read-back, tests/db_digest_reference.py for digests.  Every cell
asserts the path bits of the kernel it means to run.  Shapes are the smallest that reach each kernel:
  a  (6, 2)  8-byte narrow handle: one query, lists of 3 and 8 through the narrow group pass                         all four sets
  b  (6, 3)  sparse bucket, a third of the items from one /update-row body: queries, a list of 3, read_items, digest all four
  c  (6, 7)  PACKED with its digit-planar copy: lists, the edit body, lists again; resident == copy == numpy digest  all four
  d  (6, 7)  planar-resident: as c, plus read_ref at corners of every plane                                          all four
  e  (4, 7) / (6, 3), G = 2  PACKED row shards and sparse shards over the loopback world                             N3, V1
  f  (7, 7), G = 2  planar row shards: partial buffers against the PACKED shards', lists of 9 and 3, the edit body   N3
  g  (6, 7)  a sparse bucket's export_rows into a PACKED, a planar-resident and a sparse handle                      N3, S16
  h  (6, 7)  every response of a list on the planar handle decodes to its item                                       S16, V0
S16 on a sparse bucket (b, g): lib/server stores bytes (loading.rs:290 asserts log2 p = 8, and so does oracle/sparse_server.cpp), so
there is no SparseDb of a p = 512 bucket.  The buckets of b and g hold full records in every column, where lib/server's response is
spiral-rs's over the zero-filled file (tests/test_sparse_bucket.py::test_sparse_oracle_semantics): S16's bucket queries are compared
with oracle.Params.process_query over those words, and the p = 256 sets with both oracles, which must agree.
Nearly all of the module's time is the oracle's: the (6, 7) pools cost 6 to 18 oracle queries per set, computed once.
tests/test_emulated_param_matrix.py runs a subset on the emulated device."""
import threading

import numpy as np
import pytest

from db_digest_reference import N
from param_matrix import (BATCH_BITS, DIGEST_SEED, LISTS, POOL, assert_packed_list, assert_packed_single, assert_planar_list, body, cfg,
                          corners, dense, digest_reference, planes_of, sparse_records)
from test_gpu_narrow_batch import switch
from test_gpu_planar_shards import _assert_pass
from test_gpu_sharded_batch import _partial
from test_gpu_sparse_batch import Bucket, batch_min
from test_gpu_sparse_shards import Sharded

pytestmark = pytest.mark.gpu

ALL = ["N3", "V0", "V1", "S16"]
SPARSE_GROUP, SPARSE, SCATTER_OUT = "sparse_group_pass", "sweep_sparse", "scatter_out"


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _same_digest(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1, 2), np.asarray(want, dtype=np.uint64).reshape(-1, 2)
    assert got.shape == want.shape and (got == want).all(), (what, np.nonzero((got != want).any(axis=1))[0].tolist())


def _pack_bit(name, taken):
    assert ("pack_v1" in taken) == (name == "V1"), taken


# ---- a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_a_narrow_handle(sp, oracle_mod, name):
    c = dense(sp, oracle_mod, name, 6, 2, 8)
    st = c.before
    db = sp.Database(c.p).load_items(c.blob)
    assert db.format() == "words8" and db.device_bytes() == c.planes * N * c.npr * c.d0 * 8
    sp.paths_taken()
    got = sp.process_query(c.p, c.gpps[0], st.qs[0], db)
    taken = sp.paths_taken()
    assert "sweep_narrow" in taken and "sweep_narrow_group" not in taken and not BATCH_BITS & taken, taken
    _pack_bit(name, taken)
    assert got == st.want(0)
    for B in (3, 8):
        with switch(sp, "narrow_batch_min", 2):
            sp.paths_taken()
            got = c.batch(db, st, B)
            taken = sp.paths_taken()
        assert "sweep_narrow_group" in taken and "sweep_narrow" not in taken and not BATCH_BITS & taken, (B, taken)
        assert [g == st.want(i) for i, g in enumerate(got)] == [True] * B, B


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def _filled_bucket(b, shards=None):
    """a third of the items, an empty and a short record among them, as ONE /update-row body on the library's side"""
    recs, file = sparse_records(b.o)
    for i, d in recs:
        if b.o.pt_modulus == 256:      # lib/server stores bytes (loading.rs:290 asserts log2 p = 8): no SparseDb of an S16 bucket
            b.sdb.update_item_raw(i, d)
        b.items[i] = d
    for db in shards or [b.gdb]:
        assert db.update_rows(body(recs)) == (len(recs), 4 + b.size)      # (records a shard skips count as applied)
    absent = next(i for i in range(b.o.num_items) if i not in b.items)
    return recs, file, absent


@pytest.mark.parametrize("name", ALL)
def test_b_sparse_bucket(sp, oracle_mod, name):
    """S16: oracle.SparseDb restates lib/server, which stores bytes (p = 256 only).  With every column of the bucket populated no
    all-zero shortcut of lib/server's fold fires and its response is spiral-rs's over the zero-filled file
    (tests/test_sparse_bucket.py::test_sparse_oracle_semantics), so the p = 512 bucket is compared with oracle.Params.process_query
    over load_db_from_bytes words; the three other sets are compared with both, which pins that premise on these records"""
    b = Bucket(oracle_mod, cfg(name, 6, 3), n_clients=2)
    recs, file, absent = _filled_bucket(b)
    assert {i % b.num_per for i, d in recs if len(d) == b.size} == set(range(b.num_per))      # every column holds full records
    assert b.gdb.format() == "sparse" and b.gdb.sparse_items() == len(recs)
    back, present, undecodable = b.gdb.read_items(0, b.o.num_items)
    assert back == file.tobytes() and undecodable == 0
    assert np.nonzero(present)[0].tolist() == [i for i, _ in recs]
    words = b.o.load_db_from_bytes(file.tobytes())                    # absent items are zero polynomials on both sides
    _same_digest(b.gdb.digest(DIGEST_SEED), digest_reference(words, b.p.instances * b.p.n ** 2, b.num_per, b.dim0), name)
    qs = b.queries([recs[9][0], absent, recs[5][0]], 300)             # a full record, an absent item, the short record
    want = [b.o.process_query(b.clients[c][1], q, words) for c, _, q in qs]
    if name != "S16":
        assert b.want(qs) == want                                     # lib/server's own answer, where it has one
    for k in (0, 1):
        c, _, q = qs[k]
        sp.paths_taken()
        got = sp.process_query(b.p, b.clients[c][2], q, b.gdb)
        taken = sp.paths_taken()
        assert SPARSE in taken and SPARSE_GROUP not in taken and not BATCH_BITS & taken, taken
        _pack_bit(name, taken)
        assert got == want[k], k
    with batch_min(sp, 2):
        got, taken = b.ask(qs)
    assert {SPARSE_GROUP, SPARSE} <= taken and not BATCH_BITS & taken, taken
    assert [g == w for g, w in zip(got, want)] == [True] * 3


# ---- c, d ------------------------------------------------------------------------------------------------------------------------
def _lists(sp, c, db, state, name, check):
    for B in LISTS[name]:
        sp.paths_taken()
        got = c.batch(db, state, B)
        taken = sp.paths_taken()
        check(taken, B)
        _pack_bit(name, taken)
        assert [g == state.want(i) for i, g in enumerate(got)] == [True] * B, (name, B)
    sp.paths_taken()
    got = sp.process_query(c.p, c.gpps[1], state.qs[1], db)
    (assert_packed_single if check is assert_packed_list else lambda t: check(t, 1))(sp.paths_taken())
    assert got == state.want(1), name


def _assert_corner_words(db, c, corner):
    for key in corners(c.planes, c.npr):
        assert (db.read_ref(*key, 0, c.d0) == corner[key]).all(), key
    assert db.read_ref(c.planes - 1, N - 1, c.npr - 1, c.d0 - 1, 1)[0] == corner["last"]
    assert db.read_ref(0, 0, 0, 17, 3).tolist() == corner["run"].tolist()


@pytest.mark.parametrize("name", ALL)
def test_c_packed_with_its_planar_copy(sp, oracle_mod, name):
    c = dense(sp, oracle_mod, name, 6, 7, POOL[name])
    copy = c.planes * N * c.npr * c.d0 * 8
    db = sp.Database(c.p).load_items(c.blob)
    assert db.format() == "packed" and db.prepare_batch() is True and db.batch_copy_bytes() == copy
    for state, what in ((c.before, "loaded"), (c.after, "edited")):
        if state is c.after:
            assert db.update_rows(c.body) == (c.records, 4 + c.isz)
            assert db.batch_copy_bytes() == copy                      # the body patched the copy, it did not drop it
        _lists(sp, c, db, state, name, assert_packed_list)
        ref = state.references()[1]
        _same_digest(db.digest(DIGEST_SEED), ref, (name, what, "resident"))
        _same_digest(db.digest(DIGEST_SEED, which="batch_copy"), ref, (name, what, "batch copy"))
        assert db.batch_copy_bytes() == copy


@pytest.mark.parametrize("name", ALL)
def test_d_planar_resident(sp, oracle_mod, name):
    c = dense(sp, oracle_mod, name, 6, 7, POOL[name])
    db = sp.Database.planar(c.p).load_items(c.blob)
    assert db.format() == "planar" and db.device_bytes() == c.planes * N * c.npr * c.d0 * 8 and db.batch_copy_bytes() == 0
    for state, what in ((c.before, "loaded"), (c.after, "edited")):
        if state is c.after:
            assert db.update_rows(c.body) == (c.records, 4 + c.isz)
        corner, ref = state.references()
        _assert_corner_words(db, c, corner)
        _lists(sp, c, db, state, name, assert_planar_list)
        _same_digest(db.digest(DIGEST_SEED), ref, (name, what))
    back, present, undecodable = db.read_items(0, c.o.num_items)
    assert back == c.after.file.tobytes() and present.all() and undecodable == 0


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def _world(sp, G, steps):
    """every (name, fn(rank, comm)) of `steps` on G rank threads over the loopback world -> (results[rank][name], path bits of all
    ranks together per step, read while no rank runs)"""
    from sdk_amd.sharding import LoopbackWorld
    world, gate, taken = LoopbackWorld(G), threading.Barrier(G, timeout=300), {}

    def rank_main(r):
        sp.lib().sp_set_device(0)
        comm, res = world.comm(r), {}
        for step, fn in steps:
            gate.wait()
            if r == 0:
                sp.paths_taken()
            gate.wait()
            res[step] = fn(r, comm)
            gate.wait()
            if r == 0:
                taken[step] = sp.paths_taken()
        gate.wait()
        res["describe"] = comm.describe()
        return res
    try:
        return world.run(rank_main), taken
    except Exception:
        gate.abort()
        raise


@pytest.mark.parametrize("name", ["N3", "V1"])
def test_e_packed_row_shards(sp, oracle_mod, name):
    """sp_process_query_sharded and sp_process_queries_sharded_batched on PACKED row shards of 8 rows: the per-plane reduce-scatter
    and gather loops of comm.cpp at 9 and 16 planes; V1: finish_gathered with packing version 1 and four instances"""
    G = 2
    c = dense(sp, oracle_mod, name, 4, 7, 3)
    st = c.before
    shards = [sp.Database(c.p, s, G).load_items(c.blob) for s in range(G)]
    assert [d.format() for d in shards] == ["packed"] * G
    res, taken = _world(sp, G, [("one", lambda r, comm: comm.process_query(c.p, c.gpps[1], st.qs[1], shards[r])),
                                ("list", lambda r, comm: comm.process_queries_batched(c.p, c.gpp_list(3), st.qs[:3], shards[r]))])
    assert res[0]["one"] == st.want(1) and res[0]["list"] == [st.want(i) for i in range(3)]
    assert res[1]["one"] == b"" and res[1]["list"] == []
    for step, bits in taken.items():
        assert {SCATTER_OUT, "custom_transport", "expand_pruned"} <= bits and "rccl_in_library" not in bits, (step, bits)
        assert not {"sweep_batch_scatter", SPARSE, "sweep_batch_planar"} & bits, (step, bits)      # a list of 3 sweeps per query
        _pack_bit(name, bits)
    for r in range(G):
        info = res[r]["describe"]["last_list"]
        assert info["reduce_scatters"] == 3 * c.planes and info["all_gathers"] == 3, info


@pytest.mark.parametrize("name", ["N3", "V1"])
def test_e_sparse_shards(sp, oracle_mod, name):
    G = 2
    b = Sharded(oracle_mod, cfg(name, 6, 3), G)
    recs, file, absent = _filled_bucket(b, b.shards)
    assert sum(sh.sparse_items() for sh in b.shards) == len(recs) and all(sh.sparse_items() for sh in b.shards)
    qs = b.queries([recs[9][0], absent, recs[5][0]], 1100)
    want = b.want(qs)
    pps, q_list = [b.clients[c][2] for c, _, _ in qs], [q for _, _, q in qs]
    res, taken = _world(sp, G, [("one", lambda r, comm: comm.process_query(b.p, pps[0], q_list[0], b.shards[r])),
                                ("list", lambda r, comm: comm.process_queries_batched(b.p, pps, q_list, b.shards[r]))])
    assert res[0]["one"] == want[0] and res[0]["list"] == want
    assert res[1]["one"] == b"" and res[1]["list"] == []
    for step, bits in taken.items():
        assert {SPARSE, SCATTER_OUT, "custom_transport", "expand_pruned"} <= bits and not BATCH_BITS & bits, (step, bits)
        assert (SPARSE_GROUP in bits) == (step == "list"), (step, bits)
        _pack_bit(name, bits)
    for r in range(G):
        info = res[r]["describe"]["last_list"]
        assert info["reduce_scatters"] == 3 * b.planes and info["all_gathers"] == 3, info


# ---- f ---------------------------------------------------------------------------------------------------------------------------
def test_f_planar_row_shards(sp, oracle_mod):
    """N3 at 128 x 128, two shards of 64 rows: the group pass with two query tiles (9 queries) and one (3) leaves, word for word, what
    the per-plane scatter sweep leaves on a PACKED shard of the same content -- nine planes; lists with group 16 and 8 against the
    oracle over the unsharded words; the same /update-row body on both ranks, then the list again on the edited file"""
    G, B = 2, 9
    c = dense(sp, oracle_mod, "N3", 7, 7, B)
    st, nj = c.before, c.d0 // G
    packed = [sp.Database(c.p, s, G).load_items(c.blob) for s in range(G)]
    planar = [sp.Database.planar_shard(c.p, s, G).load_items(c.blob) for s in range(G)]
    for s in range(G):
        assert packed[s].format() == "packed" and planar[s].format() == "planar"
        assert planar[s].device_bytes() == c.planes * N * c.npr * nj * 8 and planar[s].batch_copy_bytes() == 0
        want = []
        for i in range(B):
            run = sp.QueryRun(c.p, c.gpps[i % 2], st.qs[i], db=packed[s])
            for pl in range(c.planes):
                run.sweep_scatter_plane(packed[s], G, pl)
            want.append(_partial(sp, run))
            run.free()
        for n in (B, 3):
            runs = [sp.QueryRun(c.p, c.gpps[i % 2], st.qs[i], db=planar[s]) for i in range(n)]
            sp.paths_taken()
            sp.QueryRun.sweep_scatter_group(runs, planar[s], G)
            got = [_partial(sp, r) for r in runs]
            _assert_pass(sp.paths_taken(), n)
            for k in range(n):
                assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (s, n, k, int((got[k] != want[k]).sum()))
            for r in runs:
                r.free()
        del want

    def listed(state, n, group, reserve=False):
        def fn(r, comm):
            if reserve:
                comm.reserve_batch_for(c.p, planar[r], 0)
            return comm.process_queries_batched(c.p, c.gpp_list(n), state.qs[:n], planar[r], group=group)
        return fn
    res, taken = _world(sp, G, [("nine", listed(st, B, 16, reserve=True)), ("three", listed(st, 3, 8))])
    assert res[0]["nine"] == [st.want(i) for i in range(B)] and res[0]["three"] == [st.want(i) for i in range(3)]
    assert res[1]["nine"] == [] and res[1]["three"] == []
    for step, n in (("nine", B), ("three", 3)):
        _assert_pass(taken[step], n)
        assert {"custom_transport", "expand_pruned"} <= taken[step], taken[step]
    for r in range(G):
        assert res[r]["describe"]["last_list"] == {"group": 8, "reduce_scatters": 3 * c.planes, "all_gathers": 3}, res[r]["describe"]
    for db in planar:
        assert db.update_rows(c.body) == (c.records, 4 + c.isz)          # the other shard's records are counted as applied
        assert db.device_bytes() == c.planes * N * c.npr * nj * 8
    res, taken = _world(sp, G, [("edited", listed(c.after, B, 16))])
    assert res[0]["edited"] == [c.after.want(i) for i in range(B)] and res[1]["edited"] == []
    _assert_pass(taken["edited"], B)
    assert res[0]["describe"]["last_list"] == {"group": 16, "reduce_scatters": B * c.planes, "all_gathers": B}


# ---- g ---------------------------------------------------------------------------------------------------------------------------
_migrations = {}


def _migration_case(oracle_mod, name):
    """the oracle's side, once per set: a sparse bucket filled to a third, its file, one query for a held item answered by
    lib/server's SparseDb and by spiral-rs over the dense words of the same file, the numpy digest of those words"""
    if name not in _migrations:
        c = cfg(name, 6, 7)
        o = oracle_mod.Params(c)
        recs, file = sparse_records(o, seed=53)
        cl = oracle_mod.Client(o)
        pp = cl.generate_keys(71)
        q = cl.generate_query(recs[9][0], 500)
        words = o.load_db_from_bytes(file.tobytes())
        dense_resp = o.process_query(pp, q, words)
        # every column holds full records, so no all-zero shortcut of lib/server's fold fires and a bucket's response is spiral-rs's
        # over the zero-filled file (tests/test_sparse_bucket.py::test_sparse_oracle_semantics).  S16: lib/server stores bytes
        # (loading.rs:290 asserts log2 p = 8), there is no SparseDb of a p = 512 bucket, and the dense response stands for it
        assert {i % o.num_per for i, d in recs if len(d) == o.db_item_size} == set(range(o.num_per))
        sparse = dense_resp
        if o.pt_modulus == 256:
            bucket = oracle_mod.SparseDb(o)
            for i, d in recs:
                bucket.update_item_raw(i, d)
            sparse = bucket.process_query(pp, q)
            assert sparse == dense_resp
            del bucket
        _migrations[name] = dict(cfg=c, o=o, recs=recs, file=file, pp=pp, q=q, stored=[i for i, _ in recs],
                                 sparse=sparse, dense=dense_resp,
                                 digest=digest_reference(words, planes_of(c), o.num_per, o.dim0))
    return _migrations[name]


@pytest.mark.parametrize("name", ["N3", "S16"])
def test_g_export_rows_moves_a_bucket_to_every_format(sp, oracle_mod, name):
    m = _migration_case(oracle_mod, name)
    o, file = m["o"], m["file"]
    p = sp.Params(m["cfg"])
    gpp = sp.PublicParameters.deserialize(p, m["pp"])
    src = sp.Database.sparse(p)
    assert src.update_rows(body(m["recs"]))[0] == len(m["recs"])
    exported = src.export_rows()
    assert exported == body([(i, file[i].tobytes()) for i in m["stored"]])
    del src
    for kind, make, check in (("packed", sp.Database, assert_packed_single), ("planar", sp.Database.planar, lambda t: assert_planar_list(t, 1)),
                              ("sparse", sp.Database.sparse, lambda t: (SPARSE in t and not BATCH_BITS & t) or pytest.fail(str(t)))):
        dst = make(p)
        assert dst.format() == kind
        assert dst.update_rows(exported)[0] == len(m["stored"])
        back, present, undecodable = dst.read_items(0, o.num_items)
        assert back == file.tobytes() and undecodable == 0, kind
        assert np.nonzero(present)[0].tolist() == (m["stored"] if kind == "sparse" else list(range(o.num_items))), kind
        _same_digest(dst.digest(DIGEST_SEED), m["digest"], (name, kind))
        sp.paths_taken()
        got = sp.process_query(p, gpp, m["q"], dst)
        check(sp.paths_taken())
        assert got == (m["sparse"] if kind == "sparse" else m["dense"]), kind
        del dst


# ---- h ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S16", "V0"])
def test_h_list_decodes_its_items(sp, oracle_mod, name):
    """t_gsw = 10 and 8 leave room to decode: p = 512 with a ragged item and n = 4, end to end through a list on the planar handle"""
    c = dense(sp, oracle_mod, name, 6, 7, POOL[name])
    st = c.before
    B = POOL[name]
    db = sp.Database.planar(c.p).load_items(c.blob)
    sp.paths_taken()
    got = c.batch(db, st, B)
    assert_planar_list(sp.paths_taken(), B)
    for i in range(B):
        assert got[i] == st.want(i), i
        plain = c.cls[i % 2].decode_response(got[i])
        item = c.blob[st.idxs[i] * c.isz:(st.idxs[i] + 1) * c.isz].tobytes()
        assert plain[:c.isz] == item and not any(plain[c.isz:]), i
