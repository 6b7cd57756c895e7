"""Planar-resident databases (sp_db_create_planar): a handle whose only resident form is the digit-planar layout of
sdk_amd/csrc/sweep_planar.hpp, written by the kernels of planar_resident.hpp and read by k_sweep_planar with one query tile (1 .. 8
queries) or two (9 .. 16).  Every comparison is byte equality: with the oracle's words (read_ref), with the oracle's process_query,
or with a PACKED handle of the same content.

Shapes: 64 x 128 (one 64-row block, one 128-column chunk: four-wave workgroups, ring of 2), 128 x 256 (two blocks, two chunks: the
eight-wave split and the ring of 4) and, once, 512 x 128 (the 64 KiB of LDS of one tile).  The path bits name the pass: the one-tile
planar pass is sweep_batch | sweep_batch_mfma | sweep_batch_planar WITHOUT sweep_batch_mfma_two_tiles, which no other flow reports."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q0, Q1 = 268369921, 249561089
_SHAPES = {"64x128": (6, 7), "128x256": (7, 8)}
_ONE_TILE = {"sweep_batch", "sweep_batch_mfma", "sweep_batch_planar"}
_NOT_ONE_TILE = {"sweep_batch_mfma_two_tiles", "sweep_ring", "sweep_packed_persist", "sweep_packed", "sweep_wide", "sweep_narrow",
                 "sweep_narrow_group"}
POOL = 16          # queries per shape, under two clients' keys (query i: client i % 2); a list of B is the pool's first B


def _cfg(nu_1, nu_2):
    return {"n": 2, "nu_1": nu_1, "nu_2": nu_2, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8,
            "t_exp_right": 56, "instances": 1, "db_item_size": 256}


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


class _Ctx:
    """one shape: params, two clients, a random item file, its oracle words, a pool of queries and (lazily, once) the oracle's
    responses to them; nothing in here is changed by a test"""

    def __init__(self, sp, oracle_mod, name):
        self.sp, self.cfg = sp, _cfg(*_SHAPES[name])
        self.o = oracle_mod.Params(self.cfg)
        self.p = sp.Params(self.cfg)
        self.cls = [oracle_mod.Client(self.o), oracle_mod.Client(self.o)]
        self.pps = [self.cls[0].generate_keys(61), self.cls[1].generate_keys(62)]
        self.gpps = [sp.PublicParameters.deserialize(self.p, pp) for pp in self.pps]
        rng = np.random.default_rng(sum(_SHAPES[name]))
        self.isz, self.npr, self.d0 = self.o.db_item_size, self.o.num_per, self.o.dim0
        self.blob = rng.integers(0, 256, self.o.num_items * self.isz, dtype=np.uint8)
        self.blob.setflags(write=False)
        self._words = None
        self.idxs = [(977 * i + 3) % self.o.num_items for i in range(POOL)]
        self.qs = [self.cls[i % 2].generate_query(self.idxs[i], 900 + i) for i in range(POOL)]
        self._want = {}

    @property
    def words(self):
        if self._words is None:
            self._words = self.o.load_db_from_bytes(self.blob.tobytes())
            self._words.setflags(write=False)
        return self._words

    def want(self, i):
        if i not in self._want:
            self._want[i] = self.o.process_query(self.pps[i % 2], self.qs[i], self.words)
        return self._want[i]

    def planar(self):
        return self.sp.Database.planar(self.p).load_items(self.blob)

    def batch(self, db, B, qs=None):
        return self.sp.process_query_batch(self.p, [self.gpps[i % 2] for i in range(B)], (qs or self.qs)[:B], db)


_ctxs = {}


def _ctx(sp, oracle_mod, name):
    if name not in _ctxs:
        _ctxs[name] = _Ctx(sp, oracle_mod, name)
    return _ctxs[name]


def _planar_bytes(c):
    return 4 * 2048 * c.npr * c.d0 * 8


def _corners(c):
    """first and last plane, z, column and row (and one of each in between)"""
    return [(pl, z, ii) for pl in (0, 3) for z in (0, 1029, 2047) for ii in (0, 1, 77, c.npr - 2, c.npr - 1)]


def _assert_words(db, c, want4):
    """want4: [plane][z][ii][j]"""
    for pl, z, ii in _corners(c):
        got = db.read_ref(pl, z, ii, 0, c.d0)
        assert (got == want4[pl, z, ii]).all(), (pl, z, ii)
    assert db.read_ref(3, 2047, c.npr - 1, c.d0 - 1, 1)[0] == want4[3, 2047, c.npr - 1, c.d0 - 1]
    assert db.read_ref(0, 0, 0, 17, 3).tolist() == want4[0, 0, 0, 17:20].tolist()


# ------------------------------------------------------------------------------------------------ 1. loaders
@pytest.mark.parametrize("name", list(_SHAPES))
def test_load_items_reads_back(sp, oracle_mod, name):
    c = _ctx(sp, oracle_mod, name)
    db = c.planar()
    assert db.format() == "planar"
    assert db.device_bytes() == _planar_bytes(c) and db.batch_copy_bytes() == 0
    assert db.prepare_batch() is True
    assert db.device_bytes() == _planar_bytes(c) and db.batch_copy_bytes() == 0
    _assert_words(db, c, c.words.reshape(4, 2048, c.npr, c.d0))


@pytest.mark.parametrize("name", list(_SHAPES))
def test_load_and_load_plane_read_back(sp, oracle_mod, name):
    c = _ctx(sp, oracle_mod, name)
    want4 = c.words.reshape(4, 2048, c.npr, c.d0)
    _assert_words(sp.Database.planar(c.p).load(c.words), c, want4)
    db = sp.Database.planar(c.p)
    cut = 700                                       # two z-ranges per plane, the second first
    for pl in range(4):
        db.load_plane(pl, cut, 2048 - cut, want4[pl, cut:])
        db.load_plane(pl, 0, cut, want4[pl, :cut])
    _assert_words(db, c, want4)
    for pl, z, ii in ((1, cut - 1, 5), (1, cut, 5), (2, cut, c.npr - 1)):
        assert (db.read_ref(pl, z, ii, 0, c.d0) == want4[pl, z, ii]).all(), (pl, z, ii)


def test_limbs_above_q_are_reduced_as_on_packed(sp, oracle_mod):
    """crafted words with limbs >= q up to 2^32 - 1: the planar loader reduces them as the PACKED loader does"""
    c = _ctx(sp, oracle_mod, "64x128")
    rng = np.random.default_rng(7)
    lo = np.array([Q0, Q0 + 1, 2**32 - 1, 2**28, 0, Q0 - 1, 0x80808080, 0x7F7F7F7F], dtype=np.uint64)
    hi = np.array([Q1, Q1 + 1, 2**32 - 1, 2**28, 0, Q1 - 1, 0x80808080, 0x7F7F7F7F], dtype=np.uint64)
    n = 4 * 2048 * c.npr * c.d0
    pick = rng.integers(0, 8, n)
    words = (lo[pick] | (hi[(pick + 3) % 8] << np.uint64(32))).astype(np.uint64)
    a, b = sp.Database.planar(c.p).load(words), sp.Database(c.p).load(words)
    assert b.format() == "packed"
    w4 = words.reshape(4, 2048, c.npr, c.d0)
    for pl, z, ii in _corners(c):
        got = a.read_ref(pl, z, ii, 0, c.d0)
        assert (got == b.read_ref(pl, z, ii, 0, c.d0)).all(), (pl, z, ii)
        assert ((got & np.uint64(0xFFFFFFFF)) == (w4[pl, z, ii] & np.uint64(0xFFFFFFFF)) % np.uint64(Q0)).all()
        assert ((got >> np.uint64(32)) == (w4[pl, z, ii] >> np.uint64(32)) % np.uint64(Q1)).all()


def test_fresh_handle_is_the_zero_database_and_fill_synthetic(sp, oracle_mod):
    """the empty database is every byte 0x80 (the offset digit of 0), which reads back as zero words"""
    from sdk_amd.spiral import synth_words
    c = _ctx(sp, oracle_mod, "64x128")
    db = sp.Database.planar(c.p)
    assert db.format() == "planar" and db.device_bytes() == _planar_bytes(c)
    for pl, z, ii in _corners(c):
        assert not db.read_ref(pl, z, ii, 0, c.d0).any(), (pl, z, ii)
    db.fill_synthetic(0xC0FFEE)
    for pl, z, ii in _corners(c):
        ref = ((pl * 2048 + z) * c.npr + ii) * c.d0 + np.arange(c.d0, dtype=np.uint64)
        assert (db.read_ref(pl, z, ii, 0, c.d0) == synth_words(0xC0FFEE, ref)).all(), (pl, z, ii)


# ------------------------------------------------------------------------------------------------ 2. every group size
_planar_dbs = {}


def _loaded(c, name):
    """one loaded planar handle per shape for the read-only tests"""
    if name not in _planar_dbs:
        _planar_dbs[name] = c.planar()
    return _planar_dbs[name]


def _assert_one_tile(taken):
    assert _ONE_TILE <= taken and not (_NOT_ONE_TILE & taken), taken


def _assert_two_tiles(taken):
    assert _ONE_TILE | {"sweep_batch_mfma_two_tiles"} <= taken and not ((_NOT_ONE_TILE - {"sweep_batch_mfma_two_tiles"}) & taken), taken


@pytest.mark.parametrize("B", [1, 2, 3, 4, 7, 8, 9, 11, 16], ids=lambda b: "B%02d" % b)
@pytest.mark.parametrize("name", list(_SHAPES))
def test_every_group_size(sp, oracle_mod, name, B):
    c = _ctx(sp, oracle_mod, name)
    db = _loaded(c, name)
    sp.paths_taken()
    resp = c.batch(db, B)
    taken = sp.paths_taken()
    if B <= 8:
        _assert_one_tile(taken)
    else:
        _assert_two_tiles(taken)
    for i in range(B):
        assert resp[i] == c.want(i), (B, i)
    sp.paths_taken()
    single = sp.process_query(c.p, c.gpps[0], c.qs[0], db)
    _assert_one_tile(sp.paths_taken())
    assert single == c.want(0)
    if B == 3:     # one response decodes to the planted item
        got = c.cls[1].decode_response(resp[1])
        item = c.blob[c.idxs[1] * c.isz:(c.idxs[1] + 1) * c.isz].tobytes()
        assert all(got[t * 64:(t + 1) * 64] == item[t * 64:(t + 1) * 64] for t in range(4))


def test_stage_level_calls_on_a_planar_handle(sp, oracle_mod):
    """sp_query_begin / sp_query_sweep / sp_query_finish, and sp_bench_sweep_batch with one and with two tiles"""
    c = _ctx(sp, oracle_mod, "64x128")
    db = _loaded(c, "64x128")
    run = sp.QueryRun(c.p, c.gpps[1], c.qs[1])
    sp.paths_taken()
    run.sweep(db)
    assert run.finish() == c.want(1)
    _assert_one_tile(sp.paths_taken())
    runs = [sp.QueryRun(c.p, c.gpps[i % 2], c.qs[i]) for i in range(9)]
    assert sp.bench_sweep_batch(runs[:5], db, 1) > 0
    _assert_one_tile(sp.paths_taken())
    assert sp.bench_sweep_batch(runs, db, 1) > 0
    _assert_two_tiles(sp.paths_taken())


# ------------------------------------------------------------------------------------------------ 3. upserts in place
def _body(records):
    return b"".join(struct.pack(">II", 4 + len(d), i) + bytes(d) for i, d in records)


def _edits(c):
    """the edit list of test_planar_copy_lifecycle: first and last row and column, both columns of a lane slot, both rows of a row
    pair, an overwrite (item 1 twice), short records -> (records, the edited file)"""
    rng = np.random.default_rng(29)
    npr, d0, isz = c.npr, c.d0, c.isz
    edits = [0, 1, npr, npr + 1, (d0 - 1) * npr + npr - 1, (d0 // 2) * npr + 77, 3 * npr + 126, 3 * npr + 127, 64 * npr % c.o.num_items + 5, 1]
    after, recs = c.blob.copy(), []
    for k, it in enumerate(edits):
        rec = rng.integers(0, 256, isz - (k % 4), dtype=np.uint8)
        after[it * isz:(it + 1) * isz] = 0
        after[it * isz:it * isz + rec.size] = rec
        recs.append((it, rec.tobytes()))
    return edits, recs, after


@pytest.mark.parametrize("name", list(_SHAPES))
def test_upserts_in_place(sp, oracle_mod, name):
    c = _ctx(sp, oracle_mod, name)
    edits, recs, after = _edits(c)
    # a zero-length record and a duplicate index in the body: the zero-length one clears item 2 * npr + 9, the later record wins
    extra = 2 * c.npr + 9
    after[extra * c.isz:(extra + 1) * c.isz] = 0
    exp = c.o.load_db_from_bytes(after.tobytes())
    exp4 = exp.reshape(4, 2048, c.npr, c.d0)
    one_by_one, as_body = c.planar(), c.planar()
    for it, rec in recs:
        one_by_one.update_item(it, rec)
    one_by_one.update_item(extra, b"")
    body = _body([(edits[3], b"\x55" * c.isz)] + recs[:5] + [(extra, b"")] + recs[5:])      # edits[3] again later: the later one wins
    assert as_body.update_rows(body) == (len(recs) + 2, 4 + c.isz)
    B = 11
    idxs = [edits[i] if i < 9 else c.idxs[i] for i in range(B)]
    qs = [c.cls[i % 2].generate_query(idxs[i], 700 + i) for i in range(B)]
    # the oracle on the edited file: every member at 64 x 128; at 128 x 256, where an oracle query costs most of a second, the single
    # query and three more members (an edited row pair, the decoded one, the last) -- the two handles' lists are compared whole
    checked = range(B) if name == "64x128" else (0, 3, 4, B - 1)
    want = {i: c.o.process_query(c.pps[i % 2], qs[i], exp) for i in checked}
    lists = []
    for db in (one_by_one, as_body):
        assert db.device_bytes() == _planar_bytes(c) and db.batch_copy_bytes() == 0
        sp.paths_taken()
        lists.append(c.batch(db, B, qs))
        _assert_two_tiles(sp.paths_taken())
        for i in checked:
            assert lists[-1][i] == want[i], i
        assert sp.process_query(c.p, c.gpps[0], qs[0], db) == want[0]
        for pl, z in ((0, 0), (3, 2047)):
            for it in edits + [extra, 2, c.npr + 2]:       # the edited items and neighbours that share their entries
                j, ii = divmod(it, c.npr)
                assert db.read_ref(pl, z, ii, j, 1)[0] == exp4[pl, z, ii, j], (pl, z, it)
    assert lists[0] == lists[1]
    got = c.cls[0].decode_response(want[4])
    item = after[idxs[4] * c.isz:(idxs[4] + 1) * c.isz].tobytes()
    assert all(got[t * 64:(t + 1) * 64] == item[t * 64:(t + 1) * 64] for t in range(4))


def test_faulty_third_record_applies_the_prefix(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "64x128")
    db = c.planar()
    good = [(5, b"\x11" * c.isz), (c.npr + 6, b"\x22" * 7)]
    with pytest.raises(sp.SpiralError) as e:
        db.update_rows(_body(good) + struct.pack(">II", 4 + 3, c.o.num_items) + b"abc")
    assert e.value.rc == -1 and e.value.applied == 2 and "record 2" in str(e.value), str(e.value)
    after = c.blob.copy()
    for i, d in good:
        after[i * c.isz:(i + 1) * c.isz] = 0
        after[i * c.isz:i * c.isz + len(d)] = np.frombuffer(d, dtype=np.uint8)
    exp4 = c.o.load_db_from_bytes(after.tobytes()).reshape(4, 2048, c.npr, c.d0)
    for pl, z in ((0, 0), (2, 1000), (3, 2047)):
        assert (db.read_ref(pl, z, 5, 0, c.d0) == exp4[pl, z, 5]).all()
        assert (db.read_ref(pl, z, 6, 0, c.d0) == exp4[pl, z, 6]).all()
    # SP_E_ARG on the array form leaves the handle untouched
    with pytest.raises(sp.SpiralError):
        db.update_items([(7, b"\x33" * c.isz), (c.o.num_items, b"x")])
    assert (db.read_ref(1, 9, 7, 0, c.d0) == exp4[1, 9, 7]).all()


# ------------------------------------------------------------------------------------------------ 4. switches and refusals
def test_switches_after_creation_change_nothing(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "64x128")
    db = _loaded(c, "64x128")
    base5, base11 = c.batch(db, 5), c.batch(db, 11)
    assert base5 == [c.want(i) for i in range(5)] and base11 == [c.want(i) for i in range(11)]
    for switch, off, on in ((b"batch_planar", 0, 1), (b"batch_mfma", 0, 1), (b"batch_mfma_min", 9, 4)):
        sp.lib().sp_debug_set(switch, C.c_long(off))
        try:
            sp.paths_taken()
            assert c.batch(db, 5) == base5, switch
            _assert_one_tile(sp.paths_taken())
            assert c.batch(db, 11) == base11, switch
            _assert_two_tiles(sp.paths_taken())
            assert db.device_bytes() == _planar_bytes(c) and db.format() == "planar" and db.prepare_batch() is True
        finally:
            sp.lib().sp_debug_set(switch, C.c_long(on))


def test_creation_is_refused_where_the_format_does_not_exist(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "64x128")
    for switch in (b"batch_planar", b"batch_mfma"):
        sp.lib().sp_debug_set(switch, C.c_long(0))
        try:
            with pytest.raises(sp.SpiralError, match="batch_planar and batch_mfma"):
                sp.Database.planar(c.p)
        finally:
            sp.lib().sp_debug_set(switch, C.c_long(1))
    for nu in ((5, 7), (6, 3)):
        with pytest.raises(sp.SpiralError, match="dim0 % 64 == 0"):
            sp.Database.planar(sp.Params(_cfg(*nu)))
    with pytest.raises(sp.SpiralError, match="unsharded"):
        sp.Database.planar(c.p, 0, 2)
    assert sp.Database.planar(c.p).format() == "planar"


def test_entry_points_that_refuse_a_planar_handle(sp, oracle_mod):
    from sdk_amd.sharding import Comm
    c = _ctx(sp, oracle_mod, "64x128")
    db = _loaded(c, "64x128")
    run = sp.QueryRun(c.p, c.gpps[0], c.qs[0])
    for call in (lambda: run.sweep_scatter(db, 1), lambda: run.sweep_scatter_plane(db, 1, 0),
                 lambda: sp.QueryRun.sweep_scatter_group([run], db, 1), lambda: run.bench_sweep(db, 1),
                 lambda: run.bench_sweep(db, 1, per_plane=1)):
        with pytest.raises(sp.SpiralError, match="planar-resident"):
            call()
    comm = Comm.custom(0, 1, lambda *a: 0, lambda *a: 0)
    try:
        for call in (lambda: comm.process_query(c.p, c.gpps[0], c.qs[0], db), lambda: comm.process_queries(c.p, c.gpps[0], c.qs[:2], db),
                     lambda: comm.process_queries_batched(c.p, c.gpps[0], c.qs[:2], db)):
            with pytest.raises(sp.SpiralError, match="planar-resident"):
                call()
    finally:
        comm.free()
    # the refused calls enqueued nothing: the query still sweeps and finishes
    run.sweep(db)
    assert run.finish() == c.want(0)


# ------------------------------------------------------------------------------------------------ 5. the LDS boundary
def test_lds_boundary_512_rows(sp, oracle_mod):
    """512 x 128: one tile's query planes of a z-row are exactly 64 KiB of LDS, two tiles' 128 KiB; 4.3 GB of synthetic words"""
    cfg = _cfg(9, 7)
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(63)
    gpp = sp.PublicParameters.deserialize(p, pp)
    seed = 0x5EED
    db = sp.Database.planar(p).fill_synthetic(seed)
    assert db.device_bytes() == 4 * 2048 * 128 * 512 * 8
    qs = [cl.generate_query((7919 * i + 11) % o.num_items, 300 + i) for i in range(16)]
    want = [o.process_query_synth(pp, q, seed) for q in qs]
    for B, check in ((1, _assert_one_tile), (8, _assert_one_tile), (16, _assert_two_tiles)):
        sp.paths_taken()
        assert sp.process_query_batch(p, [gpp] * B, qs[:B], db) == want[:B], B
        check(sp.paths_taken())


# ------------------------------------------------------------------------------------------------ 6. request layer
def test_server_on_a_planar_handle_equals_packed(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "64x128")
    dbs = [c.planar(), sp.Database(c.p).load_items(c.blob)]
    assert [d.format() for d in dbs] == ["planar", "packed"]
    srvs = [sp.Server(c.p, d) for d in dbs]
    uuids = [[s.setup(pp).encode() for pp in c.pps] for s in srvs]
    reads = lambda k: srvs[k].private_read([uuids[k][i % 2] + c.qs[i] for i in range(10)])     # noqa: E731
    first = reads(0)
    assert first == reads(1) and first == [c.want(i) for i in range(10)]
    recs = [(c.idxs[0], b"\x5a" * c.isz), (c.idxs[3], b"\x01\x02\x03"), (c.idxs[0] ^ 1, b"")]
    replies = [s.update_row(_body(recs)) for s in srvs]
    assert all('"status":"done updating"' in r for r in replies), replies
    second = reads(0)
    assert second == reads(1) and second[0] != first[0]
    after = c.blob.copy()
    for i, d in recs:
        after[i * c.isz:(i + 1) * c.isz] = 0
        after[i * c.isz:i * c.isz + len(d)] = np.frombuffer(d, dtype=np.uint8)
    exp = c.o.load_db_from_bytes(after.tobytes())
    for i in (0, 3):
        assert second[i] == c.o.process_query(c.pps[i % 2], c.qs[i], exp), i
    assert dbs[0].device_bytes() == _planar_bytes(c)


# ------------------------------------------------------------------------------------------------ 7. two threads
def test_two_threads_submit_lists(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "64x128")
    db = _loaded(c, "64x128")
    want = [c.want(i) for i in range(15)]
    got, errors = {}, []

    def submit(key, lo, hi):
        try:
            got[key] = sp.process_query_batch(c.p, [c.gpps[i % 2] for i in range(lo, hi)], c.qs[lo:hi], db)
        except Exception as e:                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=submit, args=("nine", 0, 9)), threading.Thread(target=submit, args=("six", 9, 15))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got["nine"] == want[:9] and got["six"] == want[9:15]
