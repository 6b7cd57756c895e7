"""Items back out of a resident database (sp_db_read_items, sp_db_export_rows), on every format.  Byte equality only.

1  independent pin: the ORACLE's load_db_from_bytes words go in through sp_db_load, so the library's own encoder is not in the loop,
   and read_items must return the file -- ragged and full chunks, a short file, items that spill into their neighbours, logp = 4, 6,
   8 and 9, 8 planes.  Every file starts 00 80 81 ff 7f: the values 0, p / 2, p / 2 + 1 and p - 1 at p = 256.
2  every format: the same file through load_items and, separately, through one /update-row body -- PACKED, planar-resident, row shards,
   PACKED column shards, planar shards, a sparse bucket and sparse shards; on shards the `present` masks are disjoint, their union is the
   held set and the bytes OR-ed over the ranks are the file's.
3  ranges and windows: db_load_window small enough that a range spans at least three windows; the SP_E_ARG cases write nothing.
4  undecodable words, built with the oracle's to_ntt: the exact count, the neighbours' bytes, export_rows' SP_E_STATE.
5  migration: export_rows of a sparse bucket applied to a sparse, a PACKED, a planar-resident and an 8-byte handle; PACKED to planar.
6  two host threads on one handle, one answering queries, one reading the database.
7  cases 2 and 5 on poisoned and on guarded buffers (the procedure of tests/test_gpu_hardened_buffers.py).
tests/test_emulated_item_readback.py runs a subset on the emulated device."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

from conftest import FAST, SMALL_INST2
from test_gpu_narrow_batch import switch
from test_gpu_planar_shards import _cfg as _planar_cfg

pytestmark = pytest.mark.gpu

Q0, Q1 = 268369921, 249561089
Q = Q0 * Q1
N = 2048
HEAD = (0x00, 0x80, 0x81, 0xff, 0x7f)
SP_E_ARG, SP_E_STATE = -1, -4
WINDOW_DEFAULT = 512 << 20
PACKED = dict(FAST, nu_1=6, nu_2=7, db_item_size=256)          # 64 x 128: PACKED words; the planar-resident shape
NARROW = dict(FAST, db_item_size=256)                          # 64 x 4: 8-byte words
SPARSE = dict(FAST, nu_1=6, nu_2=3, db_item_size=256)


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _blob(o, short=0, seed=7):
    b = np.random.default_rng(seed).integers(0, 256, o.num_items * o.db_item_size - short, dtype=np.uint8)
    b[:len(HEAD)] = HEAD
    return b


def _file(o, blob):
    """the item file as the database sees it: zeros past a short file"""
    e = np.zeros(o.num_items * o.db_item_size, dtype=np.uint8)
    e[:blob.size] = blob
    return e


def _body(records):
    return b"".join(struct.pack(">II", 4 + len(d), i) + bytes(d) for i, d in records)


class _Own:
    """the handles of a flow outside the hardened runs: kept until the flow's caller lets go of them"""

    def __init__(self, sp):
        self.sp, self.objs = sp, []

    def own(self, obj):
        self.objs.append(obj)
        return obj

    def params(self, cfg):
        return self.own(self.sp.Params(cfg))


def _no_switch():
    return 0


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
PIN = {"narrow": (NARROW, 0), "packed-ragged-chunk": (dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=1000), 0),
       "full-poly": (dict(FAST, nu_1=3, nu_2=1, db_item_size=8192), 0),
       "packed-short-file": (dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=512), 3000),
       "p16-nu2_0": (dict(FAST, nu_1=3, nu_2=0, db_item_size=300, p=16), 100),
       "p64-logp6": (dict(FAST, nu_1=3, nu_2=1, db_item_size=1000, p=64), 0),
       "p512-logp9": (dict(FAST, nu_1=3, nu_2=1, db_item_size=1000, p=512), 0),
       "inst2-8planes": (SMALL_INST2, 0),
       "5B-spill": (dict(FAST, nu_1=4, nu_2=1, db_item_size=5), 0),
       "1001B-spill": (dict(FAST, nu_1=4, nu_2=1, db_item_size=1001), 0)}


@pytest.mark.parametrize("name", list(PIN))
def test_oracle_words_read_back_as_the_file(sp, oracle_mod, name):
    cfg, short = PIN[name]
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    blob = _blob(o, short, seed=o.db_item_size)
    db = sp.Database(p).load(o.load_db_from_bytes(blob.tobytes()))
    got, present, undecodable = db.read_items(0, o.num_items)
    assert got == _file(o, blob).tobytes()
    assert undecodable == 0 and present.all() and present.size == o.num_items


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
FORMATS = {"packed": (PACKED, 1), "planar": (PACKED, 1), "row-shards-8x4": (dict(FAST, nu_1=8, nu_2=4, db_item_size=256), 2),
           "packed-row-shards": (dict(FAST, nu_1=4, nu_2=7, db_item_size=256), 2),
           "packed-column-shards": (dict(FAST, nu_1=4, nu_2=8, db_item_size=256), 2), "planar-shards-A": (_planar_cfg(7, 7), 2),
           "sparse": (SPARSE, 1), "sparse-shards": (SPARSE, 2)}
WANT_FORMAT = {"packed": "packed", "planar": "planar", "row-shards-8x4": "words8", "packed-row-shards": "packed",
               "packed-column-shards": "packed", "planar-shards-A": "planar", "sparse": "sparse", "sparse-shards": "sparse"}


def _make(sp, S, p, fmt, s, G):
    D = sp.Database
    if fmt in ("packed",):
        return S.own(D(p))
    if fmt == "planar":
        return S.own(D.planar(p))
    if fmt in ("row-shards-8x4", "packed-row-shards"):
        return S.own(D(p, s, G))
    if fmt == "packed-column-shards":
        return S.own(D(p, s, G, by_columns=True))
    if fmt == "planar-shards-A":
        return S.own(D.planar_shard(p, s, G))
    return S.own(D.sparse(p, s, G))


def _holds(fmt, o, G, s, i, stored):
    j, ii = divmod(i, o.num_per)
    if fmt == "packed-column-shards":
        return ii % G == s
    return j // (o.dim0 // G) == s and (stored is None or i in stored)


def _sparse_records(o, seed=11):
    """a scattered third of the items, one of them zero-length and one short -> [(index, bytes)]"""
    rng = np.random.default_rng(seed)
    idx = sorted(int(i) for i in rng.choice(o.num_items, o.num_items // 3, replace=False))
    recs = [(i, rng.integers(0, 256, o.db_item_size, dtype=np.uint8).tobytes()) for i in idx]
    recs[3] = (recs[3][0], b"")
    recs[5] = (recs[5][0], recs[5][1][:37])
    recs[0] = (recs[0][0], bytes(HEAD) + recs[0][1][len(HEAD):])
    return recs


def _formats_flow(fmt):
    def flow(sp, oracle_mod, S, arm):
        cfg, G = FORMATS[fmt]
        o = oracle_mod.Params(cfg)
        isz = o.db_item_size
        sparse = fmt.startswith("sparse")
        if sparse:
            recs = _sparse_records(o)
            want = np.zeros((o.num_items, isz), dtype=np.uint8)
            for i, d in recs:
                want[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
            stored = {i for i, _ in recs}
        else:
            want = _file(o, _blob(o)).reshape(o.num_items, isz)
            recs, stored = [(i, want[i].tobytes()) for i in range(o.num_items)], None
        body = _body(recs)
        arm()
        sp.paths_taken()
        p = S.params(cfg)
        for way in ("load_items", "update_rows"):
            union = np.zeros(o.num_items, dtype=np.uint8)
            ored = np.zeros(o.num_items * isz, dtype=np.uint8)
            for s in range(G):
                db = _make(sp, S, p, fmt, s, G)
                assert db.format() == WANT_FORMAT[fmt]
                if way == "update_rows":
                    assert db.update_rows(body)[0] == len(recs)
                elif sparse:
                    for i, d in recs:
                        db.update_item(i, d)
                else:
                    db.load_items(want.tobytes())
                got, present, undecodable = db.read_items(0, o.num_items)
                assert undecodable == 0
                held = np.array([_holds(fmt, o, G, s, i, stored) for i in range(o.num_items)], dtype=np.uint8)
                assert (present == held).all(), (way, s)
                mine = np.where(held[:, None] != 0, want, 0).astype(np.uint8)
                assert got == mine.tobytes(), (way, s)
                assert not (union & present).any()
                union |= present
                ored |= np.frombuffer(got, dtype=np.uint8)
            assert (union != 0).tolist() == [stored is None or i in stored for i in range(o.num_items)]
            assert ored.tobytes() == want.tobytes()
        return sp.paths_taken()
    flow.__name__ = "readback_formats_" + fmt
    return flow


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_every_format_reads_back_what_was_written(sp, oracle_mod, fmt):
    _formats_flow(fmt)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
RANGED = {"packed-16x256": dict(FAST, nu_1=4, nu_2=8, db_item_size=256), "planar-64x128": PACKED, "narrow": NARROW}
_ranged = {}


def _ranged_db(sp, oracle_mod, name):
    """one database per shape, loaded once and read whole once under the shipped window; nothing in here is changed by a test"""
    if name not in _ranged:
        cfg = RANGED[name]
        o, p = oracle_mod.Params(cfg), sp.Params(cfg)
        want = _file(o, _blob(o, seed=23))
        db = (sp.Database.planar(p) if name.startswith("planar") else sp.Database(p)).load_items(want.tobytes())
        whole, present, undecodable = db.read_items(0, o.num_items)
        assert whole == want.tobytes() and present.all() and undecodable == 0
        _ranged[name] = (o, p, db, whole)
    return _ranged[name]


@pytest.mark.parametrize("name", list(RANGED))
def test_ranges_across_small_windows(sp, oracle_mod, name):
    o, p, db, whole = _ranged_db(sp, oracle_mod, name)
    npr, isz = o.num_per, o.db_item_size
    per_item = 8 + isz + 4 * N * 8
    ranges = [(npr + 1, 1),                       # one item at an odd index
              (2 * npr + 1, 2 * npr - 3),         # starts and ends inside the row pair (2, 3)
              (npr - 3, 2 * npr + 9),             # from the end of row 0 into row 3: two row pairs
              (o.num_items - 1, 1), (o.num_items - 2 * npr - 1, 2 * npr + 1)]
    if npr > 128:
        ranges.append((npr + 100, 60))            # crosses a 128-column chunk inside a row
    with switch(sp, "db_load_window", 64 + max(1, (2 * npr - 3) // 4) * per_item, default=WINDOW_DEFAULT):
        for a, n in ranges:
            got, present, undecodable = db.read_items(a, n)
            assert got == whole[a * isz:(a + n) * isz], (a, n)
            assert present.all() and undecodable == 0
    got, _, _ = db.read_items(3, 2 * npr)         # the buffer grows back before the first kernel of this call
    assert got == whole[3 * isz:(3 + 2 * npr) * isz]
    got, present, undecodable = db.read_items(5, 0)
    assert got == b"" and present.size == 0 and undecodable == 0


def test_bad_ranges_write_nothing(sp, oracle_mod):
    o, p, db, whole = _ranged_db(sp, oracle_mod, "narrow")
    isz, n_items = o.db_item_size, o.num_items
    L = sp.lib()
    for item0, count, cap in ((n_items - 1, 2, 2 * isz), (2 ** 64 - 1, 2, 2 * isz), (0, 2, 2 * isz - 1)):
        out = np.full(2 * isz + 16, 0xCC, dtype=np.uint8)
        present = np.full(4, 0xCC, dtype=np.uint8)
        undecodable = C.c_size_t(0xCCCC)
        rc = L.sp_db_read_items(C.c_void_p(db.h), C.c_size_t(item0), C.c_size_t(count), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                C.c_size_t(cap), present.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(undecodable))
        assert rc == SP_E_ARG, (item0, count, cap)
        assert (out == 0xCC).all() and (present == 0xCC).all() and undecodable.value == 0xCCCC
    # count == 0: SP_OK and nothing written, at the end of the range too
    out = np.full(16, 0xCC, dtype=np.uint8)
    rc = L.sp_db_read_items(C.c_void_p(db.h), C.c_size_t(n_items), C.c_size_t(0), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(0),
                            None, None)
    assert rc == 0 and (out == 0xCC).all()
    # the export: a range past the end, and a buffer below the records of the range
    body = np.full(3 * (8 + isz), 0xCC, dtype=np.uint8)
    blen, nrec = C.c_size_t(7), C.c_size_t(7)
    for item0, count, cap in ((n_items - 1, 2, body.size), (0, 3, body.size - 1)):
        rc = L.sp_db_export_rows(C.c_void_p(db.h), C.c_size_t(item0), C.c_size_t(count), body.ctypes.data_as(C.POINTER(C.c_uint8)),
                                 C.c_size_t(cap), C.byref(blen), C.byref(nrec))
        assert rc == SP_E_ARG and blen.value == 0 and nrec.value == 0 and (body == 0xCC).all()
    L.sp_db_export_rows_bound.restype = C.c_size_t
    assert L.sp_db_export_rows_bound(C.c_void_p(db.h), C.c_size_t(3)) == 3 * (8 + isz)
    assert db.export_rows(4, 3) == _body([(i, whole[i * isz:(i + 1) * isz]) for i in (4, 5, 6)])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_undecodable_words_are_counted_and_never_exported(sp, oracle_mod):
    """words the loader never writes, at the edges of its image: a coefficient h + 1 stored positive, the coefficient Q - (p - h), a
    word whose low limb is one valid item's and whose high limb another's (what a check of the low limb alone would let through), and
    an item of all-random words.  A bad coefficient behind the chunk's bytes (z >= W) is not looked at."""
    cfg = NARROW
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    npr, d0, isz, pt = o.num_per, o.dim0, o.db_item_size, 256
    h, W = pt // 2, (isz // 4) * 8 // 8
    blob = _file(o, _blob(o, seed=41))
    words = o.load_db_from_bytes(blob.tobytes()).reshape(4, N, npr, d0).copy()
    rng = np.random.default_rng(43)

    def poly(raw):
        w = o.to_ntt(np.asarray(raw, dtype=np.uint64)).reshape(2, N)
        return w[0] | (w[1] << np.uint64(32))

    def put(item, plane, col):
        words[plane, :, item % npr, item // npr] = col

    def col_of(item, plane):
        return words[plane, :, item % npr, item // npr].copy()

    def valid_raw():
        x = np.zeros(N, dtype=np.uint64)
        x[:W] = rng.integers(0, pt, W)
        return np.where(x > h, Q - (pt - x), x).astype(np.uint64)

    bad = {}                                                   # item -> undecodable planes
    raw = valid_raw(); raw[3] = h + 1; put(10, 1, poly(raw)); bad[10] = {1}
    raw = valid_raw(); raw[W - 1] = Q - (pt - h); put(77, 0, poly(raw)); bad[77] = {0}
    a, b = col_of(30, 2), col_of(31, 2)
    put(131, 2, (a & np.uint64(0xffffffff)) | (b & np.uint64(0xffffffff00000000))); bad[131] = {2}
    for pl in range(4):
        put(200, pl, rng.integers(0, Q0, N, dtype=np.uint64) | (rng.integers(0, Q1, N, dtype=np.uint64) << np.uint64(32)))
    bad[200] = {0, 1, 2, 3}
    raw = valid_raw(); raw[W] = h + 1; raw[N - 1] = Q // 2; good_tail = raw.copy(); put(90, 3, poly(raw))   # bad only behind the bytes
    db = sp.Database(p).load(words.reshape(-1))
    got, present, undecodable = db.read_items(0, o.num_items)
    assert undecodable == 1 + 1 + 1 + 4 and present.all()
    got = np.frombuffer(got, dtype=np.uint8).reshape(o.num_items, 4, isz // 4)
    want = blob.reshape(o.num_items, 4, isz // 4).copy()
    want[90, 3] = np.where(good_tail[:W] > h, good_tail[:W] + pt - Q, good_tail[:W]).astype(np.uint8)
    for i in range(o.num_items):
        for pl in range(4):
            if pl not in bad.get(i, ()):
                assert (got[i, pl] == want[i, pl]).all(), (i, pl)
    # the coefficient outside the image reads as 0, the polynomial's other coefficients as they are
    assert got[10, 1, 3] == 0 and got[77, 0, W - 1] == 0
    # a range without them is clean and exports; a range with one of them does not
    assert db.read_items(11, 60)[2] == 0 and db.read_items(10, 1)[2] == 1 and db.read_items(200, 1)[2] == 4
    assert db.export_rows(11, 60) == _body([(i, blob[i * isz:(i + 1) * isz]) for i in range(11, 71)])
    with pytest.raises(sp.SpiralError) as e:
        db.export_rows()
    assert e.value.rc == SP_E_STATE and e.value.body_len == 0
    synth = sp.Database(p).fill_synthetic(5)
    assert synth.read_items(0, o.num_items)[2] > 0           # SP_OK all the same
    with pytest.raises(sp.SpiralError) as e:
        synth.export_rows(0, 8)
    assert e.value.rc == SP_E_STATE and e.value.body_len == 0


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
_migration = {}


def _migration_case(oracle_mod):
    """the oracle's side of the migration, computed once: a sparse bucket of 256-byte items, two queries, lib/server's responses over
    the SparseDb and spiral-rs's over the dense database of the same file"""
    if not _migration:
        o = oracle_mod.Params(PACKED)
        recs = _sparse_records(o, seed=53)
        recs.append((recs[7][0], recs[8][1]))                 # an overwrite
        file = np.zeros((o.num_items, o.db_item_size), dtype=np.uint8)
        bucket = oracle_mod.SparseDb(o)
        for i, d in recs:
            file[i] = 0
            file[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
            bucket.update_item_raw(i, d)
        cl = oracle_mod.Client(o)
        pp = cl.generate_keys(71)
        idxs = [recs[9][0], (recs[9][0] + 1) % o.num_items]
        qs = [cl.generate_query(i, 500 + k) for k, i in enumerate(idxs)]
        words = o.load_db_from_bytes(file.tobytes())
        _migration.update(o=o, recs=recs, file=file, pp=pp, qs=qs, stored=sorted({i for i, _ in recs}),
                          sparse=[bucket.process_query(pp, q) for q in qs], dense=[o.process_query(pp, q, words) for q in qs])
    return _migration


def _migration_flow(kinds=("sparse", "packed", "planar", "words8")):
    def flow(sp, oracle_mod, S, arm):
        m = _migration_case(oracle_mod)
        o, file = m["o"], m["file"]
        arm()
        sp.paths_taken()
        p = S.params(PACKED)
        gpp = S.own(sp.PublicParameters.deserialize(p, m["pp"]))
        src = S.own(sp.Database.sparse(p))
        src.update_rows(_body(m["recs"]))
        got, present, undecodable = src.read_items(0, o.num_items)
        assert got == file.tobytes() and undecodable == 0 and np.nonzero(present)[0].tolist() == m["stored"]
        body = src.export_rows()
        assert body == _body([(i, file[i].tobytes()) for i in m["stored"]])
        assert [sp.process_query(p, gpp, q, src) for q in m["qs"]] == m["sparse"]
        dsts = {}
        for kind in kinds:
            if kind == "words8":
                with switch(sp, "db_unpacked", 1, default=0):
                    dst = S.own(sp.Database(p))
            else:
                dst = S.own({"sparse": sp.Database.sparse, "packed": sp.Database, "planar": sp.Database.planar}[kind](p))
            assert dst.format() == kind
            assert dst.update_rows(body)[0] == len(m["stored"])
            back, pres, und = dst.read_items(0, o.num_items)
            assert back == got and und == 0
            assert np.nonzero(pres)[0].tolist() == (m["stored"] if kind == "sparse" else list(range(o.num_items)))
            assert [sp.process_query(p, gpp, q, dst) for q in m["qs"]] == (m["sparse"] if kind == "sparse" else m["dense"]), kind
            dsts[kind] = dst
        if "packed" in dsts:                                   # dense to dense: PACKED to planar-resident
            moved = S.own(sp.Database.planar(p))
            moved.update_rows(dsts["packed"].export_rows())
            assert moved.read_items(0, o.num_items)[0] == got
            assert [sp.process_query(p, gpp, q, moved) for q in m["qs"]] == m["dense"]
        return sp.paths_taken()
    flow.__name__ = "readback_migration_" + "_".join(kinds)
    return flow


def test_export_rows_moves_a_bucket_between_formats(sp, oracle_mod):
    _migration_flow()(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_reads_beside_queries_on_one_handle(sp, oracle_mod):
    m = _migration_case(oracle_mod)
    o, file = m["o"], m["file"]
    p = sp.Params(PACKED)
    gpp = sp.PublicParameters.deserialize(p, m["pp"])
    db = sp.Database(p).load_items(file.tobytes())
    assert db.format() == "packed"
    out = {}

    def ask():
        out["responses"] = [sp.process_query(p, gpp, m["qs"][k % 2], db) for k in range(5)]

    def read():
        out["reads"] = [db.read_items(0, o.num_items) for _ in range(3)]

    threads = [threading.Thread(target=ask), threading.Thread(target=read)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out["responses"] == [m["dense"][k % 2] for k in range(5)]
    for got, present, undecodable in out["reads"]:
        assert got == file.tobytes() and present.all() and undecodable == 0


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["poison", "guard"])
@pytest.mark.parametrize("what", ["formats-packed", "formats-planar", "formats-sparse", "migration"])
def test_on_hardened_buffers(oracle_mod, capfd, what, mode):
    """poison_ws = 0xA5 and guard_ws = 1 MiB act when a buffer is allocated: the flow computes the oracle's side, sets the switch, makes
    its own handles -- the read buffer among their allocations -- and lets go of every one before stderr is read"""
    from test_gpu_hardened_buffers import POISON, _hardened
    flow = _migration_flow(("sparse", "packed", "planar")) if what == "migration" else _formats_flow(what.split("-")[1])
    _hardened(flow, mode, POISON, oracle_mod, capfd)
