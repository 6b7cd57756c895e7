"""Per-item digests (sp_db_item_digests): one pair of 64-bit sums per item over the resident words, the same on every format.
Every expected value comes from the numpy restatement of tests/item_digest_reference.py, never from the library; every comparison is
exact equality of 64-bit words.  The shapes are those of tests/test_gpu_db_digest.py.

1  synthetic words on every dense form (PACKED of one and two chunks, 8-byte words, the one-row shard, a PACKED column shard, a planar
   handle, a planar row shard) == numpy over sp.synth_words for the held items, zeros with present 0 elsewhere; lane sums == the sum of
   db.digest over the planes.
2  one /update-row body on every format and shard split: equal unsharded tables == numpy over the oracle's words; shard sets add up to
   it with present flags that partition the held items; the sparse bucket's flags are the body's indices, a stored all-zero item among
   them.
3  locality: one word 1 at the two far corners through load_plane on zeros (dense forms) moves exactly its item, == R_l(j) * A_l(c); a
   sparse bucket takes no raw words, there the two corner ITEMS are stored and every other item stays (0, 0), present 0; one changed
   byte through update_item moves exactly one item in both lanes, and moves it back.
4  ranges (item0 inside a row, ends inside a row, inside one row, one item, the last item, count = 0), plane sub-ranges with additivity
   against db.digest(plane0, nplanes), and a range cut into several windows by a small db_load_window.
5  the batch copy: equal to the resident table after prepare_batch and after an upsert patched it; SP_E_STATE, output untouched, once a
   bulk load dropped it and on handles that have none.
6  every SP_E_ARG case leaves sentinel-filled out and present untouched.
7  repair end to end: differing_items names exactly the missed and the damaged records; after repair_from tables, digests and a
   query's response agree; sparse -> PACKED; unsharded -> two row shards.
8  cases 1, 2 and 5 on poisoned and on guarded buffers (the procedure of tests/test_gpu_hardened_buffers.py).
9  a table beside a running list of 8 on one handle == the table taken when idle.
tests/test_emulated_item_digests.py runs a subset on the emulated device."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

from conftest import FAST
from db_digest_reference import N, wrapping_sum
from item_digest_reference import item_digests, item_digests_plane, lane_sums, unit_item
from test_gpu_planar_shards import _cfg as _planar_cfg

pytestmark = pytest.mark.gpu

SP_E_ARG, SP_E_STATE = -1, -4
SEED = 0x5EED
SENTINEL = 0xCCCCCCCCCCCCCCCC
PACKED_1CHUNK = dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=256)     # 2 row pairs, one chunk
PACKED_2CHUNKS = dict(FAST, nu_1=3, nu_2=8, t_gsw=2, db_item_size=256)    # 4 row pairs, two chunks
WORDS8 = dict(FAST, nu_1=4, nu_2=1, db_item_size=256)                     # 16 x 2: 8-byte words
ONE_ROW = dict(FAST, nu_1=1, nu_2=7, t_gsw=1, db_item_size=256)           # its row shard 1 of 2 holds one row
EVERY = _planar_cfg(7, 7)                                                 # 128 x 128, 256-byte items
COPY = dict(FAST, nu_1=6, nu_2=7, db_item_size=256)                       # 64 x 128: PACKED words with a digit-planar copy
SPARSE_SMALL = dict(FAST, nu_1=6, nu_2=3, db_item_size=256)


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _planes(p):
    return p.instances * p.n * p.n


def _body(records):
    return b"".join(struct.pack(">II", 4 + len(d), i) + bytes(d) for i, d in records)


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1, 2), np.asarray(want, dtype=np.uint64).reshape(-1, 2)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "%d items differ, first %d: %s != %s" % (bad.size, bad[0], [hex(int(x)) for x in got[bad[0]]],
                                                                          [hex(int(x)) for x in want[bad[0]]]))


def _add(tables):
    with np.errstate(over="ignore"):
        total = np.zeros_like(tables[0])
        for t in tables:
            total = total + t
    return total


def _digest_sums(db, seed, **kw):
    return tuple(int(x) for x in wrapping_sum(list(db.digest(seed, **kw))))


def _synth_plane(sp, seed, plane, num_per, dim0, j0=0, nj=None, cols=None):
    """sp_synth_word over the reference indices of one plane -> [N][num_per][nj]; `cols`: the other columns read as zero"""
    nj = dim0 - j0 if nj is None else nj
    zi = (np.uint64(plane * N) + np.arange(N, dtype=np.uint64))[:, None] * np.uint64(num_per) + np.arange(num_per, dtype=np.uint64)[None, :]
    ref = zi[:, :, None] * np.uint64(dim0) + np.uint64(j0) + np.arange(nj, dtype=np.uint64)[None, None, :]
    w = sp.spiral.synth_words(seed, ref)
    if cols is not None:
        keep = np.zeros(num_per, dtype=bool)
        keep[cols] = True
        w = np.where(keep[None, :, None], w, np.uint64(0))
    return w


_synth_cache = {}


def _synth_tables(sp, cfg, p, j0=0, nj=None):
    """numpy tables of sp_synth_word(SEED, .) under the digest seed SEED + 1, one per plane, rows j0 .. j0 + nj - 1 (the others zero);
    computed once per shape and left unchanged"""
    key = (tuple(sorted(cfg.items())), j0, nj)
    if key not in _synth_cache:
        _synth_cache[key] = [item_digests_plane(SEED + 1, k, _synth_plane(sp, SEED, k, p.num_per, p.dim0, j0, nj), p.num_per, p.dim0, j0=j0)
                             for k in range(_planes(p))]
        for t in _synth_cache[key]:
            t.setflags(write=False)
    return _synth_cache[key]


class _Own:
    """the handles of a flow outside the hardened runs"""

    def __init__(self, sp):
        self.sp, self.objs = sp, []

    def own(self, obj):
        self.objs.append(obj)
        return obj

    def params(self, cfg):
        return self.own(self.sp.Params(cfg))


def _no_switch():
    return 0


def _unpacked(sp, make):
    """make() with the switch db_unpacked set: an 8-byte handle at a shape that would pack.  Set through sp_debug_set, as the other
    files set it: a value an earlier test left there shadows the environment"""
    from test_gpu_narrow_batch import switch
    with switch(sp, "db_unpacked", 1, default=0):
        db = make()
    assert db.format() == "words8"
    return db


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
# name -> (config, shard, shards, kind, format)
SYNTH = {"packed-2pairs-1chunk": (PACKED_1CHUNK, 0, 1, "rows", "packed"), "packed-4pairs-2chunks": (PACKED_2CHUNKS, 0, 1, "rows", "packed"),
         "words8-16x2": (WORDS8, 0, 1, "rows", "words8"), "one-row-shard": (ONE_ROW, 1, 2, "rows", "words8"),
         "packed-column-shard": (PACKED_2CHUNKS, 1, 2, "columns", "packed"), "planar-64x128": (COPY, 0, 1, "planar", "planar"),
         "planar-shard-128x128": (EVERY, 1, 2, "planar-shard", "planar")}


def _synth_flow(name):
    def flow(sp, oracle_mod, S, arm):
        cfg, s, G, kind, fmt = SYNTH[name]
        arm()
        sp.paths_taken()
        p = S.params(cfg)
        D = sp.Database
        db = S.own(D.planar(p) if kind == "planar" else D.planar_shard(p, s, G) if kind == "planar-shard" else
                   D(p, s, G, by_columns=kind == "columns")).fill_synthetic(SEED)
        assert db.format() == fmt
        got, present = db.item_digests(SEED + 1)
        n_items = p.dim0 * p.num_per
        assert got.shape == (n_items, 2) and got.dtype == np.uint64 and present.shape == (n_items,) and present.dtype == np.uint8
        j0, nj, cols = (0, p.dim0, list(range(s, p.num_per, G))) if kind == "columns" else (s * (p.dim0 // G), p.dim0 // G, None)
        held = np.zeros((p.dim0, p.num_per), dtype=np.uint8)
        held[j0:j0 + nj, cols if cols is not None else slice(None)] = 1
        # an item's pair depends on its own words alone: a column shard's table is the unsharded one with the other columns zero
        want = _add(_synth_tables(sp, cfg, p, j0, nj)) * held.reshape(-1, 1).astype(np.uint64)
        _same(got, want, name)
        assert (present == held.reshape(-1)).all(), name
        assert got[present == 1].all() and not got[present == 0].any()
        assert lane_sums(got) == _digest_sums(db, SEED + 1), name
        return sp.paths_taken()
    flow.__name__ = "item_digests_synthetic_" + name
    return flow


@pytest.mark.parametrize("name", list(SYNTH))
def test_synthetic_words(sp, oracle_mod, name):
    _synth_flow(name)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
_every = {}
EMPTY_COLUMN = 5


def _every_case(oracle_mod):
    """the one contents of case 2, computed once: about 200 records of one /update-row body, one of them all zero bytes, and the numpy
    table over the oracle's words for the same items (SparseDb.to_dense: zero polynomials for the absent ones)"""
    if not _every:
        o = oracle_mod.Params(EVERY)
        npr, n_items = o.num_per, o.num_items
        rng = np.random.default_rng(41)
        forced = [0, n_items - 1,
                  10 * npr + 20, 11 * npr + 21,          # two items of one quad (row pair 5, columns 20 and 21)
                  32 * npr + 77, 37 * npr + 77,          # two items of one 16-row group of column 77
                  70 * npr + 3]                          # stored, all zero bytes
        idx = set(forced)
        while len(idx) < 200:
            i = int(rng.integers(0, n_items))
            if i % npr != EMPTY_COLUMN:
                idx.add(i)
        recs = [(i, bytes(o.db_item_size) if i == 70 * npr + 3 else rng.integers(0, 256, o.db_item_size, dtype=np.uint8).tobytes())
                for i in sorted(idx)]
        bucket = oracle_mod.SparseDb(o)
        for i, d in recs:
            bucket.update_item_raw(i, d)
        dense = bucket.to_dense().reshape(-1, N, npr, o.dim0)
        want = item_digests(SEED, list(dense), npr, o.dim0)
        del dense
        stored = np.zeros(n_items, dtype=np.uint8)
        stored[[i for i, _ in recs]] = 1
        assert not want[70 * npr + 3].any() and want[stored == 1].any(axis=1).sum() == len(recs) - 1 and not want[stored == 0].any()
        _every.update(o=o, recs=recs, body=_body(recs), want=want, stored=stored, zero_item=70 * npr + 3)
    return _every


# format -> shards
EVERY_FORMATS = {"packed": 1, "words8": 1, "planar": 1, "sparse": 1, "packed-row-shards-2": 2, "packed-row-shards-4": 4, "column-shards-2": 2,
                 "column-shards-4": 4, "planar-shards-2": 2, "sparse-shards-2": 2, "sparse-shards-4": 4}


def _every_handle(sp, S, p, fmt, s, G):
    D = sp.Database
    if fmt == "packed" or fmt.startswith("packed-row-shards"):
        return S.own(D(p, s, G))
    if fmt == "words8":
        return S.own(_unpacked(sp, lambda: D(p)))
    if fmt == "planar":
        return S.own(D.planar(p))
    if fmt.startswith("column-shards"):
        return S.own(D(p, s, G, by_columns=True))
    if fmt.startswith("planar-shards"):
        return S.own(D.planar_shard(p, s, G))
    return S.own(D.sparse(p, s, G))


def _every_tables(sp, S, p, m, fmt):
    """the body applied to the handles of `fmt`, created and freed one after another -> [(table, present)] per shard"""
    parts = []
    for s in range(EVERY_FORMATS[fmt]):
        db = _every_handle(sp, S, p, fmt, s, EVERY_FORMATS[fmt])
        assert db.update_rows(m["body"])[0] == len(m["recs"])
        t, pr = db.item_digests(SEED)
        assert lane_sums(t) == _digest_sums(db, SEED), (fmt, s)
        parts.append((t.copy(), pr.copy()))
        S.objs.remove(db)
        db.__del__()
    return parts


def _every_flow(fmts):
    def flow(sp, oracle_mod, S, arm):
        m = _every_case(oracle_mod)
        arm()
        sp.paths_taken()
        p = S.params(EVERY)
        for fmt in fmts:
            parts = _every_tables(sp, S, p, m, fmt)
            _same(_add([t for t, _ in parts]), m["want"], (fmt, "against the oracle's words"))
            held = np.sum([pr.astype(np.int64) for _, pr in parts], axis=0)
            if "sparse" in fmt:      # the store: exactly the body's indices, the all-zero item among them, each in one shard
                assert (held == m["stored"]).all(), fmt
                assert all(not t[m["zero_item"]].any() for t, _ in parts) and held[m["zero_item"]] == 1
            else:                    # a dense handle holds the items of its rows and columns: the shards partition all items
                assert (held == 1).all(), fmt
            for t, pr in parts:
                assert not t[pr == 0].any(), fmt
        return sp.paths_taken()
    flow.__name__ = "item_digests_every_" + "_".join(fmts)
    return flow


@pytest.mark.parametrize("fmt", list(EVERY_FORMATS))
def test_one_body_every_format(sp, oracle_mod, fmt):
    _every_flow((fmt,))(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
CORNER = {"packed": (PACKED_2CHUNKS, lambda sp, p: sp.Database(p)), "words8": (WORDS8, lambda sp, p: sp.Database(p)),
          "planar": (COPY, lambda sp, p: sp.Database.planar(p)),
          "column-shard": (PACKED_2CHUNKS, lambda sp, p: sp.Database(p, 1, 2, by_columns=True)),
          "planar-shard": (EVERY, lambda sp, p: sp.Database.planar_shard(p, 1, 2))}


@pytest.mark.parametrize("name", list(CORNER))
def test_corner_words(sp, name):
    cfg, make = CORNER[name]
    p = sp.Params(cfg)
    planes, npr, dim0 = _planes(p), p.num_per, p.dim0
    db = make(sp, p)
    t, _ = db.item_digests(SEED)
    assert not t.any(), "a fresh handle"
    for plane, z, ii, j in ((planes - 1, N - 1, npr - 1, dim0 - 1), (0, 0, 0, 0)):
        row = np.zeros((1, npr, dim0), dtype=np.uint64)
        row[0, ii, j] = 1
        db.load_plane(plane, z, 1, row)
        t, _ = db.item_digests(SEED)
        holds = not (name == "column-shard" and ii % 2 != 1) and not (name == "planar-shard" and j < dim0 // 2)
        want = np.zeros((dim0 * npr, 2), dtype=np.uint64)
        if holds:
            want[j * npr + ii] = unit_item(SEED, plane, z, ii, j, npr, dim0)
            assert want[j * npr + ii].all()
        _same(t, want, (name, plane, z, ii, j))
        db.load_plane(plane, z, 1, np.zeros((1, npr, dim0), dtype=np.uint64))
    assert not db.item_digests(SEED)[0].any()


def test_corner_items_sparse(sp, oracle_mod):
    o, p = oracle_mod.Params(SPARSE_SMALL), sp.Params(SPARSE_SMALL)
    rng = np.random.default_rng(71)
    recs = [(i, rng.integers(0, 256, o.db_item_size, dtype=np.uint8).tobytes()) for i in (0, o.num_items - 1)]
    bucket = oracle_mod.SparseDb(o)
    db = sp.Database.sparse(p)
    for i, d in recs:
        bucket.update_item_raw(i, d)
        db.update_item(i, d)
    want = item_digests(SEED, list(bucket.to_dense().reshape(-1, N, o.num_per, o.dim0)), o.num_per, o.dim0)
    t, pr = db.item_digests(SEED)
    _same(t, want, "sparse corners")
    assert np.flatnonzero(pr).tolist() == [0, o.num_items - 1] and t[0].all() and t[-1].all() and not t[1:-1].any()


@pytest.mark.parametrize("fmt", ["packed", "words8", "planar", "sparse"])
def test_one_byte_moves_one_item(sp, oracle_mod, fmt):
    m = _every_case(oracle_mod)
    p = sp.Params(EVERY)
    db = _every_handle(sp, _Own(sp), p, fmt, 0, 1)
    db.update_rows(m["body"])
    before, pr = db.item_digests(SEED)
    _same(before, m["want"], fmt)
    idx, data = m["recs"][17]
    edited = bytearray(data)
    edited[70] ^= 0x10
    db.update_item(idx, bytes(edited))
    after, pr2 = db.item_digests(SEED)
    assert sp.differing_items((before, pr), (after, pr2)).tolist() == [idx]
    assert after[idx, 0] != before[idx, 0] and after[idx, 1] != before[idx, 1]
    db.update_item(idx, data)
    _same(db.item_digests(SEED)[0], before, (fmt, "the old bytes back"))
    stored = before.any(axis=1)
    assert (db.item_digests(SEED + 2)[0][stored] != before[stored]).all()   # another seed is another table


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
RANGES = {"packed": (PACKED_2CHUNKS, "dense"), "words8": (WORDS8, "dense"), "planar": (COPY, "planar"), "sparse": (SPARSE_SMALL, "sparse")}


@pytest.mark.parametrize("fmt", list(RANGES))
def test_ranges(sp, fmt):
    cfg, kind = RANGES[fmt]
    p = sp.Params(cfg)
    planes, npr, dim0 = _planes(p), p.num_per, p.dim0
    n_items, DS = npr * dim0, SEED + 1
    if kind == "sparse":
        rng = np.random.default_rng(73)
        db = sp.Database.sparse(p)
        idx = sorted({0, 1, npr - 1, npr, 3 * npr + 2, n_items - 1} | {int(i) for i in rng.integers(0, n_items, 60)})
        db.update_items([(i, rng.integers(0, 256, 256, dtype=np.uint8).tobytes()) for i in idx])
        whole, wp = db.item_digests(DS)          # (== numpy: test_one_body_every_format and test_corner_items_sparse)
        per_plane = [db.item_digests(DS, plane0=k, nplanes=1)[0] for k in range(planes)]
        assert np.flatnonzero(wp).tolist() == idx
    else:
        db = (sp.Database.planar(p) if kind == "planar" else sp.Database(p)).fill_synthetic(SEED)
        per_plane = _synth_tables(sp, cfg, p, 0, dim0)
        whole, wp = _add(per_plane), np.ones(n_items, dtype=np.uint8)
    assert db.format() == fmt
    ranges = [(npr // 2 + 1, 2 * npr), (0, npr + npr // 2), (npr + 1, max(1, npr // 2 - 1)), (2 * npr + 1, 1), (n_items - 1, 1), (3, 0),
              (n_items, 0), (0, n_items), ((dim0 - 3) * npr + 1, 3 * npr - 1), (npr, npr)]
    for item0, count in ranges:
        t, pr = db.item_digests(DS, item0, count)
        assert t.shape == (count, 2) and pr.shape == (count,)
        _same(t, whole[item0:item0 + count], (fmt, item0, count))
        assert (pr == wp[item0:item0 + count]).all(), (fmt, item0, count)
    for plane0, n in ((0, 1), (1, 2), (planes - 1, 1), (0, planes), (1, planes - 1)):
        t, pr = db.item_digests(DS, npr - 1, 2 * npr + 3, plane0=plane0, nplanes=n)
        _same(t, _add(per_plane[plane0:plane0 + n])[npr - 1:3 * npr + 2], (fmt, "planes", plane0, n))
        full = db.item_digests(DS, plane0=plane0, nplanes=n)[0]
        _same(full, _add(per_plane[plane0:plane0 + n]), (fmt, "planes", plane0, n, "whole"))
        assert lane_sums(full) == _digest_sums(db, DS, plane0=plane0, nplanes=n)
    assert db.item_digests(DS, 0, 5, plane0=planes, nplanes=0)[0].shape == (5, 2)
    # windows: a table of 16 bytes per item and a db_load_window of 1.5 rows' worth cut every range into windows of one row
    sp.lib().sp_debug_set(b"db_load_window", C.c_long(24 * npr + 64))
    try:
        for item0, count in ranges[:3] + [(0, n_items), ((dim0 - 3) * npr + 1, 3 * npr - 1)]:
            t, pr = db.item_digests(DS, item0, count)
            _same(t, whole[item0:item0 + count], (fmt, "windows", item0, count))
            assert (pr == wp[item0:item0 + count]).all()
    finally:
        sp.lib().sp_debug_set(b"db_load_window", C.c_long(512 << 20))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _copy_records(o, seed=61):
    rng = np.random.default_rng(seed)
    idx = sorted({0, o.num_items - 1} | {int(i) for i in rng.integers(0, o.num_items, 40)})
    return [(i, rng.integers(0, 256, o.db_item_size, dtype=np.uint8).tobytes()) for i in idx]


def _copy_flow(sp, oracle_mod, S, arm):
    o = oracle_mod.Params(COPY)
    blob = np.random.default_rng(59).integers(0, 256, o.num_items * o.db_item_size, dtype=np.uint8)
    recs = _copy_records(o)
    arm()
    sp.paths_taken()
    p = S.params(COPY)
    db = S.own(sp.Database(p)).load_items(blob)
    assert db.format() == "packed"
    L, u64p, u8p = sp.lib(), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)

    def refused(h):
        out, pres = np.full(2 * o.num_items, SENTINEL, dtype=np.uint64), np.full(o.num_items, 0xCC, dtype=np.uint8)
        rc = L.sp_db_item_digests(C.c_void_p(h.h), C.c_uint64(SEED), C.c_int(1), C.c_int(0), C.c_int(_planes(p)), C.c_size_t(0),
                                  C.c_size_t(o.num_items), out.ctypes.data_as(u64p), pres.ctypes.data_as(u8p))
        assert rc == SP_E_STATE and (out == SENTINEL).all() and (pres == 0xCC).all()
        with pytest.raises(sp.SpiralError) as e:
            h.item_digests(SEED, which="batch_copy")
        assert e.value.rc == SP_E_STATE

    refused(db)                                     # no copy yet, and the call never builds one
    assert db.batch_copy_bytes() == 0
    assert db.prepare_batch() is True
    resident, pr = db.item_digests(SEED)
    assert resident.all() and pr.all()
    t, cp = db.item_digests(SEED, which="batch_copy")
    _same(t, resident, "after the build")
    assert cp.all()
    db.update_items(recs)
    assert db.batch_copy_bytes() > 0
    patched = db.item_digests(SEED)[0]
    assert sp.differing_items((patched, pr), (resident, pr)).tolist() == [i for i, _ in recs]
    _same(db.item_digests(SEED, which="batch_copy")[0], patched, "after update_items patched the copy")
    _same(db.item_digests(SEED, 130, 300, which="batch_copy", plane0=1, nplanes=2)[0],
          db.item_digests(SEED, 130, 300, plane0=1, nplanes=2)[0], "a range of planes 1, 2 of the copy")
    assert lane_sums(db.item_digests(SEED, which="batch_copy", plane0=1, nplanes=2)[0]) == \
        _digest_sums(db, SEED, which="batch_copy", plane0=1, nplanes=2)
    # the same items on a planar-resident handle: the same table, and no batch copy to speak of
    planar = S.own(sp.Database.planar(p)).load_items(blob)
    planar.update_items(recs)
    _same(planar.item_digests(SEED)[0], patched, "planar-resident")
    sparse = S.own(sp.Database.sparse(p))
    sparse.update_items(recs[:3])
    for other in (planar, sparse):
        refused(other)
    db.load_items(blob)                             # a bulk load drops the copy
    assert db.batch_copy_bytes() == 0
    refused(db)
    _same(db.item_digests(SEED)[0], resident, "the first contents again")
    return sp.paths_taken()


def test_batch_copy(sp, oracle_mod):
    _copy_flow(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(sp):
    p = sp.Params(WORDS8)
    db = sp.Database(p).fill_synthetic(3)
    planes, n_items = _planes(p), p.dim0 * p.num_per
    L, u64p, u8p = sp.lib(), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)

    def call(h, which, plane0, nplanes, item0, count, out, pres):
        return L.sp_db_item_digests(h, C.c_uint64(SEED), C.c_int(which), C.c_int(plane0), C.c_int(nplanes), C.c_size_t(item0),
                                    C.c_size_t(count), None if out is None else out.ctypes.data_as(u64p),
                                    None if pres is None else pres.ctypes.data_as(u8p))

    for which, plane0, nplanes, item0, count, null_out in (
            (0, -1, 1, 0, 4, False), (0, planes - 1, 2, 0, 4, False), (0, planes + 1, 0, 0, 4, False), (0, 0, -1, 0, 4, False),
            (0, 0, 2 ** 31 - 1, 0, 4, False), (0, 0, 1, 0, 4, True), (2, 0, 1, 0, 4, False), (-1, 0, 1, 0, 4, False),
            (0, 0, 1, n_items, 1, False), (0, 0, 1, 1, n_items, False), (0, 0, 1, n_items + 1, 0, False), (0, 0, 1, 2 ** 64 - 1, 2, False)):
        out, pres = np.full(2 * n_items + 4, SENTINEL, dtype=np.uint64), np.full(n_items + 4, 0xCC, dtype=np.uint8)
        rc = call(C.c_void_p(db.h), which, plane0, nplanes, item0, count, None if null_out else out, pres)
        assert rc == SP_E_ARG, (which, plane0, nplanes, item0, count, null_out)
        assert (out == SENTINEL).all() and (pres == 0xCC).all()
    out, pres = np.full(8, SENTINEL, dtype=np.uint64), np.full(4, 0xCC, dtype=np.uint8)
    assert call(None, 0, 0, 1, 0, 1, out, pres) == SP_E_ARG
    assert call(C.c_void_p(db.h), 0, planes, 0, 0, 4, out, pres) == 0        # no planes
    assert call(C.c_void_p(db.h), 0, 0, 1, n_items, 0, out, pres) == 0       # no items
    assert call(C.c_void_p(db.h), 0, 0, 0, 0, 0, None, None) == 0
    assert (out == SENTINEL).all() and (pres == 0xCC).all()
    # two items write two pairs and two flags and nothing behind them; present may be null
    assert call(C.c_void_p(db.h), 0, 0, planes, 5, 2, out, pres) == 0
    assert (out[:4] != SENTINEL).all() and (out[4:] == SENTINEL).all() and pres.tolist() == [1, 1, 0xCC, 0xCC]
    _same(out[:4], db.item_digests(SEED)[0][5:7])
    again = np.full(8, SENTINEL, dtype=np.uint64)
    assert call(C.c_void_p(db.h), 0, 0, planes, 5, 2, again, None) == 0 and (again == out).all()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def _repair_case(oracle_mod):
    m = _every_case(oracle_mod)
    recs = m["recs"]
    missed = [recs[3][0], recs[90][0], recs[-1][0]]
    flipped = recs[40][0]
    damaged = []
    for i, d in recs:
        if i in missed:
            continue
        if i == flipped:
            d = bytearray(d)
            d[11] ^= 0x01
        damaged.append((i, bytes(d)))
    return m, sorted(missed + [flipped]), _body(damaged)


def _query_bytes(sp, oracle_mod, p, o, db, idx, decode=False):
    cl = oracle_mod.Client(o)
    gpp = sp.PublicParameters.deserialize(p, cl.generate_keys(83))
    r = sp.process_query(p, gpp, cl.generate_query(idx, 901), db)
    return bytes(cl.decode_response(r))[:o.db_item_size] if decode else r


@pytest.mark.parametrize("pair", ["packed-packed", "sparse-packed", "sparse-sparse"])
def test_repair_end_to_end(sp, oracle_mod, pair):
    m, bad, damaged = _repair_case(oracle_mod)
    p = sp.Params(EVERY)
    make = {"packed": lambda: sp.Database(p), "sparse": lambda: sp.Database.sparse(p)}
    A, B = (make[k]() for k in pair.split("-"))
    A.update_rows(m["body"])
    B.update_rows(damaged)
    ta, tb = A.item_digests(SEED), B.item_digests(SEED)
    diff = sp.differing_items(ta, tb).tolist()
    if pair == "sparse-packed":     # a dense handle holds every item: presence differs wherever the bucket stores nothing
        assert sorted(set(diff) & set(np.flatnonzero(m["stored"]).tolist())) == bad
        assert np.flatnonzero((ta[0] != tb[0]).any(axis=1)).tolist() == bad
    else:
        assert diff == bad
    repaired, gone = B.repair_from(A, SEED)
    assert repaired.tolist() == bad and gone.size == (0 if pair != "sparse-packed" else int((m["stored"] == 0).sum()))
    _same(B.item_digests(SEED)[0], ta[0], pair)
    _same(B.digest(SEED), A.digest(SEED), pair)
    if pair != "sparse-packed":
        assert sp.differing_items(A.item_digests(SEED), B.item_digests(SEED)).size == 0
    if pair == "sparse-packed":
        # a sparse bucket and a dense database answer with different noise (the bucket's expansion is pruned to its rows), so the
        # response BYTES are compared with a PACKED handle that took the whole body, and the bucket's answer by what it decodes to
        A2 = sp.Database(p)
        A2.update_rows(m["body"])
        assert _query_bytes(sp, oracle_mod, p, m["o"], A2, bad[1]) == _query_bytes(sp, oracle_mod, p, m["o"], B, bad[1])
        item = dict(m["recs"])[bad[1]]
        assert _query_bytes(sp, oracle_mod, p, m["o"], A, bad[1], decode=True) == item == \
            _query_bytes(sp, oracle_mod, p, m["o"], B, bad[1], decode=True)
    else:
        assert _query_bytes(sp, oracle_mod, p, m["o"], A, bad[1]) == _query_bytes(sp, oracle_mod, p, m["o"], B, bad[1])


def test_repair_row_shards_from_unsharded(sp, oracle_mod):
    m, bad, damaged = _repair_case(oracle_mod)
    p = sp.Params(EVERY)
    A = sp.Database(p)
    A.update_rows(m["body"])
    ta = A.item_digests(SEED)
    shards = [sp.Database(p, s, 2) for s in range(2)]
    half = p.dim0 * p.num_per // 2
    for s, B in enumerate(shards):
        B.update_rows(damaged)
        tb = B.item_digests(SEED)
        mine = [i for i in bad if s * half <= i < (s + 1) * half]
        held = np.flatnonzero(tb[1])
        assert held.tolist() == list(range(s * half, (s + 1) * half))
        assert [i for i in sp.differing_items(ta, tb).tolist() if tb[1][i]] == mine
        repaired, gone = B.repair_from(A, SEED)
        assert gone.size == 0 and [i for i in repaired.tolist() if tb[1][i]] == mine
    _same(_add([B.item_digests(SEED)[0] for B in shards]), ta[0], "two row shards")
    _same(wrapping_sum([B.digest(SEED) for B in shards]), A.digest(SEED))


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
HARDENED = {"synthetic-packed": _synth_flow("packed-2pairs-1chunk"), "synthetic-words8": _synth_flow("words8-16x2"),
            "synthetic-planar": _synth_flow("planar-64x128"), "every-packed": _every_flow(("packed",)),
            "every-planar": _every_flow(("planar",)), "every-sparse": _every_flow(("sparse",)), "batch-copy": _copy_flow}


@pytest.mark.parametrize("mode", ["poison", "guard"])
@pytest.mark.parametrize("what", list(HARDENED))
def test_on_hardened_buffers(oracle_mod, capfd, what, mode):
    """poison_ws = 0xA5 and guard_ws = 1 MiB act when a buffer is allocated: the flow computes its references, sets the switch, makes
    its own handles -- the read buffer with the table, the row keys, the flags and the slot list among their allocations -- and lets
    go of every one before stderr is read"""
    from test_gpu_hardened_buffers import POISON, _hardened
    _hardened(HARDENED[what], mode, POISON, oracle_mod, capfd)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_table_beside_a_running_list(sp, oracle_mod):
    o, p = oracle_mod.Params(COPY), sp.Params(COPY)
    blob = np.random.default_rng(59).integers(0, 256, o.num_items * o.db_item_size, dtype=np.uint8)
    cl = oracle_mod.Client(o)
    gpp = sp.PublicParameters.deserialize(p, cl.generate_keys(83))
    qs = [cl.generate_query((37 * k + 5) % o.num_items, 900 + k) for k in range(8)]
    db = sp.Database(p).load_items(blob)
    alone = sp.process_query_batch(p, [gpp] * 8, qs, db)
    want = db.item_digests(SEED)[0].copy()
    assert want.all()
    out, done = {"tables": []}, threading.Event()

    def ask():
        try:
            out["responses"] = sp.process_query_batch(p, [gpp] * 8, qs, db)
        finally:
            done.set()

    def digest():
        while len(out["tables"]) < 20:
            out["tables"].append(db.item_digests(SEED)[0].copy())
            if done.is_set():
                break

    threads = [threading.Thread(target=ask), threading.Thread(target=digest)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out["responses"] == alone
    assert 1 <= len(out["tables"]) <= 20
    for t in out["tables"]:
        _same(t, want)
