"""The database digest (sp_db_digest): one pair of 64-bit sums per plane over the resident words, the same on every format.
Every expected value comes from the numpy restatement of tests/db_digest_reference.py, never from the library.

1  synthetic words on PACKED (one and two chunks, a column shard) and 8-byte handles (a row shard of one row among them) == numpy over
   sp.synth_words.
2  loaded words with limbs >= q == numpy over the limb-wise reduced words == digest_ref_words over two z-ranges.
3  one /update-row body on every format and shard split: equal unsharded digests, shard sets that add up to them, plane 1 pinned to
   numpy over the oracle's words for the same items.
4  fresh handles of every format digest to zeros.
5  one changed byte moves exactly its chunk's plane, in both lanes, and moves it back; sub-ranges of planes.
6  the digit-planar copy beside a PACKED database: equal to the resident digest after the build and after an upsert patched it,
   SP_E_STATE once a bulk load dropped it and on handles that have none.
7  the SP_E_ARG cases write nothing.
8  cases 1, 3 and 6 on poisoned and on guarded buffers (the procedure of tests/test_gpu_hardened_buffers.py).
9  digests beside a running list of 8 on one handle.
tests/test_emulated_db_digest.py runs a subset on the emulated device."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

from conftest import FAST
from db_digest_reference import N, Q0, Q1, canon, digest_plane, wrapping_sum
from test_gpu_planar_shards import _cfg as _planar_cfg

pytestmark = pytest.mark.gpu

SP_E_ARG, SP_E_STATE = -1, -4
SEED = 0x5EED
SENTINEL = 0xCCCCCCCCCCCCCCCC
PACKED_1CHUNK = dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=256)     # 2 row pairs, one chunk
PACKED_2CHUNKS = dict(FAST, nu_1=3, nu_2=8, t_gsw=2, db_item_size=256)    # 4 row pairs, two chunks
WORDS8 = dict(FAST, nu_1=4, nu_2=1, db_item_size=256)                     # 16 x 2: 8-byte words
ONE_ROW = dict(FAST, nu_1=1, nu_2=7, t_gsw=1, db_item_size=256)           # its row shard 1 of 2 holds one row: the odd-count 8-byte form
EVERY = _planar_cfg(7, 7)                                                 # 128 x 128, t_gsw = 4, query expansion, 256-byte items
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


def _hex(d):
    return [[hex(int(x)) for x in row] for row in np.asarray(d).reshape(-1, 2)]


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1, 2), np.asarray(want, dtype=np.uint64).reshape(-1, 2)
    assert got.shape == want.shape and (got == want).all(), (what, _hex(got), _hex(want))


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


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
# name -> (config, shard, shards, by columns, format)
SYNTH = {"packed-2pairs-1chunk": (PACKED_1CHUNK, 0, 1, False, "packed"), "packed-4pairs-2chunks": (PACKED_2CHUNKS, 0, 1, False, "packed"),
         "words8-16x2": (WORDS8, 0, 1, False, "words8"), "one-row-shard": (ONE_ROW, 1, 2, False, "words8"),
         "packed-column-shard": (PACKED_2CHUNKS, 1, 2, True, "packed")}


def _synth_flow(name):
    def flow(sp, oracle_mod, S, arm):
        cfg, s, G, by_columns, fmt = SYNTH[name]
        arm()
        sp.paths_taken()
        p = S.params(cfg)
        db = S.own(sp.Database(p, s, G, by_columns=by_columns)).fill_synthetic(SEED)
        assert db.format() == fmt
        got = db.digest(SEED + 1)
        assert got.shape == (_planes(p), 2) and got.dtype == np.uint64
        j0, nj, cols = (0, p.dim0, list(range(s, p.num_per, G))) if by_columns else (s * (p.dim0 // G), p.dim0 // G, None)
        for plane in range(_planes(p)):
            words = _synth_plane(sp, SEED, plane, p.num_per, p.dim0, j0, nj, cols)
            _same(got[plane], digest_plane(SEED + 1, plane, words, N, p.num_per, p.dim0, j0), (name, plane))
        assert got.any()
        return sp.paths_taken()
    flow.__name__ = "digest_synthetic_" + name
    return flow


@pytest.mark.parametrize("name", list(SYNTH))
def test_synthetic_words(sp, oracle_mod, name):
    _synth_flow(name)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["packed", "words8"])
def test_loaded_words_are_canonicalised(sp, name):
    cfg = {"packed": PACKED_1CHUNK, "words8": WORDS8}[name]
    p = sp.Params(cfg)
    planes, npr, dim0 = _planes(p), p.num_per, p.dim0
    rng = np.random.default_rng(29)
    words = rng.integers(0, 2 ** 64, (planes, N, npr, dim0), dtype=np.uint64)
    words[0, 0, 0, :4] = [0, (Q0 - 1) | ((Q1 - 1) << 32), Q0 | (Q1 << 32), 2 ** 64 - 1]
    assert ((words & np.uint64(0xFFFFFFFF)) >= np.uint64(Q0)).any() and ((words >> np.uint64(32)) >= np.uint64(Q1)).any()
    db = sp.Database(p).load(words.reshape(-1))
    assert db.format() == name
    got = db.digest(SEED)
    for plane in range(planes):
        _same(got[plane], digest_plane(SEED, plane, canon(words[plane]), N, npr, dim0), (name, plane))
        acc = sp.digest_ref_words(p, SEED, plane, 0, words[plane, :700])
        acc = sp.digest_ref_words(p, SEED, plane, 700, words[plane, 700:], acc)
        _same(got[plane], acc, (name, plane, "digest_ref_words"))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
_every = {}
EMPTY_COLUMN = 5


def _every_case(oracle_mod):
    """the one contents of case 3, computed once: about 200 records of one /update-row body and the numpy digest of plane 1 over the
    oracle's words for the same items (SparseDb.to_dense: zero polynomials for the absent ones)"""
    if not _every:
        o = oracle_mod.Params(EVERY)
        npr, n_items = o.num_per, o.num_items
        rng = np.random.default_rng(41)
        forced = [0, n_items - 1,
                  10 * npr + 20, 11 * npr + 21,          # two items of one quad (row pair 5, columns 20 and 21)
                  32 * npr + 77, 37 * npr + 77]          # two items of one 16-row group of column 77
        idx = set(forced)
        while len(idx) < 200:
            i = int(rng.integers(0, n_items))
            if i % npr != EMPTY_COLUMN:
                idx.add(i)
        recs = [(i, rng.integers(0, 256, o.db_item_size, dtype=np.uint8).tobytes()) for i in sorted(idx)]
        assert all(i % npr != EMPTY_COLUMN for i, _ in recs)
        bucket = oracle_mod.SparseDb(o)
        for i, d in recs:
            bucket.update_item_raw(i, d)
        dense = bucket.to_dense().reshape(-1, N, npr, o.dim0)
        want1 = digest_plane(SEED, 1, dense[1], N, npr, o.dim0)
        del dense
        _every.update(o=o, recs=recs, body=_body(recs), want1=want1)
    return _every


# format -> shards; "" = unsharded
EVERY_FORMATS = {"packed": 1, "planar": 1, "sparse": 1, "packed-row-shards-2": 2, "packed-row-shards-4": 4, "column-shards-2": 2,
                 "planar-shards-2": 2, "sparse-shards-4": 4}


def _every_handle(sp, S, p, fmt, s, G):
    D = sp.Database
    if fmt == "packed" or fmt.startswith("packed-row-shards"):
        return S.own(D(p, s, G))
    if fmt == "planar":
        return S.own(D.planar(p))
    if fmt == "column-shards-2":
        return S.own(D(p, s, G, by_columns=True))
    if fmt == "planar-shards-2":
        return S.own(D.planar_shard(p, s, G))
    return S.own(D.sparse(p, s, G))


def _every_digest(sp, S, p, m, fmt):
    """the body applied to the handles of `fmt`, created and freed one after another -> the lane-wise wrapping sum of their digests"""
    parts = []
    for s in range(EVERY_FORMATS[fmt]):
        db = _every_handle(sp, S, p, fmt, s, EVERY_FORMATS[fmt])
        assert db.update_rows(m["body"])[0] == len(m["recs"])
        parts.append(db.digest(SEED).copy())
        S.objs.remove(db)
        db.__del__()
    return wrapping_sum(parts)


def _every_flow(fmts):
    def flow(sp, oracle_mod, S, arm):
        m = _every_case(oracle_mod)
        arm()
        sp.paths_taken()
        p = S.params(EVERY)
        for fmt in fmts:
            got = _every_digest(sp, S, p, m, fmt)
            _same(got[1], m["want1"], (fmt, "plane 1 against the oracle's words"))
            if "first" not in m:
                m["first"] = got
            _same(got, m["first"], fmt)
            assert got.all()
        return sp.paths_taken()
    flow.__name__ = "digest_every_" + "_".join(fmts)
    return flow


@pytest.mark.parametrize("fmt", list(EVERY_FORMATS))
def test_one_contents_every_format(sp, oracle_mod, fmt):
    _every_flow(("packed", fmt) if fmt != "packed" else ("packed",))(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
EMPTY = {"packed": (PACKED_1CHUNK, lambda D, p: D(p)), "words8": (WORDS8, lambda D, p: D(p)), "planar": (COPY, lambda D, p: D.planar(p)),
         "sparse": (SPARSE_SMALL, lambda D, p: D.sparse(p)), "row-shard": (PACKED_2CHUNKS, lambda D, p: D(p, 1, 2)),
         "column-shard": (PACKED_2CHUNKS, lambda D, p: D(p, 1, 2, by_columns=True)),
         "planar-shard": (EVERY, lambda D, p: D.planar_shard(p, 1, 2)), "sparse-shard": (SPARSE_SMALL, lambda D, p: D.sparse(p, 1, 2))}


@pytest.mark.parametrize("name", list(EMPTY))
def test_empty_handles_digest_to_zero(sp, name):
    cfg, make = EMPTY[name]
    p = sp.Params(cfg)
    db = make(sp.Database, p)
    out = np.full((_planes(p), 2), SENTINEL, dtype=np.uint64)
    got = db.digest(SEED, out=out)
    assert got.shape == (_planes(p), 2) and not got.any() and not out.any(), (name, _hex(got))
    if name in ("planar", "planar-shard"):     # the empty planar database is every byte 0x80
        run = db.read_ref(0, 3, 2, 0, 16)
        assert not run.any()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["packed", "sparse"])
def test_one_byte_moves_one_plane(sp, oracle_mod, fmt):
    m = _every_case(oracle_mod)
    o = m["o"]
    p = sp.Params(EVERY)
    db = sp.Database(p) if fmt == "packed" else sp.Database.sparse(p)
    db.update_rows(m["body"])
    planes = _planes(p)
    before = db.digest(SEED).copy()
    _same(before[1], m["want1"], fmt)
    idx, data = m["recs"][17]
    bpc = -(-o.db_item_size // planes)            # bytes per chunk: chunk c is plane c
    pos = 2 * bpc + 6                             # a byte of chunk 2
    edited = bytearray(data)
    edited[pos] ^= 0x10
    db.update_item(idx, bytes(edited))
    after = db.digest(SEED).copy()
    for plane in range(planes):
        if plane == 2:
            assert after[plane, 0] != before[plane, 0] and after[plane, 1] != before[plane, 1], _hex(after)
        else:
            _same(after[plane], before[plane], (fmt, plane))
    for plane0, n in ((0, 1), (1, 2), (2, 2), (planes - 1, 1), (0, planes)):
        _same(db.digest(SEED, plane0=plane0, nplanes=n), after[plane0:plane0 + n], (fmt, plane0, n))
    assert db.digest(SEED, plane0=planes, nplanes=0).shape == (0, 2)
    db.update_item(idx, data)
    _same(db.digest(SEED), before, (fmt, "the old bytes back"))
    # another seed is another digest
    assert (db.digest(SEED + 2) != before).all()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
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
    out = np.full((_planes(p), 2), SENTINEL, dtype=np.uint64)
    with pytest.raises(sp.SpiralError) as e:               # no copy yet, and the digest never builds one
        db.digest(SEED, which="batch_copy", out=out)
    assert e.value.rc == SP_E_STATE and (out == SENTINEL).all() and db.batch_copy_bytes() == 0
    assert db.prepare_batch() is True
    resident = db.digest(SEED).copy()
    assert resident.all()
    _same(db.digest(SEED, which="batch_copy"), resident, "after the build")
    db.update_items(recs)
    assert db.batch_copy_bytes() > 0
    patched = db.digest(SEED).copy()
    assert (patched != resident).all()
    _same(db.digest(SEED, which="batch_copy"), patched, "after update_items patched the copy")
    _same(db.digest(SEED, which="batch_copy", plane0=1, nplanes=2), patched[1:3], "planes 1, 2 of the copy")
    # the same items on a planar-resident handle: the same resident digest, and no batch copy to speak of
    planar = S.own(sp.Database.planar(p)).load_items(blob)
    planar.update_items(recs)
    _same(planar.digest(SEED), patched, "planar-resident")
    sparse = S.own(sp.Database.sparse(p))
    sparse.update_items(recs[:3])
    for other in (planar, sparse):
        with pytest.raises(sp.SpiralError) as e:
            other.digest(SEED, which="batch_copy", out=out)
        assert e.value.rc == SP_E_STATE and (out == SENTINEL).all()
    # a bulk load drops the copy
    db.load_items(blob)
    assert db.batch_copy_bytes() == 0
    with pytest.raises(sp.SpiralError) as e:
        db.digest(SEED, which="batch_copy", out=out)
    assert e.value.rc == SP_E_STATE and (out == SENTINEL).all()
    _same(db.digest(SEED), resident, "the first contents again")
    return sp.paths_taken()


def test_batch_copy(sp, oracle_mod):
    _copy_flow(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(sp):
    p = sp.Params(WORDS8)
    db = sp.Database(p).fill_synthetic(3)
    planes = _planes(p)
    L = sp.lib()
    u64p = C.POINTER(C.c_uint64)
    for which, plane0, nplanes, null_out in ((0, -1, 1, False), (0, planes - 1, 2, False), (0, planes + 1, 0, False), (0, 0, -1, False),
                                             (0, 0, 2 ** 31 - 1, False), (0, 0, 1, True), (2, 0, 1, False), (-1, 0, 1, False)):
        out = np.full(2 * planes + 4, SENTINEL, dtype=np.uint64)
        rc = L.sp_db_digest(C.c_void_p(db.h), C.c_uint64(SEED), C.c_int(which), C.c_int(plane0), C.c_int(nplanes),
                            None if null_out else out.ctypes.data_as(u64p))
        assert rc == SP_E_ARG, (which, plane0, nplanes, null_out)
        assert (out == SENTINEL).all()
    out = np.full(4, SENTINEL, dtype=np.uint64)
    assert L.sp_db_digest(None, C.c_uint64(SEED), C.c_int(0), C.c_int(0), C.c_int(1), out.ctypes.data_as(u64p)) == SP_E_ARG
    assert L.sp_db_digest(C.c_void_p(db.h), C.c_uint64(SEED), C.c_int(0), C.c_int(planes), C.c_int(0), out.ctypes.data_as(u64p)) == 0
    assert L.sp_db_digest(C.c_void_p(db.h), C.c_uint64(SEED), C.c_int(0), C.c_int(0), C.c_int(0), None) == 0
    assert (out == SENTINEL).all()
    # one plane writes one pair and nothing behind it
    assert L.sp_db_digest(C.c_void_p(db.h), C.c_uint64(SEED), C.c_int(0), C.c_int(1), C.c_int(1), out.ctypes.data_as(u64p)) == 0
    assert (out[:2] != SENTINEL).all() and (out[2:] == SENTINEL).all()
    _same(out[:2], db.digest(SEED)[1])


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
HARDENED = {"synthetic-packed": _synth_flow("packed-2pairs-1chunk"), "every-planar": _every_flow(("planar",)),
            "every-sparse": _every_flow(("sparse",)), "batch-copy": _copy_flow}


@pytest.mark.parametrize("mode", ["poison", "guard"])
@pytest.mark.parametrize("what", list(HARDENED))
def test_on_hardened_buffers(oracle_mod, capfd, what, mode):
    """poison_ws = 0xA5 and guard_ws = 1 MiB act when a buffer is allocated: the flow computes its references, sets the switch, makes
    its own handles -- the read buffer with the sums and the row keys among their allocations -- and lets go of every one before stderr
    is read"""
    from test_gpu_hardened_buffers import POISON, _hardened
    _hardened(HARDENED[what], mode, POISON, oracle_mod, capfd)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_digests_beside_a_running_list(sp, oracle_mod):
    o, p = oracle_mod.Params(COPY), sp.Params(COPY)
    blob = np.random.default_rng(59).integers(0, 256, o.num_items * o.db_item_size, dtype=np.uint8)
    cl = oracle_mod.Client(o)
    gpp = sp.PublicParameters.deserialize(p, cl.generate_keys(83))
    qs = [cl.generate_query((37 * k + 5) % o.num_items, 900 + k) for k in range(8)]
    db = sp.Database(p).load_items(blob)
    alone = sp.process_query_batch(p, [gpp] * 8, qs, db)
    want = db.digest(SEED).copy()
    assert want.all()
    out, done = {"digests": []}, threading.Event()

    def ask():
        try:
            out["responses"] = sp.process_query_batch(p, [gpp] * 8, qs, db)
        finally:
            done.set()

    def digest():
        while len(out["digests"]) < 20:
            out["digests"].append(db.digest(SEED).copy())
            if done.is_set():
                break

    threads = [threading.Thread(target=ask), threading.Thread(target=digest)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out["responses"] == alone
    assert 1 <= len(out["digests"]) <= 20
    for d in out["digests"]:
        _same(d, want)
