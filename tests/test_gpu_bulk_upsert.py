"""Bulk upserts: sp_db_update_items / sp_db_update_rows (the body of lib/server's POST /update-row, db/loading.rs:361-377
update_many_items) and sp_server_update_row, on sparse buckets, dense databases (8-byte and PACKED, whole and sharded, with a standing
digit-planar copy) and through the request layer.  The yardsticks are the oracle's: load_db_from_bytes of the edited file (dense),
SparseDb.update_item_raw record by record + process_query (sparse) -- never the single-item call of the library under test."""
import ctypes as C
import os
import re
import struct
import threading

import numpy as np
import pytest

from conftest import FAST
from test_sparse_bucket import _SMALL_SPARSE, _Bucket, _random_item

pytestmark = pytest.mark.gpu

_IDS = ["inst1", "inst2"]


def _body(records):
    """update_many_items' framing: be32 chunk_len | be32 item index | item bytes, chunk_len = 4 + len(item bytes)"""
    return b"".join(struct.pack(">II", 4 + len(d), i) + bytes(d) for i, d in records)


def _set_window(sp, n_bytes):
    sp.lib().sp_debug_set(b"db_load_window", C.c_long(n_bytes))


def _default_window():
    return int(os.environ.get("SPIRAL_DB_LOAD_WINDOW", 512 << 20))


# ------------------------------------------------------------------------------------------------ sparse buckets
def _mixed_records(b, rng):
    """~24 records over a bucket that already holds 6 items in rows 0 - 2: an index three times (the last occurrence shorter than
    the first: the zero padding must clear the old bytes), a zero-length record, records of 1 - 3 bytes, an overwrite of a key
    already present, new keys in occupied rows and one that opens row 7.  -> (records, {index: bytes of the first chunk that decode})"""
    at = lambda j, ii: j * b.num_per + ii                                          # noqa: E731
    chunk = b.size // (b.cfg.get("instances", 1) * 4)
    for j, ii in ((0, 0), (0, 9), (1, 3), (1, 15), (2, 7), (2, 8)):
        b.put(at(j, ii), _random_item(rng, b.size))
    dup, empty, old, new_row = at(1, 5), at(2, 1), at(1, 3), at(7, 14)
    recs = [(dup, _random_item(rng, b.size)), (at(0, 1), _random_item(rng, b.size)), (empty, b""),
            (at(0, 2), bytes(rng.integers(1, 256, 1, dtype=np.uint8))), (at(0, 3), bytes(rng.integers(1, 256, 2, dtype=np.uint8))),
            (at(0, 4), bytes(rng.integers(1, 256, 3, dtype=np.uint8))), (old, _random_item(rng, b.size)),
            (dup, _random_item(rng, b.size - 1)), (new_row, _random_item(rng, b.size))]
    recs += [(at(j, ii), _random_item(rng, b.size - (ii % 3))) for j, ii in ((0, 15), (1, 0), (1, 1), (1, 2), (2, 2), (2, 3), (2, 4),
                                                                               (2, 5), (2, 6), (0, 10), (0, 11), (1, 12), (1, 13))]
    recs += [(dup, _random_item(rng, chunk + chunk // 3)), (at(2, 15), _random_item(rng, b.size))]
    assert len(recs) == 24
    return recs, {"dup": dup, "old": old, "new_row": new_row, "absent": at(5, 5), "chunk": chunk}


def _apply(b, recs):
    """the records as ONE body to the library, one by one to the oracle's bucket"""
    applied, largest = b.gdb.update_rows(_body(recs))
    assert applied == len(recs) and largest == 4 + max(len(d) for _, d in recs)
    for i, d in recs:
        b.sdb.update_item_raw(i, d)
        b.items[i] = bytes(d)


def _mixed_queries(b, keys):
    """-> the four responses (each already compared with the oracle's inside _Bucket.query)"""
    return [b.query(keys["dup"], 500, decodes=keys["chunk"])[1], b.query(keys["old"], 501)[1], b.query(keys["new_row"], 502)[1],
            b.query(keys["absent"], 503)[1]]


@pytest.mark.parametrize("cfg", _SMALL_SPARSE, ids=_IDS)
def test_sparse_mixed_body(oracle_mod, cfg):
    b = _Bucket(oracle_mod, cfg)
    recs, keys = _mixed_records(b, np.random.default_rng(41))
    b.query(keys["old"], 499)                       # an index snapshot and plan exist before the body: it must dirty both
    _apply(b, recs)
    assert b.gdb.sparse_items() == len(b.items) == 6 + len({i for i, _ in recs}) - 1
    _mixed_queries(b, keys)
    # the array form, a later pair for an index winning
    b.gdb.update_items([(keys["dup"], b"\x01" * b.size), (keys["dup"], b"\x09" * 5)])
    b.sdb.update_item_raw(keys["dup"], b"\x09" * 5)
    b.items[keys["dup"]] = b"\x09" * 5
    b.query(keys["dup"], 504, decodes=5)
    with pytest.raises(b.sp.SpiralError):
        b.gdb.update_items([(0, b"x"), (b.dim0 * b.num_per, b"x")])


@pytest.mark.parametrize("cfg", _SMALL_SPARSE, ids=_IDS)
def test_sparse_growth_past_initial_capacity(oracle_mod, cfg):
    """10 items, then 70 new keys in one body: the store (64 slots) grows once, before the first kernel, the old items move with it"""
    b = _Bucket(oracle_mod, cfg)
    rng = np.random.default_rng(43)
    order = [int(i) for i in rng.permutation(b.dim0 * b.num_per)]
    for idx in order[:10]:
        b.put(idx, _random_item(rng, b.size))
    recs = [(idx, _random_item(rng, b.size)) for idx in order[10:80]]
    _apply(b, recs)
    assert b.gdb.sparse_items() == 80
    for k, idx in enumerate((order[3], recs[0][0], recs[-1][0])):
        b.query(idx, 510 + k)


@pytest.mark.parametrize("cfg", _SMALL_SPARSE, ids=_IDS)
def test_sparse_body_over_several_windows(oracle_mod, cfg):
    """the body of test_sparse_mixed_body through upload windows of ~1 KiB (2 - 4 records each): the same responses"""
    whole, cut = _Bucket(oracle_mod, cfg), _Bucket(oracle_mod, cfg)
    recs, keys = _mixed_records(whole, np.random.default_rng(41))
    assert sum(len(d) for _, d in recs) > 4 * 1024
    _apply(whole, recs)
    _set_window(cut.sp, 1024)
    try:
        _mixed_records(cut, np.random.default_rng(41))
        _apply(cut, recs)
    finally:
        _set_window(cut.sp, _default_window())
    assert cut.gdb.sparse_items() == whole.gdb.sparse_items()
    assert _mixed_queries(cut, keys) == _mixed_queries(whole, keys)


_FAULTS = ["cut-in-length", "cut-in-payload", "chunk_len-3", "too-long", "index-out-of-range"]


@pytest.mark.parametrize("cfg", _SMALL_SPARSE, ids=_IDS)
@pytest.mark.parametrize("fault", _FAULTS)
def test_faulty_third_record(oracle_mod, cfg, fault):
    """records 0 and 1 are applied, record 2 is faulty, record 3 is never looked at"""
    b = _Bucket(oracle_mod, cfg)
    rng = np.random.default_rng(47)
    i1, i2, i3, i4 = 5, 3 * b.num_per + 2, 6 * b.num_per + 9, 4 * b.num_per
    good = [(i1, _random_item(rng, b.size)), (i2, _random_item(rng, b.size - 7))]
    head = _body(good)
    third, tail = _body([(i3, _random_item(rng, b.size))]), _body([(i4, _random_item(rng, b.size))])
    body = {"cut-in-length": head + third[:2],
            "cut-in-payload": head + third[:40],
            "chunk_len-3": head + struct.pack(">I", 3) + b"\0\0\1" + tail,
            "too-long": head + _body([(i3, bytes(b.size + 1))]) + tail,
            "index-out-of-range": head + _body([(b.dim0 * b.num_per, b"abc")]) + tail}[fault]
    with pytest.raises(b.sp.SpiralError) as e:
        b.gdb.update_rows(body)
    assert e.value.applied == 2 and e.value.rc == -1
    assert "record 2 at byte offset %d" % len(head) in str(e.value), str(e.value)
    for i, d in good:
        b.sdb.update_item_raw(i, d)
        b.items[i] = d
    assert b.gdb.sparse_items() == 2
    b.query(i2, 520, decodes=b.size - 7)
    b.query(i3, 521)                                # absent on both sides
    assert b.gdb.update_rows(b"") == (0, 0) and b.gdb.sparse_items() == 2


# ------------------------------------------------------------------------------------------------ dense databases
_DENSE = {"narrow": dict(FAST, db_item_size=256), "packed": dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=600)}
_dense_cases = {}


def _dense_case(oracle_mod, name):
    """(cfg, file before, records, expected words [plane][z][ii][j] of the edited file): computed once per shape"""
    if name not in _dense_cases:
        cfg = _DENSE[name]
        o = oracle_mod.Params(cfg)
        rng = np.random.default_rng(53)
        isz, npr, d0 = o.db_item_size, o.num_per, o.dim0
        blob = rng.integers(0, 256, o.num_items * isz, dtype=np.uint8)
        at = lambda j, ii: j * npr + ii                                            # noqa: E731
        idxs = [at(2, 2), at(2, 3), at(3, 2), at(3, 3),                            # all four items of one quad
                at(1, npr - 2), at(1, npr - 1),                                    # both columns of a lane slot
                at(d0 - 2, 0), at(d0 - 1, 0),                                      # both rows of a row pair
                at(0, 0), at(d0 - 1, npr - 1),                                     # first and last row and column
                at(2, 3)]                                                          # a duplicate: the later record wins
        lens = [isz, isz - 1, isz - 2, 0, isz, 3, isz - 1, isz, 1, isz, isz // 2]
        recs = [(i, rng.integers(1, 256, n, dtype=np.uint8).tobytes()) for i, n in zip(idxs, lens)]
        after = blob.copy()
        for i, d in recs:
            after[i * isz:(i + 1) * isz] = 0
            after[i * isz:i * isz + len(d)] = np.frombuffer(d, dtype=np.uint8)
        exp = o.load_db_from_bytes(after.tobytes()).reshape(4, 2048, npr, d0)
        _dense_cases[name] = (cfg, blob, recs, exp)
    return _dense_cases[name]


@pytest.mark.parametrize("name", list(_DENSE))
def test_dense_body_by_quads(oracle_mod, name):
    """non-zero neighbours survive, every listed item is replaced: every word of planes x z in {0, 9, 2047} x columns x rows"""
    import sdk_amd as sp
    cfg, blob, recs, exp = _dense_case(oracle_mod, name)
    p = sp.Params(cfg)
    db = sp.Database(p).load_items(blob)
    assert db.update_rows(_body(recs)) == (len(recs), 4 + cfg["db_item_size"])
    for pl in range(4):
        for z in (0, 9, 2047):
            for ii in range(p.num_per):
                assert (db.read_ref(pl, z, ii, 0, p.dim0) == exp[pl, z, ii]).all(), (pl, z, ii)
    with pytest.raises(sp.SpiralError):
        db.update_items([(p.num_items(), b"x")])


@pytest.mark.parametrize("by_columns", [False, True], ids=["row-shard", "column-shard"])
@pytest.mark.parametrize("name", list(_DENSE))
def test_dense_body_on_shards(oracle_mod, name, by_columns):
    """shard 1 of 2: the records that live on shard 0 are skipped and still counted"""
    import sdk_amd as sp
    cfg, blob, recs, exp = _dense_case(oracle_mod, name)
    p = sp.Params(cfg)
    db = sp.Database(p, 1, 2, by_columns=by_columns).load_items(blob)
    assert db.update_rows(_body(recs))[0] == len(recs)
    nj = p.dim0 if by_columns else p.dim0 // 2
    want = exp if by_columns else exp[:, :, :, nj:]
    for pl in range(4):
        for z in (0, 9, 2047):
            for ii in range(1 if by_columns else 0, p.num_per, 2 if by_columns else 1):
                assert (db.read_ref(pl, z, ii, 0, nj) == want[pl, z, ii]).all(), (pl, z, ii)


def test_planar_copy_follows_one_body(oracle_mod):
    """the 64 x 128 case of test_planar_copy_lifecycle with its edits as ONE body: the digit-planar copy stays and is patched"""
    import sdk_amd as sp
    cfg = {"n": 2, "nu_1": 6, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8,
           "t_exp_right": 56, "instances": 1, "db_item_size": 256}
    o = oracle_mod.Params(cfg)
    p = sp.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(61)
    gpp = sp.PublicParameters.deserialize(p, pp)
    rng = np.random.default_rng(13)
    isz = o.db_item_size
    blob = rng.integers(0, 256, o.num_items * isz, dtype=np.uint8)
    gdb = sp.Database(p).load_items(blob)
    assert gdb.prepare_batch() is True
    copy = gdb.batch_copy_bytes()
    assert copy == 4 * 2048 * o.num_per * o.dim0 * 8
    npr, d0 = o.num_per, o.dim0
    edits = [0, 1, npr, npr + 1, (d0 - 1) * npr + npr - 1, (d0 // 2) * npr + 77, 3 * npr + 126, 3 * npr + 127, 64 * npr % o.num_items + 5, 1]
    recs = []
    for k, it in enumerate(edits):
        rec = rng.integers(0, 256, isz - (k % 4), dtype=np.uint8)
        blob[it * isz:(it + 1) * isz] = 0
        blob[it * isz:it * isz + rec.size] = rec
        recs.append((it, rec.tobytes()))
    assert gdb.update_rows(_body(recs))[0] == len(edits)
    assert gdb.batch_copy_bytes() == copy
    exp = o.load_db_from_bytes(blob.tobytes())
    B = 11
    idxs = [edits[i] if i < 9 else (977 * i + 3) % o.num_items for i in range(B)]
    qs = [cl.generate_query(idxs[i], 900 + i) for i in range(B)]
    sp.paths_taken()
    resp = sp.process_query_batch(p, [gpp] * B, qs, gdb)
    assert "sweep_batch_planar" in sp.paths_taken()
    for i in range(B):
        assert resp[i] == o.process_query(pp, qs[i], exp), (i, idxs[i])


# ------------------------------------------------------------------------------------------------ request layer
def _served_bucket(oracle_mod):
    b = _Bucket(oracle_mod, _SMALL_SPARSE[0])
    srv = b.sp.Server(b.p, b.gdb)
    return b, srv, srv.setup(b.pp).encode()


def test_server_update_row_then_private_read(oracle_mod):
    b, srv, uuid = _served_bucket(oracle_mod)
    rng = np.random.default_rng(59)
    recs = [(i, _random_item(rng, b.size - i % 5)) for i in (3, 40, 41, 127, 40)]
    reply = srv.update_row(_body(recs))
    m = re.fullmatch(r'\{"status":"done updating", "loading_time_us":(\d+), "largest_update":(\d+)\}', reply)
    assert m and int(m.group(2)) == 4 + max(len(d) for _, d in recs), reply
    for i, d in recs:
        b.sdb.update_item_raw(i, d)
    qs = [b.cl.generate_query(i, 530 + k) for k, i in enumerate((40, 127, 9))]
    assert srv.private_read([uuid + q for q in qs]) == [b.sdb.process_query(b.pp, q) for q in qs]
    with pytest.raises(b.sp.SpiralError):
        srv.update_row(_body(recs)[:-1])
    assert b.gdb.sparse_items() == 4


def test_server_update_row_wants_its_own_db(oracle_mod):
    b, srv, _ = _served_bucket(oracle_mod)
    other = b.sp.Database.sparse(b.p)
    body = np.frombuffer(_body([(1, b"abc")]), dtype=np.uint8)
    out, n = C.create_string_buffer(128), C.c_size_t(0)
    rc = b.sp.lib().sp_server_update_row(C.c_void_p(srv.h), C.c_void_p(other.h), body.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         C.c_size_t(body.size), out, C.c_size_t(128), C.byref(n))
    assert rc == -1 and other.sparse_items() == 0 and b.gdb.sparse_items() == 0          # SP_E_ARG, nothing written anywhere


def test_updates_and_reads_from_two_threads(oracle_mod):
    """one thread posts three bodies, another posts private-read lists: a list is answered from the bucket before or after a body,
    never from the middle of one -- each list equals the oracle's for one of the four bucket states"""
    b, srv, uuid = _served_bucket(oracle_mod)
    rng = np.random.default_rng(61)
    b.put(17, _random_item(rng, b.size))
    bodies = [[(17, _random_item(rng, b.size)), (33, _random_item(rng, b.size))],
              [(7 * b.num_per + 1, _random_item(rng, b.size)), (33, _random_item(rng, 9))],
              [(17, b""), (90, _random_item(rng, b.size)), (91, _random_item(rng, b.size))]]
    qs = [b.cl.generate_query(17, 540), b.cl.generate_query(33, 541)]
    states = [[b.sdb.process_query(b.pp, q) for q in qs]]
    for recs in bodies:
        for i, d in recs:
            b.sdb.update_item_raw(i, d)
        states.append([b.sdb.process_query(b.pp, q) for q in qs])
    seen, errors = [], []

    def reader():
        try:
            for _ in range(6):
                seen.append(srv.private_read([uuid + q for q in qs]))
        except Exception as e:                      # noqa: BLE001
            errors.append(e)

    def writer():
        try:
            for recs in bodies:
                srv.update_row(_body(recs))
        except Exception as e:                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=reader), threading.Thread(target=writer)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(seen) == 6 and all(r in states for r in seen)
    assert srv.private_read([uuid + q for q in qs]) == states[3]
