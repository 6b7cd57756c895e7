"""Items removed from a resident database on the device (sp_db_remove_items / _range, sp_db_sparse_trim, sp_server_remove_items;
Database.remove_items / remove_range / trim, Server.remove_items, Database.repair_from(remove=True)).  Every comparison is exact, and
the witness for the expected contents is never the library's own read-back: it is the ORACLE's words the handle was loaded from with
the removed items' words zeroed in numpy, their table from item_digests_ref_words, and for a sparse handle the oracle's SparseDb
rebuilt from the survivors only.

1  every form (A: 64 x 128 -- PACKED, planar-resident, sparse, row / column / sparse shards; B: 256 x 16 -- 8-byte words; S: 4 x 128 -- the
   smallest PACKED shape; C: 128 x 128 -- planar shards; K: 16 x 256 -- two 128-column chunks; N9: 8 x 128 at 9 planes): a list with a quad
   per single position, a whole quad, two items of one 16-row cell, first and last row, both chunks, a repeated index, indices a shard
   does not hold -> table over all planes, read_ref down the touched columns and their quad partners, present, removed, shards add up.
2  the slot cases of a sparse bucket, by table, present, sparse_items and lib/server's response bytes.
3  queries after a removal on the dense forms, alone and in a list of 9, with and without a standing batch copy.
4  record lists across at least three windows, then the same call under the shipped window.
5  remove_range.   6  trim.   7  errors write nothing.   8  repair_from(remove=True).   9  the server, lists in flight.
10 cases of 1 and 4 on poisoned and on guarded buffers (the procedure of tests/test_gpu_hardened_buffers.py).
tests/test_emulated_db_remove.py runs a subset on the emulated device."""
import ctypes as C
import threading

import numpy as np
import pytest

from param_matrix import cfg as _matrix_cfg
from test_gpu_db_copy import CHUNKS, PACKED, SHARDS, SMALLEST, SPARSE, WORDS8, _canon, _make, _shape_mask
from test_gpu_hardened_buffers import _many
from test_gpu_item_readback import N, WINDOW_DEFAULT, _Own, _no_switch
from test_gpu_narrow_batch import switch
from test_gpu_planar_shards import _cfg as _planar_cfg

pytestmark = pytest.mark.gpu

SP_E_ARG = -1
SEED = 0x5EEDC0DE
SMALL_WINDOW = 1024        # a record is 8 or 12 bytes (24 beside a batch copy): 124, 82 or 41 records per window
SETS = {"A": PACKED, "B": WORDS8, "S": SMALLEST, "C": _planar_cfg(7, 7), "K": CHUNKS, "P": SPARSE,
        "N9": dict(_matrix_cfg("N3", 3, 7), db_item_size=2304)}
FORMS = [("A", "packed"), ("A", "planar"), ("A", "sparse"), ("A", "row-shards"), ("A", "column-shards"), ("A", "sparse-shards"),
         ("B", "words8"), ("S", "packed"), ("C", "planar-shards"), ("K", "packed"), ("N9", "packed"), ("N9", "sparse")]


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _table(sp, p, o, words):
    """the host's per-item digest table of reference words [planes][N][num_per][dim0] (no device call)"""
    acc = np.zeros((o.num_items, 2), dtype=np.uint64)
    for plane in range(words.shape[0]):
        sp.item_digests_ref_words(p, SEED, plane, 0, words[plane].reshape(-1), acc)
    return acc


_cases = {}


def _case(sp, oracle_mod, name):
    """the oracle's and the host's side of a parameter set, computed once: a random item file, the oracle's words of it and their table"""
    if name not in _cases:
        cfg = SETS[name]
        o, p = oracle_mod.Params(cfg), sp.Params(cfg)
        planes = cfg["instances"] * cfg["n"] ** 2
        file = np.random.default_rng(211).integers(0, 256, (o.num_items, o.db_item_size), dtype=np.uint8)
        words = o.load_db_from_bytes(file.tobytes()).reshape(planes, N, o.num_per, o.dim0)
        _cases[name] = dict(cfg=cfg, o=o, p=p, planes=planes, file=file, words=words, t_src=_table(sp, p, o, words), zeroed={})
    return _cases[name]


class _Zeroed:
    """the case's words with the listed items' words zeroed in numpy, for the time of the block (the words are put back afterwards)"""

    def __init__(self, c, items):
        self.c, self.items = c, np.unique(np.asarray(items, dtype=np.int64))

    def __enter__(self):
        o, w = self.c["o"], self.c["words"]
        self.j, self.ii = self.items // o.num_per, self.items % o.num_per
        self.saved = w[:, :, self.ii, self.j].copy()
        w[:, :, self.ii, self.j] = 0
        return w

    def __exit__(self, *exc):
        self.c["words"][:, :, self.ii, self.j] = self.saved


def _table_without(sp, c, items):
    """the table of the oracle's words with `items` zeroed (cached per list)"""
    key = tuple(sorted(set(int(i) for i in items)))
    if key not in c["zeroed"]:
        with _Zeroed(c, key) as w:
            c["zeroed"][key] = _table(sp, c["p"], c["o"], w)
    return c["zeroed"][key]


def _list_for(o):
    """the removal list of case 1 for a shape, as (row, column) pairs -> item indices, one of them twice"""
    npr, d0 = o.num_per, o.dim0
    rc = []
    for w in range(4):                                           # a quad per position in which only that position is removed
        rc.append((w >> 1, 2 * (3 + w) + (w & 1)))
    qa = 2 if npr == 16 else 10                                  # a quad that loses all four of its items
    rc += [(2 + a, 2 * qa + b) for a in (0, 1) for b in (0, 1)]
    r1, r2 = (5, 12) if d0 >= 16 else (0, 3)                     # two items of one 16-row cell
    rc += [(r1, 40 % npr), (r2, 40 % npr)]
    rc += [(0, 50 % npr), (d0 - 1, 51 % npr)]                    # the first and the last row
    if npr > 128:
        rc += [(1, 130), (d0 - 2, npr - 1)]                      # the second 128-column chunk
    items = [j * npr + ii for j, ii in rc]
    assert len(set(items)) == len(items)
    return items + [items[0], items[5]]                          # repeated indices


def _load(sp, S, c, p, form, s, held=None):
    """shard `s` of a form loaded from the oracle's words (a sparse one: the file's items of `held`) -> (handle, held mask)"""
    o = c["o"]
    db, mask = _make(sp, S, p, form, s), _shape_mask(form, o, s)
    if form.startswith("sparse"):
        mask = mask & held
        db.update_items([(int(i), c["file"][i].tobytes()) for i in np.flatnonzero(mask)])
    else:
        db.load(c["words"].reshape(-1))
    return db, mask


def _third(o, must):
    """a scattered third of the items, the listed ones among them except the last listed"""
    held = np.zeros(o.num_items, dtype=bool)
    held[np.random.default_rng(17).choice(o.num_items, o.num_items // 3, replace=False)] = True
    held[must] = True
    held[must[-3]] = False                                       # one listed key is absent: a no-op
    return held


def _columns_match(c, db, mask, items, form):
    """read_ref down every column a removed item or its quad partner stands in, at the corner words: the oracle's word, zero where
    the item was removed -- the removed items, their quad neighbours and the other rows of their 16-row cells"""
    o = c["o"]
    gone = np.zeros(o.num_items, dtype=bool)
    gone[items] = True
    held_rows = np.flatnonzero(mask.reshape(o.dim0, o.num_per).any(axis=1))
    j_lo, j_hi = int(held_rows[0]), int(held_rows[-1])
    cols = sorted({ii ^ b for ii in (np.asarray(items) % o.num_per).tolist() for b in (0, 1)})
    for plane in (0, c["planes"] - 1):
        for z in (0, N - 1):
            for ii in cols:
                if not mask[j_lo * o.num_per + ii]:
                    continue                                     # another column shard's
                got = db.read_ref(plane, z, ii, 0, j_hi - j_lo + 1)
                want = _canon(c["words"][plane, z, ii, j_lo:j_hi + 1])
                want[gone.reshape(o.dim0, o.num_per)[j_lo:j_hi + 1, ii]] = 0
                assert (got == want).all(), (form, plane, z, ii)


def _form_flow(set_name, form):
    def flow(sp, oracle_mod, S, arm):
        c = _case(sp, oracle_mod, set_name)
        o = c["o"]
        items = _list_for(o)
        listed = np.zeros(o.num_items, dtype=bool)
        listed[items] = True
        sparse = form.startswith("sparse")
        held_all = _third(o, items) if sparse else np.ones(o.num_items, dtype=bool)
        t_want = _table_without(sp, c, items)
        arm()
        sp.paths_taken()
        p = S.params(c["cfg"])                                   # (the device handles' own: c["p"] serves the host's tables)
        total = np.zeros((o.num_items, 2), dtype=np.uint64)
        for s in range(SHARDS.get(form, 1)):
            db, mask = _load(sp, S, c, p, form, s, held_all)
            bytes_before = db.device_bytes()
            removed = db.remove_items(items)
            assert removed == int((mask & listed).sum()), (form, s)
            after = mask & ~listed if sparse else mask
            got, present = db.item_digests(SEED)
            assert (present != 0).tolist() == after.tolist(), (form, s)
            want = np.where(after[:, None], t_want, 0).astype(np.uint64)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (form, s, bad[:8].tolist(), int(bad.size))
            assert db.device_bytes() == bytes_before
            if sparse:
                assert db.sparse_items() == int(after.sum())
            else:
                _columns_match(c, db, mask, items, form)
            with np.errstate(over="ignore"):
                total += got
        whole = np.where((held_all & ~listed)[:, None], t_want, 0) if sparse else t_want
        assert (total == whole.astype(np.uint64)).all()          # the shards' tables add up to the unsharded expected table
        return sp.paths_taken()
    flow.__name__ = "db_remove_%s_%s" % (set_name, form)
    return flow


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name,form", FORMS, ids=["%s-%s" % t for t in FORMS])
def test_every_form(sp, oracle_mod, set_name, form):
    _form_flow(set_name, form)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
_buckets = {}


def _bucket_case(sp, oracle_mod):
    """set P (64 x 8) on the oracle's side: a client's keys, 40 keys in a fixed insertion order -- slot k holds KEYS[k] -- in rows 0 .. 6
    and columns 0 .. 6, but for one that is alone in row 60 and alone in column 7"""
    if not _buckets:
        c = _case(sp, oracle_mod, "P")
        o = c["o"]
        grid = [int(j * o.num_per + ii) for j in range(7) for ii in range(7)]
        grid = [grid[k] for k in np.random.default_rng(23).permutation(49)]
        keys = grid[:20] + [60 * o.num_per + 7] + grid[20:39]
        assert len(keys) == 40 and len(set(keys)) == 40
        cl = oracle_mod.Client(o)
        _buckets.update(c=c, keys=keys, spare=grid[39:], cl=cl, pp=cl.generate_keys(91), lonely=60 * o.num_per + 7, q={}, want={})
    return _buckets


def _bucket_check(sp, oracle_mod, b, db, gpp, held, ask):
    """a bucket that should hold exactly `held` (in any slot order): table, present, sparse_items, and for every index of `ask` the
    response bytes of lib/server's SparseDb rebuilt from the survivors only"""
    c = b["c"]
    o, p = c["o"], c["p"]
    mask = np.zeros(o.num_items, dtype=bool)
    mask[list(held)] = True
    got, present = db.item_digests(SEED)
    assert (present != 0).tolist() == mask.tolist()
    assert (got == np.where(mask[:, None], c["t_src"], 0).astype(np.uint64)).all()
    assert db.sparse_items() == len(held)
    bucket = oracle_mod.SparseDb(o)
    for i in sorted(held):
        bucket.update_item_raw(i, c["file"][i].tobytes())
    for k, i in enumerate(ask):
        if i not in b["q"]:
            b["q"][i] = b["cl"].generate_query(i, 700 + len(b["q"]))
        assert sp.process_query(p, gpp, b["q"][i], db) == bucket.process_query(b["pp"], b["q"][i]), (i, k)


def _filled(sp, b, keys=None):
    c = b["c"]
    db = sp.Database.sparse(c["p"])
    db.update_items([(i, c["file"][i].tobytes()) for i in (b["keys"] if keys is None else keys)])
    return db


SLOTS = {"last-slot": [39], "first-slot": [0], "interleaved": [1, 3, 5, 36, 38], "more-removed-than-survive": list(range(0, 40, 4)) + list(range(1, 40, 2)),
         "lonely-row-and-column": [20]}


@pytest.mark.parametrize("name", list(SLOTS))
def test_sparse_slot_cases(sp, oracle_mod, name):
    b = _bucket_case(sp, oracle_mod)
    keys, p = b["keys"], b["c"]["p"]
    gpp = sp.PublicParameters.deserialize(p, b["pp"])
    db = _filled(sp, b)
    _bucket_check(sp, oracle_mod, b, db, gpp, set(keys), [keys[20]])             # (a query before: the removal must publish a new index)
    gone = [keys[k] for k in sorted(set(SLOTS[name]))]
    cap = db.device_bytes()
    assert db.remove_items(gone) == len(gone)
    left = [k for k in keys if k not in gone]
    _bucket_check(sp, oracle_mod, b, db, gpp, set(left), [left[-1], left[0], gone[0]])
    assert db.device_bytes() == cap
    assert db.remove_items(gone) == 0                                             # absent now: no-ops
    _bucket_check(sp, oracle_mod, b, db, gpp, set(left), [left[len(left) // 2]])


def test_sparse_absent_keys_and_upserts_after(sp, oracle_mod):
    b = _bucket_case(sp, oracle_mod)
    keys, spare, c = b["keys"], b["spare"], b["c"]
    gpp = sp.PublicParameters.deserialize(c["p"], b["pp"])
    db = _filled(sp, b)
    assert db.remove_items([spare[0]]) == 0 and db.remove_items([spare[0], keys[7], spare[1], keys[7]]) == 1
    held = set(keys) - {keys[7]}
    _bucket_check(sp, oracle_mod, b, db, gpp, held, [keys[7], keys[39]])
    # a new key and the removed key again: they take the slots from the new count on
    db.update_items([(i, c["file"][i].tobytes()) for i in (spare[0], keys[7])])
    held |= {spare[0], keys[7]}
    _bucket_check(sp, oracle_mod, b, db, gpp, held, [spare[0], keys[7], keys[39]])
    assert db.remove_items([keys[39], spare[0]]) == 2
    db.update_item(keys[39], c["file"][keys[39]].tobytes())
    _bucket_check(sp, oracle_mod, b, db, gpp, held - {spare[0]}, [keys[39], keys[7], spare[0]])


def test_sparse_remove_every_key(sp, oracle_mod):
    b = _bucket_case(sp, oracle_mod)
    keys, c = b["keys"], b["c"]
    o, p = c["o"], c["p"]
    gpp = sp.PublicParameters.deserialize(p, b["pp"])
    db, fresh = _filled(sp, b), sp.Database.sparse(p)
    q = b["cl"].generate_query(keys[3], 777)
    sp.process_query(p, gpp, q, db)
    assert db.remove_items(keys + keys[:5]) == 40 and db.sparse_items() == 0

    def answer(d):
        try:
            return sp.process_query(p, gpp, q, d)
        except sp.SpiralError as e:
            return ("refused", str(e))

    assert answer(db) == answer(fresh)                                            # whatever a fresh handle answers or refuses
    got, present = db.item_digests(SEED)
    assert not present.any() and not got.any()
    assert db.remove_items(keys[:3]) == 0 and db.remove_range(0) == 0
    some = keys[5:25]
    db.update_items([(i, c["file"][i].tobytes()) for i in some])
    fresh.update_items([(i, c["file"][i].tobytes()) for i in some])
    _bucket_check(sp, oracle_mod, b, db, gpp, set(some), [some[0], keys[0]])
    assert answer(db) == answer(fresh) and (db.item_digests(SEED)[0] == fresh.item_digests(SEED)[0]).all()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_queries_after_removal_on_the_dense_forms(sp, oracle_mod):
    c = _case(sp, oracle_mod, "A")
    o, p = c["o"], c["p"]
    items = _list_for(o)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(71)
    idxs = [items[0], items[0] ^ 1, items[4], items[8], items[9] + o.num_per, 0, o.num_items - 1, 4097, items[10]]
    qs = [cl.generate_query(i, 600 + k) for k, i in enumerate(idxs)]
    with _Zeroed(c, items) as w:
        flat = w.reshape(-1)
        want = _many(lambda q: o.process_query(pp, q, flat), qs)
    t_want = _table_without(sp, c, items)
    gpp = sp.PublicParameters.deserialize(p, pp)
    plain = sp.Database(p).load(c["words"].reshape(-1))
    copied = sp.Database(p).load(c["words"].reshape(-1))
    assert copied.prepare_batch() and copied.batch_copy_bytes() != 0
    planar = sp.Database.planar(p).load(c["words"].reshape(-1))
    for db in (plain, copied, planar):
        assert db.remove_items(items) == len(set(items))
        assert sp.process_query(p, gpp, qs[0], db) == want[0]
        assert sp.process_query_batch(p, [gpp] * 9, qs, db) == want
        assert (db.item_digests(SEED)[0] == t_want).all()
    assert copied.batch_copy_bytes() != 0
    assert (copied.digest(SEED, which="batch_copy") == copied.digest(SEED)).all()
    assert (copied.item_digests(SEED, which="batch_copy")[0] == t_want).all()
    if plain.batch_copy_bytes():                                  # (the list of 9 built it behind the removal, from the cleared words)
        assert (plain.digest(SEED, which="batch_copy") == plain.digest(SEED)).all()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
WINDOWED = {"packed": ("A", "packed"), "packed-batch-copy": ("A", "packed"), "planar": ("A", "planar"), "words8": ("B", "words8"),
            "sparse": ("P", "sparse")}


def _window_flow(name):
    def flow(sp, oracle_mod, S, arm):
        set_name, form = WINDOWED[name]
        c = _case(sp, oracle_mod, set_name)
        o = c["o"]
        if form == "sparse":                                     # a full bucket loses its first 260 slots: 252 moves of 8 bytes
            items = list(range(260))
            held = np.ones(o.num_items, dtype=bool)
            t_want = np.where((np.arange(o.num_items) >= 260)[:, None], c["t_src"], 0).astype(np.uint64)
        else:                                                    # 300 items from inside row 0 across two row ends, every other one
            a0 = max(3, o.num_per - 50)
            items = list(range(a0, a0 + 300)) + list(range(5 * o.num_per, 7 * o.num_per, 2))
            held = None
            t_want = _table_without(sp, c, items)
        arm()
        sp.paths_taken()
        p = S.params(c["cfg"])
        tables = []
        for window in (SMALL_WINDOW, WINDOW_DEFAULT):
            db, mask = _load(sp, S, c, p, form, 0, held)
            if name == "packed-batch-copy":
                assert db.prepare_batch() and db.batch_copy_bytes() != 0
            with switch(sp, "db_load_window", window, default=WINDOW_DEFAULT):
                assert db.remove_items(items) == len(set(items))
            got, present = db.item_digests(SEED)
            assert (got == t_want).all() and (present != 0).tolist() == ([i >= 260 for i in range(o.num_items)] if form == "sparse" else [True] * o.num_items)
            if name == "packed-batch-copy":
                assert db.batch_copy_bytes() != 0 and (db.item_digests(SEED, which="batch_copy")[0] == t_want).all()
            if form == "sparse":
                assert db.sparse_items() == o.num_items - 260
            tables.append(got)
        assert (tables[0] == tables[1]).all()
        return sp.paths_taken()
    flow.__name__ = "db_remove_windows_" + name
    return flow


@pytest.mark.parametrize("name", list(WINDOWED))
def test_record_lists_across_windows(sp, oracle_mod, name):
    _window_flow(name)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "planar", "sparse"])
def test_remove_range(sp, oracle_mod, form):
    c = _case(sp, oracle_mod, "A")
    o, p = c["o"], c["p"]
    npr = o.num_per
    held = _third(o, [3, 4, 5]) if form == "sparse" else np.ones(o.num_items, dtype=bool)
    db, mask = _load(sp, _Own(sp), c, p, form, 0, held)
    gone = np.zeros(o.num_items, dtype=bool)
    for a, n in ((2 * npr, 2 * npr), (5 * npr + 7, npr + 30), (o.num_items - npr - 9, None), (17, 0)):
        hit = np.zeros(o.num_items, dtype=bool)
        hit[a:o.num_items if n is None else a + n] = True
        fresh = hit & mask & ~gone if form == "sparse" else hit & mask      # (a dense handle holds a removed item still)
        assert db.remove_range(a, n) == int(fresh.sum()), (a, n)
        gone |= hit
        after = mask & ~gone if form == "sparse" else mask
        got, present = db.item_digests(SEED)
        assert (present != 0).tolist() == after.tolist()
        assert (got == np.where(after[:, None], _table_without(sp, c, np.flatnonzero(gone)), 0).astype(np.uint64)).all(), (a, n)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_trim(sp, oracle_mod):
    b = _bucket_case(sp, oracle_mod)
    c = b["c"]
    o, p = c["o"], c["p"]
    gpp = sp.PublicParameters.deserialize(p, b["pp"])
    slot = 4 * N * 8
    db = _filled(sp, b, keys=list(range(o.num_items)))                            # 512 keys: a full store of 512 slots
    assert db.device_bytes() == 512 * slot
    assert db.trim() == 0
    keep = [i for i in range(o.num_items) if i % 4 == 1]
    assert db.remove_items([i for i in range(o.num_items) if i % 4 != 1]) == 384
    _bucket_check(sp, oracle_mod, b, db, gpp, set(keep), [keep[5], 0])
    assert db.device_bytes() == 512 * slot
    assert db.trim() == (512 - 128) * slot and db.device_bytes() == 128 * slot    # 64 * 2^k >= 128
    _bucket_check(sp, oracle_mod, b, db, gpp, set(keep), [keep[5], keep[-1], 0])
    assert db.trim() == 0
    db.update_item(0, c["file"][0].tobytes())                                     # slot 128: the store doubles again
    assert db.device_bytes() == 256 * slot
    _bucket_check(sp, oracle_mod, b, db, gpp, set(keep) | {0}, [0, keep[-1]])
    assert db.remove_range(0) == 129 and db.trim() == (256 - 64) * slot and db.device_bytes() == 64 * slot
    assert sp.Database.sparse(p).trim() == 0                                      # a fresh handle: nothing to shrink
    dense = sp.Database(p)
    with pytest.raises(sp.SpiralError) as e:
        dense.trim()
    assert e.value.rc == SP_E_ARG
    freed = C.c_size_t(0xCCCC)
    assert sp.lib().sp_db_sparse_trim(None, C.byref(freed)) == SP_E_ARG and freed.value == 0
    assert sp.lib().sp_db_sparse_trim(C.c_void_p(db.h), None) == 0


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["words8", "sparse"])
def test_errors_write_nothing(sp, oracle_mod, form):
    c = _case(sp, oracle_mod, "P")
    o, p = c["o"], c["p"]
    db, mask = _load(sp, _Own(sp), c, p, form, 0, _third(o, [1, 2, 3]))
    before, present_before = db.item_digests(SEED)
    L, n_items = sp.lib(), o.num_items
    some = [int(i) for i in np.flatnonzero(mask)[:4]]

    def items(lst, n=None):
        arr = (C.c_size_t * max(len(lst), 1))(*lst)
        removed = C.c_size_t(0xCCCC)
        rc = L.sp_db_remove_items(C.c_void_p(db.h), arr if lst is not None else None, C.c_size_t(len(lst) if n is None else n), C.byref(removed))
        return rc, removed.value

    def rng(h, item0, count):
        removed = C.c_size_t(0xCCCC)
        return L.sp_db_remove_range(C.c_void_p(h), C.c_size_t(item0), C.c_size_t(count), C.byref(removed)), removed.value

    def same():
        got, present = db.item_digests(SEED)
        return (got == before).all() and (present == present_before).all()

    assert items(some[:2] + [n_items] + some[2:]) == (SP_E_ARG, 0) and same()     # in the middle of a list
    assert items(some + [2 ** 64 - 1]) == (SP_E_ARG, 0) and same()
    assert rng(db.h, n_items - 1, 2) == (SP_E_ARG, 0) and rng(db.h, n_items + 1, 0) == (SP_E_ARG, 0) and rng(db.h, 2 ** 64 - 1, 2) == (SP_E_ARG, 0)
    assert rng(None, 0, 1) == (SP_E_ARG, 0) and same()
    removed = C.c_size_t(0xCCCC)
    assert L.sp_db_remove_items(C.c_void_p(db.h), None, C.c_size_t(3), C.byref(removed)) == SP_E_ARG and removed.value == 0     # a null list
    assert L.sp_db_remove_items(None, None, C.c_size_t(0), C.byref(removed)) == SP_E_ARG
    assert same()
    with pytest.raises(sp.SpiralError) as e:
        db.remove_items(some + [n_items])
    assert e.value.rc == SP_E_ARG and same()
    assert L.sp_db_remove_items(C.c_void_p(db.h), None, C.c_size_t(0), C.byref(removed)) == 0 and removed.value == 0
    assert items([]) == (0, 0) and rng(db.h, 9, 0) == (0, 0) and rng(db.h, n_items, 0) == (0, 0) and same()
    arr = (C.c_size_t * 2)(some[0], some[0])
    assert L.sp_db_remove_items(C.c_void_p(db.h), arr, C.c_size_t(2), None) == 0  # removed may be NULL
    after, present = db.item_digests(SEED)
    want = before.copy()
    want[some[0]] = _table_without(sp, c, [some[0]])[some[0]] if form == "words8" else 0
    assert (after == want).all() and int(present[some[0]]) == (1 if form == "words8" else 0)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_repair_from_removes_the_extra_keys(sp, oracle_mod):
    b = _bucket_case(sp, oracle_mod)
    keys, spare, c = b["keys"], b["spare"], b["c"]
    src = _filled(sp, b, keys=keys[:30])
    extra = [keys[33], spare[0], keys[38]]
    replica = _filled(sp, b, keys=keys[:25] + extra)
    replica.update_item(keys[2], b"stale")
    want_todo = sorted([keys[2]] + keys[25:30])
    todo, gone = replica.repair_from(src, SEED)                                   # the default: reported, left alone
    assert todo.tolist() == want_todo and gone.tolist() == sorted(extra)
    assert replica.sparse_items() == 33
    todo, gone = replica.repair_from(src, SEED, remove=True)
    assert todo.size == 0 and gone.tolist() == sorted(extra)
    assert replica.sparse_items() == src.sparse_items() == 30
    (ta, pa), (tb, pb) = src.item_digests(SEED), replica.item_digests(SEED)
    assert (ta == tb).all() and (pa == pb).all()
    todo, gone = replica.repair_from(src, SEED, remove=True)
    assert todo.size == 0 and gone.size == 0
    dense = sp.Database(c["p"]).load(c["words"].reshape(-1))                      # a dense self has no such items
    todo, gone = dense.repair_from(sp.Database(c["p"]).load(c["words"].reshape(-1)), SEED, remove=True)
    assert todo.size == 0 and gone.size == 0 and (dense.item_digests(SEED)[0] == c["t_src"]).all()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_server_removes_beside_lists_in_flight(sp, oracle_mod):
    b = _bucket_case(sp, oracle_mod)
    keys, c = b["keys"], b["c"]
    o, p = c["o"], c["p"]
    gone = [keys[0], keys[20], keys[31]]
    asked = [keys[0], keys[39], keys[20], keys[5]]
    qs = [b["cl"].generate_query(i, 900 + k) for k, i in enumerate(asked)]
    flavours = []
    for held in (keys, [k for k in keys if k not in gone]):
        bucket = oracle_mod.SparseDb(o)
        for i in held:
            bucket.update_item_raw(i, c["file"][i].tobytes())
        flavours.append([bucket.process_query(b["pp"], q) for q in qs])
    assert flavours[0] != flavours[1]
    db = _filled(sp, b)
    srv = sp.Server(p, db)
    uuid = srv.setup(b["pp"])
    reqs = [uuid.encode() + q for q in qs]
    assert srv.private_read(reqs) == flavours[0]
    other = _filled(sp, b)
    with pytest.raises(sp.SpiralError) as e:
        srv.remove_items(other, gone)                                             # not the server's handle
    assert e.value.rc == SP_E_ARG and other.sparse_items() == 40 and db.sparse_items() == 40
    with pytest.raises(sp.SpiralError) as e:
        srv.remove_items(db, [o.num_items])
    assert e.value.rc == SP_E_ARG
    lists, begun, stop = [], threading.Event(), threading.Event()

    def ask():
        while not stop.is_set():
            begun.set()
            lists.append(srv.private_read(reqs))

    t = threading.Thread(target=ask)
    t.start()
    try:
        assert begun.wait(120)
        begun.clear()
        assert begun.wait(120)                                                    # a list is under way
        assert srv.remove_items(db, gone + gone[:1]) == 3
        begun.clear()
        assert begun.wait(120)
        begun.clear()
        assert begun.wait(120)                                                    # (a whole list has run behind the removal)
    finally:
        stop.set()
        t.join()
    assert all(got in flavours for got in lists)                                  # wholly before or wholly after
    assert lists[0] == flavours[0] and lists[-1] == flavours[1]
    k = lists.index(flavours[1])
    assert all(got == flavours[1] for got in lists[k:])
    assert srv.private_read(reqs) == flavours[1] and db.sparse_items() == 37


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
HARDENED = {"form-packed": _form_flow("A", "packed"), "form-sparse": _form_flow("A", "sparse"),
            "windows-packed-batch-copy": _window_flow("packed-batch-copy"), "windows-planar": _window_flow("planar"),
            "windows-words8": _window_flow("words8"), "windows-sparse": _window_flow("sparse")}


@pytest.mark.parametrize("mode", ["poison", "poison-ff", "guard"])
@pytest.mark.parametrize("what", list(HARDENED))
def test_on_hardened_buffers(sp, oracle_mod, capfd, what, mode):
    from test_gpu_hardened_buffers import POISON, _hardened
    _hardened(HARDENED[what], mode.split("-")[0], 0xFF if mode == "poison-ff" else POISON, oracle_mod, capfd)
