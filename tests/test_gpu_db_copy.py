"""Items copied between resident databases on the device (sp_db_copy_items / Database.copy_from) and a running request layer switched
to the copy (sp_server_replace_db / Server.replace_db).  Every comparison is exact, and the witness for the expected words is never
the library's own read-back of `src`: it is the ORACLE's words that `src` was loaded from (load_db_from_bytes -> sp_db_load; for a
sparse `src`, the same file's items), sp_synth_word for synthetic contents, or the oracle's words of the records a sparse `dst` held.

1  every ordered pair of forms a parameter set offers (A: 64 x 128 -- PACKED, planar-resident, sparse, PACKED row shards, column shards,
   sparse shards; B: 256 x 16 -- 8-byte words, sparse, 8-byte row shards; C: 128 x 128 -- planar shards, PACKED): dst is pre-filled with
   other content, the whole range is copied, and at every coordinate dst holds src's word where both hold the item, else its old one:
   the per-item digest tables, read_ref at the corner words, `copied`, sparse_items, and the shards' tables adding up.
2  ranges across windows so small that a range spans at least three; then one call under the shipped window.
3  words that export_rows refuses (sp_db_fill_synthetic).
4  spill coefficients (db_item_size no multiple of the chunk count) survive: the oracle's response bytes for the file-loaded database.
5  queries after a copy, alone and in a list of 9, on dense and sparse destinations and beside a standing batch copy.
6  errors write nothing.
7  a copy beside a running list on `src`.
8  a server switched from a filled sparse bucket to its PACKED copy, lists in flight around the switch.
9  cases of 1 and 2 on poisoned and on guarded buffers (the procedure of tests/test_gpu_hardened_buffers.py).
tests/test_emulated_db_copy.py runs a subset on the emulated device."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from conftest import FAST
from test_gpu_item_readback import N, WINDOW_DEFAULT, _body, _no_switch, _Own, _sparse_records
from test_gpu_narrow_batch import switch
from test_gpu_planar_shards import _cfg as _planar_cfg

pytestmark = pytest.mark.gpu

Q0, Q1 = 268369921, 249561089
SP_E_ARG, SP_E_STATE = -1, -4
SEED = 0x5EEDC0DE          # of the digests
SYNTH = 0xB0B              # of a dense destination's old words
PACKED = dict(FAST, nu_1=6, nu_2=7, db_item_size=256)          # 64 x 128: PACKED, planar-capable and sparse-capable at once
WORDS8 = dict(FAST, nu_1=8, nu_2=4, db_item_size=256)          # 256 x 16: 8-byte words
SMALLEST = dict(FAST, nu_1=2, nu_2=7, t_gsw=2, db_item_size=256)   # 4 x 128: the smallest PACKED shape
CHUNKS = dict(FAST, nu_1=4, nu_2=8, db_item_size=256)          # 16 x 256: two 128-column chunks
NARROW = dict(FAST, db_item_size=256)                          # 64 x 4
SPARSE = dict(FAST, nu_1=6, nu_2=3, db_item_size=256)
SETS = {"A": (PACKED, ("packed", "planar", "sparse", "row-shards", "column-shards", "sparse-shards")),
        "B": (WORDS8, ("words8", "sparse", "row-shards")),
        "C": (_planar_cfg(7, 7), ("planar-shards", "packed")),
        "S": (SMALLEST, ("packed", "row-shards")),
        "P": (SPARSE, ("words8", "sparse", "sparse-shards"))}
SHARDS = {"row-shards": 2, "column-shards": 2, "sparse-shards": 2, "planar-shards": 2}


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _canon(w):
    w = np.asarray(w, dtype=np.uint64)
    return (w & np.uint64(0xffffffff)) % np.uint64(Q0) | (((w >> np.uint64(32)) % np.uint64(Q1)) << np.uint64(32))


def _make(sp, S, p, form, s):
    D = sp.Database
    if form in ("packed", "words8"):
        return S.own(D(p))
    if form == "planar":
        return S.own(D.planar(p))
    if form == "sparse":
        return S.own(D.sparse(p))
    if form == "row-shards":
        return S.own(D(p, s, 2))
    if form == "column-shards":
        return S.own(D(p, s, 2, by_columns=True))
    if form == "planar-shards":
        return S.own(D.planar_shard(p, s, 2))
    assert form == "sparse-shards"
    return S.own(D.sparse(p, s, 2))


def _shape_mask(form, o, s):
    """which items the shape of shard `s` of a form holds -> bool array over the items"""
    i = np.arange(o.num_items)
    if form == "column-shards":
        return (i % o.num_per) % 2 == s
    if form in SHARDS:
        return (i // o.num_per) // (o.dim0 // 2) == s
    return np.ones(o.num_items, dtype=bool)


def _table(sp, p, o, words):
    """the host's per-item digest table of reference words (no device call)"""
    w = np.asarray(words, dtype=np.uint64).reshape(4, -1)
    acc = np.zeros((o.num_items, 2), dtype=np.uint64)
    for plane in range(4):
        sp.item_digests_ref_words(p, SEED, plane, 0, w[plane], acc)
    return acc


def _synth_table(sp, p, o, seed):
    acc = np.zeros((o.num_items, 2), dtype=np.uint64)
    per_z = o.num_items
    step = min(N, max(1, (1 << 22) // per_z))
    for plane in range(4):
        for z0 in range(0, N, step):
            idx = np.arange((plane * N + z0) * per_z, (plane * N + z0 + step) * per_z, dtype=np.uint64)
            sp.item_digests_ref_words(p, SEED, plane, z0, sp.spiral.synth_words(seed, idx), acc)
    return acc


_cases = {}


def _case(sp, oracle_mod, name):
    """the oracle's and the host's side of a parameter set, computed once and never changed: the file `src` holds and its words, the
    scattered third a sparse `src` holds, the table of a dense dst's old (synthetic) words, the records and table of a sparse dst's"""
    if name not in _cases:
        cfg = SETS[name][0]
        o, p = oracle_mod.Params(cfg), sp.Params(cfg)
        rng = np.random.default_rng(101)
        file = rng.integers(0, 256, (o.num_items, o.db_item_size), dtype=np.uint8)
        words = o.load_db_from_bytes(file.tobytes())
        third = np.zeros(o.num_items, dtype=bool)
        third[[i for i, _ in _sparse_records(o)]] = True
        third[[0, o.num_items - 1]] = True                       # the corners of the item range are in it
        old_recs = [(i, d.ljust(o.db_item_size, b"\0")) for i, d in _sparse_records(o, seed=29)]
        old_file = np.zeros((o.num_items, o.db_item_size), dtype=np.uint8)
        old_held = np.zeros(o.num_items, dtype=bool)
        for i, d in old_recs:
            old_file[i] = np.frombuffer(d, dtype=np.uint8)
            old_held[i] = True
        _cases[name] = dict(cfg=cfg, o=o, p=p, file=file, words=words.reshape(4, N, o.num_per, o.dim0), third=third,
                            t_src=_table(sp, p, o, words), t_synth=_synth_table(sp, p, o, SYNTH), old_recs=old_recs, old_held=old_held,
                            t_old=_table(sp, p, o, o.load_db_from_bytes(old_file.tobytes())))
    return _cases[name]


def _sources(sp, S, c, form, p):
    """the shards of `src` in a form, loaded from the oracle's words (a sparse one: the file's items of the scattered third, whose
    words are the oracle's) -> [(handle, held mask)]"""
    o = c["o"]
    out = []
    for s in range(SHARDS.get(form, 1)):
        db, mask = _make(sp, S, p, form, s), _shape_mask(form, o, s)
        if form.startswith("sparse"):
            mask = mask & c["third"]
            db.update_items([(int(i), c["file"][i].tobytes()) for i in np.flatnonzero(mask)])
        else:
            db.load(c["words"].reshape(-1))
        out.append((db, mask))
    return out


def _destinations(sp, S, c, form, p):
    """the shards of `dst`, pre-filled with other content -> [(handle, shape mask, held before, table before)]"""
    o = c["o"]
    out = []
    for s in range(SHARDS.get(form, 1)):
        db, mask = _make(sp, S, p, form, s), _shape_mask(form, o, s)
        if form.startswith("sparse"):
            held = mask & c["old_held"]
            db.update_items([(i, d) for i, d in c["old_recs"] if held[i]])
            out.append((db, mask, held, c["t_old"]))
        else:
            db.fill_synthetic(SYNTH)
            out.append((db, mask, mask, c["t_synth"]))
    return out


def _corner_words(c, dst, mask, src_held, form):
    """read_ref at the corner words of a dense dst: first and last z, first and last column it holds, the rows at either side of a quad
    and of a 16-row group -- src's oracle word where both hold the item, else the old synthetic word"""
    o = c["o"]
    j_lo = int(np.flatnonzero(mask)[0]) // o.num_per
    j_hi = int(np.flatnonzero(mask)[-1]) // o.num_per
    cols = [ii for ii in (0, 1, o.num_per - 2, o.num_per - 1) if mask[j_lo * o.num_per + ii]]
    assert cols
    rows = sorted({j for j in (j_lo, j_lo + 1, j_lo + 2, j_lo + 15, j_lo + 16, j_hi - 1, j_hi) if j_lo <= j <= j_hi})
    for plane in (0, 3):
        for z in (0, N - 1):
            for ii in cols:
                got = dst.read_ref(plane, z, ii, 0, j_hi - j_lo + 1)
                for j in rows:
                    i = j * o.num_per + ii
                    want = (_canon(c["words"][plane, z, ii, j]) if src_held[i] else
                            np.uint64(sp_synth(SYNTH, ((plane * N + z) * o.num_per + ii) * o.dim0 + j)))
                    assert got[j - j_lo] == want, (form, plane, z, ii, j)


def sp_synth(seed, idx):
    import sdk_amd
    return sdk_amd.spiral.synth_word(seed, idx)


def _pair_flow(set_name, src_form, dst_form, item0=0, count=None):
    def flow(sp, oracle_mod, S, arm):
        c = _case(sp, oracle_mod, set_name)
        o = c["o"]
        arm()
        sp.paths_taken()
        p = S.params(c["cfg"])                                  # (the device handles' own: c["p"] serves the host's tables)
        srcs = _sources(sp, S, c, src_form, p)
        dsts = _destinations(sp, S, c, dst_form, p)
        in_range = np.zeros(o.num_items, dtype=bool)
        in_range[item0:o.num_items if count is None else item0 + count] = True
        src_held = np.zeros(o.num_items, dtype=bool)
        for _, m in srcs:
            src_held |= m
        total = np.zeros((o.num_items, 2), dtype=np.uint64)
        for dst, mask, held, t_before in dsts:
            copied = sum(dst.copy_from(src, item0, count) for src, _ in srcs)
            written = mask & src_held & in_range
            assert copied == int(written.sum()), (src_form, dst_form)
            held_after = held | written
            want = np.where(written[:, None], c["t_src"], t_before)
            want = np.where(held_after[:, None], want, 0).astype(np.uint64)
            got, present = dst.item_digests(SEED)
            assert (present != 0).tolist() == held_after.tolist(), (src_form, dst_form)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (src_form, dst_form, bad[:8].tolist(), int(bad.size))
            if dst_form.startswith("sparse"):
                assert dst.sparse_items() == int(held_after.sum())
            else:
                _corner_words(c, dst, mask, written, dst_form)
            with np.errstate(over="ignore"):
                total += got
        # the shards' tables add up to the unsharded table of the expected words
        all_written = src_held & in_range
        if dst_form.startswith("sparse"):
            whole = np.where(all_written[:, None], c["t_src"], np.where(c["old_held"][:, None], c["t_old"], 0))
        else:
            whole = np.where(all_written[:, None], c["t_src"], c["t_synth"])
        assert (total == whole.astype(np.uint64)).all()
        return sp.paths_taken()
    flow.__name__ = "db_copy_%s_%s_to_%s" % (set_name, src_form, dst_form)
    return flow


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
PAIRS = [(s, a, b) for s in ("A", "B", "C") for a in SETS[s][1] for b in SETS[s][1]]
PAIRS += [("S", "packed", "packed"), ("S", "row-shards", "packed"), ("S", "packed", "row-shards"),   # the smallest PACKED shape
          ("P", "sparse", "words8"), ("P", "words8", "sparse"), ("P", "sparse-shards", "sparse")]   # the narrow sparse shape


@pytest.mark.parametrize("set_name,src_form,dst_form", PAIRS, ids=["%s-%s-to-%s" % t for t in PAIRS])
def test_every_pair_of_forms(sp, oracle_mod, set_name, src_form, dst_form):
    _pair_flow(set_name, src_form, dst_form)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
RANGED = {"packed-16x256": (CHUNKS, "packed"), "planar-64x128": (PACKED, "planar"), "narrow": (NARROW, "words8")}
SETS.update({"R-" + k: (cfg, (form,)) for k, (cfg, form) in RANGED.items()})


def _ranges(o):
    npr = o.num_per
    g0 = 17 if o.dim0 >= 32 else 1                  # rows inside one 16-row group
    r = [(npr + 1, 1),                              # one item at an odd index
         (2 * npr + 1, 2 * npr - 3),                # starts and ends inside the row pair (2, 3)
         (npr - 3, 2 * npr + 9),                    # from the end of row 0 into row 3
         (o.num_items - 1, 1),                      # the last item
         (g0 * npr + 2, 3 * npr - 1)]               # starts and ends inside a 16-row group
    if npr > 128:
        r.append((4 * npr + 100, 60))               # crosses a 128-column chunk inside a row
    return r


def _ranged_flow(name):
    def flow(sp, oracle_mod, S, arm):
        cfg, form = RANGED[name]
        c = _case(sp, oracle_mod, "A" if cfg is PACKED else "R-" + name)
        o = c["o"]
        arm()
        sp.paths_taken()
        p = S.params(c["cfg"])
        src_form = "packed" if form == "planar" else form     # (planar from PACKED words, the others from their own form)
        src = _make(sp, S, p, src_form, 0).load(c["words"].reshape(-1))
        dst = _make(sp, S, p, form, 0).fill_synthetic(SYNTH)
        assert dst.format() == form
        want = c["t_synth"].copy()
        per_item = 80 + 4 * N * 8                   # a record, a patch cell and the staged words of an item
        with switch(sp, "db_load_window", 64 + max(1, (2 * o.num_per - 3) // 4) * per_item, default=WINDOW_DEFAULT):
            for a, n in _ranges(o):
                assert dst.copy_from(src, a, n) == n
                want[a:a + n] = c["t_src"][a:a + n]
                got, present = dst.item_digests(SEED)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert present.all() and bad.size == 0, (a, n, bad[:8].tolist(), int(bad.size))
        a, n = 3, 2 * o.num_per                     # the buffer grows back before the first kernel of this call
        assert dst.copy_from(src, a, n) == n
        want[a:a + n] = c["t_src"][a:a + n]
        assert (dst.item_digests(SEED)[0] == want).all()
        assert dst.copy_from(src, 5, 0) == 0
        return sp.paths_taken()
    flow.__name__ = "db_copy_ranges_" + name
    return flow


@pytest.mark.parametrize("name", list(RANGED))
def test_ranges_across_small_windows(sp, oracle_mod, name):
    _ranged_flow(name)(sp, oracle_mod, _Own(sp), _no_switch)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_words_that_export_refuses(sp, oracle_mod):
    c = _case(sp, oracle_mod, "A")
    o, p = c["o"], c["p"]
    src = sp.Database(p).fill_synthetic(SYNTH)
    assert src.format() == "packed"
    with pytest.raises(sp.SpiralError) as e:
        src.export_rows(0, 8)
    assert e.value.rc == SP_E_STATE
    whole = src.digest(SEED)
    rng = np.random.default_rng(5)
    for form in ("planar", "sparse", "column-shards"):
        parts = np.zeros_like(whole)
        for s in range(SHARDS.get(form, 1)):
            dst = _make(sp, _Own(sp), p, form, s)
            mask = _shape_mask(form, o, s)
            assert dst.format() == {"planar": "planar", "sparse": "sparse", "column-shards": "words8"}[form]
            assert dst.copy_from(src) == int(mask.sum())
            with np.errstate(over="ignore"):
                parts += dst.digest(SEED)
            got, present = dst.item_digests(SEED)
            assert (present != 0).tolist() == mask.tolist() and (got == np.where(mask[:, None], c["t_synth"], 0)).all()
            if form != "sparse":
                for _ in range(24):
                    plane, z, ii = int(rng.integers(4)), int(rng.integers(N)), int(rng.integers(o.num_per // 2)) * 2 + s % 2
                    got = dst.read_ref(plane, z, ii, 0, o.dim0)
                    idx = ((plane * N + z) * o.num_per + ii) * o.dim0 + np.arange(o.dim0, dtype=np.uint64)
                    assert (got == sp.spiral.synth_words(SYNTH, idx)).all(), (form, plane, z, ii)
        assert (parts == whole).all(), form
    with pytest.raises(sp.SpiralError) as e:             # still refused afterwards
        src.export_rows()
    assert e.value.rc == SP_E_STATE


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1001, 5])
def test_spill_coefficients_survive(sp, oracle_mod, size):
    cfg = dict(FAST, nu_1=4, nu_2=1, db_item_size=size)
    o, p = oracle_mod.Params(cfg), sp.Params(cfg)
    blob = np.random.default_rng(size).integers(0, 256, o.num_items * size, dtype=np.uint8).tobytes()
    words = o.load_db_from_bytes(blob)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(31)
    gpp = sp.PublicParameters.deserialize(p, pp)
    src = sp.Database(p).load_items(blob)
    dst = sp.Database(p).fill_synthetic(SYNTH)
    assert dst.copy_from(src) == o.num_items
    t = np.zeros((o.num_items, 2), dtype=np.uint64)
    for plane in range(4):
        sp.item_digests_ref_words(p, SEED, plane, 0, words.reshape(4, -1)[plane], t)
    assert (dst.item_digests(SEED)[0] == t).all()
    for k, idx in enumerate((0, 7, o.num_items - 1)):
        q = cl.generate_query(idx, 90 + k)
        assert sp.process_query(p, gpp, q, dst) == o.process_query(pp, q, words), idx


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
_served = {}


def _served_case(sp, oracle_mod):
    """set A's file served by the oracle: nine queries over the dense database, two over lib/server's bucket of the scattered third"""
    if not _served:
        c = _case(sp, oracle_mod, "A")
        o = c["o"]
        cl = oracle_mod.Client(o)
        pp = cl.generate_keys(71)
        stored = [int(i) for i in np.flatnonzero(c["third"])]
        idxs = [stored[9], (stored[9] + 1) % o.num_items, 0, o.num_items - 1, stored[40], 1234, 4097, 8000, stored[-2]]
        qs = [cl.generate_query(i, 500 + k) for k, i in enumerate(idxs)]
        bucket = oracle_mod.SparseDb(o)
        for i in stored:
            bucket.update_item_raw(i, c["file"][i].tobytes())
        flat = c["words"].reshape(-1)
        from test_gpu_hardened_buffers import _many
        _served.update(cl=cl, pp=pp, idxs=idxs, qs=qs, stored=stored, dense=_many(lambda q: o.process_query(pp, q, flat), qs),
                       sparse=_many(lambda q: bucket.process_query(pp, q), qs))
    return _served


def test_queries_after_a_copy(sp, oracle_mod):
    c, m = _case(sp, oracle_mod, "A"), _served_case(sp, oracle_mod)
    o, p = c["o"], c["p"]
    gpp = sp.PublicParameters.deserialize(p, m["pp"])
    packed = sp.Database(p).load(c["words"].reshape(-1))
    planar = sp.Database.planar(p)
    assert planar.copy_from(packed) == o.num_items
    back = sp.Database(p).fill_synthetic(SYNTH)
    assert back.copy_from(planar) == o.num_items and back.format() == "packed"
    for db in (planar, back):
        assert sp.process_query(p, gpp, m["qs"][0], db) == m["dense"][0]
        assert sp.process_query_batch(p, [gpp] * 9, m["qs"], db) == m["dense"]
    # sparse to sparse: lib/server's bytes
    bucket = sp.Database.sparse(p)
    bucket.update_items([(i, c["file"][i].tobytes()) for i in m["stored"]])
    moved = sp.Database.sparse(p)
    assert moved.copy_from(bucket) == len(m["stored"]) == moved.sparse_items()
    assert [sp.process_query(p, gpp, q, moved) for q in m["qs"][:2]] == m["sparse"][:2]
    assert sp.process_query_batch(p, [gpp] * 9, m["qs"], moved) == m["sparse"]
    # a PACKED dst with its batch copy standing: a ranged copy keeps the copy valid
    dst = sp.Database(p).fill_synthetic(SYNTH)
    assert dst.prepare_batch() and dst.batch_copy_bytes() != 0
    a = o.num_per + 5
    assert dst.copy_from(packed, 0, a) == a
    assert dst.batch_copy_bytes() != 0 and (dst.digest(SEED, which="batch_copy") == dst.digest(SEED)).all()
    assert dst.copy_from(packed, a, o.num_items - a) == o.num_items - a
    assert dst.batch_copy_bytes() != 0 and (dst.digest(SEED, which="batch_copy") == dst.digest(SEED)).all()
    assert (dst.item_digests(SEED, which="batch_copy")[0] == c["t_src"]).all()
    assert sp.process_query_batch(p, [gpp] * 9, m["qs"], dst) == m["dense"]


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(sp, oracle_mod):
    c = _case(sp, oracle_mod, "R-narrow")
    o, p = c["o"], c["p"]
    src = sp.Database(p).load(c["words"].reshape(-1))
    dst = sp.Database(p).fill_synthetic(SYNTH)
    other = sp.Database(sp.Params(c["cfg"])).fill_synthetic(3)       # same configuration, another params handle
    before = dst.digest(SEED).copy()
    L = sp.lib()

    def raw(d, s, item0, count):
        copied = C.c_size_t(0xCCCC)
        rc = L.sp_db_copy_items(C.c_void_p(d), C.c_void_p(s), C.c_size_t(item0), C.c_size_t(count), C.byref(copied))
        return rc, copied.value

    for d, s, item0, count in ((dst.h, dst.h, 0, 4), (dst.h, other.h, 0, 4), (other.h, src.h, 0, 4), (dst.h, src.h, o.num_items - 1, 2),
                               (dst.h, src.h, 2 ** 64 - 1, 2), (dst.h, src.h, o.num_items + 1, 0), (None, src.h, 0, 4), (dst.h, None, 0, 4)):
        assert raw(d, s, item0, count) == (SP_E_ARG, 0), (item0, count)
        assert (dst.digest(SEED) == before).all()
    with pytest.raises(sp.SpiralError) as e:
        dst.copy_from(dst)
    assert e.value.rc == SP_E_ARG
    assert raw(dst.h, src.h, 9, 0) == (0, 0) and raw(dst.h, src.h, o.num_items, 0) == (0, 0)
    assert L.sp_db_copy_items(C.c_void_p(dst.h), C.c_void_p(src.h), C.c_size_t(0), C.c_size_t(0), None) == 0
    assert (dst.digest(SEED) == before).all()
    assert L.sp_db_copy_items(C.c_void_p(dst.h), C.c_void_p(src.h), C.c_size_t(7), C.c_size_t(3), None) == 0     # copied may be NULL
    want = c["t_synth"].copy()
    want[7:10] = c["t_src"][7:10]
    assert (dst.item_digests(SEED)[0] == want).all()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_copy_beside_a_running_list_on_src(sp, oracle_mod):
    c, m = _case(sp, oracle_mod, "A"), _served_case(sp, oracle_mod)
    o, p = c["o"], c["p"]
    gpp = sp.PublicParameters.deserialize(p, m["pp"])
    src = sp.Database(p).load(c["words"].reshape(-1))
    dsts = [sp.Database.planar(p), sp.Database(p).fill_synthetic(SYNTH)]
    out = {}

    def ask():
        out["responses"] = [sp.process_query_batch(p, [gpp] * 9, m["qs"], src) for _ in range(2)]

    def copy():
        out["copied"] = [d.copy_from(src) for d in dsts]

    threads = [threading.Thread(target=ask), threading.Thread(target=copy)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out["responses"] == [m["dense"]] * 2
    assert out["copied"] == [o.num_items] * 2
    for d in dsts:
        assert (d.item_digests(SEED)[0] == c["t_src"]).all()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_server_switches_to_the_copy(sp, oracle_mod):
    c, m = _case(sp, oracle_mod, "A"), _served_case(sp, oracle_mod)
    o, p, cl = c["o"], c["p"], m["cl"]
    bucket = sp.Database.sparse(p)
    srv = sp.Server(p, bucket)
    srv.update_row(_body([(i, c["file"][i].tobytes()) for i in m["stored"]]))
    uuid = srv.setup(m["pp"])
    reqs = [uuid.encode() + q for q in m["qs"]]
    assert srv.private_read(reqs) == m["sparse"]
    # the dense destination holds the bucket's items and zeros elsewhere: what the oracle answers over that file
    file = np.where(c["third"][:, None], c["file"], 0).astype(np.uint8)
    words = o.load_db_from_bytes(file.tobytes())
    dense = [o.process_query(m["pp"], q, words) for q in m["qs"]]
    dst = sp.Database(p)
    assert dst.copy_from(bucket) == len(m["stored"])
    shard = sp.Database(p, 0, 2).fill_synthetic(SYNTH)
    with pytest.raises(sp.SpiralError) as e:
        srv.replace_db(shard)                                         # a row shard: SP_E_ARG, the server stays as it was
    assert e.value.rc == SP_E_ARG
    other = sp.Database(sp.Params(c["cfg"]))
    with pytest.raises(sp.SpiralError) as e:
        srv.replace_db(other)                                         # another params handle
    assert e.value.rc == SP_E_ARG
    assert srv.db is bucket and srv.private_read(reqs[:2]) == m["sparse"][:2]
    srv.replace_db(dst)
    got = srv.private_read(reqs)
    assert got == dense
    for k, i in enumerate(m["idxs"]):
        assert bytes(cl.decode_response(got[k]))[:o.db_item_size] == file[i].tobytes(), i
    new = (m["idxs"][2], bytes(range(256)))
    with pytest.raises(sp.SpiralError) as e:
        srv.update_row(_body([new]), db=bucket)                       # the old handle: SP_E_ARG
    assert e.value.rc == SP_E_ARG
    assert srv.private_read(reqs[2:3]) == dense[2:3]
    srv.update_row(_body([new]), db=dst)
    assert bytes(cl.decode_response(srv.private_read(reqs[2:3])[0]))[:256] == new[1]
    dst.update_item(new[0], file[new[0]].tobytes())
    # two host threads run lists around five switches: every list is wholly of one flavour -- one that served at some moment of the
    # list -- and at least one list was under way when a switch began (it had begun before, it ended after)
    srv.replace_db(bucket)
    clock = time.perf_counter
    flavour = {id(bucket): m["sparse"], id(dst): dense}
    lists = [[], []]                                                  # per thread: (begun, ended, responses)
    begun, stop = [threading.Event(), threading.Event()], threading.Event()

    def ask(k):
        while not stop.is_set():
            t0 = clock()
            begun[k].set()
            got = srv.private_read(reqs)
            lists[k].append((t0, clock(), got))

    def lists_under_way():
        """both threads have begun a list since this call began"""
        for ev in begun:
            ev.clear()
        for ev in begun:
            assert ev.wait(120)

    threads = [threading.Thread(target=ask, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    served = [(float("-inf"), None, bucket)]                          # (serves from at the earliest, until at the latest, handle)
    try:
        for rnd in range(5):
            target = dst if rnd % 2 == 0 else bucket
            lists_under_way()
            t0 = clock()
            srv.replace_db(target)
            t1 = clock()
            served[-1] = (served[-1][0], t1, served[-1][2])
            served.append((t0, None, target))
            lists_under_way()                                         # (the lists that were in flight have been recorded)
    finally:
        stop.set()
        for t in threads:
            t.join()
    served[-1] = (served[-1][0], float("inf"), served[-1][2])
    assert srv.db is dst and srv.private_read(reqs[:3]) == dense[:3]
    straddled = 0
    for per in lists:
        assert len(per) >= 5
        for b, e, got in per:
            allowed = [h for lo, hi, h in served if b <= hi and e >= lo]
            assert any(got == flavour[id(h)] for h in allowed), (b, e)
            straddled += any(b < lo < e for lo, _, _ in served[1:])
        assert per[0][2] == m["sparse"] and per[-1][2] == dense
    assert straddled >= 1, "no list was in flight when a switch began"


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
HARDENED = {"packed-to-planar": _pair_flow("A", "packed", "planar"), "sparse-to-packed": _pair_flow("A", "sparse", "packed"),
            "ranges-packed": _ranged_flow("packed-16x256"), "ranges-planar": _ranged_flow("planar-64x128"),
            "ranges-narrow": _ranged_flow("narrow")}


@pytest.mark.parametrize("mode", ["poison", "guard"])
@pytest.mark.parametrize("what", list(HARDENED))
def test_on_hardened_buffers(sp, oracle_mod, capfd, what, mode):
    from test_gpu_hardened_buffers import POISON, _hardened
    _case(sp, oracle_mod, "A")                                        # (the host's side: before any switch is set)
    _hardened(HARDENED[what], mode, POISON, oracle_mod, capfd)
