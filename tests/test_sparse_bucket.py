"""lib/server's sparse caller: a SparseDb bucket served by the GPU library, byte-identical to the
restatement of lib/server's process_query over the same SparseDb (oracle/sparse_server.cpp: pruned expansion,
multiply_reg_by_sparse_database, fold with the all-zero shortcuts, pack, encode)."""
import numpy as np
import pytest

from conftest import FAST


def _fill(o, oracle_mod, n_items, seed, item_bytes):
    rng = np.random.default_rng(seed)
    sdb = oracle_mod.SparseDb(o)
    items = {}
    for idx in rng.choice(o.num_items, n_items, replace=False):
        items[int(idx)] = rng.integers(0, 256, item_bytes, dtype=np.uint8).tobytes()
        sdb.update_item_raw(int(idx), items[int(idx)])
    return sdb, items


def test_sparse_oracle_semantics(oracle_mod):
    """CPU: the sparse restatement decodes present items; its bytes differ from spiral-rs's dense process_query over the
    zero-filled database exactly when fold.rs:38-44's shortcuts fire, i.e. when a whole column of the bucket is empty
    (with every column populated they coincide)."""
    cfg = dict(FAST, nu_1=4, nu_2=2, db_item_size=256)
    o = oracle_mod.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(3)
    sdb, items = _fill(o, oracle_mod, 2, 1, 256)    # at most 2 of the 4 columns hold anything: shortcuts fire
    idx = next(iter(items))
    q = cl.generate_query(idx, 4)
    r = sdb.process_query(pp, q)
    assert cl.decode_response(r)[:256] == items[idx]
    assert r != o.process_query(pp, q, sdb.to_dense())
    full, items_full = _fill(o, oracle_mod, o.num_items, 2, 256)      # nothing absent: no shortcut can fire
    q = cl.generate_query(5, 6)
    assert full.process_query(pp, q) == o.process_query(pp, q, full.to_dense())
    assert full.polys() == 4 * o.num_items


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n_items", [(dict(FAST, nu_1=9, nu_2=7, db_item_size=256), 655),
                                         (dict(FAST, nu_1=6, nu_2=4, db_item_size=16384, instances=2, version=1), 40),
                                         (dict(FAST, nu_1=3, nu_2=2, db_item_size=256, t_gsw=7, t_conv=3, t_exp_left=5, t_exp_right=5, q2_bits=22), 32)],
                         ids=["2^16-items-1pct", "two-instances-pack-v1", "full-bucket-server-gadgets"])
def test_sparse_bucket_matches_lib_server(oracle_mod, cfg, n_items):
    import sdk_amd as sp
    o = oracle_mod.Params(cfg)
    p = sp.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(11)
    gpp = sp.PublicParameters.deserialize(p, pp)
    sdb, items = _fill(o, oracle_mod, n_items, 5, cfg["db_item_size"])
    gdb = sp.Database.sparse(p)
    for idx, data in items.items():
        gdb.update_item(idx, data)
    assert gdb.sparse_items() == n_items == len(items)
    present = list(items)[:3]
    absent = next(i for i in range(o.num_items) if i not in items) if n_items < o.num_items else None
    for k, idx in enumerate(present + ([absent] if absent is not None else [])):
        q = cl.generate_query(idx, 70 + k)
        sp.paths_taken()
        resp = sp.process_query(p, gpp, q, gdb)
        taken = sp.paths_taken()
        assert {"sweep_sparse", "fold_fused"} <= taken and not ({"sweep_packed_persist", "sweep_narrow", "sweep_wide"} & taken), taken
        assert resp == sdb.process_query(pp, q), idx
        if idx in items and cfg.get("t_gsw", 8) == 8:
            chunks = cfg.get("instances", 1) * 4
            size = cfg["db_item_size"]
            got = cl.decode_response(resp)
            per = size // chunks
            assert all(got[t * per:(t + 1) * per] == items[idx][t * per:(t + 1) * per] for t in range(chunks)), idx
    # an upsert of an existing item and a new item; the next query sees both (index rebuilt)
    idx = present[0]
    newdata = bytes(reversed(items[idx]))
    gdb.update_item(idx, newdata)
    sdb.update_item_raw(idx, newdata)
    if absent is not None:
        gdb.update_item(absent, b"\x07" * 16)
        sdb.update_item_raw(absent, b"\x07" * 16)
        assert gdb.sparse_items() == n_items + 1
    q = cl.generate_query(idx, 99)
    assert sp.process_query(p, gpp, q, gdb) == sdb.process_query(pp, q)
    # the split API and the batch entry point on a sparse bucket
    run = sp.QueryRun(p, gpp, q, db=gdb).sweep(gdb)
    assert run.finish() == sdb.process_query(pp, q)
    run.free()
    assert sp.process_query_batch(p, gpp, [q, q], gdb) == [sdb.process_query(pp, q)] * 2
    with pytest.raises(sp.SpiralError):
        sp.QueryRun(p, gpp, q).sweep(gdb)          # begun without the bucket: its expansion was not pruned for it
    with pytest.raises(sp.SpiralError):
        gdb.fill_synthetic(1)


@pytest.mark.gpu
def test_sparse_sweep_time_scales_with_occupancy(oracle_mod):
    """the first-dimension step of a sparse bucket costs time in proportion to the items present"""
    import sdk_amd as sp
    import bench
    cfg = dict(FAST, nu_1=9, nu_2=7, db_item_size=256)
    p = sp.Params(cfg)
    pp = sp.PublicParameters.deserialize(p, bench.synthetic_wire_bytes(p.setup_bytes(), 1))
    q = bench.synthetic_wire_bytes(p.query_bytes(), 2)
    rng = np.random.default_rng(3)
    order = rng.permutation(1 << 16)
    gdb = sp.Database.sparse(p)
    times, filled = [], 0
    for target in (655, 2621, 10485):                 # 1 %, 4 %, 16 %
        for idx in order[filled:target]:
            gdb.update_item(int(idx), b"\x01\x02\x03")
        filled = target
        ms = []
        for _ in range(4):
            run = sp.QueryRun(p, pp, q, db=gdb).sweep(gdb)
            run.finish()
            ms.append(run.timings()[1])
            run.free()
        times.append(min(ms))
    print("sparse sweep ms at 1 / 4 / 16 %% occupancy: %s" % ["%.3f" % t for t in times])
    assert times[2] > 2.0 * times[0] and times[2] < 40 * times[0]


class _Bucket:
    """one sparse bucket on both sides: the GPU library's (sp_db_create_sparse + sp_db_update_item) and the oracle's restatement
    of lib/server (exact u128 first-dimension sums)"""

    def __init__(self, oracle_mod, cfg, key_seed=11):
        import sdk_amd as sp
        self.sp, self.cfg = sp, cfg
        self.o, self.p = oracle_mod.Params(cfg), sp.Params(cfg)
        self.cl = oracle_mod.Client(self.o)
        self.pp = self.cl.generate_keys(key_seed)
        self.gpp = sp.PublicParameters.deserialize(self.p, self.pp)
        self.sdb, self.gdb = oracle_mod.SparseDb(self.o), sp.Database.sparse(self.p)
        self.num_per, self.dim0, self.size = 1 << cfg["nu_2"], 1 << cfg["nu_1"], cfg["db_item_size"]
        self.items = {}

    def put(self, idx, data):
        self.gdb.update_item(idx, data)
        self.sdb.update_item_raw(idx, data)
        self.items[idx] = bytes(data)

    def query(self, idx, seed, shortcut=None, decodes=None):
        """the GPU response == the oracle's, and the first `decodes` bytes (default: all) of a present item decode (t_gsw = 8).
        shortcut=True: the response differs from spiral-rs's dense process_query over the zero-filled bucket, i.e. a fold
        shortcut fired; False: it equals it."""
        sp = self.sp
        q = self.cl.generate_query(idx, seed)
        sp.paths_taken()
        resp = sp.process_query(self.p, self.gpp, q, self.gdb)
        taken = sp.paths_taken()
        assert {"sweep_sparse", "fold_fused"} <= taken and not ({"sweep_packed_persist", "sweep_narrow", "sweep_wide"} & taken), taken
        assert resp == self.sdb.process_query(self.pp, q), idx
        if idx in self.items and self.cfg.get("t_gsw", 8) == 8:
            n = self.size if decodes is None else decodes
            assert self.cl.decode_response(resp)[:n] == self.items[idx].ljust(self.size, b"\0")[:n], idx
        if shortcut is not None:
            assert (resp != self.o.process_query(self.pp, q, self.sdb.to_dense())) == shortcut, idx
        return q, resp


def _random_item(rng, size):
    return rng.integers(0, 256, size, dtype=np.uint8).tobytes()


# k_sweep_sparse reduces its u64 sums every 255 items: columns of 255, 256, 511 and 512 items reduce 0, 1, 2 and 3 times
# (a full column of 512); 1024 items in one column is where the reference's wrapping u64 sums would be wrong
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,lens", [(dict(FAST, nu_1=9, nu_2=2, db_item_size=256), [255, 256, 511, 512]),
                                      (dict(FAST, nu_1=10, nu_2=1, db_item_size=256), [1024, 0]),
                                      (dict(FAST, nu_1=8, nu_2=1, db_item_size=256), [256, 17])],
                         ids=["nu1_9-255-256-511-512", "nu1_10-1024-0", "nu1_8-256-17"])
def test_sparse_deep_columns(oracle_mod, cfg, lens):
    b = _Bucket(oracle_mod, cfg)
    assert len(lens) == b.num_per
    rng = np.random.default_rng(sum(lens))
    col_rows = []
    for ii, n in enumerate(lens):
        rows = np.sort(rng.choice(b.dim0, n, replace=False))
        col_rows.append([int(j) for j in rows])
        for j in col_rows[-1]:
            b.put(j * b.num_per + ii, _random_item(rng, b.size))
    assert b.gdb.sparse_items() == sum(lens)
    seed = 200
    for ii, rows in enumerate(col_rows):
        for j in sorted({rows[0], rows[len(rows) // 2], rows[-1]} if rows else ()):   # top, middle and last present row
            b.query(j * b.num_per + ii, seed, shortcut=0 in lens)                    # (an empty column: a shortcut fires)
            seed += 1
    if 0 in lens:
        b.query(lens.index(0), seed)                                                  # an absent item


@pytest.mark.gpu
def test_sparse_full_bucket_equals_dense(oracle_mod):
    """every item present, so no shortcut fires: GPU sparse == oracle sparse (u128 sums) == oracle dense (spiral-rs's
    process_query) == GPU dense over the same items (Database.load_items); columns of 512 reduce three times"""
    cfg = dict(FAST, nu_1=9, nu_2=2, db_item_size=256)
    b = _Bucket(oracle_mod, cfg)
    num_items = b.dim0 * b.num_per
    blob = np.random.default_rng(7).integers(0, 256, (num_items, b.size), dtype=np.uint8)
    for i in range(num_items):
        b.put(i, blob[i].tobytes())
    assert b.gdb.sparse_items() == num_items
    dense = b.sp.Database(b.p).load_items(blob.tobytes())
    for k, idx in enumerate((0, 1234, num_items - 1)):
        q, resp = b.query(idx, 230 + k, shortcut=False)
        assert b.sp.process_query(b.p, b.gpp, q, dense) == resp, idx


_PATTERNS = {"col0_only": lambda ii, n: ii == 0, "last_col_only": lambda ii, n: ii == n - 1, "even_cols": lambda ii, n: ii % 2 == 0,
             "odd_cols": lambda ii, n: ii % 2 == 1, "left_half_empty": lambda ii, n: ii >= n // 2,
             "right_half_empty": lambda ii, n: ii < n // 2, "one_empty_col": lambda ii, n: ii != 5, "single_item": None}
_SMALL_SPARSE = [dict(FAST, nu_1=3, nu_2=4, db_item_size=256), dict(FAST, nu_1=3, nu_2=4, db_item_size=512, instances=2)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _SMALL_SPARSE, ids=["inst1", "inst2"])
@pytest.mark.parametrize("pattern", list(_PATTERNS))
def test_sparse_empty_column_patterns(oracle_mod, cfg, pattern):
    """whole columns empty in patterns that shortcut the fold at every level (16 columns: four levels), against lib/server's
    fold with its all-zero shortcuts (fold.rs:38-44); every case must have fired one"""
    b = _Bucket(oracle_mod, cfg)
    rng = np.random.default_rng(len(pattern))
    if _PATTERNS[pattern] is None:
        cols = {6: [3]}
    else:
        cols = {ii: sorted(int(j) for j in rng.choice(b.dim0, 2, replace=False)) for ii in range(b.num_per) if _PATTERNS[pattern](ii, b.num_per)}
    for ii, rows in cols.items():
        for j in rows:
            b.put(j * b.num_per + ii, _random_item(rng, b.size))
    first, last = min(cols), max(cols)
    b.query(cols[first][0] * b.num_per + first, 40, shortcut=True)
    b.query(cols[last][-1] * b.num_per + last, 41, shortcut=True)
    empty = next(ii for ii in range(b.num_per) if ii not in cols)
    b.query(b.num_per + empty, 42, shortcut=True)                                     # an absent item


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _SMALL_SPARSE, ids=["inst1", "inst2"])
def test_sparse_zero_and_short_items(oracle_mod, cfg):
    """present items whose bytes are zero make all-zero columns as absent ones do (the shortcuts key on values, as fold.rs
    does); items of 1-3 bytes leave every plane but the first zero, so a plane can be shortcut while the item's others are not.
    (Under those shortcuts a plane that is zero in the selected column comes back as its sibling column's, as in lib/server:
    zero items are compared byte for byte with the oracle only, short items decode in their first chunk.)"""
    b = _Bucket(oracle_mod, cfg)
    rng = np.random.default_rng(17)
    zero = b"\0" * b.size
    for ii in range(6, b.num_per):                     # columns 6.. hold ordinary items
        for j in rng.choice(b.dim0, 3, replace=False):
            b.put(int(j) * b.num_per + ii, _random_item(rng, b.size))
    b.put(2 * b.num_per + 0, b"")                      # column 0: an empty record
    b.put(5 * b.num_per + 1, zero)                     # column 1: an explicit zero record
    b.put(1 * b.num_per + 2, _random_item(rng, b.size))
    b.query(1 * b.num_per + 2, 50, shortcut=True)
    b.put(1 * b.num_per + 2, zero)                     # column 2: its only item overwritten with zeros
    for ii, n in ((3, 1), (4, 2), (5, 3)):            # columns 3-5: one short item each
        b.put(7 * b.num_per + ii, bytes(rng.integers(1, 256, n, dtype=np.uint8)))
    chunk = b.size // (cfg.get("instances", 1) * 4)
    for k, (idx, decodes) in enumerate(((2 * b.num_per, 0), (5 * b.num_per + 1, 0), (1 * b.num_per + 2, 0), (7 * b.num_per + 3, chunk),
                                        (7 * b.num_per + 4, chunk), (7 * b.num_per + 5, chunk),
                                        (next(i for i in b.items if i % b.num_per == 9), None))):
        b.query(idx, 51 + k, shortcut=True, decodes=decodes)


_ROW_CFGS = [dict(FAST, t_exp_right=56, nu_2=3, db_item_size=256), dict(FAST, nu_2=1, db_item_size=256)]
_ROW_SETS = {"row0": lambda d: [0], "last_row": lambda d: [d - 1], "all_rows": lambda d: list(range(d)), "rows_0_1": lambda d: [0, 1],
             "rows_0_8": lambda d: [0, 8], "rows_0_half": lambda d: [0, d // 2], "even_rows": lambda d: list(range(0, d, 2)),
             "odd_rows": lambda d: list(range(1, d, 2))}


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _ROW_CFGS, ids=["fast56", "nu2_1"])
@pytest.mark.parametrize("row_set", list(_ROW_SETS))
def test_sparse_pruned_expansion_row_sets(oracle_mod, cfg, row_set):
    """the pruned expansion's plan (build_pruned_plan_rows) on the edge sets of occupied rows; t_exp_right = 56 prunes beside
    stop_round, nu_2 = 1 has a single fold level"""
    b = _Bucket(oracle_mod, cfg)
    rng = np.random.default_rng(len(row_set))
    rows = _ROW_SETS[row_set](b.dim0)
    for j in rows:
        b.put(j * b.num_per + (j * 3) % b.num_per, _random_item(rng, b.size))
    for k, j in enumerate(sorted({rows[0], rows[len(rows) // 2], rows[-1]})):
        b.query(j * b.num_per + (j * 3) % b.num_per, 60 + k)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _ROW_CFGS, ids=["fast56", "nu2_1"])
def test_sparse_index_rebuilds_and_snapshots(oracle_mod, cfg):
    """ensure_sparse_index after each kind of upsert: a new key in a new row (index and expansion plan rebuilt), a new key in
    an occupied row (index rebuilt, plan shared), an overwrite (snapshot kept); a query begun before an upsert of a new key
    answers from the bucket as it was when it began"""
    b = _Bucket(oracle_mod, cfg)
    rng = np.random.default_rng(23)
    last = b.dim0 - 1
    at = lambda j, ii: j * b.num_per + ii                                          # noqa: E731
    b.put(at(0, 0), _random_item(rng, b.size))
    b.query(at(0, 0), 70)
    b.put(at(last, b.num_per - 1), _random_item(rng, b.size))                     # new row
    b.query(at(last, b.num_per - 1), 71)
    b.query(at(0, 0), 72)
    b.put(at(last, 0), _random_item(rng, b.size))                                 # occupied row
    b.query(at(last, 0), 73)
    b.put(at(0, 0), _random_item(rng, b.size))                                    # overwrite
    b.query(at(0, 0), 74)
    b.query(at(last, 0), 75)
    q = b.cl.generate_query(at(last, 0), 76)
    want = b.sdb.process_query(b.pp, q)
    run = b.sp.QueryRun(b.p, b.gpp, q, db=b.gdb)
    b.put(at(3, 0), _random_item(rng, b.size))                                    # new key, new row, after the query began
    assert b.sdb.process_query(b.pp, q) != want
    resp = run.sweep(b.gdb).finish()
    run.free()
    assert resp == want
    b.query(at(3, 0), 77)
    b.query(at(last, 0), 78)


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_sparse_bucket_query_lists(oracle_mod, in_flight):
    """sp_process_query_batch on a sparse bucket: the per-query path with `in_flight` queries in flight (db->packed == 0), eleven
    distinct queries under two clients' keys; no batched sweep and no digit-planar copy"""
    import ctypes as C
    import os
    b = _Bucket(oracle_mod, dict(FAST, nu_1=6, nu_2=3, db_item_size=256))
    cl2 = type(b.cl)(b.o)
    pp2 = cl2.generate_keys(12)
    gpp2 = b.sp.PublicParameters.deserialize(b.p, pp2)
    rng = np.random.default_rng(31)
    for idx in rng.choice(b.dim0 * b.num_per, 150, replace=False):
        b.put(int(idx), _random_item(rng, b.size))
    present = list(b.items)
    clients = [(b.cl, b.pp, b.gpp), (cl2, pp2, gpp2)]
    qs, gpps, want = [], [], []
    for k in range(11):
        cl, pp, gpp = clients[k % 2]
        qs.append(cl.generate_query(present[k], 300 + k))
        gpps.append(gpp)
        want.append(b.sdb.process_query(pp, qs[-1]))
    assert len(set(qs)) == 11
    b.sp.lib().sp_debug_set(b"batch_in_flight", C.c_long(in_flight))
    try:
        b.sp.paths_taken()
        got = b.sp.process_query_batch(b.p, gpps, qs, b.gdb)
        taken = b.sp.paths_taken()
    finally:
        b.sp.lib().sp_debug_set(b"batch_in_flight", C.c_long(int(os.environ.get("SPIRAL_BATCH_IN_FLIGHT", 3))))
    assert got == want
    for k, resp in enumerate(got):
        assert clients[k % 2][0].decode_response(resp)[:b.size] == b.items[present[k]], k
    assert "sweep_sparse" in taken and not any(t.startswith("sweep_batch") for t in taken), taken
    assert b.gdb.prepare_batch() is False and b.gdb.batch_copy_bytes() == 0
