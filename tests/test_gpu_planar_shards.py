"""Planar ROW SHARDS (sp_db_create_planar_shard): row shard s of G whose only resident form is the digit-planar layout, columns in the
order of the exchange (sdk_amd/csrc/planar_resident.hpp), read by k_sweep_planar's scatter form with one query tile (1 .. 8 queries) or
two (9 .. 16).  Every comparison is byte equality: with the oracle's words (read_ref), with the partial buffers the per-plane scatter
sweep leaves on a PACKED shard of the same content, with the oracle's process_query over the unsharded words.

Shapes, the smallest that reach each branch (nj = dim0 / G local rows, num_per / G columns per rank class):
  A (7, 7) G 2   nj 64: one block, ring of 2; a 128-column chunk spans both classes (64 columns each)
  B (8, 7) G 4   nj 64; a wave's 32 columns are exactly one class
  C (8, 7) G 2   nj 128: two blocks, ring of 4
  D (7, 8) G 2   two chunks: the eight-wave split; a chunk is one class
  E (9, 7) G 8   nj 64; a wave's columns span two classes (16 each); synthetic fill, no oracle words
  F = A with instances = 2: 8 planes
Path bits of the pass: scatter_out | sweep_batch | sweep_batch_mfma | sweep_batch_planar (| sweep_batch_mfma_two_tiles for 9 .. 16), and
sweep_batch_scatter (k_sweep_mfma_scatter's name) stays clear."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_gpu_planar_resident import _body, _corners, _edits
from test_gpu_sharded_batch import _partial

pytestmark = pytest.mark.gpu

Q0, Q1 = 268369921, 249561089
SHAPES = {"A": (7, 7, 2, 1), "B": (8, 7, 4, 1), "C": (8, 7, 2, 1), "D": (7, 8, 2, 1), "E": (9, 7, 8, 1), "F": (7, 7, 2, 2)}
ONE_TILE = {"scatter_out", "sweep_batch", "sweep_batch_mfma", "sweep_batch_planar"}
TWO_TILES = ONE_TILE | {"sweep_batch_mfma_two_tiles"}
NOT_THE_PASS = {"sweep_batch_scatter", "sweep_ring", "sweep_packed_persist", "sweep_packed", "sweep_wide", "sweep_narrow", "sweep_narrow_group"}
POOL = 19          # queries per shape under two clients' keys (query i: client i % 2); a group of B is the pool's first B
SEED = 0x5EED


def _cfg(nu_1, nu_2, instances=1, t_gsw=4):
    return {"n": 2, "nu_1": nu_1, "nu_2": nu_2, "p": 256, "q2_bits": 20, "t_gsw": t_gsw, "t_conv": 4, "t_exp_left": 8,
            "t_exp_right": 56, "instances": instances, "db_item_size": 256}


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _assert_pass(taken, B):
    assert (TWO_TILES if B > 8 else ONE_TILE) <= taken and not (NOT_THE_PASS & taken), (B, taken)
    if B <= 8:
        assert "sweep_batch_mfma_two_tiles" not in taken, taken


class _Ctx:
    """one shape: params, two clients, a random item file and its oracle words (E: the synthetic fill instead), the query pool, and
    -- lazily, once -- PACKED and planar shards of that content, the PACKED shards' per-plane scatter partials and the oracle's
    responses; nothing in here is changed by a test"""

    def __init__(self, sp, oracle_mod, name):
        nu_1, nu_2, self.G, inst = SHAPES[name]
        self.sp, self.name, self.cfg = sp, name, _cfg(nu_1, nu_2, inst)
        self.o = oracle_mod.Params(self.cfg)
        self.p = sp.Params(self.cfg)
        self.cls = [oracle_mod.Client(self.o), oracle_mod.Client(self.o)]
        self.pps = [self.cls[0].generate_keys(61), self.cls[1].generate_keys(62)]
        self.gpps = [sp.PublicParameters.deserialize(self.p, pp) for pp in self.pps]
        self.isz, self.npr, self.d0 = self.o.db_item_size, self.o.num_per, self.o.dim0
        self.nj, self.planes = self.d0 // self.G, inst * 4
        self.synthetic = name == "E"
        if not self.synthetic:
            self.blob = np.random.default_rng(nu_1 * 16 + nu_2 + inst).integers(0, 256, self.o.num_items * self.isz, dtype=np.uint8)
            self.blob.setflags(write=False)
        self._words = None
        self.idxs = [(977 * i + 3) % self.o.num_items for i in range(POOL)]
        self.qs = [self.cls[i % 2].generate_query(self.idxs[i], 900 + i) for i in range(POOL)]
        self._want, self._packed, self._planar, self._partials = {}, {}, {}, {}

    @property
    def words(self):
        if self._words is None:
            self._words = self.o.load_db_from_bytes(self.blob.tobytes())
            self._words.setflags(write=False)
        return self._words

    def want(self, i):
        if i not in self._want:
            self._want[i] = (self.o.process_query_synth(self.pps[i % 2], self.qs[i], SEED) if self.synthetic else
                             self.o.process_query(self.pps[i % 2], self.qs[i], self.words))
        return self._want[i]

    def _fill(self, db):
        return db.fill_synthetic(SEED) if self.synthetic else db.load(self.words)

    def packed(self, s):
        if s not in self._packed:
            self._packed[s] = self._fill(self.sp.Database(self.p, s, self.G))
            assert self._packed[s].format() == "packed"
        return self._packed[s]

    def planar(self, s):
        if s not in self._planar:
            self._planar[s] = self._fill(self.sp.Database.planar_shard(self.p, s, self.G))
        return self._planar[s]

    def run(self, i, db):
        return self.sp.QueryRun(self.p, self.gpps[i % 2], self.qs[i], db=db)

    def partials(self, s, n=16):
        """what sweep_scatter_plane leaves for the pool's first n queries on PACKED shard s"""
        have = self._partials.setdefault(s, [])
        while len(have) < n:
            run = self.run(len(have), self.packed(s))
            for pl in range(self.planes):
                run.sweep_scatter_plane(self.packed(s), self.G, pl)
            have.append(_partial(self.sp, run))
            run.free()
        return have

    def lists(self):
        return [self.gpps[i % 2] for i in range(POOL)], list(self.qs)


_ctxs = {}


def _ctx(sp, oracle_mod, name):
    for other_name, other in _ctxs.items():      # one shape's shards, words and reference buffers at a time (the responses stay)
        if other_name != name:
            other._packed.clear(), other._planar.clear(), other._partials.clear()
            other._words = None
    if name not in _ctxs:
        _ctxs[name] = _Ctx(sp, oracle_mod, name)
    return _ctxs[name]


def _shard_bytes(c):
    return c.planes * 2048 * c.npr * c.nj * 8


def _assert_shard_words(db, c, s, want4):
    """want4: [plane][z][ii][j] over the full dim0; the shard answers in reference columns and LOCAL rows"""
    j0 = s * c.nj
    for pl, z, ii in _corners(c):
        assert (db.read_ref(pl, z, ii, 0, c.nj) == want4[pl, z, ii, j0:j0 + c.nj]).all(), (s, pl, z, ii)
    assert db.read_ref(3, 2047, c.npr - 1, c.nj - 1, 1)[0] == want4[3, 2047, c.npr - 1, j0 + c.nj - 1]
    assert db.read_ref(0, 0, 0, 17, 3).tolist() == want4[0, 0, 0, j0 + 17:j0 + 20].tolist()


# ------------------------------------------------------------------------------------------------ 1. loaders and read-back
@pytest.mark.parametrize("name", ["A", "C"], ids=lambda n: "shape" + n)
def test_loaders_read_back_on_every_shard(sp, oracle_mod, name):
    c = _ctx(sp, oracle_mod, name)
    want4 = c.words.reshape(c.planes, 2048, c.npr, c.d0)
    cut = 700
    for s in range(c.G):
        fresh = sp.Database.planar_shard(c.p, s, c.G)
        assert fresh.format() == "planar" and fresh.device_bytes() == _shard_bytes(c) and fresh.batch_copy_bytes() == 0
        for pl, z, ii in _corners(c):
            assert not fresh.read_ref(pl, z, ii, 0, c.nj).any(), (s, pl, z, ii)
        _assert_shard_words(fresh.load_items(c.blob), c, s, want4)
        assert fresh.device_bytes() == _shard_bytes(c) and fresh.prepare_batch() is True and fresh.batch_copy_bytes() == 0
        _assert_shard_words(c.planar(s), c, s, want4)                       # sp_db_load
        db = sp.Database.planar_shard(c.p, s, c.G)
        for pl in range(c.planes):                                          # two z-ranges per plane, the second first
            db.load_plane(pl, cut, 2048 - cut, want4[pl, cut:])
            db.load_plane(pl, 0, cut, want4[pl, :cut])
        _assert_shard_words(db, c, s, want4)
        for pl, z, ii in ((1, cut - 1, 5), (1, cut, 5), (2, cut, c.npr - 1)):
            assert (db.read_ref(pl, z, ii, 0, c.nj) == want4[pl, z, ii, s * c.nj:(s + 1) * c.nj]).all(), (s, pl, z, ii)
        with pytest.raises(sp.SpiralError):
            db.read_ref(0, 0, 0, c.nj - 1, 2)                               # past the shard's rows


def test_fill_synthetic_is_the_reference_index(sp, oracle_mod):
    from sdk_amd.spiral import synth_words
    c = _ctx(sp, oracle_mod, "E")
    for s in (0, 7):
        db = c.planar(s)
        assert db.device_bytes() == _shard_bytes(c)
        for pl, z, ii in _corners(c):
            ref = ((pl * 2048 + z) * c.npr + ii) * c.d0 + s * c.nj + np.arange(c.nj, dtype=np.uint64)
            assert (db.read_ref(pl, z, ii, 0, c.nj) == synth_words(SEED, ref)).all(), (s, pl, z, ii)


def test_limbs_above_q_are_reduced_as_on_packed(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "A")
    rng = np.random.default_rng(7)
    lo = np.array([Q0, Q0 + 1, 2**32 - 1, 2**28, 0, Q0 - 1, 0x80808080, 0x7F7F7F7F], dtype=np.uint64)
    hi = np.array([Q1, Q1 + 1, 2**32 - 1, 2**28, 0, Q1 - 1, 0x80808080, 0x7F7F7F7F], dtype=np.uint64)
    pick = rng.integers(0, 8, c.planes * 2048 * c.npr * c.d0)
    words = (lo[pick] | (hi[(pick + 3) % 8] << np.uint64(32))).astype(np.uint64)
    a, b = sp.Database.planar_shard(c.p, 1, 2).load(words), sp.Database(c.p, 1, 2).load(words)
    w4 = words.reshape(c.planes, 2048, c.npr, c.d0)[..., c.nj:]
    for pl, z, ii in _corners(c):
        got = a.read_ref(pl, z, ii, 0, c.nj)
        assert (got == b.read_ref(pl, z, ii, 0, c.nj)).all(), (pl, z, ii)
        assert ((got & np.uint64(0xFFFFFFFF)) == (w4[pl, z, ii] & np.uint64(0xFFFFFFFF)) % np.uint64(Q0)).all()
        assert ((got >> np.uint64(32)) == (w4[pl, z, ii] >> np.uint64(32)) % np.uint64(Q1)).all()


# ------------------------------------------------------------------------------------------------ 2. the group pass
def _group_pass_equals_packed(sp, c, s, B):
    want = c.partials(s, B)
    shard = c.planar(s)
    runs = [c.run(i, shard) for i in range(B)]
    sp.paths_taken()
    sp.QueryRun.sweep_scatter_group(runs, shard, c.G)
    got = [_partial(sp, r) for r in runs]
    _assert_pass(sp.paths_taken(), B)
    for k in range(B):
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (c.name, s, B, k, int((got[k] != want[k]).sum()))
    with pytest.raises(sp.SpiralError):
        sp.QueryRun.sweep_scatter_group(runs, shard, c.G)      # already swept
    for r in runs:
        r.free()


@pytest.mark.parametrize("B", [1, 3, 8, 9, 11, 16], ids=lambda b: "B%02d" % b)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "F"], ids=lambda n: "shape" + n)      # (the shape varies slowest: one context at a time)
def test_group_pass_leaves_the_packed_shards_partials(sp, oracle_mod, name, B):
    """after sweep_scatter_group on a planar shard every query's partial buffer equals, word for word, what sweep_scatter_plane leaves
    for that query on a PACKED shard of the same content -- every shard, one query tile and two"""
    c = _ctx(sp, oracle_mod, name)
    for s in range(c.G):
        _group_pass_equals_packed(sp, c, s, B)


@pytest.mark.parametrize("B", [8, 16], ids=lambda b: "B%02d" % b)
def test_group_pass_where_a_waves_columns_span_two_classes(sp, oracle_mod, B):
    c = _ctx(sp, oracle_mod, "E")
    for s in (0, 7):
        _group_pass_equals_packed(sp, c, s, B)


@pytest.mark.parametrize("name", ["A", "B"], ids=lambda n: "shape" + n)
def test_single_query_scatter_sweeps_equal_packed(sp, oracle_mod, name):
    """sweep_scatter (the all-planes layout) and sweep_scatter_plane run as a group of one on a planar shard"""
    c = _ctx(sp, oracle_mod, name)
    for s in (0, c.G - 1):
        bufs = []
        for shard in (c.packed(s), c.planar(s)):
            sp.paths_taken()
            whole = c.run(1, shard).sweep_scatter(shard, c.G)
            per_plane = c.run(2, shard)
            for pl in range(c.planes):
                per_plane.sweep_scatter_plane(shard, c.G, pl)
            bufs.append((_partial(sp, whole), _partial(sp, per_plane)))
            taken = sp.paths_taken()
            if shard.format() == "planar":
                _assert_pass(taken, 1)
                with pytest.raises(sp.SpiralError):
                    c.run(0, shard).sweep(shard)                           # the plain partial stays refused on a planar shard
            whole.free(), per_plane.free()
        assert (bufs[0][0] == bufs[1][0]).all() and (bufs[0][1] == bufs[1][1]).all(), (name, s)
        assert (bufs[1][1] == c.partials(s, 3)[2]).all()


# ------------------------------------------------------------------------------------------------ 3. lists over the loopback world
def _world_run(sp, G, fn):
    from sdk_amd.sharding import LoopbackWorld
    world = LoopbackWorld(G)

    def rank_main(r):
        sp.lib().sp_set_device(0)
        return fn(r, world.comm(r))
    return world, world.run(rank_main)


@pytest.mark.parametrize("name", ["A", "B", "D"], ids=lambda n: "shape" + n)
def test_lists_of_19_in_every_group_size(sp, oracle_mod, name):
    """19 queries of two clients with group = 0 (16 here), 16, 11, 8 and 1, twice each: rank 0's responses equal the oracle's over the
    unsharded words and the per-query list on PACKED shards; the other ranks return []"""
    c = _ctx(sp, oracle_mod, name)
    pp_list, q_list = c.lists()
    expect = [c.want(i) for i in range(POOL)]
    planar, packed = [c.planar(s) for s in range(c.G)], [c.packed(s) for s in range(c.G)]

    def rank_main(r, comm):
        res = {}
        comm.reserve_batch_for(c.p, planar[r], 0)
        for group in (0, 16, 11, 8, 1):
            sp.paths_taken()
            a = comm.process_queries_batched(c.p, pp_list, q_list, planar[r], group=group)
            b = comm.process_queries_batched(c.p, pp_list, q_list, planar[r], group=group)      # buffer reuse
            res[group] = (a, b, sp.paths_taken(), comm.describe())
        res["packed"] = comm.process_queries(c.p, pp_list, q_list, packed[r])
        return res
    _, res = _world_run(sp, c.G, rank_main)
    assert res[0]["packed"] == expect
    for group, size in ((0, 16), (16, 16), (11, 11), (8, 8), (1, 1)):
        assert res[0][group][0] == expect and res[0][group][1] == expect, group
        for r in range(c.G):
            if r:
                assert res[r][group][0] == [] and res[r][group][1] == [], (group, r)
            taken, info = res[r][group][2], res[r][group][3]
            # 19 = 16 + 3, 11 + 8, 8 + 8 + 3: groups of more than 8 take two tiles, every list here has a group of at most 8 too
            _assert_pass(taken, 16 if size > 8 else 1)
            assert {"custom_transport", "expand_pruned"} <= taken, taken
            assert info["last_list"] == {"group": size, "reduce_scatters": POOL * c.planes, "all_gathers": POOL}, info


def test_list_of_16_where_a_waves_columns_span_two_classes(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "E")
    pp_list, q_list = [l[:16] for l in c.lists()]
    planar, packed = [c.planar(s) for s in range(c.G)], [c.packed(s) for s in range(c.G)]

    def rank_main(r, comm):
        sp.paths_taken()
        got = comm.process_queries_batched(c.p, pp_list, q_list, planar[r])
        return got, sp.paths_taken(), comm.process_queries(c.p, pp_list, q_list, packed[r])
    _, res = _world_run(sp, c.G, rank_main)
    assert res[0][0] == res[0][2] and len(res[0][0]) == 16
    assert res[0][0][0] == c.want(0)
    for r in range(c.G):
        _assert_pass(res[r][1], 16)
        assert r == 0 or (res[r][0] == [] and res[r][2] == [])


def test_per_query_flows_on_planar_shards(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "A")
    pp_list, q_list = [l[:3] for l in c.lists()]
    planar = [c.planar(s) for s in range(c.G)]

    def rank_main(r, comm):
        sp.paths_taken()
        one = comm.process_query(c.p, c.gpps[1], c.qs[1], planar[r])
        return one, comm.process_queries(c.p, pp_list, q_list, planar[r]), sp.paths_taken()
    _, res = _world_run(sp, c.G, rank_main)
    assert res[0][0] == c.want(1) and res[0][1] == [c.want(i) for i in range(3)]
    assert res[1][0] == b"" and res[1][1] == []
    for r in range(c.G):
        _assert_pass(res[r][2], 1)


def test_list_decodes_the_planted_item(sp, oracle_mod):
    """t_gsw = 8 leaves room to decode: the response to a query for the planted item, through a list of 9 on planar shards"""
    cfg, G, idx = _cfg(7, 7, t_gsw=8), 2, 77
    o = oracle_mod.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(91)
    item, db = o.generate_random_db_and_get_item(idx)
    q_list = [cl.generate_query((idx + 13 * k) % o.num_items, 40 + k) for k in range(9)]
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    shards = [sp.Database.planar_shard(p, s, G).load(db) for s in range(G)]

    def rank_main(r, comm):
        sp.paths_taken()
        return comm.process_queries_batched(p, gpp, q_list, shards[r]), sp.paths_taken()
    _, res = _world_run(sp, G, rank_main)
    _assert_pass(res[0][1], 9)
    assert cl.decode_response(res[0][0][0]) == o.item_to_vec(item)
    assert res[0][0][0] == o.process_query(pp, q_list[0], db) and res[0][0][8] == o.process_query(pp, q_list[8], db)


# ------------------------------------------------------------------------------------------------ 4. upserts
def _edited_shards(sp, c):
    """every rank of A takes the same body: records for both shards and a duplicate index (the later record wins)"""
    edits, recs, after = _edits(c)
    assert {it // c.npr // c.nj for it in edits} == {0, 1}                  # both shards hold edited rows
    body = _body([(edits[3], b"\x55" * c.isz)] + recs)                      # edits[3] again later, and item 1 twice inside recs
    shards = [sp.Database.planar_shard(c.p, s, c.G).load_items(c.blob) for s in range(c.G)]
    for db in shards:
        assert db.update_rows(body) == (len(recs) + 1, 4 + c.isz)           # the other shard's records are counted as applied
        assert db.device_bytes() == _shard_bytes(c)
    return edits, after, shards


def test_the_same_update_row_body_on_every_rank(sp, oracle_mod):
    """read_ref after the body equals the oracle's words of the edited file; then the faulty third record with its applied prefix"""
    c = _ctx(sp, oracle_mod, "A")
    edits, after, shards = _edited_shards(sp, c)
    exp4 = c.o.load_db_from_bytes(after.tobytes()).reshape(c.planes, 2048, c.npr, c.d0)
    for s, db in enumerate(shards):
        for pl, z in ((0, 0), (3, 2047)):
            for it in edits + [2, c.npr + 2]:                               # the edited items and neighbours that share their entries
                j, ii = divmod(it, c.npr)
                if j // c.nj == s:
                    assert db.read_ref(pl, z, ii, j - s * c.nj, 1)[0] == exp4[pl, z, ii, j], (s, pl, z, it)
    # the faulty third record: both ranks apply the same prefix (each keeps its own rows of it) and report it
    good = [(5, b"\x11" * c.isz), (c.nj * c.npr + 6, b"\x22" * 7)]
    after2 = after.copy()
    for i, d in good:
        after2[i * c.isz:(i + 1) * c.isz] = 0
        after2[i * c.isz:i * c.isz + len(d)] = np.frombuffer(d, dtype=np.uint8)
    exp2 = c.o.load_db_from_bytes(after2.tobytes()).reshape(c.planes, 2048, c.npr, c.d0)
    for s, db in enumerate(shards):
        with pytest.raises(sp.SpiralError) as e:
            db.update_rows(_body(good) + struct.pack(">II", 4 + 3, c.o.num_items) + b"abc")
        assert e.value.rc == -1 and e.value.applied == 2 and "record 2" in str(e.value), str(e.value)
        for pl, z in ((0, 0), (2, 1000), (3, 2047)):
            for ii in (5, 6):
                assert (db.read_ref(pl, z, ii, 0, c.nj) == exp2[pl, z, ii, s * c.nj:(s + 1) * c.nj]).all(), (s, pl, z, ii)
        with pytest.raises(sp.SpiralError):                                 # SP_E_ARG on the array form leaves the handle untouched
            db.update_items([(7, b"\x33" * c.isz), (c.o.num_items, b"x")])
        assert (db.read_ref(1, 9, 7, 0, c.nj) == exp2[1, 9, 7, s * c.nj:(s + 1) * c.nj]).all()


def test_list_of_9_after_the_update_row_body(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "A")
    edits, after, shards = _edited_shards(sp, c)
    exp = c.o.load_db_from_bytes(after.tobytes())
    B = 9
    idxs = [edits[i] if i < 7 else c.idxs[i] for i in range(B)]
    qs = [c.cls[i % 2].generate_query(idxs[i], 700 + i) for i in range(B)]

    def rank_main(r, comm):
        sp.paths_taken()
        return comm.process_queries_batched(c.p, [c.gpps[i % 2] for i in range(B)], qs, shards[r]), sp.paths_taken()
    _, res = _world_run(sp, c.G, rank_main)
    assert res[0][0] == [c.o.process_query(c.pps[i % 2], qs[i], exp) for i in range(B)] and res[1][0] == []
    _assert_pass(res[0][1], B)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_creation_is_refused_where_the_format_does_not_exist(sp, oracle_mod):
    c = _ctx(sp, oracle_mod, "A")
    with pytest.raises(sp.SpiralError, match="sp_db_create_planar"):
        sp.Database.planar_shard(c.p, 0, 1)
    with pytest.raises(sp.SpiralError, match="unsharded"):
        sp.Database.planar(c.p, 0, 2)
    for nu, G in (((6, 7), 2), ((7, 6), 2)):                                # nj = 32; num_per = 64
        with pytest.raises(sp.SpiralError, match="% 64 == 0"):
            sp.Database.planar_shard(sp.Params(_cfg(*nu)), 0, G)
    for bad in ((2, 2), (-1, 2), (0, 3), (0, 16)):
        with pytest.raises(sp.SpiralError):
            sp.Database.planar_shard(c.p, *bad)
    for switch in (b"batch_planar", b"batch_mfma"):
        sp.lib().sp_debug_set(switch, C.c_long(0))
        try:
            with pytest.raises(sp.SpiralError, match="batch_planar and batch_mfma"):
                sp.Database.planar_shard(c.p, 0, 2)
        finally:
            sp.lib().sp_debug_set(switch, C.c_long(1))
    assert sp.Database.planar_shard(c.p, 1, 2).format() == "planar"


def test_errors_enqueue_nothing_and_enter_no_collective(sp, oracle_mod):
    from sdk_amd.sharding import LoopbackWorld
    c = _ctx(sp, oracle_mod, "A")
    pp_list, q_list = c.lists()
    shard, other, packed = c.planar(0), c.planar(1), c.packed(0)
    four = sp.Database.planar_shard(sp.Params(_cfg(8, 7)), 0, 4)            # G different from the world's (and other params)
    world = LoopbackWorld(c.G)
    comm = world.comm(0)
    with pytest.raises(sp.SpiralError):
        comm.process_queries_batched(c.p, pp_list, q_list, shard, group=17)
    with pytest.raises(sp.SpiralError):
        comm.process_queries_batched(c.p, pp_list, q_list, packed, group=9)
    with pytest.raises(sp.SpiralError):
        comm.reserve_batch_for(c.p, shard, 17)
    with pytest.raises(sp.SpiralError):
        comm.reserve_batch_for(c.p, packed, 9)
    with pytest.raises(sp.SpiralError):
        comm.reserve_batch(c.p, 9)
    comm.reserve_batch_for(c.p, shard, 16)
    for group in (0, 16, 1):
        with pytest.raises(sp.SpiralError):
            comm.process_queries_batched(c.p, pp_list, q_list, four, group=group)
        for pos in (0, POOL - 1):
            bad = list(q_list)
            bad[pos] = bad[pos][:-8]
            with pytest.raises(sp.SpiralError):
                comm.process_queries_batched(c.p, pp_list, bad, shard, group=group)
    world4 = LoopbackWorld(4)
    for call in (lambda: world4.comm(0).process_queries_batched(c.p, pp_list, q_list, shard),        # a shard of 2 in a world of 4
                 lambda: world4.comm(0).process_queries(c.p, pp_list, q_list, shard),
                 lambda: world4.comm(0).process_query(c.p, pp_list[0], q_list[0], shard)):
        with pytest.raises(sp.SpiralError, match="planar row shard is one of 2"):
            call()
    assert world.calls == [0] * c.G and world4.calls == [0] * 4
    # stage calls: a group of 17, G different from the handle's, a query begun for another shard, a group of 9 on a PACKED shard
    runs = [c.run(i, shard) for i in range(16)]
    extra = c.run(16, shard)
    for handle, g, group in ((shard, c.G, runs + [extra]), (shard, 4, runs), (other, c.G, runs), (packed, c.G, runs[:9])):
        with pytest.raises(sp.SpiralError):
            sp.QueryRun.sweep_scatter_group(group, handle, g)
    with pytest.raises(sp.SpiralError):
        runs[0].sweep_scatter_plane(other, c.G, 0)
    with pytest.raises(sp.SpiralError):
        runs[0].sweep_scatter(shard, 4)
    # afterwards the handle still answers, and the refused calls changed no state
    sp.QueryRun.sweep_scatter_group(runs, shard, c.G)
    want = c.partials(0, 16)
    for k, r in enumerate(runs):
        assert (_partial(sp, r) == want[k]).all(), k
        r.free()
    extra.free()
