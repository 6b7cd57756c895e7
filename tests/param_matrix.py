"""The four parameter sets of tests/test_gpu_param_matrix.py, their query pools and the helpers that depend on the plane count
planes = instances * n * n.  Not a test file.

Every other test of the resident formats and list flows runs at n = 2, p = 256 with 4 or 8 planes; these sets are the ones the
reference ships, with only nu shrunk (S16: instances 11 -> 3 as well, to bound memory and the oracle's time):
  N3   9 planes: an odd count; pack with n = 3; an item fills its nine polynomials exactly
  V0  16 planes: e2e-tests/params/v0.json, n = 4
  V1  16 planes: v1.json -- packing version 1 once per instance, four instances, odd t_gsw, short expansion gadgets
  S16 12 planes: CFG_16_100000 -- p = 512 (9-bit plaintext words), a ragged item (27000 of 27648 bytes)
A pool (Dense) holds what costs oracle time -- words, responses, word and digest references -- computed once per module and never
changed by a test; a test's own handles live and die with the test."""
import struct

import numpy as np

from db_digest_reference import N, digest_plane

SETS = {
    "N3": {"n": 3, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56, "instances": 1,
           "db_item_size": 18432},
    "V0": {"n": 4, "p": 256, "q2_bits": 20, "t_gsw": 8, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56, "instances": 1,
           "db_item_size": 32768},
    "V1": {"n": 2, "p": 256, "q2_bits": 22, "t_gsw": 7, "t_conv": 3, "t_exp_left": 5, "t_exp_right": 5, "instances": 4,
           "db_item_size": 32768, "version": 1},
    "S16": {"n": 2, "p": 512, "q2_bits": 21, "t_gsw": 10, "t_conv": 4, "t_exp_left": 16, "t_exp_right": 56, "instances": 3,
            "db_item_size": 27000},
}
PLANES = {"N3": 9, "V0": 16, "V1": 16, "S16": 12}
POOL = {"N3": 9, "V0": 9, "V1": 3, "S16": 3}                        # distinct queries per (6, 7) pool, under two clients' keys
LISTS = {"N3": (1, 8, 9), "V0": (1, 8, 9), "V1": (1, 3), "S16": (1, 3)}
DIGEST_SEED = 0x5EED
HEAD = (0x00, 0x80, 0x81, 0xff, 0x7f)                                # the values 0, p / 2, p / 2 + 1 and p - 1 at p = 256

# path bits (sp.paths_taken()): what each kind of handle reports for a single query, and what it must not
PACKED_SINGLE = {"sweep_packed_persist", "sweep_packed", "sweep_ring"}
BATCH_BITS = {"sweep_batch", "sweep_batch_mfma", "sweep_batch_mfma_two_tiles", "sweep_batch_planar", "sweep_batch_scatter"}
PLANAR_ONE_TILE = {"sweep_batch", "sweep_batch_mfma", "sweep_batch_planar"}
NOT_PLANAR = {"sweep_ring", "sweep_packed_persist", "sweep_packed", "sweep_wide", "sweep_narrow", "sweep_narrow_group", "sweep_sparse"}


def cfg(name, nu_1, nu_2):
    return dict(SETS[name], nu_1=nu_1, nu_2=nu_2)


def planes_of(c):
    return c["instances"] * c["n"] ** 2


def body(records):
    """an /update-row body: be32 chunk_len | be32 item index | item bytes per record"""
    return b"".join(struct.pack(">II", 4 + len(d), i) + bytes(d) for i, d in records)


def corners(planes, npr):
    """every plane; first and last z, column (and one of each in between)"""
    return [(pl, z, ii) for pl in range(planes) for z in (0, 1029, N - 1) for ii in (0, 1, 77 % npr, npr - 2, npr - 1)]


def assert_packed_single(taken):
    assert PACKED_SINGLE & taken and not (BATCH_BITS | {"sweep_narrow", "sweep_wide", "sweep_sparse"}) & taken, taken


def assert_packed_list(taken, B):
    """a list on a PACKED handle with its digit-planar copy: 1 .. 3 the VALU group pass, 4 .. 8 the matrix-core pass over the PACKED
    words, 9 .. 16 two query tiles over the copy"""
    assert "sweep_batch" in taken and not {"sweep_wide", "sweep_narrow", "sweep_narrow_group", "sweep_sparse", "sweep_batch_scatter"} & taken, (B, taken)
    assert ("sweep_batch_mfma" in taken) == (B >= 4), (B, taken)
    assert ("sweep_batch_mfma_two_tiles" in taken) == (B > 8) and ("sweep_batch_planar" in taken) == (B > 8), (B, taken)


def assert_planar_list(taken, B):
    """a planar-resident handle reads every list size with k_sweep_planar: one query tile up to 8, two from 9"""
    assert PLANAR_ONE_TILE <= taken and not (NOT_PLANAR | {"sweep_batch_scatter"}) & taken, (B, taken)
    assert ("sweep_batch_mfma_two_tiles" in taken) == (B > 8), (B, taken)


def sparse_records(o, seed=11):
    """a scattered third of the items, one of them zero-length and one short -> ([(index, bytes)], the file [num_items][item size])"""
    rng = np.random.default_rng(seed)
    isz = o.db_item_size
    idx = sorted(int(i) for i in rng.choice(o.num_items, o.num_items // 3, replace=False))
    recs = [(i, rng.integers(0, 256, isz, dtype=np.uint8).tobytes()) for i in idx]
    recs[3] = (recs[3][0], b"")
    recs[5] = (recs[5][0], recs[5][1][:37])
    recs[0] = (recs[0][0], bytes(HEAD) + recs[0][1][len(HEAD):])
    file = np.zeros((o.num_items, isz), dtype=np.uint8)
    for i, d in recs:
        file[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return recs, file


def digest_reference(words, planes, npr, d0, seed=DIGEST_SEED):
    """tests/db_digest_reference.py over reference-layout words -> uint64 [planes][2]"""
    w4 = np.asarray(words).reshape(planes, N, npr, d0)
    return np.array([digest_plane(seed, pl, w4[pl], N, npr, d0) for pl in range(planes)], dtype=np.uint64)


class _State:
    """one content of a pool's database (the item file as loaded, or after the edit body): the queries asked of it and, from its
    oracle words, lazily and once: the responses, the words at corners(), the numpy digest"""

    def __init__(self, pool, file, idxs, seed0):
        self.pool, self.file, self.idxs = pool, file, idxs
        self.qs = [pool.cls[i % 2].generate_query(idxs[i], seed0 + i) for i in range(len(idxs))]
        self._words, self._want, self._corner, self._digest = None, {}, None, None

    @property
    def words(self):
        if self._words is None:
            self._words = self.pool.o.load_db_from_bytes(self.file.tobytes())
            self._words.setflags(write=False)
        return self._words

    def want(self, i):
        if i not in self._want:
            self._want[i] = self.pool.o.process_query(self.pool.pps[i % 2], self.qs[i], self.words)
        return self._want[i]

    def references(self):
        """(words [d0] at every corner, digest [planes][2]), both from the oracle's words in one visit"""
        if self._corner is None:
            c = self.pool
            w4 = self.words.reshape(c.planes, N, c.npr, c.d0)
            self._corner = {k: w4[k].copy() for k in corners(c.planes, c.npr)}
            self._corner["last"], self._corner["run"] = w4[c.planes - 1, N - 1, c.npr - 1, c.d0 - 1], w4[0, 0, 0, 17:20].copy()
            self._digest = digest_reference(self.words, c.planes, c.npr, c.d0)
        return self._corner, self._digest

    def drop_words(self):
        self._words = None


class Dense:
    """one set at one shape: params on both sides, two clients' keys, a random item file, `pool` distinct queries (query i: client
    i % 2) and the same after the edit list of tests/test_gpu_planar_resident.py::_edits applied as one /update-row body"""

    def __init__(self, sp, oracle_mod, name, nu_1, nu_2, pool):
        from test_gpu_planar_resident import _edits
        self.sp, self.name, self.cfg = sp, name, cfg(name, nu_1, nu_2)
        self.o, self.p = oracle_mod.Params(self.cfg), sp.Params(self.cfg)
        self.planes = planes_of(self.cfg)
        assert self.planes == PLANES[name] == self.p.instances * self.p.n * self.p.n
        self.cls = [oracle_mod.Client(self.o), oracle_mod.Client(self.o)]
        self.pps = [self.cls[0].generate_keys(61), self.cls[1].generate_keys(62)]
        self.gpps = [sp.PublicParameters.deserialize(self.p, pp) for pp in self.pps]
        self.isz, self.npr, self.d0 = self.o.db_item_size, self.o.num_per, self.o.dim0
        self.blob = np.random.default_rng(1000 * nu_1 + 10 * nu_2 + self.planes).integers(0, 256, self.o.num_items * self.isz, dtype=np.uint8)
        self.blob[:len(HEAD)] = HEAD
        self.blob.setflags(write=False)
        idxs = [(977 * i + 3) % self.o.num_items for i in range(pool)]
        self.before = _State(self, self.blob, idxs, 900)
        if self.npr >= 128:      # (the edit list names columns 126 and 127)
            self.edits, self.recs, after = _edits(self)
            after.setflags(write=False)
            # queries for edited items -- last row and column first, then both columns of a lane slot -- and one untouched item
            asked = [self.edits[4], self.edits[0], idxs[2 % pool]] + self.edits[1:4] + self.edits[5:8]
            self.after = _State(self, after, asked[:pool], 700)
            self.body = body([(self.edits[3], b"\x55" * self.isz)] + self.recs)      # edits[3] again later: the later one wins
            self.records = len(self.recs) + 1

    def gpp_list(self, B):
        return [self.gpps[i % 2] for i in range(B)]

    def batch(self, db, state, B):
        return self.sp.process_query_batch(self.p, self.gpp_list(B), state.qs[:B], db)

    def drop_words(self):
        self.before.drop_words()
        if hasattr(self, "after"):
            self.after.drop_words()


_pools = {}


def dense(sp, oracle_mod, name, nu_1, nu_2, pool):
    """the pool of (set, shape); the words of every other pool go (their responses and references stay)"""
    key = (name, nu_1, nu_2)
    for other_key, other in _pools.items():
        if other_key != key:
            other.drop_words()
    if key not in _pools:
        _pools[key] = Dense(sp, oracle_mod, name, nu_1, nu_2, pool)
    return _pools[key]
