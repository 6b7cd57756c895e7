"""Every flow of the library on workspaces that other flows have already used.

A spiral::Workspace (sdk_amd/csrc/pipeline.hpp) outlives the query that held it: it goes back to a first-in first-out pool that belongs
to the Params handle (sp_params::acquire_ws / release_ws) with its buffers, their contents, its flags (out_G, zero_shortcuts,
pipelined, right_pending, mats_w_ready, ...) and its grown sizes.  A server keeps one Params handle for its lifetime; almost every
other test of this suite makes its own and so starts on a fresh workspace.  Here a FAMILY is one Params configuration with one
long-lived Params handle, two clients' public parameters and every database handle the family's STEPS need.  A step is one flow: every
byte it returns is compared with the oracle's (computed before the walk, cached per module), it asserts the path names it must take,
and consecutive occurrences alternate between two variants (another client, item and query seed), so that what the previous
occurrence left behind is never what this one needs.

  walk 1   the family's one-workspace steps along an Eulerian circuit of the complete directed graph with loops: every ordered pair
           (A, B), (A, A) included, is adjacent once; n * n + 1 steps.  A probe QueryRun before and after reads the workspace's stream:
           the same handle, or the pool did not hand the same workspace back and the walk proved nothing.
  walk 2   one case per step M that holds several workspaces, on a fresh Params handle: M, X, M, X', ... for every step X of the family.
           M grows the pool to k workspaces (counted with probes: k distinct streams, the k + 1-th is the first again); a one-workspace
           X runs k times in a row, so that every workspace M touched sees it.  The steps that hold several workspaces come last, in the
           order of their size, because they grow the pool.

A mismatch does not end a walk: up to 10 are collected, each is run once more on a fresh Params handle -- equal to the oracle there:
a HISTORY failure, else an ordinary PARITY failure -- and the text names the step index, the pair A -> B, the variant and the first
differing byte.  tests/test_emulated_workspace_history.py runs a subset on the emulated device.

Two shapes are not the ones one might expect: a planar row shard needs dim0 / G to be a multiple of 64, which 64 x 128 at G = 2 is
not, so the planar-shard steps have a family of their own (L, 128 x 128); sp_pack packs one instance, so the two-instance family V
has no pack step.  Families D and V have no row shards, so the abandoned and refused steps that need a shard are not among theirs."""
import contextlib
import threading
import types

import numpy as np
import pytest

from conftest import SMALL_INST2
from test_gpu_bulk_upsert import _body
from test_gpu_hardened_buffers import (N, PACKED, Q, RING, SPARSE, Side, _ask, _case, _limbs, _ntt_polys, _sparse_case, env_switch)
from test_gpu_narrow_batch import NO_EXPANSION, switch
from test_gpu_sharded_batch import _partial
from test_gpu_sparse_shards import _fold_and_finish, _reduce

pytestmark = pytest.mark.gpu

PLANAR_SHARDS = {"n": 2, "nu_1": 7, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
                 "instances": 1, "db_item_size": 256}      # shape A of tests/test_gpu_planar_shards.py: 64 local rows at G = 2
CONFIGS = {"P": PACKED, "L": PLANAR_SHARDS, "S": SPARSE, "R": RING, "D": NO_EXPANSION, "V": dict(SMALL_INST2, version=1)}
MAX_MISMATCHES = 10
POOL_MAX = 16


# ---- the oracle's side of a family: computed before a walk, cached per module ----------------------------------------------------
class Ref:
    def __init__(self, oracle_mod, fam):
        self.fam, self.cfg, self.oracle = fam, CONFIGS[fam], oracle_mod
        if fam == "S":
            self.sparse = _sparse_case(oracle_mod)          # the bucket, its two clients, queries before and after the /update-row body
            self.o, self.clients = self.sparse.o, self.sparse.clients
            self._dense_with_empty_columns()
        else:
            self.case = _case(oracle_mod, self.cfg)
            self.o, self.clients, self.words = self.case.o, self.case.clients, self.case.words
        self.planes = self.cfg.get("instances", 1) * self.cfg["n"] ** 2
        self._sets, self._wants, self.memo = {}, {}, {}

    def _dense_with_empty_columns(self):
        """Family S's dense database: the dense image of a SparseDb whose items sit in second-dimension column 7 (every row, 256
        bytes) and column 3 (every second row, 40 bytes: the planes behind the first hold nothing of them); columns 0, 1, 2, 4, 5, 6
        are all-zero words in every plane.  The fold pairs column i with i + half.  Level 0: (3, 7) with an all-zero left side in the
        planes the short items do not reach ((0, 4), (1, 5), (2, 6): both sides zero); level 1: the all-zero result of (1, 5) against
        that of (3, 7); level 2: the all-zero even half against the odd one.  On every level one side ONLY is all zero somewhere --
        simulated and asserted below -- which is where fold_zero_shortcut (fold.hip) returns the other ciphertext and the reference's
        dense fold (server.rs:388-427) multiplies.  need() asserts, with the oracle alone, that lib/server's fold over the same
        items answers other bytes."""
        o, rng = self.o, np.random.default_rng(77)
        sdb, self.dense_items = self.oracle.SparseDb(o), {}
        for j in range(o.dim0):
            for ii, size in ((3, 40), (7, 256)):
                if ii == 3 and j % 2:
                    continue
                self.dense_items[j * o.num_per + ii] = rng.integers(1, 256, size, dtype=np.uint8).tobytes()
        for idx, data in self.dense_items.items():
            sdb.update_item_raw(idx, data)
        self.dense_sdb, self.words = sdb, sdb.to_dense()
        ref = self.words.reshape(-1, N, o.num_per, o.dim0)
        zero = np.array([[not ref[pl, :, ii, :].any() for ii in range(o.num_per)] for pl in range(ref.shape[0])])
        assert zero[:, [0, 1, 2, 4, 5, 6]].all() and not zero[0, 3] and not zero[:, 7].all()
        one_sided = []
        for level in range(o.db_dim_2):          # a fold result is all zero only where both inputs are
            half = zero.shape[1] // 2
            one_sided.append(bool((zero[:, :half] != zero[:, half:]).any()))
            zero = zero[:, :half] & zero[:, half:]
        assert one_sided == [True] * o.db_dim_2, one_sided

    # dense families: two sets of queries; set v is queries v .. of a list with its own seeds, so position k of the two sets differs
    # in client, item index and seed
    def qset(self, v):
        if v not in self._sets:
            if self.fam == "S":
                idxs = [7, 3 * self.o.num_per + 3, 5 * self.o.num_per + 1, 6 * self.o.num_per + 7, 9 * self.o.num_per + 4, 2 * self.o.num_per + 3]
                self._sets[v] = [((k + v) % 2, i, self.clients[(k + v) % 2][0].generate_query(i, 500 + 100 * v + k)) for k, i in enumerate(idxs[v:] + idxs[:v])]
            else:
                self._sets[v] = self.case.queries(16 + v, 300 + 400 * v)[v:]
        return self._sets[v]

    def _want_for(self, queries):
        """the oracle's responses to `queries` over the family's dense words, kept by query bytes"""
        todo = [t for t in queries if t[2] not in self._wants]
        if self.fam == "S":
            for c, _, q in todo:
                self._wants[q] = self.o.process_query(self.clients[c][1], q, self.words)
                # the database discriminates: lib/server's fold over the same items (all-zero shortcuts) answers other bytes
                assert self._wants[q] != self.dense_sdb.process_query(self.clients[c][1], q)
        else:
            for (c, _, q), w in zip(todo, self.case.want(todo)):
                self._wants[q] = w

    def need(self, n):
        """the oracle's responses to the first n queries of both sets"""
        for v in (0, 1):
            self._want_for(self.qset(v)[:n])

    def need_at(self, k):
        """... to query k of both sets"""
        for v in (0, 1):
            self._want_for(self.qset(v)[k:k + 1])

    def bucket(self, v, updated):
        """family S's sparse bucket: five queries and lib/server's responses (oracle.SparseDb.process_query), before or after the
        /update-row body.  Variant 0 is SparseCase's own list (clients 0 1 0 1 0; a present item, an absent one, the first again, two
        more; after the body: the three records' items and the last two).  Variant 1 differs from it at every position in client
        (1 0 1 0 1), item index and seed: five other present items and another absent one before the body; after it the records'
        items in another order and two more items."""
        def make():
            case = self.sparse
            if v == 0:
                return (case.qs_after, case.want_after) if updated else (case.qs, case.want)
            present = list(case.items)
            if updated:
                idxs, sdb = [case.records[1][0], case.records[2][0], case.records[0][0], present[8], present[9]], case.sdb
            else:
                taken = set(case.items) | {i for i, _ in case.records} | {case.qs[1][1]}
                absent = next(i for i in range(self.o.num_items - 1, -1, -1) if i not in taken)
                idxs, sdb = [present[5], present[6], absent, present[7], present[5]], self.once("bucket-before", self._bucket_before)
            qs = [((k + 1) % 2, i, self.clients[(k + 1) % 2][0].generate_query(i, (700 if updated else 600) + k)) for k, i in enumerate(idxs)]
            other = case.qs_after if updated else case.qs
            assert all(a[0] != b[0] and a[1] != b[1] and a[2] != b[2] for a, b in zip(qs, other))
            return qs, [sdb.process_query(self.clients[c][1], q) for c, _, q in qs]
        return self.once(("bucket", v, updated), make)

    def _bucket_before(self):
        """the bucket as it is before the /update-row body (SparseCase keeps only the SparseDb with the body applied)"""
        sdb = self.oracle.SparseDb(self.o)
        for idx, data in self.sparse.items.items():
            sdb.update_item_raw(idx, data)
        return sdb

    def q(self, v, k):
        return self.qset(v)[k]

    def w(self, v, k):
        return self._wants[self.qset(v)[k][2]]      # (KeyError: the step's prep did not ask for it -- no oracle work inside a walk)

    def once(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]


_REFS = {}


def _ref(oracle_mod, fam):
    if fam not in _REFS:
        _REFS[fam] = Ref(oracle_mod, fam)
    return _REFS[fam]


# ---- the library's side: one Params handle, public parameters, database handles made once ----------------------------------------
class Fam:
    def __init__(self, sp, R, updated=False):
        self.sp, self.R, self.S = sp, R, Side(sp)
        self.p = self.S.params(R.cfg)
        self.gpps = self.S.pps(self.p, R)
        self._dbs, self.count, self.updated = {}, {}, False
        if updated:
            self.apply_update()

    def db(self, key):
        if key not in self._dbs:
            self._dbs[key] = self._make(key)
        return self._dbs[key]

    def _make(self, key):
        sp, S, p, R = self.sp, self.S, self.p, self.R
        if key == "bucket":
            return R.sparse.bucket(S, p)
        if key == "sparse-shards2":
            shards = [S.own(sp.Database.sparse(p, s, 2)) for s in range(2)]
            for sh in shards:
                sh.update_items(list(R.sparse.items.items()))
            assert sum(sh.sparse_items() for sh in shards) == len(R.sparse.items)
            return shards
        if key == "words8":
            with switch(sp, "db_unpacked", 1, default=0):
                db = S.db(p).load(R.words)
            assert db.format() == "words8"
            return db
        if key == "planar":
            return S.own(sp.Database.planar(p)).load(R.words)
        if key.startswith("planar-shards"):
            G = int(key[-1])
            return [S.own(sp.Database.planar_shard(p, s, G)).load(R.words) for s in range(G)]
        if key.startswith("shards"):
            G = int(key[-1])
            return [S.db(p, s, G).load(R.words) for s in range(G)]
        assert key == "main", key
        return S.db(p).load(R.words)

    def apply_update(self):
        assert self.db("bucket").update_rows(_body(self.R.sparse.records)) == (3, 4 + 256)
        self.updated = True

    def close(self):
        self.S.close()


# ---- steps ------------------------------------------------------------------------------------------------------------------------
class Step:
    """run(F, v) -> [(got, want)], bytes or uint64 arrays; prep(R) computes the oracle's side; holds: workspaces held at once (1:
    walk 1; more: walk 2, where the number is counted, and asserted when `exact`)"""

    def __init__(self, name, run, prep=None, holds=1, exact=True, dbs=(), threads=True, parts=1):
        self.name, self.run, self.prep, self.holds, self.exact, self.dbs, self.threads = name, run, prep, holds, exact, dbs, threads
        self.parts = parts      # walk 2 around this step is cut into this many cases, each with every parts-th other step (a slow step)


def _paths(taken, need=(), absent=()):
    assert set(need) <= taken and not (set(absent) & taken), (sorted(need), sorted(absent), sorted(taken))


def _refused(sp, call):
    """`call` must fail with SP_E_ARG (every refusal here is an argument or state check that returns before anything is enqueued)
    and leave a text in sp_last_error"""
    with pytest.raises(sp.SpiralError) as e:
        call()
    assert "rc=-1: " in str(e.value) and str(e.value).split("rc=-1: ", 1)[1].strip(), str(e.value)
    assert sp.lib().sp_last_error(), "sp_last_error is empty after a refused call"
    return []


@contextlib.contextmanager
def _switches(sp, switches=(), env=()):
    with contextlib.ExitStack() as st:
        for nm, v, d in switches:
            st.enter_context(switch(sp, nm, v, default=d))
        for nm, v in env:
            st.enter_context(env_switch(nm, v))
        yield


def single(name, dbkey, need, absent=(), env=(), k=0):
    def run(F, v):
        sp, (c, _, q) = F.sp, F.R.q(v, k)
        sp.paths_taken()
        with _switches(sp, env=env):
            got = sp.process_query(F.p, F.gpps[c], q, F.db(dbkey))
        _paths(sp.paths_taken(), need, absent)
        return [(got, F.R.w(v, k))]
    return Step(name, run, lambda R: R.need_at(k), dbs=(dbkey,), threads=not env)


def qlist(name, dbkey, n, need, absent=(), switches=(), holds=None, exact=True):
    def run(F, v):
        sp, qs = F.sp, F.R.qset(v)[:n]
        with _switches(sp, switches):
            got, taken = _ask(sp, F.p, F.gpps, qs, F.db(dbkey))
        _paths(taken, need, absent)
        assert len(got) == n
        return [(g, F.R.w(v, k)) for k, g in enumerate(got)]
    return Step(name, run, lambda R: R.need(n), holds=holds or n, exact=exact, dbs=(dbkey,))


def _hand(F, shards, G, query, per_plane, reduced=None):
    """the row-sharded flow on one thread: a QueryRun per shard begun for it, the scatter sweeps (chunk-major, or plane by plane), the
    test's own u32 sum of rank g's chunk over the shards, fold_local on rank g's run, the gather, finish_gathered on rank 0's
    (tests/test_gpu_sparse_shards.py's _by_hand); `reduced`: fold these summed chunks instead of the runs' own"""
    sp, (c, _, q) = F.sp, query
    b = types.SimpleNamespace(sp=sp, G=G, planes=F.R.planes)
    runs = [sp.QueryRun(F.p, F.gpps[c], q, db=shards[s]) for s in range(G)]
    try:
        parts = []
        for s, run in enumerate(runs):
            if per_plane:
                for pl in range(b.planes):
                    run.sweep_scatter_plane(shards[s], G, pl)
            else:
                run.sweep_scatter(shards[s], G)
            parts.append(_partial(sp, run))
        return _fold_and_finish(b, runs, _reduce(b, parts, per_plane) if reduced is None else reduced, per_plane)
    finally:
        for r in runs:
            r.free()


def sharded(name, dbkey, G, per_plane, need=("scatter_out",), k=0, qsel=None):
    def run(F, v):
        query, want = qsel(F, v) if qsel else (F.R.q(v, k), F.R.w(v, k))
        F.sp.paths_taken()
        got = _hand(F, F.db(dbkey), G, query, per_plane)
        _paths(F.sp.paths_taken(), need)
        return [(got, want)]
    return Step(name, run, None if qsel else (lambda R: R.need_at(k)), holds=G, dbs=(dbkey,))


def scatter_group(name, dbkey, G, B, need, absent=()):
    """sp_query_sweep_scatter_group of B queries on every shard in turn (the B runs of a shard are freed before the next shard's are
    begun: at most B workspaces); then every member's summed chunks go through the flow by hand, whose response must be the oracle's"""
    def run(F, v):
        sp, shards, qs = F.sp, F.db(dbkey), F.R.qset(v)[:B]
        b = types.SimpleNamespace(sp=sp, G=G, planes=F.R.planes)
        parts = []
        for s in range(G):
            runs = [sp.QueryRun(F.p, F.gpps[c], q, db=shards[s]) for c, _, q in qs]
            try:
                sp.paths_taken()
                sp.QueryRun.sweep_scatter_group(runs, shards[s], G)
                _paths(sp.paths_taken(), need, absent)
                parts.append([_partial(sp, r) for r in runs])
            finally:
                for r in runs:
                    r.free()
        return [(_hand(F, shards, G, qs[i], True, _reduce(b, [parts[s][i] for s in range(G)], True)), F.R.w(v, i)) for i in range(B)]
    return Step(name, run, lambda R: R.need(B), holds=B, dbs=(dbkey,), parts=2 if B > 8 else 1)


# ---- steps: the stage exports -----------------------------------------------------------------------------------------------------
def _neg(o, v_fold, levels):
    """G - C of `levels` levels with an oracle whose own nu_2 may be smaller: level by level, in the first slot of a padded operand"""
    per = v_fold.size // levels
    out = []
    for lv in range(levels):
        padded = np.zeros(max(o.db_dim_2, 1) * per, dtype=np.uint64)
        padded[:per] = v_fold[lv * per:(lv + 1) * per]
        out.append(o.get_v_folding_neg(padded)[:per])
    return np.concatenate(out)


class _Exports:
    """inputs and the oracle's outputs of the stage exports for variant v (client v, its own query and random operands), each made
    when a step's prep first asks for it"""

    def __init__(self, R, v):
        self.R, self.v, self.made = R, v, {}
        assert R.q(v, 0)[0] == v

    def __getitem__(self, key):
        if key not in self.made:
            name, arg = key if isinstance(key, tuple) else (key, None)
            self.made[key] = getattr(self, "_" + name)(*(() if arg is None else (arg,)))
        return self.made[key]

    def _ctx(self):
        return self.R.o, self.R.clients[self.v][1], self.R.q(self.v, 0)[2], np.random.default_rng(1000 + self.v)

    def _q(self):
        return self.R.q(self.v, 0)[2]

    def _expand(self):
        o, pp, q, _ = self._ctx()
        return o.expand_query(pp, q)

    def _expansion(self):
        o, pp, q, _ = self._ctx()
        g, sr, mb = o.g, o.stop_round, o.t_gsw * o.db_dim_2
        v0 = np.zeros((1 << g) * 2 * o.ntt_words, dtype=np.uint64)
        v0[:2 * o.ntt_words] = o.to_ntt(o.query_deserialize_ct(q))
        return v0, g, sr, mb, o.coefficient_expansion(pp, v0, g, sr, mb)

    def _gsw(self):
        o, pp, _, _ = self._ctx()
        v_cpu, mb, w = self["expansion"][4], o.t_gsw * o.db_dim_2, 2 * o.ntt_words
        gsw_inp = np.concatenate([v_cpu[(2 * i + 1) * w:(2 * i + 2) * w] for i in range(mb)])
        return gsw_inp, o.regev_to_gsw(gsw_inp, o.pp_deserialize_flat(pp)[-2 * 2 * o.t_conv * o.ntt_words:], o.db_dim_2)

    def _pack(self):
        o, pp, _, rng = self._ctx()
        v_ct = rng.integers(0, Q, o.n * o.n * 2 * N, dtype=np.uint64)
        return v_ct, o.pack(v_ct, o.pp_deserialize_flat(pp)[:o.n * (o.n + 1) * o.t_conv * o.ntt_words])

    def _fold(self, levels):
        """(the family's own depth, and one level more: the fold buffers are regrown)"""
        o, _, _, rng = self._ctx()
        v_fold = _ntt_polys(rng, levels * 2 * 2 * o.t_gsw)
        v_neg = _neg(o, v_fold, levels)
        cts = rng.integers(0, Q, (1 << levels) * 2 * N, dtype=np.uint64)
        return cts, v_fold, v_neg, o.fold_ciphertexts(cts, v_fold, v_neg, nu=levels)[:2 * N]

    def _neg(self):
        return self["fold", self.R.o.db_dim_2][1:3]

    def _sweep(self):
        o, _, _, rng = self._ctx()
        dim0, num_per = o.dim0, min(o.num_per, 128)
        db, qv = _limbs(rng, N * num_per * dim0), _limbs(rng, N * dim0 * 2)
        return db, qv, dim0, num_per, o.multiply_reg_by_database(db, qv, dim0, num_per)


def _export_ref(R, v):
    return R.once(("exports", v), lambda: _Exports(R, v))


def export(name, body, *keys):
    """keys: what of _Exports the body reads (made by the step's prep, before the walk)"""
    def run(F, v):
        import sdk_amd.spiral as L
        E = _export_ref(F.R, v)
        F.sp.paths_taken()
        return body(L, F, F.gpps[v], E)
    return Step(name, run, lambda R: [_export_ref(R, v)[("fold", R.o.db_dim_2 + k) if isinstance(k, int) else k] for v in (0, 1) for k in keys])


def _x_expand(L, F, gpp, E):
    v_reg, v_fold = L.expand_query(F.p, gpp, E["q"])
    return [(v_reg, E["expand"][0]), (v_fold, E["expand"][1])]


def _x_expansion(L, F, gpp, E):
    v0, g, sr, mb, v_cpu = E["expansion"]
    return [(L.coefficient_expansion(F.p, gpp, v0, g, sr, mb), v_cpu)]


def _x_gsw(L, F, gpp, E):
    return [(L.regev_to_gsw(F.p, gpp, E["gsw"][0], F.R.o.db_dim_2), E["gsw"][1])]


def _x_neg(L, F, gpp, E):
    return [(L.get_v_folding_neg(F.p, E["neg"][0]), E["neg"][1])]


def _x_pack(L, F, gpp, E):
    return [(L.pack(F.p, gpp, E["pack"][0]), E["pack"][1])]


def _x_sweep(L, F, gpp, E):
    db, qv, dim0, num_per, want = E["sweep"]
    got = L.multiply_reg_by_database(F.p, db, qv, dim0, num_per)
    assert any(t.startswith("sweep_") for t in F.sp.paths_taken())
    return [(got, want)]


def _x_fold(extra, fused):
    """sp_fold_ciphertexts (the literal path, the caller's G - C written into the workspace) or sp_fold_ciphertexts_fused with
    fused_min_pairs = `fused` (1: every level fused; 0: the workspace's own threshold), at nu_2 + extra levels"""
    def body(L, F, gpp, E):
        cts, v_fold, v_neg, want = E["fold", F.R.o.db_dim_2 + extra]
        if fused is None:
            got = L.fold_ciphertexts(F.p, cts, v_fold, v_neg)[:2 * N]
            _paths(F.sp.paths_taken(), {"fold_tail_literal"}, {"fold_fused"})
        else:
            got = L.fold_ciphertexts_fused(F.p, cts, v_fold, fused_min_pairs=fused)[:2 * N]
            taken = F.sp.paths_taken()
            _paths(taken, {"fold_fused"} if fused == 1 else (), {"fold_tail_literal"})
        return [(got, want)]
    return body


def fold_exports(fused_variants=(None, 1, 0)):
    names = {None: "fold-literal", 1: "fold-fused-min1", 0: "fold-fused-min0"}
    return [export("%s-%s" % (names[f], "deep" if extra else "own"), _x_fold(extra, f), extra) for f in fused_variants for extra in (0, 1)]


# ---- steps: abandoned queries and refused calls (in every family) -----------------------------------------------------------------
def common(main, shards=None, G=2, group=0, list_holds=8, list_db=None, list_switches=()):
    """main: the family's dense unsharded handle; shards: its row shards (None: the family has none); group: the size of an abandoned
    sweep_scatter_group; list_holds: the workspaces a list of 8 holds when its element 4 is refused"""
    steps = []

    def begun(F, v, db=None, k=1):
        c, _, q = F.R.q(v, k)
        return F.sp.QueryRun(F.p, F.gpps[c], q, db=db)

    def abandon_begun(F, v):
        begun(F, v, F.db(main)).free()
        return []

    def abandon_swept(F, v):
        run = begun(F, v, F.db(main)).sweep(F.db(main))
        run.free()
        return []

    def bench_then_finish(F, v):
        run = begun(F, v, F.db(main))
        try:
            assert run.bench_sweep(F.db(main), 2) > 0
            return [(run.sweep(F.db(main)).finish(), F.R.w(v, 1))]
        finally:
            run.free()

    def short_query(F, v):
        c, _, q = F.R.q(v, 1)
        return _refused(F.sp, lambda: F.sp.process_query(F.p, F.gpps[c], q[:-1], F.db(main)))

    def short_in_list(F, v):
        qs = [(c, i, q[:-1] if k == 4 else q) for k, (c, i, q) in enumerate(F.R.qset(v)[:8] if F.R.fam != "S" else (F.R.qset(v) + F.R.qset(v))[:8])]
        with _switches(F.sp, list_switches):
            return _refused(F.sp, lambda: _ask(F.sp, F.p, F.gpps, qs, F.db(list_db or main)))

    def finish_before_sweep(F, v):
        run = begun(F, v, F.db(main))
        try:
            return _refused(F.sp, run.finish)
        finally:
            run.free()

    def fold_local_before_sweep(F, v):
        run = begun(F, v, F.db(main))
        try:
            return _refused(F.sp, lambda: run.fold_local(run.partial_ptr(), 2))
        finally:
            run.free()

    steps += [Step("abandon-begun", abandon_begun, None, dbs=(main,)),
              Step("abandon-swept", abandon_swept, None, dbs=(main,)),
              Step("bench-sweep-then-finish", bench_then_finish, lambda R: R.need_at(1), dbs=(main,)),
              Step("refused-short-query", short_query, None, dbs=(main,)),
              Step("refused-short-query-in-list8", short_in_list, None, holds=list_holds, exact=False, dbs=(list_db or main,)),
              Step("refused-finish-before-sweep", finish_before_sweep, None, dbs=(main,)),
              Step("refused-fold-local-before-sweep", fold_local_before_sweep, None, dbs=(main,))]
    if shards is None:
        return steps

    def other_shard(F, v):
        sh = F.db(shards)
        run = begun(F, v, sh[0])
        try:
            return _refused(F.sp, lambda: (run.sweep_scatter(sh[1], G) if "planar" in shards or "sparse" in shards else run.sweep(sh[1])))
        finally:
            run.free()

    def wrong_count(F, v):
        sh = F.db(shards)
        run = begun(F, v, sh[0])
        try:
            return _refused(F.sp, lambda: run.sweep_scatter(sh[0], 2 * G))
        finally:
            run.free()

    def list_on_shard(F, v):
        qs = F.R.qset(v)[:2]
        return _refused(F.sp, lambda: _ask(F.sp, F.p, F.gpps, qs, F.db(shards)[0]))

    def abandon_plane0(F, v):
        sh = F.db(shards)
        runs = [begun(F, v, sh[s]) for s in range(G)]
        for s, run in enumerate(runs):
            run.sweep_scatter_plane(sh[s], G, 0)
        for run in runs:
            run.free()
        return []

    def abandon_one_plane_folded(F, v):
        """every plane swept on every shard, plane 0's summed chunk folded on rank 0's run, every run freed"""
        sp, sh = F.sp, F.db(shards)
        b = types.SimpleNamespace(sp=sp, G=G, planes=F.R.planes)
        runs = [begun(F, v, sh[s]) for s in range(G)]
        try:
            parts = []
            for s, run in enumerate(runs):
                for pl in range(b.planes):
                    run.sweep_scatter_plane(sh[s], G, pl)
                parts.append(_partial(sp, run))
            chunk = _reduce(b, parts, True)[0]
            from test_gpu_sparse_shards import _to_device
            owner, ptr = _to_device(sp, chunk[:chunk.size // b.planes])
            runs[0].fold_local_plane(ptr, G, 0)
            runs[0].sync()
            del owner
        finally:
            for run in runs:
                run.free()
        return []

    def abandon_group(F, v):
        sh = F.db(shards)[0]
        runs = [F.sp.QueryRun(F.p, F.gpps[c], q, db=sh) for c, _, q in F.R.qset(v)[:group]]
        try:
            F.sp.QueryRun.sweep_scatter_group(runs, sh, G)
        finally:
            for run in runs:
                run.free()
        return []

    steps += [Step("refused-sweep-over-another-shard", other_shard, None, dbs=(shards,)),
              Step("refused-wrong-shard-count", wrong_count, None, dbs=(shards,)),
              Step("refused-list-on-a-row-shard", list_on_shard, None, dbs=(shards,)),
              Step("abandon-plane0-swept", abandon_plane0, None, holds=G, dbs=(shards,)),
              Step("abandon-one-plane-folded", abandon_one_plane_folded, None, holds=G, dbs=(shards,))]
    if group:
        steps.append(Step("abandon-group-swept", abandon_group, None, holds=group, dbs=(shards,)))
    return steps


# ---- the families -----------------------------------------------------------------------------------------------------------------
SINGLE_PACKED = {"sweep_packed_persist", "sweep_ring", "from_sweep4_xcd_order", "fold_fused", "fold_wave", "fold_tail_delta"}
EXPANSION_EXPORTS = [("expand-query", _x_expand, "q", "expand"), ("coefficient-expansion", _x_expansion, "expansion"), ("regev-to-gsw", _x_gsw, "gsw"),
                     ("folding-neg", _x_neg, "neg")]


def _steps_P():
    return ([single("single-packed", "main", SINGLE_PACKED),
             single("single-words8", "words8", {"sweep_wide"}, {"sweep_packed_persist", "sweep_ring"}),
             single("single-planar", "planar", {"sweep_batch_planar"}, {"sweep_packed_persist", "sweep_ring", "sweep_wide"}),
             qlist("list3-valu", "main", 3, {"sweep_batch", "expand_group"}, {"sweep_batch_mfma"}),
             qlist("list8-matrix-cores", "main", 8, {"sweep_batch_mfma", "expand_group", "expand_round_one_launch"}, {"sweep_batch_mfma_two_tiles"}),
             qlist("list16-planar-copy", "main", 16, {"sweep_batch_mfma_two_tiles", "sweep_batch_planar", "expand_group"}),
             qlist("list16-two-tiles", "main", 16, {"sweep_batch_mfma_two_tiles"}, {"sweep_batch_planar"}, switches=[("batch_planar", 0, 1)]),
             sharded("sharded-G2-chunk-major", "shards2", 2, False), sharded("sharded-G2-per-plane", "shards2", 2, True),
             sharded("sharded-G4-chunk-major", "shards4", 4, False), sharded("sharded-G4-per-plane", "shards4", 4, True),
             scatter_group("scatter-group8-packed-shard", "shards2", 2, 8, {"scatter_out", "sweep_batch_scatter"})] +
            [export(*e) for e in EXPANSION_EXPORTS] + fold_exports() +
            [export("pack", _x_pack, "pack"), export("multiply-reg-by-database", _x_sweep, "sweep")] + common("main", "shards2", group=8))


def _steps_L():
    one_tile = {"scatter_out", "sweep_batch", "sweep_batch_mfma", "sweep_batch_planar"}

    def sweep_on_planar_shard(F, v):
        c, _, q = F.R.q(v, 1)
        sh = F.db("planar-shards2")[0]
        run = F.sp.QueryRun(F.p, F.gpps[c], q, db=sh)
        try:
            return _refused(F.sp, lambda: run.sweep(sh))
        finally:
            run.free()
    return ([single("single-packed", "main", {"fold_fused"}),
             sharded("planar-sharded-G2-chunk-major", "planar-shards2", 2, False, one_tile),
             sharded("planar-sharded-G2-per-plane", "planar-shards2", 2, True, one_tile),
             scatter_group("scatter-group16-planar-shard", "planar-shards2", 2, 16, one_tile | {"sweep_batch_mfma_two_tiles"}, {"sweep_batch_scatter"}),
             Step("refused-sweep-on-a-planar-shard", sweep_on_planar_shard, None, dbs=("planar-shards2",))] +
            common("main", "planar-shards2", group=16))


def _steps_S():
    def bucket_queries(F, v, n):
        """the first n of the bucket's queries of variant v and the oracle's responses, before or after the /update-row body"""
        qs, want = F.R.bucket(v, F.updated)
        return qs[:n], want[:n]

    def prep(R):
        for v in (0, 1):
            for updated in (False, True):
                R.bucket(v, updated)

    def bucket_list(name, n, switches, need, absent, holds, exact=True):
        def run(F, v):
            qs, want = bucket_queries(F, v, n)
            with _switches(F.sp, switches):
                got, taken = _ask(F.sp, F.p, F.gpps, qs, F.db("bucket"))
            _paths(taken, need, absent)
            return list(zip(got, want))
        return Step(name, run, prep, holds=holds, exact=exact, dbs=("bucket",))

    def bucket_single(F, v):
        (query,), (want,) = bucket_queries(F, v, 1)
        F.sp.paths_taken()
        got = F.sp.process_query(F.p, F.gpps[query[0]], query[2], F.db("bucket"))
        _paths(F.sp.paths_taken(), {"sweep_sparse", "fold_fused"}, {"sparse_group_pass"})
        return [(got, want)]

    def update_then_query(F, v):
        if not F.updated:
            F.apply_update()
            assert F.db("bucket").sparse_items() == 152
        return bucket_single(F, v)

    def abandon_bucket_swept(F, v):
        (query,), _ = bucket_queries(F, v, 1)
        F.sp.QueryRun(F.p, F.gpps[query[0]], query[2], db=F.db("bucket")).sweep(F.db("bucket")).free()
        return []

    def bucket_query_over_dense(F, v):
        (query,), _ = bucket_queries(F, v, 1)
        run = F.sp.QueryRun(F.p, F.gpps[query[0]], query[2], db=F.db("bucket"))
        try:
            return _refused(F.sp, lambda: run.sweep(F.db("main")))
        finally:
            run.free()

    def shard_query(F, v):
        case = F.R.sparse
        return case.qs[3 * v], case.want[3 * v]
    group_on, group_off = [("sparse_batch_min", 2, -1)], [("sparse_batch_min", 0, -1)]
    narrow_on, narrow_off = [("narrow_batch_min", 2, -1)], [("narrow_batch_min", 0, -1)]
    return ([Step("bucket-single", bucket_single, prep, dbs=("bucket",)),
             bucket_list("bucket-list5-group", 5, group_on, {"sparse_group_pass", "fold_fused"}, (), 5),
             bucket_list("bucket-list5-one-by-one", 5, group_off, {"sweep_sparse"}, {"sparse_group_pass"}, 3, exact=False),
             sharded("sparse-sharded-G2-chunk-major", "sparse-shards2", 2, False, {"scatter_out", "sweep_sparse"}, qsel=shard_query),
             sharded("sparse-sharded-G2-per-plane", "sparse-shards2", 2, True, {"scatter_out", "sweep_sparse"}, qsel=shard_query),
             single("dense-single", "main", {"sweep_narrow"}, {"sweep_sparse"}),
             qlist("dense-list5-narrow-group", "main", 5, {"sweep_narrow_group"}, {"sweep_narrow"}, switches=narrow_on),
             qlist("dense-list5-one-by-one", "main", 5, {"sweep_narrow"}, {"sweep_narrow_group"}, switches=narrow_off, holds=3, exact=False),
             Step("update-row-then-query", update_then_query, prep, dbs=("bucket",), threads=False),
             Step("abandon-bucket-swept", abandon_bucket_swept, prep, dbs=("bucket",)),
             Step("refused-bucket-query-over-dense", bucket_query_over_dense, prep, dbs=("bucket", "main"))] +
            common("main", "sparse-shards2", list_db="bucket", list_switches=group_on))


def _steps_R():
    pipelined = {"pipelined_fold_overlap", "sweep_ring", "fold_tail_batched", "expand_split"}
    return ([single("single-pipelined", "main", pipelined),
             single("single-not-pipelined", "main", {"sweep_ring"}, {"pipelined_fold_overlap"}, env=[("pipeline", 0)]),
             sharded("sharded-G2-per-plane", "shards2", 2, True), export("expand-query", _x_expand, "q", "expand"),
             qlist("list3", "main", 3, {"sweep_batch", "expand_group"})] + common("main", "shards2"))


def _steps_D():
    return ([single("single-direct-upload", "main", {"direct_upload", "sweep_narrow"}),
             qlist("list3-in-flight", "main", 3, {"direct_upload", "sweep_narrow"}, exact=False), export("multiply-reg-by-database", _x_sweep, "sweep")] +
            fold_exports((None,)) + common("main", list_holds=3))


def _steps_V():
    return ([single("single-pack-v1", "main", {"pack_v1", "sweep_narrow"}), qlist("list3-in-flight", "main", 3, {"pack_v1", "sweep_narrow"}, exact=False)] +
            common("main", list_holds=3))


STEPS = {"P": _steps_P(), "L": _steps_L(), "S": _steps_S(), "R": _steps_R(), "D": _steps_D(), "V": _steps_V()}
# the reduced walk of family P: one workspace except for the sharded flow, which holds two
REDUCED_P = ["single-packed", "single-words8", "sharded-G2-chunk-major", "fold-literal-own", "fold-literal-deep", "fold-fused-min1-own",
             "fold-fused-min1-deep", "abandon-begun", "abandon-swept", "refused-short-query", "refused-finish-before-sweep",
             "refused-fold-local-before-sweep", "refused-sweep-over-another-shard", "refused-wrong-shard-count"]
# what the emulated device runs of them within the time of tests/test_emulated_hardened_buffers.py (it is some thousand times slower)
EMULATED_P = ["single-packed", "sharded-G2-chunk-major", "fold-literal-deep", "fold-fused-min1-deep"]
EMULATED_S = ["bucket-single", "dense-single", "update-row-then-query", "abandon-bucket-swept", "refused-bucket-query-over-dense"]
EMULATED_S_AROUND_THE_GROUP_LIST = ["bucket-single", "dense-single"]
for _fam, _steps in STEPS.items():
    assert len({s.name for s in _steps}) == len(_steps), _fam
assert not set(REDUCED_P + EMULATED_P) - {s.name for s in STEPS["P"]} and not set(EMULATED_S + EMULATED_S_AROUND_THE_GROUP_LIST) - {s.name for s in STEPS["S"]}


# ---- walks ------------------------------------------------------------------------------------------------------------------------
def circuit(n):
    """an Eulerian circuit of the complete directed graph with loops on n vertices, as the vertex sequence of n * n + 1 entries: the
    de Bruijn sequence B(n, 2) by Lyndon words, closed with its first entry"""
    a, seq = [0] * (2 * n + 1), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, n):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    seq.append(seq[0])
    assert len(seq) == n * n + 1 and len(set(zip(seq, seq[1:]))) == n * n
    return seq


def _first_diff(got, want):
    """the first differing byte offset of two answers (bytes or arrays), None when they are equal"""
    g = np.frombuffer(got, dtype=np.uint8) if isinstance(got, (bytes, bytearray)) else np.ascontiguousarray(got).view(np.uint8).ravel()
    w = np.frombuffer(want, dtype=np.uint8) if isinstance(want, (bytes, bytearray)) else np.ascontiguousarray(want).view(np.uint8).ravel()
    if g.size != w.size:
        return min(g.size, w.size)
    bad = np.flatnonzero(g != w)
    return int(bad[0]) if bad.size else None


def _probe(F):
    """the stream of the workspace the pool hands out next (a QueryRun begun and freed: it goes to the back again)"""
    c, _, q = F.R.sparse.qs[0] if F.R.fam == "S" else F.R.q(0, 0)
    run = F.sp.QueryRun(F.p, F.gpps[c], q)
    try:
        s = run.stream()
        assert s, "sp_query_stream returned null"
        return s
    finally:
        run.free()


def _pool(F):
    """the pool's workspaces in the order it hands them out, by their streams: consecutive probes until the first one comes again"""
    streams = [_probe(F)]
    while True:
        s = _probe(F)
        if s == streams[0]:
            return streams
        assert s not in streams, "the pool is not first-in first-out: %r after %r" % (s, streams)
        streams.append(s)
        assert len(streams) <= POOL_MAX, "more than %d workspaces in the pool" % POOL_MAX


def _prepare(R, steps):
    """the oracle's side of `steps` (cached in R: nothing is computed twice)"""
    for s in steps:
        if s.prep:
            s.prep(R)


class Walk:
    def __init__(self, sp, oracle_mod, fam, names=None, steps=None):
        self.sp, self.oracle, self.fam = sp, oracle_mod, fam
        self.R = _ref(oracle_mod, fam)
        self.steps = steps or [s for s in STEPS[fam] if names is None or s.name in names]
        _prepare(self.R, self.steps)
        self.bad, self.done, self.fresh = [], 0, {}

    def open(self):
        F = Fam(self.sp, self.R)
        for s in self.steps:
            for key in s.dbs:
                F.db(key)
        return F

    def run(self, F, plan):
        """plan: [(step, times)]; every answer compared, mismatches collected"""
        prev = "(start)"
        for step, times in plan:
            for rep in range(times):
                v = F.count.get(step.name, 0) % 2
                F.count[step.name] = F.count.get(step.name, 0) + 1
                where = "step %d: %s -> %s, variant %d" % (self.done, prev, step.name, v)
                try:
                    answers = step.run(F, v)
                except Exception as e:
                    raise AssertionError("%s (family %s): %s: %s" % (where, self.fam, type(e).__name__, e)) from e
                for k, (got, want) in enumerate(answers):
                    off = _first_diff(got, want)
                    if off is not None and len(self.bad) < MAX_MISMATCHES:
                        self.bad.append((where, step, v, k, off, F.updated))
                self.done += 1
                prev = step.name

    def report(self, order):
        """asserts that nothing differed; a mismatch is classified by one run of the step's variant on a fresh Params handle"""
        if not self.bad:
            return
        lines = []
        for where, step, v, k, off, updated in self.bad:
            key = (step.name, v, updated)
            if key not in self.fresh:      # (at most MAX_MISMATCHES reruns: every kept mismatch is classified)
                F = Fam(self.sp, self.R, updated=updated and step.name != "update-row-then-query")
                try:
                    self.fresh[key] = all(_first_diff(g, w) is None for g, w in step.run(F, v))
                finally:
                    F.close()
            kind = {True: "HISTORY failure: the same step and variant on a fresh Params handle equals the oracle",
                    False: "PARITY failure: the same step and variant differs from the oracle on a fresh Params handle too"}[self.fresh[key]]
            lines.append("%s, answer %d: first differing byte %d -- %s" % (where, k, off, kind))
        names = [s.name for s in self.steps]
        pytest.fail("family %s: %d answers differ from the oracle (at most %d are kept)\n  %s\nsteps: %s\norder: %s" % (
            self.fam, len(self.bad), MAX_MISMATCHES, "\n  ".join(lines), ", ".join("%d=%s" % (i, n) for i, n in enumerate(names)),
            " ".join(str(names.index(n)) for n in order)))


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


ONE_WORKSPACE = {fam: [s.name for s in steps if s.holds == 1] for fam, steps in STEPS.items()}


def _fused_steps(fam):
    """the single query and the list of test_workspaces_made_under_another_fused_min_pairs: they assert the sweeps' path names only,
    because which fold levels are fused is what that switch changes"""
    sweep, batch = {"P": ("sweep_packed_persist", "sweep_batch_mfma"), "S": ("sweep_narrow", "sweep_narrow_group"), "R": ("sweep_ring", "sweep_batch"),
                    "D": ("sweep_narrow", "sweep_narrow"), "V": ("sweep_narrow", "sweep_narrow")}[fam]
    return [single("single", "main", {sweep}),
            qlist("list", "main", {"P": 8, "S": 5}.get(fam, 3), {batch}, switches=[("narrow_batch_min", 2, -1)] if fam == "S" else (), exact=False)]


FUSED_STEPS = {fam: _fused_steps(fam) for fam in ("P", "S", "R", "D", "V")}


def _named(fam, names):
    return [s for s in STEPS[fam] if names is None or s.name in names]


# test name -> (family; None: the test's `fam` parameter, the steps it walks as a function of the family): their oracle side is
# computed in the test's set-up phase
WALKED = {"test_walk_one_workspace": (None, lambda fam: _named(fam, ONE_WORKSPACE[fam])),
          "test_walk_many_workspaces": (None, lambda fam: STEPS[fam]),
          "test_workspaces_made_under_another_fused_min_pairs": (None, lambda fam: FUSED_STEPS[fam]),
          "test_walk_reduced_famP": ("P", lambda fam: _named(fam, REDUCED_P)),
          "test_walk_emulated_famP": ("P", lambda fam: _named(fam, EMULATED_P)),
          "test_walk_emulated_famS": ("S", lambda fam: _named(fam, EMULATED_S)),
          "test_walk_many_workspaces_emulated_famS": ("S", lambda fam: _named(fam, EMULATED_S_AROUND_THE_GROUP_LIST + ["bucket-list5-group"])),
          "test_two_threads_walk_family_P": ("P", lambda fam: _named(fam, ONE_WORKSPACE[fam]))}


@pytest.fixture(autouse=True)
def oracle_side(request, oracle_mod):
    """the oracle's answers for the steps of the test that follows, in its set-up phase: a test's call is the library's work only"""
    fam, steps = WALKED[request.node.originalname]
    fam = fam or request.node.callspec.params["fam"]
    _prepare(_ref(oracle_mod, fam), steps(fam))


def _walk_one(sp, oracle_mod, fam, names=None, pool=1):
    """the Eulerian circuit over the steps on one Params handle; the pool must hold `pool` workspaces at the end, and with one
    workspace the probes before and after must see the same stream"""
    W = Walk(sp, oracle_mod, fam, names)
    F = W.open()
    try:
        before = _probe(F)
        order = [W.steps[i] for i in circuit(len(W.steps))]
        W.run(F, [(s, 1) for s in order])
        streams = _pool(F)
        assert len(streams) == pool, "%d workspaces in the pool after the walk, not %d" % (len(streams), pool)
        assert before in streams, "the pool did not hand the first workspace back: the walk proved nothing"
    finally:
        F.close()
    W.report([s.name for s in order])


@pytest.mark.parametrize("fam", sorted(STEPS), ids=lambda f: "fam" + f)
def test_walk_one_workspace(sp, oracle_mod, fam):
    """walk 1: every ordered pair of the family's one-workspace steps, on the one workspace of a fresh Params handle"""
    _walk_one(sp, oracle_mod, fam, ONE_WORKSPACE[fam])


def test_walk_reduced_famP(sp, oracle_mod):
    """a reduced walk of family P with the sharded flow in it, which holds two workspaces: the single calls alternate between them"""
    _walk_one(sp, oracle_mod, "P", REDUCED_P, pool=2)


def test_walk_emulated_famP(sp, oracle_mod):
    """... cut down to what the emulated device runs in reasonable time (tests/test_emulated_workspace_history.py)"""
    _walk_one(sp, oracle_mod, "P", EMULATED_P, pool=2)


def test_walk_emulated_famS(sp, oracle_mod):
    """walk 1 of family S over the steps that a leaked zero_shortcuts, sparse index or layout would change, for the emulated device"""
    _walk_one(sp, oracle_mod, "S", EMULATED_S)


MANY = [pytest.param(fam, s.name, part, id="fam%s-%s%s" % (fam, s.name, "-part%d" % part if s.parts > 1 else ""))
        for fam in sorted(STEPS) for s in STEPS[fam] if s.holds > 1 for part in range(s.parts)]


@pytest.mark.parametrize("fam,name,part", MANY)
def test_walk_many_workspaces(sp, oracle_mod, fam, name, part):
    """walk 2 for one step M that holds several workspaces: (M, X) and (X, M) for every step X of the family (a slow M: for every
    second X in each of two cases)"""
    M = next(s for s in STEPS[fam] if s.name == name)
    others = [s.name for s in STEPS[fam] if s is not M]
    _walk_many(sp, oracle_mod, fam, name, [name] + others[part::M.parts] if M.parts > 1 else None)


def test_walk_many_workspaces_emulated_famS(sp, oracle_mod):
    """the sparse group list of five against the two single queries of family S, for the emulated device"""
    _walk_many(sp, oracle_mod, "S", "bucket-list5-group", EMULATED_S_AROUND_THE_GROUP_LIST + ["bucket-list5-group"])


def _walk_many(sp, oracle_mod, fam, name, names=None):
    W = Walk(sp, oracle_mod, fam, names)
    M = next(s for s in W.steps if s.name == name)
    F = W.open()
    try:
        W.run(F, [(M, 1)])
        streams = _pool(F)
        k = len(streams)
        assert 2 <= k <= POOL_MAX and (k == M.holds or not M.exact), "%s left %d workspaces in the pool (expected %d)" % (name, k, M.holds)
        assert len(set(streams)) == k      # (k distinct streams, and the k + 1-th probe saw the first again: _pool)
        rest = sorted((s for s in W.steps if s.holds > 1), key=lambda s: s.holds)
        plan = []
        for X in [s for s in W.steps if s.holds == 1]:
            plan += [(M, 1), (X, k)]
        for X in rest:
            plan += [(M, 1), (X, 1)]
        plan.append((M, 1))
        W.run(F, plan)
        after = _pool(F)
        assert len(after) >= k and set(streams) <= set(after), "workspaces of the walk have left the pool"
    finally:
        F.close()
    W.report([M.name] + [s.name for s, t in plan for _ in range(t)])


# ---- fused_min_pairs is read when a workspace is made -----------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["P", "S", "R", "D", "V"], ids=lambda f: "fam" + f)
@pytest.mark.parametrize("made_with", [1, 256], ids=["made-at-1-used-at-default", "made-at-default-used-at-1"])
def test_workspaces_made_under_another_fused_min_pairs(sp, oracle_mod, fam, made_with):
    """Workspace::fused_min_pairs comes from the switch when the workspace is made and sizes its digit staging; the workspaces of the
    single query and of the list are made under one value of the switch and used under the other: the oracle's bytes both times"""
    W = Walk(sp, oracle_mod, fam, steps=FUSED_STEPS[fam])
    used_with = 256 if made_with == 1 else 1
    F = W.open()
    try:
        with switch(sp, "fused_min_pairs", made_with, default=256):
            W.run(F, [(s, 1) for s in reversed(W.steps)])      # the list first: it makes every workspace
        with switch(sp, "fused_min_pairs", used_with, default=256):
            W.run(F, [(s, 1) for s in W.steps] * 2)
    finally:
        F.close()
    W.report([s.name for s in reversed(W.steps)] + [s.name for s in W.steps] * 2)


# ---- two host threads on the same handles -----------------------------------------------------------------------------------------
def test_two_threads_walk_family_P(sp, oracle_mod):
    """two host threads against one Params handle, its public parameters and databases, each with its own half of walk 1's sequence
    (the supported pattern of tests/test_gpu_compact_clients.py's threaded case); every answer compared.  Only steps that set no
    process-wide switch; each thread counts its own occurrences, so the variants alternate per thread."""
    W = Walk(sp, oracle_mod, "P", [s.name for s in STEPS["P"] if s.holds == 1 and s.threads])
    order = [W.steps[i] for i in circuit(len(W.steps))]
    half = len(order) // 2
    F = W.open()
    walks = [Walk(sp, oracle_mod, "P", [s.name for s in W.steps]) for _ in range(2)]
    views, errors = [], []
    for t in range(2):
        view = types.SimpleNamespace(**{k: getattr(F, k) for k in ("sp", "R", "p", "gpps", "db", "updated")})
        view.count = {}
        views.append(view)

    def main(t):
        try:
            sp.lib().sp_set_device(0)
            walks[t].run(views[t], [(s, 1) for s in (order[:half + 1] if t == 0 else order[half:])])
        except BaseException as e:
            errors.append(e)
    try:
        threads = [threading.Thread(target=main, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        if errors:
            raise errors[0]
        assert 1 <= len(_pool(F)) <= 2
    finally:
        F.close()
    for t in range(2):
        walks[t].report([s.name for s in (order[:half + 1] if t == 0 else order[half:])])
