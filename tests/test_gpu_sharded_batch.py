"""The batched database pass over ROW SHARDS (sp_query_sweep_scatter_group, k_sweep_mfma_scatter) and the list call built on it
(sp_process_queries_sharded_batched): one pass over a rank's shard per group of up to 8 queries, every query's output in the
per-plane reduce-scatter layout.  The contract is byte identity -- partial buffers word for word with the per-plane scatter
sweep's, responses with the oracle's process_query over the unsharded database and with the existing list call."""
import ctypes as C

import numpy as np
import pytest

from conftest import FAST, FAST56

pytestmark = pytest.mark.gpu

SCATTER = "sweep_batch_scatter"


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _wide(nu_1, nu_2, **kw):
    return dict(FAST, nu_1=nu_1, nu_2=nu_2, db_item_size=256, **kw)


def _clients(oracle_mod, cfg, n_queries, seed):
    """two clients' public parameters, queries alternating between them: [(pp_bytes, query_bytes, item index)]"""
    o = oracle_mod.Params(cfg)
    cls = [oracle_mod.Client(o), oracle_mod.Client(o)]
    pps = [cls[0].generate_keys(seed), cls[1].generate_keys(seed + 1)]
    out = []
    for k in range(n_queries):
        idx = (311 * k + 9) % o.num_items
        out.append((k % 2, cls[k % 2].generate_query(idx, seed + 10 + k), idx))
    return o, cls, pps, out


def _partial(sp, run):
    """host copy of a run's partial buffer (uint32)"""
    run.sync()
    n = run.partial_words()
    if hasattr(sp.lib(), "sp_emulated_device_marker"):     # the CPU suite's emulated device: device memory is host memory
        return np.ctypeslib.as_array(C.cast(run.partial_ptr(), C.POINTER(C.c_uint32)), shape=(n,)).copy()
    from sdk_amd.sharding import partial_tensor
    return partial_tensor(run).cpu().numpy().view(np.uint32).copy()


KERNEL_SHAPES = [(_wide(6, 7), 2), (_wide(7, 7), 4), (_wide(8, 8), 8), (_wide(6, 7, instances=2), 2)]
KERNEL_IDS = ["64x128-G2", "128x128-G4", "256x256-G8", "64x128-G2-8planes"]


@pytest.mark.parametrize("B", [4, 5, 8])
@pytest.mark.parametrize("cfg,G", KERNEL_SHAPES, ids=KERNEL_IDS)
def test_group_pass_leaves_the_per_plane_scatter_buffers(sp, oracle_mod, cfg, G, B):
    """after sweep_scatter_group every query's partial buffer equals, word for word, what the existing per-plane scatter sweep
    leaves for the same query and shard; the pass was the scatter-form kernel"""
    o, cls, pps, qs = _clients(oracle_mod, cfg, B, 71)
    p = sp.Params(cfg)
    planes = o.instances * o.n * o.n
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    _, db = o.generate_random_db_and_get_item(5)
    for s in sorted({G - 1, 0} if G == 2 else {G - 1}):
        shard = sp.Database(p, s, G).load(db)
        want = []
        for (c, q, _) in qs:
            run = sp.QueryRun(p, gpps[c], q, db=shard)
            for pl in range(planes):
                run.sweep_scatter_plane(shard, G, pl)
            want.append(_partial(sp, run))
            run.free()
        runs = [sp.QueryRun(p, gpps[c], q, db=shard) for (c, q, _) in qs]
        sp.paths_taken()
        sp.QueryRun.sweep_scatter_group(runs, shard, G)
        got = [_partial(sp, r) for r in runs]
        taken = sp.paths_taken()
        assert {SCATTER, "scatter_out", "sweep_batch", "sweep_batch_mfma"} <= taken, taken
        for k in range(B):
            assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (s, k, int((got[k] != want[k]).sum()))
        with pytest.raises(sp.SpiralError):
            sp.QueryRun.sweep_scatter_group(runs, shard, G)      # already swept
        for r in runs:
            r.free()


def test_group_pass_fallbacks_and_errors(sp, oracle_mod):
    """groups of 1 .. 3 and the batch_mfma = 0 switch sweep per query inside the same entry point (same words, no scatter bit);
    wrong handles and states are status codes"""
    cfg, G = _wide(6, 7), 2
    o, cls, pps, qs = _clients(oracle_mod, cfg, 4, 73)
    p = sp.Params(cfg)
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    _, db = o.generate_random_db_and_get_item(5)
    shard, other = sp.Database(p, 1, G).load(db), sp.Database(p, 0, G).load(db)
    want = []
    for (c, q, _) in qs:
        run = sp.QueryRun(p, gpps[c], q, db=shard)
        for pl in range(4):
            run.sweep_scatter_plane(shard, G, pl)
        want.append(_partial(sp, run))
        run.free()
    for B, switch in ((1, None), (3, None), (4, "batch_mfma")):
        if switch:
            sp.lib().sp_debug_set(switch.encode(), C.c_long(0))
        try:
            runs = [sp.QueryRun(p, gpps[c], q, db=shard) for (c, q, _) in qs[:B]]
            sp.paths_taken()
            sp.QueryRun.sweep_scatter_group(runs, shard, G)
            got = [_partial(sp, r) for r in runs]
            taken = sp.paths_taken()
        finally:
            if switch:
                sp.lib().sp_debug_set(switch.encode(), C.c_long(1))
        assert SCATTER not in taken and "scatter_out" in taken, taken
        for k in range(B):
            assert (got[k] == want[k]).all(), (B, k)
        for r in runs:
            r.free()
    runs = [sp.QueryRun(p, gpps[c], q, db=shard) for (c, q, _) in qs]
    unsharded, four, cols = sp.Database(p).load(db), sp.Database(p, 1, 4).load(db), sp.Database(p, 1, 2, by_columns=True).load(db)
    for handle, g in ((unsharded, 2), (four, 2), (shard, 4), (cols, 2), (other, 2)):   # `other`: begun for shard 1's rows
        with pytest.raises(sp.SpiralError):
            sp.QueryRun.sweep_scatter_group(runs, handle, g)
    with pytest.raises(sp.SpiralError):
        sp.QueryRun.sweep_scatter_group(runs + runs + [runs[0]], shard, G)     # nine
    p2 = sp.Params(_wide(6, 8))
    o2 = oracle_mod.Params(_wide(6, 8))
    cl2 = oracle_mod.Client(o2)
    alien = sp.QueryRun(p2, sp.PublicParameters.deserialize(p2, cl2.generate_keys(3)), cl2.generate_query(1, 4))
    with pytest.raises(sp.SpiralError):
        sp.QueryRun.sweep_scatter_group(runs[:3] + [alien], shard, G)          # other params
    sp.QueryRun.sweep_scatter_group(runs, shard, G)                            # the failed calls enqueued nothing and changed no state
    for k, r in enumerate(runs):
        assert (_partial(sp, r) == want[k]).all()
        r.free()
    alien.free()


def _flow(sp, oracle_mod, cfg, G, n, groups, seed=81, check_existing=True):
    """the list through LoopbackWorld(G): per group size (responses twice, path bits, describe()) of every rank"""
    from sdk_amd.sharding import LoopbackWorld
    o, cls, pps, qs = _clients(oracle_mod, cfg, n, seed)
    p = sp.Params(cfg)
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    _, db = o.generate_random_db_and_get_item(5)
    expect = [o.process_query(pps[c], q, db) for (c, q, _) in qs]
    shards = [sp.Database(p, s, G).load(db) for s in range(G)]
    world = LoopbackWorld(G)
    pp_list, q_list = [gpps[c] for (c, _, _) in qs], [q for (_, q, _) in qs]

    def rank_main(r):
        sp.lib().sp_set_device(0)
        comm, res = world.comm(r), {}
        for group in groups:
            sp.paths_taken()
            a = comm.process_queries_batched(p, pp_list, q_list, shards[r], group=group)
            b = comm.process_queries_batched(p, pp_list, q_list, shards[r], group=group)     # buffer reuse
            res[group] = (a, b, sp.paths_taken(), comm.describe())
        res["existing"] = comm.process_queries(p, pp_list, q_list, shards[r]) if check_existing else None
        res["empty"] = comm.process_queries_batched(p, [], [], shards[r])
        return res
    res = world.run(rank_main)
    for group in groups:
        assert res[0][group][0] == expect and res[0][group][1] == expect, group
        for r in range(1, G):
            assert res[r][group][0] == [] and res[r][group][1] == []
    if check_existing:
        assert res[0]["existing"] == expect
    assert all(res[r]["empty"] == [] for r in range(G))
    return o, cls, qs, expect, res


@pytest.mark.parametrize("cfg,G", [(_wide(6, 7), 2), (_wide(7, 7), 4), (_wide(8, 7), 8)], ids=["G2", "G4", "G8"])
def test_batched_list_over_the_loopback_world(sp, oracle_mod, cfg, G):
    """11 queries of two clients, group = 0 (the library's choice) and 4: rank 0's responses equal the oracle's over the unsharded
    database and the existing list call's on the same shards, twice; the other ranks return []; the pass was the scatter kernel"""
    o, cls, qs, expect, res = _flow(sp, oracle_mod, cfg, G, 11, (0, 4))
    planes = o.instances * o.n * o.n
    for r in range(G):
        for group, size in ((0, 8), (4, 4)):
            taken, info = res[r][group][2], res[r][group][3]
            assert {SCATTER, "scatter_out", "custom_transport", "expand_pruned"} <= taken and "rccl_in_library" not in taken, taken
            assert info["last_list"] == {"group": size, "reduce_scatters": 11 * planes, "all_gathers": 11}, info
    c, _, idx = qs[0]
    item, _ = o.generate_random_db_and_get_item(5)
    if idx == 5:
        assert cls[c].decode_response(expect[0]) == o.item_to_vec(item)


def test_batched_list_decodes_the_planted_item(sp, oracle_mod):
    """t_gsw = 8 leaves room to decode: response of a query for the planted item, through the batched list"""
    from sdk_amd.sharding import LoopbackWorld
    cfg, G, idx = _wide(6, 7), 2, 77
    o = oracle_mod.Params(cfg)
    cl = oracle_mod.Client(o)
    pp = cl.generate_keys(91)
    item, db = o.generate_random_db_and_get_item(idx)
    q_list = [cl.generate_query((idx + 13 * k) % o.num_items, 40 + k) for k in range(5)]
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    shards = [sp.Database(p, s, G).load(db) for s in range(G)]
    world = LoopbackWorld(G)

    def rank_main(r):
        sp.lib().sp_set_device(0)
        world.comm(r).reserve_batch(p, 0)
        sp.paths_taken()
        return world.comm(r).process_queries_batched(p, gpp, q_list, shards[r]), sp.paths_taken()
    res = world.run(rank_main)
    assert SCATTER in res[0][1] and SCATTER in res[1][1]
    assert cl.decode_response(res[0][0][0]) == o.item_to_vec(item)
    assert res[0][0] == [o.process_query(pp, q, db) for q in q_list]


@pytest.mark.parametrize("name,cfg,n,group", [("group-1", _wide(6, 7), 5, 1), ("list-of-3", _wide(6, 7), 3, 0),
                                              ("nj-16", _wide(5, 7), 5, 4), ("narrow", dict(FAST56, nu_2=4), 5, 4),
                                              ("narrow-choice", dict(FAST56, nu_2=4), 5, 0)],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_batched_list_fallbacks(sp, oracle_mod, name, cfg, n, group):
    """groups the scatter-form pass does not take are swept per query inside the same entry points: the oracle's bytes, and the
    new path bit stays clear"""
    G = 2
    o, cls, qs, expect, res = _flow(sp, oracle_mod, cfg, G, n, (group,), seed=83, check_existing=False)
    for r in range(G):
        taken = res[r][group][2]
        assert SCATTER not in taken and {"scatter_out", "custom_transport"} <= taken, taken


def test_batched_list_errors_enter_no_collective(sp, oracle_mod):
    from sdk_amd.sharding import LoopbackWorld
    cfg, G = _wide(6, 7), 2
    o, cls, pps, qs = _clients(oracle_mod, cfg, 6, 85)
    p = sp.Params(cfg)
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    _, db = o.generate_random_db_and_get_item(5)
    shard, unsharded, four = sp.Database(p, 0, G).load(db), sp.Database(p).load(db), sp.Database(p, 0, 4).load(db)
    world = LoopbackWorld(G)
    comm = world.comm(0)
    pp_list, q_list = [gpps[c] for (c, _, _) in qs], [q for (_, q, _) in qs]
    for group in (0, 4, 1):
        for handle in (unsharded, four):
            with pytest.raises(sp.SpiralError):
                comm.process_queries_batched(p, pp_list, q_list, handle, group=group)
        for pos in (0, 3, 5):
            bad = list(q_list)
            bad[pos] = bad[pos][:-8]
            with pytest.raises(sp.SpiralError):
                comm.process_queries_batched(p, pp_list, bad, shard, group=group)
    with pytest.raises(sp.SpiralError):
        comm.process_queries_batched(p, pp_list, q_list, shard, group=9)
    with pytest.raises(sp.SpiralError):
        comm.reserve_batch(p, 9)
    assert world.calls == [0] * G
