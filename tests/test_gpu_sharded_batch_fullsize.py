"""The batched sharded list at the headline size: C2 (2^20 x 256 B), all G = 8 row shards on the one GPU, one pass over each
shard for a list of 8 queries.  Guarded by the free-HBM check of tests/test_gpu_fullsize.py (56 GiB of shards + 64 workspaces)."""
import gc

import pytest

from conftest import C2

pytestmark = pytest.mark.gpu

SEED = 0x123456789


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _need_hbm(gib):
    import torch
    gc.collect()
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    if free < gib * 2**30:
        pytest.skip("needs %d GiB of free HBM, %.1f available" % (gib, free / 2**30))


def test_c2_batched_list_over_eight_row_shards(sp, oracle_mod):
    """responses 0 and 7 equal the oracle's process_query_synth over the unsharded synthetic database, the rest the one-at-a-time
    sharded call's; every rank's pass was the scatter-form kernel"""
    from sdk_amd.sharding import LoopbackWorld
    _need_hbm(130)
    G = 8
    o = oracle_mod.Params(C2)
    cls = [oracle_mod.Client(o), oracle_mod.Client(o)]
    pps = [cls[0].generate_keys(501), cls[1].generate_keys(502)]
    qs = [(k % 2, cls[k % 2].generate_query((131071 * k + 777) % o.num_items, 900 + k)) for k in range(8)]
    p = sp.Params(C2)
    gpps = [sp.PublicParameters.deserialize(p, b) for b in pps]
    shards = [sp.Database(p, s, G).fill_synthetic(SEED) for s in range(G)]
    world = LoopbackWorld(G)
    pp_list, q_list = [gpps[c] for (c, _) in qs], [q for (_, q) in qs]

    def rank_main(r):
        sp.lib().sp_set_device(0)
        comm = world.comm(r)
        comm.reserve_batch(p, 8)
        sp.paths_taken()
        out = comm.process_queries_batched(p, pp_list, q_list, shards[r], group=8)
        taken = sp.paths_taken()
        singles = [comm.process_query(p, pp_list[k], q_list[k], shards[r]) for k in range(1, 7)]
        return out, taken, singles
    res = world.run(rank_main)
    for r in range(G):
        assert {"sweep_batch_scatter", "scatter_out", "expand_pruned", "custom_transport"} <= res[r][1], res[r][1]
        if r:
            assert res[r][0] == []
    got = res[0][0]
    assert len(got) == 8 and got[1:7] == res[0][2]
    for k in (0, 7):
        assert got[k] == o.process_query_synth(pps[qs[k][0]], qs[k][1], SEED), k
    del shards, world
    gc.collect()
