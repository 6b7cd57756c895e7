"""Compact client registry: public parameters kept as the wire image on the device and expanded there on demand (sp_pp_compact,
sp_pp_expand, sp_pp_expand_into, k_pp_raw_image; sp_server_set_expanded_clients, sp_server_client_stats).

The reference throughout is the CPU oracle on the same bytes, and sp_pp_deserialize -- the host path the device path must equal word
for word.  Shapes, the smallest at which the code can go wrong: FAST (expansion right on the wire), FAST56, FAST with packing version 1
(no expansion-right matrix on the wire), the n = 3 set of tests/param_matrix.py (four-row packing matrices) and the direct-upload set
of tests/test_request_layer.py.  What costs oracle time (keys, queries, responses) is computed once per shape and never changed.

tests/test_emulated_compact_clients.py runs a subset of this file on the emulated device, where there is no device-memory counter:
the `mem_get_info` comparisons are made on a real device only."""
import base64
import ctypes as C
import gc
import json
import threading

import numpy as np
import pytest

from conftest import FAST, FAST56
from param_matrix import cfg as matrix_cfg
from test_gpu_crafted_inputs import CORE, craft

pytestmark = pytest.mark.gpu

SHAPES = {"fast": FAST, "fast56": FAST56, "v1": dict(FAST, version=1), "n3": matrix_cfg("N3", 4, 2)}
DIRECT = {"n": 2, "nu_1": 4, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 8, "t_conv": 4, "t_exp_left": 8,
          "t_exp_right": 56, "instances": 1, "db_item_size": 256, "direct_upload": 1}
SEEDS = (bytes(range(32)), bytes(31) + b"\x01", b"\xff" * 32)
GUARD_BYTES = 1 << 20


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    assert sdk_amd.lib().sp_device_count() >= 1, "no HIP device visible"
    return sdk_amd


def _free_bytes():
    """free device memory, or None on the emulated device (which has no counter)"""
    import torch
    if not torch.cuda.is_available():
        return None
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


_POOLS = {}


def _pool(oracle_mod, name, clients=2, queries=9):
    """a shape's honest sessions: `clients` key sets, `queries` queries (query i under client i % clients), the database and the
    oracle's response to every query"""
    if name == "direct":
        clients, queries = 1, 5           # one pool for every test of the direct-upload set
    key = (name, clients, queries)
    if key not in _POOLS:
        c = DIRECT if name == "direct" else SHAPES[name]
        o = oracle_mod.Params(c)
        db = o.generate_random_db_and_get_item(5)[1]
        cls = [oracle_mod.Client(o) for _ in range(clients)]
        pps = [cl.generate_keys(40 + k) for k, cl in enumerate(cls)]
        qs = [cls[i % clients].generate_query((131 * i + 5) % o.num_items, 700 + i) for i in range(queries)]
        want = [o.process_query(pps[i % clients], q, db) for i, q in enumerate(qs)]
        _POOLS[key] = dict(cfg=c, o=o, db=db, pps=pps, qs=qs, want=want, clients=clients)
    return _POOLS[key]


# ---------------------------------------------------------------------------------------------------------------- 1. keystream
def _device_keystream(sp, p, seed, first, count):
    out = np.full(max(count, 1) + 1, 0xCCCCCCCCCCCCCCCC, dtype=np.uint64)
    rc = sp.lib().sp_debug_chacha20_u64_device(C.c_void_p(p.h), (C.c_uint8 * 32)(*seed), C.c_size_t(first),
                                               out.ctypes.data_as(C.c_void_p), C.c_size_t(count))
    return rc, out


@pytest.mark.parametrize("first", [0, 8, 2048, 2048 * 37 + 8])
def test_device_keystream_equals_the_host_keystream(sp, oracle_mod, first):
    """k_pp_raw_image's generator == sp_debug_chacha20_u64 (pinned to RFC 8439 and rand_chacha by the oracle) from any block boundary,
    for lengths that end inside a block and span polynomials; nothing is written past `count`"""
    p = sp.Params(FAST)
    for seed in SEEDS:
        n_host = first + 2051
        host = np.zeros(n_host, dtype=np.uint64)
        assert sp.lib().sp_debug_chacha20_u64((C.c_uint8 * 32)(*seed), host.ctypes.data_as(C.c_void_p), C.c_size_t(n_host)) == 0
        assert (host == oracle_mod.chacha20_rng_u64(seed, n_host)).all()
        for count in (0, 1, 7, 8, 9, 2051):
            rc, out = _device_keystream(sp, p, seed, first, count)
            assert rc == 0, (first, count)
            assert (out[:count] == host[first:first + count]).all(), (first, count, seed[:2])
            assert (out[count:] == 0xCCCCCCCCCCCCCCCC).all(), (first, count)


def test_device_keystream_refuses_a_start_inside_a_block(sp):
    p = sp.Params(FAST)
    rc, out = _device_keystream(sp, p, SEEDS[0], 4, 8)
    assert rc == -1 and (out == 0xCCCCCCCCCCCCCCCC).all()


# ------------------------------------------------------------------------------------------ 2. expansion equals deserialization
def _crafted_set(pp):
    yield "honest", pp
    for family in CORE:
        for part in ("whole", "quarter"):
            yield "%s-%s" % (family, part), craft(pp, family, part)


@pytest.mark.parametrize("name", list(SHAPES) + ["direct"])
def test_expansion_equals_deserialization(sp, oracle_mod, name):
    """compact(pp).expand().export() == deserialize(pp).export() == the oracle's, word for word: honest parameters (a wrong counter,
    word order, kpos or `% modulus` corner shows here) and wire words no honest client sends (copied untouched, reduced by the
    transform as the host path's are)"""
    c = _pool(oracle_mod, name)
    p = sp.Params(c["cfg"])
    for label, pp in _crafted_set(c["pps"][0]):
        want = c["o"].pp_deserialize_flat(pp)
        got = sp.PublicParameters.compact(p, pp).expand().export()
        assert got.shape == want.shape and (got == want).all(), label
        assert (sp.PublicParameters.deserialize(p, pp).export() == got).all(), label


# --------------------------------------------------------------------------------- 3. every consumer of the other two layouts
@pytest.mark.parametrize("name", list(SHAPES))
def test_responses_through_an_expanded_handle(sp, oracle_mod, name):
    """sp_process_query, a list of 3 and a list of 9 (shared-launch group expansion reads all_w; version 1 and n = 3 pack from
    pack_cat): expanded handles == deserialized handles == the oracle"""
    c = _pool(oracle_mod, name)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    exp = [sp.PublicParameters.compact(p, pp).expand() for pp in c["pps"]]
    des = [sp.PublicParameters.deserialize(p, pp) for pp in c["pps"]]
    assert sp.process_query(p, exp[0], c["qs"][0], gdb) == sp.process_query(p, des[0], c["qs"][0], gdb) == c["want"][0]
    for B in (3, 9):
        got = sp.process_query_batch(p, [exp[i % 2] for i in range(B)], c["qs"][:B], gdb)
        assert got == sp.process_query_batch(p, [des[i % 2] for i in range(B)], c["qs"][:B], gdb), B
        assert got == c["want"][:B], B


def test_direct_upload_query_through_an_expanded_handle(sp, oracle_mod):
    c = _pool(oracle_mod, "direct", clients=1, queries=5)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    pp = sp.PublicParameters.compact(p, c["pps"][0]).expand()
    assert sp.process_query(p, pp, c["qs"][0], gdb) == c["want"][0]


# --------------------------------------------------------------------------------------------------------------- 4. slot reuse
def test_slot_reuse(sp, oracle_mod):
    """a slot expanded for client A answers as A; overwritten with B and with crafted parameters it exports and answers as those;
    its size does not change, further expansions allocate nothing, and a refused expansion leaves it answering as before"""
    c = _pool(oracle_mod, "fast")
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    ppA, ppB = c["pps"]
    cA, cB = sp.PublicParameters.compact(p, ppA), sp.PublicParameters.compact(p, ppB)
    slot = cA.expand()
    size = slot.device_bytes()
    assert sp.process_query(p, slot, c["qs"][0], gdb) == c["want"][0]
    assert cB.expand_into(slot) is slot
    assert (slot.export() == c["o"].pp_deserialize_flat(ppB)).all()
    assert sp.process_query(p, slot, c["qs"][1], gdb) == c["want"][1]
    crafted = craft(ppA, "full", "quarter")
    sp.PublicParameters.compact(p, crafted).expand_into(slot)
    assert (slot.export() == c["o"].pp_deserialize_flat(crafted)).all()
    assert sp.process_query(p, slot, c["qs"][0], gdb) == c["o"].process_query(crafted, c["qs"][0], c["db"])
    assert slot.device_bytes() == size
    # a handle of sp_pp_deserialize is a slot as well
    des = sp.PublicParameters.deserialize(p, ppA)
    cB.expand_into(des)
    assert (des.export() == c["o"].pp_deserialize_flat(ppB)).all() and des.device_bytes() == size
    free = _free_bytes()
    for i in range(20):
        (cA if i % 2 else cB).expand_into(slot)
    assert _free_bytes() == free
    assert sp.process_query(p, slot, c["qs"][0], gdb) == c["want"][0]        # (the 20th was A)
    # refused: a compact handle of other params; null arguments
    other = sp.Params(FAST56)
    c56 = sp.PublicParameters.compact(other, _pool(oracle_mod, "fast56")["pps"][0])
    with pytest.raises(sp.SpiralError):
        c56.expand_into(slot)
    assert sp.lib().sp_pp_expand_into(None, C.c_void_p(slot.h)) == -1 and sp.lib().sp_pp_expand_into(C.c_void_p(cA.h), None) == -1
    assert sp.process_query(p, slot, c["qs"][0], gdb) == c["want"][0]
    assert (slot.export() == c["o"].pp_deserialize_flat(ppA)).all()


# -------------------------------------------------------------------------------------------------------------------- 5. sizes
@pytest.mark.parametrize("name", list(SHAPES) + ["direct"])
def test_sizes(sp, oracle_mod, name):
    c = _pool(oracle_mod, name)
    p = sp.Params(c["cfg"])
    comp = sp.PublicParameters.compact(p, c["pps"][0])
    assert p.setup_bytes() <= comp.device_bytes() <= p.setup_bytes() + 4096
    des = sp.PublicParameters.deserialize(p, c["pps"][0])
    assert comp.expand().device_bytes() == des.device_bytes() > 2 * (p.setup_bytes() - 32)
    with pytest.raises(sp.SpiralError):
        sp.PublicParameters.compact(p, c["pps"][0][:-8])


# ----------------------------------------------------------------------------------------------------------------- 6. registry
def _registry_pool(oracle_mod):
    return _pool(oracle_mod, "fast", clients=6, queries=6)


def _registry_sequence(sp, c, srv):
    """five clients A .. E, single-query requests A, B, A, C, B: the responses and the exact counters"""
    uuids = [srv.setup(pp) for pp in c["pps"][:5]]
    for k in (0, 1, 0, 2, 1):
        assert srv.private_read([uuids[k].encode() + c["qs"][k]]) == [c["want"][k]], k
    st = srv.client_stats()
    assert (st["hits"], st["misses"], st["evictions"], st["overflows"], st["expanded"], st["registered"]) == (1, 4, 2, 0, 2, 5), st
    return uuids


def test_registry_with_two_slots(sp, oracle_mod):
    c = _registry_pool(oracle_mod)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    srv = sp.Server(p, gdb)
    srv.set_expanded_clients(2)
    uuids = _registry_sequence(sp, c, srv)
    assert srv.clients() == 5
    # one request naming all five (A twice: one slot): two slots, three overflows at least, never more than two expanded
    order = [0, 1, 2, 3, 4, 0]
    assert srv.private_read([uuids[k].encode() + c["qs"][k] for k in order]) == [c["want"][k] for k in order]
    st = srv.client_stats()
    assert st["overflows"] >= 1 and st["expanded"] <= 2 and st["registered"] == 5, st
    assert st["hits"] + st["misses"] + st["overflows"] == 5 + 5, st
    comp = sp.PublicParameters.compact(p, c["pps"][0])
    slot_bytes = comp.expand().device_bytes()
    assert st["device_bytes"] == 5 * comp.device_bytes() + 2 * slot_bytes, st
    # forget: an expanded client (A holds a slot since the request of five: reading it once more is a hit) and a compact-only one (E
    # overflowed there)
    assert srv.private_read([uuids[0].encode() + c["qs"][0]]) == [c["want"][0]]
    assert srv.client_stats()["hits"] == st["hits"] + 1 and srv.client_stats()["expanded"] == 2
    srv.forget(uuids[0])
    assert srv.client_stats()["expanded"] == 1
    srv.forget(uuids[4])
    assert srv.client_stats()["expanded"] == 1
    for k in (0, 4):
        with pytest.raises(sp.NotFound):
            srv.private_read([uuids[k].encode() + c["qs"][k]])
        with pytest.raises(sp.NotFound):
            srv.forget(uuids[k])
    assert srv.clients() == 3 and srv.client_stats()["registered"] == 3
    assert srv.private_read([uuids[1].encode() + c["qs"][1]]) == [c["want"][1]]       # the others still answer
    assert srv.client_stats()["device_bytes"] == 3 * comp.device_bytes() + 2 * slot_bytes     # slots are kept
    with pytest.raises(sp.SpiralError):
        srv.set_expanded_clients(3)                        # after a /setup
    with pytest.raises(sp.SpiralError):
        srv.set_expanded_clients(0)


def test_registry_default_keeps_every_client_expanded(sp, oracle_mod):
    c = _registry_pool(oracle_mod)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    srv = sp.Server(p, gdb)
    uuids = [srv.setup(pp) for pp in c["pps"][:3]]
    assert srv.private_read([uuids[2].encode() + c["qs"][2]]) == [c["want"][2]]
    st = srv.client_stats()
    assert st["registered"] == st["expanded"] == 3 and st["evictions"] == st["overflows"] == 0, st
    assert st["device_bytes"] == 3 * sp.PublicParameters.deserialize(p, c["pps"][0]).device_bytes()
    with pytest.raises(sp.SpiralError):
        srv.set_expanded_clients(2)


def test_registry_json_bodies_do_not_depend_on_k(sp, oracle_mod):
    c = _registry_pool(oracle_mod)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    bodies = []
    for k in (0, 2):
        srv = sp.Server(p, gdb)
        srv.set_expanded_clients(k)
        uuids = []
        for pp in c["pps"][:3]:
            resp = json.loads(srv.setup_json(json.dumps(base64.b64encode(pp).decode())))
            assert set(resp) == {"uuid"} and len(resp["uuid"]) == 36 and resp["uuid"][14] == "4"
            uuids.append(resp["uuid"])
        body = json.dumps([base64.b64encode(uuids[i].encode() + c["qs"][i]).decode() for i in (0, 1, 2, 0)])
        bodies.append(srv.private_read_json(body))
        assert srv.private_read_json("[]") == "[]"
    assert bodies[0] == bodies[1] == json.dumps([base64.b64encode(c["want"][i]).decode() for i in (0, 1, 2, 0)], separators=(",", ":"))


# ------------------------------------------------------------------------------------------------------------ 7. direct upload
def test_direct_upload_with_two_slots(sp, oracle_mod):
    """params without query expansion at k = 2: the public parameters of a request element go through the slot's wire buffer and
    the device path; a list longer than the slots overflows; the steady state allocates nothing"""
    c = _pool(oracle_mod, "direct", clients=1, queries=5)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    srv = sp.Server(p, gdb)
    srv.set_expanded_clients(2)
    pp = c["pps"][0]
    assert srv.private_read([pp + q for q in c["qs"][:2]]) == c["want"][:2]
    free = _free_bytes()
    for _ in range(20):
        assert srv.private_read([pp + q for q in c["qs"][:2]]) == c["want"][:2]
    assert _free_bytes() == free
    assert srv.private_read([pp + q for q in c["qs"]]) == c["want"]
    st = srv.client_stats()
    assert srv.clients() == 0 and st["registered"] == 0 and st["overflows"] == 3 and st["misses"] == 2 * 21 + 2, st
    comp = sp.PublicParameters.compact(p, pp)
    assert st["device_bytes"] == 2 * (comp.device_bytes() + comp.expand().device_bytes())


# ------------------------------------------------------------------------------------------------------------------ 8. threads
def test_registry_under_threads(sp, oracle_mod):
    """four threads, six single-query requests each over six clients, two slots: every response is the oracle's and every request
    was a hit, a miss or an overflow"""
    c = _registry_pool(oracle_mod)
    p = sp.Params(c["cfg"])
    gdb = sp.Database(p).load(c["db"])
    srv = sp.Server(p, gdb)
    srv.set_expanded_clients(2)
    uuids = [srv.setup(pp) for pp in c["pps"]]
    wrong = []

    def work(t):
        try:
            for i in range(6):
                k = (t * 5 + i * (1 + t % 2 * 4)) % 6          # threads 0 and 2 walk upwards, 1 and 3 downwards
                if srv.private_read([uuids[k].encode() + c["qs"][k]]) != [c["want"][k]]:
                    wrong.append((t, i, k))
        except Exception as e:                                  # noqa: BLE001
            wrong.append((t, repr(e)))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not wrong, wrong
    st = srv.client_stats()
    assert st["hits"] + st["misses"] + st["overflows"] == 24 and st["expanded"] <= 2 and st["registered"] == 6, st


# -------------------------------------------------------------------------------------------------------------- 9. instruments
@pytest.mark.parametrize("switch,value", [("poison_ws", 0xA5), ("poison_ws", 0xFF), ("guard_ws", GUARD_BYTES)])
def test_on_hardened_buffers(sp, oracle_mod, capfd, switch, value):
    """one expansion, one expand_into and the registry sequence on poisoned buffers and between guard regions: the same bytes, no
    out-of-bounds report when the buffers are released, the switch back at 0 afterwards"""
    c = _registry_pool(oracle_mod)
    want_A, want_B = c["o"].pp_deserialize_flat(c["pps"][0]), c["o"].pp_deserialize_flat(c["pps"][1])
    capfd.readouterr()
    sp.lib().sp_debug_set(switch.encode(), C.c_long(value))
    try:
        p = sp.Params(c["cfg"])
        gdb = sp.Database(p).load(c["db"])
        slot = sp.PublicParameters.compact(p, c["pps"][0]).expand()
        assert (slot.export() == want_A).all()
        sp.PublicParameters.compact(p, c["pps"][1]).expand_into(slot)
        assert (slot.export() == want_B).all()
        assert sp.process_query(p, slot, c["qs"][1], gdb) == c["want"][1]
        srv = sp.Server(p, gdb)
        srv.set_expanded_clients(2)
        _registry_sequence(sp, c, srv)
        del srv, slot, gdb, p
        gc.collect()
    finally:
        sp.lib().sp_debug_set(switch.encode(), C.c_long(0))
    err = capfd.readouterr().err
    assert "OUT-OF-BOUNDS" not in err, err[-2000:]
