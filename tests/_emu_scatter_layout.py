"""TEST INFRASTRUCTURE (run by tests/test_emulated_library.py in a child process with SPIRAL_HIP_LIB = the emulated build): a scatter
sweep that fails must not leave its output layout behind in the pooled workspace.

With ws_prealloc = 0 a workspace's first-dimension output buffer is allocated by the first sweep.  The emulator's device-memory
budget (tests/emu/emu_streams.cpp) makes that allocation fail inside sp_query_sweep_scatter, after the call has switched the
workspace to the reduce-scatter layout of two shards.  The query is freed, its workspace returns to the pool, and the next plain
sp_process_query with the same params -- which takes that workspace -- must still equal the oracle.
Usage: python tests/_emu_scatter_layout.py   (prints scatter-layout-ok)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
import sdk_amd as sp  # noqa: E402


def main():
    L = sp.lib()
    assert hasattr(L, "sp_emulated_device_marker"), "set SPIRAL_HIP_LIB to the emulated build"
    L.emu_device_live_bytes.restype = C.c_size_t
    L.emu_set_device_budget.argtypes = [C.c_size_t]
    cfg = {"n": 2, "nu_1": 6, "nu_2": 2, "p": 256, "q2_bits": 20, "t_gsw": 8, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 8,
           "instances": 1, "db_item_size": 256}
    o = oracle.Params(cfg)
    cl = oracle.Client(o)
    pp = cl.generate_keys(17)
    idx = 101
    q = cl.generate_query(idx, 18)
    _, db = o.generate_random_db_and_get_item(idx)
    want = o.process_query(pp, q, db)
    L.sp_debug_set(b"ws_prealloc", C.c_long(0))
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    gdb = sp.Database(p).load(db)
    shard = sp.Database(p, 0, 2).load(db)
    run = sp.QueryRun(p, gpp, q, db=shard)                  # the params' only workspace, no first-dimension output buffer yet
    L.emu_set_device_budget(L.emu_device_live_bytes())      # ... and no room for one
    try:
        run.sweep_scatter(shard, 2)
    except sp.SpiralError as e:
        print("scatter sweep failed as arranged: %s" % e, flush=True)
    else:
        raise AssertionError("the scatter sweep found memory for its output buffer: the budget hook no longer bites here")
    L.emu_set_device_budget(0)
    run.free()
    assert sp.process_query(p, gpp, q, gdb) == want, "the pooled workspace kept the failed sweep's scatter layout"
    L.sp_debug_set(b"ws_prealloc", C.c_long(1))
    print("scatter-layout-ok")


if __name__ == "__main__":
    main()
