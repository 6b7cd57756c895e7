"""TEST INFRASTRUCTURE (run by tests/test_emulated_library.py in a child process with SPIRAL_HIP_LIB = the emulated build, under
AddressSanitizer where there is one): a batched pass holds the digit-planar copy it reads (sp_db::ensure_planar hands out a pin).

Thread 1 answers lists of eleven queries against a PACKED 64 x 128 database whose planar copy is built; thread 2 meanwhile switches
`batch_planar` off and on and calls sp_db_prepare_batch, which lets go of the handle's copy and builds a new one.  The database never
changes, so whichever kernel a group ran, every response must equal the oracle's.  The emulator's device memory is heap memory: a
pass that reads a copy freed (or freed and built again) under it shows as a heap error or as a response that differs.
Usage: python tests/_emu_planar_race.py   (prints planar-race-ok)"""
import ctypes as C
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
import sdk_amd as sp  # noqa: E402

LISTS = 3


def main():
    L = sp.lib()
    assert hasattr(L, "sp_emulated_device_marker"), "set SPIRAL_HIP_LIB to the emulated build"
    cfg = {"n": 2, "nu_1": 6, "nu_2": 7, "p": 256, "q2_bits": 20, "t_gsw": 4, "t_conv": 4, "t_exp_left": 8, "t_exp_right": 56,
           "instances": 1, "db_item_size": 256}
    o = oracle.Params(cfg)
    cl = oracle.Client(o)
    pp = cl.generate_keys(93)
    item, db = o.generate_random_db_and_get_item(5)
    p = sp.Params(cfg)
    gpp = sp.PublicParameters.deserialize(p, pp)
    gdb = sp.Database(p).load(db)
    assert gdb.prepare_batch() is True and gdb.batch_copy_bytes() > 0
    lists = [[cl.generate_query((173 * (11 * k + i) + 5) % o.num_items, 600 + 11 * k + i) for i in range(11)] for k in range(LISTS)]
    want = [[o.process_query(pp, q, db) for q in qs] for qs in lists]
    got, taken, errors = [], set(), []
    done = threading.Event()

    def answer():
        try:
            sp.paths_taken()
            for qs in lists:
                got.append(sp.process_query_batch(p, gpp, qs, gdb))
            taken.update(sp.paths_taken())   # (this thread's path bits)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    drops = 0
    t = threading.Thread(target=answer)
    t.start()
    while not done.wait(0.3):
        L.sp_debug_set(b"batch_planar", C.c_long(0))
        gdb.prepare_batch()                       # the handle lets go of its copy
        L.sp_debug_set(b"batch_planar", C.c_long(1))
        gdb.prepare_batch()                       # ... and builds a new one
        drops += 1
        time.sleep(0.2)
    t.join()
    assert not errors, errors
    for k in range(LISTS):
        assert got[k] == want[k], "list %d: responses differ" % k
    assert "sweep_batch_planar" in taken, taken
    assert drops >= 2, drops
    print("%d lists equal, %d drops beside them: %s" % (LISTS, drops, ",".join(sorted(x for x in taken if x.startswith("sweep")))))
    print("planar-race-ok")


if __name__ == "__main__":
    main()
