"""The host half of the per-item digests (sp_db_item_digests_ref_words): no device call, so it runs on a host without a GPU.
  * the known answers of the definition (seed 0x5EED, num_per = 2, dim0 = 4, the pattern of tests/db_digest_reference.py, all four
    planes; plane 3 alone; the single word 1) through the numpy restatement of tests/item_digest_reference.py, which every other
    item-digest test uses as its reference, and through the library;
  * additivity: the lane sums of a table are the plane digests (digest_ref_words, and that file's KNOWN) added;
  * a plane cut into z-ranges accumulates to the whole plane, in any order;
  * words with limbs >= q digest like their limb-wise reduced form;
  * bad coordinates are refused and leave the accumulator alone;
  * both symbols are exported (and declared: tests/test_abi_symbols.py reads the header)."""
import ctypes as C

import numpy as np
import pytest

from conftest import FAST
from db_digest_reference import KNOWN, KNOWN_SEED, N, Q0, Q1, canon, digest_plane, pattern_plane, wrapping_sum
from item_digest_reference import (KNOWN_LANE_SUMS, KNOWN_PLANE3_ITEM5, KNOWN_TABLE, item_digests, item_digests_plane, lane_sums,
                                   unit_item)

CFG = dict(FAST, nu_1=2, nu_2=1)   # dim0 = 4, num_per = 2, 4 planes: the shape of the known answers


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    return sdk_amd


def _as_tuples(table):
    return tuple((int(a), int(b)) for a, b in np.asarray(table).reshape(-1, 2))


def test_known_answers_numpy():
    planes = [pattern_plane(k, 2, 4) for k in range(4)]
    table = item_digests(KNOWN_SEED, planes, 2, 4)
    assert _as_tuples(table) == KNOWN_TABLE
    assert lane_sums(table) == KNOWN_LANE_SUMS
    # ... which is the four plane digests added (additivity), two of them pinned by tests/test_db_digest_host.py
    per_plane = [digest_plane(KNOWN_SEED, k, planes[k], N, 2, 4) for k in range(4)]
    assert tuple(per_plane[0]) == KNOWN["plane0"] and tuple(per_plane[3]) == KNOWN["plane3"]
    assert tuple(int(x) for x in wrapping_sum([np.array(d, dtype=np.uint64) for d in per_plane])) == KNOWN_LANE_SUMS
    t3 = item_digests_plane(KNOWN_SEED, 3, planes[3], 2, 4)
    assert _as_tuples(t3)[5] == KNOWN_PLANE3_ITEM5
    assert lane_sums(t3) == KNOWN["plane3"]


def test_single_word_numpy():
    unit = np.zeros((N, 2, 4), dtype=np.uint64)
    unit[0, 0, 0] = 1
    t = _as_tuples(item_digests_plane(KNOWN_SEED, 0, unit, 2, 4))
    assert t[0] == KNOWN["unit"] == unit_item(KNOWN_SEED, 0, 0, 0, 0, 2, 4)
    assert all(x == (0, 0) for x in t[1:])


def test_known_answers_library(sp):
    p = sp.Params(CFG)
    assert (p.dim0, p.num_per) == (4, 2)
    acc = None
    for k in range(4):
        acc = sp.item_digests_ref_words(p, KNOWN_SEED, k, 0, pattern_plane(k, 2, 4), acc)
    assert acc.shape == (8, 2) and _as_tuples(acc) == KNOWN_TABLE
    t3 = sp.item_digests_ref_words(p, KNOWN_SEED, 3, 0, pattern_plane(3, 2, 4))
    assert _as_tuples(t3)[5] == KNOWN_PLANE3_ITEM5 and lane_sums(t3) == KNOWN["plane3"]
    unit = np.zeros((N, 2, 4), dtype=np.uint64)
    unit[0, 0, 0] = 1
    t = _as_tuples(sp.item_digests_ref_words(p, KNOWN_SEED, 0, 0, unit))
    assert t[0] == KNOWN["unit"] and all(x == (0, 0) for x in t[1:])


def test_lane_sums_are_the_plane_digests(sp):
    p = sp.Params(dict(FAST, nu_1=3, nu_2=2))
    rng = np.random.default_rng(15)
    acc, planes = None, []
    for k in range(4):
        w = canon(rng.integers(0, 2 ** 64, (N, 4, 8), dtype=np.uint64))
        acc = sp.item_digests_ref_words(p, 31, k, 0, w, acc)
        planes.append(np.array(sp.digest_ref_words(p, 31, k, 0, w), dtype=np.uint64))
        one = sp.item_digests_ref_words(p, 31, k, 0, w)
        assert lane_sums(one) == tuple(int(x) for x in planes[-1]), k
        assert (one == item_digests_plane(31, k, w, 4, 8)).all()
    assert lane_sums(acc) == tuple(int(x) for x in wrapping_sum(planes))


def test_z_ranges_accumulate_to_the_plane(sp):
    p = sp.Params(dict(FAST, nu_1=3, nu_2=2))
    rng = np.random.default_rng(5)
    words = canon(rng.integers(0, 2 ** 64, (N, 4, 8), dtype=np.uint64))
    want = item_digests_plane(77, 2, words, 4, 8)
    assert (sp.item_digests_ref_words(p, 77, 2, 0, words) == want).all()
    acc = np.zeros((32, 2), dtype=np.uint64)
    for z0, z1 in ((1500, N), (0, 1), (1, 1500)):     # three ranges, out of order
        assert sp.item_digests_ref_words(p, 77, 2, z0, words[z0:z1], acc) is acc
    assert (acc == want).all()
    # the numpy restatement cut the same way
    cut = np.zeros((32, 2), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for z0, z1 in ((1500, N), (0, 1), (1, 1500)):
            cut = cut + item_digests_plane(77, 2, words[z0:z1], 4, 8, z0=z0)
    assert (cut == want).all()
    # another plane of the same words is another table
    assert (sp.item_digests_ref_words(p, 77, 1, 0, words) != want).all()


def test_non_canonical_words_equal_their_reduced_form(sp):
    p = sp.Params(CFG)
    rng = np.random.default_rng(6)
    words = rng.integers(0, 2 ** 64, (N, 2, 4), dtype=np.uint64)
    words[0, 0, :4] = [0, (Q0 - 1) | ((Q1 - 1) << 32), Q0 | (Q1 << 32), 2 ** 64 - 1]
    assert ((words & np.uint64(0xFFFFFFFF)) >= np.uint64(Q0)).any() and ((words >> np.uint64(32)) >= np.uint64(Q1)).any()
    got = sp.item_digests_ref_words(p, 9, 1, 0, words)
    assert (got == sp.item_digests_ref_words(p, 9, 1, 0, canon(words))).all()
    assert (got == item_digests_plane(9, 1, canon(words), 2, 4)).all()


def test_bad_coordinates_leave_the_accumulator(sp):
    p = sp.Params(CFG)
    L = sp.lib()
    words = np.ones((2, 2, 4), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    for plane, z0, nz, w, null_acc in ((4, 0, 2, words, False), (-1, 0, 2, words, False), (0, N - 1, 2, words, False), (0, -1, 1, words, False),
                                       (0, 0, -1, words, False), (0, 0, 2, None, False), (0, 0, 2, words, True)):
        acc = np.full(16, 0xCCCC, dtype=np.uint64)
        rc = L.sp_db_item_digests_ref_words(C.c_void_p(p.h), C.c_uint64(1), C.c_int(plane), C.c_int(z0), C.c_int(nz),
                                            w.ctypes.data_as(u64p) if w is not None else None, None if null_acc else acc.ctypes.data_as(u64p))
        assert rc == -1, (plane, z0, nz)
        assert (acc == 0xCCCC).all()
    acc = np.full(16, 0xCCCC, dtype=np.uint64)
    assert L.sp_db_item_digests_ref_words(C.c_void_p(p.h), C.c_uint64(1), C.c_int(0), C.c_int(N), C.c_int(0), None, acc.ctypes.data_as(u64p)) == 0
    assert (acc == 0xCCCC).all()   # no rows: nothing added
    assert L.sp_db_item_digests_ref_words(None, C.c_uint64(1), C.c_int(0), C.c_int(0), C.c_int(1), words.ctypes.data_as(u64p),
                                          acc.ctypes.data_as(u64p)) == -1
    assert (acc == 0xCCCC).all()


def test_symbols_are_exported(sp):
    lib = C.CDLL(sp.library_path())
    assert hasattr(lib, "sp_db_item_digests") and hasattr(lib, "sp_db_item_digests_ref_words")
    assert sp.item_digests_ref_words is not None and sp.differing_items is not None
    assert hasattr(sp.Database, "item_digests") and hasattr(sp.Database, "repair_from")


def test_differing_items_compares_lanes_and_presence(sp):
    d = np.arange(12, dtype=np.uint64).reshape(6, 2)
    pr = np.array([1, 1, 0, 1, 1, 1], dtype=np.uint8)
    assert sp.differing_items((d, pr), (d.copy(), pr.copy())).size == 0
    e, q = d.copy(), pr.copy()
    e[1, 0] ^= np.uint64(1)      # lane 0 only
    e[4, 1] ^= np.uint64(1 << 63)   # lane 1 only
    q[2] = 1                      # presence only (both digests (x, x) equal)
    assert sp.differing_items((d, pr), (e, q)).tolist() == [1, 2, 4]
    with pytest.raises(sp.SpiralError):
        sp.differing_items((d, pr), (d[:5], pr[:5]))
