"""The host half of the database digest (sp_db_digest_ref_words): no device call, so it runs on a host without a GPU.
  * the known answers of the definition (seed 0x5EED, num_per = 2, dim0 = 4, the pattern of tests/db_digest_reference.py) and mix(0):
    through the numpy restatement, which every other digest test uses as its reference, and through the library;
  * a plane cut into z-ranges accumulates to the whole plane, in any order;
  * words with limbs >= q digest like their limb-wise reduced form;
  * bad coordinates are refused and leave the accumulator alone;
  * both symbols are exported (and declared: tests/test_abi_symbols.py reads the header)."""
import ctypes as C

import numpy as np
import pytest

from conftest import FAST
from db_digest_reference import KNOWN, KNOWN_SEED, MIX0, N, Q0, Q1, canon, digest_plane, mix, pattern_plane

CFG = dict(FAST, nu_1=2, nu_2=1)   # dim0 = 4, num_per = 2, 4 planes: the shape of the known answers


@pytest.fixture(scope="module")
def sp():
    import sdk_amd
    return sdk_amd


def _known_inputs():
    unit = np.zeros((N, 2, 4), dtype=np.uint64)
    unit[0, 0, 0] = 1
    return {"plane0": (0, pattern_plane(0, 2, 4)), "plane3": (3, pattern_plane(3, 2, 4)), "unit": (0, unit)}


def test_known_answers_numpy():
    assert int(mix(0)) == MIX0
    for name, (plane, words) in _known_inputs().items():
        assert tuple(digest_plane(KNOWN_SEED, plane, words, N, 2, 4)) == KNOWN[name], name


def test_known_answers_library(sp):
    p = sp.Params(CFG)
    assert (p.dim0, p.num_per) == (4, 2)
    for name, (plane, words) in _known_inputs().items():
        got = sp.digest_ref_words(p, KNOWN_SEED, plane, 0, words)
        assert tuple(int(x) for x in got) == KNOWN[name], name


def test_z_ranges_accumulate_to_the_plane(sp):
    p = sp.Params(dict(FAST, nu_1=3, nu_2=2))
    rng = np.random.default_rng(5)
    words = canon(rng.integers(0, 2 ** 64, (N, 4, 8), dtype=np.uint64))
    want = digest_plane(77, 2, words, N, 4, 8)
    whole = sp.digest_ref_words(p, 77, 2, 0, words)
    assert [int(x) for x in whole] == want
    acc = np.zeros(2, dtype=np.uint64)
    for z0, z1 in ((1500, N), (0, 1), (1, 1500)):     # three ranges, out of order
        assert sp.digest_ref_words(p, 77, 2, z0, words[z0:z1], acc) is acc
    assert [int(x) for x in acc] == want
    # another plane of the same words is another digest
    assert [int(x) for x in sp.digest_ref_words(p, 77, 1, 0, words)] != want


def test_non_canonical_words_equal_their_reduced_form(sp):
    p = sp.Params(CFG)
    rng = np.random.default_rng(6)
    words = rng.integers(0, 2 ** 64, (N, 2, 4), dtype=np.uint64)
    words[0, 0, :4] = [0, (Q0 - 1) | ((Q1 - 1) << 32), Q0 | (Q1 << 32), 2 ** 64 - 1]
    assert ((words & np.uint64(0xFFFFFFFF)) >= np.uint64(Q0)).any() and ((words >> np.uint64(32)) >= np.uint64(Q1)).any()
    got = [int(x) for x in sp.digest_ref_words(p, 9, 1, 0, words)]
    assert got == [int(x) for x in sp.digest_ref_words(p, 9, 1, 0, canon(words))] == digest_plane(9, 1, canon(words), N, 2, 4)


def test_bad_coordinates_leave_the_accumulator(sp):
    p = sp.Params(CFG)
    L = sp.lib()
    words = np.ones((2, 2, 4), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    for plane, z0, nz, w, null_acc in ((4, 0, 2, words, False), (-1, 0, 2, words, False), (0, N - 1, 2, words, False), (0, -1, 1, words, False),
                                       (0, 0, 2, None, False), (0, 0, 2, words, True)):
        acc = np.full(2, 0xCCCC, dtype=np.uint64)
        rc = L.sp_db_digest_ref_words(C.c_void_p(p.h), C.c_uint64(1), C.c_int(plane), C.c_int(z0), C.c_int(nz),
                                      w.ctypes.data_as(u64p) if w is not None else None, None if null_acc else acc.ctypes.data_as(u64p))
        assert rc == -1, (plane, z0, nz)
        assert (acc == 0xCCCC).all()
    acc = np.full(2, 0xCCCC, dtype=np.uint64)
    assert L.sp_db_digest_ref_words(C.c_void_p(p.h), C.c_uint64(1), C.c_int(0), C.c_int(N), C.c_int(0), None, acc.ctypes.data_as(u64p)) == 0
    assert (acc == 0xCCCC).all()   # no rows: nothing added


def test_symbols_are_exported(sp):
    lib = C.CDLL(sp.library_path())
    assert hasattr(lib, "sp_db_digest") and hasattr(lib, "sp_db_digest_ref_words")
    assert sp.digest_ref_words is not None and hasattr(sp.Database, "digest")
