"""The per-item digests (sp_db_item_digests) restated in numpy, independently of the library: what tests/test_item_digests_host.py,
tests/test_gpu_item_digests.py and tests/test_emulated_item_digests.py compare with.  Built on tests/db_digest_reference.py (mix and the
keys are the plane digest's).  Not a test file."""
import numpy as np

from db_digest_reference import N, mix


def keys(seed, l, num_per, dim0, plane):
    """(A [N][num_per], R [dim0]) of lane l for one plane"""
    with np.errstate(over="ignore"):
        s = mix(np.uint64(seed) + np.uint64(l))
        c = (np.uint64(plane * N) + np.arange(N, dtype=np.uint64))[:, None] * np.uint64(num_per) + np.arange(num_per, dtype=np.uint64)[None, :]
        return mix(s ^ c) | np.uint64(1), mix(~s ^ np.arange(dim0, dtype=np.uint64)) | np.uint64(1)


def item_digests_plane(seed, plane, words, num_per, dim0, j0=0, z0=0):
    """one plane's contribution to the table: words uint64 [nz][num_per][rows] canonical, z-rows z0 .. and rows j0 .. j0 + rows - 1 of
    dim0 -> uint64 [dim0 * num_per][2], item i = j * num_per + ii; rows the words do not cover stay 0"""
    words = np.asarray(words, dtype=np.uint64)
    nz, _, rows = words.shape
    out = np.zeros((dim0, num_per, 2), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for l in (0, 1):
            A, R = keys(seed, l, num_per, dim0, plane)
            inner = (A[z0:z0 + nz, :, None] * words).sum(axis=0, dtype=np.uint64)   # [num_per][rows]
            out[j0:j0 + rows, :, l] = (inner * R[None, j0:j0 + rows]).T
    return out.reshape(dim0 * num_per, 2)


def item_digests(seed, planes_words, num_per, dim0, plane0=0, j0=0):
    """the table over planes plane0 .., planes_words[k] = the words [N][num_per][rows] of plane plane0 + k"""
    total = np.zeros((dim0 * num_per, 2), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k, w in enumerate(planes_words):
            total = total + item_digests_plane(seed, plane0 + k, w, num_per, dim0, j0=j0)
    return total


def lane_sums(table):
    """the two wrapping sums over the items of a table [items][2] -> (int, int)"""
    with np.errstate(over="ignore"):
        s = np.asarray(table, dtype=np.uint64).reshape(-1, 2).sum(axis=0, dtype=np.uint64)
    return int(s[0]), int(s[1])


def unit_item(seed, plane, z, ii, j, num_per, dim0):
    """the pair of the item that holds the single word 1 at (plane, z, ii, j): R_l(j) * A_l(c)"""
    out = []
    with np.errstate(over="ignore"):
        for l in (0, 1):
            A, R = keys(seed, l, num_per, dim0, plane)
            out.append(int(A[z, ii] * R[j]))
    return tuple(out)


# seed 0x5EED, num_per = 2, dim0 = 4, words = pattern_plane(plane, 2, 4), all four planes (the issue's table)
KNOWN_TABLE = ((0x11777012b12dcb70, 0x31ab05a168ae9880), (0x0624926103137240, 0xb5fc3bd5c1613210),
               (0x56b542b706ded504, 0x6045bdc51c20aaca), (0x6fda453df60f4850, 0x30c7ace9345fdbec),
               (0xd94ffb8302476378, 0x285d741883dca6fc), (0xb8eb0989869ddee0, 0xb353cc4690ffaad8),
               (0xe3adc62372503b9c, 0x5dd7b1966506420e), (0x48fc482e2175a330, 0x5cd42b37bac0d144))
KNOWN_LANE_SUMS = (0x9d109dc6cdda7c28, 0x0f11c952af33b66c)
KNOWN_PLANE3_ITEM5 = (0x4921a238356caa94, 0xddec82ba61bde884)
