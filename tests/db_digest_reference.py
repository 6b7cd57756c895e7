"""The database digest (sp_db_digest) restated in numpy, independently of the library: what tests/test_db_digest_host.py,
tests/test_gpu_db_digest.py and, through the latter, tests/test_emulated_db_digest.py compare with.  Not a test file."""
import numpy as np

Q0, Q1 = 268369921, 249561089
N = 2048
M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """the finalizer of sp_synth_word, on uint64 scalars or arrays (wrapping)"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def digest_plane(seed, plane, words, N, num_per, dim0, j0=0):
    """words: uint64 [N][num_per][rows], canonical; rows = dim0 (j0 = 0), or a row shard's rows j0 .. j0 + rows - 1 of dim0"""
    words = np.asarray(words, dtype=np.uint64)
    out = []
    with np.errstate(over="ignore"):
        for l in (0, 1):
            s = mix(np.uint64(seed) + np.uint64(l))
            c = (np.uint64(plane * N) + np.arange(N, dtype=np.uint64))[:, None] * np.uint64(num_per) + np.arange(num_per, dtype=np.uint64)[None, :]
            A = mix(s ^ c) | np.uint64(1)
            R = mix(~s ^ np.arange(dim0, dtype=np.uint64)) | np.uint64(1)
            R = R[j0:j0 + words.shape[2]]
            out.append(int((A * (words * R).sum(axis=2, dtype=np.uint64)).sum(dtype=np.uint64)))
    return out


def canon(words):
    """both 32-bit limbs reduced mod their primes, as the loaders reduce them"""
    w = np.asarray(words, dtype=np.uint64)
    return ((w & M32) % np.uint64(Q0)) | (((w >> np.uint64(32)) % np.uint64(Q1)) << np.uint64(32))


def pattern_plane(plane, num_per, dim0):
    """the known answers' pattern: ref = ((plane N + z) num_per + ii) dim0 + j, w = (ref mod q0) | ((3 ref + 7) mod q1) << 32"""
    ref = (np.uint64(plane) * np.uint64(N) * np.uint64(num_per * dim0)
           + np.arange(N * num_per * dim0, dtype=np.uint64)).reshape(N, num_per, dim0)
    return (ref % np.uint64(Q0)) | (((np.uint64(3) * ref + np.uint64(7)) % np.uint64(Q1)) << np.uint64(32))


def wrapping_sum(digests):
    """lane-wise sum mod 2^64 of uint64 arrays [planes][2]"""
    with np.errstate(over="ignore"):
        total = np.zeros_like(np.asarray(digests[0], dtype=np.uint64))
        for d in digests:
            total = total + np.asarray(d, dtype=np.uint64)
    return total


# seed 0x5EED, num_per = 2, dim0 = 4 (the issue's table)
KNOWN_SEED = 0x5EED
KNOWN = {"plane0": (0x59ff5baad9aff430, 0x1f8f33ba0b79fbd0), "plane3": (0x1f25a7c1c532dce4, 0xe79f7ddd562b0df0),
         "unit": (0x69445e36d493c8c5, 0x2224019134450b29)}
MIX0 = 0xe220a8397b1dcdaf
