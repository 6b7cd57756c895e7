// sp_db_copy_items, the dense writers: item-major words stage[index][plane][z] (canonical lo | hi << 32: a window that one of the gathers
// of item_readback.hpp / planar_resident.hpp has written, or a sparse bucket's store read in place) -> the resident words of an 8-byte
// or a PACKED handle.  The inverses of k_items_gather_words8 / k_items_gather_packed: nothing is decoded, nothing is encoded again, and
// there is no second re-layout pass -- a word goes from the stage to its resident position through one LDS tile.
// Each kernel is driven by a device list the host builds per window (capi_copy.hpp); an entry < 0 means "not written by this call".
// Plain vector loads and stores only.  Included by db.hip only.
#pragma once
#include "device_common.hpp"

namespace spiral {

// ---- 8-byte words [plane][z][jl][il] (row shards, column shards -- the handle's LOCAL columns -- and odd row counts alike): the items a
// window writes are a run [D0, D0 + nD) of the handle's local linear index (item_readback.hpp), src_of[L - D0] = the stage index of the
// item at L, or -1.  grid (ceil(nD / 32), N / 32, planes): the gather's 32 x 33 tile, lanes along z on the read (an item's polynomial
// is contiguous) and along the local index on the write (256-byte runs of the resident row).
__global__ __launch_bounds__(256) void k_items_scatter_words8(u64* db, const u64* stage, const int* src_of, size_t D0, size_t nD,
                                                             size_t row_words, int planes) {
  __shared__ u64 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const size_t lt = (size_t)blockIdx.x * 32;
  const int zt = blockIdx.y * 32, plane = blockIdx.z;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const size_t l = lt + ty + 8 * i;
    const int s = l < nD ? src_of[l] : -1;
    if (s >= 0) tile[ty + 8 * i][tx] = stage[((size_t)s * planes + plane) * N + zt + tx];
  }
  __syncthreads();
  const int mine = lt + tx < nD ? src_of[lt + tx] : -1;
  if (mine < 0) return;   // (after the only barrier)
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int zl = ty + 8 * i;
    db[((size_t)plane * N + zt + zl) * row_words + D0 + lt + tx] = tile[tx][zl];
  }
}

// ---- PACKED: the four words of a quad (rows 2 jp, 2 jp + 1 x columns 2 l, 2 l + 1) share one 28-byte lane group, so ONE THREAD owns a
// quad of one (plane, z): entries the call does not write (src < 0, the idea of DbQuadRec) are unpacked from the resident lane group and
// packed back with the new ones.  The host lists a quad once per launch with every item of it that the launch writes.
// A workgroup takes 64 listed quads (neighbours in the list are neighbours in a unit for a whole-range copy: 64 lanes' 16 + 12 bytes) for
// 16 z-rows of one plane; the quads' 256 words get there through the gather's tile, read as 128-byte z-runs of the stage.
// grid (ceil(n_quads / 64), N / 16, planes)
constexpr int SCATTER_Z = 16;
__global__ __launch_bounds__(256) void k_items_scatter_packed(u32* db, const u64* stage, const CopyQuadRec* quads, size_t n_quads,
                                                             int np_local, int nj, int planes) {
  __shared__ u64 tile[256][SCATTER_Z + 1];
  const int chunks = np_local >> 7, npairs = nj >> 1;
  const size_t q0 = (size_t)blockIdx.x * 64;
  const int plane = blockIdx.z, z0 = blockIdx.y * SCATTER_Z;
  {
    const int zl = threadIdx.x & (SCATTER_Z - 1);
#pragma unroll 1
    for (int pass = 0; pass < 256 / (256 / SCATTER_Z); pass++) {
      const int u = pass * (256 / SCATTER_Z) + (threadIdx.x >> 4);   // tile row: which = u >> 6, quad of the workgroup = u & 63
      const size_t k = q0 + (size_t)(u & 63);
      const int s = k < n_quads ? quads[k].src[u >> 6] : -1;
      if (s >= 0) tile[u][zl] = stage[((size_t)s * planes + plane) * N + z0 + zl];
    }
  }
  __syncthreads();
  const int k = threadIdx.x & 63, zq = threadIdx.x >> 6;
  if (q0 + (size_t)k >= n_quads) return;   // (after the only barrier)
  const CopyQuadRec r = quads[q0 + (size_t)k];
  const int chunk = r.q >> 6, lane = r.q & 63;
#pragma unroll 1
  for (int pass = 0; pass < SCATTER_Z / 4; pass++) {
    const int zl = pass * 4 + zq;
    u32* unit = db + packed_unit_offset((size_t)plane * N + z0 + zl, r.jp, chunk, npairs, chunks);
    u64 w[4];
#pragma unroll
    for (int which = 0; which < 4; which++) w[which] = r.src[which] >= 0 ? tile[which * 64 + k][zl] : unpack_word(unit, lane, which);
    pack_unit_lane(unit, lane, w[0], w[1], w[2], w[3]);
  }
}

void launch_items_scatter_words8(u64* db, const u64* stage, const int* src_of, size_t D0, size_t nD, int np_local, int nj, int planes,
                                 hipStream_t s) {
  if (nD == 0) return;
  hipLaunchKernelGGL(k_items_scatter_words8, dim3((unsigned)((nD + 31) / 32), N / 32, planes), dim3(256), 0, s, db, stage, src_of, D0, nD,
                     (size_t)nj * (size_t)np_local, planes);
  launched(0, "k_items_scatter_words8");
}
void launch_items_scatter_packed(u64* db, const u64* stage, const CopyQuadRec* quads, size_t n_quads, int np_local, int nj, int planes,
                                 hipStream_t s) {
  if (n_quads == 0) return;
  hipLaunchKernelGGL(k_items_scatter_packed, dim3((unsigned)((n_quads + 63) / 64), N / SCATTER_Z, planes), dim3(256), 0, s,
                     reinterpret_cast<u32*>(db), stage, quads, n_quads, np_local, nj, planes);
  launched(0, "k_items_scatter_packed");
}

}  // namespace spiral
