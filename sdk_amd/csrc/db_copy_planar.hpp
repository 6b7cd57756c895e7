// sp_db_copy_items, the digit-planar writer: item-major words stage[index][plane][z] (db_copy.hpp) -> the entries of a planar-resident
// handle or planar row shard.  The inverse of k_planar_gather (planar_resident.hpp); the column order of a shard is applied by
// planar_entry_of, as for every writer of that file.
//
// A word is one byte in each of the 8 entries (modulus c, digit a) of its column's 16-row group, and an entry is 16 rows' bytes: ONE
// THREAD owns a (16-row group, column) CELL of one (plane, z) and rewrites its 8 sixteen-byte entries.  Rows of the cell that the call
// does not write (src < 0) keep their digit bytes: the resident entry is read and the written rows' bytes are replaced in it; a cell
// with all 16 rows listed is stored without a read.  The host lists a cell once per launch, in the resident order of the columns, so 16
// neighbours of the list are the 16 lanes of one tile's operand (256 contiguous bytes per entry) wherever whole rows are copied.
// A workgroup takes 16 listed cells for 16 z-rows of one plane; the cells' 256 words get there through the gather's tile, read as
// 128-byte z-runs of the stage.  grid (ceil(n_cells / 16), N / 16, planes).  Plain vector loads and stores only.
// Included by sweep_planar.hip only (after planar_resident.hpp).
#pragma once
#include "planar_resident.hpp"

namespace spiral {

__global__ __launch_bounds__(256) void k_planar_scatter_items(unsigned char* planar, const u64* stage, const CopyCellRec* cells,
                                                              size_t n_cells, int num_per, int nj, int planes, PlanarCols pc) {
  __shared__ u64 tile[256][PLANAR_GATHER_Z + 1];
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const size_t c0 = (size_t)blockIdx.x * 16;
  const int plane = blockIdx.z, z0 = blockIdx.y * PLANAR_GATHER_Z;
  {
    const int zl = threadIdx.x & (PLANAR_GATHER_Z - 1);
#pragma unroll 1
    for (int pass = 0; pass < 16; pass++) {
      const int u = pass * 16 + (threadIdx.x >> 4);   // tile row: row t = u >> 4 of the group, cell n = u & 15 of the workgroup
      const size_t k = c0 + (size_t)(u & 15);
      const int s = k < n_cells ? cells[k].src[u >> 4] : -1;
      if (s >= 0) tile[u][zl] = stage[((size_t)s * planes + plane) * N + z0 + zl];
    }
  }
  __syncthreads();
  const int n = threadIdx.x & 15, zl = threadIdx.x >> 4;
  if (c0 + (size_t)n >= n_cells) return;   // (after the only barrier)
  const CopyCellRec* cell = cells + c0 + (size_t)n;
  const int j = cell->j, ii = cell->ii;
  u32 mask = 0;
#pragma unroll
  for (int t = 0; t < 16; t++) mask |= (u32)(cell->src[t] >= 0) << t;
  const size_t zp = (size_t)plane * N + (size_t)(z0 + zl);
  mf_u32x4_t* out = reinterpret_cast<mf_u32x4_t*>(planar);
#pragma unroll
  for (int c = 0; c < 2; c++) {
    u32 od[16];
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const u64 w = (mask >> t) & 1u ? tile[16 * t + n][zl] : 0ull;
      od[t] = offset_digits(c ? (u32)(w >> 32) : (u32)w);
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const size_t idx = planar_entry_of(zp, j, ii, c, a, chunks, blocks, pc);
      mf_u32x4_t o = {0u, 0u, 0u, 0u};
      if (mask != 0xffffu) o = out[idx];
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const u32 sh = 8 * (t & 3);
        if ((mask >> t) & 1u) o[t >> 2] = (o[t >> 2] & ~(0xffu << sh)) | (((od[t] >> (8 * a)) & 0xffu) << sh);
      }
      out[idx] = o;
    }
  }
}

}  // namespace spiral
