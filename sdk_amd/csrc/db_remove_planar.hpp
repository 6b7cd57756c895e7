// sp_db_remove_items, the digit-planar writer: the 8 digit bytes of every word of a removed item become 0x80, the empty database's byte
// (the offset digit of 0), in the entries of a planar-resident handle, a planar row shard, or the batch copy beside a PACKED handle.
// The column order of a shard is applied by planar_entry_of, as for every writer of planar_resident.hpp.
//
// Ownership is that of k_planar_scatter_items (db_copy_planar.hpp): ONE THREAD owns a (16-row group, column) CELL of one (plane, z) and
// rewrites its 8 sixteen-byte entries.  Rows of the cell the call does not remove keep their bytes: the resident entry is read and the
// removed rows' bytes are replaced in it; a cell that loses all 16 rows is stored without a read.  The host lists a cell once per launch.
// A workgroup takes 16 listed cells for 16 z-rows of one plane.  grid (ceil(n_cells / 16), N / 16, planes).
// Plain vector loads and stores only.  Included by sweep_planar.hip only (after planar_resident.hpp).
#pragma once
#include "planar_resident.hpp"

namespace spiral {

constexpr int PLANAR_CLEAR_Z = 16;
__global__ __launch_bounds__(256) void k_planar_clear_items(unsigned char* planar, const RemoveCellRec* cells, size_t n_cells, int num_per,
                                                            int nj, PlanarCols pc) {
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const size_t k = (size_t)blockIdx.x * 16 + (size_t)(threadIdx.x & 15);
  if (k >= n_cells) return;
  const RemoveCellRec cell = cells[k];
  const int plane = blockIdx.z, z = blockIdx.y * PLANAR_CLEAR_Z + (threadIdx.x >> 4);
  const size_t zp = (size_t)plane * N + (size_t)z;
  // byte t of an entry is row t of the cell: the bytes of the removed rows, per dword of the entry
  u32 bytes[4];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    u32 b = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) b |= (cell.mask >> (4 * w + t)) & 1u ? 0xffu << (8 * t) : 0u;
    bytes[w] = b;
  }
  mf_u32x4_t* out = reinterpret_cast<mf_u32x4_t*>(planar);
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const size_t idx = planar_entry_of(zp, cell.j, cell.ii, c, a, chunks, blocks, pc);
      mf_u32x4_t o = {0u, 0u, 0u, 0u};
      if ((cell.mask & 0xffffu) != 0xffffu) o = out[idx];
#pragma unroll
      for (int w = 0; w < 4; w++) o[w] = (o[w] & ~bytes[w]) | (0x80808080u & bytes[w]);
      out[idx] = o;
    }
}

}  // namespace spiral
