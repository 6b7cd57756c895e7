// Per-item digests (sp_db_item_digests; kernels.hpp has the definition) over digit-planar words: a planar-resident handle, a planar row
// shard and the batch copy beside a PACKED database are this one kernel.  The shape and the column order come through planar_entry_of /
// planar_col_ref (planar_resident.hpp) and nowhere else.
// Included by sweep_planar.hip only.
#pragma once
#include "db_digest_device.hpp"
#include "planar_resident.hpp"

namespace spiral {

typedef u32 idg_u32x2_t __attribute__((ext_vector_type(2)));

// A thread owns HALF of one column's 16-row group -- 8 rows, the low or the high 8 bytes of the group's 8 entries (modulus c, digit a) --
// for ITEM_DIGEST_Z z-rows of one plane: threads walk [chunk][g][block][e][lane = 16 kb + n][half] as k_digest_planar walks
// [chunk][g][block][e][lane], so a wave's 8-byte loads are 512 contiguous bytes of one operand.  The 8 words are put together from their
// digit bytes (the 0x80 offsets taken off), the thread's two column keys of the z serve all 8, and the 8 pairs of sums stay in
// registers until the z-rows are done; then each is multiplied by its row key and added into the window's table.  Only the 64-row
// blocks the window touches are walked, and a thread whose 8 rows lie outside the window loads nothing.
// grid (threads of the window's blocks / 256, N / ITEM_DIGEST_Z, planes of the range)
__global__ __launch_bounds__(256) void k_item_digest_planar(ItemDigestDesc d, const unsigned char* planar, PlanarCols pc) {
  const int chunks = d.num_per >> 7, blocks = d.nj >> 6;
  const int blk_lo = d.jl0 >> 6, nblk = ((d.jl0 + d.nrows - 1) >> 6) - blk_lo + 1;
  size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int half = (int)(r & 1), lane = (int)((r >> 1) & 63);
  r >>= 7;
  const int e = (int)(r & 1);
  r >>= 1;
  const int block = blk_lo + (int)(r % (size_t)nblk);
  r /= (size_t)nblk;
  const int g = (int)(r & 3);
  r >>= 2;
  if (r >= (size_t)chunks) return;
  const int chunk = (int)r;
  const int jg = 4 * block + (lane >> 4), row0 = 16 * jg + 8 * half - d.jl0;   // the thread's first row within the window
  if (row0 + 8 <= 0 || row0 >= d.nrows) return;
  const int ii = planar_col_ref(128 * chunk + 2 * (16 * g + (lane & 15)) + e, pc);
  const int plane = d.plane0 + (int)blockIdx.z;
  const size_t zp0 = (size_t)plane * N + (size_t)blockIdx.y * ITEM_DIGEST_Z;
  // the thread's 8 bytes of entry (zp, c, a): in units of 8 bytes, 2 * entry + half; one z-row further is z_stride on
  const idg_u32x2_t* in = reinterpret_cast<const idg_u32x2_t*>(planar);
  size_t at[2][4];
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int a = 0; a < 4; a++) at[c][a] = 2 * planar_entry_of(zp0, 16 * jg, ii, c, a, chunks, blocks, pc) + (size_t)half;
  const size_t z_stride = planar_operand_offset(1, 0, 0, 0, 0, 0, 0, chunks, blocks) / 8;
  u64 a0[8], a1[8];
#pragma unroll
  for (int t = 0; t < 8; t++) a0[t] = a1[t] = 0;
#pragma unroll 1
  for (int zl = 0; zl < ITEM_DIGEST_Z; zl++) {
    idg_u32x2_t o[2][4];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int a = 0; a < 4; a++) o[c][a] = __builtin_nontemporal_load(in + at[c][a] + (size_t)zl * z_stride);
    const u64 ck = (u64)(zp0 + (size_t)zl) * (u64)d.num_per + (u64)ii;
    const u64 k0 = digest_col_key(d.s[0], ck), k1 = digest_col_key(d.s[1], ck);
#pragma unroll
    for (int t = 0; t < 8; t++) {
      u32 x[2];
#pragma unroll
      for (int c = 0; c < 2; c++) {
        x[c] = 0;
#pragma unroll
        for (int a = 0; a < 4; a++) x[c] |= ((o[c][a][t >> 2] >> (8 * (t & 3))) & 0xffu) << (8 * a);
      }
      const u64 w = (u64)offset_digits(x[0]) | ((u64)offset_digits(x[1]) << 32);
      a0[t] += k0 * w;
      a1[t] += k1 * w;
    }
  }
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int rw = row0 + t;
    if (rw >= 0 && rw < d.nrows) {
      unsigned long long* tb = d.table + 2 * ((size_t)rw * (size_t)d.num_per + (size_t)ii);
      atomicAdd(tb, (unsigned long long)(a0[t] * d.R[rw]));
      atomicAdd(tb + 1, (unsigned long long)(a1[t] * d.R[(size_t)d.nrows + rw]));
    }
  }
}

}  // namespace spiral
