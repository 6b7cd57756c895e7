// Database digest (sp_db_digest; kernels.hpp has the definition) over digit-planar words: a planar-resident handle, a planar row shard
// and the batch copy beside a PACKED database are this one kernel.  The shape and the column order come through planar_group_at /
// planar_entry_of (planar_resident.hpp) and nowhere else.
// Included by sweep_planar.hip only.
#pragma once
#include "db_digest_device.hpp"
#include "planar_resident.hpp"

namespace spiral {

// A thread owns one column's 16-row group at a time, in planar_group_at's order: a wave's 64 threads are the 64 lanes of one operand, so
// each of its 8 loads (modulus c, digit a) is one contiguous KiB of whole 16-byte entries.  The 16 words are put together from their
// digit bytes (the 0x80 offsets taken off: an empty database, every byte 0x80, sums to 0), multiplied by the rows' keys from LDS, and the
// group's sum by the column key.  grid (workgroups per plane, planes of the range); nj <= 512 <= DIGEST_ROWS on every planar shape.
__global__ __launch_bounds__(256) void k_digest_planar(DigestDesc d, const unsigned char* planar, PlanarCols pc) {
  __shared__ DigestLds lds;
  const int chunks = d.num_per >> 7, blocks = d.nj >> 6;
  const int plane = d.plane0 + (int)blockIdx.y;
  digest_stage_rows(lds, d, 0, d.nj);
  const size_t total = (size_t)N * (size_t)d.num_per * (size_t)(d.nj >> 4);
  const mf_u32x4_t* in = reinterpret_cast<const mf_u32x4_t*>(planar);
  u64 a0 = 0, a1 = 0;
#pragma unroll 1
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const PlanarGroupAt p = planar_group_at(idx, chunks, blocks, pc);
    const size_t zp = (size_t)plane * N + p.zl;
    u32 limb[2][16];
#pragma unroll
    for (int c = 0; c < 2; c++) {
      mf_u32x4_t o[4];
#pragma unroll
      for (int a = 0; a < 4; a++) o[a] = __builtin_nontemporal_load(in + planar_entry_of(zp, 16 * p.jg, p.ii, c, a, chunks, blocks, pc));
#pragma unroll
      for (int t = 0; t < 16; t++) {
        u32 x = 0;
#pragma unroll
        for (int a = 0; a < 4; a++) x |= ((o[a][t >> 2] >> (8 * (t & 3))) & 0xffu) << (8 * a);
        limb[c][t] = offset_digits(x);
      }
    }
    u64 g0 = 0, g1 = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const u64 w = (u64)limb[0][t] | ((u64)limb[1][t] << 32);
      g0 += lds.R[0][16 * p.jg + t] * w;
      g1 += lds.R[1][16 * p.jg + t] * w;
    }
    const u64 c = (u64)zp * (u64)d.num_per + (u64)p.ii;
    a0 += digest_col_key(d.s[0], c) * g0;
    a1 += digest_col_key(d.s[1], c) * g1;
  }
  digest_reduce(lds.part, d, plane, a0, a1);
}

}  // namespace spiral
