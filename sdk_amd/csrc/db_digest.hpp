// Database digest (sp_db_digest; the definition is beside DigestDesc in kernels.hpp): the kernels over the 8-byte words, the PACKED unit
// stream and a sparse store, and the call's first kernel (row keys, zeroed sums).  The digit-planar kernel is db_digest_planar.hpp.
//
// Every kernel reads each resident byte of its plane range once, with non-temporal loads, and does per word one multiply-add per lane
// by the ROW key (from LDS; wave-uniform in the PACKED kernel, which reads it with scalar loads); the column key, one mix, multiplies a thread's sum over its rows once per column.  A sparse store has one
// row and column per slot, so there the column key is per word and the row key per workgroup.  The workgroup's partial pair goes into
// the plane's sums with two atomic adds (digest_reduce).
// Included by db.hip only.
#pragma once
#include "db_digest_device.hpp"

namespace spiral {

typedef u32 dg_u32x4_t __attribute__((ext_vector_type(4)));
typedef u32 dg_u32x3_t __attribute__((ext_vector_type(3), aligned(4)));

// the call's first kernel: sums = 0, R[l][jl] = R_l(j0 + jl)
__global__ __launch_bounds__(256) void k_digest_keys(unsigned long long* sums, u64* R, u64 s0, u64 s1, int nplanes, int j0, int nj) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < 2 * nplanes) sums[t] = 0ULL;
  if (t < nj) {
    R[t] = digest_row_key(s0, (u64)(j0 + t));
    R[(size_t)nj + t] = digest_row_key(s1, (u64)(j0 + t));
  }
}
void launch_digest_keys(unsigned long long* sums, u64* R, u64 seed, int nplanes, int j0, int nj, hipStream_t s) {
  const int n = std::max(2 * nplanes, nj);
  hipLaunchKernelGGL(k_digest_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sums, R, digest_mix(seed), digest_mix(seed + 1),
                     nplanes, j0, nj);
  launched(0, "k_digest_keys");
}

// ---- 8-byte words [plane][z][jl][il]: a workgroup owns one (plane, z), a tile of at most 256 columns and a tile of at most DIGEST_ROWS
// rows.  Lanes run along il (a wave reads 512 contiguous bytes of a row, or whole rows where the handle has fewer than 64 columns);
// with fewer than 256 columns the workgroup's threads take 256 / columns rows at a time.  A thread keeps to ONE column.
// grid (column tiles * row tiles, N, planes of the range).  Also a column shard (cm) and a row shard with an odd row count.
__global__ __launch_bounds__(256) void k_digest_words8(DigestDesc d, const u64* db, int np_local, ColMap cm) {
  __shared__ DigestLds lds;
  const int col_tiles = (np_local + 255) >> 8;
  const int ct = (int)(blockIdx.x % (unsigned)col_tiles), jt0 = (int)(blockIdx.x / (unsigned)col_tiles) * DIGEST_ROWS;
  const int n = d.nj - jt0 < DIGEST_ROWS ? d.nj - jt0 : DIGEST_ROWS;
  const int plane = d.plane0 + (int)blockIdx.z;
  const size_t zp = (size_t)plane * N + blockIdx.y;
  digest_stage_rows(lds, d, jt0, n);
  const int cols = np_local < 256 ? np_local : 256, rstep = 256 / cols;
  const int il = ct * 256 + (int)(threadIdx.x % (unsigned)cols), r0 = (int)(threadIdx.x / (unsigned)cols);
  u64 a0 = 0, a1 = 0;
  if (il < np_local && r0 < rstep) {
    const u64* p = db + (zp * (size_t)d.nj + (size_t)jt0) * (size_t)np_local + (size_t)il;
#pragma unroll 4
    for (int jl = r0; jl < n; jl += rstep) {
      const u64 w = __builtin_nontemporal_load(p + (size_t)jl * (size_t)np_local);
      a0 += lds.R[0][jl] * w;
      a1 += lds.R[1][jl] * w;
    }
    const u64 c = (u64)zp * (u64)d.num_per + (u64)(cm.off + cm.stride * il);
    a0 *= digest_col_key(d.s[0], c);
    a1 *= digest_col_key(d.s[1], c);
  }
  digest_reduce(lds.part, d, plane, a0, a1);
}

// ---- PACKED: the unit stream as the sweep walks it.  A workgroup owns one (plane, z, 128-column chunk) and a tile of DIGEST_ROWS / 2 row
// pairs, contiguous units of 1792 bytes; wave v takes every fourth unit.  Lane l owns the local columns 128 chunk + 2 l and + 1: it reads
// its 16-byte and its 12-byte piece of a unit, 7 dwords for the 4 words (rows 2 jp, 2 jp + 1 of both columns).  A unit's row pair is
// the same for the whole wave, so its four row keys are read from the table in the read buffer with SCALAR loads (the wave index goes
// through readfirstlane): they cost no vector register and no LDS, and the registers go to the loads in flight -- four units per wave.
// grid (chunks * row tiles, N, planes of the range)
constexpr int DIGEST_PACKED_UNROLL = 4;
__global__ __launch_bounds__(256) void k_digest_packed(DigestDesc d, const u32* db, int np_local, ColMap cm) {
  __shared__ u64 part[2][DIGEST_WG];
  const int chunks = np_local >> 7, npairs = d.nj >> 1;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks), jp0 = (int)(blockIdx.x / (unsigned)chunks) * (DIGEST_ROWS / 2);
  const int np = npairs - jp0 < DIGEST_ROWS / 2 ? npairs - jp0 : DIGEST_ROWS / 2;
  const int plane = d.plane0 + (int)blockIdx.z;
  const size_t zp = (size_t)plane * N + blockIdx.y;
  const int lane = threadIdx.x & 63, wave = (int)__builtin_amdgcn_readfirstlane((u32)(threadIdx.x >> 6));
  const u32* unit0 = db + packed_unit_offset(zp, jp0, chunk, npairs, chunks);
  const u64* R0 = d.R + 2 * jp0;            // R_0 of the tile's rows
  const u64* R1 = R0 + (size_t)d.nj;        // R_1
  const u32 M = 0x0FFFFFFFu;
  u64 c0l0 = 0, c0l1 = 0, c1l0 = 0, c1l1 = 0;   // column b, digest lane l
#pragma unroll DIGEST_PACKED_UNROLL
  for (int jp = wave; jp < np; jp += 4) {
    const u32* unit = unit0 + (size_t)jp * 448;
    const dg_u32x4_t p4 = __builtin_nontemporal_load(reinterpret_cast<const dg_u32x4_t*>(unit + 4 * lane));
    const dg_u32x3_t p3 = __builtin_nontemporal_load(reinterpret_cast<const dg_u32x3_t*>(unit + 256 + 3 * lane));
    // the limbs f0 .. f7 of pack_unit_lane: lo / hi of (row 0, col 0), (row 0, col 1), (row 1, col 0), (row 1, col 1)
    const u64 w00 = (u64)(p4[0] & M) | ((u64)(((p4[0] >> 28) | (p4[1] << 4)) & M) << 32);
    const u64 w01 = (u64)(((p4[1] >> 24) | (p4[2] << 8)) & M) | ((u64)(((p4[2] >> 20) | (p4[3] << 12)) & M) << 32);
    const u64 w10 = (u64)(((p4[3] >> 16) | (p3[0] << 16)) & M) | ((u64)(((p3[0] >> 12) | (p3[1] << 20)) & M) << 32);
    const u64 w11 = (u64)(((p3[1] >> 8) | (p3[2] << 24)) & M) | ((u64)(p3[2] >> 4) << 32);
    const u64 r00 = R0[2 * jp], r01 = R0[2 * jp + 1], r10 = R1[2 * jp], r11 = R1[2 * jp + 1];   // R_l(row): wave-uniform
    c0l0 += r00 * w00 + r01 * w10;
    c1l0 += r00 * w01 + r01 * w11;
    c0l1 += r10 * w00 + r11 * w10;
    c1l1 += r10 * w01 + r11 * w11;
  }
  const int il = 128 * chunk + 2 * lane;
  const u64 k0 = (u64)zp * (u64)d.num_per + (u64)(cm.off + cm.stride * il), k1 = k0 + (u64)cm.stride;
  const u64 a0 = digest_col_key(d.s[0], k0) * c0l0 + digest_col_key(d.s[0], k1) * c1l0;
  const u64 a1 = digest_col_key(d.s[1], k0) * c0l1 + digest_col_key(d.s[1], k1) * c1l1;
  digest_reduce(part, d, plane, a0, a1);
}

void launch_digest_words(const DigestDesc& d, const u64* db, int np_local, int packed, ColMap cm, hipStream_t s) {
  if (d.nplanes <= 0 || d.nj <= 0 || np_local <= 0) return;
  const unsigned row_tiles = (unsigned)((d.nj + DIGEST_ROWS - 1) / DIGEST_ROWS);
  if (packed) {
    hipLaunchKernelGGL(k_digest_packed, dim3((unsigned)(np_local >> 7) * row_tiles, N, d.nplanes), dim3(256), 0, s, d,
                       reinterpret_cast<const u32*>(db), np_local, cm);
    launched(0, "k_digest_packed");
  } else {
    hipLaunchKernelGGL(k_digest_words8, dim3((unsigned)((np_local + 255) >> 8) * row_tiles, N, d.nplanes), dim3(256), 0, s, d, db, np_local,
                       cm);
    launched(0, "k_digest_words8");
  }
}

// ---- a sparse store [slot][planes][z], canonical words: a workgroup owns one (stored item, plane) -- 16 KiB, thread t the words
// z = t + 256 i.  The item's index gives row j and column ii: the column key varies per word, the row key is the workgroup's.
// grid (stored items, planes of the range)
__global__ __launch_bounds__(256) void k_digest_sparse(DigestDesc d, const u64* polys, int planes, const DigestSlotRec* list) {
  __shared__ u64 part[2][DIGEST_WG];
  const DigestSlotRec rec = list[blockIdx.x];
  const int plane = d.plane0 + (int)blockIdx.y;
  const u64 j = rec.item / (u64)d.num_per, ii = rec.item % (u64)d.num_per;
  const u64* p = polys + ((size_t)rec.slot * (size_t)planes + (size_t)plane) * N;
  u64 a0 = 0, a1 = 0;
#pragma unroll
  for (int i = 0; i < N / 256; i++) {
    const int z = (int)threadIdx.x + 256 * i;
    const u64 w = __builtin_nontemporal_load(p + z);
    const u64 c = ((u64)plane * N + (u64)z) * (u64)d.num_per + ii;
    a0 += digest_col_key(d.s[0], c) * w;
    a1 += digest_col_key(d.s[1], c) * w;
  }
  a0 *= digest_row_key(d.s[0], j);
  a1 *= digest_row_key(d.s[1], j);
  digest_reduce(part, d, plane, a0, a1);
}
void launch_digest_sparse(const DigestDesc& d, const u64* polys, int planes, const DigestSlotRec* list, size_t n, hipStream_t s) {
  if (n == 0 || d.nplanes <= 0) return;
  hipLaunchKernelGGL(k_digest_sparse, dim3((unsigned)n, d.nplanes), dim3(256), 0, s, d, polys, planes, list);
  launched(0, "k_digest_sparse");
}

}  // namespace spiral
