// Per-item digests (sp_db_item_digests; the definition is beside ItemDigestDesc in kernels.hpp): the kernels over the 8-byte words, the
// PACKED unit stream and a sparse store.  The digit-planar kernel is db_item_digest_planar.hpp.
//
// The keys of sp_db_digest with their roles reversed: the sum of an item runs over (plane, z), so the key that varies along the stream
// is the COLUMN key A_l(plane, z, ii), one mix each, and the row key multiplies an item's finished sum once.  A dense kernel therefore
// gives one thread one column (two in the PACKED kernel) and several rows: the column keys of a z are computed once and serve every row
// the thread holds, and per word there is one multiply-add per lane.  A workgroup walks ITEM_DIGEST_Z z-rows of one plane, keeps one
// pair of sums per row in registers, multiplies each by R_l(j) at the end and adds it into the window's table with 64-bit vector
// atomics: wrapping adds commute, so the order in which workgroups arrive does not change the value.  No dense kernel uses LDS.
// Every kernel reads each resident byte of its rows and planes once, with non-temporal loads.
// Included by db.hip only.
#pragma once
#include "db_digest.hpp"

namespace spiral {

// what a thread of a dense kernel adds at the end: its sum for (window row r, reference column col), both lanes
__device__ __forceinline__ void item_digest_add(const ItemDigestDesc& d, int r, int col, u64 a0, u64 a1) {
  unsigned long long* t = d.table + 2 * ((size_t)r * (size_t)d.num_per + (size_t)col);
  atomicAdd(t, (unsigned long long)(a0 * d.R[r]));
  atomicAdd(t + 1, (unsigned long long)(a1 * d.R[(size_t)d.nrows + r]));
}

// ---- 8-byte words [plane][z][jl][il]: a workgroup owns a tile of at most 256 columns x ITEM_DIGEST_ROWS rows of the window, one plane and
// ITEM_DIGEST_Z z-rows.  Lanes run along il; a thread keeps to ONE column and holds one pair of sums per row of the tile.  With fewer
// than 256 columns the workgroup's threads split the z-rows among them (256 / columns at a time).  Per z a thread computes its two
// column keys once; per word one multiply-add per lane.  Also a column shard (cm) and the one-row shard.
// grid (column tiles * row tiles, N / ITEM_DIGEST_Z, planes of the range)
constexpr int ITEM_DIGEST_ROWS = 8;
__global__ __launch_bounds__(256) void k_item_digest_words8(ItemDigestDesc d, const u64* db, int np_local, ColMap cm) {
  const int col_tiles = (np_local + 255) >> 8;
  const int ct = (int)(blockIdx.x % (unsigned)col_tiles), jt0 = (int)(blockIdx.x / (unsigned)col_tiles) * ITEM_DIGEST_ROWS;
  const int n = d.nrows - jt0 < ITEM_DIGEST_ROWS ? d.nrows - jt0 : ITEM_DIGEST_ROWS;
  const int plane = d.plane0 + (int)blockIdx.z;
  const int cols = np_local < 256 ? np_local : 256, zstep = 256 / cols;
  const int il = ct * 256 + (int)(threadIdx.x % (unsigned)cols), zs = (int)(threadIdx.x / (unsigned)cols);
  if (il >= np_local || zs >= zstep) return;
  const int col = cm.off + cm.stride * il;
  const int z0 = (int)blockIdx.y * ITEM_DIGEST_Z;
  u64 a0[ITEM_DIGEST_ROWS], a1[ITEM_DIGEST_ROWS];
#pragma unroll
  for (int r = 0; r < ITEM_DIGEST_ROWS; r++) a0[r] = a1[r] = 0;
#pragma unroll 1
  for (int z = z0 + zs; z < z0 + ITEM_DIGEST_Z; z += zstep) {
    const size_t zp = (size_t)plane * N + (size_t)z;
    const u64* p = db + (zp * (size_t)d.nj + (size_t)(d.jl0 + jt0)) * (size_t)np_local + (size_t)il;
    u64 w[ITEM_DIGEST_ROWS];
#pragma unroll
    for (int r = 0; r < ITEM_DIGEST_ROWS; r++) w[r] = r < n ? __builtin_nontemporal_load(p + (size_t)r * (size_t)np_local) : 0ULL;
    const u64 c = (u64)zp * (u64)d.num_per + (u64)col;
    const u64 k0 = digest_col_key(d.s[0], c), k1 = digest_col_key(d.s[1], c);
#pragma unroll
    for (int r = 0; r < ITEM_DIGEST_ROWS; r++) {
      a0[r] += k0 * w[r];
      a1[r] += k1 * w[r];
    }
  }
#pragma unroll
  for (int r = 0; r < ITEM_DIGEST_ROWS; r++)
    if (r < n) item_digest_add(d, jt0 + r, col, a0[r], a1[r]);
}

// ---- PACKED: units of consecutive row pairs of one (plane, z, chunk) are contiguous, 448 dwords apart.  A workgroup owns one 128-column
// chunk, 4 * ITEM_DIGEST_PAIRS row pairs of the window, one plane and ITEM_DIGEST_Z z-rows; wave v takes ITEM_DIGEST_PAIRS consecutive row
// pairs.  Lane l owns the local columns 128 chunk + 2 l and + 1 and, per unit, rows 2 jp and 2 jp + 1 of both (k_digest_packed's pieces
// and limbs): its four column keys of a z (two columns, two lanes) serve the whole group of row pairs.  A window that begins or ends
// inside a row pair reads that pair's units whole and leaves the other row's sums out.
// grid (chunks * pair tiles, N / ITEM_DIGEST_Z, planes of the range)
constexpr int ITEM_DIGEST_PAIRS = 4;
__global__ __launch_bounds__(256) void k_item_digest_packed(ItemDigestDesc d, const u32* db, int np_local, ColMap cm) {
  const int chunks = np_local >> 7, npairs = d.nj >> 1;
  const int jp_lo = d.jl0 >> 1, jp_end = ((d.jl0 + d.nrows - 1) >> 1) + 1;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const int lane = threadIdx.x & 63, wave = (int)__builtin_amdgcn_readfirstlane((u32)(threadIdx.x >> 6));
  const int jp0 = jp_lo + ((int)(blockIdx.x / (unsigned)chunks) * 4 + wave) * ITEM_DIGEST_PAIRS;
  const int np = jp_end - jp0 < ITEM_DIGEST_PAIRS ? jp_end - jp0 : ITEM_DIGEST_PAIRS;
  if (np <= 0) return;
  const int plane = d.plane0 + (int)blockIdx.z;
  const int z0 = (int)blockIdx.y * ITEM_DIGEST_Z;
  const int il = 128 * chunk + 2 * lane;
  const int col0 = cm.off + cm.stride * il, col1 = col0 + cm.stride;
  const u32 M = 0x0FFFFFFFu;
  u64 acc[ITEM_DIGEST_PAIRS][4][2];   // [row pair][word: row a * 2 + column b][digest lane]
#pragma unroll
  for (int g = 0; g < ITEM_DIGEST_PAIRS; g++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[g][q][0] = acc[g][q][1] = 0;
#pragma unroll 1
  for (int z = z0; z < z0 + ITEM_DIGEST_Z; z++) {
    const size_t zp = (size_t)plane * N + (size_t)z;
    const u32* unit0 = db + packed_unit_offset(zp, jp0, chunk, npairs, chunks);
    dg_u32x4_t p4[ITEM_DIGEST_PAIRS];
    dg_u32x3_t p3[ITEM_DIGEST_PAIRS];
#pragma unroll
    for (int g = 0; g < ITEM_DIGEST_PAIRS; g++) {
      if (g < np) {
        p4[g] = __builtin_nontemporal_load(reinterpret_cast<const dg_u32x4_t*>(unit0 + (size_t)g * 448 + 4 * lane));
        p3[g] = __builtin_nontemporal_load(reinterpret_cast<const dg_u32x3_t*>(unit0 + (size_t)g * 448 + 256 + 3 * lane));
      } else {
        p4[g] = dg_u32x4_t{0u, 0u, 0u, 0u};
        p3[g] = dg_u32x3_t{0u, 0u, 0u};
      }
    }
    const u64 c0 = (u64)zp * (u64)d.num_per + (u64)col0, c1 = (u64)zp * (u64)d.num_per + (u64)col1;
    const u64 k00 = digest_col_key(d.s[0], c0), k01 = digest_col_key(d.s[1], c0);   // k{column}{lane}
    const u64 k10 = digest_col_key(d.s[0], c1), k11 = digest_col_key(d.s[1], c1);
#pragma unroll
    for (int g = 0; g < ITEM_DIGEST_PAIRS; g++) {
      // the limbs f0 .. f7 of pack_unit_lane: lo / hi of (row 0, col 0), (row 0, col 1), (row 1, col 0), (row 1, col 1)
      const dg_u32x4_t a = p4[g];
      const dg_u32x3_t b = p3[g];
      const u64 w00 = (u64)(a[0] & M) | ((u64)(((a[0] >> 28) | (a[1] << 4)) & M) << 32);
      const u64 w01 = (u64)(((a[1] >> 24) | (a[2] << 8)) & M) | ((u64)(((a[2] >> 20) | (a[3] << 12)) & M) << 32);
      const u64 w10 = (u64)(((a[3] >> 16) | (b[0] << 16)) & M) | ((u64)(((b[0] >> 12) | (b[1] << 20)) & M) << 32);
      const u64 w11 = (u64)(((b[1] >> 8) | (b[2] << 24)) & M) | ((u64)(b[2] >> 4) << 32);
      acc[g][0][0] += k00 * w00;
      acc[g][0][1] += k01 * w00;
      acc[g][1][0] += k10 * w01;
      acc[g][1][1] += k11 * w01;
      acc[g][2][0] += k00 * w10;
      acc[g][2][1] += k01 * w10;
      acc[g][3][0] += k10 * w11;
      acc[g][3][1] += k11 * w11;
    }
  }
#pragma unroll
  for (int g = 0; g < ITEM_DIGEST_PAIRS; g++) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
      const int r = 2 * (jp0 + g) + a - d.jl0;   // the row within the window
      if (g < np && r >= 0 && r < d.nrows) {
        item_digest_add(d, r, col0, acc[g][2 * a][0], acc[g][2 * a][1]);
        item_digest_add(d, r, col1, acc[g][2 * a + 1][0], acc[g][2 * a + 1][1]);
      }
    }
  }
}

void launch_item_digest_words(const ItemDigestDesc& d, const u64* db, int np_local, int packed, ColMap cm, hipStream_t s) {
  if (d.nplanes <= 0 || d.nrows <= 0 || np_local <= 0) return;
  if (packed) {
    const int pairs = ((d.jl0 + d.nrows - 1) >> 1) - (d.jl0 >> 1) + 1, per_wg = 4 * ITEM_DIGEST_PAIRS;
    hipLaunchKernelGGL(k_item_digest_packed, dim3((unsigned)(np_local >> 7) * (unsigned)((pairs + per_wg - 1) / per_wg), N / ITEM_DIGEST_Z,
                                                  d.nplanes),
                       dim3(256), 0, s, d, reinterpret_cast<const u32*>(db), np_local, cm);
    launched(0, "k_item_digest_packed");
  } else {
    const unsigned row_tiles = (unsigned)((d.nrows + ITEM_DIGEST_ROWS - 1) / ITEM_DIGEST_ROWS);
    hipLaunchKernelGGL(k_item_digest_words8, dim3((unsigned)((np_local + 255) >> 8) * row_tiles, N / ITEM_DIGEST_Z, d.nplanes), dim3(256), 0,
                       s, d, db, np_local, cm);
    launched(0, "k_item_digest_words8");
  }
}

// ---- a sparse store [slot][planes][z], canonical words: one workgroup per stored item of the window, over the planes of the range;
// thread t takes the words z = t + 256 i of each plane.  The column key varies per word here by construction.  The workgroup's 256
// pairs are summed through LDS, multiplied by the item's row keys and WRITTEN (no atomics: an item has one workgroup), with the item's
// present flag, at the item's place in the window.
// grid (stored items of the window)
__global__ __launch_bounds__(256) void k_item_digest_sparse(ItemDigestDesc d, const u64* polys, int planes, const DigestSlotRec* list,
                                                            unsigned long long item_base, uint8_t* present) {
  __shared__ u64 part[2][DIGEST_WG];
  const DigestSlotRec rec = list[blockIdx.x];
  const u64 j = rec.item / (u64)d.num_per, ii = rec.item % (u64)d.num_per;
  const int t = threadIdx.x;
  u64 a0 = 0, a1 = 0;
#pragma unroll 1
  for (int plane = d.plane0; plane < d.plane0 + d.nplanes; plane++) {
    const u64* p = polys + ((size_t)rec.slot * (size_t)planes + (size_t)plane) * N;
#pragma unroll 4
    for (int i = 0; i < N / 256; i++) {
      const int z = t + 256 * i;
      const u64 w = __builtin_nontemporal_load(p + z);
      const u64 c = ((u64)plane * N + (u64)z) * (u64)d.num_per + ii;
      a0 += digest_col_key(d.s[0], c) * w;
      a1 += digest_col_key(d.s[1], c) * w;
    }
  }
  part[0][t] = a0;
  part[1][t] = a1;
  __syncthreads();
#pragma unroll
  for (int h = DIGEST_WG / 2; h >= 1; h >>= 1) {
    if (t < h) {
      part[0][t] += part[0][t + h];
      part[1][t] += part[1][t + h];
    }
    __syncthreads();
  }
  const size_t pos = (size_t)(rec.item - item_base);
  if (t < 2) d.table[2 * pos + t] = (unsigned long long)(part[t][0] * digest_row_key(d.s[t], j));
  if (t == 2) present[pos] = 1;
}
void launch_item_digest_sparse(const ItemDigestDesc& d, const u64* polys, int planes, const DigestSlotRec* list, size_t n,
                               unsigned long long item_base, uint8_t* present, hipStream_t s) {
  if (n == 0 || d.nplanes <= 0) return;
  hipLaunchKernelGGL(k_item_digest_sparse, dim3((unsigned)n), dim3(256), 0, s, d, polys, planes, list, item_base, present);
  launched(0, "k_item_digest_sparse");
}

}  // namespace spiral
