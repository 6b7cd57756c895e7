// Writers and the read-back of a PLANAR-RESIDENT database (sp_db_create_planar): a handle whose only resident form is the
// digit-planar layout of sweep_planar.hpp, [plane][z][chunk][g][c][block][e][a][lane = 16 kb + n][16 bytes], 8 bytes per word and no
// PACKED words behind it.  Byte t of entry (zp, chunk, g, c, block, e, a, lane) is the offset digit
//     ((x_c(row 64 block + 16 kb + t, column 128 chunk + 2 (16 g + n) + e) >> 8 a) & 0xff) ^ 0x80,
// so a word (row j, column ii) of (plane, z) is ONE BYTE in each of the 8 entries (modulus c, digit a) of its column's 16-row group,
// and the all-zero database is every byte 0x80.
//
// Every writer works from the handle's upload buffer (words staged there in the reference order or in the 8-byte layout the item
// encoders of db.hip write) and stores straight to the planar positions:
//   * whole 16-row groups of a column (bulk loaders, the synthetic fill): one thread gathers the group's 16 words and stores its 8
//     entries whole;
//   * single items (upserts): one thread per (item, plane, z) stores the word's 8 digit bytes with BYTE stores -- two items of one
//     16-row group, or the two columns of a lane slot, share entries or cache lines but never a byte, and the caller lists an item
//     once, so no byte has two writers and nothing is read back, merged or exchanged atomically.
//
// A planar ROW SHARD (sp_db_create_planar_shard: shard s of G) holds the rows j0 .. j0 + nj - 1 of every column, and holds its columns
// in the order the exchange wants them: reference column ii is RESIDENT column
//     ii' = (ii % G) * (num_per / G) + ii / G                                                    (planar_col; PlanarCols = the two logs)
// so that the columns of one destination rank (a residue class mod G) are one contiguous run and the pass stores its output to the
// reduce-scatter layout in the same 128-byte runs as to the plain one (k_sweep_planar_scatter).  Everything above holds with "column"
// read as "resident column"; an unsharded handle is G = 1, ii' = ii.  The permutation is applied HERE and nowhere else: planar_entry_of
// takes reference columns, planar_group_at hands out reference columns.  The loaders are given full-dim0 rows and keep the window.
// Its own header, instantiated in sweep_planar.hip only: sweep.hip's kernels keep their machine code.
#pragma once
#include "sweep_planar.hpp"

namespace spiral {

// column order of a handle: lgG = log2 G, lg_npg = log2(num_per / G); {0, anything} is the identity
struct PlanarCols {
  int lgG, lg_npg;
};
__host__ __device__ __forceinline__ int planar_col(int ii, PlanarCols pc) {       // reference -> resident
  return ((ii & ((1 << pc.lgG) - 1)) << pc.lg_npg) | (ii >> pc.lgG);
}
__host__ __device__ __forceinline__ int planar_col_ref(int ic, PlanarCols pc) {   // resident -> reference
  return pc.lgG == 0 ? ic : ((ic & ((1 << pc.lg_npg) - 1)) << pc.lgG) | (ic >> pc.lg_npg);
}
// rows of the reference a handle holds: local row j is row j0 + j of dim0
struct PlanarRows {
  int dim0, j0;
};

// entry index (16-byte units) of (zp, local row j, reference column ii_ref, modulus c, digit a); byte j & 15 of it is the word's digit
__host__ __device__ __forceinline__ size_t planar_entry_of(size_t zp, int j, int ii_ref, int c, int a, int chunks, int blocks, PlanarCols pc) {
  const int ii = planar_col(ii_ref, pc);
  const int chunk = ii >> 7, col = ii & 127, slot = col >> 1, e = col & 1, g = slot >> 4, n = slot & 15;
  const int block = j >> 6, kb = (j & 63) >> 4;
  return planar_operand_offset(zp, chunk, g, block, e, c, a, chunks, blocks) / 16 + (size_t)(16 * kb + n);
}

// the 8 entries of one column's 16-row group from its 16 canonical words w[t] = row 16 jg + t
__device__ __forceinline__ void planar_store_group(unsigned char* planar, size_t zp, int jg, int ii, const u64 (&w)[16], int chunks,
                                                   int blocks, PlanarCols pc) {
  mf_u32x4_t* out = reinterpret_cast<mf_u32x4_t*>(planar);
#pragma unroll
  for (int c = 0; c < 2; c++) {
    u32 od[16];
#pragma unroll
    for (int t = 0; t < 16; t++) od[t] = offset_digits(c ? (u32)(w[t] >> 32) : (u32)w[t]);
#pragma unroll
    for (int a = 0; a < 4; a++) {
      mf_u32x4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int t = 0; t < 16; t++) o[t >> 2] |= ((od[t] >> (8 * a)) & 0xffu) << (8 * (t & 3));
      out[planar_entry_of(zp, 16 * jg, ii, c, a, chunks, blocks, pc)] = o;
    }
  }
}

// (16-row group, column) pairs of `nzp` z-rows in the order that makes a wave's 64 threads the 64 lanes of one operand: thread index
// -> [zl][chunk][g][block][e][lane = 16 kb + n] over RESIDENT columns; ii = the reference column that lives there
struct PlanarGroupAt {
  size_t zl;
  int jg, ii;
};
__device__ __forceinline__ PlanarGroupAt planar_group_at(size_t idx, int chunks, int blocks, PlanarCols pc) {
  const int lane = (int)(idx & 63);
  size_t r = idx >> 6;
  const int e = (int)(r & 1);
  r >>= 1;
  const int block = (int)(r % (size_t)blocks);
  r /= (size_t)blocks;
  const int g = (int)(r & 3);
  r >>= 2;
  const int chunk = (int)(r % (size_t)chunks);
  PlanarGroupAt p;
  p.zl = r / (size_t)chunks;
  p.jg = 4 * block + (lane >> 4);
  p.ii = planar_col_ref(128 * chunk + 2 * (16 * g + (lane & 15)) + e, pc);
  return p;
}

// sp_db_load_plane: `nz` z-rows of reference words src[zl][ii][dim0] (staged in the upload buffer) -> the entries of z-rows zp0 ..,
// rows rw.j0 .. rw.j0 + nj - 1 of them; both limbs reduced as the PACKED loader reduces them (canon_word)
__global__ __launch_bounds__(256) void k_planar_from_ref(unsigned char* planar, const u64* src, size_t zp0, int nz, int num_per, int nj,
                                                         PlanarRows rw, PlanarCols pc) {
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const size_t total = (size_t)nz * (size_t)num_per * (size_t)(nj >> 4);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const PlanarGroupAt p = planar_group_at(idx, chunks, blocks, pc);
    const u64* s = src + (p.zl * (size_t)num_per + (size_t)p.ii) * (size_t)rw.dim0 + (size_t)(rw.j0 + 16 * p.jg);
    u64 w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) w[t] = canon_word(s[t]);
    planar_store_group(planar, zp0 + p.zl, p.jg, p.ii, w, chunks, blocks, pc);
  }
}

// sp_db_fill_synthetic: word (zp, ii, j) = sp_synth_word(seed, (zp * num_per + ii) * dim0 + j0 + j), the reference index
__global__ __launch_bounds__(256) void k_planar_synth(unsigned char* planar, u64 seed, size_t zps, int num_per, int nj, PlanarRows rw,
                                                      PlanarCols pc) {
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const size_t total = zps * (size_t)num_per * (size_t)(nj >> 4);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const PlanarGroupAt p = planar_group_at(idx, chunks, blocks, pc);
    const u64 ref0 = ((u64)p.zl * (u64)num_per + (u64)p.ii) * (u64)rw.dim0 + (u64)(rw.j0 + 16 * p.jg);
    u64 w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) w[t] = synth_word(seed, ref0 + (u64)t);
    planar_store_group(planar, p.zl, p.jg, p.ii, w, chunks, blocks, pc);
  }
}

// sp_db_load_items: k_db_encode has written the 16-row group jg of the columns ii0 .. ii0 + ncols - 1 as 8-byte words
// stage[zp][16][ncols]; one thread per (zp, column)
__global__ __launch_bounds__(256) void k_planar_from_stage(unsigned char* planar, const u64* stage, size_t zps, int jg, int ii0, int ncols,
                                                           int num_per, int nj, PlanarCols pc) {
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const size_t total = zps * (size_t)ncols;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int il = (int)(idx % (size_t)ncols);
    const size_t zp = idx / (size_t)ncols;
    const u64* s = stage + zp * 16 * (size_t)ncols + (size_t)il;
    u64 w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) w[t] = s[(size_t)t * (size_t)ncols];
    planar_store_group(planar, zp, jg, ii0 + il, w, chunks, blocks, pc);
  }
}

// Upserts: k_db_encode_quads has written item r of the window as 8-byte words stage[zp][(r >> 1) & 1][np_s] at column
// 2 (r >> 2) + (r & 1) (the 8-byte layout of a database of two rows and np_s columns: item r is entry r & 3 of quad r >> 2);
// cells[r] = its (local row, local column).  One thread per (item, zp): 8 byte stores.
__host__ __device__ __forceinline__ size_t planar_stage_item_word(size_t zp, size_t r, size_t np_s) {
  return (zp * 2 + ((r >> 1) & 1)) * np_s + 2 * (r >> 2) + (r & 1);
}
__global__ __launch_bounds__(256) void k_planar_put_items(unsigned char* planar, const u64* stage, size_t zps, size_t np_s,
                                                          const PlanarPatchCell* cells, size_t n_items, int num_per, int nj,
                                                          PlanarCols pc) {
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_items * zps) return;
  const size_t r = t / zps, zp = t % zps;
  const PlanarPatchCell cell = cells[r];
  const u64 w = stage[planar_stage_item_word(zp, r, np_s)];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const u32 od = offset_digits(c ? (u32)(w >> 32) : (u32)w);
#pragma unroll
    for (int a = 0; a < 4; a++)
      planar[planar_entry_of(zp, cell.j, cell.ii, c, a, chunks, blocks, pc) * 16 + (size_t)(cell.j & 15)] = (unsigned char)(od >> (8 * a));
  }
}

// sp_db_read_ref: the canonical words lo28 | hi28 << 32 of (zp, column ii, rows jl0 .. jl0 + count - 1) from their digit bytes
__global__ __launch_bounds__(64) void k_planar_read(u64* out, const unsigned char* planar, size_t zp, int ii, int jl0, int count,
                                                    int num_per, int nj, PlanarCols pc) {
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= count) return;
  const int j = jl0 + t;
  u64 w = 0;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    u32 od = 0;
#pragma unroll
    for (int a = 0; a < 4; a++)
      od |= (u32)planar[planar_entry_of(zp, j, ii, c, a, chunks, blocks, pc) * 16 + (size_t)(j & 15)] << (8 * a);
    w |= (u64)offset_digits(od) << (32 * c);
  }
  out[t] = w;
}

// sp_db_read_items, step 1 (item_readback.hpp): the words of the local items L0 .. L0 + nL - 1 (L = local row * num_per + REFERENCE column)
// -> dst[L - L0][plane][z].  A workgroup owns one 16-row group of one tile's 16 resident columns -- (chunk, g, e, block, kb): 256 items --
// for 16 z-rows of one plane: thread (z, n) reads its lane's 16 bytes of the 8 operands (modulus c, digit a), 256 contiguous bytes per
// operand and 16 lanes, and has the 16 rows' words of column n; the items get their 128-byte z-runs from an LDS tile.
// grid (n_rowgroups * num_per / 16, N / 16, planes); rg_lo = the first 16-row group the run touches
constexpr int PLANAR_GATHER_Z = 16;
__global__ __launch_bounds__(256) void k_planar_gather(u64* dst, const unsigned char* planar, size_t L0, size_t nL, int rg_lo, int num_per,
                                                       int nj, int planes, PlanarCols pc) {
  __shared__ u64 tile[256][PLANAR_GATHER_Z + 1];
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const int cge = (int)(blockIdx.x % (unsigned)(chunks * 8)), rg = rg_lo + (int)(blockIdx.x / (unsigned)(chunks * 8));
  const int e = cge & 1, g = (cge >> 1) & 3, chunk = cge >> 3;
  const int block = rg >> 2, kb = rg & 3;
  const int plane = blockIdx.z, z0 = blockIdx.y * PLANAR_GATHER_Z;
  {
    const int n = threadIdx.x & 15, zl = threadIdx.x >> 4;
    const size_t zp = (size_t)plane * N + (size_t)(z0 + zl);
    const mf_u32x4_t* in = reinterpret_cast<const mf_u32x4_t*>(planar);
    u32 limb[2][16];
#pragma unroll
    for (int c = 0; c < 2; c++) {
#pragma unroll
      for (int t = 0; t < 16; t++) limb[c][t] = 0;
#pragma unroll
      for (int a = 0; a < 4; a++) {
        const mf_u32x4_t o = in[planar_operand_offset(zp, chunk, g, block, e, c, a, chunks, blocks) / 16 + (size_t)(16 * kb + n)];
#pragma unroll
        for (int t = 0; t < 16; t++) limb[c][t] |= ((o[t >> 2] >> (8 * (t & 3))) & 0xffu) << (8 * a);
      }
    }
#pragma unroll
    for (int t = 0; t < 16; t++) tile[16 * t + n][zl] = (u64)offset_digits(limb[0][t]) | ((u64)offset_digits(limb[1][t]) << 32);
  }
  __syncthreads();
  const int zl = threadIdx.x & (PLANAR_GATHER_Z - 1);
#pragma unroll 1
  for (int pass = 0; pass < 16; pass++) {
    const int u = pass * 16 + (threadIdx.x >> 4);   // row t = u >> 4 of the group, column n = u & 15 of the tile
    const int ii = planar_col_ref(128 * chunk + 2 * (16 * g + (u & 15)) + e, pc);
    const size_t L = (size_t)(16 * rg + (u >> 4)) * (size_t)num_per + (size_t)ii;
    if (L >= L0 && L - L0 < nL) dst[((L - L0) * planes + plane) * N + z0 + zl] = tile[u][zl];
  }
}

}  // namespace spiral
