// Item read-back (sp_db_read_items / sp_db_export_rows): the inverse of the item loaders of db.hip -- item bytes out of the resident
// NTT words (server.rs:277-357 load_item_from_seek / load_db_from_seek read backwards; loading.rs:278-359 for the upserts).
//
// An item's 2048 words per plane lie one per z, a whole (chunk, row pair) stride apart in every dense format: a workgroup that walked
// one item would fetch a 64-byte sector for 7 or 8 useful bytes.  So a window of items takes two steps:
//   1. GATHER, one kernel per resident form: the window's words -> the handle's read buffer as [item of window][plane][z], canonical
//      lo | hi << 32.  The held items of a window of consecutive item indices are a run [L0, L0 + nL) of the handle's LOCAL linear index
//      L = local row * local columns + local column in every dense form (row shards clip the run, a column shard's columns ii = g mod G
//      are its local columns ii / G), so a gather reads whole resident runs -- 256 bytes of 8-byte words, whole 1792-byte PACKED units
//      -- through an LDS tile and writes z-runs of 128 or 256 bytes.  (The digit-planar gather is k_planar_gather, planar_resident.hpp.)
//      A sparse bucket's store is [slot][plane][z] already: it is decoded in place through the window's slot list.
//   2. DECODE, one kernel for all forms: one workgroup per (held item, plane) inverse-transforms both residue vectors, undoes
//      recenter_mod and packs the logp-bit coefficients back into the chunk's bytes.
// Included by db.hip only.
#pragma once
#include "device_common.hpp"

namespace spiral {

// ---- step 1, 8-byte words [plane][z][jl][il]: for a fixed (plane, z) the window is the contiguous run L0 .. L0 + nL - 1
// grid (ceil(nL / 32), N / 32, planes): a 32 x 32 tile transpose (reads: 256-byte runs along L; writes: 256-byte runs along z)
__global__ __launch_bounds__(256) void k_items_gather_words8(u64* dst, const u64* db, size_t L0, size_t nL, size_t row_words, int planes) {
  __shared__ u64 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const size_t lt = (size_t)blockIdx.x * 32;
  const int zt = blockIdx.y * 32, plane = blockIdx.z;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int zl = ty + 8 * i;
    if (lt + tx < nL) tile[zl][tx] = db[((size_t)plane * N + zt + zl) * row_words + L0 + lt + tx];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const size_t l = lt + ty + 8 * i;
    if (l < nL) dst[(l * planes + plane) * N + zt + tx] = tile[tx][ty + 8 * i];
  }
}

// ---- step 1, PACKED: a workgroup owns one unit position (row pair jp, 128-column chunk) for 16 z-rows of one plane -- 16 whole units of
// 1792 bytes, each lane's 16 + 12 bytes read once -- and hands the unit's 256 items their 128-byte z-runs.
// grid (n_jp * chunks, N / 16, planes)
constexpr int GATHER_Z = 16;
__global__ __launch_bounds__(256) void k_items_gather_packed(u64* dst, const u32* db, size_t L0, size_t nL, int jp_lo, int np_local,
                                                            int nj, int planes) {
  __shared__ u64 tile[256][GATHER_Z + 1];
  const int chunks = np_local >> 7, npairs = nj >> 1;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks), jp = jp_lo + (int)(blockIdx.x / (unsigned)chunks);
  const int plane = blockIdx.z, z0 = blockIdx.y * GATHER_Z;
  {
    // does the window [L0, L0 + nL) meet either row's 128 columns of this unit?  (uniform per workgroup: before any barrier)
    const size_t r0 = (size_t)(2 * jp) * np_local + (size_t)chunk * 128, r1 = r0 + (size_t)np_local;
    const size_t L1 = L0 + nL;
    const bool hit = (r0 < L1 && r0 + 128 > L0) || (r1 < L1 && r1 + 128 > L0);
    if (!hit) return;
  }
  const int lane = threadIdx.x & 63, zq = threadIdx.x >> 6;
#pragma unroll 1
  for (int pass = 0; pass < GATHER_Z / 4; pass++) {
    const int zl = pass * 4 + zq;
    const u32* unit = db + packed_unit_offset((size_t)plane * N + z0 + zl, jp, chunk, npairs, chunks);
#pragma unroll
    for (int which = 0; which < 4; which++)   // which = row a * 2 + column b: item (row 2 jp + a, column 128 chunk + 2 lane + b)
      tile[which * 64 + lane][zl] = unpack_word(unit, lane, which);   // (tile rows in lane order: a wave's 64 stores are 2-way at most)
  }
  __syncthreads();
  const int zl = threadIdx.x & (GATHER_Z - 1);
#pragma unroll 1
  for (int pass = 0; pass < 256 / (256 / GATHER_Z); pass++) {
    const int u = pass * (256 / GATHER_Z) + (threadIdx.x >> 4);   // tile row: which = u >> 6, lane = u & 63
    const size_t L = (size_t)(2 * jp + (u >> 7)) * np_local + (size_t)chunk * 128 + (size_t)(2 * (u & 63) + ((u >> 6) & 1));
    if (L >= L0 && L - L0 < nL) dst[((L - L0) * planes + plane) * N + z0 + zl] = tile[u][zl];
  }
}

// ---- step 2: one workgroup per (held item k, plane); list[k] = {index of the item's polynomials in `src` ([index][plane][z]), position
// of the item in the byte window}.  Thread tau holds the words at z = 8 tau + k, and after the inverse transforms (from_ntt,
// poly.rs:646-663, without the compose) the coefficients z = tau + 256 k as residues a0 mod q0, a1 mod q1.  The loader stored
// recenter_mod(x, p, Q) (server.rs:338-341): x for x <= h = p / 2, Q - (p - x) above -- so a coefficient of its image has
// a0 == a1 <= h (x = a0) or q0 - a0 == q1 - a1 in [1, p - h - 1] (x = p - that); no 64-bit compose is needed.  Anything else is not
// the loader's: the polynomial counts as undecodable once and the coefficient reads as 0.  Only the W = ceil(nbytes * 8 / logp)
// coefficients that carry the chunk's bytes are looked at (a file-loaded database holds the next item's spill behind them).
// Output byte b = bits [8 b, 8 b + 8) of sum x_z 2^(z logp), the inverse of read_arbitrary_bits (server.rs:312-315).
__global__ __launch_bounds__(256) void k_items_decode(DevTables T, ItemDecodeDesc d) {
  __shared__ u32 lds0[LDS_WORDS];
  __shared__ u32 lds1[LDS_WORDS];
  __shared__ u32 xs[N];
  __shared__ int bad;
  const int tau = threadIdx.x;
  const int plane = (int)(blockIdx.x % (unsigned)d.planes);
  const ItemDecodeRec rec = d.list[blockIdx.x / (unsigned)d.planes];
  const int pos0 = plane * d.bytes_per_chunk;
  if (pos0 >= d.db_item_size) return;   // the chunk starts past the item: it contributes nothing (uniform per workgroup)
  const int nbytes = d.db_item_size - pos0 < d.bytes_per_chunk ? d.db_item_size - pos0 : d.bytes_per_chunk;
  const int W = (nbytes * 8 + d.logp - 1) / d.logp;   // <= N: checked by the caller
  const u64* src = d.src + ((size_t)rec.src * d.planes + plane) * N + 8 * tau;
  if (tau == 0) bad = 0;
  u32 a0[8], a1[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const u64 w = src[k];
    a0[k] = (u32)w;
    a1[k] = (u32)(w >> 32);
  }
  const u32 q0 = T.c.mod[0].q, q1 = T.c.mod[1].q;
  {
    const u32* iw = inv_tables(T.tw, 0);
    ntt_inv_block(a0, tau, lds0, lds1, iw, iw + N, q0, T.c.mod[0].two_q);
  }
  __syncthreads();
  {
    const u32* iw = inv_tables(T.tw, 1);
    ntt_inv_block(a1, tau, lds0, lds1, iw, iw + N, q1, T.c.mod[1].two_q);
  }
  const u32 h = d.pt_modulus / 2, nmax = d.pt_modulus - h - 1;
  bool any_bad = false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int z = tau + 256 * k;
    const u32 n0 = q0 - a0[k], n1 = q1 - a1[k];
    u32 x = 0;
    if (a0[k] == a1[k] && a0[k] <= h)
      x = a0[k];
    else if (n0 == n1 && n0 >= 1u && n0 <= nmax)
      x = d.pt_modulus - n0;
    else if (z < W)
      any_bad = true;
    xs[z] = x;
  }
  if (any_bad) bad = 1;   // (every writer stores the same value)
  __syncthreads();
  if (tau == 0 && bad) atomicAdd(d.undecodable, 1ULL);
  uint8_t* out = d.out + (size_t)rec.pos * (size_t)d.db_item_size + (size_t)pos0;
  for (int b = tau; b < nbytes; b += 256) {
    const int bit = 8 * b;
    int z = bit / d.logp;
    const int sh = bit - z * d.logp;
    u64 acc = (u64)xs[z] >> sh;
    for (int got = d.logp - sh; got < 8; got += d.logp) {
      z++;
      acc |= (u64)(z < W ? xs[z] : 0u) << got;
    }
    out[b] = (uint8_t)acc;
  }
}

void launch_items_gather(u64* dst, const u64* db, size_t L0, size_t nL, int np_local, int nj, int planes, int packed, hipStream_t s) {
  if (nL == 0) return;
  if (packed) {
    const int jp_lo = (int)(L0 / (size_t)np_local) / 2, jp_hi = (int)((L0 + nL - 1) / (size_t)np_local) / 2;
    hipLaunchKernelGGL(k_items_gather_packed, dim3((unsigned)(jp_hi - jp_lo + 1) * (unsigned)(np_local >> 7), N / GATHER_Z, planes), dim3(256),
                       0, s, dst, reinterpret_cast<const u32*>(db), L0, nL, jp_lo, np_local, nj, planes);
    launched(0, "k_items_gather_packed");
  } else {
    hipLaunchKernelGGL(k_items_gather_words8, dim3((unsigned)((nL + 31) / 32), N / 32, planes), dim3(256), 0, s, dst, db, L0, nL,
                       (size_t)nj * (size_t)np_local, planes);
    launched(0, "k_items_gather_words8");
  }
}
void launch_items_decode(const DevTables& T, const ItemDecodeDesc& d, size_t n_items, hipStream_t s) {
  if (n_items == 0) return;   // (n_items * planes <= UPSERT_MAX_GROUP_PLANES = 2^23: the caller cuts its windows there)
  hipLaunchKernelGGL(k_items_decode, dim3((unsigned)(n_items * (size_t)d.planes)), dim3(256), 0, s, T, d);
  launched(0, "k_items_decode");
}

}  // namespace spiral
