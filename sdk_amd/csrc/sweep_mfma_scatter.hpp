// The one-tile matrix-core pass (sweep_mfma.hpp, k_sweep_mfma_batch) over a ROW SHARD, writing what the multi-GPU exchange
// consumes: every query's output goes to that query's partial buffer in the per-plane reduce-scatter layout
//   [plane][g = ii % G][r][crt][z][ii / G],  G in {2, 4, 8}
// (sp_query_sweep_scatter_plane's, sdk_amd/sharding.py scatter_plane_layout_index; residues < q).  The interleave is fixed by
// the fold tree -- a rank's local fold pairs column i with i + half, so a rank owns a residue class of columns -- and it is
// the whole difference to k_sweep_mfma_batch: loads, digit extraction, MFMAs and the recombination are the same code.
//
// Store shapes (template parameter STORE; measurements in profiles/sharded_batch_pass.md):
//   1  from the registers: lane (kb, mp) holds columns 2 (16 g + mp) + e of four query columns; for one e the 16 lanes of a
//      group fall into G / 2 residue classes (both e: G), i.e. dword stores in runs of 128 / G bytes (64 B at G = 2, 16 B at G = 8)
//   2  staged through LDS: the four waves of the workgroup cover the 128 columns of a chunk; the chunk's 16 KiB of results
//      ([query][r][crt][g][ii / G]) are written to LDS, and after a workgroup barrier 256 threads store them as 16-byte pieces
//      in runs of 512 / G bytes.  Costs two barriers per chunk (the waves are otherwise independent) and 16.25 KiB of LDS.
// Its own header, instantiated in sweep_planar.hip only: sweep.hip's kernels keep their machine code.
#pragma once
#include "sweep_mfma.hpp"

namespace spiral {

struct SweepScatterDesc {
  const u64* db;                   // PACKED row shard: plane 0
  const u32* rq;                   // query digit table [N][nj / 16][2][64][4] (k_query_digits)
  const u32* rq_off;               // offset terms [N][2][16] (k_query_offset_terms)
  u32* out[SWEEP_BATCH_MAX];       // per query: partial buffer [plane][g][r][crt][z][ii / G]
  int batch;                       // 1 .. 8
  int planes, num_per, nj;         // nj % 32 == 0, nj <= 512, num_per % 128 == 0
  int cpw;                         // chunks per workgroup, divides num_per / 128
  int G, lgG;                      // 2, 4 or 8 and its log2
  u32 c4[2], c5[2], c6[2];         // 2^32, 2^40, 2^48 mod q_crt
};

constexpr int SCATTER_STAGE_QSTRIDE = 4 * 128 + 8;   // words per query in the LDS stage: the four lane groups of a wave (queries
                                                     // 2 kb, 2 kb + 1) then start 16 banks apart instead of on the same one
constexpr size_t SCATTER_STAGE_BYTES = (size_t)SWEEP_BATCH_MAX * SCATTER_STAGE_QSTRIDE * 4;

template <int NB, int MINWG, int STORE>
__global__ __launch_bounds__(256, MINWG) void k_sweep_mfma_scatter(DevTables T, SweepScatterDesc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_rq[];
  const int lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // slot group of this wave
  const int kb = lane >> 4, mp = lane & 15;
  const int chunks = d.num_per >> 7;
  const int wgs_per_zp = chunks / d.cpw;
  const int zp = blockIdx.x / wgs_per_zp;  // plane * N + z
  const int chunk0 = (blockIdx.x - zp * wgs_per_zp) * d.cpw;
  const int z = zp & (N - 1), plane = zp >> POLY_LEN_LOG2;
  const int steps = d.nj >> 4, npairs = d.nj >> 1;
  const int n16 = steps * 128;   // 16-byte entries of the z-row's digit table
  {
    const mf_u32x4_t* src = reinterpret_cast<const mf_u32x4_t*>(d.rq) + (size_t)z * n16;
    mf_u32x4_t* dst = reinterpret_cast<mf_u32x4_t*>(smem_rq);
    int i0 = 0;
    for (; i0 + 16 * 256 <= n16; i0 += 16 * 256) {
      mf_u32x4_t t[16];
#pragma unroll
      for (int k = 0; k < 16; k++) t[k] = src[i0 + k * 256 + threadIdx.x];
#pragma unroll
      for (int k = 0; k < 16; k++) dst[i0 + k * 256 + threadIdx.x] = t[k];
    }
    for (int i = i0 + threadIdx.x; i < n16; i += 256) dst[i] = src[i];
    __syncthreads();
  }
  const mf_u32x4_t* rql = reinterpret_cast<const mf_u32x4_t*>(smem_rq) + lane;
  u32* const stage = reinterpret_cast<u32*>(smem_rq) + (size_t)n16 * 4;   // STORE == 2: behind the digit table
  const u32* pu = reinterpret_cast<const u32*>(d.db) + packed_unit_offset((size_t)zp, 0, chunk0, npairs, chunks) +
                  (size_t)(2 * kb) * 448;
  const u32* p4 = pu + (16 * g + mp) * 4;
  const u32* p3 = pu + 256 + (16 * g + mp) * 3;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const u32 M = 0x0FFFFFFFu;
  const int total = d.cpw * steps;
  const int npl = d.num_per >> d.lgG;                 // columns per residue class
  const size_t class_words = (size_t)4 * N * npl;     // one class of one plane: [r][crt][z][ii / G]
  // queries b = 2 kb, 2 kb + 1 of this lane group (STORE == 1), picked from the kernel arguments with scalar loads + selects
  u32* out_b0 = d.out[0];
  u32* out_b1 = d.out[1];
#pragma unroll
  for (int k2 = 1; k2 < 4; k2++) {
    out_b0 = kb == k2 ? d.out[2 * k2] : out_b0;
    out_b1 = kb == k2 ? d.out[2 * k2 + 1] : out_b1;
  }
  const mf_u32x4_t off0 = reinterpret_cast<const mf_u32x4_t*>(d.rq_off)[(size_t)z * 8 + kb];
  const mf_u32x4_t off1 = reinterpret_cast<const mf_u32x4_t*>(d.rq_off)[(size_t)z * 8 + 4 + kb];
  mf_u32x4_t va[NB][2];
  mf_u32x3_t vb[NB][2];

// (the load order and the step are k_sweep_mfma_batch's: see the comments there)
#define SPS_LOAD(BUF, S)                                                                             \
  {                                                                                                  \
    const u32* q4 = p4 + (size_t)(S) * 3584;                                                         \
    const u32* q3 = p3 + (size_t)(S) * 3584;                                                         \
    va[BUF][0] = __builtin_nontemporal_load(reinterpret_cast<const mf_u32x4_t*>(q4));               \
    __builtin_amdgcn_sched_barrier(0);                                                               \
    vb[BUF][0] = __builtin_nontemporal_load(reinterpret_cast<const mf_u32x3_t*>(q3));               \
    __builtin_amdgcn_sched_barrier(0);                                                               \
    va[BUF][1] = __builtin_nontemporal_load(reinterpret_cast<const mf_u32x4_t*>(q4 + 448));         \
    __builtin_amdgcn_sched_barrier(0);                                                               \
    vb[BUF][1] = __builtin_nontemporal_load(reinterpret_cast<const mf_u32x3_t*>(q3 + 448));         \
    __builtin_amdgcn_sched_barrier(0);                                                               \
  }
#define SPS_STEP(BUF, SL)                                                                            \
  {                                                                                                  \
    u32 f[2][8];                                                                                     \
    _Pragma("unroll") for (int u = 0; u < 2; u++) {                                                  \
      const u32 d0 = va[BUF][u].x, d1 = va[BUF][u].y, d2 = va[BUF][u].z, d3 = va[BUF][u].w;          \
      const u32 d4 = vb[BUF][u].x, d5 = vb[BUF][u].y, d6 = vb[BUF][u].z;                             \
      f[u][0] = d0 & M;                                                                              \
      f[u][1] = __builtin_amdgcn_alignbit(d1, d0, 28) & M;                                           \
      f[u][2] = __builtin_amdgcn_alignbit(d2, d1, 24) & M;                                           \
      f[u][3] = __builtin_amdgcn_alignbit(d3, d2, 20) & M;                                           \
      f[u][4] = __builtin_amdgcn_alignbit(d4, d3, 16) & M;                                           \
      f[u][5] = __builtin_amdgcn_alignbit(d5, d4, 12) & M;                                           \
      f[u][6] = __builtin_amdgcn_alignbit(d6, d5, 8) & M;                                            \
      f[u][7] = d6 >> 4;                                                                             \
    }                                                                                                \
    v4i_t A[2][2];                                                                                   \
    _Pragma("unroll") for (int e = 0; e < 2; e++) _Pragma("unroll") for (int c = 0; c < 2; c++) {    \
      A[e][c][0] = (int)offset_digits(f[0][2 * e + c]);                                              \
      A[e][c][1] = (int)offset_digits(f[0][4 + 2 * e + c]);                                          \
      A[e][c][2] = (int)offset_digits(f[1][2 * e + c]);                                              \
      A[e][c][3] = (int)offset_digits(f[1][4 + 2 * e + c]);                                          \
    }                                                                                                \
    _Pragma("unroll") for (int c = 0; c < 2; c++) {                                                  \
      const mf_u32x4_t R = rql[((SL) * 2 + c) * 64];                                                 \
      _Pragma("unroll") for (int s = 0; s < 7; s++) {                                                \
        const u32 sh = (u32)(8 * (s < 3 ? 3 - s : s - 3));                                           \
        const mf_u32x4_t Bs = s < 3 ? R >> sh : R << sh;                                             \
        const v4i_t Bi = __builtin_bit_cast(v4i_t, Bs);                                              \
        acc[0][c][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Bi, A[0][c], acc[0][c][s], 0, 0, 0);    \
        acc[1][c][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Bi, A[1][c], acc[1][c][s], 0, 0, 0);    \
      }                                                                                              \
    }                                                                                                \
  }

#pragma unroll
  for (int k = 0; k < NB - 1; k++) SPS_LOAD(k, k)
  for (int ch = 0; ch < d.cpw; ch++) {
    v4i_t acc[2][2][7];  // [column tile e][crt][shift]
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
      for (int c = 0; c < 2; c++)
#pragma unroll
        for (int s = 0; s < 7; s++) acc[e][c][s] = v4i_t{0, 0, 0, 0};
    for (int s0 = 0; s0 < steps; s0 += NB) {
#pragma unroll
      for (int k = 0; k < NB; k++) {
        const int ahead = min(ch * steps + s0 + k + NB - 1, total - 1);
        SPS_LOAD((k + NB - 1) % NB, ahead)
        __builtin_amdgcn_sched_barrier(0);
        SPS_STEP(k, s0 + k)
      }
    }
    // chunk done: register i = query column 4 kb + i (b = 2 kb + i / 2, r = i % 2), lane mp = slot 16 g + mp = columns
    // cw = 2 (16 g + mp) + e of the chunk, i.e. class cw % G, position (chunk * 128 + cw) / G of the class's z-row
    const int cw0 = 32 * g + 2 * mp;
    const int chunk = chunk0 + ch;
    if (STORE == 2) __syncthreads();   // every wave has read the previous chunk's stage
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int b = 2 * kb + (i >> 1);
      if (STORE == 2 || b < d.batch) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
          const ModConst mc = c ? m1 : m0;
          const u32 oc = c ? off1[i] : off0[i];
          const u32 v0 = combine_digit_sums(acc[0][c][0][i], acc[0][c][1][i], acc[0][c][2][i], acc[0][c][3][i], acc[0][c][4][i],
                                            acc[0][c][5][i], acc[0][c][6][i], mc, d.c4[c], d.c5[c], d.c6[c], oc);
          const u32 v1 = combine_digit_sums(acc[1][c][0][i], acc[1][c][1][i], acc[1][c][2][i], acc[1][c][3][i], acc[1][c][4][i],
                                            acc[1][c][5][i], acc[1][c][6][i], mc, d.c4[c], d.c5[c], d.c6[c], oc);
          const int rc = (i & 1) * 2 + c;
          if (STORE == 2) {
            u32* st = stage + b * SCATTER_STAGE_QSTRIDE + rc * 128;
            const int G1 = d.G - 1, per = 128 >> d.lgG;
            st[(cw0 & G1) * per + (cw0 >> d.lgG)] = v0;
            st[((cw0 + 1) & G1) * per + ((cw0 + 1) >> d.lgG)] = v1;
          } else {
            u32* sel = (i >> 1) ? out_b1 : out_b0;
            u32* ob = sel + (size_t)plane * 4 * N * d.num_per + ((size_t)rc * N + z) * npl;
            const int ii0 = chunk * 128 + cw0, G1 = d.G - 1;
            __builtin_nontemporal_store(v0, ob + (size_t)(ii0 & G1) * class_words + (ii0 >> d.lgG));
            __builtin_nontemporal_store(v1, ob + (size_t)((ii0 + 1) & G1) * class_words + ((ii0 + 1) >> d.lgG));
          }
        }
      }
    }
    if (STORE == 2) {
      __syncthreads();
      // 8 queries x 4 (r, crt) x 128 words = 1024 16-byte pieces; piece q = t + 256 k: query (t >> 7) + 2 k (wave-uniform),
      // (r, crt) and the position inside the 128 words [g][ii / G] from the rest
      const int t = threadIdx.x, per = 128 >> d.lgG;
      const int bw = __builtin_amdgcn_readfirstlane(t >> 7);
      const int rc = (t >> 5) & 3, within = (t & 31) * 4;
      const int cls = within / per, idx = within - cls * per;
      const size_t o = (size_t)plane * 4 * N * d.num_per + (size_t)cls * class_words + ((size_t)rc * N + z) * npl +
                       (size_t)chunk * per + idx;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int b = bw + 2 * k;
        if (b < d.batch) {
          const mf_u32x4_t v = *reinterpret_cast<const mf_u32x4_t*>(stage + b * SCATTER_STAGE_QSTRIDE + rc * 128 + within);
          u32* ob = bw ? d.out[2 * k + 1] : d.out[2 * k];   // constant indices: scalar loads from the kernel arguments
          __builtin_nontemporal_store(v, reinterpret_cast<mf_u32x4_t*>(ob + o));
        }
      }
    }
  }
#undef SPS_LOAD
#undef SPS_STEP
}

}  // namespace spiral
