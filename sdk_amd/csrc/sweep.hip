// Database sweep = multiply_reg_by_database (server.rs:155-221) for gfx950: HBM-streaming integer kernels, one per
// database shape (PACKED wide, persistent, batched, 8-byte wide, narrow).  The judged kernel lives here.
#include "device_common.hpp"
#include "sweep_mfma.hpp"
#include "server.hpp"

namespace spiral {

// ------------------------------------------------------------------------------------------------
// database sweep  (server.rs:155-221)
// ------------------------------------------------------------------------------------------------
// WIDE (num_per >= 128): one wave per (plane, z, 128-wide ii chunk).  Lane l owns output columns
// ii = chunk*128 + 2l, 2l+1 and streams its 16 bytes of every first-dimension row j: 1 KiB
// contiguous per wave per row.  The query words for (z, j) are wave-uniform (scalar loads, SGPR
// operands of v_mad_u64_u32); no cross-lane traffic at all.  Products are < 2^56, so 256 rows are
// accumulated in u64 between Barrett folds (the reference uses u128 and one % at the end; the
// residues are identical).
// flat index of output (plane, rc = r*2+crt, z, ii) in the (possibly column-interleaved) partial buffer
__device__ __forceinline__ size_t sweep_out_index(const SweepDesc& d, int plane, int rc, int z, int ii) {
  const int G = d.out_G > 1 ? d.out_G : 1;
  const int npl = d.num_per / G;
  const size_t chunk_words = (size_t)d.planes * 4 * N * npl;
  return (size_t)(ii % G) * chunk_words + (((size_t)plane * 4 + rc) * N + z) * npl + (ii / G);
}
__device__ __forceinline__ void sweep_store_pair(const SweepDesc& d, int plane, int z, int ii0, u32 r0c0_a, u32 r0c0_b,
                                                 u32 r0c1_a, u32 r0c1_b, u32 r1c0_a, u32 r1c0_b, u32 r1c1_a,
                                                 u32 r1c1_b) {
  if (d.out_G <= 1 && d.nt_store) {
    const size_t rc = (size_t)N * d.num_per;
    u32* o = d.out + (size_t)plane * 4 * rc + (size_t)z * d.num_per + ii0;
    __builtin_nontemporal_store(mf_u32x2_t{r0c0_a, r0c0_b}, reinterpret_cast<mf_u32x2_t*>(o + 0 * rc));
    __builtin_nontemporal_store(mf_u32x2_t{r0c1_a, r0c1_b}, reinterpret_cast<mf_u32x2_t*>(o + 1 * rc));
    __builtin_nontemporal_store(mf_u32x2_t{r1c0_a, r1c0_b}, reinterpret_cast<mf_u32x2_t*>(o + 2 * rc));
    __builtin_nontemporal_store(mf_u32x2_t{r1c1_a, r1c1_b}, reinterpret_cast<mf_u32x2_t*>(o + 3 * rc));
  } else if (d.out_G <= 1) {
    const size_t rc = (size_t)N * d.num_per;
    u32* o = d.out + (size_t)plane * 4 * rc + (size_t)z * d.num_per + ii0;
    *reinterpret_cast<uint2*>(o + 0 * rc) = make_uint2(r0c0_a, r0c0_b);
    *reinterpret_cast<uint2*>(o + 1 * rc) = make_uint2(r0c1_a, r0c1_b);
    *reinterpret_cast<uint2*>(o + 2 * rc) = make_uint2(r1c0_a, r1c0_b);
    *reinterpret_cast<uint2*>(o + 3 * rc) = make_uint2(r1c1_a, r1c1_b);
  } else {
    d.out[sweep_out_index(d, plane, 0, z, ii0)] = r0c0_a;
    d.out[sweep_out_index(d, plane, 0, z, ii0 + 1)] = r0c0_b;
    d.out[sweep_out_index(d, plane, 1, z, ii0)] = r0c1_a;
    d.out[sweep_out_index(d, plane, 1, z, ii0 + 1)] = r0c1_b;
    d.out[sweep_out_index(d, plane, 2, z, ii0)] = r1c0_a;
    d.out[sweep_out_index(d, plane, 2, z, ii0 + 1)] = r1c0_b;
    d.out[sweep_out_index(d, plane, 3, z, ii0)] = r1c1_a;
    d.out[sweep_out_index(d, plane, 3, z, ii0 + 1)] = r1c1_b;
  }
}

__global__ __launch_bounds__(256) void k_sweep_wide(DevTables T, SweepDesc d) {
  const int lane = threadIdx.x & 63;
  const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int chunks = d.num_per >> 7;
  const int chunk = unit % chunks;
  const int zp = unit / chunks;  // plane * N + z
  const int z = zp & (N - 1);
  const int plane = zp >> POLY_LEN_LOG2;
  if (plane >= d.planes) return;
  const ulonglong2* p =
      reinterpret_cast<const ulonglong2*>(d.db + ((size_t)zp * d.nj) * d.num_per + (size_t)chunk * 128) + lane;
  const size_t stride = (size_t)(d.num_per >> 1);
  const uint4* __restrict__ qrow = reinterpret_cast<const uint4*>(d.qv) + ((size_t)z * d.dim0 + d.j0);
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];

  u64 a00 = 0, a01 = 0, a02 = 0, a03 = 0;  // word 0: n0_0, n0_1, n1_0, n1_1
  u64 a10 = 0, a11 = 0, a12 = 0, a13 = 0;  // word 1
  for (int jb = 0; jb < d.nj; jb += 256) {
    const int je = min(jb + 256, d.nj);
    for (int j = jb; j < je; j++) {
      // streamed once: non-temporal loads, no manual unroll (the fastest of the forms measured in round 1,
      // profiles/r01_sweep_variants.md: 6.8 TB/s)
      const ulonglong2* a = p + (size_t)j * stride;
      ulonglong2 w;
      w.x = __builtin_nontemporal_load(&a->x);
      w.y = __builtin_nontemporal_load(&a->y);
      const uint4 qa = qrow[j];  // (a0_lo, a0_hi, a1_lo, a1_hi)
      const u32 b0l = (u32)w.x, b0h = (u32)(w.x >> 32);
      const u32 b1l = (u32)w.y, b1h = (u32)(w.y >> 32);
      a00 += (u64)qa.x * b0l;
      a01 += (u64)qa.z * b0l;
      a02 += (u64)qa.y * b0h;
      a03 += (u64)qa.w * b0h;
      a10 += (u64)qa.x * b1l;
      a11 += (u64)qa.z * b1l;
      a12 += (u64)qa.y * b1h;
      a13 += (u64)qa.w * b1h;
    }
    a00 = reduce64(a00, m0);
    a01 = reduce64(a01, m0);
    a02 = reduce64(a02, m1);
    a03 = reduce64(a03, m1);
    a10 = reduce64(a10, m0);
    a11 = reduce64(a11, m0);
    a12 = reduce64(a12, m1);
    a13 = reduce64(a13, m1);
  }
  // out[plane][r][crt][z][ii]: (r0,c0) = n0_0, (r0,c1) = n1_0, (r1,c0) = n0_1, (r1,c1) = n1_1
  sweep_store_pair(d, plane, z, chunk * 128 + 2 * lane, (u32)a00, (u32)a10, (u32)a02, (u32)a12, (u32)a01, (u32)a11,
                   (u32)a03, (u32)a13);
}

// PACKED wide sweeps: as k_sweep_wide, but each lane streams 28 bytes per ROW PAIR (7 dwords = 8 limbs of 28 bits)
// instead of 32; limb extraction is 6 v_alignbit + 7 v_and per 16 multiply-accumulates.
typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
typedef u32 u32x3_t __attribute__((ext_vector_type(3), aligned(4)));

// Persistent PACKED sweep, plain form: a fixed grid of `wgs_per_cu` workgroups per CU walks the (z, chunk) streams, four row
// pairs in flight per lane.  Used where the ring form below does not divide the stream (row-pair counts that are not a
// multiple of 4: narrow row shards, odd shapes) and as the A/B partner of the ring form (pipe_ring = 0).
__global__ __launch_bounds__(256) void k_sweep_packed_persist(DevTables T, SweepDesc d, int units, int hi_prio) {
  // the sweep is a latency-bound load stream using ~20 % of the VALU slots: when fold kernels share the CU its
  // waves must win instruction arbitration or the loads in flight (and the HBM rate) drop
  if (hi_prio) __builtin_amdgcn_s_setprio(3);
  constexpr int U = 4;
  const int lane = threadIdx.x & 63;
  const int wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int nwaves = gridDim.x * 4;
  const int chunks = d.num_per >> 7;
  const int npairs = d.nj >> 1;
  const size_t ustride = 448;  // consecutive row pairs of a (zp, chunk) stream are adjacent
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const u32 M = 0x0FFFFFFFu;
  for (int unit = wave0; unit < units; unit += nwaves) {
    const int chunk = unit % chunks;
    const int zp = unit / chunks;
    const int z = zp & (N - 1);
    const int plane = zp >> POLY_LEN_LOG2;
    const u32* base = reinterpret_cast<const u32*>(d.db) + packed_unit_offset((size_t)zp, 0, chunk, npairs, chunks);
    const uint4* __restrict__ qrow = reinterpret_cast<const uint4*>(d.qv) + ((size_t)z * d.dim0 + d.j0);
    u64 a00 = 0, a01 = 0, a02 = 0, a03 = 0, a10 = 0, a11 = 0, a12 = 0, a13 = 0;
    for (int jb = 0; jb < npairs; jb += 128) {
      const int je = min(jb + 128, npairs);
      for (int jp0 = jb; jp0 < je; jp0 += U) {
        u32x4_t va[U];
        u32x3_t vb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int jp = min(jp0 + u, je - 1);
          const u32* uu = base + (size_t)jp * ustride;
          va[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(uu + lane * 4));
          vb[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(uu + 256 + lane * 3));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int jp = jp0 + u;
          if (jp < je) {
            const u32 d0 = va[u].x, d1 = va[u].y, d2 = va[u].z, d3 = va[u].w, d4 = vb[u].x, d5 = vb[u].y, d6 = vb[u].z;
            const uint4 qa = qrow[2 * jp];
            const uint4 qb = qrow[2 * jp + 1];
            const u32 f0 = d0 & M;
            const u32 f1 = __builtin_amdgcn_alignbit(d1, d0, 28) & M;
            const u32 f2 = __builtin_amdgcn_alignbit(d2, d1, 24) & M;
            const u32 f3 = __builtin_amdgcn_alignbit(d3, d2, 20) & M;
            const u32 f4 = __builtin_amdgcn_alignbit(d4, d3, 16) & M;
            const u32 f5 = __builtin_amdgcn_alignbit(d5, d4, 12) & M;
            const u32 f6 = __builtin_amdgcn_alignbit(d6, d5, 8) & M;
            const u32 f7 = d6 >> 4;
            // (row 2jp, ii 2l) = (f0, f1); (2jp, 2l+1) = (f2, f3); (2jp+1, 2l) = (f4, f5); (2jp+1, 2l+1) = (f6, f7)
            a00 += (u64)qa.x * f0; a01 += (u64)qa.z * f0; a02 += (u64)qa.y * f1; a03 += (u64)qa.w * f1;
            a10 += (u64)qa.x * f2; a11 += (u64)qa.z * f2; a12 += (u64)qa.y * f3; a13 += (u64)qa.w * f3;
            a00 += (u64)qb.x * f4; a01 += (u64)qb.z * f4; a02 += (u64)qb.y * f5; a03 += (u64)qb.w * f5;
            a10 += (u64)qb.x * f6; a11 += (u64)qb.z * f6; a12 += (u64)qb.y * f7; a13 += (u64)qb.w * f7;
          }
        }
      }
      a00 = reduce64(a00, m0); a01 = reduce64(a01, m0); a02 = reduce64(a02, m1); a03 = reduce64(a03, m1);
      a10 = reduce64(a10, m0); a11 = reduce64(a11, m0); a12 = reduce64(a12, m1); a13 = reduce64(a13, m1);
    }
    // out[plane][r][crt][z][ii]: (r0,c0) = n0_0, (r0,c1) = n1_0, (r1,c0) = n0_1, (r1,c1) = n1_1
    sweep_store_pair(d, plane, z, chunk * 128 + 2 * lane, (u32)a00, (u32)a10, (u32)a02, (u32)a12, (u32)a01, (u32)a11,
                     (u32)a03, (u32)a13);
  }
}
// Ring form (the default, and the judged kernel): two buffers of U row pairs per wave, the loads of one in flight while the
// other is multiplied, and the first buffer of a wave's NEXT (z, chunk) stream requested before the sums of this one are
// reduced and stored.  A wave of the plain form has nothing in flight while it multiplies and relies on the other 15 waves
// of its CU; when fold kernels share the CU the multiplies take longer and the HBM queue runs dry.  One workgroup per CU
// (205 VGPRs at U = 8) leaves a fold wave's 256 registers free on every SIMD.  Needs npairs % (2 U) == 0.
// (Round 3 also tried handing the streams out by an atomic ticket counter, spreading a wave's row pairs over sub-streams,
// permuting the z-rows and sweeping a plane as two chunk-parity classes: no gain, removed; profiles/r03_ring_sweep.md,
// r02_sweep_experiments.md.)
typedef __attribute__((address_space(4))) const u32x4_t sweep_const_uint4;
template <int U>
__global__ __launch_bounds__(256) void k_sweep_packed_ring(DevTables T, SweepDesc d, int units, int hi_prio) {
  if (hi_prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63;
  const int wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int nwaves = gridDim.x * 4;
  const int chunks = d.num_per >> 7;
  const int npairs = d.nj >> 1;
  const size_t ustride = 448;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const u32 M = 0x0FFFFFFFu;
  if (wave0 >= units) return;
  u32x4_t va[U], na[U];
  u32x3_t vb[U], nb[U];
#define SPR_BASE(UNIT) \
  (reinterpret_cast<const u32*>(d.db) + packed_unit_offset((size_t)((UNIT) / chunks), 0, (UNIT) % chunks, npairs, chunks))
#define SPR_LOAD(VA, VB, BASE, JP0)                                                                       \
  _Pragma("unroll") for (int uu = 0; uu < U; uu++) {                                                      \
    const u32* u = (BASE) + (size_t)((JP0) + uu) * ustride;                                               \
    VA[uu] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(u + lane * 4));                  \
    VB[uu] = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(u + 256 + lane * 3));            \
  }
#define SPR_MAC(VA, VB, JP0)                                                                                              \
  _Pragma("unroll") for (int uu = 0; uu < U; uu++) {                                                                      \
    const int jp = (JP0) + uu;                                                                                            \
    const u32 d0 = VA[uu].x, d1 = VA[uu].y, d2 = VA[uu].z, d3 = VA[uu].w, d4 = VB[uu].x, d5 = VB[uu].y, d6 = VB[uu].z;    \
    const u32x4_t qa = qrow[2 * jp];                                                                                      \
    const u32x4_t qb = qrow[2 * jp + 1];                                                                                  \
    const u32 f0 = d0 & M;                                                                                                \
    const u32 f1 = __builtin_amdgcn_alignbit(d1, d0, 28) & M;                                                             \
    const u32 f2 = __builtin_amdgcn_alignbit(d2, d1, 24) & M;                                                             \
    const u32 f3 = __builtin_amdgcn_alignbit(d3, d2, 20) & M;                                                             \
    const u32 f4 = __builtin_amdgcn_alignbit(d4, d3, 16) & M;                                                             \
    const u32 f5 = __builtin_amdgcn_alignbit(d5, d4, 12) & M;                                                             \
    const u32 f6 = __builtin_amdgcn_alignbit(d6, d5, 8) & M;                                                              \
    const u32 f7 = d6 >> 4;                                                                                               \
    a00 += (u64)qa.x * f0; a01 += (u64)qa.z * f0; a02 += (u64)qa.y * f1; a03 += (u64)qa.w * f1;                           \
    a10 += (u64)qa.x * f2; a11 += (u64)qa.z * f2; a12 += (u64)qa.y * f3; a13 += (u64)qa.w * f3;                           \
    a00 += (u64)qb.x * f4; a01 += (u64)qb.z * f4; a02 += (u64)qb.y * f5; a03 += (u64)qb.w * f5;                           \
    a10 += (u64)qb.x * f6; a11 += (u64)qb.z * f6; a12 += (u64)qb.y * f7; a13 += (u64)qb.w * f7;                           \
  }
#define SPR_FOLD                                                                                          \
  a00 = reduce64(a00, m0); a01 = reduce64(a01, m0); a02 = reduce64(a02, m1); a03 = reduce64(a03, m1);     \
  a10 = reduce64(a10, m0); a11 = reduce64(a11, m0); a12 = reduce64(a12, m1); a13 = reduce64(a13, m1);
  const u32* base = SPR_BASE(wave0);
  SPR_LOAD(va, vb, base, 0)
  for (int unit = wave0; unit < units;) {
    const int chunk = unit % chunks;
    const int zp = unit / chunks;
    const int z = zp & (N - 1);
    const int plane = zp >> POLY_LEN_LOG2;
    // the query rows through the scalar cache (s_load): as plain loads they are VECTOR loads here (the kernel stores inside
    // the unit loop, so nothing is known to be unwritten) whose return is ordered behind the database loads in flight --
    // waiting for a query row would drain the ring
    const sweep_const_uint4* qrow =
        (const sweep_const_uint4*)(uintptr_t)(reinterpret_cast<const uint4*>(d.qv) + ((size_t)z * d.dim0 + d.j0));
    u64 a00 = 0, a01 = 0, a02 = 0, a03 = 0, a10 = 0, a11 = 0, a12 = 0, a13 = 0;
    int next_unit = units;
    const u32* next_base = base;
    // blocks of at most 128 row pairs = 256 rows of < 2^56 products between Barrett folds.  No conditional code inside a
    // block (a branch lets the optimiser sink the reload of a buffer below the multiplies of the other one)
    for (int jb = 0; jb < npairs; jb += 128) {
      const int len = min(128, npairs - jb);
      int j = jb;
      for (; j + 2 * U < jb + len; j += 2 * U) {
        SPR_LOAD(na, nb, base, j + U)
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the multiply-accumulates
        SPR_MAC(va, vb, j)
        SPR_LOAD(va, vb, base, j + 2 * U)
        __builtin_amdgcn_sched_barrier(0);
        SPR_MAC(na, nb, j + U)
      }
      SPR_LOAD(na, nb, base, j + U)
      __builtin_amdgcn_sched_barrier(0);
      SPR_MAC(va, vb, j)
      const bool more = jb + 128 < npairs;
      // the wave's next stream (its own again past the end: a harmless re-read of 7 KiB)
      next_unit = unit + nwaves;
      next_base = next_unit < units ? SPR_BASE(next_unit) : base;
      const u32* nb_base = more ? base : next_base;
      const int nb_jp = more ? jb + 128 : 0;
      SPR_LOAD(va, vb, nb_base, nb_jp)
      __builtin_amdgcn_sched_barrier(0);
      SPR_MAC(na, nb, j + U)
      SPR_FOLD
    }
    sweep_store_pair(d, plane, z, chunk * 128 + 2 * lane, (u32)a00, (u32)a10, (u32)a02, (u32)a12, (u32)a01, (u32)a11,
                     (u32)a03, (u32)a13);
    base = next_base;
    unit = next_unit;
  }
#undef SPR_BASE
#undef SPR_LOAD
#undef SPR_MAC
#undef SPR_FOLD
}
void launch_sweep_persist(const DevTables& T, const SweepDesc& d, int wgs_per_cu, hipStream_t s, int n_cus) {
  const int units = d.planes * N * (d.num_per >> 7);
  const int prio = (int)tunable("sweep_prio", 1);
  const int npairs = d.nj >> 1;
  // Ring form (default): pipe_ring = row pairs per buffer (8, 4 or 2; 0 = the plain form below), the largest that divides
  // the stream evenly, on pipe_ring_wgs workgroups per CU (default ONE: four waves with two buffers of 8 row pairs each
  // keep as many bytes in flight as sixteen plain waves with one buffer of 4, alone 2.23 against 2.27 ms per plane at
  // C2 -- and a second ring workgroup per CU starves the fold kernels beside it: their loads queue behind the ring's)
  long ring = tunable("pipe_ring", 8);
  while (ring > 1 && (npairs % (2 * ring) != 0 || (ring != 2 && ring != 4 && ring != 8))) ring >>= 1;
  if (ring >= 2) {
    const int ring_wgs = (int)std::max(1L, tunable("pipe_ring_wgs", 1));
    const dim3 rgrid((unsigned)std::min(n_cus * ring_wgs, (units + 3) / 4));
    switch (ring) {
      case 2: hipLaunchKernelGGL(k_sweep_packed_ring<2>, rgrid, dim3(256), 0, s, T, d, units, prio); break;
      case 8: hipLaunchKernelGGL(k_sweep_packed_ring<8>, rgrid, dim3(256), 0, s, T, d, units, prio); break;
      default: hipLaunchKernelGGL(k_sweep_packed_ring<4>, rgrid, dim3(256), 0, s, T, d, units, prio); break;
    }
    launched(PATH_SWEEP_PERSIST | PATH_SWEEP_RING | (d.out_G > 1 ? PATH_SCATTER_OUT : 0), "k_sweep_packed_ring");
    return;
  }
  const dim3 grid((unsigned)std::min(n_cus * wgs_per_cu, (units + 3) / 4));
  hipLaunchKernelGGL(k_sweep_packed_persist, grid, dim3(256), 0, s, T, d, units, prio);
  launched(PATH_SWEEP_PERSIST | (d.out_G > 1 ? PATH_SCATTER_OUT : 0), "k_sweep_packed_persist");
}

// Multi-query PACKED sweep: B queries share one pass over the database (BASELINE configs[4]).  Per row
// pair: one 28-byte load, B x 2 scalar query rows, 16 B multiply-accumulates.  HBM-bound up to B ~ 4,
// integer-ALU-bound beyond.
// U row pairs (28 B per lane each) are in flight per wave (U = 4 needs npairs % 4 == 0: no ragged tail, straight-line
// code): with B queries' accumulators the kernel runs at 2-5 waves per SIMD, and one load per wave leaves the HBM
// pipe mostly empty (B = 8: 21 ms per pass instead of ~10).
// QLDS: the B queries' rows for this workgroup's z (B * nj * 16 B, 64 KiB at B = 8) are staged in LDS once and
// read back as broadcast ds_reads.  The scalar-load form keeps them in the 16 KiB scalar cache, which B > 4
// overflows: every query word then costs an L2 round trip and the pass takes 25 ms instead of ~10 at B = 8.
// Needs all four waves of the workgroup on the same z (chunks % 4 == 0).
// LDS staging uses a FIXED row stride per query (QLDS_ROWS rows of 16 B): with a compile-time stride every (query, row
// pair in flight) read is one base VGPR + an immediate offset; a run-time stride (nj) costs one live address register
// per (query, row pair) -- 64 VGPRs at B = 8, U = 4 -- and pushes the kernel over 256 registers.
constexpr int QLDS_ROWS = 512;
template <int B, int U, bool QLDS>
__global__ __launch_bounds__(256, 2) void k_sweep_packed_batch(DevTables T, SweepBatchDesc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_q[];
  const int lane = threadIdx.x & 63;
  const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int chunks = d.num_per >> 7;
  const int chunk = unit % chunks;
  const int zp = unit / chunks;
  const int z = zp & (N - 1);
  const int plane = zp >> POLY_LEN_LOG2;
  const uint4* qs = reinterpret_cast<const uint4*>(smem_q);  // [B][nj]
  if (QLDS) {
    const int zp0 = (blockIdx.x * 4) / chunks;  // the whole workgroup shares one (plane, z)
    const int z0 = zp0 & (N - 1);
    uint4* qw = reinterpret_cast<uint4*>(smem_q);
#pragma unroll
    for (int b = 0; b < B; b++) {
      const uint4* src = reinterpret_cast<const uint4*>(d.qv[b]) + ((size_t)z0 * d.dim0 + d.j0);
      for (int j = threadIdx.x; j < d.nj; j += 256) qw[b * QLDS_ROWS + j] = src[j];
    }
    __syncthreads();
  }
  if (plane >= d.planes) return;
  const int npairs = d.nj >> 1;
  const u32* base = reinterpret_cast<const u32*>(d.db) + packed_unit_offset((size_t)zp, 0, chunk, npairs, chunks);
  const size_t ustride = 448;  // consecutive row pairs of a (zp, chunk) stream are adjacent
  const size_t qoff = (size_t)z * d.dim0 + d.j0;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const u32 M = 0x0FFFFFFFu;
  u64 acc[B][8];
#pragma unroll
  for (int b = 0; b < B; b++)
#pragma unroll
    for (int k = 0; k < 8; k++) acc[b][k] = 0;
  // Software pipeline in PING-PONG form: two buffers of U row pairs each; while buffer A is multiplied, buffer B's loads
  // are in flight and vice versa.  The buffers are never copied into each other -- a `va = na` rotation at the loop end
  // forces a full s_waitcnt vmcnt(0) on the just-issued prefetch (a register copy needs the loaded data), which is what
  // made the first version of this kernel latency-bound (16 ms per pass at B = 8 for 7.5 ms of HBM time).  With no
  // copies the compiler waits with vmcnt(2 U) for the older buffer only.  npairs % (2 U) == 0 is required (U = 1: any).
  u32x4_t va[U], na[U];
  u32x3_t vb[U], nb[U];
#define SP_BATCH_LOAD(VA, VB, JP0)                                                                        \
  _Pragma("unroll") for (int uu = 0; uu < U; uu++) {                                                      \
    const u32* u = base + (size_t)((JP0) + uu) * ustride;                                                 \
    VA[uu] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(u + lane * 4));                  \
    VB[uu] = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(u + 256 + lane * 3));            \
  }
#define SP_BATCH_MAC16(QA, QB, b)                                                                                        \
  acc[b][0] += (u64)QA.x * f0; acc[b][1] += (u64)QA.z * f0; acc[b][2] += (u64)QA.y * f1; acc[b][3] += (u64)QA.w * f1;     \
  acc[b][4] += (u64)QA.x * f2; acc[b][5] += (u64)QA.z * f2; acc[b][6] += (u64)QA.y * f3; acc[b][7] += (u64)QA.w * f3;     \
  acc[b][0] += (u64)QB.x * f4; acc[b][1] += (u64)QB.z * f4; acc[b][2] += (u64)QB.y * f5; acc[b][3] += (u64)QB.w * f5;     \
  acc[b][4] += (u64)QB.x * f6; acc[b][5] += (u64)QB.z * f6; acc[b][6] += (u64)QB.y * f7; acc[b][7] += (u64)QB.w * f7;
// one row pair at a time (sched_barrier between them: otherwise the scheduler hoists the query reads of every row pair
// of the buffer and the kernel needs > 256 registers).  LDS form: the two query rows of query b+1 are read while query
// b's 16 multiply-accumulates issue.
#define SP_BATCH_MAC(VA, VB, JP0)                                                                                         \
  _Pragma("unroll") for (int uu = 0; uu < U; uu++) {                                                                      \
    const int jp = (JP0) + uu;                                                                                            \
    const u32 d0 = VA[uu].x, d1 = VA[uu].y, d2 = VA[uu].z, d3 = VA[uu].w, d4 = VB[uu].x, d5 = VB[uu].y, d6 = VB[uu].z;    \
    const u32 f0 = d0 & M;                                                                                                \
    const u32 f1 = __builtin_amdgcn_alignbit(d1, d0, 28) & M;                                                             \
    const u32 f2 = __builtin_amdgcn_alignbit(d2, d1, 24) & M;                                                             \
    const u32 f3 = __builtin_amdgcn_alignbit(d3, d2, 20) & M;                                                             \
    const u32 f4 = __builtin_amdgcn_alignbit(d4, d3, 16) & M;                                                             \
    const u32 f5 = __builtin_amdgcn_alignbit(d5, d4, 12) & M;                                                             \
    const u32 f6 = __builtin_amdgcn_alignbit(d6, d5, 8) & M;                                                              \
    const u32 f7 = d6 >> 4;                                                                                               \
    if (QLDS) {                                                                                                           \
      uint4 qa_n = qs[2 * jp], qb_n = qs[2 * jp + 1];                                                                     \
      _Pragma("unroll") for (int b = 0; b < B; b++) {                                                                     \
        const uint4 qa = qa_n, qb = qb_n;                                                                                 \
        if (b + 1 < B) {                                                                                                  \
          qa_n = qs[(b + 1) * QLDS_ROWS + 2 * jp];                                                                        \
          qb_n = qs[(b + 1) * QLDS_ROWS + 2 * jp + 1];                                                                    \
        }                                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                                \
        SP_BATCH_MAC16(qa, qb, b)                                                                                         \
      }                                                                                                                   \
    } else {                                                                                                              \
      _Pragma("unroll") for (int b = 0; b < B; b++) {                                                                     \
        const uint4* __restrict__ qrow = reinterpret_cast<const uint4*>(d.qv[b]) + qoff;                                  \
        const uint4 qa = qrow[2 * jp];                                                                                    \
        const uint4 qb = qrow[2 * jp + 1];                                                                                \
        SP_BATCH_MAC16(qa, qb, b)                                                                                         \
      }                                                                                                                   \
    }                                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }
#define SP_BATCH_FOLD                                                                                     \
  _Pragma("unroll") for (int b = 0; b < B; b++) {                                                         \
    acc[b][0] = reduce64(acc[b][0], m0); acc[b][1] = reduce64(acc[b][1], m0);                             \
    acc[b][2] = reduce64(acc[b][2], m1); acc[b][3] = reduce64(acc[b][3], m1);                             \
    acc[b][4] = reduce64(acc[b][4], m0); acc[b][5] = reduce64(acc[b][5], m0);                             \
    acc[b][6] = reduce64(acc[b][6], m1); acc[b][7] = reduce64(acc[b][7], m1);                             \
  }
  if (U > 1 || (npairs & 1) == 0) {
    // steady state without conditionals (a branch around the reload lets the optimiser sink the multiply-accumulates
    // of buffer A below the reload of A, which then needs a third set of registers); the last 2 U row pairs are peeled
    SP_BATCH_LOAD(va, vb, 0)
    int jp0 = 0;
    for (; jp0 + 2 * U < npairs; jp0 += 2 * U) {
      SP_BATCH_LOAD(na, nb, jp0 + U)
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the multiply-accumulates
      SP_BATCH_MAC(va, vb, jp0)
      SP_BATCH_LOAD(va, vb, jp0 + 2 * U)
      __builtin_amdgcn_sched_barrier(0);
      SP_BATCH_MAC(na, nb, jp0 + U)
      // at most 256 rows (128 row pairs) of < 2^56 products between Barrett folds
      if (((jp0 + 2 * U) & 127) == 0) SP_BATCH_FOLD
    }
    SP_BATCH_LOAD(na, nb, jp0 + U)
    __builtin_amdgcn_sched_barrier(0);
    SP_BATCH_MAC(va, vb, jp0)
    SP_BATCH_MAC(na, nb, jp0 + U)
    SP_BATCH_FOLD
  } else {  // odd number of row pairs (U == 1 only): no pipelining
    for (int jp0 = 0; jp0 < npairs; jp0++) {
      SP_BATCH_LOAD(va, vb, jp0)
      SP_BATCH_MAC(va, vb, jp0)
      if (((jp0 + 1) & 127) == 0 || jp0 + 1 >= npairs) SP_BATCH_FOLD
    }
  }
#undef SP_BATCH_LOAD
#undef SP_BATCH_MAC
#undef SP_BATCH_MAC16
#undef SP_BATCH_FOLD
  const size_t rc = (size_t)N * d.num_per;
  const size_t zi = (size_t)plane * 4 * rc + (size_t)z * d.num_per + (size_t)chunk * 128 + 2 * lane;
#pragma unroll
  for (int b = 0; b < B; b++) {
    u32* o = d.out[b] + zi;
    *reinterpret_cast<uint2*>(o + 0 * rc) = make_uint2((u32)acc[b][0], (u32)acc[b][4]);  // r=0, crt=0
    *reinterpret_cast<uint2*>(o + 1 * rc) = make_uint2((u32)acc[b][2], (u32)acc[b][6]);  // r=0, crt=1
    *reinterpret_cast<uint2*>(o + 2 * rc) = make_uint2((u32)acc[b][1], (u32)acc[b][5]);  // r=1, crt=0
    *reinterpret_cast<uint2*>(o + 3 * rc) = make_uint2((u32)acc[b][3], (u32)acc[b][7]);  // r=1, crt=1
  }
}
static bool mfma_shape_ok(int num_per, int nj) {
  // the matrix-core form needs whole 16-row steps in rings of 2 (nj % 32), the z-row's digit table(s) in LDS (nj <= 512:
  // 64 KiB per tile) and whole 128-column chunks
  return tunable("batch_mfma", 1) != 0 && nj > 0 && (nj % 32) == 0 && nj <= 512 && num_per >= 128 && (num_per % 128) == 0;
}
bool sweep_batch_wants_mfma(const SweepBatchDesc& d) {
  if (d.narrow) return false;   // VALU, no digit table
  // below batch_mfma_min queries per pass the VALU kernel is HBM-bound as well
  return mfma_shape_ok(d.num_per, d.nj) && d.batch >= (int)tunable("batch_mfma_min", 4) && d.batch <= SWEEP_GROUP_MAX &&
         (d.batch <= SWEEP_BATCH_MAX || tunable("batch_mfma_tiles", 2) >= 2);
}
int sweep_batch_group_max(int num_per, int nj) {
  // groups of 9 .. 16 exist only as the two-tile matrix-core pass: with batch_mfma_min above 8 a group of 9 would take the
  // VALU kernel, which stops at 8; and the device has to offer both tiles' z-rows of LDS to one workgroup
  if (!mfma_shape_ok(num_per, nj) || tunable("batch_mfma_tiles", 2) < 2 || tunable("batch_mfma_min", 4) > SWEEP_BATCH_MAX + 1)
    return SWEEP_BATCH_MAX;
  int dev = 0, lds_optin = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds_optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) {
    (void)hipGetLastError();
    return SWEEP_BATCH_MAX;
  }
  return (size_t)lds_optin >= (size_t)nj * 128 * 2 + 256 ? SWEEP_GROUP_MAX : SWEEP_BATCH_MAX;
}
void sweep_batch_prepare(const DevTables& T, SweepBatchDesc& d, hipStream_t s) {
  d.use_mfma = 0;
  if (!d.rq || !sweep_batch_wants_mfma(d)) return;
  // per tile of <= 8 queries: the digit table [tile][N][steps][2][64][4], then (after ALL tables) the offset terms [tile][N][32]
  const int tiles = sweep_batch_tiles(d.batch);
  const size_t entries = (size_t)N * (d.nj >> 4) * 128;
  if (d.planar && tiles == 2 && tunable("batch_tables_merged", 1) != 0) {   // both tiles in one launch each (sweep_planar.hip)
    launch_query_tables_planar2(T, d.qv, d.batch, d.dim0, d.j0, d.nj, d.rq, s);
    d.use_mfma = 1;
    return;
  }
  for (int t = 0; t < tiles; t++) {
    QueryDigitsDesc q{};
    const int nb = std::min(SWEEP_BATCH_MAX, d.batch - t * SWEEP_BATCH_MAX);
    for (int b = 0; b < nb; b++) q.qv[b] = d.qv[t * SWEEP_BATCH_MAX + b];
    q.rq = d.rq + (size_t)t * entries * 4;
    q.batch = nb;
    q.dim0 = d.dim0;
    q.j0 = d.j0;
    q.nj = d.nj;
    if (d.planar && tiles == 2) {   // same size, planar order (sweep_planar.hip)
      launch_query_digits_planar(q, entries, s);
    } else {
      hipLaunchKernelGGL(k_query_digits, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, q);
      launched(0, "k_query_digits");
    }
    hipLaunchKernelGGL(k_query_offset_terms, dim3(N), dim3(256), 0, s, T, q, d.rq + (size_t)tiles * entries * 4 + (size_t)t * N * 32);
    launched(0, "k_query_offset_terms");
  }
  d.use_mfma = 1;
}
static void launch_sweep_mfma(const DevTables& T, const SweepBatchDesc& d, hipStream_t s) {
  if (d.planar && sweep_batch_tiles(d.batch) == 2) {
    launch_sweep_planar(T, d, s);   // sweep_planar.hip
    return;
  }
  SweepMfmaDesc m{};
  m.db = d.db;
  const int tiles = sweep_batch_tiles(d.batch);
  m.rq = d.rq;
  m.rq_off = d.rq + (size_t)tiles * N * (d.nj >> 4) * 128 * 4;
  for (int b = 0; b < d.batch; b++) m.out[b] = d.out[b];
  m.batch = d.batch;
  m.planes = d.planes;
  m.num_per = d.num_per;
  m.nj = d.nj;
  const int chunks = d.num_per >> 7;
  int cpw = (int)tunable("batch_mfma_cpw", 16);
  cpw = std::max(1, std::min(cpw, chunks));
  while (chunks % cpw) cpw--;
  m.cpw = cpw;
  const u64 qs[2] = {MODULUS_0, MODULUS_1};
  for (int c = 0; c < 2; c++) {
    m.c4[c] = (u32)((1ull << 32) % qs[c]);
    m.c5[c] = (u32)((1ull << 40) % qs[c]);
    m.c6[c] = (u32)((1ull << 48) % qs[c]);
  }
  const dim3 grid((unsigned)((size_t)d.planes * N * (chunks / cpw)));
  if (tiles == 2) {
    // sixteen queries per pass (r04): both tiles' z-rows in LDS (128 KiB at nj = 512: one workgroup per CU, 224 accumulator
    // registers in AGPRs), the load ring as deep as the step count allows (one wave per SIMD has to keep the HBM pipe full
    // alone).  Measured (scripts/ubench/mfma_sweep.hip, profiles/r04_mfma_two_tiles.md): 4.19 ms per C2 plane for 16 queries
    // against 2.95 for 8 -- 1.05 instead of 1.48 ms of database pass per query.
    const size_t lds2 = (size_t)d.nj * 128 * 2 + 256;   // both tiles' digit tables of a z-row + their 16 x 16 bytes of offset terms
    const int steps = d.nj >> 4;
#define SP_MFMA2(NB_)                                                                                                  \
  {                                                                                                                    \
    /* more than 64 KiB of dynamic LDS: the limit belongs to the function ON THE CURRENT DEVICE, so it is raised on every */ \
    /* launch (a cached "already raised" would be wrong after sp_set_device; the call costs a microsecond) and checked    */ \
    if (lds2 > 65536)                                                                                                  \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_mfma_batch<NB_, 1, 0, 2>),                  \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));                           \
    hipLaunchKernelGGL((k_sweep_mfma_batch<NB_, 1, 0, 2>), grid, dim3(256), lds2, s, T, m);                            \
  }
    if (steps % 8 == 0) SP_MFMA2(8) else if (steps % 4 == 0) SP_MFMA2(4) else SP_MFMA2(2)
#undef SP_MFMA2
    launched(PATH_SWEEP_BATCH | PATH_SWEEP_MFMA | PATH_SWEEP_MFMA2, "k_sweep_mfma_batch (two query tiles)");
    return;
  }
  const size_t lds = (size_t)d.nj * 128;  // one z-row of the group's query digit table
  if (lds > 65536)
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_mfma_batch<2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // ring of 2 load buffers (one 16-row step ahead, 180 VGPRs); a ring of 4 measured the same +-2 % at 236 VGPRs (r03)
  hipLaunchKernelGGL((k_sweep_mfma_batch<2, 2>), grid, dim3(256), lds, s, T, m);
  launched(PATH_SWEEP_BATCH | PATH_SWEEP_MFMA, "k_sweep_mfma_batch");
}
void launch_sweep_batch(const DevTables& T, const SweepBatchDesc& d, hipStream_t s) {
  if (d.narrow) {   // the 8-byte narrow layout: its own kernel and translation unit (sweep_planar.hip)
    launch_sweep_narrow_batch(T, d, s);
    return;
  }
  if (d.use_mfma && d.rq) {
    launch_sweep_mfma(T, d, s);
    return;
  }
  if (d.batch > SWEEP_BATCH_MAX) throw HipError("internal: a group of more than 8 queries needs the matrix-core pass");
  const long units = (long)d.planes * N * (d.num_per >> 7);
  const dim3 grid((unsigned)((units + 3) / 4));
  const bool unroll = ((d.nj >> 1) % 8) == 0;  // U = 4 (and the U = 2 LDS form) run ping-pong: npairs % (2 U) == 0
  const int lds_min_b = (int)tunable("batch_qlds_min", 4);
  const bool qlds = unroll && ((d.num_per >> 7) % 4) == 0 && d.batch >= lds_min_b && d.nj <= QLDS_ROWS;
  const size_t lds = qlds ? (size_t)d.batch * QLDS_ROWS * 16 : 0;
#define SP_BATCH_CASE(B)                                                                              \
  case B:                                                                                             \
    if (qlds)                                          /* two row pairs per ping-pong buffer */       \
      hipLaunchKernelGGL((k_sweep_packed_batch<B, 2, true>), grid, dim3(256), lds, s, T, d);          \
    else if (unroll)                                                                                  \
      hipLaunchKernelGGL((k_sweep_packed_batch<B, 4, false>), grid, dim3(256), 0, s, T, d);           \
    else                                                                                              \
      hipLaunchKernelGGL((k_sweep_packed_batch<B, 1, false>), grid, dim3(256), 0, s, T, d);           \
    break;
  switch (d.batch) {
    SP_BATCH_CASE(1) SP_BATCH_CASE(2) SP_BATCH_CASE(3) SP_BATCH_CASE(4)
    SP_BATCH_CASE(5) SP_BATCH_CASE(6) SP_BATCH_CASE(7) SP_BATCH_CASE(8)
    default: break;
  }
#undef SP_BATCH_CASE
  launched(PATH_SWEEP_BATCH, "k_sweep_packed_batch");
}


// NARROW (num_per <= 64): one workgroup per (plane, z).  The nj*num_per words of the row block are
// contiguous; thread tau reads word tau + 256*s, i.e. fixed ii = tau % num_per and rows
// j = tau/num_per + s*(256/num_per).  Query limbs for this z are staged in LDS (16 B per row);
// partial sums are Barrett-folded to < 2^28 and combined through LDS.
__global__ __launch_bounds__(256) void k_sweep_narrow(DevTables T, SweepDesc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* qs = reinterpret_cast<uint4*>(smem);                          // [nj]
  u32* red = reinterpret_cast<u32*>(smem + (size_t)d.nj * sizeof(uint4));  // [256][4]
  const int tau = threadIdx.x;
  const int zp = blockIdx.x;
  const int z = zp & (N - 1);
  const int plane = zp >> POLY_LEN_LOG2;
  const uint4* qrow = reinterpret_cast<const uint4*>(d.qv) + ((size_t)z * d.dim0 + d.j0);
  for (int j = tau; j < d.nj; j += 256) qs[j] = qrow[j];
  __syncthreads();
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const u64* p = d.db + (size_t)zp * d.nj * d.num_per;
  const int L = d.nj * d.num_per;
  const int np_log = __ffs(d.num_per) - 1;
  u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  int cnt = 0;
  for (int f = tau; f < L; f += 256) {
    const u64 w = p[f];
    const uint4 qa = qs[f >> np_log];
    const u32 bl = (u32)w, bh = (u32)(w >> 32);
    a0 += (u64)qa.x * bl;
    a1 += (u64)qa.z * bl;
    a2 += (u64)qa.y * bh;
    a3 += (u64)qa.w * bh;
    if (++cnt == 255) {
      cnt = 0;
      a0 = reduce64(a0, m0);
      a1 = reduce64(a1, m0);
      a2 = reduce64(a2, m1);
      a3 = reduce64(a3, m1);
    }
  }
  red[tau * 4 + 0] = reduce64(a0, m0);
  red[tau * 4 + 1] = reduce64(a1, m0);
  red[tau * 4 + 2] = reduce64(a2, m1);
  red[tau * 4 + 3] = reduce64(a3, m1);
  __syncthreads();
  // 4*num_per outputs; thread t < 4*num_per: which = t / num_per, ii = t % num_per
  if (tau < 4 * d.num_per) {
    const int which = tau >> np_log, ii = tau & (d.num_per - 1);
    u64 sacc = 0;
    for (int t2 = ii; t2 < 256; t2 += d.num_per) sacc += red[t2 * 4 + which];
    const u32 r = reduce64(sacc, which < 2 ? m0 : m1);
    // which: 0 n0_0 (r0,c0)  1 n0_1 (r1,c0)  2 n1_0 (r0,c1)  3 n1_1 (r1,c1)
    const int rr = which & 1, cc = which >> 1;
    d.out[sweep_out_index(d, plane, rr * 2 + cc, z, ii)] = r;
  }
}

// NARROW with 16-byte non-temporal loads (2 <= num_per <= 64): thread tau reads words 2 tau, 2 tau + 1 (+512 s):
// the same row j, columns ii0 = (2 tau) % num_per and ii0 + 1.
__global__ __launch_bounds__(256) void k_sweep_narrow2(DevTables T, SweepDesc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* qs = reinterpret_cast<uint4*>(smem);                              // [nj]
  u32* red = reinterpret_cast<u32*>(smem + (size_t)d.nj * sizeof(uint4));  // [256][8]
  const int tau = threadIdx.x;
  const int zp = blockIdx.x;
  const int z = zp & (N - 1);
  const int plane = zp >> POLY_LEN_LOG2;
  const uint4* qrow = reinterpret_cast<const uint4*>(d.qv) + ((size_t)z * d.dim0 + d.j0);
  for (int j = tau; j < d.nj; j += 256) qs[j] = qrow[j];
  __syncthreads();
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const u64* p = d.db + (size_t)zp * d.nj * d.num_per;
  const int L = d.nj * d.num_per;
  const int np_log = __ffs(d.num_per) - 1;
  u64 a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int cnt = 0;
  for (int f = 2 * tau; f < L; f += 512) {
    ulonglong2 w;
    w.x = __builtin_nontemporal_load(p + f);
    w.y = __builtin_nontemporal_load(p + f + 1);
    const uint4 qa = qs[f >> np_log];
    const u32 b0l = (u32)w.x, b0h = (u32)(w.x >> 32), b1l = (u32)w.y, b1h = (u32)(w.y >> 32);
    a[0] += (u64)qa.x * b0l; a[1] += (u64)qa.z * b0l; a[2] += (u64)qa.y * b0h; a[3] += (u64)qa.w * b0h;
    a[4] += (u64)qa.x * b1l; a[5] += (u64)qa.z * b1l; a[6] += (u64)qa.y * b1h; a[7] += (u64)qa.w * b1h;
    if (++cnt == 255) {
      cnt = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) a[i] = reduce64(a[i], (i & 2) ? m1 : m0);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) red[tau * 8 + i] = reduce64(a[i], (i & 2) ? m1 : m0);
  __syncthreads();
  if (tau < 4 * d.num_per) {
    const int which = tau >> np_log, ii = tau & (d.num_per - 1);
    const int slot = (ii & 1) * 4 + which, first = ii >> 1, step = d.num_per >> 1;
    u64 sacc = 0;
    for (int t2 = first; t2 < 256; t2 += step) sacc += red[t2 * 8 + slot];
    const u32 r = reduce64(sacc, which < 2 ? m0 : m1);
    const int rr = which & 1, cc = which >> 1;
    d.out[sweep_out_index(d, plane, rr * 2 + cc, z, ii)] = r;
  }
}

void launch_sweep(const DevTables& T, const SweepDesc& d, hipStream_t s) {
  if (d.packed) {  // persistent grid (ring form where the row-pair count allows), sweep_persist_wgs workgroups per CU for the plain form
    launch_sweep_persist(T, d, (int)std::max(1L, tunable("sweep_persist_wgs", 4)), s);
    return;
  }
  if (d.num_per >= 128) {
    const long units = (long)d.planes * N * (d.num_per >> 7);
    hipLaunchKernelGGL(k_sweep_wide, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, T, d);
    launched(PATH_SWEEP_WIDE | (d.out_G > 1 ? PATH_SCATTER_OUT : 0), "k_sweep_wide");
  } else {
    if (d.num_per >= 2) {
      size_t sh = (size_t)d.nj * sizeof(uint4) + 256 * 8 * sizeof(u32);
      hipLaunchKernelGGL(k_sweep_narrow2, dim3((unsigned)(d.planes * N)), dim3(256), sh, s, T, d);
    } else {  // num_per == 1 (nu_2 = 0): one word per row, 8-byte loads
      size_t sh = (size_t)d.nj * sizeof(uint4) + 256 * 4 * sizeof(u32);
      hipLaunchKernelGGL(k_sweep_narrow, dim3((unsigned)(d.planes * N)), dim3(256), sh, s, T, d);
    }
    launched(PATH_SWEEP_NARROW | (d.out_G > 1 ? PATH_SCATTER_OUT : 0), "k_sweep_narrow");
  }
}

}  // namespace spiral
