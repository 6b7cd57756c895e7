// One pass over a NARROW database (8-byte words u64 [plane][z][j][ii], 2 <= num_per <= 64, unsharded) for a group of up to 8
// queries: k_sweep_narrow2's work split -- one 256-thread workgroup per (plane, z); thread tau loads words 2 tau, 2 tau + 1
// (+ 512 s) of the row block with one 16-byte non-temporal load, i.e. one row j and the columns ii0 = (2 tau) % num_per, ii0 + 1 --
// with every database word loaded ONCE per group and multiplied into every member's four (r, crt) sums.  Member b reads its own
// reoriented query d.qv[b] ([z][dim0] limb quads of 16 bytes) and writes its own sweep buffer d.out[b], unscattered
// ([plane][r * 2 + crt][z][ii], residues < q): exactly what k_sweep_narrow2 leaves there, so everything after the pass is the
// per-query flow's.
//
// Query limbs: the group's limb quads for this z are staged in LDS as [member][row] with a fixed stride of NARROW_SLAB_ROWS = 512
// rows per member (a compile-time stride: one base register + an immediate offset per member).  The rows are walked in slabs of at
// most 512, restaged per slab between two barriers, so any nj works and the staging is B x 8 KiB.
// Sums: 8 u64 per member and thread (2 columns x 4 (r, crt)): 16 VGPRs per member, 128 at B = 8.  A product of two residues is
// < (q - 1)^2 < 2^56, a folded sum is < q < 2^28, and fold_every <= 255 products are added between Barrett folds:
//   255 * (q - 1)^2 + q  <  255 * 2^56 + 2^28  <  2^64,
// so no sum wraps.  d.fold_every (switch narrow_batch_fold_every, default 255, clamped to 1 .. 255 by the launcher) exists so that
// the fold branch runs at test shapes: a thread adds nj * num_per / 512 products per sum, 64 at nu = (9, 6).
// Reduction: across the threads that share a column through LDS, ONE member at a time through one [256][8] u32 area (two barriers
// per member), with k_sweep_narrow2's summation -- canonical residues either way, so the words are the per-query kernel's.
// A group of nq < B members runs the B body with DEAD slots: the launcher points their query at member 0's and the kernel stores
// nothing for b >= d.batch.
//
// Resources (pinned by tests/test_narrow_batch_kernel_resources.py): no scratch, no spilled register; at most 88 / 128 / 208 VGPRs
// at B = 2 / 4 / 8 (two waves per SIMD at B = 8: what the LDS admits anyway); no static LDS, dynamic LDS B * 8 KiB + 8 KiB =
// 24 / 40 / 72 KiB: within 80 KiB, so two workgroups fit a CU at B = 8.
// Its own header, instantiated in sweep_planar.hip only: sweep.hip's kernels keep their machine code.
#pragma once
#include "device_common.hpp"
#include "kernels.hpp"

namespace spiral {

constexpr int NARROW_SLAB_ROWS = 512;
inline size_t sweep_narrow_batch_lds(int B) { return (size_t)B * NARROW_SLAB_ROWS * 16 + 256 * 8 * sizeof(u32); }

typedef u64 nb_u64x2_t __attribute__((ext_vector_type(2)));

// the workgroup of unit zp = plane * N + z
template <int B>
__device__ __forceinline__ void sweep_narrow_batch_unit(const DevTables& T, const SweepBatchDesc& d, const int zp, unsigned char* smem) {
  uint4* qs = reinterpret_cast<uint4*>(smem);                                              // [B][NARROW_SLAB_ROWS]
  u32* red = reinterpret_cast<u32*>(smem + (size_t)B * NARROW_SLAB_ROWS * sizeof(uint4));  // [256][8]
  const int tau = threadIdx.x;
  const int z = zp & (N - 1);
  const int plane = zp >> POLY_LEN_LOG2;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  const int np_log = __ffs(d.num_per) - 1;
  const u64* p = d.db + (size_t)zp * d.nj * d.num_per;
  const size_t qrow0 = (size_t)z * d.dim0 + d.j0;
  const int fold_every = d.fold_every;
  u64 a[B][8];
#pragma unroll
  for (int b = 0; b < B; b++)
#pragma unroll
    for (int i = 0; i < 8; i++) a[b][i] = 0;
#define SP_NB_MAC(W, ROW)                                                                                              \
  {                                                                                                                    \
    const u32 b0l = (u32)(W).x, b0h = (u32)((W).x >> 32), b1l = (u32)(W).y, b1h = (u32)((W).y >> 32);                  \
    _Pragma("unroll") for (int b = 0; b < B; b++) {                                                                    \
      const uint4 qa = qs[b * NARROW_SLAB_ROWS + (ROW)];                                                               \
      a[b][0] += (u64)qa.x * b0l; a[b][1] += (u64)qa.z * b0l; a[b][2] += (u64)qa.y * b0h; a[b][3] += (u64)qa.w * b0h;  \
      a[b][4] += (u64)qa.x * b1l; a[b][5] += (u64)qa.z * b1l; a[b][6] += (u64)qa.y * b1h; a[b][7] += (u64)qa.w * b1h;  \
    }                                                                                                                  \
  }
  int since = 0;   // products added to every sum since its last fold
  for (int j0 = 0; j0 < d.nj; j0 += NARROW_SLAB_ROWS) {
    const int rows = min(NARROW_SLAB_ROWS, d.nj - j0);
    if (j0 > 0) __syncthreads();   // the previous slab's rows have been read
#pragma unroll
    for (int b = 0; b < B; b++) {
      const uint4* src = reinterpret_cast<const uint4*>(d.qv[b]) + qrow0 + j0;
      for (int j = tau; j < rows; j += 256) qs[b * NARROW_SLAB_ROWS + j] = src[j];
    }
    __syncthreads();
    // this thread's words of the slab: 2 tau + 512 s < rows * num_per, s < n_it
    const int Ls = rows << np_log;
    const u64* ps = p + ((size_t)j0 << np_log) + 2 * tau;
    const int n_it = 2 * tau < Ls ? (Ls - 2 * tau + 511) >> 9 : 0;
    for (int s = 0; s < n_it;) {
      const int stop = min(n_it, s + fold_every - since);
      since += stop - s;
      for (; s + 4 <= stop; s += 4) {   // four loads in flight
        nb_u64x2_t w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = __builtin_nontemporal_load(reinterpret_cast<const nb_u64x2_t*>(ps + (size_t)(s + u) * 512));
#pragma unroll
        for (int u = 0; u < 4; u++) {
          SP_NB_MAC(w[u], (2 * tau + (s + u) * 512) >> np_log)
          __builtin_amdgcn_sched_barrier(0);   // one word at a time: the members' query rows of all four would not fit the registers
        }
      }
      for (; s < stop; s++) {
        const nb_u64x2_t w = __builtin_nontemporal_load(reinterpret_cast<const nb_u64x2_t*>(ps + (size_t)s * 512));
        SP_NB_MAC(w, (2 * tau + s * 512) >> np_log)
      }
      if (since >= fold_every) {
        since = 0;
#pragma unroll
        for (int b = 0; b < B; b++)
#pragma unroll
          for (int i = 0; i < 8; i++) a[b][i] = reduce64(a[b][i], (i & 2) ? m1 : m0);
      }
    }
  }
#undef SP_NB_MAC
  // 4 * num_per outputs per member; thread t < 4 * num_per: which = t / num_per (0 r0 c0, 1 r1 c0, 2 r0 c1, 3 r1 c1), ii = t % num_per
  const int which = tau >> np_log, ii = tau & (d.num_per - 1);
  const int slot = (ii & 1) * 4 + which, first = ii >> 1, step = d.num_per >> 1;
  const int rr = which & 1, cc = which >> 1;
  const size_t oi = (((size_t)plane * 4 + (rr * 2 + cc)) * N + z) * d.num_per + ii;
#pragma unroll
  for (int b = 0; b < B; b++) {
    if (b >= d.batch) break;   // dead slots store nothing (uniform: every thread leaves here)
    if (b > 0) __syncthreads();   // the previous member's sums have been read
#pragma unroll
    for (int i = 0; i < 8; i++) red[tau * 8 + i] = reduce64(a[b][i], (i & 2) ? m1 : m0);
    __syncthreads();
    if (tau < 4 * d.num_per) {
      u64 sacc = 0;
      for (int t2 = first; t2 < 256; t2 += step) sacc += red[t2 * 8 + slot];
      d.out[b][oi] = reduce64(sacc, which < 2 ? m0 : m1);
    }
  }
}

template <int B>
__global__ __launch_bounds__(256, 2) void k_sweep_narrow_batch(DevTables T, SweepBatchDesc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_q[];
  sweep_narrow_batch_unit<B>(T, d, (int)blockIdx.x, smem_q);
}

}  // namespace spiral
