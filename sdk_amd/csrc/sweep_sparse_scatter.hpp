// The sparse bucket's first-dimension multiply on a ROW SHARD, output in the reduce-scatter layouts of G ranks (included by sparse.hip
// after k_sweep_sparse / k_sweep_sparse_batch, whose loads and arithmetic these kernels repeat; only the stores differ).
//
// Column ii belongs to rank g = ii % G, which receives the SUM of every rank's chunk g and folds it relying on zeros for absent
// columns: a shard therefore writes every word of its partial buffer, zeros included (an empty column, an empty shard).  With
// npl = num_per / G, word (plane, rc = 2 r + crt, z, ii) goes to
//   out + plane * plane_stride + (ii % G) * chunk_stride + (rc * N + z) * npl + ii / G
// and one pair of strides covers both exchange forms:
//   chunk-major (sp_query_sweep_scatter):             plane_stride = 4 N npl,      chunk_stride = planes 4 N npl
//   per-plane   (sp_query_sweep_scatter_plane/_group): plane_stride = 4 N num_per,  chunk_stride = 4 N npl
// grid (num_per, planes of the launch, N / (256 ZT)): as in k_sweep_sparse_batch thread tau of z-slab s owns the ZT consecutive z
// from (256 s + tau) ZT, so that a launch of ONE plane (num_per workgroups per slab: 128 at nu_2 = 7, on 256 CUs) still fills the
// chip.  `plane0` is the first plane of the launch (item polynomials and plane_stride count from plane 0).
// Exact sums as in k_sweep_sparse: products < 2^56, a Barrett fold after every 255 items of a column (a folded sum is < q < 2^28:
// 255 * 2^56 + 2^28 < 2^64), canonical residues out.  The innermost run of the layout is ii / G: one word per workgroup.
#pragma once

namespace spiral {

struct SparseScatter {
  size_t plane_stride, chunk_stride;   // in u32 words
  int G, npl;
};

__global__ __launch_bounds__(256) void k_sweep_sparse_scatter(DevTables T, const int* col_ptr, const int* col_rows, const int* col_slots,
                                                              const u64* polys, int planes, int plane0, const u32* v, int first, int step,
                                                              u32* out, SparseScatter L) {
  constexpr int ZT = 2;
  const int ii = blockIdx.x, plane = plane0 + (int)blockIdx.y;
  const int z0 = ((int)blockIdx.z * 256 + (int)threadIdx.x) * ZT;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  u64 a[4][ZT];
#pragma unroll
  for (int rc = 0; rc < 4; rc++)
#pragma unroll
    for (int k = 0; k < ZT; k++) a[rc][k] = 0;
  const int e1 = col_ptr[ii + 1];
  for (int e = col_ptr[ii]; e < e1;) {
    const int stop = e1 - e > 255 ? e + 255 : e1;
    for (; e < stop; e++) {
      const u64* ip = polys + ((size_t)col_slots[e] * planes + plane) * N + z0;
      const u32* q = v + (size_t)(first + step * col_rows[e]) * 4 * N + z0;  // [r][crt][z], GLOBAL row
      const sp_u64x2_t w = *reinterpret_cast<const sp_u64x2_t*>(ip);
      const u32 bl[ZT] = {(u32)w.x, (u32)w.y}, bh[ZT] = {(u32)(w.x >> 32), (u32)(w.y >> 32)};
#pragma unroll
      for (int rc = 0; rc < 4; rc++) {   // r0 crt0, r0 crt1, r1 crt0, r1 crt1
        const sp_u32x2_t t = *reinterpret_cast<const sp_u32x2_t*>(q + rc * N);
        a[rc][0] += (u64)t.x * ((rc & 1) ? bh[0] : bl[0]);
        a[rc][1] += (u64)t.y * ((rc & 1) ? bh[1] : bl[1]);
      }
    }
#pragma unroll
    for (int rc = 0; rc < 4; rc++)
#pragma unroll
      for (int k = 0; k < ZT; k++) a[rc][k] = reduce64(a[rc][k], (rc & 1) ? m1 : m0);
  }
  u32* o = out + (size_t)plane * L.plane_stride + (size_t)(ii % L.G) * L.chunk_stride + (size_t)z0 * L.npl + ii / L.G;
  const size_t rc_words = (size_t)N * L.npl;
#pragma unroll
  for (int rc = 0; rc < 4; rc++)
#pragma unroll
    for (int k = 0; k < ZT; k++) o[rc * rc_words + (size_t)k * L.npl] = (u32)a[rc][k];
}

// ... and for a group of queries in ONE pass over the shard: k_sweep_sparse_batch<B> with the stores above.  A group of nq < B members
// runs the B body with DEAD slots (they read member 0's rows and store nothing).
template <int B>
__global__ __launch_bounds__(256) void k_sweep_sparse_scatter_batch(DevTables T, const int* col_ptr, const int* col_rows,
                                                                    const int* col_slots, const u64* polys, int planes, SparseGroup g,
                                                                    int nq, int first, int step, SparseScatter L) {
  constexpr int ZT = B == 2 ? 4 : 2;
  const int ii = blockIdx.x, plane = blockIdx.y;
  const int z0 = ((int)blockIdx.z * 256 + (int)threadIdx.x) * ZT;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  u64 a[B][4][ZT];
#pragma unroll
  for (int b = 0; b < B; b++)
#pragma unroll
    for (int rc = 0; rc < 4; rc++)
#pragma unroll
      for (int k = 0; k < ZT; k++) a[b][rc][k] = 0;
  const int e1 = col_ptr[ii + 1];
  for (int e = col_ptr[ii]; e < e1;) {
    const int stop = e1 - e > 255 ? e + 255 : e1;
    for (; e < stop; e++) {
      const u64* ip = polys + ((size_t)col_slots[e] * planes + plane) * N + z0;
      const size_t qo = (size_t)(first + step * col_rows[e]) * 4 * N + z0;  // [r][crt][z], GLOBAL row
      u32 bl[ZT], bh[ZT];
#pragma unroll
      for (int k = 0; k < ZT; k += 2) {
        const sp_u64x2_t w = __builtin_nontemporal_load(reinterpret_cast<const sp_u64x2_t*>(ip + k));
        bl[k] = (u32)w.x; bh[k] = (u32)(w.x >> 32);
        bl[k + 1] = (u32)w.y; bh[k + 1] = (u32)(w.y >> 32);
      }
#pragma unroll
      for (int b = 0; b < B; b++) {
        const u32* q = g.v[b] + qo;
#pragma unroll
        for (int rc = 0; rc < 4; rc++) {
          u32 x[ZT];
          if constexpr (ZT == 4) {
            const sp_u32x4_t t = *reinterpret_cast<const sp_u32x4_t*>(q + rc * N);
            x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
          } else {
            const sp_u32x2_t t = *reinterpret_cast<const sp_u32x2_t*>(q + rc * N);
            x[0] = t.x; x[1] = t.y;
          }
#pragma unroll
          for (int k = 0; k < ZT; k++) a[b][rc][k] += (u64)x[k] * ((rc & 1) ? bh[k] : bl[k]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < B; b++)
#pragma unroll
      for (int rc = 0; rc < 4; rc++)
#pragma unroll
        for (int k = 0; k < ZT; k++) a[b][rc][k] = reduce64(a[b][rc][k], (rc & 1) ? m1 : m0);
  }
  const size_t o0 = (size_t)plane * L.plane_stride + (size_t)(ii % L.G) * L.chunk_stride + (size_t)z0 * L.npl + ii / L.G;
  const size_t rc_words = (size_t)N * L.npl;
#pragma unroll
  for (int b = 0; b < B; b++) {
    if (b >= nq) break;
    u32* o = g.out[b] + o0;
#pragma unroll
    for (int rc = 0; rc < 4; rc++)
#pragma unroll
      for (int k = 0; k < ZT; k++) o[rc * rc_words + (size_t)k * L.npl] = (u32)a[b][rc][k];
  }
}

// G shards, `per_plane` = the per-plane exchange form (else chunk-major); num_per % G == 0 is the caller's (need_shard_count)
static SparseScatter sparse_scatter_layout(int planes, int num_per, int G, bool per_plane) {
  const int npl = num_per / G;
  const size_t chunk = (size_t)4 * N * npl;   // [r][crt][z][ii / G] of one plane
  return per_plane ? SparseScatter{chunk * (size_t)G, chunk, G, npl} : SparseScatter{chunk, chunk * (size_t)planes, G, npl};
}

void launch_sweep_sparse_scatter(const DevTables& T, const int* col_ptr, const int* col_rows, const int* col_slots, const u64* polys,
                                 int planes, int plane0, int n_planes, const u32* v, int first, int step, u32* out, int num_per, int G,
                                 bool per_plane, hipStream_t s) {
  hipLaunchKernelGGL(k_sweep_sparse_scatter, dim3(num_per, n_planes, N / (256 * 2)), dim3(256), 0, s, T, col_ptr, col_rows, col_slots,
                     polys, planes, plane0, v, first, step, out, sparse_scatter_layout(planes, num_per, G, per_plane));
  launched(PATH_SWEEP_SPARSE | PATH_SCATTER_OUT, "k_sweep_sparse_scatter");
}

template <int B>
static void launch_sweep_sparse_scatter_batch_b(const DevTables& T, const int* col_ptr, const int* col_rows, const int* col_slots,
                                                const u64* polys, int planes, const SparseGroup& g, int nq, int first, int step,
                                                int num_per, const SparseScatter& L, hipStream_t s) {
  constexpr int ZT = B == 2 ? 4 : 2;
  hipLaunchKernelGGL(k_sweep_sparse_scatter_batch<B>, dim3(num_per, planes, N / (256 * ZT)), dim3(256), 0, s, T, col_ptr, col_rows,
                     col_slots, polys, planes, g, nq, first, step, L);
}
// every plane of 1 <= nq <= SPARSE_GROUP_MAX members, per-plane exchange form (the caller checks nq)
void launch_sweep_sparse_scatter_batch(const DevTables& T, const int* col_ptr, const int* col_rows, const int* col_slots, const u64* polys,
                                       int planes, const SparseGroup& members, int nq, int first, int step, int num_per, int G,
                                       hipStream_t s) {
  SparseGroup g = members;
  for (int b = nq; b < SPARSE_GROUP_MAX; b++) {   // dead slots: valid rows to read, never stored
    g.v[b] = g.v[0];
    g.out[b] = nullptr;
  }
  const SparseScatter L = sparse_scatter_layout(planes, num_per, G, true);
  if (nq <= 2)
    launch_sweep_sparse_scatter_batch_b<2>(T, col_ptr, col_rows, col_slots, polys, planes, g, nq, first, step, num_per, L, s);
  else if (nq <= 4)
    launch_sweep_sparse_scatter_batch_b<4>(T, col_ptr, col_rows, col_slots, polys, planes, g, nq, first, step, num_per, L, s);
  else
    launch_sweep_sparse_scatter_batch_b<8>(T, col_ptr, col_rows, col_slots, polys, planes, g, nq, first, step, num_per, L, s);
  launched(PATH_SWEEP_SPARSE | PATH_SCATTER_OUT | PATH_SWEEP_SPARSE_GROUP, "k_sweep_sparse_scatter_batch");
}

}  // namespace spiral
