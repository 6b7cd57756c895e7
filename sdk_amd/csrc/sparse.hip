// Sparse buckets: lib/server's SparseDb caller (lib/server/src/db/sparse_db.rs:5-48,
// db/loading.rs:278-359, compute/dot_product.rs:13-220).  Only present items are stored (one packed polynomial per
// (item, plane)) and only they are multiplied: the first-dimension sweep costs time in proportion to the occupancy.
#include "device_common.hpp"

namespace spiral {

// ---- update_item_raw (loading.rs:317-359): one item -> `planes` packed NTT polynomials in its slot -------------------
// grid (planes): chunk `plane` of the item's bytes -> log2(p)-bit coefficients (util.rs:289-301; lib/server asserts
// 8 bits, loading.rs:290) -> recenter_mod (arith.rs:415-427) -> forward NTT mod q0, q1 -> lo | hi << 32.
__global__ __launch_bounds__(256) void k_sparse_item_encode(DevTables T, const uint8_t* bytes, int item_bytes,
                                                            int bytes_per_chunk, int logp, u32 pt_modulus, u64* slot_polys) {
  __shared__ u32 lds0[LDS_WORDS];
  __shared__ u32 lds1[LDS_WORDS];
  const int tau = threadIdx.x, plane = blockIdx.x;
  const int pos = plane * bytes_per_chunk;
  const int avail = item_bytes - pos;
  const int bytes_read = avail < 0 ? 0 : (avail < bytes_per_chunk ? avail : bytes_per_chunk);
  const int words_read = (bytes_read * 8 + logp - 1) / logp;
  u32 coeff[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int z = tau + 256 * k;
    u32 x = 0;
    if (z < words_read) {
      const int bit = z * logp, b0 = bit >> 3, sh = bit & 7, nb = (sh + logp + 7) >> 3;
      u64 acc = 0;
      for (int i = 0; i < nb; i++) acc |= (u64)(b0 + i < bytes_read ? bytes[pos + b0 + i] : 0) << (8 * i);
      x = (u32)((acc >> sh) & ((1ULL << logp) - 1ULL));
    }
    coeff[k] = x;
  }
  u32 lo[8];
  u32* la = lds0;
  u32* lb = lds1;
#pragma unroll 1
  for (int c = 0; c < 2; c++) {
    const ModConst m = T.c.mod[c];
    u32 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = coeff[k] > pt_modulus / 2 ? m.q - (pt_modulus - coeff[k]) : coeff[k];
    const u32* fw = T.tw + (size_t)c * 4 * N;
    if (c == 1) __syncthreads();
    ntt_fwd_block(v, tau, la, lb, fw, fw + N, m.q, m.two_q);
    if (c == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) lo[k] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) slot_polys[(size_t)plane * N + 8 * tau + k] = (u64)lo[k] | ((u64)v[k] << 32);
    }
  }
}
void launch_sparse_item_encode(const DevTables& T, const uint8_t* bytes, int item_bytes, int bytes_per_chunk, int logp,
                               u32 pt_modulus, u64* slot_polys, int planes, hipStream_t s) {
  hipLaunchKernelGGL(k_sparse_item_encode, dim3(planes), dim3(256), 0, s, T, bytes, item_bytes, bytes_per_chunk, logp,
                     pt_modulus, slot_polys);
  launched(0, "k_sparse_item_encode");
}

// ---- update_many_items (loading.rs:361-377): k_sparse_item_encode with the item as a grid dimension -------------------
// grid (n_items * planes): (item, plane) flattened along x, the item count being unbounded.  Item e's bytes are items[e].len bytes at
// win + items[e].off (not padded: what lies past them reads as zero, which is what the single-item form finds in its zero-padded
// upload), its polynomials go to slot items[e].slot.  The arithmetic is k_sparse_item_encode's.
__global__ __launch_bounds__(256) void k_sparse_items_encode(DevTables T, const uint8_t* win, const SparseItemRec* items, int planes,
                                                             int item_bytes, int bytes_per_chunk, int logp, u32 pt_modulus, u64* polys) {
  __shared__ u32 lds0[LDS_WORDS];
  __shared__ u32 lds1[LDS_WORDS];
  const int tau = threadIdx.x, plane = (int)(blockIdx.x % (unsigned)planes);
  const SparseItemRec it = items[blockIdx.x / (unsigned)planes];
  const uint8_t* bytes = win + it.off;
  u64* slot_polys = polys + (size_t)it.slot * planes * N;
  const int pos = plane * bytes_per_chunk;
  const int avail = item_bytes - pos;
  const int bytes_read = avail < 0 ? 0 : (avail < bytes_per_chunk ? avail : bytes_per_chunk);
  const int words_read = (bytes_read * 8 + logp - 1) / logp;
  const int have = it.len - pos;   // bytes of this chunk that the record carries (<= 0: none)
  u32 coeff[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int z = tau + 256 * k;
    u32 x = 0;
    if (z < words_read) {
      const int bit = z * logp, b0 = bit >> 3, sh = bit & 7, nb = (sh + logp + 7) >> 3;
      u64 acc = 0;
      for (int i = 0; i < nb; i++) acc |= (u64)(b0 + i < bytes_read && b0 + i < have ? bytes[pos + b0 + i] : 0) << (8 * i);
      x = (u32)((acc >> sh) & ((1ULL << logp) - 1ULL));
    }
    coeff[k] = x;
  }
  u32 lo[8];
  u32* la = lds0;
  u32* lb = lds1;
#pragma unroll 1
  for (int c = 0; c < 2; c++) {
    const ModConst m = T.c.mod[c];
    u32 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = coeff[k] > pt_modulus / 2 ? m.q - (pt_modulus - coeff[k]) : coeff[k];
    const u32* fw = T.tw + (size_t)c * 4 * N;
    if (c == 1) __syncthreads();
    ntt_fwd_block(v, tau, la, lb, fw, fw + N, m.q, m.two_q);
    if (c == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) lo[k] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) slot_polys[(size_t)plane * N + 8 * tau + k] = (u64)lo[k] | ((u64)v[k] << 32);
    }
  }
}
void launch_sparse_items_encode(const DevTables& T, const uint8_t* win, const SparseItemRec* items, size_t n_items, int item_bytes,
                                int bytes_per_chunk, int logp, u32 pt_modulus, u64* polys, int planes, hipStream_t s) {
  if (n_items == 0) return;   // (n_items * planes <= UPSERT_MAX_GROUP_PLANES = 2^23: the caller cuts its windows there)
  hipLaunchKernelGGL(k_sparse_items_encode, dim3((unsigned)(n_items * (size_t)planes)), dim3(256), 0, s, T, win, items, planes,
                     item_bytes, bytes_per_chunk, logp, pt_modulus, polys);
  launched(0, "k_sparse_items_encode");
}

// ---- multiply_reg_by_sparse_database (dot_product.rs:13-220) ----------------------------------------------------------
// grid (num_per, planes); thread tau owns z = tau + 256 k.  Column ii's present items are col_rows / col_slots
// [col_ptr[ii], col_ptr[ii+1]); item polynomials: polys[slot][plane][z] (lo | hi << 32); the query is read from the
// expanded ciphertexts themselves, v[ct][r][crt][z] with ct = first + step * j (contiguous in z, no reorientation).
// Exact sums: products < 2^56, Barrett fold every 256 items.  Absent columns produce zeros (the fold relies on that).
__global__ __launch_bounds__(256) void k_sweep_sparse(DevTables T, const int* col_ptr, const int* col_rows, const int* col_slots,
                                                      const u64* polys, int planes, const u32* v, int first, int step,
                                                      u32* out, int num_per) {
  const int tau = threadIdx.x, ii = blockIdx.x, plane = blockIdx.y;
  const ModConst m0 = T.c.mod[0], m1 = T.c.mod[1];
  u64 a[8][4];
#pragma unroll
  for (int k = 0; k < 8; k++) a[k][0] = a[k][1] = a[k][2] = a[k][3] = 0;
  const int e0 = col_ptr[ii], e1 = col_ptr[ii + 1];
  int since = 0;
  for (int e = e0; e < e1; e++) {
    const int j = col_rows[e];
    const u64* b = polys + ((size_t)col_slots[e] * planes + plane) * N;
    const u32* q = v + (size_t)(first + step * j) * 4 * N;  // [r][crt][z]
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int z = tau + 256 * k;
      const u64 w = b[z];
      const u32 bl = (u32)w, bh = (u32)(w >> 32);
      a[k][0] += (u64)q[z] * bl;           // r0 crt0
      a[k][1] += (u64)q[N + z] * bh;       // r0 crt1
      a[k][2] += (u64)q[2 * N + z] * bl;   // r1 crt0
      a[k][3] += (u64)q[3 * N + z] * bh;   // r1 crt1
    }
    if (++since == 255) {
      since = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        a[k][0] = reduce64(a[k][0], m0); a[k][1] = reduce64(a[k][1], m1);
        a[k][2] = reduce64(a[k][2], m0); a[k][3] = reduce64(a[k][3], m1);
      }
    }
  }
  // out[plane][r][crt][z][ii]
  const size_t rc = (size_t)N * num_per;
  u32* o = out + (size_t)plane * 4 * rc + ii;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const size_t z = tau + 256 * k;
    o[0 * rc + z * num_per] = reduce64(a[k][0], m0);
    o[1 * rc + z * num_per] = reduce64(a[k][1], m1);
    o[2 * rc + z * num_per] = reduce64(a[k][2], m0);
    o[3 * rc + z * num_per] = reduce64(a[k][3], m1);
  }
}
void launch_sweep_sparse(const DevTables& T, const int* col_ptr, const int* col_rows, const int* col_slots, const u64* polys,
                         int planes, const u32* v, int first, int step, u32* out, int num_per, hipStream_t s) {
  hipLaunchKernelGGL(k_sweep_sparse, dim3(num_per, planes), dim3(256), 0, s, T, col_ptr, col_rows, col_slots, polys, planes, v,
                     first, step, out, num_per);
  launched(PATH_SWEEP_SPARSE, "k_sweep_sparse");
}

// ---- the same multiply for a GROUP of queries that share one pass over the bucket -------------------------------------
// grid (num_per, planes, N / (256 ZT)): thread tau of z-slab s owns the ZT consecutive z from (256 s + tau) ZT, so the B x 4 x ZT
// u64 sums stay in vector registers (B = 8 and 4: ZT = 2, 128 / 64 VGPRs of sums; B = 2: ZT = 4, 64.  B = 4 with ZT = 4 was measured
// and is a third slower per pass: profiles/sparse_batch_pass.md).  Every item word is loaded ONCE per group
// (16-byte non-temporal loads: nothing reads it again before the next pass) and multiplied into every query's four (r, crt) sums;
// the query rows (plain loads: every column re-reads them) are the members' own expanded ciphertexts v_b[ct][r][crt][z] and the
// sums go to the members' own out_b[plane][r][crt][z][ii].  `first` / `step` are the group's: its members share Params.
// A group of nq < B members runs the B body with DEAD slots: they read member 0's rows and store nothing.
// Exact sums as in k_sweep_sparse: products < 2^56, a Barrett fold after every 255 items of a column (a folded sum is < q < 2^28:
// 255 * 2^56 + 2^28 < 2^64), so the sums are canonical after the loop; absent columns write zeros.
typedef u64 sp_u64x2_t __attribute__((ext_vector_type(2)));
typedef u32 sp_u32x2_t __attribute__((ext_vector_type(2)));
typedef u32 sp_u32x4_t __attribute__((ext_vector_type(4)));
template <int B>
__global__ __launch_bounds__(256) void k_sweep_sparse_batch(DevTables T, const int* col_ptr, const int* col_rows, const int* col_slots,
                                                            const u64* polys, int planes, SparseGroup g, int nq, int first, int step,
                                                            int num_per) {
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
      const size_t qo = (size_t)(first + step * col_rows[e]) * 4 * N + z0;  // [r][crt][z]
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
        for (int rc = 0; rc < 4; rc++) {   // r0 crt0, r0 crt1, r1 crt0, r1 crt1
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
  // out_b[plane][r][crt][z][ii]
  const size_t rc_words = (size_t)N * num_per;
  const size_t o0 = (size_t)plane * 4 * rc_words + (size_t)z0 * num_per + ii;
#pragma unroll
  for (int b = 0; b < B; b++) {
    if (b >= nq) break;
    u32* o = g.out[b] + o0;
#pragma unroll
    for (int rc = 0; rc < 4; rc++)
#pragma unroll
      for (int k = 0; k < ZT; k++) o[rc * rc_words + (size_t)k * num_per] = (u32)a[b][rc][k];
  }
}
template <int B>
static void launch_sweep_sparse_batch_b(const DevTables& T, const int* col_ptr, const int* col_rows, const int* col_slots,
                                        const u64* polys, int planes, const SparseGroup& g, int nq, int first, int step, int num_per,
                                        hipStream_t s) {
  constexpr int ZT = B == 2 ? 4 : 2;
  hipLaunchKernelGGL(k_sweep_sparse_batch<B>, dim3(num_per, planes, N / (256 * ZT)), dim3(256), 0, s, T, col_ptr, col_rows, col_slots,
                     polys, planes, g, nq, first, step, num_per);
}
// 1 <= nq <= SPARSE_GROUP_MAX is the caller's to check (sparse_group_pass, capi.cpp)
void launch_sweep_sparse_batch(const DevTables& T, const int* col_ptr, const int* col_rows, const int* col_slots, const u64* polys,
                               int planes, const SparseGroup& members, int nq, int first, int step, int num_per, hipStream_t s) {
  SparseGroup g = members;
  for (int b = nq; b < SPARSE_GROUP_MAX; b++) {   // dead slots: valid rows to read, never stored
    g.v[b] = g.v[0];
    g.out[b] = nullptr;
  }
  if (nq <= 2)
    launch_sweep_sparse_batch_b<2>(T, col_ptr, col_rows, col_slots, polys, planes, g, nq, first, step, num_per, s);
  else if (nq <= 4)
    launch_sweep_sparse_batch_b<4>(T, col_ptr, col_rows, col_slots, polys, planes, g, nq, first, step, num_per, s);
  else
    launch_sweep_sparse_batch_b<8>(T, col_ptr, col_rows, col_slots, polys, planes, g, nq, first, step, num_per, s);
  launched(PATH_SWEEP_SPARSE | PATH_SWEEP_SPARSE_GROUP, "k_sweep_sparse_batch");
}

}  // namespace spiral

// the same multiplies on a row shard of a sparse bucket, stored in the reduce-scatter layouts
#include "sweep_sparse_scatter.hpp"
// sp_db_copy_items into a sparse bucket: item-major words into slots
#include "db_copy_sparse.hpp"
// sp_db_remove_items on a sparse bucket: survivors moved into the removed slots
#include "db_remove_sparse.hpp"
