// sp_db_remove_items, the dense writers: the planes * 2048 words of a removed item become the empty database's words -- zero -- in the
// resident words of an 8-byte or a PACKED handle.  Nothing is staged, nothing is encoded: a launch is driven by a device list of records
// the host builds per window (capi_remove.hpp) and touches the removed items' bytes only.
// Plain vector loads and stores only.  Included by db.hip only.
#pragma once
#include "device_common.hpp"

namespace spiral {

// ---- 8-byte words [plane][z][jl][il]: locals[k] = the handle's local linear index of a removed item (item_readback.hpp), each listed
// once.  One thread per (item, plane, z), 8 z-rows per thread: lanes along the list, so neighbours of a sorted list store neighbouring
// words of a resident row.  grid (ceil(n / 64), N / 32, planes)
constexpr int CLEAR_Z = 32;
__global__ __launch_bounds__(256) void k_items_clear_words8(u64* db, const unsigned long long* locals, size_t n, size_t row_words) {
  const size_t k = (size_t)blockIdx.x * 64 + (size_t)(threadIdx.x & 63);
  if (k >= n) return;
  const size_t L = (size_t)locals[k];
  const int zq = threadIdx.x >> 6, plane = blockIdx.z, z0 = blockIdx.y * CLEAR_Z;
#pragma unroll
  for (int pass = 0; pass < CLEAR_Z / 4; pass++) db[((size_t)plane * N + (size_t)(z0 + pass * 4 + zq)) * row_words + L] = 0ull;
}

// ---- PACKED: the four words of a quad (rows 2 jp, 2 jp + 1 x columns 2 q, 2 q + 1) share one 28-byte lane group, so ONE THREAD owns a
// quad of one (plane, z) -- the ownership rule of k_items_scatter_packed and k_db_encode_quads.  It loads the lane group's 7 dwords,
// clears the 56-bit fields the mask names (bit row a * 2 + column b; field w is bits 56 w .. 56 w + 55 of the 224) and stores them.
// The host lists a quad once per launch with every item of it that the launch removes.
// A workgroup takes 64 listed quads for 16 z-rows of one plane.  grid (ceil(n_quads / 64), N / 16, planes)
constexpr int CLEAR_PACKED_Z = 16;
__global__ __launch_bounds__(256) void k_items_clear_packed(u32* db, const RemoveQuadRec* quads, size_t n_quads, int np_local, int nj) {
  const int chunks = np_local >> 7, npairs = nj >> 1;
  const size_t k = (size_t)blockIdx.x * 64 + (size_t)(threadIdx.x & 63);
  if (k >= n_quads) return;
  const RemoveQuadRec r = quads[k];
  const int zq = threadIdx.x >> 6, plane = blockIdx.z, z0 = blockIdx.y * CLEAR_PACKED_Z;
  const int chunk = r.q >> 6, lane = r.q & 63;
  const u32 m = r.mask;
  // what each of the 7 dwords keeps: field 0 = dword 0 and the low 24 bits of dword 1, field 1 = the high 8 of dword 1, dword 2 and the
  // low 16 of dword 3, field 2 = the high 16 of dword 3, dword 4 and the low 8 of dword 5, field 3 = the high 24 of dword 5 and dword 6
  const u32 k0 = m & 1u ? 0u : 0xffffffffu;
  const u32 k1 = (m & 1u ? 0u : 0x00ffffffu) | (m & 2u ? 0u : 0xff000000u);
  const u32 k2 = m & 2u ? 0u : 0xffffffffu;
  const u32 k3 = (m & 2u ? 0u : 0x0000ffffu) | (m & 4u ? 0u : 0xffff0000u);
  const u32 k4 = m & 4u ? 0u : 0xffffffffu;
  const u32 k5 = (m & 4u ? 0u : 0x000000ffu) | (m & 8u ? 0u : 0xffffff00u);
  const u32 k6 = m & 8u ? 0u : 0xffffffffu;
#pragma unroll 1
  for (int pass = 0; pass < CLEAR_PACKED_Z / 4; pass++) {
    u32* unit = db + packed_unit_offset((size_t)plane * N + (size_t)(z0 + pass * 4 + zq), r.jp, chunk, npairs, chunks);
    u32* p4 = unit + lane * 4;
    u32* p3 = unit + 256 + lane * 3;
    if (m == 0xfu) {   // the whole lane group: stored without a read
      p4[0] = p4[1] = p4[2] = p4[3] = 0u;
      p3[0] = p3[1] = p3[2] = 0u;
      continue;
    }
    const u32 d0 = p4[0], d1 = p4[1], d2 = p4[2], d3 = p4[3], d4 = p3[0], d5 = p3[1], d6 = p3[2];
    p4[0] = d0 & k0;
    p4[1] = d1 & k1;
    p4[2] = d2 & k2;
    p4[3] = d3 & k3;
    p3[0] = d4 & k4;
    p3[1] = d5 & k5;
    p3[2] = d6 & k6;
  }
}

void launch_items_clear_words8(u64* db, const unsigned long long* locals, size_t n, int np_local, int nj, int planes, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_items_clear_words8, dim3((unsigned)((n + 63) / 64), N / CLEAR_Z, planes), dim3(256), 0, s, db, locals, n,
                     (size_t)nj * (size_t)np_local);
  launched(0, "k_items_clear_words8");
}
void launch_items_clear_packed(u64* db, const RemoveQuadRec* quads, size_t n_quads, int np_local, int nj, int planes, hipStream_t s) {
  if (n_quads == 0) return;
  hipLaunchKernelGGL(k_items_clear_packed, dim3((unsigned)((n_quads + 63) / 64), N / CLEAR_PACKED_Z, planes), dim3(256), 0, s,
                     reinterpret_cast<u32*>(db), quads, n_quads, np_local, nj);
  launched(0, "k_items_clear_packed");
}

}  // namespace spiral
