// What the digest kernels share (sp_db_digest; kernels.hpp has the definition): the row keys of a tile of rows staged in LDS and the
// workgroup's partial pair added into the plane's sums.  Included by db_digest.hpp (db.hip) and db_digest_planar.hpp
// (sweep_planar.hip) only.
#pragma once
#include "device_common.hpp"

namespace spiral {

constexpr int DIGEST_WG = 256;

// LDS of a dense digest workgroup: the row keys of at most DIGEST_ROWS rows, both lanes, and one pair per thread for the reduction
struct DigestLds {
  u64 R[2][DIGEST_ROWS];
  u64 part[2][DIGEST_WG];
};

// rows [jt0, jt0 + n) of the handle's table -> lds.R[l][0 .. n), and the barrier behind it
__device__ __forceinline__ void digest_stage_rows(DigestLds& lds, const DigestDesc& d, int jt0, int n) {
  for (int i = threadIdx.x; i < n; i += DIGEST_WG) {
    lds.R[0][i] = d.R[jt0 + i];
    lds.R[1][i] = d.R[(size_t)d.nj + jt0 + i];
  }
  __syncthreads();
}

// the workgroup's 256 pairs (a0, a1) summed through LDS, then one atomic add per lane into the plane's pair: wrapping adds commute,
// so the order in which workgroups arrive does not change the value
__device__ __forceinline__ void digest_reduce(u64 (&part)[2][DIGEST_WG], const DigestDesc& d, int plane, u64 a0, u64 a1) {
  const int t = threadIdx.x;
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
  if (t < 2) atomicAdd(d.sums + 2 * (size_t)(plane - d.plane0) + t, (unsigned long long)part[t][0]);
}

}  // namespace spiral
