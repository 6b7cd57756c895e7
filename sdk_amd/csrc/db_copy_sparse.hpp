// sp_db_copy_items into a sparse bucket: its store is [slot][plane][z], which is the item-major stage's own layout (db_copy.hpp), so an
// item is one copy of planes * 2048 words -- polys[rec.slot][plane][z] = stage[rec.src][plane][z] -- in 16-byte accesses, one per
// thread.  The caller lists a slot once per launch.  Plain vector loads and stores only.  Included by sparse.hip only.
#pragma once
#include "device_common.hpp"

namespace spiral {

// grid (n_recs, planes * 4): block x is the record, block y a run of 256 sixteen-byte pieces (512 words) of the item
__global__ __launch_bounds__(256) void k_items_copy_slots(u64* polys, const u64* stage, const CopySlotRec* recs, int planes) {
  const size_t per = (size_t)planes * (N / 2);   // 16-byte pieces of an item
  const CopySlotRec r = recs[blockIdx.x];
  const size_t o = (size_t)blockIdx.y * 256 + threadIdx.x;   // < per: gridDim.y * 256 == per
  reinterpret_cast<uint4*>(polys)[(size_t)r.slot * per + o] = reinterpret_cast<const uint4*>(stage)[(size_t)r.src * per + o];
}

// One dispatch takes 2^32 - 1 work-items along x and 65535 blocks along y: the records go along x -- n_recs * 256 work-items, and the
// caller's windows keep n_recs * planes <= 2^23, so at most 2^31 -- and the 4 * planes pieces of an item along y.
void launch_items_copy_slots(u64* polys, const u64* stage, const CopySlotRec* recs, size_t n_recs, int planes, hipStream_t s) {
  if (n_recs == 0) return;   // (the caller checks n_recs * planes against UPSERT_MAX_GROUP_PLANES)
  hipLaunchKernelGGL(k_items_copy_slots, dim3((unsigned)n_recs, (unsigned)(planes * (N / 2) / 256)), dim3(256), 0, s, polys, stage, recs,
                     planes);
  launched(0, "k_items_copy_slots");
}

}  // namespace spiral
