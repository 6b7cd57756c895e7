// sp_db_remove_items on a sparse bucket: its store [slot][plane][z] stays dense in 0 .. count - 1, so the survivors that stand at or above
// the new count move into the removed slots below it -- polys[rec.dst_slot] = polys[rec.src_slot], planes * 2048 words in 16-byte
// accesses, one per thread.  The sources (survivors at or above the new count) and the destinations (removed slots below it) of a call
// are disjoint sets, so neither the order inside a launch nor the order of the windows matters.
// Plain vector loads and stores only.  Included by sparse.hip only.
#pragma once
#include "device_common.hpp"

namespace spiral {

// grid (n_recs, planes * 4): block x is the record, block y a run of 256 sixteen-byte pieces (512 words) of the item
__global__ __launch_bounds__(256) void k_sparse_move_slots(u64* polys, const RemoveSlotRec* recs, int planes) {
  const size_t per = (size_t)planes * (N / 2);   // 16-byte pieces of an item
  const RemoveSlotRec r = recs[blockIdx.x];
  const size_t o = (size_t)blockIdx.y * 256 + threadIdx.x;   // < per: gridDim.y * 256 == per
  uint4* p = reinterpret_cast<uint4*>(polys);
  p[(size_t)r.dst_slot * per + o] = p[(size_t)r.src_slot * per + o];
}

// One dispatch takes 2^32 - 1 work-items along x and 65535 blocks along y: the records go along x -- n_recs * 256 work-items, and the
// caller's windows keep n_recs * planes <= 2^23, so at most 2^31 -- and the 4 * planes pieces of an item along y.
void launch_sparse_move_slots(u64* polys, const RemoveSlotRec* recs, size_t n_recs, int planes, hipStream_t s) {
  if (n_recs == 0) return;   // (the caller checks n_recs * planes against UPSERT_MAX_GROUP_PLANES)
  hipLaunchKernelGGL(k_sparse_move_slots, dim3((unsigned)n_recs, (unsigned)(planes * (N / 2) / 256)), dim3(256), 0, s, polys, recs, planes);
  launched(0, "k_sparse_move_slots");
}

}  // namespace spiral
