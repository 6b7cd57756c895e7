// What the translation units of the extern "C" surface share: capi.cpp (error boundary, handles, the query stage machine),
// capi_batch.cpp (the list flows of sp_process_query_batch) and capi_stage.cpp (stage-level exports, benchmarks, probes).
#pragma once
#include <cstring>
#include <memory>
#include <string>

#include "../../include/spiral_hip.h"
#include "pipeline.hpp"

struct sp_query {
  sp_params* params = nullptr;
  const sp_pp* pp = nullptr;
  std::unique_ptr<spiral::Workspace> ws;
  int state = 0;  // 1 begun, 2 swept, 3 finished
  int next_plane = 0;  // sp_query_sweep_scatter_plane progress
  int next_fold_plane = 0;  // sp_query_fold_local_plane progress
  int rows_j0 = 0, rows_nj = 0;  // sp_query_begin_for_db on a row shard: only these first-dimension rows were expanded
  const sp_db* for_sparse = nullptr;  // begun for this sparse bucket: only the rows holding items were expanded
  std::shared_ptr<const sp_db::SparseIndex> sparse_index;  // ... with this snapshot of its index (kept until the query is freed)
  std::shared_ptr<const spiral::DevBuf<spiral::u64>> planar;  // the digit-planar copy a batched group's pass on this (first) workspace
                                                              // reads: pinned until the query is freed, i.e. until after its stream
                                                              // has been synchronised
  float ms[4] = {0, 0, 0, 0};
  bool streams_idle = false;  // the owner has waited for the main stream after the last enqueue (which orders stream2's work before it)
  ~sp_query() {
    if (ws && params) {
      if (!streams_idle) {
        (void)hipStreamSynchronize(ws->stream);
        (void)hipStreamSynchronize(ws->stream2);
      }
      // a pooled workspace carries nothing of the query that held it
      ws->pipelined = false;
      ws->have_sweep_span = false;
      ws->zero_shortcuts = false;
      ws->out_G = 1;
      params->release_ws(std::move(ws));
    }
  }
};

// internal hook (not declared in the public header): sets the text sp_last_error returns to this thread
extern "C" void sp_set_last_error_(const char* msg);

namespace spiral {

// The thread's last error text and the status of its last guarded() section (what a constructor-style entry point, which returns a
// handle or null, failed with) are defined once, in capi.cpp.
int guarded_status(int rc, const char* what);   // records rc and, unless SP_OK, the text; returns rc
int null_handle_rc();                           // status to report when a handle-returning entry point came back null

template <typename F>
int guarded(F&& f) {
  tunables_new_call();
  try {
    f();
    return guarded_status(SP_OK, nullptr);
  } catch (const ArgError& e) {
    return guarded_status(SP_E_ARG, e.what());
  } catch (const OomError& e) {
    return guarded_status(SP_E_OOM, e.what());
  } catch (const HipError& e) {
    return guarded_status(SP_E_HIP, e.what());
  } catch (const std::bad_alloc&) {
    return guarded_status(SP_E_OOM, "host allocation failed");
  } catch (const std::exception& e) {
    return guarded_status(SP_E_ARG, e.what());
  }
}
// a constructor-style entry point: `make` returns the handle as a std::unique_ptr; null on an error (status: null_handle_rc)
template <typename F>
auto guarded_handle(F&& make) -> decltype(make().release()) {
  decltype(make()) h;
  return guarded([&] { h = make(); }) == SP_OK ? h.release() : nullptr;
}

inline void need(bool c, const char* msg) {
  if (!c) throw ArgError(msg);
}
void check_device(int dev);   // throws unless `dev`, the device a handle was created on, is the current one

struct Scoped {  // a workspace borrowed for one stage-level call
  sp_params* P;
  std::unique_ptr<Workspace> ws;
  explicit Scoped(const sp_params* p) : P(const_cast<sp_params*>(p)), ws(P->acquire_ws()) {}
  ~Scoped() {
    (void)hipStreamSynchronize(ws->stream);
    P->release_ws(std::move(ws));
  }
  Workspace& operator*() { return *ws; }
  Workspace* operator->() { return ws.get(); }
};
void download_ntt(Workspace& W, const u32* src, size_t words, uint64_t* host, DevBuf<u64>& tmp);   // device u32 NTT words -> host u64

// a pair of timing events that cannot leak
struct TimingEvents {
  hipEvent_t a = nullptr, b = nullptr;
  TimingEvents() {
    HIP_CHECK(hipEventCreate(&a));
    if (hipEventCreate(&b) != hipSuccess) {
      (void)hipEventDestroy(a);
      throw HipError("hipEventCreate failed");
    }
  }
  ~TimingEvents() {
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
  TimingEvents(const TimingEvents&) = delete;
  TimingEvents& operator=(const TimingEvents&) = delete;
};
// Warm once, then time `iters` repetitions of `once` on stream `s`: milliseconds per repetition (per launch, where the caller says
// how many launches a repetition makes).  The events are destroyed and the stream is waited for on every path out of here (launches
// and HIP_CHECK throw), so whatever the caller pinned for the launches before this call is released only after they have run.
template <typename F>
float timed_reps(hipStream_t s, int iters, F&& once, float launches_per_rep = 1.0f) {
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  TimingEvents ev;
  once();  // warm
  HIP_CHECK(hipEventRecord(ev.a, s));
  for (int i = 0; i < iters; i++) once();
  HIP_CHECK(hipEventRecord(ev.b, s));
  HIP_CHECK(hipStreamSynchronize(s));
  float t = 0;
  HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
  return t / ((float)iters * launches_per_rep);
}

// ---- pieces of the query stage machine (capi.cpp) that the list flows and the benchmarks build on
// a query object with its workspace, nothing enqueued yet but the "begin" event (the group flow of sp_process_query_batch, which
// expands its queries together: run_begin_group); state 0 until the caller has begun it
sp_query_t* query_open(const sp_params_t* h, const sp_pp_t* pp);
// the same for a member of a sparse bucket's group: it holds `snapshot` of the bucket's index, the group's one, instead of taking its
// own, and its first-dimension output exists before anything is enqueued; query_begin_opened then begins it exactly as
// sp_query_begin_for_db begins a query (pruned expansion against the snapshot's plan on the query's own stream; throws)
sp_query_t* query_open_sparse(const sp_params_t* h, const sp_pp_t* pp, const sp_db_t* db, std::shared_ptr<const sp_db::SparseIndex> snapshot);
void query_begin_opened(sp_query_t* q, const uint8_t* query, size_t query_len, const sp_db_t* db);
void finish_impl(sp_query_t* q, bool premod, uint8_t* out, size_t out_cap, size_t* out_len);

// what one workspace of a batched group may need, as the group planner and the planar copy estimate it
size_t group_ws_bytes(const Params& p, int np_local);

using PlanarPin = std::shared_ptr<const DevBuf<u64>>;
// One batched pass of the group qs[0 .. B) over `db`, run on the first query's stream: the database, the queries' operands and
// outputs; on the matrix cores the group's query digit table with the first workspace (allocated on its first batched call, then
// reused) and, for two query tiles, the digit-planar copy -- pinned in `pin`, which the caller holds until that stream has been
// synchronised.
SweepBatchDesc group_pass(const sp_db& db, sp_query_t* const* qs, int B, bool use_planar, PlanarPin& pin);
// ... and the group's query tables and pass enqueued on `s`: the planar-resident kernels for such a handle (no switch is asked), else
// sweep_batch_prepare + launch_sweep_batch
void group_pass_launch(const sp_db& db, const DevTables& T, SweepBatchDesc& d, hipStream_t s);
// throws ArgError naming the format when `db` is planar-resident: the entry points that sweep per plane, in the scatter layout or on
// shards
void refuse_planar_resident(const sp_db_t* db, const char* what);
// The order around it.  The pass waits for every member's expansion: ev[1], recorded on the member's stream (the operand of the
// pass, qv, is written on that stream also when the odd subtree was split off); returns the first member's workspace ...
Workspace& group_pass_stream(sp_query_t* const* qs, int B);
// ... and once the pass is enqueued, member i's ev[2] is recorded on its own stream, which for i > 0 first waits for the first
// member's ev[2]: call for i = 0 first
void group_pass_done(sp_query_t* const* qs, int i);

// One pass over the sparse bucket `db` for the group qs[0 .. B), B <= SPARSE_GROUP_MAX, all begun on one snapshot of its index (the
// first member's is read): enqueued on `s`; the order around it is the caller's (group_pass_stream / group_pass_done)
void sparse_group_pass(const sp_db& db, sp_query_t* const* qs, int B, hipStream_t s);

// sp_query_sweep_scatter_group's checks (nothing enqueued on an error) and its prepared descriptor: the group's pass in the
// reduce-scatter layout on the first query's stream; false: this group or shape is not the matrix-core pass's -- the caller sweeps
// per query
void scatter_group_check(sp_query_t* const* qs, int batch, const sp_db_t* db, int G);
bool scatter_group_desc(sp_query_t* const* qs, int batch, const sp_db_t* db, int G, SweepBatchDesc& d);

}  // namespace spiral
