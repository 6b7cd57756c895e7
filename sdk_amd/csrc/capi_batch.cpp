// sp_process_query_batch: the three flows that answer a list of queries on one unsharded database.
#include <chrono>
#include <deque>

#include "capi_internal.hpp"

using namespace spiral;

namespace {

struct BatchArgs {  // sp_process_query_batch's arguments
  const sp_params_t* h;
  const sp_pp_t* const* pps;
  const uint8_t* const* queries;
  const size_t* query_lens;
  int batch;
  const sp_db_t* db;
  uint8_t* out;
  size_t out_stride;
  size_t* out_len;
  std::chrono::steady_clock::time_point t_entry;
};

// 8-byte / narrow databases: one pass per query, up to `batch_in_flight` (default 3, at most 4; 1 = one at a time)
// queries in flight -- query i + 1 is deserialised, expanded and swept on its own workspace and streams before query
// i is waited for, so that its expansion, a chain of ~30 small dependent launches, runs under its predecessors' sweeps
// and folds instead of after them.  Lists of 8: C1 994 -> 1422 queries/s, P2 828 -> 1054.
int answer_in_flight(const BatchArgs& a) {
  if (a.db->num_shards != 1 || a.db->col_G != 1) {
    sp_set_last_error_("sp_process_query_batch needs an unsharded db");
    return SP_E_ARG;
  }
  size_t depth = (size_t)std::max(1L, std::min(4L, tunable("batch_in_flight", 3)));
  std::deque<std::pair<sp_query_t*, int>> flying;  // oldest first
  int rc = SP_OK;
  auto begin = [&](int i) { return sp_query_begin_for_db(a.h, a.pps[i], a.queries[i], a.query_lens[i], a.db); };
  auto finish_oldest = [&]() -> int {
    sp_query_t* q = flying.front().first;
    const int qi = flying.front().second;
    flying.pop_front();
    int r = guarded([&] { finish_impl(q, false, a.out + (size_t)qi * a.out_stride, a.out_stride, a.out_len); });
    sp_query_free(q);
    return r;
  };
  for (int i = 0; i < a.batch && rc == SP_OK; i++) {
    sp_query_t* q = begin(i);
    if (!q && null_handle_rc() == SP_E_OOM && !flying.empty()) {
      // no memory for one more workspace (sweep_out + fold buffers, up to ~2 GiB) beside the database and the queries in
      // flight: finish those -- their workspaces return to the pool -- and go on one query at a time
      while (rc == SP_OK && !flying.empty()) rc = finish_oldest();
      if (rc != SP_OK) break;
      depth = 1;
      q = begin(i);
    }
    if (!q) {
      rc = null_handle_rc();
      break;
    }
    rc = sp_query_sweep(q, a.db);
    if (rc != SP_OK) {
      sp_query_free(q);
      break;
    }
    flying.push_back({q, i});
    while (rc == SP_OK && flying.size() >= depth) rc = finish_oldest();   // depth 1: one at a time
  }
  while (rc == SP_OK && !flying.empty()) rc = finish_oldest();
  if (rc != SP_OK) {  // keep the first error; whatever is still in flight is drained and dropped
    const std::string first = sp_last_error();
    for (auto& f : flying) {
      (void)hipStreamSynchronize(f.first->ws->stream);
      sp_query_free(f.first);
    }
    sp_set_last_error_(first.c_str());
  }
  return rc;
}

// What the two group flows below share: the queries in flight, oldest first (at most two groups: bounds the workspaces held), the
// responses copied out so far, and the previous group's pass, which the next pass waits for.
struct GroupsInFlight {
  const BatchArgs& a;
  const Params& p;
  std::vector<sp_query_t*> all_qs;
  size_t drained = 0;                // responses copied out so far
  hipEvent_t prev_pass = nullptr;
  size_t prev_group = 0;

  explicit GroupsInFlight(const BatchArgs& args) : a(args), p(args.h->p) {}
  ~GroupsInFlight() {
    for (auto* q : all_qs) sp_query_free(q);
  }

  void drain(size_t count) {   // oldest `count` queries: wait, copy the response out, give the workspace back
    for (size_t i = 0; i < count; i++) {
      Workspace& W = *all_qs[i]->ws;
      HIP_CHECK(hipStreamSynchronize(W.stream));
      memcpy(a.out + (drained + i) * a.out_stride, W.h_response, p.response_bytes());
      *a.out_len = p.response_bytes();
      // (run_finish joins the second stream into the main one before the response copy, and a split-off odd expansion subtree
      // -- not used by grouped expansions -- is joined before the fold: both streams are idle now)
      all_qs[i]->streams_idle = !W.right_pending;
    }
    for (size_t i = 0; i < count; i++) sp_query_free(all_qs[i]);
    all_qs.erase(all_qs.begin(), all_qs.begin() + count);
    drained += count;
  }
  void keep_previous_group() {   // before a new group is enqueued: only the previous one stays in flight
    if (all_qs.size() > prev_group) drain(all_qs.size() - prev_group);
  }

  void abandon() {  // let whatever was queued drain before the workspaces go back to the pool
    for (auto* q : all_qs) (void)hipStreamSynchronize(q->ws->stream);
    for (auto* q : all_qs) sp_query_free(q);
    all_qs.clear();
    prev_group = 0;
    prev_pass = nullptr;
  }
  // an error other than out of memory: the first error text is kept, whatever is still in flight is drained and dropped
  int fail(int rc) {
    const std::string first_error = sp_last_error();
    abandon();
    sp_set_last_error_(first_error.c_str());
    return rc;
  }
};

// PACKED databases, and narrow ones (below).  Groups of up to 8 queries -- 16 where the two-tile matrix-core pass applies (batch_group = 0, the default, asks
// the kernel side; a positive value caps the group) -- share one database pass.  Nothing waits for a group's folds before the next
// group's expansions and pass are queued (the passes themselves run one after the other: both are HBM-bound), and at
// most two groups hold workspaces at a time.  Measured at C2 (profiles/r02_fold_batch_experiments.md): the overlap
// buys nothing yet -- 16 queries take 2 x the time of 8, and 8 as 2 x 4 are slower (195 vs 236 queries/s) -- because
// the batched sweep's workgroups fill every CU's register file, so a fold wave only starts when the pass drains.
// Narrow databases (8-byte words, 2 <= num_per <= 64: sweep_narrow_batch_shape_ok) take the same flow with k_sweep_narrow_batch as
// the pass: groups of 8, and only groups of at least `narrow_min` members (switch narrow_batch_min) -- what is left of the list,
// a last group below the threshold or a trailing single query, is answer_in_flight's.
struct GroupedFlow : GroupsInFlight {
  // diagnostic (switch batch_trace): host time stamps of this call's phases on stderr, microseconds from entry
  const bool trace = tunable("batch_trace", 0) != 0;
  int start = 0;   // first query not yet answered (a retry after an out-of-memory resumes here)
  bool use_planar = true, one_group = false;   // what the out-of-memory ladder gives up, in this order
  int group_max = 0;
  const int narrow_min;   // > 0: a narrow database; groups below this size are not this flow's

  explicit GroupedFlow(const BatchArgs& args, int narrow_group_min = 0) : GroupsInFlight(args), narrow_min(narrow_group_min) {}

  void stamp(const char* what) const {
    if (trace)
      fprintf(stderr, "[spiral] batch %-22s %8.1f us\n", what,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a.t_entry).count());
  }

  // a list of exactly 9 .. 16 queries is one group; longer lists are cut into groups of group_max (a last group of <= 8
  // takes the one-tile pass)
  void decide_group_max() {
    // (a planar-resident database: both tiles whatever the switches say now -- they were read when it was created)
    const int shape_max = a.db->planar_resident ? planar_resident_group_max(a.db->nj) : sweep_batch_group_max(a.db->np_local, a.db->nj);
    group_max = (int)tunable("batch_group", 0);
    if (group_max <= 0) group_max = shape_max;
    group_max = std::max(1, std::min(shape_max, group_max));
    if (narrow_min > 0) group_max = SWEEP_BATCH_MAX;
    if (group_max > SWEEP_BATCH_MAX && a.batch > SWEEP_BATCH_MAX) {
      // two groups of 16 hold up to 32 workspaces: keep to groups of 8 when the device could not hold them beside the database
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < (size_t)2 * SWEEP_GROUP_MAX * group_ws_bytes(p, a.db->np_local))
        group_max = SWEEP_BATCH_MAX;
      (void)hipGetLastError();
    }
  }

  // 1. expand every query of the group [g0, g0 + B) on its own stream.  (r05: the sixteen expansions of a group are 8-10 of a step's
  // 49 ms and looked like a launch-rate problem -- 1,600 small launches, 1.5 kernels in flight.  They are not: enqueued by 1, 2, 4 or
  // 8 host threads, on 4, 8 or 16 hardware queues, or recorded and issued as ONE chain of ~100 table launches for the whole
  // group, they take the same time -- 0.5 ms of a query's expansion is transforms that fill the chip (320 k forward NTTs, more
  // than its fold has).  profiles/r05_batch16_step_timeline.md, r05_batch_expand.md; scripts/archive/r05_batch_expand/.)
  // r06: they ARE 2x off the transform rate, and the cure is the shape of the launches, not their number: a round of ONE query
  // under-fills the chip until its last rounds (a right-hand ciphertext's 57 transforms run in sequence in one workgroup), so
  // the group's rounds are shared launches with the query as one more grid dimension (run_begin_group; switch expand_group).
  sp_query_t* const* expand_group(int g0, int B) {
    const size_t first = all_qs.size();
    const bool group_expand = B >= 2 && p.expand_queries && tunable("expand_group", 1) != 0;
    for (int i = 0; i < B; i++) {
      sp_query_t* q = group_expand ? query_open(a.h, a.pps[g0 + i])
                                   : sp_query_begin(a.h, a.pps[g0 + i], a.queries[g0 + i], a.query_lens[g0 + i]);
      if (!q) {
        if (null_handle_rc() == SP_E_OOM) throw OomError(sp_last_error());   // (reported by status: the caller retries in smaller groups)
        throw ArgError(sp_last_error());
      }
      all_qs.push_back(q);
      q->ws->ensure_sweep();
    }
    sp_query_t* const* qs = all_qs.data() + first;
    stamp("workspaces acquired");
    if (group_expand) {
      Workspace* Ws[GROUP_MAX];
      for (int i = 0; i < B; i++) Ws[i] = qs[i]->ws.get();
      run_begin_group(Ws, a.pps + g0, a.queries + g0, a.query_lens + g0, B);
      for (int i = 0; i < B; i++) {
        HIP_CHECK(hipEventRecord(Ws[i]->ev[1], Ws[i]->stream));
        qs[i]->state = 1;
      }
    }
    stamp("expansions enqueued");
    return qs;
  }

  // 2. one database pass for the whole group, on the first query's stream, after the previous group's pass; the first query
  // holds the pass's pin of the planar copy
  void pass(sp_query_t* const* qs, int B) {
    Workspace& W0 = group_pass_stream(qs, B);
    if (prev_pass) HIP_CHECK(hipStreamWaitEvent(W0.stream, prev_pass, 0));
    SweepBatchDesc d = group_pass(*a.db, qs, B, use_planar, qs[0]->planar);
    // (a per-plane form of the pass with every query folding plane p beside the pass of plane p + 1 was measured in rounds
    // 2 and 3 and is slower: the pass leaves no registers for a fold workgroup; profiles/r02_fold_batch_experiments.md)
    group_pass_launch(*a.db, W0.D->T, d, W0.stream);
    group_pass_done(qs, 0);
    prev_pass = W0.ev[2];
    stamp("pass enqueued");
  }

  // 3. (rest of the) fold / pack per query, concurrently on the queries' own streams
  void folds(sp_query_t* const* qs, int B) {
    for (int i = 0; i < B; i++) {
      if (i > 0) group_pass_done(qs, i);
      run_finish(*qs[i]->ws, *qs[i]->pp, false);
    }
    prev_group = (size_t)B;
    stamp("folds enqueued");
  }

  void run_groups() {   // the list from `start` on
    check_device(a.db->device);
    for (int g0 = start; a.batch - g0 >= std::max(1, narrow_min); g0 += group_max) {
      const int B = std::min(group_max, a.batch - g0);
      if (one_group) {
        if (!all_qs.empty()) drain(all_qs.size());                        // nothing in flight beside this group
      } else {
        keep_previous_group();
      }
      sp_query_t* const* qs = expand_group(g0, B);
      pass(qs, B);
      folds(qs, B);
    }
    drain(all_qs.size());
    stamp("drained");
  }

  // Steps 1 and 2 of the out-of-memory ladder: false when the step has nothing to give up.  (1) the digit-planar copy of the
  // database (its memory is released; a later call may build it again when there is room); (2) groups of 16 and the second group in
  // flight: groups of 8, one at a time -- the in-flight queries' workspaces went back to the pool, so a group of 8 needs no more
  // than was already allocated unless the failure came before 8 workspaces existed.
  bool give_up(int step) {
    if (step == 1) {   // (abandon has released the pins of the groups in flight: dropping the handle's copy frees it)
      sp_db* wdb = const_cast<sp_db_t*>(a.db);
      std::lock_guard<std::mutex> lk(wdb->mu);
      use_planar = false;
      if (!wdb->planar) return false;
      wdb->drop_planar();
      wdb->planar_state = -2;
      return true;
    }
    if (group_max <= SWEEP_BATCH_MAX && one_group) return false;
    group_max = std::min(group_max, SWEEP_BATCH_MAX);
    one_group = true;
    return true;
  }
  // step 3: one query at a time, one workspace
  int one_at_a_time() {
    int rc = SP_OK;
    for (int i = start; i < a.batch && rc == SP_OK; i++, drained++)
      rc = sp_process_query(a.h, a.pps[i], a.queries[i], a.query_lens[i], a.db, a.out + (size_t)i * a.out_stride, a.out_stride, a.out_len);
    return rc;
  }

  int run() {
    stamp("entry");
    decide_group_max();
    stamp("group size decided");
    int rc = guarded([&] { run_groups(); });
    // Out of memory (the hipMemGetInfo estimates above are rough): give up, one after the other, what only makes the call faster, and
    // answer the REST of the list each time -- responses already copied out stay.
    // (a narrow database has no planar copy; a planar-resident one has nothing but its planar words, which are not given up)
    for (int step = narrow_min > 0 || a.db->planar_resident ? 2 : 1; rc == SP_E_OOM && step <= 3; step++) {
      abandon();
      (void)hipGetLastError();
      start = (int)drained;
      if (step == 3)
        rc = one_at_a_time();
      else if (give_up(step))
        rc = guarded([&] { run_groups(); });
    }
    if (rc != SP_OK) return fail(rc);
    if ((int)drained == a.batch) return SP_OK;
    BatchArgs rest = a;   // narrow: a last group below the threshold keeps the per-query flow
    rest.pps += drained;
    rest.queries += drained;
    rest.query_lens += drained;
    rest.batch -= (int)drained;
    rest.out += drained * a.out_stride;
    return answer_in_flight(rest);
  }
};

int answer_in_groups(const BatchArgs& a, int narrow_min = 0) {
  if (a.out_stride < a.h->p.response_bytes()) {
    sp_set_last_error_("out_stride smaller than response_bytes");
    return SP_E_ARG;
  }
  // the questions of the flow (LDS opt-in limit, free memory) are put to the CURRENT device: it has to be the database's
  const int rc = guarded([&] { check_device(a.db->device); });
  return rc != SP_OK ? rc : GroupedFlow(a, narrow_min).run();
}

// dense, unsharded 8-byte databases: the group flow where the shape is k_sweep_narrow_batch's and the list reaches the threshold
int answer_narrow(const BatchArgs& a) {
  long m = tunable("narrow_batch_min", NARROW_BATCH_MIN_DEFAULT);
  if (m < 0) m = NARROW_BATCH_MIN_DEFAULT;   // (a negative value: the shipped default again, for a caller that had overridden it)
  const int group_min = (int)std::max(2L, m);
  if (m <= 0 || group_min > SWEEP_BATCH_MAX || a.batch < group_min || !sweep_narrow_batch_shape_ok(a.db->np_local, a.db->nj))
    return answer_in_flight(a);
  return answer_in_groups(a, group_min);
}


// Sparse buckets (lib/server's SparseDb: the /private-read caller).  The list is cut into groups of at most SPARSE_GROUP_MAX = 8;
// a group of at least `sparse_batch_min` members (switch; 0 = never, negative = the shipped default, at least 2 otherwise) shares ONE pass over the bucket
// (k_sweep_sparse_batch: every item word read once per group), the rest of the list -- a last group below the threshold, a trailing
// single query -- keeps the per-query flow above with its `batch_in_flight` depth.  A group takes one snapshot of the bucket's index,
// held by all its members; each member is begun as sp_query_begin_for_db begins it (pruned expansion against that snapshot's plan
// on its own stream), the pass runs on the first member's stream after every member's expansion and after the previous group's
// pass, and the folds (all-zero shortcuts) run on the members' own streams.  As in GroupedFlow at most two groups hold workspaces,
// every workspace's buffers exist before anything of its group is enqueued, and responses are copied out in list order.  Out of
// memory: what is in flight is drained and dropped, the rest of the list is answered one query at a time.
struct SparseGroupFlow : GroupsInFlight {
  explicit SparseGroupFlow(const BatchArgs& args) : GroupsInFlight(args) {}

  void group(int g0, int B) {
    const size_t first = all_qs.size();
    auto snapshot = const_cast<sp_db_t*>(a.db)->ensure_sparse_index();
    for (int i = 0; i < B; i++) {   // every workspace (and its first-dimension output) before anything is enqueued
      sp_query_t* q = query_open_sparse(a.h, a.pps[g0 + i], a.db, snapshot);
      if (!q) {
        if (null_handle_rc() == SP_E_OOM) throw OomError(sp_last_error());
        throw ArgError(sp_last_error());
      }
      all_qs.push_back(q);
    }
    sp_query_t* const* qs = all_qs.data() + first;
    for (int i = 0; i < B; i++) {
      need(a.queries[g0 + i] != nullptr, "null argument");
      query_begin_opened(qs[i], a.queries[g0 + i], a.query_lens[g0 + i], a.db);
    }
    debug_stage(2);
    Workspace& W0 = group_pass_stream(qs, B);
    if (prev_pass) HIP_CHECK(hipStreamWaitEvent(W0.stream, prev_pass, 0));
    sparse_group_pass(*a.db, qs, B, W0.stream);
    group_pass_done(qs, 0);
    prev_pass = W0.ev[2];
    debug_stage(3);
    for (int i = 0; i < B; i++) {
      if (i > 0) group_pass_done(qs, i);
      qs[i]->ws->zero_shortcuts = true;   // lib/server's fold over a SparseDb (fold.rs:38-44)
      qs[i]->state = 2;
      run_finish(*qs[i]->ws, *qs[i]->pp, false);
    }
    prev_group = (size_t)B;
  }

  // the groups from `drained` on that reach the threshold; what is left of the list afterwards is the per-query flow's
  void run_groups(int group_min) {
    check_device(a.db->device);
    for (int g0 = (int)drained; a.batch - g0 >= group_min; g0 += SPARSE_GROUP_MAX) {
      keep_previous_group();
      group(g0, std::min(SPARSE_GROUP_MAX, a.batch - g0));
    }
    drain(all_qs.size());
  }

  int run(int group_min) {
    int rc = guarded([&] { run_groups(group_min); });
    if (rc == SP_E_OOM) {   // the rest of the list one query at a time, one workspace; responses already copied out stay
      abandon();
      (void)hipGetLastError();
      rc = SP_OK;
      for (; (int)drained < a.batch && rc == SP_OK; drained++)
        rc = sp_process_query(a.h, a.pps[drained], a.queries[drained], a.query_lens[drained], a.db, a.out + drained * a.out_stride,
                              a.out_stride, a.out_len);
      return rc;
    }
    if (rc != SP_OK) return fail(rc);
    if ((int)drained == a.batch) return SP_OK;
    BatchArgs rest = a;   // a last group below the threshold: up to `batch_in_flight` queries in flight
    rest.pps += drained;
    rest.queries += drained;
    rest.query_lens += drained;
    rest.batch -= (int)drained;
    rest.out += drained * a.out_stride;
    return answer_in_flight(rest);
  }
};

int answer_sparse(const BatchArgs& a) {
  long m = tunable("sparse_batch_min", SPARSE_BATCH_MIN_DEFAULT);
  if (m < 0) m = SPARSE_BATCH_MIN_DEFAULT;   // (a negative value: the shipped default again, for a caller that had overridden it)
  const int group_min = (int)std::max(2L, m);
  if (m <= 0 || group_min > SPARSE_GROUP_MAX || a.batch < group_min || a.db->num_shards != 1 || a.db->col_G != 1)
    return answer_in_flight(a);
  if (a.out_stride < a.h->p.response_bytes()) {
    sp_set_last_error_("out_stride smaller than response_bytes");
    return SP_E_ARG;
  }
  const int rc = guarded([&] { check_device(a.db->device); });
  return rc != SP_OK ? rc : SparseGroupFlow(a).run(group_min);
}

}  // namespace

extern "C" int sp_process_query_batch(const sp_params_t* h, const sp_pp_t* const* pps, const uint8_t* const* queries,
                                      const size_t* query_lens, int batch, const sp_db_t* db, uint8_t* out, size_t out_stride,
                                      size_t* out_len) {
  if (!h || !pps || !queries || !query_lens || batch < 0 || !db || !out || !out_len) {
    sp_set_last_error_("null argument");
    return SP_E_ARG;
  }
  tunables_new_call();  // the switches below are read before the first guarded() section of this call
  const BatchArgs a{h, pps, queries, query_lens, batch, db, out, out_stride, out_len, std::chrono::steady_clock::now()};
  const bool batched = db->packed && db->num_shards == 1 && db->col_G == 1 && !tunable("no_batch_sweep", 0);
  if (db->sparse) return answer_sparse(a);
  // lists of any length: groups of up to 16, whatever the switches say now (a planar row shard is refused per query, as any shard)
  if (db->planar_resident && db->num_shards == 1) return answer_in_groups(a);
  if (batched) return answer_in_groups(a);
  const bool narrow = !db->packed && db->num_shards == 1 && db->col_G == 1 && !tunable("no_batch_sweep", 0);
  return narrow ? answer_narrow(a) : answer_in_flight(a);
}
