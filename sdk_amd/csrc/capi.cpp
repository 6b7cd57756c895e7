// extern "C" surface of libspiral_hip.so (include/spiral_hip.h).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>

#include "../../include/spiral_hip.h"
#include "pipeline.hpp"

using namespace spiral;

static thread_local std::string g_last_error;
static thread_local int g_last_rc = SP_OK;  // status of this thread's last guarded() section: what a constructor-style entry
                                             // point (returns a handle or null) failed with

template <typename F>
static int guarded(F&& f) {
  tunables_new_call();
  auto fail = [](int rc, const char* what) {
    g_last_error = what;
    g_last_rc = rc;
    return rc;
  };
  try {
    f();
    g_last_rc = SP_OK;
    return SP_OK;
  } catch (const ArgError& e) {
    return fail(SP_E_ARG, e.what());
  } catch (const OomError& e) {
    return fail(SP_E_OOM, e.what());
  } catch (const HipError& e) {
    return fail(SP_E_HIP, e.what());
  } catch (const std::bad_alloc&) {
    return fail(SP_E_OOM, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(SP_E_ARG, e.what());
  }
}
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
// status to report when a handle-returning entry point came back null
static int null_handle_rc() { return g_last_rc != SP_OK ? g_last_rc : SP_E_ARG; }

struct sp_query {
  sp_params* params = nullptr;
  const sp_pp* pp = nullptr;
  std::unique_ptr<Workspace> ws;
  int state = 0;  // 1 begun, 2 swept, 3 finished
  int next_plane = 0;  // sp_query_sweep_scatter_plane progress
  int next_fold_plane = 0;  // sp_query_fold_local_plane progress
  int rows_j0 = 0, rows_nj = 0;  // sp_query_begin_for_db on a row shard: only these first-dimension rows were expanded
  const sp_db* for_sparse = nullptr;  // begun for this sparse bucket: only the rows holding items were expanded
  std::shared_ptr<const sp_db::SparseIndex> sparse_index;  // ... with this snapshot of its index (kept until the query is freed)
  std::shared_ptr<const DevBuf<u64>> planar;  // the digit-planar copy a batched group's pass on this (first) workspace reads: pinned
                                              // until the query is freed, i.e. until after its stream has been synchronised
  float ms[4] = {0, 0, 0, 0};
  bool streams_idle = false;  // the owner has waited for the main stream after the last enqueue (which orders stream2's work before it)
  ~sp_query() {
    if (ws && params) {
      if (!streams_idle) {
        (void)hipStreamSynchronize(ws->stream);
        (void)hipStreamSynchronize(ws->stream2);
      }
      ws->pipelined = false;
      ws->have_sweep_span = false;
      ws->zero_shortcuts = false;
      params->release_ws(std::move(ws));
    }
  }
};

namespace {

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

void need(bool c, const char* msg) {
  if (!c) throw ArgError(msg);
}

// host u64 NTT words -> device u32
void upload_ntt(Workspace& W, const uint64_t* host, size_t words, DevBuf<u32>& dst, DevBuf<u64>& tmp) {
  tmp.ensure(words);
  dst.ensure(words);
  HIP_CHECK(hipMemcpyAsync(tmp.p, host, words * 8, hipMemcpyHostToDevice, W.stream));
  launch_u64_to_u32(dst.p, tmp.p, (long)words, W.stream);
}
void download_ntt(Workspace& W, const u32* src, size_t words, uint64_t* host, DevBuf<u64>& tmp) {
  tmp.ensure(words);
  launch_u32_to_u64(tmp.p, src, (long)words, W.stream);
  HIP_CHECK(hipMemcpyAsync(host, tmp.p, words * 8, hipMemcpyDeviceToHost, W.stream));
  HIP_CHECK(hipStreamSynchronize(W.stream));
}
void upload_raw(Workspace& W, const uint64_t* host, size_t words, DevBuf<u64>& dst) {
  dst.ensure(words);
  HIP_CHECK(hipMemcpyAsync(dst.p, host, words * 8, hipMemcpyHostToDevice, W.stream));
}
void download_raw(Workspace& W, const u64* src, size_t words, uint64_t* host) {
  HIP_CHECK(hipMemcpyAsync(host, src, words * 8, hipMemcpyDeviceToHost, W.stream));
  HIP_CHECK(hipStreamSynchronize(W.stream));
}

// the fold buffers of a stage-level fold export grown to `num_per` ciphertexts and `further` levels (the workspace was sized for
// the params' own num_per)
void ensure_stage_fold(Workspace& W, size_t num_per, size_t further) {
  const size_t two_t = 2 * W.P->t_gsw;
  W.ensure_expand();
  W.foldX.ensure(num_per * 2 * POLY_LEN);
  W.foldY.ensure(std::max<size_t>(num_per / 2, 1) * 2 * POLY_LEN);
  W.fold_dig.ensure(num_per * two_t * 2 * POLY_LEN);
  W.fold_ntt.ensure(std::max<size_t>(num_per / 2, 1) * 2 * 2 * POLY_LEN);
  W.fold_mats.ensure(further * 2 * 2 * two_t * 2 * POLY_LEN);
}

void check_device(int dev) {
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  if (cur != dev) throw ArgError("handle belongs to HIP device " + std::to_string(dev) + " but the current device is " + std::to_string(cur));
}

// what one workspace of a batched group may need, as the group planner and the planar copy estimate it: three times the
// first-dimension output (a rough bound; pooled workspaces only make it conservative)
size_t group_ws_bytes(const Params& p, int np_local) { return (size_t)3 * p.planes() * 4 * POLY_LEN * (size_t)np_local * sizeof(u32); }

// bits per plaintext coefficient (ceil log2 p) and bytes of an item per plane (params.rs:188-193) of the database encoder
size_t pt_bits(const Params& p) {
  size_t logp = 0;
  while (((u64)1 << logp) < p.pt_modulus) logp++;
  return logp;
}
size_t chunk_bytes(const Params& p) { return (p.db_item_size + p.planes() - 1) / p.planes(); }

// the encoder's view of `d`; the call sites add the window (win*, file_len), the row pairs (jp0, njp) and the single-item fields
DbEncodeDesc encode_desc(const sp_db& d) {
  const Params& p = d.params->p;
  DbEncodeDesc e{};
  e.db = d.words.p;
  e.db_item_size = (int)p.db_item_size;
  e.bytes_per_chunk = (int)chunk_bytes(p);
  e.logp = (int)pt_bits(p);
  e.pt_modulus = (u32)p.pt_modulus;
  e.planes = (int)p.planes();
  e.num_per = d.np_local;
  e.cm = d.colmap();
  e.dim0 = (int)p.dim0();
  e.j0 = d.j0;
  e.nj = d.nj;
  e.packed = d.packed;
  e.only_item = -1;
  return e;
}

// one item's bytes, zero padded to db_item_size, in the handle's upload buffer (caller holds mu)
const uint8_t* upload_item(sp_db& d, const uint8_t* data, size_t len) {
  const size_t n = d.params->p.db_item_size;
  d.upload.ensure(std::max<size_t>(n, 1));
  HIP_CHECK(hipMemset(d.upload.p, 0, n));
  if (len) h2d_sync(d.upload.p, data, len);
  return d.upload.p;
}

using PlanarPin = std::shared_ptr<const DevBuf<u64>>;

// One batched pass of the group qs[0 .. B) over `db`, run on the first query's stream: the database, the queries' operands and
// outputs; on the matrix cores the group's query digit table with the first workspace (allocated on its first batched call, then
// reused) and, for two query tiles, the digit-planar copy -- pinned in `pin`, which the caller holds until that stream has been
// synchronised.
SweepBatchDesc group_pass(const sp_db& db, sp_query_t* const* qs, int B, bool use_planar, PlanarPin& pin) {
  const Params& p = db.params->p;
  Workspace& W0 = *qs[0]->ws;
  SweepBatchDesc d{};
  d.db = db.words.p;
  d.batch = B;
  d.planes = (int)p.planes();
  d.num_per = db.np_local;
  d.dim0 = (int)p.dim0();
  d.j0 = db.j0;
  d.nj = db.nj;
  for (int i = 0; i < B; i++) {
    d.qv[i] = qs[i]->ws->qv.p;
    d.out[i] = qs[i]->ws->sweep_out.p;
  }
  if (sweep_batch_wants_mfma(d)) {
    W0.batch_rq.ensure(sweep_batch_rq_words(d.nj, sweep_batch_tiles(d.batch)));
    d.rq = W0.batch_rq.p;
    if (use_planar && sweep_batch_tiles(d.batch) == 2) pin = const_cast<sp_db&>(db).ensure_planar(W0.stream);
  }
  d.planar = pin ? reinterpret_cast<const unsigned char*>(pin->p) : nullptr;
  return d;
}

}  // namespace

// The digit-planar copy of a PACKED, unsharded database (sweep_planar.hpp): what the 9 .. 16-query pass reads.  Built by
// sp_db_prepare_batch (at load time) or on first use (one gather pass over the PACKED units), only when the device has the room for
// a second copy (8 bytes per word) beside the workspaces of two groups; null = keep to the PACKED kernels.
std::shared_ptr<const DevBuf<u64>> sp_db::ensure_planar(hipStream_t s) {
  std::lock_guard<std::mutex> lk(mu);
  if (tunable("batch_planar", 1) == 0) {   // switched off: the copy's memory goes back too (once no pass holds it)
    drop_planar();
    return nullptr;
  }
  if (planar_state == 1) return planar;
  if (planar_state == -1) return nullptr;
  const Params& p = params->p;
  if (!packed || sparse || num_shards != 1 || col_G != 1 || !sweep_planar_shape_ok(np_local, nj)) {
    planar_state = -1;
    return nullptr;
  }
  planar_state = -2;   // until the copy stands: a shortfall of memory is looked at again next time
  const size_t bytes = sweep_planar_bytes((int)p.planes(), np_local, nj);
  if (!planar) {   // (a copy that is not valid and not dropped is no pass's: rebuilt in place)
    size_t fr = 0, tot = 0;
    // room for the copy + the workspaces of two groups of 16 + 4 GiB
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < bytes + 32 * group_ws_bytes(p, np_local) + ((size_t)4 << 30)) {
      (void)hipGetLastError();
      return nullptr;
    }
    try {
      planar = std::make_shared<DevBuf<u64>>((bytes + 7) / 8);
    } catch (const OomError&) {
      return nullptr;
    }
  }
  launch_packed_to_planar(reinterpret_cast<unsigned char*>(planar->p), words.p, (int)p.planes(), np_local, nj, s);
  HIP_CHECK(hipStreamSynchronize(s));
  planar_state = 1;
  return planar;
}

// present items by column + the expansion schedule pruned to the rows that hold items: rebuilt when a NEW key has been
// added (the plan only when a new row became occupied); overwrites keep the snapshot
std::shared_ptr<const sp_db::SparseIndex> sp_db::ensure_sparse_index() {
  std::lock_guard<std::mutex> lk(mu);
  if (!index_dirty && sparse_index) return sparse_index;
  const Params& p = params->p;
  const size_t num_per = p.num_per(), dim0 = p.dim0();
  std::vector<int> ptr(num_per + 1, 0), rows(slot_of.size()), slots(slot_of.size());
  std::vector<char> row_set(dim0, 0);
  for (const auto& kv : slot_of) ptr[kv.first % num_per + 1]++;
  for (size_t i = 0; i < num_per; i++) ptr[i + 1] += ptr[i];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (const auto& kv : slot_of) {
    const size_t j = kv.first / num_per, ii = kv.first % num_per;  // full_idx = j * num_per + i (dot_product.rs:164)
    rows[fill[ii]] = (int)j;
    slots[fill[ii]] = (int)kv.second;
    fill[ii]++;
    row_set[j] = 1;
  }
  auto idx = std::make_shared<SparseIndex>();
  idx->col_ptr.ensure(ptr.size());
  idx->col_rows.ensure(std::max<size_t>(rows.size(), 1));
  idx->col_slots.ensure(std::max<size_t>(slots.size(), 1));
  upload_words(idx->col_ptr.p, ptr.data(), ptr.size() * sizeof(int));
  if (!rows.empty()) {
    upload_words(idx->col_rows.p, rows.data(), rows.size() * sizeof(int));
    upload_words(idx->col_slots.p, slots.data(), slots.size() * sizeof(int));
  }
  if (slots_cap == 0) polys.ensure(1);
  if (rows_dirty || !sparse_index || !sparse_index->plan)
    idx->plan = build_pruned_plan_rows(p, row_set);  // query_expansion.rs:263-280: set_dim0 = rows of the present items
  else
    idx->plan = sparse_index->plan;                  // same occupied rows: the schedule is shared with the old snapshot
  sparse_index = idx;
  index_dirty = false;
  rows_dirty = false;
  return sparse_index;
}

extern "C" {

const char* sp_last_error(void) { return g_last_error.c_str(); }

uint64_t sp_paths_taken(int reset) { return paths_taken(reset != 0); }
int sp_debug_set(const char* name, long value) {
  if (!name) return SP_E_ARG;
  set_tunable(name, value);
  return SP_OK;
}
// internal hooks for comm.cpp (not declared in the public header)
static thread_local int g_shard_split_hint = 1;   // 0 while a list of sharded queries is being enqueued
extern "C" void sp_shard_split_hint_(int on) { g_shard_split_hint = on; }
// group = 0 of sp_process_queries_sharded_batched: 8 where a group of 8 takes the scatter-form pass on this shard and the shard
// count is one where the batched list measured faster than the pipelined one (switch batch_scatter_max_g; profiles/sharded_batch_pass.md),
// else 1 = the per-query flow.  Depends on the shard's shape and the switches only: the same answer on every rank.
extern "C" int sp_scatter_group_choice_(const sp_db_t* db, int G) {
  if (!db || !db->packed || db->col_G != 1 || db->sparse || db->num_shards != G) return 1;
  SweepBatchDesc d{};
  d.batch = SWEEP_BATCH_MAX;
  d.num_per = db->np_local;
  d.nj = db->nj;
  tunables_new_call();
  return sweep_batch_scatter_ok(d, G) && G <= (int)tunable("batch_scatter_max_g", BATCH_SCATTER_MAX_G_DEFAULT) ? SWEEP_BATCH_MAX : 1;
}
void sp_set_last_error_(const char* msg) { g_last_error = msg ? msg : ""; }
void sp_note_path_(uint64_t bits) { note_path(bits); }

const char* sp_path_name(int bit) {
  static const char* names[] = {"sweep_packed_persist", "sweep_packed", "sweep_wide", "sweep_narrow", "sweep_batch",
                                "from_sweep4", "from_sweep1", "fold_fused", "fold_tail_delta", "fold_tail_literal",
                                "pipelined_fold_overlap", "expand_pruned", "pack_v1", "direct_upload", "scatter_out",
                                "from_sweep4_xcd_order", "fold_tail_persistent", "expand_round_one_launch", "sweep_sparse",
                                "rccl_in_library", "fold_wave", "cu_split_overlap", "expand_split", "pipe_class_split",
                                "sweep_batch_mfma", "custom_transport", "from_sweep_wave",
                                "fold_tail_batched", "sweep_ring", "sweep_batch_mfma_two_tiles", "fold_wave8", "sweep_batch_planar",
                                "expand_group", "expand_wave", "sweep_batch_scatter"};
  return bit >= 0 && bit < (int)(sizeof(names) / sizeof(names[0])) ? names[bit] : nullptr;
}

int sp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
int sp_set_device(int device) {
  return guarded([&] { HIP_CHECK(hipSetDevice(device)); });
}

// ------------------------------------------------------------------------------------ Params
sp_params_t* sp_params_from_json(const char* json) {
  sp_params_t* out = nullptr;
  int rc = guarded([&] {
    need(json != nullptr, "json is null");
    auto h = std::make_unique<sp_params>();
    h->p = Params::from_json(json);
    out = h.release();
  });
  return rc == SP_OK ? out : nullptr;
}
void sp_params_free(sp_params_t* p) { delete p; }

uint64_t sp_params_get(const sp_params_t* h, const char* name) {
  if (!h || !name) return UINT64_MAX;
  const Params& p = h->p;
  std::string s(name);
  if (s == "poly_len") return p.poly_len;
  if (s == "poly_len_log2") return p.poly_len_log2;
  if (s == "crt_count") return p.crt_count;
  if (s == "modulus") return p.modulus;
  if (s == "modulus_log2") return p.modulus_log2;
  if (s == "moduli0") return p.moduli[0];
  if (s == "moduli1") return p.moduli[1];
  if (s == "n") return p.n;
  if (s == "pt_modulus") return p.pt_modulus;
  if (s == "q2_bits") return p.q2_bits;
  if (s == "t_conv") return p.t_conv;
  if (s == "t_exp_left") return p.t_exp_left;
  if (s == "t_exp_right") return p.t_exp_right;
  if (s == "t_gsw") return p.t_gsw;
  if (s == "expand_queries") return p.expand_queries;
  if (s == "db_dim_1") return p.db_dim_1;
  if (s == "db_dim_2") return p.db_dim_2;
  if (s == "instances") return p.instances;
  if (s == "db_item_size") return p.db_item_size;
  if (s == "version") return p.version;
  if (s == "g") return p.g();
  if (s == "stop_round") return p.stop_round();
  if (s == "setup_bytes") return p.setup_bytes();
  if (s == "query_bytes") return p.query_bytes();
  if (s == "num_items") return p.num_items();
  if (s == "db_words") return p.db_words();
  if (s == "response_bytes") return p.response_bytes();
  return UINT64_MAX;
}

int sp_params_ntt_table(const sp_params_t* h, int crt, int which, uint64_t* out_n) {
  return guarded([&] {
    need(h && out_n && crt >= 0 && crt < 2 && which >= 0 && which < 4, "bad table selector");
    const u32* t = h->p.table(crt, which);
    for (size_t i = 0; i < POLY_LEN; i++) out_n[i] = t[i];
  });
}

// ---------------------------------------------------------------------------------------- DB
static sp_db_t* db_create_impl(const sp_params_t* h, int shard, int num_shards, bool by_columns) {
  sp_db_t* out = nullptr;
  int rc = guarded([&] {
    need(h != nullptr, "params is null");
    const Params& p = h->p;
    need(num_shards >= 1 && shard >= 0 && shard < num_shards, "bad shard");
    auto d = std::make_unique<sp_db>();
    d->params = h;
    HIP_CHECK(hipGetDevice(&d->device));
    if (by_columns) {
      need((num_shards & (num_shards - 1)) == 0 && p.num_per() % (size_t)num_shards == 0 && (size_t)num_shards <= p.num_per(),
           "column shards: num_shards must be a power of two dividing num_per");
      d->col_g = shard;
      d->col_G = num_shards;
      d->np_local = (int)(p.num_per() / num_shards);
      d->nj = (int)p.dim0();
      d->j0 = 0;
    } else {
      need(p.dim0() % (size_t)num_shards == 0, "dim0 not divisible by num_shards");
      need(num_shards <= SP_MAX_ROW_SHARDS, "at most SP_MAX_ROW_SHARDS (8) row shards: the partial residues are summed in 32 bits");
      d->shard = shard;
      d->num_shards = num_shards;
      d->nj = (int)(p.dim0() / num_shards);
      d->j0 = shard * d->nj;
      d->np_local = (int)p.num_per();
    }
    d->packed = db_can_pack(d->np_local, d->nj) && !tunable("db_unpacked", 0) ? 1 : 0;
    // db_contiguous (default 0): physically contiguous allocation.  It gives the sweep its best case in every process
    // (profiles/r02_sweep_experiments.md) but is NOT SAFE on this stack: memory that belonged to a FREED contiguous
    // allocation is zeroed some time after the next hipMalloc already owns it (stand-alone reproducer
    // scripts/ubench/contig_repro.hip modes 4-6, profiles/r03_contiguous_alloc.md) -- the next handle's uploads vanish.
    const size_t db_words = (db_bytes((int)p.planes(), d->np_local, d->nj, d->packed) + 7) / 8;
    d->words.alloc_streaming(db_words, tunable("db_contiguous", 0) != 0);
    // (How a multi-GiB hipMalloc happens to be backed moves the sweep by up to 9 % between processes; timing the read pattern on
    // several fresh allocations and keeping the fastest was tried in round 3 -- the candidates of ONE process differ by ~1 % --
    // and removed: profiles/r03_placement.md.)
    HIP_CHECK(hipMemset(d->words.p, 0, d->words.bytes()));  // an empty bucket: absent items are zero polynomials
    const_cast<sp_params*>(h)->device_state();
    out = d.release();
  });
  return rc == SP_OK ? out : nullptr;
}
// lib/server's SparseDb (lib/server/src/db/sparse_db.rs:5-48): an empty bucket that stores only the items written to it
sp_db_t* sp_db_create_sparse(const sp_params_t* h) {
  sp_db_t* out = nullptr;
  int rc = guarded([&] {
    need(h != nullptr, "params is null");
    const Params& p = h->p;
    need(p.expand_queries, "sparse buckets serve expanded queries (lib/server's sparse path, server.rs:31-33)");
    need(fused_fold_supported(p), "sparse buckets need gadget parameters the fused fold supports (3 <= t_gsw <= 32)");
    auto d = std::make_unique<sp_db>();
    d->params = h;
    HIP_CHECK(hipGetDevice(&d->device));
    d->sparse = true;
    d->nj = (int)p.dim0();
    d->np_local = (int)p.num_per();
    const_cast<sp_params*>(h)->device_state();
    out = d.release();
  });
  return rc == SP_OK ? out : nullptr;
}
size_t sp_db_sparse_items(const sp_db_t* d) {
  if (!d || !d->sparse) return 0;
  std::lock_guard<std::mutex> lk(const_cast<sp_db*>(d)->mu);
  return d->slot_of.size();
}

sp_db_t* sp_db_create(const sp_params_t* h, int shard, int num_shards) { return db_create_impl(h, shard, num_shards, false); }
sp_db_t* sp_db_create_columns(const sp_params_t* h, int shard, int num_shards) { return db_create_impl(h, shard, num_shards, true); }
void sp_db_free(sp_db_t* d) { delete d; }
size_t sp_db_device_bytes(const sp_db_t* d) { return d ? (d->sparse ? d->polys.bytes() : d->words.bytes()) : 0; }
size_t sp_db_batch_copy_bytes(const sp_db_t* d) {
  if (!d) return 0;
  std::lock_guard<std::mutex> lk(const_cast<sp_db*>(d)->mu);
  return d->planar_state == 1 ? d->planar->bytes() : 0;
}

int sp_db_load_plane(sp_db_t* d, int plane, int z0, int nz, const uint64_t* words) {
  return guarded([&] {
    need(d && words, "null argument");
    need(!d->sparse, "a sparse bucket is filled through sp_db_update_item");
    const Params& p = d->params->p;
    need(plane >= 0 && (size_t)plane < p.planes() && z0 >= 0 && nz >= 0 && (size_t)(z0 + nz) <= POLY_LEN, "bad plane / z range");
    check_device(d->device);
    sp_db::WriteScope write(*d);
    const size_t row_words = p.num_per() * p.dim0();
    const size_t max_stage = ((size_t)64 << 20) / 8;  // 64 MiB windows
    const int zs = (int)std::max<size_t>(1, std::min<size_t>((size_t)nz, max_stage / row_words));
    d->upload.ensure((size_t)zs * row_words * 8);
    const u64* stage = reinterpret_cast<const u64*>(d->upload.p);
    for (int z = 0; z < nz; z += zs) {
      const int cnt = std::min(zs, nz - z);
      h2d_sync(d->upload.p, words + (size_t)z * row_words, (size_t)cnt * row_words * 8);
      launch_db_relayout(d->words.p, plane, stage, z0 + z, cnt, d->np_local, (int)p.dim0(), d->j0, d->nj,
                         d->packed, d->colmap(), 0);
      HIP_CHECK(hipDeviceSynchronize());
    }
  });
}

int sp_db_load(sp_db_t* d, const uint64_t* words, size_t n_words) {
  if (!d || !words) {
    g_last_error = "null argument";
    return SP_E_ARG;
  }
  const Params& p = d->params->p;
  if (n_words != p.db_words()) {
    g_last_error = "db word count " + std::to_string(n_words) + " != " + std::to_string(p.db_words());
    return SP_E_ARG;
  }
  const size_t plane_words = POLY_LEN * p.num_items();
  for (size_t pl = 0; pl < p.planes(); pl++) {
    int rc = sp_db_load_plane(d, (int)pl, 0, (int)POLY_LEN, words + pl * plane_words);
    if (rc != SP_OK) return rc;
  }
  return SP_OK;
}

int sp_db_load_items(sp_db_t* d, const uint8_t* file, size_t file_len) {
  return guarded([&] {
    need(d && (file || file_len == 0), "null argument");
    need(!d->sparse, "a sparse bucket is filled through sp_db_update_item");
    check_device(d->device);
    sp_params* h = const_cast<sp_params*>(d->params);
    const Params& p = h->p;
    DeviceState& D = h->device_state();
    sp_db::WriteScope write(*d);
    const size_t logp = pt_bits(p), chunks = p.planes(), bpc = chunk_bytes(p);
    need((bpc * 8 + logp - 1) / logp <= POLY_LEN, "item chunk does not fit one polynomial (server.rs:292)");
    need(logp >= 1 && logp <= 28, "plaintext modulus out of range");
    // windows of whole row pairs: the rows' items are contiguous in the file
    const size_t row_bytes = p.num_per() * p.db_item_size;
    const int npairs_total = (d->nj + 1) / 2;
    const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));  // bytes of raw items per upload
    const int pairs_per_win = (int)std::max<size_t>(1, std::min<size_t>((size_t)npairs_total, max_win / (2 * row_bytes)));
    // + tail: the chunks of an item cover chunks * bytes_per_chunk >= db_item_size bytes of the file, i.e. the last
    // chunk(s) of an item read into the NEXT item(s) (load_item_from_seek, server.rs:300-309) -- also for the last item
    // of a window.  The spill is chunks * bpc - db_item_size bytes, which exceeds one chunk when
    // db_item_size < (chunks - 1) * bpc (5-byte items in 4 chunks: bpc = 2, spill = 3).
    const size_t tail = std::max(bpc, chunks * bpc - p.db_item_size);
    d->upload.ensure((size_t)pairs_per_win * 2 * row_bytes + tail);   // kept: up to db_load_window + tail per handle
    for (int jp = 0; jp < npairs_total; jp += pairs_per_win) {
      const int cnt = std::min(pairs_per_win, npairs_total - jp);
      const size_t item0 = (size_t)(d->j0 + 2 * jp) * p.num_per();
      const size_t off = item0 * p.db_item_size;
      size_t want = (size_t)cnt * 2 * row_bytes + tail;
      size_t have = off < file_len ? std::min(want, file_len - off) : 0;
      if (have) h2d_sync(d->upload.p, file + off, have);
      DbEncodeDesc e = encode_desc(*d);
      e.win = d->upload.p;
      e.win_item0 = item0;
      e.win_bytes = have;
      e.file_len = file_len;
      e.jp0 = jp;
      e.njp = cnt;
      launch_db_encode(D.T, e, 0);
      HIP_CHECK(hipDeviceSynchronize());
    }
  });
}

int sp_db_update_item(sp_db_t* d, size_t item_idx, const uint8_t* data, size_t len) {
  return guarded([&] {
    need(d && (data || len == 0), "null argument");
    check_device(d->device);
    sp_params* h = const_cast<sp_params*>(d->params);
    const Params& p = h->p;
    need(item_idx < p.num_items(), "item index out of range");
    need(len <= p.db_item_size, "item longer than db_item_size");
    if (d->sparse) {
      // lib/server/src/db/loading.rs:317-359 update_item_raw + sparse_db.rs:42-48 upsert
      DeviceState& D = h->device_state();
      std::lock_guard<std::mutex> lk(d->mu);
      const size_t planes = p.planes(), poly_words = planes * POLY_LEN;
      auto it = d->slot_of.find(item_idx);
      size_t slot;
      bool new_key = false;
      if (it != d->slot_of.end()) {
        slot = it->second;
      } else {
        new_key = true;
        slot = d->slot_of.size();
        if (slot >= d->slots_cap) {  // grow the polynomial store (amortised doubling, contents preserved)
          const size_t cap = std::max<size_t>(64, d->slots_cap * 2);
          DevBuf<u64> bigger(cap * poly_words);
          if (d->slots_cap) HIP_CHECK(hipMemcpy(bigger.p, d->polys.p, d->slots_cap * poly_words * 8, hipMemcpyDeviceToDevice));
          if (d->slots_cap && tunable("h2d_cache_sync", 0) != 0) launch_cache_sync(nullptr, 0);  // (as h2d_sync)
          d->polys = std::move(bigger);
          d->slots_cap = cap;
        }
        if (!d->rows_dirty) {  // does the item open a new first-dimension row?  (then the pruned expansion plan changes)
          const size_t j_new = item_idx / p.num_per();
          bool row_known = false;
          for (const auto& kv : d->slot_of)
            if (kv.first / p.num_per() == j_new) { row_known = true; break; }
          if (!row_known) d->rows_dirty = true;
        }
        d->slot_of[item_idx] = slot;
      }
      launch_sparse_item_encode(D.T, upload_item(*d, data, len), (int)p.db_item_size, (int)chunk_bytes(p), (int)pt_bits(p),
                                (u32)p.pt_modulus, d->polys.p + slot * poly_words, (int)planes, 0);
      HIP_CHECK(hipDeviceSynchronize());
      if (new_key) d->index_dirty = true;   // an overwrite (the reference's upsert of an existing key) leaves the index alone
      return;
    }
    const size_t j = item_idx / p.num_per(), ii = item_idx % p.num_per();
    if ((int)j < d->j0 || (int)j >= d->j0 + d->nj) return;  // row lives on another shard
    if ((int)(ii % (size_t)d->col_G) != d->col_g) return;   // column lives on another shard
    DeviceState& D = h->device_state();
    std::lock_guard<std::mutex> lk(d->mu);
    DbEncodeDesc e = encode_desc(*d);
    e.win = upload_item(*d, data, len);
    e.win_item0 = item_idx;
    e.win_bytes = p.db_item_size;
    e.file_len = (item_idx + 1) * p.db_item_size;  // the record itself is complete (zero padded)
    e.jp0 = (int)(j - d->j0) / 2;
    e.njp = 1;
    e.only_item = (long)item_idx;
    e.only_q = (int)((ii / (size_t)d->col_G) / 2);
    launch_db_encode(D.T, e, 0);
    // a planar copy follows the item: its 8 entries per (plane, z), regathered from the words just written (same stream) -- an
    // upsert costs 64 KiB of writes, not a 64 GiB rebuild by the next group of 9 .. 16 queries
    if (d->planar_state == 1)
      launch_planar_patch_item(reinterpret_cast<unsigned char*>(d->planar->p), d->words.p, (int)p.planes(), d->np_local, d->nj,
                               (int)j - d->j0, (int)(ii / (size_t)d->col_G), 0);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int sp_db_fill_synthetic(sp_db_t* d, uint64_t seed) {
  return guarded([&] {
    need(d != nullptr, "null db");
    need(!d->sparse, "a sparse bucket is filled through sp_db_update_item");
    check_device(d->device);
    sp_db::WriteScope write(*d);
    const Params& p = d->params->p;
    launch_db_synth(d->words.p, seed, (int)p.planes(), d->np_local, (int)p.dim0(), d->j0, d->nj, d->packed, d->colmap(), 0);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// Everything a database needs for batched calls, built now instead of inside the first sp_process_query_batch of 9 .. 16 queries:
// the digit-planar copy of a PACKED, unsharded database (+ 8 bytes per word; sweep_planar.hpp) when the shape has one and the
// device has the room.  *built (optional): 1 = the copy stands, 0 = this database keeps to the PACKED kernels.
int sp_db_prepare_batch(sp_db_t* d, int* built) {
  return guarded([&] {
    need(d != nullptr, "null db");
    check_device(d->device);
    const bool c = !d->sparse && d->ensure_planar(nullptr);
    if (built) *built = c;
  });
}
uint64_t sp_synth_word(uint64_t seed, uint64_t ref_index) { return synth_word(seed, ref_index); }

int sp_db_read_ref(const sp_db_t* d, int plane, int z, int ii, int j0, int count, uint64_t* out) {
  return guarded([&] {
    need(d && out, "null argument");
    need(!d->sparse, "sp_db_read_ref reads dense databases");
    const Params& p = d->params->p;
    need(plane >= 0 && (size_t)plane < p.planes() && z >= 0 && z < N && ii >= 0 && (size_t)ii < p.num_per() && j0 >= 0 &&
             count >= 0 && j0 + count <= d->nj, "bad coordinates");
    need(ii % d->col_G == d->col_g, "column is held by another shard");
    check_device(d->device);
    DevBuf<u64> tmp((size_t)std::max(count, 1));
    launch_db_read(tmp.p, d->words.p, plane, z, ii / d->col_G, j0, count, d->np_local, d->nj, d->packed, 0);
    HIP_CHECK(hipMemcpy(out, tmp.p, (size_t)count * 8, hipMemcpyDeviceToHost));
  });
}

// ------------------------------------------------------------------------- PublicParameters
sp_pp_t* sp_pp_deserialize(const sp_params_t* h, const uint8_t* data, size_t len) {
  sp_pp_t* out = nullptr;
  int rc = guarded([&] {
    need(h && data, "null argument");
    const Params& p = h->p;
    if (len != p.setup_bytes()) throw ArgError("public parameter length " + std::to_string(len) + " != setup_bytes " + std::to_string(p.setup_bytes()));
    DeviceState& D = const_cast<sp_params*>(h)->device_state();
    auto pp = std::make_unique<sp_pp>();
    pp->params = h;
    pp->device = D.device;
    struct Mat { size_t count, rows, cols; };
    std::vector<Mat> mats;
    mats.push_back({p.n, p.n + 1, p.t_conv});  // client.rs:221
    size_t off = p.n * (p.n + 1) * p.t_conv;
    pp->off_packing = 0;
    if (p.expand_queries) {
      pp->off_left = off;
      mats.push_back({p.g(), 2, p.t_exp_left});
      off += p.g() * 2 * p.t_exp_left;
      pp->has_right = p.has_expansion_right_on_wire();
      if (pp->has_right) {
        pp->off_right = off;
        mats.push_back({p.stop_round() + 1, 2, p.t_exp_right});
        off += (p.stop_round() + 1) * 2 * p.t_exp_right;
      } else {
        pp->off_right = pp->off_left;
      }
      pp->off_conv = off;
      mats.push_back({1, 2, 2 * p.t_conv});
      off += 2 * 2 * p.t_conv;
    }
    pp->n_polys = off;
    // host raw image: row 0 of every matrix from the seed stream, the rest from the wire
    size_t rng_words = 0;
    for (auto& m : mats) rng_words += m.count * m.cols * POLY_LEN;
    std::vector<u64> ks(rng_words);
    chacha20_keystream_u64(data, ks.data(), rng_words);
    std::vector<u64> raw(off * POLY_LEN);
    size_t kpos = 0, wpos = SEED_LENGTH, ppos = 0;
    for (auto& m : mats)
      for (size_t i = 0; i < m.count; i++) {
        u64* dst = raw.data() + ppos * POLY_LEN;
        const size_t first = m.cols * POLY_LEN;
        for (size_t k = 0; k < first; k++) dst[k] = p.modulus - (ks[kpos + k] % p.modulus);  // client.rs:47-49
        kpos += first;
        const size_t rest = (m.rows - 1) * m.cols * POLY_LEN;
        memcpy(dst + first, data + wpos, rest * 8);
        wpos += rest * 8;
        ppos += m.rows * m.cols;
      }
    need(wpos == len && ppos == off, "internal: pp layout mismatch");
    DevBuf<u64> d_raw(raw.size());
    h2d_sync(d_raw.p, raw.data(), raw.size() * 8);
    pp->all.alloc(off * 2 * POLY_LEN);
    FwdDesc f{d_raw.p, nullptr, pp->all.p, (int)off, 1, 1, 1, 64, 1, 0, 1};  // to_ntt_alloc (client.rs:244-247)
    launch_ntt_fwd(D.T, f, 0);
    // [W_0 | W_1 | ...] for pack (server.rs:450-463)
    const size_t n = p.n, tc = p.t_conv;
    pp->pack_cat.alloc((n + 1) * n * tc * 2 * POLY_LEN);
    for (size_t rr = 0; rr < n + 1; rr++)
      for (size_t r = 0; r < n; r++)  // (copy kernel, not a copy-engine transfer: see upload_words)
        launch_copy_words(pp->pack_cat.p + (rr * n * tc + r * tc) * 2 * POLY_LEN,
                          pp->all.p + (pp->off_packing + r * (n + 1) * tc + rr * tc) * 2 * POLY_LEN, tc * 2 * POLY_LEN, 0);
    if (p.expand_queries) {   // wave-layout copy + the constants 0 | 1 (k_expand_wave)
      pp->all_w.alloc((off + 1) * 2 * POLY_LEN);
      launch_mats_to_wave(pp->all_w.p, pp->all.p, off * 2 * POLY_LEN, 0);
      std::vector<u32> zero_one(2 * POLY_LEN, 0u);
      for (size_t i = POLY_LEN; i < 2 * POLY_LEN; i++) zero_one[i] = 1u;
      h2d_sync(pp->all_w.p + off * 2 * POLY_LEN, zero_one.data(), zero_one.size() * sizeof(u32));
    }
    HIP_CHECK(hipDeviceSynchronize());
    out = pp.release();
  });
  return rc == SP_OK ? out : nullptr;
}
void sp_pp_free(sp_pp_t* p) { delete p; }

int sp_pp_export(const sp_pp_t* pp, uint64_t* out, size_t cap_words, size_t* n_words) {
  return guarded([&] {
    need(pp && out && n_words, "null argument");
    check_device(pp->device);
    const size_t words = pp->n_polys * 2 * POLY_LEN;
    *n_words = words;
    need(cap_words >= words, "output too small");
    Scoped W(pp->params);
    DevBuf<u64> tmp;
    download_ntt(*W, pp->all.p, words, out, tmp);
  });
}

// ------------------------------------------------------------------------------ process_query
// a query object with its workspace, nothing enqueued yet but the "begin" event (the group flow of sp_process_query_batch, which
// expands its queries together: run_begin_group); state 0 until the caller has begun it
static sp_query_t* query_open(const sp_params_t* h, const sp_pp_t* pp) {
  sp_query_t* out = nullptr;
  int rc = guarded([&] {
    need(h && pp, "null argument");
    need(pp->params == h, "public parameters were created for different params");
    check_device(pp->device);
    auto q = std::make_unique<sp_query>();
    q->params = const_cast<sp_params*>(h);
    q->pp = pp;
    q->ws = q->params->acquire_ws();
    HIP_CHECK(hipEventRecord(q->ws->ev[0], q->ws->stream));
    out = q.release();
  });
  return rc == SP_OK ? out : nullptr;
}

sp_query_t* sp_query_begin(const sp_params_t* h, const sp_pp_t* pp, const uint8_t* query, size_t query_len) {
  return sp_query_begin_for_db(h, pp, query, query_len, nullptr);
}

sp_query_t* sp_query_begin_for_db(const sp_params_t* h, const sp_pp_t* pp, const uint8_t* query, size_t query_len,
                                  const sp_db_t* db) {
  sp_query_t* out = nullptr;
  int rc = guarded([&] {
    need(h && pp && query, "null argument");
    need(pp->params == h, "public parameters were created for different params");
    need(!db || db->params == h, "db was created for different params");
    check_device(pp->device);
    const bool rows = db && db->num_shards > 1 && db->col_G == 1;
    const DeviceState::PrunedPlan* plan = nullptr;
    std::shared_ptr<const sp_db::SparseIndex> snap;
    if (db && db->sparse) {
      snap = const_cast<sp_db*>(db)->ensure_sparse_index();
      plan = snap->plan.get();
    }
    auto q = std::make_unique<sp_query>();
    q->sparse_index = snap;
    q->params = const_cast<sp_params*>(h);
    q->pp = pp;
    q->ws = q->params->acquire_ws();
    Workspace& W = *q->ws;
    HIP_CHECK(hipEventRecord(W.ev[0], W.stream));
    // a long (per-plane, pipelined) sweep follows: worth moving the fold's half of the expansion off the critical path
    // (r06: also before the per-plane sweeps of a ROW SHARD -- the multi-GPU flows: the even subtree, pruned to the shard's rows,
    // is short there, and the odd subtree + GSW side, which only the fold needs, then runs beside the sweeps and their exchanges
    // instead of in front of them; switch expand_split_shards)
    // NOT for a LIST of sharded queries (sp_process_queries_sharded): query k + 1 already expands under query k's sweeps there,
    // and its odd subtree beside its own sweeps costs them more than it saves -- measured, one rank of 8 alone with a null
    // transport: 2.59-2.64 -> 2.45-2.56 ms per query one at a time, 2.09-2.13 -> 2.38 in a list (profiles/r06_rank_critical_path.md);
    // comm.cpp says which it is through sp_shard_split_hint_
    const bool shard_planes = rows && db->packed && h->p.planes() > 1 && h->p.num_per() >= 1024 && g_shard_split_hint != 0 &&
                              tunable("expand_split_shards", 1) != 0;
    W.long_sweep_follows = db && !db->sparse && (sweep_is_pipelined(h->p, *db) || shard_planes);
    debug_stage(1);
    if (tunable("query_cache_sync", 0) != 0) launch_cache_sync(nullptr, W.stream);  // diagnostic: L2 write-back + invalidate per query
    run_begin(W, *pp, query, query_len, rows ? db->j0 : 0, rows ? db->nj : 0, plan);
    W.long_sweep_follows = false;
    HIP_CHECK(hipEventRecord(W.ev[1], W.stream));
    q->state = 1;
    q->for_sparse = db && db->sparse ? db : nullptr;
    q->rows_j0 = rows ? db->j0 : 0;
    q->rows_nj = rows ? db->nj : 0;
    out = q.release();
  });
  return rc == SP_OK ? out : nullptr;
}

int sp_query_sweep(sp_query_t* q, const sp_db_t* db) {
  return guarded([&] {
    need(q && db, "null argument");
    need(q->state == 1, "sp_query_sweep: query not in 'begun' state");
    need(db->params == q->params, "db was created for different params");
    need(q->rows_nj == 0 || (db->col_G == 1 && db->j0 == q->rows_j0 && db->nj == q->rows_nj),
         "the query was expanded for another row shard (sp_query_begin_for_db)");
    check_device(db->device);
    Workspace& W = *q->ws;
    need(q->for_sparse == nullptr || q->for_sparse == db, "the query was expanded for another sparse bucket");
    debug_stage(2);
    if (db->sparse) {
      // lib/server's process_query over a SparseDb (lib/server/src/server.rs:17-99): present items only, and the
      // fold takes fold.rs:38-44's all-zero shortcuts
      need(q->for_sparse == db && q->sparse_index, "a sparse bucket needs sp_query_begin_for_db(…, db) (its expansion is pruned)");
      // the snapshot the expansion was pruned with (items written after sp_query_begin are not part of this query)
      run_sweep_sparse(W, *db, q->sparse_index->col_ptr.p, q->sparse_index->col_rows.p, q->sparse_index->col_slots.p);
      W.zero_shortcuts = true;
    } else if (sweep_is_pipelined(q->params->p, *db))
      run_sweep_pipelined(W, *db);
    else
      run_sweep(W, *db);
    HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
    q->state = 2;
  });
}

int sp_query_sweep_scatter(sp_query_t* q, const sp_db_t* db, int G) {
  return guarded([&] {
    need(q && db, "null argument");
    need(q->state == 1, "sp_query_sweep_scatter: query not in 'begun' state");
    need(db->params == q->params, "db was created for different params");
    need(q->rows_nj == 0 || (db->col_G == 1 && db->j0 == q->rows_j0 && db->nj == q->rows_nj),
         "the query was expanded for another row shard (sp_query_begin_for_db)");
    const Params& p = q->params->p;
    need(G >= 1 && (G & (G - 1)) == 0 && (size_t)G <= p.num_per() && db->num_shards == G && G <= SP_MAX_ROW_SHARDS,
         "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS) and equal to the db's num_shards");
    need(db->col_G == 1 && !db->sparse, "sweep_scatter works on row shards");
    check_device(db->device);
    Workspace& W = *q->ws;
    W.out_G = G;
    run_sweep(W, *db);
    W.out_G = 1;
    HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
    q->state = 2;
  });
}

int sp_query_sweep_scatter_plane(sp_query_t* q, const sp_db_t* db, int G, int plane) {
  return guarded([&] {
    need(q && db, "null argument");
    need(db->params == q->params, "db was created for different params");
    need(q->rows_nj == 0 || (db->col_G == 1 && db->j0 == q->rows_j0 && db->nj == q->rows_nj),
         "the query was expanded for another row shard (sp_query_begin_for_db)");
    const Params& p = q->params->p;
    need(G >= 1 && (G & (G - 1)) == 0 && (size_t)G <= p.num_per() && db->num_shards == G && G <= SP_MAX_ROW_SHARDS,
         "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS) and equal to the db's num_shards");
    need(db->col_G == 1 && !db->sparse, "sweep_scatter works on row shards");
    need(plane >= 0 && (size_t)plane < p.planes(), "plane out of range");
    need(q->state == 1 && q->next_plane == plane, "sp_query_sweep_scatter_plane: planes must be swept in order after begin");
    check_device(db->device);
    Workspace& W = *q->ws;
    W.ensure_sweep();
    W.out_G = G;
    try {
      launch_plane_sweep(W, *db, (size_t)plane);
    } catch (...) {
      W.out_G = 1;
      throw;
    }
    W.out_G = 1;
    q->next_plane = plane + 1;
    if ((size_t)q->next_plane == p.planes()) {
      HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
      q->state = 2;
    }
  });
}

// One pass over the row shard for a whole group (the stage between sp_query_begin_for_db and sp_query_fold_local of the batched
// sharded list, comm.cpp).  Checks first, nothing enqueued on an error.
static void scatter_group_check(sp_query_t* const* qs, int batch, const sp_db_t* db, int G) {
  need(qs && db, "null argument");
  need(batch >= 1 && batch <= SWEEP_BATCH_MAX, "sp_query_sweep_scatter_group: 1 .. 8 queries per pass");
  const Params& p = db->params->p;
  need(db->col_G == 1 && !db->sparse, "sweep_scatter works on row shards");
  need(G >= 1 && (G & (G - 1)) == 0 && (size_t)G <= p.num_per() && db->num_shards == G && G <= SP_MAX_ROW_SHARDS,
       "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS) and equal to the db's num_shards");
  for (int i = 0; i < batch; i++) {
    need(qs[i] && qs[i]->ws, "null query");
    need(qs[i]->params == db->params, "db was created for different params");
    need(qs[i]->rows_nj == 0 || (db->j0 == qs[i]->rows_j0 && db->nj == qs[i]->rows_nj),
         "the query was expanded for another row shard (sp_query_begin_for_db)");
    for (int k = 0; k < i; k++) need(qs[k] != qs[i], "sp_query_sweep_scatter_group: the same query twice");
  }
  check_device(db->device);
}
// the group's pass in the reduce-scatter layout on the first query's stream (prepared descriptor); false: this group or shape is
// not the matrix-core pass's -- the caller sweeps per query
static bool scatter_group_desc(sp_query_t* const* qs, int batch, const sp_db_t* db, int G, SweepBatchDesc& d) {
  for (int i = 0; i < batch; i++) qs[i]->ws->ensure_sweep();
  if (!db->packed || G < 2) return false;
  PlanarPin none;
  d = group_pass(*db, qs, batch, false, none);
  return d.rq != nullptr && sweep_batch_scatter_ok(d, G);
}

int sp_query_sweep_scatter_group(sp_query_t* const* qs, int batch, const sp_db_t* db, int G) {
  return guarded([&] {
    scatter_group_check(qs, batch, db, G);
    for (int i = 0; i < batch; i++)
      need(qs[i]->state == 1 && qs[i]->next_plane == 0, "sp_query_sweep_scatter_group: every query must be in 'begun' state, no plane swept");
    const size_t planes = db->params->p.planes();
    SweepBatchDesc d{};
    if (scatter_group_desc(qs, batch, db, G, d)) {
      // ordered after every query's expansion (ev[1], recorded by sp_query_begin_for_db on the query's stream; the operand of
      // the pass, qv, is written on that stream also when the odd subtree was split off) ...
      Workspace& W0 = *qs[0]->ws;
      for (int i = 1; i < batch; i++) HIP_CHECK(hipStreamWaitEvent(W0.stream, qs[i]->ws->ev[1], 0));
      sweep_batch_prepare(W0.D->T, d, W0.stream);
      launch_sweep_batch_scatter(W0.D->T, d, G, W0.stream);
      HIP_CHECK(hipEventRecord(W0.ev[2], W0.stream));
      // ... and every query's own stream after the pass
      for (int i = 1; i < batch; i++) {
        Workspace& W = *qs[i]->ws;
        HIP_CHECK(hipStreamWaitEvent(W.stream, W0.ev[2], 0));
        HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
      }
    } else {
      // groups of 1 .. 3, rows that are not whole 32-row blocks, 8-byte databases, batch_mfma = 0: the per-query scatter sweep
      for (int i = 0; i < batch; i++) {
        Workspace& W = *qs[i]->ws;
        W.out_G = G;
        try {
          for (size_t pl = 0; pl < planes; pl++) launch_plane_sweep(W, *db, pl);
        } catch (...) {
          W.out_G = 1;
          throw;
        }
        W.out_G = 1;
        HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
      }
    }
    for (int i = 0; i < batch; i++) {
      qs[i]->next_plane = (int)planes;
      qs[i]->state = 2;
    }
  });
}

int sp_query_fold_local(sp_query_t* q, const void* reduced_chunk, int G) {
  return guarded([&] {
    need(q && reduced_chunk, "null argument");
    need(q->state == 2, "sp_query_fold_local: sweep has not run");
    const Params& p = q->params->p;
    need(G >= 1 && (G & (G - 1)) == 0 && (size_t)G <= p.num_per() && G <= SP_MAX_ROW_SHARDS,
         "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS)");
    run_fold_local(*q->ws, (const u32*)reduced_chunk, G);
    q->state = 4;
  });
}
int sp_query_fold_local_plane(sp_query_t* q, const void* reduced_plane_chunk, int G, int plane) {
  return guarded([&] {
    need(q && reduced_plane_chunk, "null argument");
    const Params& p = q->params->p;
    need(G >= 1 && (G & (G - 1)) == 0 && (size_t)G <= p.num_per() && G <= SP_MAX_ROW_SHARDS,
         "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS)");
    need(plane >= 0 && (size_t)plane < p.planes(), "plane out of range");
    // plane `plane` must have been swept (its exchange is the caller's to order on sp_query_stream2)
    need((q->state == 1 && plane < q->next_plane) || q->state == 2, "sp_query_fold_local_plane: plane has not been swept");
    need(plane == q->next_fold_plane, "sp_query_fold_local_plane: planes must be folded in order");
    run_fold_local_plane(*q->ws, (const u32*)reduced_plane_chunk, G, plane);
    q->next_fold_plane = plane + 1;
  });
}

int sp_query_fold_local_join(sp_query_t* q) {
  return guarded([&] {
    need(q, "null argument");
    need(q->state == 2 && (size_t)q->next_fold_plane == q->params->p.planes(),
         "sp_query_fold_local_join: every plane must have been swept and folded");
    run_fold_local_join(*q->ws);
    q->state = 4;
  });
}

void* sp_query_stream2(sp_query_t* q) { return q && q->ws ? (void*)q->ws->stream2 : nullptr; }

void* sp_query_local_cts_ptr(sp_query_t* q) { return q && q->ws ? (void*)q->ws->final_cts.p : nullptr; }
size_t sp_query_local_cts_words(const sp_query_t* q) { return q ? q->params->p.planes() * 2 * POLY_LEN : 0; }

int sp_query_finish_gathered(sp_query_t* q, const void* gathered, int G, uint8_t* out, size_t out_cap, size_t* out_len) {
  return guarded([&] {
    need(q && gathered && out && out_len, "null argument");
    need(q->state == 4, "sp_query_finish_gathered: local fold has not run");
    const Params& p = q->params->p;
    need(out_cap >= p.response_bytes(), "output buffer smaller than response_bytes");
    Workspace& W = *q->ws;
    run_finish_gathered(W, *q->pp, (const u64*)gathered, G);
    HIP_CHECK(hipStreamSynchronize(W.stream));
    memcpy(out, W.h_response, p.response_bytes());
  *out_len = p.response_bytes();
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, W.ev[0], W.ev[1]));
    q->ms[0] = t;
    HIP_CHECK(hipEventElapsedTime(&t, W.ev[1], W.ev[2]));
    q->ms[1] = t;
    HIP_CHECK(hipEventElapsedTime(&t, W.ev[2], W.ev[3]));
    q->ms[2] = t;
    HIP_CHECK(hipEventElapsedTime(&t, W.ev[3], W.ev[4]));
    q->ms[3] = t;
    q->state = 3;
  });
}

void* sp_query_partial_ptr(sp_query_t* q) {
  if (!q || !q->ws) return nullptr;
  // valid before the first sweep too (callers set up their exchange buffers up front)
  if (guarded([&] { q->ws->ensure_sweep(); }) != SP_OK) return nullptr;
  return (void*)q->ws->sweep_out.p;
}
size_t sp_query_partial_words(const sp_query_t* q) {
  if (!q) return 0;
  const Params& p = q->params->p;
  return p.planes() * 4 * POLY_LEN * p.num_per();
}
void* sp_query_stream(sp_query_t* q) { return q && q->ws ? (void*)q->ws->stream : nullptr; }

int sp_query_sync(sp_query_t* q) {
  return guarded([&] {
    need(q && q->ws, "null query");
    HIP_CHECK(hipStreamSynchronize(q->ws->stream));
    HIP_CHECK(hipStreamSynchronize(q->ws->stream2));
  });
}

static void finish_impl(sp_query_t* q, bool premod, uint8_t* out, size_t out_cap, size_t* out_len) {
  need(q && out && out_len, "null argument");
  need(q->state == 2, "sp_query_finish: sweep has not run");
  const Params& p = q->params->p;
  need(out_cap >= p.response_bytes(), "output buffer smaller than response_bytes");
  Workspace& W = *q->ws;
  debug_stage(3);
  run_finish(W, *q->pp, premod);
  HIP_CHECK(hipStreamSynchronize(W.stream));
  memcpy(out, W.h_response, p.response_bytes());
  *out_len = p.response_bytes();
  float t = 0;
  HIP_CHECK(hipEventElapsedTime(&t, W.ev[0], W.ev[1]));
  q->ms[0] = t;
  HIP_CHECK(hipEventElapsedTime(&t, W.ev[1], W.ev[2]));
  q->ms[1] = t;
  HIP_CHECK(hipEventElapsedTime(&t, W.ev[2], W.ev[3]));
  q->ms[2] = t;
  HIP_CHECK(hipEventElapsedTime(&t, W.ev[3], W.ev[4]));
  q->ms[3] = t;
  if (W.have_sweep_span) {
    // pipelined sweeps: [1] = first sweep launch begins -> last sweep launch done (on the stream that carries them),
    // [2] = what is left of the span expanded -> folded (the exposed part of the last plane's fold)
    float sw = 0, tot = 0;
    HIP_CHECK(hipEventElapsedTime(&sw, W.ev_sw[0], W.ev_sw[1]));
    HIP_CHECK(hipEventElapsedTime(&tot, W.ev[1], W.ev[3]));
    q->ms[1] = sw;
    q->ms[2] = tot > sw ? tot - sw : 0.f;
    W.have_sweep_span = false;
  }
  q->state = 3;
}

int sp_query_finish(sp_query_t* q, uint8_t* out, size_t out_cap, size_t* out_len) {
  // premod: the partial buffer may hold a sum of up to 8 residues (multi-GPU); % q is the identity otherwise
  return guarded([&] { finish_impl(q, true, out, out_cap, out_len); });
}

int sp_query_timings(const sp_query_t* q, float* ms4) {
  if (!q || !ms4 || q->state != 3) {
    g_last_error = "timings are available after sp_query_finish";
    return SP_E_STATE;
  }
  memcpy(ms4, q->ms, sizeof(q->ms));
  return SP_OK;
}
void sp_query_free(sp_query_t* q) { delete q; }

int sp_process_query(const sp_params_t* h, const sp_pp_t* pp, const uint8_t* query, size_t query_len,
                     const sp_db_t* db, uint8_t* out, size_t out_cap, size_t* out_len) {
  if (db && (db->num_shards != 1 || db->col_G != 1)) {
    g_last_error = "sp_process_query needs an unsharded db; use sp_query_begin/sweep/finish for shards";
    return SP_E_ARG;
  }
  sp_query_t* q = sp_query_begin_for_db(h, pp, query, query_len, db);  // (sparse: pruned expansion; wide: split expansion)
  if (!q) return null_handle_rc();
  int rc = sp_query_sweep(q, db);
  if (rc == SP_OK) rc = guarded([&] { finish_impl(q, false, out, out_cap, out_len); });
  sp_query_free(q);
  return rc;
}

int sp_process_query_batch(const sp_params_t* h, const sp_pp_t* const* pps, const uint8_t* const* queries,
                           const size_t* query_lens, int batch, const sp_db_t* db, uint8_t* out, size_t out_stride,
                           size_t* out_len) {
  if (!h || !pps || !queries || !query_lens || batch < 0 || !db || !out || !out_len) {
    g_last_error = "null argument";
    return SP_E_ARG;
  }
  const Params& p = h->p;
  tunables_new_call();  // the switches below are read before the first guarded() section of this call
  // diagnostic (switch batch_trace): host time stamps of this call's phases on stderr, microseconds from entry
  const bool trace = tunable("batch_trace", 0) != 0;
  const auto t_entry = std::chrono::steady_clock::now();
  auto stamp = [&](const char* what) {
    if (trace)
      fprintf(stderr, "[spiral] batch %-22s %8.1f us\n", what,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_entry).count());
  };
  const bool batched = db->packed && db->num_shards == 1 && db->col_G == 1 && !tunable("no_batch_sweep", 0);
  if (!batched) {
    // 8-byte / narrow databases: one pass per query, up to `batch_in_flight` (default 3, at most 4; 1 = one at a time)
    // queries in flight -- query i + 1 is deserialised, expanded and swept on its own workspace and streams before query
    // i is waited for, so that its expansion, a chain of ~30 small dependent launches, runs under its predecessors' sweeps
    // and folds instead of after them.  Lists of 8: C1 994 -> 1422 queries/s, P2 828 -> 1054.
    if (db->num_shards != 1 || db->col_G != 1) {
      g_last_error = "sp_process_query_batch needs an unsharded db";
      return SP_E_ARG;
    }
    size_t depth = (size_t)std::max(1L, std::min(4L, tunable("batch_in_flight", 3)));
    std::deque<std::pair<sp_query_t*, int>> flying;  // oldest first
    int rc = SP_OK;
    auto finish_oldest = [&]() -> int {
      sp_query_t* q = flying.front().first;
      const int qi = flying.front().second;
      flying.pop_front();
      int r = guarded([&] { finish_impl(q, false, out + (size_t)qi * out_stride, out_stride, out_len); });
      sp_query_free(q);
      return r;
    };
    for (int i = 0; i < batch && rc == SP_OK; i++) {
      sp_query_t* q = sp_query_begin_for_db(h, pps[i], queries[i], query_lens[i], db);
      if (!q && g_last_rc == SP_E_OOM && !flying.empty()) {
        // no memory for one more workspace (sweep_out + fold buffers, up to ~2 GiB) beside the database and the queries in
        // flight: finish those -- their workspaces return to the pool -- and go on one query at a time
        while (rc == SP_OK && !flying.empty()) rc = finish_oldest();
        if (rc != SP_OK) break;
        depth = 1;
        q = sp_query_begin_for_db(h, pps[i], queries[i], query_lens[i], db);
      }
      if (!q) {
        rc = null_handle_rc();
        break;
      }
      rc = sp_query_sweep(q, db);
      if (rc != SP_OK) {
        sp_query_free(q);
        break;
      }
      flying.push_back({q, i});
      while (rc == SP_OK && flying.size() >= depth) rc = finish_oldest();   // depth 1: one at a time
    }
    while (rc == SP_OK && !flying.empty()) rc = finish_oldest();
    if (rc != SP_OK) {  // keep the first error; whatever is still in flight is drained and dropped
      const std::string first = g_last_error;
      for (auto& f : flying) {
        (void)hipStreamSynchronize(f.first->ws->stream);
        sp_query_free(f.first);
      }
      g_last_error = first;
    }
    return rc;
  }
  if (out_stride < p.response_bytes()) {
    g_last_error = "out_stride smaller than response_bytes";
    return SP_E_ARG;
  }
  // Groups of up to 8 queries -- 16 where the two-tile matrix-core pass applies (batch_group = 0, the default, asks the
  // kernel side; a positive value caps the group) -- share one database pass.  Nothing waits for a group's folds before the next
  // group's expansions and pass are queued (the passes themselves run one after the other: both are HBM-bound), and at
  // most two groups hold workspaces at a time.  Measured at C2 (profiles/r02_fold_batch_experiments.md): the overlap
  // buys nothing yet -- 16 queries take 2 x the time of 8, and 8 as 2 x 4 are slower (195 vs 236 queries/s) -- because
  // the batched sweep's workgroups fill every CU's register file, so a fold wave only starts when the pass drains.
  {  // the questions below (LDS opt-in limit, free memory) are put to the CURRENT device: it has to be the database's
    const int rc0 = guarded([&] { check_device(db->device); });
    if (rc0 != SP_OK) return rc0;
  }
  stamp("entry");
  const int shape_max = sweep_batch_group_max(db->np_local, db->nj);
  int group_max = (int)tunable("batch_group", 0);
  if (group_max <= 0) group_max = shape_max;
  group_max = std::max(1, std::min(shape_max, group_max));
  if (group_max > SWEEP_BATCH_MAX && batch > SWEEP_BATCH_MAX) {
    // two groups of 16 hold up to 32 workspaces: keep to groups of 8 when the device could not hold them beside the database
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < (size_t)2 * SWEEP_GROUP_MAX * group_ws_bytes(p, db->np_local))
      group_max = SWEEP_BATCH_MAX;
    (void)hipGetLastError();
  }
  stamp("group size decided");
  // a list of exactly 9 .. 16 queries is one group; longer lists are cut into groups of group_max (a last group of <= 8
  // takes the one-tile pass)
  std::vector<sp_query_t*> all_qs;   // queries in flight (at most two groups: bounds the workspaces held)
  size_t drained = 0;                // responses copied out so far
  hipEvent_t prev_pass = nullptr;
  auto drain = [&](size_t count) {   // oldest `count` queries: wait, copy the response out, give the workspace back
    for (size_t i = 0; i < count; i++) {
      Workspace& W = *all_qs[i]->ws;
      HIP_CHECK(hipStreamSynchronize(W.stream));
      memcpy(out + (drained + i) * out_stride, W.h_response, p.response_bytes());
      *out_len = p.response_bytes();
      // (run_finish joins the second stream into the main one before the response copy, and a split-off odd expansion subtree
      // -- not used by grouped expansions -- is joined before the fold: both streams are idle now)
      all_qs[i]->streams_idle = !W.right_pending;
    }
    for (size_t i = 0; i < count; i++) sp_query_free(all_qs[i]);
    all_qs.erase(all_qs.begin(), all_qs.begin() + count);
    drained += count;
  };
  size_t prev_group = 0;
  int start = 0;   // first query not yet answered (a retry after an out-of-memory resumes here)
  bool use_planar = true, one_group = false;   // what the out-of-memory ladder below gives up, in this order
  auto run_groups = [&] {
    check_device(db->device);
    for (int g0 = start; g0 < batch; g0 += group_max) {
      const int B = std::min(group_max, batch - g0);
      if (one_group) {
        if (!all_qs.empty()) drain(all_qs.size());                        // nothing in flight beside this group
      } else if (all_qs.size() > prev_group) {
        drain(all_qs.size() - prev_group);                                // keep only the previous group in flight
      }
      // 1. expand every query of the group on its own stream.  (r05: the sixteen expansions of a group are 8-10 of a step's 49 ms
      // and looked like a launch-rate problem -- 1,600 small launches, 1.5 kernels in flight.  They are not: enqueued by 1, 2, 4 or
      // 8 host threads, on 4, 8 or 16 hardware queues, or recorded and issued as ONE chain of ~100 table launches for the whole
      // group, they take the same time -- 0.5 ms of a query's expansion is transforms that fill the chip (320 k forward NTTs, more
      // than its fold has).  profiles/r05_batch16_step_timeline.md, r05_batch_expand.md; scripts/archive/r05_batch_expand/.)
      // r06: they ARE 2x off the transform rate, and the cure is the shape of the launches, not their number: a round of ONE query
      // under-fills the chip until its last rounds (a right-hand ciphertext's 57 transforms run in sequence in one workgroup), so
      // the group's rounds are shared launches with the query as one more grid dimension (run_begin_group; switch expand_group).
      const size_t first = all_qs.size();
      const bool group_expand = B >= 2 && p.expand_queries && tunable("expand_group", 1) != 0;
      for (int i = 0; i < B; i++) {
        sp_query_t* q = group_expand ? query_open(h, pps[g0 + i]) : sp_query_begin(h, pps[g0 + i], queries[g0 + i], query_lens[g0 + i]);
        if (!q) {
          if (g_last_rc == SP_E_OOM) throw OomError(g_last_error);   // (reported by status: the caller retries in smaller groups)
          throw ArgError(g_last_error);
        }
        all_qs.push_back(q);
        q->ws->ensure_sweep();
      }
      sp_query_t* const* qs = all_qs.data() + first;
      stamp("workspaces acquired");
      if (group_expand) {
        Workspace* Ws[GROUP_MAX];
        for (int i = 0; i < B; i++) Ws[i] = qs[i]->ws.get();
        run_begin_group(Ws, pps + g0, queries + g0, query_lens + g0, B);
        for (int i = 0; i < B; i++) {
          HIP_CHECK(hipEventRecord(Ws[i]->ev[1], Ws[i]->stream));
          qs[i]->state = 1;
        }
      }
      stamp("expansions enqueued");
      // 2. one database pass for the whole group, on the first query's stream, after the previous group's pass; the first query
      // holds the pass's pin of the planar copy
      Workspace& W0 = *qs[0]->ws;
      for (int i = 1; i < B; i++) HIP_CHECK(hipStreamWaitEvent(W0.stream, qs[i]->ws->ev[1], 0));
      if (prev_pass) HIP_CHECK(hipStreamWaitEvent(W0.stream, prev_pass, 0));
      SweepBatchDesc d = group_pass(*db, qs, B, use_planar, qs[0]->planar);
      sweep_batch_prepare(W0.D->T, d, W0.stream);
      // (a per-plane form of the pass with every query folding plane p beside the pass of plane p + 1 was measured in rounds
      // 2 and 3 and is slower: the pass leaves no registers for a fold workgroup; profiles/r02_fold_batch_experiments.md)
      launch_sweep_batch(W0.D->T, d, W0.stream);
      HIP_CHECK(hipEventRecord(W0.ev[2], W0.stream));
      prev_pass = W0.ev[2];
      stamp("pass enqueued");
      // 3. (rest of the) fold / pack per query, concurrently on the queries' own streams
      for (int i = 0; i < B; i++) {
        Workspace& W = *qs[i]->ws;
        if (i > 0) {
          HIP_CHECK(hipStreamWaitEvent(W.stream, W0.ev[2], 0));
          HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
        }
        run_finish(W, *qs[i]->pp, false);
      }
      prev_group = (size_t)B;
      stamp("folds enqueued");
    }
    drain(all_qs.size());
    stamp("drained");
  };
  auto abandon = [&] {  // let whatever was queued drain before the workspaces go back to the pool
    for (auto* q : all_qs) (void)hipStreamSynchronize(q->ws->stream);
    for (auto* q : all_qs) sp_query_free(q);
    all_qs.clear();
    prev_group = 0;
    prev_pass = nullptr;
  };
  int rc = guarded(run_groups);
  // Out of memory (the hipMemGetInfo estimates above are rough): give up, one after the other, what only makes the call faster, and
  // answer the REST of the list each time -- responses already copied out stay.  (1) the digit-planar copy of the database (its
  // memory is released; a later call may build it again when there is room); (2) groups of 16 and the second group in flight:
  // groups of 8, one at a time -- the in-flight queries' workspaces went back to the pool, so a group of 8 needs no more than was
  // already allocated unless the failure came before 8 workspaces existed; (3) one query at a time, one workspace.
  for (int step = 1; rc == SP_E_OOM && step <= 3; step++) {
    abandon();
    (void)hipGetLastError();
    start = (int)drained;
    if (step == 1) {   // (abandon has released the pins of the groups in flight: dropping the handle's copy frees it)
      sp_db* wdb = const_cast<sp_db_t*>(db);
      std::lock_guard<std::mutex> lk(wdb->mu);
      use_planar = false;
      if (!wdb->planar) continue;   // nothing to give back here: next step
      wdb->drop_planar();
      wdb->planar_state = -2;
    } else if (step == 2) {
      if (group_max <= SWEEP_BATCH_MAX && one_group) continue;
      group_max = std::min(group_max, SWEEP_BATCH_MAX);
      one_group = true;
    } else {
      rc = SP_OK;
      for (int i = start; i < batch && rc == SP_OK; i++, drained++)
        rc = sp_process_query(h, pps[i], queries[i], query_lens[i], db, out + (size_t)i * out_stride, out_stride, out_len);
      break;
    }
    rc = guarded(run_groups);
  }
  if (rc != SP_OK) {
    const std::string first_error = g_last_error;
    abandon();
    g_last_error = first_error;
  }
  for (auto* q : all_qs) sp_query_free(q);
  return rc;
}

int sp_bench_sweep(sp_query_t* q, const sp_db_t* db, int iters, float* ms_per_launch) {
  return sp_bench_sweep_ex(q, db, iters, -1, ms_per_launch);
}

int sp_bench_sweep_ex(sp_query_t* q, const sp_db_t* db, int iters, int per_plane_launches, float* ms_per_launch) {
  return guarded([&] {
    need(q && db && ms_per_launch && iters > 0, "bad argument");
    need(q->state >= 1, "query not begun");
    check_device(db->device);
    Workspace& W = *q->ws;
    TimingEvents ev;
    // the same launches process_query issues for this database (one per plane when the sweep is pipelined)
    const Params& p = q->params->p;
    const bool per_plane = per_plane_launches < 0 ? sweep_is_pipelined(p, *db) : per_plane_launches != 0;
    need(!per_plane || db->col_G == 1, "per-plane launches need a row-sharded or unsharded db");
    auto sweep_once = [&] {
      if (!per_plane) return run_sweep(W, *db);
      W.ensure_sweep();
      for (size_t pl = 0; pl < p.planes(); pl++) launch_plane_sweep(W, *db, pl);
    };
    sweep_once();  // warm
    HIP_CHECK(hipEventRecord(ev.a, W.stream));
    for (int i = 0; i < iters; i++) sweep_once();
    HIP_CHECK(hipEventRecord(ev.b, W.stream));
    HIP_CHECK(hipStreamSynchronize(W.stream));
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
    *ms_per_launch = t / ((float)iters * (per_plane ? (float)p.planes() : 1.0f));
  });
}

int sp_bench_sweep_batch(sp_query_t* const* qs, int batch, const sp_db_t* db, int iters, float* ms_per_pass) {
  return guarded([&] {
    need(qs && db && ms_per_pass && iters > 0 && batch >= 1 && batch <= sweep_batch_group_max(db ? db->np_local : 0, db ? db->nj : 0), "bad argument");
    need(db->packed && db->num_shards == 1 && db->col_G == 1, "the batched pass needs an unsharded PACKED database");
    check_device(db->device);
    for (int i = 0; i < batch; i++) {
      need(qs[i] && qs[i]->state >= 1, "query not begun");
      need(qs[i]->params == db->params, "query and db were created for different params");
    }
    Workspace& W0 = *qs[0]->ws;
    for (int i = 0; i < batch; i++) {
      qs[i]->ws->ensure_sweep();
      HIP_CHECK(hipStreamSynchronize(qs[i]->ws->stream));   // expansions done: the pass is timed alone
      HIP_CHECK(hipStreamSynchronize(qs[i]->ws->stream2));
    }
    PlanarPin pin;   // held for the whole call: on every path out the pass's stream is synchronised before it is released
    SweepBatchDesc d = group_pass(*db, qs, batch, true, pin);
    struct Drain {
      hipStream_t s;
      ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{W0.stream};
    TimingEvents ev;   // destroyed on every path out of here (launches and HIP_CHECK throw)
    auto pass = [&] {
      sweep_batch_prepare(W0.D->T, d, W0.stream);
      launch_sweep_batch(W0.D->T, d, W0.stream);
    };
    pass();  // warm
    HIP_CHECK(hipEventRecord(ev.a, W0.stream));
    for (int i = 0; i < iters; i++) pass();
    HIP_CHECK(hipEventRecord(ev.b, W0.stream));
    HIP_CHECK(hipStreamSynchronize(W0.stream));
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
    *ms_per_pass = t / (float)iters;
  });
}

int sp_bench_sweep_scatter_group(sp_query_t* const* qs, int batch, const sp_db_t* db, int G, int layout, int iters, float* ms_per_pass) {
  return guarded([&] {
    need(ms_per_pass && iters > 0 && (layout == 0 || layout == 1), "bad argument");
    scatter_group_check(qs, batch, db, G);
    for (int i = 0; i < batch; i++) {
      need(qs[i]->state >= 1, "query not begun");
      HIP_CHECK(hipStreamSynchronize(qs[i]->ws->stream));   // expansions done: the pass is timed alone
      HIP_CHECK(hipStreamSynchronize(qs[i]->ws->stream2));
    }
    SweepBatchDesc d{};
    need(scatter_group_desc(qs, batch, db, G, d), "this group / shard does not take the scatter-form pass (sp_query_sweep_scatter_group would sweep per query)");
    Workspace& W0 = *qs[0]->ws;
    struct Drain {
      hipStream_t s;
      ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{W0.stream};
    TimingEvents ev;
    auto pass = [&] {
      sweep_batch_prepare(W0.D->T, d, W0.stream);
      if (layout == 1)
        launch_sweep_batch_scatter(W0.D->T, d, G, W0.stream);
      else
        launch_sweep_batch(W0.D->T, d, W0.stream);   // the same rows, plain [z][ii] output: the scatter form's lower bound
    };
    pass();  // warm
    HIP_CHECK(hipEventRecord(ev.a, W0.stream));
    for (int i = 0; i < iters; i++) pass();
    HIP_CHECK(hipEventRecord(ev.b, W0.stream));
    HIP_CHECK(hipStreamSynchronize(W0.stream));
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
    *ms_per_pass = t / (float)iters;
  });
}

int sp_sweep_launches(const sp_params_t* h, const sp_db_t* db) {
  if (!h || !db) return 0;
  return sweep_is_pipelined(h->p, *db) ? (int)h->p.planes() : 1;
}

// Placement probe: launches `blocks` small workgroups on a stream whose CU mask has bits [bit_lo, bit_hi) set (the
// whole device when bit_hi <= bit_lo) and reports the XCC / HW_ID registers each one saw.
int sp_debug_cu_probe(int bit_lo, int bit_hi, int blocks, uint32_t* out2) {
  return guarded([&] {
    need(out2 && blocks > 0 && blocks <= 65536, "bad argument");
    hipStream_t s = nullptr;
    if (bit_hi > bit_lo) {
      hipDeviceProp_t prop;
      int dev = 0;
      HIP_CHECK(hipGetDevice(&dev));
      HIP_CHECK(hipGetDeviceProperties(&prop, dev));
      std::vector<uint32_t> m((prop.multiProcessorCount + 31) / 32, 0u);
      for (int k = bit_lo; k < bit_hi && k < prop.multiProcessorCount; k++) m[k / 32] |= 1u << (k % 32);
      HIP_CHECK(hipExtStreamCreateWithCUMask(&s, (uint32_t)m.size(), m.data()));
    } else {
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    DevBuf<u32> d((size_t)blocks * 2);
    launch_cu_probe(d.p, blocks, s);
    HIP_CHECK(hipMemcpyAsync(out2, d.p, (size_t)blocks * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    (void)hipStreamDestroy(s);
  });
}

// Resident-data check (diagnostic): for each of tw, neg1, gadget_gsw, lists, pp.all, pp.pack_cat -> 4 values:
// checksum as a kernel on a fresh non-blocking stream sees it, checksum of a device-to-host copy, the kernel view again
// after k_cache_sync (L2 write-back + invalidate on every XCD), and the checksum of the host original where the
// library still has it (tw; 0 otherwise).  A kernel view that differs from the copy view is a stale cache line.
int sp_debug_chacha20_u64(const uint8_t seed[32], uint64_t* out, size_t count) {
  if (!seed || (!out && count)) {
    g_last_error = "null argument";
    return SP_E_ARG;
  }
  chacha20_keystream_u64(seed, out, count);
  return SP_OK;
}

int sp_debug_resident_check(const sp_params_t* h, const sp_pp_t* pp, uint64_t* out, int cap) {
  return guarded([&] {
    need(h && pp && out && cap >= 24, "bad argument");
    DeviceState& D = const_cast<sp_params*>(h)->device_state();
    struct Item { const u32* p; size_t n; const u32* host; };
    const Item items[6] = {{D.tw.p, D.tw.n, h->p.ntt_tables.data()}, {D.neg1.p, D.neg1.n, nullptr},
                           {D.gadget_gsw.p, D.gadget_gsw.n, nullptr}, {(const u32*)D.lists.p, D.lists.n, nullptr},
                           {pp->all.p, pp->all.n, nullptr}, {pp->pack_cat.p, pp->pack_cat.n, nullptr}};
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevBuf<unsigned long long> acc(12);
    DevBuf<u32> sink(1);
    auto host_sum = [](const u32* p, size_t n) {
      unsigned long long a = 0;
      for (size_t i = 0; i < n; i++) a += (unsigned long long)p[i] * (unsigned long long)((i << 1) | 1);
      return a;
    };
    HIP_CHECK(hipMemsetAsync(acc.p, 0, 12 * 8, s));
    for (int i = 0; i < 6; i++) launch_checksum(items[i].p, items[i].n, acc.p + i, s);
    launch_cache_sync(sink.p, s);
    for (int i = 0; i < 6; i++) launch_checksum(items[i].p, items[i].n, acc.p + 6 + i, s);
    unsigned long long k[12];
    HIP_CHECK(hipMemcpyAsync(k, acc.p, sizeof(k), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < 6; i++) {
      std::vector<u32> hostcopy(items[i].n);
      if (items[i].n) HIP_CHECK(hipMemcpy(hostcopy.data(), items[i].p, items[i].n * 4, hipMemcpyDeviceToHost));
      out[4 * i + 0] = k[i];
      out[4 * i + 1] = host_sum(hostcopy.data(), items[i].n);
      out[4 * i + 2] = k[6 + i];
      out[4 * i + 3] = items[i].host ? host_sum(items[i].host, items[i].n) : 0;
    }
    (void)hipStreamDestroy(s);
  });
}

// transform-core micro-benchmark (profiling aid): ns per 2048-point forward NTT with M vectors per thread
int sp_bench_ntt(const sp_params_t* h, int M, int blocks, int reps, float* ns_per_ntt) {
  return guarded([&] {
    need(h && ns_per_ntt && blocks > 0 && reps > 0, "bad argument");
    Scoped W(h);
    DevBuf<u32> scratch((size_t)blocks * 256);
    const float ms = bench_ntt_core(W->D->T, M, blocks, reps, scratch.p, W->stream);
    *ns_per_ntt = ms * 1e6f / ((float)blocks * reps * (M == 1 || M == 2 ? M : 4));
  });
}

// ------------------------------------------------------------------------------- stage level
int sp_to_ntt(const sp_params_t* h, const uint64_t* raw, uint64_t* out, size_t count) {
  return guarded([&] {
    need(h && raw && out, "null argument");
    if (count == 0) return;
    Scoped W(h);
    DevBuf<u64> d_raw, tmp;
    DevBuf<u32> d_ntt(count * 2 * POLY_LEN);
    upload_raw(*W, raw, count * POLY_LEN, d_raw);
    FwdDesc f{d_raw.p, nullptr, d_ntt.p, (int)count, 1, 1, 1, 64, 1, 0, 1};
    launch_ntt_fwd(W->D->T, f, W->stream);
    download_ntt(*W, d_ntt.p, count * 2 * POLY_LEN, out, tmp);
  });
}

int sp_from_ntt(const sp_params_t* h, const uint64_t* ntt, uint64_t* out, size_t count) {
  return guarded([&] {
    need(h && ntt && out, "null argument");
    if (count == 0) return;
    Scoped W(h);
    DevBuf<u64> tmp, d_raw(count * POLY_LEN);
    DevBuf<u32> d_ntt;
    upload_ntt(*W, ntt, count * 2 * POLY_LEN, d_ntt, tmp);
    InvDesc inv{};
    inv.src = d_ntt.p;
    inv.poly_stride = 2 * POLY_LEN;
    inv.crt_stride = POLY_LEN;
    inv.z_stride = 1;
    inv.dst = d_raw.p;
    inv.n_polys = (int)count;
    launch_ntt_inv(W->D->T, inv, W->stream);
    download_raw(*W, d_raw.p, count * POLY_LEN, out);
  });
}

int sp_ntt_forward(const sp_params_t* h, uint64_t* data, size_t count) {
  return guarded([&] {
    need(h && data, "null argument");
    if (count == 0) return;
    // each [crt] half is transformed under its own modulus: run the (value mod q_c -> NTT) kernel on
    // every half and keep the matching modulus
    std::vector<u64> full(count * 2 * 2 * POLY_LEN);
    int rc = sp_to_ntt(h, data, full.data(), count * 2);
    if (rc != SP_OK) throw HipError(g_last_error);
    for (size_t i = 0; i < count; i++)
      for (size_t c = 0; c < 2; c++)
        memcpy(data + (i * 2 + c) * POLY_LEN, full.data() + ((i * 2 + c) * 2 + c) * POLY_LEN, POLY_LEN * 8);
  });
}

int sp_ntt_inverse(const sp_params_t* h, uint64_t* data, size_t count) {
  return guarded([&] {
    need(h && data, "null argument");
    if (count == 0) return;
    // inverse both residues on the device; the per-modulus outputs are the residues of the composed value
    std::vector<u64> raw(count * POLY_LEN);
    int rc = sp_from_ntt(h, data, raw.data(), count);
    if (rc != SP_OK) throw HipError(g_last_error);
    for (size_t i = 0; i < count; i++)
      for (size_t z = 0; z < POLY_LEN; z++) {
        data[(i * 2 + 0) * POLY_LEN + z] = raw[i * POLY_LEN + z] % h->p.moduli[0];
        data[(i * 2 + 1) * POLY_LEN + z] = raw[i * POLY_LEN + z] % h->p.moduli[1];
      }
  });
}

int sp_multiply(const sp_params_t* h, const uint64_t* a, size_t ar, size_t ac, const uint64_t* b, size_t bc,
                uint64_t* res) {
  return guarded([&] {
    need(h && a && b && res && ar && ac && bc, "bad argument");
    Scoped W(h);
    DevBuf<u64> tmp;
    DevBuf<u32> dA, dBt, dR(ar * bc * 2 * POLY_LEN);
    upload_ntt(*W, a, ar * ac * 2 * POLY_LEN, dA, tmp);
    // B is ac x bc; the MAC kernel wants the K operands of one output column contiguous: transpose on host
    std::vector<u64> bt(ac * bc * 2 * POLY_LEN);
    for (size_t k = 0; k < ac; k++)
      for (size_t j = 0; j < bc; j++)
        memcpy(bt.data() + (j * ac + k) * 2 * POLY_LEN, b + (k * bc + j) * 2 * POLY_LEN, 2 * POLY_LEN * 8);
    DevBuf<u64> tmp2;
    upload_ntt(*W, bt.data(), bt.size(), dBt, tmp2);
    MacDesc m{};
    m.A = dA.p;
    m.B = dBt.p;
    m.out = dR.p;
    m.R = (int)ar;
    m.K = (int)ac;
    m.batch_inner = (int)bc;
    m.batch_outer = 1;
    m.B_inner_stride = (long)ac;
    m.split_k = (int)ac;
    m.out_batch_stride = 1;
    m.out_row_stride = (int)bc;
    launch_mac(W->D->T, m, W->stream);
    download_ntt(*W, dR.p, ar * bc * 2 * POLY_LEN, res, tmp);
  });
}

int sp_add(const sp_params_t* h, const uint64_t* a, const uint64_t* b, size_t count, uint64_t* res) {
  return guarded([&] {
    need(h && a && b && res && count, "bad argument");
    Scoped W(h);
    DevBuf<u64> tmp, tmp2;
    DevBuf<u32> dA, dB, dR(count * 2 * POLY_LEN);
    upload_ntt(*W, a, count * 2 * POLY_LEN, dA, tmp);
    upload_ntt(*W, b, count * 2 * POLY_LEN, dB, tmp2);
    launch_add(W->D->T, dR.p, dA.p, dB.p, (int)count, W->stream);
    download_ntt(*W, dR.p, count * 2 * POLY_LEN, res, tmp);
  });
}
int sp_add_into(const sp_params_t* h, uint64_t* res, const uint64_t* a, size_t count) {
  return guarded([&] {
    need(h && a && res && count, "bad argument");
    Scoped W(h);
    DevBuf<u64> tmp, tmp2;
    DevBuf<u32> dA, dR;
    upload_ntt(*W, res, count * 2 * POLY_LEN, dR, tmp);
    upload_ntt(*W, a, count * 2 * POLY_LEN, dA, tmp2);
    launch_add(W->D->T, dR.p, dR.p, dA.p, (int)count, W->stream);   // in place, as add_into (poly.rs:500-512)
    download_ntt(*W, dR.p, count * 2 * POLY_LEN, res, tmp);
  });
}
int sp_scalar_multiply(const sp_params_t* h, const uint64_t* scalar, const uint64_t* b, size_t count, uint64_t* res) {
  return guarded([&] {
    need(h && scalar && b && res && count, "bad argument");
    Scoped W(h);
    DevBuf<u64> tmp, tmp2;
    DevBuf<u32> dS, dB(2 * count * 2 * POLY_LEN), dIn;
    upload_ntt(*W, scalar, 2 * POLY_LEN, dS, tmp);
    upload_ntt(*W, b, count * 2 * POLY_LEN, dIn, tmp2);
    // the kernel the expansion uses (coefficient_expansion, server.rs:105-110): polys [count, 2 count) = scalar * polys [0, count)
    launch_copy_words(dB.p, dIn.p, count * 2 * POLY_LEN, W->stream);
    launch_scalar_mul(W->D->T, dB.p, (long)count, 0, dS.p, (int)count, W->stream);
    download_ntt(*W, dB.p + count * 2 * POLY_LEN, count * 2 * POLY_LEN, res, tmp);
  });
}

int sp_automorph(const sp_params_t* h, const uint64_t* a, size_t count, size_t t, uint64_t* res) {
  return guarded([&] {
    need(h && a && res && (t & 1), "bad argument (t must be odd)");
    if (count == 0) return;
    Scoped W(h);
    DevBuf<u64> dA, dR(count * POLY_LEN);
    upload_raw(*W, a, count * POLY_LEN, dA);
    launch_automorph(W->D->T, dR.p, dA.p, (int)count, (int)t, W->stream);
    download_raw(*W, dR.p, count * POLY_LEN, res);
  });
}

int sp_gadget_invert_rdim(const sp_params_t* h, const uint64_t* inp, size_t rows_in, size_t cols, uint64_t* out,
                          size_t rows_out, size_t rdim) {
  return guarded([&] {
    need(h && inp && out && rdim && rows_out % rdim == 0 && rdim <= rows_in, "bad argument");
    Scoped W(h);
    DevBuf<u64> dI, dO(rows_out * cols * POLY_LEN);
    upload_raw(*W, inp, rows_in * cols * POLY_LEN, dI);
    launch_gadget_raw(dO.p, dI.p, (int)rows_in, (int)cols, (int)rows_out, (int)rdim, (int)h->p.bits_per(rows_out / rdim), W->stream);
    download_raw(*W, dO.p, rows_out * cols * POLY_LEN, out);
  });
}

int sp_reorient_reg_ciphertexts(const sp_params_t* h, const uint64_t* v_reg, uint64_t* out) {
  return guarded([&] {
    need(h && v_reg && out, "null argument");
    const Params& p = h->p;
    Scoped W(h);
    DevBuf<u64> tmp, dO(POLY_LEN * p.dim0() * 2);
    DevBuf<u32> dV;
    upload_ntt(*W, v_reg, p.dim0() * 2 * 2 * POLY_LEN, dV, tmp);
    launch_reorient(dO.p, dV.p, 0, 1, (int)p.dim0(), W->stream);
    download_raw(*W, dO.p, POLY_LEN * p.dim0() * 2, out);
  });
}

int sp_multiply_reg_by_database(const sp_params_t* h, const uint64_t* db, const uint64_t* v_firstdim, size_t dim0,
                                size_t num_per, uint64_t* out) {
  return guarded([&] {
    need(h && db && v_firstdim && out, "null argument");
    need(dim0 >= 1 && num_per >= 1 && (num_per & (num_per - 1)) == 0 && num_per <= 65536 && dim0 <= 65536, "bad dimensions");
    Scoped W(h);
    const size_t words = POLY_LEN * num_per * dim0;
    DevBuf<u64> d_ref(words), d_dev(words), d_q, d_out(num_per * 4 * POLY_LEN);
    DevBuf<u32> d_res(4 * POLY_LEN * num_per);
    HIP_CHECK(hipMemcpyAsync(d_ref.p, db, words * 8, hipMemcpyHostToDevice, W->stream));
    const int packed = db_can_pack((int)num_per, (int)dim0) && !tunable("db_unpacked", 0) ? 1 : 0;
    launch_db_relayout(d_dev.p, 0, d_ref.p, 0, N, (int)num_per, (int)dim0, 0, (int)dim0, packed, ColMap{}, W->stream);
    upload_raw(*W, v_firstdim, POLY_LEN * dim0 * 2, d_q);
    // the reference sums limb products in u128 and is exact for any limbs (server.rs:186-217); the sweep kernels sum up to 256
    // products in u64 and need limbs < q: reduced here, as the loaders reduce the database words (same residues)
    launch_canon_words(d_q.p, POLY_LEN * dim0 * 2, W->stream);
    SweepDesc d{d_dev.p, d_q.p, d_res.p, 1, (int)num_per, (int)dim0, 0, (int)dim0, packed, 1};
    launch_sweep(W->D->T, d, W->stream);
    launch_sweep_out_to_ref(d_out.p, d_res.p, (int)num_per, W->stream);
    download_raw(*W, d_out.p, num_per * 4 * POLY_LEN, out);
  });
}

int sp_coefficient_expansion(const sp_params_t* h, const sp_pp_t* pp, uint64_t* v, size_t g, size_t stop_round,
                             size_t max_bits_to_gen_right) {
  return guarded([&] {
    need(h && pp && v, "null argument");
    const Params& p = h->p;
    need(p.expand_queries, "params have no query expansion");
    // the schedule (pruning) is derived from params exactly as expand_query derives it (server.rs:536-564)
    const size_t sr = p.db_dim_2 > 0 ? p.stop_round() : 0, mb = p.db_dim_2 > 0 ? p.t_gsw * p.db_dim_2 : 0;
    need(g == p.g() && stop_round == sr && max_bits_to_gen_right == mb, "g / stop_round / max_bits_to_gen_right must match params");
    check_device(pp->device);
    Scoped W(h);
    W->ensure_expand();
    const size_t words = ((size_t)1 << g) * 2 * 2 * POLY_LEN;
    DevBuf<u64> tmp;
    tmp.ensure(words);
    HIP_CHECK(hipMemcpyAsync(tmp.p, v, words * 8, hipMemcpyHostToDevice, W->stream));
    launch_u64_to_u32(W->v.p, tmp.p, (long)words, W->stream);
    run_coefficient_expansion(*W, *pp, g);
    download_ntt(*W, W->v.p, words, v, tmp);
  });
}

int sp_regev_to_gsw(const sp_params_t* h, const sp_pp_t* pp, const uint64_t* v_inp, uint64_t* v_gsw, size_t num_gsw) {
  return guarded([&] {
    need(h && pp && v_inp && v_gsw, "null argument");
    const Params& p = h->p;
    need(num_gsw == p.db_dim_2 && num_gsw > 0, "num_gsw must equal nu_2");
    check_device(pp->device);
    Scoped W(h);
    W->ensure_expand();
    const size_t nb = num_gsw * p.t_gsw;
    DevBuf<u64> tmp;
    DevBuf<u32> dV;
    upload_ntt(*W, v_inp, nb * 2 * 2 * POLY_LEN, dV, tmp);
    std::vector<int> ct(nb), poly(nb);
    for (size_t b = 0; b < nb; b++) {
      ct[b] = (int)b;
      poly[b] = (int)(2 * b);
    }
    DevBuf<int> dl(2 * nb);
    HIP_CHECK(hipMemcpyAsync(dl.p, ct.data(), nb * sizeof(int), hipMemcpyHostToDevice, W->stream));
    HIP_CHECK(hipMemcpyAsync(dl.p + nb, poly.data(), nb * sizeof(int), hipMemcpyHostToDevice, W->stream));
    run_regev_to_gsw(*W, *pp, dV.p, dl.p, dl.p + nb);
    // gather the right halves (2 x 2t_gsw per GSW ct)
    const size_t two_t = 2 * p.t_gsw;
    DevBuf<u32> dense(num_gsw * 2 * two_t * 2 * POLY_LEN);
    for (size_t d = 0; d < num_gsw; d++)
      for (size_t r = 0; r < 2; r++)
        HIP_CHECK(hipMemcpyAsync(dense.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN,
                                 W->fold_mats.p + ((d * 2 + r) * 2 * two_t + two_t) * 2 * POLY_LEN,
                                 two_t * 2 * POLY_LEN * sizeof(u32), hipMemcpyDeviceToDevice, W->stream));
    download_ntt(*W, dense.p, num_gsw * 2 * two_t * 2 * POLY_LEN, v_gsw, tmp);
  });
}

int sp_get_v_folding_neg(const sp_params_t* h, const uint64_t* v_folding, uint64_t* out) {
  return guarded([&] {
    need(h && v_folding && out, "null argument");
    const Params& p = h->p;
    const size_t nu2 = p.db_dim_2, two_t = 2 * p.t_gsw;
    if (nu2 == 0) return;
    Scoped W(h);
    W->ensure_expand();
    DevBuf<u64> tmp;
    DevBuf<u32> dense;
    upload_ntt(*W, v_folding, nu2 * 2 * two_t * 2 * POLY_LEN, dense, tmp);
    for (size_t d = 0; d < nu2; d++)
      for (size_t r = 0; r < 2; r++)
        HIP_CHECK(hipMemcpyAsync(W->fold_mats.p + ((d * 2 + r) * 2 * two_t + two_t) * 2 * POLY_LEN,
                                 dense.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN, two_t * 2 * POLY_LEN * sizeof(u32),
                                 hipMemcpyDeviceToDevice, W->stream));
    run_folding_neg(*W);
    for (size_t d = 0; d < nu2; d++)
      for (size_t r = 0; r < 2; r++)
        HIP_CHECK(hipMemcpyAsync(dense.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN,
                                 W->fold_mats.p + ((d * 2 + r) * 2 * two_t) * 2 * POLY_LEN,
                                 two_t * 2 * POLY_LEN * sizeof(u32), hipMemcpyDeviceToDevice, W->stream));
    download_ntt(*W, dense.p, nu2 * 2 * two_t * 2 * POLY_LEN, out, tmp);
  });
}

int sp_expand_query(const sp_params_t* h, const sp_pp_t* pp, const uint8_t* query, size_t query_len,
                    uint64_t* v_reg_reoriented, uint64_t* v_folding) {
  return guarded([&] {
    need(h && pp && query && v_reg_reoriented, "null argument");
    const Params& p = h->p;
    check_device(pp->device);
    Scoped W(h);
    run_begin(*W, *pp, query, query_len);
    join_right(*W);  // the GSW side is produced on the second stream
    download_raw(*W, W->qv.p, POLY_LEN * p.dim0() * 2, v_reg_reoriented);
    const size_t nu2 = p.db_dim_2, two_t = 2 * p.t_gsw;
    if (nu2 > 0) {
      need(v_folding != nullptr, "v_folding is null");
      DevBuf<u32> dense(nu2 * 2 * two_t * 2 * POLY_LEN);
      for (size_t d = 0; d < nu2; d++)
        for (size_t r = 0; r < 2; r++)
          HIP_CHECK(hipMemcpyAsync(dense.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN,
                                   W->fold_mats.p + ((d * 2 + r) * 2 * two_t + two_t) * 2 * POLY_LEN,
                                   two_t * 2 * POLY_LEN * sizeof(u32), hipMemcpyDeviceToDevice, W->stream));
      DevBuf<u64> tmp;
      download_ntt(*W, dense.p, nu2 * 2 * two_t * 2 * POLY_LEN, v_folding, tmp);
    }
  });
}

int sp_fold_ciphertexts(const sp_params_t* h, uint64_t* cts, size_t num_per, const uint64_t* v_folding,
                        const uint64_t* v_folding_neg) {
  return guarded([&] {
    need(h && cts && v_folding && v_folding_neg, "null argument");
    const Params& p = h->p;
    need(num_per >= 1 && (num_per & (num_per - 1)) == 0, "num_per must be a power of two");
    size_t further = 0;
    while (((size_t)1 << further) < num_per) further++;
    if (further == 0) return;
    const size_t two_t = 2 * p.t_gsw;
    Scoped W(h);
    ensure_stage_fold(*W, num_per, further);
    DevBuf<u64> tmp;
    DevBuf<u32> dF, dFn;
    upload_ntt(*W, v_folding, further * 2 * two_t * 2 * POLY_LEN, dF, tmp);
    DevBuf<u64> tmp2;
    upload_ntt(*W, v_folding_neg, further * 2 * two_t * 2 * POLY_LEN, dFn, tmp2);
    for (size_t d = 0; d < further; d++)
      for (size_t r = 0; r < 2; r++) {
        u32* row = W->fold_mats.p + ((d * 2 + r) * 2 * two_t) * 2 * POLY_LEN;
        HIP_CHECK(hipMemcpyAsync(row, dFn.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN, two_t * 2 * POLY_LEN * sizeof(u32), hipMemcpyDeviceToDevice, W->stream));
        HIP_CHECK(hipMemcpyAsync(row + two_t * 2 * POLY_LEN, dF.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN, two_t * 2 * POLY_LEN * sizeof(u32), hipMemcpyDeviceToDevice, W->stream));
      }
    HIP_CHECK(hipMemcpyAsync(W->foldX.p, cts, num_per * 2 * POLY_LEN * 8, hipMemcpyHostToDevice, W->stream));
    W->mats_w_ready = false;   // (whatever wave-layout operands the pooled workspace holds are not this call's)
    // the stage export honours the caller's v_folding_neg: literal path, every digit
    u64* res = run_fold(*W, FoldOpts{1L << 60, false, false}, W->foldX.p, W->foldY.p, 1, (int)num_per, -1);
    download_raw(*W, res, 2 * POLY_LEN, cts);
  });
}

int sp_fold_ciphertexts_fused(const sp_params_t* h, uint64_t* cts, size_t num_per, const uint64_t* v_folding,
                              long fused_min_pairs) {
  return guarded([&] {
    need(h && cts && v_folding, "null argument");
    const Params& p = h->p;
    need(num_per >= 1 && (num_per & (num_per - 1)) == 0, "num_per must be a power of two");
    size_t further = 0;
    while (((size_t)1 << further) < num_per) further++;
    if (further == 0) return;
    const size_t two_t = 2 * p.t_gsw;
    Scoped W(h);
    ensure_stage_fold(*W, num_per, further);
    DevBuf<u64> tmp;
    DevBuf<u32> dF;
    upload_ntt(*W, v_folding, further * 2 * two_t * 2 * POLY_LEN, dF, tmp);
    for (size_t d = 0; d < further; d++)
      for (size_t r = 0; r < 2; r++) {
        u32* row = W->fold_mats.p + ((d * 2 + r) * 2 * two_t) * 2 * POLY_LEN;
        HIP_CHECK(hipMemcpyAsync(row + two_t * 2 * POLY_LEN, dF.p + ((d * 2 + r) * two_t) * 2 * POLY_LEN, two_t * 2 * POLY_LEN * sizeof(u32), hipMemcpyDeviceToDevice, W->stream));
      }
    launch_folding_neg(W->D->T, W->fold_mats.p, W->D->gadget_gsw.p, (int)further, (int)two_t, W->stream);
    run_mats_to_wave(*W, further);
    HIP_CHECK(hipMemcpyAsync(W->foldX.p, cts, num_per * 2 * POLY_LEN * 8, hipMemcpyHostToDevice, W->stream));
    // the caller's ciphertexts: below Q (what the reference's invariants give, and what lets the kernels skip the dead top
    // digit) only if every coefficient says so -- checked here, on the host copy
    bool below_q = true;
    for (size_t i = 0; i < num_per * 2 * POLY_LEN && below_q; i++) below_q = cts[i] < p.modulus;
    const FoldOpts o{fused_min_pairs > 0 ? fused_min_pairs : W->fused_min_pairs, true, below_q};
    u64* res = run_fold(*W, o, W->foldX.p, W->foldY.p, 1, (int)num_per, -1);
    download_raw(*W, res, 2 * POLY_LEN, cts);
  });
}

int sp_pack(const sp_params_t* h, const sp_pp_t* pp, const uint64_t* v_ct, uint64_t* out) {
  return guarded([&] {
    need(h && pp && v_ct && out, "null argument");
    const Params& p = h->p;
    need(p.instances == 1, "sp_pack packs one instance (n*n cts); call per instance");
    check_device(pp->device);
    Scoped W(h);
    W->ensure_finish();
    HIP_CHECK(hipMemcpyAsync(W->final_cts.p, v_ct, p.n * p.n * 2 * POLY_LEN * 8, hipMemcpyHostToDevice, W->stream));
    run_pack(*W, *pp);
    DevBuf<u64> tmp;
    download_ntt(*W, W->pack_res.p, (p.n + 1) * p.n * 2 * POLY_LEN, out, tmp);
  });
}

int sp_encode(const sp_params_t* h, const uint64_t* v_packed, uint8_t* out, size_t out_cap, size_t* out_len) {
  return guarded([&] {
    need(h && v_packed && out && out_len, "null argument");
    need(out_cap >= h->p.response_bytes(), "output buffer smaller than response_bytes");
    *out_len = encode_response(h->p, v_packed, out);
  });
}

}  // extern "C"
