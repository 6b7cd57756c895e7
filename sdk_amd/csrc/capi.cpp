// extern "C" surface of libspiral_hip.so (include/spiral_hip.h): the error boundary, params, databases, public parameters, the query
// stage machine and sp_process_query.  The list flows are in capi_batch.cpp, the stage-level exports in capi_stage.cpp.
#include <cstdlib>
#include <new>

#include "capi_internal.hpp"

using namespace spiral;

static thread_local std::string g_last_error;
static thread_local int g_last_rc = SP_OK;  // status of this thread's last guarded() section: what a constructor-style entry
                                             // point (returns a handle or null) failed with
static thread_local int g_shard_split_hint = 1;   // 0 while a list of sharded queries is being enqueued
int spiral::guarded_status(int rc, const char* what) {
  if (rc != SP_OK) g_last_error = what;
  g_last_rc = rc;
  return rc;
}
int spiral::null_handle_rc() { return g_last_rc != SP_OK ? g_last_rc : SP_E_ARG; }

void spiral::check_device(int dev) {
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  if (cur != dev) throw ArgError("handle belongs to HIP device " + std::to_string(dev) + " but the current device is " + std::to_string(cur));
}

void spiral::download_ntt(Workspace& W, const u32* src, size_t words, uint64_t* host, DevBuf<u64>& tmp) {
  tmp.ensure(words);
  launch_u32_to_u64(tmp.p, src, (long)words, W.stream);
  HIP_CHECK(hipMemcpyAsync(host, tmp.p, words * 8, hipMemcpyDeviceToHost, W.stream));
  HIP_CHECK(hipStreamSynchronize(W.stream));
}

// three times the first-dimension output (a rough bound; pooled workspaces only make it conservative)
size_t spiral::group_ws_bytes(const Params& p, int np_local) { return (size_t)3 * p.planes() * 4 * POLY_LEN * (size_t)np_local * sizeof(u32); }

namespace {

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


// does this sparse bucket (or row shard of one, sp_db_create_sparse_shard) store item `idx`?  Its row j = idx / num_per is the shard's
bool sparse_holds(const sp_db& d, size_t idx) {
  const size_t j = idx / d.params->p.num_per();
  return j >= (size_t)d.j0 && j < (size_t)d.j0 + (size_t)d.nj;
}

// room for `slots` polynomial sets in a sparse bucket's store: amortised doubling from 64, contents preserved (caller holds mu)
void sparse_reserve(sp_db& d, size_t slots) {
  size_t cap = d.slots_cap;
  while (cap < slots) cap = std::max<size_t>(64, cap * 2);
  if (cap == d.slots_cap) return;
  const size_t poly_words = d.params->p.planes() * POLY_LEN;
  DevBuf<u64> bigger(cap * poly_words);
  if (d.slots_cap) HIP_CHECK(hipMemcpy(bigger.p, d.polys.p, d.slots_cap * poly_words * 8, hipMemcpyDeviceToDevice));
  if (d.slots_cap && tunable("h2d_cache_sync", 0) != 0) launch_cache_sync(nullptr, 0);  // (as h2d_sync)
  d.polys = std::move(bigger);
  d.slots_cap = cap;
}

// ---- sp_db_update_items: many upserts per launch
struct UpsertRec {
  size_t idx;
  const uint8_t* data;
  size_t len;
};
// One upload window of a bulk upsert: `groups` encode groups (a sparse bucket's items, a dense database's touched quads) from
// `first`, whose records carry `bytes` bytes; `cells` = entries of the planar patch list.  The device image of a window is
// [group table | cell table | item bytes], each part from a 16-byte boundary: one copy per window.
struct UpsertWindow {
  size_t first = 0, groups = 0, bytes = 0, cells = 0;
};
size_t round16(size_t x) { return (x + 15) & ~(size_t)15; }
// the windows of a call: at most db_load_window item bytes each (a group larger than that travels alone) and at most
// UPSERT_MAX_GROUP_PLANES / planes groups, which keeps the encode launches and the patch launch below 2^31 blocks along grid.x
template <typename BytesOf>
std::vector<UpsertWindow> upsert_windows(size_t n_groups, size_t planes, BytesOf&& bytes_of) {
  const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));
  const size_t max_groups = std::max<size_t>(1, UPSERT_MAX_GROUP_PLANES / planes);
  std::vector<UpsertWindow> wins;
  for (size_t g = 0; g < n_groups; g++) {
    const size_t b = bytes_of(g);
    if (wins.empty() || wins.back().groups >= max_groups || (wins.back().groups && wins.back().bytes + b > max_win)) {
      wins.emplace_back();
      wins.back().first = g;
    }
    wins.back().groups++;
    wins.back().bytes += b;
  }
  return wins;
}

// a sparse bucket: update_many_items (loading.rs:361-377) over sparse_db.rs:42-48 upsert; `recs` hold each index once, in order of
// first appearance (caller holds mu)
void upsert_sparse(sp_db& d, const std::vector<UpsertRec>& all) {
  sp_params* h = const_cast<sp_params*>(d.params);
  const Params& p = h->p;
  std::vector<UpsertRec> own;   // a row shard stores the items of its rows only: the others take no slot
  if (d.num_shards > 1) {
    for (const UpsertRec& r : all)
      if (sparse_holds(d, r.idx)) own.push_back(r);
  }
  const std::vector<UpsertRec>& recs = d.num_shards > 1 ? own : all;
  if (recs.empty()) return;
  DeviceState& D = h->device_state();
  const size_t planes = p.planes();
  // new keys: slots in order of first appearance, the store grown once for all of them, before the first kernel
  size_t n_new = 0;
  for (const UpsertRec& r : recs) n_new += d.slot_of.count(r.idx) == 0;
  sparse_reserve(d, d.slot_of.size() + n_new);
  const std::vector<UpsertWindow> wins = upsert_windows(recs.size(), planes, [&](size_t g) { return recs[g].len; });
  size_t image = 1;
  for (const UpsertWindow& w : wins) image = std::max(image, round16(w.groups * sizeof(SparseItemRec)) + w.bytes);
  d.upload.ensure(image);
  std::vector<uint8_t> host(image);
  if (n_new && !d.rows_dirty) {  // does a new item open a new first-dimension row?  (then the pruned expansion plan changes)
    std::vector<char> row_set(p.dim0(), 0);
    for (const auto& kv : d.slot_of) row_set[kv.first / p.num_per()] = 1;
    for (const UpsertRec& r : recs)
      if (!row_set[r.idx / p.num_per()]) d.rows_dirty = true;
  }
  std::vector<SparseItemRec> table;
  for (const UpsertWindow& w : wins) {
    table.resize(w.groups);
    const size_t bytes0 = round16(w.groups * sizeof(SparseItemRec));
    size_t off = 0;
    for (size_t g = 0; g < w.groups; g++) {
      const UpsertRec& r = recs[w.first + g];
      auto it = d.slot_of.find(r.idx);
      if (it == d.slot_of.end()) it = d.slot_of.emplace(r.idx, d.slot_of.size()).first;
      table[g] = SparseItemRec{(unsigned long long)off, (int)r.len, (int)it->second};
      if (r.len) memcpy(host.data() + bytes0 + off, r.data, r.len);
      off += r.len;
    }
    memcpy(host.data(), table.data(), w.groups * sizeof(SparseItemRec));
    h2d_sync(d.upload.p, host.data(), bytes0 + w.bytes);
    launch_sparse_items_encode(D.T, d.upload.p + bytes0, reinterpret_cast<const SparseItemRec*>(d.upload.p), w.groups,
                               (int)p.db_item_size, (int)chunk_bytes(p), (int)pt_bits(p), (u32)p.pt_modulus, d.polys.p, (int)planes, 0);
    HIP_CHECK(hipDeviceSynchronize());
  }
  if (n_new) d.index_dirty = true;   // overwrites (the reference's upsert of an existing key) leave the index alone
}

// a dense database or shard: the records it holds grouped by quad (local row pair, local column pair), a quad listed once with every
// item of it that the call updates -- two items of a quad share a PACKED lane group and must be one workgroup's (caller holds mu)
void upsert_dense(sp_db& d, const std::vector<UpsertRec>& recs) {
  sp_params* h = const_cast<sp_params*>(d.params);
  const Params& p = h->p;
  DeviceState& D = h->device_state();
  const size_t planes = p.planes(), npq = ((size_t)d.np_local + 1) / 2;
  struct Quad {
    int jp, q;
    long rec[4];
  };
  std::vector<Quad> quads;
  std::unordered_map<size_t, size_t> quad_of;
  for (size_t i = 0; i < recs.size(); i++) {
    const size_t j = recs[i].idx / p.num_per(), ii = recs[i].idx % p.num_per();
    if ((int)j < d.j0 || (int)j >= d.j0 + d.nj) continue;   // row lives on another shard
    if ((int)(ii % (size_t)d.col_G) != d.col_g) continue;   // column lives on another shard
    const int jl = (int)j - d.j0, il = (int)(ii / (size_t)d.col_G);
    auto it = quad_of.emplace((size_t)(jl / 2) * npq + (size_t)(il / 2), quads.size());
    if (it.second) quads.push_back(Quad{jl / 2, il / 2, {-1, -1, -1, -1}});
    quads[it.first->second].rec[(jl & 1) * 2 + (il & 1)] = (long)i;
  }
  auto quad_bytes = [&](size_t g) {
    size_t b = 0;
    for (long r : quads[g].rec) b += r >= 0 ? recs[(size_t)r].len : 0;
    return b;
  };
  std::vector<UpsertWindow> wins = upsert_windows(quads.size(), planes, quad_bytes);
  const bool patch = d.planar_state == 1;   // a planar copy follows its items: the 16-row groups of the touched columns are regathered
  size_t image = 1;
  for (UpsertWindow& w : wins) {
    w.cells = patch ? 2 * w.groups : 0;   // (a quad's two rows share a 16-row group: its two columns; an upper bound, see below)
    image = std::max(image, round16(w.groups * sizeof(DbQuadRec)) + round16(w.cells * sizeof(PlanarPatchCell)) + w.bytes);
  }
  d.upload.ensure(image);
  std::vector<uint8_t> host(image);
  std::vector<DbQuadRec> table;
  std::vector<PlanarPatchCell> cells;
  std::unordered_map<size_t, char> cell_seen;
  for (const UpsertWindow& w : wins) {
    table.resize(w.groups);
    cells.clear();
    cell_seen.clear();
    const size_t cells0 = round16(w.groups * sizeof(DbQuadRec)), bytes0 = cells0 + round16(w.cells * sizeof(PlanarPatchCell));
    size_t off = 0;
    for (size_t g = 0; g < w.groups; g++) {
      const Quad& q = quads[w.first + g];
      DbQuadRec t{};
      t.jp = q.jp;
      t.q = q.q;
      for (int ab = 0; ab < 4; ab++) {
        t.src[ab] = -1;
        if (q.rec[ab] < 0) continue;
        const UpsertRec& r = recs[(size_t)q.rec[ab]];
        t.src[ab] = (long long)off;
        t.len[ab] = (int)r.len;
        if (r.len) memcpy(host.data() + bytes0 + off, r.data, r.len);
        off += r.len;
        const int jl = 2 * q.jp + (ab >> 1), il = 2 * q.q + (ab & 1);
        if (patch && cell_seen.emplace((size_t)(jl >> 4) * (size_t)d.np_local + (size_t)il, 1).second) cells.push_back(PlanarPatchCell{jl, il});
      }
      table[g] = t;
    }
    memcpy(host.data(), table.data(), w.groups * sizeof(DbQuadRec));
    if (!cells.empty()) memcpy(host.data() + cells0, cells.data(), cells.size() * sizeof(PlanarPatchCell));
    h2d_sync(d.upload.p, host.data(), bytes0 + w.bytes);
    DbEncodeDesc e = encode_desc(d);
    e.win = d.upload.p + bytes0;
    launch_db_encode_quads(D.T, e, reinterpret_cast<const DbQuadRec*>(d.upload.p), w.groups, 0);
    if (patch)   // same stream, after the encode
      launch_planar_patch_items(reinterpret_cast<unsigned char*>(d.planar->p), d.words.p, (int)planes, d.np_local, d.nj,
                                reinterpret_cast<const PlanarPatchCell*>(d.upload.p + cells0), cells.size(), 0);
    HIP_CHECK(hipDeviceSynchronize());
  }
}

// ---- planar-resident databases (sp_db_create_planar): every writer stages words in the handle's upload buffer and stores them to their
// planar positions from there (planar_resident.hpp); no buffer of the database's size other than the planar words ever exists
constexpr size_t PLANAR_STAGE_BYTES = (size_t)64 << 20;   // 8-byte words staged per launch, at most (one item or column at least)
unsigned char* planar_words(sp_db& d) { return reinterpret_cast<unsigned char*>(d.words.p); }
// the handle as the writers of planar_resident.hpp take it: its row window and, on a row shard (sp_db_create_planar_shard), the
// resident column order of a shard of num_shards
PlanarShardShape planar_shape(const sp_db& d) { return PlanarShardShape{(int)d.params->p.dim0(), d.j0, d.num_shards}; }

// upserts: `recs` hold each index once.  Per window the existing list encoder (k_db_encode_quads: chunks, log2(p)-bit coefficients,
// recenter_mod, forward NTT) writes the items' words as an 8-byte database of two rows in the upload buffer -- item r of the window is
// entry r & 3 of quad r >> 2 -- and k_planar_put_items stores each word's 8 digit bytes.  The device image of a window is
// [quad table | cell table | item bytes | staged words], each part from a 16-byte boundary (caller holds mu)
void upsert_planar(sp_db& d, const std::vector<UpsertRec>& all) {
  sp_params* h = const_cast<sp_params*>(d.params);
  // a row shard keeps the records of its rows (the others are some other rank's: skipped, and counted as applied by the callers)
  std::vector<UpsertRec> recs;
  recs.reserve(all.size());
  for (const UpsertRec& r : all)
    if (sparse_holds(d, r.idx)) recs.push_back(r);
  if (recs.empty()) return;
  const Params& p = h->p;
  DeviceState& D = h->device_state();
  const size_t planes = p.planes(), word_bytes = planes * POLY_LEN * 8;   // staged bytes of one item
  const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));
  const size_t max_items = std::max<size_t>(1, std::min(PLANAR_STAGE_BYTES / word_bytes, UPSERT_MAX_GROUP_PLANES / planes));
  std::vector<UpsertWindow> wins;   // groups = items here
  for (size_t i = 0; i < recs.size(); i++) {
    if (wins.empty() || wins.back().groups >= max_items || wins.back().bytes + recs[i].len > max_win) {
      wins.emplace_back();
      wins.back().first = i;
    }
    wins.back().groups++;
    wins.back().bytes += recs[i].len;
  }
  auto layout = [&](const UpsertWindow& w, size_t& cells0, size_t& bytes0, size_t& stage0, size_t& np_s) {
    const size_t quads = (w.groups + 3) / 4;
    np_s = 2 * quads;
    cells0 = round16(quads * sizeof(DbQuadRec));
    bytes0 = cells0 + round16(w.groups * sizeof(PlanarPatchCell));
    stage0 = bytes0 + round16(w.bytes);
    return stage0 + 2 * np_s * word_bytes;   // [plane][z][2 rows][np_s columns]
  };
  size_t image = 1, cells0, bytes0, stage0, np_s;
  for (const UpsertWindow& w : wins) image = std::max(image, layout(w, cells0, bytes0, stage0, np_s));
  d.upload.ensure(image);   // before the first kernel: nothing is allocated between the launches below
  std::vector<uint8_t> host;
  for (const UpsertWindow& w : wins) {
    layout(w, cells0, bytes0, stage0, np_s);
    host.assign(stage0, 0);
    DbQuadRec* table = reinterpret_cast<DbQuadRec*>(host.data());
    PlanarPatchCell* cells = reinterpret_cast<PlanarPatchCell*>(host.data() + cells0);
    for (size_t q = 0; q < np_s / 2; q++) {
      table[q].jp = 0;
      table[q].q = (int)q;
      for (int ab = 0; ab < 4; ab++) table[q].src[ab] = -1;
    }
    size_t off = 0;
    for (size_t r = 0; r < w.groups; r++) {
      const UpsertRec& rec = recs[w.first + r];
      table[r >> 2].src[r & 3] = (long long)off;
      table[r >> 2].len[r & 3] = (int)rec.len;
      if (rec.len) memcpy(host.data() + bytes0 + off, rec.data, rec.len);
      off += rec.len;
      cells[r] = PlanarPatchCell{(int)(rec.idx / p.num_per()) - d.j0, (int)(rec.idx % p.num_per())};
    }
    h2d_sync(d.upload.p, host.data(), stage0);
    u64* stage = reinterpret_cast<u64*>(d.upload.p + stage0);
    DbEncodeDesc e = encode_desc(d);
    e.db = stage;
    e.packed = 0;
    e.num_per = (int)np_s;
    e.nj = 2;
    e.j0 = 0;
    e.cm = ColMap{0, 1, (int)np_s};
    e.win = d.upload.p + bytes0;
    launch_db_encode_quads(D.T, e, reinterpret_cast<const DbQuadRec*>(d.upload.p), np_s / 2, 0);
    launch_planar_put_items(planar_words(d), stage, (int)planes, np_s, reinterpret_cast<const PlanarPatchCell*>(d.upload.p + cells0), w.groups,
                            d.np_local, d.nj, planar_shape(d), 0);   // same stream, after the encode
    HIP_CHECK(hipDeviceSynchronize());
  }
}

// `n` checked records in call order -> what sp_db_update_item on each in turn would leave: a later record for an index wins
// (deduplicated here, before anything is launched; the survivors keep the order of first appearance, which is the order sequential
// calls hand out a sparse bucket's slots in)
void upsert_many(sp_db& d, const UpsertRec* in, size_t n) {
  if (n == 0) return;
  std::vector<UpsertRec> recs;
  recs.reserve(n);
  std::unordered_map<size_t, size_t> at;
  at.reserve(n);
  for (size_t i = 0; i < n; i++) {
    auto it = at.emplace(in[i].idx, recs.size());
    if (it.second)
      recs.push_back(in[i]);
    else
      recs[it.first->second] = in[i];
  }
  std::lock_guard<std::mutex> lk(d.mu);
  if (d.sparse)
    upsert_sparse(d, recs);
  else if (d.planar_resident)
    upsert_planar(d, recs);
  else
    upsert_dense(d, recs);
}
// sp_db_update_item's own bounds for an entry of a list: "" when it passes, else the fault (the text is built only then)
std::string upsert_fault(const Params& p, size_t idx, size_t len) {
  if (idx >= p.num_items()) return "item index " + std::to_string(idx) + " out of range (num_items " + std::to_string(p.num_items()) + ")";
  if (len > p.db_item_size) return std::to_string(len) + " item bytes, db_item_size is " + std::to_string(p.db_item_size);
  return std::string();
}

}  // namespace

SweepBatchDesc spiral::group_pass(const sp_db& db, sp_query_t* const* qs, int B, bool use_planar, PlanarPin& pin) {
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
  if (db.planar_resident) {   // the resident words are the planar operands: one or two tiles' tables, nothing to pin
    W0.batch_rq.ensure(sweep_batch_rq_words(d.nj, sweep_batch_tiles(d.batch)));
    d.rq = W0.batch_rq.p;
    d.planar = reinterpret_cast<const unsigned char*>(db.words.p);
    return d;
  }
  d.narrow = !db.packed;   // the 8-byte layout: callers come here only where sweep_narrow_batch_shape_ok holds
  if (sweep_batch_wants_mfma(d)) {
    W0.batch_rq.ensure(sweep_batch_rq_words(d.nj, sweep_batch_tiles(d.batch)));
    d.rq = W0.batch_rq.p;
    if (use_planar && sweep_batch_tiles(d.batch) == 2) pin = const_cast<sp_db&>(db).ensure_planar(W0.stream);
  }
  d.planar = pin ? reinterpret_cast<const unsigned char*>(pin->p) : nullptr;
  return d;
}
void spiral::group_pass_launch(const sp_db& db, const DevTables& T, SweepBatchDesc& d, hipStream_t s) {
  if (db.planar_resident) {
    sweep_planar_resident_prepare(T, d, s);
    launch_sweep_planar_resident(T, d, s);
    return;
  }
  sweep_batch_prepare(T, d, s);
  launch_sweep_batch(T, d, s);
}
void spiral::refuse_planar_resident(const sp_db_t* db, const char* what) {
  if (db && db->planar_resident)
    throw ArgError(std::string(what) + " does not take a planar-resident database (sp_db_create_planar): its words are read by the group pass only");
}
// the scatter sweeps take a planar ROW SHARD (sp_db_create_planar_shard) and keep refusing the unsharded handle, G = 1 included
static void refuse_planar_unsharded(const sp_db_t* db, const char* what) {
  if (db && db->num_shards == 1) refuse_planar_resident(db, what);
}
// `B` begun queries' pass over a planar row shard on qs[0]'s stream, ordered after every expansion: planes [plane0, plane0 + n_planes)
// in the per-plane layout, or all of them in sp_query_sweep_scatter's (all_planes).  The group's query tables are built in front of
// plane 0 and stay in qs[0]'s workspace for the planes that follow.  The caller orders the members' streams after it (group_pass_done).
static void planar_shard_pass(sp_query_t* const* qs, int B, const sp_db_t* db, int G, int plane0, int n_planes, bool all_planes) {
  const int planes = (int)db->params->p.planes();
  for (int i = 0; i < B; i++) qs[i]->ws->ensure_sweep();   // every buffer before anything is enqueued
  PlanarPin none;
  SweepBatchDesc d = group_pass(*db, qs, B, false, none);
  d.planes = n_planes;
  d.planar += sweep_planar_bytes(1, db->np_local, db->nj) * (size_t)plane0;
  Workspace& W0 = group_pass_stream(qs, B);
  if (plane0 == 0)
    sweep_planar_resident_prepare(W0.D->T, d, W0.stream);
  else
    d.use_mfma = 1;
  launch_sweep_planar_scatter(W0.D->T, d, G, plane0, planes, all_planes, W0.stream);
}
Workspace& spiral::group_pass_stream(sp_query_t* const* qs, int B) {
  Workspace& W0 = *qs[0]->ws;
  for (int i = 1; i < B; i++) HIP_CHECK(hipStreamWaitEvent(W0.stream, qs[i]->ws->ev[1], 0));
  return W0;
}
void spiral::group_pass_done(sp_query_t* const* qs, int i) {
  Workspace& W = *qs[i]->ws;
  if (i > 0) HIP_CHECK(hipStreamWaitEvent(W.stream, qs[0]->ws->ev[2], 0));
  HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
}

void spiral::sparse_group_pass(const sp_db& db, sp_query_t* const* qs, int B, hipStream_t s) {
  need(B >= 1 && B <= SPARSE_GROUP_MAX, "a sparse bucket's pass takes 1 .. 8 queries");
  Workspace* Ws[SPARSE_GROUP_MAX];
  for (int i = 0; i < B; i++) {
    need(qs[i] && qs[i]->for_sparse == &db && qs[i]->sparse_index == qs[0]->sparse_index,
         "the queries of a sparse bucket's group must have been begun on one snapshot of its index");
    Ws[i] = qs[i]->ws.get();
  }
  const sp_db::SparseIndex& idx = *qs[0]->sparse_index;
  run_sweep_sparse_group(Ws, B, db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p, s);
}

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

// ---- pieces of the query stage machine (below) that are not entry points themselves
// the head of every query: the handles checked, a sparse bucket's index snapshot taken, the workspace acquired and the "begin" event
// recorded; state 0
static std::unique_ptr<sp_query> open_query(const sp_params_t* h, const sp_pp_t* pp, const sp_db_t* db,
                                            std::shared_ptr<const sp_db::SparseIndex> snapshot = nullptr) {
  need(h && pp, "null argument");
  need(pp->params == h, "public parameters were created for different params");
  need(!db || db->params == h, "db was created for different params");
  check_device(pp->device);
  auto q = std::make_unique<sp_query>();
  if (db && db->sparse) q->sparse_index = snapshot ? std::move(snapshot) : const_cast<sp_db*>(db)->ensure_sparse_index();
  q->params = const_cast<sp_params*>(h);
  q->pp = pp;
  q->ws = q->params->acquire_ws();
  HIP_CHECK(hipEventRecord(q->ws->ev[0], q->ws->stream));
  return q;
}
sp_query_t* spiral::query_open(const sp_params_t* h, const sp_pp_t* pp) {
  return guarded_handle([&] { return open_query(h, pp, nullptr); });
}

// the rest of sp_query_begin_for_db once the query is open: the expansion (pruned to a row shard's rows or to a sparse bucket's
// occupied rows, the snapshot the query holds) enqueued on the query's stream, ev[1] recorded; state 1
static void begin_opened(sp_query* q, const uint8_t* query, size_t query_len, const sp_db_t* db) {
  const sp_params* h = q->params;
  const sp_pp* pp = q->pp;
  Workspace& W = *q->ws;
  const bool rows = db && db->num_shards > 1 && db->col_G == 1;
  const DeviceState::PrunedPlan* plan = q->sparse_index ? q->sparse_index->plan.get() : nullptr;
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
}
sp_query_t* spiral::query_open_sparse(const sp_params_t* h, const sp_pp_t* pp, const sp_db_t* db,
                                      std::shared_ptr<const sp_db::SparseIndex> snapshot) {
  return guarded_handle([&] {
    need(db && db->sparse && snapshot, "null argument");
    auto q = open_query(h, pp, db, std::move(snapshot));
    q->ws->ensure_sweep();
    return q;
  });
}
void spiral::query_begin_opened(sp_query_t* q, const uint8_t* query, size_t query_len, const sp_db_t* db) {
  need(q && query && q->state == 0, "null argument");
  begin_opened(q, query, query_len, db);
}

// a begun query goes over `db` only if it was expanded for every row, or for the rows of exactly this row shard
static void need_rows_of(const sp_query_t* q, const sp_db_t* db) {
  need(q->rows_nj == 0 || (db->col_G == 1 && db->j0 == q->rows_j0 && db->nj == q->rows_nj),
       "the query was expanded for another row shard (sp_query_begin_for_db)");
}
// the shard count of the scatter sweeps (with `db`: it is one of G shards) and of the local folds
static void need_shard_count(const Params& p, int G, const sp_db_t* db = nullptr) {
  const bool ok = G >= 1 && (G & (G - 1)) == 0 && (size_t)G <= p.num_per() && G <= SP_MAX_ROW_SHARDS;
  if (!db) return need(ok, "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS)");
  need(ok && db->num_shards == G, "G must be a power of two <= min(num_per, SP_MAX_ROW_SHARDS) and equal to the db's num_shards");
}
static void need_row_shard(const sp_db_t* db) { need(db->col_G == 1, "sweep_scatter works on row shards"); }
// a sparse bucket (or row shard of one) is swept by the queries begun for it, each with the snapshot of the index it was begun on
static void need_begun_for(const sp_query_t* q, const sp_db_t* db) {
  need(q->for_sparse == nullptr || q->for_sparse == db, "the query was expanded for another sparse bucket");
  if (db->sparse) need(q->for_sparse == db && q->sparse_index, "a sparse bucket needs sp_query_begin_for_db(…, db) (its expansion is pruned)");
}
// switch sparse_batch_min as the list flow reads it (capi_batch.cpp): the smallest group that shares one pass, 0 = none does
static int sparse_group_min() {
  long m = tunable("sparse_batch_min", SPARSE_BATCH_MIN_DEFAULT);
  if (m < 0) m = SPARSE_BATCH_MIN_DEFAULT;
  return m == 0 || m > SPARSE_GROUP_MAX ? 0 : (int)std::max(2L, m);
}
// one query's scatter sweep over a sparse row shard, planes [plane0, plane0 + n_planes), on its own stream; the folds that follow
// (sp_query_fold_local*, sp_query_finish_gathered) take lib/server's all-zero shortcuts (fold.rs:38-44)
static void sweep_sparse_scatter(sp_query_t* q, const sp_db_t* db, int G, int plane0, int n_planes, bool per_plane) {
  const sp_db::SparseIndex& idx = *q->sparse_index;
  run_sweep_sparse_scatter(*q->ws, *db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p, G, plane0, n_planes, per_plane);
  q->ws->zero_shortcuts = true;
}
// the workspace's first-dimension output in the reduce-scatter layout of G shards while the scope's sweep launches are enqueued:
// plain again on every path out of it, so that the workspace never goes on to another stage, or back to the pool, in scatter layout
struct ScatterLayout {
  Workspace& W;
  ScatterLayout(Workspace& w, int G) : W(w) { W.out_G = G; }
  ~ScatterLayout() { W.out_G = 1; }
};

void spiral::scatter_group_check(sp_query_t* const* qs, int batch, const sp_db_t* db, int G) {
  need(qs && db, "null argument");
  refuse_planar_unsharded(db, "sp_query_sweep_scatter_group");
  if (db->planar_resident)   // a planar row shard: both query tiles where the device offers their LDS to one workgroup
    need(batch >= 1 && batch <= planar_resident_group_max(db->nj), "sp_query_sweep_scatter_group: 1 .. 16 queries per pass over a planar row shard "
                                                                   "(1 .. 8 where two query tiles' tables do not fit one workgroup's LDS)");
  else
    need(batch >= 1 && batch <= SWEEP_BATCH_MAX, "sp_query_sweep_scatter_group: 1 .. 8 queries per pass (1 .. 16 over a planar row shard, "
                                                 "sp_db_create_planar_shard)");
  need_row_shard(db);
  need_shard_count(db->params->p, G, db);
  for (int i = 0; i < batch; i++) {
    need(qs[i] && qs[i]->ws, "null query");
    need(qs[i]->params == db->params, "db was created for different params");
    need_rows_of(qs[i], db);
    need_begun_for(qs[i], db);
    for (int k = 0; k < i; k++) need(qs[k] != qs[i], "sp_query_sweep_scatter_group: the same query twice");
  }
  check_device(db->device);
}
bool spiral::scatter_group_desc(sp_query_t* const* qs, int batch, const sp_db_t* db, int G, SweepBatchDesc& d) {
  for (int i = 0; i < batch; i++) qs[i]->ws->ensure_sweep();
  if (!db->packed || db->sparse || G < 2) return false;   // (a planar row shard has its own pass: planar_shard_pass)
  PlanarPin none;
  d = group_pass(*db, qs, batch, false, none);
  return d.rq != nullptr && sweep_batch_scatter_ok(d, G);
}

// the end of both finishing calls: wait for the stream, the response out, the stage timings (the spans between the workspace's
// five events) in
static void collect_response(sp_query_t* q, uint8_t* out, size_t* out_len) {
  const Workspace& W = *q->ws;
  HIP_CHECK(hipStreamSynchronize(W.stream));
  *out_len = q->params->p.response_bytes();
  memcpy(out, W.h_response, *out_len);
  for (int k = 0; k < 4; k++) {
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, W.ev[k], W.ev[k + 1]));
    q->ms[k] = t;
  }
}

void spiral::finish_impl(sp_query_t* q, bool premod, uint8_t* out, size_t out_cap, size_t* out_len) {
  need(q && out && out_len, "null argument");
  need(q->state == 2, "sp_query_finish: sweep has not run");
  const Params& p = q->params->p;
  need(out_cap >= p.response_bytes(), "output buffer smaller than response_bytes");
  Workspace& W = *q->ws;
  debug_stage(3);
  run_finish(W, *q->pp, premod);
  collect_response(q, out, out_len);
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

extern "C" {

const char* sp_last_error(void) { return g_last_error.c_str(); }

uint64_t sp_paths_taken(int reset) { return paths_taken(reset != 0); }
int sp_debug_set(const char* name, long value) {
  if (!name) return SP_E_ARG;
  set_tunable(name, value);
  return SP_OK;
}
// internal hooks for comm.cpp (not declared in the public header)
extern "C" void sp_shard_split_hint_(int on) { g_shard_split_hint = on; }
// group = 0 of sp_process_queries_sharded_batched: 8 where a group of 8 takes the scatter-form pass on this shard and the shard
// count is one where the batched list measured faster than the pipelined one (switch batch_scatter_max_g; profiles/sharded_batch_pass.md),
// else 1 = the per-query flow.  Depends on the shard's shape and the switches only: the same answer on every rank.
extern "C" int sp_scatter_group_choice_(const sp_db_t* db, int G) {
  if (db && db->sparse) {   // 8 where the list flow's switch lets a group share one pass over a sparse shard at all
    tunables_new_call();
    return db->col_G == 1 && db->num_shards == G && sparse_group_min() != 0 ? SPARSE_GROUP_MAX : 1;
  }
  // a planar row shard: 16 where the shape allows two query tiles, else 8 (the handle's format was decided when it was created)
  if (db && db->planar_resident) return db->num_shards == G && G > 1 ? planar_resident_group_max(db->nj) : 1;
  if (!db || !db->packed || db->col_G != 1 || db->num_shards != G) return 1;
  SweepBatchDesc d{};
  d.batch = SWEEP_BATCH_MAX;
  d.num_per = db->np_local;
  d.nj = db->nj;
  tunables_new_call();
  return sweep_batch_scatter_ok(d, G) && G <= (int)tunable("batch_scatter_max_g", BATCH_SCATTER_MAX_G_DEFAULT) ? SWEEP_BATCH_MAX : 1;
}
// the largest group sp_process_queries_sharded_batched takes on this shard: 16 / 8 on a planar row shard (its two-tile rule), 8 elsewhere
extern "C" int sp_shard_group_max_(const sp_db_t* db) {
  return db && db->planar_resident && db->num_shards > 1 ? planar_resident_group_max(db->nj) : SWEEP_BATCH_MAX;
}
extern "C" int sp_db_num_shards_(const sp_db_t* db) { return db ? db->num_shards : 0; }
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
                                "expand_group", "expand_wave", "sweep_batch_scatter", "sparse_group_pass", "sweep_narrow_group"};
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
  return guarded_handle([&] {
    need(json != nullptr, "json is null");
    auto h = std::make_unique<sp_params>();
    h->p = Params::from_json(json);
    return h;
  });
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
  return guarded_handle([&] {
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
    return d;
  });
}
// lib/server's SparseDb (lib/server/src/db/sparse_db.rs:5-48): an empty bucket that stores only the items written to it -- or, as
// row shard `shard` of `num_shards` (sp_db_create's rule), only those of them whose row j = item / num_per it holds
sp_db_t* sp_db_create_sparse_shard(const sp_params_t* h, int shard, int num_shards) {
  return guarded_handle([&] {
    need(h != nullptr, "params is null");
    const Params& p = h->p;
    need(p.expand_queries, "sparse buckets serve expanded queries (lib/server's sparse path, server.rs:31-33)");
    need(fused_fold_supported(p), "sparse buckets need gadget parameters the fused fold supports (3 <= t_gsw <= 32)");
    need(num_shards >= 1 && shard >= 0 && shard < num_shards, "bad shard");
    need(p.dim0() % (size_t)num_shards == 0, "dim0 not divisible by num_shards");
    need(num_shards <= SP_MAX_ROW_SHARDS, "at most SP_MAX_ROW_SHARDS (8) row shards: the partial residues are summed in 32 bits");
    auto d = std::make_unique<sp_db>();
    d->params = h;
    HIP_CHECK(hipGetDevice(&d->device));
    d->sparse = true;
    d->shard = shard;
    d->num_shards = num_shards;
    d->nj = (int)(p.dim0() / num_shards);
    d->j0 = shard * d->nj;
    d->np_local = (int)p.num_per();
    const_cast<sp_params*>(h)->device_state();
    return d;
  });
}
sp_db_t* sp_db_create_sparse(const sp_params_t* h) { return sp_db_create_sparse_shard(h, 0, 1); }
// A database whose only resident form is the digit-planar layout (sweep_planar.hpp): one copy of 8 bytes per word that every query
// of every list size reads.  Unsharded; the empty database (all-zero polynomials) is every byte 0x80, the offset digit of 0.
sp_db_t* sp_db_create_planar(const sp_params_t* h) {
  return guarded_handle([&] {
    need(h != nullptr, "params is null");
    const Params& p = h->p;
    if (!planar_resident_shape_ok((int)std::min<size_t>(p.num_per(), 1u << 30), (int)std::min<size_t>(p.dim0(), 1u << 30)))
      throw ArgError("sp_db_create_planar: the digit-planar layout needs dim0 % 64 == 0, dim0 <= 512 and num_per % 128 == 0 (dim0 = " +
                     std::to_string(p.dim0()) + ", num_per = " + std::to_string(p.num_per()) + ")");
    need(tunable("batch_planar", 1) != 0 && tunable("batch_mfma", 1) != 0,
         "sp_db_create_planar: the switches batch_planar and batch_mfma must be on when a planar-resident database is created");
    auto d = std::make_unique<sp_db>();
    d->params = h;
    HIP_CHECK(hipGetDevice(&d->device));
    d->planar_resident = true;
    d->planar_state = -1;   // no copy beside the words, ever
    d->packed = 0;
    d->nj = (int)p.dim0();
    d->np_local = (int)p.num_per();
    const size_t bytes = sweep_planar_bytes((int)p.planes(), d->np_local, d->nj);   // a multiple of 8
    d->words.alloc_streaming(bytes / 8, tunable("db_contiguous", 0) != 0);   // throws OomError
    HIP_CHECK(hipMemset(d->words.p, 0x80, bytes));
    HIP_CHECK(hipDeviceSynchronize());
    const_cast<sp_params*>(h)->device_state();
    return d;
  });
}
// Row shard `shard` of `num_shards` whose only resident form is the digit-planar layout, columns in the order of the exchange
// (planar_resident.hpp): what the sharded flows read with the 1 .. 16-query scatter pass (k_sweep_planar_scatter).
sp_db_t* sp_db_create_planar_shard(const sp_params_t* h, int shard, int num_shards) {
  return guarded_handle([&] {
    need(h != nullptr, "params is null");
    const Params& p = h->p;
    need(num_shards != 1, "sp_db_create_planar_shard: one shard is the whole database: use sp_db_create_planar");
    need((num_shards == 2 || num_shards == 4 || num_shards == 8) && shard >= 0 && shard < num_shards,
         "sp_db_create_planar_shard: num_shards must be 2, 4 or 8 and 0 <= shard < num_shards");
    need(p.dim0() % (size_t)num_shards == 0, "dim0 not divisible by num_shards");
    const size_t nj = p.dim0() / (size_t)num_shards;
    if (!planar_resident_shape_ok((int)std::min<size_t>(p.num_per(), 1u << 30), (int)std::min<size_t>(nj, 1u << 30)) ||
        p.num_per() / (size_t)num_shards < 2)
      throw ArgError("sp_db_create_planar_shard: the digit-planar layout needs (dim0 / num_shards) % 64 == 0, dim0 / num_shards <= 512 and "
                     "num_per % 128 == 0 (dim0 / num_shards = " + std::to_string(nj) + ", num_per = " + std::to_string(p.num_per()) + ")");
    need(tunable("batch_planar", 1) != 0 && tunable("batch_mfma", 1) != 0,
         "sp_db_create_planar_shard: the switches batch_planar and batch_mfma must be on when a planar-resident database is created");
    auto d = std::make_unique<sp_db>();
    d->params = h;
    HIP_CHECK(hipGetDevice(&d->device));
    d->planar_resident = true;
    d->planar_state = -1;   // no copy beside the words, ever
    d->packed = 0;
    d->shard = shard;
    d->num_shards = num_shards;
    d->nj = (int)nj;
    d->j0 = shard * d->nj;
    d->np_local = (int)p.num_per();
    const size_t bytes = sweep_planar_bytes((int)p.planes(), d->np_local, d->nj);   // a multiple of 8
    d->words.alloc_streaming(bytes / 8, tunable("db_contiguous", 0) != 0);   // throws OomError
    HIP_CHECK(hipMemset(d->words.p, 0x80, bytes));
    HIP_CHECK(hipDeviceSynchronize());
    const_cast<sp_params*>(h)->device_state();
    return d;
  });
}
const char* sp_db_format(const sp_db_t* d) {
  if (!d) return "";
  return d->sparse ? "sparse" : d->planar_resident ? "planar" : d->packed ? "packed" : "words8";
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
      if (d->planar_resident)   // the window of z-rows straight to planar entries
        launch_planar_from_ref(planar_words(*d), stage, plane, z0 + z, cnt, d->np_local, d->nj, planar_shape(*d), 0);
      else
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
    if (d->planar_resident) {
      // windows of one 16-row group (the rows of one planar entry): its raw items, then per span of `ncols` columns the existing
      // encoder writes the span as an 8-byte database of 16 rows x ncols columns behind them in the upload buffer and
      // k_planar_from_stage stores whole entries.  The tail is that of the PACKED loader below.
      const size_t tail = std::max(bpc, chunks * bpc - p.db_item_size);
      const size_t raw = round16(16 * row_bytes + tail);
      int ncols = 128;   // divides num_per
      while (ncols > 2 && chunks * POLY_LEN * 16 * (size_t)ncols * 8 > PLANAR_STAGE_BYTES) ncols /= 2;
      d->upload.ensure(raw + chunks * POLY_LEN * 16 * (size_t)ncols * 8);
      u64* stage = reinterpret_cast<u64*>(d->upload.p + raw);
      for (int jg = 0; jg < d->nj / 16; jg++) {
        const size_t item0 = (size_t)(d->j0 + 16 * jg) * p.num_per();   // (a row shard: the file's rows j0 ..)
        const size_t off = item0 * p.db_item_size;
        const size_t have = off < file_len ? std::min(16 * row_bytes + tail, file_len - off) : 0;
        if (have) h2d_sync(d->upload.p, file + off, have);
        for (int ii0 = 0; ii0 < d->np_local; ii0 += ncols) {
          DbEncodeDesc e = encode_desc(*d);
          e.db = stage;
          e.packed = 0;
          e.num_per = ncols;
          e.cm = ColMap{ii0, 1, d->np_local};
          e.j0 = d->j0 + 16 * jg;
          e.nj = 16;
          e.win = d->upload.p;
          e.win_item0 = item0;
          e.win_bytes = have;
          e.file_len = file_len;
          e.jp0 = 0;
          e.njp = 8;
          launch_db_encode(D.T, e, 0);
          launch_planar_from_stage(planar_words(*d), stage, (int)chunks, jg, ii0, ncols, d->np_local, d->nj, planar_shape(*d), 0);
        }
        HIP_CHECK(hipDeviceSynchronize());
      }
      return;
    }
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
      if (!sparse_holds(*d, item_idx)) return;   // the row lives on another shard: no slot is taken
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
        sparse_reserve(*d, slot + 1);  // grows the polynomial store when it is full
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
    if (d->planar_resident) {   // a list of one: the item's 8 digit bytes per (plane, z)
      const UpsertRec one{item_idx, data, len};
      upsert_many(*d, &one, 1);
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

int sp_db_update_items(sp_db_t* d, const size_t* item_idx, const uint8_t* const* data, const size_t* lens, size_t n) {
  return guarded([&] {
    need(d && ((item_idx && data && lens) || n == 0), "null argument");
    check_device(d->device);
    const Params& p = d->params->p;
    std::vector<UpsertRec> recs(n);
    for (size_t i = 0; i < n; i++) {   // every entry is checked before the first is written
      if (item_idx[i] >= p.num_items() || lens[i] > p.db_item_size) throw ArgError("entry " + std::to_string(i) + ": " + upsert_fault(p, item_idx[i], lens[i]));
      need(data[i] || lens[i] == 0, "null argument");
      recs[i] = UpsertRec{item_idx[i], data[i], lens[i]};
    }
    upsert_many(*d, recs.data(), n);
  });
}

int sp_db_update_rows(sp_db_t* d, const uint8_t* body, size_t body_len, size_t* applied, size_t* largest_update) {
  if (applied) *applied = 0;
  if (largest_update) *largest_update = 0;
  return guarded([&] {
    need(d && (body || body_len == 0), "null argument");
    check_device(d->device);
    const Params& p = d->params->p;
    // update_many_items (loading.rs:361-377): be32 chunk_len | chunk = be32 item index | item bytes (update_item, :301-315)
    auto be32 = [&](size_t at) { return ((size_t)body[at] << 24) | ((size_t)body[at + 1] << 16) | ((size_t)body[at + 2] << 8) | (size_t)body[at + 3]; };
    std::vector<UpsertRec> recs;
    std::string fault;
    size_t off = 0, largest = 0;
    while (off < body_len && fault.empty()) {
      const size_t left = body_len - off;
      const size_t chunk_len = left >= 4 ? be32(off) : 0;
      if (left < 4)
        fault = "the body ends inside its length";
      else if (chunk_len > left - 4)
        fault = "chunk_len " + std::to_string(chunk_len) + " but the body has " + std::to_string(left - 4) + " more bytes";
      else if (chunk_len < 4)
        fault = "chunk_len " + std::to_string(chunk_len) + " does not hold the item index";
      else if (be32(off + 4) >= p.num_items() || chunk_len - 4 > p.db_item_size)
        // item bytes 0 .. db_item_size as sp_db_update_item; the reference's bound (loading.rs:305-310) is whole chunks
        fault = upsert_fault(p, be32(off + 4), chunk_len - 4);
      else {
        recs.push_back(UpsertRec{be32(off + 4), body + off + 8, chunk_len - 4});
        largest = std::max(largest, chunk_len);
        off += 4 + chunk_len;
      }
    }
    if (!fault.empty()) fault = "/update-row record " + std::to_string(recs.size()) + " at byte offset " + std::to_string(off) + ": " + fault;
    // the records before a faulty one are applied: the reference applies while it parses
    upsert_many(*d, recs.data(), recs.size());
    if (applied) *applied = recs.size();
    if (largest_update) *largest_update = largest;
    if (!fault.empty()) throw ArgError(fault + " (" + std::to_string(recs.size()) + " records applied)");
  });
}

int sp_db_fill_synthetic(sp_db_t* d, uint64_t seed) {
  return guarded([&] {
    need(d != nullptr, "null db");
    need(!d->sparse, "a sparse bucket is filled through sp_db_update_item");
    check_device(d->device);
    sp_db::WriteScope write(*d);
    const Params& p = d->params->p;
    if (d->planar_resident)
      launch_planar_synth(planar_words(*d), seed, (int)p.planes(), d->np_local, d->nj, planar_shape(*d), 0);
    else
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
    // (a planar-resident database is what the lists read already: nothing to build, nothing allocated)
    const bool c = d->planar_resident || (!d->sparse && d->ensure_planar(nullptr));
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
    if (d->planar_resident)
      launch_planar_read(tmp.p, reinterpret_cast<const unsigned char*>(d->words.p), plane, z, ii, j0, count, d->np_local, d->nj,
                         planar_shape(*d), 0);
    else
      launch_db_read(tmp.p, d->words.p, plane, z, ii / d->col_G, j0, count, d->np_local, d->nj, d->packed, 0);
    HIP_CHECK(hipMemcpy(out, tmp.p, (size_t)count * 8, hipMemcpyDeviceToHost));
  });
}

// ------------------------------------------------------------------------- PublicParameters
sp_pp_t* sp_pp_deserialize(const sp_params_t* h, const uint8_t* data, size_t len) {
  return guarded_handle([&] {
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
    return pp;
  });
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
sp_query_t* sp_query_begin(const sp_params_t* h, const sp_pp_t* pp, const uint8_t* query, size_t query_len) {
  return sp_query_begin_for_db(h, pp, query, query_len, nullptr);
}

sp_query_t* sp_query_begin_for_db(const sp_params_t* h, const sp_pp_t* pp, const uint8_t* query, size_t query_len,
                                  const sp_db_t* db) {
  return guarded_handle([&] {
    need(h && pp && query, "null argument");
    auto q = open_query(h, pp, db);
    begin_opened(q.get(), query, query_len, db);
    return q;
  });
}

int sp_query_sweep(sp_query_t* q, const sp_db_t* db) {
  return guarded([&] {
    need(q && db, "null argument");
    need(q->state == 1, "sp_query_sweep: query not in 'begun' state");
    need(db->params == q->params, "db was created for different params");
    need_rows_of(q, db);
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
    } else if (db->planar_resident) {
      // a planar row shard keeps its columns in the exchange's order and has the scatter-form pass only: no plain partial
      need(db->num_shards == 1, "sp_query_sweep does not take a planar row shard (sp_db_create_planar_shard): use sp_query_sweep_scatter*");
      // a group of one: the one-tile pass on the query's own stream (the VALU and ring kernels never see this handle)
      W.ensure_sweep();
      sp_query_t* one[1] = {q};
      PlanarPin none;
      SweepBatchDesc d = group_pass(*db, one, 1, false, none);
      group_pass_launch(*db, W.D->T, d, W.stream);
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
    refuse_planar_unsharded(db, "sp_query_sweep_scatter");
    need(q->state == 1, "sp_query_sweep_scatter: query not in 'begun' state");
    need(db->params == q->params, "db was created for different params");
    need_rows_of(q, db);
    need_shard_count(q->params->p, G, db);
    need_row_shard(db);
    need_begun_for(q, db);
    check_device(db->device);
    Workspace& W = *q->ws;
    if (db->sparse) {   // chunk-major: chunk g = [plane][r][crt][z][ii / G]
      sweep_sparse_scatter(q, db, G, 0, (int)q->params->p.planes(), false);
    } else if (db->planar_resident) {   // a group of one, the same chunk-major layout
      sp_query_t* one[1] = {q};
      planar_shard_pass(one, 1, db, G, 0, (int)q->params->p.planes(), true);
    } else {
      ScatterLayout scatter(W, G);
      run_sweep(W, *db);
    }
    HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
    q->state = 2;
  });
}

int sp_query_sweep_scatter_plane(sp_query_t* q, const sp_db_t* db, int G, int plane) {
  return guarded([&] {
    need(q && db, "null argument");
    refuse_planar_unsharded(db, "sp_query_sweep_scatter_plane");
    need(db->params == q->params, "db was created for different params");
    need_rows_of(q, db);
    const Params& p = q->params->p;
    need_shard_count(p, G, db);
    need_row_shard(db);
    need_begun_for(q, db);
    need(plane >= 0 && (size_t)plane < p.planes(), "plane out of range");
    need(q->state == 1 && q->next_plane == plane, "sp_query_sweep_scatter_plane: planes must be swept in order after begin");
    check_device(db->device);
    Workspace& W = *q->ws;
    W.ensure_sweep();
    if (db->sparse) {
      sweep_sparse_scatter(q, db, G, plane, 1, true);
    } else if (db->planar_resident) {   // a group of one: this plane's z-range
      sp_query_t* one[1] = {q};
      planar_shard_pass(one, 1, db, G, plane, 1, false);
    } else {
      ScatterLayout scatter(W, G);
      launch_plane_sweep(W, *db, (size_t)plane);
    }
    q->next_plane = plane + 1;
    if ((size_t)q->next_plane == p.planes()) {
      HIP_CHECK(hipEventRecord(W.ev[2], W.stream));
      q->state = 2;
    }
  });
}

// One pass over the row shard for a whole group (the stage between sp_query_begin_for_db and sp_query_fold_local of the batched
// sharded list, comm.cpp).  Checks first, nothing enqueued on an error.
int sp_query_sweep_scatter_group(sp_query_t* const* qs, int batch, const sp_db_t* db, int G) {
  return guarded([&] {
    scatter_group_check(qs, batch, db, G);
    for (int i = 0; i < batch; i++)
      need(qs[i]->state == 1 && qs[i]->next_plane == 0, "sp_query_sweep_scatter_group: every query must be in 'begun' state, no plane swept");
    const size_t planes = db->params->p.planes();
    SweepBatchDesc d{};
    if (db->sparse) {
      // a sparse row shard: one pass (k_sweep_sparse_scatter_batch) for a group of at least `sparse_batch_min` members that hold ONE
      // snapshot of the shard's index; a single query, members begun either side of an upsert or the switch at 0: each member's
      // own sweep with its own snapshot, the same words.  Decided from the switch and the handles, never from the occupancy.
      const int group_min = sparse_group_min();
      bool shared = batch >= 2 && group_min != 0 && batch >= group_min;
      for (int i = 1; i < batch; i++) shared = shared && qs[i]->sparse_index == qs[0]->sparse_index;
      for (int i = 0; i < batch; i++) qs[i]->ws->ensure_sweep();   // every buffer before anything is enqueued
      if (shared) {
        Workspace* Ws[SPARSE_GROUP_MAX];
        for (int i = 0; i < batch; i++) Ws[i] = qs[i]->ws.get();
        const sp_db::SparseIndex& idx = *qs[0]->sparse_index;
        Workspace& W0 = group_pass_stream(qs, batch);
        run_sweep_sparse_scatter_group(Ws, batch, *db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p, G, W0.stream);
        for (int i = 0; i < batch; i++) {
          group_pass_done(qs, i);
          qs[i]->ws->zero_shortcuts = true;
        }
      } else {
        for (int i = 0; i < batch; i++) {
          sweep_sparse_scatter(qs[i], db, G, 0, (int)planes, true);
          HIP_CHECK(hipEventRecord(qs[i]->ws->ev[2], qs[i]->ws->stream));
        }
      }
    } else if (db->planar_resident) {
      // a planar row shard: one pass (k_sweep_planar_scatter) for every group size, one query tile or two
      planar_shard_pass(qs, batch, db, G, 0, (int)planes, false);
      for (int i = 0; i < batch; i++) group_pass_done(qs, i);
    } else if (scatter_group_desc(qs, batch, db, G, d)) {
      // ordered after every query's expansion (ev[1], recorded by sp_query_begin_for_db) ...
      Workspace& W0 = group_pass_stream(qs, batch);
      sweep_batch_prepare(W0.D->T, d, W0.stream);
      launch_sweep_batch_scatter(W0.D->T, d, G, W0.stream);
      // ... and every query's own stream after the pass
      for (int i = 0; i < batch; i++) group_pass_done(qs, i);
    } else {
      // groups of 1 .. 3, rows that are not whole 32-row blocks, 8-byte databases, batch_mfma = 0: the per-query scatter sweep
      for (int i = 0; i < batch; i++) {
        Workspace& W = *qs[i]->ws;
        ScatterLayout scatter(W, G);
        for (size_t pl = 0; pl < planes; pl++) launch_plane_sweep(W, *db, pl);
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
    need_shard_count(q->params->p, G);
    run_fold_local(*q->ws, (const u32*)reduced_chunk, G);
    q->state = 4;
  });
}
int sp_query_fold_local_plane(sp_query_t* q, const void* reduced_plane_chunk, int G, int plane) {
  return guarded([&] {
    need(q && reduced_plane_chunk, "null argument");
    const Params& p = q->params->p;
    need_shard_count(p, G);
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
    run_finish_gathered(*q->ws, *q->pp, (const u64*)gathered, G);
    collect_response(q, out, out_len);
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

}  // extern "C"

#include "capi_readback.hpp"   // sp_db_read_items, sp_db_export_rows_bound, sp_db_export_rows
#include "capi_copy.hpp"       // sp_db_copy_items (after capi_readback.hpp: its windows and the read buffer)
#include "capi_remove.hpp"     // sp_db_remove_items, sp_db_remove_range, sp_db_sparse_trim (after capi_readback.hpp: what a handle holds)
#include "capi_digest.hpp"     // sp_db_digest, sp_db_digest_ref_words
#include "capi_item_digest.hpp"   // sp_db_item_digests, sp_db_item_digests_ref_words
#include "capi_compact.hpp"    // sp_pp_compact, sp_pp_expand, sp_pp_expand_into, sp_pp_device_bytes, sp_debug_chacha20_u64_device

// The build lists of this tree (Makefile, tests/emu/build_emulated_library.py) compile capi_batch.cpp and capi_stage.cpp as
// translation units of their own and say so with SPIRAL_CAPI_SPLIT.  A list that names capi.cpp alone, as every list did before the
// file was split, still builds the whole surface.
#ifndef SPIRAL_CAPI_SPLIT
#include "capi_batch.cpp"
#include "capi_stage.cpp"
#endif
