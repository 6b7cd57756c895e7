// sp_db_remove_items / sp_db_remove_range / sp_db_sparse_trim: items taken out of a resident database on the device, on every format.
// A sparse bucket loses the key -- its store stays dense in 0 .. count - 1: the survivors at or above the new count move into the removed
// slots below it (k_sparse_move_slots, db_remove_sparse.hpp) -- and a dense handle, which holds every item of its shape, gets the empty
// database's words in the item's place (k_items_clear_words8, k_items_clear_packed of db_remove.hpp; k_planar_clear_items of
// db_remove_planar.hpp, also on the batch copy that stands beside a PACKED handle).  The host side: the checked, deduplicated list, the
// windows, and the record lists the kernels are driven by.  The lists travel through the handle's upload buffer; nothing else is staged.
// Writers under the handle's `mu` on the null stream, as sp_db_update_items.  Included by capi.cpp only, after capi_copy.hpp.
#pragma once

namespace {

// records per window: the device image [records | cells of the batch copy], each part from a 16-byte boundary, stays within
// db_load_window bytes (one record where that is smaller), and every launch within one dispatch -- with n records and P planes,
// n * P <= UPSERT_MAX_GROUP_PLANES = 2^23:
//   the clears: x <= ceil(n / 16) blocks, y = 2048 / 16 or / 32, z = P;  k_sparse_move_slots: x = n blocks = n * 256 <= 2^31 work-items,
//   y = 4 P (<= 65535).
size_t remove_window_recs(const Params& p, size_t rec_bytes) {
  const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));
  const size_t fit = max_win > 32 ? (max_win - 32) / rec_bytes : 0;   // (32: the parts' rounding)
  return std::max<size_t>(1, std::min<size_t>(fit, std::max<size_t>(1, UPSERT_MAX_GROUP_PLANES / p.planes())));
}

// a sparse bucket or sparse shard: `keys` are distinct.  Returns how many of them were present (caller holds mu)
size_t remove_sparse(sp_db& d, const std::vector<size_t>& keys) {
  const Params& p = d.params->p;
  const size_t planes = p.planes(), n = d.slot_of.size();
  std::vector<size_t> gone;           // the listed keys that are present
  std::vector<char> removed(n, 0);    // by slot
  for (size_t k : keys) {
    const auto it = d.slot_of.find(k);
    if (it == d.slot_of.end()) continue;
    gone.push_back(k);
    removed[it->second] = 1;
  }
  const size_t m = gone.size(), n1 = n - m;
  if (m == 0) return 0;
  // holes: the removed slots below the new count; movers: the surviving slots at or above it -- equally many, paired in ascending order
  std::vector<size_t> key_at(n);
  for (const auto& kv : d.slot_of) key_at[kv.second] = kv.first;
  std::vector<RemoveSlotRec> moves;
  for (size_t hole = 0, mover = n1; hole < n1; hole++) {
    if (!removed[hole]) continue;
    while (removed[mover]) mover++;   // (as many survivors in [n1, n) as holes in [0, n1))
    moves.push_back(RemoveSlotRec{(int)mover, (int)hole});
    mover++;
  }
  const size_t cap = remove_window_recs(p, sizeof(RemoveSlotRec));
  d.upload.ensure(std::max<size_t>(1, std::min(cap, moves.size()) * sizeof(RemoveSlotRec)));   // before the first kernel
  d.index_dirty = true;   // the next query publishes a new snapshot and pruned plan; queries begun earlier keep theirs
  d.rows_dirty = true;
  // the removed keys that stand at or above the new count leave no hole: nothing moves for them
  for (size_t k : gone)
    if (d.slot_of.find(k)->second >= n1) d.slot_of.erase(k);
  // window by window: the keys of the window's holes leave the map first, its movers are retargeted behind the launch and its
  // synchronisation -- a call that fails leaves no key that points at a slot whose move was not issued
  for (size_t a = 0; a < moves.size(); a += cap) {
    const size_t cnt = std::min(cap, moves.size() - a);
    if (cnt * planes > UPSERT_MAX_GROUP_PLANES) throw HipError("internal: a removal window larger than one dispatch");
    for (size_t k = a; k < a + cnt; k++) d.slot_of.erase(key_at[(size_t)moves[k].dst_slot]);
    h2d_sync(d.upload.p, moves.data() + a, cnt * sizeof(RemoveSlotRec));
    launch_sparse_move_slots(d.polys.p, reinterpret_cast<const RemoveSlotRec*>(d.upload.p), cnt, (int)planes, 0);
    HIP_CHECK(hipDeviceSynchronize());
    for (size_t k = a; k < a + cnt; k++) d.slot_of[key_at[(size_t)moves[k].src_slot]] = (size_t)moves[k].dst_slot;
  }
  return m;
}

// a dense handle: `all` are distinct and ascending.  Returns how many of them the shape holds (caller holds mu)
size_t remove_dense(sp_db& d, const std::vector<size_t>& all) {
  const Params& p = d.params->p;
  const size_t planes = p.planes(), np = p.num_per();
  // the held items by local row and column, ordered so that the items of one record -- a PACKED quad, a digit-planar cell -- are
  // neighbours: a window cuts the list anywhere, and a record cut in two is two records of two synchronised launches
  struct Held {
    size_t key;
    int jl, il;   // local row; local column (planar: the reference column)
  };
  std::vector<Held> held;
  const int G = d.num_shards, npg = (int)np / std::max(G, 1);
  for (size_t idx : all) {
    if (!dense_holds(d, idx)) continue;
    Held h;
    h.jl = (int)(idx / np) - d.j0;
    h.il = (int)((idx % np) / (size_t)d.col_G);
    if (d.planar_resident) {
      const size_t ic = (size_t)(h.il % G) * (size_t)npg + (size_t)(h.il / G);   // resident column (planar_resident.hpp)
      h.key = (((size_t)(h.jl >> 4) * np + ic) << 4) | (size_t)(h.jl & 15);
    } else if (d.packed) {
      h.key = (((size_t)(h.jl >> 1) * (size_t)d.np_local + (size_t)(h.il & ~1)) << 1) | (size_t)(((h.jl & 1) << 1) | (h.il & 1));
    } else {
      h.key = (size_t)h.jl * (size_t)d.np_local + (size_t)h.il;   // the local linear index itself
    }
    held.push_back(h);
  }
  if (held.empty()) return 0;
  std::sort(held.begin(), held.end(), [](const Held& x, const Held& y) { return x.key < y.key; });
  const bool patch = d.packed && !d.planar_resident && d.planar_state == 1 && d.planar;   // a PACKED handle's batch copy follows its items
  const size_t rec_bytes = d.planar_resident ? sizeof(RemoveCellRec) : d.packed ? sizeof(RemoveQuadRec) : sizeof(unsigned long long);
  const size_t cap = std::min(held.size(), remove_window_recs(p, rec_bytes + (patch ? sizeof(RemoveCellRec) : 0)));
  const size_t cells0 = round16(cap * rec_bytes);
  d.upload.ensure(cells0 + (patch ? cap * sizeof(RemoveCellRec) : 0));   // before the first kernel
  std::vector<uint8_t> host(cells0 + (patch ? cap * sizeof(RemoveCellRec) : 0));
  std::vector<unsigned long long> locals;
  std::vector<RemoveQuadRec> quads;
  std::vector<RemoveCellRec> cells;
  std::unordered_map<size_t, size_t> cell_at;   // (16-row group, column) -> its record in the window's cell list
  auto add_cell = [&](int jl, int ii) {
    const auto ins = cell_at.emplace((size_t)(jl >> 4) * np + (size_t)ii, cells.size());
    if (ins.second) cells.push_back(RemoveCellRec{jl & ~15, ii, 0u});
    cells[ins.first->second].mask |= 1u << (jl & 15);
  };
  for (size_t a = 0; a < held.size(); a += cap) {
    const size_t cnt = std::min(cap, held.size() - a);
    locals.clear();
    quads.clear();
    cells.clear();
    cell_at.clear();
    for (size_t k = a; k < a + cnt; k++) {
      const Held& h = held[k];
      if (d.planar_resident) {
        add_cell(h.jl, h.il);
      } else if (d.packed) {
        if (quads.empty() || quads.back().jp != (h.jl >> 1) || quads.back().q != (h.il >> 1)) quads.push_back(RemoveQuadRec{h.jl >> 1, h.il >> 1, 0u});
        quads.back().mask |= 1u << (((h.jl & 1) << 1) | (h.il & 1));
        if (patch) add_cell(h.jl, h.il);   // (a PACKED handle with a batch copy is unsharded: local = reference coordinates)
      } else {
        locals.push_back((unsigned long long)h.key);
      }
    }
    const void* recs = d.planar_resident ? (const void*)cells.data() : d.packed ? (const void*)quads.data() : (const void*)locals.data();
    const size_t n_recs = d.planar_resident ? cells.size() : d.packed ? quads.size() : locals.size();
    memcpy(host.data(), recs, n_recs * rec_bytes);
    size_t image = n_recs * rec_bytes;
    if (patch) {
      memcpy(host.data() + cells0, cells.data(), cells.size() * sizeof(RemoveCellRec));
      image = cells0 + cells.size() * sizeof(RemoveCellRec);
    }
    h2d_sync(d.upload.p, host.data(), image);
    if (d.planar_resident) {
      launch_planar_clear_items(planar_words(d), reinterpret_cast<const RemoveCellRec*>(d.upload.p), n_recs, d.np_local, d.nj, (int)planes,
                                planar_shape(d), 0);
    } else if (d.packed) {
      launch_items_clear_packed(d.words.p, reinterpret_cast<const RemoveQuadRec*>(d.upload.p), n_recs, d.np_local, d.nj, (int)planes, 0);
      if (patch)   // same stream: the copy's bytes of the same items
        launch_planar_clear_items(reinterpret_cast<unsigned char*>(d.planar->p), reinterpret_cast<const RemoveCellRec*>(d.upload.p + cells0),
                                  cells.size(), d.np_local, d.nj, (int)planes, PlanarShardShape{}, 0);
    } else {
      launch_items_clear_words8(d.words.p, reinterpret_cast<const unsigned long long*>(d.upload.p), n_recs, d.np_local, d.nj, (int)planes, 0);
    }
    HIP_CHECK(hipDeviceSynchronize());   // (the lists are reused by the next window)
  }
  return held.size();
}

// `idx` has been checked against num_items; deduplicated here, before anything is enqueued
size_t remove_many(sp_db& d, std::vector<size_t>& idx) {
  if (idx.empty()) return 0;
  check_device(d.device);
  std::sort(idx.begin(), idx.end());
  idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
  std::lock_guard<std::mutex> lk(d.mu);
  return d.sparse ? remove_sparse(d, idx) : remove_dense(d, idx);
}

}  // namespace

extern "C" {

int sp_db_remove_items(sp_db_t* d, const size_t* item_idx, size_t n, size_t* removed) {
  if (removed) *removed = 0;
  return guarded([&] {
    need(d != nullptr, "null db");
    need(item_idx || n == 0, "null argument");
    const size_t num_items = d->params->p.num_items();
    for (size_t i = 0; i < n; i++)   // every entry is checked before anything is written
      if (item_idx[i] >= num_items)
        throw ArgError("entry " + std::to_string(i) + ": item index " + std::to_string(item_idx[i]) + " out of range (num_items " +
                       std::to_string(num_items) + ")");
    std::vector<size_t> idx(item_idx, item_idx + n);
    const size_t m = remove_many(*d, idx);
    if (removed) *removed = m;
  });
}

int sp_db_remove_range(sp_db_t* d, size_t item0, size_t count, size_t* removed) {
  if (removed) *removed = 0;
  return guarded([&] {
    read_range_check(d, item0, count);
    std::vector<size_t> idx;
    if (d->sparse) {   // the keys of the range that are present, from whichever of the range and the key map is shorter
      std::lock_guard<std::mutex> lk(d->mu);
      if (count < d->slot_of.size()) {
        for (size_t i = item0; i < item0 + count; i++)
          if (d->slot_of.count(i)) idx.push_back(i);
      } else {
        for (const auto& kv : d->slot_of)
          if (kv.first >= item0 && kv.first - item0 < count) idx.push_back(kv.first);
      }
    } else {
      idx.resize(count);
      for (size_t i = 0; i < count; i++) idx[i] = item0 + i;
    }
    const size_t m = remove_many(*d, idx);
    if (removed) *removed = m;
  });
}

int sp_db_sparse_trim(sp_db_t* d, size_t* freed_bytes) {
  if (freed_bytes) *freed_bytes = 0;
  return guarded([&] {
    need(d != nullptr, "null db");
    need(d->sparse, "sp_db_sparse_trim takes a sparse bucket (sp_db_create_sparse, sp_db_create_sparse_shard)");
    check_device(d->device);
    std::lock_guard<std::mutex> lk(d->mu);
    // the capacity sparse_reserve would have chosen for the current count: doubling from 64
    const size_t count = d->slot_of.size();
    size_t cap = 64;
    while (cap < count) cap *= 2;
    if (cap >= d->slots_cap) return;   // nothing shrinks (a fresh handle has no store yet)
    const size_t poly_words = d->params->p.planes() * POLY_LEN, before = d->polys.bytes();
    DevBuf<u64> smaller(cap * poly_words);
    if (count) HIP_CHECK(hipMemcpy(smaller.p, d->polys.p, count * poly_words * 8, hipMemcpyDeviceToDevice));
    if (count && tunable("h2d_cache_sync", 0) != 0) launch_cache_sync(nullptr, 0);  // (as sparse_reserve)
    d->polys = std::move(smaller);
    d->slots_cap = cap;
    if (freed_bytes) *freed_bytes = before - d->polys.bytes();
  });
}

}  // extern "C"
