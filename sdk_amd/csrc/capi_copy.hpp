// sp_db_copy_items: items from one resident database into another on the device, word for word -- what dst.update_rows(src.export_rows())
// does through item bytes and the host, without the decode, the host copy and the second encode, and exact for every word (spill
// coefficients, synthetic words and arbitrary sp_db_load words included).  The host side: the windows of a range, what both handles
// hold, and the record lists the writers of db_copy.hpp / db_copy_planar.hpp / db_copy_sparse.hpp are driven by.  The staging words and
// the lists live in the SOURCE's read buffer (capi_readback.hpp).  Included by capi.cpp only, after capi_readback.hpp.
#pragma once

namespace {

// the read buffer's parts for windows of `cap` items: [16 bytes | records | patch cells | gathered words], each from a 16-byte boundary.
// An item costs at most one record of the largest kind (a digit-planar cell of its own; a quad, a slot and an entry of the 8-byte run
// list are smaller) and one patch cell of a PACKED destination's batch copy.
constexpr size_t COPY_REC_BYTES = sizeof(CopyCellRec);
static_assert(COPY_REC_BYTES >= sizeof(CopyQuadRec) && COPY_REC_BYTES >= sizeof(CopySlotRec) && COPY_REC_BYTES >= sizeof(int), "record budget");
struct CopyLayout {
  size_t recs0, cells0, words0, total;
};
size_t copy_item_bytes(const sp_db& src) {
  return COPY_REC_BYTES + sizeof(PlanarPatchCell) + (src.sparse ? 0 : src.params->p.planes() * POLY_LEN * 8);   // (a sparse store is read in place)
}
CopyLayout copy_layout(const sp_db& src, size_t cap) {
  CopyLayout l;
  l.recs0 = 16;
  l.cells0 = l.recs0 + round16(cap * COPY_REC_BYTES);
  l.words0 = l.cells0 + round16(cap * sizeof(PlanarPatchCell));
  l.total = l.words0 + cap * (copy_item_bytes(src) - COPY_REC_BYTES - sizeof(PlanarPatchCell));
  return l;
}
// items per window: the buffer stays within db_load_window bytes (one item where that is smaller) and every launch of the window within
// what one dispatch takes -- 2^32 - 1 WORK-ITEMS along x (blocks along x times the 256 of a workgroup), 65535 blocks along y and z.
// With n items and P planes, n * P <= UPSERT_MAX_GROUP_PLANES = 2^23 (a sparse source's windows reach it: an item costs them a record):
//   gathers and the 8-byte / PACKED / planar scatters: x <= ceil(n / 16) blocks, y = 2048 / 16 or / 32, z = P;
//   k_items_copy_slots: x = n blocks = n * 256 <= 2^31 work-items, y = 4 P (<= 65535: P <= 2^14 is far above any parameter set);
//   the patch launch behind a PACKED destination's batch copy (launch_planar_patch_items) puts everything on x: cells * P * 2^14
//   work-items, cells <= n -- so with a copy standing n * P <= COPY_PATCH_ITEM_PLANES = 2^17, which keeps it at 2^31.
constexpr size_t COPY_PATCH_ITEM_PLANES = (size_t)1 << 17;
size_t copy_window_items(const sp_db& src, bool patch) {
  const Params& p = src.params->p;
  const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));
  const size_t fit = max_win > 64 ? (max_win - 64) / copy_item_bytes(src) : 0;   // (64: the head and the parts' rounding)
  const size_t item_planes = patch ? COPY_PATCH_ITEM_PLANES : UPSERT_MAX_GROUP_PLANES;
  return std::max<size_t>(1, std::min<size_t>({fit, std::max<size_t>(1, item_planes / p.planes()), p.num_items()}));
}

// one item of a window: its index and where its words stand in the stage (a position of the gathered run, or the source's slot)
struct CopyItem {
  size_t idx;
  int stage;
};

// items item0 .. item0 + count - 1 that `src` holds and `dst`'s shape holds -> dst; returns how many.  The arguments have been checked.
size_t copy_items_impl(sp_db& dst, const sp_db& src, size_t item0, size_t count) {
  if (count == 0) return 0;
  check_device(src.device);
  const Params& p = src.params->p;
  const size_t planes = p.planes(), np = p.num_per();
  sp_db::ReadBack& rb = src.readback;
  std::lock_guard<std::mutex> turn(rb.mu);     // src: a reader's turn at its read buffer and stream
  std::lock_guard<std::mutex> write(dst.mu);   // dst: a writer (sp_db_update_items)
  // a sparse source is read under ONE snapshot of its key map; its lock is not held across device work
  std::vector<std::pair<size_t, size_t>> snap;   // (item, slot), by item
  if (src.sparse) {
    std::lock_guard<std::mutex> idx(const_cast<sp_db&>(src).mu);
    if (count < src.slot_of.size()) {
      for (size_t i = item0; i < item0 + count; i++) {
        const auto it = src.slot_of.find(i);
        if (it != src.slot_of.end()) snap.emplace_back(i, it->second);
      }
    } else {
      for (const auto& kv : src.slot_of)
        if (kv.first >= item0 && kv.first - item0 < count) snap.emplace_back(kv.first, kv.second);
      std::sort(snap.begin(), snap.end());
    }
  }
  // the items of the window [a, a + n) that both hold, in index order; for a dense source also the run [L0, L0 + nL) of its local linear
  // index from the first to the last of them (what the gather brings into the stage: stage position = local index - L0)
  size_t snap_at = 0;
  auto window_items = [&](size_t a, size_t n, std::vector<CopyItem>& items, size_t& L0, size_t& nL) {
    items.clear();
    L0 = nL = 0;
    if (src.sparse) {
      while (snap_at < snap.size() && snap[snap_at].first < a) snap_at++;
      for (; snap_at < snap.size() && snap[snap_at].first < a + n; snap_at++)
        if (dense_holds(dst, snap[snap_at].first)) items.push_back(CopyItem{snap[snap_at].first, (int)snap[snap_at].second});
      return;
    }
    const size_t lo = std::max(a, (size_t)src.j0 * np), hi = std::min(a + n, ((size_t)src.j0 + (size_t)src.nj) * np);
    for (size_t i = lo; i < hi; i++) {
      if (!dense_holds(src, i) || !dense_holds(dst, i)) continue;
      const size_t L = dense_local(src, i);
      if (items.empty()) L0 = L;
      items.push_back(CopyItem{i, (int)(L - L0)});
      nL = L - L0 + 1;
    }
  };
  const bool patch = !dst.sparse && !dst.planar_resident && dst.planar_state == 1;   // a PACKED destination's batch copy follows its items
  const size_t cap = copy_window_items(src, patch);
  std::vector<CopyItem> items;
  size_t L0 = 0, nL = 0;
  // everything the call allocates, before its first kernel (allocation rule): the buffer for the largest window,
  // and a sparse destination's store for every new key of the call.  The keys themselves enter the key map window by window, each
  // window's once its launch has been issued (below): a call that fails leaves no key whose slot was never written.
  const CopyLayout lay = copy_layout(src, cap);
  if (!rb.stream) HIP_CHECK(hipStreamCreateWithFlags(&rb.stream, hipStreamNonBlocking));
  rb.buf.ensure(lay.total);
  std::vector<char> dst_rows;   // a sparse destination's occupied first-dimension rows (a new one changes the pruned expansion plan)
  if (dst.sparse) {
    size_t fresh = 0;
    for (size_t a = item0; a < item0 + count; a += cap) {
      window_items(a, std::min(cap, item0 + count - a), items, L0, nL);
      for (const CopyItem& it : items) fresh += dst.slot_of.count(it.idx) == 0;
    }
    snap_at = 0;
    if (fresh) {
      sparse_reserve(dst, dst.slot_of.size() + fresh);
      dst_rows.assign(p.dim0(), 0);
      for (const auto& kv : dst.slot_of) dst_rows[kv.first / np] = 1;
    }
  }
  hipStream_t s = rb.stream;
  uint8_t* recs_dev = rb.buf.p + lay.recs0;
  PlanarPatchCell* cells_dev = reinterpret_cast<PlanarPatchCell*>(rb.buf.p + lay.cells0);
  u64* words_dev = reinterpret_cast<u64*>(rb.buf.p + lay.words0);
  std::vector<int> run;
  std::vector<CopyQuadRec> quads;
  std::vector<CopyCellRec> cells;
  std::vector<CopySlotRec> slots;
  std::vector<PlanarPatchCell> pcells;
  std::unordered_map<size_t, size_t> at;   // quad or cell key -> its record in the window's list
  std::unordered_map<size_t, char> seen;   // (16-row group, column) keys of the window's patch list
  size_t copied = 0;
  for (size_t a = item0; a < item0 + count; a += cap) {
    window_items(a, std::min(cap, item0 + count - a), items, L0, nL);
    if (items.empty()) continue;   // nothing of this window is in both: no device work
    const u64* stage = words_dev;
    if (src.sparse)
      stage = src.polys.p;
    else if (src.planar_resident)
      launch_planar_gather(words_dev, reinterpret_cast<const unsigned char*>(src.words.p), L0, nL, src.np_local, src.nj, (int)planes,
                           planar_shape(src), s);
    else
      launch_items_gather(words_dev, src.words.p, L0, nL, src.np_local, src.nj, (int)planes, src.packed, s);
    auto upload = [&](const void* host, size_t bytes) { HIP_CHECK(hipMemcpyAsync(recs_dev, host, bytes, hipMemcpyHostToDevice, s)); };
    at.clear();
    if (dst.sparse) {
      // an existing key is overwritten in its slot; the window's new keys take the next slots in index order, and enter the key map
      // only after the launch that writes those slots has been issued
      slots.clear();
      size_t next = dst.slot_of.size();
      for (const CopyItem& it : items) {
        const auto have = dst.slot_of.find(it.idx);
        slots.push_back(CopySlotRec{it.stage, (int)(have != dst.slot_of.end() ? have->second : next++)});
      }
      if (slots.size() * planes > UPSERT_MAX_GROUP_PLANES) throw HipError("internal: a copy window larger than one dispatch");
      upload(slots.data(), slots.size() * sizeof(CopySlotRec));
      launch_items_copy_slots(dst.polys.p, stage, reinterpret_cast<const CopySlotRec*>(recs_dev), slots.size(), (int)planes, s);
      if (next != dst.slot_of.size()) {
        for (size_t k = 0; k < items.size(); k++) {
          if (!dst.slot_of.emplace(items[k].idx, (size_t)slots[k].slot).second) continue;
          if (!dst_rows[items[k].idx / np]) dst.rows_dirty = true;
          dst_rows[items[k].idx / np] = 1;
        }
        dst.index_dirty = true;
      }
    } else if (dst.planar_resident) {
      // a cell = (16-row group, reference column), listed once; sorted into the resident order of the columns [chunk][g][e][n], so
      // that neighbours of the list are neighbours of an operand
      cells.clear();
      for (const CopyItem& it : items) {
        const int jl = (int)(it.idx / np) - dst.j0, ii = (int)(it.idx % np);
        const auto ins = at.emplace((size_t)(jl >> 4) * np + (size_t)ii, cells.size());
        if (ins.second) {
          CopyCellRec c;
          c.j = jl & ~15;
          c.ii = ii;
          for (int t = 0; t < 16; t++) c.src[t] = -1;
          cells.push_back(c);
        }
        cells[ins.first->second].src[jl & 15] = it.stage;
      }
      const int G = dst.num_shards, npg = (int)np / G;
      auto order = [&](const CopyCellRec& c) {
        const size_t ic = (size_t)(c.ii % G) * (size_t)npg + (size_t)(c.ii / G);   // resident column (planar_resident.hpp)
        return ((size_t)(c.j >> 4) * np) + ((ic >> 5) << 5) + ((ic & 1) << 4) + ((ic >> 1) & 15);
      };
      std::sort(cells.begin(), cells.end(), [&](const CopyCellRec& x, const CopyCellRec& y) { return order(x) < order(y); });
      upload(cells.data(), cells.size() * sizeof(CopyCellRec));
      launch_planar_scatter_items(planar_words(dst), stage, reinterpret_cast<const CopyCellRec*>(recs_dev), cells.size(), dst.np_local, dst.nj,
                                  (int)planes, planar_shape(dst), s);
    } else if (dst.packed) {
      // a quad = (local row pair, local column pair), listed once with every item of it that this window writes; the patch list names
      // each touched (16-row group, column) once, as sp_db_update_items does
      quads.clear();
      pcells.clear();
      seen.clear();
      const size_t npq = (size_t)dst.np_local / 2;
      for (const CopyItem& it : items) {
        const size_t L = dense_local(dst, it.idx);
        const int jl = (int)(L / (size_t)dst.np_local), il = (int)(L % (size_t)dst.np_local);
        const auto ins = at.emplace((size_t)(jl / 2) * npq + (size_t)(il / 2), quads.size());
        if (ins.second) quads.push_back(CopyQuadRec{jl / 2, il / 2, {-1, -1, -1, -1}});
        quads[ins.first->second].src[(jl & 1) * 2 + (il & 1)] = it.stage;
        if (patch && seen.emplace((size_t)(jl >> 4) * (size_t)dst.np_local + (size_t)il, 1).second) pcells.push_back(PlanarPatchCell{jl, il});
      }
      upload(quads.data(), quads.size() * sizeof(CopyQuadRec));
      if (!pcells.empty()) HIP_CHECK(hipMemcpyAsync(cells_dev, pcells.data(), pcells.size() * sizeof(PlanarPatchCell), hipMemcpyHostToDevice, s));
      launch_items_scatter_packed(dst.words.p, stage, reinterpret_cast<const CopyQuadRec*>(recs_dev), quads.size(), dst.np_local, dst.nj,
                                  (int)planes, s);
      if (!pcells.empty())   // same stream, after the scatter
        launch_planar_patch_items(reinterpret_cast<unsigned char*>(dst.planar->p), dst.words.p, (int)planes, dst.np_local, dst.nj, cells_dev,
                                  pcells.size(), s);
    } else {
      // 8-byte words: the written items are a run of the destination's local linear index
      const size_t D0 = dense_local(dst, items.front().idx), nD = dense_local(dst, items.back().idx) - D0 + 1;
      run.assign(nD, -1);
      for (const CopyItem& it : items) run[dense_local(dst, it.idx) - D0] = it.stage;
      upload(run.data(), run.size() * sizeof(int));
      launch_items_scatter_words8(dst.words.p, stage, reinterpret_cast<const int*>(recs_dev), D0, nD, dst.np_local, dst.nj, (int)planes, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));   // (the lists and the stage are reused by the next window)
    copied += items.size();
  }
  return copied;
}

}  // namespace

extern "C" {

int sp_db_copy_items(sp_db_t* dst, const sp_db_t* src, size_t item0, size_t count, size_t* copied) {
  if (copied) *copied = 0;
  return guarded([&] {
    need(dst && src, "null db");
    need(dst != src, "sp_db_copy_items: dst and src are one handle");
    need(dst->params == src->params, "sp_db_copy_items: the handles were made from different params handles");
    need(dst->device == src->device, "sp_db_copy_items: the handles live on different devices (copies across devices are out of scope)");
    read_range_check(src, item0, count);
    const size_t n = copy_items_impl(*dst, *src, item0, count);
    if (copied) *copied = n;
  });
}

// internal hook of sp_server_replace_db (endpoint.cpp sees handles through the public header only): may a server of `params` that
// serves `cur` switch to `next`?  The same params handle and device, and unsharded
int sp_db_can_replace_(const sp_params_t* params, const sp_db_t* cur, const sp_db_t* next) {
  return params && cur && next && next->params == params && next->device == cur->device && next->num_shards == 1 && next->col_G == 1;
}

}  // extern "C"
