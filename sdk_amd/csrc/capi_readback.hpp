// sp_db_read_items / sp_db_export_rows: items back out of a resident database, on every format -- the inverse of sp_db_load_items and
// the upserts (server.rs:277-357 load_item_from_seek / load_db_from_seek; lib/server/src/db/loading.rs:278-359 update_item_raw).
// The host side: which items a handle holds, the windows of a range, the handle's read buffer.  Kernels: item_readback.hpp, and
// k_planar_gather of planar_resident.hpp.  Included by capi.cpp only (it uses that file's encoder helpers).
#pragma once

namespace {

// does this handle hold item `idx`, by its shape alone?  (a dense database holds all-zero items too; a sparse bucket: and is it stored)
bool dense_holds(const sp_db& d, size_t idx) {
  const size_t np = d.params->p.num_per(), j = idx / np, ii = idx % np;
  return j >= (size_t)d.j0 && j < (size_t)d.j0 + (size_t)d.nj && (int)(ii % (size_t)d.col_G) == d.col_g;
}
// the handle's local linear index of an item it holds: local row * local columns + local column
size_t dense_local(const sp_db& d, size_t idx) {
  const size_t np = d.params->p.num_per();
  return (idx / np - (size_t)d.j0) * (size_t)d.np_local + (idx % np) / (size_t)d.col_G;
}

// the read buffer's parts for windows of `cap` items: [counter: 16 bytes | list | bytes | words], each from a 16-byte boundary
struct ReadLayout {
  size_t list0, bytes0, words0, total;
};
ReadLayout read_layout(const sp_db& d, size_t cap) {
  const Params& p = d.params->p;
  ReadLayout l;
  l.list0 = 16;
  l.bytes0 = l.list0 + round16(cap * sizeof(ItemDecodeRec));
  l.words0 = l.bytes0 + round16(cap * p.db_item_size);
  l.total = l.words0 + (d.sparse ? 0 : cap * p.planes() * POLY_LEN * 8);   // (a sparse bucket's store is decoded in place)
  return l;
}
// items per window: the read buffer stays within db_load_window bytes (one item where that is smaller) and a decode launch within the
// grid (UPSERT_MAX_GROUP_PLANES, as the bulk upserts)
size_t read_window_items(const sp_db& d) {
  const Params& p = d.params->p;
  const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));
  const size_t per_item = sizeof(ItemDecodeRec) + p.db_item_size + (d.sparse ? 0 : p.planes() * POLY_LEN * 8);
  const size_t fit = max_win > 64 ? (max_win - 64) / per_item : 0;   // (64: the counter and the parts' rounding)
  return std::max<size_t>(1, std::min<size_t>({fit, std::max<size_t>(1, UPSERT_MAX_GROUP_PLANES / p.planes()), p.num_items()}));
}

void read_range_check(const sp_db_t* d, size_t item0, size_t count) {
  need(d != nullptr, "null db");
  const Params& p = d->params->p;
  need(item0 <= p.num_items() && count <= p.num_items() - item0, "item range past num_items");
}

// items item0 .. item0 + count - 1 -> out (count * db_item_size bytes), present (count bytes, may be null); returns the undecodable
// chunk polynomials among the held items.  The range has been checked.
size_t read_items_impl(const sp_db& d, size_t item0, size_t count, uint8_t* out, uint8_t* present) {
  if (count == 0) return 0;
  check_device(d.device);
  sp_params* h = const_cast<sp_params*>(d.params);
  const Params& p = h->p;
  DeviceState& D = h->device_state();
  const size_t logp = pt_bits(p), planes = p.planes(), bpc = chunk_bytes(p), isz = p.db_item_size;
  need((bpc * 8 + logp - 1) / logp <= POLY_LEN, "item chunk does not fit one polynomial (server.rs:292)");
  need(logp >= 1 && logp <= 28, "plaintext modulus out of range");
  sp_db::ReadBack& rb = d.readback;
  std::lock_guard<std::mutex> lk(rb.mu);
  const size_t cap = read_window_items(d);
  // everything the call allocates, before its first kernel (allocation rule): the buffer takes the largest
  // window's size on the first call, whatever that call reads, and grows again only when db_load_window has been raised since
  const ReadLayout L = read_layout(d, cap);
  if (!rb.stream) HIP_CHECK(hipStreamCreateWithFlags(&rb.stream, hipStreamNonBlocking));
  rb.buf.ensure(L.total);
  hipStream_t s = rb.stream;
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(rb.buf.p);
  ItemDecodeRec* list_dev = reinterpret_cast<ItemDecodeRec*>(rb.buf.p + L.list0);
  uint8_t* bytes_dev = rb.buf.p + L.bytes0;
  u64* words_dev = reinterpret_cast<u64*>(rb.buf.p + L.words0);
  HIP_CHECK(hipMemsetAsync(counter, 0, 16, s));
  std::vector<ItemDecodeRec> list;
  for (size_t a = item0; a < item0 + count; a += cap) {
    const size_t n = std::min(cap, item0 + count - a);
    list.clear();
    size_t L0 = 0;
    if (d.sparse) {
      std::lock_guard<std::mutex> idx(const_cast<sp_db&>(d).mu);   // host-only: the key map (writers are excluded by the caller)
      for (size_t i = a; i < a + n; i++) {
        const auto it = d.slot_of.find(i);
        if (it != d.slot_of.end()) list.push_back(ItemDecodeRec{(int)it->second, (int)(i - a)});
      }
    } else {
      // the rows the handle holds clip the window; within them the held items are a run of its local linear index
      const size_t np = p.num_per();
      const size_t lo = std::max(a, (size_t)d.j0 * np), hi = std::min(a + n, ((size_t)d.j0 + (size_t)d.nj) * np);
      for (size_t i = lo; i < hi; i++) {
        if (!dense_holds(d, i)) continue;
        if (list.empty()) L0 = dense_local(d, i);
        list.push_back(ItemDecodeRec{(int)list.size(), (int)(i - a)});
      }
    }
    uint8_t* dst = out + (a - item0) * isz;
    if (present) {
      memset(present + (a - item0), 0, n);
      for (const ItemDecodeRec& r : list) present[a - item0 + (size_t)r.pos] = 1;
    }
    if (list.empty()) {   // nothing of this window is held: zeros, no device work
      memset(dst, 0, n * isz);
      continue;
    }
    HIP_CHECK(hipMemsetAsync(bytes_dev, 0, n * isz, s));
    HIP_CHECK(hipMemcpyAsync(list_dev, list.data(), list.size() * sizeof(ItemDecodeRec), hipMemcpyHostToDevice, s));
    ItemDecodeDesc e{};
    if (d.sparse) {
      e.src = d.polys.p;
    } else {
      if (d.planar_resident)
        launch_planar_gather(words_dev, reinterpret_cast<const unsigned char*>(d.words.p), L0, list.size(), d.np_local, d.nj, (int)planes,
                             planar_shape(d), s);
      else
        launch_items_gather(words_dev, d.words.p, L0, list.size(), d.np_local, d.nj, (int)planes, d.packed, s);
      e.src = words_dev;
    }
    e.list = list_dev;
    e.out = bytes_dev;
    e.undecodable = counter;
    e.planes = (int)planes;
    e.db_item_size = (int)isz;
    e.bytes_per_chunk = (int)bpc;
    e.logp = (int)logp;
    e.pt_modulus = (u32)p.pt_modulus;
    launch_items_decode(D.T, e, list.size(), s);
    HIP_CHECK(hipMemcpyAsync(dst, bytes_dev, n * isz, hipMemcpyDeviceToHost, s));   // the window's bytes, once
    HIP_CHECK(hipStreamSynchronize(s));   // (`list` and the window are reused by the next one)
  }
  unsigned long long undec = 0;
  HIP_CHECK(hipMemcpyAsync(&undec, counter, sizeof undec, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return (size_t)undec;
}

}  // namespace

extern "C" {

int sp_db_read_items(const sp_db_t* d, size_t item0, size_t count, uint8_t* out, size_t out_cap, uint8_t* present, size_t* undecodable) {
  return guarded([&] {
    read_range_check(d, item0, count);
    const size_t isz = d->params->p.db_item_size;
    need(out_cap / std::max<size_t>(isz, 1) >= count, "out_cap < count * db_item_size");
    if (count == 0) return;   // SP_OK, nothing written
    need(out != nullptr, "null argument");
    const size_t undec = read_items_impl(*d, item0, count, out, present);
    if (undecodable) *undecodable = undec;
  });
}

size_t sp_db_export_rows_bound(const sp_db_t* d, size_t count) { return d ? count * (8 + d->params->p.db_item_size) : 0; }

int sp_db_export_rows(const sp_db_t* d, size_t item0, size_t count, uint8_t* body, size_t body_cap, size_t* body_len, size_t* records) {
  if (body_len) *body_len = 0;
  if (records) *records = 0;
  bool undecodable = false;
  const int rc = guarded([&] {
    read_range_check(d, item0, count);
    if (count == 0) return;
    const Params& p = d->params->p;
    const size_t isz = p.db_item_size, rec_bytes = 8 + isz;
    need(4 + isz <= 0xffffffffull, "db_item_size does not fit a record's be32 length");
    // the records the range yields, from the handle's shape and key map alone: the buffer is checked before any device work
    size_t held = 0;
    if (d->sparse) {
      std::lock_guard<std::mutex> idx(const_cast<sp_db*>(d)->mu);
      for (size_t i = item0; i < item0 + count; i++) held += d->slot_of.count(i);
    } else {
      for (size_t i = item0; i < item0 + count; i++) held += dense_holds(*d, i);
    }
    need(body != nullptr || held == 0, "null argument");
    need(body_cap / rec_bytes >= held, "body_cap is smaller than the records of the range (sp_db_export_rows_bound)");
    auto be32 = [](uint8_t* at, size_t v) {
      at[0] = (uint8_t)(v >> 24);
      at[1] = (uint8_t)(v >> 16);
      at[2] = (uint8_t)(v >> 8);
      at[3] = (uint8_t)v;
    };
    // pieces of at most 64 MiB of item bytes on the host
    const size_t piece = std::max<size_t>(1, ((size_t)64 << 20) / std::max<size_t>(isz, 1));
    std::vector<uint8_t> items(std::min(piece, count) * isz), present(std::min(piece, count));
    size_t off = 0, n_rec = 0;
    for (size_t a = item0; a < item0 + count; a += piece) {
      const size_t n = std::min(piece, item0 + count - a);
      if (read_items_impl(*d, a, n, items.data(), present.data()) != 0) {
        undecodable = true;
        return;
      }
      for (size_t k = 0; k < n; k++) {
        if (!present[k]) continue;
        be32(body + off, 4 + isz);
        be32(body + off + 4, a + k);
        memcpy(body + off + 8, items.data() + k * isz, isz);
        off += rec_bytes;
        n_rec++;
      }
    }
    if (body_len) *body_len = off;
    if (records) *records = n_rec;
  });
  if (rc == SP_OK && undecodable)
    return guarded_status(SP_E_STATE, "sp_db_export_rows: the range holds words that are no item's (undecodable polynomials, see sp_db_read_items): nothing exported");
  return rc;
}

}  // extern "C"
