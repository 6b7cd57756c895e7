// sp_db_item_digests / sp_db_item_digests_ref_words: one pair of 64-bit sums per ITEM over the resident words, in reference coordinates
// (the definition is beside ItemDigestDesc in kernels.hpp).  The host side: the windows of whole rows a range is cut into, which kernel a
// handle's resident form takes, the call's share of the handle's read buffer, the pin on the batch copy.  Kernels: db_item_digest.hpp,
// db_item_digest_planar.hpp.  Included by capi.cpp only, after capi_readback.hpp (dense_holds) and capi_digest.hpp.
#pragma once

namespace {

// the pairs of items item0 .. item0 + count - 1 over planes plane0 .. plane0 + nplanes - 1 -> out[2 * count], present[count] (may be
// null); `copy` = the pinned batch copy or null (the handle's resident words).  The arguments have been checked, count and nplanes > 0.
// The read buffer holds [table: 16 bytes per item of a window | R | a sparse window's present flags | its slot list].
void item_digests_impl(const sp_db& d, uint64_t seed, int plane0, int nplanes, const DevBuf<u64>* copy, size_t item0, size_t count,
                       uint64_t* out, uint8_t* present) {
  check_device(d.device);
  const Params& p = d.params->p;
  const size_t np = p.num_per(), row_lo = item0 / np, row_end = (item0 + count - 1) / np + 1;
  // a sparse store is summed under ONE snapshot of its key map (host-only: `mu` is let go before any device work)
  std::vector<DigestSlotRec> slots;
  if (d.sparse) {
    {
      std::lock_guard<std::mutex> idx(const_cast<sp_db&>(d).mu);
      for (const auto& kv : d.slot_of)
        if (kv.first >= item0 && kv.first - item0 < count) slots.push_back(DigestSlotRec{(unsigned long long)kv.second, (unsigned long long)kv.first});
    }
    std::sort(slots.begin(), slots.end(), [](const DigestSlotRec& a, const DigestSlotRec& b) { return a.item < b.item; });
  }
  // windows of whole rows: the table of a window stays within db_load_window bytes (one row where that is smaller) and within the
  // 2^30 pairs launch_digest_keys zeroes
  const size_t max_win = (size_t)std::max<long>(1, tunable("db_load_window", (long)512 << 20));
  const size_t per_row = np * 16 + 16 + (d.sparse ? np * (1 + sizeof(DigestSlotRec)) : 0);
  const size_t win_rows = std::max<size_t>(1, std::min<size_t>({max_win > 64 ? (max_win - 64) / per_row : 0, ((size_t)1 << 29) / np + 1,
                                                                row_end - row_lo}));
  // everything the call allocates, before its first kernel (allocation rule)
  const size_t R0 = round16(win_rows * np * 16), pres0 = R0 + round16(2 * win_rows * 8);
  const size_t list0 = pres0 + (d.sparse ? round16(win_rows * np) : 0);
  const size_t total = list0 + std::max<size_t>(16, std::min(slots.size(), win_rows * np) * sizeof(DigestSlotRec));
  // the staging of the result: out and present are written only once the whole call has succeeded
  std::vector<uint64_t> pairs(2 * count, 0);
  std::vector<uint8_t> flags(count, 0);
  sp_db::ReadBack& rb = d.readback;
  std::lock_guard<std::mutex> lk(rb.mu);
  if (!rb.stream) HIP_CHECK(hipStreamCreateWithFlags(&rb.stream, hipStreamNonBlocking));
  rb.buf.ensure(total);
  hipStream_t s = rb.stream;
  ItemDigestDesc e{};
  e.table = reinterpret_cast<unsigned long long*>(rb.buf.p);
  u64* R = reinterpret_cast<u64*>(rb.buf.p + R0);
  uint8_t* pres_dev = rb.buf.p + pres0;
  DigestSlotRec* list_dev = reinterpret_cast<DigestSlotRec*>(rb.buf.p + list0);
  e.R = R;
  e.s[0] = digest_mix(seed);
  e.s[1] = digest_mix(seed + 1);
  e.plane0 = plane0;
  e.nplanes = nplanes;
  e.num_per = (int)np;
  e.nj = d.sparse ? 0 : d.nj;
  size_t slot_at = 0;   // (sparse) the first record of `slots` not yet consumed
  for (size_t ra = row_lo; ra < row_end; ra += win_rows) {
    const size_t rb_end = std::min(row_end, ra + win_rows);
    // the requested items of this window
    const size_t a = std::max(item0, ra * np), b = std::min(item0 + count, rb_end * np);
    if (d.sparse) {
      size_t n = 0;
      while (slot_at + n < slots.size() && slots[slot_at + n].item < b) n++;
      if (n == 0) continue;   // nothing of this window is stored: zeros, present 0, no device work
      const size_t items = (rb_end - ra) * np;
      launch_digest_keys(e.table, R, seed, (int)items, 0, 0, s);   // the window's table zeroed (a sparse store needs no key table)
      HIP_CHECK(hipMemsetAsync(pres_dev, 0, items, s));
      HIP_CHECK(hipMemcpyAsync(list_dev, slots.data() + slot_at, n * sizeof(DigestSlotRec), hipMemcpyHostToDevice, s));
      launch_item_digest_sparse(e, d.polys.p, (int)p.planes(), list_dev, n, (unsigned long long)(ra * np), pres_dev, s);
      HIP_CHECK(hipMemcpyAsync(pairs.data() + 2 * (a - item0), e.table + 2 * (a - ra * np), (b - a) * 16, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(flags.data() + (a - item0), pres_dev + (a - ra * np), b - a, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));   // (the window's parts are reused by the next one)
      slot_at += n;
      continue;
    }
    // the rows the handle holds clip the window
    const size_t lo = std::max(ra, (size_t)d.j0), hi = std::min(rb_end, (size_t)d.j0 + (size_t)d.nj);
    if (lo >= hi) continue;
    e.jl0 = (int)(lo - (size_t)d.j0);
    e.nrows = (int)(hi - lo);
    launch_digest_keys(e.table, R, seed, (int)((hi - lo) * np), (int)lo, e.nrows, s);
    if (copy)
      launch_item_digest_planar(e, reinterpret_cast<const unsigned char*>(copy->p), PlanarShardShape{}, s);
    else if (d.planar_resident)
      launch_item_digest_planar(e, reinterpret_cast<const unsigned char*>(d.words.p), planar_shape(d), s);
    else
      launch_item_digest_words(e, d.words.p, d.np_local, d.packed, d.colmap(), s);
    const size_t ca = std::max(a, lo * np), cb = std::min(b, hi * np);   // the requested items among the window's held rows
    if (ca < cb) HIP_CHECK(hipMemcpyAsync(pairs.data() + 2 * (ca - item0), e.table + 2 * (ca - lo * np), (cb - ca) * 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = ca; i < cb; i++) flags[i - item0] = dense_holds(d, i) ? 1 : 0;
  }
  memcpy(out, pairs.data(), pairs.size() * 8);
  if (present) memcpy(present, flags.data(), flags.size());
}

}  // namespace

extern "C" {

int sp_db_item_digests(const sp_db_t* d, uint64_t seed, int which, int plane0, int nplanes, size_t item0, size_t count, uint64_t* out,
                       uint8_t* present) {
  bool no_copy = false;
  const int rc = guarded([&] {
    read_range_check(d, item0, count);
    need(which == SP_DIGEST_RESIDENT || which == SP_DIGEST_BATCH_COPY, "unknown `which` (SP_DIGEST_RESIDENT, SP_DIGEST_BATCH_COPY)");
    const size_t planes = d->params->p.planes();
    need(plane0 >= 0 && nplanes >= 0 && (size_t)plane0 <= planes && (size_t)nplanes <= planes - (size_t)plane0, "plane range past the planes");
    if (count == 0 || nplanes == 0) return;   // SP_OK, nothing written
    need(out != nullptr, "null argument");
    // the batch copy is pinned as sp_db_digest pins it, and never built here
    std::shared_ptr<const DevBuf<u64>> pin;
    if (which == SP_DIGEST_BATCH_COPY) {
      {
        std::lock_guard<std::mutex> lk(const_cast<sp_db*>(d)->mu);
        if (!d->sparse && !d->planar_resident && d->planar_state == 1 && d->planar) pin = d->planar;
      }
      if (!pin) {
        no_copy = true;
        return;
      }
    }
    item_digests_impl(*d, seed, plane0, nplanes, pin.get(), item0, count, out, present);
  });
  if (rc == SP_OK && no_copy)
    return guarded_status(SP_E_STATE, "sp_db_item_digests: no valid digit-planar copy stands beside this database (sp_db_prepare_batch builds one beside a PACKED, unsharded database)");
  return rc;
}

int sp_db_item_digests_ref_words(const sp_params_t* h, uint64_t seed, int plane, int z0, int nz, const uint64_t* words, uint64_t* acc) {
  return guarded([&] {
    need(h != nullptr && acc != nullptr, "null argument");
    const Params& p = h->p;
    need(plane >= 0 && (size_t)plane < p.planes() && z0 >= 0 && nz >= 0 && z0 <= N && nz <= N - z0, "bad coordinates");
    if (nz == 0) return;
    need(words != nullptr, "null argument");
    const size_t num_per = p.num_per(), dim0 = p.dim0();
    std::vector<u64> R(dim0);
    for (int l = 0; l < 2; l++) {
      const u64 s = digest_mix(seed + (u64)l);
      for (size_t j = 0; j < dim0; j++) R[j] = digest_row_key(s, (u64)j);
      const uint64_t* w = words;
      for (int z = z0; z < z0 + nz; z++)
        for (size_t ii = 0; ii < num_per; ii++, w += dim0) {
          const u64 A = digest_col_key(s, ((u64)plane * N + (u64)z) * (u64)num_per + (u64)ii);
          for (size_t j = 0; j < dim0; j++)   // both limbs reduced as the loaders reduce them (canon_word)
            acc[2 * (j * num_per + ii) + (size_t)l] +=
                R[j] * (A * ((u64)((u32)w[j] % (u32)MODULUS_0) | ((u64)((u32)(w[j] >> 32) % (u32)MODULUS_1) << 32)));
        }
    }
  });
}

}  // extern "C"
