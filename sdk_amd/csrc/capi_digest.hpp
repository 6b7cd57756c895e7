// sp_db_digest / sp_db_digest_ref_words: one pair of 64-bit sums per plane over the resident words, in reference coordinates (the
// definition is beside DigestDesc in kernels.hpp).  The host side: which kernel a handle's resident form takes, the call's share of the
// handle's read buffer, the pin on the batch copy.  Kernels: db_digest.hpp, db_digest_planar.hpp.  Included by capi.cpp only.
#pragma once

namespace {

// the digest of planes plane0 .. plane0 + nplanes - 1 -> out[2 * nplanes]; `copy` = the pinned batch copy (SP_DIGEST_BATCH_COPY) or null
// (the handle's resident words).  The arguments have been checked.  The read buffer holds [sums | R | a sparse store's slot list].
void digest_impl(const sp_db& d, uint64_t seed, int plane0, int nplanes, const DevBuf<u64>* copy, uint64_t* out) {
  check_device(d.device);
  const Params& p = d.params->p;
  // a sparse store is summed under ONE snapshot of its key map (host-only: `mu` is let go before any device work)
  std::vector<DigestSlotRec> slots;
  if (d.sparse) {
    std::lock_guard<std::mutex> idx(const_cast<sp_db&>(d).mu);
    slots.reserve(d.slot_of.size());
    for (const auto& kv : d.slot_of) slots.push_back(DigestSlotRec{(unsigned long long)kv.second, (unsigned long long)kv.first});
  }
  const int nj = d.sparse ? 0 : d.nj;
  sp_db::ReadBack& rb = d.readback;
  std::lock_guard<std::mutex> lk(rb.mu);
  // everything the call allocates, before its first kernel (allocation rule)
  const size_t R0 = round16((size_t)2 * nplanes * 8), list0 = R0 + round16((size_t)2 * nj * 8);
  if (!rb.stream) HIP_CHECK(hipStreamCreateWithFlags(&rb.stream, hipStreamNonBlocking));
  rb.buf.ensure(list0 + std::max<size_t>(16, slots.size() * sizeof(DigestSlotRec)));
  hipStream_t s = rb.stream;
  DigestDesc e{};
  e.sums = reinterpret_cast<unsigned long long*>(rb.buf.p);
  u64* R = reinterpret_cast<u64*>(rb.buf.p + R0);
  e.R = R;
  e.s[0] = digest_mix(seed);
  e.s[1] = digest_mix(seed + 1);
  e.plane0 = plane0;
  e.nplanes = nplanes;
  e.num_per = (int)p.num_per();
  e.nj = nj;
  launch_digest_keys(e.sums, R, seed, nplanes, d.j0, nj, s);
  if (d.sparse) {
    if (!slots.empty()) {
      DigestSlotRec* list = reinterpret_cast<DigestSlotRec*>(rb.buf.p + list0);
      HIP_CHECK(hipMemcpyAsync(list, slots.data(), slots.size() * sizeof(DigestSlotRec), hipMemcpyHostToDevice, s));
      launch_digest_sparse(e, d.polys.p, (int)p.planes(), list, slots.size(), s);
    }
  } else if (copy) {
    launch_digest_planar(e, reinterpret_cast<const unsigned char*>(copy->p), PlanarShardShape{}, s);
  } else if (d.planar_resident) {
    launch_digest_planar(e, reinterpret_cast<const unsigned char*>(d.words.p), planar_shape(d), s);
  } else {
    launch_digest_words(e, d.words.p, d.np_local, d.packed, d.colmap(), s);
  }
  std::vector<uint64_t> sums((size_t)2 * nplanes);
  HIP_CHECK(hipMemcpyAsync(sums.data(), e.sums, sums.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  memcpy(out, sums.data(), sums.size() * 8);   // (written only once the whole call has succeeded)
}

}  // namespace

extern "C" {

int sp_db_digest(const sp_db_t* d, uint64_t seed, int which, int plane0, int nplanes, uint64_t* out) {
  bool no_copy = false;
  const int rc = guarded([&] {
    need(d != nullptr, "null db");
    need(which == SP_DIGEST_RESIDENT || which == SP_DIGEST_BATCH_COPY, "unknown `which` (SP_DIGEST_RESIDENT, SP_DIGEST_BATCH_COPY)");
    const size_t planes = d->params->p.planes();
    need(plane0 >= 0 && nplanes >= 0 && (size_t)plane0 <= planes && (size_t)nplanes <= planes - (size_t)plane0, "plane range past the planes");
    if (nplanes == 0) return;   // SP_OK, nothing written
    need(out != nullptr, "null argument");
    // the batch copy is PINNED as a pass pins it (the shared_ptr, taken under `mu`): a concurrent drop cannot free it under the kernel.
    // Never built here: the digest speaks for the copy that stands.
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
    digest_impl(*d, seed, plane0, nplanes, pin.get(), out);
  });
  if (rc == SP_OK && no_copy)
    return guarded_status(SP_E_STATE, "sp_db_digest: no valid digit-planar copy stands beside this database (sp_db_prepare_batch builds one beside a PACKED, unsharded database)");
  return rc;
}

int sp_db_digest_ref_words(const sp_params_t* h, uint64_t seed, int plane, int z0, int nz, const uint64_t* words, uint64_t acc[2]) {
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
      u64 sum = 0;
      const uint64_t* w = words;
      for (int z = z0; z < z0 + nz; z++)
        for (size_t ii = 0; ii < num_per; ii++, w += dim0) {
          u64 col = 0;
          for (size_t j = 0; j < dim0; j++)   // both limbs reduced as the loaders reduce them (canon_word)
            col += R[j] * ((u64)((u32)w[j] % (u32)MODULUS_0) | ((u64)((u32)(w[j] >> 32) % (u32)MODULUS_1) << 32));
          sum += digest_col_key(s, ((u64)plane * N + (u64)z) * (u64)num_per + (u64)ii) * col;
        }
      acc[l] += sum;
    }
  });
}

}  // extern "C"
