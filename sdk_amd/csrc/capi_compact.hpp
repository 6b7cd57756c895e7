// sp_pp_compact / sp_pp_expand / sp_pp_expand_into: a client's public parameters kept as the wire image on the device and expanded
// there on demand.  The host side: the layout of the handle (what sp_pp_deserialize lays out), the per-polynomial table of
// k_pp_raw_image, the per-(params, device) staging and stream (DeviceState::PpExpand), the launches after the raw image -- those of
// sp_pp_deserialize, on the expansion's stream.  Kernel: pp_raw_image.hpp.  Included by capi.cpp only.
#pragma once

namespace {

struct PpMat { size_t count, rows, cols; };

// the matrices in wire order and the handle's offsets, as sp_pp_deserialize computes them (client.rs:221-259)
std::vector<PpMat> pp_layout(const Params& p, sp_pp& pp) {
  std::vector<PpMat> mats;
  mats.push_back({p.n, p.n + 1, p.t_conv});
  size_t off = p.n * (p.n + 1) * p.t_conv;
  pp.off_packing = 0;
  if (p.expand_queries) {
    pp.off_left = off;
    mats.push_back({p.g(), 2, p.t_exp_left});
    off += p.g() * 2 * p.t_exp_left;
    pp.has_right = p.has_expansion_right_on_wire();
    if (pp.has_right) {
      pp.off_right = off;
      mats.push_back({p.stop_round() + 1, 2, p.t_exp_right});
      off += (p.stop_round() + 1) * 2 * p.t_exp_right;
    } else {
      pp.off_right = pp.off_left;
    }
    pp.off_conv = off;
    mats.push_back({1, 2, 2 * p.t_conv});
    off += 2 * 2 * p.t_conv;
  }
  pp.n_polys = off;
  return mats;
}

// table[poly] of k_pp_raw_image: row 0 of a matrix continues the keystream (kpos runs on over the matrices, a polynomial is 256
// blocks), the other rows continue the wire
std::vector<u64> pp_raw_table(const Params& p, const std::vector<PpMat>& mats, size_t n_polys) {
  std::vector<u64> t;
  t.reserve(n_polys);
  u64 kpos = 0, wpos = SEED_LENGTH / 8;
  for (const PpMat& m : mats)
    for (size_t i = 0; i < m.count; i++) {
      for (size_t c = 0; c < m.cols; c++, kpos += POLY_LEN) t.push_back(kpos);
      for (size_t r = 0; r < (m.rows - 1) * m.cols; r++, wpos += POLY_LEN) t.push_back(PP_RAW_WIRE | wpos);
    }
  need(wpos * 8 == p.setup_bytes() && t.size() == n_polys, "internal: pp layout mismatch");
  return t;
}

// the stream of the expansions, created with the first one; caller holds E.mu
hipStream_t pp_expand_stream(DeviceState::PpExpand& E) {
  if (!E.stream) HIP_CHECK(hipStreamCreateWithFlags(&E.stream, hipStreamNonBlocking));
  return E.stream;
}

// an expanded handle with every buffer allocated and nothing of a client in it: the offsets, `all`, `pack_cat`, `all_w` with its
// constants 0 | 1 -- written here, once per handle, never by an expansion
std::unique_ptr<sp_pp> pp_alloc_slot(const sp_params_t* h, int device) {
  const Params& p = h->p;
  auto pp = std::make_unique<sp_pp>();
  pp->params = h;
  pp->device = device;
  pp_layout(p, *pp);
  const size_t off = pp->n_polys;
  pp->all.alloc(off * 2 * POLY_LEN);
  pp->pack_cat.alloc((p.n + 1) * p.n * p.t_conv * 2 * POLY_LEN);
  if (p.expand_queries) {
    pp->all_w.alloc((off + 1) * 2 * POLY_LEN);
    std::vector<u32> zero_one(2 * POLY_LEN, 0u);
    for (size_t i = POLY_LEN; i < 2 * POLY_LEN; i++) zero_one[i] = 1u;
    h2d_sync(pp->all_w.p + off * 2 * POLY_LEN, zero_one.data(), zero_one.size() * sizeof(u32));
  }
  return pp;
}

// the expansion proper: raw image, forward transform, [W_0 | W_1 | ...] for pack, the wave-layout twin.  Everything is enqueued on the
// per-device stream and waited for there; the one staging buffer is why one expansion runs at a time.
void pp_expand_impl(const sp_ppc& c, sp_pp& slot) {
  check_device(c.device);
  const Params& p = c.params->p;
  DeviceState& D = const_cast<sp_params*>(c.params)->device_state();
  DeviceState::PpExpand& E = D.pp_expand;
  std::lock_guard<std::mutex> lk(E.mu);
  hipStream_t s = pp_expand_stream(E);
  const size_t off = slot.n_polys;
  if (E.table.n == 0) {   // once per (params, device), before the first kernel
    sp_pp shape;
    const std::vector<u64> t = pp_raw_table(p, pp_layout(p, shape), off);
    E.raw.alloc(off * POLY_LEN);
    E.table.alloc(t.size());
    upload_words(E.table.p, t.data(), t.size() * 8);
  }
  const PpRawDesc d{E.raw.p, reinterpret_cast<const u64*>(c.image.p), E.table.p, (u64)off * POLY_LEN, p.modulus,
                    (u64)(((unsigned __int128)1 << 64) / p.modulus)};
  launch_pp_raw_image(d, (int)off, s);
  FwdDesc f{E.raw.p, nullptr, slot.all.p, (int)off, 1, 1, 1, 64, 1, 0, 1};  // to_ntt_alloc (client.rs:244-247)
  launch_ntt_fwd(D.T, f, s);
  const size_t n = p.n, tc = p.t_conv;
  for (size_t rr = 0; rr < n + 1; rr++)
    for (size_t r = 0; r < n; r++)
      launch_copy_words(slot.pack_cat.p + (rr * n * tc + r * tc) * 2 * POLY_LEN,
                        slot.all.p + (slot.off_packing + r * (n + 1) * tc + rr * tc) * 2 * POLY_LEN, tc * 2 * POLY_LEN, s);
  if (p.expand_queries) launch_mats_to_wave(slot.all_w.p, slot.all.p, off * 2 * POLY_LEN, s);
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

sp_ppc_t* sp_pp_compact(const sp_params_t* h, const uint8_t* data, size_t len) {
  return guarded_handle([&] {
    need(h && data, "null argument");
    const Params& p = h->p;
    if (len != p.setup_bytes()) throw ArgError("public parameter length " + std::to_string(len) + " != setup_bytes " + std::to_string(p.setup_bytes()));
    DeviceState& D = const_cast<sp_params*>(h)->device_state();
    auto c = std::make_unique<sp_ppc>();
    c->params = h;
    c->device = D.device;
    c->image.alloc((len + 255) / 256 * 256);
    h2d_sync(c->image.p, data, len);
    return c;
  });
}
void sp_ppc_free(sp_ppc_t* c) { delete c; }
size_t sp_ppc_device_bytes(const sp_ppc_t* c) { return c ? c->image.bytes() : 0; }
size_t sp_pp_device_bytes(const sp_pp_t* pp) { return pp ? pp->all.bytes() + pp->pack_cat.bytes() + pp->all_w.bytes() : 0; }

// internal hook (not declared in the public header; the request layer's direct-upload slots): overwrite a compact handle's image
int sp_ppc_assign_(sp_ppc_t* c, const uint8_t* data, size_t len) {
  return guarded([&] {
    need(c && data, "null argument");
    need(len == c->params->p.setup_bytes(), "public parameter length != setup_bytes");
    check_device(c->device);
    h2d_sync(c->image.p, data, len);
  });
}

sp_pp_t* sp_pp_expand(const sp_ppc_t* c) {
  return guarded_handle([&] {
    need(c != nullptr, "null argument");
    check_device(c->device);
    auto pp = pp_alloc_slot(c->params, c->device);
    pp_expand_impl(*c, *pp);
    return pp;
  });
}

int sp_pp_expand_into(const sp_ppc_t* c, sp_pp_t* slot) {
  return guarded([&] {
    need(c && slot, "null argument");
    need(slot->params == c->params, "the slot was expanded for different params");
    need(slot->device == c->device, "the slot lives on another device");
    pp_expand_impl(*c, *slot);
  });
}

int sp_debug_chacha20_u64_device(const sp_params_t* h, const uint8_t seed[32], size_t first_word, uint64_t* out, size_t count) {
  return guarded([&] {
    need(h && seed && (out || count == 0), "null argument");
    need(first_word % 8 == 0, "first_word must be a multiple of 8 (one ChaCha block is 8 words)");
    if (count == 0) return;
    DeviceState& D = const_cast<sp_params*>(h)->device_state();
    const size_t polys = (count + POLY_LEN - 1) / POLY_LEN;
    std::vector<u64> t(polys);
    for (size_t i = 0; i < polys; i++) t[i] = (u64)first_word + (u64)i * POLY_LEN;
    // a diagnostic: its three buffers are the call's own, allocated before its one kernel
    DevBuf<u64> key(SEED_LENGTH / 8), table(polys), words(count);
    h2d_sync(key.p, seed, SEED_LENGTH);
    h2d_sync(table.p, t.data(), polys * 8);
    std::vector<u64> host(count);
    {
      std::lock_guard<std::mutex> lk(D.pp_expand.mu);
      hipStream_t s = pp_expand_stream(D.pp_expand);
      launch_pp_raw_image(PpRawDesc{words.p, key.p, table.p, (u64)count, 0, 0}, (int)polys, s);
      HIP_CHECK(hipMemcpyAsync(host.data(), words.p, count * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    memcpy(out, host.data(), count * 8);
  });
}

}  // extern "C"
