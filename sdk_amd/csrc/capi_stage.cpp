// Stage-level exports of libspiral_hip.so (one stage of the answer path on host operands) and its sp_bench_* / sp_debug_* entry points.
#include "capi_internal.hpp"

using namespace spiral;

namespace {

// host u64 NTT words -> device u32
void upload_ntt(Workspace& W, const uint64_t* host, size_t words, DevBuf<u32>& dst, DevBuf<u64>& tmp) {
  tmp.ensure(words);
  dst.ensure(words);
  HIP_CHECK(hipMemcpyAsync(tmp.p, host, words * 8, hipMemcpyHostToDevice, W.stream));
  launch_u64_to_u32(dst.p, tmp.p, (long)words, W.stream);
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

// A dense operand [level][r][2 t_gsw] (polynomials) and one half of the workspace's interleaved rows of fold_mats,
// [level][r][ G - C | C ]: the left (0) or right (1) half of `levels` levels copied into the rows or out of them, on the stream.
enum MatsCopy { TO_MATS, FROM_MATS };
void copy_mats_half(Workspace& W, MatsCopy dir, int half, size_t levels, u32* dense) {
  const size_t row = 2 * W.P->t_gsw * 2 * POLY_LEN;   // words of one dense row
  for (size_t k = 0; k < levels * 2; k++) {
    u32 *m = W.fold_mats.p + (k * 2 + half) * row, *d = dense + k * row;
    HIP_CHECK(hipMemcpyAsync(dir == TO_MATS ? m : d, dir == TO_MATS ? d : m, row * sizeof(u32), hipMemcpyDeviceToDevice, W.stream));
  }
}
size_t mats_half_words(const Params& p, size_t levels) { return levels * 2 * 2 * p.t_gsw * 2 * POLY_LEN; }

// What both fold exports do around their own part: the checks, a workspace grown for `num_per` ciphertexts, v_folding in the right
// halves of fold_mats; `prepare(W, further, left, tmp)` fills the left halves -- staging an operand of its own, if it has one, in
// `left` / `tmp`, which live until the stream has been waited for -- and says how to fold; the result replaces cts[0].
template <typename F>
void stage_fold(const sp_params_t* h, uint64_t* cts, size_t num_per, const uint64_t* v_folding, F&& prepare) {
  need(num_per >= 1 && (num_per & (num_per - 1)) == 0, "num_per must be a power of two");
  size_t further = 0;
  while (((size_t)1 << further) < num_per) further++;
  if (further == 0) return;
  Scoped W(h);
  ensure_stage_fold(*W, num_per, further);
  DevBuf<u64> tmp, tmp2;
  DevBuf<u32> dF, left;
  upload_ntt(*W, v_folding, mats_half_words(h->p, further), dF, tmp);
  copy_mats_half(*W, TO_MATS, 1, further, dF.p);
  const FoldOpts o = prepare(*W, further, left, tmp2);
  HIP_CHECK(hipMemcpyAsync(W->foldX.p, cts, num_per * 2 * POLY_LEN * 8, hipMemcpyHostToDevice, W->stream));
  u64* res = run_fold(*W, o, W->foldX.p, W->foldY.p, 1, (int)num_per, -1);
  download_raw(*W, res, 2 * POLY_LEN, cts);
}

}  // namespace

extern "C" {

int sp_bench_sweep(sp_query_t* q, const sp_db_t* db, int iters, float* ms_per_launch) {
  return sp_bench_sweep_ex(q, db, iters, -1, ms_per_launch);
}

int sp_bench_sweep_ex(sp_query_t* q, const sp_db_t* db, int iters, int per_plane_launches, float* ms_per_launch) {
  return guarded([&] {
    need(q && db && ms_per_launch && iters > 0, "bad argument");
    refuse_planar_resident(db, "sp_bench_sweep");
    need(q->state >= 1, "query not begun");
    check_device(db->device);
    Workspace& W = *q->ws;
    // the same launches process_query issues for this database (one per plane when the sweep is pipelined)
    const Params& p = q->params->p;
    const bool per_plane = per_plane_launches < 0 ? sweep_is_pipelined(p, *db) : per_plane_launches != 0;
    need(!per_plane || db->col_G == 1, "per-plane launches need a row-sharded or unsharded db");
    auto sweep_once = [&] {
      if (!per_plane) return run_sweep(W, *db);
      W.ensure_sweep();
      for (size_t pl = 0; pl < p.planes(); pl++) launch_plane_sweep(W, *db, pl);
    };
    *ms_per_launch = timed_reps(W.stream, iters, sweep_once, per_plane ? (float)p.planes() : 1.0f);
  });
}

int sp_bench_sweep_batch(sp_query_t* const* qs, int batch, const sp_db_t* db, int iters, float* ms_per_pass) {
  return guarded([&] {
    if (qs && db && db->sparse) {   // a sparse bucket: the group's one pass (k_sweep_sparse_batch), 1 .. 8 queries begun for this bucket
      need(ms_per_pass && iters > 0 && batch >= 1 && batch <= SPARSE_GROUP_MAX, "bad argument");
      check_device(db->device);
      for (int i = 0; i < batch; i++) {
        need(qs[i] && qs[i]->state >= 1, "query not begun");
        need(qs[i]->params == db->params, "query and db were created for different params");
        qs[i]->ws->ensure_sweep();
        HIP_CHECK(hipStreamSynchronize(qs[i]->ws->stream));   // expansions done: the pass is timed alone
        HIP_CHECK(hipStreamSynchronize(qs[i]->ws->stream2));
      }
      hipStream_t s = qs[0]->ws->stream;
      *ms_per_pass = timed_reps(s, iters, [&] { sparse_group_pass(*db, qs, batch, s); });
      return;
    }
    const int group_max = !db ? 0 : db->planar_resident ? planar_resident_group_max(db->nj) : sweep_batch_group_max(db->np_local, db->nj);
    need(qs && db && ms_per_pass && iters > 0 && batch >= 1 && batch <= group_max, "bad argument");
    // ... or an unsharded narrow one (8-byte words, 2 <= num_per <= 64) for 2 .. 8 queries: the group's one pass, k_sweep_narrow_batch
    // (a single query is never a group there: it is refused as on every other 8-byte database)
    const bool narrow = !db->packed && db->num_shards == 1 && db->col_G == 1 && batch >= 2 && sweep_narrow_batch_shape_ok(db->np_local, db->nj);
    need(narrow || (db->planar_resident && db->num_shards == 1) || (db->packed && db->num_shards == 1 && db->col_G == 1),
         "the batched pass needs an unsharded PACKED database");
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
    PlanarPin pin;   // held for the whole call: on every path out the pass's stream is synchronised (timed_reps) before it is released
    SweepBatchDesc d = group_pass(*db, qs, batch, true, pin);
    *ms_per_pass = timed_reps(W0.stream, iters, [&] { group_pass_launch(*db, W0.D->T, d, W0.stream); });
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
    if (db->sparse) {
      // a sparse row shard, members of one snapshot: the scatter-form kernels (one query: k_sweep_sparse_scatter, every plane in one
      // launch; 2 .. 8: k_sweep_sparse_scatter_batch) or, layout 0, the plain-layout kernels over the same items (comparison only)
      Workspace* Ws[SPARSE_GROUP_MAX];
      for (int i = 0; i < batch; i++) {
        need(qs[i]->sparse_index == qs[0]->sparse_index, "the queries of a sparse bucket's group must have been begun on one snapshot of its index");
        qs[i]->ws->ensure_sweep();
        Ws[i] = qs[i]->ws.get();
      }
      const sp_db::SparseIndex& idx = *qs[0]->sparse_index;
      Workspace& W0 = *qs[0]->ws;
      const int planes = (int)db->params->p.planes();
      *ms_per_pass = timed_reps(W0.stream, iters, [&] {
        if (batch == 1 && layout == 1)
          run_sweep_sparse_scatter(W0, *db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p, G, 0, planes, true);
        else if (batch == 1)
          run_sweep_sparse(W0, *db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p);
        else if (layout == 1)
          run_sweep_sparse_scatter_group(Ws, batch, *db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p, G, W0.stream);
        else
          run_sweep_sparse_group(Ws, batch, *db, idx.col_ptr.p, idx.col_rows.p, idx.col_slots.p, W0.stream);
      });
      return;
    }
    if (db->planar_resident) {   // a planar row shard: k_sweep_planar_scatter, every plane, per-plane layout (there is no plain form)
      need(layout == 1, "a planar row shard has the scatter-form pass only (layout 1)");
      for (int i = 0; i < batch; i++) qs[i]->ws->ensure_sweep();
      PlanarPin none;
      SweepBatchDesc pd = group_pass(*db, qs, batch, false, none);
      Workspace& Wp = *qs[0]->ws;
      const int planes = (int)db->params->p.planes();
      *ms_per_pass = timed_reps(Wp.stream, iters, [&] {
        sweep_planar_resident_prepare(Wp.D->T, pd, Wp.stream);
        launch_sweep_planar_scatter(Wp.D->T, pd, G, 0, planes, false, Wp.stream);
      });
      return;
    }
    SweepBatchDesc d{};
    need(scatter_group_desc(qs, batch, db, G, d), "this group / shard does not take the scatter-form pass (sp_query_sweep_scatter_group would sweep per query)");
    Workspace& W0 = *qs[0]->ws;
    *ms_per_pass = timed_reps(W0.stream, iters, [&] {
      sweep_batch_prepare(W0.D->T, d, W0.stream);
      if (layout == 1)
        launch_sweep_batch_scatter(W0.D->T, d, G, W0.stream);
      else
        launch_sweep_batch(W0.D->T, d, W0.stream);   // the same rows, plain [z][ii] output: the scatter form's lower bound
    });
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
    sp_set_last_error_("null argument");
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
    if (rc != SP_OK) throw HipError(sp_last_error());
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
    if (rc != SP_OK) throw HipError(sp_last_error());
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
    DevBuf<u32> dense(mats_half_words(p, num_gsw));
    copy_mats_half(*W, FROM_MATS, 1, num_gsw, dense.p);
    download_ntt(*W, dense.p, dense.n, v_gsw, tmp);
  });
}

int sp_get_v_folding_neg(const sp_params_t* h, const uint64_t* v_folding, uint64_t* out) {
  return guarded([&] {
    need(h && v_folding && out, "null argument");
    const Params& p = h->p;
    const size_t nu2 = p.db_dim_2;
    if (nu2 == 0) return;
    Scoped W(h);
    W->ensure_expand();
    DevBuf<u64> tmp;
    DevBuf<u32> dense;
    upload_ntt(*W, v_folding, mats_half_words(p, nu2), dense, tmp);
    copy_mats_half(*W, TO_MATS, 1, nu2, dense.p);
    run_folding_neg(*W);
    copy_mats_half(*W, FROM_MATS, 0, nu2, dense.p);
    download_ntt(*W, dense.p, mats_half_words(p, nu2), out, tmp);
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
    const size_t nu2 = p.db_dim_2;
    if (nu2 > 0) {
      need(v_folding != nullptr, "v_folding is null");
      DevBuf<u32> dense(mats_half_words(p, nu2));
      copy_mats_half(*W, FROM_MATS, 1, nu2, dense.p);
      DevBuf<u64> tmp;
      download_ntt(*W, dense.p, dense.n, v_folding, tmp);
    }
  });
}

int sp_fold_ciphertexts(const sp_params_t* h, uint64_t* cts, size_t num_per, const uint64_t* v_folding,
                        const uint64_t* v_folding_neg) {
  return guarded([&] {
    need(h && cts && v_folding && v_folding_neg, "null argument");
    stage_fold(h, cts, num_per, v_folding, [&](Workspace& W, size_t further, DevBuf<u32>& dFn, DevBuf<u64>& tmp) {
      upload_ntt(W, v_folding_neg, mats_half_words(h->p, further), dFn, tmp);
      copy_mats_half(W, TO_MATS, 0, further, dFn.p);
      W.mats_w_ready = false;   // (whatever wave-layout operands the pooled workspace holds are not this call's)
      // the stage export honours the caller's v_folding_neg: literal path, every digit
      return FoldOpts{1L << 60, false, false};
    });
  });
}

int sp_fold_ciphertexts_fused(const sp_params_t* h, uint64_t* cts, size_t num_per, const uint64_t* v_folding,
                              long fused_min_pairs) {
  return guarded([&] {
    need(h && cts && v_folding, "null argument");
    stage_fold(h, cts, num_per, v_folding, [&](Workspace& W, size_t further, DevBuf<u32>&, DevBuf<u64>&) {
      launch_folding_neg(W.D->T, W.fold_mats.p, W.D->gadget_gsw.p, (int)further, (int)(2 * h->p.t_gsw), W.stream);
      run_mats_to_wave(W, further);
      // the caller's ciphertexts: below Q (what the reference's invariants give, and what lets the kernels skip the dead top
      // digit) only if every coefficient says so -- checked here, on the host copy
      bool below_q = true;
      for (size_t i = 0; i < num_per * 2 * POLY_LEN && below_q; i++) below_q = cts[i] < h->p.modulus;
      return FoldOpts{fused_min_pairs > 0 ? fused_min_pairs : W.fused_min_pairs, true, below_q};
    });
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
