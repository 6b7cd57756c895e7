// The 9 .. 16-query database pass over the DIGIT-PLANAR copy of a PACKED database (sweep_planar.hpp) and the one-time gather that
// builds the copy.  Its own translation unit: sweep.hip's kernels -- the judged single-query sweep among them -- compile to the same
// machine code whether or not this file changes (bench.py replays the sweep's PMC traffic record only into a library whose
// kernel has the recorded signature, sdk_amd/kernel_signature.py).
// (of sweep_mfma.hpp's one-tile table kernels, which come along with the shared digit helpers, only k_query_offset_terms is launched
// from here: by the one-tile pass over a planar-resident database, at the end of this file)
#pragma clang diagnostic ignored "-Wunused-function"
#include "device_common.hpp"
#include "sweep_planar.hpp"
#include "sweep_mfma_scatter.hpp"
#include "sweep_narrow_batch.hpp"
#include "planar_resident.hpp"
#include "db_copy_planar.hpp"
#include "db_remove_planar.hpp"
#include "db_digest_planar.hpp"
#include "db_item_digest_planar.hpp"
#include "server.hpp"

namespace spiral {

// second launch bound of the one-tile pass over a planar-resident database: waves per SIMD the registers have to allow (see
// launch_sweep_planar_resident)
constexpr int PLANAR1_MINWG = 2;

void launch_query_digits_planar(const QueryDigitsDesc& q, size_t entries, hipStream_t s) {
  hipLaunchKernelGGL(k_query_digits_planar, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, q);
  launched(0, "k_query_digits_planar");
}

// both tiles of a 9 .. 16-query group: tables [tile][N][blocks][2][4][64][16 B], then the offset terms [tile][N][32]
void launch_query_tables_planar2(const DevTables& T, const u64* const* qv, int batch, int dim0, int j0, int nj, u32* rq, hipStream_t s) {
  QueryDigits2Desc q{};
  for (int b = 0; b < batch && b < SWEEP_GROUP_MAX; b++) q.qv[b] = qv[b];
  q.rq = rq;
  q.batch = batch;
  q.dim0 = dim0;
  q.j0 = j0;
  q.nj = nj;
  const size_t entries = (size_t)N * (nj >> 4) * 128;   // 16-byte entries of one tile's table (== N * blocks * 8 * 64)
  hipLaunchKernelGGL(k_query_digits_planar2, dim3((unsigned)((entries / 8 + 255) / 256), 2), dim3(256), 0, s, q);   // a thread per 8 entries
  launched(0, "k_query_digits_planar2");
  hipLaunchKernelGGL(k_query_offset_terms2, dim3(N, 2), dim3(256), 0, s, T, q, rq + (size_t)2 * entries * 4);
  launched(0, "k_query_offset_terms2");
}

// ---- digit-planar database (sweep_planar.hpp) ----------------------------------------------------------------------------
bool sweep_planar_shape_ok(int num_per, int nj) {
  // whole 64-row blocks, the z-row's query planes of both tiles in LDS (nj <= 512), whole 128-column chunks
  return tunable("batch_planar", 1) != 0 && tunable("batch_mfma", 1) != 0 && nj > 0 && (nj % 64) == 0 && nj <= 512 && num_per >= 128 &&
         (num_per % 128) == 0;
}
size_t sweep_planar_bytes(int planes, int num_per, int nj) { return (size_t)planes * N * (size_t)num_per * (size_t)nj * 8; }
// one 16-byte planar entry, index [zp][chunk][g][c][block][e][a][lane], gathered from the PACKED units
static __device__ __forceinline__ mf_u32x4_t planar_gather_entry(const u32* packed, size_t idx, int num_per, int nj) {
  const int chunks = num_per >> 7, blocks = nj >> 6, npairs = nj >> 1;
  const int lane = (int)(idx & 63);
  size_t r = idx >> 6;
  const int a = (int)(r & 3), e = (int)((r >> 2) & 1);
  r >>= 3;
  const int block = (int)(r % blocks);
  r /= blocks;
  const int c = (int)(r & 1);
  r >>= 1;
  const int g = (int)(r & 3);
  r >>= 2;
  const int chunk = (int)(r % chunks);
  const size_t zp = r / chunks;
  const int kb = lane >> 4, n = lane & 15;
  const int slot = 16 * g + n;   // PACKED lane slot: columns 2 slot, 2 slot + 1 of the chunk; this tile's column is 2 slot + e
  mf_u32x4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 16; t++) {
    const int j = 64 * block + 16 * kb + t;
    const u32* unit = packed + packed_unit_offset(zp, j >> 1, chunk, npairs, chunks);
    const u64 w = unpack_word(unit, slot, (j & 1) * 2 + e);
    const u32 x = c ? (u32)(w >> 32) : (u32)w;
    o[t >> 2] |= ((offset_digits(x) >> (8 * a)) & 0xffu) << (8 * (t & 3));
  }
  return o;
}
__global__ __launch_bounds__(256) void k_packed_to_planar(unsigned char* planar, const u32* packed, size_t entries, int num_per, int nj) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < entries; idx += (size_t)gridDim.x * 256)
    reinterpret_cast<mf_u32x4_t*>(planar)[idx] = planar_gather_entry(packed, idx, num_per, nj);
}
void launch_packed_to_planar(unsigned char* planar, const u64* packed, int planes, int num_per, int nj, hipStream_t s) {
  const size_t entries = sweep_planar_bytes(planes, num_per, nj) / 16;
  hipLaunchKernelGGL(k_packed_to_planar, dim3(256 * 64), dim3(256), 0, s, planar, reinterpret_cast<const u32*>(packed), entries, num_per, nj);
  launched(0, "k_packed_to_planar");
}
// sp_db_update_item on a database that has a planar copy: the item (local row j, local column ii) is one word per (plane, z) of
// the PACKED words = one byte in each of the 8 entries (modulus c, digit a) of that (plane, z): regather those, one per thread
__global__ __launch_bounds__(256) void k_planar_patch_item(unsigned char* planar, const u32* packed, size_t zps, int num_per, int nj, int j, int ii) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= zps * 8) return;
  const size_t zp = t >> 3;
  const int c = (int)((t >> 2) & 1), a = (int)(t & 3);
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const int chunk = ii >> 7, col = ii & 127, slot = col >> 1, e = col & 1, g = slot >> 4, n = slot & 15;
  const int block = j >> 6, kb = (j & 63) >> 4;
  const size_t idx = planar_operand_offset(zp, chunk, g, block, e, c, a, chunks, blocks) / 16 + (size_t)(16 * kb + n);
  reinterpret_cast<mf_u32x4_t*>(planar)[idx] = planar_gather_entry(packed, idx, num_per, nj);
}
void launch_planar_patch_item(unsigned char* planar, const u64* packed, int planes, int num_per, int nj, int j, int ii, hipStream_t s) {
  const size_t zps = (size_t)planes * N;
  hipLaunchKernelGGL(k_planar_patch_item, dim3((unsigned)((zps * 8 + 255) / 256)), dim3(256), 0, s, planar,
                     reinterpret_cast<const u32*>(packed), zps, num_per, nj, j, ii);
  launched(0, "k_planar_patch_item");
}
// sp_db_update_items: the list form.  cells[e] = (local row j, local column ii) stands for the column's 16-row group j >> 4, whose 16
// bytes per (plane, z, modulus c, digit a) are ONE entry: thread (e, zp, c, a) regathers it from the words the encode launch before it
// on the stream has written.  The caller lists a (j >> 4, ii) once, so no entry has two writers.
__global__ __launch_bounds__(256) void k_planar_patch_items(unsigned char* planar, const u32* packed, size_t zps, int num_per, int nj,
                                                            const PlanarPatchCell* cells, size_t n_cells) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per = zps * 8;
  if (t >= n_cells * per) return;
  const PlanarPatchCell cell = cells[t / per];
  const size_t r = t % per;
  const size_t zp = r >> 3;
  const int c = (int)((r >> 2) & 1), a = (int)(r & 3);
  const int j = cell.j, ii = cell.ii;
  const int chunks = num_per >> 7, blocks = nj >> 6;
  const int chunk = ii >> 7, col = ii & 127, slot = col >> 1, e = col & 1, g = slot >> 4, n = slot & 15;
  const int block = j >> 6, kb = (j & 63) >> 4;
  const size_t idx = planar_operand_offset(zp, chunk, g, block, e, c, a, chunks, blocks) / 16 + (size_t)(16 * kb + n);
  reinterpret_cast<mf_u32x4_t*>(planar)[idx] = planar_gather_entry(packed, idx, num_per, nj);
}
void launch_planar_patch_items(unsigned char* planar, const u64* packed, int planes, int num_per, int nj, const PlanarPatchCell* cells,
                               size_t n_cells, hipStream_t s) {
  if (n_cells == 0) return;
  const size_t zps = (size_t)planes * N;   // (n_cells * 64 * planes <= 2^30 blocks: see UPSERT_MAX_GROUP_PLANES)
  hipLaunchKernelGGL(k_planar_patch_items, dim3((unsigned)((n_cells * zps * 8 + 255) / 256)), dim3(256), 0, s, planar,
                     reinterpret_cast<const u32*>(packed), zps, num_per, nj, cells, n_cells);
  launched(0, "k_planar_patch_items");
}
// the 9 .. 16-query pass over the planar copy: 3.47 ms per C2 plane against 4.19 for k_sweep_mfma_batch<8, 1, 0, 2> on the PACKED
// words (scripts/ubench/mfma_planar.hip, profiles/r05_mfma_planar.md); eight waves per workgroup share the z-row's query planes
// where the workgroup has two chunks to split, units of the load ring as the row count allows
void launch_sweep_planar(const DevTables& T, const SweepBatchDesc& d, hipStream_t s) {
  SweepPlanarDesc m{};
  m.db = d.planar;
  m.rq = reinterpret_cast<const unsigned char*>(d.rq);
  m.rq_off = d.rq + (size_t)2 * N * (d.nj >> 4) * 128 * 4;
  for (int b = 0; b < d.batch; b++) m.out[b] = d.out[b];
  m.batch = d.batch;
  m.planes = d.planes;
  m.num_per = d.num_per;
  m.nj = d.nj;
  const int chunks = d.num_per >> 7;
  int cpw = (int)tunable("batch_mfma_cpw", 16);
  cpw = std::max(1, std::min(cpw, chunks));
  while (chunks % cpw) cpw--;
  m.cpw = cpw;
  const u64 qs[2] = {MODULUS_0, MODULUS_1};
  for (int c = 0; c < 2; c++) {
    m.c4[c] = (u32)((1ull << 32) % qs[c]);
    m.c5[c] = (u32)((1ull << 40) % qs[c]);
    m.c6[c] = (u32)((1ull << 48) % qs[c]);
  }
  const dim3 grid((unsigned)((size_t)d.planes * N * (chunks / cpw)));
  const size_t lds = (size_t)2 * (d.nj >> 6) * 8 * 64 * 16;   // both tiles' query planes of one z-row
  const bool eight = (cpw % 2) == 0;
  const bool ring4 = ((2 * (d.nj >> 6)) % 4) == 0;
#define SP_PLANAR(NBUF_, WAVES_)                                                                                          \
  {                                                                                                                        \
    if (lds > 65536)                                                                                                       \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_planar<NBUF_, 2, 0, 1, WAVES_>),                \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                \
    hipLaunchKernelGGL((k_sweep_planar<NBUF_, 2, 0, 1, WAVES_>), grid, dim3(64 * WAVES_), lds, s, T, m);                    \
  }
  if (eight && ring4) SP_PLANAR(4, 8) else if (eight) SP_PLANAR(2, 8) else if (ring4) SP_PLANAR(4, 4) else SP_PLANAR(2, 4)
#undef SP_PLANAR
  launched(PATH_SWEEP_BATCH | PATH_SWEEP_MFMA | PATH_SWEEP_MFMA2 | PATH_SWEEP_PLANAR, "k_sweep_planar");
}

// ---- the one-tile pass over a row shard in the reduce-scatter layout (sweep_mfma_scatter.hpp) --------------------------------
bool sweep_batch_scatter_ok(const SweepBatchDesc& d, int G) {
  return tunable("batch_scatter", 1) != 0 && (G == 2 || G == 4 || G == 8) && d.batch <= SWEEP_BATCH_MAX && sweep_batch_wants_mfma(d);
}
void launch_sweep_batch_scatter(const DevTables& T, const SweepBatchDesc& d, int G, hipStream_t s) {
  if (!d.use_mfma || !d.rq || !sweep_batch_scatter_ok(d, G)) throw HipError("internal: the scatter-form batched pass does not take this group");
  SweepScatterDesc m{};
  m.db = d.db;
  m.rq = d.rq;
  m.rq_off = d.rq + (size_t)N * (d.nj >> 4) * 128 * 4;
  for (int b = 0; b < d.batch; b++) m.out[b] = d.out[b];
  for (int b = d.batch; b < SWEEP_BATCH_MAX; b++) m.out[b] = d.out[0];   // never stored to (b < batch in the kernel)
  m.batch = d.batch;
  m.planes = d.planes;
  m.num_per = d.num_per;
  m.nj = d.nj;
  m.G = G;
  m.lgG = G == 2 ? 1 : G == 4 ? 2 : 3;
  const int chunks = d.num_per >> 7;
  int cpw = (int)tunable("batch_mfma_cpw", 16);
  cpw = std::max(1, std::min(cpw, chunks));
  while (chunks % cpw) cpw--;
  m.cpw = cpw;
  const u64 qs[2] = {MODULUS_0, MODULUS_1};
  for (int c = 0; c < 2; c++) {
    m.c4[c] = (u32)((1ull << 32) % qs[c]);
    m.c5[c] = (u32)((1ull << 40) % qs[c]);
    m.c6[c] = (u32)((1ull << 48) % qs[c]);
  }
  const dim3 grid((unsigned)((size_t)d.planes * N * (chunks / cpw)));
  // store shape: switch batch_scatter_store (1 = dword stores from the registers, 2 = staged through LDS); the default is the
  // measured winner (profiles/sharded_batch_pass.md)
  const bool staged = tunable("batch_scatter_store", BATCH_SCATTER_STORE_DEFAULT) == 2;
  const size_t lds = (size_t)d.nj * 128 + (staged ? SCATTER_STAGE_BYTES : 0);   // one z-row of the digit table (+ the stage)
#define SP_SCATTER(STORE_)                                                                                              \
  {                                                                                                                      \
    if (lds > 65536)                                                                                                     \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_mfma_scatter<2, 2, STORE_>),                  \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                              \
    hipLaunchKernelGGL((k_sweep_mfma_scatter<2, 2, STORE_>), grid, dim3(256), lds, s, T, m);                             \
  }
  if (staged) SP_SCATTER(2) else SP_SCATTER(1)
#undef SP_SCATTER
  launched(PATH_SWEEP_BATCH | PATH_SWEEP_MFMA | PATH_SCATTER_OUT | PATH_SWEEP_BATCH_SCATTER, "k_sweep_mfma_scatter");
}

// ---- one pass over a narrow database for a group of up to 8 queries (sweep_narrow_batch.hpp) ---------------------------------
bool sweep_narrow_batch_shape_ok(int num_per, int nj) {
  return num_per >= 2 && num_per <= 64 && (num_per & (num_per - 1)) == 0 && nj > 0;
}
void launch_sweep_narrow_batch(const DevTables& T, const SweepBatchDesc& d0, hipStream_t s) {
  if (!d0.narrow || d0.batch < 1 || d0.batch > SWEEP_BATCH_MAX || !sweep_narrow_batch_shape_ok(d0.num_per, d0.nj))
    throw HipError("internal: the narrow batched pass does not take this group");
  SweepBatchDesc d = d0;
  for (int b = d.batch; b < SWEEP_BATCH_MAX; b++) {   // dead slots: valid rows to read, never stored
    d.qv[b] = d.qv[0];
    d.out[b] = nullptr;
  }
  const long fe = d.fold_every > 0 ? d.fold_every : tunable("narrow_batch_fold_every", 255);
  d.fold_every = (int)std::max(1L, std::min(255L, fe));
  const dim3 grid((unsigned)((size_t)d.planes * N));
#define SP_NARROW_BATCH(B_)                                                                                              \
  {                                                                                                                       \
    const size_t lds = sweep_narrow_batch_lds(B_);                                                                        \
    /* more than 64 KiB of dynamic LDS: raised on every launch, on the current device (see launch_sweep_mfma) */          \
    if (lds > 65536)                                                                                                      \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_narrow_batch<B_>),                             \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                               \
    hipLaunchKernelGGL((k_sweep_narrow_batch<B_>), grid, dim3(256), lds, s, T, d);                                        \
  }
  if (d.batch <= 2) SP_NARROW_BATCH(2) else if (d.batch <= 4) SP_NARROW_BATCH(4) else SP_NARROW_BATCH(8)
#undef SP_NARROW_BATCH
  launched(PATH_SWEEP_NARROW_GROUP, "k_sweep_narrow_batch");
}

// ---- planar-resident databases (sp_db_create_planar; planar_resident.hpp) ----------------------------------------------------
// the shape rule alone: what was decided from the switches when the handle was created holds for its life
bool planar_resident_shape_ok(int num_per, int nj) { return nj > 0 && (nj % 64) == 0 && nj <= 512 && num_per >= 128 && (num_per % 128) == 0; }
// groups of 9 .. 16 need both tiles' z-rows of query planes in one workgroup's LDS (nj * 256 bytes)
int planar_resident_group_max(int nj) {
  int dev = 0, lds_optin = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds_optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) {
    (void)hipGetLastError();
    return SWEEP_BATCH_MAX;
  }
  return (size_t)lds_optin >= (size_t)nj * 256 ? SWEEP_GROUP_MAX : SWEEP_BATCH_MAX;
}
// a handle's row window and column order as the kernels take them (an unsharded handle: every row, the identity)
static PlanarRows planar_rows(const PlanarShardShape& sh, int nj) { return PlanarRows{sh.dim0 > 0 ? sh.dim0 : nj, sh.j0}; }
static PlanarCols planar_cols(const PlanarShardShape& sh, int num_per) {
  int lgG = 0, lgn = 0;
  while ((1 << lgG) < sh.G) lgG++;
  while ((1 << lgn) < num_per) lgn++;
  return PlanarCols{lgG, lgn - lgG};
}
void launch_planar_from_ref(unsigned char* planar, const u64* src, int plane, int z0, int nz, int num_per, int nj, PlanarShardShape sh,
                            hipStream_t s) {
  if (nz <= 0) return;
  const size_t threads = (size_t)nz * (size_t)num_per * (size_t)(nj >> 4);
  hipLaunchKernelGGL(k_planar_from_ref, dim3((unsigned)std::min<size_t>((threads + 255) / 256, 256 * 64)), dim3(256), 0, s, planar, src,
                     (size_t)plane * N + (size_t)z0, nz, num_per, nj, planar_rows(sh, nj), planar_cols(sh, num_per));
  launched(0, "k_planar_from_ref");
}
void launch_planar_synth(unsigned char* planar, u64 seed, int planes, int num_per, int nj, PlanarShardShape sh, hipStream_t s) {
  hipLaunchKernelGGL(k_planar_synth, dim3(256 * 64), dim3(256), 0, s, planar, seed, (size_t)planes * N, num_per, nj, planar_rows(sh, nj),
                     planar_cols(sh, num_per));
  launched(0, "k_planar_synth");
}
void launch_planar_from_stage(unsigned char* planar, const u64* stage, int planes, int jg, int ii0, int ncols, int num_per, int nj,
                              PlanarShardShape sh, hipStream_t s) {
  const size_t threads = (size_t)planes * N * (size_t)ncols;
  hipLaunchKernelGGL(k_planar_from_stage, dim3((unsigned)std::min<size_t>((threads + 255) / 256, 256 * 64)), dim3(256), 0, s, planar, stage,
                     (size_t)planes * N, jg, ii0, ncols, num_per, nj, planar_cols(sh, num_per));
  launched(0, "k_planar_from_stage");
}
void launch_planar_put_items(unsigned char* planar, const u64* stage, int planes, size_t np_s, const PlanarPatchCell* cells, size_t n_items,
                             int num_per, int nj, PlanarShardShape sh, hipStream_t s) {
  if (n_items == 0) return;
  const size_t zps = (size_t)planes * N;   // (n_items * planes * N / 256 blocks: the caller's windows keep n_items * planes <= 2^23)
  hipLaunchKernelGGL(k_planar_put_items, dim3((unsigned)((n_items * zps + 255) / 256)), dim3(256), 0, s, planar, stage, zps, np_s, cells,
                     n_items, num_per, nj, planar_cols(sh, num_per));
  launched(0, "k_planar_put_items");
}
void launch_planar_read(u64* out, const unsigned char* planar, int plane, int z, int ii, int jl0, int count, int num_per, int nj,
                        PlanarShardShape sh, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_planar_read, dim3((count + 63) / 64), dim3(64), 0, s, out, planar, (size_t)plane * N + (size_t)z, ii, jl0, count,
                     num_per, nj, planar_cols(sh, num_per));
  launched(0, "k_planar_read");
}
void launch_planar_gather(u64* dst, const unsigned char* planar, size_t L0, size_t nL, int num_per, int nj, int planes, PlanarShardShape sh,
                          hipStream_t s) {
  if (nL == 0) return;
  const int rg_lo = (int)(L0 / (size_t)num_per) >> 4, rg_hi = (int)((L0 + nL - 1) / (size_t)num_per) >> 4;
  hipLaunchKernelGGL(k_planar_gather, dim3((unsigned)(rg_hi - rg_lo + 1) * (unsigned)(num_per >> 4), N / PLANAR_GATHER_Z, planes), dim3(256), 0,
                     s, dst, planar, L0, nL, rg_lo, num_per, nj, planes, planar_cols(sh, num_per));
  launched(0, "k_planar_gather");
}
void launch_planar_scatter_items(unsigned char* planar, const u64* stage, const CopyCellRec* cells, size_t n_cells, int num_per, int nj,
                                 int planes, PlanarShardShape sh, hipStream_t s) {
  if (n_cells == 0) return;
  hipLaunchKernelGGL(k_planar_scatter_items, dim3((unsigned)((n_cells + 15) / 16), N / PLANAR_GATHER_Z, planes), dim3(256), 0, s, planar, stage,
                     cells, n_cells, num_per, nj, planes, planar_cols(sh, num_per));
  launched(0, "k_planar_scatter_items");
}
void launch_planar_clear_items(unsigned char* planar, const RemoveCellRec* cells, size_t n_cells, int num_per, int nj, int planes,
                               PlanarShardShape sh, hipStream_t s) {
  if (n_cells == 0) return;
  hipLaunchKernelGGL(k_planar_clear_items, dim3((unsigned)((n_cells + 15) / 16), N / PLANAR_CLEAR_Z, planes), dim3(256), 0, s, planar, cells,
                     n_cells, num_per, nj, planar_cols(sh, num_per));
  launched(0, "k_planar_clear_items");
}
// sp_db_digest over digit-planar words: about 32 sixteen-row groups per thread where the plane has that many, so a workgroup's copy of the
// row keys is read many times over
void launch_digest_planar(const DigestDesc& d, const unsigned char* planar, PlanarShardShape sh, hipStream_t s) {
  if (d.nplanes <= 0 || d.nj <= 0) return;
  if (d.nj > DIGEST_ROWS) throw HipError("internal: a planar database of more than DIGEST_ROWS rows");
  const size_t groups = (size_t)N * (size_t)d.num_per * (size_t)(d.nj >> 4);
  const unsigned wgs = (unsigned)std::max<size_t>(1, std::min<size_t>((groups + 255) / 256, std::max<size_t>(4096, groups / (256 * 32))));
  hipLaunchKernelGGL(k_digest_planar, dim3(wgs, d.nplanes), dim3(256), 0, s, d, planar, planar_cols(sh, d.num_per));
  launched(0, "k_digest_planar");
}
// sp_db_item_digests over digit-planar words: one thread per half of a (16-row group, column) of the 64-row blocks the window touches
void launch_item_digest_planar(const ItemDigestDesc& d, const unsigned char* planar, PlanarShardShape sh, hipStream_t s) {
  if (d.nplanes <= 0 || d.nrows <= 0) return;
  const int nblk = ((d.jl0 + d.nrows - 1) >> 6) - (d.jl0 >> 6) + 1;
  const size_t threads = (size_t)(d.num_per >> 7) * 4 * (size_t)nblk * 2 * 64 * 2;
  hipLaunchKernelGGL(k_item_digest_planar, dim3((unsigned)((threads + 255) / 256), N / ITEM_DIGEST_Z, d.nplanes), dim3(256), 0, s, d, planar,
                     planar_cols(sh, d.num_per));
  launched(0, "k_item_digest_planar");
}
// The group's query tables for a pass over a planar-resident database (d.planar = its words): one tile's planar tables and offset
// terms for 1 .. 8 queries, both tiles' for 9 .. 16.  No switch is asked: the handle's format was decided when it was created.
void sweep_planar_resident_prepare(const DevTables& T, SweepBatchDesc& d, hipStream_t s) {
  if (!d.planar || !d.rq || d.batch < 1 || d.batch > SWEEP_GROUP_MAX) throw HipError("internal: not a group of a planar-resident database");
  d.use_mfma = 1;
  if (sweep_batch_tiles(d.batch) == 2) {
    launch_query_tables_planar2(T, d.qv, d.batch, d.dim0, d.j0, d.nj, d.rq, s);
    return;
  }
  QueryDigitsDesc q{};
  for (int b = 0; b < d.batch; b++) q.qv[b] = d.qv[b];
  q.rq = d.rq;
  q.batch = d.batch;
  q.dim0 = d.dim0;
  q.j0 = d.j0;
  q.nj = d.nj;
  const size_t entries = (size_t)N * (d.nj >> 4) * 128;
  launch_query_digits_planar(q, entries, s);
  hipLaunchKernelGGL(k_query_offset_terms, dim3(N), dim3(256), 0, s, T, q, d.rq + entries * 4);
  launched(0, "k_query_offset_terms");
}
// The pass: 9 .. 16 queries take launch_sweep_planar as it is; 1 .. 8 take the same kernel with ONE query tile: 56 accumulator
// registers where two tiles hold 112, and half the LDS (nj * 128 bytes: 64 KiB at 512 rows, the default limit, two workgroups of a
// CU's 160 KiB).  Workgroup shape and ring depth are chosen as for two tiles.  The registers the compiler reports (gfx950, bound of two
// waves per SIMD): 155 with the ring of 4 units, 125 with the ring of 2 -- three and four waves per SIMD.  Four-wave workgroups
// therefore run two per CU at 512 rows (LDS-bound) and more at fewer rows; eight-wave workgroups run one per CU with the ring of 4
// (two waves per SIMD, as the two-tile pass) and two with the ring of 2.  Compiled for four waves per SIMD the ring of 4 spills (212
// bytes of scratch), so that bound is not asked for.  tests/test_planar_resident_kernel_resources.py holds these numbers.
void launch_sweep_planar_resident(const DevTables& T, const SweepBatchDesc& d, hipStream_t s) {
  if (!d.planar || !d.rq || !d.use_mfma) throw HipError("internal: not a prepared group of a planar-resident database");
  if (sweep_batch_tiles(d.batch) == 2) {
    launch_sweep_planar(T, d, s);
    return;
  }
  SweepPlanarDesc m{};
  m.db = d.planar;
  m.rq = reinterpret_cast<const unsigned char*>(d.rq);
  m.rq_off = d.rq + (size_t)N * (d.nj >> 4) * 128 * 4;
  for (int b = 0; b < d.batch; b++) m.out[b] = d.out[b];
  for (int b = d.batch; b < SWEEP_MFMA_MAX; b++) m.out[b] = d.out[0];   // never stored to (b < batch in the kernel)
  m.batch = d.batch;
  m.planes = d.planes;
  m.num_per = d.num_per;
  m.nj = d.nj;
  const int chunks = d.num_per >> 7;
  int cpw = (int)tunable("batch_mfma_cpw", 16);
  cpw = std::max(1, std::min(cpw, chunks));
  while (chunks % cpw) cpw--;
  m.cpw = cpw;
  const u64 qs[2] = {MODULUS_0, MODULUS_1};
  for (int c = 0; c < 2; c++) {
    m.c4[c] = (u32)((1ull << 32) % qs[c]);
    m.c5[c] = (u32)((1ull << 40) % qs[c]);
    m.c6[c] = (u32)((1ull << 48) % qs[c]);
  }
  const dim3 grid((unsigned)((size_t)d.planes * N * (chunks / cpw)));
  const size_t lds = (size_t)d.nj * 128;   // one tile's query planes of one z-row
  const bool eight = (cpw % 2) == 0;
  const bool ring4 = ((2 * (d.nj >> 6)) % 4) == 0;
#define SP_PLANAR1(NBUF_, WAVES_)                                                                                             \
  {                                                                                                                            \
    if (lds > 65536)                                                                                                           \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_planar<NBUF_, 1, 0, PLANAR1_MINWG, WAVES_>),        \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                    \
    hipLaunchKernelGGL((k_sweep_planar<NBUF_, 1, 0, PLANAR1_MINWG, WAVES_>), grid, dim3(64 * WAVES_), lds, s, T, m);            \
  }
  if (eight && ring4) SP_PLANAR1(4, 8) else if (eight) SP_PLANAR1(2, 8) else if (ring4) SP_PLANAR1(4, 4) else SP_PLANAR1(2, 4)
#undef SP_PLANAR1
  launched(PATH_SWEEP_BATCH | PATH_SWEEP_MFMA | PATH_SWEEP_PLANAR, "k_sweep_planar (one query tile)");
}

// ---- the pass over a planar ROW SHARD (sp_db_create_planar_shard), in the reduce-scatter layout ------------------------------------
// k_sweep_planar's scatter form: one query tile for 1 .. 8 queries, two for 9 .. 16; workgroup shape and ring depth by the rules of the
// plain form (64 local rows: two units per pass, so the ring of 2).  The shard's resident column order (planar_resident.hpp) makes the
// stores the plain form's; only the addresses differ, and they come from the descriptor, so the per-plane layout of
// sp_query_sweep_scatter_plane / _group and the all-planes layout of sp_query_sweep_scatter are one kernel.
// Path bits: scatter_out with sweep_batch | sweep_batch_mfma | sweep_batch_planar (| sweep_batch_mfma_two_tiles), a combination no other
// flow reports; sweep_batch_scatter stays the name of k_sweep_mfma_scatter's pass over a PACKED shard and is NOT set here.
void launch_sweep_planar_scatter(const DevTables& T, const SweepBatchDesc& d, int G, int plane0, int total_planes, bool all_planes,
                                 hipStream_t s) {
  if (!d.planar || !d.rq || !d.use_mfma || d.batch < 1 || d.batch > SWEEP_GROUP_MAX || !(G == 2 || G == 4 || G == 8) ||
      !planar_resident_shape_ok(d.num_per, d.nj) || d.num_per / G < 2 || plane0 < 0 || d.planes < 1 || plane0 + d.planes > total_planes ||
      (all_planes && plane0 != 0))
    throw HipError("internal: not a prepared group of a planar row shard");
  const int tiles = sweep_batch_tiles(d.batch);
  const int npg = d.num_per / G;
  SweepPlanarDesc m{};
  m.db = d.planar;
  m.rq = reinterpret_cast<const unsigned char*>(d.rq);
  m.rq_off = d.rq + (size_t)tiles * N * (d.nj >> 4) * 128 * 4;
  m.plane_stride = all_planes ? (size_t)4 * N * npg : (size_t)4 * N * d.num_per;
  m.class_stride = all_planes ? (size_t)total_planes * 4 * N * npg : (size_t)4 * N * npg;
  for (m.lg_npg = 0; (1 << m.lg_npg) < npg; m.lg_npg++) {}
  const size_t out0 = all_planes ? 0 : (size_t)plane0 * m.plane_stride;
  for (int b = 0; b < SWEEP_MFMA_MAX; b++) m.out[b] = d.out[b < d.batch ? b : 0] + out0;   // (b >= batch: never stored to)
  m.batch = d.batch;
  m.planes = d.planes;
  m.num_per = d.num_per;
  m.nj = d.nj;
  const int chunks = d.num_per >> 7;
  int cpw = (int)tunable("batch_mfma_cpw", 16);
  cpw = std::max(1, std::min(cpw, chunks));
  while (chunks % cpw) cpw--;
  m.cpw = cpw;
  const u64 qs[2] = {MODULUS_0, MODULUS_1};
  for (int c = 0; c < 2; c++) {
    m.c4[c] = (u32)((1ull << 32) % qs[c]);
    m.c5[c] = (u32)((1ull << 40) % qs[c]);
    m.c6[c] = (u32)((1ull << 48) % qs[c]);
  }
  const dim3 grid((unsigned)((size_t)d.planes * N * (chunks / cpw)));
  const size_t lds = (size_t)tiles * d.nj * 128;   // the tiles' query planes of one z-row
  const bool eight = (cpw % 2) == 0;
  const bool ring4 = ((2 * (d.nj >> 6)) % 4) == 0;
#define SP_PLANAR_SC(NBUF_, QT_, MINWG_, WAVES_)                                                                               \
  {                                                                                                                            \
    if (lds > 65536)                                                                                                           \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_planar_scatter<NBUF_, QT_, MINWG_, WAVES_>),        \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                    \
    hipLaunchKernelGGL((k_sweep_planar_scatter<NBUF_, QT_, MINWG_, WAVES_>), grid, dim3(64 * WAVES_), lds, s, T, m);            \
  }
  if (tiles == 2) {
    if (eight && ring4) SP_PLANAR_SC(4, 2, 1, 8) else if (eight) SP_PLANAR_SC(2, 2, 1, 8) else if (ring4) SP_PLANAR_SC(4, 2, 1, 4) else SP_PLANAR_SC(2, 2, 1, 4)
  } else {
    if (eight && ring4) SP_PLANAR_SC(4, 1, PLANAR1_MINWG, 8) else if (eight) SP_PLANAR_SC(2, 1, PLANAR1_MINWG, 8)
    else if (ring4) SP_PLANAR_SC(4, 1, PLANAR1_MINWG, 4) else SP_PLANAR_SC(2, 1, PLANAR1_MINWG, 4)
  }
#undef SP_PLANAR_SC
  launched(PATH_SCATTER_OUT | PATH_SWEEP_BATCH | PATH_SWEEP_MFMA | PATH_SWEEP_PLANAR | (tiles == 2 ? PATH_SWEEP_MFMA2 : 0),
           tiles == 2 ? "k_sweep_planar_scatter" : "k_sweep_planar_scatter (one query tile)");
}

}  // namespace spiral
