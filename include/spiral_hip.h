/*
 * spiral_hip.h -- C ABI of libspiral_hip.so: the MI355X (gfx950) implementation of the Spiral PIR
 * server answer path of blyssprivacy/sdk `lib/spiral-rs` (feature `server`).
 *
 * This is the drop-in boundary.  Every entry point names the reference interface it replaces
 * (file:line under /root/reference/lib/spiral-rs/src/).  Plain pointers and sizes only; all
 * multi-byte data is little-endian / native-endian exactly as the reference's `to_ne_bytes`
 * wire formats on x86-64 (client.rs:58,77,292; util.rs:294-319).
 *
 * Conventions
 *   - Opaque handles, freed by the matching *_free.  The library never frees caller memory.
 *   - Functions returning `int` return SP_OK (0) or a negative SP_E_* code; the message is in
 *     sp_last_error() (thread-local).  Nothing panics/aborts across the ABI; a Rust shim turns a
 *     non-zero status into the `panic!`/`assert!` the reference would have raised
 *     (client.rs:213,304; server.rs:131-132,434-439).
 *   - "ref layout": PolyMatrixRaw = rows*cols*N u64 (poly.rs:31-35,92-94); PolyMatrixNTT =
 *     rows*cols*crt_count*N u64, each < moduli[crt] (poly.rs:263-265).  N = poly_len = 2048,
 *     crt_count = 2, moduli {268369921, 249561089} (util.rs:245-248).
 *   - Every compute entry point runs on the HIP device; there is no CPU fallback.  If no gfx950
 *     device is usable the call fails with SP_E_HIP.
 *   - Handles are immutable after creation and may be shared by host threads; each call takes a
 *     private workspace + HIP stream from an internal pool.
 */
#ifndef SPIRAL_HIP_H
#define SPIRAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK 0
#define SP_E_ARG (-1)    /* bad argument / length mismatch (reference: assert_eq! on sizes) */
#define SP_E_HIP (-2)    /* HIP runtime error or no device */
#define SP_E_OOM (-3)    /* device or host allocation failed */
#define SP_E_STATE (-4)  /* call sequence error */
#define SP_E_NOTFOUND (-5) /* unknown client uuid (lib/server Error::NotFound -> HTTP 404, lib/server/src/error.rs:7-34) */

/* Row shards per database: each shard emits partial residues < q < 2^28 that the exchange step sums element-wise in
 * 32 bits (ncclSum on ncclUint32); 8 * (q - 1) < 2^31, so 8 is the largest shard count that can never overflow.
 * sp_db_create and the sp_query_sweep_scatter / fold_local family reject larger counts with SP_E_ARG. */
#define SP_MAX_ROW_SHARDS 8

typedef struct sp_params sp_params_t; /* spiral_rs::params::Params           params.rs:49-82   */
typedef struct sp_pp sp_pp_t;         /* spiral_rs::client::PublicParameters client.rs:146-152 */
typedef struct sp_ppc sp_ppc_t;       /* a client's public parameters as sent: the wire image on the device, not expanded */
typedef struct sp_db sp_db_t;         /* the `db: &[u64]` argument of process_query, device-resident */
typedef struct sp_query sp_query_t;   /* one in-flight query (expanded), for the multi-GPU split */

const char* sp_last_error(void);
/* Diagnostics: bit mask of the kernels / flows the CALLING THREAD's library calls went through since the last reset
 * (bit b is named by sp_path_name(b): sweep_packed_persist, from_sweep4, fold_fused, fold_tail_delta,
 * pipelined_fold_overlap, expand_pruned, ...).  Tests use it to assert that the bytes they compared were produced by
 * the production code path (e.g. the persistent PACKED sweep + fused fold + fold/sweep overlap at full size) and not
 * by a silently selected fallback kernel.  reset != 0 clears the mask after reading it. */
uint64_t sp_paths_taken(int reset);
const char* sp_path_name(int bit); /* NULL past the last defined bit */
/* Run-time tunables for A/B measurements inside one process (the same switches as the SPIRAL_<NAME> environment
 * variables of DESIGN.md section 8, e.g. "pipe_ring", "pipe_tail_defer", "sweep_prio", "batch_group"): takes effect on the next launch / next workspace. */
int sp_debug_set(const char* name, long value);
/* Number of visible HIP devices (0 if none); selects `device` for this thread's subsequent calls. */
int sp_device_count(void);
int sp_set_device(int device);

/* ------------------------------------------------------------------ Params
 * util.rs:219-263 params_from_json(): keys n, nu_1, nu_2, p, q2_bits, t_gsw, t_conv, t_exp_left,
 * t_exp_right, instances, db_item_size, version; presence of "direct_upload" disables query
 * expansion.  Single or double quotes are accepted (the reference's presets use single quotes and
 * `.replace("'", "\"")`, util.rs:104-120). */
sp_params_t* sp_params_from_json(const char* json);
/* The params handle owns the device tables and the pool of workspaces every other handle made from it borrows (spiral-rs:
 * `&'a Params` in PublicParameters, Query, the database slice): free those first -- sp_query_t, sp_pp_t, sp_db_t, sp_server_t,
 * a reserved sp_comm_t -- then the params. */
void sp_params_free(sp_params_t*);
/* Field / derived-size accessor: poly_len, crt_count, modulus, moduli0, moduli1, n, pt_modulus,
 * q2_bits, t_conv, t_exp_left, t_exp_right, t_gsw, expand_queries, db_dim_1, db_dim_2, instances,
 * db_item_size, version, g (params.rs:129), stop_round (:134), setup_bytes (:146), query_bytes
 * (:169), num_items (:120), db_words (instances*n*n*num_items*N), response_bytes
 * (server.rs:476-480).  Returns UINT64_MAX for an unknown name. */
uint64_t sp_params_get(const sp_params_t*, const char* name);
/* ntt_tables[crt][which][0..N) (params.rs:85-96, ntt.rs:39-65); which: 0 fwd, 1 fwd', 2 inv, 3 inv' */
int sp_params_ntt_table(const sp_params_t*, int crt, int which, uint64_t* out_n);

/* --------------------------------------------------------------------- DB
 * The reference passes the whole preprocessed database as `db: &[u64]` on every call
 * (server.rs:650-655) in the layout [instance][trial][z][ii][j], word = lo28 | hi28 << 32
 * (server.rs:262-270).  A per-call host pointer cannot be streamed at HBM rate, so residency is the
 * one deliberate API change: register once, query many times.
 * Row sharding (multi-GPU): shard `s` of `S` holds first-dimension rows j in [s*dim0/S, (s+1)*dim0/S). */
sp_db_t* sp_db_create(const sp_params_t*, int shard, int num_shards);
/* Column sharding (the zero-reduction alternative): shard s of S (a power of two) holds the
 * output columns ii = s (mod S) of every row.  Each shard's sweep yields complete first-dimension outputs
 * for its columns, so the flow is sp_query_sweep -> sp_query_fold_local(q, sp_query_partial_ptr(q), S) ->
 * gather of the local results -> sp_query_finish_gathered; no partial sums cross GPUs. */
sp_db_t* sp_db_create_columns(const sp_params_t*, int shard, int num_shards);
/* A sparse bucket: lib/server's SparseDb (lib/server/src/db/sparse_db.rs:5-48).  Starts empty; items arrive through
 * sp_db_update_item (= update_item_raw + upsert, db/loading.rs:317-359) and only they are stored (one packed NTT
 * polynomial per (item, plane)) and multiplied, so the first-dimension step costs time in proportion to the occupancy.
 * sp_process_query / sp_query_begin_for_db + sweep + finish on such a handle follow lib/server's process_query
 * (lib/server/src/server.rs:17-99): expansion pruned to the rows that hold items (compute/query_expansion.rs:213-357),
 * multiply_reg_by_sparse_database (compute/dot_product.rs:13-220; exact sums mod q, not the reference's wrapping u64),
 * and fold_ciphertexts with the all-zero shortcuts of compute/fold.rs:38-44 -- so the response bytes are lib/server's,
 * which differ from spiral-rs's dense process_query over the zero-filled database wherever a shortcut fires (both
 * decode to the item).  Updates must not run concurrently with queries on the same handle (the reference holds a
 * RwLock write guard, bin/server.rs:33,48).  Needs expand_queries and 3 <= t_gsw <= 32. */
sp_db_t* sp_db_create_sparse(const sp_params_t*);
/* Row shard `shard` of `num_shards` of a sparse bucket, for the multi-GPU flows: sp_db_create's shard rule (dim0 % num_shards == 0,
 * num_shards <= SP_MAX_ROW_SHARDS, rows j in [shard * dim0 / num_shards, (shard + 1) * dim0 / num_shards)) and
 * sp_db_create_sparse's parameter rule; sp_db_create_sparse(p) is (p, 0, 1).  The handle stores only the items whose row
 * j = item_idx / num_per it holds: sp_db_update_item / _items / _rows skip the others (no slot is taken, sp_db_sparse_items does not
 * count them, sp_db_update_rows counts them as applied; an index >= num_items is SP_E_ARG on every shard), so every rank can be
 * handed the same /update-row body.  sp_db_format stays "sparse", sp_db_device_bytes is the local store.  A query begun for the
 * shard (sp_query_begin_for_db) is expanded for the shard's OCCUPIED rows only -- pruning skips subtrees and changes no value --
 * and an empty shard of a non-empty bucket works (empty row set, the GSW side still expanded).  sp_query_sweep leaves the plain
 * partial [plane][r][crt][z][ii] (callers who sum themselves finish with sp_query_finish and its % q); the sp_query_sweep_scatter*
 * family and sp_process_quer{y,ies}_sharded* take the shard as they take a dense row shard, writing EVERY word of the partial
 * buffer (zeros for absent columns: the reduce-scatter sums all ranks' words) and folding with lib/server's all-zero shortcuts,
 * so rank 0's response is lib/server's process_query over the whole SparseDb.  sp_process_query, sp_process_query_batch and
 * sp_server_* answer a shard with num_shards > 1 as they answer a dense row shard (SP_E_ARG). */
sp_db_t* sp_db_create_sparse_shard(const sp_params_t*, int shard, int num_shards);
size_t sp_db_sparse_items(const sp_db_t*); /* items present */
/* A PLANAR-RESIDENT database: an unsharded handle whose only resident form is the digit-planar layout that the matrix-core
 * group pass reads, [plane][z][128-column chunk][wave g][modulus c][64-row block][tile e][digit a][lane][16 bytes] (8 bytes per
 * word, +14 % against PACKED, and no second copy): every query of every list size reads it -- 1 .. 8 queries per pass with one
 * query tile, 9 .. 16 with two -- so lists of 9 .. 16 keep their fast pass at sizes where a PACKED database has no room for
 * the copy of sp_db_prepare_batch.  Choose it where lists dominate; a single query reads 8 instead of 7 bytes per word.
 * Shapes: dim0 % 64 == 0, dim0 <= 512, num_per % 128 == 0 (else SP_E_ARG); the switches batch_planar and batch_mfma must be on
 * when it is created (else SP_E_ARG) and are not looked at again: afterwards they, batch_mfma_min and batch_mfma_tiles change
 * nothing on this handle and never free its words; SP_E_OOM when the words do not fit.  Starts as the empty bucket.
 * Loaders, upserts, sp_db_read_ref, sp_process_query, sp_query_begin / sweep / finish, sp_process_query_batch,
 * sp_bench_sweep_batch and sp_server_* work as on a PACKED handle (same bytes); sp_db_prepare_batch builds nothing and reports
 * 1, sp_db_batch_copy_bytes is 0.  The sp_query_sweep_scatter* family, sp_process_quer{y,ies}_sharded* and sp_bench_sweep[_ex]
 * refuse it with SP_E_ARG ("planar-resident"). */
sp_db_t* sp_db_create_planar(const sp_params_t*);
/* A PLANAR ROW SHARD: row shard `shard` of `num_shards` (2, 4 or 8; sp_db_create's rule: rows j in [shard * dim0 / S,
 * (shard + 1) * dim0 / S)) whose only resident form is the digit-planar layout.  It is what lets a sharded LIST take the 16-query pass:
 * sp_query_sweep_scatter_group and sp_process_queries_sharded_batched take 1 .. 16 queries per pass on it (1 .. 8 on every other
 * shard), and the pass over 16 costs about what the pass over 8 costs.  Cost: 8 bytes per word resident instead of 7, so a single
 * sharded query reads 14 % more than on a PACKED shard; choose it where lists dominate.
 * Shapes (sp_db_create_planar's rule on the LOCAL rows): nj = dim0 / S a multiple of 64 and <= 512, num_per % 128 == 0; the switches
 * batch_planar and batch_mfma must be on at creation (all else SP_E_ARG); num_shards == 1 is SP_E_ARG (use sp_db_create_planar, which
 * the sharded entry points keep refusing, G = 1 included).  sp_db_format is "planar", sp_db_device_bytes the local words at 8 bytes.
 * Resident column order: local column ii is stored at resident column (ii % S) * (num_per / S) + ii / S, so the columns that go to
 * one rank of the exchange are one contiguous run and the pass stores the reduce-scatter layout in the same 128-byte runs as the
 * plain one; sp_db_read_ref and every writer keep speaking reference coordinates.
 * sp_db_load, _load_plane, _load_items, _fill_synthetic, _update_item, _update_items, _update_rows and _read_ref work as on a dense
 * PACKED row shard: the loaders are handed full-dim0 rows and keep the shard's, upserts of rows the shard does not hold are skipped
 * (and counted as applied), so every rank takes the same /update-row body.  No buffer of the shard's size other than the planar words
 * ever exists.  Queries: sp_query_begin_for_db, then the sp_query_sweep_scatter* family (below) and sp_process_quer{y,ies}_sharded*;
 * sp_query_sweep (the plain partial) REFUSES a planar row shard (SP_E_ARG: its column order is the exchange's), and so does
 * sp_bench_sweep[_ex] ("planar-resident", as on the unsharded handle; sp_bench_sweep_scatter_group times its pass); sp_process_query,
 * sp_process_query_batch, sp_bench_sweep_batch and sp_server_* answer it as they answer any row shard (SP_E_ARG). */
sp_db_t* sp_db_create_planar_shard(const sp_params_t*, int shard, int num_shards);
/* "packed" (7-byte words), "words8" (8-byte words), "sparse" or "planar"; no device call */
const char* sp_db_format(const sp_db_t*);
void sp_db_free(sp_db_t*);
/* Upload (a z-range of) one (instance,trial) plane given in the reference layout [z][ii][j] with
 * the FULL dim0 rows per (z,ii); the shard keeps only its rows.  `words` points at row z0.
 * Equivalent of handing generate_random_db_and_get_item / load_db_from_seek /
 * load_preprocessed_db_from_file output (server.rs:223-275, 320-386) to process_query.
 * The handle keeps one device-side upload buffer (not counted by sp_db_device_bytes) from its first load on: at most 64 MiB
 * here, db_load_window (512 MiB) + one item's spill once sp_db_load_items has used it; nothing is allocated or freed between the
 * kernels of a load (allocation rule). */
int sp_db_load_plane(sp_db_t*, int plane, int z0, int nz, const uint64_t* words);
/* Whole database in one call: `words` = instances*n*n*N*num_per*dim0 u64 in the reference layout. */
int sp_db_load(sp_db_t*, const uint64_t* words, size_t n_words);
/* Build the database on the device from the raw item file: the GPU form of load_db_from_seek
 * (server.rs:320-357) over an in-memory file image.  `file` holds num_items records of db_item_size
 * bytes (a shorter file reads as zeros past its end, as the reference's failed seek/short read do);
 * each record is split into instances*n*n chunks of bytes_per_chunk bytes, log2(p)-bit coefficients,
 * recenter_mod, forward NTT, packed words -- written straight into the resident layout. */
int sp_db_load_items(sp_db_t*, const uint8_t* file, size_t file_len);
/* Upsert one item in place (the /write path: lib/server/src/db/loading.rs:317-359 update_item_raw over a
 * densified bucket; sp_db_create starts from the empty bucket = all-zero polynomials, which is what the
 * reference's SparseDb yields for absent rows).  `data` is zero-padded to db_item_size.  On a row shard
 * that does not hold the item's row the call is a no-op. */
int sp_db_update_item(sp_db_t*, size_t item_idx, const uint8_t* data, size_t len);
/* Upsert n items in one call: what n calls of sp_db_update_item(item_idx[i], data[i], lens[i]), i = 0 .. n-1 in that order, leave
 * on the handle -- a later entry for an index wins (the list is deduplicated on the host, last occurrence kept, before anything is
 * launched), a sparse bucket's new keys take their slots in order of first appearance and its store grows once, entries a row or
 * column shard does not hold are skipped.  The bytes travel through the handle's upload buffer in windows of at most
 * db_load_window bytes; per window one copy, one encode launch over all its items ((item, plane) workgroups on a sparse bucket,
 * (touched quad, plane) workgroups on a dense database), one patch launch when a digit-planar copy stands, one device
 * synchronisation.  Every index and length is checked before anything is written: SP_E_ARG leaves the handle as it was. */
int sp_db_update_items(sp_db_t*, const size_t* item_idx, const uint8_t* const* data, const size_t* lens, size_t n);
/* The body of POST /update-row (lib/server/src/bin/server.rs:31-43 -> update_many_items, db/loading.rs:361-377): records
 * be32 chunk_len | be32 item index | chunk_len - 4 item bytes, applied through sp_db_update_items.  *largest_update = the largest
 * chunk_len (the 4 index bytes included), what the reference returns (loading.rs:368-370).  Lengths: a record carries
 * 0 .. db_item_size item bytes, as sp_db_update_item; the reference's bound (update_item, loading.rs:305-310) is
 * instances * n * n * bytes_per_chunk, which is db_item_size rounded up to whole chunks: the two differ only where db_item_size
 * is not a multiple of the chunk count, and there the reference's extra bytes lie past the item.  A faulty record -- cut inside
 * its length or payload, chunk_len < 4, too long, index >= num_items -- ends the call with SP_E_ARG and a text that names the
 * record number and its byte offset; the records before it HAVE been applied and *applied is their count (the reference applies
 * while it parses and then returns Err or panics: the applied prefix is what its clients see too).  An empty body is SP_OK with
 * *applied = 0.  Records a shard skips count as applied.  applied / largest_update may be null. */
int sp_db_update_rows(sp_db_t*, const uint8_t* body, size_t body_len, size_t* applied, size_t* largest_update);
/* Synthetic benchmark database generated on the device: reference-layout word index i holds
 * sp_synth_word(seed, i).  (Roofline runs at sizes no host buffer can hold.) */
int sp_db_fill_synthetic(sp_db_t*, uint64_t seed);
/* Build now what batched calls would otherwise build inside the first sp_process_query_batch of 9 .. 16 queries: the
 * digit-planar copy of an unsharded PACKED database (8 more bytes per word) that the two-tile matrix-core pass reads --
 * when the shape has one and the device has the room (call it after the load, e.g. where bin/server.rs:98-141 has loaded
 * the database).  *built (may be null): 1 = the copy stands, 0 = this database keeps to the PACKED kernels.  The copy
 * follows sp_db_update_item in place (8 sixteen-byte entries per (plane, z)); the bulk loaders drop it. */
int sp_db_prepare_batch(sp_db_t*, int* built);
uint64_t sp_synth_word(uint64_t seed, uint64_t ref_index);
/* Read back words of the reference-layout view (debug / tests): plane, z, ii, j0..j0+count within the shard's rows */
int sp_db_read_ref(const sp_db_t*, int plane, int z, int ii, int j0, int count, uint64_t* out);
/* Items back out of the resident words, on every format: the inverse of sp_db_load_items (server.rs:277-357 load_item_from_seek /
 * load_db_from_seek) and of the upserts (lib/server/src/db/loading.rs:278-359), run on the device.  For item i = j * num_per + ii and
 * chunk c = the plane index: the 2048 resident words at (plane c, z, ii, j) are inverse-transformed mod both primes (from_ntt,
 * poly.rs:646-663), recenter_mod (server.rs:338-341) is undone -- with h = p / 2 a coefficient v <= h is x = v, v >= Q - (p - h - 1) is
 * x = v - Q + p, anything else is not in the loader's image -- and the first W = ceil(nbytes * 8 / logp) coefficients are packed back,
 * logp = ceil(log2 p) bits each, into the chunk's nbytes bytes [c * bpc, min((c + 1) * bpc, db_item_size)) of the item,
 * bpc = ceil(db_item_size / chunks) (the inverse of read_arbitrary_bits, server.rs:312-315).  Coefficients from W on and bits past the
 * chunk's bytes are ignored: where db_item_size is not a multiple of the chunk count, a file-loaded database holds the next item's
 * spill there.
 * out + k * db_item_size receives item item0 + k; present[k] (may be NULL) is 1 when this handle holds the item: a dense unsharded handle
 * holds every item (all-zero ones included), a row shard the items of its rows, a column shard those of its columns, a sparse bucket
 * or sparse shard the items in its store.  An item the handle does not hold reads as present 0 and db_item_size zero bytes.  Items
 * speak reference coordinates on every format (a planar row shard's resident column order and a column shard's local columns included).
 * A chunk polynomial with a coefficient z < W outside the loader's image is UNDECODABLE: it counts once in *undecodable (may be NULL; the
 * count over the held items of the range), that coefficient reads as 0 and the call still returns SP_OK -- what a sp_db_fill_synthetic
 * handle or arbitrary sp_db_load words yield.  count == 0: SP_OK, nothing written.  item0 + count > num_items or
 * out_cap < count * db_item_size: SP_E_ARG, nothing enqueued, nothing written.
 * Read-only: may run beside queries on the same handle and beside other readers, not beside the writers (the rule of
 * sp_db_update_item).  The handle keeps one device-side READ buffer of its own (not counted by sp_db_device_bytes) from the first read on:
 * at most db_load_window bytes (one item's words and bytes where that is smaller); a range is cut into windows of items, per window one
 * gather launch (none on a sparse store), one decode launch and one copy out; nothing is allocated or freed between the kernels of a
 * call (allocation rule).  Readers of one handle take turns at its buffer; they do not take the lock the lists hold. */
int sp_db_read_items(const sp_db_t*, size_t item0, size_t count, uint8_t* out, size_t out_cap,
                     uint8_t* present /* count bytes, may be NULL */, size_t* undecodable /* may be NULL */);
/* count * (8 + db_item_size): a body_cap that always suffices for `count` items; no device call */
size_t sp_db_export_rows_bound(const sp_db_t*, size_t count);
/* The held items of the range as the body of POST /update-row (lib/server/src/db/loading.rs:361-377 update_many_items), one record per
 * held item in index order: be32(4 + db_item_size) | be32(item index) | db_item_size item bytes.  sp_db_update_rows applies it to any
 * handle of the same Params, so dst.update_rows(src.export_rows()) moves a live bucket to another format or shard count, and the body
 * is a snapshot.  *body_len = bytes written, *records = their count (either may be NULL).  body_cap smaller than the records of the range:
 * SP_E_ARG before any device work (the held items are known from the handle's shape and key map).  When at least one polynomial of the
 * range is undecodable the call returns SP_E_STATE with *body_len = 0: an export that zeroes data silently is worse than none.
 * The one inexact case: where db_item_size is not a multiple of the chunk count, a file-loaded source (sp_db_load_items) and its
 * re-import agree on every item byte but not on the spill coefficients behind them (the records are zero padded, loading.rs:317-359) --
 * their responses decode alike, the response bytes may differ.  Threading: as sp_db_read_items. */
int sp_db_export_rows(const sp_db_t*, size_t item0, size_t count, uint8_t* body, size_t body_cap,
                      size_t* body_len, size_t* records);
/* Items from one resident database into another, on the device and word for word.  For every item i of [item0, item0 + count) that
 * `src` holds (`present` of sp_db_read_items) and that `dst`'s shape holds -- the item's row lies in a row shard's rows, its column in a
 * column shard's columns; a sparse bucket or sparse shard takes the items of its rows (sp_db_create_sparse_shard) -- dst's
 * 2048 * planes resident words of i become src's canonical words lo | hi << 32 (what sp_db_read_ref returns).  Nothing is decoded and
 * nothing is encoded again, so unlike dst.update_rows(src.export_rows()) the copy is exact where db_item_size is not a multiple of the
 * chunk count (the spill coefficients travel), it takes sp_db_fill_synthetic and arbitrary sp_db_load words, and no item byte visits
 * the host.  Items src does not hold leave dst untouched (one record per held item, the semantics of that pair of calls); a dense src
 * copies every item it holds, all-zero ones included, into a sparse dst.  Items speak reference coordinates on every format (a planar
 * row shard's resident column order and a column shard's local columns are undone or applied inside the call).  Every format to every
 * format: PACKED, 8-byte words, planar-resident, sparse, and row, column, planar and sparse shards in either role; re-sharding on one
 * device is the intersection of what the two handles hold.  A sparse dst takes new keys in index order, its store grows at most once,
 * before the call's first kernel, and an existing key is overwritten in its slot.  A PACKED dst beside which a digit-planar batch copy
 * stands (sp_db_prepare_batch) keeps the copy valid: the touched (16-row group, column) cells are regathered as after
 * sp_db_update_items.  *copied (may be NULL) = items written.  count == 0: SP_OK, nothing written.
 * SP_E_ARG, nothing enqueued and nothing written: item0 + count > num_items; a null handle; dst == src; handles made from different
 * sp_params_t handles; handles on different devices (copies across devices are out of scope).  Any other failure (SP_E_OOM, SP_E_HIP) may
 * leave dst partly updated -- the windows before the failing one are written -- but a sparse dst never keeps a key whose slot no
 * launch was issued for: new keys enter its key map window by window, behind the window's launch.
 * Threading: dst follows the writers' rule (sp_db_update_item: not beside queries or readers of dst); src follows the readers' rule
 * (sp_db_read_items: beside queries and other readers of src, taking its turn at src's read buffer and stream); a sparse src is read
 * under one host-side snapshot of its key map, and no lock of src is held across device work.
 * The staging words and the record lists live in src's read buffer, in windows of at most db_load_window bytes, sized before the first
 * kernel; per window at most one gather launch (none for a sparse src, whose store is read in place), one scatter launch and, where a
 * batch copy stands, one patch launch; nothing is allocated or freed between the kernels of a call. */
int sp_db_copy_items(sp_db_t* dst, const sp_db_t* src, size_t item0, size_t count, size_t* copied /* may be NULL */);
/* Remove items from a resident database on the device, on every format: PACKED, 8-byte words, planar-resident, sparse, and row, column,
 * planar and sparse shards.  Items speak reference coordinates on every format; indices a shard does not hold (a row or column outside
 * its shape) are skipped and not counted.  The list is deduplicated on the host: a repeated index counts once.
 * A sparse bucket or sparse shard loses the KEY: with n slots in use and m distinct listed keys present, the count becomes n - m,
 * *removed = m, absent keys are no-ops.  The store stays dense: the survivors at or above slot n - m move, in ascending order, into the
 * removed slots below it (one launch per window of the move list), sp_db_sparse_items drops by m, `present` of sp_db_read_items /
 * sp_db_item_digests becomes 0 for the removed keys, and the next query publishes a new index snapshot and pruned expansion plan
 * (queries begun earlier keep theirs).  Removal never reallocates: sp_db_device_bytes stays (sp_db_sparse_trim gives memory back).
 * After its last key is removed the bucket behaves as one fresh from sp_db_create_sparse.
 * A dense handle holds every item of its shape: the item's planes * 2048 words become the empty database's words (zero), `present`
 * stays 1, *removed = the distinct listed indices the shape holds.  Only the removed items' bytes are touched -- no staging of item
 * words, no encode; a window of the call is a record list only.  A PACKED handle beside which a digit-planar batch copy stands
 * (sp_db_prepare_batch) keeps the copy valid: the same items' bytes are cleared in the copy by a second launch of the window.
 * SP_E_ARG, nothing enqueued and the handle exactly as it was: an index >= num_items anywhere in the list, item0 + count > num_items, a
 * null handle, a null list with n > 0.  n == 0 / count == 0: SP_OK.  Any other failure (SP_E_HIP) may leave the windows before the
 * failing one applied, but a sparse bucket never keeps a key that points at a slot whose move was not issued.
 * Threading: the writers' rule of sp_db_update_item (not beside queries or readers of the handle).  The record lists travel through the
 * handle's upload buffer in windows of at most db_load_window bytes, sized before the first kernel: one copy in, one launch (two where a
 * batch copy stands) and one synchronisation per window; nothing is allocated or freed between the kernels of a call. */
int sp_db_remove_items(sp_db_t*, const size_t* item_idx, size_t n, size_t* removed /* may be NULL */);
int sp_db_remove_range(sp_db_t*, size_t item0, size_t count, size_t* removed /* may be NULL */);
/* Give a sparse bucket's unused store back: the store is reallocated to the smallest capacity its growth rule would have chosen for the
 * current count (64 * 2^k >= count, at least 64 slots) and the live slots are copied across; *freed_bytes = the difference in
 * sp_db_device_bytes, 0 (and SP_OK) when nothing shrinks.  SP_E_ARG on a handle that is not sparse.  The writers' rule. */
int sp_db_sparse_trim(sp_db_t*, size_t* freed_bytes /* may be NULL */);
/* A digest of the resident words, computed on the device in about one database pass: one pair of 64-bit sums per plane
 * (plane = instance * n^2 + trial), defined over REFERENCE coordinates, so every resident format, every shard split and a sparse bucket
 * give the same value for the same contents.  With N = 2048, w(plane, z, ii, j) the canonical word lo | hi << 32 that sp_db_read_ref
 * returns (a word the handle does not hold -- another shard's row or column, an absent item of a sparse bucket -- counts as 0) and all
 * arithmetic mod 2^64:
 *     mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^ x >> 31
 *     for lane l in {0, 1}:  s_l = mix(seed + l)
 *         A_l(c) = mix(s_l ^ c) | 1,   c = (plane * N + z) * num_per + ii        (one key per (plane, z, column))
 *         R_l(j) = mix(~s_l ^ j) | 1,  j = GLOBAL first-dimension row             (one key per row)
 *         D_l[plane] = sum over z, ii of  A_l(c) * (sum over j of R_l(j) * w(plane, z, ii, j))
 * out[2k], out[2k + 1] = (D_0, D_1) of plane plane0 + k.  The digest is linear in the words: the empty bucket digests to (0, 0), the
 * digests of the shards of a bucket (row, column, planar row, sparse), added lane by lane with wrap-around, are the unsharded digest,
 * and a sparse bucket digests like the dense one that holds the same items.  The keys are odd: changing one word changes both lanes.
 * which: SP_DIGEST_RESIDENT = the handle's resident words; SP_DIGEST_BATCH_COPY = the digit-planar copy beside a PACKED database
 * (sp_db_prepare_batch) while it stands: SP_E_STATE, `out` untouched, when no valid copy stands (also on a planar-resident or sparse
 * handle).  The call never builds a copy, and pins the one it reads as a pass does, so a concurrent drop cannot free it under the kernel.
 * plane0 < 0, plane0 + nplanes > planes, a null pointer or an unknown `which`: SP_E_ARG, nothing enqueued, nothing written.
 * nplanes == 0: SP_OK.  Works on every handle: packed, 8-byte, planar-resident, sparse and every shard kind (a row shard sums its rows
 * with the global j, a column shard its columns with the reference ii, a planar row shard undoes its column order, a sparse handle sums
 * its store under one snapshot of its key map).
 * One kernel per resident form, each reading every resident byte of the plane range once.  Read-only, threading as sp_db_read_items:
 * beside queries and other readers of the handle, not beside a writer.  It takes its turn at the handle's read buffer and stream (the
 * partial sums and the row keys live there); nothing is allocated or freed between the kernels of a call. */
#define SP_DIGEST_RESIDENT 0
#define SP_DIGEST_BATCH_COPY 1
int sp_db_digest(const sp_db_t*, uint64_t seed, int which, int plane0, int nplanes, uint64_t* out /* 2 * nplanes */);
/* The same sums on the HOST, from words in the reference layout: adds to acc[0], acc[1] the contribution of rows z0 .. z0 + nz - 1 of
 * one plane, words[z - z0][ii][j] with the full dim0 -- exactly what sp_db_load_plane takes -- after reducing both 32-bit limbs mod
 * their primes as the loaders do.  No device call: works with no GPU present.  A host that streams a database through
 * sp_db_load_plane accumulates this beside the upload and compares with sp_db_digest afterwards. */
int sp_db_digest_ref_words(const sp_params_t*, uint64_t seed, int plane, int z0, int nz, const uint64_t* words, uint64_t acc[2]);
/* Per-ITEM digests of the resident words: which items differ, where sp_db_digest says whether any does.  Computed on the device in about
 * one pass over the rows of the range, 16 bytes per item back instead of db_item_size.  The keys are those of sp_db_digest (mix, s_l,
 * A_l, R_l above), w(plane, z, ii, j) is the canonical word sp_db_read_ref returns (0 for a word the handle does not hold), all
 * arithmetic mod 2^64.  For item i = j * num_per + ii, lane l in {0, 1} and the plane range P = [plane0, plane0 + nplanes):
 *     E_l(i) = R_l(j) * sum over plane in P, z in [0, N) of  A_l((plane * N + z) * num_per + ii) * w(plane, z, ii, j)
 * out[2k], out[2k + 1] = (E_0, E_1) of item item0 + k.  Consequences: the sum over ALL items of E_l is the sum over P of sp_db_digest's
 * D_l[plane] (wrapping); an all-zero item digests to (0, 0); the tables of the shards of a bucket, added lane by lane, are the unsharded
 * table; changing one word changes both lanes of exactly one item; every resident format, the batch copy, every shard kind and a sparse
 * bucket give the same table for the same contents.
 * present[k] (may be NULL) has the meaning it has in sp_db_read_items: a dense handle holds the items of its rows and columns, all-zero
 * ones included; a sparse handle the items in its store.  An item not held reads as (0, 0) with present 0: on a sparse bucket the flag
 * is what separates "absent" from "stored and all zero".
 * which: SP_DIGEST_RESIDENT or SP_DIGEST_BATCH_COPY, with the pinning rule of sp_db_digest; the call never builds a copy and returns
 * SP_E_STATE, `out` untouched, when none stands.  count == 0 or nplanes == 0: SP_OK, nothing written.  A bad plane range,
 * item0 + count > num_items, a null `out` or an unknown `which`: SP_E_ARG, nothing enqueued, nothing written.  out and present are
 * written only once the whole call has succeeded.
 * Read-only, threading as sp_db_digest: beside queries and other readers, not beside a writer; it takes its turn at the handle's read
 * buffer and stream.  A sparse store is summed under one snapshot of its key map, taken on the host; the handle's lock is never held
 * across device work.  Everything the call needs -- the table of 16 bytes per item of a window, the row keys, a sparse window's flags
 * and slot list -- is sized before its first kernel and lives in the read buffer; nothing is allocated or freed between kernels.  A
 * range whose table would exceed db_load_window is cut into windows of whole rows (at least one row), each reading only its own rows.
 * A dense call reads the rows item0 / num_per .. (item0 + count - 1) / num_per of the plane range and nothing else -- with the
 * granularity of the resident form: the other row of a PACKED row pair, the other rows of a digit-planar 8-row half group share the
 * bytes of a requested row -- and copies out the requested items only.  One kernel per resident form; the sums of a dense form meet in
 * the table through wrapping 64-bit atomic adds, so the result does not depend on the order of arrival. */
int sp_db_item_digests(const sp_db_t*, uint64_t seed, int which, int plane0, int nplanes, size_t item0, size_t count,
                       uint64_t* out /* 2 * count: E_0, E_1 per item */, uint8_t* present /* count bytes, may be NULL */);
/* The same table on the HOST, from words in the reference layout: adds into acc[2 * i + l], i = j * num_per + ii over ALL num_items
 * items, the contribution of rows z0 .. z0 + nz - 1 of one plane, words[z - z0][ii][j] with the full dim0 -- what sp_db_load_plane
 * takes -- after reducing both 32-bit limbs mod their primes as the loaders do.  No device call.  A host that streams a database
 * through sp_db_load_plane accumulates the table beside the upload.  Bad coordinates or a null pointer: SP_E_ARG, acc untouched.
 * nz == 0: SP_OK. */
int sp_db_item_digests_ref_words(const sp_params_t*, uint64_t seed, int plane, int z0, int nz, const uint64_t* words,
                                 uint64_t* acc /* 2 * num_items */);
size_t sp_db_device_bytes(const sp_db_t*);      /* the resident database words */
size_t sp_db_batch_copy_bytes(const sp_db_t*);  /* the digit-planar copy beside them while it stands (sp_db_prepare_batch), else 0 */

/* ------------------------------------------------------- PublicParameters
 * client.rs:212-259 PublicParameters::deserialize(params, data): 32-byte seed, row 0 of every
 * matrix regenerated as Q - (ChaCha20Rng(seed).gen::<u64>() % Q) (client.rs:47-49, 68-75), other
 * rows read as LE u64, everything NTT'd and kept device-resident.  len must equal setup_bytes. */
sp_pp_t* sp_pp_deserialize(const sp_params_t*, const uint8_t* data, size_t len);
void sp_pp_free(sp_pp_t*);
/* NTT-form matrices in wire order, ref layout (tests): v_packing[n], v_expansion_left[g],
 * v_expansion_right[stop_round+1] (if present on the wire), v_conversion[1]. */
int sp_pp_export(const sp_pp_t*, uint64_t* out, size_t cap_words, size_t* n_words);
/* What an expanded handle keeps on the device: the NTT-form matrices, their wave-layout twin (where the params expand queries) and
 * the concatenated packing matrices.  The same for a handle of sp_pp_deserialize and of sp_pp_expand. */
size_t sp_pp_device_bytes(const sp_pp_t*);

/* The COMPACT form of a client's public parameters: the wire image itself, uploaded and kept on the device (row 0 of every matrix is
 * the 32-byte seed, the other rows are the client's words), about a quarter of what the expanded handle holds.  len must equal
 * setup_bytes: checked before any device work.  sp_pp_compact uploads and does nothing else; nothing is validated beyond the length,
 * as in sp_pp_deserialize (words >= Q stay as sent). */
sp_ppc_t* sp_pp_compact(const sp_params_t*, const uint8_t* data, size_t len);
void sp_ppc_free(sp_ppc_t*);
size_t sp_ppc_device_bytes(const sp_ppc_t*); /* the image: setup_bytes, rounded up to the allocation's granule */
/* The device-side inverse of the wire format (k_pp_raw_image: ChaCha20 keystream, Q - (ks % Q), the wire's rows; then the forward
 * transform and the two derived layouts, the launches of sp_pp_deserialize): a fresh handle, word for word the one
 * sp_pp_deserialize builds from the same bytes, taken by every entry point that takes that one. */
sp_pp_t* sp_pp_expand(const sp_ppc_t*);
/* The same INTO an expanded handle of the same params and device (from sp_pp_deserialize or sp_pp_expand), overwriting the client it
 * held: nothing is allocated or freed on the device (the raw image is staged in a buffer the library keeps per params and device),
 * and the call waits for its own work only.  The caller sees to it that no query that reads `slot` is in flight.  A slot of other
 * params or of another device, or a null argument: SP_E_ARG, the slot is as it was. */
int sp_pp_expand_into(const sp_ppc_t*, sp_pp_t* slot);

/* ---------------------------------------------------------- process_query
 * server.rs:650-741 process_query(params, public_params, query, db) -> Vec<u8>, with
 * Query::deserialize (client.rs:303-329) folded in.  `query` is the 32-byte seed followed by the
 * serialized query body (query_bytes long).  Requires a db created with num_shards == 1.
 * out must hold response_bytes. */
int sp_process_query(const sp_params_t*, const sp_pp_t*, const uint8_t* query, size_t query_len,
                     const sp_db_t*, uint8_t* out, size_t out_cap, size_t* out_len);
/* The per-request loop of lib/server (bin/server.rs:152-158: process_query for every query of the list) as one call: the
 * responses are those of `batch` sp_process_query calls, out + i * out_stride each.  On an unsharded PACKED database the
 * queries share database passes in groups -- up to 8 per pass, up to 16 where the two-tile matrix-core pass applies (which
 * reads the digit-planar copy of the database when one stands: sp_db_prepare_batch) -- with the next group's expansions
 * queued behind the current group's folds; on 8-byte (narrow) databases it is one pass per query with up to three queries
 * in flight on their own streams -- except that on an unsharded 8-byte database with 2 <= num_per <= 64 the list is cut into groups
 * of 8 and a group of at least `narrow_batch_min` members (sp_debug_set / SPIRAL_NARROW_BATCH_MIN; shipped 0, 0 = never, negative =
 * the shipped value) takes the PACKED flow with ONE pass over the database (k_sweep_narrow_batch), a last group below the threshold and
 * a trailing single query staying per query.  On a sparse bucket (sp_db_create_sparse) the list is cut into groups of at most 8, and a
 * group of at least `sparse_batch_min` members (sp_debug_set / SPIRAL_SPARSE_BATCH_MIN; shipped 2, 0 = never, negative = the shipped value) shares ONE pass over the
 * bucket's present items under one snapshot of its index, each member with its own pruned expansion and its own fold; smaller
 * groups and a trailing single query are answered per query as on 8-byte databases.  Out of memory is handled inside the call (the planar copy is given back, then groups of
 * 8 one at a time, then one query at a time) before it is reported. */
int sp_process_query_batch(const sp_params_t*, const sp_pp_t* const* pps, const uint8_t* const* queries,
                           const size_t* query_lens, int batch, const sp_db_t*, uint8_t* out,
                           size_t out_stride, size_t* out_len);

/* Multi-GPU split of process_query around the one exchange step (sum of per-shard partial
 * first-dimension outputs):
 *   begin  : Query::deserialize + expand_query + get_v_folding_neg     (server.rs:664-680; G - C itself is not materialised:
 *            every fold step of the library is the delta form, which reads C only -- DESIGN.md section 3)
 *   sweep  : multiply_reg_by_database over this shard's rows             (server.rs:698-705)
 *            -> partial residues (u32, < q) at sp_query_partial_ptr(), layout
 *               [plane][r][crt][z][ii], sp_query_partial_words() u32 words; DEVICE memory
 *   ...    : caller sums the partial buffers of all shards element-wise (RCCL ncclSum on u32;
 *            8 shards * (q-1) < 2^31) and, on the rank that finishes, writes the sum back.
 *   finish : % q, from_ntt, fold_ciphertexts, pack, encode                (server.rs:707-740)
 * All three enqueue on the query's HIP stream; sp_query_sync() waits for it. */
/* Distributed-fold variant (what bench.py uses for N > 1), G = number of row shards = ranks, a power of two:
 *   sweep_scatter : as sweep, but the partial buffer is column-interleaved: chunk g (contiguous,
 *                   partial_words/G u32) holds columns ii = g mod G as [plane][r][crt][z][ii / G]
 *   ...           : caller reduce-scatters the partial buffers (RCCL ncclSum, u32): rank g receives chunk g
 *   fold_local    : % q, from_ntt and the top nu_2 - log2(G) fold levels on this rank's columns
 *                   -> planes 2x1 raw cts at sp_query_local_cts_ptr() (DEVICE, local_cts_words u64)
 *   ...           : caller gathers the G local results on the finishing rank: [g][plane][2][N]
 *   finish_gathered: the last log2(G) fold levels (leaf g = rank g), pack, encode.
 * On a sparse row shard (sp_db_create_sparse_shard) the sweeps multiply the shard's present items only, under the snapshot the
 * query was begun on, and fold_local* / finish_gathered take the all-zero shortcuts of lib/server's fold (fold.rs:38-44).
 * On a planar row shard (sp_db_create_planar_shard) sweep_scatter and sweep_scatter_plane run the group pass of
 * sp_query_sweep_scatter_group for a group of one (k_sweep_planar_scatter, one query tile; _plane launches that plane's z-range) and
 * leave the same words as on a PACKED shard of the same content. */
int sp_query_sweep_scatter(sp_query_t*, const sp_db_t*, int G);
/* The same sweep one (instance, trial) plane per launch, planes in order 0 .. planes-1.  Plane p's region of the
 * partial buffer ([p * partial_words/planes, (p+1) * partial_words/planes)) is laid out [g][r][crt][z][ii / G], so
 * each plane can be reduce-scattered on its own, overlapping the exchange of plane p with the sweep of plane p+1;
 * the concatenation of the received chunks is the [plane][r][crt][z][ii / G] buffer sp_query_fold_local takes. */
int sp_query_sweep_scatter_plane(sp_query_t*, const sp_db_t*, int G, int plane);
/* ALL planes for a GROUP of 1 .. 8 queries begun for this row shard (sp_query_begin_for_db) with ONE pass over the shard's
 * rows: afterwards every sp_query_partial_ptr(qs[i]) holds, word for word, what `planes` calls of
 * sp_query_sweep_scatter_plane(qs[i], shard, G, p) would have left, and sp_query_fold_local / sp_query_finish_gathered take
 * over unchanged.  The pass runs on qs[0]'s stream, ordered after every query's expansion; each query's own stream is
 * ordered after the pass.  From 4 queries on PACKED shards with whole 32-row blocks (G = 2, 4, 8) it is one launch of the
 * matrix-core kernel in its scatter form (path bits scatter_out, sweep_batch, sweep_batch_mfma, sweep_batch_scatter); every
 * other group or shape is swept per query inside the same call (the bit sweep_batch_scatter stays clear).  SP_E_ARG, nothing
 * enqueued: column-sharded or unsharded handle with G > 1, G != the handle's shard count, a query begun for other
 * params / rows or not in the 'begun' state.
 * On a sparse row shard (sp_db_create_sparse_shard): a group of 2 .. 8 members that hold ONE snapshot of the shard's index and
 * reach `sparse_batch_min` shares one pass over the shard's items (k_sweep_sparse_scatter_batch; path bits sweep_sparse,
 * scatter_out, sparse_group_pass); a group of 1, members begun either side of an upsert, or sparse_batch_min = 0 are swept per
 * query with their own snapshots inside the same call (sweep_sparse, scatter_out) -- the same words either way.
 * On a planar row shard (sp_db_create_planar_shard): 1 .. 16 queries per pass (1 .. 8 where the device does not offer two query
 * tiles' tables, nj * 256 bytes of LDS, to one workgroup; batch > 8 on any other shard stays SP_E_ARG), always ONE launch of
 * k_sweep_planar_scatter -- one query tile for 1 .. 8, two for 9 .. 16.  Path bits: scatter_out, sweep_batch, sweep_batch_mfma,
 * sweep_batch_planar, plus sweep_batch_mfma_two_tiles for 9 .. 16 -- no other flow reports scatter_out together with
 * sweep_batch_planar; sweep_batch_scatter stays clear (it names the PACKED shards' k_sweep_mfma_scatter). */
int sp_query_sweep_scatter_group(sp_query_t* const* qs, int batch, const sp_db_t* shard, int G);
int sp_query_fold_local(sp_query_t*, const void* reduced_chunk_dev, int G);
/* The local fold one plane at a time on the query's SECOND stream (sp_query_stream2), planes in order: plane p may
 * be folded as soon as it has been swept and its reduced chunk ([r][crt][z][ii / G]) is complete — the caller orders
 * stream2 after that exchange — so the fold of plane p runs beside the sweep / exchange of the later planes.
 * sp_query_fold_local_join() orders the main stream after all of them (replaces sp_query_fold_local). */
int sp_query_fold_local_plane(sp_query_t*, const void* reduced_plane_chunk_dev, int G, int plane);
int sp_query_fold_local_join(sp_query_t*);
void* sp_query_stream2(sp_query_t*);
void* sp_query_local_cts_ptr(sp_query_t*);
size_t sp_query_local_cts_words(const sp_query_t*);
int sp_query_finish_gathered(sp_query_t*, const void* gathered_dev, int G, uint8_t* out, size_t out_cap, size_t* out_len);
sp_query_t* sp_query_begin(const sp_params_t*, const sp_pp_t*, const uint8_t* query, size_t query_len);
/* The same for a query that will sweep `db`: on a row shard only the first-dimension ciphertexts of the shard's
 * rows are expanded (the even subtree of coefficient_expansion is pruned to their ancestors; server.rs:58-111 is
 * otherwise unchanged, the GSW side is complete).  The sweep calls then insist on a database with those rows.
 * db == NULL, unsharded or column-sharded: identical to sp_query_begin. */
sp_query_t* sp_query_begin_for_db(const sp_params_t*, const sp_pp_t*, const uint8_t* query, size_t query_len,
                                  const sp_db_t* db);
/* (a planar row shard, sp_db_create_planar_shard, is refused with SP_E_ARG: it has the scatter-form sweeps only) */
int sp_query_sweep(sp_query_t*, const sp_db_t*);
void* sp_query_partial_ptr(sp_query_t*);
size_t sp_query_partial_words(const sp_query_t*);
int sp_query_sync(sp_query_t*);
int sp_query_finish(sp_query_t*, uint8_t* out, size_t out_cap, size_t* out_len);
void sp_query_free(sp_query_t*);
/* HIP stream (hipStream_t) the query's work is enqueued on -- for event timing by the caller. */
void* sp_query_stream(sp_query_t*);
/* Stage timings of the last finish()ed query in milliseconds (HIP events on the query stream):
 * [0] expand+conversion+folding_neg, [1] db sweep, [2] from_ntt+fold, [3] pack+encode(+D2H). */
int sp_query_timings(const sp_query_t*, float* ms4);

/* ----------------------------------------------------------------- multi-GPU, collectives inside the library
 * One process per GPU, the database row-sharded (sp_db_create(params, rank, world)).  The reference has no
 * multi-node / multi-device code (it is CPU-only); the caller this serves is lib/server's request handler
 * (lib/server/src/bin/server.rs:98-141), which would call sp_process_query_sharded where it calls process_query
 * (server.rs:650-655) today -- on every rank, with the same query bytes; rank 0 gets the response.
 * Built-in transport: RCCL (librccl linked directly): ncclReduceScatter(ncclUint32, ncclSum) of each plane's partial
 * Regev ciphertexts on the communicator's own stream while the next plane is swept, then ncclAllGather(ncclUint64)
 * of one locally folded ciphertext per plane per rank.  world must be a power of two <= SP_MAX_ROW_SHARDS.
 *   rank 0   : sp_comm_unique_id(id)  -> hand the SP_COMM_ID_BYTES bytes to every rank (any side channel)
 *   all ranks: sp_comm_create(rank, world, id)   (collective: returns when every rank has joined)
 * One sharded query at a time per communicator (calls are serialised inside; every rank must issue them in the
 * same order).  *out_len = 0 on ranks other than 0. */
typedef struct sp_comm sp_comm_t;
#define SP_COMM_ID_BYTES 128
int sp_comm_unique_id(uint8_t* id128);
sp_comm_t* sp_comm_create(int rank, int world, const uint8_t* id128);
/* Custom transport: the host supplies the two collectives (its own RCCL/MPI setup, or an in-process loopback for
 * tests).  Both are ENQUEUE operations on `hip_stream` (hipStream_t): they must order their device work after what
 * is already on that stream and must not block the host on it.  Return 0 on success.
 *   reduce_scatter_u32: send = world chunks of recv_count u32 each; recv (recv_count u32) = element-wise sum over
 *                       ranks of chunk[rank]                      (ncclReduceScatter semantics)
 *   all_gather_u64    : recv = world blocks of send_count u64, block g = rank g's send   (ncclAllGather semantics) */
typedef struct sp_comm_ops {
  int (*reduce_scatter_u32)(void* user, const void* send, void* recv, size_t recv_count, void* hip_stream);
  int (*all_gather_u64)(void* user, const void* send, void* recv, size_t send_count, void* hip_stream);
  void* user;
} sp_comm_ops_t;
sp_comm_t* sp_comm_create_custom(int rank, int world, const sp_comm_ops_t* ops);
void sp_comm_free(sp_comm_t*);
int sp_comm_rank(const sp_comm_t*);
int sp_comm_world(const sp_comm_t*);
void* sp_comm_stream(sp_comm_t*); /* hipStream_t the collectives are enqueued on */
int sp_comm_barrier(sp_comm_t*);  /* one tiny all-gather + host wait: every rank has reached this call */
/* process_query (server.rs:650-741) over a row-sharded database; `shard` = this rank's sp_db_create(params, rank,
 * world) -- or sp_db_create_sparse_shard / sp_db_create_planar_shard(params, rank, world): the same bytes.  Byte-identical to
 * sp_process_query over the unsharded database.  A planar row shard of another shard count than the communicator's world is
 * SP_E_ARG before anything is enqueued (here and in the two list calls). */
int sp_process_query_sharded(sp_comm_t*, const sp_params_t*, const sp_pp_t*, const uint8_t* query, size_t query_len,
                             const sp_db_t* shard, uint8_t* out, size_t out_cap, size_t* out_len);
/* The same for a LIST of queries (what a /private-read request carries, lib/server/src/bin/server.rs:152-158),
 * software-pipelined: query k + 1 is deserialised and expanded while query k's planes are swept and exchanged, so the
 * replicated expansion leaves the per-query critical path.  Every rank passes the same list; response k is written at
 * out + k * out_stride on rank 0 (out_stride >= response_bytes), *out_len = response_bytes there and 0 elsewhere.
 * Byte-identical to n calls of sp_process_query_sharded. */
int sp_process_queries_sharded(sp_comm_t*, const sp_params_t*, const sp_pp_t* const* pps, const uint8_t* const* queries,
                               const size_t* query_lens, int n, const sp_db_t* shard, uint8_t* out, size_t out_stride,
                               size_t* out_len);
/* The same list with the DATABASE PASS SHARED inside groups of up to 8 queries: per group, `B` pruned expansions, one
 * sp_query_sweep_scatter_group over the rank's shard, then per query (in list order) `planes` reduce_scatter_u32 into that
 * query's region of the rank's receive buffer, and per query (in list order) sp_query_fold_local, all_gather_u64 and, on rank
 * 0, sp_query_finish_gathered.  group: 1 .. 8, or 0 = the library's choice (8 where the scatter-form pass applies to the
 * shard, else the per-query flow of sp_process_queries_sharded).  The sequence of collectives is a function of (n, group,
 * params, shard shape) alone, so every rank issues the same one.  Every query's length is checked before anything is begun:
 * a bad list enters no collective.  Same outputs and the same bytes as sp_process_queries_sharded.
 * On a planar row shard (sp_db_create_planar_shard) group is 1 .. 16, and 0 = 16 where the shard's shape allows two query tiles
 * (nj * 256 bytes of LDS per workgroup), otherwise 8; group > 8 on any other shard stays SP_E_ARG.  (The out-of-memory ladder of
 * sp_process_query_batch is NOT part of this call: a rank that stepped its group size down alone would issue another sequence of
 * collectives than its peers.  SP_E_OOM is returned; reserve with sp_comm_reserve_batch_for up front.) */
int sp_process_queries_sharded_batched(sp_comm_t*, const sp_params_t*, const sp_pp_t* const* pps, const uint8_t* const* queries,
                                       const size_t* query_lens, int n, const sp_db_t* shard, int group, uint8_t* out,
                                       size_t out_stride, size_t* out_len);
/* sp_comm_reserve plus the receive / gather buffers and events of a group of `group` (1 .. 8; 0 = 8) queries. */
int sp_comm_reserve_batch(sp_comm_t*, const sp_params_t* params, int group);
/* The same for the groups a batched list takes on `shard`: group 1 .. the shard's largest (16 on a planar row shard whose shape
 * allows two query tiles, else 8), 0 = that largest; beyond it SP_E_ARG. */
int sp_comm_reserve_batch_for(sp_comm_t*, const sp_params_t* params, const sp_db_t* shard, int group);
/* Allocates the communicator's exchange buffers and events for `params` now, so that no sharded query allocates
 * anything (otherwise the first query with new params does).  Not a collective. */
int sp_comm_reserve(sp_comm_t*, const sp_params_t* params);
/* milliseconds of the last sharded query on this rank (HIP events): [0] the per-plane sweep launches (the exchanges of
 * the earlier planes run beside them), [1] exchange tail + local fold + all-gather, [2] the part of the exchange that is NOT
 * hidden behind the sweeps: last sweep launch done -> last plane's reduce-scatter done (exchange stream) */
int sp_comm_timings(const sp_comm_t*, float* ms3);
/* One line of JSON into buf: transport ("rccl" / "custom"), RCCL version, rank / world / device, bytes one rank sends and
 * receives per plane reduce-scatter and in the all-gather, the three sp_comm_timings values.  For the logs of a first run on a
 * multi-GPU node (the reference has no multi-device code; bench.py --gpus N prints it per rank). */
int sp_comm_describe(const sp_comm_t*, char* buf, size_t cap);

/* ------------------------------------------------------ request layer (lib/server's binary without the HTTP transport)
 * ServerState of lib/server/src/bin/server.rs:21-28: the params, the resident database and the
 * RwLock<HashMap<uuid, PublicParameters>> that POST /setup fills and POST /private-read consults.  `params` and `db` are
 * borrowed and must outlive the handle.  All entry points may be called concurrently from several host threads; writes to the
 * database while the server answers go through sp_server_update_row. */
typedef struct sp_server sp_server_t;
sp_server_t* sp_server_create(const sp_params_t* params, const sp_db_t* db);
void sp_server_free(sp_server_t*);
size_t sp_server_clients(const sp_server_t*); /* registered public-parameter sets */
/* POST /setup (bin/server.rs:71-94) after base64 decoding: deserialize (length must be setup_bytes), NTT, keep resident
 * under a fresh UUIDv4; uuid_out37 receives the 36 characters + NUL. */
int sp_server_setup(sp_server_t*, const uint8_t* pp_bytes, size_t len, char* uuid_out37);
/* The same on the HTTP body: a JSON string holding base64(public parameters); out = {"uuid":"..."} (NUL-terminated). */
int sp_server_setup_json(sp_server_t*, const char* body, size_t body_len, char* out, size_t out_cap, size_t* out_len);
/* Drop a client's public parameters (not in the reference, which never evicts). SP_E_NOTFOUND for an unknown uuid. */
int sp_server_forget(sp_server_t*, const char* uuid);
/* POST /private-read (bin/server.rs:98-164) on decoded requests: request i is uuid (36 bytes) || serialized query when
 * the params expand queries (bin/server.rs:107-121), serialized public parameters || query otherwise (:123-138).  The
 * reference answers the list one query at a time (:152-158); here the whole list goes through the batch scheduler
 * (sp_process_query_batch: groups of <= 16 queries (two tiles of 8 on the matrix cores; <= 8 elsewhere) share one pass over the database, each with its own client's public
 * parameters).  Response i (response_bytes long) is written at out + i * out_stride.  A malformed length is SP_E_ARG
 * (the reference asserts), an unknown uuid SP_E_NOTFOUND; nothing is answered in either case. */
int sp_server_private_read(sp_server_t*, const uint8_t* const* requests, const size_t* request_lens, int n, uint8_t* out,
                           size_t out_stride, size_t* out_lens);
/* The same on the HTTP body: JSON list of base64 strings in, JSON list of base64 strings out (NUL-terminated; the text
 * serde_json / the base64 crate produce: no spaces, standard alphabet, padding). */
int sp_server_private_read_json(sp_server_t*, const char* body, size_t body_len, char* out, size_t out_cap, size_t* out_len);
size_t sp_server_private_read_json_bound(const sp_server_t*, int n_queries); /* out_cap that always suffices */
/* POST /update-row (bin/server.rs:31-43) on the raw body: sp_db_update_rows on the server's database under the write side of the
 * server's reader-writer lock for it (RwLock<SparseDb>, bin/server.rs:24,35); sp_server_private_read[_json] hold the read side
 * (:102) for their whole list, so a list is answered from the bucket before or after a body, never from the middle of one.  `db`
 * must be the handle the server was created on (sp_server_create took it const): any other is SP_E_ARG.  out = the reference's
 * reply {"status":"done updating", "loading_time_us":N, "largest_update":M} (NUL-terminated; 128 bytes always suffice).  A faulty
 * record: sp_db_update_rows' status and text, the prefix applied, nothing written to out. */
int sp_server_update_row(sp_server_t*, sp_db_t* db, const uint8_t* body, size_t body_len, char* out, size_t out_cap, size_t* out_len);
/* Switch a running server to another database handle -- a bucket moved to another format with sp_db_copy_items, say -- under the write
 * side of the same lock: lists in flight hold the read side, so a list is answered wholly from the old or wholly from the new handle.
 * `new_db` must be from the server's params, on the device of the handle it replaces, and unsharded: SP_E_ARG otherwise, and the
 * server stays as it was.  Afterwards sp_server_update_row insists on new_db.  The old handle stays the caller's to free; new_db is
 * borrowed as sp_server_create borrows. */
int sp_server_replace_db(sp_server_t*, const sp_db_t* new_db);
/* sp_db_remove_items on the server's database under the write side of the same lock: a list in flight is answered wholly before or
 * wholly after the removal.  `db` must be the handle the server serves now (sp_server_create, sp_server_replace_db): any other is
 * SP_E_ARG.  *removed (may be NULL) as sp_db_remove_items. */
int sp_server_remove_items(sp_server_t*, sp_db_t* db, const size_t* item_idx, size_t n, size_t* removed);
/* Compact client registry.  max_expanded = 0 (the default): every client is expanded at /setup and stays so until it is forgotten.
 * max_expanded = k > 0 (only while the server has no clients, else SP_E_ARG): /setup keeps the COMPACT handle (sp_pp_compact) only, and
 * the server owns at most k expanded slots, allocated on first use and kept until sp_server_free.  /private-read, per distinct uuid
 * of its list: an expanded client is a HIT (its slot is pinned for the request and becomes the most recently used); otherwise a MISS
 * takes an unallocated slot, else the least recently used unpinned one (an EVICTION), and expands into it (sp_pp_expand_into); when
 * every slot is pinned by this or a concurrent request the client is expanded into a temporary handle that lives for the request (an
 * OVERFLOW): a request never fails because of k.  sp_server_forget drops the compact image; the client's slot is free once unpinned.
 * Direct-upload params with k > 0: the public parameters of a request element are copied into the slot's own wire buffer
 * (setup_bytes, kept) and expanded into the slot; elements beyond the free slots overflow; sp_server_clients stays 0. */
int sp_server_set_expanded_clients(sp_server_t*, size_t max_expanded);
/* out: registered clients, clients expanded now, hits, misses, evictions, overflows, device bytes of all compact images plus all
 * allocated slots.  With max_expanded = 0 registered == expanded and the bytes are those of the expanded handles. */
int sp_server_client_stats(const sp_server_t*, uint64_t out[7]);

/* Stand-alone timed sweep for the roofline measurement: issues the db-sweep launches of one query over `db`
 * (the same kernel and launch shapes sp_process_query uses) `iters` times with the query slice of `q`, HIP events
 * on the launch stream around the whole batch; returns average milliseconds per kernel launch in *ms_per_launch.
 * sp_sweep_launches() = kernel launches per query sweep (a wide single-GPU database is swept one launch per plane, so
 * that the from_ntt and the fold of what has been swept overlap the rest of the sweep; 1 otherwise). */
int sp_sweep_launches(const sp_params_t*, const sp_db_t*);
int sp_bench_sweep(sp_query_t* q, const sp_db_t* db, int iters, float* ms_per_launch);
/* per_plane_launches: 1 = one launch per plane (what sp_query_sweep_scatter_plane issues), 0 = one launch,
 * -1 = what sp_query_sweep would do for this db (sp_bench_sweep). */
int sp_bench_sweep_ex(sp_query_t* q, const sp_db_t* db, int iters, int per_plane_launches, float* ms_per_launch);
/* The same for the BATCHED pass of sp_process_query_batch (BASELINE configs[4]): the `batch` (<= 16 where the two-tile pass applies, else <= 8) begun queries `qs`
 * share database passes exactly as a group of sp_process_query_batch does (query digit table + k_sweep_mfma_batch on
 * the matrix cores from 4 queries, k_sweep_packed_batch below; one launch over all planes); returns average
 * milliseconds per PASS.  The queries' partial buffers hold the pass's outputs afterwards.  On a sparse bucket: the group's
 * one pass (k_sweep_sparse_batch) for 1 .. 8 queries begun for that bucket (sp_query_begin_for_db) on one snapshot of its index;
 * an unsharded 8-byte database with 2 <= num_per <= 64: the group's one pass (k_sweep_narrow_batch) for 2 .. 8 begun queries. */
int sp_bench_sweep_batch(sp_query_t* const* qs, int batch, const sp_db_t* db, int iters, float* ms_per_pass);
/* ... and for the pass of sp_query_sweep_scatter_group over a row shard (queries begun for it): layout 1 = the scatter-form
 * pass as the group call launches it, 0 = the existing one-tile pass over the same rows writing the plain [z][ii] layout
 * (comparison only: what the interleaved stores cost).  SP_E_ARG where the group call would sweep per query.
 * On a sparse row shard (queries begun on one snapshot): layout 1 = k_sweep_sparse_scatter (one query, every plane in one launch)
 * or k_sweep_sparse_scatter_batch (2 .. 8), layout 0 = k_sweep_sparse / k_sweep_sparse_batch over the same items.
 * On a planar row shard: layout 1 = k_sweep_planar_scatter for 1 .. 16 queries (tables + pass); layout 0 is SP_E_ARG (the plain
 * form over `nj` rows is sp_bench_sweep_batch on an unsharded planar database of that many rows). */
int sp_bench_sweep_scatter_group(sp_query_t* const* qs, int batch, const sp_db_t* shard, int G, int layout, int iters,
                                 float* ms_per_pass);

/* Diagnostics: where workgroups land.  `blocks` 64-thread workgroups are launched on a stream whose CU mask has bits
 * [bit_lo, bit_hi) set (no mask when bit_hi <= bit_lo); out2[2b] = HW_REG_XCC_ID, out2[2b+1] = HW_REG_HW_ID of
 * workgroup b.  Used to verify the CU partition of the fold / sweep overlap (SPIRAL_CU_SPLIT). */
int sp_debug_cu_probe(int bit_lo, int bit_hi, int blocks, uint32_t* out2);
/* Diagnostic: checksums of the resident tables / index lists / public parameters as seen by a kernel, by a
 * device-to-host copy, by a kernel after an L2 write-back + invalidate, and of the host original (24 values). */
int sp_debug_resident_check(const sp_params_t* params, const sp_pp_t* pp, uint64_t* out, int cap);
/* The library's ChaCha20 keystream as u64 words (rand_chacha 0.3.1 ChaCha20Rng::from_seed(seed).gen::<u64>(), client.rs:47-49:
 * what regenerates row 0 of the public parameters and of a query; no GPU needed): tests compare it with the RFC 8439-pinned
 * restatement word for word, on lengths that exercise the eight-block AVX2 body and the one-block tail. */
int sp_debug_chacha20_u64(const uint8_t seed[32], uint64_t* out, size_t count);
/* The same stream from the DEVICE's generator (k_pp_raw_image, what sp_pp_expand regenerates row 0 with): words first_word ..
 * first_word + count - 1; first_word % 8 == 0 (a ChaCha block is 8 words), any count, 0 included.  Needs a GPU. */
int sp_debug_chacha20_u64_device(const sp_params_t*, const uint8_t seed[32], size_t first_word, uint64_t* out, size_t count);

/* Profiling aid: nanoseconds per 2048-point forward NTT of the transform core alone (M = 1, 2 or 4 coefficient
 * vectors per thread, `blocks` workgroups each chaining `reps` transforms, no memory traffic but twiddles). */
int sp_bench_ntt(const sp_params_t*, int M, int blocks, int reps, float* ns_per_ntt);

/* ------------------------------------------------------------ stage level
 * 1:1 with the reference's pub functions, operating on caller-owned host arrays in ref layout.
 * These exist for parity tests and for callers (lib/server) that drive stages themselves.
 *
 * Operand contract.  Operands in NTT form (one residue below its prime per word) must be canonical, < q: the reference's own
 * pointwise code wraps a u64 on larger words, so there is no defined answer to match.  Raw coefficients, wire words and
 * database words (lo | hi << 32) may be ANY u64 wherever the reference is exact for them: to_ntt reduces every word mod both
 * primes; the database loaders and sp_multiply_reg_by_database reduce both 32-bit limbs of `db` and of `v_firstdim` (the
 * reference sums their products in u128, server.rs:186-217: same residues).  tests/test_gpu_crafted_inputs.py holds the
 * exports to this. */

/* ntt.rs:67-113 / 212-258: in-place forward / inverse negacyclic NTT of `count` polys (crt*N each) */
int sp_ntt_forward(const sp_params_t*, uint64_t* data, size_t count);
int sp_ntt_inverse(const sp_params_t*, uint64_t* data, size_t count);
/* poly.rs:613-638 to_ntt / to_ntt_no_reduce: raw[count][N] -> ntt[count][crt*N] */
int sp_to_ntt(const sp_params_t*, const uint64_t* raw, uint64_t* out, size_t count);
/* poly.rs:646-663 from_ntt: ntt[count][crt*N] -> raw[count][N] (iNTT + CRT compose, params.rs:207-214) */
int sp_from_ntt(const sp_params_t*, const uint64_t* ntt, uint64_t* out, size_t count);
/* poly.rs:437-458 multiply: res[ar x bc] = a[ar x ac] * b[ac x bc] (NTT form) */
int sp_multiply(const sp_params_t*, const uint64_t* a, size_t ar, size_t ac, const uint64_t* b, size_t bc,
                uint64_t* res);
/* poly.rs:483-498 add, :500-512 add_into, :575-588 scalar_multiply over `count` NTT polynomials (2 * 2048 words each;
 * `scalar` is one polynomial): res = a + b; res += a; res = scalar * b, all pointwise mod the two primes.  The reference's
 * add does not re-reduce a sum below 2 q of canonical inputs differently from these: inputs are reduced mod q first. */
int sp_add(const sp_params_t*, const uint64_t* a, const uint64_t* b, size_t count, uint64_t* res);
int sp_add_into(const sp_params_t*, uint64_t* res, const uint64_t* a, size_t count);
int sp_scalar_multiply(const sp_params_t*, const uint64_t* scalar, const uint64_t* b, size_t count, uint64_t* res);
/* poly.rs:539-551 automorph on `count` raw polys (x -> x^t, sign flip Q - a, Q for a == 0) */
int sp_automorph(const sp_params_t*, const uint64_t* a, size_t count, size_t t, uint64_t* res);
/* gadget.rs:34-60 gadget_invert_rdim followed by to_ntt_no_reduce is what the pipeline uses; this
 * export returns the raw digits: inp[rows_in x cols] -> out[rows_out x cols] */
int sp_gadget_invert_rdim(const sp_params_t*, const uint64_t* inp, size_t rows_in, size_t cols, uint64_t* out,
                          size_t rows_out, size_t rdim);
/* util.rs:323-355 reorient_reg_ciphertexts: v_reg[dim0] 2x1 NTT -> out[N*dim0*2] packed lo|hi<<32 */
int sp_reorient_reg_ciphertexts(const sp_params_t*, const uint64_t* v_reg, uint64_t* out);
/* server.rs:155-221 multiply_reg_by_database: db = one plane [N][num_per][dim0] (ref layout),
 * v_firstdim = [N][dim0][2]; out = num_per 2x1 NTT cts (ref layout, out[i].data[r*2N + crt*N + z]).  Limbs of either
 * operand may be anything up to 2^32 - 1 (both are reduced on upload). */
int sp_multiply_reg_by_database(const sp_params_t*, const uint64_t* db, const uint64_t* v_firstdim, size_t dim0,
                                size_t num_per, uint64_t* out);
/* server.rs:19-121 coefficient_expansion on v[2^g] 2x1 NTT cts in place (v_w_* from pp; v_neg1 internal) */
int sp_coefficient_expansion(const sp_params_t*, const sp_pp_t*, uint64_t* v, size_t g, size_t stop_round,
                             size_t max_bits_to_gen_right);
/* server.rs:123-151 regev_to_gsw (idx_factor 1, idx_offset 0): v_inp[t_gsw*num_gsw] 2x1 NTT ->
 * v_gsw[num_gsw] 2 x 2t_gsw NTT, V = pp.v_conversion[0] */
int sp_regev_to_gsw(const sp_params_t*, const sp_pp_t*, const uint64_t* v_inp, uint64_t* v_gsw, size_t num_gsw);
/* server.rs:505-523 get_v_folding_neg: v_folding[nu_2] 2 x 2t_gsw NTT -> same shape */
int sp_get_v_folding_neg(const sp_params_t*, const uint64_t* v_folding, uint64_t* out);
/* server.rs:525-591 expand_query: v_reg_reoriented[N*dim0*2], v_folding[nu_2] 2 x 2t_gsw NTT */
int sp_expand_query(const sp_params_t*, const sp_pp_t*, const uint8_t* query, size_t query_len,
                    uint64_t* v_reg_reoriented, uint64_t* v_folding);
/* server.rs:388-427 fold_ciphertexts: cts[num_per] raw 2x1 in/out (result in cts[0]; the other
 * entries are scratch in the reference too and are returned unmodified here) */
int sp_fold_ciphertexts(const sp_params_t*, uint64_t* cts, size_t num_per, const uint64_t* v_folding,
                        const uint64_t* v_folding_neg);
/* The same fold the way process_query runs it -- every step in the delta form  ct_i + C (*) (G^-1(ct_{i+half}) - G^-1(ct_i)),
 * which equals (G - C) (*) ct_i + C (*) ct_{i+half} exactly (this export still forms G - C = get_v_folding_neg(v_folding) on the
 * device, server.rs:505-523; nothing reads it) -- and levels with at least `fused_min_pairs` pairs go through the fused
 * one-workgroup-per-step kernel (0: the library's default threshold, 1: every level fused); the remaining levels use
 * the three-launch tree tail.  Result in cts[0 .. 2N); byte-identical to
 * fold_ciphertexts(cts, v_folding, get_v_folding_neg(v_folding)). */
int sp_fold_ciphertexts_fused(const sp_params_t*, uint64_t* cts, size_t num_per, const uint64_t* v_folding,
                              long fused_min_pairs);
/* server.rs:429-468 pack: v_ct[n*n] raw 2x1, v_w = pp.v_packing -> (n+1) x n NTT */
int sp_pack(const sp_params_t*, const sp_pp_t*, const uint64_t* v_ct, uint64_t* out);
/* server.rs:470-503 encode: v_packed[instances] raw (n+1) x n -> response bytes */
int sp_encode(const sp_params_t*, const uint64_t* v_packed, uint8_t* out, size_t out_cap, size_t* out_len);

#ifdef __cplusplus
}
#endif
#endif /* SPIRAL_HIP_H */
