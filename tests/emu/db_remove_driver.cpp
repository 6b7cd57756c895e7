// TEST INFRASTRUCTURE: items removed from resident databases through the C ABI (sp_db_remove_items / sp_db_remove_range /
// sp_db_sparse_trim: k_items_clear_packed, k_items_clear_words8, k_planar_clear_items, k_sparse_move_slots), linked against the emulated
// library (plain or AddressSanitizer build).  No Python in the process.  The pattern of db_copy_driver.cpp.
//   db_remove_driver params.json chain [db_load_window ...]
// chain = "packed-words8-sparse": words the program makes itself go into a PACKED handle and an 8-byte handle of the same shape
//         (sp_db_load_plane), and from the PACKED one into a sparse bucket (sp_db_copy_items: slot = item index);
//         "planar-shards": two planar row shards of synthetic words (sp_db_fill_synthetic: known from their reference index).
// Per listed db_load_window (default: the shipped one; 1 = one-record windows) the handles are made anew and lose the same list: a quad
// per single position, a whole quad, three rows of one 16-row cell, the first and the last row and column, a run across a row end, a
// repeated index; the sparse bucket then loses a range as well and is trimmed.  Every handle is then checked against the words that
// went in with the removed items' words zeroed: its per-item digest table (every word of every item, sp_db_item_digests) against the
// host's table of those words (sp_db_item_digests_ref_words), `present`, and on the dense forms word for word through sp_db_read_ref at
// the first, second, middle and last z of every plane, column and row.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spiral_hip.h"

static const uint64_t Q0 = 268369921ull, Q1 = 249561089ull, DIGEST_SEED = 0xD16E57ull;
static const int N = 2048;

static std::vector<unsigned char> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> b((size_t)n + 1);
  if (fread(b.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  b.resize((size_t)n);
  return b;
}

#define OK(call)                                                        \
  do {                                                                  \
    if ((call) != SP_OK) {                                              \
      fprintf(stderr, "%s: %s\n", #call, sp_last_error());              \
      return 3;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<unsigned char> json = slurp(argv[1]);
  json.push_back(0);
  const bool chain_planar = strcmp(argv[2], "planar-shards") == 0;
  if (!chain_planar && strcmp(argv[2], "packed-words8-sparse") != 0) return 2;
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const size_t n_items = (size_t)sp_params_get(p, "num_items");
  const size_t num_per = (size_t)1 << sp_params_get(p, "db_dim_2"), dim0 = (size_t)1 << sp_params_get(p, "db_dim_1");
  const int planes = 4;
  const size_t plane_words = (size_t)N * n_items;
  const uint64_t SEED_IN = 5;
  if (num_per < 128 || dim0 < 16) return 2;
  // the words that go in, in the reference layout [plane][z][ii][j]: the program's own (a 64-bit LCG, both limbs below their primes), or
  // sp_synth_word of the reference index where the handles are filled synthetically
  auto word_in = [&](uint64_t ref) -> uint64_t {
    if (chain_planar) return sp_synth_word(SEED_IN, ref);
    uint64_t x = ref * 6364136223846793005ull + 1442695040888963407ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 32;
    return ((x & 0xffffffffull) % Q0) | (((x >> 32) % Q1) << 32);
  };
  // the list (row, column) and which items it removes
  std::vector<size_t> list;
  auto add = [&](size_t j, size_t ii) { list.push_back(j * num_per + ii); };
  for (size_t w = 0; w < 4; w++) add(w >> 1, 2 * (3 + w) + (w & 1));   // a quad per position
  for (size_t w = 0; w < 4; w++) add(2 + (w >> 1), 20 + (w & 1));      // a whole quad
  add(5, 40), add(9, 40), add(12, 40);                                 // rows of one 16-row cell
  add(0, 0), add(0, num_per - 1), add(dim0 - 1, 0), add(dim0 - 1, num_per - 1);
  for (size_t k = 0; k < 7; k++) list.push_back(7 * num_per - 3 + k);  // across the end of row 6
  add(dim0 / 2, 77), add(dim0 / 2 - 1, 77);                            // (on a pair of row shards: one each)
  list.push_back(list[2]), list.push_back(list[9]);                    // repeated
  std::vector<char> gone(n_items, 0);
  size_t n_gone = 0;
  for (size_t i : list) n_gone += !gone[i], gone[i] = 1;
  // the sparse bucket afterwards loses a range too
  const size_t r0 = 3 * num_per + 5, rn = 2 * num_per;
  std::vector<char> gone_sparse(gone);
  size_t n_range = 0;
  for (size_t i = r0; i < r0 + rn; i++) n_range += !gone_sparse[i], gone_sparse[i] = 1;
  // host tables of the words with the removed items' words zeroed, z-rows in pieces
  std::vector<uint64_t> t_dense(2 * n_items, 0), t_sparse(2 * n_items, 0), piece;
  const int zs = 16;
  piece.resize((size_t)zs * n_items);
  for (int which = 0; which < (chain_planar ? 1 : 2); which++)
    for (int plane = 0; plane < planes; plane++)
      for (int z0 = 0; z0 < N; z0 += zs) {
        const uint64_t ref0 = ((uint64_t)plane * N + (uint64_t)z0) * n_items;
        for (size_t k = 0; k < piece.size(); k++) {
          const size_t item = (k % dim0) * num_per + (k / dim0) % num_per;   // ref = (zp * num_per + ii) * dim0 + j
          piece[k] = (which ? gone_sparse : gone)[item] ? 0 : word_in(ref0 + k);
        }
        OK(sp_db_item_digests_ref_words(p, DIGEST_SEED, plane, z0, zs, piece.data(), which ? t_sparse.data() : t_dense.data()));
      }
  int bad = 0, runs = 0;
  for (int a = 3; a < argc || runs == 0; a++, runs++) {
    if (a < argc) OK(sp_debug_set("db_load_window", atol(argv[a])));
    std::vector<sp_db_t*> dense;
    sp_db_t* bucket = nullptr;
    if (chain_planar) {
      for (int s = 0; s < 2; s++) {
        dense.push_back(sp_db_create_planar_shard(p, s, 2));
        if (!dense.back()) return 3;
        OK(sp_db_fill_synthetic(dense.back(), SEED_IN));
      }
    } else {
      dense.push_back(sp_db_create(p, 0, 1));
      OK(sp_debug_set("db_unpacked", 1));
      dense.push_back(sp_db_create(p, 0, 1));
      OK(sp_debug_set("db_unpacked", 0));
      if (!dense[0] || !dense[1] || strcmp(sp_db_format(dense[0]), "packed") != 0 || strcmp(sp_db_format(dense[1]), "words8") != 0) return 3;
      std::vector<uint64_t> plane_in(plane_words);
      for (int plane = 0; plane < planes; plane++) {
        for (size_t k = 0; k < plane_words; k++) plane_in[k] = word_in((uint64_t)plane * plane_words + k);
        for (sp_db_t* d : dense) OK(sp_db_load_plane(d, plane, 0, N, plane_in.data()));
      }
      bucket = sp_db_create_sparse(p);
      size_t copied = 0;
      if (!bucket) return 3;
      OK(sp_db_copy_items(bucket, dense[0], 0, n_items, &copied));
      if (copied != n_items) bad++;
    }
    // exactly-sized heap blocks: one word past any of them is a sanitizer report
    std::vector<size_t> exact(list);
    size_t removed = 0, total = 0;
    for (sp_db_t* d : dense) {
      OK(sp_db_remove_items(d, exact.data(), exact.size(), &removed));
      total += removed;
    }
    if (total != n_gone * (chain_planar ? 1 : 2) && bad++ < 8) fprintf(stderr, "run %d: %zu items removed, %zu expected\n", runs, total, n_gone);
    std::vector<uint64_t> got(2 * n_items, 0xCC), sum(2 * n_items, 0);
    std::vector<uint8_t> present(n_items, 0xCC);
    for (size_t k = 0; k < dense.size(); k++) {
      OK(sp_db_item_digests(dense[k], DIGEST_SEED, 0, 0, planes, 0, n_items, got.data(), present.data()));
      for (size_t i = 0; i < n_items; i++) {
        const bool held = !chain_planar || (i / num_per) / (dim0 / 2) == k;
        const uint64_t w0 = held ? t_dense[2 * i] : 0, w1 = held ? t_dense[2 * i + 1] : 0;
        if ((got[2 * i] != w0 || got[2 * i + 1] != w1 || present[i] != (held ? 1 : 0)) && bad++ < 8)
          fprintf(stderr, "run %d: handle %zu: item %zu differs from the expected words\n", runs, k, i);
      }
      const size_t nj = chain_planar ? dim0 / 2 : dim0, j0 = chain_planar ? k * nj : 0;
      std::vector<uint64_t> col(nj);
      const int zs_read[4] = {0, 1, N / 2 - 1, N - 1};
      for (int plane = 0; plane < planes; plane++)
        for (int zi = 0; zi < 4; zi++)
          for (size_t ii = 0; ii < num_per; ii++) {
            OK(sp_db_read_ref(dense[k], plane, zs_read[zi], (int)ii, 0, (int)nj, col.data()));
            for (size_t j = 0; j < nj; j++) {
              const uint64_t ref = (((uint64_t)plane * N + (uint64_t)zs_read[zi]) * num_per + ii) * dim0 + j0 + j;
              const uint64_t want = gone[(j0 + j) * num_per + ii] ? 0 : word_in(ref);
              if (col[j] != want && bad++ < 8) fprintf(stderr, "run %d: handle %zu: word (%d, %d, %zu, %zu) differs\n", runs, k, plane, zs_read[zi], ii, j0 + j);
            }
          }
    }
    if (bucket) {
      size_t freed = 0;
      const size_t bytes = sp_db_device_bytes(bucket);
      OK(sp_db_remove_items(bucket, exact.data(), exact.size(), &removed));
      if (removed != n_gone || sp_db_sparse_items(bucket) != n_items - n_gone) bad++;
      OK(sp_db_remove_range(bucket, r0, rn, &removed));
      if (removed != n_range || sp_db_sparse_items(bucket) != n_items - n_gone - n_range || sp_db_device_bytes(bucket) != bytes) bad++;
      OK(sp_db_sparse_trim(bucket, &freed));   // (the count is still above half of the capacity: nothing shrinks)
      if (freed != bytes - sp_db_device_bytes(bucket)) bad++;
      OK(sp_db_item_digests(bucket, DIGEST_SEED, 0, 0, planes, 0, n_items, got.data(), present.data()));
      for (size_t i = 0; i < n_items; i++)
        if ((got[2 * i] != t_sparse[2 * i] || got[2 * i + 1] != t_sparse[2 * i + 1] || present[i] != (gone_sparse[i] ? 0 : 1)) && bad++ < 8)
          fprintf(stderr, "run %d: bucket: item %zu differs from the expected words\n", runs, i);
      // ... and nearly all of it: the store shrinks to the 64-slot minimum and keeps the survivors' words
      OK(sp_db_remove_range(bucket, 40, n_items - 40, &removed));
      OK(sp_db_sparse_trim(bucket, &freed));
      if (freed == 0 || freed != bytes - sp_db_device_bytes(bucket)) bad++;
      OK(sp_db_item_digests(bucket, DIGEST_SEED, 0, 0, planes, 0, n_items, got.data(), present.data()));
      for (size_t i = 0; i < n_items; i++) {
        const bool held = i < 40 && !gone_sparse[i];
        if ((got[2 * i] != (held ? t_sparse[2 * i] : 0) || got[2 * i + 1] != (held ? t_sparse[2 * i + 1] : 0) || present[i] != (held ? 1 : 0)) && bad++ < 8)
          fprintf(stderr, "run %d: trimmed bucket: item %zu differs from the expected words\n", runs, i);
      }
    }
    for (sp_db_t* d : dense) sp_db_free(d);
    sp_db_free(bucket);
  }
  sp_params_free(p);
  printf("%d runs over %zu items (%s): %s\n", runs, n_items, argv[2], bad ? "MISMATCH" : "every word equal to the expected words");
  return bad ? 1 : 0;
}
