// TEST INFRASTRUCTURE: items copied between resident databases through the C ABI (sp_db_copy_items: a gather of item_readback.hpp /
// planar_resident.hpp, then k_items_copy_slots, k_items_scatter_words8, k_items_scatter_packed or k_planar_scatter_items), linked
// against the emulated library (plain or AddressSanitizer build).  No Python in the process.  The pattern of item_readback_driver.cpp.
//   db_copy_driver params.json chain [db_load_window ...]
// chain = "packed-sparse-words8": words the program makes itself go into a PACKED handle (sp_db_load), from there into an empty sparse
//         bucket, from there into an 8-byte handle of the same shape that held synthetic words;
//         "planar-shards-packed": two planar row shards of synthetic words (sp_db_fill_synthetic: the words are known from their
//         reference index) into one PACKED handle that held other synthetic words.
// Per listed db_load_window (default: the shipped one): the first run copies the whole range, the later ones -- one-item windows, say --
// a range of 300 items that starts inside a row and crosses two row ends.  The destination is then checked against the words that went
// in: its per-item digest table (every word of every item, sp_db_item_digests) against the host's table of those words
// (sp_db_item_digests_ref_words; outside the range: of the old words), and word for word through sp_db_read_ref at the first, second,
// middle and last z of every plane, column and row.
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
  const bool chain_planar = strcmp(argv[2], "planar-shards-packed") == 0;
  if (!chain_planar && strcmp(argv[2], "packed-sparse-words8") != 0) return 2;
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const size_t n_items = (size_t)sp_params_get(p, "num_items");
  const size_t num_per = (size_t)1 << sp_params_get(p, "db_dim_2"), dim0 = (size_t)1 << sp_params_get(p, "db_dim_1");
  const int planes = 4;
  const size_t plane_words = (size_t)N * n_items;
  const uint64_t SEED_NEW = 5, SEED_OLD = 9;
  // the words that go in, in the reference layout [plane][z][ii][j]: the program's own (a 64-bit LCG, both limbs below their primes), or
  // sp_synth_word of the reference index where the source is filled synthetically
  auto word_in = [&](uint64_t ref) -> uint64_t {
    if (chain_planar) return sp_synth_word(SEED_NEW, ref);
    uint64_t x = ref * 6364136223846793005ull + 1442695040888963407ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 32;
    return ((x & 0xffffffffull) % Q0) | (((x >> 32) % Q1) << 32);
  };
  // host tables of the new and the old words, z-rows in pieces
  std::vector<uint64_t> t_new(2 * n_items, 0), t_old(2 * n_items, 0), piece;
  const int zs = 16;
  piece.resize((size_t)zs * n_items);
  for (int which = 0; which < 2; which++)
    for (int plane = 0; plane < planes; plane++)
      for (int z0 = 0; z0 < N; z0 += zs) {
        const uint64_t ref0 = ((uint64_t)plane * N + (uint64_t)z0) * n_items;
        for (size_t k = 0; k < piece.size(); k++) piece[k] = which ? sp_synth_word(SEED_OLD, ref0 + k) : word_in(ref0 + k);
        OK(sp_db_item_digests_ref_words(p, DIGEST_SEED, plane, z0, zs, piece.data(), which ? t_old.data() : t_new.data()));
      }
  int bad = 0, runs = 0;
  for (int a = 3; a < argc || runs == 0; a++, runs++) {
    if (a < argc) OK(sp_debug_set("db_load_window", atol(argv[a])));
    const size_t item0 = runs == 0 ? 0 : num_per - 50, count = runs == 0 ? n_items : 300;   // (num_per >= 128 on both chains)
    std::vector<sp_db_t*> srcs;
    sp_db_t *mid = nullptr, *dst = nullptr;
    if (chain_planar) {
      for (int s = 0; s < 2; s++) {
        srcs.push_back(sp_db_create_planar_shard(p, s, 2));
        if (!srcs.back()) return 3;
        OK(sp_db_fill_synthetic(srcs.back(), SEED_NEW));
      }
      dst = sp_db_create(p, 0, 1);
      if (!dst || strcmp(sp_db_format(dst), "packed") != 0) return 3;
    } else {
      srcs.push_back(sp_db_create(p, 0, 1));
      if (!srcs.back() || strcmp(sp_db_format(srcs.back()), "packed") != 0) return 3;
      std::vector<uint64_t> plane_in(plane_words);
      for (int plane = 0; plane < planes; plane++) {
        for (size_t k = 0; k < plane_words; k++) plane_in[k] = word_in((uint64_t)plane * plane_words + k);
        OK(sp_db_load_plane(srcs.back(), plane, 0, N, plane_in.data()));
      }
      mid = sp_db_create_sparse(p);
      OK(sp_debug_set("db_unpacked", 1));
      dst = sp_db_create(p, 0, 1);
      OK(sp_debug_set("db_unpacked", 0));
      if (!mid || !dst || strcmp(sp_db_format(dst), "words8") != 0) return 3;
    }
    OK(sp_db_fill_synthetic(dst, SEED_OLD));
    size_t copied = 0, total = 0;
    if (chain_planar) {
      for (sp_db_t* s : srcs) {
        OK(sp_db_copy_items(dst, s, item0, count, &copied));
        total += copied;
      }
    } else {
      OK(sp_db_copy_items(mid, srcs[0], item0, count, &copied));
      if (copied != count || sp_db_sparse_items(mid) != count) bad++;
      OK(sp_db_copy_items(dst, mid, 0, n_items, &total));   // (the bucket holds the range only)
    }
    if (total != count && bad++ < 8) fprintf(stderr, "run %d: %zu items copied, %zu expected\n", runs, total, count);
    // exactly-sized heap blocks: one word past any of them is a sanitizer report
    std::vector<uint64_t> got(2 * n_items, 0xCC);
    std::vector<uint8_t> present(n_items, 0xCC);
    OK(sp_db_item_digests(dst, DIGEST_SEED, 0, 0, planes, 0, n_items, got.data(), present.data()));
    for (size_t i = 0; i < n_items; i++) {
      const std::vector<uint64_t>& t = i >= item0 && i - item0 < count ? t_new : t_old;
      if ((got[2 * i] != t[2 * i] || got[2 * i + 1] != t[2 * i + 1] || present[i] != 1) && bad++ < 8)
        fprintf(stderr, "run %d: item %zu differs from the words that went in\n", runs, i);
    }
    std::vector<uint64_t> col(dim0);
    const int zs_read[4] = {0, 1, N / 2 - 1, N - 1};
    for (int plane = 0; plane < planes; plane++)
      for (int zi = 0; zi < 4; zi++)
        for (size_t ii = 0; ii < num_per; ii++) {
          OK(sp_db_read_ref(dst, plane, zs_read[zi], (int)ii, 0, (int)dim0, col.data()));
          for (size_t j = 0; j < dim0; j++) {
            const size_t i = j * num_per + ii;
            const uint64_t ref = (((uint64_t)plane * N + (uint64_t)zs_read[zi]) * num_per + ii) * dim0 + j;
            const uint64_t want = i >= item0 && i - item0 < count ? word_in(ref) : sp_synth_word(SEED_OLD, ref);
            if (col[j] != want && bad++ < 8) fprintf(stderr, "run %d: word (%d, %d, %zu, %zu) differs\n", runs, plane, zs_read[zi], ii, j);
          }
        }
    for (sp_db_t* s : srcs) sp_db_free(s);
    sp_db_free(mid);
    sp_db_free(dst);
  }
  sp_params_free(p);
  printf("%d runs over %zu items (%s): %s\n", runs, n_items, argv[2], bad ? "MISMATCH" : "every word equal to the words that went in");
  return bad ? 1 : 0;
}
