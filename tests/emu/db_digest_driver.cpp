// TEST INFRASTRUCTURE: a database filled through the C ABI, digested on the (emulated) device (sp_db_digest: k_digest_keys and the kernel
// of the handle's resident form -- k_digest_words8, k_digest_packed, k_digest_planar, k_digest_sparse) and compared with this program's
// own scalar loop, linked against the emulated library (plain or AddressSanitizer build).  No Python in the process.  The pattern of
// item_readback_driver.cpp.
//   db_digest_driver params.json format
// format = "dense" (PACKED or 8-byte words, as the shape decides: random words with limbs >= q through sp_db_load, the loop runs over the
// words it loaded), "planar" or "planar-shards" (both of two, their digests added; sp_db_fill_synthetic, the loop runs over
// sp_synth_word of the reference indices) or "sparse" (five items upserted into a sparse bucket and into a dense handle: equal
// digests, and the loop runs over sp_db_read_ref of the dense handle at the items' cells).  Every output block has exactly the size the
// call may write: one word past it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spiral_hip.h"

static const uint64_t Q0 = 268369921ull, Q1 = 249561089ull;
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

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static uint64_t canon(uint64_t w) { return ((w & 0xffffffffull) % Q0) | (((w >> 32) % Q1) << 32); }

// the definition, word by word: sums[2 plane + l] += A_l(c) R_l(j) w
struct Scalar {
  uint64_t s_[2];
  size_t num_per;
  std::vector<uint64_t> sums;
  Scalar(uint64_t seed, size_t planes, size_t num_per_) : num_per(num_per_), sums(2 * planes, 0) { s_[0] = mix(seed), s_[1] = mix(seed + 1); }
  void add(size_t plane, size_t z, size_t ii, size_t j, uint64_t w) {
    for (int l = 0; l < 2; l++) {
      const uint64_t s = s_[l];
      const uint64_t A = mix(s ^ (uint64_t)((plane * N + z) * num_per + ii)) | 1, R = mix(~s ^ (uint64_t)j) | 1;
      sums[2 * plane + l] += A * (R * w);
    }
  }
};

static bool digest(const sp_db_t* db, uint64_t seed, size_t planes, std::vector<uint64_t>& total) {
  std::vector<uint64_t> out(2 * planes, 0xCCCCCCCCCCCCCCCCull);
  if (sp_db_digest(db, seed, SP_DIGEST_RESIDENT, 0, (int)planes, out.data()) != SP_OK) {
    fprintf(stderr, "sp_db_digest: %s\n", sp_last_error());
    return false;
  }
  for (size_t pl = 0; pl < planes; pl++) {   // every plane once more on its own, into a block of one pair
    std::vector<uint64_t> one(2, 0xCCCCCCCCCCCCCCCCull);
    if (sp_db_digest(db, seed, SP_DIGEST_RESIDENT, (int)pl, 1, one.data()) != SP_OK || one[0] != out[2 * pl] || one[1] != out[2 * pl + 1]) {
      fprintf(stderr, "plane %zu alone differs from the whole call\n", pl);
      return false;
    }
  }
  for (size_t k = 0; k < 2 * planes; k++) total[k] += out[k];
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<unsigned char> json = slurp(argv[1]);
  json.push_back(0);
  const char* format = argv[2];
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const size_t n = (size_t)sp_params_get(p, "n"), planes = (size_t)sp_params_get(p, "instances") * n * n;
  const size_t num_per = (size_t)1 << sp_params_get(p, "db_dim_2"), dim0 = (size_t)1 << sp_params_get(p, "db_dim_1");
  const size_t isz = (size_t)sp_params_get(p, "db_item_size"), n_items = (size_t)sp_params_get(p, "num_items");
  const uint64_t seed = 0x5EED, fill = 0xF111;
  Scalar want(seed, planes, num_per);
  std::vector<uint64_t> got(2 * planes, 0);
  const bool sparse = strcmp(format, "sparse") == 0, shards = strcmp(format, "planar-shards") == 0, planar = strcmp(format, "planar") == 0;
  if (sparse) {
    sp_db_t* bucket = sp_db_create_sparse(p);
    sp_db_t* dense = sp_db_create(p, 0, 1);
    if (!bucket || !dense) return 3;
    const size_t idx[5] = {0, n_items - 1, num_per + 1, 2 * num_per + 1, n_items / 2 + 3};
    std::vector<unsigned char> item(isz);
    uint64_t x = 88172645463325252ull;
    for (size_t k = 0; k < 5; k++) {
      for (size_t b = 0; b < isz; b++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        item[b] = (unsigned char)x;
      }
      if (sp_db_update_item(bucket, idx[k], item.data(), isz) != SP_OK || sp_db_update_item(dense, idx[k], item.data(), isz) != SP_OK) return 3;
      uint64_t w = 0;
      for (size_t pl = 0; pl < planes; pl++)
        for (size_t z = 0; z < (size_t)N; z++) {
          if (sp_db_read_ref(dense, (int)pl, (int)z, (int)(idx[k] % num_per), (int)(idx[k] / num_per), 1, &w) != SP_OK) return 3;
          want.add(pl, z, idx[k] % num_per, idx[k] / num_per, w);
        }
    }
    std::vector<uint64_t> of_dense(2 * planes, 0);
    if (!digest(bucket, seed, planes, got) || !digest(dense, seed, planes, of_dense)) return 1;
    if (of_dense != got) {
      fprintf(stderr, "the sparse bucket and the dense handle of the same items digest differently\n");
      return 1;
    }
    sp_db_free(bucket);
    sp_db_free(dense);
  } else if (planar || shards) {
    const int S = shards ? 2 : 1;
    for (int s = 0; s < S; s++) {
      sp_db_t* db = shards ? sp_db_create_planar_shard(p, s, S) : sp_db_create_planar(p);
      if (!db) {
        fprintf(stderr, "create: %s\n", sp_last_error());
        return 3;
      }
      if (sp_db_fill_synthetic(db, fill) != SP_OK || !digest(db, seed, planes, got)) return 1;
      sp_db_free(db);
    }
    for (size_t pl = 0; pl < planes; pl++)
      for (size_t z = 0; z < (size_t)N; z++)
        for (size_t ii = 0; ii < num_per; ii++)
          for (size_t j = 0; j < dim0; j++) want.add(pl, z, ii, j, sp_synth_word(fill, ((pl * N + z) * num_per + ii) * dim0 + j));
  } else {
    sp_db_t* db = sp_db_create(p, 0, 1);
    if (!db) return 3;
    std::vector<uint64_t> words(planes * N * num_per * dim0);
    uint64_t x = 0x2545F4914F6CDD1Dull;
    for (uint64_t& w : words) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      w = x;
    }
    words[1] = (Q0 - 1) | ((Q1 - 1) << 32), words[2] = Q0 | (Q1 << 32), words[3] = ~0ull, words[4] = 0;
    if (sp_db_load(db, words.data(), words.size()) != SP_OK) {
      fprintf(stderr, "load: %s\n", sp_last_error());
      return 3;
    }
    if (!digest(db, seed, planes, got)) return 1;
    sp_db_free(db);
    size_t k = 0;
    for (size_t pl = 0; pl < planes; pl++)
      for (size_t z = 0; z < (size_t)N; z++)
        for (size_t ii = 0; ii < num_per; ii++)
          for (size_t j = 0; j < dim0; j++) want.add(pl, z, ii, j, canon(words[k++]));
    // the host half agrees too: one plane, two z-ranges
    uint64_t acc[2] = {0, 0};
    const uint64_t* plane1 = words.data() + (size_t)N * num_per * dim0;
    if (sp_db_digest_ref_words(p, seed, 1, 0, 5, plane1, acc) != SP_OK ||
        sp_db_digest_ref_words(p, seed, 1, 5, N - 5, plane1 + 5 * num_per * dim0, acc) != SP_OK || acc[0] != got[2] || acc[1] != got[3]) {
      fprintf(stderr, "sp_db_digest_ref_words differs from the device's plane 1\n");
      return 1;
    }
  }
  sp_params_free(p);
  const bool equal = got == want.sums;
  bool nonzero = true;
  for (uint64_t v : got) nonzero = nonzero && v != 0;
  printf("digest of %zu planes (%s): %s\n", planes, format, equal && nonzero ? "equal to the scalar loop" : "MISMATCH");
  return equal && nonzero ? 0 : 1;
}
