// TEST INFRASTRUCTURE: a database filled through the C ABI, its per-item digests taken on the (emulated) device (sp_db_item_digests:
// k_digest_keys and the kernel of the handle's resident form -- k_item_digest_words8, k_item_digest_packed, k_item_digest_planar,
// k_item_digest_sparse) and compared with this program's own scalar loop, linked against the emulated library (plain or
// AddressSanitizer build).  No Python in the process.  The pattern of db_digest_driver.cpp.
//   item_digest_driver params.json format
// format = "dense" (PACKED or 8-byte words, as the shape decides: random words with limbs >= q through sp_db_load, the loop runs over the
// words it loaded), "planar" or "planar-shards" (both of two, their tables added; sp_db_fill_synthetic, the loop runs over
// sp_synth_word of the reference indices) or "sparse" (five items upserted into a sparse bucket and into a dense handle: equal tables
// on the stored items, and the loop runs over sp_db_read_ref of the dense handle at the items' cells).  The table is taken whole, range
// by range and plane by plane; every output block has exactly the size the call may write: one word past it is a sanitizer report.
#include <algorithm>
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

// the definition, word by word: table[plane][2 i + l] += R_l(j) A_l(c) w   (per plane, so that plane ranges can be checked)
struct Scalar {
  uint64_t s_[2];
  size_t num_per, n_items;
  std::vector<uint64_t> t;
  Scalar(uint64_t seed, size_t planes, size_t num_per_, size_t n_items_) : num_per(num_per_), n_items(n_items_), t(planes * 2 * n_items_, 0) {
    s_[0] = mix(seed), s_[1] = mix(seed + 1);
  }
  void add(size_t plane, size_t z, size_t ii, size_t j, uint64_t w) {
    for (int l = 0; l < 2; l++) {
      const uint64_t s = s_[l];
      const uint64_t A = mix(s ^ (uint64_t)((plane * N + z) * num_per + ii)) | 1, R = mix(~s ^ (uint64_t)j) | 1;
      t[(plane * n_items + j * num_per + ii) * 2 + (size_t)l] += R * (A * w);
    }
  }
  uint64_t at(size_t plane0, size_t nplanes, size_t i, int l) const {
    uint64_t v = 0;
    for (size_t pl = plane0; pl < plane0 + nplanes; pl++) v += t[(pl * n_items + i) * 2 + (size_t)l];
    return v;
  }
};

// one call into blocks of exactly its size, added into total[2 * (i - item0) + l] (a shard set adds up) and flags |= present
static bool take(const sp_db_t* db, uint64_t seed, int plane0, int nplanes, size_t item0, size_t count, uint64_t* total, unsigned char* flags) {
  std::vector<uint64_t> out(2 * count, 0xCCCCCCCCCCCCCCCCull);
  std::vector<uint8_t> pres(count, 0xCC);
  if (sp_db_item_digests(db, seed, SP_DIGEST_RESIDENT, plane0, nplanes, item0, count, out.data(), pres.data()) != SP_OK) {
    fprintf(stderr, "sp_db_item_digests: %s\n", sp_last_error());
    return false;
  }
  for (size_t k = 0; k < count; k++) {
    if (pres[k] > 1) {
      fprintf(stderr, "present[%zu] = %d\n", k, pres[k]);
      return false;
    }
    if (!pres[k] && (out[2 * k] || out[2 * k + 1])) {
      fprintf(stderr, "item %zu is not held and not (0, 0)\n", item0 + k);
      return false;
    }
    total[2 * k] += out[2 * k];
    total[2 * k + 1] += out[2 * k + 1];
    flags[k] |= pres[k];
  }
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
  Scalar want(seed, planes, num_per, n_items);
  const bool sparse = strcmp(format, "sparse") == 0, shards = strcmp(format, "planar-shards") == 0, planar = strcmp(format, "planar") == 0;
  std::vector<sp_db_t*> handles;
  std::vector<unsigned char> held(n_items, 1);   // what the handles hold together
  std::vector<uint64_t> words;
  if (sparse) {
    sp_db_t* bucket = sp_db_create_sparse(p);
    sp_db_t* dense = sp_db_create(p, 0, 1);
    if (!bucket || !dense) return 3;
    std::fill(held.begin(), held.end(), 0);
    const size_t idx[5] = {0, n_items - 1, num_per + 1, 2 * num_per + 1, n_items / 2 + 3};
    std::vector<unsigned char> item(isz);
    uint64_t x = 88172645463325252ull;
    for (size_t k = 0; k < 5; k++) {
      for (size_t b = 0; b < isz; b++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        item[b] = (unsigned char)x;
      }
      if (sp_db_update_item(bucket, idx[k], item.data(), isz) != SP_OK || sp_db_update_item(dense, idx[k], item.data(), isz) != SP_OK) return 3;
      held[idx[k]] = 1;
      uint64_t w = 0;
      for (size_t pl = 0; pl < planes; pl++)
        for (size_t z = 0; z < (size_t)N; z++) {
          if (sp_db_read_ref(dense, (int)pl, (int)z, (int)(idx[k] % num_per), (int)(idx[k] / num_per), 1, &w) != SP_OK) return 3;
          want.add(pl, z, idx[k] % num_per, idx[k] / num_per, w);
        }
    }
    // the dense handle of the same items: the same pairs, every item present
    std::vector<uint64_t> of_dense(2 * n_items, 0), of_bucket(2 * n_items, 0);
    std::vector<unsigned char> fd(n_items, 0), fb(n_items, 0);
    if (!take(dense, seed, 0, (int)planes, 0, n_items, of_dense.data(), fd.data()) ||
        !take(bucket, seed, 0, (int)planes, 0, n_items, of_bucket.data(), fb.data()))
      return 1;
    if (of_dense != of_bucket || std::count(fd.begin(), fd.end(), 1) != (long)n_items || fb != held) {
      fprintf(stderr, "the sparse bucket and the dense handle of the same items differ\n");
      return 1;
    }
    sp_db_free(dense);
    handles.push_back(bucket);
  } else if (planar || shards) {
    const int S = shards ? 2 : 1;
    for (int s = 0; s < S; s++) {
      sp_db_t* db = shards ? sp_db_create_planar_shard(p, s, S) : sp_db_create_planar(p);
      if (!db) {
        fprintf(stderr, "create: %s\n", sp_last_error());
        return 3;
      }
      if (sp_db_fill_synthetic(db, fill) != SP_OK) return 1;
      handles.push_back(db);
    }
    for (size_t pl = 0; pl < planes; pl++)
      for (size_t z = 0; z < (size_t)N; z++)
        for (size_t ii = 0; ii < num_per; ii++)
          for (size_t j = 0; j < dim0; j++) want.add(pl, z, ii, j, sp_synth_word(fill, ((pl * N + z) * num_per + ii) * dim0 + j));
  } else {
    sp_db_t* db = sp_db_create(p, 0, 1);
    if (!db) return 3;
    words.resize(planes * N * num_per * dim0);
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
    handles.push_back(db);
    size_t k = 0;
    for (size_t pl = 0; pl < planes; pl++)
      for (size_t z = 0; z < (size_t)N; z++)
        for (size_t ii = 0; ii < num_per; ii++)
          for (size_t j = 0; j < dim0; j++) want.add(pl, z, ii, j, canon(words[k++]));
  }

  // the table whole, range by range (inside a row, across rows, one item, the last item) and plane by plane
  struct Call {
    size_t plane0, nplanes, item0, count;
  };
  std::vector<Call> calls = {{0, planes, 0, n_items},
                             {0, planes, num_per / 2 + 1, 2 * num_per},
                             {0, planes, 0, num_per + num_per / 2},
                             {0, planes, num_per + 1, std::max<size_t>(1, num_per / 2 - 1)},
                             {0, planes, 2 * num_per + 1, 1},
                             {0, planes, n_items - 1, 1},
                             {1, planes - 1, (dim0 - 3) * num_per + 1, 3 * num_per - 1}};
  for (size_t pl = 0; pl < planes; pl++) calls.push_back(Call{pl, 1, 0, n_items});
  size_t pairs = 0;
  bool equal = true, nonzero = false;
  for (const Call& c : calls) {
    std::vector<uint64_t> got(2 * c.count, 0);
    std::vector<unsigned char> flags(c.count, 0);
    for (sp_db_t* db : handles)
      if (!take(db, seed, (int)c.plane0, (int)c.nplanes, c.item0, c.count, got.data(), flags.data())) return 1;
    for (size_t k = 0; k < c.count; k++) {
      for (int l = 0; l < 2; l++) {
        const uint64_t w = want.at(c.plane0, c.nplanes, c.item0 + k, l);
        if (got[2 * k + (size_t)l] != w) {
          if (equal) fprintf(stderr, "planes %zu+%zu item %zu lane %d: %016llx != %016llx\n", c.plane0, c.nplanes, c.item0 + k, l,
                             (unsigned long long)got[2 * k + (size_t)l], (unsigned long long)w);
          equal = false;
        }
        nonzero = nonzero || w != 0;
      }
      if (flags[k] != held[c.item0 + k]) {
        if (equal) fprintf(stderr, "item %zu: present %d\n", c.item0 + k, flags[k]);
        equal = false;
      }
      pairs++;
    }
  }
  // nothing to do writes nothing and needs no block
  if (sp_db_item_digests(handles[0], seed, SP_DIGEST_RESIDENT, 0, (int)planes, 3, 0, nullptr, nullptr) != SP_OK ||
      sp_db_item_digests(handles[0], seed, SP_DIGEST_RESIDENT, (int)planes, 0, 0, 4, nullptr, nullptr) != SP_OK)
    equal = false;
  if (!words.empty()) {
    // the host half agrees too: plane 1 in two z-ranges == the device's plane 1
    std::vector<uint64_t> acc(2 * n_items, 0);
    const uint64_t* plane1 = words.data() + (size_t)N * num_per * dim0;
    if (sp_db_item_digests_ref_words(p, seed, 1, 0, 5, plane1, acc.data()) != SP_OK ||
        sp_db_item_digests_ref_words(p, seed, 1, 5, N - 5, plane1 + 5 * num_per * dim0, acc.data()) != SP_OK)
      equal = false;
    for (size_t i = 0; i < n_items; i++)
      if (acc[2 * i] != want.at(1, 1, i, 0) || acc[2 * i + 1] != want.at(1, 1, i, 1)) {
        if (equal) fprintf(stderr, "sp_db_item_digests_ref_words differs at item %zu of plane 1\n", i);
        equal = false;
      }
  }
  for (sp_db_t* db : handles) sp_db_free(db);
  sp_params_free(p);
  printf("%zu pairs in %zu calls (%s): %s\n", pairs, calls.size(), format, equal && nonzero ? "equal to the scalar loop" : "MISMATCH");
  return equal && nonzero ? 0 : 1;
}
