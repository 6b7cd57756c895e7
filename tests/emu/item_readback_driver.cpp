// TEST INFRASTRUCTURE: an item file into a database through the C ABI and every item back out of it (sp_db_read_items: the gather of
// the handle's format -- k_items_gather_words8, k_items_gather_packed, k_planar_gather -- and k_items_decode; sp_db_export_rows), linked
// against the emulated library (plain or AddressSanitizer build).  No Python in the process.  The pattern of planar_shard_driver.cpp.
//   item_readback_driver params.json items.bin format [db_load_window ...]
// items.bin = at most num_items records of db_item_size bytes (a shorter file reads as zeros past its end); format = "dense" (PACKED or
// 8-byte words, as the shape decides), "planar", "planar-shards" (both of two) or "sparse" (every third item upserted).  Per listed
// db_load_window (default: the shipped one) every item is read back in one call -- cut into windows by the library: the bit-packing
// tail of an item and the last, shorter window are where an out-of-bounds access would hide -- and once more in ranges of 7 items
// at either end of the database, and compared with the file; the export's records are checked against the same bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spiral_hip.h"

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

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::vector<unsigned char> json = slurp(argv[1]), items = slurp(argv[2]);
  json.push_back(0);
  const char* format = argv[3];
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const size_t n_items = (size_t)sp_params_get(p, "num_items"), isz = (size_t)sp_params_get(p, "db_item_size");
  const size_t num_per = (size_t)1 << sp_params_get(p, "db_dim_2"), dim0 = (size_t)1 << sp_params_get(p, "db_dim_1");
  if (items.size() > n_items * isz) return 2;
  std::vector<unsigned char> file(n_items * isz, 0);
  memcpy(file.data(), items.data(), items.size());
  const bool sparse = strcmp(format, "sparse") == 0, shards = strcmp(format, "planar-shards") == 0;
  const int S = shards ? 2 : 1;
  int bad = 0, runs = 0;
  for (int a = 4; a < argc || runs == 0; a++, runs++) {
    if (a < argc && sp_debug_set("db_load_window", atol(argv[a])) != SP_OK) return 3;
    for (int s = 0; s < S; s++) {
      sp_db_t* db = sparse ? sp_db_create_sparse(p) : shards ? sp_db_create_planar_shard(p, s, S)
                    : strcmp(format, "planar") == 0 ? sp_db_create_planar(p) : sp_db_create(p, 0, 1);
      if (!db) {
        fprintf(stderr, "create: %s\n", sp_last_error());
        return 3;
      }
      std::vector<unsigned char> want(file), held(n_items, 1);
      if (sparse) {
        for (size_t i = 0; i < n_items; i++) {
          held[i] = i % 3 == 1;
          if (!held[i])
            memset(want.data() + i * isz, 0, isz);
          else if (sp_db_update_item(db, i, file.data() + i * isz, isz) != SP_OK)
            return 3;
        }
      } else {
        if (sp_db_load_items(db, items.data(), items.size()) != SP_OK) {
          fprintf(stderr, "load: %s\n", sp_last_error());
          return 3;
        }
        for (size_t i = 0; i < n_items; i++) {
          held[i] = (i / num_per) / (dim0 / (size_t)S) == (size_t)s;
          if (!held[i]) memset(want.data() + i * isz, 0, isz);
        }
      }
      // exactly-sized heap blocks: one byte past any of them is a sanitizer report
      std::vector<unsigned char> got(n_items * isz, 0xCC), present(n_items, 0xCC);
      size_t undecodable = 99;
      if (sp_db_read_items(db, 0, n_items, got.data(), got.size(), present.data(), &undecodable) != SP_OK) {
        fprintf(stderr, "sp_db_read_items: %s\n", sp_last_error());
        return 1;
      }
      if (undecodable != 0 || got != want || present != held) {
        if (bad++ < 8) fprintf(stderr, "run %d shard %d: the whole read differs (undecodable %zu)\n", runs, s, undecodable);
      }
      for (size_t i0 = 0; i0 < n_items; i0 += 7) {
        if (i0 >= 35 && i0 + 42 < n_items) continue;   // the first and the last ranges (the last one is short)
        const size_t n = n_items - i0 < 7 ? n_items - i0 : 7;
        std::vector<unsigned char> part(n * isz, 0xCC);
        if (sp_db_read_items(db, i0, n, part.data(), part.size(), nullptr, nullptr) != SP_OK) return 1;
        if (memcmp(part.data(), want.data() + i0 * isz, n * isz) != 0 && bad++ < 8)
          fprintf(stderr, "run %d shard %d: items %zu .. differ\n", runs, s, i0);
      }
      size_t n_held = 0;
      for (size_t i = 0; i < n_items; i++) n_held += held[i];
      std::vector<unsigned char> body(n_held * (8 + isz), 0xCC);   // below sp_db_export_rows_bound: what the held items need
      size_t body_len = 0, records = 0;
      if (sp_db_export_rows(db, 0, n_items, body.data(), body.size(), &body_len, &records) != SP_OK) {
        fprintf(stderr, "sp_db_export_rows: %s\n", sp_last_error());
        return 1;
      }
      size_t off = 0;
      bool body_ok = records == n_held && body_len == body.size();
      for (size_t i = 0; i < n_items && body_ok; i++) {
        if (!held[i]) continue;
        const unsigned char* r = body.data() + off;
        const size_t len = ((size_t)r[0] << 24) | ((size_t)r[1] << 16) | ((size_t)r[2] << 8) | r[3];
        const size_t idx = ((size_t)r[4] << 24) | ((size_t)r[5] << 16) | ((size_t)r[6] << 8) | r[7];
        body_ok = len == 4 + isz && idx == i && memcmp(r + 8, want.data() + i * isz, isz) == 0;
        off += 8 + isz;
      }
      if (!body_ok && bad++ < 8) fprintf(stderr, "run %d shard %d: the exported body differs\n", runs, s);
      sp_db_free(db);
    }
  }
  sp_params_free(p);
  printf("%d runs over %zu items (%s): %s\n", runs, n_items, format, bad ? "MISMATCH" : "every item equal to the file's");
  return bad ? 1 : 0;
}
