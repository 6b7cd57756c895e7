// TEST INFRASTRUCTURE: an item file and one /update-row body on both PLANAR ROW SHARDS of a database through the C ABI
// (sp_db_create_planar_shard, sp_db_load_items: k_db_encode + k_planar_from_stage with the shard's row window and column order;
// sp_db_update_rows: k_db_encode_quads + k_planar_put_items, the other shard's records skipped; sp_db_read_ref: k_planar_read), linked
// against the emulated library (plain or AddressSanitizer build).  No Python in the process.  The pattern of planar_resident_driver.cpp.
//   planar_shard_driver params.json items.bin body.bin expected.bin records num_shards [db_load_window ...]
// items.bin = num_items records of db_item_size bytes; expected.bin = the oracle's words of the edited file, u64 [plane][z in {0, 9,
// 2047}][column ii][row j of the full dim0].  The body is applied once per listed db_load_window (default: the shipped one), each
// time to shards loaded afresh -- every shard takes the whole body -- and every word read back must equal the oracle's.
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
  if (argc < 7) return 2;
  std::vector<unsigned char> json = slurp(argv[1]), items = slurp(argv[2]), body = slurp(argv[3]), want = slurp(argv[4]);
  json.push_back(0);
  const size_t records = (size_t)atol(argv[5]);
  const int S = atoi(argv[6]);
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const int planes = (int)(sp_params_get(p, "instances") * sp_params_get(p, "n") * sp_params_get(p, "n"));
  const int dim0 = 1 << sp_params_get(p, "db_dim_1"), num_per = 1 << sp_params_get(p, "db_dim_2");
  const int nj = dim0 / S;
  const int zs[3] = {0, 9, 2047};
  if (S < 2 || dim0 % S != 0 || want.size() != (size_t)planes * 3 * num_per * dim0 * 8) {
    fprintf(stderr, "expected.bin has %zu bytes\n", want.size());
    return 2;
  }
  int bad = 0, runs = 0;
  for (int a = 7; a < argc || runs == 0; a++, runs++) {
    if (a < argc && sp_debug_set("db_load_window", atol(argv[a])) != SP_OK) return 3;
    for (int s = 0; s < S; s++) {
      sp_db_t* db = sp_db_create_planar_shard(p, s, S);
      if (!db || strcmp(sp_db_format(db), "planar") != 0 || sp_db_load_items(db, items.data(), items.size()) != SP_OK) {
        fprintf(stderr, "load: %s\n", sp_last_error());
        return 3;
      }
      size_t applied = 0, largest = 0;
      if (sp_db_update_rows(db, body.data(), body.size(), &applied, &largest) != SP_OK || applied != records) {
        fprintf(stderr, "sp_db_update_rows: %zu of %zu records applied: %s\n", applied, records, sp_last_error());
        return 1;
      }
      std::vector<uint64_t> got((size_t)nj);
      const unsigned char* w = want.data() + (size_t)s * nj * 8;
      for (int pl = 0; pl < planes; pl++)
        for (int z : zs)
          for (int ii = 0; ii < num_per; ii++, w += (size_t)dim0 * 8) {
            if (sp_db_read_ref(db, pl, z, ii, 0, nj, got.data()) != SP_OK) return 3;
            if (memcmp(got.data(), w, (size_t)nj * 8) != 0) {
              if (bad++ < 8) fprintf(stderr, "run %d shard %d: plane %d z %d column %d differs\n", runs, s, pl, z, ii);
            }
          }
      sp_db_free(db);
    }
  }
  sp_params_free(p);
  printf("%d runs of one body of %zu records on %d shards: %s\n", runs, records, S, bad ? "MISMATCH" : "all words equal to the oracle's");
  return bad ? 1 : 0;
}
