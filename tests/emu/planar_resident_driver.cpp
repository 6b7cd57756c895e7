// TEST INFRASTRUCTURE: an item file and one /update-row body on a PLANAR-RESIDENT database through the C ABI (sp_db_create_planar,
// sp_db_load_items: k_db_encode + k_planar_from_stage; sp_db_update_rows: k_db_encode_quads + k_planar_put_items; sp_db_read_ref:
// k_planar_read), linked against the emulated library (plain or AddressSanitizer build).  No Python in the process.  The pattern of
// bulk_upsert_driver.cpp.
//   planar_resident_driver params.json items.bin body.bin expected.bin records [db_load_window ...]
// items.bin = num_items records of db_item_size bytes (sp_db_load_items); expected.bin = the oracle's words of the edited file,
// u64 [plane][z in {0, 9, 2047}][column ii][row j].  The body is applied once per listed db_load_window (default: the shipped one),
// each time to a database loaded afresh, and every word read back (sp_db_read_ref) must equal the oracle's.
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
  if (argc < 6) return 2;
  std::vector<unsigned char> json = slurp(argv[1]), items = slurp(argv[2]), body = slurp(argv[3]), want = slurp(argv[4]);
  json.push_back(0);
  const size_t records = (size_t)atol(argv[5]);
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const int planes = (int)(sp_params_get(p, "instances") * sp_params_get(p, "n") * sp_params_get(p, "n"));
  const int dim0 = 1 << sp_params_get(p, "db_dim_1"), num_per = 1 << sp_params_get(p, "db_dim_2");
  const int zs[3] = {0, 9, 2047};
  if (want.size() != (size_t)planes * 3 * num_per * dim0 * 8) {
    fprintf(stderr, "expected.bin has %zu bytes\n", want.size());
    return 2;
  }
  int bad = 0, runs = 0;
  for (int a = 6; a < argc || runs == 0; a++, runs++) {
    if (a < argc && sp_debug_set("db_load_window", atol(argv[a])) != SP_OK) return 3;
    sp_db_t* db = sp_db_create_planar(p);
    if (!db || strcmp(sp_db_format(db), "planar") != 0 || sp_db_load_items(db, items.data(), items.size()) != SP_OK) {
      fprintf(stderr, "load: %s\n", sp_last_error());
      return 3;
    }
    size_t applied = 0, largest = 0;
    if (sp_db_update_rows(db, body.data(), body.size(), &applied, &largest) != SP_OK || applied != records) {
      fprintf(stderr, "sp_db_update_rows: %zu of %zu records applied: %s\n", applied, records, sp_last_error());
      return 1;
    }
    std::vector<uint64_t> got((size_t)dim0);
    const unsigned char* w = want.data();
    for (int pl = 0; pl < planes; pl++)
      for (int z : zs)
        for (int ii = 0; ii < num_per; ii++, w += (size_t)dim0 * 8) {
          if (sp_db_read_ref(db, pl, z, ii, 0, dim0, got.data()) != SP_OK) return 3;
          if (memcmp(got.data(), w, (size_t)dim0 * 8) != 0) {
            if (bad++ < 8) fprintf(stderr, "run %d: plane %d z %d column %d differs\n", runs, pl, z, ii);
          }
        }
    sp_db_free(db);
  }
  sp_params_free(p);
  printf("%d runs of one body of %zu records: %s\n", runs, records, bad ? "MISMATCH" : "all words equal to the oracle's");
  return bad ? 1 : 0;
}
