// TEST INFRASTRUCTURE: public parameters kept compact and expanded on the (emulated) device through the C ABI (sp_pp_compact,
// sp_pp_expand, sp_pp_expand_into: k_pp_raw_image, then the launches of sp_pp_deserialize) and compared with this program's own scalar
// restatement of the raw image, linked against the emulated library (plain or AddressSanitizer build).  No Python in the process.  The
// pattern of db_digest_driver.cpp.
//   compact_clients_driver params.json
// Three wire images (pseudo-random words, words >= Q and all-ones among them, under different seeds) are expanded: the first into a
// fresh handle, the others into that handle (a slot) and into a handle of sp_pp_deserialize, in turn.  After each expansion the slot is
// exported into a block of exactly the words a call may write, brought back to coefficients (sp_from_ntt) and compared, word for word,
// with   row 0: Q - (ks % Q) mod Q   other rows: wire word mod Q   -- ks from this program's own one-block ChaCha20.  The export also
// equals sp_pp_deserialize's of the same bytes.  The device keystream (sp_debug_chacha20_u64_device) is read into blocks of exactly
// `count` words.  Every device buffer is a heap block of exactly its size: one word past it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spiral_hip.h"

static const size_t N = 2048;

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

// RFC 8439 block function with rand_chacha's 64-bit counter (words 12 | 13), nonce 0
static uint32_t rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
static void qr(uint32_t* s, int a, int b, int c, int d) {
  s[a] += s[b], s[d] = rotl(s[d] ^ s[a], 16);
  s[c] += s[d], s[b] = rotl(s[b] ^ s[c], 12);
  s[a] += s[b], s[d] = rotl(s[d] ^ s[a], 8);
  s[c] += s[d], s[b] = rotl(s[b] ^ s[c], 7);
}
static void keystream(const unsigned char* seed, uint64_t first_word, uint64_t* out, size_t count) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  memcpy(in + 4, seed, 32);
  in[14] = in[15] = 0;
  for (size_t done = 0; done < count;) {
    const uint64_t word = first_word + done, ctr = word / 8;
    in[12] = (uint32_t)ctr, in[13] = (uint32_t)(ctr >> 32);
    uint32_t s[16];
    memcpy(s, in, sizeof(s));
    for (int r = 0; r < 10; r++) {
      qr(s, 0, 4, 8, 12), qr(s, 1, 5, 9, 13), qr(s, 2, 6, 10, 14), qr(s, 3, 7, 11, 15);
      qr(s, 0, 5, 10, 15), qr(s, 1, 6, 11, 12), qr(s, 2, 7, 8, 13), qr(s, 3, 4, 9, 14);
    }
    for (size_t k = word % 8; k < 8 && done < count; k++, done++)
      out[done] = (uint64_t)(s[2 * k] + in[2 * k]) | ((uint64_t)(s[2 * k + 1] + in[2 * k + 1]) << 32);
  }
}

struct Mat { size_t count, rows, cols; };

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<unsigned char> json = slurp(argv[1]);
  json.push_back(0);
  sp_params_t* p = sp_params_from_json((const char*)json.data());
  if (!p) return 3;
  const auto get = [&](const char* k) { return (size_t)sp_params_get(p, k); };
  const uint64_t Q = sp_params_get(p, "modulus");
  const size_t n = get("n"), tc = get("t_conv"), tl = get("t_exp_left"), tr = get("t_exp_right"), setup = get("setup_bytes");
  std::vector<Mat> mats;   // wire order (client.rs:221-259)
  mats.push_back({n, n + 1, tc});
  if (get("expand_queries")) {
    mats.push_back({get("g"), 2, tl});
    if (get("version") == 0 || tr != tl) mats.push_back({get("stop_round") + 1, 2, tr});
    mats.push_back({1, 2, 2 * tc});
  }
  size_t polys = 0;
  for (const Mat& m : mats) polys += m.count * m.rows * m.cols;

  // the device keystream into blocks of exactly `count` words
  const size_t firsts[3] = {0, 8, 2048 * 3 + 16}, counts[5] = {1, 7, 8, 9, 2051};
  unsigned char seed0[32];
  for (int i = 0; i < 32; i++) seed0[i] = (unsigned char)(7 * i + 1);
  for (size_t first : firsts)
    for (size_t count : counts) {
      std::vector<uint64_t> got(count, 0xCCCCCCCCCCCCCCCCull), want(count);
      keystream(seed0, first, want.data(), count);
      if (sp_debug_chacha20_u64_device(p, seed0, first, got.data(), count) != SP_OK || got != want) {
        fprintf(stderr, "device keystream from word %zu, %zu words: %s\n", first, count, sp_last_error());
        return 1;
      }
    }
  if (sp_debug_chacha20_u64_device(p, seed0, 0, nullptr, 0) != SP_OK || sp_debug_chacha20_u64_device(p, seed0, 4, nullptr, 0) == SP_OK) return 1;

  sp_pp_t* slot = nullptr;
  sp_pp_t* slot2 = nullptr;   // a handle of sp_pp_deserialize used as a slot
  uint64_t x = 0x9E3779B97F4A7C15ull;
  bool ok = true;
  for (int client = 0; client < 3 && ok; client++) {
    std::vector<unsigned char> wire(setup);
    uint64_t* body = nullptr;
    for (size_t b = 0; b < 32; b++) wire[b] = (unsigned char)(client * 41 + b * 3);
    std::vector<uint64_t> words((setup - 32) / 8);
    for (uint64_t& w : words) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      w = client == 2 ? x : x % Q;   // the third client sends any 64-bit word
    }
    words[0] = Q, words[1] = Q - 1, words[2] = ~0ull, words[3] = 0, words[words.size() - 1] = ~0ull;
    body = words.data();
    memcpy(wire.data() + 32, body, words.size() * 8);

    // the image, restated: coefficients mod Q of every polynomial
    std::vector<uint64_t> want(polys * N);
    size_t kpos = 0, wpos = 0, ppos = 0;
    for (const Mat& m : mats)
      for (size_t i = 0; i < m.count; i++) {
        const size_t first = m.cols * N, rest = (m.rows - 1) * m.cols * N;
        keystream(wire.data(), kpos, want.data() + ppos * N, first);
        for (size_t k = 0; k < first; k++) want[ppos * N + k] = (Q - want[ppos * N + k] % Q) % Q;
        for (size_t k = 0; k < rest; k++) want[ppos * N + first + k] = words[wpos + k] % Q;
        kpos += first, wpos += rest, ppos += m.rows * m.cols;
      }
    if (wpos != words.size() || ppos != polys) return 3;

    sp_ppc_t* c = sp_pp_compact(p, wire.data(), wire.size());
    if (!c || sp_ppc_device_bytes(c) < setup || sp_ppc_device_bytes(c) > setup + 4096) {
      fprintf(stderr, "sp_pp_compact: %s\n", sp_last_error());
      return 1;
    }
    sp_pp_t* des = sp_pp_deserialize(p, wire.data(), wire.size());
    if (!des) return 1;
    if (!slot) {
      slot = sp_pp_expand(c);
      slot2 = sp_pp_deserialize(p, wire.data(), wire.size());
      if (!slot || !slot2) {
        fprintf(stderr, "sp_pp_expand: %s\n", sp_last_error());
        return 1;
      }
    }
    for (sp_pp_t* s : {slot, slot2}) {
      if (sp_pp_expand_into(c, s) != SP_OK) {
        fprintf(stderr, "sp_pp_expand_into: %s\n", sp_last_error());
        return 1;
      }
      if (sp_pp_device_bytes(s) != sp_pp_device_bytes(des)) ok = false;
      std::vector<uint64_t> got(polys * 2 * N, 0xCCCCCCCCCCCCCCCCull), ref(polys * 2 * N), coeff(polys * N);
      size_t nw = 0;
      if (sp_pp_export(s, got.data(), got.size(), &nw) != SP_OK || nw != got.size() || sp_pp_export(des, ref.data(), ref.size(), &nw) != SP_OK ||
          sp_from_ntt(p, got.data(), coeff.data(), polys) != SP_OK) {
        fprintf(stderr, "export: %s\n", sp_last_error());
        return 1;
      }
      if (got != ref) {
        fprintf(stderr, "client %d: the expansion differs from sp_pp_deserialize\n", client);
        ok = false;
      }
      if (coeff != want) {
        size_t k = 0;
        while (coeff[k] == want[k]) k++;
        fprintf(stderr, "client %d: polynomial %zu, coefficient %zu differs from the restated image\n", client, k / N, k % N);
        ok = false;
      }
    }
    sp_pp_free(des);
    sp_ppc_free(c);
  }
  // refused: null arguments leave the slot alone
  if (sp_pp_expand_into(nullptr, slot) == SP_OK || sp_pp_expand(nullptr) != nullptr) ok = false;
  sp_pp_free(slot);
  sp_pp_free(slot2);
  sp_params_free(p);
  printf("expansions of %zu polynomials: %s\n", polys, ok ? "equal to the scalar restatement" : "MISMATCH");
  return ok ? 0 : 1;
}
