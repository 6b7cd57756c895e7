// The request layer either side of the answer path: what lib/server's binary does around
// process_query, without the HTTP transport.
//   ServerState            lib/server/src/bin/server.rs:21-28   params + database + RwLock<HashMap<uuid, PublicParameters>>
//   POST /setup            bin/server.rs:71-94    JSON string of base64(public parameters) -> {"uuid":"..."}
//   POST /update-row       bin/server.rs:31-43    raw body of be32 chunk_len | be32 item index | item bytes records, applied under the
//                                                  write side of RwLock<SparseDb> (:24,35) -> sp_db_update_rows: one launch per window
//   POST /private-read     bin/server.rs:98-164   JSON list of base64 requests; request = uuid (36 bytes) || query when the
//                                                  params expand queries, public parameters || query otherwise; the
//                                                  reference answers them one by one (:152-158) -- here the list goes
//                                                  through sp_process_query_batch: <= 8 queries per database pass.
// Uses only the public C ABI (include/spiral_hip.h); framing (JSON list of strings, standard base64 with padding,
// what serde_json / the base64 crate emit) is plain host code.
#include <array>
#include <atomic>
#include <thread>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <sys/random.h>
#include <memory>
#include <mutex>
#include <random>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/spiral_hip.h"

extern "C" void sp_set_last_error_(const char* msg);  // capi.cpp
extern "C" int sp_db_can_replace_(const sp_params_t* params, const sp_db_t* cur, const sp_db_t* next);  // capi_copy.hpp
extern "C" int sp_ppc_assign_(sp_ppc_t* c, const uint8_t* data, size_t len);  // capi_compact.hpp: overwrite a compact handle's image

namespace {

constexpr size_t UUID_V4_STR_BYTES = 36;  // bin/server.rs:96

struct Fail {
  int rc;
  std::string msg;
};

const char B64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

std::string b64_encode(const uint8_t* d, size_t n) {
  std::string out;
  out.reserve((n + 2) / 3 * 4);
  for (size_t i = 0; i < n; i += 3) {
    const uint32_t a = d[i], b = i + 1 < n ? d[i + 1] : 0, c = i + 2 < n ? d[i + 2] : 0;
    const uint32_t v = (a << 16) | (b << 8) | c;
    out += B64[(v >> 18) & 63];
    out += B64[(v >> 12) & 63];
    out += i + 1 < n ? B64[(v >> 6) & 63] : '=';
    out += i + 2 < n ? B64[v & 63] : '=';
  }
  return out;
}

bool b64_decode(const char* s, size_t n, std::vector<uint8_t>& out) {
  // function-local static initialised by a lambda: thread-safe (sp_server_* may be entered concurrently)
  static const std::array<int8_t, 256> tab = [] {
    std::array<int8_t, 256> t;
    t.fill(-1);
    for (int i = 0; i < 64; i++) t[(unsigned char)B64[i]] = (int8_t)i;
    return t;
  }();
  if (n % 4 != 0) return false;
  out.clear();
  out.reserve(n / 4 * 3);
  for (size_t i = 0; i < n; i += 4) {
    int v[4];
    int pad = 0;
    for (int k = 0; k < 4; k++) {
      const char c = s[i + k];
      if (c == '=') {
        if (i + 4 != n || k < 2) return false;
        v[k] = 0;
        pad++;
      } else {
        if (pad) return false;
        v[k] = tab[(unsigned char)c];
        if (v[k] < 0) return false;
      }
    }
    const uint32_t w = ((uint32_t)v[0] << 18) | ((uint32_t)v[1] << 12) | ((uint32_t)v[2] << 6) | (uint32_t)v[3];
    out.push_back((uint8_t)(w >> 16));
    if (pad < 2) out.push_back((uint8_t)(w >> 8));
    if (pad < 1) out.push_back((uint8_t)w);
  }
  return true;
}

void skip_ws(const char*& p, const char* e) {
  while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++;
}
// a JSON string holding base64 text: no escapes other than \/ can occur in what serde_json / JSON.stringify emit for it
bool parse_string(const char*& p, const char* e, std::string& out) {
  skip_ws(p, e);
  if (p >= e || *p != '"') return false;
  p++;
  out.clear();
  while (p < e && *p != '"') {
    if (*p == '\\') {
      if (p + 1 < e && p[1] == '/') {
        out += '/';
        p += 2;
        continue;
      }
      return false;
    }
    out += *p++;
  }
  if (p >= e) return false;
  p++;
  return true;
}
bool parse_string_list(const char* s, size_t n, std::vector<std::string>& out) {
  const char* p = s;
  const char* e = s + n;
  skip_ws(p, e);
  if (p >= e || *p != '[') return false;
  p++;
  skip_ws(p, e);
  out.clear();
  if (p < e && *p == ']') {
    p++;
  } else {
    for (;;) {
      std::string item;
      if (!parse_string(p, e, item)) return false;
      out.push_back(std::move(item));
      skip_ws(p, e);
      if (p < e && *p == ',') {
        p++;
        continue;
      }
      if (p < e && *p == ']') {
        p++;
        break;
      }
      return false;
    }
  }
  skip_ws(p, e);
  return p == e;
}

std::string uuid_v4() {
  // The uuid is the only credential naming a client's resident public parameters in /private-read: 16 bytes from the
  // kernel's CSPRNG, as Uuid::new_v4 in the reference (lib/server/src/bin/server.rs:87), not a seeded Mersenne Twister.
  uint8_t b[16];
  size_t got = 0;
  while (got < sizeof(b)) {
    const ssize_t r = getrandom(b + got, sizeof(b) - got, 0);
    if (r < 0) {
      if (errno == EINTR) continue;
      throw Fail{SP_E_ARG, "getrandom failed"};
    }
    got += (size_t)r;
  }
  b[6] = (uint8_t)((b[6] & 0x0F) | 0x40);  // version 4
  b[8] = (uint8_t)((b[8] & 0x3F) | 0x80);  // RFC 4122 variant
  static const char hex[] = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < 16; i++) {
    if (i == 4 || i == 6 || i == 8 || i == 10) s += '-';
    s += hex[b[i] >> 4];
    s += hex[b[i] & 15];
  }
  return s;
}

}  // namespace

struct sp_server {
  const sp_params_t* params = nullptr;
  const sp_db_t* db = nullptr;
  size_t setup_bytes = 0, query_bytes = 0, response_bytes = 0;
  bool expand_queries = true;
  mutable std::shared_mutex mu;  // bin/server.rs:26 RwLock<HashMap<String, PublicParameters>>
  std::unordered_map<std::string, std::shared_ptr<sp_pp_t>> pub_params;
  // bin/server.rs:24 RwLock<SparseDb>: /private-read holds it shared for its whole list (:102), /update-row exclusively (:35)
  mutable std::shared_mutex db_mu;
  // writers of db_mu that are waiting or at work: a new list stands back while there is one (DbRead), so that lists which overlap without
  // a gap -- two host threads asking in a loop -- cannot keep /update-row or sp_server_replace_db out for ever (the platform's
  // reader-writer lock prefers readers)
  mutable std::atomic<int> db_writers{0};
  // ---- compact registry (sp_server_set_expanded_clients(k > 0)): every client is kept as its wire image on the device, at most
  // max_expanded of them are expanded at a time, into slots the server allocates on first use and keeps.  Everything below is under
  // reg_mu, expansions into slots included: one expansion runs at a time on a device anyway (its staging buffer is the device's one).
  // A request pins the slots it reads until it has been answered; only a slot nobody pins is recycled.
  size_t max_expanded = 0;
  struct Slot {
    std::shared_ptr<sp_pp_t> pp;     // the expanded handle: sp_pp_expand the first time, sp_pp_expand_into from then on
    std::shared_ptr<sp_ppc_t> wire;  // direct-upload params: the slot's own wire buffer (setup_bytes), overwritten per request element
    std::string owner;               // the uuid whose parameters the slot holds; empty: nobody's (never used, forgotten, direct upload)
    int pins = 0;
    uint64_t used = 0;               // the registry's clock at the last hit or expansion; 0 once the owner is forgotten
  };
  mutable std::mutex reg_mu;
  std::unordered_map<std::string, std::shared_ptr<sp_ppc_t>> compact;
  std::unordered_map<std::string, size_t> slot_of;  // the expanded clients
  std::vector<Slot> slots;                          // capacity max_expanded from the start: never reallocated
  uint64_t clock = 0, hits = 0, misses = 0, evictions = 0, overflows = 0;
};

// the read side of db_mu for one list, taken behind every writer that is waiting
struct DbRead {
  std::shared_lock<std::shared_mutex> lk;
  explicit DbRead(const sp_server& s) : lk(s.db_mu, std::defer_lock) {
    while (s.db_writers.load(std::memory_order_acquire) > 0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    lk.lock();
  }
};
// ... and the write side, announced before it is waited for
struct DbWrite {
  const sp_server& s;
  std::unique_lock<std::shared_mutex> lk;
  explicit DbWrite(const sp_server& srv) : s(srv), lk(srv.db_mu, std::defer_lock) {
    s.db_writers.fetch_add(1, std::memory_order_acq_rel);
    lk.lock();
  }
  ~DbWrite() {
    lk.unlock();
    s.db_writers.fetch_sub(1, std::memory_order_acq_rel);
  }
};

template <typename F>
static int guarded_ep(F&& f) {
  try {
    f();
    return SP_OK;
  } catch (const Fail& e) {
    sp_set_last_error_(e.msg.c_str());
    return e.rc;
  } catch (const std::bad_alloc&) {
    sp_set_last_error_("host allocation failed");
    return SP_E_OOM;
  } catch (const std::exception& e) {
    sp_set_last_error_(e.what());
    return SP_E_ARG;
  }
}

static std::shared_ptr<sp_pp_t> deserialize_pp(const sp_server& S, const uint8_t* data, size_t len) {
  if (len != S.setup_bytes)  // bin/server.rs:83 assert_eq!(client_pub_params.len(), data.params.setup_bytes())
    throw Fail{SP_E_ARG, "public parameters: " + std::to_string(len) + " bytes, setup_bytes is " + std::to_string(S.setup_bytes)};
  sp_pp_t* pp = sp_pp_deserialize(S.params, data, len);
  if (!pp) throw Fail{SP_E_ARG, std::string("sp_pp_deserialize: ") + sp_last_error()};
  return std::shared_ptr<sp_pp_t>(pp, [](sp_pp_t* x) { sp_pp_free(x); });
}

static std::shared_ptr<sp_ppc_t> compact_pp(const sp_server& S, const uint8_t* data, size_t len) {
  if (len != S.setup_bytes)
    throw Fail{SP_E_ARG, "public parameters: " + std::to_string(len) + " bytes, setup_bytes is " + std::to_string(S.setup_bytes)};
  sp_ppc_t* c = sp_pp_compact(S.params, data, len);
  if (!c) throw Fail{SP_E_ARG, std::string("sp_pp_compact: ") + sp_last_error()};
  return std::shared_ptr<sp_ppc_t>(c, [](sp_ppc_t* x) { sp_ppc_free(x); });
}
static std::shared_ptr<sp_pp_t> expand_pp(const sp_ppc_t* c) {
  sp_pp_t* pp = sp_pp_expand(c);
  if (!pp) throw Fail{SP_E_ARG, std::string("sp_pp_expand: ") + sp_last_error()};
  return std::shared_ptr<sp_pp_t>(pp, [](sp_pp_t* x) { sp_pp_free(x); });
}

// POST /setup after decoding: the client under a fresh uuid -- expanded (max_expanded = 0) or as its compact image
static std::string register_client(sp_server& S, const uint8_t* data, size_t len) {
  bool compact;
  {
    std::lock_guard<std::mutex> lk(S.reg_mu);
    compact = S.max_expanded > 0;
  }
  if (compact) {
    auto c = compact_pp(S, data, len);
    const std::string id = uuid_v4();
    std::lock_guard<std::mutex> lk(S.reg_mu);
    S.compact[id] = std::move(c);
    return id;
  }
  auto pp = deserialize_pp(S, data, len);
  const std::string id = uuid_v4();
  std::unique_lock<std::shared_mutex> lk(S.mu);
  S.pub_params[id] = std::move(pp);
  return id;
}

// the slots a request has pinned, released when it has been answered (or has failed)
struct Pins {
  sp_server& S;
  std::vector<size_t> held;
  explicit Pins(sp_server& s) : S(s) {}
  ~Pins() {
    std::lock_guard<std::mutex> lk(S.reg_mu);
    for (size_t i : held) S.slots[i].pins--;
  }
};

// a slot for a miss (caller holds reg_mu): an unallocated one, else the least recently used one nobody pins (a forgotten client's
// first), its owner evicted; -1: every slot is pinned
static long take_slot(sp_server& S) {
  long idx = -1;
  if (S.slots.size() < S.max_expanded) {
    S.slots.emplace_back();
    idx = (long)S.slots.size() - 1;
  } else {
    for (size_t i = 0; i < S.slots.size(); i++)
      if (S.slots[i].pins == 0 && (idx < 0 || S.slots[i].used < S.slots[(size_t)idx].used)) idx = (long)i;
  }
  if (idx >= 0 && !S.slots[(size_t)idx].owner.empty()) {
    S.evictions++;
    S.slot_of.erase(S.slots[(size_t)idx].owner);
    S.slots[(size_t)idx].owner.clear();
    S.slots[(size_t)idx].used = 0;
  }
  return idx;
}
// ... and `image` expanded into it (caller holds reg_mu); a failure leaves the slot nobody's
static void fill_slot(sp_server::Slot& sl, const sp_ppc_t* image) {
  if (!sl.pp) {
    sl.pp = expand_pp(image);
  } else if (sp_pp_expand_into(image, sl.pp.get()) != SP_OK) {
    throw Fail{SP_E_ARG, std::string("sp_pp_expand_into: ") + sp_last_error()};
  }
}

// the expanded parameters of client `uuid` for one request: a hit, a miss or an overflow (sp_server_set_expanded_clients)
static std::shared_ptr<sp_pp_t> expanded_client(sp_server& S, const std::string& uuid, int i, Pins& pins) {
  std::shared_ptr<sp_ppc_t> image;
  {
    std::lock_guard<std::mutex> lk(S.reg_mu);
    auto c = S.compact.find(uuid);
    if (c == S.compact.end()) throw Fail{SP_E_NOTFOUND, "request " + std::to_string(i) + ": unknown uuid " + uuid};
    auto it = S.slot_of.find(uuid);
    if (it != S.slot_of.end()) {
      sp_server::Slot& sl = S.slots[it->second];
      S.hits++;
      sl.pins++;
      sl.used = ++S.clock;
      pins.held.push_back(it->second);
      return sl.pp;
    }
    const long idx = take_slot(S);
    if (idx >= 0) {
      sp_server::Slot& sl = S.slots[(size_t)idx];
      fill_slot(sl, c->second.get());
      S.misses++;
      sl.owner = uuid;
      S.slot_of[uuid] = (size_t)idx;
      sl.pins++;
      sl.used = ++S.clock;
      pins.held.push_back((size_t)idx);
      return sl.pp;
    }
    S.overflows++;
    image = c->second;   // (kept past a concurrent forget)
  }
  return expand_pp(image.get());   // dies with the request
}

// direct-upload params with expanded slots: the element's public parameters through the slot's wire buffer into the slot
static std::shared_ptr<sp_pp_t> expanded_upload(sp_server& S, const uint8_t* data, Pins& pins) {
  {
    std::lock_guard<std::mutex> lk(S.reg_mu);
    const long idx = take_slot(S);
    if (idx >= 0) {
      sp_server::Slot& sl = S.slots[(size_t)idx];
      if (!sl.wire)
        sl.wire = compact_pp(S, data, S.setup_bytes);
      else if (sp_ppc_assign_(sl.wire.get(), data, S.setup_bytes) != SP_OK)
        throw Fail{SP_E_ARG, std::string("public parameters: ") + sp_last_error()};
      fill_slot(sl, sl.wire.get());
      S.misses++;
      sl.pins++;
      sl.used = ++S.clock;
      pins.held.push_back((size_t)idx);
      return sl.pp;
    }
    S.overflows++;
  }
  return expand_pp(compact_pp(S, data, S.setup_bytes).get());
}

// the body of private_read for a list of already base64-decoded requests
static void private_read(sp_server& S, const uint8_t* const* reqs, const size_t* lens, int n, uint8_t* out, size_t stride,
                         size_t* out_lens) {
  if (n == 0) return;
  if (stride < S.response_bytes) throw Fail{SP_E_ARG, "out_stride smaller than response_bytes"};
  std::vector<std::shared_ptr<sp_pp_t>> keep((size_t)n);
  std::vector<const sp_pp_t*> pps((size_t)n);
  std::vector<const uint8_t*> qs((size_t)n);
  std::vector<size_t> qlens((size_t)n, S.query_bytes);
  size_t max_expanded;
  {
    std::lock_guard<std::mutex> lk(S.reg_mu);
    max_expanded = S.max_expanded;
  }
  Pins pins(S);   // (released when this function returns or throws: sp_process_query_batch has answered the whole list by then)
  std::unordered_map<std::string, std::shared_ptr<sp_pp_t>> seen;   // one slot per distinct uuid of the list
  for (int i = 0; i < n; i++) {
    if (S.expand_queries) {
      // bin/server.rs:107-121: uuid || query, the uuid names public parameters uploaded through /setup
      if (lens[i] != UUID_V4_STR_BYTES + S.query_bytes)
        throw Fail{SP_E_ARG, "request " + std::to_string(i) + ": " + std::to_string(lens[i]) + " bytes, expected uuid (36) + query_bytes (" +
                                 std::to_string(S.query_bytes) + ")"};
      const std::string uuid((const char*)reqs[i], UUID_V4_STR_BYTES);
      if (max_expanded > 0) {
        auto s = seen.find(uuid);
        keep[i] = s != seen.end() ? s->second : (seen[uuid] = expanded_client(S, uuid, i, pins));
      } else {
        std::shared_lock<std::shared_mutex> lk(S.mu);
        auto it = S.pub_params.find(uuid);
        if (it == S.pub_params.end()) throw Fail{SP_E_NOTFOUND, "request " + std::to_string(i) + ": unknown uuid " + uuid};  // Error::NotFound
        keep[i] = it->second;
      }
      qs[i] = reqs[i] + UUID_V4_STR_BYTES;
    } else {
      // bin/server.rs:123-138: the public parameters travel with the query
      if (lens[i] != S.setup_bytes + S.query_bytes)
        throw Fail{SP_E_ARG, "request " + std::to_string(i) + ": expected setup_bytes + query_bytes"};
      keep[i] = max_expanded > 0 ? expanded_upload(S, reqs[i], pins) : deserialize_pp(S, reqs[i], S.setup_bytes);
      qs[i] = reqs[i] + S.setup_bytes;
    }
    pps[i] = keep[i].get();
  }
  size_t one = 0;
  const int rc = sp_process_query_batch(S.params, pps.data(), qs.data(), qlens.data(), n, S.db, out, stride, &one);
  if (rc != SP_OK) throw Fail{rc, std::string("sp_process_query_batch: ") + sp_last_error()};
  for (int i = 0; i < n; i++) out_lens[i] = one;
}

extern "C" {

sp_server_t* sp_server_create(const sp_params_t* params, const sp_db_t* db) {
  sp_server_t* out = nullptr;
  const int rc = guarded_ep([&] {
    if (!params || !db) throw Fail{SP_E_ARG, "null argument"};
    auto s = std::make_unique<sp_server>();
    s->params = params;
    s->db = db;
    s->setup_bytes = (size_t)sp_params_get(params, "setup_bytes");
    s->query_bytes = (size_t)sp_params_get(params, "query_bytes");
    s->response_bytes = (size_t)sp_params_get(params, "response_bytes");
    s->expand_queries = sp_params_get(params, "expand_queries") != 0;
    out = s.release();
  });
  return rc == SP_OK ? out : nullptr;
}

void sp_server_free(sp_server_t* s) { delete s; }

size_t sp_server_clients(const sp_server_t* s) {
  if (!s) return 0;
  std::shared_lock<std::shared_mutex> lk(s->mu);
  std::lock_guard<std::mutex> reg(s->reg_mu);
  return s->pub_params.size() + s->compact.size();
}

int sp_server_set_expanded_clients(sp_server_t* s, size_t max_expanded) {
  return guarded_ep([&] {
    if (!s) throw Fail{SP_E_ARG, "null argument"};
    std::shared_lock<std::shared_mutex> lk(s->mu);
    std::lock_guard<std::mutex> reg(s->reg_mu);
    if (!s->pub_params.empty() || !s->compact.empty())
      throw Fail{SP_E_ARG, "sp_server_set_expanded_clients: the server has clients (set it before the first /setup)"};
    if (max_expanded < s->slots.size())
      throw Fail{SP_E_ARG, "sp_server_set_expanded_clients: " + std::to_string(s->slots.size()) + " slots are allocated already"};
    s->slots.reserve(max_expanded);
    s->max_expanded = max_expanded;
  });
}

int sp_server_client_stats(const sp_server_t* s, uint64_t out[7]) {
  return guarded_ep([&] {
    if (!s || !out) throw Fail{SP_E_ARG, "null argument"};
    std::shared_lock<std::shared_mutex> lk(s->mu);
    std::lock_guard<std::mutex> reg(s->reg_mu);
    uint64_t bytes = 0;
    for (const auto& kv : s->pub_params) bytes += sp_pp_device_bytes(kv.second.get());
    for (const auto& kv : s->compact) bytes += sp_ppc_device_bytes(kv.second.get());
    for (const auto& sl : s->slots) bytes += sp_pp_device_bytes(sl.pp.get()) + sp_ppc_device_bytes(sl.wire.get());
    out[0] = s->pub_params.size() + s->compact.size();
    out[1] = s->pub_params.size() + s->slot_of.size();
    out[2] = s->hits;
    out[3] = s->misses;
    out[4] = s->evictions;
    out[5] = s->overflows;
    out[6] = bytes;
  });
}

int sp_server_setup(sp_server_t* s, const uint8_t* pp_bytes, size_t len, char* uuid_out37) {
  return guarded_ep([&] {
    if (!s || !pp_bytes || !uuid_out37) throw Fail{SP_E_ARG, "null argument"};
    const std::string id = register_client(*s, pp_bytes, len);
    memcpy(uuid_out37, id.c_str(), UUID_V4_STR_BYTES + 1);
  });
}

int sp_server_forget(sp_server_t* s, const char* uuid) {
  return guarded_ep([&] {
    if (!s || !uuid) throw Fail{SP_E_ARG, "null argument"};
    {
      std::unique_lock<std::shared_mutex> lk(s->mu);
      if (s->pub_params.erase(uuid) != 0) return;
    }
    // a compact client: the image goes; its slot, if it has one, is nobody's and is recycled first, once no request pins it
    std::lock_guard<std::mutex> reg(s->reg_mu);
    if (s->compact.erase(uuid) == 0) throw Fail{SP_E_NOTFOUND, std::string("unknown uuid ") + uuid};
    auto it = s->slot_of.find(uuid);
    if (it != s->slot_of.end()) {
      s->slots[it->second].owner.clear();
      s->slots[it->second].used = 0;
      s->slot_of.erase(it);
    }
  });
}

int sp_server_setup_json(sp_server_t* s, const char* body, size_t body_len, char* out, size_t out_cap, size_t* out_len) {
  return guarded_ep([&] {
    if (!s || !body || !out || !out_len) throw Fail{SP_E_ARG, "null argument"};
    const char* p = body;
    std::string b64;
    if (!parse_string(p, body + body_len, b64)) throw Fail{SP_E_ARG, "/setup body is not a JSON string"};
    skip_ws(p, body + body_len);
    if (p != body + body_len) throw Fail{SP_E_ARG, "/setup body: trailing data"};
    std::vector<uint8_t> raw;
    if (!b64_decode(b64.data(), b64.size(), raw)) throw Fail{SP_E_ARG, "/setup body is not valid base64"};
    char id[UUID_V4_STR_BYTES + 1];
    const std::string u = register_client(*s, raw.data(), raw.size());
    memcpy(id, u.c_str(), UUID_V4_STR_BYTES + 1);
    const std::string resp = std::string("{\"uuid\":\"") + id + "\"}";  // serde_json::to_string(&UuidResponse { uuid })
    if (resp.size() + 1 > out_cap) throw Fail{SP_E_ARG, "output buffer too small"};
    memcpy(out, resp.c_str(), resp.size() + 1);
    *out_len = resp.size();
  });
}

int sp_server_private_read(sp_server_t* s, const uint8_t* const* requests, const size_t* request_lens, int n, uint8_t* out,
                           size_t out_stride, size_t* out_lens) {
  return guarded_ep([&] {
    if (!s || n < 0 || (n > 0 && (!requests || !request_lens || !out || !out_lens))) throw Fail{SP_E_ARG, "null argument"};
    DbRead db_lk(*s);
    private_read(*s, requests, request_lens, n, out, out_stride, out_lens);
  });
}

size_t sp_server_private_read_json_bound(const sp_server_t* s, int n_queries) {
  if (!s || n_queries < 0) return 0;
  return 2 + (size_t)n_queries * ((s->response_bytes + 2) / 3 * 4 + 3) + 1;
}

int sp_server_private_read_json(sp_server_t* s, const char* body, size_t body_len, char* out, size_t out_cap, size_t* out_len) {
  return guarded_ep([&] {
    if (!s || !body || !out || !out_len) throw Fail{SP_E_ARG, "null argument"};
    std::vector<std::string> items;
    if (!parse_string_list(body, body_len, items)) throw Fail{SP_E_ARG, "/private-read body is not a JSON list of strings"};
    const int n = (int)items.size();
    std::vector<std::vector<uint8_t>> raw((size_t)n);
    std::vector<const uint8_t*> reqs((size_t)n);
    std::vector<size_t> lens((size_t)n);
    for (int i = 0; i < n; i++) {
      if (!b64_decode(items[i].data(), items[i].size(), raw[i])) throw Fail{SP_E_ARG, "request " + std::to_string(i) + " is not valid base64"};
      reqs[i] = raw[i].data();
      lens[i] = raw[i].size();
    }
    std::vector<uint8_t> resp((size_t)n * s->response_bytes);
    std::vector<size_t> rl((size_t)n, 0);
    DbRead db_lk(*s);
    private_read(*s, reqs.data(), lens.data(), n, resp.data(), s->response_bytes, rl.data());
    std::string js = "[";  // serde_json::to_string(&Vec<String>)
    for (int i = 0; i < n; i++) {
      if (i) js += ',';
      js += '"';
      js += b64_encode(resp.data() + (size_t)i * s->response_bytes, rl[i]);
      js += '"';
    }
    js += ']';
    if (js.size() + 1 > out_cap) throw Fail{SP_E_ARG, "output buffer too small (see sp_server_private_read_json_bound)"};
    memcpy(out, js.c_str(), js.size() + 1);
    *out_len = js.size();
  });
}

int sp_server_update_row(sp_server_t* s, sp_db_t* db, const uint8_t* body, size_t body_len, char* out, size_t out_cap, size_t* out_len) {
  return guarded_ep([&] {
    if (!s || !db || (!body && body_len) || !out || !out_len) throw Fail{SP_E_ARG, "null argument"};
    const auto t0 = std::chrono::steady_clock::now();
    size_t applied = 0, largest = 0;
    {
      DbWrite db_lk(*s);  // bin/server.rs:35 data.db.write()
      if (db != s->db) throw Fail{SP_E_ARG, "/update-row: db is not the handle this server serves (sp_server_create, sp_server_replace_db)"};
      const int rc = sp_db_update_rows(db, body, body_len, &applied, &largest);
      if (rc != SP_OK) throw Fail{rc, sp_last_error()};
    }
    const long long us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    // bin/server.rs:38-42 format!
    const std::string resp = "{\"status\":\"done updating\", \"loading_time_us\":" + std::to_string(us) + ", \"largest_update\":" +
                             std::to_string(largest) + "}";
    if (resp.size() + 1 > out_cap) throw Fail{SP_E_ARG, "output buffer too small"};
    memcpy(out, resp.c_str(), resp.size() + 1);
    *out_len = resp.size();
  });
}

int sp_server_replace_db(sp_server_t* s, const sp_db_t* new_db) {
  return guarded_ep([&] {
    if (!s || !new_db) throw Fail{SP_E_ARG, "null argument"};
    // the write side: every list in flight has been answered from the old handle, every later one reads the new
    DbWrite db_lk(*s);
    if (!sp_db_can_replace_(s->params, s->db, new_db))
      throw Fail{SP_E_ARG, "sp_server_replace_db: new_db must be an unsharded handle of the server's params on the device of the handle it replaces"};
    s->db = new_db;
  });
}

int sp_server_remove_items(sp_server_t* s, sp_db_t* db, const size_t* item_idx, size_t n, size_t* removed) {
  if (removed) *removed = 0;
  return guarded_ep([&] {
    if (!s || !db || (!item_idx && n)) throw Fail{SP_E_ARG, "null argument"};
    DbWrite db_lk(*s);   // every list in flight has been answered before the removal, every later one is answered after it
    if (db != s->db) throw Fail{SP_E_ARG, "sp_server_remove_items: db is not the handle this server serves (sp_server_create, sp_server_replace_db)"};
    const int rc = sp_db_remove_items(db, item_idx, n, removed);
    if (rc != SP_OK) throw Fail{rc, sp_last_error()};
  });
}

}  // extern "C"
