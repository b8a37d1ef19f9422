// BATCHER CHECK — test infrastructure only.  The Take batcher
// (patrol_amd/csrc/phip_batcher.cpp) on the CPU, over a model engine.
//
// The batcher is host code that reaches the device only through the public C
// ABI, so this program is compiled together with phip_batcher.cpp,
// phip_host.cpp and patrol_oracle.cc and defines the symbols those two product
// files leave open: no GPU, no HIP runtime linked.
//
//   model engine   phip_apply_mixed runs a batch through the oracle's
//                  orc_apply_mixed on one repo, in index order;
//                  phip_apply_mixed_egress does the same and then writes one
//                  datagram per distinct name of the batch, in first-appearance
//                  order: phip_marshal of the name's state after the batch
//                  (n_incast = 0).  phip_egress_caps returns the header's
//                  figures.  phip_take / phip_peek return an error (phip_host.cpp
//                  references them, the batcher never calls them).
//                  hipHostMalloc / hipHostFree / hipGetLastError sit on malloc.
//   knobs          a delay per call; "call k fails with PHIP_ERR_FULL, writing
//                  nothing"; "calls k = r mod m produce eg.n = 0".
//   log            every call: with egress or not, n, the `now` column, a copy
//                  of the egress bytes.  Request id carries now = T0 + id, so
//                  the log is the exact composition and order of every batch.
//                  The engine also checks what it is handed (monotone
//                  name_offs, kind all PHIP_OP_TAKE, result columns present).
//
//   batcher_check NAME | all | list
//
// Every scenario prints one JSON line with "ok", its counts and the times it
// measured; the exit status is non-zero on any failure.  A thread polls
// phip_batcher_stats in a tight loop through every scenario (under
// ThreadSanitizer that is what shows an unlocked counter).  The checks behind
// each scenario are stated at its function.  Built plain by `make`, and by
// hand as batcher_check_tsan / batcher_check_asan (see the Makefile).
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include <unistd.h>

#include <hip/hip_runtime_api.h>

#include "patrolhip.h"

extern "C" {
// patrol_oracle.cc
void* orc_repo_new();
void orc_repo_free(void* r);
void orc_apply_mixed(void* r, const uint8_t* kind, const uint8_t* names, const uint32_t* offs,
                     uint32_t n, const int64_t* now, const int64_t* freq, const int64_t* per,
                     const uint64_t* count, const uint64_t* added, const uint64_t* taken,
                     const int64_t* elapsed, uint8_t* status, uint64_t* remaining,
                     uint64_t* have_bits, uint64_t* reply_added, uint64_t* reply_taken,
                     int64_t* reply_elapsed, int64_t* reply_created);
int orc_get(void* r, const uint8_t* name, uint32_t len, uint64_t* added, uint64_t* taken,
            int64_t* elapsed, int64_t* created);
int64_t orc_dump(void* r, uint8_t* names, uint64_t cap, uint64_t* offs, uint64_t* added,
                 uint64_t* taken, int64_t* elapsed, int64_t* created, uint64_t max_n);
}

namespace {

using Clock = std::chrono::steady_clock;
constexpr int64_t T0 = 1700000000000000000ll;
constexpr double kBoundMs = 2000.0;   // the bound set against the 10 s window
constexpr uint32_t kLongWindowUs = 10u * 1000u * 1000u;

double ms_since(Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}
void sleep_us(uint32_t us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

// ------------------------------------------------------------ reporting ----
struct Report {
  std::mutex mu;
  std::vector<std::string> errs;   // the first few, in full
  uint64_t failures = 0;
  std::ostringstream extra;        // further JSON fields of the scenario (main thread only)
  std::string scenario;
  Clock::time_point t0;
  uint64_t requests = 0, calls = 0, max_batch = 0;   // summed by verify()

  void fail(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> l(mu);
    if (++failures <= 8) errs.push_back(buf);
  }
  // the scenario's JSON line (under mu: the watchdog may print it too)
  void print(bool timed_out) {
    std::lock_guard<std::mutex> l(mu);
    std::string e;
    for (const std::string& s : errs) {
      e += e.empty() ? "\"" : ", \"";
      for (char c : s) e += (c == '"' || c == '\\' || (unsigned char)c < 0x20) ? '\'' : c;
      e += "\"";
    }
    printf("{\"scenario\": \"%s\", \"ok\": %s, \"ms\": %.1f, \"requests\": %llu, "
           "\"engine_calls\": %llu, \"largest_batch\": %llu%s, \"failures\": %llu, "
           "\"errors\": [%s]%s}\n",
           scenario.c_str(), (failures == 0 && !timed_out) ? "true" : "false", ms_since(t0),
           (unsigned long long)requests, (unsigned long long)calls, (unsigned long long)max_batch,
           extra.str().c_str(), (unsigned long long)failures, e.c_str(),
           timed_out ? ", \"watchdog\": true" : "");
    fflush(stdout);
  }
};
Report* g_rep = nullptr;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) g_rep->fail(__VA_ARGS__); \
  } while (0)

// One call of the model engine, as logged.
struct Call {
  bool egress = false, failed = false;
  uint32_t n = 0;
  std::vector<int64_t> now;
  uint32_t eg_n = 0;
  std::vector<uint8_t> bytes;    // [0, offs[eg_n])
  std::vector<uint64_t> offs;    // eg_n + 1 entries
};

}  // namespace

// ------------------------------------------------------------ model engine ----
struct phip_handle {
  void* repo = nullptr;
  std::mutex mu;                 // held through a call, as the engine's own mutex is
  std::vector<Call> log;
  uint64_t violations = 0;
  // knobs, set before the batcher opens
  uint32_t delay_us = 0;
  int64_t fail_call = -1;                  // this call returns PHIP_ERR_FULL, writing nothing
  uint32_t zero_mod = 0, zero_rem = 0;     // calls k with k % zero_mod == zero_rem: eg.n = 0
};

namespace {

int engine(phip_handle* h, const phip_ops* ops, const phip_results* res, phip_egress* eg) {
  if (eg) {
    eg->n = eg->n_incast = 0;
    eg->bytes = 0;
  }
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> l(h->mu);
  bool bad = !ops || !res || !res->status || !res->remaining || !res->reply;
  if (!bad && ops->n)
    bad = !ops->kind || !ops->names || !ops->name_offs || !ops->now || !ops->freq || !ops->per ||
          !ops->count;
  const uint32_t n = bad ? 0 : ops->n;
  for (uint32_t i = 0; i < n && !bad; ++i)
    bad = ops->kind[i] != PHIP_OP_TAKE || ops->name_offs[i + 1] < ops->name_offs[i] ||
          ops->name_offs[i + 1] - ops->name_offs[i] > PHIP_MAX_NAME_LEN;
  if (!bad && eg) {
    const uint64_t need = n ? 25ull * n + (ops->name_offs[n] - ops->name_offs[0]) : 0;
    bad = !eg->out || !eg->offs || eg->max_msgs < n || eg->out_cap < need;
  }
  if (bad) {
    ++h->violations;
    return PHIP_ERR_INVALID;
  }
  const uint64_t k = h->log.size();
  Call c;
  c.egress = eg != nullptr;
  c.n = n;
  c.now.assign(ops->now, ops->now + n);
  if (h->delay_us) sleep_us(h->delay_us);
  if ((int64_t)k == h->fail_call) {
    c.failed = true;
    h->log.push_back(std::move(c));
    return PHIP_ERR_FULL;
  }
  std::vector<uint64_t> ra(n), rt(n);
  std::vector<int64_t> re(n), rc(n);
  orc_apply_mixed(h->repo, ops->kind, ops->names, ops->name_offs, n, ops->now, ops->freq, ops->per,
                  ops->count, nullptr, nullptr, nullptr, res->status, res->remaining, nullptr,
                  ra.data(), rt.data(), re.data(), rc.data());
  for (uint32_t i = 0; i < n; ++i) res->reply[i] = phip_state{ra[i], rt[i], re[i], rc[i]};
  if (eg) {
    uint64_t o = 0;
    uint32_t nd = 0;
    eg->offs[0] = 0;
    if (!(h->zero_mod && k % h->zero_mod == h->zero_rem)) {
      std::unordered_set<std::string> seen;
      for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* nm = ops->names + ops->name_offs[i];
        const uint32_t len = ops->name_offs[i + 1] - ops->name_offs[i];
        if (!seen.emplace((const char*)nm, len).second) continue;
        phip_state st{};
        orc_get(h->repo, nm, len, &st.added, &st.taken, &st.elapsed, &st.created);
        o += (uint64_t)phip_marshal(nm, len, &st, eg->out + o);
        eg->offs[++nd] = o;
      }
    }
    eg->n = nd;
    eg->bytes = o;
    c.eg_n = nd;
    c.bytes.assign(eg->out, eg->out + o);
    c.offs.assign(eg->offs, eg->offs + nd + 1);
  }
  h->log.push_back(std::move(c));
  return PHIP_OK;
}

}  // namespace

extern "C" {

int phip_apply_mixed(phip_handle* h, const phip_ops* ops, const phip_results* res, uint32_t) {
  return engine(h, ops, res, nullptr);
}

int phip_apply_mixed_egress(phip_handle* h, const phip_ops* ops, const phip_results* res,
                            phip_egress* eg, uint32_t) {
  if (!eg) return PHIP_ERR_INVALID;
  return engine(h, ops, res, eg);
}

int phip_egress_caps(uint32_t n_ops, uint64_t name_bytes, uint32_t, uint32_t* max_msgs,
                     uint64_t* out_cap) {
  if (!max_msgs || !out_cap) return PHIP_ERR_INVALID;
  *max_msgs = 2 * n_ops;
  *out_cap = 2 * (25ull * n_ops + name_bytes);
  return PHIP_OK;
}

int phip_take(phip_handle*, const uint8_t*, const uint32_t*, uint32_t, const int64_t*,
              const int64_t*, const int64_t*, const uint64_t*, uint64_t*, uint8_t*, uint32_t) {
  return PHIP_ERR_INVALID;
}

int phip_peek(phip_handle*, const phip_ops*, const phip_peek_results*, uint32_t) {
  return PHIP_ERR_INVALID;
}

hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
  *ptr = malloc(size);
  return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* ptr) {
  free(ptr);
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }

}  // extern "C"

namespace {

// --------------------------------------------------------- stats poller ----
// Polls phip_batcher_stats of every registered batcher in a tight loop; every
// figure is a running total or a maximum, so none may ever go down.
struct Poller {
  std::mutex mu;
  std::vector<std::pair<phip_batcher*, std::array<uint64_t, 8>>> bs;
  std::atomic<bool> hold{false}, quit{false};
  std::atomic<uint64_t> polls{0};
  std::thread th;

  void start() {
    th = std::thread([this] {
      while (!quit.load()) {
        if (!hold.load()) {
          std::lock_guard<std::mutex> l(mu);
          for (auto& e : bs) {
            std::array<uint64_t, 8> v{};
            const int k = phip_batcher_stats(e.first, v.data(), 8);
            CHECK(k == 8, "phip_batcher_stats wrote %d figures", k);
            for (int i = 0; i < 8; ++i)
              CHECK(v[i] >= e.second[i], "stats out[%d] went down: %llu -> %llu", i,
                    (unsigned long long)e.second[i], (unsigned long long)v[i]);
            e.second = v;
            polls.fetch_add(1, std::memory_order_relaxed);
          }
        }
        std::this_thread::yield();
      }
    });
  }
  void stop() {
    quit.store(true);
    th.join();
  }
  // (main thread only; `hold` lets it past a poller that never leaves the mutex for long)
  void add(phip_batcher* b) {
    hold.store(true);
    {
      std::lock_guard<std::mutex> l(mu);
      bs.emplace_back(b, std::array<uint64_t, 8>{});
    }
    hold.store(false);
  }
  void remove(phip_batcher* b) {
    hold.store(true);
    {
      std::lock_guard<std::mutex> l(mu);
      for (size_t i = 0; i < bs.size(); ++i)
        if (bs[i].first == b) bs.erase(bs.begin() + i--);
    }
    hold.store(false);
  }
};
Poller g_poll;

// ------------------------------------------------------------- requests ----
// About 20 names: the empty one, a 231-byte one, inline-sized (<= 22 bytes)
// and longer ones, bytes outside ASCII.
const std::vector<std::string>& names() {
  static const std::vector<std::string> v = [] {
    std::vector<std::string> n;
    n.push_back("");
    std::string big(PHIP_MAX_NAME_LEN, 'x');
    for (size_t i = 0; i < big.size(); ++i) big[i] = (char)('a' + i % 26);
    n.push_back(big);
    n.push_back("a");
    n.push_back("b");
    n.push_back(std::string("\0", 1));
    n.push_back(std::string("\0\0", 2));
    n.push_back("\xff\xfe\x80");
    n.push_back(std::string(22, 'q'));
    n.push_back(std::string(23, 'q'));
    n.push_back(big.substr(0, 230));
    for (int i = 0; i < 10; ++i) n.push_back("user:" + std::to_string(i * 7919));
    return n;
  }();
  return v;
}

struct Spec {
  uint32_t name;
  int64_t freq, per;
  uint64_t count;
};
struct Out {
  int rc = 1;   // (no entry point returns 1)
  uint64_t remaining = 0, seq = ~0ull;
  uint8_t ok = 0;
  uint64_t eg_seen = 0;   // stats out[5] read right after the take returned
  phip_take_reply reply{};
};

// One model engine, one batcher over it, the requests sent and what came back.
struct World {
  phip_handle h;
  phip_batcher* b = nullptr;
  bool egress = false;
  std::vector<Spec> reqs;
  std::vector<Out> outs;
  std::atomic<uint32_t> entered{0}, returned{0};
  uint64_t stats[8] = {};
  double close_ms = 0;

  World() { h.repo = orc_repo_new(); }
  ~World() {
    if (b) close();
    orc_repo_free(h.repo);
  }
  World(const World&) = delete;

  void make_reqs(uint32_t n, uint64_t seed) {
    static const int64_t rates[][2] = {{100, 1000000000ll}, {5, 1000000000ll}, {0, 1000000000ll},
                                       {3, 60000000000ll},  {1, 1},            {7, 0},
                                       {1000, 1000000ll}};
    std::mt19937_64 rng(seed);
    const uint32_t nn = (uint32_t)names().size();
    reqs.resize(n);
    outs.assign(n, Out{});
    for (Spec& s : reqs) {
      // half of the traffic on four names, so that batches repeat names
      s.name = (rng() & 1) ? (uint32_t)(rng() % 4) : (uint32_t)(rng() % nn);
      const auto& r = rates[rng() % (sizeof rates / sizeof rates[0])];
      s.freq = r[0];
      s.per = r[1];
      s.count = rng() % 4;   // 0 included
    }
  }
  void open(uint32_t window_us, uint32_t max_batch, uint32_t ring) {
    phip_batcher_config cfg{window_us, max_batch};
    egress = ring != 0;
    const int rc = ring ? phip_batcher_open_egress(&h, &cfg, ring, &b) : phip_batcher_open(&h, &cfg, &b);
    CHECK(rc == PHIP_OK && b, "batcher open: rc %d", rc);
    if (rc != PHIP_OK || !b) {
      g_rep->print(false);
      exit(1);
    }
    g_poll.add(b);
  }
  void close() {
    phip_batcher_stats(b, stats, 8);
    g_poll.remove(b);
    const auto t0 = Clock::now();
    phip_batcher_close(b);
    close_ms = ms_since(t0);
    b = nullptr;
  }
  void take(uint32_t id, bool reply) {
    const Spec& s = reqs[id];
    Out& o = outs[id];
    const std::string& nm = names()[s.name];
    const uint8_t* p = (const uint8_t*)nm.data();
    if (reply) {
      o.rc = phip_batcher_take_reply(b, p, (uint32_t)nm.size(), T0 + id, s.freq, s.per, s.count,
                                     &o.reply);
      if (o.rc == PHIP_OK) {
        o.remaining = o.reply.remaining;
        o.ok = o.reply.ok;
        o.seq = o.reply.seq;
      }
    } else {
      o.rc = phip_batcher_take(b, p, (uint32_t)nm.size(), T0 + id, s.freq, s.per, s.count,
                               &o.remaining, &o.ok, &o.seq);
    }
    if (egress) {
      uint64_t st[8];
      phip_batcher_stats(b, st, 8);
      o.eg_seen = st[5];
    }
    returned.fetch_add(1);
  }
  size_t calls() {
    std::lock_guard<std::mutex> l(h.mu);
    return h.log.size();
  }
};

// `threads` takers, thread t issuing requests [t * per, (t + 1) * per) one after
// another, all released together; thread t then waits t * stagger_us before its
// first take.  *released (may be null) is the release time.
std::vector<std::thread> start_takers(World& w, uint32_t threads, uint32_t per, bool reply,
                                      Clock::time_point* released = nullptr, uint32_t stagger_us = 0) {
  auto go = std::make_shared<std::atomic<bool>>(false);
  auto ready = std::make_shared<std::atomic<uint32_t>>(0);
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < threads; ++t)
    th.emplace_back([&w, t, per, reply, go, ready, stagger_us] {
      ready->fetch_add(1);
      while (!go->load(std::memory_order_acquire)) std::this_thread::yield();
      if (stagger_us) sleep_us(t * stagger_us);
      for (uint32_t j = 0; j < per; ++j) {
        if (j == 0) w.entered.fetch_add(1);
        w.take(t * per + j, reply);
      }
    });
  while (ready->load() < threads) std::this_thread::yield();
  if (released) *released = Clock::now();
  go->store(true, std::memory_order_release);
  return th;
}
void join_all(std::vector<std::thread>& th) {
  for (auto& t : th) t.join();
  th.clear();
}
// Waits (at most bound_ms) until pred(); true when it held.
template <class P>
bool wait_for(P pred, double bound_ms = kBoundMs) {
  const auto t0 = Clock::now();
  while (!pred()) {
    if (ms_since(t0) > bound_ms) return false;
    sleep_us(200);
  }
  return true;
}

struct Row {
  std::string name;
  uint64_t a, t;
  int64_t e, c;
  bool operator==(const Row& o) const {
    return name == o.name && a == o.a && t == o.t && e == o.e && c == o.c;
  }
};
std::vector<Row> dump(void* repo) {
  std::vector<uint8_t> nb(1 << 16);
  uint64_t offs[129], a[128], t[128];
  int64_t e[128], c[128];
  const int64_t n = orc_dump(repo, nb.data(), nb.size(), offs, a, t, e, c, 128);
  std::vector<Row> v;
  for (int64_t i = 0; i < n; ++i)
    v.push_back({std::string((const char*)nb.data() + offs[i], offs[i + 1] - offs[i]), a[i], t[i], e[i], c[i]});
  CHECK(n >= 0, "oracle dump does not fit");
  return v;
}

// What the engine log says about the run, shared by verify() and verify_egress().
struct Order {
  std::vector<uint32_t> ids;        // the concatenated log: request ids in engine order
  std::vector<int64_t> call_of;     // per request: its call, -1 when the log lacks it
  std::vector<uint64_t> pos;        // per request: its place in `ids`
  std::vector<uint64_t> first_pos;  // per call: the place of its first request
};
Order log_order(World& w) {
  Order o;
  const size_t nreq = w.reqs.size();
  o.call_of.assign(nreq, -1);
  o.pos.assign(nreq, 0);
  for (size_t ci = 0; ci < w.h.log.size(); ++ci) {
    const Call& c = w.h.log[ci];
    o.first_pos.push_back(o.ids.size());
    CHECK(c.n > 0, "call %zu ran an empty batch", ci);
    for (int64_t now : c.now) {
      const int64_t id = now - T0;
      if (id < 0 || (size_t)id >= nreq) {
        CHECK(false, "call %zu holds an unknown request (now - T0 = %lld)", ci, (long long)id);
        continue;
      }
      CHECK(o.call_of[id] < 0, "request %lld is in the log twice", (long long)id);
      o.call_of[id] = (int64_t)ci;
      o.pos[id] = o.ids.size();
      o.ids.push_back((uint32_t)id);
    }
  }
  return o;
}

// The core check, after the batcher is closed.  `sent`: how many of w.reqs were
// issued (the first `sent` ids).
//  - the log holds every issued request exactly once;
//  - a request returns PHIP_ERR_FULL exactly when its call is the failed one, else 0;
//  - seq equals the request's place in the concatenated log (so the seqs of an
//    unfailed run are a permutation of 0..n-1 and the log is in seq order);
//  - (remaining, ok) -- and with `reply` state, created, datagram -- equal a fresh
//    oracle applying the surviving requests one by one in that order;
//  - the engine's final table equals that oracle's.
Order verify(World& w, bool reply, uint32_t sent) {
  std::lock_guard<std::mutex> l(w.h.mu);
  CHECK(w.h.violations == 0, "the engine was handed %llu malformed calls",
        (unsigned long long)w.h.violations);
  Order o = log_order(w);
  CHECK(o.ids.size() == sent, "the log holds %zu requests, %u were issued", o.ids.size(), sent);
  uint64_t largest = 0;
  for (const Call& c : w.h.log) largest = std::max<uint64_t>(largest, c.n);
  g_rep->requests += sent;
  g_rep->calls += w.h.log.size();
  g_rep->max_batch = std::max(g_rep->max_batch, largest);
  for (uint32_t id = 0; id < sent; ++id) {
    const Out& r = w.outs[id];
    if (o.call_of[id] < 0) {
      CHECK(false, "request %u never reached the engine (rc %d)", id, r.rc);
      continue;
    }
    const bool failed = w.h.log[o.call_of[id]].failed;
    CHECK(r.rc == (failed ? PHIP_ERR_FULL : PHIP_OK), "request %u in call %lld: rc %d", id,
          (long long)o.call_of[id], r.rc);
    if (!failed && r.rc == PHIP_OK)
      CHECK(r.seq == o.pos[id], "request %u: seq %llu, place in the log %llu", id,
            (unsigned long long)r.seq, (unsigned long long)o.pos[id]);
  }
  void* ref = orc_repo_new();
  for (uint32_t id : o.ids) {
    if (w.h.log[o.call_of[id]].failed) continue;
    const Spec& s = w.reqs[id];
    const Out& r = w.outs[id];
    const std::string& nm = names()[s.name];
    const uint8_t kind = PHIP_OP_TAKE;
    const uint32_t offs[2] = {0, (uint32_t)nm.size()};
    const int64_t now = T0 + id;
    uint8_t st = 0;
    uint64_t rem = 0;
    phip_state ps{};
    orc_apply_mixed(ref, &kind, (const uint8_t*)nm.data(), offs, 1, &now, &s.freq, &s.per, &s.count,
                    nullptr, nullptr, nullptr, &st, &rem, nullptr, &ps.added, &ps.taken, &ps.elapsed,
                    &ps.created);
    if (r.rc != PHIP_OK) continue;
    const uint8_t ok = (st & 0x7F) == PHIP_ST_TAKE_OK;
    CHECK(r.remaining == rem && r.ok == ok, "request %u: (remaining, ok) = (%llu, %d), oracle (%llu, %d)",
          id, (unsigned long long)r.remaining, r.ok, (unsigned long long)rem, ok);
    if (reply) {
      const phip_take_reply& p = r.reply;
      CHECK(std::memcmp(&p.state, &ps, sizeof ps) == 0, "request %u: reply state differs", id);
      CHECK(p.created == ((st & PHIP_ST_CREATED) ? 1 : 0), "request %u: created %d", id, p.created);
      uint8_t dg[PHIP_BUCKET_PACKET_SIZE];
      const int sz = phip_marshal((const uint8_t*)nm.data(), (uint32_t)nm.size(), &ps, dg);
      CHECK(sz == 25 + (int)nm.size() && p.datagram_len == sz && std::memcmp(p.datagram, dg, sz) == 0,
            "request %u: reply datagram differs (len %d, oracle %d)", id, p.datagram_len, sz);
    }
  }
  CHECK(dump(ref) == dump(w.h.repo), "the engine's final table differs from the oracle's");
  orc_repo_free(ref);
  return o;
}

// --------------------------------------------------------------- egress ----
struct Drained {
  uint64_t batch, first_seq;
  uint32_t requests, n, n_incast;
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> offs;
};
struct Drain {
  std::mutex mu;
  std::vector<Drained> got;
  std::vector<uint64_t> done_order;
  std::atomic<bool> stop{false};   // set once every taker has returned
};

Drained copy_batch(const phip_egress_batch& eb) {
  Drained d{eb.batch, eb.first_seq, eb.requests, eb.n, eb.n_incast, {}, {}};
  d.offs.assign(eb.offs, eb.offs + eb.n + 1);
  d.bytes.assign(eb.bytes, eb.bytes + eb.offs[eb.n]);
  return d;
}
bool same_as_slot(const Drained& d, const phip_egress_batch& eb) {
  return std::memcmp(eb.offs, d.offs.data(), d.offs.size() * 8) == 0 &&
         std::memcmp(eb.bytes, d.bytes.data(), d.bytes.size()) == 0;
}

// A drainer: takes a batch, copies it, holds the slot for hold_us, compares the
// slot with the copy again (a slot reused while handed out shows here), gives
// it back.  Ends when `stop` is set and nothing is queued any more.
void drainer(World& w, Drain& D, uint32_t hold_us) {
  for (;;) {
    phip_egress_batch eb;
    const int r = phip_batcher_egress_next(w.b, 5, &eb);
    if (r < 0) {
      CHECK(false, "egress_next: %d", r);
      return;
    }
    if (r == 0) {
      if (D.stop.load()) return;
      continue;
    }
    Drained d = copy_batch(eb);
    if (hold_us) sleep_us(hold_us);
    CHECK(same_as_slot(d, eb), "batch %llu: its slot changed while it was handed out",
          (unsigned long long)eb.batch);
    std::lock_guard<std::mutex> l(D.mu);   // (done inside: done_order is the order of the calls)
    const int rc = phip_batcher_egress_done(w.b, eb.batch);
    CHECK(rc == PHIP_OK, "egress_done(%llu): %d", (unsigned long long)eb.batch, rc);
    D.done_order.push_back(eb.batch);
    D.got.push_back(std::move(d));
  }
}

// After close.  The calls that queued egress are those with egress, no failure
// and n > 0 datagrams, in log order; the k-th of them is batch k.
//  - every batch number 0..m-1 came out exactly once (with `complete`: m is all of them);
//  - n, n_incast, requests, first_seq, offs and bytes equal the log's;
//  - first_seq rises strictly; requests sum to the requests of those calls;
//  - stats: out[5] = queued batches, out[6] = their datagrams;
//  - each taker's out[5] reading was at least its own batch's 1-based number.
void verify_egress(World& w, const Order& o, std::vector<Drained> got, bool complete) {
  std::sort(got.begin(), got.end(), [](const Drained& a, const Drained& b) { return a.batch < b.batch; });
  std::vector<size_t> queued;
  std::vector<uint64_t> number(w.h.log.size(), 0);   // per call: 1-based egress number, 0 none
  uint64_t datagrams = 0, reqsum = 0;
  for (size_t ci = 0; ci < w.h.log.size(); ++ci) {
    const Call& c = w.h.log[ci];
    if (c.egress && !c.failed && c.eg_n) {
      queued.push_back(ci);
      number[ci] = queued.size();
      datagrams += c.eg_n;
    }
  }
  if (complete)
    CHECK(got.size() == queued.size(), "%zu batches came out, %zu were queued", got.size(), queued.size());
  CHECK(got.size() <= queued.size(), "%zu batches came out, only %zu were queued", got.size(), queued.size());
  for (size_t k = 0; k < got.size() && k < queued.size(); ++k) {
    const Drained& d = got[k];
    const Call& c = w.h.log[queued[k]];
    CHECK(d.batch == k, "egress batch %zu carries number %llu", k, (unsigned long long)d.batch);
    CHECK(d.n == c.eg_n && d.n_incast == 0 && d.requests == c.n, "batch %zu: n %u incast %u requests %u, log %u 0 %u",
          k, d.n, d.n_incast, d.requests, c.eg_n, c.n);
    CHECK(d.first_seq == o.first_pos[queued[k]], "batch %zu: first_seq %llu, log %llu", k,
          (unsigned long long)d.first_seq, (unsigned long long)o.first_pos[queued[k]]);
    if (k) CHECK(d.first_seq > got[k - 1].first_seq, "batch %zu: first_seq does not rise", k);
    CHECK(d.offs == c.offs && d.bytes == c.bytes, "batch %zu: bytes differ from the engine's copy", k);
    reqsum += d.requests;
  }
  if (complete) {
    uint64_t want = 0;
    for (size_t ci : queued) want += w.h.log[ci].n;
    CHECK(reqsum == want, "requests fields sum to %llu, the queued calls held %llu",
          (unsigned long long)reqsum, (unsigned long long)want);
  }
  CHECK(w.stats[5] == queued.size() && w.stats[6] == datagrams, "stats out[5] %llu out[6] %llu, log %zu %llu",
        (unsigned long long)w.stats[5], (unsigned long long)w.stats[6], queued.size(),
        (unsigned long long)datagrams);
  for (size_t id = 0; id < w.outs.size(); ++id) {
    if (w.outs[id].rc != PHIP_OK || o.call_of[id] < 0) continue;
    const uint64_t mine = number[o.call_of[id]];
    CHECK(w.outs[id].eg_seen >= mine, "request %zu returned with out[5] = %llu before its batch's egress (%llu) was queued",
          id, (unsigned long long)w.outs[id].eg_seen, (unsigned long long)mine);
  }
}

// ------------------------------------------------------------ scenarios ----

// 16 threads x 100 takes over the names, mixed rates (freq = 0 included), with
// window_us 0 and 50, through phip_batcher_take and phip_batcher_take_reply:
// verify(), the seqs a permutation, the stats, and a 232-byte name refused
// before any engine call.
void sc_order() {
  const uint32_t T = 16, PER = 100, N = T * PER;
  for (uint32_t window : {0u, 50u})
    for (bool reply : {false, true}) {
      World w;
      w.make_reqs(N, 11 + window + reply);
      w.open(window, 0, 0);
      const std::string big(PHIP_MAX_NAME_LEN + 1, 'z');
      uint64_t rem = 7, seq = 7;
      uint8_t ok = 7;
      phip_take_reply tr;
      const int rc1 = phip_batcher_take(w.b, (const uint8_t*)big.data(), 232, T0, 1, 1, 1, &rem, &ok, &seq);
      const int rc2 = phip_batcher_take_reply(w.b, (const uint8_t*)big.data(), 232, T0, 1, 1, 1, &tr);
      CHECK(rc1 == PHIP_ERR_NAME_TOO_LARGE && rc2 == PHIP_ERR_NAME_TOO_LARGE && w.calls() == 0,
            "232-byte name: rc %d / %d, %zu engine calls", rc1, rc2, w.calls());
      auto th = start_takers(w, T, PER, reply);
      join_all(th);
      w.close();
      verify(w, reply, N);
      std::vector<uint64_t> seqs;
      for (const Out& o : w.outs) seqs.push_back(o.seq);
      std::sort(seqs.begin(), seqs.end());
      bool perm = true;
      for (uint32_t i = 0; i < N; ++i) perm = perm && seqs[i] == i;
      CHECK(perm, "the seqs are no permutation of 0..%u", N - 1);
      uint64_t largest = 0;
      for (const Call& c : w.h.log) largest = std::max<uint64_t>(largest, c.n);
      CHECK(w.stats[0] == w.h.log.size() && w.stats[1] == N && w.stats[2] == largest && w.stats[4] == 0,
            "stats %llu %llu %llu errors %llu; log: %zu calls, largest %llu",
            (unsigned long long)w.stats[0], (unsigned long long)w.stats[1], (unsigned long long)w.stats[2],
            (unsigned long long)w.stats[4], w.h.log.size(), (unsigned long long)largest);
    }
}

// window 10 s, max_batch 8.  8 threads released together all return within 2 s
// (waiting the window out cannot pass); with 64 threads no logged batch holds
// more than 8 requests, and they too return within 2 s (64 = 8 full batches).
// Each once with the takers arriving in one burst and once a little apart: in
// a burst the dispatcher may find all 8 queued at its first look, apart it is
// already waiting for the window when the 8th arrives and has to be woken.
void sc_max_batch() {
  for (uint32_t T : {8u, 64u})
    for (uint32_t stagger : {0u, T == 8 ? 1000u : 200u}) {
      World w;
      w.make_reqs(T, 21 + T);
      w.open(kLongWindowUs, 8, 0);
      Clock::time_point t0;
      auto th = start_takers(w, T, 1, false, &t0, stagger);
      join_all(th);
      const double ms = ms_since(t0);
      CHECK(ms < kBoundMs, "%u takers, %u us apart, took %.1f ms to return (window 10 s, max_batch 8)", T,
            stagger, ms);
      g_rep->extra << ", \"return_ms_" << T << (stagger ? "_apart" : "_burst") << "\": " << ms;
      w.close();
      verify(w, false, T);
      for (const Call& c : w.h.log) CHECK(c.n <= 8, "a batch of %u requests with max_batch 8", c.n);
    }
}

// Call 3 fails with PHIP_ERR_FULL: exactly its callers get the error (verify()),
// out[4] == 1; with egress the failed batch consumes no batch number.
void sc_engine_error() {
  for (uint32_t ring : {0u, 4u}) {
    const uint32_t T = 8, PER = 50;
    World w;
    w.make_reqs(T * PER, 31 + ring);
    w.h.fail_call = 3;
    w.h.delay_us = 20;
    w.open(50, 0, ring);
    Drain D;
    std::thread dr;
    if (ring) dr = std::thread(drainer, std::ref(w), std::ref(D), 0);
    auto th = start_takers(w, T, PER, false);
    join_all(th);
    D.stop.store(true);
    if (ring) dr.join();
    w.close();
    const Order o = verify(w, false, T * PER);
    uint32_t refused = 0;
    for (const Out& r : w.outs) refused += r.rc == PHIP_ERR_FULL;
    const bool ran = w.h.log.size() > 3 && w.h.log[3].failed;
    CHECK(ran && refused == w.h.log[3].n, "%u callers were refused, the failed call held %u", refused,
          ran ? w.h.log[3].n : 0);
    CHECK(w.stats[4] == 1, "stats out[4] = %llu after one failed batch", (unsigned long long)w.stats[4]);
    if (ring) verify_egress(w, o, D.got, true);
    g_rep->extra << (ring ? ", \"refused_egress\": " : ", \"refused_plain\": ") << refused;
  }
}

// window 10 s, 48 callers blocked in their take, then close: it returns within
// 2 s and every caller has rc 0 and a distinct seq (verify()).  20 times.
void sc_close_blocked() {
  double worst = 0;
  for (int it = 0; it < 20; ++it) {
    const uint32_t T = 48;
    World w;
    w.make_reqs(T, 41 + it);
    w.open(kLongWindowUs, 0, 0);
    auto th = start_takers(w, T, 1, false);
    CHECK(wait_for([&] { return w.entered.load() == T; }), "the takers did not start");
    sleep_us(40000);   // from `entered` to the batcher's queue is a few instructions
    w.close();
    join_all(th);
    worst = std::max(worst, w.close_ms);
    CHECK(w.close_ms < kBoundMs, "close took %.1f ms with %u callers blocked", w.close_ms, T);
    verify(w, false, T);
  }
  g_rep->extra << ", \"close_ms_max\": " << worst;
}

// Ring of 2, one drainer holding every slot about 200 us: verify_egress().
void sc_egress_order() {
  const uint32_t T = 8, PER = 60;
  World w;
  w.make_reqs(T * PER, 51);
  w.h.delay_us = 20;
  w.open(50, 16, 2);
  Drain D;
  std::thread dr(drainer, std::ref(w), std::ref(D), 200);
  auto th = start_takers(w, T, PER, false);
  join_all(th);
  D.stop.store(true);
  dr.join();
  w.close();
  const Order o = verify(w, false, T * PER);
  verify_egress(w, o, D.got, true);
  for (const Out& r : w.outs) CHECK(r.rc == PHIP_OK, "a take returned %d", r.rc);
  uint64_t reqsum = 0;
  for (const Drained& d : D.got) reqsum += d.requests;
  CHECK(reqsum == T * PER, "the requests fields sum to %llu of %u", (unsigned long long)reqsum, T * PER);
  g_rep->extra << ", \"egress_batches\": " << D.got.size();
}

// Every third call produces no datagram: its callers return normally, the
// numbering has no hole and out[5] counts the queued batches only.
void sc_zero_datagrams() {
  const uint32_t T = 8, PER = 40;
  World w;
  w.make_reqs(T * PER, 61);
  w.h.zero_mod = 3;
  w.h.zero_rem = 1;
  w.h.delay_us = 20;
  w.open(50, 16, 3);
  Drain D;
  std::thread dr(drainer, std::ref(w), std::ref(D), 50);
  auto th = start_takers(w, T, PER, false);
  join_all(th);
  D.stop.store(true);
  dr.join();
  w.close();
  const Order o = verify(w, false, T * PER);
  verify_egress(w, o, D.got, true);
  size_t empty = 0;
  for (const Call& c : w.h.log) empty += c.eg_n == 0;
  CHECK(empty > 0 && empty < w.h.log.size() && w.stats[5] == w.h.log.size() - empty,
        "%zu of %zu calls were empty, out[5] = %llu", empty, w.h.log.size(), (unsigned long long)w.stats[5]);
  for (const Out& r : w.outs) CHECK(r.rc == PHIP_OK, "a take returned %d", r.rc);
  g_rep->extra << ", \"egress_batches\": " << D.got.size() << ", \"empty_calls\": " << empty;
}

// Ring of 2, max_batch 1, 6 takers, nobody gives a slot back: exactly 2 calls
// run and 2 takers return, also once a batch is handed out; after done the
// rest proceed; out[7] > 0.
void sc_backpressure() {
  const uint32_t T = 6;
  World w;
  w.make_reqs(T, 71);
  w.open(0, 1, 2);
  auto th = start_takers(w, T, 1, false);
  CHECK(wait_for([&] { return w.returned.load() >= 2; }), "two takers did not return");
  sleep_us(100000);
  CHECK(w.calls() == 2 && w.returned.load() == 2, "ring full: %zu calls, %u takers returned", w.calls(),
        w.returned.load());
  std::vector<Drained> got;
  phip_egress_batch eb;
  int r = phip_batcher_egress_next(w.b, 1000, &eb);
  CHECK(r == 1 && eb.batch == 0, "egress_next: %d", r);
  if (r == 1) {
    Drained d = copy_batch(eb);
    sleep_us(50000);
    CHECK(w.calls() == 2 && w.returned.load() == 2, "one batch handed out: %zu calls, %u takers returned",
          w.calls(), w.returned.load());
    CHECK(same_as_slot(d, eb), "the handed-out slot changed");
    CHECK(phip_batcher_egress_done(w.b, eb.batch) == PHIP_OK, "egress_done failed");
    got.push_back(std::move(d));
    while (got.size() < T) {
      r = phip_batcher_egress_next(w.b, 1000, &eb);
      CHECK(r == 1, "egress_next after done: %d with %zu batches out", r, got.size());
      if (r != 1) break;
      got.push_back(copy_batch(eb));
      CHECK(phip_batcher_egress_done(w.b, eb.batch) == PHIP_OK, "egress_done failed");
    }
  }
  if (got.size() == T) {
    join_all(th);
  } else {   // the ring is stuck: close runs what is left without egress
    w.close();
    join_all(th);
  }
  if (w.b) w.close();
  const Order o = verify(w, false, T);
  verify_egress(w, o, got, got.size() == T);
  CHECK(w.stats[7] > 0, "out[7] = 0 although the dispatcher waited for a slot");
  g_rep->extra << ", \"slot_wait_ms\": " << w.stats[7] / 1e6;
}

// Ring of 3, three drainers with different hold times (done arrives out of
// order): each number handed out once, the set is 0..out[5]-1, payloads intact.
void sc_drainers() {
  const uint32_t T = 8, PER = 60;
  World w;
  w.make_reqs(T * PER, 81);
  w.h.delay_us = 10;
  w.open(50, 8, 3);
  Drain D;
  std::vector<std::thread> dr;
  for (uint32_t hold : {20u, 200u, 600u}) dr.emplace_back(drainer, std::ref(w), std::ref(D), hold);
  auto th = start_takers(w, T, PER, false);
  join_all(th);
  D.stop.store(true);
  join_all(dr);
  w.close();
  const Order o = verify(w, false, T * PER);
  verify_egress(w, o, D.got, true);
  CHECK(D.got.size() == w.stats[5], "%zu batches out, out[5] = %llu", D.got.size(), (unsigned long long)w.stats[5]);
  size_t inversions = 0;
  for (size_t i = 1; i < D.done_order.size(); ++i) inversions += D.done_order[i] < D.done_order[i - 1];
  g_rep->extra << ", \"egress_batches\": " << D.got.size() << ", \"done_out_of_order\": " << inversions;
}

// egress_done refuses a number never handed out, one already done and
// number + ring size, and the ring works afterwards; both egress calls refuse a
// plain batcher; egress_next(0) on an empty ring returns 0 at once.
void sc_done_misuse() {
  World w;
  w.make_reqs(3, 91);
  w.open(0, 0, 2);
  phip_egress_batch eb;
  const auto t0 = Clock::now();
  int r = phip_batcher_egress_next(w.b, 0, &eb);
  const double ms = ms_since(t0);
  // no wait is asked for; the allowance is for a descheduled thread
  CHECK(r == 0 && ms < 500.0, "egress_next(0) on an empty ring: %d after %.1f ms", r, ms);
  g_rep->extra << ", \"next0_ms\": " << ms;
  std::vector<Drained> got;
  auto refuse = [&](uint64_t batch, const char* what) {
    const int rc = phip_batcher_egress_done(w.b, batch);
    CHECK(rc == PHIP_ERR_INVALID, "egress_done(%llu), %s: %d", (unsigned long long)batch, what, rc);
  };
  auto next = [&](uint64_t want) {
    r = phip_batcher_egress_next(w.b, 1000, &eb);
    CHECK(r == 1 && eb.batch == want, "egress_next: %d, batch %llu, expected %llu", r,
          (unsigned long long)eb.batch, (unsigned long long)want);
    if (r == 1) got.push_back(copy_batch(eb));
    return r == 1;
  };
  w.take(0, false);
  refuse(0, "queued, never handed out");
  refuse(7, "never queued");
  if (next(0)) {
    refuse(2, "number + ring size");
    refuse(1, "never queued");
    CHECK(phip_batcher_egress_done(w.b, 0) == PHIP_OK, "egress_done(0) failed");
    refuse(0, "already done");
    refuse(2, "number + ring size, after done");
  }
  w.take(1, false);
  if (next(1)) CHECK(phip_batcher_egress_done(w.b, 1) == PHIP_OK, "egress_done(1) failed");
  w.take(2, false);   // slot 0 again
  if (next(2)) {
    refuse(0, "the slot's earlier batch");
    CHECK(same_as_slot(got.back(), eb), "a refused done changed the slot");
    CHECK(phip_batcher_egress_done(w.b, 2) == PHIP_OK, "egress_done(2) failed");
  }
  w.close();
  const Order o = verify(w, false, 3);
  verify_egress(w, o, got, true);

  World p;
  p.make_reqs(1, 92);
  p.open(0, 0, 0);
  r = phip_batcher_egress_next(p.b, 0, &eb);
  const int rc = phip_batcher_egress_done(p.b, 0);
  CHECK(r == PHIP_ERR_INVALID && rc == PHIP_ERR_INVALID, "plain batcher: egress_next %d, egress_done %d", r, rc);
  p.take(0, false);
  p.close();
  verify(p, false, 1);
}

// Ring of 2 full with nobody draining and takers waiting behind it, and on a
// second batcher a thread blocked in egress_next(-1) on an empty ring; close
// both: the blocked call returns 0, the waiting takers rc 0, their batches ran
// through phip_apply_mixed without egress, each close returns within 2 s.
void sc_close_ring_full() {
  const uint32_t T = 5;
  World w;
  w.make_reqs(T, 101);
  w.open(0, 1, 2);
  World e;
  e.open(0, 0, 2);
  std::atomic<int> blocked{-9};
  std::atomic<bool> in{false};
  std::thread waiter([&] {
    phip_egress_batch eb;
    in.store(true);
    blocked.store(phip_batcher_egress_next(e.b, -1, &eb));
  });
  auto th = start_takers(w, T, 1, false);
  CHECK(wait_for([&] { return w.returned.load() >= 2 && w.entered.load() == T && in.load(); }),
        "the ring did not fill");
  sleep_us(50000);
  CHECK(w.calls() == 2 && w.returned.load() == 2 && blocked.load() == -9,
        "before close: %zu calls, %u takers returned, egress_next %d", w.calls(), w.returned.load(),
        blocked.load());
  w.close();
  join_all(th);
  e.close();
  waiter.join();
  CHECK(blocked.load() == 0, "the blocked egress_next returned %d", blocked.load());
  CHECK(w.close_ms < kBoundMs && e.close_ms < kBoundMs, "close took %.1f ms and %.1f ms", w.close_ms, e.close_ms);
  verify(w, false, T);
  for (const Out& r : w.outs) CHECK(r.rc == PHIP_OK, "a take returned %d", r.rc);
  CHECK(w.h.log.size() == T, "%zu calls", w.h.log.size());
  for (size_t ci = 0; ci < w.h.log.size(); ++ci)
    CHECK(w.h.log[ci].egress == (ci < 2), "call %zu ran %s egress", ci, w.h.log[ci].egress ? "with" : "without");
  CHECK(w.stats[5] == 2 && e.h.log.empty(), "out[5] = %llu", (unsigned long long)w.stats[5]);
  g_rep->extra << ", \"close_ms\": " << w.close_ms << ", \"close_idle_ms\": " << e.close_ms;
}

const struct {
  const char* name;
  void (*fn)();
} kScenarios[] = {
    {"order", sc_order},
    {"max_batch", sc_max_batch},
    {"engine_error", sc_engine_error},
    {"close_blocked", sc_close_blocked},
    {"egress_order", sc_egress_order},
    {"zero_datagrams", sc_zero_datagrams},
    {"backpressure", sc_backpressure},
    {"drainers", sc_drainers},
    {"done_misuse", sc_done_misuse},
    {"close_ring_full", sc_close_ring_full},
};

// A scenario that stops making progress (a batch number that never comes, a
// lost wakeup) says so instead of hanging its caller.
constexpr double kWatchdogMs = 45000.0;

bool run(const char* name, void (*fn)()) {
  Report rep;
  rep.scenario = name;
  rep.t0 = Clock::now();
  g_rep = &rep;
  std::atomic<bool> finished{false};
  std::thread dog([&] {
    while (!finished.load()) {
      if (ms_since(rep.t0) > kWatchdogMs) {
        rep.print(true);
        _exit(3);
      }
      sleep_us(2000);
    }
  });
  g_poll.polls.store(0);
  g_poll.start();
  fn();
  g_poll.stop();
  g_poll.quit.store(false);
  finished.store(true);
  dog.join();
  CHECK(g_poll.polls.load() > 0, "the stats poller never ran");
  rep.print(false);
  g_rep = nullptr;
  return rep.failures == 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc == 2 ? argv[1] : "";
  if (what == "list") {
    for (const auto& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  bool found = false, ok = true;
  for (const auto& s : kScenarios)
    if (what == "all" || what == s.name) {
      found = true;
      ok = run(s.name, s.fn) && ok;
    }
  if (!found) {
    fprintf(stderr, "usage: %s NAME | all | list\n", argv[0]);
    return 2;
  }
  return ok ? 0 : 1;
}
