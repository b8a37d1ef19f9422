// Host-side pieces of the drop-in boundary that need no GPU: Patrol's rate
// parser, the wire encoder used for egress (unicast replies / broadcast), and
// the API.takeBucket handler logic running over the engine.
//
// ParseRate (bucket.go:102-123) is only ever used with its error ignored
// (api.go:61), so what matters is the Rate value Go returns beside each
// error; this file reproduces strconv.Atoi / time.ParseDuration closely
// enough to return the same values (tests/test_host.py checks every case of
// tests/golden/parse_rate.json).
#include <cstdint>
#include <cstring>
#include <string>

#include "patrolhip.h"
#include "phip_device.hpp"
#include "phip_host.hpp"

namespace {

using u64 = uint64_t;
using i64 = int64_t;

struct Cursor {
  const char* p;
  const char* end;
  bool done() const { return p == end; }
  char peek() const { return *p; }
  bool digit() const { return p != end && *p >= '0' && *p <= '9'; }
};

// strconv.Atoi for 64-bit int: {value, ok}.  Syntax errors give 0, range
// errors the clamped bound (strconv.ParseInt semantics).
bool atoi64(const char* s, size_t n, i64* out) {
  *out = 0;
  if (n == 0) return false;
  size_t k = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; k = 1; }
  if (k == n) return false;
  // Unsigned accumulate with left-to-right error detection (ParseUint).
  u64 acc = 0;
  bool range = false;
  for (; k < n; ++k) {
    unsigned d = (unsigned char)s[k] - '0';
    if (d > 9) return false;                       // syntax error -> 0
    if (acc > (UINT64_MAX - d) / 10) { range = true; break; }
    acc = acc * 10 + d;
  }
  // The short fast path of Atoi (len < 19) can neither overflow nor differ.
  const u64 lim = 1ull << 63;
  if (range || (!neg && acc >= lim) || (neg && acc > lim)) {
    *out = neg ? INT64_MIN : INT64_MAX;
    return false;
  }
  *out = neg ? (i64)(0 - acc) : (i64)acc;
  return true;
}

u64 unit_ns(const char* u, size_t n, bool* ok) {
  struct { const char* s; u64 v; } tab[] = {
      {"ns", 1ull}, {"us", 1000ull}, {"\xC2\xB5s", 1000ull}, {"\xCE\xBCs", 1000ull},
      {"ms", 1000000ull}, {"s", 1000000000ull}, {"m", 60000000000ull}, {"h", 3600000000000ull}};
  for (auto& e : tab)
    if (strlen(e.s) == n && memcmp(e.s, u, n) == 0) { *ok = true; return e.v; }
  *ok = false;
  return 0;
}

// time.ParseDuration: {ns, ok}; every error yields 0.
bool parse_duration(const char* s, size_t n, i64* out) {
  *out = 0;
  Cursor c{s, s + n};
  bool neg = false;
  if (!c.done() && (c.peek() == '-' || c.peek() == '+')) { neg = c.peek() == '-'; ++c.p; }
  if (c.end - c.p == 1 && c.peek() == '0') return true;
  if (c.done()) return false;
  const u64 two63 = 1ull << 63;
  u64 total = 0;
  while (!c.done()) {
    if (!(c.peek() == '.' || c.digit())) return false;
    u64 whole = 0;
    const char* start = c.p;
    while (c.digit()) {
      if (whole > two63 / 10) return false;
      whole = whole * 10 + (u64)(c.peek() - '0');
      if (whole > two63) return false;
      ++c.p;
    }
    bool had_whole = c.p != start;
    u64 frac = 0;
    double scale = 1.0;
    bool had_frac = false;
    if (!c.done() && c.peek() == '.') {
      ++c.p;
      const char* fs = c.p;
      bool stop = false;
      while (c.digit()) {
        if (!stop) {
          u64 nx = frac * 10 + (u64)(c.peek() - '0');
          if (frac > (two63 - 1) / 10 || nx > two63) stop = true;
          else { frac = nx; scale *= 10; }
        }
        ++c.p;
      }
      had_frac = c.p != fs;
    }
    if (!had_whole && !had_frac) return false;
    const char* us = c.p;
    while (!c.done() && c.peek() != '.' && !c.digit()) ++c.p;
    if (c.p == us) return false;
    bool uok;
    u64 unit = unit_ns(us, (size_t)(c.p - us), &uok);
    if (!uok) return false;
    if (whole > two63 / unit) return false;
    whole *= unit;
    if (frac > 0) {
      whole += (u64)((double)frac * ((double)unit / scale));
      if (whole > two63) return false;
    }
    total += whole;
    if (total > two63) return false;
  }
  if (neg) { *out = (i64)(0 - total); return true; }
  if (total > two63 - 1) return false;
  *out = (i64)total;
  return true;
}

// strconv.ParseUint(s, 10, 64): syntax error 0, range error MaxUint64.
u64 parse_count(const char* s, size_t n) {
  if (n == 0) return 0;
  u64 acc = 0;
  for (size_t k = 0; k < n; ++k) {
    unsigned d = (unsigned char)s[k] - '0';
    if (d > 9) return 0;
    if (acc > (UINT64_MAX - d) / 10) return UINT64_MAX;
    acc = acc * 10 + d;
  }
  return acc;
}

}  // namespace

namespace phip_host {

int api_prepare(const uint8_t* name, uint32_t len, const char* rate, uint32_t rate_len,
                const char* count, uint32_t count_len, int64_t* freq, int64_t* per, uint64_t* n,
                char* body, uint32_t* body_len) {
  (void)name;
  if (len > PHIP_MAX_NAME_LEN) {                                  // api.go:55-58
    static const char msg[] = "bucket name larger than 231";
    memcpy(body, msg, sizeof msg - 1);
    *body_len = sizeof msg - 1;
    return 400;
  }
  phip_parse_rate(rate, rate_len, freq, per);                     // api.go:61, error ignored
  *n = parse_count(count, count_len);                             // api.go:62-65
  if (*n == 0) *n = 1;
  return 0;
}

}  // namespace phip_host

extern "C" {

int phip_parse_rate(const char* s, uint32_t len, int64_t* freq, int64_t* per) {
  *freq = 0;
  *per = 0;
  if (!s && len) return PHIP_ERR_INVALID;
  const char* colon = len ? (const char*)memchr(s, ':', len) : nullptr;
  size_t flen = colon ? (size_t)(colon - s) : len;
  if (!atoi64(s, flen, freq)) return PHIP_ERR_INVALID;
  std::string unit = colon ? std::string(colon + 1, s + len) : std::string("1s");
  // bucket.go:117: a bare unit means one of it (micro sign U+00B5 only).
  static const char* bare[] = {"ns", "us", "\xC2\xB5s", "ms", "s", "m", "h"};
  for (const char* b : bare)
    if (unit == b) { unit = "1" + unit; break; }
  return parse_duration(unit.data(), unit.size(), per) ? PHIP_OK : PHIP_ERR_INVALID;
}

int phip_marshal(const uint8_t* name, uint32_t len, const phip_state* st, uint8_t* out) {
  if (!st || !out || (!name && len)) return PHIP_ERR_INVALID;
  if (len > PHIP_MAX_NAME_LEN) return PHIP_ERR_NAME_TOO_LARGE;   // bucket.go:54-57
  const u64 words[3] = {st->added, st->taken, (u64)st->elapsed};
  for (int w = 0; w < 3; ++w)
    for (int b = 0; b < 8; ++b) out[w * 8 + b] = (uint8_t)(words[w] >> (56 - 8 * b));
  out[24] = (uint8_t)len;
  if (len) memcpy(out + PHIP_BUCKET_FIXED_SIZE, name, len);
  return PHIP_BUCKET_FIXED_SIZE + (int)len;
}

int phip_api_take(phip_handle* h, const uint8_t* name, uint32_t len, const char* rate,
                  uint32_t rate_len, const char* count, uint32_t count_len, int64_t now,
                  char* body, uint32_t* body_len) {
  if (!body || !body_len) return PHIP_ERR_INVALID;
  int64_t freq, per;
  uint64_t n;
  const int pre = phip_host::api_prepare(name, len, rate, rate_len, count, count_len, &freq, &per,
                                         &n, body, body_len);
  if (pre) return pre;
  uint32_t offs[2] = {0, len};
  uint8_t empty = 0;
  uint64_t rem = 0;
  uint8_t ok = 0;
  int rc = phip_take(h, len ? name : &empty, offs, 1, &now, &freq, &per, &n, &rem, &ok, 0);
  if (rc < 0) return rc;
  std::string s = std::to_string(rem);                            // api.go:84-85
  memcpy(body, s.data(), s.size());
  *body_len = (uint32_t)s.size();
  return ok ? 200 : 429;
}

// Peek on the host (patrolhip.h "Peek"): phip::peek_eval is the function
// k_peek calls, compiled here for the host from the same header.
int phip_peek_eval(const phip_state* s, int64_t now, int64_t freq, int64_t per, uint64_t count,
                   uint64_t* remaining, uint64_t* have, int64_t* retry_at) {
  if (!remaining || !have || !retry_at) return PHIP_ERR_INVALID;
  const phip_state st = s ? *s : phip_state{0, 0, 0, now};   // absent: GetBucket's (repo.go:189-211)
  const phip::PeekResult r =
      phip::peek_eval(phip::as_f64(st.added), phip::as_f64(st.taken), st.elapsed, st.created, now,
                      phip::rate_interval(freq, per), (double)freq, (double)count);
  *remaining = r.remaining;
  *have = r.have_bits;
  *retry_at = r.retry_at;
  return r.ok ? PHIP_ST_TAKE_OK : PHIP_ST_TAKE_DENIED;
}

// API.takeBucket's parsing (api.go:55-65) over one phip_peek: nothing is taken.
int phip_api_peek(phip_handle* h, const uint8_t* name, uint32_t len, const char* rate,
                  uint32_t rate_len, const char* count, uint32_t count_len, int64_t now,
                  char* body, uint32_t* body_len, int64_t* retry_after_ns) {
  if (!body || !body_len) return PHIP_ERR_INVALID;
  int64_t freq, per;
  uint64_t n;
  const int pre = phip_host::api_prepare(name, len, rate, rate_len, count, count_len, &freq, &per,
                                         &n, body, body_len);
  if (pre) return pre;
  uint32_t offs[2] = {0, len};
  uint8_t empty = 0;
  uint8_t st = 0;
  uint64_t rem = 0;
  int64_t at = 0;
  phip_ops q{};
  q.n = 1;
  q.names = len ? name : &empty;
  q.name_offs = offs;
  q.now = &now;
  q.freq = &freq;
  q.per = &per;
  q.count = &n;
  phip_peek_results res{};
  res.status = &st;
  res.remaining = &rem;
  res.retry_at = &at;
  const int rc = phip_peek(h, &q, &res, 0);
  if (rc < 0) return rc;
  const std::string s = std::to_string(rem);                      // api.go:84-85
  memcpy(body, s.data(), s.size());
  *body_len = (uint32_t)s.size();
  const bool ok = (st & 0x3F) == PHIP_ST_TAKE_OK;
  if (retry_after_ns) {
    if (ok) *retry_after_ns = 0;
    else if (at == PHIP_PEEK_NEVER) *retry_after_ns = -1;
    else {   // at > now: the difference fits 64 unsigned bits
      const u64 d = (u64)at - (u64)now;
      *retry_after_ns = d > (u64)INT64_MAX ? INT64_MAX : (i64)d;
    }
  }
  return ok ? 200 : 429;
}

// Throttled sweep on the host (patrolhip.h "Throttled sweep"): phip::throttle_match
// is the function the sweep's kernels call, over the same derived rule table.
int phip_throttle_match(const phip_throttle_rule* rules, uint32_t n_rules, const uint8_t* name,
                        uint32_t len, int32_t* rule_out) {
  if (!rules || !rule_out || (!name && len) || n_rules < 1 || n_rules > PHIP_THROTTLE_MAX_RULES)
    return PHIP_ERR_INVALID;
  phip::ThrottleRules R{};
  R.n = n_rules;
  for (uint32_t i = 0; i < n_rules; ++i) {
    if (rules[i].prefix_len > PHIP_THROTTLE_MAX_PREFIX) return PHIP_ERR_INVALID;
    R.r[i] = phip::throttle_rule(rules[i]);
  }
  u64 w[2] = {0, 0};   // the first 16 name bytes, as a record carries them
  for (uint32_t k = 0; k < len && k < 16; ++k) w[k >> 3] |= (u64)name[k] << ((k & 7) * 8);
  *rule_out = phip::throttle_match(R, w[0], w[1], len).rule;
  return PHIP_OK;
}

// Partition digests (patrolhip.h "Partition digests"): the two host helpers.
int phip_digest_diff(const phip_digest_part* a, const phip_digest_part* b, uint32_t log2_parts,
                     uint64_t* mask, uint64_t* ndiff) {
  if (!a || !b || !mask || log2_parts > PHIP_DIGEST_MAX_LOG2_PARTS) return PHIP_ERR_INVALID;
  const u64 parts = 1ull << log2_parts;
  const u64 words = parts < 64 ? 1 : parts / 64;
  u64 nd = 0;
  for (u64 w = 0; w < words; ++w) {
    u64 bits = 0;
    for (u64 p = w * 64; p < parts && p < (w + 1) * 64; ++p)
      if (a[p].sum != b[p].sum || a[p].count != b[p].count) {
        bits |= 1ull << (p & 63);
        ++nd;
      }
    mask[w] = bits;
  }
  if (ndiff) *ndiff = nd;
  return PHIP_OK;
}

int phip_digest_fold(const phip_digest_part* in, uint32_t log2_in, uint32_t log2_out,
                     phip_digest_part* out) {
  if (!in || !out || log2_in > PHIP_DIGEST_MAX_LOG2_PARTS || log2_out > log2_in)
    return PHIP_ERR_INVALID;
  // entry p of the coarse level: the 2^(in - out) consecutive fine entries
  // from p << (in - out); ascending p reads at or ahead of every write, so
  // in == out works in place
  const u64 n_out = 1ull << log2_out, span = 1ull << (log2_in - log2_out);
  for (u64 p = 0; p < n_out; ++p) {
    u64 s = 0, c = 0;
    for (u64 q = p * span; q < (p + 1) * span; ++q) {
      s += in[q].sum;
      c += in[q].count;
    }
    out[p].sum = s;
    out[p].count = c;
  }
  return PHIP_OK;
}

}  // extern "C"
