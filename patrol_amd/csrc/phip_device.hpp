// Device-side building blocks of libpatrolhip (gfx950).
//
//  * the order-preserving 64-bit key encoding ("E-encoding") that lets one
//    unsigned atomicMax reproduce Go's asymmetric `if b.x < o.x { b.x = o.x }`
//    merge (bucket.go:250-256) for every stored value and every replica value
//    except -0.0 (DESIGN.md §3.2 has the proof sketch);
//  * the op-for-op restatement of Bucket.Take (bucket.go:186-225) on doubles,
//    including Go's time.Time saturation and amd64 uint64(float64) rules;
//  * the slot record of the device hash table and name canonicalisation.
//
// Compiled with -ffp-contract=off: every + - / below is one IEEE-754 binary64
// operation, exactly as the Go compiler emits them on amd64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "patrolhip.h"

namespace phip {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;
typedef unsigned char u8;
typedef unsigned short u16;

constexpr u64 kSign = 0x8000000000000000ull;
constexpr u64 kInfBits = 0x7FF0000000000000ull;      // +Inf
constexpr u64 kNanBase = 0xFFE0000000000002ull;      // first E-code of a NaN
constexpr u64 kNanPerSign = (1ull << 52) - 1;        // NaN payloads per sign
constexpr u64 kEPosZero = kInfBits;                  // E(+0.0)
constexpr u64 kENegZero = kInfBits + 1;              // E(-0.0)

__host__ __device__ inline bool is_nan_bits(u64 b) { return (b & ~kSign) > kInfBits; }
__host__ __device__ inline bool is_zero_bits(u64 b) { return (b & ~kSign) == 0; }

// E: float64 bits -> u64 such that unsigned order is
//   negatives (by value) < +0 < -0 < positives (by value) < NaNs.
// It is a bijection on all 2^64 patterns.  Placing -0 just above +0 makes
// max(E(b), E(o)) equal E(Go's merge result) for every stored b and every
// replica o != -0.0 (a NaN replica is mapped to 0 = E(-Inf), a no-op).
__host__ __device__ inline u64 enc_f64(u64 b) {
  u64 mag = b & ~kSign;
  if (mag > kInfBits) {                            // NaN
    u64 idx = mag - kInfBits - 1;
    if (b & kSign) idx += kNanPerSign;
    return kNanBase + idx;
  }
  if (b & kSign) return mag == 0 ? kENegZero : kInfBits - mag;
  return mag == 0 ? kEPosZero : kInfBits + 1 + mag;
}

__host__ __device__ inline u64 dec_f64(u64 e) {
  if (e < kInfBits) return kSign | (kInfBits - e);
  if (e == kEPosZero) return 0;
  if (e == kENegZero) return kSign;
  if (e < kNanBase) return e - kInfBits - 1;
  u64 idx = e - kNanBase;
  if (idx < kNanPerSign) return kInfBits + 1 + idx;
  return kSign | (kInfBits + 1 + idx - kNanPerSign);
}

// Replica value as an atomicMax operand (NaN is never adopted by Go's `<`).
__host__ __device__ inline u64 enc_replica(u64 b) { return is_nan_bits(b) ? 0ull : enc_f64(b); }

__host__ __device__ inline double as_f64(u64 b) { return __builtin_bit_cast(double, b); }
__host__ __device__ inline u64 as_bits(double x) { return __builtin_bit_cast(u64, x); }

// ------------------------------------------------------------- Take -----
// x86-64 CVTTSD2SQ (what Go's amd64 backend uses for float->int).
__host__ __device__ inline i64 cvttsd2sq(double x) {
  if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) return (i64)kSign;
  return (i64)x;
}
// Go uint64(float64) on amd64: cutoff at 2^63 (ssagen floatToUint).
__host__ __device__ inline u64 go_u64(double x) {
  if (x < 9223372036854775808.0) return (u64)cvttsd2sq(x);
  return (u64)cvttsd2sq(x - 9223372036854775808.0) | kSign;
}

// Rate.Interval (bucket.go:146-148) folded with the zero tests of
// Rate.Tokens (bucket.go:132-137): 0 means "Tokens() returns 0".  Computed
// once per op when the ordered stream is gathered (k_gather_ops).
__host__ __device__ inline i64 rate_interval(i64 freq, i64 per) {
  if (freq == 0 || per == 0) return 0;
  if (freq == -1 && per == (i64)kSign) return (i64)kSign;   // Go's MinInt64 / -1 wraps
  return per / freq;
}

// Go float64 + and - as amd64 executes them (ADDSD/SUBSD, the left Go
// operand in the destination register), down to the NaN bits: a NaN operand
// comes back quieted with its sign and payload, the left one first, and an
// invalid operation (Inf - Inf) gives the x86 default NaN 0xFFF8000000000000.
// gfx950 computes a - b as a + (-b), which flips the sign of a NaN b and
// returns the positive default NaN, so results that are NaN are rebuilt here.
constexpr u64 kQuietBit = 0x0008000000000000ull;
constexpr u64 kX86DefaultNaN = 0xFFF8000000000000ull;

__host__ __device__ inline double x86_nan_fix(double r, double a, double b) {
  if (__builtin_expect(r == r, 1)) return r;
  const u64 ab = as_bits(a), bb = as_bits(b);
  if (is_nan_bits(ab)) return as_f64(ab | kQuietBit);
  if (is_nan_bits(bb)) return as_f64(bb | kQuietBit);
  return as_f64(kX86DefaultNaN);
}
__host__ __device__ inline double go_add(double a, double b) { return x86_nan_fix(a + b, a, b); }
__host__ __device__ inline double go_sub(double a, double b) { return x86_nan_fix(a - b, a, b); }

// dt of Take (bucket.go:198-207): last = created.Add(elapsed) (exact),
// clamped to now, then now.Sub(last) saturating to the int64 range.  The
// int64 fast path is exact whenever created + elapsed does not overflow.
__host__ __device__ inline i64 take_dt(i64 created, i64 elapsed, i64 now) {
  i64 last;
  if (__builtin_expect(!__builtin_add_overflow(created, elapsed, &last), 1)) {
    if (now < last) return 0;
    i64 d;
    return __builtin_sub_overflow(now, last, &d) ? 0x7FFFFFFFFFFFFFFFll : d;
  }
  __int128 l = (__int128)created + (__int128)elapsed;
  if ((__int128)now < l) return 0;
  __int128 dd = (__int128)now - l;
  return dd > (__int128)0x7FFFFFFFFFFFFFFFll ? 0x7FFFFFFFFFFFFFFFll : (i64)dd;
}

// The eviction sweep's rule (phip_evict_idle): idle = now - (created +
// elapsed) is exactly Take's dt -- the exact 128-bit `last`, 0 when now <
// last (a merged elapsed ahead of the local clock), saturating at INT64_MAX
// -- and a bucket is idle iff idle >= idle_ns (idle_ns > 0).
__device__ inline bool bucket_idle(i64 created, i64 elapsed, i64 now, i64 idle_ns) {
  return take_dt(created, elapsed, now) >= idle_ns;
}

struct TakeResult {
  u64 remaining;
  u64 have_bits;
  bool ok;
};

// Bucket.Take (bucket.go:186-225), in the reference's exact operation order,
// with Rate.Interval precomputed (rate_interval).  `created` and `now` are
// int64 ns; created.Add(elapsed) is exact (128-bit, as time.Time cannot
// overflow here), now.Sub(last) saturates like time.Time.Sub, and
// elapsed += dt wraps like Go int64.
// capacity = float64(Freq) and t = float64(n) come precomputed (k_pack_ops).
__host__ __device__ inline TakeResult take_step(double& added, double& taken, i64& elapsed,
                                                i64 created, i64 now, i64 interval,
                                                double capacity, double t) {
  //                                                              :192 capacity
  if (added == 0) added = capacity;                            // :194-196
  const i64 dt = take_dt(created, elapsed, now);                // :198-207
  double tokens = go_sub(added, taken);                        // :204
  // :210, bucket.go:132-143; 0/interval is a zero with interval's sign
  double add = !interval ? 0.0 : dt ? (double)dt / (double)interval : (interval < 0 ? -0.0 : 0.0);
  double missing = go_sub(capacity, tokens);                   // :211
  if (add > missing) add = missing;                            // :211-213
  //                                                              :215 t
  double have = go_add(tokens, add);                           // :216
  if (t > have) return TakeResult{go_u64(have), as_bits(have), false};   // :216-218
  elapsed = (i64)((u64)elapsed + (u64)dt);                     // :220
  added = go_add(added, add);                                  // :221
  taken = go_add(taken, t);                                    // :222
  double rem = go_sub(added, taken);
  return TakeResult{go_u64(rem), as_bits(rem), true};          // :224
}

// ------------------------------------------------------------- Peek -----
// phip_peek / phip_peek_eval (patrolhip.h "Peek"): Take evaluated on a copy of
// a bucket's state, plus the least clock reading at which the same Take would
// be granted.
struct PeekResult {
  u64 remaining;
  u64 have_bits;
  i64 retry_at;   // now (granted), the least later reading that grants, or PHIP_PEEK_NEVER
  bool ok;
};

// take_step's verdict alone, at the reading `at`, from the parts of it that do
// not depend on the clock (tokens = added - taken after :194-196, missing =
// capacity - tokens, fi = float64(interval)).  A NaN's payload and a zero's
// sign cannot change `t > have`, so the plain + stands in for go_add.
__host__ __device__ inline bool take_ok_at(i64 created, i64 elapsed, i64 at, i64 interval,
                                           double fi, double tokens, double missing, double t) {
  const i64 dt = take_dt(created, elapsed, at);
  double add = !interval ? 0.0 : (double)dt / fi;
  if (add > missing) add = missing;
  return !(t > tokens + add);
}

// One lane's own verdict on "does anybody still search" (the host form).
struct PeekVoteSelf {
  __host__ __device__ inline bool operator()(bool pending) const { return pending; }
};

// The retry search of a query denied at `now` (search == true; a lane with
// search == false gets `now` back): the least reading in (now, INT64_MAX] that
// grants, or PHIP_PEEK_NEVER.  From a denial the verdict is monotone in the
// clock, so after one probe of INT64_MAX (false: never) a
// bisection keeps lo denied / hi granted and halves hi - lo <= 2^64 - 1 in 64
// steps: at most 65 verdicts.  `any` turns "this lane still searches" into
// "some lane of the wave does" (k_peek, k_throttle_write: a ballot), so the
// loop is uniform across a wave and a wave without a searching lane skips it;
// every lane of the wave must make the call.
template <class Vote = PeekVoteSelf>
__host__ __device__ inline i64 retry_search(bool search, i64 created, i64 elapsed, i64 now,
                                            i64 interval, double fi, double tokens, double missing,
                                            double t, Vote any = Vote()) {
  i64 retry_at = now;
  const i64 kMax = 0x7FFFFFFFFFFFFFFFll;
  if (any(search)) {
    if (search && !take_ok_at(created, elapsed, kMax, interval, fi, tokens, missing, t)) {
      retry_at = (i64)kSign;   // PHIP_PEEK_NEVER
      search = false;
    }
  }
  i64 lo = now, hi = kMax;   // (searching lanes: lo denied, hi granted, lo < hi)
  for (int step = 0; step < 64; ++step) {
    const u64 gap = (u64)hi - (u64)lo;
    const bool pending = search && gap > 1;
    if (!any(pending)) break;
    if (pending) {
      const i64 mid = (i64)((u64)lo + (gap >> 1));
      if (take_ok_at(created, elapsed, mid, interval, fi, tokens, missing, t)) hi = mid;
      else lo = mid;
    }
  }
  if (search) retry_at = hi;
  return retry_at;
}

// The evaluation.  Step 1 is take_step itself on the copy, so status,
// remaining and have are what a TAKE op reports.  A denied query then runs
// retry_search: at most 66 verdicts a query, none when it was granted.  Every
// lane of a wave must make the call (retry_search's vote).
template <class Vote = PeekVoteSelf>
__host__ __device__ inline PeekResult peek_eval(double added, double taken, i64 elapsed,
                                                i64 created, i64 now, i64 interval,
                                                double capacity, double t, Vote any = Vote()) {
  double a = added, k = taken;
  i64 e = elapsed;
  const TakeResult r = take_step(a, k, e, created, now, interval, capacity, t);
  PeekResult out{r.remaining, r.have_bits, now, r.ok};
  const double fi = (double)interval;
  const double tokens = (added == 0 ? capacity : added) - taken;
  const double missing = capacity - tokens;
  out.retry_at = retry_search(!r.ok, created, elapsed, now, interval, fi, tokens, missing, t, any);
  return out;
}

// ---------------------------------------------------------- throttled -----
// phip_export_throttled / phip_throttle_match (patrolhip.h "Throttled sweep"):
// the caller's rule table as the kernels take it, by value.  A rule's prefix
// is two little-endian words (its byte masks follow from its length), so that
// a match is two and-compares on the first 16 name bytes a record carries
// (Rec: an inline name has all its bytes in the record, a long one its first
// 16); the rate is held as take_step wants it, derived once on the host as
// k_pack_ops does.
struct ThrottleRule {
  u64 p0, p1;        // prefix bytes 0..7, 8..15; bytes past len are zero
  i64 interval;      // rate_interval(freq, per)
  double capacity;   // float64(freq)
  double t;          // float64(count)
  u32 len;
  u32 pad;
};
struct ThrottleRules {
  ThrottleRule r[PHIP_THROTTLE_MAX_RULES];
  u32 n;
};

__host__ __device__ inline u64 low_bytes_mask(u32 k) {   // k in 0..8
  return k >= 8 ? ~0ull : (1ull << (8 * k)) - 1;
}

inline ThrottleRule throttle_rule(const phip_throttle_rule& in) {
  ThrottleRule o{};
  u64 w[2] = {0, 0};
  for (u32 k = 0; k < in.prefix_len; ++k) w[k >> 3] |= (u64)in.prefix[k] << ((k & 7) * 8);
  o.p0 = w[0];
  o.p1 = w[1];
  o.interval = rate_interval(in.freq, in.per);
  o.capacity = (double)in.freq;
  o.t = (double)in.count;
  o.len = in.prefix_len;
  return o;
}

// The first rule, in array order, that matches a name of `len` bytes whose
// first 16 bytes are n0, n1 (little-endian words; what lies past the name does
// not matter: a rule longer than the name never matches, and a shorter one
// masks it off): its index, or -1, and its rate.  A rule matches iff len >=
// its prefix length and the first prefix-length bytes are equal.  The loop is
// uniform (the rules are kernel arguments, read with scalar loads); a lane
// keeps its first hit by selects, so no lane indexes the arguments.
struct ThrottleHit {
  int rule;
  i64 interval;
  double capacity, t;
};
__host__ __device__ inline ThrottleHit throttle_match(const ThrottleRules& R, u64 n0, u64 n1,
                                                      u32 len) {
  ThrottleHit h{-1, 0, 0.0, 0.0};
  u32 i = 0;
  do {   // (R.n >= 1: every caller checks n_rules first)
    const ThrottleRule& q = R.r[i];
    // (& not &&: three compares and selects, no branch per clause)
    const u64 m0 = low_bytes_mask(q.len < 8 ? q.len : 8);   // 0xFF for each prefix byte
    const u64 m1 = low_bytes_mask(q.len < 8 ? 0 : q.len - 8);
    const bool m = (h.rule < 0) & (len >= q.len) & ((n0 & m0) == q.p0) & ((n1 & m1) == q.p1);
    h.rule = m ? (int)i : h.rule;
    h.interval = m ? q.interval : h.interval;
    h.capacity = m ? q.capacity : h.capacity;
    h.t = m ? q.t : h.t;
  } while (++i < R.n);
  return h;
}

// ------------------------------------------------------------ frames -----
// phip_unframe / phip_frame_cuts (patrolhip.h "Packed frames"): the two rules,
// once, for the host forms and the kernels alike.
//
// The splitting rule over frame bytes[o .. end): emit(j, p) for record j of
// the frame, which starts at byte p; returns the frame's record count (>= 1).
// While PHIP_BUCKET_FIXED_SIZE bytes are left and the record its length byte
// announces fits, that is a record; what is left when that fails becomes one
// last, malformed record; an empty frame is one empty record.  Every step but
// the last advances by at least PHIP_BUCKET_FIXED_SIZE bytes: at most
// (end - o) / PHIP_BUCKET_FIXED_SIZE + 1 steps, whatever the bytes hold.
template <class Emit>
__host__ __device__ inline u32 frame_walk(const u8* bytes, u64 o, u64 end, Emit emit) {
  u64 p = o;
  u32 j = 0;
  while (end - p >= PHIP_BUCKET_FIXED_SIZE) {
    const u64 sz = PHIP_BUCKET_FIXED_SIZE + (u64)bytes[p + PHIP_BUCKET_FIXED_SIZE - 1];
    if (sz > end - p) break;
    emit(j++, p);
    p += sz;
  }
  if (p < end || j == 0) emit(j++, p);
  return j;
}

// A frame entry as the unframe check takes it, from the offsets alone: false
// when it decreases, is longer than frame_bytes, or (lim != 0, a checked
// batch) ends past lim.
__host__ __device__ inline bool frame_entry_ok(u64 o, u64 end, u64 lim, u32 frame_bytes) {
  return end >= o && end - o <= frame_bytes && (lim == 0 || end <= lim);
}

// The cut rule's test: a frame that starts at byte o0 may take the record
// that ends at byte e (a decreasing entry never fits).
__host__ __device__ inline bool frame_fits(u64 o0, u64 e, u32 frame_bytes) {
  return e >= o0 && e - o0 <= frame_bytes;
}

// The cut rule over one run of records [r0, r1) (r1 - r0 <= PHIP_FRAME_TILE):
// greedy frames, emit(k, first) for the run's frame k and its first record;
// returns the run's frame count, or ~0u at a record that fits no frame.
template <class Emit>
__host__ __device__ inline u32 frame_cut_run(const uint64_t* offs, u64 r0, u64 r1, u32 frame_bytes,
                                             Emit emit) {
  u32 k = 0;
  u64 first = r0;
  while (first < r1) {
    const u64 o0 = offs[first];
    u64 j = first;
    while (j < r1 && frame_fits(o0, offs[j + 1], frame_bytes)) ++j;
    if (j == first) return ~0u;
    emit(k++, first);
    first = j;
  }
  return k;
}

// Bucket.Merge for one `other` (bucket.go:250-260) on raw values.
__host__ __device__ inline void go_merge(double& a, double& t, i64& e, double oa, double ot,
                                         i64 oe) {
  if (a < oa) a = oa;
  if (t < ot) t = ot;
  if (e < oe) e = oe;
}

// Bucket.IsZero (bucket.go:165-170): -0.0 == 0 is true.
__host__ __device__ inline bool state_is_zero(u64 a_bits, u64 t_bits, i64 e) {
  return is_zero_bits(a_bits) && is_zero_bits(t_bits) && e == 0;
}

// ------------------------------------------------------------ table -----
// One 64-byte slot record = one HBM burst holding everything a lookup and a
// merge touch, ordered so that the Receive fast path reads only the first
// 48 bytes (three 16-byte loads) for names of up to 14 bytes:
//   [ 0,16) tag, added     tag = FNV-1a 64 of the name (0 = empty; a 0 hash is stored as 1)
//   [16,32) taken, elapsed added/taken are E-encoded float64
//   [32,48) name0, name1   canonical name words 0-1
//   [48,64) created, name2 canonical name word 2
// Canonical name (24 bytes, words name0..name2): byte 0 = len, byte 1 = flags
// (kRec*), then len <= 22: bytes 2..2+len = the name, zero padded (names of
// up to 14 bytes end in name1, so name2 = 0); len > 22: bytes 4..7 = arena
// offset, bytes 8..23 = the first 16 bytes (fast reject), full name in the arena.
struct alignas(64) Rec {
  u64 tag;
  u64 added;
  u64 taken;
  i64 elapsed;
  u64 name0;
  u64 name1;
  i64 created;
  u64 name2;
};
static_assert(sizeof(Rec) == 64, "slot record must be one 64-byte burst");

constexpr u32 kInlineName = 22;
constexpr u32 kShortName = 14;     // fits name0/name1: the 48-byte fast path
constexpr u64 kRecPublished = 1u;   // name and state written (visible after a kernel boundary)
constexpr u64 kRecNew = 2u;         // created by the current batch

__host__ __device__ inline u32 rec_flags(const Rec& r) { return (u32)((r.name0 >> 8) & 0xFFu); }
__host__ __device__ inline u64 with_flags(u64 w0, u64 f) { return (w0 & ~0xFF00ull) | (f << 8); }

constexpr u64 kFnvOffset = 0xcbf29ce484222325ull;
constexpr u64 kFnvPrime = 0x100000001b3ull;

// h * 0x100000001b3 == h * 0x1b3 + (h << 40)
__host__ __device__ inline u64 fnv_step(u64 h, u8 c) {
  h ^= c;
  return h * 0x1b3ull + (h << 40);
}

__host__ __device__ inline u64 tag_of(u64 h) { return h ? h : 1ull; }

struct Name {
  u64 w0, w1, w2;   // canonical 24-byte field (see Rec), flags byte 0
  u64 h;            // FNV-1a 64
  u64 off;          // byte offset of the name in its source blob
  u32 len;
};

__host__ __device__ inline void put_name_byte(Name& nm, u32 pos, u8 c) {
  u64 v = (u64)c << ((pos & 7) * 8);
  if (pos < 8) nm.w0 |= v;
  else if (pos < 16) nm.w1 |= v;
  else nm.w2 |= v;
}

// Reads name bytes src[off .. off+len), hashes and canonicalises them.
__host__ __device__ inline void load_name(const u8* src, u64 off, u32 len, Name& nm) {
  nm.w0 = len & 0xFFu; nm.w1 = 0; nm.w2 = 0; nm.h = kFnvOffset; nm.off = off; nm.len = len;
  const bool inl = len <= kInlineName;
  for (u32 k = 0; k < len; ++k) {
    u8 c = src[off + k];
    nm.h = fnv_step(nm.h, c);
    if (inl) put_name_byte(nm, k + 2, c);
    else if (k < 16) put_name_byte(nm, k + 8, c);
  }
}

}  // namespace phip
