// fold_model: test infrastructure only.  A stand-alone host program built
// from the product's own kernel header: the pure functions of the hot-bucket
// block fold (step_sop, window_quiet, window_absorbable, join_state,
// state_grew, ... in patrol_amd/csrc/phip_kernels.hpp) are __host__
// __device__, so the very text k_fold_block runs is compiled for the CPU here
// and checked where no GPU is needed.  It makes no HIP runtime call.
//
//   fold_model replay FILE [OUT]
//     Folds one bucket's segment one op at a time with the host-compiled
//     step_sop, writes every op's results to OUT (default FILE.out), then
//     classifies every kFoldWin window the way k_fold_block decides it and
//     prints one JSON object (fields: see replay()).
//
//     FILE, little-endian, every column padded to a multiple of 8 bytes:
//       u32 magic 0x314d4650 ("PFM1"), u32 n, u32 seeded (0: the bucket is
//       absent at batch start), u32 0
//       u64 added bits, u64 taken bits, i64 elapsed, i64 created   (the seed)
//       u8  kind[n]   (PHIP_OP_TAKE / RECEIVE / UPSERT)
//       i64 now[n], i64 freq[n], i64 per[n], u64 count[n]
//       u64 added[n], u64 taken[n], i64 elapsed[n]                 (bits)
//     OUT, same conventions:
//       u32 magic 0x324d4650 ("PFM2"), u32 n, u32 final existed, u32 0
//       u64 added bits, u64 taken bits, i64 elapsed, i64 created   (final)
//       u8  status[n], u64 remaining[n], u64 have[n], u8 has_reply[n]
//       u64 reply added[n], u64 reply taken[n], i64 reply elapsed[n],
//       i64 reply created[n]      (zero where has_reply is 0)
//
//     Window classes (while the segment is not exact the state a window
//     starts from is the true sequential state S_w, so no R / G bookkeeping):
//       Q quiet:    window_quiet(sum, S_w)
//       A absorbed: not quiet, segment not exact, and
//                   window_absorbable(sum, S_w, join_state(S_w, gmax_of(sum)))
//       F folded:   otherwise
//     The segment turns exact at the first folded window with kSumDirty or at
//     the first Take / creating op in a folded window whose change fails
//     state_grew.  Window summaries follow the comment above struct WinSum.
//     Every Q and A window is also checked op by op against what its class
//     claims ("violations", always 0 unless a predicate is unsound).
//
//   fold_model sweep N SEED
//     Soundness sweep of the two window predicates over N random windows and
//     a constructed integer-exact family at the absorbing bound; exits
//     non-zero on any violation, or when fewer than 10 % of the samples were
//     absorbable windows with Takes or fewer than 1 % quiet windows with
//     Takes (a vacuous sweep; a window without Takes is absorbable whatever
//     the bound says, so it does not count).  Prints its counts as JSON.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../patrol_amd/csrc/phip_kernels.hpp"

using namespace phip;

namespace {

// k_pack_ops for one op (the kernel packs a batch; the arithmetic is this).
OpRec pack_op(u32 kind, i64 now, i64 freq, i64 per, u64 count, u64 a, u64 t, i64 e) {
  if (kind == PHIP_OP_TAKE)
    return OpRec{now, (u64)rate_interval(freq, per), as_bits((double)freq), as_bits((double)count)};
  return OpRec{now, a, t, (u64)e};
}

bool same_state(const FState& x, const FState& y) {
  return x.existed == y.existed && as_bits(x.a) == as_bits(y.a) && as_bits(x.t) == as_bits(y.t) &&
         x.e == y.e && x.c == y.c;
}

// The summary of ops [p0, p1) from the definition above struct WinSum
// (what k_gather_huge reduces in parallel).
WinSum summarize(const OpRec* op, const u32* val, u32 p0, u32 p1) {
  WinSum q;
  memset(&q, 0, sizeof q);
  bool take = false;
  for (u32 j = p0; j < p1; ++j) {
    const u32 kind = val[j] >> kOpIdxBits;
    const OpRec& r = op[j];
    if (kind == PHIP_OP_TAKE) {
      if (!take) {
        take = true;
        q.now_min = q.now_max = r.now;
        q.interval = r.x; q.cap = r.y; q.t = r.z;
        q.flags |= kSumTake;
      } else {
        if (r.now < q.now_min) q.now_min = r.now;
        if (r.now > q.now_max) q.now_max = r.now;
        if (r.x != q.interval || r.y != q.cap || r.z != q.t) q.flags |= kSumMixed;
      }
    } else if (kind == PHIP_OP_UPSERT || !state_is_zero(r.x, r.y, (i64)r.z)) {
      q.flags |= kSumMerge;
      if (r.x == kSign || r.y == kSign) q.flags |= kSumDirty;
      const u64 ea = enc_replica(r.x), et = enc_replica(r.y), ee = r.z ^ kSign;
      if (ea > q.ea) q.ea = ea;
      if (et > q.et) q.et = et;
      if (ee > q.ee) q.ee = ee;
    }
  }
  return q;
}

// ------------------------------------------------------------- replay ----
std::vector<unsigned char> read_file(const char* path) {
  std::vector<unsigned char> b;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  unsigned char buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
  fclose(f);
  return b;
}

size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

int replay(const char* in_path, const char* out_path) {
  const std::vector<unsigned char> in = read_file(in_path);
  if (in.size() < 48) { fprintf(stderr, "fold_model: short file\n"); return 2; }
  u32 hdr[4];
  memcpy(hdr, in.data(), 16);
  const u32 n = hdr[1];
  if (hdr[0] != 0x314d4650u || n == 0 || n > kOpIdxMask ||
      in.size() != 48 + pad8(n) + (size_t)n * 56) {
    fprintf(stderr, "fold_model: bad header or size\n");
    return 2;
  }
  u64 seed[4];
  memcpy(seed, in.data() + 16, 32);
  const unsigned char* p = in.data() + 48;
  const u8* kind = p; p += pad8(n);
  std::vector<i64> now(n), freq(n), per(n), el(n);
  std::vector<u64> cnt(n), ad(n), tk(n);
  memcpy(now.data(), p, (size_t)n * 8); p += (size_t)n * 8;
  memcpy(freq.data(), p, (size_t)n * 8); p += (size_t)n * 8;
  memcpy(per.data(), p, (size_t)n * 8); p += (size_t)n * 8;
  memcpy(cnt.data(), p, (size_t)n * 8); p += (size_t)n * 8;
  memcpy(ad.data(), p, (size_t)n * 8); p += (size_t)n * 8;
  memcpy(tk.data(), p, (size_t)n * 8); p += (size_t)n * 8;
  memcpy(el.data(), p, (size_t)n * 8);

  std::vector<OpRec> op(n);
  std::vector<u32> val(n);
  for (u32 i = 0; i < n; ++i) {
    if (kind[i] > PHIP_OP_UPSERT) { fprintf(stderr, "fold_model: bad kind at %u\n", i); return 2; }
    op[i] = pack_op(kind[i], now[i], freq[i], per[i], cnt[i], ad[i], tk[i], el[i]);
    val[i] = i | ((u32)kind[i] << kOpIdxBits);
  }

  FState S;
  if (hdr[2]) {
    S.a = as_f64(seed[0]); S.t = as_f64(seed[1]); S.e = (i64)seed[2]; S.c = (i64)seed[3];
    S.existed = true;
  } else {   // k_publish's record of a bucket the batch creates
    S.a = 0.0; S.t = 0.0; S.e = 0; S.c = 0; S.existed = false;
  }

  std::vector<u8> o_st(pad8(n), 0), o_hr(pad8(n), 0);
  std::vector<u64> o_rem(n, 0), o_have(n, 0), o_ra(n, 0), o_rt(n, 0);
  std::vector<i64> o_re(n, 0), o_rc(n, 0);

  const u32 nwin = (n + kFoldWin - 1) / kFoldWin;
  std::string classes(nwin, '?');
  u64 n_quiet = 0, n_abs = 0, n_fold = 0, violations = 0;
  u64 take_ok = 0, take_denied = 0, denied_changed = 0, raising = 0, inc_reply = 0, inc_noreply = 0;
  u64 runs = 1, run_at_window_start = 0, change_at_window_first_op = 0;
  bool exact = false, g_nonempty_at_exact = false;
  const char* why = "never";
  i64 exact_pos = -1, exact_run = -1;
  GMax G{0, 0, 0};

  for (u32 w = 0; w < nwin; ++w) {
    const u32 p0 = w * kFoldWin, p1 = p0 + kFoldWin < n ? p0 + kFoldWin : n;
    const WinSum sum = summarize(op.data(), val.data(), p0, p1);
    const FState Sw = S;
    char cls = 'F';
    if (window_quiet(sum, Sw)) cls = 'Q';
    else if (!exact && window_absorbable(sum, Sw, join_state(Sw, gmax_of(sum)))) cls = 'A';
    classes[w] = cls;
    if (cls == 'Q') ++n_quiet; else if (cls == 'A') ++n_abs; else ++n_fold;
    if (cls == 'F' && !exact && (sum.flags & kSumDirty)) {
      exact = true;
      why = "negzero";
      exact_pos = p0;
      g_nonempty_at_exact = !gmax_empty(G);
      if (g_nonempty_at_exact) { exact_run = (i64)runs; ++runs; }   // a run holding the true state
      else exact_run = (i64)runs - 1;
    }
    for (u32 j = p0; j < p1; ++j) {
      const SOp sop = make_sop(op[j], val[j]);
      FState S2;
      OpOut out;
      const bool chg = eval_sop(sop, S, S2, out);
      {   // apply_sop is the same code without the outputs
        FState S3;
        if (apply_sop(sop, S, S3) != chg || !same_state(S2, S3)) ++violations;
      }
      const u32 st = out.st & 0x7F;
      const bool is_take = sop.kind == PHIP_OP_TAKE;
      if (st == PHIP_ST_TAKE_OK) ++take_ok;
      if (st == PHIP_ST_TAKE_DENIED) { ++take_denied; if (chg && S.existed) ++denied_changed; }
      if (st == PHIP_ST_INCAST_REPLY) ++inc_reply;
      if (st == PHIP_ST_INCAST_NOREPLY) ++inc_noreply;
      if (st == PHIP_ST_MERGED && chg && S.existed) ++raising;
      if (cls == 'Q' && chg) ++violations;
      if (cls == 'A' && is_take && (chg || st != PHIP_ST_TAKE_DENIED)) ++violations;
      if (cls == 'F') {
        const bool counts = exact || is_take || !S.existed;   // absorbing: merges need no run
        if (chg && counts) {
          if (!exact && !state_grew(S, S2)) {
            exact = true;
            why = "lowered";
            exact_pos = j;
            exact_run = (i64)runs;
            g_nonempty_at_exact = !gmax_empty(G);
          }
          ++runs;
          if ((j + 1) % kFoldWin == 0 && j + 1 < n) ++run_at_window_start;
          if (j % kFoldWin == 0) ++change_at_window_first_op;
        }
      }
      G = gmax(G, merge_contrib(op[j], val[j]));
      o_st[j] = out.st; o_rem[j] = out.rem; o_have[j] = out.have; o_hr[j] = out.has_reply;
      if (out.has_reply) {
        o_ra[j] = as_bits(S2.a); o_rt[j] = as_bits(S2.t); o_re[j] = S2.e; o_rc[j] = S2.c;
      }
      S = S2;
    }
    if (cls == 'A' && !same_state(S, join_state(Sw, gmax_of(sum)))) ++violations;
    if (cls == 'Q' && !same_state(S, Sw)) ++violations;
  }

  FILE* f = fopen(out_path, "wb");
  if (!f) { perror(out_path); return 2; }
  const u32 ohdr[4] = {0x324d4650u, n, S.existed ? 1u : 0u, 0};
  const u64 fin[4] = {as_bits(S.a), as_bits(S.t), (u64)S.e, (u64)S.c};
  bool ok = fwrite(ohdr, 16, 1, f) == 1 && fwrite(fin, 32, 1, f) == 1 &&
            fwrite(o_st.data(), 1, o_st.size(), f) == o_st.size() &&
            fwrite(o_rem.data(), 8, n, f) == n && fwrite(o_have.data(), 8, n, f) == n &&
            fwrite(o_hr.data(), 1, o_hr.size(), f) == o_hr.size() &&
            fwrite(o_ra.data(), 8, n, f) == n && fwrite(o_rt.data(), 8, n, f) == n &&
            fwrite(o_re.data(), 8, n, f) == n && fwrite(o_rc.data(), 8, n, f) == n;
  ok = fclose(f) == 0 && ok;
  if (!ok) { fprintf(stderr, "fold_model: write failed\n"); return 2; }

  // exact.pos: the op (lowered) or the window's first op (negzero) where the
  // segment turned exact; exact.run: the first exact run; exact.g_nonempty:
  // whether merges had been absorbed by then.  runs: the initial run plus
  // every state change k_fold_block would record; run_at_window_start: runs
  // that begin at a window's first op (the change was the last op of the
  // window before); change_at_window_first_op: runs begun by a window's
  // first op.
  printf("{\"ops\": %u, \"window\": %u, \"windows\": %u, \"quiet\": %llu, \"absorbed\": %llu, "
         "\"folded\": %llu, \"classes\": \"%s\", \"exact\": {\"why\": \"%s\", \"pos\": %lld, "
         "\"run\": %lld, \"g_nonempty\": %s}, \"runs\": %llu, \"run_at_window_start\": %llu, "
         "\"change_at_window_first_op\": %llu, "
         "\"take_ok\": %llu, \"take_denied\": %llu, \"denied_changed\": %llu, "
         "\"raising_merges\": %llu, \"incast_reply\": %llu, \"incast_noreply\": %llu, "
         "\"violations\": %llu}\n",
         n, kFoldWin, nwin, n_quiet, n_abs, n_fold, classes.c_str(), why, exact_pos, exact_run,
         g_nonempty_at_exact ? "true" : "false", runs, run_at_window_start,
         change_at_window_first_op, take_ok, take_denied,
         denied_changed, raising, inc_reply, inc_noreply, violations);
  return violations ? 1 : 0;
}

// -------------------------------------------------------------- sweep ----
struct Rng {
  u64 s;
  u64 next() {   // splitmix64
    u64 z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  u64 below(u64 n) { return next() % n; }
  bool chance(u32 pct) { return below(100) < pct; }
  i64 range(i64 lo, i64 hi) { return lo + (i64)below((u64)(hi - lo) + 1); }
  double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

constexpr i64 kT0 = 1700000000000000000ll;
constexpr i64 kI64Max = 0x7FFFFFFFFFFFFFFFll;

const u64 kSpecialF[] = {0x0ull, kSign, kInfBits, kSign | kInfBits, 0x7FF8000000000000ull,
                         0xFFF8000000000001ull, 0x7FF0000000000001ull, 0x3FF0000000000000ull,
                         0xBFF0000000000000ull, 0x1ull, kSign | 1ull, 0x7FEFFFFFFFFFFFFFull,
                         0xFFEFFFFFFFFFFFFFull, 0x4340000000000000ull /* 2^53 */,
                         0x43E0000000000000ull /* 2^63 */, 0x7E37E43C8800759Cull /* 1e300 */};
const i64 kSpecialI[] = {0, 1, -1, kI64Max, kI64Max - 1, -kI64Max - 1, -kI64Max, 1ll << 62,
                         -(1ll << 62), kT0, -kT0, 1000000000ll, -1000000000ll};

u64 wild_f(Rng& r) {
  const u32 k = (u32)r.below(10);
  if (k < 3) return kSpecialF[r.below(sizeof kSpecialF / sizeof kSpecialF[0])];
  if (k < 4) return r.next();                                      // any bit pattern
  if (k < 5) return as_bits(-(r.unit() * 1e4));                    // negative
  if (k < 6) return as_bits((double)r.below(1000000) * 1e12);      // huge
  return as_bits((double)r.below(10000) + (r.chance(50) ? r.unit() * 100.0 : 0.0));
}
i64 wild_i(Rng& r) {
  const u32 k = (u32)r.below(10);
  if (k < 3) return kSpecialI[r.below(sizeof kSpecialI / sizeof kSpecialI[0])];
  if (k < 4) return (i64)r.next();
  if (k < 5) return kI64Max - (i64)r.below(1ull << 40);            // near overflow
  if (k < 6) return -(i64)r.below(1ull << 40);
  return (i64)r.below(1ull << 40);
}

struct Window {
  FState R;
  GMax G0;
  std::vector<OpRec> op;
  std::vector<u32> val;
};

// The rate-limited hot bucket the fold was written for: tokens near zero,
// replicas close to the state, clocks around created + elapsed.
void gen_regime(Rng& r, Window& W) {
  const i64 iv_pool[] = {10000000, 1000000000, 1, 333333333, 50000};
  const i64 iv = iv_pool[r.below(5)];
  const i64 freq = 1 + (i64)r.below(200), count = 1 + (i64)r.below(4);
  const double base = (double)r.below(100000);
  FState& R = W.R;
  R.t = base + (r.chance(30) ? r.unit() : 0.0);
  R.a = R.t + (r.chance(50) ? (double)r.below(3) : r.unit() * 3.0);
  if (R.a == 0) R.a = 1.0;
  R.c = kT0 - r.range(0, 1000000000);
  R.e = r.range(0, 3000000000ll);
  R.existed = true;
  const i64 last = R.c + R.e;
  const u32 merge_mode = (u32)r.below(4);   // 0: none, 1: stale, 2: raising, 3: both
  W.G0 = GMax{0, 0, 0};
  if (r.chance(40))
    W.G0 = GMax{enc_replica(as_bits(R.a - r.unit() * 2.0 + 0.5)),
                enc_replica(as_bits(R.t - 1.0 + r.unit() * 1.5)),
                (u64)(R.e + r.range(-1000000, 1000000)) ^ kSign};
  const u32 L = 1 + (u32)r.below(24);
  const i64 span = r.chance(60) ? iv / 2 : iv * (i64)(1 + r.below(4));
  for (u32 j = 0; j < L; ++j) {
    const u32 k = (u32)r.below(10);
    u32 kind;
    OpRec o;
    if (k < 5) {
      kind = PHIP_OP_TAKE;
      const i64 now = last + r.range(-span, span);   // not monotone
      o = OpRec{now, (u64)iv, as_bits((double)freq), as_bits((double)count)};
    } else if (k < 6 || merge_mode == 0) {
      kind = PHIP_OP_RECEIVE;   // an incast request
      o = OpRec{kT0, 0, 0, 0};
    } else {
      kind = r.chance(85) ? PHIP_OP_RECEIVE : PHIP_OP_UPSERT;
      const bool up = merge_mode == 2 || (merge_mode == 3 && r.chance(50));
      const double da = up ? r.unit() * 1.5 : -r.unit() * 50.0;
      const double dt = up ? r.unit() * 1.5 : -r.unit() * 50.0;
      o = OpRec{kT0, as_bits(R.a + da), as_bits(R.t + dt),
                (u64)(R.e + (up ? r.range(0, span) : -r.range(0, 1000000000)))};
    }
    W.op.push_back(o);
    W.val.push_back(j | (kind << kOpIdxBits));
  }
}

// Anything goes: special values in every field, every interval sign.
void gen_wild(Rng& r, Window& W) {
  FState& R = W.R;
  R.a = as_f64(wild_f(r)); R.t = as_f64(wild_f(r));
  R.e = wild_i(r); R.c = r.chance(50) ? kT0 - r.range(0, 1000000000) : wild_i(r);
  R.existed = !r.chance(3);
  W.G0 = GMax{0, 0, 0};
  if (r.chance(50))
    W.G0 = GMax{enc_replica(wild_f(r)), enc_replica(wild_f(r)), (u64)wild_i(r) ^ kSign};
  const i64 ivs[] = {10000000, 1, 0, -10000000, -1, kI64Max, -kI64Max - 1, 1000000000};
  const bool shared = r.chance(80);
  i64 iv = ivs[r.below(8)];
  double cap = (double)r.range(-5, 200), t = (double)r.below(5);
  const u32 L = 1 + (u32)r.below(16);
  for (u32 j = 0; j < L; ++j) {
    const u32 k = (u32)r.below(10);
    u32 kind;
    OpRec o;
    if (k < 4) {
      kind = PHIP_OP_TAKE;
      if (!shared && r.chance(30)) { iv = ivs[r.below(8)]; t = (double)r.below(5); }
      const i64 now = r.chance(70) ? kT0 + r.range(-2000000000ll, 2000000000ll) : wild_i(r);
      o = OpRec{now, (u64)iv, as_bits(cap), as_bits(t)};
    } else if (k < 5) {
      kind = PHIP_OP_RECEIVE;
      o = OpRec{kT0, r.chance(50) ? 0 : kSign, 0, 0};   // incast requests (IsZero: -0.0 too)
    } else {
      kind = r.chance(80) ? PHIP_OP_RECEIVE : PHIP_OP_UPSERT;
      o = OpRec{kT0, wild_f(r), wild_f(r), (u64)wild_i(r)};
    }
    W.op.push_back(o);
    W.val.push_back(j | (kind << kOpIdxBits));
  }
}

struct SweepCounts {
  u64 samples = 0, quiet = 0, absorbable = 0, violations = 0, family = 0;
  // the samples that test the arithmetic: windows with Takes; those where
  // only the absorbing bound holds and the window's merges raise the state
  u64 quiet_take = 0, absorbable_take = 0, absorbable_raised = 0;
};

void report(const char* what, const Window& W, u32 j) {
  static u32 shown = 0;
  if (++shown > 8) return;   // the first few say it all
  fprintf(stderr, "violation: %s at op %u; R = %016llx %016llx %lld %lld, G0 = %llx %llx %llx\n",
          what, j, (unsigned long long)as_bits(W.R.a), (unsigned long long)as_bits(W.R.t),
          (long long)W.R.e,
          (long long)W.R.c, (unsigned long long)W.G0.a, (unsigned long long)W.G0.t,
          (unsigned long long)W.G0.e);
  for (size_t k = 0; k < W.op.size(); ++k)
    fprintf(stderr, "  op %zu kind %u now %lld x %016llx y %016llx z %016llx\n", k,
            W.val[k] >> kOpIdxBits, (long long)W.op[k].now, (unsigned long long)W.op[k].x,
            (unsigned long long)W.op[k].y, (unsigned long long)W.op[k].z);
}

// What a true predicate promises, checked against the sequential fold.
void check_window(const Window& W, SweepCounts& C, bool* quiet_out = nullptr,
                  bool* abs_out = nullptr) {
  const u32 L = (u32)W.op.size();
  const WinSum sum = summarize(W.op.data(), W.val.data(), 0, L);
  // as k_fold_block forms them: Xs from the merges before the window, Xe
  // with the window's own maxima on top
  const FState Xs = join_state(W.R, W.G0);
  const FState Xe = join_state(W.R, gmax(W.G0, gmax_of(sum)));
  const bool quiet = window_quiet(sum, Xs);
  const bool absorb = window_absorbable(sum, Xs, Xe);
  ++C.samples;
  C.quiet += quiet;
  C.absorbable += absorb;
  if (sum.flags & kSumTake) {
    C.quiet_take += quiet;
    C.absorbable_take += absorb;
    C.absorbable_raised += absorb && !quiet && !same_state(Xs, Xe);
  }
  if (quiet_out) *quiet_out = quiet;
  if (abs_out) *abs_out = absorb;
  if (!quiet && !absorb) return;
  FState S = Xs;
  GMax g{0, 0, 0};
  for (u32 j = 0; j < L; ++j) {
    const SOp sop = make_sop(W.op[j], W.val[j]);
    FState S2;
    OpOut out;
    const bool chg = eval_sop(sop, S, S2, out);
    const bool is_take = sop.kind == PHIP_OP_TAKE;
    bool bad = false;
    if (quiet && chg) { report("quiet window, op changed the state", W, j); bad = true; }
    if (is_take && (chg || (out.st & 0x7F) != PHIP_ST_TAKE_DENIED)) {
      report("Take succeeded or changed the state", W, j);
      bad = true;
    }
    g = gmax(g, merge_contrib(W.op[j], W.val[j]));
    // the state every later op sees is the join k_huge_outputs rebuilds
    if (absorb && !same_state(S2, join_state(Xs, g))) {
      report("state after op differs from join_state(Xs, G prefix)", W, j);
      bad = true;
    }
    if (bad) { ++C.violations; return; }
    S = S2;
  }
  if (absorb && !same_state(S, join_state(Xs, gmax_of(sum)))) {
    report("end state differs from join_state(Xs, window maxima)", W, L);
    ++C.violations;
  }
  if (quiet && !same_state(S, Xs)) {
    report("quiet window, end state differs", W, L);
    ++C.violations;
  }
}

// Constructed family: every quantity an integer and dt a multiple of the
// interval, so tok + add is exact and equals Take's `have`; one Take at
// now_max on Xs == Xe with t at bound - 1, bound, bound + 1.  The Take must
// succeed up to the bound, and both predicates must hold exactly above it:
// sampling never lands on equality, this does.
void family(SweepCounts& C) {
  const i64 ivs[] = {1, 7, 10000000, 1000000000};
  for (i64 iv : ivs)
    for (i64 tok = 0; tok <= 3; ++tok)
      for (i64 k = 0; k <= 5; ++k)
        for (i64 taken : {0ll, 5ll, 1000000ll})
          for (int stale_merge = 0; stale_merge < 2; ++stale_merge)
            for (i64 d = -1; d <= 1; ++d) {
              const i64 bound = tok + k, t = bound + d;
              if (t < 0) continue;
              Window W;
              W.R.a = (double)(taken + tok); W.R.t = (double)taken;
              if (W.R.a == 0) continue;   // the added = capacity write is another case
              W.R.c = kT0; W.R.e = 12345 * iv; W.R.existed = true;
              W.G0 = GMax{0, 0, 0};
              const i64 now = W.R.c + W.R.e + k * iv;
              const double cap = (double)(bound + 10);   // missing never caps the refill
              if (stale_merge) {   // a merge that raises nothing: Xe == Xs still
                W.op.push_back(OpRec{kT0, as_bits(W.R.a), as_bits(W.R.t), (u64)W.R.e});
                W.val.push_back(0u | ((u32)PHIP_OP_RECEIVE << kOpIdxBits));
                W.op.push_back(OpRec{now - iv, (u64)iv, as_bits(cap), as_bits((double)t)});
                W.val.push_back(1u | ((u32)PHIP_OP_TAKE << kOpIdxBits));
              }
              W.val.push_back((u32)W.op.size() | ((u32)PHIP_OP_TAKE << kOpIdxBits));
              W.op.push_back(OpRec{now, (u64)iv, as_bits(cap), as_bits((double)t)});
              bool quiet = false, absorb = false;
              SweepCounts F;
              check_window(W, F, &quiet, &absorb);
              C.violations += F.violations;
              ++C.family;
              // the ground truth: Take at now_max is denied iff t > bound
              FState S = W.R, S2;
              OpOut out;
              eval_sop(make_sop(W.op.back(), W.val.back()), S, S2, out);
              const bool denied = (out.st & 0x7F) == PHIP_ST_TAKE_DENIED;
              // (have: Take's `have` when denied, what is left when granted)
              if (denied != (t > bound) ||
                  out.have != as_bits((double)(denied ? bound : bound - t))) {
                report("family: have is not the bound", W, 0);
                ++C.violations;
              }
              if (absorb != (t > bound)) {
                report(absorb ? "family: absorbable at or below the bound"
                              : "family: not absorbable above the bound", W, 0);
                ++C.violations;
              }
              if (quiet != (t > bound)) {
                report(quiet ? "family: quiet at or below the bound"
                             : "family: not quiet above the bound", W, 0);
                ++C.violations;
              }
            }
}

int sweep(u64 n, u64 seed) {
  Rng r{seed};
  SweepCounts C;
  for (u64 i = 0; i < n && C.violations < 8; ++i) {
    Window W;
    if (r.chance(55)) gen_regime(r, W); else gen_wild(r, W);
    check_window(W, C);
  }
  const SweepCounts R = C;   // the random part
  family(C);
  // the floors count windows with Takes only: a window without one is
  // absorbable whatever the bound says
  const bool vacuous = R.absorbable_take * 10 < R.samples || R.quiet_take * 100 < R.samples;
  printf("{\"samples\": %llu, \"absorbable\": %llu, \"quiet\": %llu, "
         "\"absorbable_with_takes\": %llu, "
         "\"quiet_with_takes\": %llu, \"absorbable_only_raised\": %llu, \"family\": %llu, "
         "\"violations\": %llu, \"vacuous\": %s}\n",
         R.samples, R.absorbable, R.quiet, R.absorbable_take, R.quiet_take, R.absorbable_raised,
         C.family, C.violations, vacuous ? "true" : "false");
  return (C.violations || vacuous) ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "replay")) {
    const std::string out = argc >= 4 ? argv[3] : std::string(argv[2]) + ".out";
    return replay(argv[2], out.c_str());
  }
  if (argc == 4 && !strcmp(argv[1], "sweep"))
    return sweep(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
  fprintf(stderr, "usage: fold_model replay FILE [OUT] | fold_model sweep N SEED\n");
  return 2;
}
