// peek_eval (phip_device.hpp) on the host over the int64 / float64 edge grid,
// for a run under the host sanitizers: the function k_peek calls is compiled
// here for the CPU, with its own main, and touches no GPU.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I include -I patrol_amd/csrc -o tools/peek_eval_check tools/peek_eval_check.cpp
//   ./tools/peek_eval_check
//
// Every grid point is also checked against the definition of retry_at
// (patrolhip.h "Peek") with take_step itself as the verdict: granted gives now;
// a finite answer is granted there and denied one reading earlier; never is
// denied at INT64_MAX.  Prints the counts; exit status 1 on a violation.
#include <cstdio>
#include <cstdlib>

#include "phip_device.hpp"

using namespace phip;

static bool ok_at(u64 a, u64 t, i64 e, i64 c, i64 at, i64 iv, double cap, double n) {
  double x = as_f64(a), y = as_f64(t);
  return take_step(x, y, e, c, at, iv, cap, n).ok;
}

int main() {
  const i64 kMax = 0x7FFFFFFFFFFFFFFFll, kMin = (i64)kSign, T0 = 1700000000000000000ll;
  const u64 f64s[] = {0x7FF8000000000000ull, 0x7FF0000000000001ull, 0xFFF8000000000001ull, 0ull, kSign,
                      kInfBits, kSign | kInfBits, as_bits(-1.0), as_bits(-1e300),
                      as_bits(9007199254740992.0), 1ull, kSign | 1ull, as_bits(1.0), as_bits(0.5),
                      as_bits(100.0), as_bits(99.0), as_bits(9223372036854775808.0)};
  const i64 i64s[] = {0, 1, -1, kMax, kMin, kMax - 1, kMin + 1, 1ll << 62, -(1ll << 62), T0, -T0};
  const i64 nows[] = {0, -1, kMax, kMin, kMax - 1, T0, T0 + 1, T0 + 999999999, -T0, 1ll << 62};
  const i64 rates[][2] = {{0, 1000000000}, {5, 0}, {-3, 1000000000}, {3, -1000000000}, {10, 3},
                          {-1, kMin}, {1, kMax}, {kMax, kMax}, {1, 1}, {2, 7}, {100, 1000000000},
                          {3, 1000000000}, {30, 60000000000ll}, {kMin, kMin}};
  const u64 counts[] = {0, 1, 5, 101, 1ull << 63, ~0ull};
  unsigned long long n = 0, granted = 0, finite = 0, never = 0, sum = 0;
  for (u64 a : f64s) for (u64 t : f64s) for (i64 e : i64s) for (i64 c : i64s)
    for (i64 now : nows) for (auto& r : rates) for (u64 cnt : counts) {
      const i64 iv = rate_interval(r[0], r[1]);
      const double cap = (double)r[0], want = (double)cnt;
      const PeekResult p = peek_eval(as_f64(a), as_f64(t), e, c, now, iv, cap, want);
      const bool ok = ok_at(a, t, e, c, now, iv, cap, want);
      bool good = p.ok == ok;
      if (ok) { good = good && p.retry_at == now; ++granted; }
      else if (p.retry_at == kMin) { good = good && !ok_at(a, t, e, c, kMax, iv, cap, want); ++never; }
      else {
        good = good && p.retry_at > now && ok_at(a, t, e, c, p.retry_at, iv, cap, want) &&
               !ok_at(a, t, e, c, p.retry_at - 1, iv, cap, want);
        ++finite;
      }
      if (!good) {
        printf("violation: a=%llx t=%llx e=%lld c=%lld now=%lld rate=%lld/%lld count=%llu -> %lld\n",
               a, t, e, c, now, r[0], r[1], cnt, p.retry_at);
        return 1;
      }
      sum += p.remaining ^ p.have_bits ^ (u64)p.retry_at;
      ++n;
    }
  printf("peek_eval_check: %llu points (%llu granted, %llu finite, %llu never), checksum %016llx: clean\n",
         n, granted, finite, never, sum);
  return 0;
}
