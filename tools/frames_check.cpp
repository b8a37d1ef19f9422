// The packed-frames rules on the host (phip_device.hpp: frame_walk,
// frame_entry_ok, frame_cut_run -- the functions the kernels and the host
// forms of phip_unframe / phip_frame_cuts share) and phip_frame_reply_peers
// (phip_udp.cpp), for a run under the host sanitizers: compiled for the CPU
// with its own main, touches no GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -I /opt/rocm/include -I include -I patrol_amd/csrc \
//       -o tools/frames_check tools/frames_check.cpp patrol_amd/csrc/phip_udp.cpp
//   ./tools/frames_check
//
// Every buffer is allocated at its exact size, so a read past a frame's end or
// a store past the counted records is a sanitizer report.  Each case is also
// checked against a second, byte-at-a-time statement of the rule.  Prints the
// case count and "clean"; exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "phip_device.hpp"

using namespace phip;

// phip_udp.cpp's phip_incast_replies refers to it; nothing here calls either.
extern "C" int phip_marshal(const uint8_t*, uint32_t, const phip_state*, uint8_t*) {
  return PHIP_ERR_INVALID;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int fail(const char* what, unsigned c) {
  std::printf("MISMATCH: %s (case %u)\n", what, c);
  return 1;
}

// One frame of `len` bytes at its exact size: walked, and compared with the
// rule restated over sizes.
static int check_walk(const std::vector<u8>& frame, unsigned c) {
  const u64 len = frame.size();
  std::vector<u64> want;
  if (len == 0) want.push_back(0);
  u64 p = 0;
  while (len - p >= 25 && 25 + (u64)frame[p + 24] <= len - p) {
    want.push_back(p);
    p += 25 + frame[p + 24];
  }
  if (p < len) want.push_back(p);
  std::vector<u64> got(want.size());   // exact: a record too many is a heap overflow
  u32 steps = 0;
  const u32 n = frame_walk(frame.data(), 0, len, [&](u32 j, u64 q) {
    got[j] = q;
    ++steps;
  });
  if (n != want.size() || steps != n || got != want) return fail("frame_walk", c);
  if (n > len / 25 + 1) return fail("walk bound", c);
  return 0;
}

static int check_cuts(const std::vector<uint64_t>& offs, u32 fb, unsigned c) {
  const u64 n = offs.size() - 1;
  for (u64 r0 = 0; r0 < n; r0 += PHIP_FRAME_TILE) {
    const u64 r1 = r0 + PHIP_FRAME_TILE < n ? r0 + PHIP_FRAME_TILE : n;
    std::vector<u64> firsts;
    const u32 k = frame_cut_run(offs.data(), r0, r1, fb, [&](u32 j, u64 first) {
      if (j != firsts.size()) std::abort();
      firsts.push_back(first);
    });
    bool oversized = false;
    for (u64 i = r0; i < r1; ++i) oversized |= offs[i + 1] - offs[i] > fb;
    if (oversized != (k == ~0u)) return fail("oversized record", c);
    if (oversized) continue;
    if (k != firsts.size() || firsts.empty() || firsts[0] != r0) return fail("run start", c);
    for (u32 f = 0; f < k; ++f) {
      const u64 a = firsts[f], b = f + 1 < k ? firsts[f + 1] : r1;
      if (b <= a || offs[b] - offs[a] > fb) return fail("frame size", c);
      if (b < r1 && offs[b + 1] - offs[a] <= fb) return fail("not greedy", c);
    }
  }
  return 0;
}

int main() {
  unsigned cases = 0;
  // the walk: edge frames, then random frames whose length bytes are random
  const size_t edge[] = {0, 1, 24, 25, 26, 49, 50, 255, 256, 1450, 1472, 65507};
  for (size_t len : edge)
    for (int fill : {0, 1, 230, 231, 255}) {
      std::vector<u8> f(len, (u8)fill);
      if (check_walk(f, cases++)) return 1;
    }
  for (int it = 0; it < 4000; ++it) {
    std::vector<u8> f(rnd() % 1600);
    for (auto& b : f) b = (rnd() & 3) ? (u8)(rnd() % 12) : (u8)rnd();
    if (check_walk(f, cases++)) return 1;
  }
  // the entry check
  if (!frame_entry_ok(10, 10, 0, 256) || frame_entry_ok(11, 10, 0, 256) ||
      frame_entry_ok(0, 257, 0, 256) || !frame_entry_ok(0, 256, 256, 256) ||
      frame_entry_ok(0, 256, 255, 256) || frame_entry_ok(1ull << 40, (1ull << 40) + 1, 4096, 256))
    return fail("frame_entry_ok", cases);
  ++cases;
  // the cuts
  const u32 fbs[] = {256, 1472, 8972, 65507};
  const u64 ns[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 8193};
  for (u32 fb : fbs)
    for (u64 n : ns)
      for (int kind = 0; kind < 3; ++kind) {
        std::vector<uint64_t> offs(n + 1);
        offs[0] = rnd() % 1000;
        for (u64 i = 0; i < n; ++i)
          offs[i + 1] = offs[i] + (kind == 0 ? 25 : kind == 1 ? 25 + rnd() % 232 : 200 + rnd() % 60);
        if (check_cuts(offs, fb, cases++)) return 1;
      }
  {
    std::vector<uint64_t> dec = {100, 130, 90, 60};   // an end below its frame's start fits no frame
    if (frame_cut_run(dec.data(), 0, 3, 256, [](u32, u64) {}) != ~0u)
      return fail("decreasing entry", cases);
    ++cases;
  }
  // phip_frame_reply_peers: out[k] = peers[rec_frame[src[k]]]
  {
    const u32 nframes = 5, nrec = 17, nsrc = 9;
    std::vector<u8> peers((size_t)nframes * PHIP_PEER_BYTES);
    for (auto& b : peers) b = (u8)rnd();
    std::vector<u32> rec_frame(nrec), src(nsrc);
    for (u32 k = 0; k < nrec; ++k) rec_frame[k] = k * nframes / nrec;
    for (u32 k = 0; k < nsrc; ++k) src[k] = (u32)(rnd() % nrec);
    std::vector<u8> out((size_t)nsrc * PHIP_PEER_BYTES);
    if (phip_frame_reply_peers(peers.data(), rec_frame.data(), src.data(), nsrc, out.data()) != PHIP_OK)
      return fail("frame_reply_peers rc", cases);
    for (u32 k = 0; k < nsrc; ++k)
      if (std::memcmp(&out[(size_t)k * PHIP_PEER_BYTES],
                      &peers[(size_t)rec_frame[src[k]] * PHIP_PEER_BYTES], PHIP_PEER_BYTES))
        return fail("frame_reply_peers", cases);
    if (phip_frame_reply_peers(nullptr, nullptr, nullptr, 0, nullptr) != PHIP_OK ||
        phip_frame_reply_peers(nullptr, rec_frame.data(), src.data(), 1, out.data()) != PHIP_ERR_INVALID)
      return fail("frame_reply_peers arguments", cases);
    ++cases;
  }
  std::printf("%u cases clean\n", cases);
  return 0;
}
