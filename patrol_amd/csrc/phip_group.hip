// Shard group: the buckets of one node hash-sharded by name over
// its GPUs, one phip_handle and one RCCL rank per GPU.  The reference has a
// single map behind one mutex (repo.go:171-235) fed by one Receive goroutine
// (repo.go:54-92); here every GPU owns the buckets whose name hashes to it,
// messages that arrive anywhere are routed to their owner, and simulated
// replicas converge by an all-reduce(max).
//
// Per member and call, one host thread: it binds its GPU and queues the
// member's work on three streams, synchronising only to read the split sizes
// of each chunk's exchange.  With one process per GPU the calling thread is
// the member's thread.
//
// Owner-routed Receive is pipelined by chunks of kChunk messages, over two
// send sets and two receive sets: while chunk k travels (exchange stream: the
// split sizes, then the grouped per-peer send/recv), the pack of chunk k+1
// (pack stream) and the owner's merge of chunk k-1 (the handle's stream) run
// beside it.
//
// Members sharing one GPU (phip_group_open_all with a device listed more
// than once: several shards' tables on one device, e.g. to rehearse an
// N-GPU group on one) exchange without RCCL, which refuses two ranks on one
// device: the member threads meet at a barrier once every member's packed
// send buffers and split sizes are ready, and each copies its segments from
// its peers' buffers with device copies; the all-reduce is an element-wise
// max over the members' joins.  The packing, segment offsets, source order
// and merge are the same code as the RCCL path.
//
// The *_replies forms of Receive also answer the incast requests (zero
// states, repo.go:86-90) that arrived at each member.  Every chunk's split
// sizes carry the number of zero-state messages its member holds, so all
// members know alike whether a round has requests; such a round leaves the
// pipeline (reply_round): its owners merge with phip_receive_soa_replies, the
// answers alone travel back along a plan made of their per-source counts, and
// the source appends them to the caller's buffers in batch order.  A round
// without requests runs the path of the call without replies.
#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "patrolhip.h"
#include "phip_host.hpp"

namespace {

typedef uint64_t u64;
typedef unsigned int u32;

// A device buffer that only grows.
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      if (e != hipSuccess) return e;
    }
    const size_t want = std::max(bytes, cap * 3 / 2) + 64;   // +64: 8-byte over-read slack
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Messages per pipelined chunk.  The send sets' name space is sized from the
// chunks' real name bytes (the batch's offsets at the chunk boundaries, one
// small read per call), so a name of any length fits and a set holds no more
// than its largest chunk needs.
constexpr uint32_t kChunk = 1u << 24;
constexpr uint32_t kSmallChunk = 1u << 12;   // PHIP_GROUP_SMALL_CHUNKS

// One travelling column: its entry's size, whether a segment of it is
// addressed by message (Seg's so/sc, ro/rc) or by name byte (sb/sbytes,
// rb/rbytes), an entry on the wire (`per` elements of `type`) and the bytes
// its buffer keeps past the last entry (the kernels' over-read slack).
struct Col {
  u32 elem;
  bool by_bytes;
  ncclDataType_t type;
  u32 per;
  u32 slack;
};
constexpr u32 kMaxCols = 7;
struct Cols {
  u32 n;
  Col c[kMaxCols];
};
constexpr Col kLens = {4, false, ncclUint32, 1, 4}, kNames = {1, true, ncclUint8, 1, 64},
              kByte = {1, false, ncclUint8, 1, 8}, kWord = {8, false, ncclUint64, 1, 8},
              kReply = {sizeof(phip_state), false, ncclUint64, sizeof(phip_state) / 8, 0};
// The three column sets that travel, and their columns' places in a ColSet:
// messages (phip_route_pack's send columns), ops (phip_route_pack_ops'; the
// three operand words serve both kinds) and the results of applied ops.
constexpr Cols kMsgCols = {5, {kLens, kNames, kWord, kWord, kWord}};
constexpr Cols kOpCols = {7, {kLens, kNames, kByte, kWord, kWord, kWord, kWord}};
constexpr Cols kResCols = {4, {kByte, kWord, kWord, kReply}};
// phip_group_peek's: a query is an op without its kind byte, an answer is
// status, remaining, have and retry_at (25 bytes), and the state evaluated
// behind them under PHIP_GROUP_PEEK_STATE.
constexpr Cols kQryCols = {6, {kLens, kNames, kWord, kWord, kWord, kWord}};
constexpr Cols kPeekCols = {4, {kByte, kWord, kWord, kWord}};
constexpr Cols kPeekStateCols = {5, {kByte, kWord, kWord, kWord, kReply}};
// The answers to a round's incast requests on their way back (the *_replies
// forms): every datagram's length, the datagrams' bytes back to back (a
// segment of them is addressed by byte, as names are) and the request's
// position in the segment its source sent.
constexpr Cols kBackCols = {3, {kLens, kNames, kLens}};
enum { C_LENS, C_NAMES, MSG_A, MSG_T, MSG_E };
enum { O_KIND = C_NAMES + 1, O_NOW, O_X0, O_X1, O_X2 };
enum { R_STATUS, R_REM, R_HAVE, R_REPLY };
enum { Q_NOW = C_NAMES + 1, Q_X0, Q_X1, Q_X2 };
enum { P_STATUS, P_REM, P_HAVE, P_AT, P_STATE };
enum { B_LENS, B_BYTES, B_POS };

// The buffers of one column set, sized and moved by its table.
struct ColSet {
  const Cols* cols;
  Buf b[kMaxCols];
  explicit ColSet(const Cols& c) : cols(&c) {}
  // Room for n entries and nb name bytes, and never less than one entry (RCCL
  // is handed every column's pointer, also for an empty segment).
  hipError_t ensure(u64 n, u64 nb) {
    for (u32 i = 0; i < cols->n; ++i) {
      const Col& c = cols->c[i];
      hipError_t e = b[i].ensure(std::max<u64>((c.by_bytes ? nb : n) * c.elem + c.slack, c.elem));
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void release() {
    for (Buf& x : b) x.release();
  }
  template <class T>
  T* at(u32 i) const { return (T*)b[i].p; }
};

// One chunk's split sizes: dev (device) and host (pinned) hold [6 * world] u64:
//   send counts | send name bytes | send chunk totals | recv counts | recv name bytes | recv chunk totals
// (the chunk totals: every member's chunk count K, so that all members run
// the same number of exchange rounds).  A chunk total's low half is K; its
// high half is the number of zero-state messages the member's chunk holds
// (the *_replies forms count them; 0 otherwise), so that every member knows
// from exchanged values alone whether the round has requests to answer.
constexpr u64 kRoundMask = 0xFFFFFFFFull;
struct Sizes {
  Buf dev;
  uint64_t* host = nullptr;
};

// Receive's pipeline state for the chunks of one parity (chunk k uses lane
// k & 1 and the member's sizes k & 1): the chunk's send buffers (owner-major,
// phip_route_pack's layout) and its received segments (sources in rank
// order), merged while the next chunk travels.
struct Lane {
  ColSet send{kMsgCols}, recv{kMsgCols};
  Buf offs;                       // the received names' offsets
  hipEvent_t ev_pack = nullptr, ev_sz = nullptr, ev_x = nullptr;
  bool x_pending = false;         // ev_x recorded for an exchange reading `send`
  u64 n = 0;                      // messages received into `recv`
  hipEvent_t ev_recv = nullptr;   // its exchange (exchange stream)
  hipEvent_t ev_merged = nullptr; // its merge (handle stream)
  bool merge_pending = false;     // ev_merged recorded for a merge reading `recv`
  bool to_merge = false;          // `recv` holds a chunk no merge was queued for yet
  // The *_replies forms: where every packed message of the chunk stood in it
  // (send position -> chunk index), and the owner's answers to the chunk's
  // requests as phip_receive_soa_replies writes them (their datagrams into
  // rsend's byte column), split by source for the way back.
  Buf src, roffs, rsrc;
  ColSet rsend{kBackCols};
};

// One member's part of a *_replies call: the caller's buffers and how far
// they are filled (the rounds append), and phip_group_reply_stats' words.
struct Replies {
  phip_reply_egress* rq = nullptr;
  u64 budget = 0;
  u64 n = 0, bytes = 0, replies = 0, skipped = 0;
  bool cut = false;               // a round did not fit: later rounds only count
};
enum { RS_ROUNDS, RS_RETURNS, RS_BOUND, RS_WRITTEN, RS_WORDS };

// Segment boundaries by peer, as a kernel argument (world <= 64).
struct SegBounds {
  u32 at[65];
};

// Busy spans of one group call per stage (0 pack, 1 exchange, 2 merge):
// event pairs recorded around each chunk's work on the stream it runs on,
// summed after the call (phip_group_stage_ms).
struct StageTimer {
  std::vector<hipEvent_t> ev[3];   // pairs per stage: [2k] start, [2k+1] end
  size_t used[3] = {0, 0, 0};
  bool on = false;
  void reset() { used[0] = used[1] = used[2] = 0; }
  hipError_t mark(int s, hipStream_t st) {
    if (!on) return hipSuccess;
    if (used[s] == ev[s].size()) {
      hipEvent_t e;
      hipError_t r = hipEventCreate(&e);
      if (r != hipSuccess) return r;
      ev[s].push_back(e);
    }
    return hipEventRecord(ev[s][used[s]++], st);
  }
  hipError_t sum(int s, float* ms) {
    *ms = 0;
    for (size_t k = 0; k + 1 < used[s]; k += 2) {
      float x = 0;
      hipError_t r = hipEventSynchronize(ev[s][k + 1]);
      if (r == hipSuccess) r = hipEventElapsedTime(&x, ev[s][k], ev[s][k + 1]);
      if (r != hipSuccess) return r;
      *ms += x;
    }
    return hipSuccess;
  }
  void release() {
    for (auto& v : ev)
      for (hipEvent_t e : v) (void)hipEventDestroy(e);
    for (auto& v : ev) v.clear();
  }
};

constexpr u32 kOpsSizes = 2;   // Member::sz of the ops path (0, 1: Receive's lanes)
constexpr u32 kBackSizes = 3;  // ... and of the answers' way back (the *_replies forms)

struct Member {
  phip_handle* h = nullptr;
  bool own = false;            // opened by the group (phip_group_open_all)
  int device = 0;
  u32 rank = 0;
  ncclComm_t comm = nullptr;
  hipStream_t sp = nullptr, sx = nullptr;   // pack stream, exchange stream
  hipEvent_t ev_done = nullptr;             // the call's last exchange
  Lane lane[2];
  // phip_group_apply_mixed's per-round buffers, apart from Receive's lanes
  // (its path touches none of them).  One round's ops packed owner-major
  // (osrc, their places in the batch, stays here: it is the results' way
  // back) and as the owner received them (sources in rank order, ooffs their
  // names' offsets); the results of applying them, in that order, and the
  // results the owners returned to this source, in send order.
  ColSet osend{kOpCols}, orecv{kOpCols}, ores{kResCols}, oback{kResCols};
  Buf osrc, ooffs;
  // phip_group_peek's, in the same roles (osrc, ooffs and the ops path's split
  // sizes serve both: a group runs one call at a time).  pres / pback take the
  // call's answer columns, with or without the state (PeekPath::begin).
  ColSet qsend{kQryCols}, qrecv{kQryCols}, pres{kPeekCols}, pback{kPeekCols};
  Sizes sz[4];
  Buf scan_tmp, ae, bounds;
  // The *_replies forms, source side: the answers the owners returned (owners
  // in rank order), the sort by batch index and the gather's scratch; the
  // ring form's device copies of the caller's host buffers; the last call's
  // phip_group_reply_stats.
  ColSet rback{kBackCols};
  Buf gkey_in, gval_in, gkey, gval, gaoff, gslen, gsend, gctr;
  Buf ring_out, ring_offs, ring_src;
  hipEvent_t ev_rep = nullptr;
  u64 rstats[RS_WORDS] = {0, 0, 0, 0};
  u64* host_k = nullptr;       // pinned [world]: this member's chunk count, to every peer
  u64 k_local = 0;             // (shared-device groups read each other's)
  StageTimer tm;
  std::string err;
};

}  // namespace

// A reusable barrier of the member threads of one call (shared-device
// exchange).  abort() releases every waiter with false: a member that fails
// before a barrier must not leave the others waiting.
struct Barrier {
  std::mutex mu;
  std::condition_variable cv;
  u32 n = 0, count = 0, gen = 0;
  bool aborted = false;
  bool wait() {
    std::unique_lock<std::mutex> l(mu);
    if (aborted) return false;
    const u32 g0 = gen;
    if (++count == n) {
      count = 0;
      ++gen;
      cv.notify_all();
      return true;
    }
    cv.wait(l, [&] { return gen != g0 || aborted; });
    return !aborted;
  }
  void abort() {
    std::lock_guard<std::mutex> l(mu);
    aborted = true;
    cv.notify_all();
  }
  void reset(u32 members) {
    std::lock_guard<std::mutex> l(mu);
    n = members;
    count = 0;
    aborted = false;
  }
};

struct phip_group {
  u32 world = 0;
  std::vector<Member> m;
  std::string err;
  bool shared = false;   // every member on one device: exchange by device copies (no RCCL)
  Barrier bar;
};

namespace {

int fail(Member& mb, int code, const char* fmt, ...) {
  char tmp[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(tmp, sizeof tmp, fmt, ap);
  va_end(ap);
  mb.err = tmp;
  return code;
}

#define GHIP(mb, x)                                                                        \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess)                                                                  \
      return fail((mb), PHIP_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                               \
  } while (0)

#define GNCCL(mb, x)                                                                        \
  do {                                                                                      \
    ncclResult_t r_ = (x);                                                                  \
    if (r_ != ncclSuccess)                                                                  \
      return fail((mb), PHIP_ERR_RCCL, "%s: %s (%s:%d)", #x, ncclGetErrorString(r_), __FILE__, \
                  __LINE__);                                                                \
  } while (0)

#define GPHIP(mb, x)                                                                   \
  do {                                                                                 \
    int rc_ = (x);                                                                     \
    if (rc_ != PHIP_OK)                                                                \
      return fail((mb), rc_, "%s: %s", #x, phip_last_error((mb).h));                    \
  } while (0)

// Run f(member index) on one host thread per local member (the calling
// thread when there is one); returns the first member's error.  A member
// that fails releases the others from the call's barriers.
template <class F>
int for_members(phip_group* g, F f) {
  const size_t n = g->m.size();
  std::vector<int> rc(n, PHIP_OK);
  g->bar.reset((u32)n);
  if (n == 1) {
    rc[0] = f(0);
  } else {
    std::vector<std::thread> th;
    th.reserve(n);
    for (size_t i = 0; i < n; ++i)
      th.emplace_back([&, i] {
        rc[i] = f(i);
        if (rc[i] != PHIP_OK) g->bar.abort();
      });
    for (auto& t : th) t.join();
  }
  for (size_t i = 0; i < n; ++i)
    if (rc[i] != PHIP_OK) {
      g->err = "member " + std::to_string(i) + ": " + g->m[i].err;
      return rc[i];
    }
  g->err.clear();
  return PHIP_OK;
}

// The exchange plan of one chunk of one member, shared by the RCCL and the
// shared-device paths: with hs = the chunk's split sizes (Sizes::host),
// peer p's entry gives
//   send side: where the member's packed segment for owner p lies in its
//              owner-major send buffers (so messages / sb name bytes in) and
//              its size (sc, sbytes);
//   recv side: where the segment source p sends this member lands in the
//              chunk's part of the receive buffers (ro / rb: sources in rank
//              order) and its size (rc, rbytes).
struct Seg {
  u64 so, sb, sc, sbytes;
  u64 ro, rb, rc, rbytes;
};
void segment_plan(const u64* hs, u32 W, std::vector<Seg>* plan) {
  plan->resize(W);
  u64 so = 0, sb = 0, ro = 0, rb = 0;
  for (u32 p = 0; p < W; ++p) {
    Seg& g = (*plan)[p];
    g.so = so; g.sb = sb; g.sc = hs[p]; g.sbytes = hs[W + p];
    g.ro = ro; g.rb = rb; g.rc = hs[3 * W + p]; g.rbytes = hs[4 * W + p];
    so += g.sc; sb += g.sbytes; ro += g.rc; rb += g.rbytes;
  }
}

// The plan with its roles swapped: the way back of what the plan brought
// (each owner returns to source p what p sent it, to where p sent it from).
Seg swapped(const Seg& s) { return Seg{s.ro, s.rb, s.rc, s.rbytes, s.so, s.sb, s.sc, s.sbytes}; }

// Segment p of one side of another member's sizes alone (side = its host
// block at 0: where its segment for owner p lies in its send buffers; at
// 3 * W: where source p's segment lies in its receive buffers), as a send
// side: what a shared-device peer reads of that member's sizes.
Seg seg_at(const u64* side, u32 W, u32 p) {
  Seg g{};
  for (u32 q = 0; q < p; ++q) {
    g.so += side[q];
    g.sb += side[W + q];
  }
  g.sc = side[p];
  g.sbytes = side[W + p];
  return g;
}

// A shared-device peer's part in a move: the set this member copies from and
// where its segment lies in it.
struct Peer {
  const ColSet* from;
  Seg at;
};
template <class F>
std::vector<Peer> peers_of(const phip_group* g, const Member& mb, u32 si, u32 side, F set) {
  std::vector<Peer> v;
  if (g->shared)
    for (const Member& m : g->m)
      v.push_back({&set(m), seg_at(m.sz[si].host + side, g->world, mb.rank)});
  return v;
}

// The part of a segment a column covers: by message or by name byte.
struct Span {
  u64 off, cnt;
};
Span send_span(const Col& c, const Seg& s) {
  return c.by_bytes ? Span{s.sb, s.sbytes} : Span{s.so, s.sc};
}
Span recv_span(const Col& c, const Seg& s) {
  return c.by_bytes ? Span{s.rb, s.rbytes} : Span{s.ro, s.rc};
}

// Moves a column set along a plan on stream st: for every peer p, the send
// side of plan[p] out of `from` to p, and p's segment into the receive side
// of plan[p] in `to`; one send and one receive per peer and column, this
// member's own segment a device copy unless rccl_self.  In a shared-device
// group (no RCCL) the member copies every segment out of its peers' sets
// instead, after a barrier that the caller keeps.
int move_segments(phip_group* g, Member& mb, const std::vector<Seg>& plan, const ColSet& from,
                  ColSet& to, hipStream_t st, bool rccl_self, const std::vector<Peer>& peers) {
  const u32 W = g->world;
  const Cols& cols = *to.cols;
  if (from.cols != to.cols) return fail(mb, PHIP_ERR_INVALID, "internal: column sets differ");
  auto copy = [&](const ColSet& src, const Seg& s, const Seg& d) -> int {
    for (u32 i = 0; i < cols.n; ++i) {
      const Col& c = cols.c[i];
      const Span f = send_span(c, s), t = recv_span(c, d);
      if (t.cnt)
        GHIP(mb, hipMemcpyAsync(to.at<uint8_t>(i) + t.off * c.elem, src.at<uint8_t>(i) + f.off * c.elem,
                                t.cnt * c.elem, hipMemcpyDeviceToDevice, st));
    }
    return PHIP_OK;
  };
  int rc;
  if (g->shared) {
    for (u32 p = 0; p < W; ++p) {
      const Seg& s = peers[p].at;   // the source's send side
      if (s.sc != plan[p].rc || s.sbytes != plan[p].rbytes)
        return fail(mb, PHIP_ERR_INVALID, "internal: member %u sends %llu/%llu, %u expects %llu/%llu",
                    p, (unsigned long long)s.sc, (unsigned long long)s.sbytes, mb.rank,
                    (unsigned long long)plan[p].rc, (unsigned long long)plan[p].rbytes);
      if ((rc = copy(*peers[p].from, s, plan[p]))) return rc;
    }
    return PHIP_OK;
  }
  const Seg& own = plan[mb.rank];
  if (own.sc != own.rc || own.sbytes != own.rbytes)
    return fail(mb, PHIP_ERR_INVALID, "internal: own segment %llu/%llu vs %llu/%llu",
                (unsigned long long)own.sc, (unsigned long long)own.sbytes,
                (unsigned long long)own.rc, (unsigned long long)own.rbytes);
  if (!rccl_self && (rc = copy(from, own, own))) return rc;
  GNCCL(mb, ncclGroupStart());
  for (u32 p = 0; p < W; ++p) {
    if (p == mb.rank && !rccl_self) continue;
    for (u32 i = 0; i < cols.n; ++i) {
      const Col& c = cols.c[i];
      const Span f = send_span(c, plan[p]), t = recv_span(c, plan[p]);
      GNCCL(mb, ncclSend(from.at<uint8_t>(i) + f.off * c.elem, f.cnt * c.per, c.type, p, mb.comm, st));
      GNCCL(mb, ncclRecv(to.at<uint8_t>(i) + t.off * c.elem, t.cnt * c.per, c.type, p, mb.comm, st));
    }
  }
  GNCCL(mb, ncclGroupEnd());
  return PHIP_OK;
}

// A chunk's split sizes (stage 1) on stream st: every member learns what each
// source sends it (RCCL; shared-device groups read each other's after a
// barrier, adopt_sizes), and the block goes to its pinned mirror.
int exchange_sizes(phip_group* g, Member& mb, Sizes& s, hipStream_t st) {
  const u32 W = g->world;
  u64* sz = (u64*)s.dev.p;
  GHIP(mb, mb.tm.mark(1, st));
  if (!g->shared) {
    GNCCL(mb, ncclGroupStart());
    GNCCL(mb, ncclAllToAll(sz, sz + 3 * W, 1, ncclUint64, mb.comm, st));
    GNCCL(mb, ncclAllToAll(sz + W, sz + 4 * W, 1, ncclUint64, mb.comm, st));
    GNCCL(mb, ncclAllToAll(sz + 2 * W, sz + 5 * W, 1, ncclUint64, mb.comm, st));
    GNCCL(mb, ncclGroupEnd());
  }
  GHIP(mb, hipMemcpyAsync(s.host, sz, 6 * W * sizeof(u64), hipMemcpyDeviceToHost, st));
  GHIP(mb, mb.tm.mark(1, st));
  return PHIP_OK;
}

// Once sizes si are in the member's pinned mirror: a shared-device member
// waits until every member's are and takes what member p packed for it from
// p's.  The first chunk's totals give the call's round count *K: every member
// runs max(K) rounds (a shorter batch sends empty chunks).
int adopt_sizes(phip_group* g, Member& mb, u32 si, bool first, u64* K) {
  const u32 W = g->world;
  u64* hs = mb.sz[si].host;
  if (g->shared) {
    if (!g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
    for (u32 p = 0; p < W; ++p) {
      const u64* ps = g->m[p].sz[si].host;
      hs[3 * W + p] = ps[mb.rank];
      hs[4 * W + p] = ps[W + mb.rank];
      hs[5 * W + p] = g->m[p].k_local | (ps[2 * W + mb.rank] & ~kRoundMask);
    }
  }
  if (first) {
    for (u32 p = 0; p < W; ++p) *K = std::max<u64>(*K, hs[5 * W + p] & kRoundMask);
    *K = std::max<u64>(*K, 1);
  }
  return PHIP_OK;
}

// The zero-state messages source p holds in this round (the *_replies forms;
// 0 from every other call): the chunk total's high half.
u64 zero_states_of(const u64* hs, u32 W, u32 p) { return hs[5 * W + p] >> 32; }

// What one round sends and receives; a receive side past 2^32 is refused.
struct Totals {
  u64 c_send = 0, c_recv = 0, b_recv = 0;
};
int round_totals(Member& mb, const std::vector<Seg>& plan, const char* round, const char* items,
                 Totals* t) {
  *t = Totals{};
  for (const Seg& s : plan) {
    t->c_send += s.sc;
    t->c_recv += s.rc;
    t->b_recv += s.rbytes;
  }
  if (t->c_recv > 0xFFFFFFFFull || t->b_recv > 0xFFFFFFFFull)
    return fail(mb, PHIP_ERR_INVALID, "routed %s of %llu %s / %llu name bytes exceeds 2^32", round,
                (unsigned long long)t->c_recv, items, (unsigned long long)t->b_recv);
  return PHIP_OK;
}

// name_offs at the chunk boundaries: out[k] = offs[min(k * chunk, n)] (T =
// u64: a wire batch's datagram offsets).
template <class T>
__global__ void k_chunk_bounds(const T* __restrict__ offs, u32 n, u64 chunk, u64 kc,
                               T* __restrict__ out) {
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= kc) out[k] = offs[k * chunk < n ? k * chunk : n];
}

// A batch of n entries in rounds of `chunk`: the member's round count, where
// the split sizes carry it to the peers, and the name offsets at the round
// boundaries ((*bnd)[k + 1] - (*bnd)[k]: the name bytes of round k), read
// back on stream st, which it synchronises.
template <class T>
int chunk_bounds(phip_group* g, Member& mb, hipStream_t st, const T* offs, u32 n, u64 chunk,
                 std::vector<T>* bnd) {
  const u64 kc = ((u64)n + chunk - 1) / chunk;
  mb.k_local = kc;
  for (u32 p = 0; p < g->world; ++p) mb.host_k[p] = kc;
  bnd->assign(kc + 1, 0);
  if (n == 0) return PHIP_OK;
  GHIP(mb, mb.bounds.ensure((kc + 1) * sizeof(T)));
  k_chunk_bounds<T><<<(unsigned)((kc + 1 + 255) / 256), 256, 0, st>>>(offs, n, chunk, kc,
                                                                      (T*)mb.bounds.p);
  GHIP(mb, hipGetLastError());
  GHIP(mb, hipMemcpyAsync(bnd->data(), mb.bounds.p, (kc + 1) * sizeof(T), hipMemcpyDeviceToHost, st));
  GHIP(mb, hipStreamSynchronize(st));
  return PHIP_OK;
}

// Name offsets of n received entries from their lengths: offs[0] = 0 and an
// inclusive scan into offs[1..n], on stream st.
int offsets_from_lens(Member& mb, const u32* lens, u64 n, u32* offs, hipStream_t st) {
  GHIP(mb, hipMemsetAsync(offs, 0, sizeof(u32), st));
  size_t tb = 0;
  GHIP(mb, rocprim::inclusive_scan(nullptr, tb, lens, offs + 1, (size_t)n, rocprim::plus<u32>(), st));
  GHIP(mb, mb.scan_tmp.ensure(tb));
  GHIP(mb, rocprim::inclusive_scan(mb.scan_tmp.p, tb, lens, offs + 1, (size_t)n,
                                   rocprim::plus<u32>(), st));
  return PHIP_OK;
}

// The owner's merge of one received chunk (lengths, packed names, states):
// the names' offsets, then phip_receive_soa (sources in rank order, each in
// its order), on the handle's stream behind the chunk's exchange.
int merge_chunk(Member& mb, Lane& ln, hipStream_t st, int64_t now) {
  ln.to_merge = false;
  if (ln.n) {
    GHIP(mb, hipStreamWaitEvent(st, ln.ev_recv, 0));
    GHIP(mb, mb.tm.mark(2, st));
    GHIP(mb, ln.offs.ensure(ln.n * 4 + 8));
    int rc;
    if ((rc = offsets_from_lens(mb, ln.recv.at<u32>(C_LENS), ln.n, (u32*)ln.offs.p, st))) return rc;
    phip_msgs rm{};
    rm.n = (u32)ln.n;
    rm.names = ln.recv.at<uint8_t>(C_NAMES);
    rm.name_offs = (const u32*)ln.offs.p;
    rm.added = ln.recv.at<u64>(MSG_A);
    rm.taken = ln.recv.at<u64>(MSG_T);
    rm.elapsed = ln.recv.at<int64_t>(MSG_E);
    GPHIP(mb, phip_receive_soa(mb.h, &rm, now, nullptr, PHIP_DEVICE_PTRS | PHIP_RECV_CLASSIFY));
    GHIP(mb, mb.tm.mark(2, st));
  }
  GHIP(mb, hipEventRecord(ln.ev_merged, st));
  ln.merge_pending = true;
  return PHIP_OK;
}

// Chunk k of a batch: messages [k * chunk, ...) (empty past the batch).
phip_msgs chunk_of(const phip_msgs& in, u64 chunk, u64 k) {
  phip_msgs c = in;
  const u64 lo = k * chunk;
  c.n = lo < in.n ? (u32)std::min<u64>(chunk, in.n - lo) : 0u;
  if (c.n) {
    c.name_offs = in.name_offs + lo;   // absolute offsets into the same blob
    c.added = in.added + lo;
    c.taken = in.taken + lo;
    c.elapsed = in.elapsed + lo;
  }
  return c;
}

// What member_receive asks of a member's batch, decoded (MsgBatch) or raw
// datagrams (WireBatch): its length, the merge of the whole of it where there
// is nothing to route, its chunks' name bytes (bounds synchronises st and
// sets the member's round count), the combine's directory and the pack of
// chunk k into a send set.
struct MsgBatch {
  const phip_msgs& in;
  std::vector<u32> bnd;   // name_offs at the chunk boundaries
  u32 n() const { return in.n; }
  int whole(Member& mb, int64_t now) {
    GPHIP(mb, phip_receive_soa(mb.h, &in, now, nullptr, PHIP_DEVICE_PTRS | PHIP_RECV_CLASSIFY));
    return PHIP_OK;
  }
  int bounds(phip_group* g, Member& mb, hipStream_t st, u64 chunk) {
    return chunk_bounds(g, mb, st, in.name_offs, in.n, chunk, &bnd);
  }
  u64 chunk_bytes(u64, u64 k) const { return (u64)(bnd[k + 1] - bnd[k]); }
  int dir(Member& mb, u32 W, const void** d) { return phip_host::route_dir(mb.h, mb.sp, &in, W, d); }
  int pack(Member& mb, u64 chunk, u64 k, u32 W, const void* d, const ColSet& ss, u64* sz, u32* src) {
    const phip_msgs c = chunk_of(in, chunk, k);
    return phip_host::route_pack(mb.h, mb.sp, &c, W, d, ss.at<uint8_t>(C_NAMES), ss.at<uint32_t>(C_LENS),
                                 ss.at<uint64_t>(MSG_A), ss.at<uint64_t>(MSG_T), ss.at<int64_t>(MSG_E), sz,
                                 sz + W, src);
  }
  // the *_replies forms: chunk k's zero-state count into the chunk totals,
  // and the whole batch with its answers where there is nothing to route
  int count_zero(Member& mb, u64 chunk, u64 k, u32 W, u64* totals) {
    const phip_msgs c = chunk_of(in, chunk, k);
    return phip_host::count_zero(mb.h, mb.sp, &c, W, totals);
  }
  int whole_replies(Member& mb, int64_t now, phip_reply_egress* rq) {
    GPHIP(mb, phip_receive_soa_replies(mb.h, &in, now, nullptr, rq, PHIP_DEVICE_PTRS | PHIP_RECV_CLASSIFY));
    return PHIP_OK;
  }
};

// A wire batch cut at its stop: in.n datagrams, every one well formed (the
// pre-pass of phip_group_receive_datagrams ran before).
struct WireBatch {
  phip_wire in;
  std::vector<u64> bnd;   // the datagram offsets at the chunk boundaries
  u32 n() const { return in.n; }
  // one owner: the handle's own wire path reads the datagrams in place
  int whole(Member& mb, int64_t now) {
    GPHIP(mb, phip_receive_datagrams(mb.h, in.bytes, in.offs, in.n, now, nullptr, nullptr,
                                     PHIP_DEVICE_PTRS));
    return PHIP_OK;
  }
  int bounds(phip_group* g, Member& mb, hipStream_t st, u64 chunk) {
    return chunk_bounds(g, mb, st, in.offs, in.n, chunk, &bnd);
  }
  // the sum of size - 25 over the chunk: its name bytes and any trailing ones
  u64 chunk_bytes(u64 chunk, u64 k) const {
    const u64 cnt = std::min<u64>(chunk, in.n - k * chunk);
    return bnd[k + 1] - bnd[k] - cnt * PHIP_BUCKET_FIXED_SIZE;
  }
  int dir(Member& mb, u32 W, const void** d) { return phip_host::route_dir_wire(mb.h, mb.sp, &in, W, d); }
  phip_wire chunk_of(u64 chunk, u64 k) const {
    phip_wire c = in;
    const u64 lo = k * chunk;
    c.n = lo < in.n ? (u32)std::min<u64>(chunk, in.n - lo) : 0u;
    if (c.n) c.offs = in.offs + lo;   // absolute offsets into the same bytes
    return c;
  }
  int pack(Member& mb, u64 chunk, u64 k, u32 W, const void* d, const ColSet& ss, u64* sz, u32* src) {
    const phip_wire c = chunk_of(chunk, k);
    return phip_host::route_pack_wire(mb.h, mb.sp, &c, W, d, ss.at<uint8_t>(C_NAMES),
                                      ss.at<uint32_t>(C_LENS), ss.at<uint64_t>(MSG_A),
                                      ss.at<uint64_t>(MSG_T), ss.at<int64_t>(MSG_E), sz, sz + W, src);
  }
  // (as MsgBatch's: the three header words of every datagram of the chunk)
  int count_zero(Member& mb, u64 chunk, u64 k, u32 W, u64* totals) {
    const phip_wire c = chunk_of(chunk, k);
    return phip_host::count_zero_wire(mb.h, mb.sp, &c, W, totals);
  }
  int whole_replies(Member& mb, int64_t now, phip_reply_egress* rq) {
    GPHIP(mb, phip_receive_datagrams_replies(mb.h, in.bytes, in.offs, in.n, now, nullptr, nullptr, rq,
                                             PHIP_DEVICE_PTRS));
    return PHIP_OK;
  }
};

// ---- the answers of a round with incast requests (the *_replies forms) ----
// The peer whose segment [at[p], at[p + 1]) holds entry x (empty segments are
// passed over).
__device__ inline u32 seg_of(const SegBounds& b, u32 W, u32 x) {
  u32 p = 0;
  while (p + 1 < W && x >= b.at[p + 1]) ++p;
  return p;
}

// Owner: the chunk's n answers (src: the request's place in the received
// chunk, sources in rank order, so the list is grouped by source already;
// offs: the datagrams' offsets) split at the received segments' boundaries
// `at`: every answer's length and its request's position within its source's
// segment, and per source the answers and their bytes, the way back's split
// sizes.
__global__ void k_reply_split(const u32* __restrict__ src, const u64* __restrict__ offs, u32 n,
                              SegBounds at, u32 W, u32* __restrict__ lens, u32* __restrict__ pos,
                              unsigned long long* __restrict__ counts,
                              unsigned long long* __restrict__ bytes) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const u32 x = src[k], p = seg_of(at, W, x);
  const u32 len = (u32)(offs[k + 1] - offs[k]);
  lens[k] = len;
  pos[k] = x - at.at[p];
  atomicAdd(&counts[p], 1ull);
  atomicAdd(&bytes[p], (unsigned long long)len);
}

// Source: returned answer j (owners in rank order, `from` their segments'
// boundaries) answers the message this member packed at position pos[j] of
// its send segment for that owner (starting at so.at[owner]); send_src turns
// the send position into the chunk index, base the chunk's first batch index.
__global__ void k_back_keys(const u32* __restrict__ pos, u32 n, SegBounds from, SegBounds so, u32 W,
                            const u32* __restrict__ send_src, u32 base, u32* __restrict__ keys,
                            u32* __restrict__ vals) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u32 p = seg_of(from, W, j);
  keys[j] = base + send_src[so.at[p] + pos[j]];
  vals[j] = j;
}

__global__ void k_gather_lens(const u32* __restrict__ vals, const u32* __restrict__ lens, u32 n,
                              u64* __restrict__ out) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = lens[vals[k]];
}

// Source: the round's answers in batch order (answer k of the round: returned
// answer vals[k], for batch index keys[k], its bytes at aoff[.] of the
// returned bytes, ending at end[k] of the round's output) appended behind
// the n0 datagrams / b0 bytes the rounds before wrote, as far as max_msgs and
// the byte budget allow (a prefix: end[] grows).  One wave a datagram: a
// byte run of any length and alignment, byte by byte.  ctr[0]: datagrams
// written, ctr[1]: the output's end.
__global__ __launch_bounds__(256) void k_reply_gather(
    const u32* __restrict__ vals, const u32* __restrict__ keys, const u32* __restrict__ lens,
    const u32* __restrict__ aoff, const u64* __restrict__ end, u32 n, const uint8_t* __restrict__ in,
    u64 n0, u64 b0, u64 max_msgs, u64 budget, uint8_t* __restrict__ out, u64* __restrict__ offs,
    u32* __restrict__ src, unsigned long long* __restrict__ ctr) {
  const u32 k = (blockIdx.x * blockDim.x + threadIdx.x) / 64, lane = threadIdx.x & 63;
  if (k >= n) return;
  const u64 e = b0 + end[k];
  if (n0 + k >= max_msgs || e > budget) return;
  const u32 j = vals[k], len = lens[j];
  const uint8_t* from = in + aoff[j];
  uint8_t* to = out + (e - len);
  for (u32 x = lane; x < len; x += 64) to[x] = from[x];
  if (lane == 0) {
    offs[n0 + k + 1] = e;
    if (src) src[n0 + k] = keys[k];
    atomicMax(&ctr[0], (unsigned long long)k + 1);
    atomicMax(&ctr[1], (unsigned long long)e);
  }
}

// Round k of a *_replies call in which some member holds a zero-state message
// (every member takes this path: the decision comes from exchanged values).
// The owner merges its received chunk with phip_receive_soa_replies into
// lane-owned buffers sized from `bound` (the requests it can have received),
// splits the answers by source and returns them: the per-source counts as
// split sizes, then lengths, bytes and positions along that plan on the
// exchange stream (RCCL calls stay in one order: behind this round's exchange,
// before the next round's sizes).  The source sorts what came back by batch
// index and appends what fits to the caller's buffers.  The round is finished
// when this returns.
int reply_round(phip_group* g, Member& mb, u32 si, u64 k, u64 chunk, const std::vector<Seg>& plan,
                u64 bound, int64_t now, bool rccl_self, Replies& rp, hipStream_t st) {
  const u32 W = g->world;
  Lane& ln = mb.lane[si];
  Sizes& zs = mb.sz[kBackSizes];
  int rc;
  GHIP(mb, zs.dev.ensure((size_t)6 * W * 8));
  u64* sz = (u64*)zs.dev.p;
  GHIP(mb, ln.rsend.ensure(bound, bound ? bound * PHIP_BUCKET_PACKET_SIZE + 8 : 0));
  GHIP(mb, hipMemsetAsync(sz, 0, (size_t)6 * W * 8, st));
  u64 wrote = 0;
  if (ln.n && bound) {
    ln.to_merge = false;
    GHIP(mb, hipStreamWaitEvent(st, ln.ev_recv, 0));
    GHIP(mb, mb.tm.mark(2, st));
    GHIP(mb, ln.offs.ensure(ln.n * 4 + 8));
    GHIP(mb, ln.roffs.ensure((bound + 1) * 8));
    GHIP(mb, ln.rsrc.ensure(bound * 4));
    if ((rc = offsets_from_lens(mb, ln.recv.at<u32>(C_LENS), ln.n, (u32*)ln.offs.p, st))) return rc;
    phip_msgs rm{};
    rm.n = (u32)ln.n;
    rm.names = ln.recv.at<uint8_t>(C_NAMES);
    rm.name_offs = (const u32*)ln.offs.p;
    rm.added = ln.recv.at<u64>(MSG_A);
    rm.taken = ln.recv.at<u64>(MSG_T);
    rm.elapsed = ln.recv.at<int64_t>(MSG_E);
    phip_reply_egress q{};
    q.out = ln.rsend.at<uint8_t>(B_BYTES);
    q.out_cap = bound * PHIP_BUCKET_PACKET_SIZE + 8;
    q.offs = (u64*)ln.roffs.p;
    q.src = (u32*)ln.rsrc.p;
    q.max_msgs = (u32)bound;
    GPHIP(mb, phip_receive_soa_replies(mb.h, &rm, now, nullptr, &q, PHIP_DEVICE_PTRS | PHIP_RECV_CLASSIFY));
    if ((u64)q.n + q.skipped != q.replies)
      return fail(mb, PHIP_ERR_INVALID, "internal: %u answers for a bound of %llu requests", q.replies,
                  (unsigned long long)bound);
    wrote = q.n;
    rp.skipped += q.skipped;
    if (wrote) {
      SegBounds at{};
      for (u32 p = 0; p < W; ++p) at.at[p] = (u32)plan[p].ro;
      k_reply_split<<<(unsigned)((wrote + 255) / 256), 256, 0, st>>>(
          q.src, q.offs, (u32)wrote, at, W, ln.rsend.at<u32>(B_LENS), ln.rsend.at<u32>(B_POS),
          (unsigned long long*)sz, (unsigned long long*)(sz + W));
      GHIP(mb, hipGetLastError());
    }
    GHIP(mb, mb.tm.mark(2, st));
    GHIP(mb, hipEventRecord(ln.ev_merged, st));
    ln.merge_pending = true;
  } else if ((rc = merge_chunk(mb, ln, st, now))) {
    return rc;
  }
  mb.rstats[RS_RETURNS] += 1;
  mb.rstats[RS_BOUND] += bound;
  mb.rstats[RS_WRITTEN] += wrote;
  // the way back: its split sizes behind the owner's split, then the segments
  GHIP(mb, hipEventRecord(mb.ev_rep, st));
  GHIP(mb, hipStreamWaitEvent(mb.sx, mb.ev_rep, 0));
  if ((rc = exchange_sizes(g, mb, zs, mb.sx))) return rc;
  GHIP(mb, hipStreamSynchronize(mb.sx));
  u64 unused = 0;
  if ((rc = adopt_sizes(g, mb, kBackSizes, false, &unused))) return rc;
  std::vector<Seg> back;
  segment_plan(zs.host, W, &back);
  Totals tb;
  if ((rc = round_totals(mb, back, "round", "answers", &tb))) return rc;
  if (tb.c_send != wrote)
    return fail(mb, PHIP_ERR_INVALID, "internal: split %llu of %llu answers",
                (unsigned long long)tb.c_send, (unsigned long long)wrote);
  GHIP(mb, mb.rback.ensure(tb.c_recv, tb.b_recv));
  GHIP(mb, mb.tm.mark(1, mb.sx));
  if ((rc = move_segments(g, mb, back, ln.rsend, mb.rback, mb.sx, rccl_self,
                          peers_of(g, mb, kBackSizes, 0, [&](const Member& m) -> const ColSet& {
                            return m.lane[si].rsend;
                          }))))
    return rc;
  GHIP(mb, mb.tm.mark(1, mb.sx));
  // every source holds its answers before an owner's next round rewrites them
  GHIP(mb, hipStreamSynchronize(mb.sx));
  if (g->shared && !g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
  // the source: into the caller's buffers, in batch order
  const u64 R = tb.c_recv;
  rp.replies += R;
  if (!R || rp.cut) return PHIP_OK;
  for (Buf* b : {&mb.gkey_in, &mb.gval_in, &mb.gkey, &mb.gval, &mb.gaoff}) GHIP(mb, b->ensure(R * 4));
  for (Buf* b : {&mb.gslen, &mb.gsend}) GHIP(mb, b->ensure(R * 8));
  GHIP(mb, mb.gctr.ensure(16));
  SegBounds from{}, so{};
  for (u32 p = 0; p < W; ++p) {
    from.at[p] = (u32)back[p].ro;
    so.at[p] = (u32)plan[p].so;
  }
  u32 *kin = (u32*)mb.gkey_in.p, *vin = (u32*)mb.gval_in.p, *keys = (u32*)mb.gkey.p,
      *vals = (u32*)mb.gval.p, *aoff = (u32*)mb.gaoff.p;
  const u32* lens = mb.rback.at<u32>(B_LENS);
  const unsigned grid = (unsigned)((R + 255) / 256);
  size_t t1 = 0, t2 = 0, t3 = 0;
  GHIP(mb, rocprim::exclusive_scan(nullptr, t1, lens, aoff, 0u, (size_t)R, rocprim::plus<u32>(), st));
  GHIP(mb, rocprim::radix_sort_pairs(nullptr, t2, kin, keys, vin, vals, (size_t)R, 0, 32, st));
  GHIP(mb, rocprim::inclusive_scan(nullptr, t3, (u64*)mb.gslen.p, (u64*)mb.gsend.p, (size_t)R,
                                   rocprim::plus<u64>(), st));
  GHIP(mb, mb.scan_tmp.ensure(std::max(t1, std::max(t2, t3))));
  GHIP(mb, mb.tm.mark(2, st));
  GHIP(mb, hipMemsetAsync(mb.gctr.p, 0, 16, st));
  k_back_keys<<<grid, 256, 0, st>>>(mb.rback.at<u32>(B_POS), (u32)R, from, so, W, (const u32*)ln.src.p,
                                    (u32)(k * chunk), kin, vin);
  GHIP(mb, hipGetLastError());
  GHIP(mb, rocprim::exclusive_scan(mb.scan_tmp.p, t1, lens, aoff, 0u, (size_t)R, rocprim::plus<u32>(), st));
  GHIP(mb, rocprim::radix_sort_pairs(mb.scan_tmp.p, t2, kin, keys, vin, vals, (size_t)R, 0, 32, st));
  k_gather_lens<<<grid, 256, 0, st>>>(vals, lens, (u32)R, (u64*)mb.gslen.p);
  GHIP(mb, hipGetLastError());
  GHIP(mb, rocprim::inclusive_scan(mb.scan_tmp.p, t3, (u64*)mb.gslen.p, (u64*)mb.gsend.p, (size_t)R,
                                   rocprim::plus<u64>(), st));
  k_reply_gather<<<(unsigned)((R * 64 + 255) / 256), 256, 0, st>>>(
      vals, keys, lens, aoff, (const u64*)mb.gsend.p, (u32)R, mb.rback.at<uint8_t>(B_BYTES), rp.n,
      rp.bytes, rp.rq->max_msgs, rp.budget, rp.rq->out, rp.rq->offs, rp.rq->src,
      (unsigned long long*)mb.gctr.p);
  GHIP(mb, hipGetLastError());
  GHIP(mb, mb.tm.mark(2, st));
  u64 c[2] = {0, 0};
  GHIP(mb, hipMemcpyAsync(c, mb.gctr.p, sizeof c, hipMemcpyDeviceToHost, st));
  GHIP(mb, hipStreamSynchronize(st));
  if (c[0]) {
    rp.n += c[0];
    rp.bytes = c[1];
  }
  rp.cut = c[0] < R;
  return PHIP_OK;
}

template <class Batch>
int member_receive(phip_group* g, Member& mb, Batch&& in, int64_t now, uint64_t* sent,
                   uint64_t* merged, uint32_t flags, Replies* rp = nullptr) {
  const u32 W = g->world;
  const u32 n = in.n();
  GHIP(mb, hipSetDevice(mb.device));
  hipStream_t st = (hipStream_t)phip_host::handle_stream(mb.h);
  // PHIP_GROUP_RCCL_SELF: the member's own segment goes through RCCL too (a
  // send/recv pair to itself), so that the per-peer exchange below runs at
  // world 1, on one GPU, with the plan the multi-GPU group uses
  const bool rccl_self = (flags & PHIP_GROUP_RCCL_SELF) && !g->shared;
  mb.tm.reset();
  if (rp) std::fill(mb.rstats, mb.rstats + RS_WORDS, 0);
  if (W == 1 && !rccl_self) {
    // One owner: every message is this member's, so there is nothing to
    // pack or exchange; the batch is merged as it came (the sender-side
    // combine is subsumed by the fast path's hot directory).
    if (sent) *sent = n;
    if (merged) *merged = n;
    if (rp) {
      // ... with its answers, the handle's own reply egress writing straight
      // into the caller's buffers (an empty batch too: offs[0] = 0); the
      // counters in the group's terms
      phip_reply_egress q = *rp->rq;
      GHIP(mb, mb.tm.mark(2, st));
      if (int r = in.whole_replies(mb, now, &q)) return r;
      GHIP(mb, mb.tm.mark(2, st));
      rp->n = q.n;
      rp->bytes = q.bytes;
      rp->skipped = q.skipped;
      rp->replies = q.replies - q.skipped;
      mb.rstats[RS_ROUNDS] = 1;
      mb.rstats[RS_WRITTEN] = q.n;
      return PHIP_OK;
    }
    if (n == 0) return PHIP_OK;
    GHIP(mb, mb.tm.mark(2, st));
    if (int r = in.whole(mb, now)) return r;
    GHIP(mb, mb.tm.mark(2, st));
    return PHIP_OK;
  }
  if (rp) GHIP(mb, hipMemsetAsync(rp->rq->offs, 0, sizeof(u64), st));   // (no answer: offs[0] = 0)
  // The batch's producers are on the handle's stream: both pipeline streams
  // start behind it.
  GHIP(mb, hipEventRecord(mb.ev_done, st));
  GHIP(mb, hipStreamWaitEvent(mb.sp, mb.ev_done, 0));
  GHIP(mb, hipStreamWaitEvent(mb.sx, mb.ev_done, 0));
  // (PHIP_GROUP_SMALL_CHUNKS, testing: many rounds on small batches)
  const u64 chunk = (flags & PHIP_GROUP_SMALL_CHUNKS) ? kSmallChunk : kChunk;
  const u64 cmax = std::max<u64>(1, std::min<u64>(n, chunk));
  int rc;
  // name bytes per chunk and lane: the offsets at the chunk boundaries
  if ((rc = in.bounds(g, mb, st, chunk))) return rc;
  const u64 k_local = mb.k_local;
  u64 set_bytes[2] = {0, 0};
  for (u64 k = 0; k < k_local; ++k)
    set_bytes[k & 1] = std::max<u64>(set_bytes[k & 1], in.chunk_bytes(chunk, k));
  for (u32 si = 0; si < 2; ++si) {
    GHIP(mb, mb.lane[si].send.ensure(cmax, set_bytes[si]));
    GHIP(mb, mb.sz[si].dev.ensure((size_t)6 * W * 8));
    if (rp) GHIP(mb, mb.lane[si].src.ensure(cmax * 4 + 4));
    mb.lane[si].x_pending = false;
    mb.lane[si].to_merge = false;
  }
  // 1. the combine's directory, from a sample of the whole batch
  const void* dir = nullptr;
  if ((flags & PHIP_ROUTE_COMBINE) && n && in.dir(mb, W, &dir) != PHIP_OK)
    return fail(mb, PHIP_ERR_HIP, "route directory: %s", phip_host::last_error(mb.h));
  // 2. pack chunk k into lane k & 1 (pack stream), once no exchange reads it
  auto pack = [&](u64 k) -> int {
    Lane& ln = mb.lane[k & 1];
    const ColSet& ss = ln.send;
    if (ln.x_pending) GHIP(mb, hipStreamWaitEvent(mb.sp, ln.ev_x, 0));
    u64* sz = (u64*)mb.sz[k & 1].dev.p;
    GHIP(mb, mb.tm.mark(0, mb.sp));
    if (in.pack(mb, chunk, k, W, dir, ss, sz, rp ? (u32*)ln.src.p : nullptr) != PHIP_OK)
      return fail(mb, PHIP_ERR_HIP, "route pack: %s", phip_host::last_error(mb.h));
    GHIP(mb, hipMemcpyAsync(sz + 2 * W, mb.host_k, W * 8, hipMemcpyHostToDevice, mb.sp));
    // the *_replies forms: the chunk's zero-state messages, to every owner
    if (rp && in.count_zero(mb, chunk, k, W, sz + 2 * W) != PHIP_OK)
      return fail(mb, PHIP_ERR_HIP, "zero-state count: %s", phip_host::last_error(mb.h));
    GHIP(mb, mb.tm.mark(0, mb.sp));
    GHIP(mb, hipEventRecord(ln.ev_pack, mb.sp));
    return PHIP_OK;
  };
  // 3. chunk k's split sizes, behind its pack (exchange stream)
  auto sizes = [&](u64 k) -> int {
    Lane& ln = mb.lane[k & 1];
    GHIP(mb, hipStreamWaitEvent(mb.sx, ln.ev_pack, 0));
    if (int r = exchange_sizes(g, mb, mb.sz[k & 1], mb.sx)) return r;
    GHIP(mb, hipEventRecord(ln.ev_sz, mb.sx));
    return PHIP_OK;
  };
  if ((rc = pack(0)) || (rc = sizes(0))) return rc;
  if (k_local > 1 && (rc = pack(1))) return rc;
  u64 K = 1, n_send = 0, recv_msgs = 0;
  u64 packed = k_local > 1 ? 2 : 1;   // chunks whose pack is queued
  std::vector<Seg> plan;
  for (u64 k = 0; k < K; ++k) {
    const u32 si = k & 1;
    Lane& ln = mb.lane[si];
    GHIP(mb, hipEventSynchronize(ln.ev_sz));
    if ((rc = adopt_sizes(g, mb, si, k == 0, &K))) return rc;
    segment_plan(mb.sz[si].host, W, &plan);
    Totals t;
    if ((rc = round_totals(mb, plan, "chunk", "messages", &t))) return rc;
    // room in the lane's receive set, once the merge of the chunk it held
    // before is done
    if (ln.merge_pending) GHIP(mb, hipEventSynchronize(ln.ev_merged));
    ln.merge_pending = false;
    GHIP(mb, ln.recv.ensure(t.c_recv, t.b_recv));
    // 4. the segments
    GHIP(mb, mb.tm.mark(1, mb.sx));
    if ((rc = move_segments(g, mb, plan, ln.send, ln.recv, mb.sx, rccl_self,
                            peers_of(g, mb, si, 0, [&](const Member& m) -> const ColSet& {
                              return m.lane[si].send;
                            }))))
      return rc;
    GHIP(mb, mb.tm.mark(1, mb.sx));
    GHIP(mb, hipEventRecord(ln.ev_x, mb.sx));
    GHIP(mb, hipEventRecord(ln.ev_recv, mb.sx));
    ln.x_pending = true;
    ln.n = t.c_recv;
    ln.to_merge = true;
    n_send += t.c_send;
    recv_msgs += t.c_recv;
    // the *_replies forms: does any member's chunk hold a zero-state message,
    // and how many requests can have reached this owner (never the chunk size)
    bool requests = false;
    u64 bound = 0;
    if (rp)
      for (u32 p = 0; p < W; ++p) {
        const u64 z = zero_states_of(mb.sz[si].host, W, p);
        requests |= z != 0;
        bound += std::min<u64>(z, plan[p].rc);
      }
    // 6. the owner's merge of chunk k-1 beside chunk k's exchange (chunk
    //    order: the merges queue on the handle's stream; a shared-device
    //    member merges before it waits for its copies)
    const bool merge_prev = k >= 1 && mb.lane[(k - 1) & 1].to_merge;
    if (g->shared) {
      if (merge_prev && (rc = merge_chunk(mb, mb.lane[(k - 1) & 1], st, now))) return rc;
      // every member has copied chunk k out of every lane k & 1 before any
      // packs chunk k + 2 into it
      GHIP(mb, hipEventSynchronize(ln.ev_x));
      if (!g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
    }
    // A round with requests is finished here -- the merges in chunk order,
    // the answers' way back, the gather -- before the next round's sizes are
    // queued; a round without runs the path it always did.
    if (requests) {
      if (!g->shared && merge_prev && (rc = merge_chunk(mb, mb.lane[(k - 1) & 1], st, now))) return rc;
      if ((rc = reply_round(g, mb, si, k, chunk, plan, bound, now, rccl_self, *rp, st))) return rc;
    }
    // 5. next: chunk k+1's sizes behind chunk k's exchange (RCCL keeps one
    //    order per communicator), chunk k+2's pack into the lane just sent
    if (k + 1 < K) {
      if (packed < k + 2) {   // a chunk past this member's batch: an empty pack
        if ((rc = pack(k + 1))) return rc;
        packed = k + 2;
      }
      if ((rc = sizes(k + 1))) return rc;
      if (k + 2 < K && packed < k + 3) {
        if ((rc = pack(k + 2))) return rc;
        packed = k + 3;
      }
    }
    // (a round with requests has merged chunk k-1 already)
    if (!g->shared && k >= 1 && mb.lane[(k - 1) & 1].to_merge &&
        (rc = merge_chunk(mb, mb.lane[(k - 1) & 1], st, now)))
      return rc;
  }
  if (sent) *sent = n_send;
  if (merged) *merged = recv_msgs;
  if (rp) mb.rstats[RS_ROUNDS] = K;
  // the last chunk's merge; the handle's stream ends behind every exchange
  // (the next call's packs reuse the send sets)
  if (mb.lane[(K - 1) & 1].to_merge && (rc = merge_chunk(mb, mb.lane[(K - 1) & 1], st, now))) return rc;
  GHIP(mb, hipEventRecord(mb.ev_done, mb.sx));
  GHIP(mb, hipStreamWaitEvent(st, mb.ev_done, 0));
  return PHIP_OK;
}

// Round k of an op batch: ops [k * chunk, ...) (empty past the batch).
phip_ops ops_chunk_of(const phip_ops& in, u64 chunk, u64 k) {
  phip_ops c = in;
  const u64 lo = k * chunk;
  c.n = lo < in.n ? (u32)std::min<u64>(chunk, in.n - lo) : 0u;
  if (c.n) {
    if (in.kind) c.kind = in.kind + lo;   // (a query batch has none)
    c.name_offs = in.name_offs + lo;   // absolute offsets into the same blob
    c.now = in.now + lo;
    if (in.freq) c.freq = in.freq + lo;
    if (in.per) c.per = in.per + lo;
    if (in.count) c.count = in.count + lo;
    if (in.added) c.added = in.added + lo;
    if (in.taken) c.taken = in.taken + lo;
    if (in.elapsed) c.elapsed = in.elapsed + lo;
  }
  return c;
}

phip_results results_from(const phip_results& r, u64 lo) {
  phip_results c = r;
  if (c.status) c.status += lo;
  if (c.remaining) c.remaining += lo;
  if (c.have) c.have += lo;
  if (c.reply) c.reply += lo;
  return c;
}

phip_peek_results peek_results_from(const phip_peek_results& r, u64 lo) {
  phip_peek_results c = r;
  if (c.status) c.status += lo;
  if (c.remaining) c.remaining += lo;
  if (c.have) c.have += lo;
  if (c.retry_at) c.retry_at += lo;
  if (c.state) c.state += lo;
  return c;
}

// What member_routed asks of a routed call over an op batch: the member's
// four column sets of the call (a round packed owner-major, as the owner
// received it, the owner's results, the results returned to this source),
// what an entry is called in an error, the call on the one handle where there
// is nothing to route, the pack of one round (split sizes into sz), the
// owner's step over the n entries it received (their names' offsets in
// mb.ooffs) and the scatter of a round's n returned results into the caller's
// columns from entry lo on.
//
// phip_group_apply_mixed: the ops with their kind byte forward, one
// phip_apply_mixed at the owner, the four result columns back.
struct OpsPath {
  const phip_results& res;
  static constexpr ColSet Member::*kSend = &Member::osend, Member::*kRecv = &Member::orecv,
                          Member::*kRes = &Member::ores, Member::*kBack = &Member::oback;
  static constexpr const char* kItems = "ops";
  void begin(Member&) const {}
  int direct(Member& mb, const phip_ops& in) const {
    GPHIP(mb, phip_apply_mixed(mb.h, &in, &res, PHIP_DEVICE_PTRS));
    return PHIP_OK;
  }
  int pack(Member& mb, hipStream_t st, const phip_ops& c, u32 W, u64* sz) const {
    const ColSet& ss = mb.osend;
    if (phip_host::route_pack_ops(mb.h, st, &c, W, ss.at<uint8_t>(C_NAMES), ss.at<uint32_t>(C_LENS),
                                  ss.at<uint8_t>(O_KIND), ss.at<int64_t>(O_NOW), ss.at<uint64_t>(O_X0),
                                  ss.at<uint64_t>(O_X1), ss.at<uint64_t>(O_X2), (uint32_t*)mb.osrc.p,
                                  sz, sz + W) != PHIP_OK)
      return fail(mb, PHIP_ERR_HIP, "route pack ops: %s", phip_host::last_error(mb.h));
    return PHIP_OK;
  }
  // One phip_apply_mixed over the round (sources in rank order, each in its
  // order).  The three operand words serve both kinds: k_pack_ops reads
  // freq/per/count under TAKE and added/taken/elapsed otherwise.
  int owner(Member& mb, u64 n) const {
    const ColSet& rs = mb.orecv;
    phip_ops ro{};
    ro.n = (u32)n;
    ro.kind = rs.at<uint8_t>(O_KIND);
    ro.names = rs.at<uint8_t>(C_NAMES);
    ro.name_offs = (const u32*)mb.ooffs.p;
    ro.now = rs.at<int64_t>(O_NOW);
    ro.freq = rs.at<int64_t>(O_X0);
    ro.per = rs.at<int64_t>(O_X1);
    ro.count = rs.at<uint64_t>(O_X2);
    ro.added = rs.at<uint64_t>(O_X0);
    ro.taken = rs.at<uint64_t>(O_X1);
    ro.elapsed = rs.at<int64_t>(O_X2);
    phip_results rr{};
    rr.status = mb.ores.at<uint8_t>(R_STATUS);
    rr.remaining = mb.ores.at<uint64_t>(R_REM);
    rr.have = mb.ores.at<uint64_t>(R_HAVE);
    rr.reply = mb.ores.at<phip_state>(R_REPLY);
    GPHIP(mb, phip_apply_mixed(mb.h, &ro, &rr, PHIP_DEVICE_PTRS));
    return PHIP_OK;
  }
  int scatter(Member& mb, hipStream_t st, u32 n, u64 lo) const {
    const phip_results out = results_from(res, lo);
    if (phip_host::results_scatter(mb.h, st, (const uint32_t*)mb.osrc.p, n,
                                   mb.oback.at<uint8_t>(R_STATUS), mb.oback.at<uint64_t>(R_REM),
                                   mb.oback.at<uint64_t>(R_HAVE), mb.oback.at<phip_state>(R_REPLY),
                                   &out) != PHIP_OK)
      return fail(mb, PHIP_ERR_HIP, "results scatter: %s", phip_host::last_error(mb.h));
    return PHIP_OK;
  }
};

// phip_group_peek: the queries without a kind byte forward, one read-only
// phip_peek at the owner, the peek columns back, with the evaluated state
// only when the call asked for it (every process alike).  Nothing of any
// handle is written.
struct PeekPath {
  const phip_peek_results& res;
  bool with_state;
  static constexpr ColSet Member::*kSend = &Member::qsend, Member::*kRecv = &Member::qrecv,
                          Member::*kRes = &Member::pres, Member::*kBack = &Member::pback;
  static constexpr const char* kItems = "queries";
  void begin(Member& mb) const {   // the answer columns of this call
    mb.pres.cols = mb.pback.cols = with_state ? &kPeekStateCols : &kPeekCols;
  }
  int direct(Member& mb, const phip_ops& in) const {
    GPHIP(mb, phip_peek(mb.h, &in, &res, PHIP_DEVICE_PTRS));
    return PHIP_OK;
  }
  int pack(Member& mb, hipStream_t st, const phip_ops& c, u32 W, u64* sz) const {
    const ColSet& ss = mb.qsend;
    if (phip_host::route_pack_queries(mb.h, st, &c, W, ss.at<uint8_t>(C_NAMES), ss.at<uint32_t>(C_LENS),
                                      ss.at<int64_t>(Q_NOW), ss.at<uint64_t>(Q_X0),
                                      ss.at<uint64_t>(Q_X1), ss.at<uint64_t>(Q_X2),
                                      (uint32_t*)mb.osrc.p, sz, sz + W) != PHIP_OK)
      return fail(mb, PHIP_ERR_HIP, "route pack queries: %s", phip_host::last_error(mb.h));
    return PHIP_OK;
  }
  int owner(Member& mb, u64 n) const {
    const ColSet& rs = mb.qrecv;
    phip_ops rq{};
    rq.n = (u32)n;
    rq.names = rs.at<uint8_t>(C_NAMES);
    rq.name_offs = (const u32*)mb.ooffs.p;
    rq.now = rs.at<int64_t>(Q_NOW);
    rq.freq = rs.at<int64_t>(Q_X0);
    rq.per = rs.at<int64_t>(Q_X1);
    rq.count = rs.at<uint64_t>(Q_X2);
    phip_peek_results rr{};
    rr.status = mb.pres.at<uint8_t>(P_STATUS);
    rr.remaining = mb.pres.at<uint64_t>(P_REM);
    rr.have = mb.pres.at<uint64_t>(P_HAVE);
    rr.retry_at = mb.pres.at<int64_t>(P_AT);
    if (with_state) rr.state = mb.pres.at<phip_state>(P_STATE);
    GPHIP(mb, phip_peek(mb.h, &rq, &rr, PHIP_DEVICE_PTRS));
    return PHIP_OK;
  }
  int scatter(Member& mb, hipStream_t st, u32 n, u64 lo) const {
    const phip_peek_results out = peek_results_from(res, lo);
    if (phip_host::peek_results_scatter(
            mb.h, st, (const uint32_t*)mb.osrc.p, n, mb.pback.at<uint8_t>(P_STATUS),
            mb.pback.at<uint64_t>(P_REM), mb.pback.at<uint64_t>(P_HAVE), mb.pback.at<int64_t>(P_AT),
            with_state ? mb.pback.at<phip_state>(P_STATE) : nullptr, &out) != PHIP_OK)
      return fail(mb, PHIP_ERR_HIP, "peek results scatter: %s", phip_host::last_error(mb.h));
    return PHIP_OK;
  }
};

// One member's part of an owner-routed call over an op batch (OpsPath: the
// order rule in patrolhip.h; PeekPath: read-only, so no order shows and the
// rounds only bound the scratch and keep the members' collective calls alike).
// The rounds run one after another on the handle's stream: pack, split
// sizes, the entries to their owners, the owner's step, the results back to
// their sources, the scatter into the caller's columns.  An ordered round
// cannot start before the one before it was applied, and a Take's caller
// waits for its result, so there is nothing to overlap across rounds.
// osrc, ooffs and the split sizes serve both paths: a group runs one call at
// a time.
template <class Path>
int member_routed(phip_group* g, Member& mb, const phip_ops& in, const Path& path, uint64_t* sent,
                  uint64_t* done, uint32_t flags) {
  const u32 W = g->world;
  const u32 n = in.n;
  GHIP(mb, hipSetDevice(mb.device));
  hipStream_t st = (hipStream_t)phip_host::handle_stream(mb.h);
  const bool rccl_self = (flags & PHIP_GROUP_RCCL_SELF) && !g->shared;
  mb.tm.reset();
  if (W == 1 && !rccl_self) {   // one owner: nothing to route
    if (sent) *sent = n;
    if (done) *done = n;
    if (n == 0) return PHIP_OK;
    GHIP(mb, mb.tm.mark(2, st));
    if (int r = path.direct(mb, in)) return r;
    GHIP(mb, mb.tm.mark(2, st));
    return PHIP_OK;
  }
  const u64 chunk = (flags & PHIP_GROUP_SMALL_CHUNKS) ? kSmallChunk : kChunk;
  const u64 cmax = std::max<u64>(1, std::min<u64>(n, chunk));
  int rc;
  // name bytes of the largest round: the offsets at the chunk boundaries
  std::vector<u32> bnd;
  if ((rc = chunk_bounds(g, mb, st, in.name_offs, n, chunk, &bnd))) return rc;
  u64 max_bytes = 0;
  for (u64 k = 0; k < mb.k_local; ++k) max_bytes = std::max<u64>(max_bytes, (u64)(bnd[k + 1] - bnd[k]));
  path.begin(mb);
  Sizes& zs = mb.sz[kOpsSizes];
  ColSet &ss = mb.*Path::kSend, &rs = mb.*Path::kRecv, &res = mb.*Path::kRes, &bk = mb.*Path::kBack;
  GHIP(mb, ss.ensure(cmax, max_bytes));
  GHIP(mb, mb.osrc.ensure(cmax * 4 + 4));
  GHIP(mb, bk.ensure(cmax, 0));
  GHIP(mb, zs.dev.ensure((size_t)6 * W * 8));
  u64* sz = (u64*)zs.dev.p;
  u64 K = 1, n_send = 0, n_recv = 0;
  std::vector<Seg> plan, back(W);
  for (u64 k = 0; k < K; ++k) {
    // 1. the pack of round k
    const phip_ops c = ops_chunk_of(in, chunk, k);
    GHIP(mb, mb.tm.mark(0, st));
    if ((rc = path.pack(mb, st, c, W, sz))) return rc;
    GHIP(mb, hipMemcpyAsync(sz + 2 * W, mb.host_k, W * 8, hipMemcpyHostToDevice, st));
    GHIP(mb, mb.tm.mark(0, st));
    // 2. the split sizes
    if ((rc = exchange_sizes(g, mb, zs, st))) return rc;
    GHIP(mb, hipStreamSynchronize(st));
    if ((rc = adopt_sizes(g, mb, kOpsSizes, k == 0, &K))) return rc;
    segment_plan(zs.host, W, &plan);
    Totals t;
    if ((rc = round_totals(mb, plan, "round", Path::kItems, &t))) return rc;
    if (t.c_send != c.n)
      return fail(mb, PHIP_ERR_INVALID, "internal: packed %llu of %u %s", (unsigned long long)t.c_send,
                  c.n, Path::kItems);
    GHIP(mb, rs.ensure(t.c_recv, t.b_recv));
    GHIP(mb, mb.ooffs.ensure(t.c_recv * 4 + 8));
    GHIP(mb, res.ensure(t.c_recv, 0));
    // 3. the entries to their owners
    GHIP(mb, mb.tm.mark(1, st));
    if ((rc = move_segments(g, mb, plan, ss, rs, st, rccl_self,
                            peers_of(g, mb, kOpsSizes, 0, [](const Member& m) -> const ColSet& {
                              return m.*Path::kSend;
                            }))))
      return rc;
    GHIP(mb, mb.tm.mark(1, st));
    // 4. the owner's step: the names' offsets, then one call over the round
    if (t.c_recv) {
      GHIP(mb, mb.tm.mark(2, st));
      if ((rc = offsets_from_lens(mb, rs.at<u32>(C_LENS), t.c_recv, (u32*)mb.ooffs.p, st))) return rc;
      if ((rc = path.owner(mb, t.c_recv))) return rc;
      GHIP(mb, mb.tm.mark(2, st));
    }
    // 5. the results back to their sources: source p's segment [ro, ro + rc)
    //    of the owner's result buffers lands at [so, so + sc) of p's returned
    //    columns (the forward plan with its roles swapped).  In a shared-device
    //    group every owner's results are complete before any source copies
    //    them, and every source has copied before an owner reuses its buffers.
    if (g->shared) {
      GHIP(mb, hipStreamSynchronize(st));
      if (!g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
    }
    for (u32 p = 0; p < W; ++p) back[p] = swapped(plan[p]);
    GHIP(mb, mb.tm.mark(1, st));
    if ((rc = move_segments(g, mb, back, res, bk, st, rccl_self,
                            peers_of(g, mb, kOpsSizes, 3 * W, [](const Member& m) -> const ColSet& {
                              return m.*Path::kRes;
                            }))))
      return rc;
    GHIP(mb, mb.tm.mark(1, st));
    if (g->shared) {
      GHIP(mb, hipStreamSynchronize(st));
      if (!g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
    }
    // 6. into the caller's columns, at the entries' places in the batch
    if (c.n) {
      GHIP(mb, mb.tm.mark(2, st));
      if ((rc = path.scatter(mb, st, c.n, k * chunk))) return rc;
      GHIP(mb, mb.tm.mark(2, st));
    }
    n_send += t.c_send;
    n_recv += t.c_recv;
  }
  if (sent) *sent = n_send;
  if (done) *done = n_recv;
  GHIP(mb, hipStreamSynchronize(st));   // the results are the caller's to read
  return PHIP_OK;
}

__global__ void k_max_into(int64_t* __restrict__ dst, const int64_t* __restrict__ src, u64 n) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && src[i] > dst[i]) dst[i] = src[i];
}

int member_anti_entropy(phip_group* g, Member& mb, int64_t* reps, uint32_t nrep, uint64_t B) {
  GHIP(mb, hipSetDevice(mb.device));
  mb.tm.reset();
  hipStream_t st = (hipStream_t)phip_host::handle_stream(mb.h);
  if (g->world == 1) {   // nothing to exchange: the fused local join
    GHIP(mb, mb.tm.mark(0, st));
    GPHIP(mb, phip_ae_join(mb.h, reps, nrep, B, PHIP_DEVICE_PTRS));
    GHIP(mb, mb.tm.mark(0, st));
    return PHIP_OK;
  }
  GHIP(mb, mb.ae.ensure((size_t)3 * B * 8 * (g->shared ? 2 : 1)));
  int64_t* j = (int64_t*)mb.ae.p;
  GHIP(mb, mb.tm.mark(0, st));
  GPHIP(mb, phip_ae_local_max(mb.h, reps, nrep, B, j, PHIP_DEVICE_PTRS));
  GHIP(mb, mb.tm.mark(0, st));
  if (g->shared) {   // the all-reduce: every member's join, max'd element-wise
    if (!g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
    int64_t* jm = j + 3 * B;
    GHIP(mb, hipMemcpyAsync(jm, j, 3 * B * 8, hipMemcpyDeviceToDevice, st));
    for (const Member& p : g->m) {
      if (&p == &mb) continue;
      k_max_into<<<(unsigned)((3 * B + 255) / 256), 256, 0, st>>>(jm, (const int64_t*)p.ae.p, 3 * B);
      GHIP(mb, hipGetLastError());
    }
    GHIP(mb, hipStreamSynchronize(st));
    if (!g->bar.wait()) return fail(mb, PHIP_ERR_INVALID, "another member failed");
    GHIP(mb, mb.tm.mark(2, st));
    GPHIP(mb, phip_ae_apply(mb.h, reps, nrep, B, jm, PHIP_DEVICE_PTRS));
    GHIP(mb, mb.tm.mark(2, st));
    return PHIP_OK;
  }
  GHIP(mb, mb.tm.mark(1, st));
  GNCCL(mb, ncclAllReduce(j, j, 3 * B, ncclInt64, ncclMax, mb.comm, st));
  GHIP(mb, mb.tm.mark(1, st));
  GHIP(mb, mb.tm.mark(2, st));
  GPHIP(mb, phip_ae_apply(mb.h, reps, nrep, B, j, PHIP_DEVICE_PTRS));
  GHIP(mb, mb.tm.mark(2, st));
  return PHIP_OK;
}

void destroy(phip_group* g) {
  for (auto& mb : g->m) {
    (void)hipSetDevice(mb.device);
    if (mb.h) (void)phip_flush(mb.h);
    if (mb.sp) (void)hipStreamSynchronize(mb.sp);
    if (mb.sx) (void)hipStreamSynchronize(mb.sx);
    if (mb.comm) (void)ncclCommDestroy(mb.comm);
    for (Lane& ln : mb.lane) {
      ln.send.release();
      ln.recv.release();
      ln.offs.release();
      for (Buf* b : {&ln.src, &ln.roffs, &ln.rsrc}) b->release();
      ln.rsend.release();
      for (hipEvent_t ev : {ln.ev_pack, ln.ev_sz, ln.ev_x, ln.ev_recv, ln.ev_merged})
        if (ev) (void)hipEventDestroy(ev);
    }
    for (ColSet* s : {&mb.osend, &mb.orecv, &mb.ores, &mb.oback, &mb.qsend, &mb.qrecv, &mb.pres,
                      &mb.pback})
      s->release();
    for (Sizes& s : mb.sz) {
      s.dev.release();
      if (s.host) (void)hipHostFree(s.host);
    }
    for (Buf* b : {&mb.osrc, &mb.ooffs, &mb.scan_tmp, &mb.ae, &mb.bounds, &mb.gkey_in, &mb.gval_in,
                   &mb.gkey, &mb.gval, &mb.gaoff, &mb.gslen, &mb.gsend, &mb.gctr, &mb.ring_out,
                   &mb.ring_offs, &mb.ring_src})
      b->release();
    mb.rback.release();
    if (mb.ev_rep) (void)hipEventDestroy(mb.ev_rep);
    mb.tm.release();
    if (mb.host_k) (void)hipHostFree(mb.host_k);
    if (mb.ev_done) (void)hipEventDestroy(mb.ev_done);
    if (mb.sp) (void)hipStreamDestroy(mb.sp);
    if (mb.sx) (void)hipStreamDestroy(mb.sx);
    if (mb.own && mb.h) phip_close(mb.h);
  }
  delete g;
}

// Per member: the pipeline's two streams, the pinned mirrors of the split
// sizes and the lanes' events.
int alloc_member_state(phip_group* g) {
  for (auto& mb : g->m) {
    if (hipSetDevice(mb.device) != hipSuccess ||
        hipStreamCreateWithFlags(&mb.sp, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&mb.sx, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&mb.ev_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&mb.ev_rep, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&mb.host_k, (size_t)g->world * sizeof(u64), 0) != hipSuccess)
      return PHIP_ERR_HIP;
    for (Sizes& s : mb.sz)
      if (hipHostMalloc(&s.host, 6 * (size_t)g->world * sizeof(u64), 0) != hipSuccess)
        return PHIP_ERR_HIP;
    for (Lane& ln : mb.lane)
      for (hipEvent_t* ev : {&ln.ev_pack, &ln.ev_sz, &ln.ev_x, &ln.ev_recv, &ln.ev_merged})
        if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) return PHIP_ERR_HIP;
  }
  return PHIP_OK;
}

// A group call over checked batches (names_len; phip_msgs or phip_ops): every
// local member's offset column in full before any chunk is packed (the route
// kernels do not check as they go), behind pre(member, its stream, i).  One
// malformed entry anywhere and none of this process's batches is applied; the
// members still run the exchange, with empty batches, so that the peers of a
// multi-rank group never wait for a rank that left early.  run(i, batch) is
// the member's call; `what` names an entry in the error text.
template <class Batch, class Pre, class Run>
int checked_call(phip_group* g, const Batch* batches, const char* what, Pre pre, Run run) {
  const size_t nl = g->m.size();
  std::vector<uint32_t> bad(nl, ~0u);
  if (int rc = for_members(g, [&](size_t i) {
        Member& mb = g->m[i];
        GHIP(mb, hipSetDevice(mb.device));
        hipStream_t st = (hipStream_t)phip_host::handle_stream(mb.h);
        if (int r = pre(mb, st, i)) return r;
        const Batch& b = batches[i];
        if (phip_host::check_offsets(mb.h, st, b.names, b.name_offs, b.names_len, b.n, &bad[i]) !=
            PHIP_OK)
          return fail(mb, PHIP_ERR_HIP, "name offsets check: %s", phip_host::last_error(mb.h));
        return (int)PHIP_OK;
      }))
    return rc;
  size_t ib = 0;
  while (ib < nl && bad[ib] == ~0u) ++ib;
  if (ib < nl) {
    std::vector<Batch> none(batches, batches + nl);
    for (Batch& b : none) b.n = 0;
    const int rc = for_members(g, [&](size_t i) { return run(i, none[i]); });
    const std::string xerr = rc != PHIP_OK ? "; and the empty exchange failed: " + g->err : "";
    g->err = "member " + std::to_string(ib) + ": malformed name offsets at " + what + " " +
             std::to_string(bad[ib]) + " (names_len check): no local batch applied" + xerr;
    return PHIP_ERR_INVALID;
  }
  return for_members(g, [&](size_t i) { return run(i, batches[i]); });
}

bool wire_flags_ok(uint32_t flags) {
  constexpr uint32_t kAllowed =
      PHIP_DEVICE_PTRS | PHIP_ROUTE_COMBINE | PHIP_GROUP_RCCL_SELF | PHIP_GROUP_SMALL_CHUNKS;
  return (flags & PHIP_DEVICE_PTRS) && !(flags & ~kAllowed);
}

// phip_group_receive_datagrams over the local members' wire batches, behind
// pre(member, its stream, i).  The pre-pass of every member first (the Go
// loop's stop rule, repo.go:70-74, and a checked batch's offsets): member i
// then runs the exchange over datagrams [0, stop_i), or over none when any
// local batch's offsets were rejected (checked_call's rule: the peers of a
// multi-rank group never wait for a rank that left early).
template <class Pre>
int receive_wire(phip_group* g, const phip_wire* batches, int64_t now, uint64_t* sent,
                 uint64_t* merged, uint32_t* stopped, uint32_t flags, Pre pre,
                 std::vector<Replies>* reps = nullptr) {
  const size_t nl = g->m.size();
  std::vector<uint32_t> stop(nl, 0), bad(nl, ~0u);
  if (int rc = for_members(g, [&](size_t i) {
        Member& mb = g->m[i];
        GHIP(mb, hipSetDevice(mb.device));
        hipStream_t st = (hipStream_t)phip_host::handle_stream(mb.h);
        if (int r = pre(mb, st, i)) return r;
        if (phip_host::wire_scan(mb.h, st, &batches[i], &stop[i], &bad[i]) != PHIP_OK)
          return fail(mb, PHIP_ERR_HIP, "datagram pre-pass: %s", phip_host::last_error(mb.h));
        return (int)PHIP_OK;
      }))
    return rc;
  size_t ib = 0;
  while (ib < nl && bad[ib] == ~0u) ++ib;
  std::vector<phip_wire> cut(batches, batches + nl);
  for (size_t i = 0; i < nl; ++i) {
    cut[i].n = ib < nl ? 0 : stop[i];
    if (stopped) stopped[i] = cut[i].n;
  }
  const int rc = for_members(g, [&](size_t i) {
    return member_receive(g, g->m[i], WireBatch{cut[i], {}}, now, sent ? sent + i : nullptr,
                          merged ? merged + i : nullptr, flags, reps ? &(*reps)[i] : nullptr);
  });
  if (ib < nl) {
    const std::string xerr = rc != PHIP_OK ? "; and the empty exchange failed: " + g->err : "";
    g->err = "member " + std::to_string(ib) + ": malformed datagram offsets at datagram " +
             std::to_string(bad[ib]) + " (bytes_len check): no local batch applied" + xerr;
    return PHIP_ERR_INVALID;
  }
  if (rc != PHIP_OK) return rc;
  for (size_t i = 0; i < nl; ++i)
    if (stop[i] < batches[i].n) {
      g->err = "member " + std::to_string(i) + ": short buffer at datagram " + std::to_string(stop[i]);
      return PHIP_ERR_SHORT_BUFFER;
    }
  return PHIP_OK;
}

// ---- the *_replies forms' entry ----
void replies_zero(phip_reply_egress* rq, size_t nl) {
  for (size_t i = 0; i < nl; ++i) {
    rq[i].n = rq[i].replies = rq[i].skipped = 0;
    rq[i].bytes = 0;
  }
}

// phip_reply_egress' bounds for every local member, before anything of any
// member is applied; dev: the buffers are device memory (phip_export_sweep's
// rules).
bool replies_ok(const phip_reply_egress* rq, size_t nl, bool dev) {
  for (size_t i = 0; i < nl; ++i) {
    const phip_reply_egress& q = rq[i];
    if (!q.out || !q.offs || !q.max_msgs || q.out_cap < PHIP_BUCKET_PACKET_SIZE) return false;
    if (dev && ((reinterpret_cast<uintptr_t>(q.out) & 7) || (q.out_cap & 7) ||
                q.out_cap < PHIP_BUCKET_PACKET_SIZE + 8))
      return false;
  }
  return true;
}

std::vector<Replies> replies_of(phip_reply_egress* rq, size_t nl) {
  std::vector<Replies> v(nl);
  for (size_t i = 0; i < nl; ++i) {
    v[i].rq = &rq[i];
    v[i].budget = rq[i].out_cap - 8;
  }
  return v;
}

// The call's out fields: what the rounds wrote (a stopped member's answers
// before its stop included), zeros after any other error.
int replies_done(int rc, const std::vector<Replies>& reps, phip_reply_egress* rq) {
  replies_zero(rq, reps.size());
  if (rc != PHIP_OK && rc != PHIP_ERR_SHORT_BUFFER) return rc;
  for (size_t i = 0; i < reps.size(); ++i) {
    rq[i].n = (u32)reps[i].n;
    rq[i].replies = (u32)reps[i].replies;
    rq[i].skipped = (u32)reps[i].skipped;
    rq[i].bytes = reps[i].bytes;
  }
  return rc;
}

// phip_group_ring_receive, and with rq (host buffers) its replies form: the
// members write into device copies the group keeps, and what was written is
// copied back.
int ring_receive(phip_group* g, phip_ring* const* rings, const uint32_t* slots, int64_t now,
                 uint64_t* sent, uint64_t* merged, uint32_t* stopped, uint32_t flags,
                 phip_reply_egress* rq) {
  const size_t nl = g->m.size();
  std::vector<phip_wire> batches(nl, phip_wire{});
  std::vector<void*> copied(nl, nullptr);
  // (refused before anything is queued: every slot stays submitted)
  for (size_t i = 0; i < nl; ++i)
    if (rings[i])
      if (int rc = phip_host::ring_slot(rings[i], slots[i], g->m[i].h, &batches[i], &copied[i]))
        return rc;
  // the device form of the caller's caps: a byte budget of out_cap rounded
  // down to a multiple of 8
  std::vector<phip_reply_egress> dq;
  std::vector<Replies> reps;
  int rc0 = PHIP_OK;
  if (rq) {
    dq.assign(rq, rq + nl);
    for (size_t i = 0; i < nl && rc0 == PHIP_OK; ++i) {
      Member& mb = g->m[i];
      dq[i].out_cap = (rq[i].out_cap & ~7ull) + 8;
      if (hipSetDevice(mb.device) != hipSuccess || mb.ring_out.ensure(dq[i].out_cap) != hipSuccess ||
          mb.ring_offs.ensure(((size_t)rq[i].max_msgs + 1) * 8) != hipSuccess ||
          mb.ring_src.ensure((size_t)rq[i].max_msgs * 4) != hipSuccess) {
        g->err = "member " + std::to_string(i) + ": no device memory for the reply buffers";
        rc0 = PHIP_ERR_HIP;
      }
      dq[i].out = (uint8_t*)mb.ring_out.p;
      dq[i].offs = (uint64_t*)mb.ring_offs.p;
      dq[i].src = (uint32_t*)mb.ring_src.p;
    }
    if (rc0 != PHIP_OK) return rc0;   // (nothing queued: every slot stays submitted)
    reps = replies_of(dq.data(), nl);
  }
  int rc = receive_wire(g, batches.data(), now, sent, merged, stopped, flags,
                        [&](Member& mb, hipStream_t st, size_t i) {
                          // the member's streams all start behind st
                          if (copied[i])
                            GHIP(mb, hipStreamWaitEvent(st, (hipEvent_t)copied[i], 0));
                          return (int)PHIP_OK;
                        },
                        rq ? &reps : nullptr);
  // A slot is free once its member's streams have read it: the pack stream,
  // the exchange behind it, and the handle's stream (the pre-pass; a world of
  // one merges from the slot).  After an error they drain first.
  int rc2 = PHIP_OK;
  for (size_t i = 0; i < nl; ++i) {
    Member& mb = g->m[i];
    if (!rings[i] && !rq) continue;
    if (hipSetDevice(mb.device) != hipSuccess || hipStreamSynchronize(mb.sp) != hipSuccess ||
        hipStreamSynchronize(mb.sx) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)phip_host::handle_stream(mb.h)) != hipSuccess)
      rc2 = PHIP_ERR_HIP;
    if (rings[i]) phip_host::ring_release(rings[i], slots[i]);
  }
  if (rc == PHIP_OK && rc2 != PHIP_OK) g->err = "draining the members' streams failed";
  if (rc == PHIP_OK) rc = rc2;
  if (!rq) return rc;
  replies_done(rc, reps, dq.data());
  for (size_t i = 0; i < nl; ++i) {
    rq[i].n = dq[i].n;
    rq[i].replies = dq[i].replies;
    rq[i].skipped = dq[i].skipped;
    rq[i].bytes = dq[i].bytes;
    if (rc != PHIP_OK && rc != PHIP_ERR_SHORT_BUFFER) continue;
    const Member& mb = g->m[i];
    bool ok = hipSetDevice(mb.device) == hipSuccess &&
              hipMemcpy(rq[i].offs, dq[i].offs, ((size_t)dq[i].n + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && dq[i].bytes)
      ok = hipMemcpy(rq[i].out, dq[i].out, dq[i].bytes, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && dq[i].n && rq[i].src)
      ok = hipMemcpy(rq[i].src, dq[i].src, (size_t)dq[i].n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) {
      g->err = "member " + std::to_string(i) + ": copying the answers back failed";
      replies_zero(rq, nl);
      return PHIP_ERR_HIP;
    }
  }
  return rc;
}

}  // namespace

extern "C" {

int phip_group_unique_id(uint8_t* id) {
  if (!id) return PHIP_ERR_INVALID;
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return PHIP_ERR_RCCL;
  std::memcpy(id, u.internal, PHIP_GROUP_ID_BYTES);
  return PHIP_OK;
}

int phip_group_open_all(const phip_config* cfg, const int32_t* devices, uint32_t n,
                        phip_group** out) {
  if (!cfg || !devices || !out || n == 0 || n > 64) return PHIP_ERR_INVALID;
  *out = nullptr;
  phip_group* g = new phip_group;
  g->world = n;
  g->m.resize(n);
  std::vector<int> devs(devices, devices + n);
  for (u32 i = 0; i < n; ++i) {
    phip_config c = *cfg;
    c.device = devices[i];
    g->m[i].device = devices[i];
    g->m[i].rank = i;
    g->m[i].own = true;
    int rc = phip_open(&c, &g->m[i].h);
    if (rc) {
      destroy(g);
      return rc;
    }
  }
  // one device listed more than once: RCCL takes one rank per device, so the
  // members exchange by device copies (all of them on that one device)
  std::vector<int> sorted = devs;
  std::sort(sorted.begin(), sorted.end());
  const bool repeated = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
  if (repeated) {
    if (sorted.front() != sorted.back()) {   // mixed: some devices shared, some not
      destroy(g);
      return PHIP_ERR_INVALID;
    }
    g->shared = n > 1;
  } else {
    std::vector<ncclComm_t> comms(n);
    if (ncclCommInitAll(comms.data(), (int)n, devs.data()) != ncclSuccess) {
      destroy(g);
      return PHIP_ERR_RCCL;
    }
    for (u32 i = 0; i < n; ++i) g->m[i].comm = comms[i];
  }
  if (int rc = alloc_member_state(g)) {
    destroy(g);
    return rc;
  }
  *out = g;
  return PHIP_OK;
}

int phip_group_open_rank(phip_handle* h, const uint8_t* id, uint32_t nranks, uint32_t rank,
                         phip_group** out) {
  if (!h || !id || !out || nranks == 0 || nranks > 64 || rank >= nranks) return PHIP_ERR_INVALID;
  *out = nullptr;
  phip_group* g = new phip_group;
  g->world = nranks;
  g->m.resize(1);
  Member& mb = g->m[0];
  mb.h = h;
  mb.device = phip_host::handle_device(h);
  mb.rank = rank;
  ncclUniqueId u;
  std::memcpy(u.internal, id, PHIP_GROUP_ID_BYTES);
  if (hipSetDevice(mb.device) != hipSuccess ||
      ncclCommInitRank(&mb.comm, (int)nranks, u, (int)rank) != ncclSuccess) {
    mb.comm = nullptr;
    destroy(g);
    return PHIP_ERR_RCCL;
  }
  if (int rc = alloc_member_state(g)) {
    destroy(g);
    return rc;
  }
  *out = g;
  return PHIP_OK;
}

void phip_group_close(phip_group* g) {
  if (g) destroy(g);
}

const char* phip_group_last_error(const phip_group* g) { return g ? g->err.c_str() : "null group"; }
uint32_t phip_group_world(const phip_group* g) { return g ? g->world : 0; }
uint32_t phip_group_local(const phip_group* g) { return g ? (uint32_t)g->m.size() : 0; }
phip_handle* phip_group_handle(phip_group* g, uint32_t i) {
  return (g && i < g->m.size()) ? g->m[i].h : nullptr;
}

int phip_group_receive(phip_group* g, const phip_msgs* batches, int64_t now, uint64_t* sent,
                       uint64_t* merged, uint32_t flags) {
  if (!g || !batches || !(flags & PHIP_DEVICE_PTRS)) return PHIP_ERR_INVALID;
  return checked_call(
      g, batches, "message", [](Member&, hipStream_t, size_t) { return (int)PHIP_OK; },
      [&](size_t i, const phip_msgs& b) {
        return member_receive(g, g->m[i], MsgBatch{b, {}}, now, sent ? sent + i : nullptr,
                              merged ? merged + i : nullptr, flags);
      });
}

int phip_group_receive_datagrams(phip_group* g, const phip_wire* batches, int64_t now,
                                 uint64_t* sent, uint64_t* merged, uint32_t* stopped,
                                 uint32_t flags) {
  if (!g || !batches || !wire_flags_ok(flags)) return PHIP_ERR_INVALID;
  for (size_t i = 0; i < g->m.size(); ++i)
    if (batches[i].n && (!batches[i].bytes || !batches[i].offs)) return PHIP_ERR_INVALID;
  return receive_wire(g, batches, now, sent, merged, stopped, flags,
                      [](Member&, hipStream_t, size_t) { return (int)PHIP_OK; });
}

int phip_group_ring_receive(phip_group* g, phip_ring* const* rings, const uint32_t* slots,
                            int64_t now, uint64_t* sent, uint64_t* merged, uint32_t* stopped,
                            uint32_t flags) {
  if (!g || !rings || !slots || !wire_flags_ok(flags)) return PHIP_ERR_INVALID;
  return ring_receive(g, rings, slots, now, sent, merged, stopped, flags, nullptr);
}

// The replies forms (patrolhip.h "Group reply egress"): the call each is named
// after, with one Replies per local member travelling through member_receive.
int phip_group_receive_datagrams_replies(phip_group* g, const phip_wire* batches, int64_t now,
                                         uint64_t* sent, uint64_t* merged, uint32_t* stopped,
                                         phip_reply_egress* rq, uint32_t flags) {
  if (!g || !batches || !rq || !wire_flags_ok(flags)) return PHIP_ERR_INVALID;
  const size_t nl = g->m.size();
  replies_zero(rq, nl);
  for (size_t i = 0; i < nl; ++i)
    if (batches[i].n && (!batches[i].bytes || !batches[i].offs)) return PHIP_ERR_INVALID;
  if (!replies_ok(rq, nl, true)) return PHIP_ERR_INVALID;
  std::vector<Replies> reps = replies_of(rq, nl);
  const int rc = receive_wire(g, batches, now, sent, merged, stopped, flags,
                              [](Member&, hipStream_t, size_t) { return (int)PHIP_OK; }, &reps);
  return replies_done(rc, reps, rq);
}

int phip_group_receive_replies(phip_group* g, const phip_msgs* batches, int64_t now, uint64_t* sent,
                               uint64_t* merged, phip_reply_egress* rq, uint32_t flags) {
  if (!g || !batches || !rq || !wire_flags_ok(flags)) return PHIP_ERR_INVALID;
  const size_t nl = g->m.size();
  replies_zero(rq, nl);
  if (!replies_ok(rq, nl, true)) return PHIP_ERR_INVALID;
  std::vector<Replies> reps = replies_of(rq, nl);
  const int rc = checked_call(
      g, batches, "message", [](Member&, hipStream_t, size_t) { return (int)PHIP_OK; },
      [&](size_t i, const phip_msgs& b) {
        return member_receive(g, g->m[i], MsgBatch{b, {}}, now, sent ? sent + i : nullptr,
                              merged ? merged + i : nullptr, flags, &reps[i]);
      });
  return replies_done(rc, reps, rq);
}

int phip_group_ring_receive_replies(phip_group* g, phip_ring* const* rings, const uint32_t* slots,
                                    int64_t now, uint64_t* sent, uint64_t* merged,
                                    uint32_t* stopped, phip_reply_egress* rq, uint32_t flags) {
  if (!g || !rings || !slots || !rq || !wire_flags_ok(flags)) return PHIP_ERR_INVALID;
  replies_zero(rq, g->m.size());
  if (!replies_ok(rq, g->m.size(), false)) return PHIP_ERR_INVALID;
  return ring_receive(g, rings, slots, now, sent, merged, stopped, flags, rq);
}

int phip_group_reply_stats(phip_group* g, uint32_t i, uint64_t* out, int max) {
  if (!g || !out || i >= g->m.size()) return 0;
  const int n = std::min<int>(std::max(max, 0), RS_WORDS);
  for (int k = 0; k < n; ++k) out[k] = g->m[i].rstats[k];
  return n;
}

int phip_group_apply_mixed(phip_group* g, const phip_ops* batches, const phip_results* results,
                           uint64_t* sent, uint64_t* applied, uint32_t flags) {
  constexpr uint32_t kAllowed = PHIP_DEVICE_PTRS | PHIP_GROUP_RCCL_SELF | PHIP_GROUP_SMALL_CHUNKS;
  if (!g || !batches || !(flags & PHIP_DEVICE_PTRS) || (flags & ~kAllowed)) return PHIP_ERR_INVALID;
  const size_t nl = g->m.size();
  for (size_t i = 0; i < nl; ++i) {
    const phip_ops& b = batches[i];
    if (b.n && (!b.kind || !b.names || !b.name_offs || !b.now)) return PHIP_ERR_INVALID;
  }
  std::vector<phip_results> res(nl);   // (a NULL results: no column wanted)
  for (size_t i = 0; i < nl; ++i) res[i] = results ? results[i] : phip_results{};
  // Ops that are not applied report status 0: the status columns are zeroed
  // first, then the batches checked by phip_group_receive's rule.
  return checked_call(
      g, batches, "op",
      [&](Member& mb, hipStream_t st, size_t i) {
        if (res[i].status && batches[i].n)
          GHIP(mb, hipMemsetAsync(res[i].status, 0, batches[i].n, st));
        return (int)PHIP_OK;
      },
      [&](size_t i, const phip_ops& b) {
        return member_routed(g, g->m[i], b, OpsPath{res[i]}, sent ? sent + i : nullptr,
                             applied ? applied + i : nullptr, flags);
      });
}

int phip_group_peek(phip_group* g, const phip_ops* batches, const phip_peek_results* results,
                    uint64_t* sent, uint64_t* answered, uint32_t flags) {
  constexpr uint32_t kAllowed =
      PHIP_DEVICE_PTRS | PHIP_GROUP_RCCL_SELF | PHIP_GROUP_SMALL_CHUNKS | PHIP_GROUP_PEEK_STATE;
  if (!g || !batches || !(flags & PHIP_DEVICE_PTRS) || (flags & ~kAllowed)) return PHIP_ERR_INVALID;
  const size_t nl = g->m.size();
  std::vector<phip_peek_results> res(nl);   // (a NULL results: no column wanted)
  for (size_t i = 0; i < nl; ++i) {
    const phip_ops& b = batches[i];
    if (b.n && (!b.names || !b.name_offs || !b.now)) return PHIP_ERR_INVALID;
    res[i] = results ? results[i] : phip_peek_results{};
    // the state column travels only when every process asked for it
    if (res[i].state && !(flags & PHIP_GROUP_PEEK_STATE)) return PHIP_ERR_INVALID;
  }
  // Queries that are not answered report status 0 (phip_group_apply_mixed's rule).
  return checked_call(
      g, batches, "query",
      [&](Member& mb, hipStream_t st, size_t i) {
        if (res[i].status && batches[i].n)
          GHIP(mb, hipMemsetAsync(res[i].status, 0, batches[i].n, st));
        return (int)PHIP_OK;
      },
      [&](size_t i, const phip_ops& b) {
        return member_routed(g, g->m[i], b, PeekPath{res[i], (flags & PHIP_GROUP_PEEK_STATE) != 0},
                             sent ? sent + i : nullptr, answered ? answered + i : nullptr, flags);
      });
}

int phip_group_set_timing(phip_group* g, int on) {
  if (!g) return PHIP_ERR_INVALID;
  for (Member& mb : g->m) mb.tm.on = on != 0;
  return PHIP_OK;
}

int phip_group_stage_ms(phip_group* g, uint32_t i, float* ms) {
  if (!g || !ms || i >= g->m.size()) return PHIP_ERR_INVALID;
  Member& mb = g->m[i];
  if (hipSetDevice(mb.device) != hipSuccess) return PHIP_ERR_HIP;
  for (int s = 0; s < 3; ++s)
    if (mb.tm.sum(s, &ms[s]) != hipSuccess) return PHIP_ERR_HIP;
  return PHIP_OK;
}

int phip_group_rccl_info(phip_group* g, uint32_t i, int32_t* version, int32_t* comm_count,
                         char* lib_path, uint32_t path_cap) {
  if (!g || i >= g->m.size()) return PHIP_ERR_INVALID;
  const Member& mb = g->m[i];
  int v = 0;
  if (ncclGetVersion(&v) != ncclSuccess) return PHIP_ERR_RCCL;
  if (version) *version = v;
  int c = 0;
  if (mb.comm && ncclCommCount(mb.comm, &c) != ncclSuccess) return PHIP_ERR_RCCL;
  if (comm_count) *comm_count = c;
  if (lib_path && path_cap) {
    Dl_info di{};
    const char* p = dladdr((const void*)&ncclGetVersion, &di) && di.dli_fname ? di.dli_fname : "";
    std::snprintf(lib_path, path_cap, "%s", p);
  }
  return PHIP_OK;
}

int phip_group_anti_entropy(phip_group* g, int64_t* const* replicas, uint32_t nrep,
                            uint64_t nbuckets, uint32_t flags) {
  if (!g || !replicas || nrep == 0 || !(flags & PHIP_DEVICE_PTRS)) return PHIP_ERR_INVALID;
  if (nbuckets == 0) return PHIP_OK;
  return for_members(g, [&](size_t i) {
    return member_anti_entropy(g, g->m[i], replicas[i], nrep, nbuckets);
  });
}

// Eviction is local per shard (a bucket lives on its owner alone): every
// member sweeps its own table, with no exchange.
int phip_group_evict_idle(phip_group* g, int64_t now, int64_t idle_ns, uint64_t min_evict,
                          phip_evict_stats* out, uint32_t flags) {
  if (!g) return PHIP_ERR_INVALID;
  return for_members(g, [&](size_t i) {
    Member& mb = g->m[i];
    GHIP(mb, hipSetDevice(mb.device));
    GPHIP(mb, phip_evict_idle(mb.h, now, idle_ns, min_evict, out ? out + i : nullptr, flags));
    return (int)PHIP_OK;
  });
}

}  // extern "C"
