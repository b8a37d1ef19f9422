// libpatrolhip host orchestration: the C ABI of include/patrolhip.h.
//
// Pipelines:
//   fast receive  classify -> hot directory -> k_receive_fast
//                 -> [insert rounds -> k_receive_list(miss list)]
//   ordered       resolve -> [insert rounds -> resolve(miss)] -> sort(slot, seq)
//                 (ops packed to 32-byte records, kind in the sort value)
//                 -> run-length segments
//                 -> k_fold_thread / k_fold_wave / k_fold_block (stream2)
// Everything runs on the handle's own HIP stream; host synchronisation only
// reads back small counters (phip_kernels.hpp "counter words") between stages.
#include <sys/random.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "patrolhip.h"
#include "phip_kernels.hpp"
#include "phip_host.hpp"

using namespace phip;

namespace {

// The ordered path's (slot, seq) sort: slots have L <= 31 bits (25 for the
// C2/C3 tables), so 8-bit places spend a whole fourth pass on one bit; wider
// places (PHIP_SORT_BITS) cover 25 bits in three.
#ifndef PHIP_SORT_BITS
#define PHIP_SORT_BITS 9
#endif
#ifndef PHIP_SORT_BLOCK
#define PHIP_SORT_BLOCK 1024
#endif
#ifndef PHIP_SORT_ITEMS
#define PHIP_SORT_ITEMS 8
#endif
using SlotSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<
        rocprim::kernel_config<PHIP_SORT_BLOCK, PHIP_SORT_ITEMS>,
        rocprim::kernel_config<PHIP_SORT_BLOCK, PHIP_SORT_ITEMS>, PHIP_SORT_BITS,
        rocprim::block_radix_rank_algorithm::match>>;

enum BufId {
  B_NAMES, B_OFFS, B_A, B_T, B_E, B_KIND, B_NOW, B_FREQ, B_PER, B_COUNT,
  B_STATUS, B_REM, B_HAVE, B_REPLY,
  B_BYTES, B_DOFFS, B_NOFF, B_NLEN, B_DA, B_DT, B_DE,
  B_MISS, B_MISS2, B_RETRY, B_CSLOT, B_CMSG,
  B_SLOT, B_IDX, B_SSLOT, B_SIDX, B_USLOT, B_SCNT, B_SSTART, B_LONG, B_HUGE, B_TEMP, B_DUMP,
  B_OPS, B_HOFF, B_HOP, B_HVAL, B_RPOS, B_RST, B_RUNN, B_SEGEX, B_WOFF, B_SUMS, B_WRUN,
  B_WING, B_SEGXF, B_FOLDDBG, B_SMALL, B_HUGE2, B_LONG2,
  B_STATES, B_NAME1, B_HOT, B_ROUTE, B_EXPORT, B_MSHARD, B_MSCNT, B_FSCNT, B_DEDUP, B_DSET, B_TSTATS, B_SEGT, B_RHOT,
  B_DLIST, B_DTAB, B_DMARK, B_SMAP, B_SOFF, B_SLEN, B_SA, B_ST, B_SE, B_SSTAT, B_SREP, B_NCHK,
  B_EVICT, B_ULOG, B_ULCNT, B_SWEEP, B_DIGEST, B_DIGOUT,
  B_EGSZ, B_EGTILE, B_EGOUT, B_EGOFFS,
  B_PEEKAT, B_PEEKST, B_TOP,
  B_RQCTR, B_RQSEL, B_RQTILE, B_RQOUT, B_RQOFFS, B_RQSRC, B_RQSTAT, B_RQREP,
  B_FRAME, B_FRRECS, B_FRMAP,
  B_COUNT_
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct Timing {
  const char* name;
  hipEvent_t a, b;
};

// A fast Receive pass ("fast receive" below: what each kind enqueues).
enum class PassKind { kOptimistic, kClassified, kIsolating };
struct FastPass {
  PassKind kind = PassKind::kClassified;
  u32 n = 0;
  u32 par = 0;          // batch parity: its shard counters (fast_counts) and
  u32* c = nullptr;     // its counter set (fctr)
  const HotHdr* hot = nullptr;   // the hot directory (nullptr: none)
  const HotEntry* dir = nullptr;
  void* hot_zero = nullptr;   // the directory kernel's count tables, for the fast kernel to clear
  bool hot_join = false;      // the directory was built on stream2 (fast_back joins it)
  bool built = false;         // its front launched k_hot_dir
  u32 hot_age = 0;            // passes its directory served before this one (0: built for it)
  u32 hot_nw = 0;             // a kept directory's layout in the kernel (k_receive_fast's NW; 0: today's)
  // optimistic, queued behind a pass not settled yet: that pass's counter
  // set, the kernel's gate (nullptr: none); and whether the host, reading the
  // same words in that pass's mirror, found it shut (receive_queued)
  const u32* gate = nullptr;
  bool gate_shut = false;
  u8* fill = nullptr;   // optimistic, no k_hot_dir launch: the status column its back fills
  u8* mark = nullptr;   // isolating: the status column, or a cleared one (k_dirty_pass)
  UndoLog log{};        // optimistic: the undo log (cnt: set by the front; base, cap: by the back)
};

}  // namespace

struct phip_handle {
  int device = 0;
  int ncu = 256;             // compute units (persistent grid size)
  // The fast-pass policy: read by pass_kind alone, moved by apply_policy alone.
  // Dirty-bucket isolation (phip_kernels.hpp "Dirty buckets"): always
  // (PHIP_CFG_ISOLATE), or while iso_left > 0 -- kIsoKeep fast passes after
  // the last one that met a dirty message.
  bool iso_always = false;
  u32 iso_left = 0;
  // The optimistic pass (phip_kernels.hpp "The optimistic pass"): a decoded
  // batch of a pass that does not isolate runs without classification, unless
  // the handle was opened with PHIP_CFG_CLASSIFY_FIRST or one of its last
  // kOptBackoff fast passes overflowed its undo log (opt_left counts down).
  bool classify_first = false;
  u32 opt_left = 0;
  struct LastStats {   // phip_last_stats lays them out
    uint64_t hot_entries = 0, hot_hits = 0, misses = 0;   // last fast batch
    uint64_t ordered = 0;    // messages it sent through the ordered path
    uint64_t log_count = 0, log_over = 0;   // last optimistic pass: log entries, messages
                                            // that found the log full
    uint64_t hot_age = 0;     // passes the batch's directory served before it (FastPass::hot_age)
    uint64_t gate_shut = 0;   // the batch's first optimistic kernel found its gate shut
  } stats;
  // The kept hot directory (keep_take / keep_collect, beside apply_policy).
  // B_HOT holds two directory slots, built into alternately; `slot` is the one
  // built last.  An optimistic pass takes it without a build while the builds
  // agree, the hit fraction holds, it is young and no record has moved.
  struct HotKeep {
    void* base = nullptr;   // the B_HOT allocation the slots lie in
    u32 slot = 0;           // the slot built last
    bool have = false;      // `slot` holds a directory, built under `gen`
    u64 gen = 0;            // layout_gen at that build
    u32 served = 0;         // passes that took it, the one it was built for included
    // from the passes collected so far
    bool agree = false;     // the latest build collected: kept * 8 >= own * 7, own > 0
    u32 maxlen = ~0u;       // that build's longest selected name (kCtrHotMaxLen), in bytes
    u64 ref_hits = 0, ref_n = 0;   // that build's batch: messages folded, messages
    bool sagged = false;    // a pass collected since folded < 7/8 of ref_hits / ref_n
  } keep;
  hipStream_t stream = nullptr;      // the stream every call runs on (own_stream or the caller's)
  hipStream_t own_stream = nullptr;  // created by phip_open
  hipStream_t stream2 = nullptr;   // second stream: the hot-bucket fold overlaps the others
  hipStream_t stream3 = nullptr;   // third stream: the other huge segments beside the largest
  // fourth stream: the thread folds beside the wave folds, created by the
  // first ordered batch that folds (a stream created at open would shift how
  // a process's later streams, e.g. a group's pack and exchange streams, map
  // onto its hardware queues: the bench's c4 leg took 8.3 instead of 6.9 ms)
  hipStream_t stream4 = nullptr;
  hipEvent_t ev_t4a = nullptr, ev_t4b = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // The B_HOT allocation whose count tables are zero, or will be when the
  // launches queued so far have run (build_hot, fast_back); nullptr: not so.
  void* hot_clean = nullptr;
  hipEvent_t ev_fork3 = nullptr, ev_join3 = nullptr;
  hipEvent_t ev_gather = nullptr, ev_gather3 = nullptr;   // huge-segment gathers done
  hipEvent_t ev_pack = nullptr;   // ordered path: op records packed (stream2)
  std::mutex mu;
  std::string err;
  u32 L = 0;
  u32 L_open = 0;            // log2_slots at phip_open: phip_evict_idle shrinks no further
  u64 cap = 0;
  u64 max_load = 0;
  u32 load_pct = 90;
  bool grow = true;          // !PHIP_CFG_NO_GROW
  bool small = true;         // !PHIP_CFG_NO_SMALL
  u64 grows = 0;             // table rehashes so far
  // layout generation: bumped by everything that moves, removes or re-seeds a
  // record or an arena name -- wherever the slot array is replaced or reloaded:
  //   grow_table (k_rehash into a new array),
  //   phip_evict_idle's move (k_evict_move: idle records dropped, the rest and
  //     their arena names placed anew),
  //   phip_restore (array and arena overwritten by the image).
  // Nothing else writes Rec::tag or the name words of a published record:
  // k_claim / k_publish and k_small_mixed's inserts claim empty slots and
  // append to the arena (phip_seed goes through them), k_clear_new* and the
  // dirty marks touch the flags byte only.  A sweep cursor (phip_export_sweep)
  // made under another value starts over, and a kept hot directory
  // (HotKeep::gen) is dropped.  Never 0, the value of a zeroed cursor.
  u64 layout_gen = 1;
  u64 long_need = 0;         // arena bytes the last reserve() counted
  Rec* recs = nullptr;
  u32* aux = nullptr;
  // PHIP_CFG_TRACK_CHANGES: the change set (phip_kernels.hpp "change set"), two
  // bit sets of mark_words(cap) words in one allocation, allocated, replaced
  // and freed with the table; null pointers on a handle that keeps none
  bool track = false;
  Marks marks{};
  // PHIP_CFG_TRACK_USAGE: the usage baseline (phip_kernels.hpp "top talkers"),
  // one u64 per slot, allocated, replaced and freed where the marks are; null
  // on a handle that keeps none
  bool usage = false;
  u64* base = nullptr;
  u8* arena = nullptr;
  u64 arena_cap = 0;
  u64 arena_open = 0;        // arena bytes at phip_open: a compacted arena is no smaller
  u64* arena_cursor = nullptr;
  u32* ctr = nullptr;        // device counters: kCtrWords general, then two fast-pass sets (fctr)
  // pinned mirror: kCtrWords of the general set, then kCtrWords per fast-pass
  // set (fmirror) -- a queued pass's successor is enqueued before the host
  // reads the pass's counters, and stores its own beside them
  u32* ctr_host = nullptr;
  u32* ctr_map = nullptr;    // ctr_host as the device sees it (k_shard_scan stores there)
  u32 fpar = 0;              // parity of the last fast batch (its shard counters in B_FSCNT)
  u64 nfast = 0;             // fast passes begun (a queued front is redone after a nested one)
  u64 n_buckets = 0;
  u64 tag_mask = ~0ull;
  u64 seed = 0;              // placement seed (Table::home, seeded_mix)
  DevBuf buf[B_COUNT_];
  bool timing = false;
  bool timing_accumulate = false;   // phip_set_timing(h, 2): keep every call's timings
  std::vector<Timing> timings;
  std::vector<Timing> event_pool;
  size_t pool_used = 0;
  u8* small_pin = nullptr;   // pinned staging of small ordered batches (both ways)
  size_t small_pin_cap = 0;
  // PHIP_RECV_ASYNC: a decoded batch whose fast pass is queued; its counters
  // are read, and its misses / dirty buckets finished, at the handle's next
  // call (or phip_flush)
  struct Pending {
    bool active = false;
    SoaIn<NamesOffs> in{};
    i64 now = 0;
    OutView ow{};
    FastPass pass{};   // its queued pass (front and back enqueued)
  } pend;
  hipEvent_t ev_ctr[2] = {nullptr, nullptr};   // a batch's counters reached its mirror (by parity)
  int deferred_rc = 0;   // a queued batch's error met by a call that returns no status
};

namespace {

int set_err(phip_handle* h, int code, const char* fmt, ...) {
  char tmp[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(tmp, sizeof tmp, fmt, ap);
  va_end(ap);
  if (h) h->err = tmp;
  return code;
}

#define HIPCHK(h, x)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      return set_err((h), PHIP_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                 \
  } while (0)

template <class T>
int ensure(phip_handle* h, BufId id, size_t count, T** out) {
  size_t bytes = std::max<size_t>(count * sizeof(T), 64) + 64;  // +64: 8-byte over-read slack
  DevBuf& b = h->buf[id];
  if (b.cap < bytes) {
    size_t want = std::max(bytes, b.cap * 3 / 2);
    if (b.p) HIPCHK(h, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    HIPCHK(h, hipMalloc(&b.p, want));
    b.cap = want;
  }
  *out = (T*)b.p;
  return PHIP_OK;
}

inline Table table(phip_handle* h) {
  Table t;
  t.recs = h->recs;
  t.aux = h->aux;
  t.arena = h->arena;
  t.L = h->L;
  t.tag_mask = h->tag_mask;
  t.seed = h->seed;
  return t;
}

inline unsigned grid_for(u64 n, unsigned block = kBlock) {
  return (unsigned)std::max<u64>(1, (n + block - 1) / block);
}

// Event-timed launch helper (the pool entry is held by index: a nested
// Launch may grow the pool).
struct Launch {
  phip_handle* h;
  const char* name;
  size_t idx = ~size_t(0);
  hipStream_t s;
  Launch(phip_handle* h_, const char* n, hipStream_t st = nullptr)
      : h(h_), name(n), s(st ? st : h_->stream) {
    if (!h->timing) return;
    if (h->pool_used == h->event_pool.size()) {
      Timing tm{n, nullptr, nullptr};
      if (hipEventCreate(&tm.a) != hipSuccess) return;
      if (hipEventCreate(&tm.b) != hipSuccess) {
        (void)hipEventDestroy(tm.a);
        return;
      }
      h->event_pool.push_back(tm);
    }
    idx = h->pool_used++;
    h->event_pool[idx].name = n;
    if (hipEventRecord(h->event_pool[idx].a, s) != hipSuccess) idx = ~size_t(0);
  }
  ~Launch() {
    if (idx < h->event_pool.size()) {
      Timing& t = h->event_pool[idx];
      if (hipEventRecord(t.b, s) == hipSuccess) h->timings.push_back(t);
    }
  }
};

// Device counters (phip_kernels.hpp "counter words"): the general set to the
// host's mirror.
int read_ctr(phip_handle* h) {
  HIPCHK(h, hipMemcpyAsync(h->ctr_host, h->ctr, kCtrWords * sizeof(u32), hipMemcpyDeviceToHost,
                           h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int reset_ctr(phip_handle* h) {
  k_batch_reset<<<1, kShards, 0, h->stream>>>(h->ctr, nullptr);
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// (c: the mirror read -- the general set's, or a fast pass's own)
int check_flags(phip_handle* h, const u32* c) {
  if (c[kCtrBadName])
    return set_err(h, PHIP_ERR_INVALID, "malformed name offsets (names_len check): nothing applied");
  if (c[kCtrTableFull]) return set_err(h, PHIP_ERR_FULL, "hash table full (probe wrapped)");
  if (c[kCtrArenaFull]) return set_err(h, PHIP_ERR_ARENA, "long-name arena exhausted");
  return PHIP_OK;
}
int check_flags(phip_handle* h) { return check_flags(h, h->ctr_host); }

// A stats call's words into the caller's array of `max`; returns how many.
template <int N>
int copy_words(const uint64_t (&v)[N], uint64_t* out, int max) {
  int k = 0;
  for (; k < max && k < N; ++k) out[k] = v[k];
  return k;
}

// Every entry point binds the handle's device first: Go goroutines migrate
// across OS threads, and the HIP current device is per thread.
int finish_pending(phip_handle* h, bool* worked = nullptr, bool* shut = nullptr);
int after_error(phip_handle* h, int rc);

// (finish_queued: a batch PHIP_RECV_ASYNC queued is finished first, and its
// error is this call's)
int begin_call(phip_handle* h, bool finish_queued = true) {
  if (h->deferred_rc) {   // (phip_len / phip_capacity finished a queued batch that failed)
    const int rc = h->deferred_rc;
    h->deferred_rc = 0;
    return rc;
  }
  h->err.clear();
  if (h->timing && !h->timing_accumulate) {
    h->timings.clear();
    h->pool_used = 0;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (finish_queued && h->pend.active) {
    int rc = finish_pending(h);
    if (rc) return after_error(h, rc);
  }
  return PHIP_OK;
}

// Copy a host array into a device staging buffer (or pass device pointers).
template <class T>
int stage(phip_handle* h, BufId id, const T* src, size_t count, bool dev, const T** out) {
  if (!src) { *out = nullptr; return PHIP_OK; }
  if (dev) { *out = src; return PHIP_OK; }
  T* d;
  int rc = ensure(h, id, count, &d);
  if (rc) return rc;
  if (count) HIPCHK(h, hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  *out = d;
  return PHIP_OK;
}

template <class T>
int out_buf(phip_handle* h, BufId id, T* user, size_t count, bool dev, T** out) {
  if (!user) { *out = nullptr; return PHIP_OK; }
  if (dev) { *out = user; return PHIP_OK; }
  return ensure(h, id, count, out);
}

template <class T>
int copy_back(phip_handle* h, T* user, const T* dev_buf, size_t count, bool dev) {
  if (!user || dev || !count) return PHIP_OK;
  HIPCHK(h, hipMemcpyAsync(user, dev_buf, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return PHIP_OK;
}

// ---- datagram outputs (sweep, change set, reply egress, batch egress) ----
// The output arguments of a call that writes datagrams and an offsets column,
// checked before anything is applied; `what` starts the message.  *budget:
// the bytes the datagrams may take (a device buffer keeps 8 bytes of slack for
// the whole-word stores).
int datagram_args(phip_handle* h, const char* what, const uint8_t* out, uint64_t out_cap,
                  const uint64_t* offs, uint32_t max_msgs, bool dev, u64* budget) {
  if (!out || !offs) return set_err(h, PHIP_ERR_INVALID, "%s: out and offs are required", what);
  if (!max_msgs) return set_err(h, PHIP_ERR_INVALID, "%s: max_msgs must be positive", what);
  if (out_cap < PHIP_BUCKET_PACKET_SIZE)
    return set_err(h, PHIP_ERR_INVALID, "%s: out_cap below one datagram (%d bytes)", what,
                   PHIP_BUCKET_PACKET_SIZE);
  if (dev && ((reinterpret_cast<uintptr_t>(out) & 7) || (out_cap & 7) ||
              out_cap < PHIP_BUCKET_PACKET_SIZE + 8))
    return set_err(h, PHIP_ERR_INVALID,
                   "%s: a device buffer is 8-byte aligned, a multiple of 8 and >= %d bytes", what,
                   PHIP_BUCKET_PACKET_SIZE + 8);
  *budget = dev ? out_cap - 8 : out_cap;
  return PHIP_OK;
}

// A host-pointer call gets back only what was written: `bytes` bytes of
// datagrams and n + 1 offsets, staging to caller, on the handle's stream (the
// caller synchronises).
int datagrams_back(phip_handle* h, uint8_t* out, const u8* d_out, u64 bytes, uint64_t* offs,
                   const u64* d_offs, u64 n) {
  if (bytes) HIPCHK(h, hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(offs, d_offs, (n + 1) * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
  return PHIP_OK;
}

// No datagrams: offs[0] = 0, a device pointer's on the stream (sync: no
// synchronise of the caller's follows).
int datagrams_none(phip_handle* h, uint64_t* offs, bool dev, bool sync) {
  if (!dev) {
    offs[0] = 0;
    return PHIP_OK;
  }
  HIPCHK(h, hipMemsetAsync(offs, 0, sizeof(u64), h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

// ----------------------------------------------------------- inserts -----
inline u64 load_limit(u64 cap, u32 pct) { return cap * pct / 100; }

// The change set of a table of `cap` slots: words per set, and a cleared pair
// of sets (one allocation, freed through Marks::state) enqueued on the stream.
inline u64 mark_words(u64 cap) { return std::max<u64>(cap / 32, 1); }
int alloc_marks(phip_handle* h, u64 cap, Marks* out) {
  const u64 w = mark_words(cap);
  u32* p = nullptr;
  if (hipMalloc(&p, 2 * w * sizeof(u32)) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(h, PHIP_ERR_FULL, "change set of %llu slots: device memory", (unsigned long long)cap);
  }
  if (hipMemsetAsync(p, 0, 2 * w * sizeof(u32), h->stream) != hipSuccess) {
    (void)hipFree(p);
    return set_err(h, PHIP_ERR_HIP, "change set: clearing failed");
  }
  *out = Marks{p, p + w};
  return PHIP_OK;
}
// The usage baseline of a table of `cap` slots, cleared (+0.0) on the stream.
int alloc_base(phip_handle* h, u64 cap, u64** out) {
  u64* p = nullptr;
  if (hipMalloc(&p, cap * sizeof(u64)) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(h, PHIP_ERR_FULL, "usage baseline of %llu slots: device memory",
                   (unsigned long long)cap);
  }
  if (hipMemsetAsync(p, 0, cap * sizeof(u64), h->stream) != hipSuccess) {
    (void)hipFree(p);
    return set_err(h, PHIP_ERR_HIP, "usage baseline: clearing failed");
  }
  *out = p;
  return PHIP_OK;
}

// Rehash the table into 2^newL slots (k_rehash).  Both tables are resident
// while records move; the old one is freed after.
int grow_table(phip_handle* h, u32 newL) {
  const u64 ncap = 1ull << newL;
  Rec* nrecs = nullptr;
  u32* naux = nullptr;
  Marks nmarks{};
  u64* nbase = nullptr;
  if (hipMalloc(&nrecs, ncap * sizeof(Rec)) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(h, PHIP_ERR_FULL, "table growth to 2^%u slots: device memory", newL);
  }
  if (hipMalloc(&naux, ncap * sizeof(u32)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(nrecs);
    return set_err(h, PHIP_ERR_FULL, "table growth to 2^%u slots: device memory", newL);
  }
  // from here on an error frees the new table (the old one stays live)
  auto drop_new = [&](int rc) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(nrecs);
    (void)hipFree(naux);
    if (nmarks.state) (void)hipFree(nmarks.state);
    if (nbase) (void)hipFree(nbase);
    return rc;
  };
  if (h->track)
    if (int rc = alloc_marks(h, ncap, &nmarks)) return drop_new(rc);
  if (h->usage)
    if (int rc = alloc_base(h, ncap, &nbase)) return drop_new(rc);
  if (hipMemsetAsync(nrecs, 0, ncap * sizeof(Rec), h->stream) != hipSuccess ||
      hipMemsetAsync(naux, 0, ncap * sizeof(u32), h->stream) != hipSuccess ||
      hipMemsetAsync(h->ctr + kCtrTableFull, 0, sizeof(u32), h->stream) != hipSuccess)
    return drop_new(set_err(h, PHIP_ERR_HIP, "table growth: clearing the new table failed"));
  Table nt = table(h);
  nt.recs = nrecs;
  nt.aux = naux;
  nt.L = newL;
  {
    Launch l(h, "k_rehash");
    k_rehash<<<grid_for(h->cap), kBlock, 0, h->stream>>>(h->recs, h->aux, h->cap, nt, h->ctr,
                                                         h->marks, nmarks, h->base, nbase);
  }
  if (hipGetLastError() != hipSuccess)
    return drop_new(set_err(h, PHIP_ERR_HIP, "k_rehash launch failed"));
  int rc;
  if ((rc = read_ctr(h))) return drop_new(rc);   // synchronises: the old table is no longer read
  if (h->ctr_host[kCtrTableFull])
    return drop_new(set_err(h, PHIP_ERR_INVALID, "internal: rehash probe wrapped"));
  HIPCHK(h, hipFree(h->recs));
  HIPCHK(h, hipFree(h->aux));
  if (h->marks.state) HIPCHK(h, hipFree(h->marks.state));
  if (h->base) HIPCHK(h, hipFree(h->base));
  h->recs = nrecs;
  h->aux = naux;
  h->marks = nmarks;
  h->base = nbase;
  h->L = newL;
  h->cap = ncap;
  h->max_load = load_limit(ncap, h->load_pct);
  ++h->grows;
  ++h->layout_gen;
  return PHIP_OK;
}

int grow_arena(phip_handle* h, u64 used, u64 want) {
  u64 ncap = std::max<u64>(h->arena_cap * 2, want);
  u8* na = nullptr;
  if (hipMalloc(&na, ncap + 64) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(h, PHIP_ERR_ARENA, "arena growth to %llu bytes: device memory",
                   (unsigned long long)ncap);
  }
  if (used) HIPCHK(h, hipMemcpyAsync(na, h->arena, used, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipFree(h->arena));
  h->arena = na;
  h->arena_cap = ncap;
  return PHIP_OK;
}

// Room for `bound` more buckets and the long names of list[0..nlist), before
// any of them is claimed: grow the table / arena, or refuse with nothing
// claimed.  *grew is set when the table was rehashed (slot numbers changed).
template <class Src>
int reserve(phip_handle* h, Src src, const u32* list, u32 nlist, u64 bound, bool* grew) {
  u64* lb = (u64*)(h->ctr + kCtrLongBytes);
  HIPCHK(h, hipMemsetAsync(lb, 0, sizeof(u64), h->stream));
  k_list_long_bytes<Src><<<grid_for(nlist), kBlock, 0, h->stream>>>(src, nlist, list, lb);
  HIPCHK(h, hipGetLastError());
  u64 used = 0;
  HIPCHK(h, hipMemcpyAsync(&used, h->arena_cursor, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
  int rc;
  if ((rc = read_ctr(h))) return rc;
  u64 need;
  std::memcpy(&need, h->ctr_host + kCtrLongBytes, sizeof need);
  h->long_need = need;
  if (used + need > h->arena_cap) {
    if (!h->grow)
      return set_err(h, PHIP_ERR_ARENA, "long-name arena: %llu of %llu bytes used, %llu more needed",
                     (unsigned long long)used, (unsigned long long)h->arena_cap,
                     (unsigned long long)need);
    if ((rc = grow_arena(h, used, used + need))) return rc;
  }
  if (h->n_buckets + bound > h->max_load) {
    u32 L = h->L;
    while (L < 31 && h->n_buckets + bound > load_limit(1ull << L, h->load_pct)) ++L;
    if (!h->grow || h->n_buckets + bound > load_limit(1ull << L, h->load_pct))
      return set_err(h, PHIP_ERR_FULL,
                     "table load limit: %llu buckets + up to %llu new > %llu allowed in 2^%u slots",
                     (unsigned long long)h->n_buckets, (unsigned long long)bound,
                     (unsigned long long)(h->grow ? load_limit(1ull << L, h->load_pct) : h->max_load),
                     h->grow ? L : h->L);
    if ((rc = grow_table(h, L))) return rc;
    *grew = true;
  }
  return PHIP_OK;
}

// Insert every name of `list` (all known to be absent) into the table, after
// reserve() made room for all of them.  Claimed slots are accumulated in
// B_CSLOT/B_CMSG; *n_claimed returns their count (callers clear the NEW flag
// once done).  Every claimed slot is published before an error returns, so a
// failing round leaves no claimed-but-unnamed slot behind.
template <class Src>
int dedupe_names(phip_handle* h, Src src, const u32* list, u32 n, u32** out, u32* nout);

// `distinct`: the list holds each name once (a k_dedupe output); otherwise a
// name may be listed many times (a fast batch's misses), and a list whose
// length alone would pass the load limit is bounded by its distinct names
// first, so that one new hot name does not grow (or, without growth, fill)
// the table for the thousands of messages naming it.
template <class Src>
int insert_names(phip_handle* h, Src src, u32* list, u32 nlist, const int64_t* now_arr, i64 now0,
                 u32* n_claimed, bool* grew = nullptr, bool distinct = false) {
  u32 *cslot, *cmsg, *retry, *cur = list;
  int rc;
  *n_claimed = 0;
  bool g = false;
  u64 bound = nlist;
  // the names whose long-name arena bytes reserve() counts: the list, or its
  // distinct names once they are known (one new long hot name listed by
  // 65535 misses needs its bytes once)
  const u32* blist = list;
  u32 nb = nlist;
  if (!distinct && nlist > 1 && h->n_buckets + nlist > h->max_load) {
    u32 *dd, nd = 0;
    if ((rc = dedupe_names(h, src, list, nlist, &dd, &nd))) return rc;
    // names that share a 64-bit tag count once there: with full tags that is
    // a birthday rarity; narrowed test tags keep the list's length (and the
    // bytes of every listed name)
    if (h->tag_mask == ~0ull) {
      bound = nd;
      blist = dd;
      nb = nd;
    }
  }
  if ((rc = reserve(h, src, blist, nb, bound, &g))) return rc;
  if (grew) *grew = g;
  if ((rc = ensure(h, B_CSLOT, nlist, &cslot)) || (rc = ensure(h, B_CMSG, nlist, &cmsg)) ||
      (rc = ensure(h, B_RETRY, nlist, &retry)))
    return rc;
  u32 total = 0, ncur = nlist;
  // kCtrClaimed counts this call's claims (B_CSLOT/B_CMSG positions): a batch
  // can run the pipeline twice (finish_many_misses, resolve_all), so it starts
  // from zero here, not at the batch's reset_ctr.
  HIPCHK(h, hipMemsetAsync(h->ctr + kCtrClaimed, 0, sizeof(u32), h->stream));
  // Swap buffers between rounds: round k reads `cur`, writes retries to `nxt`.
  u32* nxt = retry;
  u32* spare = nullptr;
  if ((rc = ensure(h, B_MISS2, nlist, &spare))) return rc;
  // Every round claims at least one slot while names are pending (a pending
  // name met a slot claimed in that same round), so this terminates; with a
  // 64-bit tag a second round is already rare.
  while (ncur > 0) {
    HIPCHK(h, hipMemsetAsync(h->ctr + kCtrRetry, 0, sizeof(u32), h->stream));
    {
      Launch l(h, "k_claim");
      k_claim<Src><<<grid_for(ncur), kBlock, 0, h->stream>>>(src, ncur, cur, table(h), cslot, cmsg,
                                                              nxt, h->ctr);
    }
    HIPCHK(h, hipGetLastError());
    if ((rc = read_ctr(h))) return rc;
    u32 claimed_total = h->ctr_host[kCtrClaimed];   // (cumulative over the rounds)
    u32 fresh = claimed_total - total;
    // The round's claims are published before any error is reported.
    if (fresh) {
      Launch l(h, "k_publish");
      k_publish<Src><<<grid_for(fresh), kBlock, 0, h->stream>>>(
          src, total, fresh, cslot, cmsg, table(h), h->arena, h->arena_cap, h->arena_cursor, now_arr,
          now0, h->ctr);
    }
    HIPCHK(h, hipGetLastError());
    h->n_buckets += fresh;
    total = claimed_total;
    *n_claimed = total;
    ncur = h->ctr_host[kCtrRetry];
    if ((rc = check_flags(h))) return rc;
    if (fresh == 0 && ncur != 0)
      return set_err(h, PHIP_ERR_INVALID, "internal: insert round made no progress");
    // next round reads the retries
    cur = nxt;
    nxt = (nxt == retry) ? spare : retry;
  }
  *n_claimed = total;
  // An arena overflow would show only in the last publish's flags (it cannot
  // happen after reserve(); checked all the same when long names were inserted).
  if (h->long_need) {
    if ((rc = read_ctr(h)) || (rc = check_flags(h))) return rc;
  }
  return PHIP_OK;
}

int clear_new(phip_handle* h, u32 n_claimed) {
  if (!n_claimed) return PHIP_OK;
  u32* cslot = (u32*)h->buf[B_CSLOT].p;
  Launch l(h, "k_clear_new");
  k_clear_new<<<grid_for(n_claimed), kBlock, 0, h->stream>>>(cslot, n_claimed, table(h));
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// After a failed batch: no slot may keep the NEW flag (the ordered fold reads
// it as "GetBucket is creating this bucket", phip_kernels.hpp load_state),
// whichever insert call of the batch claimed it.  Returns rc.
int after_error(phip_handle* h, int rc) {
  if (rc == PHIP_OK) return rc;
  // Nothing of the failed call may still run when it returns: the side
  // streams (the hot directory of a batch whose front was queued, the
  // ordered path's folds) may still read the caller's inputs.
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  if (h->stream3) (void)hipStreamSynchronize(h->stream3);
  if (h->stream4) (void)hipStreamSynchronize(h->stream4);
  if (rc == PHIP_ERR_HIP) return rc;
  std::string keep = h->err;
  k_clear_new_all<<<grid_for(h->cap), kBlock, 0, h->stream>>>(table(h), h->cap);
  if (hipGetLastError() == hipSuccess) (void)hipStreamSynchronize(h->stream);
  h->err = keep;
  return rc;
}

// ------------------------------------------------------- fast receive ----
// Hot directory of a fast batch (phip_kernels.hpp k_hot_dir): one launch on
// `st`, no host round trip.  Sets the pass's header/directory to hand to
// k_receive_fast (left nullptr: none) and its hot_zero, the kernel's count
// tables and sync words, which have to be zero at its next launch: the fast
// kernel that takes the directory clears them (fast_back).  Only a buffer just
// created, or one whose directory no fast kernel took, is cleared in front.
// B_HOT: those tables, the candidate list, then two {HotHdr, HotEntry[kHotMaxExt]}
// slots built into alternately (HotKeep), so that the kernel's last workgroup
// reads the directory before while it writes the new one.
// status: nothing runs beside the kernel (an optimistic batch): one sample
// per lane, up to kHotSampleMaxAlone of them, and further workgroups fill the
// batch's status column; nullptr: it shares the chip with k_classify, which
// writes the statuses, and takes up to kHotSampleMax.
constexpr size_t kHotSlotBytes = sizeof(HotHdr) + kHotMaxExt * sizeof(HotEntry);
constexpr size_t kHotSlotsAt = kHotZeroBytes + kHotDirCandMax * sizeof(u32);
template <class Src>
int build_hot(phip_handle* h, Src src, u32 n, hipStream_t st, u8* status, FastPass* p) {
  if (n < kHotMinBatch) return PHIP_OK;
  constexpr size_t kCnt = size_t(1) << kHotDirCntBits;
  u8* base;
  int rc;
  if ((rc = ensure(h, B_HOT, kHotSlotsAt + 2 * kHotSlotBytes, &base))) return rc;
  u32* ckeys = (u32*)base;
  u32* ccnt = ckeys + kCnt;
  u32* sync = ccnt + kCnt;
  u32* cand = sync + kHotSyncWords;
  u8* slots = base + kHotSlotsAt;
  constexpr size_t kSlot = kHotSlotBytes;
  // The slot not built last; the one built last, while it still describes the
  // table, is the directory the kernel's agreement sums compare with.
  phip_handle::HotKeep& kp = h->keep;
  // (only an optimistic pass's build is asked whether it agrees)
  const bool prev = p->kind == PassKind::kOptimistic && kp.have && kp.base == base &&
                    kp.gen == h->layout_gen;
  const HotHdr* phdr = prev ? (const HotHdr*)(slots + kp.slot * kSlot) : nullptr;
  kp.slot = kp.base == base ? kp.slot ^ 1u : 0u;
  kp.base = base;
  kp.have = true;
  kp.gen = h->layout_gen;
  kp.served = 1;
  HotHdr* hdr = (HotHdr*)(slots + kp.slot * kSlot);
  HotEntry* dir = (HotEntry*)(hdr + 1);
  if (h->hot_clean != base) HIPCHK(h, hipMemsetAsync(base, 0, kHotZeroBytes, st));
  h->hot_clean = nullptr;
  const u32 smax = status ? kHotSampleMaxAlone : kHotSampleMax;
  const u32 stride = std::max<u32>(64, (n + smax - 1) / smax);
  const u32 nsample = (n + stride - 1) / stride;
  {
    Launch l(h, "k_hot_dir", st);
    if (status) {
      // (fill workgroups: 64 bytes of statuses a lane and pass, 1024 lanes
      // resident a compute unit)
      constexpr unsigned kT = kHotAloneThreads;
      const unsigned nblk = grid_for(nsample, kT);
      const unsigned fill =
          std::min<unsigned>(grid_for(n, kT * 64), 1024 / kT * (unsigned)h->ncu);
      k_hot_dir<Src, kT, 1><<<nblk + fill, kT, 0, st>>>(
          src, n, stride, nsample, table(h), ckeys, ccnt, sync, cand, hdr, dir, nblk, status, phdr,
          phdr ? (const HotEntry*)(phdr + 1) : nullptr, p->c);
    } else {
      const unsigned nblk = grid_for(nsample, kHotSamplePerBlock);
      k_hot_dir<Src, 256, 4><<<nblk, 256, 0, st>>>(
          src, n, stride, nsample, table(h), ckeys, ccnt, sync, cand, hdr, dir, nblk, nullptr, phdr,
          phdr ? (const HotEntry*)(phdr + 1) : nullptr, p->c);
    }
  }
  HIPCHK(h, hipGetLastError());
  p->hot = hdr;
  p->dir = dir;
  p->hot_zero = base;
  p->built = true;
  return PHIP_OK;
}

inline unsigned fast_grid_on(u32 ncu, u32 n) {
  const u64 tiles = ((u64)n + kFastBlock - 1) / kFastBlock;
  return (unsigned)std::max<u64>(1, std::min<u64>(tiles, (u64)ncu * kFastPerCU));
}
inline unsigned fast_grid(phip_handle* h, u32 n) { return fast_grid_on((u32)h->ncu, n); }


// A sharded append list over `units` units of up to `per_unit` entries
// (counters zeroed on the stream).
int sharded(phip_handle* h, BufId base_id, u32 units, u32 per_unit, Sharded* out,
            bool zero = true) {
  int rc;
  out->cap = shard_cap(units, per_unit);
  if ((rc = ensure(h, base_id, (size_t)kShards * out->cap, &out->base)) ||
      (rc = ensure(h, B_MSCNT, 2 * kShards, &out->cnt)))
    return rc;
  if (zero) HIPCHK(h, hipMemsetAsync(out->cnt, 0, kShards * sizeof(u32), h->stream));
  return PHIP_OK;
}

// Pack a sharded list into `out`: the total lands in ctr[total_slot] and is
// returned in *total (one counter read-back).
int pack_sharded(phip_handle* h, const Sharded& sh, u32 total_slot, u32* out, u32* total) {
  k_shard_scan<<<1, kShards, 0, h->stream>>>(sh.cnt, h->ctr, total_slot, nullptr, 0, nullptr,
                                             nullptr, nullptr);
  HIPCHK(h, hipGetLastError());
  int rc;
  if ((rc = read_ctr(h))) return rc;
  *total = h->ctr_host[total_slot];
  if (*total) {
    Launch l(h, "k_shard_compact");
    dim3 grid(grid_for(h->ctr_host[kCtrShardMax]), kShards);
    k_shard_compact<<<grid, 256, 0, h->stream>>>(sh.base, sh.cap, sh.cnt, out);
    HIPCHK(h, hipGetLastError());
  }
  return PHIP_OK;
}

// A fast batch in three parts, so that a queued batch (PHIP_RECV_ASYNC) can
// put the next batch's front in front of its own read-back:
// fast_begin (the front: parity, counter set, k_batch_reset, then by kind),
// fast_back (the fast kernel, which clears the directory's count tables for
// the next batch, then the launch that packs the miss shards' offsets and
// stores the counters in the host's mapped mirror -- queued: and resets the
// next batch's -- with ev_ctr behind it) and fast_settle (the counters read:
// a failed speculation run again, the policy moved, the pass collected).
//   kind        front, main stream but marked    back, main stream
//   optimistic  k_hot_dir with the status fill   k_receive_fast<Opt>, k_shard_scan
//               (a kept directory: nothing)      (then the kernel fills the column)
//   classified  k_classify (fills the column),   k_receive_fast, k_shard_scan
//               k_hot_dir on stream2
//   isolating   as classified                    k_dirty_build, k_receive_fast,
//                                                k_dirty_pass, k_batch_end
// The miss list's shard counters alternate between two sets by batch parity
// (B_FSCNT): the next batch's front resets its own set while the batch
// before still has to pack its list from the other.

// What a caller asks of a pass: the handle's policy; the policy, and it may be
// optimistic (the caller can undo it: a decoded batch's first pass); or isolation
// forced on or off (finish_many_misses' nested pass, as the pass it finishes ran).
enum class PassAsk { kPolicy, kMayUndo, kIsolate, kNoIsolate };

// The one place that decides what a pass is.  Wire input is never optimistic.
template <class In>
PassKind pass_kind(const phip_handle* h, PassAsk ask) {
  if (ask == PassAsk::kIsolate) return PassKind::kIsolating;
  if (ask == PassAsk::kNoIsolate) return PassKind::kClassified;
  if (h->iso_always || h->iso_left > 0) return PassKind::kIsolating;
  if (ask == PassAsk::kMayUndo && In::kSoa && !h->classify_first && h->opt_left == 0)
    return PassKind::kOptimistic;
  return PassKind::kClassified;
}

// The per-wave entry counts of an optimistic pass's log, sized for the
// largest grid.  No reset: every wave of the pass stores its count, and a
// queued batch's kernel runs only after the batch before is collected (and,
// if it failed, undone).
inline size_t undo_counts(const phip_handle* h) { return (size_t)h->ncu * kFastPerCU * (kFastBlock / 64); }

// The undo log of an optimistic pass over n messages on `ncu` compute units:
// the fast kernel's grid, its waves, the entries of a wave's region
// (undo_wave_cap) and the 16-byte halves the whole log takes (the ensure()
// count).
struct UndoLayout {
  u32 grid, waves, cap;
  u64 halves;
};
inline UndoLayout undo_layout(u32 n, u32 ncu) {
  UndoLayout l;
  l.grid = fast_grid_on(ncu, n);
  l.waves = l.grid * (kFastBlock / 64);
  l.cap = undo_wave_cap(n, l.grid);
  l.halves = (u64)l.waves * l.cap * 2;
  return l;
}

// A fast pass's device counters: one of two sets by batch parity, apart
// from the general set every other path uses (ordered batches, inserts, the
// miss path), so that a queued batch's front -- its classification's
// counters -- survives the previous batch's leftover work, and is queued
// again only when that work ran a nested fast pass or grew the table.
inline u32* fctr(phip_handle* h, u32 par) { return h->ctr + kCtrWords * (1 + par); }

inline u32* fast_counts(phip_handle* h, u32 par) {
  return (u32*)h->buf[B_FSCNT].p + par * 2 * kShards;
}

// The dirty-bucket set and list (phip_kernels.hpp "Dirty buckets").
int dirty_set(phip_handle* h, DirtySet* d, u32** dlist) {
  int rc;
  u64* b;
  if ((rc = ensure(h, B_DTAB, DirtySet::kWords, &b)) || (rc = ensure(h, B_DLIST, kDirtyCap, dlist)))
    return rc;
  *d = DirtySet::at(b);
  return PHIP_OK;
}
// The ordered sub-batch dirty_finish builds (kSubBatchCap entries: at most 5
// per dirty message).
struct SubBatch {
  uint64_t *off, *a, *t;
  int64_t* e;
  u8* len;
  u32* map;
};
int sub_batch(phip_handle* h, SubBatch* b) {
  constexpr size_t m = kSubBatchCap;
  int rc;
  if ((rc = ensure(h, B_SOFF, m, &b->off)) || (rc = ensure(h, B_SLEN, m, &b->len)) ||
      (rc = ensure(h, B_SA, m, &b->a)) || (rc = ensure(h, B_ST, m, &b->t)) ||
      (rc = ensure(h, B_SE, m, &b->e)) || (rc = ensure(h, B_SMAP, m, &b->map)))
    return rc;
  return PHIP_OK;
}

int fast_shards(phip_handle* h, u32 n, u32 par, Sharded* out) {
  int rc;
  u32* c;
  out->cap = shard_cap((n + 63) / 64, 64);
  if ((rc = ensure(h, B_MSHARD, (size_t)kShards * out->cap, &out->base)) ||
      (rc = ensure(h, B_FSCNT, 4 * kShards, &c)))
    return rc;
  out->cnt = fast_counts(h, par);
  return PHIP_OK;
}

// Start the hot directory of a classified fast batch on stream2, beside
// k_classify (fast_back joins it).
template <class Src>
int fork_hot(phip_handle* h, Src src, FastPass* p) {
  if (p->n < kHotMinBatch) return PHIP_OK;
  // ev_fork: recorded by the front before the classification (stream2 waits
  // only for the batch's producers, not for k_classify)
  HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  int rc;
  if ((rc = build_hot(h, src, p->n, h->stream2, nullptr, p))) return rc;
  HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
  p->hot_join = true;
  return PHIP_OK;
}

// An optimistic pass's front: no classification, and nothing runs beside the
// directory, so it is built on the main stream with no hop, its launch also
// filling the status column (k_hot_dir's fill workgroups; why a fill:
// front_classified).  A batch too small for a directory gets a plain fill,
// one without a status column the directory a classified batch builds.
// While the handle keeps a directory (keep_take), the front launches nothing
// for it: the pass takes the slot built last, the kernel validates its entries
// as it loads them, and the status column is the back's to fill (fast_back).
bool keep_take(phip_handle* h, FastPass* p);
template <class HotSrc>
int front_optimistic(phip_handle* h, HotSrc hsrc, u8* status, FastPass* p) {
  int rc;
  if ((rc = ensure(h, B_ULCNT, undo_counts(h), &p->log.cnt))) return rc;
  if (keep_take(h, p)) {
    p->fill = status;
    return PHIP_OK;
  }
  if (p->n >= kHotMinBatch && status)
    return build_hot(h, hsrc, p->n, h->stream, status, p);
  if (status) HIPCHK(h, hipMemsetAsync(status, PHIP_ST_MERGED, p->n, h->stream));
  if (p->n >= kHotMinBatch) HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
  return fork_hot(h, hsrc, p);
}

// A classified or isolating pass's front.  Enqueue order matters at this
// size (2 ms per 100M messages): the classification goes right behind the
// counter reset, so the GPU starts reading the batch while the host still
// enqueues the directory on stream2.
template <class In, class HotSrc>
int front_classified(phip_handle* h, In in, HotSrc hsrc, u8* status, FastPass* p) {
  int rc;
  const u32 n = p->n;
  u32* dlist = nullptr;
  DirtySet dset;
  // (the classification lists the dirty messages either way: the policy
  // learns of them, and an isolating pass builds its set from the list)
  if ((rc = dirty_set(h, &dset, &dlist))) return rc;
  if (p->kind == PassKind::kIsolating) {
    p->mark = status;
    if (!status) {   // (marks need a column: a cleared one)
      if ((rc = ensure(h, B_DMARK, n, &p->mark))) return rc;
      HIPCHK(h, hipMemsetAsync(p->mark, 0, n, h->stream));
    }
  }
  // A small batch classifies in a few µs, less than the directory kernel
  // takes: that chain goes first then.
  const bool hot_first = n < (1u << 23);
  // Statuses: the fast kernel merges most of the batch and writes none; the
  // column is filled with PHIP_ST_MERGED up front (by k_classify_soa2 as it
  // streams the batch, else a fill on the main stream), and every message
  // the kernel leaves is written again after it (k_receive_list and
  // k_mark_created for misses, the ordered path for dirty buckets).  Byte
  // stores from the fast kernel's lanes cost it 2%; a fill on stream2 beside
  // the classification slowed the classification more than it cost here
  // (DESIGN.md §4).
  if (n >= kHotMinBatch) HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
  if (hot_first && (rc = fork_hot(h, hsrc, p))) return rc;
  {
    bool done = false;
    if constexpr (In::kSoa) {
      if ((((uintptr_t)in.ma | (uintptr_t)in.mt) & 15) == 0) {
        Launch l(h, "k_classify");
        // checked names (names_len): their offsets too (0.1 ms per 100M
        // messages; on stream2 beside this pass it cost 0.12)
        NamesOffs chk{};
        if constexpr (In::kOffs) chk = in.src;
        k_classify_soa2<<<grid_for((n + 1) / 2), kBlock, 0, h->stream>>>(in.ma, in.mt, in.me, n,
                                                                          p->c, status, chk, dlist);
        done = true;
      }
    }
    if (!done) {
      if (status) HIPCHK(h, hipMemsetAsync(status, PHIP_ST_MERGED, n, h->stream));
      Launch l(h, "k_classify");
      k_classify<In><<<grid_for(n), kBlock, 0, h->stream>>>(in, n, p->c, dlist);
    }
  }
  HIPCHK(h, hipGetLastError());
  return hot_first ? PHIP_OK : fork_hot(h, hsrc, p);
}

// A pass's front: what it is (pass_kind), its parity and counter set, the
// counter reset (reset = false: the batch queued just before, nothing
// since, reset the counters in its last launch), then the kind's front.
template <class In, class HotSrc>
int fast_begin(phip_handle* h, In in, HotSrc hsrc, u32 n, u8* status, PassAsk ask, bool reset,
               FastPass* p) {
  int rc;
  u32* c;
  *p = FastPass{};
  p->kind = pass_kind<In>(h, ask);
  p->n = n;
  if ((rc = ensure(h, B_FSCNT, 4 * kShards, &c))) return rc;
  // the pass's counter set and shard counters (the other parity's); their
  // reset is the first thing any kind of pass puts on the stream
  p->par = h->fpar ^= 1u;
  p->c = fctr(h, p->par);
  ++h->nfast;
  if (reset) {
    k_batch_reset<<<1, kShards, 0, h->stream>>>(p->c, fast_counts(h, p->par));
    HIPCHK(h, hipGetLastError());
  }
  if (p->kind == PassKind::kOptimistic) return front_optimistic(h, hsrc, status, p);
  h->keep.agree = false;   // (any other pass builds as ever, and the kept state goes)
  return front_classified(h, in, hsrc, status, p);
}

// Whether an optimistic pass's back over n messages finds its buffers -- the
// miss list, its shards, the undo log -- large enough as they stand (ensure()
// would replace none): a gated back is enqueued while the batch before still
// needs their contents.
inline bool holds(const phip_handle* h, BufId id, size_t bytes) {
  return h->buf[id].cap >= std::max<size_t>(bytes, 64) + 64;
}
inline bool back_fits(const phip_handle* h, u32 n) {
  return holds(h, B_MISS, (size_t)n * sizeof(u32)) &&
         holds(h, B_MSHARD, (size_t)kShards * shard_cap((n + 63) / 64, 64) * sizeof(u32)) &&
         holds(h, B_FSCNT, 4 * kShards * sizeof(u32)) &&
         holds(h, B_ULOG, (size_t)undo_layout(n, (u32)h->ncu).halves * sizeof(u64x2));
}

// The fast kernel is enqueued behind the classification without a host
// round trip; it reads the counters itself.
template <class In>
int fast_back(phip_handle* h, In in, FastPass& p, bool queued) {
  const u32 n = p.n;
  const bool iso = p.kind == PassKind::kIsolating;
  u32* miss;
  int rc;
  Sharded msh;
  DirtySet dset{};
  SubBatch sb{};
  u32* dlist = nullptr;
  if ((rc = ensure(h, B_MISS, n, &miss)) || (rc = fast_shards(h, n, p.par, &msh))) return rc;
  if (iso) {
    // the dirty set behind the classification (a batch without a dirty
    // message returns at once: one launch of ~3 us)
    if ((rc = dirty_set(h, &dset, &dlist)) || (rc = sub_batch(h, &sb))) return rc;
    Launch l(h, "k_dirty_build");
    k_dirty_build<In><<<1, 1024, 0, h->stream>>>(in, n, p.c, dlist, dset, table(h));
    HIPCHK(h, hipGetLastError());
  }
  if (p.hot_join) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
  switch (p.kind) {
    case PassKind::kOptimistic:
      if constexpr (In::kSoa) {   // (pass_kind: no other input is optimistic)
        // (the log is sized here, not in the front: a queued front runs before
        // the batch before is collected, and that batch's undo reads the log)
        const UndoLayout ul = undo_layout(n, (u32)h->ncu);
        p.log.cap = ul.cap;
        if ((rc = ensure(h, B_ULOG, (size_t)ul.halves, &p.log.base))) return rc;
        // The status column of a pass whose front launched no k_hot_dir:
        // stored by the kernel's own chunks, or (PHIP_STATUS_IN_KERNEL=0) by a
        // fill in front of it.  DESIGN.md §4 round 9 has both measured.
        u8* kstatus = PHIP_STATUS_IN_KERNEL ? p.fill : nullptr;
        if (p.fill && !kstatus) HIPCHK(h, hipMemsetAsync(p.fill, PHIP_ST_MERGED, n, h->stream));
        Launch l(h, "k_receive_fast");
        // (hot_nw: a kept directory in a compact layout, keep_take)
        auto* kern = p.hot_nw == 2   ? k_receive_fast<In, true, 2>
                     : p.hot_nw == 3 ? k_receive_fast<In, true, 3>
                                     : k_receive_fast<In, true, 0>;
        kern<<<ul.grid, kFastBlock, 0, h->stream>>>(
            in, 0, n, table(h), msh, p.c, p.hot, p.dir, nullptr, nullptr, p.log,
            (uint4*)p.hot_zero, p.hot_age != 0, p.gate, kstatus);
      }
      break;
    case PassKind::kClassified:
    case PassKind::kIsolating: {
      Launch l(h, "k_receive_fast");
      k_receive_fast<In><<<fast_grid(h, n), kFastBlock, 0, h->stream>>>(
          in, 0, n, table(h), msh, p.c, p.hot, p.dir, iso ? dset.key : nullptr, p.mark,
          UndoLog{}, (uint4*)p.hot_zero, 0u, nullptr, nullptr);
    }
  }
  HIPCHK(h, hipGetLastError());
  if (p.hot_zero) h->hot_clean = p.hot_zero;   // (queued behind every user of the tables)
  if (iso) {
    // the messages the fast kernel marked (an isolated batch's only: others
    // return at once), then the dirty buckets' records unmarked and their
    // ordered sub-batch built in the launch that ends the batch
    {
      Launch l(h, "k_dirty_pass");
      const unsigned g = (unsigned)std::max<u64>(
          1, std::min<u64>(((u64)n + 1023) / 1024, (u64)h->ncu * 2));
      k_dirty_pass<In><<<g, 1024, 0, h->stream>>>(in, n, p.c, p.mark, dset.key, table(h), msh);
      HIPCHK(h, hipGetLastError());
    }
    k_batch_end<In><<<1, kShards, 0, h->stream>>>(
        in, p.c, dset.key, table(h),
        SubOut{sb.off, sb.len, sb.a, sb.t, sb.e, sb.map, kSubBatchCap}, msh.cnt,
        h->ctr_map + kCtrWords * (1 + p.par), kCtrWords,
        queued ? fast_counts(h, p.par ^ 1u) : nullptr, fctr(h, p.par ^ 1u));
  } else {
    k_shard_scan<<<1, kShards, 0, h->stream>>>(msh.cnt, p.c, kCtrMiss,
                                               h->ctr_map + kCtrWords * (1 + p.par), kCtrWords,
                                               queued ? fast_counts(h, p.par ^ 1u) : nullptr,
                                               fctr(h, p.par ^ 1u), p.gate);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev_ctr[p.par], h->stream));
  if (!queued) HIPCHK(h, hipEventSynchronize(h->ev_ctr[p.par]));
  return PHIP_OK;
}

// The isolation policy: kIsoKeep passes after one that met a dirty message.
constexpr u32 kIsoKeep = 256;
// An optimistic pass whose undo log overflowed (a batch that grows a field
// with most of its cold messages: uniform keys) left the overflowing
// messages unmerged.  They are on its miss list, but that list is not used
// for them: the insert pipeline may refuse a batch (PHIP_CFG_NO_GROW) before
// it merges anything, and a message naming an existing bucket must be merged
// even then.  Such a pass counts as failed, like one that met a dirty
// message, and the handle's next kOptBackoff fast passes classify first.
constexpr u32 kOptBackoff = 256;

// The one place that moves the policy: a pass's counters (mirrored to the
// host) applied to opt_left and iso_left, with an optimistic pass's log
// statistics.  True: a failed speculation, to be undone -- the pass met a dirty
// message or a malformed name entry, or its log overflowed (the pass that runs
// the batch again then classifies first).  iso_left moves only with a pass
// that stands: that second pass reports the dirty message.
//
// The kept directory's policy lives here too.  keep_take (a pass's front): an
// optimistic pass of kHotMinBatch messages or more, with a status column or
// none, takes the directory built last, without a build, when
//   - among the passes collected, the latest build agreed with the directory
//     before it: kept * 8 >= own * 7 with own > 0 (k_hot_dir's sums),
//   - no pass collected since folded less than 7/8 of the fraction hot_hits / n
//     that build's batch folded,
//   - the directory has served fewer than kHotKeepPasses passes (a bucket that
//     turns hot later does not lower the hit fraction, it only contends on its
//     record: the age bound finds it),
//   - no record has moved (layout_gen).
// These are conditions, not tuned figures.  Every other pass builds as ever;
// one that is not optimistic drops the kept state (fast_begin).  keep_collect
// (a pass that stands, from its counters): the agreement of a build, the sag.
constexpr u32 kHotKeepPasses = 32;
bool keep_take(phip_handle* h, FastPass* p) {
  phip_handle::HotKeep& k = h->keep;
  if (p->n < kHotMinBatch || !k.have || !k.agree || k.sagged || k.served >= kHotKeepPasses ||
      k.gen != h->layout_gen || k.base != h->buf[B_HOT].p)
    return false;
  p->hot = (const HotHdr*)((u8*)k.base + kHotSlotsAt + k.slot * kHotSlotBytes);
  p->dir = (const HotEntry*)(p->hot + 1);
  p->hot_age = k.served++;
  // The layout the kernel holds it in, from the longest name the latest build
  // collected selected: two name words an entry and the whole extended
  // selection, three words and its first kHotMax3 entries (the better part:
  // k_hot_dir orders them by count), or today's and the first HotHdr::n.  A
  // queued pass may take a slot built after that build, not collected yet; the
  // kernel leaves out any entry whose name its layout does not hold, so the
  // choice costs hits at worst.
  p->hot_nw = k.maxlen <= kShortName ? 2u : k.maxlen <= kInlineName ? 3u : 0u;
  return true;
}
// (a pass served by the kept directory folded less than 7/8 of the fraction
// the latest build's batch folded; the reference is a built pass, which folds
// through the first HotHdr::n entries only, so a kept pass in a compact layout
// of more entries folds more than its build did and cannot sag for that reason)
bool keep_sagged(const phip_handle* h, const FastPass& p, const u32* c) {
  const phip_handle::HotKeep& k = h->keep;
  return p.hot_age != 0 && (unsigned __int128)c[kCtrHotHits] * k.ref_n * 8 <
                               (unsigned __int128)k.ref_hits * p.n * 7;
}
void keep_collect(phip_handle* h, const FastPass& p, const u32* c) {
  phip_handle::HotKeep& k = h->keep;
  if (p.kind != PassKind::kOptimistic) {
    k.agree = false;
    return;
  }
  if (p.built) {
    k.agree = c[kCtrHotOwn] > 0 && (u64)c[kCtrHotKept] * 8 >= (u64)c[kCtrHotOwn] * 7;
    k.maxlen = c[kCtrHotMaxLen];
    k.ref_hits = c[kCtrHotHits];
    k.ref_n = p.n;
    k.sagged = false;
  } else if (keep_sagged(h, p, c)) {
    k.sagged = true;
  }
}

inline const u32* fmirror(const phip_handle* h, u32 par) { return h->ctr_host + kCtrWords * (1 + par); }

bool apply_policy(phip_handle* h, const FastPass& p) {
  const u32* c = fmirror(h, p.par);
  if (p.kind == PassKind::kOptimistic) {
    h->stats.log_count = c[kCtrLogCount];
    h->stats.log_over = c[kCtrLogOver];
    // (An overflow under a kept directory that no longer folds its share is
    // the directory's: the hot set moved, and the buckets now hot went
    // through the table path, every lane of a wave logging the same records.
    // The pass fails and the batch runs again classified, which drops the kept
    // state; the handle does not back off.)
    if (c[kCtrLogOver] && !keep_sagged(h, p, c)) h->opt_left = kOptBackoff;
    if (c[kCtrDirty] < p.n || c[kCtrStop] < p.n || c[kCtrLogOver]) return true;
  } else if (h->opt_left) {
    --h->opt_left;
  }
  if (c[kCtrDirty] < p.n) h->iso_left = kIsoKeep;
  else if (h->iso_left) --h->iso_left;
  keep_collect(h, p, c);
  return false;
}

// What a settled pass left to do (finish_receive).  first_dirty: n when the
// dirty buckets were set apart (an isolating pass, at most kDirtyCap dirty
// messages, short names), else the first dirty message (the prefix rule).
struct FastOutcome {
  u32 first_dirty = 0;
  u32 nmiss = 0;         // misses of the clean prefix, listed in B_MISS
  u32 stop = 0;          // the first malformed datagram or name entry (n: none)
  u32 ndef = 0;          // entries of the ordered sub-batch (the dirty buckets, run_deferred)
  bool iso_ran = false;  // the pass was isolating (its nested pass must be too)
  bool again = false;    // a failed speculation: a second fast pass ran the batch again
};

int fast_collect(phip_handle* h, const FastPass& p, FastOutcome* o) {
  int rc;
  const u32* c = fmirror(h, p.par);
  if ((rc = check_flags(h, c))) return rc;
  o->nmiss = c[kCtrMiss];
  if (o->nmiss) {
    Sharded msh;
    if ((rc = fast_shards(h, p.n, p.par, &msh))) return rc;
    Launch l(h, "k_shard_compact");
    dim3 grid(grid_for(c[kCtrShardMax]), kShards);
    k_shard_compact<<<grid, 256, 0, h->stream>>>(msh.base, msh.cap, msh.cnt,
                                                 (u32*)h->buf[B_MISS].p);
    HIPCHK(h, hipGetLastError());
  }
  const u32 nd = c[kCtrNDirty];
  o->iso_ran = p.kind == PassKind::kIsolating;
  const bool apart = o->iso_ran && nd != 0 && nd <= kDirtyCap;
  o->first_dirty = apart ? p.n : std::min<u32>(c[kCtrDirty], p.n);
  o->stop = std::min<u32>(c[kCtrStop], p.n);
  o->ndef = apart ? c[kCtrNDefer] : 0;
  h->stats.ordered = 0;   // (finish_receive: the messages it sends through the ordered path)
  h->stats.hot_entries = c[kCtrHotEntries];
  h->stats.hot_hits = c[kCtrHotHits];
  h->stats.misses = o->nmiss;
  h->stats.hot_age = p.hot_age;
  h->stats.gate_shut = p.gate_shut;
  return PHIP_OK;
}

// Settles a pass whose back is enqueued and whose counters have arrived.  A
// failed speculation is undone (k_undo: every record it touched back to its
// state before the batch; its miss list goes with its counters, nothing was
// created) and the batch run again, synchronously, under the policy as it
// stands (the status column is filled again).  Then the pass is collected.
template <class In, class HotSrc>
int fast_settle(phip_handle* h, In in, HotSrc hsrc, u8* status, FastPass* p, FastOutcome* o) {
  int rc;
  o->again = apply_policy(h, *p);
  if (o->again) {
    {
      Launch l(h, "k_undo");
      k_undo<<<fast_grid(h, p->n) * (kFastBlock / 64), 256, 0, h->stream>>>(p->log, table(h));
      HIPCHK(h, hipGetLastError());
    }
    if ((rc = fast_begin(h, in, hsrc, p->n, status, PassAsk::kPolicy, true, p)) ||
        (rc = fast_back(h, in, *p, false)))
      return rc;
    (void)apply_policy(h, *p);   // (not optimistic: it stands)
  }
  return fast_collect(h, *p, o);
}

// The whole fast path of a batch (SoaIn or WireIn; hsrc: its names for the
// hot-directory sample), synchronously: its clean prefix applied (*o).
template <class In, class HotSrc>
int fast_apply(phip_handle* h, In in, HotSrc hsrc, u32 n, u8* status, PassAsk ask,
               FastOutcome* o) {
  int rc;
  FastPass p;
  if ((rc = fast_begin(h, in, hsrc, n, status, ask, true, &p)) ||
      (rc = fast_back(h, in, p, false)))
    return rc;
  return fast_settle(h, in, hsrc, status, &p, o);
}

// One message per distinct name of list[0..n) (k_dedupe) into B_DEDUP.
template <class Src>
int dedupe_names(phip_handle* h, Src src, const u32* list, u32 n, u32** out, u32* nout) {
  int rc;
  u32 setbits = 1;
  while ((1ull << setbits) < 2ull * n) ++setbits;
  u64* set;
  Sharded dsh;
  if ((rc = ensure(h, B_DSET, size_t(1) << setbits, &set)) ||
      (rc = ensure(h, B_DEDUP, n, out)) ||
      (rc = sharded(h, B_MSHARD, grid_for(n), kBlock, &dsh)))
    return rc;
  HIPCHK(h, hipMemsetAsync(set, 0, (size_t(1) << setbits) * sizeof(u64), h->stream));
  {
    Launch l(h, "k_dedupe");
    k_dedupe<Src><<<grid_for(n), kBlock, 0, h->stream>>>(src, n, list, table(h), set, setbits, dsh);
    HIPCHK(h, hipGetLastError());
  }
  return pack_sharded(h, dsh, kCtrAux, *out, nout);
}

// Many misses (an insert-heavy batch: a node starting empty, a fresh key
// range): create each distinct missing name once (k_dedupe, then the insert
// pipeline over one message per name), then merge by running the fast pass
// again over the whole clean prefix [0, prefix).  In that prefix every merge
// is an order-free max, so the messages the first pass already merged are
// merged again to no effect, and the hot directory now covers the new hot
// buckets: their messages fold in LDS instead of each sending a
// device-scope atomic to one record (134 ms per 100M-message batch through
// k_receive_list).  *o: the first pass's outcome; the second's
// misses (names k_dedupe dropped for a shared tag, in B_MISS) replace its own.
template <class Src>
int finish_many_misses(phip_handle* h, Src src, const uint64_t* a, const uint64_t* t,
                       const int64_t* e, u32 prefix, i64 now, u8* status, FastOutcome* o) {
  u32* miss = (u32*)h->buf[B_MISS].p;
  const u32 nmiss = o->nmiss;
  int rc;
  // 1. distinct names
  u32 *dedup, nd = 0;
  if ((rc = dedupe_names(h, src, miss, nmiss, &dedup, &nd))) return rc;
  // 2. create them (aux = ~0 and the NEW flag on every claimed slot)
  u32 n_claimed = 0;
  if ((rc = insert_names(h, src, dedup, nd, nullptr, now, &n_claimed, nullptr, true))) return rc;
  // 3. creator tracking over the first pass's misses (every message of a new
  //    bucket is among them), before the second pass reuses B_MISS
  if (status) {
    Launch l(h, "k_first_seen");
    k_first_seen<Src><<<grid_for(nmiss), kBlock, 0, h->stream>>>(src, nmiss, miss, table(h));
    HIPCHK(h, hipGetLastError());
  }
  // 4. the fast pass again
  // (as the pass being finished did: its dirty buckets stay apart)
  FastOutcome o2;
  if ((rc = fast_apply(h, SoaIn<Src>{src, a, t, e}, src, prefix, status,
                       o->iso_ran ? PassAsk::kIsolate : PassAsk::kNoIsolate, &o2)))
    return rc;
  // The sub-batch run_deferred runs is the last pass's: this pass rebuilt it
  // (whether it runs, the prefix and the stop stay the first's, finish_receive).
  o->nmiss = o2.nmiss;
  o->ndef = o2.ndef;
  // 5. PHIP_ST_CREATED after the second pass wrote its statuses
  if (status && n_claimed) {
    Launch l(h, "k_mark_created");
    k_mark_created_slots<<<grid_for(n_claimed), kBlock, 0, h->stream>>>(
        (const u32*)h->buf[B_CSLOT].p, n_claimed, table(h), status);
    HIPCHK(h, hipGetLastError());
  }
  return clear_new(h, n_claimed);
}

// The messages the fast pass missed: create their buckets, merge them with
// creator tracking (PHIP_ST_CREATED on the first message of a new bucket).
template <class Src>
int finish_misses(phip_handle* h, Src src, const uint64_t* a, const uint64_t* t, const int64_t* e,
                  i64 now, u8* status, FastOutcome* o) {
  if (o->nmiss == 0) return PHIP_OK;
  int rc;
  if (o->nmiss >= kManyMisses &&
      (rc = finish_many_misses(h, src, a, t, e, std::min(o->stop, o->first_dirty), now, status, o)))
    return rc;
  const u32 nmiss = o->nmiss;
  if (nmiss == 0) return PHIP_OK;
  u32* miss = (u32*)h->buf[B_MISS].p;
  u32 n_claimed = 0;
  if ((rc = insert_names(h, src, miss, nmiss, nullptr, now, &n_claimed))) return rc;
  HIPCHK(h, hipMemsetAsync(h->ctr + kCtrMiss, 0, sizeof(u32), h->stream));
  u32* miss2;
  if ((rc = ensure(h, B_MISS2, nmiss, &miss2))) return rc;
  {
    Launch l(h, "k_receive_list");
    k_receive_list<Src><<<grid_for(nmiss), kBlock, 0, h->stream>>>(
        src, a, t, e, nmiss, miss, table(h), status, miss2, h->ctr);
  }
  HIPCHK(h, hipGetLastError());
  {
    Launch l(h, "k_mark_created");
    k_mark_created<Src><<<grid_for(nmiss), kBlock, 0, h->stream>>>(src, nmiss, miss, table(h),
                                                                    status);
  }
  HIPCHK(h, hipGetLastError());
  if ((rc = read_ctr(h))) return rc;
  if (const u32 left = h->ctr_host[kCtrMiss])
    return set_err(h, PHIP_ERR_INVALID, "internal: %u names missing after insert", left);
  return clear_new(h, n_claimed);
}

// ------------------------------------------------------------ ordered ----

// A launch for the run-time output mask (out_mask): CALL(M) with M a
// compile-time constant.
#define PHIP_OUT_DISPATCH(mask, CALL) \
  switch (mask) {                     \
    case 0: CALL(0); break;           \
    case 1: CALL(1); break;           \
    case 2: CALL(2); break;           \
    case 3: CALL(3); break;           \
    case 4: CALL(4); break;           \
    case 5: CALL(5); break;           \
    case 6: CALL(6); break;           \
    case 7: CALL(7); break;           \
    case 8: CALL(8); break;           \
    case 9: CALL(9); break;           \
    case 10: CALL(10); break;         \
    case 11: CALL(11); break;         \
    case 12: CALL(12); break;         \
    case 13: CALL(13); break;         \
    case 14: CALL(14); break;         \
    default: CALL(15); break;         \
  }

template <class Src>
int resolve_all(phip_handle* h, Src src, u32 n, const int64_t* now_arr, i64 now0, u32** slot_out,
                u32* n_claimed, SortVals sv = SortVals{nullptr, 0, nullptr}) {
  u32 *slot, *miss;
  int rc;
  Sharded rsh;
  if ((rc = ensure(h, B_SLOT, n, &slot)) || (rc = ensure(h, B_MISS, n, &miss)) ||
      (rc = sharded(h, B_MSHARD, grid_for(n), kBlock, &rsh)))
    return rc;
  if ((rc = reset_ctr(h))) return rc;
  {
    // (kResPer ops per thread; a persistent version that took the hot names'
    // slots from C2's directory in LDS first lost: 1.85 against 1.49 ms on
    // C3 with one op per thread)
    Launch l(h, "k_resolve");
    k_resolve_batch<Src><<<grid_for(n, kBlock * kResPer), kBlock, 0, h->stream>>>(
        src, n, table(h), slot, rsh, h->ctr, sv);
  }
  HIPCHK(h, hipGetLastError());
  u32 nmiss = 0;
  if ((rc = pack_sharded(h, rsh, kCtrMiss, miss, &nmiss))) return rc;
  if ((rc = check_flags(h))) return rc;
  *n_claimed = 0;
  bool grew = false;
  if (nmiss >= kManyMisses) {
    // Many new names (an ordered batch on a fresh key range, a large seed):
    // create each once, then resolve the misses again; names k_dedupe
    // dropped for a shared tag miss again and take the general rounds below.
    u32 *dedup, nd = 0;
    if ((rc = dedupe_names(h, src, miss, nmiss, &dedup, &nd)) ||
        (rc = insert_names(h, src, dedup, nd, now_arr, now0, n_claimed, &grew, true)))
      return rc;
    Sharded r2;
    if ((rc = sharded(h, B_MSHARD, grid_for(nmiss), kBlock, &r2))) return rc;
    {
      Launch l(h, "k_resolve_miss");
      k_resolve<Src><<<grid_for(nmiss), kBlock, 0, h->stream>>>(src, nmiss, miss, table(h), slot,
                                                                 r2, h->ctr, SortVals{});
    }
    HIPCHK(h, hipGetLastError());
    if ((rc = pack_sharded(h, r2, kCtrMiss, miss, &nmiss))) return rc;
  }
  if (nmiss) {
    u32 more = 0;
    bool g2 = false;
    if ((rc = insert_names(h, src, miss, nmiss, now_arr, now0, &more, &g2))) return rc;
    grew |= g2;
    *n_claimed += more;
    if (!grew) {
      Launch l(h, "k_resolve_miss");
      k_resolve<Src><<<grid_for(nmiss), kBlock, 0, h->stream>>>(src, nmiss, miss, table(h), slot,
                                                                 Sharded{}, h->ctr, SortVals{});
      HIPCHK(h, hipGetLastError());
    }
  }
  if (grew) {
    // The table was rehashed: every op's slot is looked up again.
    Launch l(h, "k_resolve");
    k_resolve<Src><<<grid_for(n), kBlock, 0, h->stream>>>(src, n, nullptr, table(h), slot,
                                                           Sharded{}, h->ctr, SortVals{});
    HIPCHK(h, hipGetLastError());
  }
  *slot_out = slot;
  return PHIP_OK;
}

// phip_apply_mixed_egress' part of ordered(): where the batch's datagrams go (device
// memory) and the caps its caller checked against the batch's worst case.
struct EgressOut {
  u8* out;
  u64* offs;
  u32 max_msgs;
  u64 budget;
};

// What runs behind an ordered batch's folds (behind_folds; ow.status is
// required): the batch's egress into *eg, or, eg == nullptr, its marks in the
// change set of a handle that keeps one.  uniform: every op has one kind,
// known to the host, and the kernels read no kinds; wants: that kind is TAKE
// or UPSERT (false unless uniform).
struct Behind {
  bool uniform, wants;
  const EgressOut* eg;
};

// An ordered batch, sorted by slot and cut into one segment per bucket it
// names (segment_batch): device pointers into the handle's buffers.
struct Segs {
  u32 n;              // ops of the batch
  u32 nseg;           // segments (kCtrSegs, k_seg_finish)
  u32 nlong;          // entries of lng (kCtrLongSegs, k_seg_finish)
  u32 nhuge;          // entries of huge (kCtrHugeSegs, k_seg_finish)
  const u32* uslot;   // by segment: the bucket's slot (k_seg_write)
  const u32* sstart;  // by segment: its first position in the sorted order (k_seg_write)
  const u32* scnt;    // by segment: its ops (k_seg_finish)
  const u32* sidx;    // by sorted position: op index | kind << kOpIdxBits (the sort's values)
  u32* lng;           // the segments of kLongSeg < ops <= kHugeSeg (k_seg_finish, fold_rest)
  const u32* huge;    // the segments over kHugeSeg ops (k_seg_finish)
  const OpRec* opr;   // by op index: the op records (k_pack_ops)
};

// What runs behind the folds, on the main stream: the batch egress
// (phip_kernels.hpp "batch egress"; the totals stay in the egress counter
// words for the caller) or the marks (phip_kernels.hpp "change set"), either
// behind k_egress_wants when mixed kinds meet segments above kLongSeg ops.
int behind_folds(phip_handle* h, const Behind& b, const Segs& sg, const u8* status) {
  const u32 ntiles = (sg.nseg + kSweepTile - 1) / kSweepTile;
  const bool ask = !b.uniform && (sg.nlong || sg.nhuge);
  u32* esz = nullptr;
  u64* tile_bytes = nullptr;
  int rc;
  // one buffer: the tiles' byte sums, then their counts (both sections each)
  if (((b.eg || ask) && (rc = ensure(h, B_EGSZ, sg.nseg, &esz))) ||
      (b.eg && (rc = ensure(h, B_EGTILE, 3 * (size_t)ntiles, &tile_bytes))))
    return rc;
  if (ask) {
    Launch l(h, "k_egress_wants");
    k_egress_wants<<<(sg.nlong + kBlock / 64 - 1) / (kBlock / 64) + sg.nhuge, kBlock, 0,
                     h->stream>>>(sg.lng, sg.nlong, sg.huge, sg.nhuge, sg.sstart, sg.scnt, sg.sidx,
                                  esz);
  }
  if (!b.eg) {
    Launch l(h, "k_changes_mark");
#define PHIP_MARK(U)                                              \
  k_changes_mark<U><<<grid_for(sg.nseg), kBlock, 0, h->stream>>>( \
      sg.uslot, sg.sstart, sg.scnt, sg.sidx, sg.nseg, status, b.wants, esz, h->marks)
    if (b.uniform) PHIP_MARK(true); else PHIP_MARK(false);
#undef PHIP_MARK
    HIPCHK(h, hipGetLastError());
    return PHIP_OK;
  }
  u32* tile_cnt = (u32*)(tile_bytes + 2 * (size_t)ntiles);
  {
    Launch l(h, "k_egress_count");
#define PHIP_COUNT(U)                                                                          \
  k_egress_count<U><<<ntiles, kBlock, 0, h->stream>>>(h->recs, sg.uslot, sg.sstart, sg.scnt, \
                                                      sg.sidx, sg.nseg, status, b.wants, esz, \
                                                      ntiles, tile_cnt, tile_bytes)
    if (b.uniform) PHIP_COUNT(true); else PHIP_COUNT(false);
#undef PHIP_COUNT
  }
  {
    Launch l(h, "k_egress_scan");
    k_egress_scan<<<1, kSweepBlock, 0, h->stream>>>(tile_cnt, tile_bytes, ntiles, h->ctr);
  }
  {
    // (long names are bounded by the arena's size, as in the sweep)
    Launch l(h, "k_egress_write");
    k_egress_write<<<ntiles, kSweepBlock, 0, h->stream>>>(
        h->recs, h->arena, h->arena_cap, sg.uslot, esz, sg.nseg, ntiles, tile_cnt, tile_bytes,
        b.eg->max_msgs, b.eg->budget, b.eg->out, b.eg->offs, h->ctr);
  }
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// A side stream's way back.  While armed (ev: the event that ends the side
// stream's work), the main stream waits on ev when the Join goes out of scope:
// no return from ordered() leaves a fork open.  join(): that wait, checked.
struct Join {
  phip_handle* h;
  hipEvent_t ev = nullptr;
  int join() {
    hipEvent_t e = ev;
    ev = nullptr;
    if (e) HIPCHK(h, hipStreamWaitEvent(h->stream, e, 0));
    return PHIP_OK;
  }
  ~Join() { if (ev) (void)hipStreamWaitEvent(h->stream, ev, 0); }
};

// stream4 and its events, on first use (phip_handle::stream4 says why not at open).
int thread_stream(phip_handle* h) {
  if (!h->ev_t4a) HIPCHK(h, hipEventCreateWithFlags(&h->ev_t4a, hipEventDisableTiming));
  if (!h->ev_t4b) HIPCHK(h, hipEventCreateWithFlags(&h->ev_t4b, hipEventDisableTiming));
  if (!h->stream4) HIPCHK(h, hipStreamCreateWithFlags(&h->stream4, hipStreamNonBlocking));
  return PHIP_OK;
}

// [schedule]
// ordered()'s schedule: what each stream runs, in the order the host issues
// it, and every event edge ("rec" records the event, "wait" waits on it).
// Different segments touch different slots, so the three fold families
// overlap.  [huge]: batches with segments over kHugeSeg ops only; [split]:
// with more than PHIP_HUGE_FIRST of them only.
//
//   main (h->stream)       stream2                stream3 [split]    stream4
//   ---------------------  ---------------------  -----------------  ---------------
//   -- segment_batch --
//   rec ev_fork            wait ev_fork
//   resolve_all            k_pack_ops
//   radix_sort_pairs       rec ev_pack
//   segments, read_ctr
//   wait ev_pack
//   -- fold_huge [huge] --
//   default fills
//   rec ev_fork            wait ev_fork
//                          [split] k_huge_order
//                          k_huge_offsets
//                          [split] rec ev_fork3   wait ev_fork3
//                          k_gather_huge
//   wait ev_gather         rec ev_gather
//                          k_fold_block
//                          k_huge_outputs
//                                                 k_gather_huge2
//   wait ev_gather3                               rec ev_gather3
//                                                 k_fold_block2
//                                                 k_huge_outputs2
//                          wait ev_join3          rec ev_join3
//                          rec ev_join
//   -- fold_rest --
//   rec ev_t4a                                                       wait ev_t4a
//   rocprim::partition                                               k_fold_thread
//   k_fold_wave                                                      rec ev_t4b
//   wait ev_t4b
//   [huge] wait ev_join
//   behind_folds
//
// ev_pack: the op records are read by the folds only, so k_pack_ops runs
// beside the resolve (bound by probe latency), the sort and the segmentation.
// fold_huge: the largest huge segments (PHIP_HUGE_FIRST of them, moved to the
// front of the list by k_huge_order) run gather -> fold -> outputs on stream2,
// the others the same chain on stream3: the largest segments' folds are the
// longest sequential chains, so they start as soon as their own (smaller)
// gather is done.
// ev_gather, ev_gather3: the wave and thread folds start behind the gathers;
// the gathers alone, then the latency-bound block folds beside those
// bandwidth-bound folds, is the shorter schedule.
// fold_rest: the thread folds beside the wave folds, 6.37-6.38 against
// 6.45-6.50 ms per C3 step.
// ev_pack, ev_t4b, ev_join: waited on by ordered() itself, through a Join each.
// [/schedule]

// The batch's Segs: the buffers sized, k_pack_ops forked (*pack armed), every
// op's slot resolved, the sort and the segmentation; one host round trip.
template <class Src>
int segment_batch(phip_handle* h, Src src, u32 n, const OpView& ov, Segs* sg, Join* pack) {
  int rc;
  u32 *idx, *sslot, *sidx, *uslot, *scnt, *sstart, *lng, *huge;
  OpRec* opr;
  if ((rc = ensure(h, B_IDX, n, &idx)) || (rc = ensure(h, B_SSLOT, n, &sslot)) ||
      (rc = ensure(h, B_SIDX, n, &sidx)) || (rc = ensure(h, B_USLOT, n, &uslot)) ||
      (rc = ensure(h, B_SCNT, n, &scnt)) || (rc = ensure(h, B_SSTART, n, &sstart)) ||
      (rc = ensure(h, B_LONG, n, &lng)) || (rc = ensure(h, B_HUGE, n, &huge)) ||
      (rc = ensure(h, B_OPS, n, &opr)))
    return rc;
  HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  {
    Launch l(h, "k_pack_ops", h->stream2);
    k_pack_ops<<<grid_for(n, kBlock * kPackPer), kBlock, 0, h->stream2>>>(ov, n, opr);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev_pack, h->stream2));
  pack->ev = h->ev_pack;
  u32 *slot, n_claimed = 0;   // (n_claimed unused: the folds' store_state clears the NEW flags)
  if ((rc = resolve_all(h, src, n, ov.now, ov.now0, &slot, &n_claimed,
                        SortVals{ov.kind, ov.kind0, idx})))
    return rc;
  // Stable radix sort of (slot, seq) pairs: per-bucket arrival order kept.
  // (A hot split, the hot buckets' ops partitioned by name before the sort
  // and the sort ordering only the rest, was built and measured in round 6:
  // slower)
  size_t tb = 0;
  HIPCHK(h, rocprim::radix_sort_pairs<SlotSortConfig>(nullptr, tb, slot, sslot, idx, sidx, n, 0u, h->L,
                                                       h->stream));
  // segmentation buffers and scan temp sized before the sort is enqueued (a
  // larger B_TEMP must not replace the one the sort is using)
  const u32 ntiles = (u32)(((u64)n + kSegTile - 1) / kSegTile);
  u32* segt;
  size_t tbs = 0;
  if ((rc = ensure(h, B_SEGT, 2 * ((size_t)ntiles + 1), &segt))) return rc;
  u32* const segb = segt + ntiles + 1;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tbs, segt, segb, 0u, (size_t)ntiles + 1,
                                    rocprim::plus<u32>(), h->stream));
  u8* temp;
  if ((rc = ensure(h, B_TEMP, std::max(tb, tbs), &temp))) return rc;
  {
    Launch l(h, "radix_sort_pairs");
    HIPCHK(h, rocprim::radix_sort_pairs<SlotSortConfig>(temp, tb, slot, sslot, idx, sidx, n, 0u,
                                                         h->L, h->stream));
  }
  {
    Launch l(h, "segments");
    k_seg_count<<<ntiles, 256, 0, h->stream>>>(sslot, n, segt, h->ctr);
    HIPCHK(h, rocprim::exclusive_scan(temp, tbs, segt, segb, 0u, (size_t)ntiles + 1,
                                      rocprim::plus<u32>(), h->stream));
    k_seg_write<<<ntiles, 256, 0, h->stream>>>(sslot, n, segb, uslot, sstart);
    k_seg_finish<<<std::max(1u, std::min<u32>(ntiles, (u32)h->ncu * 4)), 256, 0, h->stream>>>(
        segb, ntiles, sstart, n, scnt, lng, huge, h->ctr);
    HIPCHK(h, hipGetLastError());
    if ((rc = read_ctr(h))) return rc;
  }
  const u32* c = h->ctr_host;
  *sg = Segs{n,     c[kCtrSegs], c[kCtrLongSegs], c[kCtrHugeSegs],
             uslot, sstart,      scnt,            sidx,            lng, huge, opr};
  return PHIP_OK;
}

#ifdef PHIP_FOLD_STATS
// A diagnostics build (tools/build_variants.sh "stats:-DPHIP_FOLD_STATS")
// prints per hot segment ops / windows / windows folded / rounds / bursts
// / ops walked / runs / cycles to stderr, once stream2 has run the chains.
int fold_stats_dump(phip_handle* h, const u64* fold_dbg, u32 nhuge) {
  std::vector<u64> d((size_t)nhuge * 16);
  HIPCHK(h, hipMemcpyAsync(d.data(), fold_dbg, d.size() * 8, hipMemcpyDeviceToHost, h->stream2));
  HIPCHK(h, hipStreamSynchronize(h->stream2));
  std::vector<u32> ord(nhuge);
  for (u32 k = 0; k < nhuge; ++k) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](u32 x, u32 y) { return d[16 * x + 7] > d[16 * y + 7]; });
  fprintf(stderr, "fold: %u huge segments\n", nhuge);
  for (u32 i = 0; i < nhuge && i < 6; ++i) {
    const u32 k = ord[i];
    const u64* e = &d[16 * k];
    fprintf(stderr, "fold[%u] ops %llu windows %llu folded %llu rounds %llu bursts %llu walked "
            "%llu runs %llu us %.1f | scan %.1f stage %.1f prefix %.1f round %.1f burst %.1f "
            "| burst iterations %llu (stopped at a merge %llu)\n",
            k, e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7] / 100.0, e[8] / 100.0,
            e[9] / 100.0, e[10] / 100.0, e[11] / 100.0, e[12] / 100.0, e[13], e[14]);
  }
  return PHIP_OK;
}
#endif

// The huge segments' folds, one workgroup each, on stream2 and stream3 (the
// schedule's fold_huge rows); *huge: armed with ev_join.
int fold_huge(phip_handle* h, const Segs& sg, const OutView& ow, Join* huge) {
  const u32 n = sg.n, nhuge = sg.nhuge;
  int rc;
  // k_huge_outputs stores only results that differ from the defaults
  // (write_out_nd): the defaults go in first, as streams
  if (ow.status) HIPCHK(h, hipMemsetAsync(ow.status, PHIP_ST_MERGED, n, h->stream));
  if (ow.remaining) HIPCHK(h, hipMemsetAsync(ow.remaining, 0, (size_t)n * 8, h->stream));
  if (ow.have) HIPCHK(h, hipMemsetAsync(ow.have, 0, (size_t)n * 8, h->stream));
  u64 *hoff, *woff;
  OpRec* hop;
  u32 *hval, *rpos, *runn, *wrun, *segxf;
  RunState* rst;
  u8* segex;
  WinSum* sums;
  GMax* wing;
  const size_t nwin_max = (size_t)n / kFoldWin + nhuge + 1;
  if ((rc = ensure(h, B_WOFF, (size_t)nhuge + 1, &woff)) ||
      (rc = ensure(h, B_SUMS, nwin_max, &sums)) || (rc = ensure(h, B_WRUN, nwin_max, &wrun)) ||
      (rc = ensure(h, B_HOFF, nhuge, &hoff)) || (rc = ensure(h, B_HOP, n, &hop)) ||
      (rc = ensure(h, B_HVAL, n, &hval)) || (rc = ensure(h, B_RPOS, (size_t)n + nhuge, &rpos)) ||
      (rc = ensure(h, B_RST, (size_t)n + nhuge, &rst)) || (rc = ensure(h, B_RUNN, nhuge, &runn)) ||
      (rc = ensure(h, B_SEGEX, nhuge, &segex)) || (rc = ensure(h, B_WING, nwin_max, &wing)) ||
      (rc = ensure(h, B_SEGXF, nhuge, &segxf)))
    return rc;
  const u32 kFirst = std::min<u32>(PHIP_HUGE_FIRST, kHugeFirstMax);
  const bool split = kFirst > 0 && nhuge > kFirst;
  const u32 hsplit = split ? kFirst : nhuge;
  u32* hl2 = nullptr;   // [split] the list with the largest in front
  if (split && (rc = ensure(h, B_HUGE2, nhuge, &hl2))) return rc;
  const u32* hl = split ? hl2 : sg.huge;
  HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  if (split) {
    k_huge_order<<<1, 1024, 0, h->stream2>>>(sg.huge, nhuge, sg.scnt, kFirst, hl2);
    HIPCHK(h, hipGetLastError());
  }
  k_huge_offsets<<<1, 1024, 0, h->stream2>>>(hl, nhuge, sg.scnt, hoff, woff);
  HIPCHK(h, hipGetLastError());
  if (split) {
    HIPCHK(h, hipEventRecord(h->ev_fork3, h->stream2));
    HIPCHK(h, hipStreamWaitEvent(h->stream3, h->ev_fork3, 0));
  }
  u64* fold_dbg = nullptr;
#ifdef PHIP_FOLD_STATS
  if ((rc = ensure(h, B_FOLDDBG, (size_t)nhuge * 16, &fold_dbg))) return rc;
#endif
  // gather / outputs: window-striding grids of 8 workgroups per CU (the
  // window count is known on the device only)
  const unsigned hgrid = (unsigned)std::min<size_t>(nwin_max, (size_t)h->ncu * 8);
  // one chain per group: segments [h0, h1) of the list on stream st, its
  // gather's event ev waited on by the main stream
  auto chain = [&](u32 h0, u32 h1, hipStream_t st, hipEvent_t ev, const char* ng,
                   const char* nf, const char* no) -> int {
    {
      Launch l(h, ng, st);
      k_gather_huge<<<hgrid, kBlock, 0, st>>>(hl, h1, hoff, woff, sg.sstart, sg.scnt, sg.sidx,
                                               sg.opr, hop, hval, sums, h0);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(ev, st));
    HIPCHK(h, hipStreamWaitEvent(h->stream, ev, 0));
    {
      Launch l(h, nf, st);
      k_fold_block<<<h1 - h0, kFoldThreads, 0, st>>>(hl, h1, sg.uslot, hoff, sg.scnt, hval, hop,
                                                     h->recs, rpos, rst, runn, segex, segxf, woff,
                                                     sums, wrun, wing, fold_dbg, h0);
    }
    HIPCHK(h, hipGetLastError());
    {
      Launch l(h, no, st);
#define PHIP_HUGE_OUT(M)                                                                         \
  k_huge_outputs<M><<<hgrid, kBlock, 0, st>>>(hl, h1, hoff, woff, sg.scnt, hval, hop, rpos, rst, \
                                              runn, segex, segxf, wrun, wing, ow, h0)
      PHIP_OUT_DISPATCH(out_mask(ow), PHIP_HUGE_OUT);
#undef PHIP_HUGE_OUT
    }
    HIPCHK(h, hipGetLastError());
    return PHIP_OK;
  };
  if ((rc = chain(0, hsplit, h->stream2, h->ev_gather, "k_gather_huge", "k_fold_block",
                  "k_huge_outputs")))
    return rc;
  if (split) {
    if ((rc = chain(hsplit, nhuge, h->stream3, h->ev_gather3, "k_gather_huge2", "k_fold_block2",
                    "k_huge_outputs2")))
      return rc;
    HIPCHK(h, hipEventRecord(h->ev_join3, h->stream3));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_join3, 0));
  }
  HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
  huge->ev = h->ev_join;
#ifdef PHIP_FOLD_STATS
  if ((rc = fold_stats_dump(h, fold_dbg, nhuge))) return rc;
#endif
  return PHIP_OK;
}

// The other segments' folds: the short ones, one thread each, on stream4
// (*threads: armed with ev_t4b), the long ones, one wave each, on the main
// stream.  sg->lng: replaced by the list in the order the wave folds took it.
int fold_rest(phip_handle* h, Segs* sg, const OutView& ow, Join* threads) {
  int rc;
  if ((rc = thread_stream(h))) return rc;
  hipStream_t ts = h->stream4;
  HIPCHK(h, hipEventRecord(h->ev_t4a, h->stream));
  HIPCHK(h, hipStreamWaitEvent(ts, h->ev_t4a, 0));
  {
    Launch l(h, "k_fold_thread", ts);
#define PHIP_FOLD_THREAD(M)                                                                  \
  k_fold_thread<M><<<grid_for(sg->nseg), kBlock, 0, ts>>>(sg->uslot, sg->sstart, sg->scnt, \
                                                          sg->nseg, sg->sidx, sg->opr, h->recs, ow)
    PHIP_OUT_DISPATCH(out_mask(ow), PHIP_FOLD_THREAD);
#undef PHIP_FOLD_THREAD
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipEventRecord(h->ev_t4b, ts));
  threads->ev = h->ev_t4b;
  const u32 nlong = sg->nlong;
  if (!nlong) return PHIP_OK;
  // the long segments over kBigLongSeg ops first (their sequential chains
  // are the longest), then the rest
  if (nlong > 1) {
    u32* lng2;
    u8* temp;
    if ((rc = ensure(h, B_LONG2, nlong, &lng2))) return rc;
    size_t tb = 0;
    HIPCHK(h, rocprim::partition(nullptr, tb, sg->lng, lng2, h->ctr + kCtrAux, (size_t)nlong,
                                 BigLongSeg{sg->scnt}, h->stream));
    if ((rc = ensure(h, B_TEMP, tb, &temp))) return rc;
    HIPCHK(h, rocprim::partition(temp, tb, sg->lng, lng2, h->ctr + kCtrAux, (size_t)nlong,
                                 BigLongSeg{sg->scnt}, h->stream));
    sg->lng = lng2;
  }
  Launch l(h, "k_fold_wave");
#define PHIP_FOLD_WAVE(M)                                                                      \
  k_fold_wave<M><<<nlong, 64, 0, h->stream>>>(sg->lng, nlong, sg->uslot, sg->sstart, sg->scnt, \
                                              sg->sidx, sg->opr, h->recs, ow)
  PHIP_OUT_DISPATCH(out_mask(ow), PHIP_FOLD_WAVE);
#undef PHIP_FOLD_WAVE
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// Apply a mixed op stream in seq order, by the schedule above.  The NEW flag
// of created buckets is consumed (cleared) by the fold itself.  behind: what
// runs once every fold has joined the main stream (ow.status is required).
template <class Src>
int ordered(phip_handle* h, Src src, u32 n, const OpView& ov, const OutView& ow,
            const Behind* behind = nullptr) {
  if (n == 0) return PHIP_OK;
  if (n > kMaxOrderedOps)
    return set_err(h, PHIP_ERR_INVALID, "ordered batch of %u ops exceeds 2^30", n);
  int rc;
  Segs sg{};
  Join pack{h}, threads{h}, huge{h};
  if ((rc = segment_batch(h, src, n, ov, &sg, &pack)) || (rc = pack.join())) return rc;
  if (sg.nhuge && (rc = fold_huge(h, sg, ow, &huge))) return rc;
  if ((rc = fold_rest(h, &sg, ow, &threads))) return rc;
  if ((rc = threads.join()) || (rc = huge.join())) return rc;
  return behind ? behind_folds(h, *behind, sg, ow.status) : PHIP_OK;
}

int stage_names(phip_handle* h, const uint8_t* names, const uint32_t* offs, u32 n, bool dev,
                NamesOffs* src, u32 names_len = 0) {
  const u32* d_offs;
  int rc;
  if ((rc = stage(h, B_OFFS, offs, (size_t)n + 1, dev, &d_offs))) return rc;
  const u8* d_names;
  size_t nb = 0;
  if (!dev) nb = offs[n];
  if ((rc = stage(h, B_NAMES, names, nb, dev, &d_names))) return rc;
  if (!dev && nb == 0) {
    u8* p;
    if ((rc = ensure(h, B_NAMES, 1, &p))) return rc;
    d_names = p;
  }
  src->blob = d_names;
  src->offs = d_offs;
  // (a device batch's offsets are checked on the device when the caller gave
  // the blob's length; a host batch's were checked on the host)
  src->lim = dev ? names_len : 0;
  return PHIP_OK;
}

// Datagram offsets from the host: non-decreasing, so every datagram the
// kernels read lies inside the bytes[offs[0] .. offs[n]) that were copied.
bool datagrams_ok(const uint64_t* offs, u32 n) {
  for (u32 i = 0; i < n; ++i)
    if (offs[i + 1] < offs[i]) return false;
  return true;
}

bool names_ok(const uint32_t* offs, u32 n) {
  for (u32 i = 0; i < n; ++i) {
    if (offs[i + 1] < offs[i]) return false;
    if (offs[i + 1] - offs[i] > PHIP_MAX_NAME_LEN) return false;
  }
  return true;
}

int outputs(phip_handle* h, const phip_results* res, u32 n, bool dev, OutView* ow) {
  int rc;
  phip_results r{};
  if (res) r = *res;
  if ((rc = out_buf(h, B_STATUS, r.status, n, dev, &ow->status)) ||
      (rc = out_buf(h, B_REM, r.remaining, n, dev, &ow->remaining)) ||
      (rc = out_buf(h, B_HAVE, r.have, n, dev, &ow->have)) ||
      (rc = out_buf(h, B_REPLY, r.reply, n, dev, &ow->reply)))
    return rc;
  // an entry with no reply state (a merged replica) reads as zeros, on every
  // path (the staged buffer would otherwise hand back an earlier call's data)
  if (ow->reply) HIPCHK(h, hipMemsetAsync(ow->reply, 0, (size_t)n * sizeof(phip_state), h->stream));
  return PHIP_OK;
}

// outputs() of a Receive batch.  It holds no TAKE op, and no receive path
// stores a remaining or have: a column of those the caller passed all the
// same reads zero in every entry (patrolhip.h "Result columns"), here as on
// the one-launch small path, instead of the caller's bytes (device form) or an
// earlier call's staged results (host form).  No cost unless they are passed.
int receive_outputs(phip_handle* h, const phip_results* res, u32 n, bool dev, OutView* ow) {
  if (int rc = outputs(h, res, n, dev, ow)) return rc;
  if (ow->remaining) HIPCHK(h, hipMemsetAsync(ow->remaining, 0, (size_t)n * 8, h->stream));
  if (ow->have) HIPCHK(h, hipMemsetAsync(ow->have, 0, (size_t)n * 8, h->stream));
  return PHIP_OK;
}

int copy_outputs(phip_handle* h, const phip_results* res, u32 n, bool dev, const OutView& ow) {
  if (!res || dev) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PHIP_OK;
  }
  int rc;
  if ((rc = copy_back(h, res->status, ow.status, n, dev)) ||
      (rc = copy_back(h, res->remaining, ow.remaining, n, dev)) ||
      (rc = copy_back(h, res->have, ow.have, n, dev)) ||
      (rc = copy_back(h, res->reply, ow.reply, n, dev)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

// A batch from message k on.
inline NamesOffs shifted(NamesOffs s, u32 k) {
  s.offs += k;
  return s;
}
inline NamesPairs shifted(NamesPairs s, u32 k) {
  s.off += k;
  s.len += k;
  return s;
}
inline OutView shifted(OutView o, u32 k) {
  if (o.status) o.status += k;
  if (o.remaining) o.remaining += k;
  if (o.have) o.have += k;
  if (o.reply) o.reply += k;
  return o;
}

// ------------------------------------------------ incast reply egress ----
// phip_receive_*_replies (patrolhip.h "Incast reply egress"; kernels in
// phip_kernels.hpp under the same heading).  A call's ReplyEg travels with the
// batch to the path that holds its replies: run_deferred (reply_deferred) or
// the ordered suffix (reply_suffix); a batch that reaches neither launched
// nothing and reply_collect writes the zeros on the host.
struct ReplyEg {
  phip_reply_egress* rq;   // the caller's (host memory), out fields zeroed at entry
  bool dev;                // out / offs / src are device memory
  u64 budget;              // bytes the datagrams may take
  ReplyOut R{};            // where the kernels write (reply_begin)
  bool launched = false;
};

// Output buffers for at most `bound` replies (the caller's, or the handle's
// for a host-pointer call) and the cleared counter block.
int reply_begin(phip_handle* h, ReplyEg* eg, u64 bound) {
  int rc;
  const phip_reply_egress& q = *eg->rq;
  ReplyOut& R = eg->R;
  R.out = q.out;
  R.offs = reinterpret_cast<u64*>(q.offs);
  R.src = q.src;
  R.max_msgs = q.max_msgs;
  R.budget = eg->budget;
  if (!eg->dev) {
    const u64 msgs = std::min<u64>(q.max_msgs, bound);
    if ((rc = ensure(h, B_RQOUT, (size_t)std::min<u64>(eg->budget, msgs * PHIP_BUCKET_PACKET_SIZE),
                     &R.out)) ||
        (rc = ensure(h, B_RQOFFS, (size_t)msgs + 1, &R.offs)) ||
        (rc = ensure(h, B_RQSRC, (size_t)msgs, &R.src)))
      return rc;
  }
  if ((rc = ensure(h, B_RQCTR, kRqWords, &R.ctr))) return rc;
  HIPCHK(h, hipMemsetAsync(R.ctr, 0, kRqWords * sizeof(u64), h->stream));
  eg->launched = true;
  return PHIP_OK;
}

// The deferred sub-batch's replies: selected and ordered by batch index in one
// workgroup, written one lane per datagram.  No column of the batch's size.
int reply_deferred(phip_handle* h, ReplyEg* eg, const SubBatch& sb, const u8* blob, const u8* st2,
                   const phip_state* rep2, u32 nd) {
  int rc;
  u32* sel;
  if ((rc = reply_begin(h, eg, kDirtyCap)) || (rc = ensure(h, B_RQSEL, kDirtyCap, &sel))) return rc;
  const NamesPairs names{blob, sb.off, sb.len};
  {
    Launch l(h, "k_reply_select");
    k_reply_select<<<1, kReplySelBlock, 0, h->stream>>>(sb.map, st2, nd, names, sel, eg->R);
  }
  {
    Launch l(h, "k_reply_write");
    const u32 most = std::min<u32>(std::min<u32>(nd, kDirtyCap), eg->R.max_msgs);
    k_reply_write<<<grid_for(most), kBlock, 0, h->stream>>>(sel, rep2, names, eg->R);
  }
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// The ordered suffix's replies from its status and reply columns (m messages
// from batch index `first` on, already in batch order): count, scan, write.
template <class Src>
int reply_suffix(phip_handle* h, ReplyEg* eg, Src src, const u8* status, const phip_state* reply,
                 u32 m, u32 first) {
  int rc;
  const u32 ntiles = grid_for(m);
  u64* tile_bytes;
  if ((rc = reply_begin(h, eg, m)) || (rc = ensure(h, B_RQTILE, 2 * (size_t)ntiles, &tile_bytes)))
    return rc;
  u32* tile_cnt = (u32*)(tile_bytes + ntiles);
  {
    Launch l(h, "k_reply_count");
    k_reply_count<<<ntiles, kBlock, 0, h->stream>>>(src, status, m, tile_cnt, tile_bytes, eg->R.ctr);
  }
  {
    Launch l(h, "k_reply_scan");
    k_reply_scan<<<1, kSweepBlock, 0, h->stream>>>(tile_cnt, tile_bytes, ntiles, eg->R.ctr);
  }
  {
    Launch l(h, "k_reply_place");
    k_reply_place<<<ntiles, kBlock, 0, h->stream>>>(src, status, reply, m, first, tile_cnt,
                                                     tile_bytes, eg->R);
  }
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// The call's out fields; a host-pointer call gets back only what was written.
// A batch whose replies no path was reached for has none: zeros, offs[0] = 0
// (a device offs[0] is cleared on the stream; sync: the caller's own
// synchronise does not follow).
int reply_collect(phip_handle* h, ReplyEg* eg, bool sync = false) {
  phip_reply_egress& q = *eg->rq;
  if (!eg->launched) return datagrams_none(h, q.offs, eg->dev, sync);
  int rc;
  u64 c[kRqWords];
  HIPCHK(h, hipMemcpyAsync(c, eg->R.ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (c[kRqErr] || c[kRqN] > q.max_msgs || c[kRqBytes] > eg->budget ||
      c[kRqN] + c[kRqSkipped] > c[kRqReplies])
    return set_err(h, PHIP_ERR_INVALID,
                   "internal: reply egress wrote %llu datagrams, %llu bytes of %llu replies (flag %llu)",
                   (unsigned long long)c[kRqN], (unsigned long long)c[kRqBytes],
                   (unsigned long long)c[kRqReplies], (unsigned long long)c[kRqErr]);
  if (!eg->dev) {
    if ((rc = datagrams_back(h, q.out, eg->R.out, c[kRqBytes], q.offs, eg->R.offs, c[kRqN])))
      return rc;
    if (q.src && c[kRqN])
      HIPCHK(h, hipMemcpyAsync(q.src, eg->R.src, c[kRqN] * sizeof(u32), hipMemcpyDeviceToHost,
                               h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  q.n = (u32)c[kRqN];
  q.bytes = c[kRqBytes];
  q.replies = (u32)c[kRqReplies];
  q.skipped = (u32)c[kRqSkipped];
  return PHIP_OK;
}

// The last fast pass's ordered sub-batch (nd entries: its dirty buckets' dirty
// messages and the merges of their cells, dirty_finish) through the ordered path,
// its statuses and replies scattered back.  The dirty buckets' other
// messages were merged by the fast pass (before each bucket's first dirty
// message) or folded into the cells (after it); no other bucket is touched,
// and Receive is per bucket (repo.go:77-106), so applying the sub-batch
// after the rest of the batch gives each dirty bucket the Go loop's states.
// eg: the batch's incast replies are written from the sub-batch's own statuses
// and reply states (reply_deferred), whatever columns the caller asked for.
template <class Src>
int run_deferred(phip_handle* h, Src src, i64 now, const OutView& ow, u32 nd,
                 ReplyEg* eg = nullptr) {
  // (kSubBatchOver included: dirty_finish counted more entries than the
  // sub-batch holds and wrote none)
  if (nd > kSubBatchCap) {
    h->stats.ordered = 0;
    return set_err(h, PHIP_ERR_HIP, "ordered sub-batch over its %u entries", kSubBatchCap);
  }
  h->stats.ordered = nd;
  if (nd == 0) return PHIP_OK;
  int rc;
  SubBatch sb;
  u8* st2 = nullptr;
  phip_state* rep2 = nullptr;
  if ((rc = sub_batch(h, &sb)) || ((ow.status || eg) && (rc = ensure(h, B_SSTAT, nd, &st2))) ||
      ((ow.reply || eg) && (rc = ensure(h, B_SREP, nd, &rep2))))
    return rc;
  if (rep2) HIPCHK(h, hipMemsetAsync(rep2, 0, (size_t)nd * sizeof(phip_state), h->stream));
  OpView ov{};
  ov.kind = nullptr; ov.kind0 = PHIP_OP_RECEIVE;
  ov.now = nullptr; ov.now0 = now;
  ov.a = sb.a; ov.t = sb.t; ov.e = sb.e;
  if ((rc = ordered(h, NamesPairs{src.blob, sb.off, sb.len}, nd, ov,
                    OutView{st2, nullptr, nullptr, rep2})))
    return rc;
  if (ow.status || ow.reply) {
    k_defer_scatter<<<grid_for(nd), kBlock, 0, h->stream>>>(sb.map, nd, st2, rep2, ow);
    HIPCHK(h, hipGetLastError());
  }
  if (eg) return reply_deferred(h, eg, sb, src.blob, st2, rep2, nd);
  return PHIP_OK;
}

// After the fast path, what its outcome left: the clean prefix's new buckets
// (finish_misses), then the ordered path over messages [first_dirty, stop),
// which starts from the state the prefix left (the Go loop's state at that
// message) -- or, when the fast pass deferred the dirty buckets
// (first_dirty == n), over their messages (run_deferred).
// eg: the batch's incast replies, from whichever of the two holds them (a
// clean message is no request); the suffix's status and reply columns are the
// caller's, or the handle's own for the suffix alone.
template <class Src>
int finish_receive(phip_handle* h, Src src, const uint64_t* a, const uint64_t* t,
                   const int64_t* e, i64 now, const OutView& ow, FastOutcome o,
                   ReplyEg* eg = nullptr) {
  int rc;
  const bool deferred = o.ndef != 0;   // (the first pass's; finish_misses may run a second)
  if ((rc = finish_misses(h, src, a, t, e, now, ow.status, &o))) return rc;
  if (deferred) return run_deferred(h, src, now, ow, o.ndef, eg);
  const u32 stop = o.stop, k = o.first_dirty;
  h->stats.ordered = k < stop ? stop - k : 0;
  if (k >= stop) return PHIP_OK;
  OpView ov{};
  ov.kind = nullptr; ov.kind0 = PHIP_OP_RECEIVE;
  ov.now = nullptr; ov.now0 = now;
  ov.a = a + k; ov.t = t + k; ov.e = e + k;
  OutView ow2 = shifted(ow, k);
  if (eg && ((!ow2.status && (rc = ensure(h, B_RQSTAT, stop - k, &ow2.status))) ||
             (!ow2.reply && (rc = ensure(h, B_RQREP, stop - k, &ow2.reply)))))
    return rc;
  if ((rc = ordered(h, shifted(src, k), stop - k, ov, ow2))) return rc;
  return eg ? reply_suffix(h, eg, shifted(src, k), ow2.status, ow2.reply, stop - k, k) : PHIP_OK;
}

// Statuses of a batch that stopped at message `stop` (kCtrStop), as the Go
// loop exits at a short datagram (repo.go:70-74): that message reads
// PHIP_ST_SHORT, every later one PHIP_ST_NOT_PROCESSED.
int fill_stopped(phip_handle* h, u8* status, u32 n, u32 stop) {
  if (!status || stop >= n) return PHIP_OK;
  HIPCHK(h, hipMemsetAsync(status + stop, PHIP_ST_NOT_PROCESSED, n - stop, h->stream));
  HIPCHK(h, hipMemsetAsync(status + stop, PHIP_ST_SHORT, 1, h->stream));
  return PHIP_OK;
}

// A checked batch (names_len) whose first malformed name entry is message
// `stop` < n (k_classify_soa2) stopped there: the call returns
// PHIP_ERR_INVALID.
int stopped_at_bad_name(phip_handle* h, const OutView& ow, u32 n, u32 stop) {
  if (stop >= n) return PHIP_OK;
  if (int rc = fill_stopped(h, ow.status, n, stop)) return rc;
  if (ow.status) HIPCHK(h, hipStreamSynchronize(h->stream));
  return set_err(h, PHIP_ERR_INVALID,
                 "malformed name offsets at message %u (names_len check): the batch stopped there",
                 stop);
}

// Receive-mode batch (decoded): the fast path over its clean prefix, the
// ordered path from its first incast or -0.0 on.
template <class Src>
int receive_decoded(phip_handle* h, Src src, const uint64_t* a, const uint64_t* t,
                    const int64_t* e, u32 n, i64 now, const OutView& ow, PassAsk ask,
                    ReplyEg* eg = nullptr) {
  int rc;
  FastOutcome o;
  if ((rc = fast_apply(h, SoaIn<Src>{src, a, t, e}, src, n, ow.status, ask, &o)) ||
      (rc = finish_receive(h, src, a, t, e, now, ow, o, eg)))
    return rc;
  // (a batch that stopped had sent the replies before: they are collected first)
  if (eg && (rc = reply_collect(h, eg))) return rc;
  return stopped_at_bad_name(h, ow, n, o.stop);   // (a checked batch's malformed entry)
}

// PHIP_RECV_ASYNC: the queued batch's counters, then what its fast pass left
// (misses, dirty buckets).  *worked: whether anything was left (its work
// has used the counters and maybe moved the table).
int finish_pending(phip_handle* h, bool* worked, bool* shut) {
  if (worked) *worked = false;
  if (shut) *shut = false;
  if (!h->pend.active) return PHIP_OK;
  phip_handle::Pending p = h->pend;
  h->pend.active = false;
  HIPCHK(h, hipEventSynchronize(h->ev_ctr[p.pass.par]));
  // (the words a successor's gate read, before a second pass of this batch
  // stores its own over them)
  if (shut && (*shut = gate_shut(fmirror(h, p.pass.par))))
    h->hot_clean = nullptr;   // (the gated kernel cleared no count table: a front's k_hot_dir may have run)
  if (p.pass.gate && fmirror(h, p.pass.par)[kCtrGateShut])
    return set_err(h, PHIP_ERR_INVALID, "internal: a pass ran on as gated, its kernel found the gate shut");
  int rc;
  FastOutcome o;
  // (a failed speculation runs a fast pass of its own: the caller queues its front again)
  if ((rc = fast_settle(h, p.in, p.in.src, p.ow.status, &p.pass, &o))) return rc;
  if (!o.again && o.nmiss == 0 && o.first_dirty >= o.stop && o.ndef == 0)
    return stopped_at_bad_name(h, p.ow, p.pass.n, o.stop);   // (a checked batch's malformed entry)
  if (worked) *worked = true;
  if ((rc = finish_receive(h, p.in.src, p.in.ma, p.in.mt, p.in.me, p.now, p.ow, o)) ||
      (rc = stopped_at_bad_name(h, p.ow, p.pass.n, o.stop)))
    return rc;
  // The leftover work (the miss merges, the ordered path's folds, which also
  // join stream2/stream4 into the handle's stream) writes this batch's
  // statuses and replies: they are final when the call that finished the
  // batch returns (patrolhip.h PHIP_RECV_ASYNC), and the caller may then
  // free or reuse them.  Only batches that left work pay this wait.
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

// Whether an op's phip_results.reply entry is written (step_sop): Takes,
// Upserts and incast requests carry the bucket's state right after the op.
inline bool has_reply_state(u8 status, u8 kind) {
  const u8 st = status & 0x7F;
  return kind == PHIP_OP_TAKE || kind == PHIP_OP_UPSERT || st == PHIP_ST_INCAST_REPLY ||
         st == PHIP_ST_INCAST_NOREPLY;
}

// A host-pointer batch of at most kSmallMax ops through k_small_mixed: one
// pinned copy in, one launch, one pinned copy out (the large path takes a
// dozen launches and several host round trips, ~0.2 ms whatever the size).
// *done = false leaves the batch to the large path with nothing changed: too
// many ops or name bytes, a bucket bound past the load limit (the large path
// grows the table), or a long-name arena the kernel found too small.
// eg (phip_apply_mixed_egress, its caps checked by the caller): the same
// launch, k_small_mixed<true>, also writes the batch's egress into the staging
// buffer; it travels back with the results when its worst case is small, and
// in a second copy of just the bytes written otherwise.
// track (phip_apply_mixed on a handle that keeps a change set, never with eg):
// the same launch, k_small_mixed<false, true>, also sets the batch's marks.
int small_mixed(phip_handle* h, const phip_ops* ops, const phip_results* res, bool* done,
                phip_egress* eg = nullptr, bool track = false) {
  *done = false;
  const u32 n = ops->n;
  if (n > kSmallMax || h->n_buckets + n > h->max_load) return PHIP_OK;
  const u64 nbytes = ops->name_offs[n];
  if (nbytes > (u64)kSmallMax * PHIP_MAX_NAME_LEN) return PHIP_OK;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const bool take = ops->freq != nullptr, state = ops->added != nullptr;
  // inputs: offsets | kind | now | freq per count | added taken elapsed | names
  const size_t o_kind = al(4 * ((size_t)n + 1)), o_now = o_kind + al(n), o_freq = o_now + 8 * n;
  const size_t o_per = o_freq + 8 * n, o_count = o_per + 8 * n, o_a = o_count + 8 * n;
  const size_t o_t = o_a + 8 * n, o_e = o_t + 8 * n, o_names = o_e + 8 * n;
  const size_t in_bytes = al(o_names + nbytes + 8);
  // outputs: header | status | remaining | have | reply
  const size_t o_st = sizeof(SmallHdr), o_rem = al(o_st + n), o_have = o_rem + 8 * n;
  const size_t o_reply = o_have + 8 * n, out_bytes = o_reply + sizeof(phip_state) * n;
  // egress: header | offsets | datagrams (the batch's worst case, 8 bytes of slack)
  const u32 eg_msgs = 2 * n;
  const u64 eg_budget = 2 * ((u64)PHIP_BUCKET_FIXED_SIZE * n + (nbytes - ops->name_offs[0]));
  const size_t o_eg = al(out_bytes), o_egoffs = o_eg + sizeof(SmallEgHdr);
  const size_t o_egdata = al(o_egoffs + 8 * ((size_t)eg_msgs + 1));
  const size_t eg_end = al(o_egdata + (size_t)eg_budget + 8);
  const size_t total = in_bytes + (eg ? eg_end : out_bytes);
  if (h->small_pin_cap < total) {
    if (h->small_pin) HIPCHK(h, hipHostFree(h->small_pin));
    h->small_pin = nullptr;
    h->small_pin_cap = 0;
    const size_t want = std::max<size_t>(total, 1 << 20);
    HIPCHK(h, hipHostMalloc(&h->small_pin, want, 0));
    h->small_pin_cap = want;
  }
  u8 *d = nullptr, *pin = h->small_pin;
  int rc;
  if ((rc = ensure(h, B_SMALL, total, &d))) return rc;
  std::memcpy(pin, ops->name_offs, 4 * ((size_t)n + 1));
  std::memcpy(pin + o_kind, ops->kind, n);
  std::memcpy(pin + o_now, ops->now, 8 * n);
  if (take) {
    std::memcpy(pin + o_freq, ops->freq, 8 * n);
    std::memcpy(pin + o_per, ops->per, 8 * n);
    std::memcpy(pin + o_count, ops->count, 8 * n);
  }
  if (state) {
    std::memcpy(pin + o_a, ops->added, 8 * n);
    std::memcpy(pin + o_t, ops->taken, 8 * n);
    std::memcpy(pin + o_e, ops->elapsed, 8 * n);
  }
  std::memcpy(pin + o_names, ops->names, nbytes);
  std::memset(pin + o_names + nbytes, 0, 8);
  std::memset(pin + in_bytes, 0, sizeof(SmallHdr));
  HIPCHK(h, hipMemcpyAsync(d, pin, in_bytes + sizeof(SmallHdr), hipMemcpyHostToDevice, h->stream));
  NamesOffs src{d + o_names, (const u32*)d};
  OpView ov{};
  ov.kind = d + o_kind;
  ov.now = (const int64_t*)(d + o_now);
  if (take) {
    ov.freq = (const int64_t*)(d + o_freq);
    ov.per = (const int64_t*)(d + o_per);
    ov.count = (const uint64_t*)(d + o_count);
  }
  if (state) {
    ov.a = (const uint64_t*)(d + o_a);
    ov.t = (const uint64_t*)(d + o_t);
    ov.e = (const int64_t*)(d + o_e);
  }
  u8* dout = d + in_bytes;
  phip_results r{};
  if (res) r = *res;
  OutView ow{};
  // (the egress and the marks read who created what; the reply column's
  // filter below reads which RECEIVE ops were incast requests)
  ow.status = (r.status || r.reply || eg || track) ? dout + o_st : nullptr;
  ow.remaining = r.remaining ? (uint64_t*)(dout + o_rem) : nullptr;
  ow.have = r.have ? (uint64_t*)(dout + o_have) : nullptr;
  ow.reply = r.reply ? (phip_state*)(dout + o_reply) : nullptr;
  {
    Launch l(h, "k_small_mixed");
    if (eg)
      k_small_mixed<true><<<1, kSmallMax, 0, h->stream>>>(
          src, ov, n, table(h), h->arena, h->arena_cap, h->arena_cursor, ow, (SmallHdr*)dout,
          SmallEgress<true>{dout + o_egdata, (u64*)(dout + o_egoffs), (SmallEgHdr*)(dout + o_eg),
                            eg_msgs, eg_budget});
    else if (track)
      k_small_mixed<false, true><<<1, kSmallMax, 0, h->stream>>>(
          src, ov, n, table(h), h->arena, h->arena_cap, h->arena_cursor, ow, (SmallHdr*)dout,
          SmallEgress<false>{}, SmallMarks<true>{h->marks});
    else
      k_small_mixed<false><<<1, kSmallMax, 0, h->stream>>>(src, ov, n, table(h), h->arena,
                                                           h->arena_cap, h->arena_cursor, ow,
                                                           (SmallHdr*)dout, SmallEgress<false>{});
  }
  HIPCHK(h, hipGetLastError());
  // the header and the columns the caller asked for, in one copy (with the
  // egress: its header too, and all of it when its worst case is small)
  constexpr size_t kEgOneCopy = 64 << 10;
  const bool eg_one = eg && eg_end - o_eg <= kEgOneCopy;
  const size_t back = eg ? (eg_one ? eg_end : o_egoffs)
                         : r.reply ? out_bytes : r.have ? o_reply : r.remaining ? o_have : o_rem;
  u8* pout = pin + in_bytes;
  HIPCHK(h, hipMemcpyAsync(pout, dout, back, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  SmallHdr hd;
  std::memcpy(&hd, pout, sizeof hd);
  h->n_buckets += hd.created;
  if (hd.fallback) return PHIP_OK;
  if (hd.full) return set_err(h, PHIP_ERR_FULL, "internal: small batch probe wrapped the table");
  if (eg) {
    SmallEgHdr eh;
    std::memcpy(&eh, pout + o_eg, sizeof eh);
    if (eh.err || eh.n > eg_msgs || eh.n_incast > eh.n || eh.bytes > eg_budget)
      return set_err(h, PHIP_ERR_INVALID, "internal: egress of %u datagrams, %llu bytes (flag %u)",
                     eh.n, (unsigned long long)eh.bytes, eh.err);
    if (!eg_one) {
      // only what was written travels back
      HIPCHK(h, hipMemcpyAsync(pout + o_egoffs, dout + o_egoffs, 8 * ((size_t)eh.n + 1),
                               hipMemcpyDeviceToHost, h->stream));
      if (eh.bytes)
        HIPCHK(h, hipMemcpyAsync(pout + o_egdata, dout + o_egdata, eh.bytes, hipMemcpyDeviceToHost,
                                 h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    std::memcpy(eg->offs, pout + o_egoffs, 8 * ((size_t)eh.n + 1));
    std::memcpy(eg->out, pout + o_egdata, eh.bytes);
    eg->n_incast = eh.n_incast;
    eg->n = eh.n;
    eg->bytes = eh.bytes;
  }
  if (r.status) std::memcpy(r.status, pout + o_st, n);
  if (r.remaining) std::memcpy(r.remaining, pout + o_rem, 8 * n);
  if (r.have) std::memcpy(r.have, pout + o_have, 8 * n);
  if (r.reply) {
    // reply states are defined for Takes, Upserts and incasts (step_sop);
    // the other entries read as zeros, as on the large path (outputs())
    const phip_state* src_r = (const phip_state*)(pout + o_reply);
    // (the statuses came back in the same copy: ow.status is set whenever
    // the reply column is asked for)
    const u8* stp = pout + o_st;
    for (u32 i = 0; i < n; ++i)
      r.reply[i] = has_reply_state(stp[i], ops->kind ? ops->kind[i] : (u8)PHIP_OP_RECEIVE)
                       ? src_r[i] : phip_state{};
  }
  *done = true;
  return PHIP_OK;
}


// A uniform-kind host batch (Receive or Upsert of decoded states, all at one
// clock reading) through small_mixed: the ordered code is the same Go loop
// (repo.go:78-90, :215-235), so statuses, replies and states are those of
// the large paths.
int small_uniform(phip_handle* h, const phip_msgs* m, u8 kind, int64_t now, const phip_results* res,
                  bool* done) {
  *done = false;
  if (!h->small || m->n > kSmallMax) return PHIP_OK;
  std::vector<u8> kinds(m->n, kind);
  std::vector<int64_t> nows(m->n, now);
  phip_ops ops{};
  ops.n = m->n;
  ops.kind = kinds.data();
  ops.names = m->names;
  ops.name_offs = m->name_offs;
  ops.now = nows.data();
  ops.added = m->added;
  ops.taken = m->taken;
  ops.elapsed = m->elapsed;
  return small_mixed(h, &ops, res, done);
}

// The incast replies of a small batch, marshalled on the host from the result
// block its one launch copied back: the messages whose status is a reply, in
// batch order, the first that fit both caps (the device paths' cut: nothing
// is written behind a reply that did not fit).
void marshal_replies(const uint8_t* names, const uint32_t* name_offs, const uint8_t* status,
                     const phip_state* reply, u32 n, phip_reply_egress* rq) {
  u64 pos = 0;
  u32 m = 0;
  bool cut = false;
  rq->offs[0] = 0;
  for (u32 i = 0; i < n; ++i) {
    if ((status[i] & 0x7F) != PHIP_ST_INCAST_REPLY) continue;
    ++rq->replies;
    const u32 len = name_offs[i + 1] - name_offs[i];
    if (len > PHIP_MAX_NAME_LEN) {   // (bucket.go:48: no datagram carries it)
      ++rq->skipped;
      continue;
    }
    cut = cut || m >= rq->max_msgs || pos + PHIP_BUCKET_FIXED_SIZE + len > rq->out_cap;
    if (cut) continue;
    pos += (u64)phip_marshal(names + name_offs[i], len, &reply[i], rq->out + pos);
    if (rq->src) rq->src[m] = i;
    rq->offs[++m] = pos;
  }
  rq->n = m;
  rq->bytes = pos;
}

// small_uniform for a Receive batch whose replies are asked for (rq): the
// same launch, with the status and reply columns in the block it copies back
// whether or not the caller takes them.
int small_uniform_replies(phip_handle* h, const phip_msgs* m, int64_t now, const phip_results* res,
                          phip_reply_egress* rq, bool* done) {
  *done = false;
  if (!h->small || m->n > kSmallMax) return PHIP_OK;
  std::vector<u8> st;
  std::vector<phip_state> rp;
  phip_results r{};
  if (res) r = *res;
  if (!r.status) { st.resize(m->n); r.status = st.data(); }
  if (!r.reply) { rp.resize(m->n); r.reply = rp.data(); }
  if (int rc = small_uniform(h, m, PHIP_OP_RECEIVE, now, &r, done)) return rc;
  if (*done) marshal_replies(m->names, m->name_offs, r.status, r.reply, m->n, rq);
  return PHIP_OK;
}

// ReplicatedRepo.Receive over at most kSmallMax host datagrams: decoded on
// the host (UnmarshalBinary, bucket.go:71-91: a datagram under 25 bytes or
// shorter than its name is io.ErrShortBuffer, where the Go loop stops), the
// prefix before the first short one through small_mixed.  rq: that prefix's
// incast replies (small_uniform_replies).
int small_datagrams(phip_handle* h, const uint8_t* bytes, const uint64_t* offs, uint32_t n,
                    int64_t now, const phip_results* res, uint32_t* stop_index, bool* done,
                    phip_reply_egress* rq = nullptr) {
  *done = false;
  if (!h->small || n > kSmallMax) return PHIP_OK;
  std::vector<uint64_t> a(n), t(n);
  std::vector<int64_t> e(n);
  std::vector<uint32_t> no(n + 1);
  std::vector<uint8_t> names;
  names.reserve((size_t)n * 16 + 8);
  auto be64 = [](const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v = (v << 8) | p[k];
    return v;
  };
  u32 stop = n;
  for (u32 i = 0; i < n; ++i) {
    const uint8_t* d = bytes + offs[i];
    const uint64_t sz = offs[i + 1] - offs[i];
    if (sz < PHIP_BUCKET_FIXED_SIZE || sz - PHIP_BUCKET_FIXED_SIZE < d[24]) { stop = i; break; }
    a[i] = be64(d);
    t[i] = be64(d + 8);
    e[i] = (int64_t)be64(d + 16);
    no[i] = (uint32_t)names.size();
    names.insert(names.end(), d + PHIP_BUCKET_FIXED_SIZE, d + PHIP_BUCKET_FIXED_SIZE + d[24]);
  }
  no[stop] = (uint32_t)names.size();
  names.resize(names.size() + 8, 0);
  if (stop) {
    phip_msgs m{};
    m.n = stop;
    m.names = names.data();
    m.name_offs = no.data();
    m.added = a.data();
    m.taken = t.data();
    m.elapsed = e.data();
    bool ok = false;
    int rc;
    if ((rc = rq ? small_uniform_replies(h, &m, now, res, rq, &ok)
                 : small_uniform(h, &m, PHIP_OP_RECEIVE, now, res, &ok)))
      return rc;
    if (!ok) return PHIP_OK;   // the large path takes the whole batch
  } else if (rq) {
    rq->offs[0] = 0;
  }
  if (res && stop < n) {   // the short datagram and everything after it
    if (res->status) {
      std::memset(res->status + stop, PHIP_ST_NOT_PROCESSED, n - stop);
      res->status[stop] = PHIP_ST_SHORT;
    }
    // (the other columns read zero from the stop on, as on the large path)
    if (res->remaining) std::memset(res->remaining + stop, 0, 8 * (size_t)(n - stop));
    if (res->have) std::memset(res->have + stop, 0, 8 * (size_t)(n - stop));
    if (res->reply) std::memset(res->reply + stop, 0, sizeof(phip_state) * (size_t)(n - stop));
  }
  if (stop_index) *stop_index = stop;
  *done = true;
  if (stop < n) return set_err(h, PHIP_ERR_SHORT_BUFFER, "short buffer at datagram %u", stop);
  return PHIP_OK;
}
}  // namespace

// ------------------------------------------------------- owner routing ----
// The pack of phip_route_pack (and of phip_group_receive's chunks), queued on
// stream `st` without a host synchronisation.
// One workgroup per tile of `span` messages.  12 workgroups
// per CU: k_route_count holds 4 per CU, k_route_scatter 3, so both grids run
// in whole rounds (no tail round of a quarter of the chip).
// (tiles per CU: 12 = whole rounds of both grids; fewer, longer tiles also
// mean fewer combined messages, one per hot name a workgroup saw)
#ifndef PHIP_ROUTE_WG_PER_CU
#define PHIP_ROUTE_WG_PER_CU 12
#endif
struct RoutePlan {
  u32 nblk, ntile, span;
  size_t cells;
};
static RoutePlan route_plan(const phip_handle* h, u32 n, u32 world) {
  RoutePlan p;
  p.nblk = (u32)std::max<u64>(1, std::min<u64>((n + kRouteStep - 1) / kRouteStep,
                                                (u64)h->ncu * PHIP_ROUTE_WG_PER_CU));
  p.ntile = p.nblk;   // one tile per workgroup, a whole number of scatter steps
  p.span = (u32)((((u64)n + p.ntile - 1) / p.ntile + kRouteStep - 1) / kRouteStep * kRouteStep);
  p.cells = (size_t)world * p.ntile;
  return p;
}

// Scratch of a pack of up to n messages, all in B_ROUTE: the per-(owner,
// tile) cells, the route codes, its own counter block and the scans'
// temporary storage.  Sized before anything is queued: the packs of a
// pipelined exchange reuse it in stream order, and the owner's merges that
// run beside them (phip_group_receive) touch none of it.
static int route_scratch(phip_handle* h, u32 n, u32 world, u8** base, u32** pctr, size_t* scan_bytes,
                         u8** temp) {
  const RoutePlan p = route_plan(h, n, world);
  size_t tb = 0;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, (u32*)nullptr, (u32*)nullptr, 0u, p.cells,
                                    rocprim::plus<u32>(), h->stream));
  // cells | codes | counter block | scan temp (16-byte aligned parts)
  const size_t ctr_off = (4 * p.cells * sizeof(u32) + 2 * (size_t)n + 15) & ~(size_t)15;
  const size_t tmp_off = (ctr_off + kCtrWords * sizeof(u32) + 255) & ~(size_t)255;
  int rc;
  if ((rc = ensure(h, B_ROUTE, tmp_off + tb, base))) return rc;
  *pctr = (u32*)(*base + ctr_off);
  *scan_bytes = tb;
  *temp = *base + tmp_off;
  return PHIP_OK;
}

// Sender-side combine: the hot names of a strided sample of the
// whole batch, counted by name hash (the buckets live on other ranks, so
// there is no slot to count), as a directory for every pack of the batch.
// Src: the batch's name source (NamesOffs: decoded messages; Datagrams: raw
// datagrams, phip_route_pack_datagrams).
template <class Src>
static int route_dir_src(phip_handle* h, hipStream_t st, const Src& src, u32 n, u32 world,
                         const void** out) {
  *out = nullptr;
  if (n < kRouteMinBatch) return PHIP_OK;
  constexpr size_t kCnt = size_t(1) << kHotCntBits;
  const size_t zero_bytes = 3 * kCnt * sizeof(u32) + kHotHist * sizeof(u32) + sizeof(HotHdr);
  u8* hb;
  int rc;
  if ((rc = ensure(h, B_RHOT, zero_bytes + kRouteHotMax * sizeof(RouteHot), &hb))) return rc;
  u32* ckeys = (u32*)hb;
  u32* ccnt = ckeys + kCnt;
  u32* cidx = ccnt + kCnt;
  u32* hist = cidx + kCnt;
  HotHdr* hdr = (HotHdr*)(hist + kHotHist);
  RouteHot* d = (RouteHot*)(hdr + 1);
  HIPCHK(h, hipMemsetAsync(hb, 0, zero_bytes, st));
  const u32 stride = std::max<u32>(64, (n + kHotSampleMax - 1) / kHotSampleMax);
  const u32 nsample = (n + stride - 1) / stride;
  {
    Launch l(h, "k_route_sample", st);
    k_route_sample<Src><<<grid_for(nsample, kHotSamplePerBlock), 256, 0, st>>>(
        src, n, stride, nsample, ckeys, ccnt, cidx);
    k_hot_hist<<<grid_for(kCnt), kBlock, 0, st>>>(ccnt, hist);
    k_hot_select<<<1, 256, 0, st>>>(hist, hdr, kRouteHotMax);
    k_route_dir_build<Src><<<grid_for(kCnt), kBlock, 0, st>>>(ckeys, ccnt, cidx, hdr, src, world, d);
  }
  HIPCHK(h, hipGetLastError());
  *out = hdr;
  return PHIP_OK;
}
static int route_dir_on(phip_handle* h, hipStream_t st, const phip_msgs& m, u32 world, const void** out) {
  return route_dir_src(h, st, NamesOffs{m.names, m.name_offs, m.names_len}, m.n, world, out);
}

// The skeleton of a stable owner partition of n entries, queued on `st` with
// no host synchronisation: the plan and scratch (B_ROUTE), the per-(owner,
// tile) cells, their two scans and the per-owner totals into counts / nbytes
// (device).  `count` fills cnt / bytes / code and `scatter` writes the send
// buffers from cbase / bbase; both launch on `st` with the plan and the
// carved scratch.
struct RouteCells {
  u32 *cnt, *bytes, *cbase, *bbase, *pctr;
  u16* code;
};
template <class Count, class Scatter>
static int route_pack_with(phip_handle* h, hipStream_t st, u32 n, u32 world, uint64_t* counts,
                           uint64_t* nbytes, Count count, Scatter scatter) {
  if (n == 0) {
    HIPCHK(h, hipMemsetAsync(counts, 0, world * sizeof(uint64_t), st));
    HIPCHK(h, hipMemsetAsync(nbytes, 0, world * sizeof(uint64_t), st));
    return PHIP_OK;
  }
  const RoutePlan p = route_plan(h, n, world);
  u8 *base, *temp;
  RouteCells c;
  size_t tb;
  int rc;
  if ((rc = route_scratch(h, n, world, &base, &c.pctr, &tb, &temp))) return rc;
  c.cnt = (u32*)base;
  c.bytes = c.cnt + p.cells;
  c.cbase = c.bytes + p.cells;
  c.bbase = c.cbase + p.cells;
  c.code = (u16*)(c.bbase + p.cells);
  count(p, c);
  HIPCHK(h, hipGetLastError());
  {
    Launch l(h, "route_scan", st);
    HIPCHK(h, rocprim::exclusive_scan(temp, tb, c.cnt, c.cbase, 0u, p.cells, rocprim::plus<u32>(),
                                      st));
    HIPCHK(h, rocprim::exclusive_scan(temp, tb, c.bytes, c.bbase, 0u, p.cells, rocprim::plus<u32>(),
                                      st));
  }
  scatter(p, c);
  k_route_totals<<<1, kRouteMaxWorld, 0, st>>>(c.cnt, c.bytes, c.cbase, c.bbase, p.ntile, world,
                                               counts, nbytes);
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}

// Stable owner partition of m's messages into owner-major send buffers, the
// per-owner totals into counts / nbytes (device).  With a directory (dir) a
// clean batch's hot names are max-combined (k_route_count classifies the
// batch on the way; a dirty one is counted again without combining).
// Src = Datagrams (the wire form): the kernels take the replica fields from
// the datagrams' headers and a, t, e are not read (NULL).
template <class Src>
static int route_pack_src(phip_handle* h, hipStream_t st, const Src& src, const uint64_t* a,
                          const uint64_t* t, const int64_t* e, u32 n, u32 world, const void* dir,
                          uint8_t* send_names, uint32_t* send_lens, uint64_t* send_added,
                          uint64_t* send_taken, int64_t* send_elapsed, uint64_t* counts,
                          uint64_t* nbytes, uint32_t* send_src = nullptr) {
  const HotHdr* hot = (const HotHdr*)dir;
  const RouteHot* rdir = hot ? (const RouteHot*)(hot + 1) : nullptr;
  return route_pack_with(
      h, st, n, world, counts, nbytes,
      [&](const RoutePlan& p, const RouteCells& c) {
        k_batch_reset<<<1, kShards, 0, st>>>(c.pctr, nullptr);
        Launch l(h, "k_route_count", st);
        k_route_count<Src><<<p.nblk, kRouteBlock, 0, st>>>(
            src, a, t, e, n, p.span, world, p.ntile, hot, rdir, c.pctr, c.code,
            c.cnt, c.bytes, hot ? kRouteCombine : kRoutePlain);
        if (hot)
          k_route_count<Src><<<p.nblk, kRouteBlock, 0, st>>>(
              src, a, t, e, n, p.span, world, p.ntile, hot, rdir, c.pctr, c.code,
              c.cnt, c.bytes, kRouteRecount);
      },
      [&](const RoutePlan& p, const RouteCells& c) {
        Launch l(h, send_src ? "k_route_scatter_src" : "k_route_scatter", st);
        if (send_src)   // (the replies forms of the group: the same pack, keeping every message's index)
          k_route_scatter<WithSrcIdx<Src>><<<p.nblk, kRouteBlock, 0, st>>>(
              WithSrcIdx<Src>{src, send_src}, a, t, e, n, p.span, world, p.ntile, hot, rdir, c.pctr,
              c.code, c.cbase, c.bbase, send_names, send_lens, send_added, send_taken, send_elapsed);
        else
          k_route_scatter<Src><<<p.nblk, kRouteBlock, 0, st>>>(
              src, a, t, e, n, p.span, world, p.ntile, hot, rdir, c.pctr, c.code,
              c.cbase, c.bbase, send_names, send_lens, send_added, send_taken, send_elapsed);
      });
}
static int route_pack_on(phip_handle* h, hipStream_t st, const phip_msgs& m, u32 world, const void* dir,
                  uint8_t* send_names, uint32_t* send_lens, uint64_t* send_added,
                  uint64_t* send_taken, int64_t* send_elapsed, uint64_t* counts,
                  uint64_t* nbytes, uint32_t* send_src = nullptr) {
  return route_pack_src(h, st, NamesOffs{m.names, m.name_offs, m.names_len}, m.added, m.taken,
                        m.elapsed, m.n, world, dir, send_names, send_lens, send_added, send_taken,
                        send_elapsed, counts, nbytes, send_src);
}

// Stable owner partition of an op stream (phip_route_pack_ops, and the chunks
// of phip_group_apply_mixed) into owner-major send buffers: route_pack_on's
// skeleton (B_ROUTE, which nothing of ordered() touches); ordered ops never
// combine.  Peek: the query pack of phip_group_peek (k_route_ops_scatter's
// peek form: no kind column is read or written, the operands are the TAKE
// ones); the count pass reads only names and serves both.
template <bool Peek = false>
static int route_pack_ops_on(phip_handle* h, hipStream_t st, const phip_ops& ops, u32 world,
                             uint8_t* send_names, uint32_t* send_lens, uint8_t* send_kind,
                             int64_t* send_now, uint64_t* send_x0, uint64_t* send_x1,
                             uint64_t* send_x2, uint32_t* send_src, uint64_t* counts,
                             uint64_t* nbytes) {
  const u32 n = ops.n;
  NamesOffs src{ops.names, ops.name_offs, ops.names_len};
  const RouteOps ro{ops.kind, ops.now, ops.freq, ops.per, ops.count, ops.added, ops.taken,
                    ops.elapsed};
  return route_pack_with(
      h, st, n, world, counts, nbytes,
      [&](const RoutePlan& p, const RouteCells& c) {
        Launch l(h, "k_route_ops_count", st);
        k_route_ops_count<NamesOffs><<<p.nblk, kRouteBlock, 0, st>>>(src, n, p.span, world, p.ntile,
                                                                      c.code, c.cnt, c.bytes);
      },
      [&](const RoutePlan& p, const RouteCells& c) {
        Launch l(h, Peek ? "k_route_ops_scatter_peek" : "k_route_ops_scatter", st);
        k_route_ops_scatter<NamesOffs, Peek><<<p.nblk, kRouteBlock, 0, st>>>(
            src, ro, n, p.span, world, p.ntile, c.code, c.cbase, c.bbase, send_names, send_lens,
            send_kind, send_now, send_x0, send_x1, send_x2, send_src);
      });
}

// A checked batch's offset column (names_len != 0) in one pass on `st`,
// before anything of the batch is routed: *first_bad is its first malformed
// entry (NamesOffs::bad), ~0 when there is none or the batch is unchecked.
// Synchronises `st`.
static int check_offsets_on(phip_handle* h, hipStream_t st, const uint8_t* names,
                            const uint32_t* name_offs, u32 names_len, u32 n, u32* first_bad) {
  *first_bad = ~0u;
  if (n == 0 || names_len == 0) return PHIP_OK;
  u32* d;
  int rc;
  if ((rc = ensure(h, B_NCHK, 1, &d))) return rc;
  HIPCHK(h, hipMemsetAsync(d, 0xFF, sizeof(u32), st));
  {
    Launch l(h, "k_offs_check", st);
    k_offs_check<<<grid_for(n), kBlock, 0, st>>>(NamesOffs{names, name_offs, names_len}, n, d);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(first_bad, d, sizeof(u32), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return PHIP_OK;
}

// The pre-pass of a routed wire batch on `st`, which it synchronises
// (k_wire_scan): *stop is the first malformed datagram or n, *first_bad the
// first entry whose offsets a checked batch (bytes_len != 0) rejects, ~0 when
// there is none.
static int wire_scan_on(phip_handle* h, hipStream_t st, const uint8_t* bytes, const uint64_t* offs,
                        u64 bytes_len, u32 n, u32* stop, u32* first_bad) {
  *stop = n;
  *first_bad = ~0u;
  if (n == 0) return PHIP_OK;
  u32* d;
  int rc;
  if ((rc = ensure(h, B_NCHK, 2, &d))) return rc;
  HIPCHK(h, hipMemsetAsync(d, 0xFF, 2 * sizeof(u32), st));
  {
    Launch l(h, "k_wire_scan", st);
    k_wire_scan<<<grid_for(n), kBlock, 0, st>>>(bytes, offs, n, bytes_len, d);
  }
  HIPCHK(h, hipGetLastError());
  u32 r[2];
  HIPCHK(h, hipMemcpyAsync(r, d, sizeof r, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  *stop = std::min(r[0], n);
  *first_bad = r[1];
  return PHIP_OK;
}

// ===================================================================== ABI
extern "C" {

int phip_abi_version(void) { return PHIP_ABI_VERSION; }

// phip_build_id: patrol_amd/Makefile links it from build/build_id.o (a hash
// of every source and the flags); single-command builds of the sources
// (tools/build_variants.sh) name theirs with -DPHIP_BUILD_ID.
#ifdef PHIP_BUILD_ID
const char* phip_build_id(void) { return PHIP_BUILD_ID; }
#endif

int phip_open(const phip_config* cfg, phip_handle** out) {
  if (!cfg || !out) return PHIP_ERR_INVALID;
  *out = nullptr;
  if (cfg->log2_slots < 4 || cfg->log2_slots > 31) return PHIP_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PHIP_ERR_NO_DEVICE;
  if (cfg->device < 0 || cfg->device >= ndev) return PHIP_ERR_NO_DEVICE;
  phip_handle* h = new phip_handle;
  h->device = cfg->device;
  h->L = h->L_open = cfg->log2_slots;
  h->cap = 1ull << h->L;
  h->load_pct = cfg->max_load_pct ? std::min<u32>(cfg->max_load_pct, 95) : 90;
  h->max_load = load_limit(h->cap, h->load_pct);
  h->grow = !(cfg->flags & PHIP_CFG_NO_GROW);
  h->iso_always = cfg->flags & PHIP_CFG_ISOLATE;
  h->classify_first = cfg->flags & PHIP_CFG_CLASSIFY_FIRST;
  h->small = !(cfg->flags & PHIP_CFG_NO_SMALL);
  h->track = cfg->flags & PHIP_CFG_TRACK_CHANGES;
  h->usage = cfg->flags & PHIP_CFG_TRACK_USAGE;
  h->arena_cap = h->arena_open = cfg->arena_bytes ? cfg->arena_bytes : (1ull << 20);
  if (cfg->debug_tag_bits && cfg->debug_tag_bits < 64) h->tag_mask = (1ull << cfg->debug_tag_bits) - 1;
  if (cfg->flags & PHIP_CFG_FIXED_SEED) {
    h->seed = cfg->hash_seed;
  } else if (getrandom(&h->seed, sizeof h->seed, 0) != (ssize_t)sizeof h->seed) {
    // no entropy source: a seed from the clock and the handle's address
    h->seed = seeded_mix((u64)std::chrono::steady_clock::now().time_since_epoch().count(),
                         (u64)(uintptr_t)h);
  }
  auto fail = [&](hipError_t e) {
    phip_close(h);
    (void)e;
    return PHIP_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(h->device)) != hipSuccess) return fail(e);
  if ((e = hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, h->device)) !=
      hipSuccess)
    return fail(e);
  if ((e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking)) != hipSuccess)
    return fail(e);
  h->stream = h->own_stream;
  if ((e = hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking)) != hipSuccess) return fail(e);
  if ((e = hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking)) != hipSuccess) return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)) != hipSuccess) return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming)) != hipSuccess) return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_fork3, hipEventDisableTiming)) != hipSuccess) return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_join3, hipEventDisableTiming)) != hipSuccess) return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_gather, hipEventDisableTiming)) != hipSuccess) return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_gather3, hipEventDisableTiming)) != hipSuccess)
    return fail(e);
  if ((e = hipEventCreateWithFlags(&h->ev_pack, hipEventDisableTiming)) != hipSuccess) return fail(e);
  for (hipEvent_t& ev : h->ev_ctr)
    if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&h->recs, h->cap * sizeof(Rec))) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&h->aux, h->cap * sizeof(u32))) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&h->arena, h->arena_cap + 64)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&h->arena_cursor, 64)) != hipSuccess) return fail(e);
  if ((e = hipMalloc(&h->ctr, 3 * kCtrWords * sizeof(u32))) != hipSuccess) return fail(e);
  if ((e = hipHostMalloc(&h->ctr_host, 3 * kCtrWords * sizeof(u32),
                         hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
      (e = hipHostGetDevicePointer((void**)&h->ctr_map, h->ctr_host, 0)) != hipSuccess)
    return fail(e);
  if ((e = hipMemsetAsync(h->recs, 0, h->cap * sizeof(Rec), h->stream)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(h->aux, 0, h->cap * sizeof(u32), h->stream)) != hipSuccess) return fail(e);
  if (h->track && alloc_marks(h, h->cap, &h->marks)) return fail(hipErrorOutOfMemory);
  if (h->usage && alloc_base(h, h->cap, &h->base)) return fail(hipErrorOutOfMemory);
  if ((e = hipMemsetAsync(h->arena_cursor, 0, 64, h->stream)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(h->ctr, 0, 3 * kCtrWords * sizeof(u32), h->stream)) != hipSuccess)
    return fail(e);
  if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
  *out = h;
  return PHIP_OK;
}

void phip_close(phip_handle* h) {
  // Teardown is best effort: every resource is released whatever the
  // earlier calls return.
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->pend.active) (void)after_error(h, finish_pending(h));   // a queued PHIP_RECV_ASYNC batch
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  if (h->stream3) (void)hipStreamSynchronize(h->stream3);
  if (h->stream4) (void)hipStreamSynchronize(h->stream4);
  for (auto& b : h->buf)
    if (b.p) (void)hipFree(b.p);
  for (auto& t : h->event_pool) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  if (h->recs) (void)hipFree(h->recs);
  if (h->aux) (void)hipFree(h->aux);
  if (h->marks.state) (void)hipFree(h->marks.state);
  if (h->base) (void)hipFree(h->base);
  if (h->arena) (void)hipFree(h->arena);
  if (h->arena_cursor) (void)hipFree(h->arena_cursor);
  if (h->ctr) (void)hipFree(h->ctr);
  if (h->ctr_host) (void)hipHostFree(h->ctr_host);
  if (h->small_pin) (void)hipHostFree(h->small_pin);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_fork3) (void)hipEventDestroy(h->ev_fork3);
  if (h->ev_join3) (void)hipEventDestroy(h->ev_join3);
  if (h->ev_gather) (void)hipEventDestroy(h->ev_gather);
  if (h->ev_gather3) (void)hipEventDestroy(h->ev_gather3);
  if (h->ev_pack) (void)hipEventDestroy(h->ev_pack);
  for (hipEvent_t ev : h->ev_ctr)
    if (ev) (void)hipEventDestroy(ev);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->stream3) (void)hipStreamDestroy(h->stream3);
  if (h->stream4) (void)hipStreamDestroy(h->stream4);
  if (h->ev_t4a) (void)hipEventDestroy(h->ev_t4a);
  if (h->ev_t4b) (void)hipEventDestroy(h->ev_t4b);
  if (h->own_stream) {
    (void)hipStreamSynchronize(h->own_stream);
    (void)hipStreamDestroy(h->own_stream);
  }
  delete h;
}

const char* phip_last_error(const phip_handle* h) { return h ? h->err.c_str() : "null handle"; }

int phip_flush(phip_handle* h) {
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

// (a queued PHIP_RECV_ASYNC batch is finished first: its new buckets count)
// (their own result carries no status: a queued batch's error is kept for the
// handle's next call that returns one)
uint64_t phip_len(phip_handle* h) {
  if (!h) return 0;
  std::lock_guard<std::mutex> g(h->mu);
  if (!h->deferred_rc) h->deferred_rc = begin_call(h);
  return h->n_buckets;
}
uint64_t phip_capacity(phip_handle* h) {
  if (!h) return 0;
  std::lock_guard<std::mutex> g(h->mu);
  if (!h->deferred_rc) h->deferred_rc = begin_call(h);
  return h->cap;
}

int phip_seed(phip_handle* h, const uint8_t* names, const uint32_t* name_offs, uint32_t n,
              const phip_state* states, uint32_t flags) {
  if (!h || (n && (!names || !name_offs || !states))) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (n == 0) return PHIP_OK;
  bool dev = flags & PHIP_DEVICE_PTRS;
  if (!dev && !names_ok(name_offs, n)) return set_err(h, PHIP_ERR_NAME_TOO_LARGE, "name > 231 bytes");
  int rc;
  NamesOffs src;
  if ((rc = stage_names(h, names, name_offs, n, dev, &src))) return rc;
  const phip_state* d_st;
  if ((rc = stage(h, B_STATES, states, n, dev, &d_st))) return rc;
  u32* slot;
  u32 n_claimed = 0;
  if ((rc = resolve_all(h, src, n, nullptr, 0, &slot, &n_claimed))) return after_error(h, rc);
  // aux is the per-slot "last writer" scratch: clear, pick the last entry of
  // each name, apply it, clear again.
  k_seed_finish<<<grid_for(n), kBlock, 0, h->stream>>>(slot, n, table(h));
  k_seed_pick<<<grid_for(n), kBlock, 0, h->stream>>>(slot, n, table(h));
  k_seed_apply<<<grid_for(n), kBlock, 0, h->stream>>>(slot, n, d_st, table(h));
  k_seed_finish<<<grid_for(n), kBlock, 0, h->stream>>>(slot, n, table(h));
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_get(phip_handle* h, const uint8_t* name, uint32_t len, phip_state* out) {
  if (!h || (!name && len) || !out) return PHIP_ERR_INVALID;
  if (len > PHIP_MAX_NAME_LEN) return 0;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  u8* d_name;
  Rec* d_rec;
  int rc;
  if ((rc = ensure(h, B_NAME1, 256 + sizeof(Rec) + 16, &d_name))) return rc;
  d_rec = (Rec*)(d_name + 256);
  int* d_found = (int*)(d_name + 256 + sizeof(Rec));
  if (len) HIPCHK(h, hipMemcpyAsync(d_name, name, len, hipMemcpyHostToDevice, h->stream));
  k_get_one<<<1, 64, 0, h->stream>>>(d_name, len, table(h), d_rec, d_found);
  HIPCHK(h, hipGetLastError());
  Rec r;
  int found = 0;
  HIPCHK(h, hipMemcpyAsync(&r, d_rec, sizeof(Rec), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&found, d_found, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!found) return 0;
  out->added = dec_f64(r.added);
  out->taken = dec_f64(r.taken);
  out->elapsed = r.elapsed;
  out->created = r.created;
  return 1;
}

// Snapshot image: header, the 2^L slot records as they lie in HBM, then the
// used part of the long-name arena.  Restoring it into a handle of the same
// table size reproduces the table exactly (slots, probe chains, arena
// offsets), with no rehash.
struct SnapHeader {
  char magic[8];
  u32 abi, log2_slots;
  u64 n_buckets, arena_used, rec_bytes, reserved[3];
};
static_assert(sizeof(SnapHeader) == 64, "snapshot header");
constexpr char kSnapMagic[8] = {'P', 'H', 'I', 'P', 'S', 'N', 'P', '1'};

static u64 arena_used(phip_handle* h) {
  u64 used = 0;
  if (hipMemcpyAsync(&used, h->arena_cursor, sizeof(u64), hipMemcpyDeviceToHost, h->stream) !=
          hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return ~0ull;
  return std::min<u64>(used, h->arena_cap);
}

uint64_t phip_snapshot_bytes(phip_handle* h) {
  if (!h) return 0;
  std::lock_guard<std::mutex> g(h->mu);
  if (begin_call(h)) return 0;
  const u64 used = arena_used(h);
  if (used == ~0ull) return 0;
  return sizeof(SnapHeader) + h->cap * sizeof(Rec) + used;
}

int phip_snapshot(phip_handle* h, uint8_t* out, uint64_t cap) {
  if (!h || !out) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  const u64 used = arena_used(h);
  if (used == ~0ull) return set_err(h, PHIP_ERR_HIP, "snapshot: arena cursor read failed");
  const u64 need = sizeof(SnapHeader) + h->cap * sizeof(Rec) + used;
  if (cap < need) return set_err(h, PHIP_ERR_INVALID, "snapshot needs %llu bytes", (unsigned long long)need);
  SnapHeader hd{};
  std::memcpy(hd.magic, kSnapMagic, 8);
  hd.abi = PHIP_ABI_VERSION;
  hd.log2_slots = h->L;
  hd.n_buckets = h->n_buckets;
  hd.arena_used = used;
  hd.rec_bytes = sizeof(Rec);
  hd.reserved[0] = h->seed;   // the records lie where this seed placed them
  std::memcpy(out, &hd, sizeof hd);
  u8* p = out + sizeof hd;
  HIPCHK(h, hipMemcpyAsync(p, h->recs, h->cap * sizeof(Rec), hipMemcpyDeviceToHost, h->stream));
  if (used) HIPCHK(h, hipMemcpyAsync(p + h->cap * sizeof(Rec), h->arena, used, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_restore(phip_handle* h, const uint8_t* in, uint64_t len) {
  if (!h || !in || len < sizeof(SnapHeader)) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  SnapHeader hd;
  std::memcpy(&hd, in, sizeof hd);
  if (std::memcmp(hd.magic, kSnapMagic, 8) || hd.abi != PHIP_ABI_VERSION || hd.rec_bytes != sizeof(Rec))
    return set_err(h, PHIP_ERR_INVALID, "not a snapshot of this ABI");
  if (hd.log2_slots < 4 || hd.log2_slots > 31)
    return set_err(h, PHIP_ERR_INVALID, "snapshot of 2^%u slots", hd.log2_slots);
  const u64 scap = 1ull << hd.log2_slots;
  if (len != sizeof hd + scap * sizeof(Rec) + hd.arena_used)
    return set_err(h, PHIP_ERR_INVALID, "snapshot truncated");
  if (hd.n_buckets > load_limit(scap, h->load_pct))
    return set_err(h, PHIP_ERR_FULL, "snapshot above the handle's load limit");
  if (hd.arena_used > h->arena_cap) {
    if (!h->grow) return set_err(h, PHIP_ERR_ARENA, "snapshot arena larger than the handle's");
    if (int rc = grow_arena(h, 0, hd.arena_used)) return rc;
  }
  if (hd.log2_slots != h->L) {
    // The image's table size wins (the table may have grown since it was
    // opened): the handle's table is replaced by one of that size.
    Rec* nrecs = nullptr;
    u32* naux = nullptr;
    Marks nmarks{};
    u64* nbase = nullptr;
    if (hipMalloc(&nrecs, scap * sizeof(Rec)) != hipSuccess ||
        hipMalloc(&naux, scap * sizeof(u32)) != hipSuccess ||
        (h->track && alloc_marks(h, scap, &nmarks)) ||
        (h->usage && alloc_base(h, scap, &nbase))) {
      (void)hipGetLastError();
      if (nrecs) (void)hipFree(nrecs);
      if (naux) (void)hipFree(naux);
      if (nmarks.state) (void)hipFree(nmarks.state);
      return set_err(h, PHIP_ERR_FULL, "restore: no device memory for 2^%u slots", hd.log2_slots);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipFree(h->recs));
    HIPCHK(h, hipFree(h->aux));
    if (h->marks.state) HIPCHK(h, hipFree(h->marks.state));
    if (h->base) HIPCHK(h, hipFree(h->base));
    h->recs = nrecs;
    h->aux = naux;
    h->marks = nmarks;
    h->base = nbase;
    h->L = hd.log2_slots;
    h->cap = scap;
    h->max_load = load_limit(scap, h->load_pct);
  }
  ++h->layout_gen;   // (replaced above or reloaded below: the slots' contents change either way)
  const u8* p = in + sizeof hd;
  HIPCHK(h, hipMemcpyAsync(h->recs, p, h->cap * sizeof(Rec), hipMemcpyHostToDevice, h->stream));
  if (hd.arena_used)
    HIPCHK(h, hipMemcpyAsync(h->arena, p + h->cap * sizeof(Rec), hd.arena_used, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(h->aux, 0, h->cap * sizeof(u32), h->stream));
  // (a snapshot holds no change set: the image's buckets start unmarked)
  if (h->marks.state)
    HIPCHK(h, hipMemsetAsync(h->marks.state, 0, 2 * mark_words(h->cap) * sizeof(u32), h->stream));
  // (nor a usage baseline: the image's buckets count from zero)
  if (h->base) HIPCHK(h, hipMemsetAsync(h->base, 0, h->cap * sizeof(u64), h->stream));
  HIPCHK(h, hipMemcpyAsync(h->arena_cursor, &hd.arena_used, sizeof(u64), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->n_buckets = hd.n_buckets;
  h->seed = hd.reserved[0];   // the image's placement
  return PHIP_OK;
}

int phip_export_datagrams(phip_handle* h, const uint8_t* names, const uint32_t* name_offs,
                          uint32_t n, uint8_t* out, uint8_t* found, uint32_t flags) {
  if (!h || (n && (!names || !name_offs || !out || !found))) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (n == 0) return PHIP_OK;
  const bool dev = flags & PHIP_DEVICE_PTRS;
  if (!dev && !names_ok(name_offs, n)) return set_err(h, PHIP_ERR_NAME_TOO_LARGE, "name > 231 bytes");
  int rc;
  NamesOffs src;
  if ((rc = stage_names(h, names, name_offs, n, dev, &src))) return rc;
  const size_t nbytes = dev ? 0 : (size_t)PHIP_BUCKET_FIXED_SIZE * n + (name_offs[n] - name_offs[0]);
  u8 *d_out, *d_found;
  if ((rc = out_buf(h, B_EXPORT, out, nbytes, dev, &d_out)) ||
      (rc = out_buf(h, B_STATUS, found, n, dev, &d_found)))
    return rc;
  {
    Launch l(h, "k_export");
    k_export<<<grid_for(n), kBlock, 0, h->stream>>>(src, n, table(h), d_out, d_found);
  }
  HIPCHK(h, hipGetLastError());
  if ((rc = copy_back(h, out, d_out, nbytes, dev)) || (rc = copy_back(h, found, d_found, n, dev)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

// Peek (patrolhip.h "Peek"): one launch of k_peek over the queries, staged as
// phip_export_datagrams stages its names.  Nothing of the handle changes: no
// reserve, no insert, no counter word, no mark.
int phip_peek(phip_handle* h, const phip_ops* q, const phip_peek_results* res, uint32_t flags) {
  if (!h || !q) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (flags & ~PHIP_DEVICE_PTRS)
    return set_err(h, PHIP_ERR_INVALID, "peek: unknown flag bits 0x%x", flags);
  const u32 n = q->n;
  if (n == 0) return PHIP_OK;
  if (!q->names || !q->name_offs)
    return set_err(h, PHIP_ERR_INVALID, "peek: names and name_offs are required");
  const bool dev = flags & PHIP_DEVICE_PTRS;
  if (!dev && !names_ok(q->name_offs, n)) return set_err(h, PHIP_ERR_NAME_TOO_LARGE, "name > 231 bytes");
  int rc;
  NamesOffs src;
  if ((rc = stage_names(h, q->names, q->name_offs, n, dev, &src, q->names_len))) return rc;
  // a checked device batch: the offset column first, so that no name is read
  // and no result written for a batch with a malformed entry
  u32 first_bad;
  if ((rc = check_offsets_on(h, h->stream, src.blob, src.offs, src.lim, n, &first_bad))) return rc;
  if (first_bad != ~0u)
    return set_err(h, PHIP_ERR_INVALID, "peek: malformed name offsets at query %u (names_len check)",
                   first_bad);
  OpView ov{};
  phip_peek_results r{};
  if (res) r = *res;
  PeekOut po{};
  if ((rc = stage(h, B_NOW, q->now, n, dev, &ov.now)) ||
      (rc = stage(h, B_FREQ, q->freq, n, dev, &ov.freq)) ||
      (rc = stage(h, B_PER, q->per, n, dev, &ov.per)) ||
      (rc = stage(h, B_COUNT, q->count, n, dev, &ov.count)) ||
      (rc = out_buf(h, B_STATUS, r.status, n, dev, &po.status)) ||
      (rc = out_buf(h, B_REM, r.remaining, n, dev, &po.remaining)) ||
      (rc = out_buf(h, B_HAVE, r.have, n, dev, &po.have)) ||
      (rc = out_buf(h, B_PEEKAT, r.retry_at, n, dev, &po.retry_at)) ||
      (rc = out_buf(h, B_PEEKST, r.state, n, dev, &po.state)))
    return rc;
  {
    Launch l(h, "k_peek");
    k_peek<<<grid_for(n), kBlock, 0, h->stream>>>(src, ov, n, table(h), po);
  }
  HIPCHK(h, hipGetLastError());
  if ((rc = copy_back(h, r.status, po.status, n, dev)) ||
      (rc = copy_back(h, r.remaining, po.remaining, n, dev)) ||
      (rc = copy_back(h, r.have, po.have, n, dev)) ||
      (rc = copy_back(h, r.retry_at, po.retry_at, n, dev)) ||
      (rc = copy_back(h, r.state, po.state, n, dev)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_dump(phip_handle* h, uint8_t* names, uint64_t names_cap, uint64_t* name_offs,
              phip_state* states, uint64_t max_n, uint64_t* n_out, uint64_t* names_bytes_out) {
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  int rc;
  u32* list;
  // count the occupied slots first, then size the list by that count
  if ((rc = reset_ctr(h))) return rc;
  k_dump_collect<<<grid_for(h->cap), kBlock, 0, h->stream>>>(h->recs, h->cap, nullptr, h->ctr);
  HIPCHK(h, hipGetLastError());
  if ((rc = read_ctr(h))) return rc;
  const u32 occupied = h->ctr_host[kCtrOccupied];
  if ((rc = ensure(h, B_DUMP, (size_t)occupied + 1, &list))) return rc;
  if ((rc = reset_ctr(h))) return rc;
  k_dump_collect<<<grid_for(h->cap), kBlock, 0, h->stream>>>(h->recs, h->cap, list, h->ctr);
  HIPCHK(h, hipGetLastError());
  if ((rc = read_ctr(h))) return rc;
  u32 n = h->ctr_host[kCtrOccupied];
  if (n != occupied) return set_err(h, PHIP_ERR_INVALID, "internal: table changed during dump");
  Rec* d_out;
  if ((rc = ensure(h, B_TEMP, (size_t)n * sizeof(Rec), (u8**)&d_out))) return rc;
  k_dump_gather<<<grid_for(n), kBlock, 0, h->stream>>>(list, n, h->recs, d_out);
  HIPCHK(h, hipGetLastError());
  std::vector<Rec> recs(n);
  if (n) HIPCHK(h, hipMemcpyAsync(recs.data(), d_out, n * sizeof(Rec), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // Long names come from the arena.
  std::vector<u8> arena;
  u64 cursor = 0;
  HIPCHK(h, hipMemcpy(&cursor, h->arena_cursor, 8, hipMemcpyDeviceToHost));
  cursor = std::min(cursor, h->arena_cap);
  if (cursor) {
    arena.resize(cursor);
    HIPCHK(h, hipMemcpy(arena.data(), h->arena, cursor, hipMemcpyDeviceToHost));
  }
  u64 total = 0;
  for (auto& r : recs) total += r.name0 & 0xFF;   // byte 0 = length
  if (n_out) *n_out = n;
  if (names_bytes_out) *names_bytes_out = total;
  if (!names) return PHIP_OK;
  if (total > names_cap || n > max_n || !name_offs || !states)
    return set_err(h, PHIP_ERR_INVALID, "dump buffers too small");
  u64 o = 0;
  for (u32 k = 0; k < n; ++k) {
    const Rec& r = recs[k];
    u32 len = r.name0 & 0xFF;
    name_offs[k] = o;
    if (len <= kInlineName) {
      const u64 w[3] = {r.name0, r.name1, r.name2};
      for (u32 j = 0; j < len; ++j) names[o + j] = (u8)(w[(j + 2) >> 3] >> (((j + 2) & 7) * 8));
    } else {
      u64 aoff = r.name0 >> 32;
      if (aoff + len <= arena.size()) std::memcpy(names + o, arena.data() + aoff, len);
    }
    o += len;
    states[k].added = dec_f64(r.added);
    states[k].taken = dec_f64(r.taken);
    states[k].elapsed = r.elapsed;
    states[k].created = r.created;
  }
  name_offs[n] = o;
  return PHIP_OK;
}

// The incast-reply form of a receive call: its out fields read zero unless the
// call gets as far as its replies (reply_zero, first thing in each entry
// point), and reply_enter refuses its arguments before anything is applied.
static void reply_zero(phip_reply_egress* rq) {
  rq->n = rq->replies = rq->skipped = 0;
  rq->bytes = 0;
}
static int reply_enter(phip_handle* h, phip_reply_egress* rq, uint32_t flags, ReplyEg* eg) {
  if (flags & PHIP_RECV_ASYNC)
    return set_err(h, PHIP_ERR_INVALID, "replies: PHIP_RECV_ASYNC batches return none");
  eg->rq = rq;
  eg->dev = flags & PHIP_DEVICE_PTRS;
  return datagram_args(h, "replies", rq->out, rq->out_cap, rq->offs, rq->max_msgs, eg->dev,
                       &eg->budget);
}

// phip_receive_soa, and with rq phip_receive_soa_replies (never queued).
static int receive_soa(phip_handle* h, const phip_msgs* m, int64_t now, const phip_results* res,
                       uint32_t flags, phip_reply_egress* rq) {
  if (!h || !m) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  bool dev = flags & PHIP_DEVICE_PTRS;
  u32 n = m->n;
  const PassAsk ask = (flags & PHIP_RECV_CLASSIFY) ? PassAsk::kPolicy : PassAsk::kMayUndo;
  ReplyEg egs{}, *eg = rq ? &egs : nullptr;
  if (rq)
    if (int rc0 = reply_enter(h, rq, flags, eg)) return rc0;
  if ((flags & PHIP_RECV_ASYNC) && dev && n >= kHotMinBatch && m->names && m->name_offs &&
      m->added && m->taken && m->elapsed) {
    // Queue this batch's front (reset, directory with the status fill, or
    // classification and directory) behind the batch queued before, read that batch's
    // counters meanwhile and finish it, then queue this batch's fast pass
    // and return.  The front's counters are a fast-pass set of their own
    // (fctr), so the previous batch's leftover work leaves it standing
    // unless that work ran a fast pass itself or grew the table (below).
    if (int rc0 = begin_call(h, false)) return rc0;
    NamesOffs src{m->names, m->name_offs, m->names_len};
    SoaIn<NamesOffs> in{src, m->added, m->taken, m->elapsed};
    OutView ow{};
    FastPass pass;
    int rc;
    bool worked = false;
    if ((rc = receive_outputs(h, res, n, true, &ow))) return rc;
    const bool prev = h->pend.active;
    const phip_handle::HotKeep keep0 = h->keep;
    if ((rc = fast_begin(h, in, src, n, ow.status, ask, !prev, &pass)))
      return after_error(h, rc);
    // An optimistic pass behind a batch not settled yet goes on the stream
    // whole, front and back, before the host waits for that batch: its kernel
    // is gated on that batch's counters (k_receive_fast's `gate`), so the GPU
    // goes from one fast kernel to the next while the host settles.  Shut --
    // the host reads the same words in that batch's mirror -- the kernel
    // wrote nothing; the batch is finished as ever and this pass queued again
    // from its front (the directory state as before the gated front, the count
    // tables as that front's k_hot_dir left them).
    // (only where the back allocates nothing: that batch's log and miss shards
    // are still to be read)
    if (prev && pass.kind == PassKind::kOptimistic && back_fits(h, n)) {
      pass.gate = fctr(h, h->pend.pass.par);
      if ((rc = fast_back(h, in, pass, true))) return after_error(h, rc);
      bool shut = false;
      const u64 nfast = h->nfast;
      if ((rc = finish_pending(h, &worked, &shut))) return after_error(h, rc);
      if (shut) {
        if (h->nfast == nfast) {
          // (no pass of that batch's built since: the slot, its age and
          // generation go back; what collecting that batch learned stays)
          phip_handle::HotKeep k = keep0;
          k.agree = h->keep.agree;
          k.maxlen = h->keep.maxlen;
          k.ref_hits = h->keep.ref_hits;
          k.ref_n = h->keep.ref_n;
          k.sagged = h->keep.sagged;
          h->keep = k;
        }
        if ((rc = fast_begin(h, in, src, n, ow.status, ask, true, &pass)))
          return after_error(h, rc);
        pass.gate_shut = true;
        if ((rc = fast_back(h, in, pass, true))) return after_error(h, rc);
      } else if (worked) {
        return after_error(h, set_err(h, PHIP_ERR_INVALID, "internal: work left behind an open gate"));
      }
      h->pend = {true, in, now, ow, pass};
      return PHIP_OK;
    }
    const u64 nfast = h->nfast, grows = h->grows;
    if (prev && (rc = finish_pending(h, &worked))) return after_error(h, rc);
    // The leftover work of the batch before (its misses, its dirty buckets)
    // runs on the general counters and leaves this front standing, unless it
    // ran a fast pass of its own (the directory and dirty list buffers) or
    // grew the table (the directory's slots).
    // (a failed optimistic pass ran the batch again, a fast pass of its own:
    // the front queued again follows the policy as that batch left it)
    if (worked && (h->nfast != nfast || h->grows != grows) &&
        (rc = fast_begin(h, in, src, n, ow.status, ask, true, &pass)))
      return after_error(h, rc);
    if ((rc = fast_back(h, in, pass, true))) return after_error(h, rc);
    h->pend = {true, in, now, ow, pass};
    return PHIP_OK;
  }
  if (int rc0 = begin_call(h)) return rc0;
  if (n == 0) return eg ? reply_collect(h, eg, true) : PHIP_OK;
  if (!m->names || !m->name_offs || !m->added || !m->taken || !m->elapsed) return PHIP_ERR_INVALID;
  if (!dev && !names_ok(m->name_offs, n)) return set_err(h, PHIP_ERR_NAME_TOO_LARGE, "name > 231 bytes");
  int rc;
  if (!dev) {
    bool done = false;
    if ((rc = rq ? small_uniform_replies(h, m, now, res, rq, &done)
                 : small_uniform(h, m, PHIP_OP_RECEIVE, now, res, &done)))
      return after_error(h, rc);
    if (done) return PHIP_OK;
  }
  NamesOffs src;
  const uint64_t *a, *t;
  const int64_t* e;
  OutView ow{};
  if ((rc = stage_names(h, m->names, m->name_offs, n, dev, &src, m->names_len)) ||
      (rc = stage(h, B_A, m->added, n, dev, &a)) || (rc = stage(h, B_T, m->taken, n, dev, &t)) ||
      (rc = stage(h, B_E, m->elapsed, n, dev, &e)) || (rc = receive_outputs(h, res, n, dev, &ow)))
    return rc;
  if ((rc = receive_decoded(h, src, a, t, e, n, now, ow, ask, eg))) return after_error(h, rc);
  return copy_outputs(h, res, n, dev, ow);
}

int phip_receive_soa(phip_handle* h, const phip_msgs* m, int64_t now, const phip_results* res,
                     uint32_t flags) {
  return receive_soa(h, m, now, res, flags, nullptr);
}

int phip_receive_soa_replies(phip_handle* h, const phip_msgs* m, int64_t now,
                             const phip_results* res, phip_reply_egress* rq, uint32_t flags) {
  if (!rq) return PHIP_ERR_INVALID;
  reply_zero(rq);
  return receive_soa(h, m, now, res, flags, rq);
}

}  // extern "C"

namespace {
// ReplicatedRepo.Receive over datagrams already in device memory (the
// caller's, the staging buffers, or a ring slot's copy); results go to
// device (dev) or host buffers.  Called with the handle's mutex held.
int receive_datagrams_dev(phip_handle* h, const u8* d_bytes, const uint64_t* d_offs, u32 n,
                          int64_t now, const phip_results* res, uint32_t* stop_index, bool dev,
                          ReplyEg* eg = nullptr) {
  int rc;
  OutView ow{};
  if ((rc = receive_outputs(h, res, n, dev, &ow))) return rc;
  // Fast path straight from the wire bytes: k_classify reads the headers
  // (and finds the first malformed datagram), k_receive_fast reads every
  // datagram in place; no decoded copy is written.
  // Only a clean prefix with new buckets, or an incast / -0.0 past the dirty
  // set's reach, has the datagrams decoded to the SoA form, for the paths
  // that need it; a batch's dirty buckets (at most kDirtyCap dirty messages)
  // go through the ordered path as a sub-batch dirty_finish
  // reads from the wire.
  FastOutcome o;
  if ((rc = fast_apply(h, WireIn{d_bytes, d_offs}, Datagrams{d_bytes, d_offs}, n, ow.status,
                       PassAsk::kPolicy, &o)))
    return after_error(h, rc);
  const u32 stop = o.stop;   // (the first short datagram)
  if ((rc = fill_stopped(h, ow.status, n, stop))) return rc;
  if (o.first_dirty < stop || o.nmiss || o.ndef) {
    uint64_t *a, *t, *no;
    int64_t* e;
    u8* nl;
    if ((rc = ensure(h, B_DA, n, &a)) || (rc = ensure(h, B_DT, n, &t)) ||
        (rc = ensure(h, B_DE, n, &e)) || (rc = ensure(h, B_NOFF, n, &no)) ||
        (rc = ensure(h, B_NLEN, n, &nl)))
      return rc;
    if (o.first_dirty < stop || o.nmiss) {   // (a batch whose dirty buckets alone are left reads no decode)
      Launch l(h, "k_decode");
      k_decode<<<grid_for(stop), kBlock, 0, h->stream>>>(d_bytes, d_offs, stop, a, t, e, no, nl,
                                                          h->ctr);
      HIPCHK(h, hipGetLastError());
    }
    if ((rc = finish_receive(h, NamesPairs{d_bytes, no, nl}, a, t, e, now, ow, o, eg)))
      return after_error(h, rc);
  }
  if ((rc = copy_outputs(h, res, n, dev, ow))) return rc;
  // (the replies of the messages before a short datagram were sent: collected
  // before the stop is reported)
  if (eg && (rc = reply_collect(h, eg))) return after_error(h, rc);
  if (dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (stop_index) *stop_index = stop;
  if (stop < n) return set_err(h, PHIP_ERR_SHORT_BUFFER, "short buffer at datagram %u", stop);
  return PHIP_OK;
}

// ---- packed frames (patrolhip.h "Packed frames"; kernels in phip_kernels.hpp
// "packed frames") ----
// The call's device buffer: the counters, the tile arrays of the scan, and
// (unframe) a record count per frame.
struct FrameBuf {
  u64* ctr;
  u64* tile_bytes;
  u32* tile_cnt;
  u32* fcnt;
  FrameBuf(u64* p, u32 ntiles)
      : ctr(p), tile_bytes(p + kFrWords), tile_cnt(reinterpret_cast<u32*>(p + kFrWords + ntiles)),
        fcnt(reinterpret_cast<u32*>(p + kFrWords + ntiles + ((size_t)ntiles + 1) / 2)) {}
  static size_t words(u32 ntiles, u32 per_entry) {
    return kFrWords + (size_t)ntiles + ((size_t)ntiles + 1) / 2 + ((size_t)per_entry + 1) / 2;
  }
};

bool frame_bytes_ok(uint32_t fb) { return fb >= PHIP_FRAME_MIN_BYTES && fb <= PHIP_FRAME_MAX_BYTES; }

// The counters behind a frames call's write pass, read back: the one
// synchronise of a device-pointer call.  *total: the records or frames the
// call needs (saturated), also when they do not fit `cap`.
int frame_close(phip_handle* h, const u64* ctr, const char* what, const char* unit, u32 cap,
                u32* total) {
  u64 c[kFrWords];
  HIPCHK(h, hipMemcpyAsync(c, ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (c[kFrBad] != ~0ull)
    return set_err(h, PHIP_ERR_INVALID, "%s: entry %llu is malformed or longer than frame_bytes", what,
                   (unsigned long long)c[kFrBad]);
  *total = (u32)std::min<u64>(c[kFrN], ~0u);
  if (c[kFrN] > cap)
    return set_err(h, PHIP_ERR_INVALID, "%s: %llu %s, room for %u", what, (unsigned long long)c[kFrN],
                   unit, cap);
  return PHIP_OK;
}

// phip_unframe over device memory, queued on the handle's stream: check,
// count, scan, write, then the counters' read-back.
int unframe_dev(phip_handle* h, const u8* d_bytes, const uint64_t* d_foffs, u32 n, u64 lim, u32 fb,
                uint64_t* d_rec_offs, u32* d_rec_frame, u32 max_recs, u32* n_recs) {
  *n_recs = 0;
  if (n == 0) {
    HIPCHK(h, hipMemcpyAsync(d_rec_offs, d_foffs, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PHIP_OK;
  }
  int rc;
  u64* p;
  const u32 ntiles = grid_for(n);
  if ((rc = ensure(h, B_FRAME, FrameBuf::words(ntiles, n), &p))) return rc;
  const FrameBuf b(p, ntiles);
  HIPCHK(h, hipMemsetAsync(b.ctr, 0xFF, kFrWords * sizeof(u64), h->stream));
  {
    Launch l(h, "k_frame_check");
    k_frame_check<<<ntiles, kBlock, 0, h->stream>>>(d_foffs, n, lim, fb, b.ctr);
  }
  {
    Launch l(h, "k_frame_count");
    k_frame_count<<<ntiles, kBlock, 0, h->stream>>>(d_bytes, d_foffs, n, b.ctr, b.fcnt, b.tile_cnt,
                                                    b.tile_bytes);
  }
  {
    Launch l(h, "k_frame_scan");
    k_frame_scan<<<1, kSweepBlock, 0, h->stream>>>(b.tile_cnt, b.tile_bytes, ntiles, b.ctr);
  }
  {
    Launch l(h, "k_frame_write");
    k_frame_write<<<ntiles, kBlock, 0, h->stream>>>(d_bytes, d_foffs, n, b.ctr, b.fcnt, b.tile_cnt,
                                                    max_recs, d_rec_offs, d_rec_frame);
  }
  HIPCHK(h, hipGetLastError());
  return frame_close(h, b.ctr, "unframe", "records", max_recs, n_recs);
}

// phip_frame_cuts over device memory, likewise.
int frame_cuts_dev(phip_handle* h, const uint64_t* d_offs, u32 n, u32 fb, uint64_t* d_frame_offs,
                   u32* d_frame_first, u32 max_frames, u32* n_frames) {
  *n_frames = 0;
  if (n == 0) {
    HIPCHK(h, hipMemcpyAsync(d_frame_offs, d_offs, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PHIP_OK;
  }
  int rc;
  u64* p;
  const u32 ntiles = (u32)(((u64)n + PHIP_FRAME_TILE - 1) / PHIP_FRAME_TILE);
  const unsigned grid = (ntiles + kCutWaves - 1) / kCutWaves;
  if ((rc = ensure(h, B_FRAME, FrameBuf::words(ntiles, 0), &p))) return rc;
  const FrameBuf b(p, ntiles);
  HIPCHK(h, hipMemsetAsync(b.ctr, 0xFF, kFrWords * sizeof(u64), h->stream));
  {
    Launch l(h, "k_frame_cut_count");
    k_frame_cut_count<<<grid, kBlock, 0, h->stream>>>(d_offs, n, fb, b.ctr, b.tile_cnt,
                                                      b.tile_bytes, ntiles);
  }
  {
    Launch l(h, "k_frame_scan");
    k_frame_scan<<<1, kSweepBlock, 0, h->stream>>>(b.tile_cnt, b.tile_bytes, ntiles, b.ctr);
  }
  {
    Launch l(h, "k_frame_cut_write");
    k_frame_cut_write<<<grid, kBlock, 0, h->stream>>>(d_offs, n, fb, b.ctr, b.tile_cnt, ntiles,
                                                      max_frames, d_frame_offs, d_frame_first);
  }
  HIPCHK(h, hipGetLastError());
  return frame_close(h, b.ctr, "frame cuts", "frames", max_frames, n_frames);
}

// The host walk of phip_unframe: every entry checked from the offsets before
// any byte is read, then frame_walk per frame; emit(k, frame, p) for record k.
// Touches no device and no handle.  *total: the records the frames hold.
template <class Emit>
int unframe_host(const uint8_t* bytes, const uint64_t* foffs, u32 n, u64 lim, u32 fb, Emit emit,
                 u64* total) {
  *total = 0;
  for (u32 f = 0; f < n; ++f)
    if (!frame_entry_ok(foffs[f], foffs[f + 1], lim, fb)) return PHIP_ERR_INVALID;
  u64 k = 0;
  for (u32 f = 0; f < n; ++f) {
    const u32 c = frame_walk(bytes, foffs[f], foffs[f + 1], [&](u32 j, u64 p) { emit(k + j, f, p); });
    k += c;
  }
  *total = k;
  return PHIP_OK;
}

// What the frames forms of a receive call add to it.
struct FrameAsk {
  u32 frame_bytes;
  u32* rec_frame;   // the caller's column (optional)
  u32 max_recs;
  u32* n_recs_out;
};

// Unframe over a device batch into the handle's record columns, then the
// datagram path over the records, all on the handle's stream (lock held,
// begin_call done).  dev: the caller's pointers are device memory (else host:
// a ring slot's device copy, rec_frame copied back).
int frames_receive_dev(phip_handle* h, const u8* d_bytes, const uint64_t* d_foffs, u32 n_frames,
                       u64 lim, const FrameAsk& fr, int64_t now, const phip_results* res,
                       uint32_t* stop_index, bool dev, ReplyEg* eg) {
  int rc;
  uint64_t* d_ro;
  u32* d_rf = nullptr;
  if ((rc = ensure(h, B_FRRECS, (size_t)fr.max_recs + 1, &d_ro))) return rc;
  if (fr.rec_frame && dev) d_rf = fr.rec_frame;
  else if (fr.rec_frame && (rc = ensure(h, B_FRMAP, (size_t)fr.max_recs, &d_rf))) return rc;
  u32 nrec = 0;
  rc = unframe_dev(h, d_bytes, d_foffs, n_frames, lim, fr.frame_bytes, d_ro, d_rf, fr.max_recs, &nrec);
  *fr.n_recs_out = nrec;
  if (rc) return rc;
  if (fr.rec_frame && !dev && nrec) {
    HIPCHK(h, hipMemcpyAsync(fr.rec_frame, d_rf, (size_t)nrec * sizeof(u32), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (stop_index) *stop_index = nrec;
  if (nrec == 0) return eg ? reply_collect(h, eg, true) : PHIP_OK;
  return receive_datagrams_dev(h, d_bytes, d_ro, nrec, now, res, stop_index, dev, eg);
}
}  // namespace

extern "C" {

static int receive_datagrams_begun(phip_handle* h, const uint8_t* bytes, const uint64_t* offs,
                                   uint32_t n, int64_t now, const phip_results* res,
                                   uint32_t* stop_index, uint32_t flags, ReplyEg* eg);

// phip_receive_datagrams, and with rq phip_receive_datagrams_replies.
static int receive_datagrams(phip_handle* h, const uint8_t* bytes, const uint64_t* offs, uint32_t n,
                             int64_t now, const phip_results* res, uint32_t* stop_index,
                             uint32_t flags, phip_reply_egress* rq) {
  if (!h || (n && (!bytes || !offs))) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  ReplyEg egs{}, *eg = rq ? &egs : nullptr;
  if (rq)
    if (int rc0 = reply_enter(h, rq, flags, eg)) return rc0;
  if (int rc0 = begin_call(h)) return rc0;
  return receive_datagrams_begun(h, bytes, offs, n, now, res, stop_index, flags, eg);
}

// The datagram call behind its entry (lock held, reply_enter and begin_call
// done): phip_receive_frames' device form comes in here behind its unframe.
static int receive_datagrams_begun(phip_handle* h, const uint8_t* bytes, const uint64_t* offs,
                                   uint32_t n, int64_t now, const phip_results* res,
                                   uint32_t* stop_index, uint32_t flags, ReplyEg* eg) {
  phip_reply_egress* rq = eg ? eg->rq : nullptr;
  if (stop_index) *stop_index = n;
  if (n == 0) return eg ? reply_collect(h, eg, true) : PHIP_OK;
  bool dev = flags & PHIP_DEVICE_PTRS;
  int rc;
  const uint64_t* d_offs;
  const u8* d_bytes;
  if (!dev && !datagrams_ok(offs, n))
    return set_err(h, PHIP_ERR_INVALID, "datagram offsets decrease");
  if (!dev) {
    bool done = false;
    rc = small_datagrams(h, bytes, offs, n, now, res, stop_index, &done, rq);
    if (done || (rc && rc != PHIP_ERR_SHORT_BUFFER)) return rc == PHIP_ERR_SHORT_BUFFER ? rc : after_error(h, rc);
  }
  if ((rc = stage(h, B_DOFFS, offs, (size_t)n + 1, dev, &d_offs))) return rc;
  size_t nb = dev ? 0 : offs[n];
  if ((rc = stage(h, B_BYTES, bytes, nb, dev, &d_bytes))) return rc;
  return receive_datagrams_dev(h, d_bytes, d_offs, n, now, res, stop_index, dev, eg);
}

int phip_receive_datagrams(phip_handle* h, const uint8_t* bytes, const uint64_t* offs, uint32_t n,
                           int64_t now, const phip_results* res, uint32_t* stop_index,
                           uint32_t flags) {
  return receive_datagrams(h, bytes, offs, n, now, res, stop_index, flags, nullptr);
}

int phip_receive_datagrams_replies(phip_handle* h, const uint8_t* bytes, const uint64_t* offs,
                                   uint32_t n, int64_t now, const phip_results* res,
                                   uint32_t* stop_index, phip_reply_egress* rq, uint32_t flags) {
  if (!rq) return PHIP_ERR_INVALID;
  reply_zero(rq);
  return receive_datagrams(h, bytes, offs, n, now, res, stop_index, flags, rq);
}

// ------------------------------------------------------------ ingest ring --
// Pinned host slots, each with its own device copy; the copies run on the
// ring's stream, so filling and copying slot k+1 overlaps merging slot k.
struct phip_ring {
  phip_handle* h = nullptr;
  hipStream_t copy = nullptr;
  std::mutex mu;
  u32 max_msgs = 0;
  u64 max_bytes = 0;
  enum State { kFree, kAcquired, kSubmitted };
  struct Slot {
    u8* hbytes = nullptr;
    uint64_t* hoffs = nullptr;
    u8* dbytes = nullptr;
    uint64_t* doffs = nullptr;
    hipEvent_t copied = nullptr;
    u32 n = 0;
    State state = kFree;
  };
  std::vector<Slot> slots;
  u32 next_acquire = 0, next_receive = 0;
  std::string err;
};

void phip_ring_close(phip_ring* r) {
  if (!r) return;
  (void)hipSetDevice(r->h->device);
  if (r->copy) (void)hipStreamSynchronize(r->copy);
  for (auto& s : r->slots) {
    if (s.hbytes) (void)hipHostFree(s.hbytes);
    if (s.hoffs) (void)hipHostFree(s.hoffs);
    if (s.dbytes) (void)hipFree(s.dbytes);
    if (s.doffs) (void)hipFree(s.doffs);
    if (s.copied) (void)hipEventDestroy(s.copied);
  }
  if (r->copy) (void)hipStreamDestroy(r->copy);
  delete r;
}

int phip_ring_open(phip_handle* h, uint32_t nslots, uint32_t max_msgs, uint64_t max_bytes,
                   phip_ring** out) {
  if (!out) return PHIP_ERR_INVALID;
  *out = nullptr;
  if (!h || nslots < 1 || nslots > 64 || max_msgs < 1 || max_bytes < 1) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  phip_ring* r = new phip_ring;
  r->h = h;
  r->max_msgs = max_msgs;
  r->max_bytes = max_bytes;
  r->slots.resize(nslots);
  auto fail = [&](hipError_t e, const char* what) {
    set_err(h, PHIP_ERR_HIP, "phip_ring_open: %s failed: %s", what, hipGetErrorString(e));
    phip_ring_close(r);
    return PHIP_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking)) != hipSuccess)
    return fail(e, "hipStreamCreate");
  // +64: the fast path's 8-byte over-read slack past the last datagram.
  const size_t nbytes = max_bytes + 64, noffs = ((size_t)max_msgs + 1) * sizeof(uint64_t);
  for (auto& s : r->slots) {
    if ((e = hipHostMalloc(&s.hbytes, nbytes, 0)) != hipSuccess) return fail(e, "hipHostMalloc");
    if ((e = hipHostMalloc(&s.hoffs, noffs, 0)) != hipSuccess) return fail(e, "hipHostMalloc");
    if ((e = hipMalloc(&s.dbytes, nbytes)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc(&s.doffs, noffs)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming)) != hipSuccess)
      return fail(e, "hipEventCreate");
    s.hoffs[0] = 0;
  }
  *out = r;
  return PHIP_OK;
}

int phip_ring_acquire(phip_ring* r, uint32_t* slot, uint8_t** bytes, uint64_t** offs) {
  if (!r || !slot || !bytes || !offs) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(r->mu);
  phip_ring::Slot& s = r->slots[r->next_acquire];
  if (s.state != phip_ring::kFree) return PHIP_ERR_BUSY;
  s.state = phip_ring::kAcquired;
  *slot = r->next_acquire;
  *bytes = s.hbytes;
  *offs = s.hoffs;
  s.hoffs[0] = 0;
  r->next_acquire = (r->next_acquire + 1) % (u32)r->slots.size();
  return PHIP_OK;
}

int phip_ring_submit(phip_ring* r, uint32_t slot, uint32_t n) {
  if (!r || slot >= r->slots.size() || n > r->max_msgs) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(r->mu);
  phip_ring::Slot& s = r->slots[slot];
  if (s.state != phip_ring::kAcquired) return PHIP_ERR_BUSY;
  const u64 nb = s.hoffs[n];
  if (s.hoffs[0] != 0 || nb > r->max_bytes || !datagrams_ok(s.hoffs, n)) return PHIP_ERR_INVALID;
  hipError_t e = hipSetDevice(r->h->device);
  if (e != hipSuccess) {
    r->err = hipGetErrorString(e);
    return PHIP_ERR_HIP;
  }
  if ((e = hipMemcpyAsync(s.doffs, s.hoffs, ((size_t)n + 1) * sizeof(uint64_t),
                          hipMemcpyHostToDevice, r->copy)) != hipSuccess ||
      (nb && (e = hipMemcpyAsync(s.dbytes, s.hbytes, nb, hipMemcpyHostToDevice, r->copy)) !=
                 hipSuccess) ||
      (e = hipEventRecord(s.copied, r->copy)) != hipSuccess) {
    r->err = hipGetErrorString(e);
    return PHIP_ERR_HIP;
  }
  s.n = n;
  s.state = phip_ring::kSubmitted;
  return PHIP_OK;
}

// phip_ring_receive, and with rq (host memory) phip_ring_receive_replies; with
// fr the slot holds frames (phip_ring_receive_frames, _replies): they are
// split on the device copy, and the records take the datagram path.
static int ring_receive(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                        uint32_t* stop_index, phip_reply_egress* rq,
                        const FrameAsk* fr = nullptr) {
  if (!r || slot >= r->slots.size()) return PHIP_ERR_INVALID;
  phip_ring::Slot* s;
  {
    std::lock_guard<std::mutex> g(r->mu);
    s = &r->slots[slot];
    if (s->state != phip_ring::kSubmitted || slot != r->next_receive) return PHIP_ERR_BUSY;
  }
  phip_handle* h = r->h;
  int rc;
  {
    std::lock_guard<std::mutex> g(h->mu);
    ReplyEg egs{}, *eg = rq ? &egs : nullptr;
    // (refused arguments leave the slot submitted, as a busy slot does)
    if (rq && (rc = reply_enter(h, rq, 0, eg))) return rc;
    if ((rc = begin_call(h))) return rc;
    if (stop_index) *stop_index = s->n;
    // A small slot is merged from its pinned host bytes in one launch (the
    // device copy is not waited for; the slot is freed only after it
    // finished, below); a larger one from the device copy.
    bool done = false;
    if (!fr && s->n && s->n <= kSmallMax) {
      rc = small_datagrams(h, s->hbytes, s->hoffs, s->n, now, res, stop_index, &done, rq);
      if (done || (rc && rc != PHIP_ERR_SHORT_BUFFER)) {
        if (rc && rc != PHIP_ERR_SHORT_BUFFER) rc = after_error(h, rc);
        done = true;
        const hipError_t ce = hipEventSynchronize(s->copied);
        if (ce != hipSuccess && rc == PHIP_OK)
          rc = set_err(h, PHIP_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(ce));
      }
    }
    if (!done) {
      hipError_t e = hipStreamWaitEvent(h->stream, s->copied, 0);
      if (e != hipSuccess)
        rc = set_err(h, PHIP_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
      else if (fr)   // (a checked batch: phip_ring_submit read the slot's byte count)
        rc = frames_receive_dev(h, s->dbytes, s->doffs, s->n, s->hoffs[s->n], *fr, now, res,
                                stop_index, false, eg);
      else if (s->n == 0)
        rc = eg ? reply_collect(h, eg) : PHIP_OK;
      else
        rc = receive_datagrams_dev(h, s->dbytes, s->doffs, s->n, now, res, stop_index, false, eg);
    }
    // On success the stream has drained (results copied back), so the slot's
    // host and device buffers are free; after an error wait for them first.
    if (rc) (void)hipStreamSynchronize(h->stream);  // drain; rc already set
  }
  std::lock_guard<std::mutex> g(r->mu);
  s->state = phip_ring::kFree;
  r->next_receive = (r->next_receive + 1) % (u32)r->slots.size();
  return rc;
}

int phip_ring_receive(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                      uint32_t* stop_index) {
  return ring_receive(r, slot, now, res, stop_index, nullptr);
}

int phip_ring_receive_replies(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                              uint32_t* stop_index, phip_reply_egress* rq) {
  if (!rq) return PHIP_ERR_INVALID;
  reply_zero(rq);
  return ring_receive(r, slot, now, res, stop_index, rq);
}

// ---- packed frames: the entry points ----
int phip_unframe(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs, uint32_t n_frames,
                 uint64_t bytes_len, uint32_t frame_bytes, uint64_t* rec_offs, uint32_t* rec_frame,
                 uint32_t max_recs, uint32_t* n_recs_out, uint32_t flags) {
  if (!n_recs_out) return PHIP_ERR_INVALID;
  *n_recs_out = 0;
  if ((flags & ~PHIP_DEVICE_PTRS) || !foffs || !rec_offs || !frame_bytes_ok(frame_bytes))
    return PHIP_ERR_INVALID;
  if (!(flags & PHIP_DEVICE_PTRS)) {   // the host walk: no handle, no device
    u64 total;
    const int rc = unframe_host(bytes, foffs, n_frames, bytes_len, frame_bytes,
                                [&](u64 k, u32 f, u64 p) {
                                  if (k >= max_recs) return;
                                  rec_offs[k] = p;
                                  if (rec_frame) rec_frame[k] = f;
                                }, &total);
    if (rc) return rc;
    *n_recs_out = (uint32_t)std::min<u64>(total, ~0u);
    if (total > max_recs) return PHIP_ERR_INVALID;
    rec_offs[total] = foffs[n_frames];
    return PHIP_OK;
  }
  if (!h || (n_frames && !bytes)) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  return unframe_dev(h, bytes, foffs, n_frames, bytes_len, frame_bytes, rec_offs, rec_frame,
                     max_recs, n_recs_out);
}

int phip_frame_cuts(phip_handle* h, const uint64_t* offs, uint32_t n, uint32_t frame_bytes,
                    uint64_t* frame_offs, uint32_t* frame_first, uint32_t max_frames,
                    uint32_t* n_frames_out, uint32_t flags) {
  if (!n_frames_out) return PHIP_ERR_INVALID;
  *n_frames_out = 0;
  if ((flags & ~PHIP_DEVICE_PTRS) || !offs || !frame_offs || !frame_bytes_ok(frame_bytes))
    return PHIP_ERR_INVALID;
  if (!(flags & PHIP_DEVICE_PTRS)) {   // frame_cut_run per run of records: no handle, no device
    u64 total = 0;
    for (u64 r0 = 0; r0 < n; r0 += PHIP_FRAME_TILE) {
      const u64 r1 = std::min<u64>(n, r0 + PHIP_FRAME_TILE);
      const u32 k = frame_cut_run(offs, r0, r1, frame_bytes, [&](u32 j, u64 first) {
        if (total + j >= max_frames) return;
        frame_offs[total + j] = offs[first];
        if (frame_first) frame_first[total + j] = (uint32_t)first;
      });
      if (k == ~0u) return PHIP_ERR_INVALID;
      total += k;
    }
    *n_frames_out = (uint32_t)total;   // (a frame holds a record: at most n)
    if (total > max_frames) return PHIP_ERR_INVALID;
    frame_offs[total] = offs[n];
    return PHIP_OK;
  }
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  return frame_cuts_dev(h, offs, n, frame_bytes, frame_offs, frame_first, max_frames, n_frames_out);
}

// phip_receive_frames, and with rq phip_receive_frames_replies.  Host
// pointers: the host walk, then the datagram call over the records.  Device
// pointers: unframe and the datagram path on the handle's stream.
static int receive_frames(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs,
                          uint32_t n_frames, int64_t now, const phip_results* res,
                          uint32_t* stop_index, phip_reply_egress* rq, const FrameAsk& fr,
                          uint32_t flags) {
  if (!fr.n_recs_out) return PHIP_ERR_INVALID;
  *fr.n_recs_out = 0;
  if (!h || !foffs || (n_frames && !bytes)) return PHIP_ERR_INVALID;
  if (!frame_bytes_ok(fr.frame_bytes)) {
    std::lock_guard<std::mutex> g(h->mu);
    return set_err(h, PHIP_ERR_INVALID, "frames: frame_bytes %u outside [%d, %d]", fr.frame_bytes,
                   PHIP_FRAME_MIN_BYTES, PHIP_FRAME_MAX_BYTES);
  }
  if (!(flags & PHIP_DEVICE_PTRS)) {
    std::vector<uint64_t> ro;
    u64 total;
    const int rc = unframe_host(bytes, foffs, n_frames, foffs[n_frames], fr.frame_bytes,
                                [&](u64 k, u32 f, u64 p) {
                                  if (k >= fr.max_recs) return;
                                  ro.push_back(p);
                                  if (fr.rec_frame) fr.rec_frame[k] = f;
                                }, &total);
    *fr.n_recs_out = (uint32_t)std::min<u64>(total, ~0u);
    if (rc || total > fr.max_recs) {
      std::lock_guard<std::mutex> g(h->mu);
      return set_err(h, PHIP_ERR_INVALID, rc ? "frames: a malformed or oversized frame entry"
                                             : "frames: more records than max_recs");
    }
    ro.push_back(foffs[n_frames]);
    return receive_datagrams(h, bytes, ro.data(), (uint32_t)total, now, res, stop_index, flags, rq);
  }
  std::lock_guard<std::mutex> g(h->mu);
  ReplyEg egs{}, *eg = rq ? &egs : nullptr;
  if (rq)
    if (int rc0 = reply_enter(h, rq, flags, eg)) return rc0;
  if (int rc0 = begin_call(h)) return rc0;
  return frames_receive_dev(h, bytes, foffs, n_frames, 0, fr, now, res, stop_index, true, eg);
}

int phip_receive_frames(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs,
                        uint32_t n_frames, int64_t now, const phip_results* res,
                        uint32_t* stop_index, uint32_t frame_bytes, uint32_t* rec_frame,
                        uint32_t max_recs, uint32_t* n_recs_out, uint32_t flags) {
  return receive_frames(h, bytes, foffs, n_frames, now, res, stop_index, nullptr,
                        FrameAsk{frame_bytes, rec_frame, max_recs, n_recs_out}, flags);
}

int phip_receive_frames_replies(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs,
                                uint32_t n_frames, int64_t now, const phip_results* res,
                                uint32_t* stop_index, phip_reply_egress* rq, uint32_t frame_bytes,
                                uint32_t* rec_frame, uint32_t max_recs, uint32_t* n_recs_out,
                                uint32_t flags) {
  if (!rq) return PHIP_ERR_INVALID;
  reply_zero(rq);
  return receive_frames(h, bytes, foffs, n_frames, now, res, stop_index, rq,
                        FrameAsk{frame_bytes, rec_frame, max_recs, n_recs_out}, flags);
}

int phip_ring_receive_frames(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                             uint32_t frame_bytes, uint32_t* rec_frame, uint32_t max_recs,
                             uint32_t* n_recs_out, uint32_t* stop_index) {
  if (!n_recs_out || !frame_bytes_ok(frame_bytes)) return PHIP_ERR_INVALID;
  *n_recs_out = 0;
  const FrameAsk fr{frame_bytes, rec_frame, max_recs, n_recs_out};
  return ring_receive(r, slot, now, res, stop_index, nullptr, &fr);
}

int phip_ring_receive_frames_replies(phip_ring* r, uint32_t slot, int64_t now,
                                     const phip_results* res, uint32_t frame_bytes,
                                     uint32_t* rec_frame, uint32_t max_recs, uint32_t* n_recs_out,
                                     uint32_t* stop_index, phip_reply_egress* rq) {
  if (!rq || !n_recs_out || !frame_bytes_ok(frame_bytes)) return PHIP_ERR_INVALID;
  reply_zero(rq);
  *n_recs_out = 0;
  const FrameAsk fr{frame_bytes, rec_frame, max_recs, n_recs_out};
  return ring_receive(r, slot, now, res, stop_index, rq, &fr);
}

int phip_upsert_soa(phip_handle* h, const phip_msgs* m, int64_t now, const phip_results* res,
                    uint32_t flags) {
  if (!h || !m) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  u32 n = m->n;
  if (n == 0) return PHIP_OK;
  if (!m->names || !m->name_offs || !m->added || !m->taken || !m->elapsed) return PHIP_ERR_INVALID;
  bool dev = flags & PHIP_DEVICE_PTRS;
  if (!dev && !names_ok(m->name_offs, n)) return set_err(h, PHIP_ERR_NAME_TOO_LARGE, "name > 231 bytes");
  int rc;
  if (!dev) {
    bool done = false;
    if ((rc = small_uniform(h, m, PHIP_OP_UPSERT, now, res, &done))) return after_error(h, rc);
    if (done) return PHIP_OK;
  }
  NamesOffs src;
  const uint64_t *a, *t;
  const int64_t* e;
  OutView ow{};
  if ((rc = stage_names(h, m->names, m->name_offs, n, dev, &src, m->names_len)) ||
      (rc = stage(h, B_A, m->added, n, dev, &a)) || (rc = stage(h, B_T, m->taken, n, dev, &t)) ||
      (rc = stage(h, B_E, m->elapsed, n, dev, &e)) || (rc = outputs(h, res, n, dev, &ow)))
    return rc;
  OpView ov{};
  ov.kind0 = PHIP_OP_UPSERT;
  ov.now0 = now;
  ov.a = a; ov.t = t; ov.e = e;
  if ((rc = ordered(h, src, n, ov, ow))) return after_error(h, rc);
  return copy_outputs(h, res, n, dev, ow);
}

// The caps of a batch's egress (patrolhip.h "Coalesced egress"): every op a
// new bucket's TAKE, a request and a state datagram each.
static bool egress_need(u64 n, u64 name_bytes, bool dev, u64* msgs, u64* cap) {
  // (an ordered batch has at most 2^30 ops; the bound on the bytes keeps the sums in 64 bits)
  if (n > kMaxOrderedOps || name_bytes > (u64)kMaxOrderedOps * PHIP_BUCKET_PACKET_SIZE) return false;
  *msgs = 2 * n;
  u64 c = 2 * (PHIP_BUCKET_FIXED_SIZE * n + name_bytes);
  if (dev) c = ((c + 7) & ~7ull) + 8;   // (the sweep's device form: a multiple of 8, 8 bytes past the budget)
  *cap = c;
  return true;
}

int phip_egress_caps(uint32_t n_ops, uint64_t name_bytes, uint32_t flags, uint32_t* max_msgs,
                     uint64_t* out_cap) {
  u64 m, c;
  if (!max_msgs || !out_cap || (flags & ~PHIP_DEVICE_PTRS) ||
      !egress_need(n_ops, name_bytes, flags & PHIP_DEVICE_PTRS, &m, &c))
    return PHIP_ERR_INVALID;
  *max_msgs = (u32)m;
  *out_cap = c;
  return PHIP_OK;
}

// phip_apply_mixed (eg == nullptr: exactly that call) and
// phip_apply_mixed_egress, on the same paths: small_mixed, or ordered() with
// the egress launches behind its folds.
static int apply_mixed(phip_handle* h, const phip_ops* ops, const phip_results* res,
                       phip_egress* eg, uint32_t flags) {
  if (eg) eg->n_incast = eg->n = 0, eg->bytes = 0;
  if (!h || !ops) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  u32 n = ops->n;
  bool dev = flags & PHIP_DEVICE_PTRS;
  if (eg && (!eg->out || !eg->offs))
    return set_err(h, PHIP_ERR_INVALID, "egress: out and offs are required");
  if (n == 0) return eg ? datagrams_none(h, eg->offs, dev, true) : PHIP_OK;
  if (!ops->kind || !ops->names || !ops->name_offs || !ops->now) return PHIP_ERR_INVALID;
  if (!dev && !names_ok(ops->name_offs, n)) return set_err(h, PHIP_ERR_NAME_TOO_LARGE, "name > 231 bytes");
  bool uniform = false;
  if (!dev) {
    bool need_take = false, need_state = false;
    uniform = true;
    for (u32 i = 0; i < n; ++i) {
      if (ops->kind[i] > PHIP_OP_UPSERT) return set_err(h, PHIP_ERR_INVALID, "bad op kind at %u", i);
      if (ops->kind[i] == PHIP_OP_TAKE) need_take = true; else need_state = true;
      uniform &= ops->kind[i] == ops->kind[0];
    }
    if (need_take && (!ops->freq || !ops->per || !ops->count)) return PHIP_ERR_INVALID;
    if (need_state && (!ops->added || !ops->taken || !ops->elapsed)) return PHIP_ERR_INVALID;
  }
  int rc;
  // the change set: this call's TAKE / UPSERT ops mark their buckets, unless
  // its datagrams leave with it (eg)
  const bool track = h->track && !eg;
  EgressOut eo{};
  u64 need_cap = 0;
  if (eg) {
    // the caps, before anything is applied: a valid call never truncates
    const u64 name_bytes = !dev ? (u64)ops->name_offs[n] - ops->name_offs[0]
                                : ops->names_len ? (u64)ops->names_len : (u64)PHIP_MAX_NAME_LEN * n;
    u64 need_msgs;
    if (!egress_need(n, name_bytes, dev, &need_msgs, &need_cap))
      return set_err(h, PHIP_ERR_INVALID, "egress: a batch of %u ops exceeds 2^30", n);
    if (dev && ((reinterpret_cast<uintptr_t>(eg->out) & 7) || (eg->out_cap & 7)))
      return set_err(h, PHIP_ERR_INVALID, "egress: a device buffer is 8-byte aligned and a multiple of 8");
    if (eg->max_msgs < need_msgs || eg->out_cap < need_cap)
      return set_err(h, PHIP_ERR_INVALID,
                     "egress: max_msgs %u, out_cap %llu below the batch's worst case %llu, %llu "
                     "(phip_egress_caps): nothing applied",
                     eg->max_msgs, (unsigned long long)eg->out_cap, (unsigned long long)need_msgs,
                     (unsigned long long)need_cap);
    eo.max_msgs = (u32)need_msgs;
    eo.budget = dev ? need_cap - 8 : need_cap;
  }
  // what runs behind the ordered path's folds: the egress, or the marks
  const Behind behind{uniform, uniform && ops->kind[0] != PHIP_OP_RECEIVE, eg ? &eo : nullptr};
  if (!dev && h->small) {
    bool done = false;
    if ((rc = small_mixed(h, ops, res, &done, eg, track))) {
      if (eg) eg->n_incast = eg->n = 0, eg->bytes = 0;
      return after_error(h, rc);
    }
    if (done) return PHIP_OK;
  }
  NamesOffs src;
  OpView ov{};
  const u8* kind;
  OutView ow{};
  if ((rc = stage_names(h, ops->names, ops->name_offs, n, dev, &src, ops->names_len)) ||
      (rc = stage(h, B_KIND, ops->kind, n, dev, &kind)) ||
      (rc = stage(h, B_NOW, ops->now, n, dev, &ov.now)) ||
      (rc = stage(h, B_FREQ, ops->freq, n, dev, &ov.freq)) ||
      (rc = stage(h, B_PER, ops->per, n, dev, &ov.per)) ||
      (rc = stage(h, B_COUNT, ops->count, n, dev, &ov.count)) ||
      (rc = stage(h, B_A, ops->added, n, dev, &ov.a)) ||
      (rc = stage(h, B_T, ops->taken, n, dev, &ov.t)) ||
      (rc = stage(h, B_E, ops->elapsed, n, dev, &ov.e)) || (rc = outputs(h, res, n, dev, &ow)))
    return rc;
  ov.kind = kind;
  // the statuses say which buckets the batch created: a column of the
  // library's own when the caller asked for none
  if ((track || eg) && !ow.status && (rc = ensure(h, B_STATUS, n, &ow.status))) return rc;
  if (!eg) {
    if ((rc = ordered(h, src, n, ov, ow, track ? &behind : nullptr))) return after_error(h, rc);
    return copy_outputs(h, res, n, dev, ow);
  }
  eo.out = eg->out;
  eo.offs = reinterpret_cast<u64*>(eg->offs);
  if (!dev && ((rc = ensure(h, B_EGOUT, (size_t)need_cap + 8, &eo.out)) ||
               (rc = ensure(h, B_EGOFFS, 2 * (size_t)n + 1, &eo.offs))))
    return rc;
  if ((rc = ordered(h, src, n, ov, ow, &behind))) return after_error(h, rc);
  if ((rc = read_ctr(h))) return rc;
  const u32* c = h->ctr_host;
  u64 bytes;
  std::memcpy(&bytes, c + kCtrEgBytes, sizeof bytes);
  if (c[kCtrEgErr] || c[kCtrEgN] > eo.max_msgs || bytes > eo.budget || c[kCtrEgIncast] > c[kCtrEgN])
    return set_err(h, PHIP_ERR_INVALID, "internal: egress of %u datagrams, %llu bytes (flag %u)",
                   c[kCtrEgN], (unsigned long long)bytes, c[kCtrEgErr]);
  // (the copies wait for copy_outputs' synchronise)
  if (!dev && (rc = datagrams_back(h, eg->out, eo.out, bytes, eg->offs, eo.offs, c[kCtrEgN])))
    return rc;
  if ((rc = copy_outputs(h, res, n, dev, ow))) return rc;
  eg->n_incast = c[kCtrEgIncast];
  eg->n = c[kCtrEgN];
  eg->bytes = bytes;
  return PHIP_OK;
}

int phip_apply_mixed(phip_handle* h, const phip_ops* ops, const phip_results* res, uint32_t flags) {
  return apply_mixed(h, ops, res, nullptr, flags);
}

int phip_apply_mixed_egress(phip_handle* h, const phip_ops* ops, const phip_results* res,
                            phip_egress* eg, uint32_t flags) {
  if (!eg) return PHIP_ERR_INVALID;
  return apply_mixed(h, ops, res, eg, flags);
}

int phip_take(phip_handle* h, const uint8_t* names, const uint32_t* name_offs, uint32_t n,
              const int64_t* now, const int64_t* freq, const int64_t* per, const uint64_t* count,
              uint64_t* remaining_out, uint8_t* ok_out, uint32_t flags) {
  if (!h) return PHIP_ERR_INVALID;
  if (n == 0) return PHIP_OK;
  if (flags & PHIP_DEVICE_PTRS) return set_err(h, PHIP_ERR_INVALID, "phip_take: use phip_apply_mixed for device pointers");
  std::vector<u8> kind(n, PHIP_OP_TAKE), st(n);
  phip_ops ops{};
  ops.n = n;
  ops.kind = kind.data();
  ops.names = names;
  ops.name_offs = name_offs;
  ops.now = now;
  ops.freq = freq;
  ops.per = per;
  ops.count = count;
  phip_results res{};
  res.status = st.data();
  res.remaining = remaining_out;
  int rc = phip_apply_mixed(h, &ops, &res, flags);
  if (rc) return rc;
  if (ok_out)
    for (u32 i = 0; i < n; ++i) ok_out[i] = (st[i] & 0x7F) == PHIP_ST_TAKE_OK;
  return PHIP_OK;
}

int phip_hash_names(phip_handle* h, const uint8_t* names, const uint32_t* name_offs, uint32_t n,
                    uint64_t* out, uint32_t flags) {
  if ((n && (!names || !name_offs)) || (n && !out)) return PHIP_ERR_INVALID;
  if (!(flags & PHIP_DEVICE_PTRS)) {
    for (u32 i = 0; i < n; ++i) {
      u64 hh = kFnvOffset;
      for (u32 k = name_offs[i]; k < name_offs[i + 1]; ++k) hh = fnv_step(hh, names[k]);
      out[i] = hh;
    }
    return PHIP_OK;
  }
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (n == 0) return PHIP_OK;
  k_hash_names<<<grid_for(n), kBlock, 0, h->stream>>>(NamesOffs{names, name_offs}, n, out);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_route_pack(phip_handle* h, const phip_msgs* m, uint32_t world, uint8_t* send_names,
                    uint32_t* send_lens, uint64_t* send_added, uint64_t* send_taken,
                    int64_t* send_elapsed, uint64_t* counts, uint64_t* name_bytes,
                    uint32_t flags) {
  if (!h || !m || !(flags & PHIP_DEVICE_PTRS) || world == 0 || world > kRouteMaxWorld)
    return PHIP_ERR_INVALID;
  const u32 n = m->n;
  if (n && (!m->names || !m->name_offs || !m->added || !m->taken || !m->elapsed || !send_names ||
            !send_lens || !send_added || !send_taken || !send_elapsed || !counts || !name_bytes))
    return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  int rc;
  // (the route kernels do not check as they go: a checked batch's offsets
  // first, so that no malformed entry is ever hashed or copied)
  u32 first_bad;
  if ((rc = check_offsets_on(h, h->stream, m->names, m->name_offs, m->names_len, n, &first_bad)))
    return rc;
  if (first_bad != ~0u)
    return set_err(h, PHIP_ERR_INVALID,
                   "malformed name offsets at message %u (names_len check): nothing packed",
                   first_bad);
  const void* dir = nullptr;
  if ((flags & PHIP_ROUTE_COMBINE) && (rc = route_dir_on(h, h->stream, *m, world, &dir))) return rc;
  if ((rc = route_pack_on(h, h->stream, *m, world, dir, send_names, send_lens, send_added,
                          send_taken, send_elapsed, counts, name_bytes)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_route_pack_datagrams(phip_handle* h, const phip_wire* w, uint32_t world,
                              uint8_t* send_names, uint32_t* send_lens, uint64_t* send_added,
                              uint64_t* send_taken, int64_t* send_elapsed, uint64_t* counts,
                              uint64_t* name_bytes, uint32_t* stop, uint32_t flags) {
  if (!h || !w || !(flags & PHIP_DEVICE_PTRS) || (flags & ~(PHIP_DEVICE_PTRS | PHIP_ROUTE_COMBINE)) ||
      world == 0 || world > kRouteMaxWorld || !counts || !name_bytes)
    return PHIP_ERR_INVALID;
  const u32 n = w->n;
  if (n && (!w->bytes || !w->offs || !send_names || !send_lens || !send_added || !send_taken ||
            !send_elapsed))
    return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (stop) *stop = n;
  int rc;
  // the Go loop's stop rule first (repo.go:70-74): the route kernels read
  // well-formed datagrams only
  u32 at, first_bad;
  if ((rc = wire_scan_on(h, h->stream, w->bytes, w->offs, w->bytes_len, n, &at, &first_bad)))
    return rc;
  if (first_bad != ~0u)
    return set_err(h, PHIP_ERR_INVALID,
                   "malformed datagram offsets at datagram %u (bytes_len check): nothing packed",
                   first_bad);
  if (stop) *stop = at;
  const Datagrams src{w->bytes, w->offs};
  const void* dir = nullptr;
  if ((flags & PHIP_ROUTE_COMBINE) && (rc = route_dir_src(h, h->stream, src, at, world, &dir)))
    return rc;
  if ((rc = route_pack_src(h, h->stream, src, nullptr, nullptr, nullptr, at, world, dir, send_names,
                           send_lens, send_added, send_taken, send_elapsed, counts, name_bytes)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (at < n) return set_err(h, PHIP_ERR_SHORT_BUFFER, "short buffer at datagram %u", at);
  return PHIP_OK;
}

int phip_route_pack_ops(phip_handle* h, const phip_ops* ops, uint32_t world, uint8_t* send_names,
                        uint32_t* send_lens, uint8_t* send_kind, int64_t* send_now,
                        uint64_t* send_x0, uint64_t* send_x1, uint64_t* send_x2,
                        uint32_t* send_src, uint64_t* counts, uint64_t* name_bytes,
                        uint32_t flags) {
  if (!h || !ops || flags != PHIP_DEVICE_PTRS || world == 0 || world > kRouteMaxWorld ||
      !counts || !name_bytes)
    return PHIP_ERR_INVALID;
  const u32 n = ops->n;
  const bool peek = !ops->kind && !send_kind;   // the query pack: no kind column on either side
  if (n && ((!peek && (!ops->kind || !send_kind)) || !ops->names || !ops->name_offs || !ops->now ||
            !send_names || !send_lens || !send_now || !send_x0 || !send_x1 || !send_x2 || !send_src))
    return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  int rc;
  u32 first_bad;
  if ((rc = check_offsets_on(h, h->stream, ops->names, ops->name_offs, ops->names_len, n,
                             &first_bad)))
    return rc;
  if (first_bad != ~0u)
    return set_err(h, PHIP_ERR_INVALID,
                   "malformed name offsets at op %u (names_len check): nothing packed", first_bad);
  rc = peek ? route_pack_ops_on<true>(h, h->stream, *ops, world, send_names, send_lens, nullptr,
                                      send_now, send_x0, send_x1, send_x2, send_src, counts,
                                      name_bytes)
            : route_pack_ops_on(h, h->stream, *ops, world, send_names, send_lens, send_kind,
                                send_now, send_x0, send_x1, send_x2, send_src, counts, name_bytes);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_ae_local_max(phip_handle* h, const int64_t* replicas, uint32_t nrep, uint64_t nbuckets,
                      int64_t* out, uint32_t flags) {
  if (!h || !(flags & PHIP_DEVICE_PTRS) || (nbuckets && (!replicas || !out)) || nrep == 0)
    return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (nbuckets == 0) return PHIP_OK;
  {
    Launch l(h, "k_ae_local_max");
    k_ae_local_max<<<dim3(grid_for(nbuckets), 3), kBlock, 0, h->stream>>>(replicas, nrep, nbuckets,
                                                                         out);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_ae_apply(phip_handle* h, int64_t* replicas, uint32_t nrep, uint64_t nbuckets,
                  const int64_t* joined, uint32_t flags) {
  if (!h || !(flags & PHIP_DEVICE_PTRS) || (nbuckets && (!replicas || !joined)) || nrep == 0)
    return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (nbuckets == 0) return PHIP_OK;
  {
    Launch l(h, "k_ae_apply");
    k_ae_apply<<<dim3(grid_for(nbuckets), 3), kBlock, 0, h->stream>>>(replicas, nrep, nbuckets,
                                                                     joined);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_ae_join(phip_handle* h, int64_t* replicas, uint32_t nrep, uint64_t nbuckets,
                 uint32_t flags) {
  if (!h || !(flags & PHIP_DEVICE_PTRS) || (nbuckets && !replicas) || nrep == 0)
    return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  if (nbuckets == 0) return PHIP_OK;
  {
    Launch l(h, "k_ae_join");
    k_ae_join<<<dim3(grid_for((nbuckets + 1) / 2), 3), kBlock, 0, h->stream>>>(replicas, nrep,
                                                                                nbuckets);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

int phip_last_timings(phip_handle* h, const char** names, float* ms, int max) {
  if (!h) return 0;
  std::lock_guard<std::mutex> g(h->mu);
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  int k = 0;
  for (auto& t : h->timings) {
    if (k >= max) break;
    float v = 0;
    if (hipEventElapsedTime(&v, t.a, t.b) != hipSuccess) v = -1.0f;
    if (names) names[k] = t.name;
    if (ms) ms[k] = v;
    ++k;
  }
  return k;
}

void phip_set_timing(phip_handle* h, int on) {
  if (!h) return;
  std::lock_guard<std::mutex> g(h->mu);
  h->timing = on != 0;
  h->timing_accumulate = on == 2;
  h->timings.clear();
  h->pool_used = 0;
  // events for a timed loop made up front, not inside it
  while (on == 2 && h->event_pool.size() < 1024) {
    Timing tm{"", nullptr, nullptr};
    if (hipEventCreate(&tm.a) != hipSuccess) break;
    if (hipEventCreate(&tm.b) != hipSuccess) {
      (void)hipEventDestroy(tm.a);
      break;
    }
    h->event_pool.push_back(tm);
  }
}

int phip_set_stream(phip_handle* h, void* stream) {
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  // work already queued on the previous stream comes first
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stream = stream ? (hipStream_t)stream : h->own_stream;
  return PHIP_OK;
}

// Eviction sweep (patrolhip.h "Evict idle buckets"): the count pass, then --
// unless it is a dry run or too little is idle -- grow_table's sequence with
// k_evict_move in k_rehash's place: allocate and clear the new table (and a
// new arena when the old one holds anything), move, read the counters, swap,
// free.  Until the swap every error frees the new memory and leaves the old
// table and arena as they were.  Nothing else in the handle holds slot
// numbers or arena offsets across calls (a queued batch, the one thing that
// could, was finished by begin_call), so, as after growth, nothing is reset.
static int evict_idle(phip_handle* h, i64 now, i64 idle_ns, u64 min_evict, phip_evict_stats* out,
                      u32 flags) {
  int rc;
  u64* ev;
  if ((rc = ensure(h, B_EVICT, kEvWords, &ev))) return rc;
  HIPCHK(h, hipMemsetAsync(ev, 0, kEvWords * sizeof(u64), h->stream));
  {
    Launch l(h, "k_evict_count");
    k_evict_count<<<std::min<unsigned>(grid_for(h->cap), 8u * (unsigned)h->ncu), kBlock, 0,
                    h->stream>>>(h->recs, h->cap, now, idle_ns, ev);
  }
  HIPCHK(h, hipGetLastError());
  u64 c[kEvWords] = {};
  HIPCHK(h, hipMemcpyAsync(c, ev, sizeof c, hipMemcpyDeviceToHost, h->stream));
  const u64 used = arena_used(h);   // (synchronises)
  if (used == ~0ull) return set_err(h, PHIP_ERR_HIP, "evict: arena cursor read failed");
  const u64 n_idle = c[kEvIdle], keep = c[kEvKeep], long_bytes = c[kEvLongBytes];
  phip_evict_stats st{};
  st.idle = n_idle;
  st.buckets = h->n_buckets;
  st.slots = h->cap;
  st.arena_used = used;
  if (out) *out = st;
  if ((flags & PHIP_EVICT_DRY_RUN) || n_idle < std::max<u64>(min_evict, 1)) return PHIP_OK;

  u32 newL = h->L;
  if (flags & PHIP_EVICT_SHRINK)
    for (u32 l = std::min(h->L_open, h->L); l < h->L; ++l)
      if (keep <= load_limit(1ull << l, h->load_pct) / 2) {
        newL = l;
        break;
      }
  const u64 ncap = 1ull << newL;
  const u64 narena_cap = used ? std::max(h->arena_open, long_bytes) : 0;
  Rec* nrecs = nullptr;
  u32* naux = nullptr;
  u8* narena = nullptr;
  Marks nmarks{};
  u64* nbase = nullptr;
  if (hipMalloc(&nrecs, ncap * sizeof(Rec)) != hipSuccess ||
      hipMalloc(&naux, ncap * sizeof(u32)) != hipSuccess ||
      (narena_cap && hipMalloc(&narena, narena_cap + 64) != hipSuccess) ||
      (h->track && alloc_marks(h, ncap, &nmarks)) ||
      (h->usage && alloc_base(h, ncap, &nbase))) {
    (void)hipGetLastError();
    if (nrecs) (void)hipFree(nrecs);
    if (naux) (void)hipFree(naux);
    if (narena) (void)hipFree(narena);
    if (nmarks.state) (void)hipFree(nmarks.state);
    return set_err(h, PHIP_ERR_FULL, "evict: device memory for 2^%u slots and %llu arena bytes",
                   newL, (unsigned long long)narena_cap);
  }
  // from here on an error frees the new table and arena (the old ones stay live)
  auto drop_new = [&](int err) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(nrecs);
    (void)hipFree(naux);
    if (narena) (void)hipFree(narena);
    if (nmarks.state) (void)hipFree(nmarks.state);
    if (nbase) (void)hipFree(nbase);
    return err;
  };
  if (hipMemsetAsync(nrecs, 0, ncap * sizeof(Rec), h->stream) != hipSuccess ||
      hipMemsetAsync(naux, 0, ncap * sizeof(u32), h->stream) != hipSuccess ||
      // (both flags: kCtrTableFull is the next word)
      hipMemsetAsync(h->ctr + kCtrArenaFull, 0, 2 * sizeof(u32), h->stream) != hipSuccess)
    return drop_new(set_err(h, PHIP_ERR_HIP, "evict: clearing the new table failed"));
  Table nt = table(h);
  nt.recs = nrecs;
  nt.aux = naux;
  nt.arena = narena ? narena : h->arena;
  nt.L = newL;
  {
    Launch l(h, "k_evict_move");
    k_evict_move<<<grid_for(h->cap, kEvictBlock), kEvictBlock, 0, h->stream>>>(
        h->recs, h->aux, h->cap, h->arena, used, now, idle_ns, nt, ncap, narena, narena_cap, ev,
        h->ctr, h->marks, nmarks, h->base, nbase);
  }
  if (hipGetLastError() != hipSuccess)
    return drop_new(set_err(h, PHIP_ERR_HIP, "k_evict_move launch failed"));
  if (hipMemcpyAsync(c, ev, sizeof c, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return drop_new(set_err(h, PHIP_ERR_HIP, "evict: counter read failed"));
  if ((rc = read_ctr(h))) return drop_new(rc);   // synchronises: the old table is no longer read
  if (h->ctr_host[kCtrTableFull])
    return drop_new(set_err(h, PHIP_ERR_INVALID, "internal: evict probe wrapped"));
  if (h->ctr_host[kCtrArenaFull] || c[kEvCursor] != long_bytes)
    return drop_new(set_err(h, PHIP_ERR_INVALID,
                            "internal: evict moved %llu long-name bytes, counted %llu",
                            (unsigned long long)c[kEvCursor], (unsigned long long)long_bytes));
  if (narena &&
      (hipMemcpyAsync(h->arena_cursor, &c[kEvCursor], sizeof(u64), hipMemcpyHostToDevice,
                      h->stream) != hipSuccess ||
       hipStreamSynchronize(h->stream) != hipSuccess))
    return drop_new(set_err(h, PHIP_ERR_HIP, "evict: setting the arena cursor failed"));
  Rec* orecs = h->recs;
  u32* oaux = h->aux;
  u32* omarks = h->marks.state;
  u64* obase = h->base;
  u8* oarena = narena ? h->arena : nullptr;
  h->recs = nrecs;
  h->aux = naux;
  h->marks = nmarks;
  h->base = nbase;
  h->L = newL;
  h->cap = ncap;
  h->max_load = load_limit(ncap, h->load_pct);
  h->n_buckets = keep;
  ++h->layout_gen;
  if (narena) {
    h->arena = narena;
    h->arena_cap = narena_cap;
  }
  st.evicted = n_idle;
  st.buckets = keep;
  st.slots = ncap;
  st.arena_used = narena ? c[kEvCursor] : used;
  st.arena_freed = used - st.arena_used;
  if (out) *out = st;
  HIPCHK(h, hipFree(orecs));
  HIPCHK(h, hipFree(oaux));
  if (omarks) HIPCHK(h, hipFree(omarks));
  if (obase) HIPCHK(h, hipFree(obase));
  if (oarena) HIPCHK(h, hipFree(oarena));
  return PHIP_OK;
}

int phip_evict_idle(phip_handle* h, int64_t now, int64_t idle_ns, uint64_t min_evict,
                    phip_evict_stats* out, uint32_t flags) {
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (idle_ns <= 0) return set_err(h, PHIP_ERR_INVALID, "evict: idle_ns must be positive");
  if (flags & ~(PHIP_EVICT_SHRINK | PHIP_EVICT_DRY_RUN))
    return set_err(h, PHIP_ERR_INVALID, "evict: unknown flag bits 0x%x", flags);
  return evict_idle(h, now, idle_ns, min_evict, out, flags);
}

}  // extern "C"

namespace {
// ---- the sweep window (export sweep, throttled sweep) ----
// One call's window of slots: [s0, s_end), ntiles tiles of PHIP_SWEEP_TILE.
struct SweepWindow {
  u64 s0, s_end;
  u32 ntiles;
  bool restarted;   // the cursor was another layout's: the window begins at slot 0
};

// The window at the cursor: W slots, rounded up to whole tiles (one at least)
// and cut at the table's end.  empty: the call asks for nothing (an empty
// partition mask), reads no slot and is done.
SweepWindow sweep_open(const phip_handle* h, const phip_sweep_cursor* cur, u64 W,
                       bool empty = false) {
  SweepWindow w{};
  w.s0 = cur->slot;
  if ((cur->slot || cur->layout) && cur->layout != h->layout_gen) {
    w.s0 = 0;
    w.restarted = true;
  }
  w.s0 = empty ? h->cap : std::min<u64>(w.s0, h->cap);
  W = std::max<u64>(W, PHIP_SWEEP_TILE);
  W = (W + PHIP_SWEEP_TILE - 1) / PHIP_SWEEP_TILE * PHIP_SWEEP_TILE;
  w.s_end = std::min<u64>(w.s0 + W, h->cap);
  w.ntiles = (u32)((w.s_end - w.s0 + PHIP_SWEEP_TILE - 1) / PHIP_SWEEP_TILE);
  return w;
}

// The sweep's counter words, read back: one synchronise.
int sweep_read(phip_handle* h, const u64* ctr, u64 (&c)[kSwWords]) {
  HIPCHK(h, hipMemcpyAsync(c, ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PHIP_OK;
}

// The end of a window call.  c: the counters behind the write pass (zeros for
// a window without tiles, which launched nothing), checked against the call's
// caps; what / unit name the sweep and its entries in the messages.  The
// cursor moves to the first record not written -- kSwNext counts from
// next_base -- or to the window's end.
int sweep_close(phip_handle* h, const SweepWindow& w, const u64 (&c)[kSwWords], const char* what,
                const char* unit, u64 max_n, u64 budget, u64 next_base, phip_sweep_cursor* cur,
                phip_sweep_stats* st) {
  if (c[kSwErr])
    return set_err(h, PHIP_ERR_INVALID, "internal: %s met a long name outside the arena", what);
  if (c[kSwN] > max_n || c[kSwBytes] > budget)
    return set_err(h, PHIP_ERR_INVALID, "internal: %s wrote %llu %s, %llu bytes", what,
                   (unsigned long long)c[kSwN], unit, (unsigned long long)c[kSwBytes]);
  const u64 next = w.ntiles && c[kSwNext] != ~0ull ? next_base + c[kSwNext] : w.s_end;
  cur->slot = next;
  cur->layout = h->layout_gen;
  phip_sweep_stats s{};
  s.n = c[kSwN];
  s.bytes = c[kSwBytes];
  s.slots_scanned = w.s_end - w.s0;
  s.restarted = w.restarted;
  s.done = next >= h->cap;
  *st = s;
  return PHIP_OK;
}

// Count mode: the counters cleared, launch(grid, buffer) over the whole table
// on the striding grid (a few workgroups per compute unit), the two sums read
// back.  mw: the words of a mask behind the counters.
template <class F>
int sweep_count_mode(phip_handle* h, size_t mw, F launch, phip_sweep_stats* st) {
  int rc;
  u64* ctr;
  u64 c[kSwWords];
  if ((rc = ensure(h, B_SWEEP, SweepBuf::words(mw, 0), &ctr))) return rc;
  HIPCHK(h, hipMemsetAsync(ctr, 0, kSwWords * sizeof(u64), h->stream));
  if ((rc = launch(std::min<unsigned>(grid_for(h->cap), 8u * (unsigned)h->ncu),
                   SweepBuf(ctr, mw, 0))))
    return rc;
  HIPCHK(h, hipGetLastError());
  if ((rc = sweep_read(h, ctr, c))) return rc;
  phip_sweep_stats s{};
  s.n = c[kSwN];
  s.bytes = c[kSwBytes];
  s.slots_scanned = h->cap;
  *st = s;
  return PHIP_OK;
}
}  // namespace

extern "C" {
// Export sweep (patrolhip.h "Anti-entropy sweep"; kernels in phip_kernels.hpp
// "export sweep").  One window of slots per call: count per tile, scan, write.
// A device-pointer call reads the four counters back once, at its end; a
// host-pointer call also reads the window's totals after the scan, to size
// its staging buffers by what the window holds instead of by the caller's caps.
// phip_export_sweep is the no-mask case (parts == false: the kernels'
// unfiltered instantiations, the unfiltered window); phip_export_sweep_parts
// copies its mask once per call behind the counters of the sweep's buffer and
// widens the window by the share of the partitions it asks for.
static int export_sweep(phip_handle* h, phip_sweep_cursor* cur, int64_t now, int64_t idle_ns,
                        bool parts, uint32_t log2_parts, const uint64_t* part_mask, uint8_t* out,
                        uint64_t out_cap, uint64_t* offs, uint32_t max_msgs, phip_sweep_stats* st,
                        uint32_t flags) {
  if (!h || !cur || !st) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (flags & ~(PHIP_DEVICE_PTRS | PHIP_SWEEP_COUNT))
    return set_err(h, PHIP_ERR_INVALID, "sweep: unknown flag bits 0x%x", flags);
  if (idle_ns < 0) return set_err(h, PHIP_ERR_INVALID, "sweep: idle_ns must not be negative");
  if (parts && (!part_mask || log2_parts > PHIP_DIGEST_MAX_LOG2_PARTS))
    return set_err(h, PHIP_ERR_INVALID, "sweep: a partition mask and log2_parts <= %d are required",
                   PHIP_DIGEST_MAX_LOG2_PARTS);
  const bool dev = flags & PHIP_DEVICE_PTRS;
  // the mask's words, and m: its set bits among the first 2^k
  const u64 nparts = parts ? 1ull << log2_parts : 1;
  const size_t mw = parts ? (size_t)std::max<u64>(nparts / 64, 1) : 0;
  u64 m = 0;
  for (size_t w = 0; w < mw; ++w)
    m += (u64)__builtin_popcountll(nparts < 64 ? part_mask[w] & ((1ull << nparts) - 1)
                                               : part_mask[w]);
  const bool none = parts && !m;
  int rc;
  if (flags & PHIP_SWEEP_COUNT) {
    if (out) return set_err(h, PHIP_ERR_INVALID, "sweep: count mode takes no output buffer");
    if (none) {
      *st = phip_sweep_stats{};
      return PHIP_OK;
    }
    return sweep_count_mode(h, mw, [&](unsigned grid, const SweepBuf& b) -> int {
      if (parts)
        HIPCHK(h, hipMemcpyAsync(b.mask, part_mask, mw * sizeof(u64), hipMemcpyHostToDevice,
                                 h->stream));
      Launch l(h, "k_sweep_count");
      if (parts)
        k_sweep_count<false, true><<<grid, kBlock, 0, h->stream>>>(
            h->recs, 0, h->cap, now, idle_ns, nullptr, nullptr, b.ctr,
            SweepParts<true>{b.mask, log2_parts});
      else
        k_sweep_count<false, false><<<grid, kBlock, 0, h->stream>>>(
            h->recs, 0, h->cap, now, idle_ns, nullptr, nullptr, b.ctr, SweepParts<false>{});
      return PHIP_OK;
    }, st);
  }
  u64 budget;
  if ((rc = datagram_args(h, "sweep", out, out_cap, offs, max_msgs, dev, &budget))) return rc;
  // four slots per datagram asked for, times the partitions per partition
  // asked for (4 * 2^32 * 2^20 < 2^64: the product cannot wrap); an empty
  // mask reads no slot and is done
  const u64 share = (nparts + std::max<u64>(m, 1) - 1) / std::max<u64>(m, 1);
  const SweepWindow w = sweep_open(h, cur, 4ull * max_msgs * share, none);
  u64 c[kSwWords] = {};
  u8* d_out = out;
  u64* d_offs = reinterpret_cast<u64*>(offs);
  if (w.ntiles) {
    u64* ctr;
    if ((rc = ensure(h, B_SWEEP, SweepBuf::words(mw, w.ntiles), &ctr))) return rc;
    const SweepBuf b(ctr, mw, w.ntiles);
    const SweepParts<true> sp{b.mask, log2_parts};
    if (parts)
      HIPCHK(h, hipMemcpyAsync(b.mask, part_mask, mw * sizeof(u64), hipMemcpyHostToDevice,
                               h->stream));
    {
      Launch l(h, "k_sweep_count");
      if (parts)
        k_sweep_count<true, true><<<w.ntiles, kBlock, 0, h->stream>>>(
            h->recs, w.s0, w.s_end, now, idle_ns, b.tile_cnt, b.tile_bytes, ctr, sp);
      else
        k_sweep_count<true, false><<<w.ntiles, kBlock, 0, h->stream>>>(
            h->recs, w.s0, w.s_end, now, idle_ns, b.tile_cnt, b.tile_bytes, ctr,
            SweepParts<false>{});
    }
    {
      Launch l(h, "k_sweep_scan");
      k_sweep_scan<<<1, kSweepBlock, 0, h->stream>>>(b.tile_cnt, b.tile_bytes, w.ntiles, ctr);
    }
    HIPCHK(h, hipGetLastError());
    if (!dev) {
      // staging sized by what the window holds, not by the caller's caps
      if ((rc = sweep_read(h, ctr, c)) ||
          (rc = ensure(h, B_EXPORT, (size_t)std::min<u64>(out_cap, c[kSwBytes]), &d_out)) ||
          (rc = ensure(h, B_OFFS, (size_t)std::min<u64>(max_msgs, c[kSwN]) + 1, &d_offs)))
        return rc;
    }
    {
      // (long names are bounded by the arena's size, not its cursor: reading
      // the cursor would cost a device-pointer call a second round trip)
      Launch l(h, "k_sweep_write");
      if (parts)
        k_sweep_write<true><<<w.ntiles, kSweepBlock, 0, h->stream>>>(
            h->recs, h->arena, h->arena_cap, w.s0, w.s_end, now, idle_ns, b.tile_cnt, b.tile_bytes,
            max_msgs, budget, d_out, d_offs, ctr, sp);
      else
        k_sweep_write<false><<<w.ntiles, kSweepBlock, 0, h->stream>>>(
            h->recs, h->arena, h->arena_cap, w.s0, w.s_end, now, idle_ns, b.tile_cnt, b.tile_bytes,
            max_msgs, budget, d_out, d_offs, ctr, SweepParts<false>{});
    }
    HIPCHK(h, hipGetLastError());
    if ((rc = sweep_read(h, ctr, c))) return rc;
  }
  if ((rc = sweep_close(h, w, c, "sweep", "datagrams", max_msgs, budget, 0, cur, st))) return rc;
  if (!w.ntiles) return datagrams_none(h, offs, dev, true);
  if (!dev) {
    if ((rc = datagrams_back(h, out, d_out, st->bytes, offs, d_offs, st->n))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return PHIP_OK;
}

int phip_export_sweep(phip_handle* h, phip_sweep_cursor* cur, int64_t now, int64_t idle_ns,
                      uint8_t* out, uint64_t out_cap, uint64_t* offs, uint32_t max_msgs,
                      phip_sweep_stats* st, uint32_t flags) {
  return export_sweep(h, cur, now, idle_ns, false, 0, nullptr, out, out_cap, offs, max_msgs, st,
                      flags);
}

int phip_export_sweep_parts(phip_handle* h, phip_sweep_cursor* cur, int64_t now, int64_t idle_ns,
                            uint32_t log2_parts, const uint64_t* part_mask, uint8_t* out,
                            uint64_t out_cap, uint64_t* offs, uint32_t max_msgs,
                            phip_sweep_stats* st, uint32_t flags) {
  return export_sweep(h, cur, now, idle_ns, true, log2_parts, part_mask, out, out_cap, offs,
                      max_msgs, st, flags);
}

// Throttled sweep (patrolhip.h "Throttled sweep"; kernels in phip_kernels.hpp
// "throttled sweep"): the sweep's window, tile arrays and scan, with the rule
// table -- rates derived here, once -- as a kernel argument.  Nothing of the
// handle changes but its scratch buffers.
int phip_export_throttled(phip_handle* h, phip_sweep_cursor* cur, const phip_throttle_rule* rules,
                          uint32_t n_rules, int64_t now, int64_t min_wait_ns,
                          const phip_throttled_out* out, phip_sweep_stats* st, uint32_t flags) {
  if (!h || !cur || !st || !rules) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (flags & ~(PHIP_DEVICE_PTRS | PHIP_SWEEP_COUNT))
    return set_err(h, PHIP_ERR_INVALID, "throttled: unknown flag bits 0x%x", flags);
  if (n_rules < 1 || n_rules > PHIP_THROTTLE_MAX_RULES)
    return set_err(h, PHIP_ERR_INVALID, "throttled: n_rules must be 1..%d", PHIP_THROTTLE_MAX_RULES);
  ThrottleRules R{};
  R.n = n_rules;
  for (u32 i = 0; i < n_rules; ++i) {
    if (rules[i].prefix_len > PHIP_THROTTLE_MAX_PREFIX)
      return set_err(h, PHIP_ERR_INVALID, "throttled: rule %u has a prefix over %d bytes", i,
                     PHIP_THROTTLE_MAX_PREFIX);
    R.r[i] = throttle_rule(rules[i]);
  }
  if (min_wait_ns < 0)
    return set_err(h, PHIP_ERR_INVALID, "throttled: min_wait_ns must not be negative");
  i64 later;
  if (__builtin_add_overflow((i64)now, (i64)min_wait_ns, &later)) later = INT64_MAX;
  const bool dev = flags & PHIP_DEVICE_PTRS;
  int rc;
  if (flags & PHIP_SWEEP_COUNT) {
    if (out) return set_err(h, PHIP_ERR_INVALID, "throttled: count mode takes no output");
    return sweep_count_mode(h, 0, [&](unsigned grid, const SweepBuf& b) -> int {
      Launch l(h, "k_throttle_count");
      k_throttle_count<false><<<grid, kBlock, 0, h->stream>>>(h->recs, 0, h->cap, now, later, nullptr,
                                                              nullptr, b.ctr, R);
      return PHIP_OK;
    }, st);
  }
  if (!out || !out->names || !out->offs)
    return set_err(h, PHIP_ERR_INVALID, "throttled: out, its names and its offs are required");
  const phip_throttled_out o = *out;
  if (!o.max_entries) return set_err(h, PHIP_ERR_INVALID, "throttled: max_entries must be positive");
  if (o.names_cap < PHIP_MAX_NAME_LEN)
    return set_err(h, PHIP_ERR_INVALID, "throttled: names_cap below one name (%d bytes)",
                   PHIP_MAX_NAME_LEN);
  const u64 budget = o.names_cap;
  const SweepWindow w = sweep_open(h, cur, 4ull * o.max_entries);
  const u32 nwin = (u32)(w.s_end - w.s0);
  u64 c[kSwWords] = {};
  ThrottledOut d{o.names, reinterpret_cast<u64*>(o.offs), reinterpret_cast<i64*>(o.retry_at),
                 reinterpret_cast<u64*>(o.remaining), o.rule};
  if (w.ntiles) {
    u64* ctr;
    if ((rc = ensure(h, B_SWEEP, SweepBuf::words(0, w.ntiles), &ctr))) return rc;
    const SweepBuf b(ctr, 0, w.ntiles);
    {
      Launch l(h, "k_throttle_count");
      k_throttle_count<true><<<w.ntiles, kBlock, 0, h->stream>>>(h->recs, w.s0, w.s_end, now, later,
                                                                 b.tile_cnt, b.tile_bytes, ctr, R);
    }
    {
      Launch l(h, "k_sweep_scan");
      k_sweep_scan<<<1, kSweepBlock, 0, h->stream>>>(b.tile_cnt, b.tile_bytes, w.ntiles, ctr);
    }
    HIPCHK(h, hipGetLastError());
    if (!dev) {
      // staging sized by what the window holds, not by the caller's caps
      if ((rc = sweep_read(h, ctr, c))) return rc;
      const size_t ne = (size_t)std::min<u64>(o.max_entries, c[kSwN]);
      if ((rc = ensure(h, B_EXPORT, (size_t)std::min<u64>(o.names_cap, c[kSwBytes]), &d.names)) ||
          (rc = ensure(h, B_OFFS, ne + 1, &d.offs)) ||
          (rc = out_buf(h, B_PEEKAT, reinterpret_cast<i64*>(o.retry_at), ne, false, &d.retry_at)) ||
          (rc = out_buf(h, B_REM, reinterpret_cast<u64*>(o.remaining), ne, false, &d.remaining)) ||
          (rc = out_buf(h, B_STATUS, o.rule, ne, false, &d.rule)))
        return rc;
    }
    {
      // (long names are bounded by the arena's size, as in export_sweep; the
      // kernel finds the tile arrays behind ctr by SweepBuf)
      Launch l(h, "k_throttle_write");
      k_throttle_write<<<w.ntiles, kSweepBlock, 0, h->stream>>>(
          h->recs + w.s0, nwin, h->arena, h->arena_cap, now, later, o.max_entries, budget, d, ctr, R);
    }
    // the retry search, one lane per written entry; their number is on the
    // device (the counter word), the grid goes by what the host knows of it:
    // the window's total after the scan, or (device pointers) the window
    const u64 most = std::min<u64>(o.max_entries, dev ? nwin : c[kSwN]);
    if (d.retry_at && most) {
      Launch l(h, "k_throttle_retry");
      const unsigned grid = std::min<unsigned>(grid_for(most), 16u * (unsigned)h->ncu);
      k_throttle_retry<<<grid, kBlock, 0, h->stream>>>(h->recs + w.s0, nwin, now, d.retry_at, ctr, R);
    }
    HIPCHK(h, hipGetLastError());
    if ((rc = sweep_read(h, ctr, c))) return rc;
  }
  // (k_throttle_write counts slots from the window's first)
  if ((rc = sweep_close(h, w, c, "throttled sweep", "entries", o.max_entries, budget, w.s0, cur, st)))
    return rc;
  if (!w.ntiles) return datagrams_none(h, o.offs, dev, true);
  if (!dev) {
    if ((rc = datagrams_back(h, o.names, d.names, st->bytes, o.offs, d.offs, st->n)) ||
        (rc = copy_back(h, reinterpret_cast<i64*>(o.retry_at), d.retry_at, st->n, false)) ||
        (rc = copy_back(h, reinterpret_cast<u64*>(o.remaining), d.remaining, st->n, false)) ||
        (rc = copy_back(h, o.rule, d.rule, st->n, false)))
      return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return PHIP_OK;
}

// Top talkers (patrolhip.h "Top talkers"; kernels in phip_kernels.hpp "top
// talkers").  Every launch of the longest case is enqueued at once -- six
// digit passes, the tie count, its scan, the collect, the sort -- and the
// counter words on the device tell each kernel whether its stage is still
// wanted, so there is no round trip between the passes: the one read-back is
// at the end.  Scratch: the sweep's tile arrays (one count per tile, for the
// ties) and the top buffer of O(bins + k) words; nothing per slot.  A
// host-pointer call stages its columns by the caller's caps (at most k entries
// and k names) and copies back what was written.
int phip_export_top(phip_handle* h, const phip_top_query* q, const phip_top_out* out,
                    phip_top_stats* st, uint32_t flags) {
  if (!h || !q || !st) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (flags & ~(PHIP_DEVICE_PTRS | PHIP_SWEEP_COUNT | PHIP_TOP_MARK))
    return set_err(h, PHIP_ERR_INVALID, "top: unknown flag bits 0x%x", flags);
  if (q->k < 1 || q->k > PHIP_TOP_MAX)
    return set_err(h, PHIP_ERR_INVALID, "top: k must be 1..%d", PHIP_TOP_MAX);
  if (q->prefix_len > PHIP_THROTTLE_MAX_PREFIX)
    return set_err(h, PHIP_ERR_INVALID, "top: a prefix over %d bytes", PHIP_THROTTLE_MAX_PREFIX);
  if (q->metric > PHIP_TOP_SINCE_MARK)
    return set_err(h, PHIP_ERR_INVALID, "top: metric %u is not known", q->metric);
  const bool since = q->metric == PHIP_TOP_SINCE_MARK, mark = flags & PHIP_TOP_MARK;
  if ((since || mark) && !h->usage)
    return set_err(h, PHIP_ERR_INVALID, "top: the handle was opened without PHIP_CFG_TRACK_USAGE");
  if (mark && (flags & PHIP_SWEEP_COUNT))
    return set_err(h, PHIP_ERR_INVALID, "top: count mode does not mark");
  if (q->idle_ns < 0) return set_err(h, PHIP_ERR_INVALID, "top: idle_ns must not be negative");
  TopQuery Q{};
  {
    phip_throttle_rule r{};
    memcpy(r.prefix, q->prefix, sizeof r.prefix);
    r.prefix_len = q->prefix_len;
    Q.R.n = 1;
    Q.R.r[0] = throttle_rule(r);
    Q.now = q->now;
    Q.idle_ns = q->idle_ns;
  }
  const bool dev = flags & PHIP_DEVICE_PTRS;
  // the table-reading kernels by metric: launch(the baseline, or its empty form)
  auto by_metric = [&](auto launch) {
    if (since)
      launch(TopBase<true>{h->base});
    else
      launch(TopBase<false>{});
  };
  int rc;
  if (flags & PHIP_SWEEP_COUNT) {
    if (out) return set_err(h, PHIP_ERR_INVALID, "top: count mode takes no output");
    phip_sweep_stats cs{};
    if ((rc = sweep_count_mode(h, 0, [&](unsigned grid, const SweepBuf& b) -> int {
          Launch l(h, "k_top_count");
          by_metric([&](auto tb) {
            k_top_count<<<grid, kBlock, 0, h->stream>>>(h->recs, h->cap, Q, b.ctr, tb);
          });
          return PHIP_OK;
        }, &cs)))
      return rc;
    phip_top_stats s{};
    s.population = cs.n;
    s.passes = 1;
    *st = s;
    return PHIP_OK;
  }
  if (!out || !out->names || !out->offs)
    return set_err(h, PHIP_ERR_INVALID, "top: out, its names and its offs are required");
  const phip_top_out o = *out;
  if (o.names_cap < PHIP_MAX_NAME_LEN)
    return set_err(h, PHIP_ERR_INVALID, "top: names_cap below one name (%d bytes)",
                   PHIP_MAX_NAME_LEN);
  const u32 k = q->k;
  const u32 ntiles = (u32)((h->cap + kSweepTile - 1) / kSweepTile);
  u64 *sw, *tb;
  if ((rc = ensure(h, B_SWEEP, SweepBuf::words(0, ntiles), &sw)) ||
      (rc = ensure(h, B_TOP, TopBuf::words(), &tb)))
    return rc;
  const SweepBuf b(sw, 0, ntiles);
  const TopBuf t(tb);
  TopOut d{o.names, reinterpret_cast<u64*>(o.offs), reinterpret_cast<u64*>(o.taken), o.state};
  if (!dev) {
    const size_t nb = (size_t)std::min<u64>(o.names_cap, (u64)k * PHIP_MAX_NAME_LEN);
    if ((rc = ensure(h, B_EXPORT, nb, &d.names)) || (rc = ensure(h, B_OFFS, (size_t)k + 1, &d.offs)) ||
        (rc = out_buf(h, B_REM, reinterpret_cast<u64*>(o.taken), k, false, &d.taken)) ||
        (rc = out_buf(h, B_PEEKST, o.state, k, false, &d.state)))
      return rc;
  }
  HIPCHK(h, hipMemsetAsync(t.ctr, 0, TopBuf::clear_bytes(), h->stream));
  const unsigned grid = std::min<unsigned>(grid_for(h->cap), 8u * (unsigned)h->ncu);
  for (u32 done = 0; done < 64; done += kTopBits) {
    {
      Launch l(h, "k_top_hist");
      by_metric([&](auto tb) {
        k_top_hist<<<grid, kBlock, 0, h->stream>>>(h->recs, h->cap, Q, t.ctr, t.hist, tb);
      });
    }
    {
      Launch l(h, "k_top_pick");
      k_top_pick<<<1, kTopPickBlock, 0, h->stream>>>(t.ctr, t.hist, k);
    }
  }
  {
    Launch l(h, "k_top_ties");
    by_metric([&](auto tb) {
      k_top_ties<<<ntiles, kBlock, 0, h->stream>>>(h->recs, h->cap, Q, t.ctr, b.tile_cnt,
                                                   b.tile_bytes, tb);
    });
  }
  {
    Launch l(h, "k_top_scan");
    k_top_scan<<<1, kSweepBlock, 0, h->stream>>>(t.ctr, b.tile_cnt, b.tile_bytes, ntiles);
  }
  {
    Launch l(h, "k_top_collect");
    by_metric([&](auto tb) {
      k_top_collect<<<ntiles, kSweepBlock, 0, h->stream>>>(h->recs, h->cap, Q, t.ctr, b.tile_cnt,
                                                           t.key, t.slot, tb);
    });
  }
  {
    // (long names are bounded by the arena's size, as in export_sweep)
    Launch l(h, "k_top_emit");
    k_top_emit<<<1, kTopEmitBlock, 0, h->stream>>>(h->recs, h->arena, h->arena_cap, t.ctr, t.key,
                                                   t.slot, d, o.names_cap,
                                                   since ? h->base : nullptr);
  }
  if (mark) {
    // PHIP_TOP_MARK: the new baseline behind the list, under this call's lock
    // (its two counts land in spare words of the top buffer and are not read)
    Launch l(h, "k_usage_mark");
    k_usage_mark<<<grid, kBlock, 0, h->stream>>>(h->recs, h->cap, h->base, t.ctr + kTpMark);
  }
  HIPCHK(h, hipGetLastError());
  u64 c[kTpWords];
  HIPCHK(h, hipMemcpyAsync(c, t.ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (c[kTpErr] || c[kTpMode] == kTopRefine || c[kTpN] > k || c[kTpBytes] > o.names_cap ||
      (c[kTpMode] != kTopEmpty && c[kTpCnt] < c[kTpK]))
    return set_err(h, PHIP_ERR_INVALID,
                   "internal: top wrote %llu entries, %llu bytes of %llu candidates (mode %llu, flag %llu)",
                   (unsigned long long)c[kTpN], (unsigned long long)c[kTpBytes],
                   (unsigned long long)c[kTpCnt], (unsigned long long)c[kTpMode],
                   (unsigned long long)c[kTpErr]);
  phip_top_stats s{};
  s.n = c[kTpN];
  s.bytes = c[kTpBytes];
  s.population = c[kTpPop];
  s.passes = (uint32_t)c[kTpPasses];
  s.truncated = (uint32_t)c[kTpTrunc];
  *st = s;
  if (!dev) {
    if ((rc = datagrams_back(h, o.names, d.names, s.bytes, o.offs, d.offs, s.n)) ||
        (rc = copy_back(h, reinterpret_cast<u64*>(o.taken), d.taken, s.n, false)) ||
        (rc = copy_back(h, o.state, d.state, s.n, false)))
      return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return PHIP_OK;
}

// The usage mark (patrolhip.h "Windowed top talkers"): one pass of k_usage_mark
// on count mode's grid, its two sums read back.  Nothing but the baseline
// column is written.
int phip_usage_mark(phip_handle* h, phip_usage_stats* st, uint32_t flags) {
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (flags) return set_err(h, PHIP_ERR_INVALID, "usage mark: unknown flag bits 0x%x", flags);
  if (!h->usage)
    return set_err(h, PHIP_ERR_INVALID, "usage mark: the handle was opened without PHIP_CFG_TRACK_USAGE");
  phip_sweep_stats cs{};
  if (int rc = sweep_count_mode(h, 0, [&](unsigned grid, const SweepBuf& b) -> int {
        Launch l(h, "k_usage_mark");
        k_usage_mark<<<grid, kBlock, 0, h->stream>>>(h->recs, h->cap, h->base, b.ctr);
        return PHIP_OK;
      }, &cs))
    return rc;
  if (st) {
    st->buckets = cs.n;
    st->active = cs.bytes;
  }
  return PHIP_OK;
}

// Change-set export (patrolhip.h "Change set"; kernels in phip_kernels.hpp
// "change set"): count per tile of the bit sets, the egress' scan, write.  The
// totals of a full drain stand in the egress counter words after the scan; the
// write cuts them to what fitted.  As in the sweep, a device-pointer call reads
// the counters back once, at its end, and a host-pointer call also after the
// scan, to size its staging buffers by what is pending instead of by the caps.
int phip_export_changed(phip_handle* h, uint8_t* out, uint64_t out_cap, uint64_t* offs,
                        uint32_t max_msgs, phip_changes_stats* st, uint32_t flags) {
  if (!h || !st) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (!h->track)
    return set_err(h, PHIP_ERR_INVALID, "changes: the handle was opened without PHIP_CFG_TRACK_CHANGES");
  if (flags & ~(PHIP_DEVICE_PTRS | PHIP_SWEEP_COUNT))
    return set_err(h, PHIP_ERR_INVALID, "changes: unknown flag bits 0x%x", flags);
  const bool dev = flags & PHIP_DEVICE_PTRS, count = flags & PHIP_SWEEP_COUNT;
  int rc;
  u64 budget = 0;
  if (count) {
    if (out) return set_err(h, PHIP_ERR_INVALID, "changes: count mode takes no output buffer");
  } else if ((rc = datagram_args(h, "changes", out, out_cap, offs, max_msgs, dev, &budget))) {
    return rc;
  }
  const u64 nwords = mark_words(h->cap);
  const u32 ntiles = (u32)((h->cap + kSweepTile - 1) / kSweepTile);
  // one buffer: the tiles' byte sums, then their counts (both sections each)
  u64* tile_bytes;
  if ((rc = ensure(h, B_EGTILE, 3 * (size_t)ntiles, &tile_bytes))) return rc;
  u32* tile_cnt = (u32*)(tile_bytes + 2 * (size_t)ntiles);
  HIPCHK(h, hipMemsetAsync(h->ctr + kCtrChgMarks, 0, 2 * sizeof(u32), h->stream));
  {
    Launch l(h, "k_changed_count");
    k_changed_count<<<ntiles, kBlock, 0, h->stream>>>(h->recs, h->cap, nwords, h->marks, ntiles,
                                                      tile_cnt, tile_bytes, h->ctr);
  }
  {
    Launch l(h, "k_egress_scan");
    k_egress_scan<<<1, kSweepBlock, 0, h->stream>>>(tile_cnt, tile_bytes, ntiles, h->ctr);
  }
  HIPCHK(h, hipGetLastError());
  const u32* c = h->ctr_host;
  u64 bytes;
  phip_changes_stats s{};
  if (count) {
    if ((rc = read_ctr(h))) return rc;
    std::memcpy(&bytes, c + kCtrEgBytes, sizeof bytes);
    s.n = c[kCtrEgN];
    s.bytes = bytes;
    s.n_incast = c[kCtrEgIncast];
    s.pending = c[kCtrChgMarks];
    s.done = s.pending == 0;
    *st = s;
    return PHIP_OK;
  }
  u8* d_out = out;
  u64* d_offs = reinterpret_cast<u64*>(offs);
  if (!dev) {
    if ((rc = read_ctr(h))) return rc;
    std::memcpy(&bytes, c + kCtrEgBytes, sizeof bytes);
    if ((rc = ensure(h, B_EGOUT, (size_t)std::min<u64>(out_cap, bytes), &d_out)) ||
        (rc = ensure(h, B_EGOFFS, (size_t)std::min<u64>(max_msgs, c[kCtrEgN]) + 1, &d_offs)))
      return rc;
  }
  {
    // (long names are bounded by the arena's size, as in the sweep)
    Launch l(h, "k_changed_write");
    k_changed_write<<<ntiles, kSweepBlock, 0, h->stream>>>(
        h->recs, h->cap, nwords, h->arena, h->arena_cap, h->marks, ntiles, tile_cnt, tile_bytes,
        max_msgs, budget, d_out, d_offs, h->ctr);
  }
  HIPCHK(h, hipGetLastError());
  if ((rc = read_ctr(h))) return rc;
  std::memcpy(&bytes, c + kCtrEgBytes, sizeof bytes);
  if (c[kCtrEgErr] || c[kCtrEgN] > max_msgs || bytes > budget || c[kCtrChgCleared] > c[kCtrChgMarks])
    return set_err(h, PHIP_ERR_INVALID,
                   "internal: change set wrote %u datagrams, %llu bytes, cleared %u of %u (flag %u)",
                   c[kCtrEgN], (unsigned long long)bytes, c[kCtrChgCleared], c[kCtrChgMarks],
                   c[kCtrEgErr]);
  s.n = c[kCtrEgN];
  s.bytes = bytes;
  // (kCtrEgIncast: every pending request; the written ones are a prefix of the output)
  s.n_incast = std::min<u32>(c[kCtrEgIncast], c[kCtrEgN]);
  s.pending = c[kCtrChgMarks] - c[kCtrChgCleared];
  s.done = s.pending == 0;
  if (!dev) {
    if ((rc = datagrams_back(h, out, d_out, s.bytes, offs, d_offs, s.n))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  *st = s;
  return PHIP_OK;
}

// Table digest (patrolhip.h "Partition digests"; kernels in phip_kernels.hpp
// "table digest").  Up to 2^12 partitions: k_digest sums in LDS and stores one
// table per workgroup, k_digest_reduce adds them up -- nothing to clear.  From
// 2^13 on: k_digest adds into the cleared result with global atomics, and
// k_digest_reduce only sums the workgroups' record and byte counts.  The
// result is built in the caller's device buffer, or in the handle's and copied.
int phip_table_digest(phip_handle* h, uint32_t log2_parts, phip_digest_part* out,
                      phip_digest_stats* st, uint32_t flags) {
  if (!h) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;   // (finishes a queued PHIP_RECV_ASYNC batch)
  if (flags & ~PHIP_DEVICE_PTRS)
    return set_err(h, PHIP_ERR_INVALID, "digest: unknown flag bits 0x%x", flags);
  if (!out || log2_parts > PHIP_DIGEST_MAX_LOG2_PARTS)
    return set_err(h, PHIP_ERR_INVALID, "digest: out and log2_parts <= %d are required",
                   PHIP_DIGEST_MAX_LOG2_PARTS);
  const bool dev = flags & PHIP_DEVICE_PTRS;
  if (dev && (reinterpret_cast<uintptr_t>(out) & 7))
    return set_err(h, PHIP_ERR_INVALID, "digest: a device buffer is 8-byte aligned");
  const u32 k = log2_parts;
  const size_t nparts = (size_t)1 << k;
  const bool lds = k <= kDigestLdsLog2;
  // two workgroups of 16 waves a compute unit (48 KiB of LDS each)
  const unsigned grid =
      std::min<unsigned>(grid_for(h->cap, 2 * kDigestBlock), 2u * (unsigned)h->ncu);
  int rc;
  // one buffer: the stats, the workgroups' counts, then their tables
  u64* stats;
  if ((rc = ensure(h, B_DIGEST, kDgWords + (size_t)grid * kDgWords + (lds ? 2 * grid * nparts : 0),
                   &stats)))
    return rc;
  u64* pstat = stats + kDgWords;
  u64* partial = pstat + (size_t)grid * kDgWords;
  phip_digest_part* res = out;
  if (!dev && (rc = ensure(h, B_DIGOUT, nparts, &res))) return rc;
  if (!lds) HIPCHK(h, hipMemsetAsync(res, 0, nparts * sizeof(phip_digest_part), h->stream));
  {
    Launch l(h, "k_digest");
    if (lds)
      k_digest<true><<<grid, kDigestBlock, 0, h->stream>>>(h->recs, h->cap, k, partial, nullptr,
                                                           pstat);
    else
      k_digest<false><<<grid, kDigestBlock, 0, h->stream>>>(h->recs, h->cap, k, nullptr, res,
                                                            pstat);
  }
  {
    Launch l(h, "k_digest_reduce");
    const unsigned rgrid = lds ? (unsigned)((nparts + 63) / 64) + 1 : 1;
    k_digest_reduce<<<rgrid, kDigestBlock, 0, h->stream>>>(partial, grid, k, res, pstat, stats);
  }
  HIPCHK(h, hipGetLastError());
  u64 sw[kDgWords] = {};
  HIPCHK(h, hipMemcpyAsync(sw, stats, sizeof sw, hipMemcpyDeviceToHost, h->stream));
  if (!dev)
    HIPCHK(h, hipMemcpyAsync(out, res, nparts * sizeof(phip_digest_part), hipMemcpyDeviceToHost,
                             h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (st) {
    st->records = sw[kDgRecords];
    st->bytes = sw[kDgBytes];
    st->slots_scanned = h->cap;
  }
  return PHIP_OK;
}

int phip_table_stats(phip_handle* h, uint64_t* out, int max) {
  if (!h || !out) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = begin_call(h)) return rc0;
  u64* d;
  int rc;
  if ((rc = ensure(h, B_TSTATS, 2, &d))) return rc;
  HIPCHK(h, hipMemsetAsync(d, 0, 2 * sizeof(u64), h->stream));
  {
    Launch l(h, "k_table_stats");
    k_table_stats<<<grid_for(h->cap), kBlock, 0, h->stream>>>(table(h), h->cap, d);
  }
  HIPCHK(h, hipGetLastError());
  u64 r[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(r, d, sizeof r, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint64_t v[4] = {h->n_buckets, h->cap, r[0], r[1]};
  return copy_words(v, out, max);
}

int phip_last_stats(phip_handle* h, uint64_t* out, int max) {
  if (!h || !out) return 0;
  std::lock_guard<std::mutex> g(h->mu);
  // a queued PHIP_RECV_ASYNC batch is finished first, so the stats are its
  // own (its error, if any, is kept for the next call that returns one)
  if (h->pend.active && !h->deferred_rc) h->deferred_rc = begin_call(h);
  const phip_handle::LastStats& s = h->stats;
  const uint64_t v[9] = {s.hot_entries, s.hot_hits,  s.misses,   h->grows,  s.ordered,
                         s.log_count,   s.log_over,  s.hot_age,  s.gate_shut};   // (patrolhip.h's order)
  return copy_words(v, out, max);
}

int phip_undo_log_layout(uint32_t n, uint32_t compute_units, uint64_t* out, int max) {
  if (!out || !compute_units) return 0;
  const UndoLayout l = undo_layout(n, compute_units);
  const uint64_t v[4] = {l.grid, l.waves, l.cap, l.halves * sizeof(u64x2)};
  return copy_words(v, out, max);
}

}  // extern "C"

namespace phip_host {
void* handle_stream(phip_handle* h) { return h ? (void*)h->stream : nullptr; }
// (route_dir / route_pack use the handle's counters on the group's stream: a
// batch PHIP_RECV_ASYNC queued on the handle is finished first, so its
// kernels never race them)
int finish_queued(phip_handle* h) {
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->pend.active) return PHIP_OK;
  const int rc = finish_pending(h);
  return rc ? after_error(h, rc) : PHIP_OK;
}
int route_dir(phip_handle* h, void* stream, const phip_msgs* m, uint32_t world, const void** dir) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return route_dir_on(h, (hipStream_t)stream, *m, world, dir);
}
int route_pack(phip_handle* h, void* stream, const phip_msgs* m, uint32_t world, const void* dir,
               uint8_t* names, uint32_t* lens, uint64_t* a, uint64_t* t, int64_t* e,
               uint64_t* counts, uint64_t* nbytes, uint32_t* src) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return route_pack_on(h, (hipStream_t)stream, *m, world, dir, names, lens, a, t, e, counts, nbytes,
                       src);
}
// The chunk's zero-state count (k_zero_count) on `stream`, added into the high
// halves of out[0 .. nout).
template <class Fields>
static int count_zero_on(phip_handle* h, hipStream_t st, const Fields& f, u32 n, u32 nout, uint64_t* out) {
  if (!n) return PHIP_OK;
  const u32 grid = (u32)std::min<u64>(grid_for(n), (u64)h->ncu * 8);
  Launch l(h, "k_zero_count", st);
  k_zero_count<Fields><<<grid, kBlock, 0, st>>>(f, n, nout, (unsigned long long*)out);
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}
int count_zero(phip_handle* h, void* stream, const phip_msgs* m, uint32_t nout, uint64_t* out) {
  std::lock_guard<std::mutex> g(h->mu);
  return count_zero_on(h, (hipStream_t)stream, SoaFields{m->added, m->taken, m->elapsed}, m->n, nout, out);
}
int count_zero_wire(phip_handle* h, void* stream, const phip_wire* w, uint32_t nout, uint64_t* out) {
  std::lock_guard<std::mutex> g(h->mu);
  return count_zero_on(h, (hipStream_t)stream, WireFields{Datagrams{w->bytes, w->offs}}, w->n, nout, out);
}
int route_pack_ops(phip_handle* h, void* stream, const phip_ops* ops, uint32_t world,
                   uint8_t* names, uint32_t* lens, uint8_t* kind, int64_t* now, uint64_t* x0,
                   uint64_t* x1, uint64_t* x2, uint32_t* src, uint64_t* counts, uint64_t* nbytes) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return route_pack_ops_on(h, (hipStream_t)stream, *ops, world, names, lens, kind, now, x0, x1, x2,
                           src, counts, nbytes);
}
int route_pack_queries(phip_handle* h, void* stream, const phip_ops* q, uint32_t world,
                       uint8_t* names, uint32_t* lens, int64_t* now, uint64_t* x0, uint64_t* x1,
                       uint64_t* x2, uint32_t* src, uint64_t* counts, uint64_t* nbytes) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return route_pack_ops_on<true>(h, (hipStream_t)stream, *q, world, names, lens, nullptr, now, x0,
                                 x1, x2, src, counts, nbytes);
}
int peek_results_scatter(phip_handle* h, void* stream, const uint32_t* src, uint32_t n,
                         const uint8_t* status, const uint64_t* remaining, const uint64_t* have,
                         const int64_t* retry_at, const phip_state* state,
                         const phip_peek_results* out) {
  if (!n || !out) return PHIP_OK;
  const PeekOut po{out->status, out->remaining, out->have, out->retry_at, state ? out->state : nullptr};
  if (!po.status && !po.remaining && !po.have && !po.retry_at && !po.state) return PHIP_OK;
  k_peek_results_scatter<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(
      src, n, status, remaining, have, retry_at, state, po);
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}
int results_scatter(phip_handle* h, void* stream, const uint32_t* src, uint32_t n,
                    const uint8_t* status, const uint64_t* remaining, const uint64_t* have,
                    const phip_state* reply, const phip_results* out) {
  if (!n || !out) return PHIP_OK;
  const OutView ow{out->status, out->remaining, out->have, out->reply};
  if (!ow.status && !ow.remaining && !ow.have && !ow.reply) return PHIP_OK;
  k_route_results_scatter<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(src, n, status, remaining,
                                                                           have, reply, ow);
  HIPCHK(h, hipGetLastError());
  return PHIP_OK;
}
int check_offsets(phip_handle* h, void* stream, const uint8_t* names, const uint32_t* name_offs,
                  uint32_t names_len, uint32_t n, uint32_t* first_bad) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return check_offsets_on(h, (hipStream_t)stream, names, name_offs, names_len, n, first_bad);
}
int wire_scan(phip_handle* h, void* stream, const phip_wire* w, uint32_t* stop, uint32_t* first_bad) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return wire_scan_on(h, (hipStream_t)stream, w->bytes, w->offs, w->bytes_len, w->n, stop, first_bad);
}
int route_dir_wire(phip_handle* h, void* stream, const phip_wire* w, uint32_t world, const void** dir) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return route_dir_src(h, (hipStream_t)stream, Datagrams{w->bytes, w->offs}, w->n, world, dir);
}
int route_pack_wire(phip_handle* h, void* stream, const phip_wire* w, uint32_t world, const void* dir,
                    uint8_t* names, uint32_t* lens, uint64_t* a, uint64_t* t, int64_t* e,
                    uint64_t* counts, uint64_t* nbytes, uint32_t* src) {
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc0 = finish_queued(h)) return rc0;
  return route_pack_src(h, (hipStream_t)stream, Datagrams{w->bytes, w->offs}, nullptr, nullptr,
                        nullptr, w->n, world, dir, names, lens, a, t, e, counts, nbytes, src);
}
int ring_slot(phip_ring* r, uint32_t slot, const phip_handle* h, phip_wire* w, void** copied) {
  if (!r || r->h != h || slot >= r->slots.size()) return PHIP_ERR_INVALID;
  std::lock_guard<std::mutex> g(r->mu);
  const phip_ring::Slot& s = r->slots[slot];
  if (s.state != phip_ring::kSubmitted || slot != r->next_receive) return PHIP_ERR_BUSY;
  *w = phip_wire{s.n, 0, s.dbytes, s.doffs, 0};
  *copied = (void*)s.copied;
  return PHIP_OK;
}
void ring_release(phip_ring* r, uint32_t slot) {
  std::lock_guard<std::mutex> g(r->mu);
  r->slots[slot].state = phip_ring::kFree;
  r->next_receive = (r->next_receive + 1) % (u32)r->slots.size();
}
const char* last_error(phip_handle* h) { return h ? h->err.c_str() : ""; }
int handle_device(const phip_handle* h) { return h ? h->device : -1; }
}  // namespace phip_host
