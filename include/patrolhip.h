/*
 * libpatrolhip — MI355X (gfx950) bucket-state engine for Patrol.
 *
 * A C ABI (plain pointers and sizes, no C++ types, no exceptions) that a Go
 * maintainer binds with cgo to replace Patrol's in-memory bucket map and its
 * two hot loops (INTEGRATION.md shows the binding):
 *
 *   Patrol seam (reference file:line)                 replaced by
 *   ------------------------------------------------  ------------------------------
 *   Repo interface              repo.go:15-18          phip_open / phip_get / batched calls
 *   NewLocalRepo(clock, bs...)  repo.go:179-185        phip_open + phip_seed
 *   LocalRepo.GetBucket         repo.go:189-211        device table find-or-create (inside every batch)
 *   LocalRepo.UpsertBucket      repo.go:215-235        phip_upsert_soa
 *   ReplicatedRepo.Receive loop repo.go:54-92,108-120  phip_receive_datagrams / phip_receive_soa
 *   Bucket.UnmarshalBinary      bucket.go:71-91        device decode inside phip_receive_datagrams
 *   Bucket.MarshalBinary        bucket.go:51-68        phip_marshal (host; unicast/broadcast egress)
 *   Bucket.Merge                bucket.go:240-263      device merge inside receive/upsert/apply
 *   Bucket.Take                 bucket.go:186-225      phip_take / phip_apply_mixed
 *   Bucket.IsZero               bucket.go:165-170      receive status (merge vs incast)
 *   ParseRate                   bucket.go:102-123      phip_parse_rate (host)
 *   API.takeBucket              api.go:51-86           phip_api_take (host handler logic over phip_take)
 *
 * Semantics are the Go reference's, op for op, in batch index order ("seq"):
 * a batch gives exactly the results of running the Go code on its elements
 * one after another (DESIGN.md §3 explains how the parallel kernels keep that
 * guarantee).  Buckets are identified by their full name (the FNV-1a hash is
 * only the table's probe key; names are always compared).
 *
 * Conventions
 *  - Return 0 (PHIP_OK) or a negative phip_err; never abort.  Details in
 *    phip_last_error().
 *  - Input buffers are caller-owned and only read during the call; output
 *    buffers are caller-owned.  Host pointers are staged into the library's
 *    own device buffers.  With PHIP_DEVICE_PTRS every pointer of that call
 *    (inputs and outputs) is device memory of the handle's GPU; the call then
 *    runs without host copies (the form bench.py times).
 *  - Times are int64 nanoseconds since the Unix epoch (the `clock()` reading
 *    Patrol passes around); durations are int64 ns (time.Duration).
 *  - float64 values cross the ABI as IEEE-754 bit patterns (uint64) so NaN
 *    payloads and -0.0 survive bit-exactly.
 *  - One handle per GPU; calls on a handle are serialised by an internal
 *    mutex and every entry point sets its device (cgo goroutines migrate
 *    between OS threads).
 */
#ifndef PATROLHIP_H
#define PATROLHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHIP_ABI_VERSION 3

/* bucket.go:36-44 */
#define PHIP_BUCKET_FIXED_SIZE 25
#define PHIP_BUCKET_PACKET_SIZE 256
/* Names are 0..PHIP_MAX_NAME_LEN bytes (bucket.go:44-48).  Host batches are
 * checked (PHIP_ERR_NAME_TOO_LARGE); a batch passed by device pointers is
 * not read on the host, so its producer guarantees the bound.  (A datagram
 * carries its name length in one byte: phip_receive_datagrams takes names
 * of up to 255 bytes, as UnmarshalBinary does, bucket.go:72-91.) */
#define PHIP_MAX_NAME_LEN 231

typedef struct phip_handle phip_handle;

typedef enum phip_err {
  PHIP_OK = 0,
  PHIP_ERR_INVALID = -1,        /* bad argument */
  PHIP_ERR_HIP = -2,            /* HIP runtime error */
  PHIP_ERR_FULL = -3,           /* table load factor limit reached */
  PHIP_ERR_ARENA = -4,          /* long-name arena exhausted */
  PHIP_ERR_SHORT_BUFFER = -5,   /* io.ErrShortBuffer from a datagram (bucket.go:72,84) */
  PHIP_ERR_NAME_TOO_LARGE = -6, /* ErrNameTooLarge (bucket.go:48) */
  PHIP_ERR_NO_DEVICE = -7,
  PHIP_ERR_IO = -8,             /* socket error (phip_udp_*; errno holds the cause) */
  PHIP_ERR_BUSY = -9,           /* ring slot not available (phip_ring_*) */
  PHIP_ERR_RCCL = -10           /* RCCL call failed (phip_group_*) */
} phip_err;

/* Per-op status codes (one uint8 per op). */
enum {
  PHIP_ST_MERGED = 1,          /* non-zero remote merged: repo.go:78-79                 */
  PHIP_ST_INCAST_REPLY = 2,    /* zero remote, existed && !local.IsZero(): repo.go:86-90 */
  PHIP_ST_INCAST_NOREPLY = 3,  /* zero remote otherwise                                  */
  PHIP_ST_SHORT = 4,           /* datagram failed UnmarshalBinary: Receive returns      */
  PHIP_ST_NOT_PROCESSED = 5,   /* after a PHIP_ST_SHORT (the Go loop has exited)        */
  PHIP_ST_TAKE_OK = 6,         /* Take returned ok=true                                 */
  PHIP_ST_TAKE_DENIED = 7,     /* Take returned ok=false (HTTP 429)                     */
  PHIP_ST_UPSERT_INSERTED = 8, /* UpsertBucket inserted the state as-is (repo.go:225-230) */
  PHIP_ST_ABSENT = 0x40,       /* flag (phip_peek only): the bucket does not exist      */
  PHIP_ST_CREATED = 0x80       /* flag: this op's GetBucket created the bucket          */
};

/* Op kinds for phip_apply_mixed. */
enum {
  PHIP_OP_TAKE = 0,     /* GetBucket + Take(now, Rate{freq, per}, count) (api.go:67-74)   */
  PHIP_OP_RECEIVE = 1,  /* received replica state (repo.go:78-90)                         */
  PHIP_OP_UPSERT = 2    /* LocalRepo.UpsertBucket of a distinct state (repo.go:215-235)   */
};

/* Call flags. */
#define PHIP_DEVICE_PTRS 0x1u   /* all pointers of the call are device memory */
#define PHIP_ROUTE_COMBINE 0x2u /* phip_route_pack: combine hot names at the sender */
#define PHIP_GROUP_RCCL_SELF 0x4u /* phip_group_receive (testing): a member's own segment also
                                     travels through RCCL (ncclSend/ncclRecv to itself) instead
                                     of a device copy, and a world-1 group exchanges through
                                     RCCL instead of merging its send buffers in place, so the
                                     per-peer RCCL exchange runs on a single GPU */
#define PHIP_GROUP_SMALL_CHUNKS 0x8u /* phip_group_receive (testing): pipeline the exchange in
                                        chunks of 4096 messages instead of 2^24, so that small
                                        batches run many pack / exchange rounds */
#define PHIP_GROUP_PEEK_STATE 0x10u /* phip_group_peek: the 32-byte state column returns over the
                                       exchange too (every process of the group passes it alike) */
#define PHIP_RECV_ASYNC 0x20u /* phip_receive_soa with PHIP_DEVICE_PTRS, >= 2^16 messages: the
                                 call queues the batch and returns; the batch is finished
                                 (misses created, its dirty buckets through the ordered path,
                                 outputs final) by the handle's next call or phip_flush,
                                 which also returns its error (phip_len and phip_capacity
                                 finish it too, and leave its error to the handle's next
                                 call that returns a status).  Inputs and outputs must stay
                                 untouched until then.  A receive call queues its batch's
                                 classification and hot directory behind the batch before
                                 it, so the host's read-back of that batch overlaps them. */

#define PHIP_RECV_CLASSIFY 0x100u /* phip_receive_soa: classify this batch before it is merged,
                                     as PHIP_CFG_CLASSIFY_FIRST does for every batch of a
                                     handle (the shard group's merges pass it) */

/* phip_config.flags */
#define PHIP_CFG_NO_GROW 0x1u   /* refuse (PHIP_ERR_FULL / PHIP_ERR_ARENA) instead of growing */
#define PHIP_CFG_NO_SMALL 0x2u  /* ordered batches of <= 1024 host ops also take the large,
                                   multi-launch path (by default they run as one launch) */
#define PHIP_CFG_FIXED_SEED 0x4u /* place buckets with hash_seed as given (0: the unseeded
                                    placement) instead of a random per-handle seed */
#define PHIP_CFG_ISOLATE 0x8u   /* set every Receive batch's dirty buckets apart (phip_receive_soa
                                   "Order"); by default a handle does so from the first batch
                                   after one that held an incast or -0.0 field until 256
                                   clean batches in a row (a clean batch pays ~30 us for it) */
#define PHIP_CFG_CLASSIFY_FIRST 0x10u /* classify every decoded Receive batch before it is merged.
                                   By default a batch of a handle that does not set dirty
                                   buckets apart is merged optimistically, with an undo log:
                                   a batch that turns out to hold an incast, a -0.0 field or
                                   a malformed name entry is undone and run again classified,
                                   with the same results.  For A/B measurements and tests. */
#define PHIP_CFG_TRACK_CHANGES 0x20u /* the handle keeps a change set: the buckets its TAKE /
                                   UPSERT ops touched, for phip_export_changed ("Change set"
                                   below).  Two bits per slot; without the flag a handle
                                   launches exactly what it launched before the flag existed */
#define PHIP_CFG_TRACK_USAGE 0x40u /* the handle keeps a usage baseline: every bucket's `taken`
                                   at the last phip_usage_mark, for phip_export_top's metric
                                   PHIP_TOP_SINCE_MARK ("Windowed top talkers" below).  One
                                   uint64 per slot beside the table: 8 bytes a slot, 256 MB
                                   at 2^25 slots */

typedef struct phip_config {
  int32_t device;        /* HIP device ordinal                                          */
  uint32_t log2_slots;   /* initial table capacity = 2^log2_slots slots (4..31)         */
  uint64_t arena_bytes;  /* initial device arena for names longer than 22 bytes         */
  uint32_t max_load_pct; /* load factor that triggers growth (default 90, at most 95)  */
  uint32_t debug_tag_bits; /* 0 in production; 1..63 truncates the name hash so tests can
                              force tag collisions (names are always compared)          */
  uint32_t flags;        /* PHIP_CFG_*                                                   */
  uint32_t reserved;
  uint64_t hash_seed;    /* only with PHIP_CFG_FIXED_SEED (see "Placement" below)        */
} phip_config;
/*
 * Placement.  A bucket's tag is FNV-1a 64 of its name (also the shard map's
 * key, phip_group_*); its home slot is the top log2_slots bits of a 64-bit
 * mix of (tag ^ seed), with a seed drawn from the OS for every handle.  Go's
 * map, which the reference keeps its buckets in (repo.go:175), hashes with a
 * per-process random seed too: names chosen to collide under one placement
 * do not pile up on one probe chain under another.  Names are always
 * compared, so the seed never changes results, only where records lie.
 */
/*
 * Capacity.  Go's map never refuses a bucket (repo.go:204-207,225-227), so by
 * default the table and the long-name arena grow: before a batch creates
 * buckets, the engine reserves room for all of them (an upper bound: the
 * batch's distinct missing names) and rehashes into a table of 2x the slots
 * (k_rehash) or a larger arena whenever the reservation would pass
 * max_load_pct or the arena's end.  PHIP_ERR_FULL / PHIP_ERR_ARENA are then
 * only returned when growth is impossible (2^31 slots, device memory) or
 * disabled (PHIP_CFG_NO_GROW).  Such a refusal comes before any bucket of
 * the insert step is claimed: no bucket of the refused names is created, and
 * the table holds exactly what it held plus the merges the call's per-op
 * statuses report as applied (merges into existing buckets commute, so
 * re-submitting the other ops later is exact).
 */

/* Bucket state as Patrol holds it (bucket.go:20-32, name excluded). */
typedef struct phip_state {
  uint64_t added;    /* float64 bits */
  uint64_t taken;    /* float64 bits */
  int64_t elapsed;   /* time.Duration ns */
  int64_t created;   /* local creation time, ns since the Unix epoch */
} phip_state;

/*
 * Decoded replica states (the fields UnmarshalBinary fills, bucket.go:78-87).
 * Name i is names[name_offs[i] .. name_offs[i+1]).  With PHIP_DEVICE_PTRS the
 * names blob must stay readable 8 bytes past name_offs[n].
 *
 * names_len (the field was `reserved` before; same layout): the names blob's
 * length in bytes, or 0.  Host batches are checked on the host either way.
 * A device batch with names_len != 0 is checked on the device: every entry
 * must have name_offs[i] <= name_offs[i+1] <= names_len and at most
 * PHIP_MAX_NAME_LEN bytes.  No kernel then reads the blob at a malformed
 * entry's offsets, and the call returns PHIP_ERR_INVALID:
 *   - phip_receive_soa: the batch stops at the first malformed message k, as
 *     the Go loop stops at a short datagram (repo.go:70-74): messages before
 *     k are received as usual, k gets PHIP_ST_SHORT and every later one
 *     PHIP_ST_NOT_PROCESSED (a queued batch reports it from the call that
 *     finishes it);
 *   - phip_upsert_soa / phip_apply_mixed (phip_ops.names_len): nothing of the
 *     batch is applied;
 *   - phip_route_pack: nothing is packed;
 *   - phip_group_receive: none of the process's batches is applied (see
 *     there).
 * With names_len == 0 a device batch's offsets are trusted: a wild offset is
 * a read of device memory the kernels do not own.  A queued batch's input
 * columns must stay untouched until it is finished (PHIP_RECV_ASYNC): a
 * column reused early reads as corrupted offsets.
 */
typedef struct phip_msgs {
  uint32_t n;
  uint32_t names_len;
  const uint8_t* names;
  const uint32_t* name_offs; /* n+1 entries */
  const uint64_t* added;     /* float64 bits */
  const uint64_t* taken;     /* float64 bits */
  const int64_t* elapsed;
} phip_msgs;

/* A mixed ordered stream (one entry per op, applied in index order). */
typedef struct phip_ops {
  uint32_t n;
  uint32_t names_len;        /* the names blob's length, or 0 (see phip_msgs)   */
  const uint8_t* kind;       /* PHIP_OP_*                                       */
  const uint8_t* names;
  const uint32_t* name_offs; /* n+1 entries                                     */
  const int64_t* now;        /* clock() reading of each op (also `created`)     */
  const int64_t* freq;       /* Rate.Freq   (TAKE)                              */
  const int64_t* per;        /* Rate.Per ns (TAKE)                              */
  const uint64_t* count;     /* n tokens    (TAKE)                              */
  const uint64_t* added;     /* float64 bits (RECEIVE/UPSERT)                   */
  const uint64_t* taken;     /* float64 bits (RECEIVE/UPSERT)                   */
  const int64_t* elapsed;    /* (RECEIVE/UPSERT)                                */
} phip_ops;

/* Per-op results (any pointer may be NULL).
 *
 * Result columns.  Each pointer is a column of n entries, n the batch's size
 * (phip_msgs.n, phip_ops.n, the datagram count), in host memory or, with
 * PHIP_DEVICE_PTRS, device memory; a column needs its entry type's alignment
 * and no more.  After a call that returns PHIP_OK, and after one that stopped
 * (below), a column that was passed is written in all n entries and nowhere
 * else, whatever other columns were passed with it and whatever path the
 * batch took.  An entry the column does not apply to reads zero:
 *   - remaining and have of a RECEIVE or UPSERT op, and so every entry of
 *     them after phip_receive_soa, phip_receive_datagrams, phip_ring_receive,
 *     their _replies forms and phip_upsert_soa;
 *   - reply of a merged replica (PHIP_ST_MERGED of a RECEIVE op);
 *   - remaining, have and reply of every message at or after a Receive
 *     batch's stop, a short datagram (PHIP_ERR_SHORT_BUFFER) or a checked
 *     batch's malformed entry (PHIP_ERR_INVALID from phip_receive_soa with
 *     names_len, phip_msgs): status reads PHIP_ST_SHORT there and
 *     PHIP_ST_NOT_PROCESSED after it, and the columns of the messages before
 *     it are those of a batch that ended there.
 * Nothing the caller passes in (names, offsets, operands, datagrams) is ever
 * written.  A batch queued with PHIP_RECV_ASYNC has its columns written by
 * the call that finishes it.
 * A call refused with any other error (PHIP_ERR_INVALID for bad arguments, a
 * checked phip_upsert_soa / phip_apply_mixed batch or egress caps too small;
 * PHIP_ERR_FULL for a table that may not grow; ...) leaves the columns
 * undefined: untouched, partly written, or, from host memory, not copied
 * back. */
typedef struct phip_results {
  uint8_t* status;           /* PHIP_ST_* (| PHIP_ST_CREATED)                   */
  uint64_t* remaining;       /* TAKE: uint64(remaining) as Go returns it        */
  uint64_t* have;            /* TAKE: float64 bits of the value truncated       */
  phip_state* reply;         /* the bucket's state right after the op, for:
                                  TAKE: what UpsertBucket broadcasts after the take
                                        (api.go:74, repo.go:123-127);
                                  UPSERT: the upserted bucket (repo.go:123-127);
                                  RECEIVE of a zero state (incast): the local state,
                                        unchanged by it: the unicast payload of an
                                        INCAST_REPLY (repo.go:86-90), and what
                                        GetBucket found or created (repo.go:189-211).
                                  A merged replica (PHIP_ST_MERGED of a RECEIVE op)
                                  has no reply state: its entry is all zeros.       */
} phip_results;

/* ---- lifecycle ---- */
int phip_abi_version(void);
/* 16 hex digits naming the library's sources (a hash of csrc/, this header
 * and the Makefile taken when the library was built): counter profiles and
 * bench lines record it, so a measurement can be tied to the code that ran. */
const char* phip_build_id(void);
int phip_open(const phip_config* cfg, phip_handle** out);
void phip_close(phip_handle* h);
const char* phip_last_error(const phip_handle* h);
int phip_flush(phip_handle* h);                    /* hipStreamSynchronize */
/* Run every later call of this handle on `stream` (a hipStream_t of the
 * handle's device, e.g. the producer's stream of PHIP_DEVICE_PTRS inputs, so
 * that no cross-stream synchronisation is needed); NULL restores the
 * handle's own stream.  Work queued earlier is finished first. */
int phip_set_stream(phip_handle* h, void* stream);
uint64_t phip_len(phip_handle* h);                 /* number of buckets */
uint64_t phip_capacity(phip_handle* h);            /* number of slots */

/* ---- repo ---- */
/* NewLocalRepo(clock, bs...): insert (or overwrite) buckets as given. */
int phip_seed(phip_handle* h, const uint8_t* names, const uint32_t* name_offs, uint32_t n,
              const phip_state* states, uint32_t flags);
/* Lookup without creating.  Returns 1 found, 0 absent, <0 error. */
int phip_get(phip_handle* h, const uint8_t* name, uint32_t len, phip_state* out);
/* Dump every bucket (unordered).  Call with names==NULL to size: *n_out and
 * *names_bytes_out are filled.  name_offs has n+1 entries. */
/* Snapshot / restore (the reference has none and recovers a
 * restarted node through incast, repo.go:96-106).  phip_snapshot writes
 * phip_snapshot_bytes(h) bytes into a host buffer: a 64-byte header (magic
 * "PHIPSNP1", ABI version, log2_slots, bucket count, arena bytes), the 2^L
 * slot records as they lie in HBM (64 B each), then the used long-name arena.
 * phip_restore loads such an image into a handle opened with the same
 * log2_slots (and an arena at least as large): the table is reproduced
 * exactly, with no rehash.  phip_dump + phip_seed is the portable route
 * between different table sizes. */
uint64_t phip_snapshot_bytes(phip_handle* h);
int phip_snapshot(phip_handle* h, uint8_t* out, uint64_t cap);
int phip_restore(phip_handle* h, const uint8_t* in, uint64_t len);

/* Egress batching (replaces the per-peer, per-take marshal of
 * repo.go:129-158 broadcast and :160-169 unicast): the current state of each
 * named bucket as its byte-identical MarshalBinary datagram (bucket.go:51-68).
 * Datagram i is out[25*i + (name_offs[i] - name_offs[0])], 25 + len_i bytes
 * long, so `out` holds 25*n + name bytes and the datagrams are back to back
 * in the order given (ready for one sendmmsg).  found[i] = 1 when the bucket
 * exists; an absent bucket's datagram bytes are zero.  Host or device
 * pointers (PHIP_DEVICE_PTRS). */
int phip_export_datagrams(phip_handle* h, const uint8_t* names, const uint32_t* name_offs,
                          uint32_t n, uint8_t* out, uint8_t* found, uint32_t flags);

/* Evict idle buckets (the reference has no counterpart: repo.go:175 is a map
 * that only grows, and a restarted Go process starts with an empty one).
 *
 * Rule.  last = created + elapsed, exact in 128 bits as Take computes it
 * (bucket.go:198); idle = now - last, 0 when now < last (a replica's merged
 * elapsed can run ahead of the local clock) and saturating at INT64_MAX.  A
 * bucket is idle iff idle >= idle_ns.  idle_ns <= 0 is PHIP_ERR_INVALID.
 *
 * Semantics.  Evicting a bucket is, for that bucket, what a node restart is
 * in the reference: the next GetBucket creates it afresh with created = now
 * and reports PHIP_ST_CREATED / phip_take_reply.created, so the caller sends
 * the zero-state incast request (repo.go:96-106) and the peers' states merge
 * back in as they arrive.
 *
 * Choosing idle_ns.  Keep idle_ns >= per for every rate served.  Then the
 * first Take on a recreated bucket returns the same (ok, remaining) as it
 * would have on the evicted one: dt >= per makes Tokens(dt) >= Freq, so the
 * refill clamps to capacity - tokens (bucket.go:210-213) and have == capacity
 * either way.
 *
 * Two passes.  k_evict_count reads every slot once and counts the idle
 * buckets, the survivors and the survivors' long-name bytes.  On a dry run
 * (PHIP_EVICT_DRY_RUN), or with fewer than min_evict idle buckets (the
 * caller's hysteresis; 0 is treated as 1), the call returns there: *out is
 * filled, nothing is rebuilt.  Otherwise k_evict_move moves the survivors into
 * a fresh table and their long names into a fresh, byte-packed arena (of at
 * least the handle's opening arena_bytes), and the old ones are freed: no
 * tombstones, no lookup kernel changes.  With PHIP_EVICT_SHRINK the new table
 * has 2^L' slots, L' the smallest with L_open <= L' <= L_now and survivors <=
 * load_limit(2^L', max_load_pct) / 2 (L_open: the log2_slots the handle was
 * opened with; growth doubles at the limit, so the population must double
 * before the table grows again); without it the slot count is unchanged.
 * On any failure (PHIP_ERR_FULL when device memory runs out, HIP errors) the
 * old table and arena stay live and unchanged.  Unknown flag bits are
 * PHIP_ERR_INVALID.  The call is serialised with every other call of the
 * handle (the Take batcher's dispatcher included); a batch queued with
 * PHIP_RECV_ASYNC is finished first, and its error is this call's.
 * phip_snapshot / phip_restore keep working: the image has the new
 * log2_slots and arena bytes. */
#define PHIP_EVICT_SHRINK  0x40u  /* also pick a smaller table (rule above) */
#define PHIP_EVICT_DRY_RUN 0x80u  /* count only; the table is not touched   */
typedef struct phip_evict_stats {
  uint64_t idle;        /* buckets that met the rule                          */
  uint64_t evicted;     /* buckets removed (0 on a dry run or under min_evict)*/
  uint64_t buckets;     /* phip_len afterwards                                */
  uint64_t slots;       /* phip_capacity afterwards                           */
  uint64_t arena_used;  /* long-name arena bytes in use afterwards            */
  uint64_t arena_freed; /* bytes the compaction gave back                     */
} phip_evict_stats;
int phip_evict_idle(phip_handle* h, int64_t now, int64_t idle_ns, uint64_t min_evict,
                    phip_evict_stats* out /* may be NULL */, uint32_t flags);
int phip_dump(phip_handle* h, uint8_t* names, uint64_t names_cap, uint64_t* name_offs,
              phip_state* states, uint64_t max_n, uint64_t* n_out, uint64_t* names_bytes_out);

/* Anti-entropy sweep: the live table as wire datagrams, a bounded piece per
 * call (the reference has no counterpart: a Patrol node gets state one bucket
 * at a time, by a zero-state incast request per bucket it touches,
 * repo.go:96-106, and never pushes its state anywhere).  A caller loops
 *     phip_export_sweep -> phip_udp_send_batch (or a peer handle's
 *     phip_receive_datagrams)
 * until st->done, and the peer has merged everything this table knows.
 *
 * Output.  Datagram i is out[offs[i] .. offs[i+1]), offs[0] = 0: the bucket's
 * byte-identical MarshalBinary (bucket.go:51-68: added, taken, elapsed
 * big-endian, one length byte, the name), back to back -- the layout
 * phip_udp_send_batch and phip_receive_datagrams take, offs uint64 as theirs.
 * Within a call the buckets appear in slot order.
 *
 * Which buckets.  Every published record of the slots the call covers, except:
 *  - a record whose state is zero (Bucket.IsZero, bucket.go:165-170): its
 *    datagram would be an incast request to the receiver (repo.go:78,86-90),
 *    not a merge, and carries nothing a merge could use;
 *  - with idle_ns > 0, a record phip_evict_idle's rule calls idle at `now`
 *    (idle = now - (created + elapsed) >= idle_ns, the same arithmetic).  This
 *    keeps the buckets whose last successful Take or merged `elapsed` lies
 *    within idle_ns of `now`.  It is not a change log: a denied Take and a
 *    merge that raises only added / taken do not move `elapsed`, and such a
 *    bucket is filtered as if untouched.  idle_ns == 0: no filter; idle_ns < 0
 *    is PHIP_ERR_INVALID;
 *  - a record whose name is longer than PHIP_MAX_NAME_LEN (only a datagram
 *    can bring one in): MarshalBinary refuses it (bucket.go:48).
 * NaN, -0.0 and negative fields are exported as they are (the receiver's
 * ordered path handles -0.0).
 *
 * Bounds and progress.  A call writes at most max_msgs datagrams and at most
 * out_cap bytes, cut at a record (never at a tile or window), and sets *cur to
 * the slot of the first record it did not write, or to the end of the slots
 * it covered.  max_msgs == 0 or out_cap < PHIP_BUCKET_PACKET_SIZE (one
 * datagram of a PHIP_MAX_NAME_LEN-byte name) is PHIP_ERR_INVALID, so every
 * valid call makes progress.
 *
 * Window.  A call reads the slots [cur->slot, cur->slot + W) clipped to the
 * table, W = max(4 * max_msgs, PHIP_SWEEP_TILE) rounded up to a multiple of
 * PHIP_SWEEP_TILE, and never the rest of the table: a sweep in small batches
 * stays linear in the table size.  A call may write fewer than max_msgs
 * datagrams, or none, with done == 0: loop until done.
 *
 * Rebuilds.  The handle counts its table layouts: growth, the move of
 * phip_evict_idle and phip_restore each begin a new one, and slot numbers
 * mean nothing across them.  The cursor carries the count it was made under;
 * a cursor of another layout starts again at slot 0 and the call reports
 * restarted = 1.  That is no error: merges are idempotent, so a bucket sent
 * twice is harmless.  A zeroed cursor (the start) never reports it.  A cursor
 * belongs to the handle that filled it.
 *
 * Count mode.  PHIP_SWEEP_COUNT with out == NULL (offs, out_cap and max_msgs
 * are ignored): one count pass over the whole table under the same filter;
 * st->n and st->bytes receive what a whole sweep would write, to size
 * buffers by, and *cur is left untouched.
 *
 * Pointers and flags.  Host pointers, or PHIP_DEVICE_PTRS: `out` must then be
 * 8-byte aligned and out_cap a multiple of 8 and at least
 * PHIP_BUCKET_PACKET_SIZE + 8, else PHIP_ERR_INVALID; the byte budget is
 * out_cap - 8, so the next 8-byte boundary past offs[n] lies inside the buffer
 * and out / offs can go unchanged into another handle's
 * phip_receive_datagrams(..., PHIP_DEVICE_PTRS), which reads aligned words.
 * With host pointers only the bytes and offsets written are copied back.
 * cur and st are host memory either way.  Unknown flag bits are
 * PHIP_ERR_INVALID.  The call is serialised with the handle's other calls, as
 * phip_evict_idle is; a batch queued with PHIP_RECV_ASYNC is finished first,
 * and its error is this call's. */
#define PHIP_SWEEP_TILE 4096      /* slots: the window's granule (see "Window") */
#define PHIP_SWEEP_COUNT 0x200u   /* count only (see "Count mode")              */
typedef struct phip_sweep_cursor {
  uint64_t slot;   /* next slot to read                              */
  uint64_t layout; /* the table layout the slot number belongs to    */
} phip_sweep_cursor; /* all zero = start */
typedef struct phip_sweep_stats {
  uint64_t n;             /* datagrams written (count mode: datagrams the whole table would give) */
  uint64_t bytes;         /* = offs[n]                                                            */
  uint64_t slots_scanned; /* slots this call read (one pass's worth)                              */
  uint32_t done;          /* 1: the cursor reached the end of the table                           */
  uint32_t restarted;     /* 1: the table was rebuilt since the cursor was made; began at slot 0  */
} phip_sweep_stats;
int phip_export_sweep(phip_handle* h, phip_sweep_cursor* cur, int64_t now, int64_t idle_ns,
                      uint8_t* out, uint64_t out_cap, uint64_t* offs /* max_msgs+1 */,
                      uint32_t max_msgs, phip_sweep_stats* st, uint32_t flags);

/* Partition digests: what a table holds, in 16 bytes per partition of the
 * name space, so that two replicas find where they differ without sweeping
 * (the Dynamo / Riak anti-entropy scheme; the reference has no counterpart).
 * One reconcile round between two nodes:
 *     both:  phip_table_digest(h, k, mine)              exchange 16 * 2^k bytes
 *     both:  phip_digest_diff(mine, theirs, k, mask, &ndiff)
 *     both:  loop phip_export_sweep_parts(h, &cur, ..., k, mask, ...) until
 *            st.done, into the peer's phip_receive_datagrams
 * after which, NaN fields aside (below), the digests are equal.
 *
 * Definitions (tests/_digest_cases.py restates them).  fmix(x) is murmur3's
 * 64-bit finaliser: x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33;
 * x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33.  canon(bits) is 0 for
 * 0x8000000000000000 and bits otherwise: +0 and -0 never converge under Merge
 * (Go's `<` keeps the zero seen first), so replicas that differ only in the
 * sign of a zero count as equal.
 *  - Covered records: exactly those phip_export_sweep writes with idle_ns = 0:
 *    published, state not zero (a zero state's datagram would be an incast
 *    request, and a bucket one side holds as a zero state and the other not at
 *    all must not make them differ), name of at most PHIP_MAX_NAME_LEN bytes.
 *    There is no idle filter: `created` is local to a node.
 *  - Partition: k = log2_parts, 0 <= k <= PHIP_DIGEST_MAX_LOG2_PARTS;
 *    part(tag, k) = k ? fmix(tag) >> (64 - k) : 0, where tag is the record's
 *    stored tag: FNV-1a 64 of the name (phip_hash_names), masked by
 *    phip_config.debug_tag_bits, 0 stored as 1.  It is the same on every node,
 *    under every placement seed, table size and rebuild.  (The mix: the shard
 *    map spends the tag's own top bits, and truncated test tags have none.)
 *    Two tables are comparable only if opened with the same debug_tag_bits.
 *  - Record hash, on IEEE bit patterns, never on created, flags or offsets:
 *        h = fmix(tag + 0x9E3779B97F4A7C15)
 *        h = fmix(h ^ canon(added));  h = fmix(h ^ canon(taken))
 *        h = fmix(h ^ (uint64_t)elapsed)
 *  - Entry p: sum = the covered records' h of partition p added mod 2^64,
 *    count = how many.  Entries are additive: entry p at level k - 1 is entry
 *    2p + entry 2p + 1 at level k (phip_digest_fold), so one pass at a fine
 *    level gives every coarser one.
 * Limits.  Names whose 64-bit tags collide are told apart by the table but not
 * by the digest: a swap of states between two such names goes unseen (it takes
 * an FNV-1a 64 collision).  A NaN field never converges (a local NaN sticks, a
 * replica's NaN is never adopted): a partition holding a bucket whose replicas
 * disagree on a NaN differs in every round and its few buckets are re-sent
 * every round -- harmless, bounded by the partition.  Likewise fields below
 * zero against a bucket the peer lacks or holds as a zero state: the receiver
 * creates the bucket at zero and Merge never lowers, so one negative field
 * takes a second round (the receiver's zero comes back), and a bucket all of
 * whose fields are <= 0 never converges (the receiver's state stays zero, and
 * a zero state is never sent).  The sums are no defence against a peer that
 * crafts states.
 *
 * phip_table_digest reads the whole table once and leaves it untouched.  out:
 * 2^log2_parts entries, host memory, or device memory (8-byte aligned) with
 * PHIP_DEVICE_PTRS; any other flag bit, log2_parts > 20 or out == NULL is
 * PHIP_ERR_INVALID, and a refused call touches neither out nor st.  st (host
 * memory, may be NULL): records and bytes are what count mode reports with
 * idle_ns = 0.  Serialised with the handle's other calls; a batch queued with
 * PHIP_RECV_ASYNC is finished first, and its error is this call's.
 *
 * phip_digest_diff / phip_digest_fold are host only (no handle, no GPU).
 * diff: bit p of mask (word p >> 6, bit p & 63; max(1, 2^k / 64) words) is set
 * iff sum or count of entry p differ; bits beyond 2^k are zero; *ndiff (may be
 * NULL) is the number of set bits.  fold: level log2_in to level log2_out <=
 * log2_in (greater: PHIP_ERR_INVALID); in and out may be the same buffer.
 *
 * phip_export_sweep_parts is phip_export_sweep -- the same output, caps, cut
 * at a record, cursor and layout count, restarted, pointer rules and count
 * mode, idle_ns composing as there -- with one more condition on which
 * buckets: bit part(tag, log2_parts) of part_mask must be set.  part_mask is
 * host memory either way (max(1, 2^k / 64) words); NULL or log2_parts > 20 is
 * PHIP_ERR_INVALID.  Window: with m set bits among the first 2^k, m == 0 reads
 * no slot and returns n = 0, done = 1, slots_scanned = 0, offs[0] = 0 and the
 * cursor at the end of the table (count mode: n = bytes = 0); otherwise
 * W = max(4 * max_msgs * ceil(2^k / m), PHIP_SWEEP_TILE) rounded up to a
 * multiple of PHIP_SWEEP_TILE (saturating, clipped to the table), so that a
 * window holds about as many qualifying records as the unfiltered sweep's; a
 * call still never reads past its window. */
#define PHIP_DIGEST_MAX_LOG2_PARTS 20
typedef struct phip_digest_part {
  uint64_t sum;   /* covered records' hashes, added mod 2^64 */
  uint64_t count; /* covered records                         */
} phip_digest_part;
typedef struct phip_digest_stats {
  uint64_t records;       /* sum of count = count mode's n with idle_ns = 0        */
  uint64_t bytes;         /* sum of 25 + name length of them = count mode's bytes  */
  uint64_t slots_scanned; /* the table's slots                                     */
} phip_digest_stats;
int phip_table_digest(phip_handle* h, uint32_t log2_parts, phip_digest_part* out /* 2^k */,
                      phip_digest_stats* st /* may be NULL */, uint32_t flags);
int phip_digest_diff(const phip_digest_part* a, const phip_digest_part* b, uint32_t log2_parts,
                     uint64_t* mask, uint64_t* ndiff /* may be NULL */);
int phip_digest_fold(const phip_digest_part* in, uint32_t log2_in, uint32_t log2_out,
                     phip_digest_part* out /* 2^log2_out */);
int phip_export_sweep_parts(phip_handle* h, phip_sweep_cursor* cur, int64_t now, int64_t idle_ns,
                            uint32_t log2_parts, const uint64_t* part_mask, uint8_t* out,
                            uint64_t out_cap, uint64_t* offs /* max_msgs+1 */, uint32_t max_msgs,
                            phip_sweep_stats* st, uint32_t flags);

/* ---- hot path ---- */
/* ReplicatedRepo.Receive over n raw datagrams (byte-identical wire format,
 * bucket.go:59-64): bytes[offs[i] .. offs[i+1]).  `now` is the clock reading
 * used for buckets created by this batch.  Stops at the first malformed
 * datagram like the Go loop (repo.go:72-73): *stop_index receives its index
 * (or n) and the call returns PHIP_ERR_SHORT_BUFFER when one was found.
 * With PHIP_DEVICE_PTRS, `bytes` must be 8-byte aligned and readable up to
 * the next 8-byte boundary past offs[n] (the fast path reads the datagrams
 * in place as aligned words). */
int phip_receive_datagrams(phip_handle* h, const uint8_t* bytes, const uint64_t* offs, uint32_t n,
                           int64_t now, const phip_results* res, uint32_t* stop_index,
                           uint32_t flags);
/* The same loop over pre-decoded states.
 * Order: a message's result depends only on the earlier messages naming its
 * bucket (repo.go:77-106), and only incasts (a zero state) and -0.0 fields
 * make that order visible.  A batch with at most 4096 such "dirty" messages,
 * each named in at most 14 bytes, has its other buckets merged in one
 * order-free pass and only its dirty buckets' sequences (each dirty message,
 * and one merge of the clean messages between two of them) applied in order
 * afterwards (phip_kernels.hpp "Dirty buckets"; phip_receive_datagrams
 * alike).  Larger dirty sets apply everything from the first dirty message
 * on in order.  The results are the Go loop's either way. */
int phip_receive_soa(phip_handle* h, const phip_msgs* m, int64_t now, const phip_results* res,
                     uint32_t flags);
/* LocalRepo.UpsertBucket for each state, in order. */
int phip_upsert_soa(phip_handle* h, const phip_msgs* m, int64_t now, const phip_results* res,
                    uint32_t flags);
/* Ordered mixed stream of TAKE / RECEIVE / UPSERT ops. */
int phip_apply_mixed(phip_handle* h, const phip_ops* ops, const phip_results* res, uint32_t flags);

/* Coalesced egress: a batch's replication traffic, written by the batch's own
 * call.  In the reference every take ends in UpsertBucket, whose broadcast
 * sends the bucket's state to every peer, granted or denied (api.go:67-74,
 * repo.go:123-158), and a take whose GetBucket created the bucket sends a
 * zero-state incast request first (repo.go:96-106): one datagram per peer per
 * take.  phip_apply_mixed_egress is phip_apply_mixed -- the same statuses,
 * results, errors, flags and checked-offset rule -- plus one datagram per
 * bucket the batch touched, in the layout phip_udp_send_batch and a peer's
 * phip_receive_datagrams take: datagram i is out[offs[i] .. offs[i+1]),
 * offs[0] = 0, bytes = offs[n].
 *
 * State section, datagrams [n_incast, n).  For every bucket named by at least
 * one PHIP_OP_TAKE or PHIP_OP_UPSERT op of the batch: the byte-identical
 * MarshalBinary (bucket.go:51-68) of the state the table holds after the
 * batch's last op.  A bucket named only by PHIP_OP_RECEIVE ops gets nothing:
 * received merges are never rebroadcast (repo.go:78-79), and its incast
 * replies stay in phip_results.reply, unicast to one peer.  Left out, by the
 * sweep's rule (phip_export_sweep with idle_ns = 0): a bucket whose final
 * state is zero (its datagram would be an incast request) and a name over
 * PHIP_MAX_NAME_LEN.
 *
 * Incast section, datagrams [0, n_incast).  For every bucket the batch created
 * whose first op in batch order is a TAKE -- the op that reports
 * PHIP_ST_CREATED -- the request ReplicatedRepo.GetBucket broadcasts: 24 zero
 * bytes, the length byte, the name.  A bucket created by a RECEIVE or UPSERT
 * op sends none (repo.go:78, repo.go:215-235).
 *
 * Each section is in table slot order, as the sweep writes.
 *
 * What coalescing means, and its limit.  A peer that merges the state section
 * ends where it would after merging the reference's per-op broadcasts in
 * order, whenever each bucket's post-op states are field-wise non-decreasing:
 * Merge keeps the field-wise maximum, and the final state is then that
 * maximum.  Takes at one rate per bucket with a non-decreasing clock are such
 * a sequence.  It does not hold in general: a take at a smaller capacity than
 * the tokens held lowers `added` (bucket.go:210-213, missing < 0), and a peer
 * that saw the intermediate state would keep the higher value.  The datagram
 * is the final state, which is what the reference's last broadcast of that
 * bucket carries; the join of the intermediate states is not computed.
 *
 * Caps.  Checked before anything is applied, against the batch's worst case
 * (every op a new bucket's TAKE): max_msgs >= 2 * n and out_cap >=
 * 2 * (25 * n + name_bytes), name_bytes being name_offs[n] - name_offs[0] for
 * a host batch, names_len for a checked device batch and 231 * n for an
 * unchecked one.  With PHIP_DEVICE_PTRS `out` must be 8-byte aligned and
 * out_cap a multiple of 8 with 8 bytes more than that, as phip_export_sweep
 * requires, and out / offs then go unchanged into a peer handle's
 * phip_receive_datagrams(..., PHIP_DEVICE_PTRS).  phip_egress_caps (host
 * arithmetic only; flags: 0 or PHIP_DEVICE_PTRS) returns exactly these
 * figures.  Caps below them are PHIP_ERR_INVALID with the table and every
 * output untouched, so a valid call never truncates.
 *
 * eg is host memory; out and offs follow PHIP_DEVICE_PTRS like every other
 * pointer of the call, and a host-pointer call copies back only the bytes and
 * offsets written.  res may be NULL, and so may any column of it.  n == 0
 * gives n = n_incast = bytes = 0 and offs[0] = 0.  On any error return the
 * three out fields are zero.  The call is serialised with the handle's other
 * calls; a batch queued with PHIP_RECV_ASYNC is finished first. */
typedef struct phip_egress {
  uint8_t*  out;       /* in: datagram bytes */
  uint64_t  out_cap;   /* in */
  uint64_t* offs;      /* in: max_msgs + 1 entries */
  uint32_t  max_msgs;  /* in */
  uint32_t  n_incast;  /* out */
  uint32_t  n;         /* out: all datagrams */
  uint32_t  reserved;
  uint64_t  bytes;     /* out: = offs[n] */
} phip_egress;
int phip_egress_caps(uint32_t n_ops, uint64_t name_bytes, uint32_t flags, uint32_t* max_msgs,
                     uint64_t* out_cap);
int phip_apply_mixed_egress(phip_handle* h, const phip_ops* ops, const phip_results* res,
                            phip_egress* eg, uint32_t flags);

/* Change set: the buckets this handle's own takes touched since they were
 * last exported, for a replicator that runs on its own clock.  A handle opened
 * with PHIP_CFG_TRACK_CHANGES remembers them; phip_export_changed writes their
 * replication traffic in the layout of "Coalesced egress" above and forgets
 * what it wrote:
 *     every window:  loop phip_export_changed -> phip_udp_send_batch per peer
 *                    (or a peer handle's phip_receive_datagrams) until st->done
 * This is "Coalesced egress" with the window chosen by the caller instead of
 * by the batch: a take pays a mark, not a datagram, and a bucket taken from in
 * a hundred batches of one window leaves once.
 *
 * What marks.  Two marks per bucket, the two rules of "Coalesced egress" made
 * persistent:
 *  - state pending: a PHIP_OP_TAKE or PHIP_OP_UPSERT op named the bucket (every
 *    take ends in UpsertBucket's broadcast, granted or denied, api.go:67-74,
 *    repo.go:123-158);
 *  - request pending: a batch created the bucket and its first op on it is a
 *    TAKE, the op that reports PHIP_ST_CREATED (GetBucket's incast request,
 *    repo.go:96-106).
 * They are set by every call that runs ordered ops: phip_apply_mixed, phip_take,
 * phip_api_take, the batcher, and the owner's apply inside
 * phip_group_apply_mixed (every owner marks its own table:
 * phip_group_handle(g, i) and this call are the owners' egress).  They are set
 * behind the batch's last op, once the batch stands.  Nothing is set by
 * PHIP_OP_RECEIVE ops and the phip_receive_* calls (received merges are never
 * rebroadcast, repo.go:78-79), by phip_upsert_soa and phip_seed
 * (LocalRepo.UpsertBucket broadcasts nothing, repo.go:215-235), by
 * phip_apply_mixed_egress (its datagrams left with the call), or by a batch
 * that is refused (PHIP_ERR_FULL / PHIP_ERR_ARENA before any claim, a
 * malformed offset column).
 *
 * Output.  Datagram i is out[offs[i] .. offs[i+1]), offs[0] = 0, bytes =
 * offs[n].  The requests come first, datagrams [0, n_incast): 24 zero bytes,
 * the length byte, the name.  The states follow, [n_incast, n): the
 * byte-identical MarshalBinary (bucket.go:51-68) of the state the table holds
 * at the export.  Each section is in table slot order.  Left out, as in the
 * egress and the sweep: a state that is zero and a name over PHIP_MAX_NAME_LEN;
 * their marks are cleared all the same.  The coalescing limit is the one
 * stated under "Coalesced egress": the datagram is the final state, the join
 * of the intermediate states is not computed.
 *
 * Bounds and progress.  A call writes at most max_msgs datagrams and out_cap
 * bytes, cut at a record.  max_msgs == 0 or out_cap < PHIP_BUCKET_PACKET_SIZE
 * is PHIP_ERR_INVALID, so every valid call with something pending makes
 * progress.  A mark is cleared exactly when its datagram was written or was
 * left out by the rule above; what was cut stays pending for the next call.
 * The state section starts only in a call whose request section left no
 * request pending, so no bucket's state ever leaves before its request, across
 * calls as within one.  st->pending counts the marks still set after the call
 * (requests and states), st->done = (pending == 0).  An argument error reads
 * and clears nothing.
 *
 * Count mode.  PHIP_SWEEP_COUNT with out == NULL (offs, out_cap and max_msgs
 * are ignored): st->n, st->n_incast and st->bytes of a full drain, st->pending
 * the marks set, and nothing is cleared.
 *
 * Layout changes.  The marks belong to buckets, not slots: table growth and
 * phip_evict_idle's move carry a surviving bucket's marks along, an evicted
 * bucket's marks go with it (as after a node restart), and phip_restore clears
 * the set (a snapshot does not hold it).
 *
 * Pointers and flags.  Host pointers, or PHIP_DEVICE_PTRS under
 * phip_export_sweep's rules: `out` 8-byte aligned, out_cap a multiple of 8 and
 * at least PHIP_BUCKET_PACKET_SIZE + 8, the byte budget out_cap - 8; out / offs
 * then go unchanged into phip_receive_datagrams(..., PHIP_DEVICE_PTRS).  st is
 * host memory.  Unknown flag bits, and a handle opened without
 * PHIP_CFG_TRACK_CHANGES, are PHIP_ERR_INVALID.  The call is serialised with
 * the handle's other calls; a batch queued with PHIP_RECV_ASYNC is finished
 * first, and its error is this call's. */
typedef struct phip_changes_stats {
  uint64_t n;         /* datagrams written (count mode: what a full drain would write) */
  uint64_t bytes;     /* = offs[n]                                                      */
  uint32_t n_incast;  /* the requests, datagrams [0, n_incast)                          */
  uint32_t done;      /* 1: nothing is pending after this call                          */
  uint64_t pending;   /* marks still set after this call (requests + states)            */
} phip_changes_stats;
int phip_export_changed(phip_handle* h, uint8_t* out, uint64_t out_cap,
                        uint64_t* offs /* max_msgs+1 */, uint32_t max_msgs,
                        phip_changes_stats* st, uint32_t flags);
/* All-TAKE convenience form of phip_apply_mixed. */
int phip_take(phip_handle* h, const uint8_t* names, const uint32_t* name_offs, uint32_t n,
              const int64_t* now, const int64_t* freq, const int64_t* per, const uint64_t* count,
              uint64_t* remaining_out, uint8_t* ok_out, uint32_t flags);

/* Peek: batched read-only quota queries with an exact retry time.  Every other
 * entry point that answers "may this request pass?" also spends the tokens
 * (GetBucket + Bucket.Take, bucket.go:186-225, api.go:67-74).  Peek answers
 * the two questions a deployed rate limiter is asked without spending any: how
 * much is left for this key (an X-RateLimit-Remaining header, a dashboard, a
 * per-user and a per-org limit checked before taking from either), and when
 * may a denied key come back (the Retry-After of a 429, the expiry of a deny
 * entry cached at a load balancer).
 *
 * A query is (name, now, freq, per, count): the TAKE operands of phip_ops.
 *  1. State read.  A present bucket gives its record (added, taken, elapsed,
 *     created).  An absent bucket gives what GetBucket would have created
 *     (repo.go:189-211): the zero state with created = now.  Nothing is created.
 *  2. Evaluation.  Bucket.Take runs on that copy with Rate{freq, per} and
 *     count tokens, bit-exact as everywhere here.  status is PHIP_ST_TAKE_OK or
 *     PHIP_ST_TAKE_DENIED, with PHIP_ST_ABSENT or-ed in for an absent bucket;
 *     remaining and have are exactly what phip_apply_mixed reports for a TAKE
 *     op with these operands applied to that state (phip_results.remaining /
 *     .have).  count is used as given, 0 included: api.go:63's 0 -> 1 belongs
 *     to the HTTP helper (phip_api_peek).
 *  3. retry_at (int64 ns on the clock of `now`).  Let ok(t) be step 2 with
 *     `now` replaced by t and everything else unchanged (an absent bucket's
 *     created stays the query's `now`).  Granted: retry_at = now.  Denied: the
 *     least t in (now, INT64_MAX] with ok(t); if ok(INT64_MAX) is false,
 *     PHIP_PEEK_NEVER (INT64_MIN, which no valid answer can be: those are >
 *     now).  The value is defined by this predicate, not by a formula: from a
 *     denial ok(t) goes from false to true at most once (Take's dt does not
 *     decrease in t, nor do dt / interval, its clamp and tokens + it when
 *     interval > 0; with interval <= 0 the refill never grows and the answer
 *     is never), and the library bisects it: at most 66
 *     evaluations of Take's verdict a query, none for a granted one.
 *  4. Nothing is written: table, arena, change set, layout count, the hot
 *     directory and phip_len stay as they are.  The call is serialised with
 *     the handle's other calls, as phip_export_datagrams is; a batch queued
 *     with PHIP_RECV_ASYNC is finished first, its error is this call's, and
 *     the peek sees its merges.
 *
 * phip_peek.  Of q it reads n, names, name_offs, names_len, now, freq, per and
 * count; a NULL operand column reads as zeros; kind, added, taken and elapsed
 * are ignored.  Any column of res may be NULL, and so may res.  Host pointers
 * are staged as phip_export_datagrams stages them (one stream synchronise), and
 * a name over PHIP_MAX_NAME_LEN is PHIP_ERR_NAME_TOO_LARGE; PHIP_DEVICE_PTRS
 * makes every pointer device memory; any other flag bit is PHIP_ERR_INVALID.
 * A device batch with names_len != 0 has its offset column checked first (the
 * rule of phip_msgs): a malformed entry is PHIP_ERR_INVALID, no name is read
 * and the result columns are untouched.  n == 0 is PHIP_OK.
 *
 * phip_peek_eval is steps 2 and 3 on the host (no handle, no GPU), the same
 * function the kernel calls: a handler that holds a phip_take_reply.state
 * computes the Retry-After of the 429 it just issued without a device call.
 * s == NULL stands for an absent bucket.  Returns the status byte (without
 * PHIP_ST_ABSENT), or PHIP_ERR_INVALID when one of the three outputs is NULL.
 *
 * phip_api_peek is phip_api_take's request parsing (api.go:55-65: ParseRate's
 * values beside its errors, count 0 -> 1, 400 with ErrNameTooLarge's text
 * before any device call) over one phip_peek: the body is `remaining` in
 * decimal, the return 200 or 429 (or 400, or < 0).  *retry_after_ns (may be
 * NULL): 0 with 200; with 429 retry_at - now, saturating at INT64_MAX, or -1
 * for never; untouched otherwise.
 *
 * The sharded form is phip_group_peek ("Owner-routed phip_peek" below): every
 * query is answered by the handle that owns its name.  Not here: a PEEK kind
 * inside ordered streams and peeks through the Take batcher.  The reverse
 * question -- which buckets are denied now -- is "Throttled sweep"
 * below. */
#define PHIP_PEEK_NEVER INT64_MIN
typedef struct phip_peek_results { /* any pointer may be NULL */
  uint8_t* status;     /* PHIP_ST_TAKE_OK / _DENIED (| PHIP_ST_ABSENT)          */
  uint64_t* remaining; /* uint64(remaining) as Go returns it                    */
  uint64_t* have;      /* float64 bits, as phip_results.have                    */
  int64_t* retry_at;   /* now, the least later reading that grants, or NEVER    */
  phip_state* state;   /* the state evaluated (absent: zeros, created = now)    */
} phip_peek_results;
int phip_peek(phip_handle* h, const phip_ops* q, const phip_peek_results* res, uint32_t flags);
int phip_peek_eval(const phip_state* s /* NULL: absent */, int64_t now, int64_t freq, int64_t per,
                   uint64_t count, uint64_t* remaining, uint64_t* have, int64_t* retry_at);
int phip_api_peek(phip_handle* h, const uint8_t* name, uint32_t len, const char* rate,
                  uint32_t rate_len, const char* count, uint32_t count_len, int64_t now,
                  char* body, uint32_t* body_len, int64_t* retry_after_ns);

/* Throttled sweep: the buckets a rate denies now, with their retry times.
 * Peek answers for names the caller already has; this answers the reverse
 * question -- which keys are throttled right now, and until when -- for a deny
 * list pushed to a load balancer or edge cache, a dashboard of throttled
 * tenants, a "throttled buckets per class" metric.  It is the export sweep's
 * resumable window walk ("Anti-entropy sweep") with Peek's evaluation as the
 * filter; a caller loops phip_export_throttled until st->done.
 *
 * Rules.  The table stores no rate: a rate arrives with each request
 * (api.go:55-65).  The caller says which rate belongs to which bucket with
 * 1..PHIP_THROTTLE_MAX_RULES rules, name prefix -> (freq, per, count).
 *  - Match.  Rule r matches a name iff len >= prefix_len and the first
 *    prefix_len bytes are equal; prefix_len == 0 matches every name, the empty
 *    one too.  The first matching rule in array order gives the bucket's
 *    query; bytes of `prefix` past prefix_len are ignored.  A bucket that no
 *    rule matches is not reported.  phip_throttle_match is the same function
 *    on the host (no handle, no GPU), the one the kernels call.
 *  - A prefix is at most PHIP_THROTTLE_MAX_PREFIX = 16 bytes: a table record
 *    carries an inline name (up to 22 bytes) whole and the first 16 bytes of a
 *    longer one, so matching never reads the name arena.
 *  - count is used as given, 0 included, as phip_peek uses it.
 *
 * Which buckets.  A record is reported iff it is published, its name is at
 * most PHIP_MAX_NAME_LEN bytes (a 232..255-byte name that came in by datagram
 * is skipped, as the export sweep skips it), a rule matches, and with that
 * rule's (freq, per, count) Take evaluated on a copy of the record's state
 * (step 2 of "Peek") is denied at `now` and also denied at now + min_wait_ns,
 * the sum saturating at INT64_MAX.  With min_wait_ns == 0 the two conditions
 * are one; min_wait_ns > 0 leaves out denials that end within the wait, which
 * are not worth caching.  By Peek's monotonicity the second condition is
 * retry_at > now + min_wait_ns, or never; the contract is the predicate, not
 * that formula.  min_wait_ns < 0 is PHIP_ERR_INVALID.  Unlike the export
 * sweep, a zero-state record is not special: it is evaluated like any other
 * (added == 0 becomes capacity, bucket.go:194-196).
 *
 * Per entry.  Entry i's name is names[offs[i] .. offs[i+1]), offs[0] = 0, the
 * names back to back (an empty name is an entry of no bytes).  retry_at[i] is
 * exactly what phip_peek gives a denied query: the least t > now that grants,
 * or PHIP_PEEK_NEVER; remaining[i] is what the denied TAKE reports; rule[i] is
 * the index of the rule that matched.  All are bit-exact against phip_peek /
 * phip_peek_eval for the same (state, now, rate, count).  Within a call the
 * entries are in slot order.  retry_at, remaining and rule may each be NULL.
 *
 * Bounds, window, cursor, rebuilds: the export sweep's.  A call writes at most
 * max_entries entries and at most names_cap name bytes, cut at a record, and
 * sets *cur to the slot of the first record it did not write, or to the end
 * of the slots it covered.  It reads the slots [cur->slot, cur->slot + W)
 * clipped to the table, W = max(4 * max_entries, PHIP_SWEEP_TILE) rounded up
 * to a multiple of PHIP_SWEEP_TILE, and never the rest.  A cursor of another
 * table layout starts again at slot 0 and the call reports restarted = 1; a
 * zeroed cursor never does.  st->n, st->bytes (= offs[n]: name bytes only),
 * st->slots_scanned and st->done are filled as there.  max_entries == 0 or
 * names_cap < PHIP_MAX_NAME_LEN is PHIP_ERR_INVALID, so every valid call makes
 * progress.
 *
 * Count mode.  PHIP_SWEEP_COUNT with out == NULL: one pass over the whole
 * table; st->n and st->bytes receive what a whole sweep would report, and
 * *cur is left untouched.
 *
 * Pointers.  rules, cur, st and the phip_throttled_out struct are host memory.
 * The five buffers inside it are host memory, or device memory with
 * PHIP_DEVICE_PTRS (no alignment asked beyond each column's own type; every
 * byte of names_cap is budget).  A host-pointer call copies back only what
 * was written.
 *
 * Errors and locking.  n_rules outside 1..PHIP_THROTTLE_MAX_RULES, a
 * prefix_len above PHIP_THROTTLE_MAX_PREFIX, NULL rules / cur / st, a missing
 * out / names / offs outside count mode, or any flag bit other than
 * PHIP_DEVICE_PTRS and PHIP_SWEEP_COUNT is PHIP_ERR_INVALID, with nothing read
 * from the table and nothing written.  The call is serialised with the
 * handle's other calls; a batch queued with PHIP_RECV_ASYNC is finished first,
 * its error is this call's, and the sweep sees its merges.
 *
 * Nothing is written to the handle: table, arena, change set, layout count,
 * the hot directory and phip_len stay as they are.
 *
 * Stated limit.  `created` is local to a node (it is not on the wire), so the
 * list is this node's view.  Not here: rates stored per bucket, prefixes over
 * 16 bytes, a group-wide sweep (each owner's phip_group_handle can be swept
 * meanwhile). */
#define PHIP_THROTTLE_MAX_RULES 8
#define PHIP_THROTTLE_MAX_PREFIX 16
typedef struct phip_throttle_rule { /* 48 bytes */
  uint8_t prefix[PHIP_THROTTLE_MAX_PREFIX];
  uint32_t prefix_len; /* 0..16; 0 matches every name, the empty one too */
  uint32_t reserved;
  int64_t freq, per;   /* Rate{freq, per} */
  uint64_t count;      /* tokens asked for, used as given (as phip_peek) */
} phip_throttle_rule;
typedef struct phip_throttled_out { /* names and offs required outside count mode */
  uint8_t* names;      /* entry i's name is names[offs[i] .. offs[i+1]) */
  uint64_t names_cap;
  uint64_t* offs;      /* max_entries + 1 entries, offs[0] = 0 */
  uint32_t max_entries, reserved;
  int64_t* retry_at;   /* may be NULL */
  uint64_t* remaining; /* may be NULL */
  uint8_t* rule;       /* may be NULL: index of the rule that matched */
} phip_throttled_out;
int phip_export_throttled(phip_handle* h, phip_sweep_cursor* cur, const phip_throttle_rule* rules,
                          uint32_t n_rules, int64_t now, int64_t min_wait_ns,
                          const phip_throttled_out* out, phip_sweep_stats* st, uint32_t flags);
/* host only, no handle: *rule_out = index of the first matching rule, or -1;
 * PHIP_ERR_INVALID for n_rules outside 1..8, a prefix_len over 16, NULL rules
 * or rule_out, or a NULL name with len > 0 */
int phip_throttle_match(const phip_throttle_rule* rules, uint32_t n_rules, const uint8_t* name,
                        uint32_t len, int32_t* rule_out);

/* Top talkers: the k buckets that took the most.
 * The exports above report, in slot order, whatever passes a per-record test.
 * This one answers "who uses the service most": the k qualifying buckets with
 * the largest `taken` (a bucket's lifetime token count, the cluster-wide max
 * after merges), found by a radix select on the device in a few passes over
 * the table instead of a dump and a host sort.
 *
 * Which buckets qualify.  A record qualifies iff it is published, its name is
 * at most PHIP_MAX_NAME_LEN bytes, the prefix matches -- phip_throttle_match's
 * rule for the one prefix of the query: len >= prefix_len and the first
 * prefix_len bytes equal, prefix_len == 0 matches every name, bytes of
 * `prefix` past prefix_len are ignored -- with idle_ns > 0 it is not idle at
 * `now` by phip_evict_idle's rule (idle = now - (created + elapsed), exact,
 * 0 when that is negative, saturating; idle iff idle >= idle_ns), and its
 * decoded `taken` bits t satisfy 0 < t <= 0x7FF0000000000000: positive, +Inf
 * included.  +0.0, -0.0, negatives and NaNs never rank.  On that range the
 * order of the raw bits, the float order and the order of the stored codes are
 * one order.  idle_ns == 0: no idle filter; idle_ns < 0: PHIP_ERR_INVALID.
 * metric selects the ranking key: 0 = taken, PHIP_TOP_SINCE_MARK = taken since
 * the last usage mark ("Windowed top talkers" below), anything else
 * PHIP_ERR_INVALID.
 *
 * Order.  Entries come out by `taken` descending, equal `taken` in ascending
 * slot order.  The list is the first min(k, population) entries of that total
 * order, so on an unchanged table top(k) is exactly the first k entries of
 * top(k') for every k < k'.  Slots follow from the handle's placement seed:
 * which of several buckets tied at the cut are reported depends on that seed
 * (and on the table's layout), and on nothing else.
 *
 * Output.  Entry i's name is names[offs[i] .. offs[i+1]), offs[0] = 0, the
 * names back to back as in phip_throttled_out.  taken[i] (float64 bits) and
 * state[i] are bit-exact copies of the record, decoded as phip_get gives them;
 * each may be NULL.  Only entries [0, n) and offs[0 .. n] are written, nothing
 * past them.
 *
 * Bounds.  k is 1..PHIP_TOP_MAX.  names_cap < PHIP_MAX_NAME_LEN is
 * PHIP_ERR_INVALID.  A list that runs out of name bytes is cut at an entry,
 * from the bottom ranks: it is then the first n entries of the uncut list and
 * st->truncated = 1.
 *
 * Stats.  n and bytes (= offs[n]); population, the buckets that qualified;
 * passes, the kernels of this call that read every slot of the table -- at
 * most 8 (six 12-bit digits of the key, the tie count, the collect), far fewer
 * when the top keys differ in their leading digits.
 *
 * Count mode.  PHIP_SWEEP_COUNT with out == NULL: one pass, st->population
 * only (n and bytes 0).
 *
 * Pointers.  q, st and the phip_top_out struct are host memory.  The buffers
 * in it are host memory, or device memory with PHIP_DEVICE_PTRS (no alignment
 * asked beyond each column's type; every byte of names_cap is budget).  A
 * host-pointer call copies back only what was written.
 *
 * Errors and locking.  k outside 1..PHIP_TOP_MAX, prefix_len over
 * PHIP_THROTTLE_MAX_PREFIX, a metric above PHIP_TOP_SINCE_MARK, idle_ns < 0,
 * NULL q or st, a missing out / names / offs outside count mode (an `out` in
 * count mode), names_cap below one name, or any flag bit other than
 * PHIP_DEVICE_PTRS, PHIP_SWEEP_COUNT and PHIP_TOP_MARK is PHIP_ERR_INVALID,
 * with nothing read from the table and nothing written.  The call is
 * serialised with the handle's other calls; a batch queued with
 * PHIP_RECV_ASYNC is finished first, its error is this call's, and the list
 * sees its merges.
 *
 * Nothing is written to the handle: table, arena, change set, layout count,
 * the hot directory and phip_len stay as they are (PHIP_TOP_MARK rewrites the
 * usage baseline, and nothing else).
 *
 * Stated limits.  Metric 0's `taken` is a lifetime total, not a rate, and two
 * of its lists cannot be diffed into one: a bucket in neither list may have
 * taken the most in between.  "Who took the most since then" is metric
 * PHIP_TOP_SINCE_MARK on a handle that tracks usage.  Not here: metrics above
 * 1, more than one baseline per handle, prefixes over 16 bytes, k above
 * PHIP_TOP_MAX.
 *
 * Windowed top talkers: a usage baseline and the top k since the mark.
 * A handle opened with PHIP_CFG_TRACK_USAGE keeps base[slot], the float64 bits
 * of the bucket's `taken` at the last mark, beside its table (8 bytes a slot).
 * The column starts as zeros, and +0.0 is the baseline of every bucket created
 * after a mark: before any mark, and for such a bucket, "since the mark" is
 * "since the bucket began".  `taken` only rises, and after merges it is the
 * cluster-wide max, so a difference of two readings is cluster-wide usage in
 * between, with nothing to add up across nodes.
 *
 * phip_usage_mark(h, st, 0): one streaming pass.  base becomes the decoded
 * `taken` of every published record and 0 in every other slot.  st (may be
 * NULL): buckets, the published records baselined; active, of those the ones
 * with 0 < taken - base <= +Inf just before the call, names of any length --
 * the population metric 1 would have reported with no prefix and no idle
 * filter, plus the names over PHIP_MAX_NAME_LEN.  flags must be 0; that, and a
 * handle opened without PHIP_CFG_TRACK_USAGE, is PHIP_ERR_INVALID with nothing
 * read or written.  Serialised with the handle's other calls; a batch queued
 * with PHIP_RECV_ASYNC is finished first, and its error is this call's.  A
 * mark writes nothing but the column: table, arena, change set, hot directory,
 * phip_len and the layout count stay, and a sweep cursor taken before it
 * continues without `restarted`.
 *
 * metric = PHIP_TOP_SINCE_MARK.  The key of a record is the bits of d = taken -
 * base, one IEEE-754 double subtraction (round to nearest, denormals kept).  A
 * record ranks iff it passes every test above except the one on `taken`
 * itself, and 0 < bits(d) <= 0x7FF0000000000000: +Inf - finite ranks first;
 * Inf - Inf, a NaN `taken`, a zero and a negative difference never rank.
 * Everything else is metric 0's contract with "key" read for `taken`: the
 * order (key descending, equal keys in ascending slot order), top(k) the head
 * of top(k'), the names_cap cut, the stats, count mode (the population is the
 * buckets active since the mark) and the refusals.  out->taken[i] holds the
 * key bits, the difference; out->state[i] is the record, so its taken is the
 * current total.  phip_top_merge orders whatever the taken column holds, so
 * lists of this metric merge as they are.  On a handle opened without
 * PHIP_CFG_TRACK_USAGE the metric is PHIP_ERR_INVALID, with nothing read.
 *
 * PHIP_TOP_MARK: report and re-mark in one call.  With phip_usage_mark and
 * phip_export_top as two calls, the takes that land between them are in the
 * new baseline and in no list.  With this flag the call marks the whole table
 * (whatever the prefix) right behind its list, under the handle's lock: no op
 * of the handle falls between the two, and successive calls tile time exactly.
 * The mark happens iff the call returns PHIP_OK, truncated or not: a caller
 * who sizes names_cap too small loses the tail of that window.  Allowed with
 * either metric; with PHIP_SWEEP_COUNT, or on a handle that does not track
 * usage, PHIP_ERR_INVALID with nothing touched.
 *
 * Layout changes.  The baseline belongs to the bucket, not the slot: table
 * growth and phip_evict_idle's move (PHIP_EVICT_SHRINK included) carry a
 * surviving bucket's baseline along, an evicted bucket's baseline goes with it
 * (if the bucket comes back it counts from zero, as after a node restart), and
 * phip_restore clears the column (a snapshot does not hold it, and
 * phip_snapshot_bytes does not count it).
 *
 * phip_top_merge (host only, no handle, no GPU): the top k of n_lists lists in
 * phip_export_top's layout, list i holding ns[i] entries -- the members of a
 * shard group, whose tables are disjoint, or replicas of different nodes.
 * `taken` is required in every list and `state` may be NULL (its entries then
 * merge as zero states); of `out`, names, names_cap and offs are required,
 * taken and state may be NULL.  The result is in the same order, by `taken`
 * descending; slots mean nothing across lists, so equal `taken` falls by list
 * index, then by position in the list.  A name present more than once is kept
 * once, with the larger `taken` and that entry's state and place (equal
 * `taken`: the first).  The list is cut at an entry when names_cap runs out.
 * *n_out receives the entries written, offs[0 .. *n_out] their bounds.
 * PHIP_ERR_INVALID for n_lists == 0, k outside 1..PHIP_TOP_MAX, NULL lists /
 * ns / out / n_out / out->names / out->offs, or a list with entries and no
 * names, offs or taken. */
#define PHIP_TOP_MAX 4096          /* largest k */
#define PHIP_TOP_SINCE_MARK 1      /* phip_top_query.metric: taken since the last usage mark */
#define PHIP_TOP_MARK 0x400u       /* phip_export_top: mark the whole table behind the list */
typedef struct phip_top_query {    /* host memory */
  uint8_t prefix[PHIP_THROTTLE_MAX_PREFIX];
  uint32_t prefix_len; /* 0..16; 0 matches every name */
  uint32_t metric;     /* 0 = taken, PHIP_TOP_SINCE_MARK */
  int64_t now, idle_ns;/* idle_ns > 0: skip buckets idle at now; 0: no filter */
  uint32_t k, reserved;/* 1..PHIP_TOP_MAX */
} phip_top_query;
typedef struct phip_top_out {      /* names and offs required outside count mode */
  uint8_t* names;      /* entry i's name is names[offs[i] .. offs[i+1]) */
  uint64_t names_cap;
  uint64_t* offs;      /* k + 1 entries, offs[0] = 0 */
  uint64_t* taken;     /* may be NULL: float64 bits of entry i's taken */
  phip_state* state;   /* may be NULL: the record's state as phip_get gives it */
} phip_top_out;
typedef struct phip_top_stats {
  uint64_t n, bytes;   /* entries written, offs[n] */
  uint64_t population; /* buckets that qualified */
  uint32_t passes;     /* kernels of this call that read every slot of the table */
  uint32_t truncated;  /* 1: names_cap ended the list before min(k, population) */
} phip_top_stats;
int phip_export_top(phip_handle* h, const phip_top_query* q, const phip_top_out* out,
                    phip_top_stats* st, uint32_t flags);
int phip_top_merge(const phip_top_out* lists, const uint64_t* ns, uint32_t n_lists, uint32_t k,
                   const phip_top_out* out, uint64_t* n_out);
typedef struct phip_usage_stats {
  uint64_t buckets;    /* published records baselined by this call */
  uint64_t active;     /* of those, 0 < taken - base <= +Inf just before it */
} phip_usage_stats;
int phip_usage_mark(phip_handle* h, phip_usage_stats* st /* may be NULL */, uint32_t flags);

/* ---- host helpers (no device work) ---- */
/* ParseRate: returns 0 or <0 on error; freq and per receive the values Go
 * returns beside the error (api.go:61 uses them). */
int phip_parse_rate(const char* s, uint32_t len, int64_t* freq, int64_t* per);
/* MarshalBinary: writes 25+len bytes to out (>= 256 bytes), returns the size
 * or PHIP_ERR_NAME_TOO_LARGE. */
int phip_marshal(const uint8_t* name, uint32_t len, const phip_state* s, uint8_t* out);
/* API.takeBucket (api.go:51-86) over this engine: returns the HTTP status
 * code (200/429/400) and writes the response body (<= 64 bytes). */
int phip_api_take(phip_handle* h, const uint8_t* name, uint32_t len, const char* rate,
                  uint32_t rate_len, const char* count, uint32_t count_len, int64_t now,
                  char* body, uint32_t* body_len);

/* ---- request-coalescing Take batcher ----
 * Replaces the per-request GetBucket -> Take -> UpsertBucket of the HTTP
 * handler (api.go:67-74; Bucket.Take bucket.go:186-225) for callers that
 * serve one request per thread (a Go goroutine per HTTP request calling
 * through cgo).  Each call enqueues one Take and blocks until its batch ran:
 * a dispatcher thread closes a batch window_us after the batch's first
 * request arrived, or at max_batch requests, and runs it with
 * phip_apply_mixed (arrival order = op order, so each bucket sees its Takes
 * in the order they were enqueued).  Requests arriving while a batch runs
 * form the next one.  Thread-safe; the handle must not be closed before the
 * batcher. */
typedef struct phip_batcher phip_batcher;
typedef struct phip_batcher_config {
  uint32_t window_us;   /* batch window after its first request (0: dispatch at once)  */
  uint32_t max_batch;   /* requests per batch at most (0: 65536)                       */
} phip_batcher_config;
int phip_batcher_open(phip_handle* h, const phip_batcher_config* cfg, phip_batcher** out);
/* Runs the requests already queued, then stops the dispatcher. */
void phip_batcher_close(phip_batcher* b);
/* GetBucket + Take(now, Rate{freq, per}, count): *remaining and *ok as Go's
 * Take returns them (ok = 1 means HTTP 200, 0 means 429).  *seq (optional)
 * receives the request's arrival number: the requests of a batcher took
 * effect exactly as Go running them one by one in seq order. */
int phip_batcher_take(phip_batcher* b, const uint8_t* name, uint32_t len, int64_t now,
                      int64_t freq, int64_t per, uint64_t count, uint64_t* remaining,
                      uint8_t* ok, uint64_t* seq);
/* API.takeBucket (api.go:51-86) through the batcher: phip_api_take's
 * contract (HTTP status 200/429/400, body <= 64 bytes). */
int phip_batcher_api_take(phip_batcher* b, const uint8_t* name, uint32_t len, const char* rate,
                          uint32_t rate_len, const char* count, uint32_t count_len, int64_t now,
                          char* body, uint32_t* body_len);
/* out[0] batches run, out[1] requests served, out[2] largest batch,
 * out[3] ns spent in phip_apply_mixed, out[4] batches that failed; past
 * those, for a batcher opened with phip_batcher_open_egress (zeros otherwise):
 * out[5] egress batches queued, out[6] datagrams queued, out[7] ns the
 * dispatcher waited for a free egress slot.
 * Returns the number written (<= 8; a caller passing max = 5 sees the first
 * five as before). */
int phip_batcher_stats(phip_batcher* b, uint64_t* out, int max);
/* Everything the reference handler does after GetBucket -> Take ->
 * UpsertBucket (api.go:67-74), from the same batched launch: whether the
 * Take's GetBucket created the bucket (ReplicatedRepo.GetBucket then sends
 * its zero-state incast request, repo.go:96-106: datagram bytes [24, len)
 * with 24 zero bytes in front) and the MarshalBinary datagram of the state
 * right after the Take, which UpsertBucket broadcasts (repo.go:123-158). */
typedef struct phip_take_reply {
  uint64_t remaining;      /* uint64(remaining) as Take returns it (the HTTP body)          */
  uint8_t ok;              /* 1: HTTP 200, 0: 429                                            */
  uint8_t created;         /* this request's GetBucket created the bucket                    */
  uint16_t datagram_len;   /* 25 + len(name); 0 when nothing was taken (HTTP 400)           */
  uint32_t reserved;
  uint64_t seq;            /* arrival number (phip_batcher_take)                             */
  phip_state state;        /* the bucket right after the Take                                */
  uint8_t datagram[PHIP_BUCKET_PACKET_SIZE]; /* MarshalBinary(state) (bucket.go:51-68)       */
} phip_take_reply;
int phip_batcher_take_reply(phip_batcher* b, const uint8_t* name, uint32_t len, int64_t now,
                            int64_t freq, int64_t per, uint64_t count, phip_take_reply* out);
/* API.takeBucket (api.go:51-86) through the batcher, as phip_batcher_api_take,
 * plus *out for the replication it triggers (out->datagram_len = 0 on 400). */
int phip_batcher_api_take_reply(phip_batcher* b, const uint8_t* name, uint32_t len,
                                const char* rate, uint32_t rate_len, const char* count,
                                uint32_t count_len, int64_t now, char* body, uint32_t* body_len,
                                phip_take_reply* out);

/* The batcher with coalesced egress ("Coalesced egress" above): every batch
 * runs through phip_apply_mixed_egress into the next of `egress_slots` pinned
 * host buffers (0: 4), each sized by phip_egress_caps(max_batch,
 * 231 * max_batch, 0), and a batch that produced datagrams (n > 0) is queued
 * for phip_batcher_egress_next.  Batches come out in order, numbered from 0
 * without gaps.  A caller of a take entry point is woken only after its
 * batch's egress is queued, so when a take returns its replication is already
 * with the sender.  The per-request entry points work as with
 * phip_batcher_open, phip_take_reply.datagram included; phip_batcher_open
 * itself is unchanged and produces no egress.
 *
 * Somebody has to drain.  When every slot is queued or handed out the
 * dispatcher waits for phip_batcher_egress_done before it runs the next batch
 * -- the reference's handler waits for its WriteTo calls too -- and the takes
 * of that batch wait with it (phip_batcher_stats out[7] counts the time).
 *
 * phip_batcher_egress_next: 1 with *out filled (bytes / offs as
 * phip_udp_send_batch takes them: datagrams [0, n_incast) are incast
 * requests, [n_incast, n) states; valid until phip_batcher_egress_done(batch)
 * gives the slot back), 0 after timeout_ms without a batch (< 0: no timeout)
 * or on a batcher being closed, < 0 on error (not an egress batcher).
 * phip_batcher_close wakes a blocked phip_batcher_egress_next, which returns 0,
 * and a blocked dispatcher, whose remaining batches then run without egress;
 * batches still queued at close are dropped with the ring, so drain first. */
int phip_batcher_open_egress(phip_handle* h, const phip_batcher_config* cfg,
                             uint32_t egress_slots, phip_batcher** out);
typedef struct phip_egress_batch {
  const uint8_t* bytes;
  const uint64_t* offs;
  uint32_t n, n_incast;
  uint64_t batch;        /* batch number, from 0 */
  uint64_t first_seq;    /* arrival number of its first request */
  uint32_t requests, reserved;
} phip_egress_batch;
int phip_batcher_egress_next(phip_batcher* b, int timeout_ms, phip_egress_batch* out);
int phip_batcher_egress_done(phip_batcher* b, uint64_t batch);

/* ---- batched UDP ingest (command.go's replicator) ----
 * The reference's Receive goroutine reads ONE datagram per iteration into a
 * 256-byte buffer under a 3 s deadline (repo.go:54-73,108-120) and answers
 * each incast with its own WriteTo (repo.go:86-90,160-169).  The batched
 * pipeline is:
 *
 *   phip_ring_acquire      a free pinned host slot (bytes + offs arrays)
 *   phip_udp_recv_batch    recvmmsg straight into that slot
 *   phip_ring_submit       hipMemcpyAsync of the slot on the ring's copy
 *                          stream (returns at once; the next slot can be
 *                          filled while this one is copied and merged)
 *   phip_ring_receive      the handle's stream waits for the copy, then
 *                          phip_receive_datagrams over the device copy;
 *                          results land in host buffers; the slot is freed
 *   phip_incast_replies +  MarshalBinary of the batch's INCAST_REPLY states
 *   phip_udp_send_batch    and one sendmmsg back to their peers
 *
 * Peers are sockaddr_storage records (PHIP_PEER_BYTES each). */
#define PHIP_PEER_BYTES 128

typedef struct phip_ring phip_ring;
/* nslots pinned slots of max_msgs datagrams / max_bytes bytes each (max_bytes
 * >= 256 * max_msgs lets phip_udp_recv_batch fill a slot to max_msgs). */
int phip_ring_open(phip_handle* h, uint32_t nslots, uint32_t max_msgs, uint64_t max_bytes,
                   phip_ring** out);
void phip_ring_close(phip_ring* r);
/* The next slot in ring order, if it is free (PHIP_ERR_BUSY: that slot is
 * still submitted and not yet received).  *bytes / *offs are pinned host
 * arrays of max_bytes and max_msgs + 1 entries; the caller writes datagram i
 * to bytes[offs[i] .. offs[i+1]) with offs[0] = 0. */
int phip_ring_acquire(phip_ring* r, uint32_t* slot, uint8_t** bytes, uint64_t** offs);
/* Start the host->device copy of the slot's first n datagrams. */
int phip_ring_submit(phip_ring* r, uint32_t slot, uint32_t n);
/* ReplicatedRepo.Receive over a submitted slot (phip_receive_datagrams
 * semantics; res holds host pointers) and release the slot.  Slots must be
 * received in the order they were submitted. */
int phip_ring_receive(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                      uint32_t* stop_index);

/* recvmmsg up to max_msgs datagrams from fd: waits up to timeout_ms for the
 * first (a timeout returns PHIP_OK with *n_out = 0, as the Go loop continues
 * on a Timeout error), then takes what is queued without waiting.  Each
 * datagram is cut at PHIP_BUCKET_PACKET_SIZE bytes (Go's read buffer) and
 * packed back to back: datagram i is bytes[offs[i] .. offs[i+1]), offs[0] = 0.
 * peers (optional) receives each sender's address. */
int phip_udp_recv_batch(int fd, uint8_t* bytes, uint64_t cap, uint64_t* offs, uint32_t max_msgs,
                        uint8_t* peers, int timeout_ms, uint32_t* n_out);
/* MarshalBinary (bucket.go:51-68) of reply[i] under datagram i's name for
 * every message whose status is PHIP_ST_INCAST_REPLY, in batch order, packed
 * into out / out_offs (as phip_udp_recv_batch packs); out_peers (optional)
 * receives the matching peers[i]. */
int phip_incast_replies(const uint8_t* bytes, const uint64_t* offs, uint32_t n,
                        const uint8_t* status, const phip_state* reply, const uint8_t* peers,
                        uint8_t* out, uint64_t cap, uint64_t* out_offs, uint8_t* out_peers,
                        uint32_t* n_out);
/* sendmmsg datagrams bytes[offs[i] .. offs[i+1]) for i < n, datagram i to
 * peers + i * peer_stride (stride 0: every datagram to one peer, e.g. an
 * egress batch from phip_export_datagrams; peers NULL: a connected socket). */
int phip_udp_send_batch(int fd, const uint8_t* bytes, const uint64_t* offs, uint32_t n,
                        const uint8_t* peers, uint32_t peer_stride, uint32_t* sent_out);

/* ---- Incast reply egress ----
 * The unicast answers to a batch's incast requests (repo.go:86-90,160-169) as
 * datagrams written on the device, ready for phip_udp_send_batch: the Receive
 * counterpart of "Coalesced egress".  Each call below is the receive call it
 * is named after -- the same statuses, results, table effects, stop rule,
 * errors and checked-offset rule; res may be NULL, and so may any column of
 * it -- and in addition fills rq.  No per-message reply column is needed
 * anywhere: on a large device batch's common path (its dirty buckets run as a
 * sub-batch of a few thousand entries) none exists even inside the library.
 *
 * Which messages.  Exactly those whose status is PHIP_ST_INCAST_REPLY: a zero
 * remote state (Bucket.IsZero compares with ==, so a state of -0.0 fields is a
 * request too) for a bucket that existed and was not zero at that point of the
 * Go loop (repo.go:78-90).  Datagrams are in batch order.
 *
 * Datagram k is out[offs[k] .. offs[k+1]), offs[0] = 0: MarshalBinary
 * (bucket.go:51-68), byte for byte, of the state phip_results.reply[i] holds
 * for that message -- the local state at that message in loop order, not the
 * state after the batch -- under the request's own name; src[k] = i, the
 * message's batch index (src may be NULL).  With caps that do not cut and no
 * name over PHIP_MAX_NAME_LEN, out / offs equal what phip_incast_replies
 * writes from the same call's full status and reply columns, and
 * phip_reply_peers(peers, src, n, ..) its out_peers.
 *
 * Left out and counted.  A reply under a name longer than PHIP_MAX_NAME_LEN
 * (only a datagram brings one in; MarshalBinary refuses it, bucket.go:48) has
 * no datagram: `skipped` counts them over the whole batch.  `replies` is the
 * whole batch's reply count, whatever was written.
 *
 * Bounds.  The first datagrams in batch order that fit max_msgs and the byte
 * budget are written, cut at a record; n < replies - skipped says some were
 * cut, which is not an error (incast is best-effort UDP, and the caller can
 * fetch those buckets with phip_export_datagrams).  max_msgs == 0, out == NULL,
 * offs == NULL or out_cap < PHIP_BUCKET_PACKET_SIZE is PHIP_ERR_INVALID before
 * anything is applied.
 *
 * Pointers.  rq is host memory; out, offs and src follow PHIP_DEVICE_PTRS like
 * every other pointer of the call.  Device buffers follow phip_export_sweep's
 * rules: out 8-byte aligned, out_cap a multiple of 8 and at least
 * PHIP_BUCKET_PACKET_SIZE + 8, the byte budget out_cap - 8; out / offs then go
 * unchanged into a peer handle's phip_receive_datagrams(..., PHIP_DEVICE_PTRS).
 * A host-pointer call copies back only what was written.
 *
 * Stopped batches (a short datagram; a checked device batch's malformed offset
 * entry): the replies of the messages before the stop are written and the out
 * fields valid -- the Go loop had sent them before it returned -- and the
 * return code is the stopped call's (PHIP_ERR_SHORT_BUFFER / PHIP_ERR_INVALID).
 * On every other error the four out fields are zero.  A batch of no messages
 * gives zeros and offs[0] = 0.
 *
 * Flags.  PHIP_RECV_ASYNC is PHIP_ERR_INVALID: a queued batch returns no
 * replies.  PHIP_RECV_CLASSIFY is allowed.  Not covered either:
 * PHIP_OP_RECEIVE ops inside phip_apply_mixed.  The shard group has its own
 * forms ("Group reply egress").  phip_ring_receive_replies is phip_ring_receive with rq's
 * buffers in host memory; res may leave out reply and status.
 * phip_incast_replies stays for callers that hold the full columns. */
typedef struct phip_reply_egress {   /* 56 bytes */
  uint8_t*  out;       /* in:  datagram bytes                                  */
  uint64_t  out_cap;   /* in                                                   */
  uint64_t* offs;      /* in:  max_msgs + 1 entries                            */
  uint32_t* src;       /* in:  max_msgs entries, may be NULL                   */
  uint32_t  max_msgs;  /* in                                                   */
  uint32_t  n;         /* out: datagrams written                               */
  uint32_t  replies;   /* out: messages of the batch with PHIP_ST_INCAST_REPLY */
  uint32_t  skipped;   /* out: of those, names over PHIP_MAX_NAME_LEN          */
  uint64_t  bytes;     /* out: = offs[n]                                       */
} phip_reply_egress;
int phip_receive_soa_replies(phip_handle* h, const phip_msgs* m, int64_t now,
                             const phip_results* res, phip_reply_egress* rq, uint32_t flags);
int phip_receive_datagrams_replies(phip_handle* h, const uint8_t* bytes, const uint64_t* offs,
                                   uint32_t n, int64_t now, const phip_results* res,
                                   uint32_t* stop_index, phip_reply_egress* rq, uint32_t flags);
int phip_ring_receive_replies(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                              uint32_t* stop_index, phip_reply_egress* rq);
/* host only: out_peers[k] = peers[src[k]] (PHIP_PEER_BYTES each), for phip_udp_send_batch */
int phip_reply_peers(const uint8_t* peers, const uint32_t* src, uint32_t n, uint8_t* out_peers);

/* ---- Packed frames ----
 * Between two patrol-hip nodes nothing forces one bucket record per UDP
 * datagram.  A run of back-to-back MarshalBinary records (bucket.go:51-68) is
 * self-delimiting -- byte 24 of a record is its name length -- and every
 * export here writes such a run, every wire receive takes one as (bytes,
 * offs).  A frame is a UDP payload of 1..N whole records: a coarser offsets
 * column over the same bytes.  phip_frame_cuts makes that column for the
 * egress side (phip_udp_send_batch then sends frames, the bytes untouched);
 * phip_unframe recovers the per-record offsets from received frames, and the
 * phip_*receive_frames* calls put it in front of the receive calls.
 *
 * Opt-in per peer.  The reference reads 256 bytes and UnmarshalBinary ignores
 * what follows the name (bucket.go:71-91, repo.go:57,114): a Go peer sees only
 * a frame's first record.  A frame of one record is byte for byte today's
 * datagram, and no datagram call changes.
 *
 * Splitting rule (phip_unframe).  Frame f is bytes[foffs[f] .. foffs[f+1]).
 * Walked from its start: while at least PHIP_BUCKET_FIXED_SIZE bytes are left
 * and 25 + bytes[p+24] fits in what is left, that is one record; whatever is
 * left when that fails, 1 byte or more, is one last record -- malformed by
 * construction, so the receive calls' stop rule (repo.go:70-74) fires there;
 * an empty frame yields one empty record.  Every frame yields at least one
 * record, records are contiguous in frame order: record k is
 * bytes[rec_offs[k] .. rec_offs[k+1]), rec_frame[k] its frame.  One difference
 * from the datagram calls: a datagram's bytes after the name are ignored, a
 * frame's are parsed as further records.
 *
 * Cut rule (phip_frame_cuts).  Records are taken in runs of PHIP_FRAME_TILE; a
 * new frame starts at each run's first record, and inside a run cuts are
 * greedy: a frame takes records while its size stays at most frame_bytes.
 * Records are never split (one longer than frame_bytes is PHIP_ERR_INVALID)
 * and keep their order, so an export's "requests in front" survives.
 *
 * Pointers and flags.  flags is 0 (host pointers) or PHIP_DEVICE_PTRS.  The
 * host forms are plain host walks that touch no device and ignore h (NULL is
 * fine): they run on a machine without a GPU.  With PHIP_DEVICE_PTRS the
 * kernels run on the handle's stream, every array is device memory, and
 * `bytes` is aligned and padded as phip_receive_datagrams demands; the only
 * host wait is the read-back of the count.
 *
 * phip_unframe errors (PHIP_ERR_INVALID, nothing written): frame_bytes outside
 * [PHIP_FRAME_MIN_BYTES, PHIP_FRAME_MAX_BYTES]; a frame longer than
 * frame_bytes or a decreasing entry; in a checked batch (bytes_len != 0) an
 * entry that breaks foffs[f] <= foffs[f+1] <= bytes_len.  The check runs from
 * the offsets alone before any byte is read: nothing is read at a bad entry
 * and no frame is walked, and a walk takes at most frame_bytes / 25 + 1 steps
 * whatever the bytes hold.  n_recs > max_recs is PHIP_ERR_INVALID too:
 * *n_recs_out holds the count needed and rec_offs is unspecified.  rec_offs
 * has max_recs + 1 entries, rec_frame (optional) max_recs.
 *
 * phip_frame_cuts: frame_offs has max_frames + 1 entries, of which
 * n_frames + 1 are written, a subset of offs; frame_first (optional) receives
 * each frame's first record.  n = 0 gives 0 frames and frame_offs[0] =
 * offs[0]; n_frames > max_frames is PHIP_ERR_INVALID with the count needed in
 * *n_frames_out.
 *
 * One-call ingest.  phip_receive_frames / phip_receive_frames_replies are
 * phip_unframe followed by phip_receive_datagrams / _replies over the records
 * (on the same stream for device pointers): the same statuses, results, table
 * effects, stop rule and reply egress, with max_recs the capacity of the
 * result columns.  *stop_index and the reply egress's src[] are record
 * indices; rec_frame (optional, max_recs entries) maps them to frames, and
 * phip_frame_reply_peers to the senders.  An unframe error, n_recs > max_recs
 * included, merges nothing.  The ring forms run over a slot that was filled
 * with frames (offs = frame offsets, phip_ring_submit(slot, n_frames)
 * unchanged; the ring is opened with max_msgs = frames and max_bytes >=
 * frame_bytes * frames; res, rec_frame and rq's buffers are host memory). */
#define PHIP_FRAME_MIN_BYTES     256     /* any record fits */
#define PHIP_FRAME_DEFAULT_BYTES 1472    /* 1500 - 20 - 8 */
#define PHIP_FRAME_MAX_BYTES     65507
#define PHIP_FRAME_TILE          4096    /* records: a frame never spans a tile boundary */
int phip_unframe(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs, uint32_t n_frames,
                 uint64_t bytes_len, uint32_t frame_bytes, uint64_t* rec_offs,
                 uint32_t* rec_frame /* optional */, uint32_t max_recs, uint32_t* n_recs_out,
                 uint32_t flags);
int phip_frame_cuts(phip_handle* h, const uint64_t* offs, uint32_t n, uint32_t frame_bytes,
                    uint64_t* frame_offs, uint32_t* frame_first /* optional */,
                    uint32_t max_frames, uint32_t* n_frames_out, uint32_t flags);
int phip_receive_frames(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs,
                        uint32_t n_frames, int64_t now, const phip_results* res,
                        uint32_t* stop_index, uint32_t frame_bytes,
                        uint32_t* rec_frame /* optional */, uint32_t max_recs,
                        uint32_t* n_recs_out, uint32_t flags);
int phip_receive_frames_replies(phip_handle* h, const uint8_t* bytes, const uint64_t* foffs,
                                uint32_t n_frames, int64_t now, const phip_results* res,
                                uint32_t* stop_index, phip_reply_egress* rq, uint32_t frame_bytes,
                                uint32_t* rec_frame /* optional */, uint32_t max_recs,
                                uint32_t* n_recs_out, uint32_t flags);
int phip_ring_receive_frames(phip_ring* r, uint32_t slot, int64_t now, const phip_results* res,
                             uint32_t frame_bytes, uint32_t* rec_frame /* optional */,
                             uint32_t max_recs, uint32_t* n_recs_out, uint32_t* stop_index);
int phip_ring_receive_frames_replies(phip_ring* r, uint32_t slot, int64_t now,
                                     const phip_results* res, uint32_t frame_bytes,
                                     uint32_t* rec_frame /* optional */, uint32_t max_recs,
                                     uint32_t* n_recs_out, uint32_t* stop_index,
                                     phip_reply_egress* rq);
/* host only: phip_udp_recv_batch with windows of frame_bytes instead of
 * PHIP_BUCKET_PACKET_SIZE -- a longer datagram is cut to frame_bytes -- so that
 * frame f is bytes[foffs[f] .. foffs[f+1]), foffs[0] = 0; frame_bytes outside
 * [PHIP_FRAME_MIN_BYTES, PHIP_FRAME_MAX_BYTES] is PHIP_ERR_INVALID. */
int phip_udp_recv_frames(int fd, uint8_t* bytes, uint64_t cap, uint64_t* foffs,
                         uint32_t max_frames, uint32_t frame_bytes, uint8_t* peers, int timeout_ms,
                         uint32_t* n_out);
/* host only: out_peers[k] = peers[rec_frame[src[k]]] (PHIP_PEER_BYTES each): the
 * senders of a frames call's reply datagrams, peers by frame */
int phip_frame_reply_peers(const uint8_t* peers, const uint32_t* rec_frame, const uint32_t* src,
                           uint32_t n, uint8_t* out_peers);

/* ---- shard layer ---- */
/* FNV-1a 64 of each name (the table's probe key; also the shard map:
 * owner = ((hash >> 32) * world) >> 32).  Host pointers need no GPU (h may be
 * NULL); with PHIP_DEVICE_PTRS the hashes are computed on h's GPU. */
int phip_hash_names(phip_handle* h, const uint8_t* names, const uint32_t* name_offs, uint32_t n,
                    uint64_t* out, uint32_t flags);

/* Owner routing, the exchange step of a sharded merge: the n
 * decoded messages of m are stable-partitioned by owner = ((FNV-1a(name) >>
 * 32) * world) >> 32 into owner-major send buffers (send_* have n entries,
 * send_names holds every name byte; names are packed back to back, so
 * send_lens carries their lengths).  counts[o] / name_bytes[o] (world
 * entries, device memory) receive each owner's message and byte counts: the
 * splits of the all-to-all that moves the segments to their owners.  Device
 * pointers only; world <= 64.
 *
 * With PHIP_ROUTE_COMBINE (SURVEY §8e "sender-side combine"), a batch of
 * >= 2^20 messages with no incast and no -0.0 field has the messages of its
 * hottest names (a sampled directory of <= 512 short names) max-combined
 * per workgroup: each workgroup sends one message per hot name it saw,
 * carrying the field-wise maxima (NaN for a float field no message of the
 * group raised), after its other messages.  Merging that message equals
 * merging the ones it replaces (merges commute in that domain); messages
 * whose three fields are all <= 0 or NaN are never combined, so a combined
 * message is never an incast.  counts / name_bytes then describe the
 * combined buffers (never more than without the flag).  A dirty or smaller
 * batch is packed exactly as without the flag. */
int phip_route_pack(phip_handle* h, const phip_msgs* m, uint32_t world, uint8_t* send_names,
                    uint32_t* send_lens, uint64_t* send_added, uint64_t* send_taken,
                    int64_t* send_elapsed, uint64_t* counts, uint64_t* name_bytes,
                    uint32_t flags);

/* A batch of raw wire datagrams (MarshalBinary, bucket.go:51-68) in device
 * memory: datagram i is bytes[offs[i] .. offs[i+1]).  32 bytes. */
typedef struct phip_wire {
  uint32_t n;
  uint32_t reserved;
  const uint8_t* bytes;   /* 8-byte aligned, readable to the next 8-byte boundary past offs[n] */
  const uint64_t* offs;   /* n+1 entries */
  uint64_t bytes_len;     /* 0: offsets trusted, as phip_receive_datagrams(PHIP_DEVICE_PTRS) trusts them */
} phip_wire;

/* phip_route_pack read straight from the wire: the same stable owner
 * partition, into the same owner-major send buffers with the same counts /
 * name_bytes, of the datagrams of w as they arrived (the name at offs[i] + 25
 * with its length byte, added / taken / elapsed from the big-endian header,
 * bucket.go:59-64); no decoded copy is written.  The field bits travel
 * unchanged (-0.0, NaN payloads, zero states); bytes after the name are
 * ignored (bucket.go:78-87).  send_* need n entries, send_names
 * offs[n] - offs[0] - 25 * n bytes.  Device pointers only; world <= 64;
 * PHIP_ROUTE_COMBINE as for phip_route_pack (the directory is sampled from the
 * datagrams, the count pass classifies from the header fields).
 *
 * Stop rule (the Receive loop, repo.go:70-74, returns at the first datagram
 * UnmarshalBinary rejects): only the datagrams before the first malformed one
 * (size < 25, or a length byte larger than what is left of the datagram) are
 * packed.  *stop (host memory, optional) receives that index, or n; when one
 * was found the call returns PHIP_ERR_SHORT_BUFFER with [0, stop) packed and
 * counts / name_bytes describing them.  A checked batch (w->bytes_len != 0)
 * with an entry that is not offs[i] <= offs[i+1] <= bytes_len is
 * PHIP_ERR_INVALID: nothing is packed, nothing is read at that entry.  Any
 * flag besides PHIP_DEVICE_PTRS and PHIP_ROUTE_COMBINE is PHIP_ERR_INVALID. */
int phip_route_pack_datagrams(phip_handle* h, const phip_wire* w, uint32_t world,
                              uint8_t* send_names, uint32_t* send_lens, uint64_t* send_added,
                              uint64_t* send_taken, int64_t* send_elapsed, uint64_t* counts,
                              uint64_t* name_bytes, uint32_t* stop, uint32_t flags);

/* Stable owner partition of an op stream (device pointers only, world <= 64):
 * op j of the send buffers is op send_src[j] of `ops`; owner-major, each owner's
 * ops in their batch order.  x0/x1/x2 carry the op's three operands by kind:
 * TAKE freq/per/count, RECEIVE and UPSERT added/taken/elapsed (bit patterns).
 * A NULL operand column of `ops` reads as zeros.  counts / name_bytes as
 * phip_route_pack.  No combining: ordered ops never combine.
 * The send_* columns have ops->n entries, send_names holds every name byte.
 * flags must be exactly PHIP_DEVICE_PTRS (PHIP_ROUTE_COMBINE included, any
 * other bit is PHIP_ERR_INVALID).  A checked batch (ops->names_len != 0) with
 * a malformed offset entry is PHIP_ERR_INVALID and nothing is packed.  The
 * `kind` values of a device batch are the producer's to guarantee, as for
 * phip_apply_mixed.
 * The query pack (phip_group_peek's): with ops->kind and send_kind both NULL
 * the batch is a batch of peek queries: no kind column is read or written,
 * x0/x1/x2 are always freq/per/count, and everything else is as above.  One
 * of the two NULL alone is PHIP_ERR_INVALID. */
int phip_route_pack_ops(phip_handle* h, const phip_ops* ops, uint32_t world,
                        uint8_t* send_names, uint32_t* send_lens, uint8_t* send_kind,
                        int64_t* send_now, uint64_t* send_x0, uint64_t* send_x1,
                        uint64_t* send_x2, uint32_t* send_src,
                        uint64_t* counts, uint64_t* name_bytes, uint32_t flags);

/* Anti-entropy over simulated replicas (BASELINE configs[4]).  `replicas`
 * holds nrep replicas of nbuckets buckets, each as three int64 planes
 * [r][0..2][i]: E codes (the order-preserving key of the engine, mirrored by
 * patrol_amd.shard.e_encode) of added and taken, then elapsed ns.  Device
 * pointers only (flags must include PHIP_DEVICE_PTRS).
 * phip_ae_local_max writes out[3][nbuckets], the field-wise join of the local
 * replicas in signed form (E ^ 2^63 for the float planes; a NaN replica value
 * never wins, as Go's `<` never adopts one), ready for an RCCL all-reduce(MAX)
 * across GPUs.  phip_ae_apply then sets every local replica to
 * max(own, joined): Bucket.Merge (bucket.go:240-263) of every replica into
 * every other one, a replica's own NaN sticking. */
int phip_ae_local_max(phip_handle* h, const int64_t* replicas, uint32_t nrep, uint64_t nbuckets,
                      int64_t* out, uint32_t flags);
int phip_ae_apply(phip_handle* h, int64_t* replicas, uint32_t nrep, uint64_t nbuckets,
                  const int64_t* joined, uint32_t flags);
/* The join of one GPU's replicas with no exchange: phip_ae_local_max then
 * phip_ae_apply in one pass (each field read once, written only where the
 * join raises it).  What phip_group_anti_entropy runs in a world of one. */
int phip_ae_join(phip_handle* h, int64_t* replicas, uint32_t nrep, uint64_t nbuckets,
                 uint32_t flags);

/* ---- shard group: owner routing and anti-entropy over RCCL ----
 * A group is the set of GPUs the buckets are hash-sharded over (owner =
 * ((FNV-1a(name) >> 32) * world) >> 32), each GPU one table (a phip_handle)
 * and one rank of an RCCL communicator (xGMI between the GPUs of a node).
 * It replaces the single-table Receive loop (repo.go:54-92) of one node by a
 * sharded one, with no Python or torch on the path:
 *   - phip_group_open_all: one process driving n GPUs (ncclCommInitAll); the
 *     group opens and owns a handle per GPU (cfg->device is ignored).  A
 *     device listed more than once (all entries the same device) gives n
 *     shards on that one GPU, which exchange by device copies instead of
 *     RCCL (RCCL takes one rank per device): the same packing, segments and
 *     merge order, to rehearse an n-GPU group on one;
 *   - phip_group_open_rank: one process per GPU (ncclCommInitRank) around the
 *     caller's handle; rank 0 makes the id with phip_group_unique_id and the
 *     caller hands it to every rank by its own means.
 * Calls taking one argument per local member (index i = local member i) run
 * the members concurrently, one host thread each. */
#define PHIP_GROUP_ID_BYTES 128
typedef struct phip_group phip_group;
int phip_group_unique_id(uint8_t* id /* PHIP_GROUP_ID_BYTES */);
int phip_group_open_all(const phip_config* cfg, const int32_t* devices, uint32_t n,
                        phip_group** out);
int phip_group_open_rank(phip_handle* h, const uint8_t* id, uint32_t nranks, uint32_t rank,
                         phip_group** out);
/* Destroys the communicators, and the handles phip_group_open_all opened. */
void phip_group_close(phip_group* g);
const char* phip_group_last_error(const phip_group* g);
uint32_t phip_group_world(const phip_group* g);
uint32_t phip_group_local(const phip_group* g);          /* local members */
phip_handle* phip_group_handle(phip_group* g, uint32_t i);
/* Owner-routed Receive (the C4 step): batches[i] (device pointers on member
 * i's GPU, as phip_receive_soa takes them) are the messages that arrived at
 * member i, addressed to buckets of every shard.  Each member packs its batch
 * by owner (phip_route_pack; PHIP_ROUTE_COMBINE max-combines a clean batch's
 * hot names at the sender), the members exchange the packed segments (one
 * all-to-all of the split sizes, then grouped send/recv per column), and
 * every owner merges what it received (phip_receive_soa, `now` for buckets
 * it creates).  The pack, the exchange and the merge are pipelined by chunks
 * of 2^24 messages (while chunk k travels, the pack of chunk k+1 and the
 * owner's merge of chunk k-1 run); an owner merges chunk by chunk (one
 * phip_receive_soa each), sources in rank order within a chunk, every
 * source's messages in their order (as peers' datagrams interleave in
 * Patrol: per-bucket order from one source is kept).  Every member runs the
 * longest batch's number of rounds (a shorter batch sends empty chunks).  sent[i] /
 * merged[i] (optional) receive the messages member i sent after the combine
 * and merged.  A world of one (without PHIP_GROUP_RCCL_SELF) has nothing to
 * route: the batch is merged as it came, PHIP_ROUTE_COMBINE is ignored (the
 * fast path's hot directory does what the combine would) and sent / merged
 * are the batch's raw message count.
 *
 * Checked batches (phip_msgs.names_len != 0): every local member's offset
 * column is checked in full (one pass, the rule of phip_msgs) before any of
 * its chunks is packed.  If any local batch holds a malformed entry, none of
 * this process's batches is applied -- in a world of one included, where
 * phip_receive_soa alone would apply the messages before it -- the call
 * returns PHIP_ERR_INVALID and phip_group_last_error names the member and the
 * message.  The process still takes part in the exchange, with empty batches
 * (sent[i] = 0; merged[i] counts what its peers sent it), so the other ranks
 * of a multi-process group do not wait for it.  No name of a malformed entry
 * is hashed or copied.  With names_len == 0 the offsets are trusted. */
int phip_group_receive(phip_group* g, const phip_msgs* batches, int64_t now, uint64_t* sent,
                       uint64_t* merged, uint32_t flags);
/* Owner-routed Receive from the wire: phip_group_receive over what a Patrol
 * peer actually sends.  batches[i] holds the raw datagrams that arrived at
 * member i (device memory of its GPU, e.g. a ring slot's copy); each member
 * packs them by owner in place (phip_route_pack_datagrams), and the exchange
 * and the owner's merge are phip_group_receive's in every respect: chunks of
 * 2^24 datagrams (4096 with PHIP_GROUP_SMALL_CHUNKS), an owner merging chunk
 * by chunk with the sources in rank order, PHIP_ROUTE_COMBINE,
 * PHIP_GROUP_RCCL_SELF, shared-device groups, every member running the
 * longest batch's number of rounds.
 *
 * Stop rule (repo.go:70-74).  One pre-pass per member over its whole batch
 * (offsets and length bytes only) finds stop_i, the first malformed datagram
 * (size < 25 or a length byte larger than what is left), before any chunk is
 * packed.  Member i packs datagrams [0, stop_i), its round count comes from
 * stop_i, and nothing at or past stop_i is hashed, copied or sent;
 * stopped[i] (optional, one per local member) receives stop_i (n when there
 * is none).  If any local member stopped, the call returns
 * PHIP_ERR_SHORT_BUFFER after everything before the stops was exchanged and
 * merged, and phip_group_last_error names the first such member and its
 * index; the peers never wait.
 *
 * Checked batches (bytes_len != 0): the same pre-pass checks offs[i] <=
 * offs[i+1] <= bytes_len; a violation is PHIP_ERR_INVALID under
 * phip_group_receive's rule (none of this process's batches is applied, the
 * process still runs the rounds with empty batches, stopped[] is 0), and
 * nothing is read at the bad entry.
 *
 * A chunk's send buffers are sized from the datagram offsets at the chunk's
 * boundaries (the sum of size - 25: an upper bound, trailing bytes count).
 * A world of one without PHIP_GROUP_RCCL_SELF has nothing to route: datagrams
 * [0, stop) go to the handle's own wire path (phip_receive_datagrams), sent =
 * merged = stop, and PHIP_ROUTE_COMBINE is ignored.
 *
 * Flags: PHIP_DEVICE_PTRS is required; PHIP_ROUTE_COMBINE,
 * PHIP_GROUP_RCCL_SELF and PHIP_GROUP_SMALL_CHUNKS are the others; any other
 * bit is PHIP_ERR_INVALID.
 *
 * An incast request (the all-zero state) routed this way is merged at its
 * owner (the bucket is created); its answer comes from the replies form,
 * phip_group_receive_datagrams_replies ("Group reply egress").  There is no
 * batcher over the group. */
int phip_group_receive_datagrams(phip_group* g, const phip_wire* batches, int64_t now,
                                 uint64_t* sent, uint64_t* merged,
                                 uint32_t* stopped /* per member */, uint32_t flags);
/* The socket edge of a sharded node (the Receive goroutine, repo.go:54-92,
 * over one ring per member): phip_group_receive_datagrams over the device
 * copies of one submitted slot per local member.  rings[i] was opened on
 * phip_group_handle(g, i) (a ring of any other handle is PHIP_ERR_INVALID;
 * NULL is an empty batch for member i) and slots[i] must be that ring's next
 * submitted slot, else PHIP_ERR_BUSY as phip_ring_receive reports it; a
 * refused call leaves every slot submitted.  Member i's streams wait for its
 * slot's copy, not the host.  A slot is freed only after the member's pack and
 * exchange streams have finished reading it, after an error too, once they
 * have drained.  The one-launch small-slot shortcut of phip_ring_receive does
 * not apply.  sent, merged, stopped, flags and the return value are
 * phip_group_receive_datagrams' (the slots' offsets were checked at submit). */
int phip_group_ring_receive(phip_group* g, phip_ring* const* rings, const uint32_t* slots,
                            int64_t now, uint64_t* sent, uint64_t* merged, uint32_t* stopped,
                            uint32_t flags);
/* ---- Group reply egress ----
 * The shard group's answers to incast requests (repo.go:86-90,160-169): the
 * other half of the protocol for a sharded node.  Each of the three calls
 * below is the group receive call it is named after -- the same tables, sent /
 * merged / stopped, stop rule, checked-offset rule, flags and return codes --
 * and in addition fills rq[i] (a phip_reply_egress, "Incast reply egress")
 * for every local member i with the answers to the requests that arrived in
 * member i's batch, wherever their buckets live.
 *
 * Which messages.  Exactly the messages of member i's batch whose Receive at
 * their owner has status PHIP_ST_INCAST_REPLY, in the order the group defines:
 * a bucket sees its messages in the order (round, source rank, index in the
 * source's batch), and an answer carries the bucket's state at that point,
 * not the state after the call.
 *
 * Layout.  Datagram k is out[offs[k] .. offs[k+1]), offs[0] = 0: MarshalBinary
 * (bucket.go:51-68), byte for byte, of that state under the request's own
 * name.  src[k] is the message's index in member i's batch (src may be NULL),
 * so phip_reply_peers(peers_i, src, n, ..) works unchanged.  Datagrams are in
 * batch order across all rounds and all owners.
 *
 * Bounds are phip_reply_egress': the first datagrams in batch order that fit
 * max_msgs and the byte budget are written, cut at a record.  max_msgs == 0, a
 * NULL out / offs or an out_cap below one datagram in any rq[i], or a NULL
 * rq, is PHIP_ERR_INVALID before anything of any member is applied.
 *
 * Counters.  They differ from the single-handle form:
 *   n        datagrams written;
 *   replies  the answers that came back for member i's requests, whatever the
 *            caps let through: n < replies says some were cut;
 *   skipped  counted where it is known: the answers member i left out AS AN
 *            OWNER because the name is over PHIP_MAX_NAME_LEN, whoever asked
 *            (they never travel, so `replies` of the asking member excludes
 *            them);
 *   bytes    = offs[n].
 * A world of one without PHIP_GROUP_RCCL_SELF has nothing to route: the batch
 * goes to phip_receive_datagrams_replies / phip_receive_soa_replies, and its
 * counters are reported in the same terms (replies excludes skipped).
 *
 * Pointers.  phip_group_receive_datagrams_replies and
 * phip_group_receive_replies require PHIP_DEVICE_PTRS; out / offs / src are
 * device memory of member i's GPU under phip_export_sweep's rules (8-byte
 * aligned, out_cap a multiple of 8 and at least PHIP_BUCKET_PACKET_SIZE + 8,
 * the byte budget out_cap - 8).  phip_group_ring_receive_replies takes host
 * buffers in rq, as phip_ring_receive_replies does, and copies back only
 * what was written; its byte budget is out_cap rounded down to a multiple of
 * 8.
 *
 * Stops and errors.  A member stopped at a malformed datagram: the answers to
 * its requests before the stop are returned, the out fields are valid and the
 * call returns PHIP_ERR_SHORT_BUFFER as phip_group_receive_datagrams does.  A
 * refused checked batch, or any other error: the four out fields of every
 * local rq are zero.
 *
 * Flags: the receive call's own set (phip_group_receive_replies refuses
 * unknown bits too).  PHIP_ROUTE_COMBINE is accepted: a pack that combined is
 * a clean pack and holds no request (a zero state never combines), and a
 * chunk that holds a request packs plain.
 *
 * How.  Every member counts the zero-state messages of each chunk it packs
 * (one pass over the replica fields) and sends the count with the split
 * sizes; a round in which every count is 0 runs exactly the path of the call
 * without replies, and no return exchange.  In a round with requests every
 * owner merges its chunk with phip_receive_soa_replies into buffers sized from
 * the requests it can have received (sum over sources p of min(zero states of
 * p, messages p sent here)), and only the answers travel back: their
 * per-source counts as split sizes, then lengths, bytes and positions along
 * that plan.  The source turns positions into batch indices, sorts the
 * round's answers by index and appends what fits; once a round is cut, later
 * rounds only count.  Such a round finishes before the next round's exchange
 * starts.
 *
 * Out of scope: PHIP_RECV_ASYNC with replies, answers to PHIP_OP_RECEIVE ops
 * inside phip_apply_mixed (its reply column stays), and a batcher over the
 * group. */
int phip_group_receive_datagrams_replies(phip_group* g, const phip_wire* batches, int64_t now,
                                         uint64_t* sent, uint64_t* merged, uint32_t* stopped,
                                         phip_reply_egress* rq /* one per local member */,
                                         uint32_t flags);
int phip_group_receive_replies(phip_group* g, const phip_msgs* batches, int64_t now,
                               uint64_t* sent, uint64_t* merged,
                               phip_reply_egress* rq /* one per local member */, uint32_t flags);
int phip_group_ring_receive_replies(phip_group* g, phip_ring* const* rings, const uint32_t* slots,
                                    int64_t now, uint64_t* sent, uint64_t* merged,
                                    uint32_t* stopped, phip_reply_egress* rq, uint32_t flags);
/* The last *_replies call of member i: out[0] rounds run, out[1] rounds that
 * ran a return exchange, out[2] the request bound the member received as an
 * owner, summed over rounds, out[3] the answers it wrote as an owner.
 * Returns the number written (<= 4). */
int phip_group_reply_stats(phip_group* g, uint32_t i, uint64_t* out, int max);
/* Owner-routed phip_apply_mixed: batches[i] / results[i] belong to local member i
 * (device memory of its GPU; any results pointer may be NULL, results itself
 * too).  The sharded form of POST /take (api.go:51-86): an op that arrived at
 * member i for a bucket of member j is applied at j, in order, and its result
 * comes back to i.
 *
 * Order rule.  The call runs K rounds, K the largest ceil(n / chunk) over the
 * members of the group; chunk is 2^24, or 4096 with PHIP_GROUP_SMALL_CHUNKS
 * (phip_group_receive's constants).  In round k every member packs ops
 * [k * chunk, (k + 1) * chunk) of its batch by owner (phip_route_pack_ops; a
 * member whose batch has ended sends an empty round), the segments travel to
 * their owners, and every owner applies what it received with ONE
 * phip_apply_mixed: sources in rank order, each source's round-k ops in their
 * index order.  A bucket's ops therefore take effect in the order
 *     (round, source rank, index in the source's batch);
 * buckets are independent, so the whole call equals the Go code run over all
 * ops sorted by that key.  Ordered ops never combine.
 *
 * Results.  results[i] entry j is the result of op j of batches[i]: status
 * (with PHIP_ST_CREATED), remaining, have and reply, each exactly what
 * phip_apply_mixed reports for that op at its owner.  All four columns always
 * return over the exchange (49 bytes per op: the members of a multi-process
 * group cannot see each other's NULL pointers); they come back in send order
 * and the source scatters them to the ops' places, skipping a column the
 * caller passed as NULL.  sent[i] / applied[i] (optional) receive the ops
 * member i sent and the ops it applied as an owner.
 *
 * Flags.  PHIP_DEVICE_PTRS is required; PHIP_GROUP_RCCL_SELF and
 * PHIP_GROUP_SMALL_CHUNKS as for phip_group_receive; any other bit
 * (PHIP_ROUTE_COMBINE included) is PHIP_ERR_INVALID.  A world of one without
 * PHIP_GROUP_RCCL_SELF has nothing to route: the batch goes straight to
 * phip_apply_mixed and the results straight into the caller's buffers.
 *
 * Checked batches (phip_ops.names_len != 0): phip_group_receive's rule.
 * Every local batch's offset column is checked in full before any pack; if
 * any holds a malformed entry, none of this process's batches is applied, the
 * process still runs every round with empty batches (so peers do not wait),
 * the call returns PHIP_ERR_INVALID and phip_group_last_error names the
 * member and the op.  A device batch's `kind` values are the producer's to
 * guarantee, as for phip_apply_mixed.
 *
 * Errors follow phip_group_receive: a failing member releases the call's
 * barriers and its error is the call's.  Every status column the caller
 * passed is zeroed first, so an op that was not applied (a failed call, a
 * rejected batch) reports status 0, which no applied op has. */
int phip_group_apply_mixed(phip_group* g, const phip_ops* batches,
                           const phip_results* results, uint64_t* sent,
                           uint64_t* applied, uint32_t flags);
/* Owner-routed phip_peek: batches[i] / results[i] belong to local member i
 * (device memory of its GPU; any results pointer may be NULL, results itself
 * too).  The sharded form of a read-only quota query (X-RateLimit-Remaining,
 * Retry-After, a per-user and a per-org limit checked before taking from
 * either): a query that arrived at member i for a bucket of member j is
 * evaluated at j, and its answer comes back to i.
 *
 * Queries.  Of each batch the call reads what phip_peek reads: n, names,
 * name_offs, names_len, now, freq, per and count.  names, name_offs and now
 * are required when n != 0; a NULL freq, per or count column reads as zeros.
 * kind, added, taken and elapsed are ignored and may be NULL (kind is never
 * read).
 *
 * Results.  results[i] entry j is exactly what phip_peek reports for query j
 * of batches[i] on the handle that owns its name (the owner of a name among w
 * shards: phip_route_pack): status, with PHIP_ST_ABSENT or-ed in when the
 * owner does not hold the bucket, remaining, have, retry_at, and state under
 * PHIP_GROUP_PEEK_STATE.  An absent bucket is evaluated with created = the
 * query's own now, as on one handle.  All n entries of every column passed
 * are written and nothing outside them ("Result columns" at phip_results).
 *
 * Nothing is written on any member: tables, arenas, change sets, layout
 * counts, hot directories and phip_len stay as they are.  Each owner's step
 * is one phip_peek with PHIP_DEVICE_PTRS on its handle, so "Peek" item 4
 * holds per member (a batch queued with PHIP_RECV_ASYNC is finished first).
 *
 * Rounds.  Queries are read-only, so their order cannot show and there is no
 * order rule.  The call still runs phip_group_apply_mixed's rounds: K is the
 * largest ceil(n / chunk) over the members of the group, chunk is 2^24, or
 * 4096 with PHIP_GROUP_SMALL_CHUNKS, and a member whose batch has ended sends
 * empty rounds.  The rounds bound the scratch buffers and keep every member's
 * collective calls alike; they run one after another on the handle's stream.
 *
 * What travels.  Forward, per query: its name bytes, their length, now and
 * the three operand words (no kind byte).  Back: status, remaining, have and
 * retry_at, 25 bytes a query, always (the members of a multi-process group
 * cannot see each other's NULL pointers).  The 32-byte state column returns
 * only under PHIP_GROUP_PEEK_STATE, which every process of the group must
 * pass alike; a non-NULL results[i].state without the flag is
 * PHIP_ERR_INVALID before any exchange, and with the flag a NULL state
 * pointer is skipped at the scatter, as any column the caller passed as NULL.
 * sent[i] / answered[i] (optional) receive the queries member i sent and the
 * queries it answered as an owner.
 *
 * Flags.  PHIP_DEVICE_PTRS is required; PHIP_GROUP_RCCL_SELF and
 * PHIP_GROUP_SMALL_CHUNKS as for phip_group_receive, PHIP_GROUP_PEEK_STATE as
 * above; any other bit is PHIP_ERR_INVALID, with nothing exchanged and the
 * result columns untouched.  A world of one without PHIP_GROUP_RCCL_SELF has
 * nothing to route: the batch goes straight to phip_peek with the caller's
 * buffers.
 *
 * Checked batches (phip_ops.names_len != 0), errors, the barriers of a
 * shared-device group and phip_group_last_error: phip_group_apply_mixed's
 * rules.  Every local batch's offset column is checked in full before any
 * pack; if any holds a malformed entry, the process still runs every round
 * with empty batches (so peers do not wait), the call returns
 * PHIP_ERR_INVALID and phip_group_last_error names the member and the query.
 * Every status column the caller passed is zeroed first, so a query that was
 * not answered (a failed call, a rejected batch) reports status 0, which no
 * answered query has. */
int phip_group_peek(phip_group* g, const phip_ops* batches /* one per local member */,
                    const phip_peek_results* results /* one per local member, may be NULL */,
                    uint64_t* sent, uint64_t* answered, uint32_t flags);
/* Anti-entropy round over simulated replicas (BASELINE configs[4]):
 * replicas[i] holds member i's nrep replicas in phip_ae_local_max's layout
 * (device memory).  Local join (phip_ae_local_max), RCCL all-reduce(MAX) of
 * the [3, nbuckets] join across the group, phip_ae_apply: afterwards every
 * replica of every member is the CvRDT join of all of them. */
int phip_group_anti_entropy(phip_group* g, int64_t* const* replicas, uint32_t nrep,
                            uint64_t nbuckets, uint32_t flags);
/* phip_evict_idle on every local member, concurrently (one host thread
 * each).  Eviction is local per shard, so there is no exchange: each member
 * sweeps its own table by the same rule.  out (optional) receives one record
 * per local member. */
int phip_group_evict_idle(phip_group* g, int64_t now, int64_t idle_ns, uint64_t min_evict,
                          phip_evict_stats* out /* one per local member, may be NULL */,
                          uint32_t flags);
/* Stage timing of the group's calls (off by default): with it on, every
 * later phip_group_receive / phip_group_anti_entropy records HIP events
 * around each chunk's work on the stream it runs on, and
 * phip_group_stage_ms reads member i's busy time of the last call per stage
 * (the sum over its chunks): ms[0] pack (phip_route_pack; the local join of
 * an anti-entropy round), ms[1] exchange (split sizes and segments over RCCL
 * or device copies; the all-reduce), ms[2] the owner's merges (the apply).
 * phip_group_apply_mixed: ms[0] the pack (phip_route_pack_ops), ms[1] both
 * exchanges (ops out, results back), ms[2] the owner's phip_apply_mixed plus
 * the results scatter.  phip_group_peek: ms[0] the query pack, ms[1] both
 * exchanges (queries out, answers back), ms[2] the owner's phip_peek plus the
 * answers' scatter.
 * The stages overlap, so their sum can exceed the call.  The read
 * synchronises on the events. */
int phip_group_set_timing(phip_group* g, int on);
int phip_group_stage_ms(phip_group* g, uint32_t i, float* ms /* [3] */);
/* The RCCL member i's communicator runs on: ncclGetVersion, ncclCommCount
 * (must equal the world; 0 for a shared-device group, which has none) and
 * the path of the librccl the library's RCCL symbols resolved to (dladdr).
 * A process that loaded another librccl first (torch's, same soname
 * librccl.so.1) shares that one copy. */
int phip_group_rccl_info(phip_group* g, uint32_t i, int32_t* version, int32_t* comm_count,
                         char* lib_path, uint32_t path_cap);

/* ---- diagnostics ---- */
/* Per-kernel timing of the last hot-path call (every call since
 * phip_set_timing(h, 2) in that mode), measured with HIP events on the
 * handle's stream: writes up to max entries of (name, ms) and returns the
 * count. */
int phip_last_timings(phip_handle* h, const char** names, float* ms, int max);
/* Enable (1) or disable (0) event timing (off by default); 2 keeps the
 * timings of every later call until the next phip_set_timing, so a timed
 * loop can read them once, after it ends (the reads synchronise). */
void phip_set_timing(phip_handle* h, int on);
/* Counters of the last fast-path Receive batch: out[0] hot-directory
 * entries, out[1] messages folded through the directory, out[2] messages
 * that missed the table (inserted); out[3] table growths (rehashes) since
 * phip_open; out[4] messages of the batch that went through the ordered path
 * (the dirty buckets' sub-batch, or the suffix from the first dirty
 * message: phip_receive_soa); out[5] undo-log entries of the handle's last
 * optimistic pass and out[6] the messages of that pass that found their
 * wave's log full (such a pass is undone and the batch run again classified,
 * as one that met a dirty message; the handle then classifies its next 256
 * fast passes first); out[7] the passes the batch's hot directory had served
 * before this one (0: it was built for this batch; a handle keeps a
 * directory for later optimistic passes while consecutive builds select the
 * same buckets and the fraction folded holds, at most 32 passes, and drops it
 * whenever records move); out[8] 1 if the batch's first optimistic kernel,
 * queued behind a PHIP_RECV_ASYNC batch not yet finished, found its gate shut
 * (that batch left work; this one was then queued again behind it).
 * Returns the number written (<= 9).
 * Not a plain counter read: a batch queued with PHIP_RECV_ASYNC is finished
 * first (the call waits for it), so that the counters are that batch's.  The
 * call has no status to return an error in: if finishing the batch fails, its
 * error is kept and returned by the handle's next call that returns one. */
int phip_last_stats(phip_handle* h, uint64_t* out, int max);
/* The undo log an optimistic Receive pass over n messages keeps on a device
 * with `compute_units` compute units (host arithmetic only, no device call):
 * out[0] workgroups of the pass, out[1] its waves (one log region each),
 * out[2] entries of a region (32 bytes each: half the messages of the busiest
 * wave, 24 more, and 64 kept for the hot directory's flush), out[3] bytes of
 * the whole log.  Returns the number written (<= 4). */
int phip_undo_log_layout(uint32_t n, uint32_t compute_units, uint64_t* out, int max);
/* Placement quality of the table (one scan of the slots): out[0] buckets,
 * out[1] slots, out[2] the longest probe distance of a bucket from its home
 * slot, out[3] the sum of those distances.  Returns the number written
 * (<= 4) or < 0. */
int phip_table_stats(phip_handle* h, uint64_t* out, int max);

#ifdef __cplusplus
}
#endif
#endif /* PATROLHIP_H */
