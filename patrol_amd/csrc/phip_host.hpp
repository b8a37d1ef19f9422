// Host helpers shared by the C-ABI entry points (not exported).
#pragma once
#include <cstdint>

#include "patrolhip.h"

namespace phip_host {

// The stream every call of the handle runs on (its own or phip_set_stream's)
// and its device: the shard group (phip_group.hip) queues its RCCL calls there.
void* handle_stream(phip_handle* h);
int handle_device(const phip_handle* h);

// Owner routing as phip_route_pack does it, queued on `stream` (a hipStream_t
// of the handle's device) with no host synchronisation: the pipelined
// exchange of phip_group_receive packs chunk k+1 while chunk k travels.
//   route_dir:  the sender-side combine's hot-name directory, from a strided
//               sample of the whole batch m (nullptr below kRouteMinBatch);
//   route_pack: the stable owner partition of m (one chunk) into owner-major
//               send buffers, with the per-owner totals in counts / nbytes
//               (device), combining with `dir` when it is not null.
// The scratch they use is the handle's, reused in stream order: every pack
// of one call must be queued on the same stream, none larger than the first.
int route_dir(phip_handle* h, void* stream, const phip_msgs* m, uint32_t world, const void** dir);
int route_pack(phip_handle* h, void* stream, const phip_msgs* m, uint32_t world, const void* dir,
               uint8_t* names, uint32_t* lens, uint64_t* a, uint64_t* t, int64_t* e,
               uint64_t* counts, uint64_t* nbytes, uint32_t* src = nullptr);
// The same for an ordered op stream (phip_route_pack_ops' pack of one chunk,
// no combine), and the results' way back: entry j of the returned columns
// (send order) into out's columns at src[j]; a NULL column of out is skipped.
// Both are queued on `stream` with no host synchronisation.
int route_pack_ops(phip_handle* h, void* stream, const phip_ops* ops, uint32_t world,
                   uint8_t* names, uint32_t* lens, uint8_t* kind, int64_t* now, uint64_t* x0,
                   uint64_t* x1, uint64_t* x2, uint32_t* src, uint64_t* counts, uint64_t* nbytes);
int results_scatter(phip_handle* h, void* stream, const uint32_t* src, uint32_t n,
                    const uint8_t* status, const uint64_t* remaining, const uint64_t* have,
                    const phip_state* reply, const phip_results* out);
// The read side (phip_group_peek): the query pack is route_pack_ops without a
// kind column on either side (q->kind is not read; the operand words are
// always freq, per, count), and the answers' way back is results_scatter over
// the peek columns (state == NULL: the call did not return that column).
int route_pack_queries(phip_handle* h, void* stream, const phip_ops* q, uint32_t world,
                       uint8_t* names, uint32_t* lens, int64_t* now, uint64_t* x0, uint64_t* x1,
                       uint64_t* x2, uint32_t* src, uint64_t* counts, uint64_t* nbytes);
int peek_results_scatter(phip_handle* h, void* stream, const uint32_t* src, uint32_t n,
                         const uint8_t* status, const uint64_t* remaining, const uint64_t* have,
                         const int64_t* retry_at, const phip_state* state,
                         const phip_peek_results* out);
// The route kernels do not check a batch's name offsets as they go.
// check_offsets: one pass over a checked batch's offset column (names_len !=
// 0; NamesOffs::bad's rule) on `stream`, which it synchronises: *first_bad is
// the first malformed entry, ~0 when there is none (or names_len == 0).  It
// takes the names view of a batch (a phip_msgs' or a phip_ops' names,
// name_offs, names_len and n): phip_group_receive and phip_group_apply_mixed
// run it over every local batch before any pack.
int check_offsets(phip_handle* h, void* stream, const uint8_t* names, const uint32_t* name_offs,
                  uint32_t names_len, uint32_t n, uint32_t* first_bad);
// The wire forms (phip_group_receive_datagrams): w is a batch of raw
// datagrams, or one chunk of it (offs advanced; the offsets stay absolute).
//   wire_scan:  the pre-pass over offsets and length bytes on `stream`, which
//               it synchronises: *stop is the first malformed datagram (or
//               w->n), *first_bad the first entry a checked batch's offsets
//               rule rejects (~0: none);
//   route_dir_wire / route_pack_wire: route_dir / route_pack read from the
//               datagrams in place; every datagram of w must be well formed.
int wire_scan(phip_handle* h, void* stream, const phip_wire* w, uint32_t* stop, uint32_t* first_bad);
int route_dir_wire(phip_handle* h, void* stream, const phip_wire* w, uint32_t world, const void** dir);
int route_pack_wire(phip_handle* h, void* stream, const phip_wire* w, uint32_t world, const void* dir,
                    uint8_t* names, uint32_t* lens, uint64_t* a, uint64_t* t, int64_t* e,
                    uint64_t* counts, uint64_t* nbytes, uint32_t* src = nullptr);
// What the replies forms of the group add at the source (phip_group_*_replies).
// route_pack / route_pack_wire with src != nullptr also write src[j], the
// chunk index of the message packed at send position j (~0 for a combined
// message, which stands for many and is never a request); without it they
// launch the kernels they always did.  count_zero / count_zero_wire: one pass
// over the chunk's replica fields on `stream` that adds its zero-state count
// (Bucket.IsZero's ==) << 32 to out[0 .. nout) (device), no synchronisation.
int count_zero(phip_handle* h, void* stream, const phip_msgs* m, uint32_t nout, uint64_t* out);
int count_zero_wire(phip_handle* h, void* stream, const phip_wire* w, uint32_t nout, uint64_t* out);
// A ring's slot as a group member's batch (phip_group_ring_receive): the
// slot's device copy as *w and its `copied` event (a hipEvent_t), when the
// ring was opened on h (else PHIP_ERR_INVALID) and the slot is the ring's next
// submitted one (else PHIP_ERR_BUSY; the slot stays submitted).  ring_release
// frees the slot once nothing reads it any more.
int ring_slot(phip_ring* r, uint32_t slot, const phip_handle* h, phip_wire* w, void** copied);
void ring_release(phip_ring* r, uint32_t slot);
const char* last_error(phip_handle* h);

// The request parsing of API.takeBucket (api.go:55-65): the name-length check
// (returns 400 with ErrNameTooLarge's text as the body), ParseRate with its
// error ignored (the Rate Go returns beside the error), count 0 / error -> 1.
// Returns 0 when the Take should run.
int api_prepare(const uint8_t* name, uint32_t len, const char* rate, uint32_t rate_len,
                const char* count, uint32_t count_len, int64_t* freq, int64_t* per, uint64_t* n,
                char* body, uint32_t* body_len);

}  // namespace phip_host
