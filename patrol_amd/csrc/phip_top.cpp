// phip_top_merge (patrolhip.h "Top talkers"): the top k of several
// phip_export_top lists, on the host.  Plain C++ over the C ABI's structs and
// nothing else, so that tools/top_merge_check.cpp builds it for the CPU under
// the host sanitizers beside its own main.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "patrolhip.h"

namespace {

struct Entry {
  uint64_t taken;
  uint32_t list;
  uint64_t pos;
};

// the total order of the result: taken descending, then list, then position
bool before(const Entry& a, const Entry& b) {
  if (a.taken != b.taken) return a.taken > b.taken;
  if (a.list != b.list) return a.list < b.list;
  return a.pos < b.pos;
}

std::string_view name_of(const phip_top_out& l, uint64_t i) {
  return std::string_view(reinterpret_cast<const char*>(l.names) + l.offs[i],
                          (size_t)(l.offs[i + 1] - l.offs[i]));
}

}  // namespace

extern "C" int phip_top_merge(const phip_top_out* lists, const uint64_t* ns, uint32_t n_lists,
                              uint32_t k, const phip_top_out* out, uint64_t* n_out) {
  if (!lists || !ns || !out || !n_out || !out->names || !out->offs || n_lists == 0 || k < 1 ||
      k > PHIP_TOP_MAX)
    return PHIP_ERR_INVALID;
  size_t total = 0;
  for (uint32_t l = 0; l < n_lists; ++l) {
    if (ns[l] && (!lists[l].names || !lists[l].offs || !lists[l].taken)) return PHIP_ERR_INVALID;
    total += (size_t)ns[l];
  }
  // one entry per name: the one that ranks first among those of that name
  // (the larger taken; equal taken: the earlier list, then position)
  std::vector<Entry> all;
  all.reserve(total);
  std::unordered_map<std::string_view, size_t> seen;
  seen.reserve(total);
  for (uint32_t l = 0; l < n_lists; ++l)
    for (uint64_t i = 0; i < ns[l]; ++i) {
      const Entry e{lists[l].taken[i], l, i};
      auto ins = seen.emplace(name_of(lists[l], i), all.size());
      if (ins.second) all.push_back(e);
      else if (before(e, all[ins.first->second])) all[ins.first->second] = e;
    }
  const size_t want = std::min<size_t>(k, all.size());
  std::partial_sort(all.begin(), all.begin() + (ptrdiff_t)want, all.end(), before);
  uint64_t n = 0, bytes = 0;
  out->offs[0] = 0;
  for (; n < want; ++n) {
    const Entry& e = all[n];
    const phip_top_out& src = lists[e.list];
    const std::string_view nm = name_of(src, e.pos);
    if (bytes + nm.size() > out->names_cap) break;   // cut at an entry
    if (!nm.empty()) memcpy(out->names + bytes, nm.data(), nm.size());
    bytes += nm.size();
    out->offs[n + 1] = bytes;
    if (out->taken) out->taken[n] = e.taken;
    if (out->state) out->state[n] = src.state ? src.state[e.pos] : phip_state{0, 0, 0, 0};
  }
  *n_out = n;
  return PHIP_OK;
}
