// phip_top_merge (patrol_amd/csrc/phip_top.cpp) under the host sanitizers: a
// stand-alone program with its own main, built together with that file for the
// CPU -- no GPU, no handle, nothing loaded into another process.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -static-libasan -static-libubsan -I include -o tools/top_merge_check tools/top_merge_check.cpp patrol_amd/csrc/phip_top.cpp
//   ./tools/top_merge_check cases.txt
//
// cases.txt is what tests/test_top_abi.py writes from tests/_top_cases.py's
// merge_cases(), with the Python merge's answer behind every case:
//   <number of cases>
//   <k> <n_lists>
//     <n>                                      per list
//       <name hex or -> <taken> <added> <elapsed> <created>     per entry
//   <n_expected>
//       <name hex or -> <taken> <added> <elapsed> <created>
// Every buffer is sized exactly (names_cap = the bytes expected, k + 1 offsets
// or fewer where the case holds fewer entries), so a write past what the
// contract allows is a sanitizer report.  Then the refusals, and the names_cap
// cut.  Prints the counts; exit status 1 on a mismatch.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "patrolhip.h"

namespace {

struct Row {
  std::string name;
  phip_state st;
};

struct List {
  std::vector<uint8_t> names;
  std::vector<uint64_t> offs, taken;
  std::vector<phip_state> state;
  phip_top_out view(bool with_state = true) {
    // (exact sizes: an empty vector's data() may be null, which the contract
    // allows for a list without entries)
    return phip_top_out{names.data(), names.size(), offs.data(), taken.data(),
                        with_state ? state.data() : nullptr};
  }
};

bool read_row(FILE* f, Row* r) {
  char hex[600];
  uint64_t t, a;
  int64_t e, c;
  if (fscanf(f, "%599s %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64, hex, &t, &a, &e, &c) != 5)
    return false;
  r->name.clear();
  if (strcmp(hex, "-") != 0)
    for (size_t i = 0; hex[i] && hex[i + 1]; i += 2) {
      unsigned v;
      sscanf(hex + i, "%2x", &v);
      r->name.push_back((char)v);
    }
  r->st = phip_state{a, t, e, c};
  return true;
}

List make_list(const std::vector<Row>& rows) {
  List l;
  l.offs.push_back(0);
  for (const Row& r : rows) {
    l.names.insert(l.names.end(), r.name.begin(), r.name.end());
    l.offs.push_back(l.names.size());
    l.taken.push_back(r.st.taken);
    l.state.push_back(r.st);
  }
  return l;
}

int fail(const char* what, long c) {
  printf("top_merge_check: case %ld: %s\n", c, what);
  return 1;
}

int refusals() {
  std::vector<Row> rows = {{"a", {2, 1, 0, 0}}, {"b", {2, 1, 0, 0}}};
  List l = make_list(rows);
  phip_top_out in = l.view();
  uint64_t ns = 2, n = 99;
  uint8_t names[8];
  uint64_t offs[4];
  phip_top_out out{names, sizeof names, offs, nullptr, nullptr};
  phip_top_out no_names = out, no_offs = out, in_no_taken = in;
  no_names.names = nullptr;
  no_offs.offs = nullptr;
  in_no_taken.taken = nullptr;
  const int rcs[] = {
      phip_top_merge(&in, &ns, 0, 2, &out, &n),       phip_top_merge(&in, &ns, 1, 0, &out, &n),
      phip_top_merge(&in, &ns, 1, PHIP_TOP_MAX + 1, &out, &n),
      phip_top_merge(nullptr, &ns, 1, 2, &out, &n),   phip_top_merge(&in, nullptr, 1, 2, &out, &n),
      phip_top_merge(&in, &ns, 1, 2, nullptr, &n),    phip_top_merge(&in, &ns, 1, 2, &out, nullptr),
      phip_top_merge(&in, &ns, 1, 2, &no_names, &n),  phip_top_merge(&in, &ns, 1, 2, &no_offs, &n),
      phip_top_merge(&in_no_taken, &ns, 1, 2, &out, &n)};
  for (int rc : rcs)
    if (rc != PHIP_ERR_INVALID) return 1;
  if (n != 99) return 1;
  // k == PHIP_TOP_MAX is taken; a list without state merges as zero states
  phip_state st[2] = {{9, 9, 9, 9}, {9, 9, 9, 9}};
  phip_top_out in2 = l.view(false);
  out.state = st;
  if (phip_top_merge(&in2, &ns, 1, PHIP_TOP_MAX, &out, &n) != PHIP_OK || n != 2) return 1;
  if (st[0].added || st[0].created || st[1].taken) return 1;
  // names_cap cut at an entry: "a" fits one byte, "b" does not
  out.names_cap = 1;
  out.state = nullptr;
  if (phip_top_merge(&in, &ns, 1, 2, &out, &n) != PHIP_OK || n != 1 || offs[1] != 1 || names[0] != 'a')
    return 1;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (refusals()) {
    printf("top_merge_check: refusals: mismatch\n");
    return 1;
  }
  if (argc < 2) {
    printf("top_merge_check: refusals clean (no case file given)\n");
    return 0;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    printf("top_merge_check: cannot open %s\n", argv[1]);
    return 1;
  }
  long ncases = 0, entries = 0;
  if (fscanf(f, "%ld", &ncases) != 1) return fail("no case count", -1);
  for (long c = 0; c < ncases; ++c) {
    unsigned k, n_lists;
    if (fscanf(f, "%u %u", &k, &n_lists) != 2) return fail("short header", c);
    std::vector<List> lists;
    for (unsigned l = 0; l < n_lists; ++l) {
      unsigned long n;
      if (fscanf(f, "%lu", &n) != 1) return fail("short list", c);
      std::vector<Row> rows(n);
      for (Row& r : rows)
        if (!read_row(f, &r)) return fail("short row", c);
      lists.push_back(make_list(rows));
    }
    unsigned long n_exp;
    if (fscanf(f, "%lu", &n_exp) != 1) return fail("no expectation", c);
    std::vector<Row> exp(n_exp);
    for (Row& r : exp)
      if (!read_row(f, &r)) return fail("short expectation", c);
    const List want = make_list(exp);
    std::vector<phip_top_out> views;
    std::vector<uint64_t> ns;
    for (List& l : lists) {
      views.push_back(l.view());
      ns.push_back(l.taken.size());
    }
    // outputs of exactly the expected size
    // (one spare byte keeps the pointer non-null for an empty result; it is
    // not budget and must stay as it is)
    std::vector<uint8_t> names(want.names.size() + 1, 0x5A);
    std::vector<uint64_t> offs(n_exp + 1, 0x5A5A), taken(n_exp);
    std::vector<phip_state> state(n_exp);
    phip_top_out out{names.data(), want.names.size(), offs.data(), taken.data(), state.data()};
    uint64_t n = ~0ull;
    if (phip_top_merge(views.data(), ns.data(), n_lists, k, &out, &n) != PHIP_OK)
      return fail("refused", c);
    if (n != n_exp) return fail("entry count differs", c);
    if (names.back() != 0x5A) return fail("wrote past names_cap", c);
    names.pop_back();
    if (offs != want.offs || names != want.names || taken != want.taken) return fail("list differs", c);
    for (unsigned long i = 0; i < n_exp; ++i)
      if (memcmp(&state[i], &want.state[i], sizeof(phip_state)) != 0) return fail("state differs", c);
    entries += (long)n_exp;
  }
  fclose(f);
  printf("top_merge_check: %ld cases, %ld entries, refusals: clean\n", ncases, entries);
  return 0;
}
