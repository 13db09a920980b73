// Stand-alone host check (no GPU, no Python) of r0h_logup_check_balance_host and of a host session handle (r0h_session_balance_new
// with no context, _add_host, _add_tuples, _report; csrc/balance_host.cpp over csrc/logup_host.cpp's walk), meant for a sanitizer
// build: their lists are compared with a restatement that keeps every tuple's exact per-identity vector in a std::map (no
// fingerprint), on the witness as given and on EDITS copies of it with one word replaced each; the chain list's own promises are
// checked on the way -- strictly ascending (first_row, fraction), net in [1, p), members >= 1, n_out independent of capacity, a smaller
// capacity a prefix.
// Build and run: tools/fuzz/run_balance_check.sh (writes tuple circuits, the trace circuit's witness and a two-segment session with
// the tests' helpers first).
//   balance_host_check BLOB DATA GLOBAL PO2 CODE|- [EDITS]
//   balance_host_check session BLOB EDITS (PO2 DATA GLOBAL)...
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "../../hyperfridge-r0_amd/csrc/circuit.hpp"

using namespace r0h;

namespace r0h {
const char* make_error(const char* fmt, ...) {  // (csrc/ctx.cpp's, which comes with the device context)
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return strdup(buf);
}
// What balance_host.cpp refers to and this program does not link: the session handle, driven below, shares the file with the chain's
// check, and the linker wants every name its entry points mention.  A handle made with a context retains it and keeps its classes in
// the device's table (ctx.cpp, balance.hip); the verifier's side reads an ELF (image.cpp).  No handle here has a context: freeing one
// passes through session_table_free, a no-op without a table; the other six are not reached.  (logup_host_check.cpp links logup_host.cpp with make_error alone.)
void ctx_retain(r0h_ctx*) {}
void ctx_release(r0h_ctx*) {}
void session_table_free(r0h_session_balance*) {}
const char* session_table_add_list(r0h_session_balance*, uint32_t, const uint64_t*, const uint32_t*, const uint32_t*, size_t) { return make_error("no device"); }
const char* session_table_report(r0h_session_balance*, r0h_session_imbalance*, size_t, size_t*) { return make_error("no device"); }
const char* session_table_stats(r0h_session_balance*, uint64_t*, uint64_t*) { return make_error("no device"); }
const char* elf_image(const uint8_t*, size_t, std::vector<std::pair<uint32_t, uint32_t>>&, uint32_t*, uint8_t[32]) { return make_error("no executor"); }
}  // namespace r0h

static std::vector<uint32_t> read_words(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  std::vector<uint32_t> w;
  uint32_t buf[4096];
  size_t k;
  while ((k = fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + k);
  fclose(f);
  return w;
}

struct Entry { uint64_t first, sum, members; };
typedef std::map<std::vector<uint32_t>, Entry> Classes;  // every class by its exact vector of canonical per-identity part sums

static void put(Classes& classes, const std::vector<uint32_t>& vec, uint64_t first, uint32_t numerator) {
  Entry& e = classes.emplace(vec, Entry{~0ull, 0, 0}).first->second;
  e.first = std::min(e.first, first);
  e.sum += numerator;
  e.members++;
}
// the tuples of accumulators [first_acc, first_acc + count) on one witness into `classes`; `first_of` orders a class's members
template <class FirstOf>
static void exact(Classes& classes, const r0h_circuit& c, uint32_t first_acc, uint32_t count, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global, FirstOf first_of) {
  const size_t n = (size_t)1 << po2;
  std::map<uint64_t, size_t> ids;  // in order of first appearance, as the session handle numbers them
  for (uint32_t j = first_acc; j < first_acc + count; j++)
    for (const LogupFraction& f : c.logup.accs[j].fr)
      for (const LogupPart& q : f.parts) ids.emplace(q.ch_kind ? (uint64_t)q.ch_kind << 32 | q.ch_idx : 0, ids.size());
  auto form = [&](const Lf& lf, size_t r) {
    uint32_t acc = 0;
    for (const LfTerm& t : lf.terms) {
      uint32_t v = enc(t.coef);
      if (t.global) v = mul(v, global[t.global - 1]);
      if (t.col) v = mul(v, (((t.col - 1) >> 28) == R0H_GROUP_CODE ? code : data)[(size_t)((t.col - 1) & 0xfffffu) * n + r]);
      acc = add(acc, v);
    }
    return acc;
  };
  std::vector<uint32_t> vec(ids.size());
  for (uint32_t j = first_acc; j < first_acc + count; j++)
    for (uint32_t s = 0; s < 4; s++) {
      const LogupFraction& f = c.logup.accs[j].fr.at(s);
      for (size_t r = 0; r < n; r++) {
        const uint32_t num = form(f.num, r);
        if (!num) continue;
        std::fill(vec.begin(), vec.end(), 0u);
        for (const LogupPart& q : f.parts) {
          uint32_t& cell = vec.at(ids.at(q.ch_kind ? (uint64_t)q.ch_kind << 32 | q.ch_idx : 0));
          cell = add(cell, form(q.lf, r));
        }
        for (uint32_t& v : vec) v = dec(v);
        put(classes, vec, first_of((uint32_t)r, 4 * j + s), dec(num));
      }
    }
}
// the classes that do not balance, lowest first member first
static std::vector<std::pair<std::vector<uint32_t>, Entry>> imbalanced(const Classes& classes) {
  std::vector<std::pair<std::vector<uint32_t>, Entry>> bad;
  for (const auto& kv : classes)
    if (kv.second.sum % P) bad.push_back(kv);
  std::sort(bad.begin(), bad.end(), [](const auto& a, const auto& b) { return a.second.first < b.second.first; });
  return bad;
}

static size_t check_once(const std::vector<uint32_t>& blob, const r0h_circuit& c, uint32_t po2, const uint32_t* code, const std::vector<uint32_t>& data, const std::vector<uint32_t>& global,
                         const char* what) {
  size_t total = 0;
  const char* e = r0h_logup_check_balance_host(blob.data(), blob.size(), po2, code, data.data(), global.data(), nullptr, 0, &total);
  if (e) { fprintf(stderr, "%s: %s\n", what, e); exit(1); }
  std::vector<r0h_imbalance> all(total + 1), some(total / 2 + 1);
  size_t n_all = 0, n_some = 0;
  if ((e = r0h_logup_check_balance_host(blob.data(), blob.size(), po2, code, data.data(), global.data(), all.data(), total, &n_all)) ||
      (e = r0h_logup_check_balance_host(blob.data(), blob.size(), po2, code, data.data(), global.data(), some.data(), total / 2, &n_some))) {
    fprintf(stderr, "%s: %s\n", what, e);
    exit(1);
  }
  if (n_all != total || n_some != total) { fprintf(stderr, "%s: n_out moves with the capacity: %zu, %zu, %zu\n", what, total, n_all, n_some); exit(1); }
  all.resize(total);
  for (size_t k = 0; k < total; k++) {
    const r0h_imbalance& a = all[k];
    if (a.net == 0 || a.net >= P || a.members == 0 || a.fraction >= 4 * c.logup.n_chain || a.first_row >> po2) { fprintf(stderr, "%s: entry %zu is out of range\n", what, k); exit(1); }
    if (k && ((uint64_t)all[k - 1].first_row << 32 | all[k - 1].fraction) >= ((uint64_t)a.first_row << 32 | a.fraction)) { fprintf(stderr, "%s: entry %zu is out of order\n", what, k); exit(1); }
    if (k < total / 2 && memcmp(&some[k], &a, sizeof a)) { fprintf(stderr, "%s: a smaller capacity is no prefix at entry %zu\n", what, k); exit(1); }
  }
  Classes classes;
  exact(classes, c, 0, c.logup.n_chain, po2, code, data.data(), global.data(), [](uint32_t row, uint32_t fraction) { return (uint64_t)row << 32 | fraction; });
  std::vector<r0h_imbalance> want;
  for (const auto& kv : imbalanced(classes)) {
    const Entry& e = kv.second;
    want.push_back(r0h_imbalance{(uint32_t)e.first, (uint32_t)(e.first >> 32), (uint32_t)(e.sum % P), (uint32_t)std::min<uint64_t>(e.members, 0xffffffffull)});
  }
  if (want.size() != total || (total && memcmp(want.data(), all.data(), total * sizeof(r0h_imbalance)))) {
    fprintf(stderr, "%s: the host function reports %zu classes, the exact restatement %zu, or they differ\n", what, total, want.size());
    exit(1);
  }
  return total;
}

struct Segment { uint32_t po2; std::vector<uint32_t> data, global; };

static void fail(const char* what, const char* e) { fprintf(stderr, "%s: %s\n", what, e); exit(1); }

// A host session handle over `segments` (source k: segment k) and a list from outside (source: the number of segments) against the
// exact restatement over the accumulators with a public total: the whole report, and a capacity of one its first entry.
static size_t session_once(const std::vector<uint32_t>& blob, const r0h_circuit& c, const std::vector<Segment>& segments, const std::vector<uint32_t>& numerators,
                           const std::vector<uint32_t>& values, const char* what) {
  const uint32_t n_chain = c.logup.n_chain, n_own = (uint32_t)c.logup.accs.size() - n_chain, outside = (uint32_t)segments.size();
  r0h_session_balance* sb = nullptr;
  const char* e = r0h_session_balance_new(nullptr, blob.data(), blob.size(), &sb);
  if (e) fail(what, e);
  const size_t n_ids = r0h_session_balance_n_identities(sb);
  Classes classes;
  for (uint32_t k = 0; k < segments.size(); k++) {
    const Segment& s = segments[k];
    if ((e = r0h_session_balance_add_host(sb, k, s.po2, nullptr, s.data.data(), s.global.data()))) fail(what, e);
    exact(classes, c, n_chain, n_own, s.po2, nullptr, s.data.data(), s.global.data(), [k](uint32_t row, uint32_t fraction) { return session_first(k, row, fraction); });
  }
  if ((e = r0h_session_balance_add_tuples(sb, outside, numerators.data(), values.data(), numerators.size()))) fail(what, e);
  for (size_t i = 0; i < numerators.size(); i++)
    if (numerators[i]) put(classes, std::vector<uint32_t>(values.begin() + i * n_ids, values.begin() + (i + 1) * n_ids), session_first(outside, (uint32_t)i, SESSION_OUTSIDE_FRACTION), numerators[i]);
  const auto want = imbalanced(classes);
  size_t total = 0, again = 0;
  std::vector<r0h_session_imbalance> got(want.size() + 1);
  r0h_session_imbalance lowest;
  if ((e = r0h_session_balance_report(sb, got.data(), got.size(), &total)) || (e = r0h_session_balance_report(sb, &lowest, 1, &again))) fail(what, e);
  if (total != want.size() || again != total || (total && memcmp(&lowest, &got[0], sizeof lowest))) fail(what, "the session handle and the exact restatement count different classes, or a capacity of one is no prefix");
  for (size_t k = 0; k < total; k++) {
    const Entry& w = want[k].second;
    const r0h_session_imbalance& g = got[k];
    if (session_first(g.source, g.first_row, g.fraction) != w.first || g.net != w.sum % P || g.members != w.members || g.n_values != n_ids || memcmp(g.values, want[k].first.data(), 4 * n_ids))
      fail(what, "the session handle's report differs from the exact restatement");
  }
  uint64_t stats[4];
  if ((e = r0h_session_balance_stats(sb, stats))) fail(what, e);
  if (stats[3] != classes.size()) fail(what, "the session handle holds another number of classes than the exact restatement");
  r0h_session_balance_free(sb);
  return total;
}

//   balance_host_check session BLOB EDITS (PO2 DATA GLOBAL)...
static int session_main(int argc, char** argv) {
  const std::vector<uint32_t> blob = read_words(argv[2]);
  const size_t edits = (size_t)atol(argv[3]);
  r0h_circuit c;
  const char* e = parse_blob(&c, blob.data(), blob.size());
  if (e) { fprintf(stderr, "%s\n", e); return 1; }
  std::vector<Segment> segments;
  for (int a = 4; a + 2 < argc; a += 3) {
    segments.push_back(Segment{(uint32_t)atoi(argv[a]), read_words(argv[a + 1]), read_words(argv[a + 2])});
    Segment& s = segments.back();
    s.global.resize(std::max<size_t>(s.global.size(), c.n_global + 1), 0);
    if (s.po2 < 4 || s.po2 > R0H_MAX_PO2 || s.data.size() != (size_t)c.group_size[R0H_GROUP_DATA] << s.po2) { fprintf(stderr, "witness does not fit the circuit\n"); return 2; }
  }
  r0h_session_balance* probe = nullptr;
  if ((e = r0h_session_balance_new(nullptr, blob.data(), blob.size(), &probe))) { fprintf(stderr, "%s\n", e); return 1; }
  const size_t n_ids = r0h_session_balance_n_identities(probe);
  r0h_session_balance_free(probe);
  // from outside: random tuples, one of them twice with opposite numerators (a class that closes), one with a numerator of zero (no tuple)
  std::mt19937_64 rng(blob.size() * 1000003ull + segments.size());
  std::vector<uint32_t> numerators, values;
  for (size_t i = 0; i < 12; i++) {
    numerators.push_back(i == 5 ? 0u : 1u + (uint32_t)(rng() % (P - 1)));
    for (size_t k = 0; k < n_ids; k++) values.push_back((uint32_t)(rng() % P));
  }
  numerators.push_back(P - numerators[3]);
  values.insert(values.end(), values.begin() + 3 * n_ids, values.begin() + 4 * n_ids);
  const size_t alone = session_once(blob, c, segments, {}, {}, "segments alone"), honest = session_once(blob, c, segments, numerators, values, "as given");
  size_t moved = 0;
  for (size_t k = 0; k < edits; k++) {
    std::vector<Segment> bad = segments;
    std::vector<uint32_t>& data = bad[rng() % bad.size()].data;
    const size_t at = rng() % data.size();
    const uint32_t pick[] = {0u, ONE, P - 1, (uint32_t)(rng() % P), add(data[at], ONE), sub(data[at], ONE)};
    data[at] = pick[rng() % 6];
    char what[64];
    snprintf(what, sizeof what, "session edit %zu (word %zu)", k, at);
    moved += session_once(blob, c, bad, numerators, values, what) != honest;
  }
  printf("session balance: %zu segments, %zu identities: %zu classes from the segments alone, %zu with %zu tuples from outside; %zu single-word edits, %zu of them move the count: equal to the exact restatement throughout\n",
         segments.size(), n_ids, alone, honest, numerators.size(), edits, moved);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 7 && !strcmp(argv[1], "session")) return session_main(argc, argv);
  if (argc < 6) { fprintf(stderr, "usage: %s BLOB DATA GLOBAL PO2 CODE|- [EDITS]\n", argv[0]); return 2; }
  const std::vector<uint32_t> blob = read_words(argv[1]), data = read_words(argv[2]);
  std::vector<uint32_t> global = read_words(argv[3]);
  const uint32_t po2 = (uint32_t)atoi(argv[4]);
  const std::vector<uint32_t> code = strcmp(argv[5], "-") ? read_words(argv[5]) : std::vector<uint32_t>();
  const size_t edits = argc > 6 ? (size_t)atol(argv[6]) : 20;
  r0h_circuit c;
  const char* e = parse_blob(&c, blob.data(), blob.size());
  if (e) { fprintf(stderr, "%s\n", e); return 1; }
  global.resize(std::max<size_t>(global.size(), c.n_global + 1), 0);
  if (po2 < 4 || po2 > R0H_MAX_PO2 || data.size() != (size_t)c.group_size[R0H_GROUP_DATA] << po2 || (!code.empty() && code.size() != (size_t)c.group_size[R0H_GROUP_CODE] << po2)) {
    fprintf(stderr, "witness does not fit the circuit\n");
    return 2;
  }
  const uint32_t* code_words = code.empty() ? nullptr : code.data();
  const size_t honest = check_once(blob, c, po2, code_words, data, global, "as given");
  std::mt19937_64 rng(po2 * 1000003ull + data.size());
  size_t moved = 0, most = 0;
  for (size_t k = 0; k < edits; k++) {
    std::vector<uint32_t> bad = data;
    const size_t at = rng() % bad.size();
    const uint32_t pick[] = {0u, ONE, P - 1, (uint32_t)(rng() % P), add(bad[at], ONE), sub(bad[at], ONE)};
    bad[at] = pick[rng() % 6];
    char what[64];
    snprintf(what, sizeof what, "edit %zu (word %zu)", k, at);
    const size_t found = check_once(blob, c, po2, code_words, bad, global, what);
    moved += found != honest;
    most = std::max(most, found);
  }
  printf("balance: %u chain fractions on 2^%u rows: %zu classes as given; %zu single-word edits, %zu of them move the count (at most %zu classes): equal to the exact restatement throughout\n",
         4 * c.logup.n_chain, po2, honest, edits, moved, most);
  return 0;
}
