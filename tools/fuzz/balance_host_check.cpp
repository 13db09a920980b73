// Stand-alone host check (no GPU, no Python) of r0h_logup_check_balance_host (csrc/logup_host.cpp), meant for a sanitizer build: the
// function's list is compared with a restatement that keeps every tuple's exact per-identity vector in a std::map (no fingerprint), on
// the witness as given and on EDITS copies of it with one word replaced each; the list's own promises are checked on the way -- strictly
// ascending (first_row, fraction), net in [1, p), members >= 1, n_out independent of capacity, a smaller capacity a prefix.
// Build and run: tools/fuzz/run_balance_check.sh (writes tuple circuits and the trace circuit's witness with the tests' helpers first).
//   balance_host_check BLOB DATA GLOBAL PO2 CODE|- [EDITS]
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
// logup_host.cpp also holds the session balance's handle; what a device handle or the verifier's side would call is not reached here
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

// every class by its exact vector of per-identity part sums
static std::vector<r0h_imbalance> exact(const r0h_circuit& c, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global) {
  const size_t n = (size_t)1 << po2;
  std::map<uint64_t, size_t> ids;
  for (uint32_t j = 0; j < c.logup.n_chain; j++)
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
  std::map<std::vector<uint32_t>, Entry> classes;
  std::vector<uint32_t> vec(ids.size());
  for (uint32_t j = 0; j < c.logup.n_chain; j++)
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
        auto it = classes.emplace(vec, Entry{~0ull, 0, 0}).first;
        it->second.first = std::min<uint64_t>(it->second.first, (uint64_t)r << 32 | (4 * j + s));
        it->second.sum += dec(num);
        it->second.members++;
      }
    }
  std::vector<Entry> bad;
  for (const auto& kv : classes)
    if (kv.second.sum % P) bad.push_back(kv.second);
  std::sort(bad.begin(), bad.end(), [](const Entry& a, const Entry& b) { return a.first < b.first; });
  std::vector<r0h_imbalance> out;
  for (const Entry& e : bad) out.push_back(r0h_imbalance{(uint32_t)e.first, (uint32_t)(e.first >> 32), (uint32_t)(e.sum % P), (uint32_t)std::min<uint64_t>(e.members, 0xffffffffull)});
  return out;
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
  const std::vector<r0h_imbalance> want = exact(c, po2, code, data.data(), global.data());
  if (want.size() != total || (total && memcmp(want.data(), all.data(), total * sizeof(r0h_imbalance)))) {
    fprintf(stderr, "%s: the host function reports %zu classes, the exact restatement %zu, or they differ\n", what, total, want.size());
    exit(1);
  }
  return total;
}

int main(int argc, char** argv) {
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
