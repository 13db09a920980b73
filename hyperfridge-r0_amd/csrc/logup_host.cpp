// Host side of the log-derivative argument (blob section LOGUP): the multiplicity columns of a witness that lives in host memory --
// what the tests' reference witness (r0h_vm_trace_witness) is completed with, and what a caller that builds its own DATA group needs
// before committing it -- and the balance check of the chain links (r0h_logup_check_balance_host: the compiled form the device's is
// compared with).  The device forms are in csrc/logup.hip; these are plain loops over the same description.
#include <string.h>

#include <vector>

#include "../../include/r0hip_circuit.h"
#include "circuit.hpp"

#include <algorithm>
#include <set>
#include <unordered_map>

using namespace r0h;

namespace r0h {
// the lookups alone, table by table, chain links in order: numerator and value (a lookup's second part: the parser sees to it); the
// challenge part of a lookup and fractions without a table are not on the list
const char* logup_lookup_list(const r0h_circuit* c, const uint32_t* global, LookupList* out) {
  R0H_REQUIRE(c->logup.tables.size() <= 2, "r0h_logup_multiplicities: at most two tables");
  std::set<uint32_t> cols;
  auto form = [&](const Lf& lf) {
    out->words.push_back((uint32_t)lf.terms.size());
    for (const LfTerm& t : lf.terms) {
      uint32_t coef = enc(t.coef);
      if (t.global) coef = mul(coef, global ? global[t.global - 1] : 0u);
      out->words.push_back(coef);
      out->words.push_back(t.col ? ((t.col - 1) & 0xfffffu) + 1 : 0u);
      if (t.col) cols.insert((t.col - 1) & 0xfffffu);
    }
  };
  for (uint32_t k = 0; k < c->logup.tables.size(); k++) {
    out->begin[k] = (uint32_t)out->words.size();
    for (uint32_t j = 0; j < c->logup.n_chain; j++)
      for (const LogupFraction& f : c->logup.accs[j].fr) {
        if (f.table != k + 1) continue;
        form(f.num);
        form(f.parts[1].lf);
        out->entries[k]++;
      }
    out->begin[k + 1] = (uint32_t)out->words.size();
  }
  out->n_cols = (uint32_t)cols.size();
  return nullptr;
}
}  // namespace r0h

extern "C" {

const char* r0h_logup_multiplicities_host(const uint32_t* blob, size_t blob_words, uint32_t po2, uint32_t* data, const uint32_t* global) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && data, "r0h_logup_multiplicities_host: NULL argument");
  r0h_circuit c;
  R0H_TRY(parse_blob(&c, blob, blob_words));
  if (c.logup.tables.empty()) return nullptr;
  R0H_REQUIRE(po2 >= 16 && po2 <= R0H_MAX_PO2, "r0h_logup_multiplicities_host: the tables have 2^16 rows: po2 %u outside [16, %u]", po2, (unsigned)R0H_MAX_PO2);
  const size_t n = (size_t)1 << po2;
  std::vector<std::vector<uint32_t>> hist(c.logup.tables.size(), std::vector<uint32_t>(65536, 0));
  std::vector<uint64_t> slots(c.logup.tables.size(), 0);
  for (uint32_t j = 0; j < c.logup.n_chain; j++)
    for (const LogupFraction& f : c.logup.accs[j].fr)
      if (f.table) slots[f.table - 1] += n;
  for (size_t k = 0; k < slots.size(); k++)
    R0H_REQUIRE(slots[k] <= P - 1, "r0h_logup_multiplicities_host: table %zu has %llu lookup slots at 2^%u rows: more than p - 1", k, (unsigned long long)slots[k], po2);
  auto form = [&](const Lf& lf, size_t r) {  // a lookup's forms read DATA columns, public inputs and constants (the parser sees to it)
    uint32_t acc = 0;
    for (const LfTerm& t : lf.terms) {
      uint32_t v = enc(t.coef);
      if (t.global) v = mul(v, global ? global[t.global - 1] : 0u);
      if (t.col) v = mul(v, data[(size_t)((t.col - 1) & 0xfffffu) * n + r]);
      acc = add(acc, v);
    }
    return acc;
  };
  for (uint32_t j = 0; j < c.logup.n_chain; j++)
    for (const LogupFraction& f : c.logup.accs[j].fr) {
      if (!f.table) continue;
      for (size_t r = 0; r < n; r++) {
        const uint32_t num = form(f.num, r);
        R0H_REQUIRE(num == 0 || num == ONE, "r0h_logup_multiplicities_host: row %zu: a lookup's numerator is neither 0 nor 1", r);
        if (num != ONE) continue;
        uint32_t v = dec(neg(form(f.parts[1].lf, r)));
        if (c.logup.tables[f.table - 1].kind == R0H_TABLE_AND) {
          v -= R0H_TAG_AND;
          R0H_REQUIRE(!(v >> 24) && ((v & 255u) & ((v >> 8) & 255u)) == v >> 16, "r0h_logup_multiplicities_host: row %zu looks up a value that is not in the byte-AND table", r);
          v &= 0xffffu;
        } else {
          R0H_REQUIRE(!(v >> 16), "r0h_logup_multiplicities_host: row %zu looks up %u in the 16-bit range table", r, v);
        }
        hist[f.table - 1][v]++;
      }
    }
  for (size_t k = 0; k < c.logup.tables.size(); k++) {
    uint32_t* col = data + (size_t)c.logup.tables[k].data_col * n;
    memset(col, 0, n * 4);
    for (uint32_t v = 0; v < 65536; v++) col[v] = enc(hist[k][v]);
  }
  return nullptr;
  R0H_GUARD_END
}

uint32_t r0h_circuit_n_chain_fractions(const r0h_circuit* c) { return c ? 4 * c->logup.n_chain : 0; }

const char* r0h_logup_check_balance_host(const uint32_t* blob, size_t blob_words, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global, r0h_imbalance* out,
                                         size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && data && n_out && (out || !capacity), "r0h_logup_check_balance_host: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_logup_check_balance_host: po2 %u outside [4, %u]", po2, (unsigned)R0H_MAX_PO2);
  r0h_circuit c;
  R0H_TRY(parse_blob(&c, blob, blob_words));
  *n_out = 0;
  const size_t n = (size_t)1 << po2;
  const uint32_t n_chain = c.logup.n_chain;
  R0H_REQUIRE(((uint64_t)(4 * n_chain) << po2) <= 0xffffffffull, "r0h_logup_check_balance_host: %u fractions on 2^%u rows: more than 2^32 - 1 tuples", 4 * n_chain, po2);
  for (uint32_t i = 0; i + c.n_late < c.n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_logup_check_balance_host: global[%u] not canonical", i);
  auto check = [&](const Lf& lf) -> const char* {
    for (const LfTerm& t : lf.terms) {
      R0H_REQUIRE(!t.global || global, "r0h_logup_check_balance_host: a form reads a public input and none were given");
      R0H_REQUIRE(!t.col || ((t.col - 1) >> 28) != R0H_GROUP_CODE || code, "r0h_logup_check_balance_host: a form reads the CODE group and none was given");
    }
    return nullptr;
  };
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
  struct Class { uint64_t sum = 0, first = ~0ull, members = 0; };
  std::unordered_map<uint64_t, Class> classes;
  for (uint32_t j = 0; j < n_chain; j++)
    for (uint32_t slot = 0; slot < c.logup.accs[j].fr.size(); slot++) {
      const LogupFraction& f = c.logup.accs[j].fr[slot];
      const uint32_t fi = 4 * j + slot;
      R0H_TRY(check(f.num));
      std::vector<uint32_t> w0, w1;
      for (const LogupPart& q : f.parts) {
        R0H_TRY(check(q.lf));
        const uint64_t identity = q.ch_kind ? (uint64_t)q.ch_kind << 32 | q.ch_idx : 0;
        w0.push_back(balance_weight(0, identity));
        w1.push_back(balance_weight(1, identity));
      }
      for (size_t r = 0; r < n; r++) {
        const uint32_t num = form(f.num, r);
        if (!num) continue;
        uint32_t h0 = 0, h1 = 0;
        for (size_t q = 0; q < f.parts.size(); q++) {
          const uint32_t v = form(f.parts[q].lf, r);
          h0 = add(h0, mul(w0[q], v));
          h1 = add(h1, mul(w1[q], v));
        }
        Class& cl = classes[balance_key(h0, h1)];
        cl.sum += dec(num);
        cl.members++;
        cl.first = std::min<uint64_t>(cl.first, (uint64_t)r << 32 | fi);
      }
    }
  std::vector<const Class*> bad;
  for (const auto& kv : classes)
    if (kv.second.sum % P) bad.push_back(&kv.second);
  std::sort(bad.begin(), bad.end(), [](const Class* a, const Class* b) { return a->first < b->first; });
  *n_out = bad.size();
  for (size_t k = 0; k < bad.size() && k < capacity; k++)
    out[k] = r0h_imbalance{(uint32_t)bad[k]->first, (uint32_t)(bad[k]->first >> 32), (uint32_t)(bad[k]->sum % P), (uint32_t)std::min<uint64_t>(bad[k]->members, 0xffffffffull)};
  return nullptr;
  R0H_GUARD_END
}

}  // extern "C"
