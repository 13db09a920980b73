// Host side of the log-derivative argument (blob section LOGUP): the multiplicity columns of a witness that lives in host memory --
// what the tests' reference witness (r0h_vm_trace_witness) is completed with, and what a caller that builds its own DATA group needs
// before committing it -- the lookup list the device's counting kernel walks, and what the host's balance checks (balance_host.cpp)
// share: a linear form at a row, what it needs of its caller, the walk over the tuples of a range of accumulators.  The device forms
// are in csrc/logup.hip and csrc/balance.hip.
#include <set>

#include "../../include/r0hip_circuit.h"
#include "circuit.hpp"

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

uint32_t eval_lf(const Lf& lf, const uint32_t* code, const uint32_t* data, const uint32_t* global, size_t n, size_t r) {
  uint32_t acc = 0;
  for (const LfTerm& t : lf.terms) {
    uint32_t v = enc(t.coef);
    if (t.global) v = mul(v, global ? global[t.global - 1] : 0u);
    if (t.col) v = mul(v, (((t.col - 1) >> 28) == R0H_GROUP_CODE ? code : data)[(size_t)((t.col - 1) & 0xfffffu) * n + r]);
    acc = add(acc, v);
  }
  return acc;
}

const char* require_lf_inputs(const char* caller, const Lf& lf, const uint32_t* code, const uint32_t* global) {
  for (const LfTerm& t : lf.terms) {
    R0H_REQUIRE(!t.global || global, "%s: a form reads a public input and none were given", caller);
    R0H_REQUIRE(!t.col || ((t.col - 1) >> 28) != R0H_GROUP_CODE || code, "%s: a form reads the CODE group and none was given", caller);
  }
  return nullptr;
}

std::vector<uint64_t> tuple_identities(const r0h_circuit& c, uint32_t first, uint32_t count) {
  std::vector<uint64_t> ids;
  for (uint32_t j = first; j < first + count; j++)
    for (const LogupFraction& f : c.logup.accs[j].fr)
      for (const LogupPart& q : f.parts)
        if (std::find(ids.begin(), ids.end(), part_identity(q)) == ids.end()) ids.push_back(part_identity(q));
  return ids;
}

const char* walk_tuples(const char* caller, const r0h_circuit& c, uint32_t first, uint32_t count, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global,
                        const std::function<const char*(const HostTuple&)>& each) {
  const size_t n = (size_t)1 << po2;
  const std::vector<uint64_t> ids = tuple_identities(c, first, count);
  const std::vector<uint32_t> w = balance_weights(ids);
  std::vector<uint32_t> sums(ids.size());
  for (uint32_t j = first; j < first + count; j++)
    for (const LogupFraction& f : c.logup.accs[j].fr) {
      R0H_TRY(require_lf_inputs(caller, f.num, code, global));
      for (const LogupPart& q : f.parts) R0H_TRY(require_lf_inputs(caller, q.lf, code, global));
    }
  for (uint32_t j = first; j < first + count; j++)
    for (uint32_t slot = 0; slot < c.logup.accs[j].fr.size(); slot++) {
      const LogupFraction& f = c.logup.accs[j].fr[slot];
      std::vector<size_t> id;
      for (const LogupPart& q : f.parts) id.push_back((size_t)(std::find(ids.begin(), ids.end(), part_identity(q)) - ids.begin()));
      for (size_t r = 0; r < n; r++) {
        const uint32_t num = eval_lf(f.num, code, data, global, n, r);
        if (!num) continue;
        std::fill(sums.begin(), sums.end(), 0u);
        for (size_t q = 0; q < f.parts.size(); q++) sums[id[q]] = add(sums[id[q]], eval_lf(f.parts[q].lf, code, data, global, n, r));
        uint32_t h0 = 0, h1 = 0;
        for (size_t k = 0; k < ids.size(); k++) {
          h0 = add(h0, mul(w[k], sums[k]));
          h1 = add(h1, mul(w[ids.size() + k], sums[k]));
          sums[k] = dec(sums[k]);
        }
        R0H_TRY(each(HostTuple{balance_key(h0, h1), dec(num), (uint32_t)r, 4 * j + slot, sums.data()}));
      }
    }
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
  for (uint32_t j = 0; j < c.logup.n_chain; j++)
    for (const LogupFraction& f : c.logup.accs[j].fr) {
      if (!f.table) continue;
      for (size_t r = 0; r < n; r++) {
        const uint32_t num = eval_lf(f.num, nullptr, data, global, n, r);  // a lookup's forms read DATA columns, public inputs and constants (the parser sees to it)
        R0H_REQUIRE(num == 0 || num == ONE, "r0h_logup_multiplicities_host: row %zu: a lookup's numerator is neither 0 nor 1", r);
        if (num != ONE) continue;
        uint32_t v = dec(neg(eval_lf(f.parts[1].lf, nullptr, data, global, n, r)));
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

}  // extern "C"
