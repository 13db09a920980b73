// Host side of the log-derivative argument (blob section LOGUP): the multiplicity columns of a witness that lives in host memory --
// what the tests' reference witness (r0h_vm_trace_witness) is completed with, and what a caller that builds its own DATA group needs
// before committing it -- and the balance check of the chain links (r0h_logup_check_balance_host: the compiled form the device's is
// compared with), and of the session balance (r0h_session_balance_*: the handle, the identities, the host handle's classes, the
// verifier's side, report and message; a device handle's table is logup.hip's).  The device forms are in csrc/logup.hip; these are
// plain loops over the same description.
#include <stdarg.h>
#include <string.h>

#include <vector>

#include "../../include/r0hip_circuit.h"
#include "circuit.hpp"
#include "receipt_types.hpp"

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

// ---- the session balance (include/r0hip.h)
namespace {
uint32_t session_id_index(const r0h_session_balance* sb, const LogupPart& q) {
  const uint64_t identity = q.ch_kind ? (uint64_t)q.ch_kind << 32 | q.ch_idx : 0;
  return (uint32_t)(std::find(sb->ids.begin(), sb->ids.end(), identity) - sb->ids.begin());
}
// one tuple into a host handle's classes
void session_host_insert(r0h_session_balance* sb, uint64_t key, uint32_t numerator, uint64_t first, const uint32_t* values) {
  auto it = sb->classes.find(key);
  if (it == sb->classes.end()) {
    it = sb->classes.emplace(key, SessionClass()).first;
    for (size_t k = 0; k < sb->ids.size(); k++) it->second.values[k] = values[k];
  }
  SessionClass& cl = it->second;
  cl.sum += numerator;
  if (cl.sum >> 62) cl.sum %= P;
  cl.members++;
  cl.first = std::min(cl.first, first);
}
const char* session_room(const r0h_session_balance* sb, uint64_t more, const char* caller) {
  R0H_REQUIRE(sb->tuples + more <= 0xffffffffull, "%s: more than 2^32 - 1 tuples in one handle", caller);
  return nullptr;
}
}  // namespace

const char* r0h_session_balance_new(r0h_ctx* ctx, const uint32_t* blob, size_t blob_words, r0h_session_balance** sb_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && sb_out, "r0h_session_balance_new: NULL argument");
  std::unique_ptr<r0h_session_balance> sb(new r0h_session_balance());
  r0h_circuit& c = sb->circuit;
  R0H_TRY(parse_blob(&c, blob, blob_words));
  R0H_REQUIRE(4 * c.logup.accs.size() <= SESSION_OUTSIDE_FRACTION, "r0h_session_balance_new: %zu fractions: more than 255", 4 * c.logup.accs.size());
  const uint32_t first_late = c.n_global - c.n_late;
  for (uint32_t j = c.logup.n_chain; j < c.logup.accs.size(); j++)
    for (uint32_t slot = 0; slot < c.logup.accs[j].fr.size(); slot++) {
      const LogupFraction& f = c.logup.accs[j].fr[slot];
      auto check = [&](const Lf& lf) -> const char* {
        for (const LfTerm& t : lf.terms) {
          R0H_REQUIRE(!t.global || t.global - 1 < first_late, "r0h_session_balance_new: fraction %u reads the value of late public input %u: it does not exist before the challenge", 4 * j + slot,
                      t.global - 1);
          if (t.global) sb->reads_global = true;
        }
        return nullptr;
      };
      R0H_TRY(check(f.num));
      for (const LogupPart& q : f.parts) {
        R0H_TRY(check(q.lf));
        if (session_id_index(sb.get(), q) == sb->ids.size()) sb->ids.push_back(q.ch_kind ? (uint64_t)q.ch_kind << 32 | q.ch_idx : 0);
      }
    }
  R0H_REQUIRE(sb->ids.size() <= SESSION_MAX_IDS, "r0h_session_balance_new: %zu challenge identities under the public-total accumulators: more than %u", sb->ids.size(), SESSION_MAX_IDS);
  sb->weights.resize(2 * sb->ids.size());
  for (uint32_t j = 0; j < 2; j++)
    for (size_t k = 0; k < sb->ids.size(); k++) sb->weights[j * sb->ids.size() + k] = balance_weight(j, sb->ids[k]);
  if (ctx) {
    sb->ctx = ctx;
    ctx_retain(ctx);
  }
  *sb_out = sb.release();
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_free(r0h_session_balance* sb) {
  if (!sb) return nullptr;
  session_table_free(sb);
  if (sb->ctx) ctx_release(sb->ctx);
  delete sb;
  return nullptr;
}

uint32_t r0h_session_balance_n_identities(const r0h_session_balance* sb) { return sb ? (uint32_t)sb->ids.size() : 0; }

const char* r0h_session_balance_identity(const r0h_session_balance* sb, uint32_t k, uint32_t* kind_out, uint32_t* index_out) {
  R0H_REQUIRE(sb && kind_out && index_out, "r0h_session_balance_identity: NULL argument");
  R0H_REQUIRE(k < sb->ids.size(), "r0h_session_balance_identity: identity %u of %zu", k, sb->ids.size());
  *kind_out = (uint32_t)(sb->ids[k] >> 32);
  *index_out = (uint32_t)sb->ids[k];
  return nullptr;
}

const char* r0h_session_balance_add_host(r0h_session_balance* sb, uint32_t source, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && data, "r0h_session_balance_add_host: NULL argument");
  R0H_REQUIRE(!sb->ctx, "r0h_session_balance_add_host: this handle was made with a context: its segments are added with r0h_session_balance_add");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_session_balance_add_host: po2 %u outside [4, %u]", po2, (unsigned)R0H_MAX_PO2);
  const r0h_circuit& c = sb->circuit;
  const size_t n = (size_t)1 << po2, n_ids = sb->ids.size();
  R0H_REQUIRE(!sb->reads_global || global, "r0h_session_balance_add_host: a form reads a public input and none were given");
  for (uint32_t i = 0; i + c.n_late < c.n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_session_balance_add_host: global[%u] not canonical", i);
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
  for (uint32_t j = c.logup.n_chain; j < c.logup.accs.size(); j++)
    for (const LogupFraction& f : c.logup.accs[j].fr) {
      auto check = [&](const Lf& lf) -> const char* {
        for (const LfTerm& t : lf.terms) R0H_REQUIRE(!t.col || ((t.col - 1) >> 28) != R0H_GROUP_CODE || code, "r0h_session_balance_add_host: a form reads the CODE group and none was given");
        return nullptr;
      };
      R0H_TRY(check(f.num));
      for (const LogupPart& q : f.parts) R0H_TRY(check(q.lf));
    }
  for (uint32_t j = c.logup.n_chain; j < c.logup.accs.size(); j++)
    for (uint32_t slot = 0; slot < c.logup.accs[j].fr.size(); slot++) {
      const LogupFraction& f = c.logup.accs[j].fr[slot];
      std::vector<uint32_t> id;
      for (const LogupPart& q : f.parts) id.push_back(session_id_index(sb, q));
      for (size_t r = 0; r < n; r++) {
        const uint32_t num = form(f.num, r);
        if (!num) continue;
        R0H_TRY(session_room(sb, 1, "r0h_session_balance_add_host"));
        uint32_t sums[SESSION_MAX_IDS] = {0, 0, 0, 0, 0, 0, 0, 0}, h0 = 0, h1 = 0;
        for (size_t q = 0; q < f.parts.size(); q++) sums[id[q]] = add(sums[id[q]], form(f.parts[q].lf, r));
        for (size_t k = 0; k < n_ids; k++) {
          h0 = add(h0, mul(sb->weights[k], sums[k]));
          h1 = add(h1, mul(sb->weights[n_ids + k], sums[k]));
          sums[k] = dec(sums[k]);
        }
        session_host_insert(sb, balance_key(h0, h1), dec(num), session_first(source, (uint32_t)r, 4 * j + slot), sums);
        sb->tuples++;
      }
    }
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_add_tuples(r0h_session_balance* sb, uint32_t source, const uint32_t* numerators, const uint32_t* values, size_t n) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb, "r0h_session_balance_add_tuples: NULL argument");
  R0H_REQUIRE(n <= SESSION_MAX_LIST, "r0h_session_balance_add_tuples: %zu tuples in one call: more than 2^24", n);
  const size_t n_ids = sb->ids.size();
  R0H_REQUIRE((numerators && values) || !n || !n_ids, "r0h_session_balance_add_tuples: NULL argument");
  if (!n || !n_ids) return nullptr;  // (a circuit without public-total accumulators has no classes to put them in)
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> kept_num, kept_val;  // numerators of zero are no tuples: dropped here, their indices stay the others' rows
  size_t tuples = 0;
  for (size_t i = 0; i < n; i++) {
    R0H_REQUIRE(numerators[i] < P, "r0h_session_balance_add_tuples: numerator %zu is not canonical", i);
    uint32_t h0 = 0, h1 = 0;
    for (size_t k = 0; k < n_ids; k++) {
      const uint32_t v = values[i * n_ids + k];
      R0H_REQUIRE(v < P, "r0h_session_balance_add_tuples: value %zu of tuple %zu is not canonical", k, i);
      h0 = add(h0, mul(sb->weights[k], enc(v)));
      h1 = add(h1, mul(sb->weights[n_ids + k], enc(v)));
    }
    keys[i] = balance_key(h0, h1);
    tuples += numerators[i] != 0;
  }
  R0H_TRY(session_room(sb, tuples, "r0h_session_balance_add_tuples"));
  if (sb->ctx) {
    R0H_TRY(session_table_add_list(sb, source, keys.data(), numerators, values, n));
  } else {
    for (size_t i = 0; i < n; i++)
      if (numerators[i]) session_host_insert(sb, keys[i], numerators[i], session_first(source, (uint32_t)i, SESSION_OUTSIDE_FRACTION), values + i * n_ids);
  }
  sb->tuples += tuples;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_add_verifier_side(r0h_session_balance* sb, const uint8_t* elf, size_t elf_len, const uint8_t* journal, size_t journal_len) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb, "r0h_session_balance_add_verifier_side: NULL argument");
  // the trace circuit's session tuple: 1 under alpha_g, -address under "one", -lo, -hi, -tag under gamma, gamma^2, gamma^3 (claim.cpp)
  const uint64_t want[5] = {2ull << 32 | R0H_TRACE_GAMMA, 0, 2ull << 32 | (R0H_TRACE_GAMMA + 4), 2ull << 32 | (R0H_TRACE_GAMMA + 8), 2ull << 32 | (R0H_TRACE_GAMMA + 12)};
  size_t at[5];
  for (int k = 0; k < 5; k++) at[k] = (size_t)(std::find(sb->ids.begin(), sb->ids.end(), want[k]) - sb->ids.begin());
  R0H_REQUIRE(!memcmp(sb->circuit.info, "R0HIP_TRACE:v5__", 16) && sb->ids.size() == 5 && *std::max_element(at, at + 5) < 5,
              "r0h_session_balance_add_verifier_side: the handle's circuit is not the trace circuit");
  R0H_REQUIRE(journal_len % 4 == 0 || !journal, "r0h_session_balance_add_verifier_side: a journal of %zu bytes: COMMIT moves words", journal_len);
  auto side = [&](uint32_t source, const std::vector<std::pair<uint32_t, uint32_t>>& words, uint32_t tag) -> const char* {
    std::vector<uint32_t> num(words.size(), P - 1), val(5 * words.size());
    for (size_t i = 0; i < words.size(); i++) {
      uint32_t* v = &val[5 * i];
      v[at[0]] = 1;
      v[at[1]] = (P - words[i].first % P) % P;
      v[at[2]] = (P - (words[i].second & 0xffffu)) % P;
      v[at[3]] = (P - (words[i].second >> 16)) % P;
      v[at[4]] = P - tag;
    }
    for (size_t i = 0; i < words.size(); i += SESSION_MAX_LIST) {  // (rows of a later call would start at 0 again: an image of more than 2^24 words is not met)
      R0H_REQUIRE(i == 0, "r0h_session_balance_add_verifier_side: more than 2^24 words on one side");
      R0H_TRY(r0h_session_balance_add_tuples(sb, source, num.data(), val.data(), words.size()));
    }
    return nullptr;
  };
  if (elf) {
    std::vector<std::pair<uint32_t, uint32_t>> image;
    uint32_t entry = 0;
    uint8_t image_id[32];
    R0H_TRY(elf_image(elf, elf_len, image, &entry, image_id));
    R0H_TRY(side(R0H_SESSION_SOURCE_IMAGE, image, R0H_SESSION_TAG_IMAGE));
  }
  if (journal) {
    std::vector<std::pair<uint32_t, uint32_t>> words;
    for (size_t j = 0; j < journal_len / 4; j++) {
      const uint8_t* b = journal + 4 * j;
      words.emplace_back(R0H_JOURNAL_BASE / 4 + (uint32_t)j, (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24);
    }
    R0H_TRY(side(R0H_SESSION_SOURCE_JOURNAL, words, R0H_SESSION_TAG_JOURNAL));
  }
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_report(r0h_session_balance* sb, r0h_session_imbalance* out, size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && n_out && (out || !capacity), "r0h_session_balance_report: NULL argument");
  *n_out = 0;
  if (sb->ctx) return session_table_report(sb, out, capacity, n_out);
  std::vector<const SessionClass*> bad;
  for (const auto& kv : sb->classes)
    if (kv.second.sum % P) bad.push_back(&kv.second);
  std::sort(bad.begin(), bad.end(), [](const SessionClass* a, const SessionClass* b) { return a->first < b->first; });
  *n_out = bad.size();
  for (size_t k = 0; k < bad.size() && k < capacity; k++) {
    const SessionClass& cl = *bad[k];
    out[k] = r0h_session_imbalance{(uint32_t)(cl.first >> 32), (uint32_t)(cl.first & 255u), (uint32_t)(cl.first >> 8) & 0xffffffu, (uint32_t)(cl.sum % P),
                                   (uint32_t)std::min<uint64_t>(cl.members, 0xffffffffull), (uint32_t)sb->ids.size(), {0, 0, 0, 0, 0, 0, 0, 0}};
    memcpy(out[k].values, cl.values, sizeof cl.values);
  }
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_message(r0h_session_balance* sb, char** text_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && text_out, "r0h_session_balance_message: NULL argument");
  *text_out = nullptr;
  r0h_session_imbalance first;
  size_t n_bad = 0;
  R0H_TRY(r0h_session_balance_report(sb, &first, 1, &n_bad));
  if (!n_bad) return nullptr;
  std::string cls;
  for (uint32_t k = 0; k < first.n_values; k++) cls += (k ? ", " : "") + std::to_string(first.values[k]);
  // (make_error's strings are what r0h_free_error releases)
  *text_out = const_cast<char*>(make_error("session fraction %u does not balance: net %u over %u tuples, first in source %u at row %u, class (%s); %zu classes in all", first.fraction, first.net,
                                           first.members, first.source, first.first_row, cls.c_str(), n_bad));
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_stats(r0h_session_balance* sb, uint64_t stats_out[4]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && stats_out, "r0h_session_balance_stats: NULL argument");
  stats_out[0] = sb->tuples;
  stats_out[1] = 0;
  stats_out[2] = sb->grows;
  stats_out[3] = sb->classes.size();
  if (sb->ctx) R0H_TRY(session_table_stats(sb, &stats_out[1], &stats_out[3]));
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_ctx_set_check_session(r0h_ctx* ctx, int on) {
  R0H_REQUIRE(ctx, "r0h_ctx_set_check_session: ctx is NULL");
  ctx->check_session = on != 0;
  for (r0h_ctx* h : ctx->helpers) h->check_session = ctx->check_session;
  return nullptr;
}

}  // extern "C"
