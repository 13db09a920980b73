// Host side of the balance checks (include/r0hip.h; the device's side is csrc/balance.hip): the chain links' check in plain loops
// (r0h_logup_check_balance_host: the compiled form the device's is compared with), and the session balance's handle -- the
// identities, a host handle's classes, the verifier's side, report and message, export and merge (every entry of a merged list is
// checked here, for both kinds of handle); a device handle's table is balance.hip's, behind the
// session_table_* functions.  The tuples come from logup_host.cpp's walk_tuples.
#include <string.h>

#include <algorithm>
#include <unordered_map>

#include "../../include/r0hip_circuit.h"
#include "circuit.hpp"
#include "receipt_types.hpp"

using namespace r0h;

extern "C" {

const char* r0h_logup_check_balance_host(const uint32_t* blob, size_t blob_words, uint32_t po2, const uint32_t* code, const uint32_t* data, const uint32_t* global, r0h_imbalance* out,
                                         size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(blob && data && n_out && (out || !capacity), "r0h_logup_check_balance_host: NULL argument");
  R0H_REQUIRE(po2 >= 4 && po2 <= R0H_MAX_PO2, "r0h_logup_check_balance_host: po2 %u outside [4, %u]", po2, (unsigned)R0H_MAX_PO2);
  r0h_circuit c;
  R0H_TRY(parse_blob(&c, blob, blob_words));
  *n_out = 0;
  const uint32_t n_chain = c.logup.n_chain;
  R0H_REQUIRE(((uint64_t)(4 * n_chain) << po2) <= 0xffffffffull, "r0h_logup_check_balance_host: %u fractions on 2^%u rows: more than 2^32 - 1 tuples", 4 * n_chain, po2);
  for (uint32_t i = 0; i + c.n_late < c.n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_logup_check_balance_host: global[%u] not canonical", i);
  struct Class { uint64_t sum = 0, first = ~0ull, members = 0; };
  std::unordered_map<uint64_t, Class> classes;
  R0H_TRY(walk_tuples("r0h_logup_check_balance_host", c, 0, n_chain, po2, code, data, global, [&](const HostTuple& t) -> const char* {
    Class& cl = classes[t.key];
    cl.sum += t.numerator;
    cl.members++;
    cl.first = std::min<uint64_t>(cl.first, (uint64_t)t.row << 32 | t.fraction);
    return nullptr;
  }));
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
  const uint32_t first_late = c.n_global - c.n_late, n_chain = c.logup.n_chain, n_own = (uint32_t)c.logup.accs.size() - n_chain;
  auto check = [&](const Lf& lf, uint32_t fraction) -> const char* {
    for (const LfTerm& t : lf.terms) {
      R0H_REQUIRE(!t.global || t.global - 1 < first_late, "r0h_session_balance_new: fraction %u reads the value of late public input %u: it does not exist before the challenge", fraction, t.global - 1);
      sb->reads_global |= t.global != 0;
    }
    return nullptr;
  };
  for (uint32_t j = n_chain; j < n_chain + n_own; j++)
    for (uint32_t slot = 0; slot < c.logup.accs[j].fr.size(); slot++) {
      const LogupFraction& f = c.logup.accs[j].fr[slot];
      R0H_TRY(check(f.num, 4 * j + slot));
      for (const LogupPart& q : f.parts) R0H_TRY(check(q.lf, 4 * j + slot));
    }
  sb->ids = tuple_identities(c, n_chain, n_own);
  R0H_REQUIRE(sb->ids.size() <= SESSION_MAX_IDS, "r0h_session_balance_new: %zu challenge identities under the public-total accumulators: more than %u", sb->ids.size(), SESSION_MAX_IDS);
  sb->weights = balance_weights(sb->ids);
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
  for (uint32_t i = 0; i + c.n_late < c.n_global; i++) R0H_REQUIRE(!global || global[i] < P, "r0h_session_balance_add_host: global[%u] not canonical", i);
  return walk_tuples("r0h_session_balance_add_host", c, c.logup.n_chain, (uint32_t)c.logup.accs.size() - c.logup.n_chain, po2, code, data, global, [&](const HostTuple& t) -> const char* {
    R0H_TRY(session_room(sb, 1, "r0h_session_balance_add_host"));
    session_host_insert(sb, t.key, t.numerator, session_first(source, t.row, t.fraction), t.sums);
    sb->tuples++;
    return nullptr;
  });
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
  for (size_t k = 0; k < bad.size() && k < capacity; k++) out[k] = session_entry(bad[k]->first, bad[k]->sum, bad[k]->members, sb->ids.size(), bad[k]->values);
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

const char* r0h_session_balance_export(r0h_session_balance* sb, r0h_session_class* out, size_t capacity, size_t* n_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(sb && n_out && (out || !capacity), "r0h_session_balance_export: NULL argument");
  *n_out = 0;
  std::vector<r0h_session_class> all;
  if (sb->ctx) {
    R0H_TRY(session_table_export(sb, &all));
  } else {
    all.reserve(sb->classes.size());
    for (const auto& kv : sb->classes) {
      const SessionClass& cl = kv.second;
      r0h_session_class e = {kv.first, (uint32_t)(cl.sum % P), (uint32_t)std::min<uint64_t>(cl.members, 0xffffffffull), (uint32_t)(cl.first >> 32), (uint32_t)(cl.first >> 8) & 0xffffffu,
                             (uint32_t)(cl.first & 255u), (uint32_t)sb->ids.size(), {0, 0, 0, 0, 0, 0, 0, 0}};
      memcpy(e.values, cl.values, sizeof e.values);
      all.push_back(e);
    }
  }
  std::sort(all.begin(), all.end(), [](const r0h_session_class& a, const r0h_session_class& b) { return a.key < b.key; });  // (a key is held once)
  *n_out = all.size();
  if (!all.empty() && capacity) memcpy(out, all.data(), std::min(all.size(), capacity) * sizeof(r0h_session_class));
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_session_balance_merge(r0h_session_balance* sb, const r0h_session_class* classes, size_t n) {
  R0H_GUARD_BEGIN
  static_assert(sizeof(r0h_session_class) == 64, "a class travels as one 64-byte record");
  R0H_REQUIRE(sb && (classes || !n), "r0h_session_balance_merge: NULL argument");
  R0H_REQUIRE(n <= SESSION_MAX_LIST, "r0h_session_balance_merge: %zu classes in one call: more than 2^24", n);
  const size_t n_ids = sb->ids.size();
  std::vector<r0h_session_class> list(classes, classes + n);  // what is taken in: the words behind n_values are zero whatever the caller left there
  std::vector<uint64_t> keys(n);
  uint64_t members = 0;
  for (size_t i = 0; i < n; i++) {
    r0h_session_class& e = list[i];
    R0H_REQUIRE(e.n_values == n_ids, "r0h_session_balance_merge: entry %zu has %u values, the handle has %zu identities", i, e.n_values, n_ids);
    R0H_REQUIRE(e.key, "r0h_session_balance_merge: entry %zu has key 0", i);
    R0H_REQUIRE(e.net < P, "r0h_session_balance_merge: net of entry %zu is not canonical", i);
    R0H_REQUIRE(e.fraction <= SESSION_OUTSIDE_FRACTION, "r0h_session_balance_merge: entry %zu has fraction %u: more than 255", i, e.fraction);
    R0H_REQUIRE(e.first_row < (1u << 24), "r0h_session_balance_merge: entry %zu has first row %u: not below 2^24", i, e.first_row);
    uint32_t h0 = 0, h1 = 0;
    for (size_t k = 0; k < 8; k++) {
      if (k >= n_ids) {
        e.values[k] = 0;
        continue;
      }
      R0H_REQUIRE(e.values[k] < P, "r0h_session_balance_merge: value %zu of entry %zu is not canonical", k, i);
      h0 = add(h0, mul(sb->weights[k], enc(e.values[k])));
      h1 = add(h1, mul(sb->weights[n_ids + k], enc(e.values[k])));
    }
    R0H_REQUIRE(e.key == balance_key(h0, h1), "r0h_session_balance_merge: the key of entry %zu is not the fingerprint of its values", i);
    keys[i] = e.key;
    members += e.members;
  }
  std::sort(keys.begin(), keys.end());
  const uint64_t distinct = (uint64_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
  if (sb->ctx) {
    R0H_TRY(session_table_merge(sb, list.data(), n, distinct));
  } else {
    for (const r0h_session_class& e : list) {
      auto it = sb->classes.find(e.key);
      if (it == sb->classes.end()) {
        it = sb->classes.emplace(e.key, SessionClass()).first;
        memcpy(it->second.values, e.values, sizeof e.values);
      }
      SessionClass& cl = it->second;
      cl.sum = (cl.sum + e.net) % P;
      cl.members = std::min<uint64_t>(cl.members + e.members, 0xffffffffull);
      cl.first = std::min(cl.first, session_first(e.source, e.first_row, e.fraction));
    }
  }
  sb->tuples = std::min<uint64_t>(sb->tuples + members, 0xffffffffull);
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
