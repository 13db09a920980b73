// The circuit blob's parser: host tables of an r0h_circuit from the words of include/r0hip_circuit.h, with every index the
// sequencer, the verifier, the code generator and the column programs later follow validated here.  This is the one function that
// reads an untrusted circuit; it is plain host code (no device work, no HIP call), and tools/fuzz builds it as such.
#include "circuit.hpp"

namespace r0h {

const char* parse_blob(r0h_circuit* c, const uint32_t* w, size_t n_words) {
  R0H_REQUIRE(n_words >= 3 && w[0] == R0H_BLOB_MAGIC && w[1] == 1, "circuit blob: bad magic or version");
  size_t pos = 3;
  bool seen[16] = {false};
  for (uint32_t s = 0; s < w[2]; s++) {
    R0H_REQUIRE(pos + 2 <= n_words, "circuit blob: truncated section header");
    uint32_t tag = w[pos], len = w[pos + 1];
    const uint32_t* p = w + pos + 2;
    R0H_REQUIRE(pos + 2 + len <= n_words, "circuit blob: section %u overruns the blob", tag);
    if (tag < 16) seen[tag] = true;
    switch (tag) {
      case R0H_SEC_GROUPS:
        R0H_REQUIRE(len >= 3, "circuit blob: GROUPS too short");
        memcpy(c->group_size, p, 12);
        break;
      case R0H_SEC_TAPS: {
        R0H_REQUIRE(len >= 1 && len == 1 + 3 * (size_t)p[0], "circuit blob: TAPS length mismatch");
        c->taps.resize(p[0]);
        if (p[0]) memcpy(c->taps.data(), p + 1, 12 * (size_t)p[0]);
        break;
      }
      case R0H_SEC_GLOBALS:
        R0H_REQUIRE(len >= 2 && (len == 2 + (size_t)p[0] || len == 2), "circuit blob: GLOBALS length mismatch");
        if (len == 2) { c->n_global = p[0]; c->n_mix = p[1]; c->global_cols.assign(p[0], 0); break; }
        c->n_global = p[0]; c->n_mix = p[1];
        c->global_cols.assign(p + 2, p + 2 + p[0]);
        break;
      case R0H_SEC_POLY:
        R0H_REQUIRE(len >= 2 && len == 2 + 4 * (size_t)p[0], "circuit blob: POLY length mismatch");
        c->ret = p[1];
        c->steps.resize(p[0]);
        if (p[0]) memcpy(c->steps.data(), p + 2, 16 * (size_t)p[0]);
        break;
      case R0H_SEC_WITGEN: {
        R0H_REQUIRE(len >= 1 && len >= 2 + 2 * (size_t)p[0], "circuit blob: WITGEN too short");
        c->code_cols.resize(p[0]);
        if (p[0]) memcpy(c->code_cols.data(), p + 1, 8 * (size_t)p[0]);
        const uint32_t* q = p + 1 + 2 * (size_t)p[0];
        R0H_REQUIRE(len == 2 + 2 * (size_t)p[0] + 5 * (size_t)q[0], "circuit blob: WITGEN length mismatch");
        c->data_cols.resize(q[0]);
        if (q[0]) memcpy(c->data_cols.data(), q + 1, 20 * (size_t)q[0]);
        break;
      }
      case R0H_SEC_ACCUM:
        R0H_REQUIRE(len >= 1 && len == 1 + 3 * (size_t)p[0], "circuit blob: ACCUM length mismatch");
        c->acc_cols.resize(p[0]);
        if (p[0]) memcpy(c->acc_cols.data(), p + 1, 12 * (size_t)p[0]);
        break;
      case R0H_SEC_ACCUM_FP: return make_error("circuit blob: section 8 (ACCUM_FP) is retired");
      case R0H_SEC_INFO:
        R0H_REQUIRE(len == 4, "circuit blob: INFO must be 4 words");
        memcpy(c->info, p, 16);
        break;
      case R0H_SEC_LATE:
        R0H_REQUIRE(len == 1, "circuit blob: LATE must be 1 word");
        c->n_late = p[0];
        break;
      case R0H_SEC_PERIODIC:
        R0H_REQUIRE(len >= 2 && p[0] && (uint64_t)p[0] * p[1] + 2 == len, "circuit blob: PERIODIC length mismatch");
        c->period = p[0];
        c->periodic.assign(p + 2, p + len);
        for (uint32_t v : c->periodic) R0H_REQUIRE(v < P, "circuit blob: PERIODIC value is not a canonical field word");
        break;
      case R0H_SEC_SPONGE:
        R0H_REQUIRE(len == 3, "circuit blob: SPONGE must be 3 words");
        c->has_sponge = true; c->sponge_code = p[0]; c->sponge_data = p[1]; c->sponge_global = p[2];
        break;
      case R0H_SEC_LOGUP: {
        size_t at = 0;
        auto word = [&](uint32_t* out) -> bool { if (at >= len) return false; *out = p[at++]; return true; };
        auto form = [&](Lf* lf) -> bool {
          uint32_t n;
          if (!word(&n) || n > 64) return false;
          lf->terms.resize(n);
          for (LfTerm& t : lf->terms)
            if (!word(&t.coef) || !word(&t.global) || !word(&t.col) || t.coef >= P) return false;
          return true;
        };
        uint32_t n_acc = 0, n_tab = 0;
        R0H_REQUIRE(word(&n_acc) && word(&n_tab) && n_acc >= 1 && n_acc <= 64 && n_tab <= 8, "circuit blob: LOGUP header");
        c->logup.tables.resize(n_tab);
        for (uint32_t k = 0; k < n_tab; k++) {
          LogupTable& t = c->logup.tables[k];
          R0H_REQUIRE(word(&t.data_col) && word(&t.kind) && (t.kind == R0H_TABLE_R16 || t.kind == R0H_TABLE_AND), "circuit blob: LOGUP table");
          R0H_REQUIRE(t.kind == k + 1, "circuit blob: LOGUP table %u is not of kind %u", k, k + 1);
        }
        c->logup.accs.resize(n_acc);
        bool chain_over = false;
        for (LogupAcc& a : c->logup.accs) {
          uint32_t nf = 0;
          R0H_REQUIRE(word(&nf) && word(&a.final_global) && nf == 4, "circuit blob: a LOGUP accumulator has four fractions");
          if (a.final_global == 0xffffffffu) { R0H_REQUIRE(!chain_over, "circuit blob: LOGUP chain links come first"); c->logup.n_chain++; }
          else chain_over = true;
          a.fr.resize(nf);
          for (LogupFraction& f : a.fr) {
            uint32_t np = 0;
            R0H_REQUIRE(word(&f.table) && f.table <= 2 && form(&f.num) && word(&np) && np >= 1 && np <= 8, "circuit blob: LOGUP fraction");
            f.parts.resize(np);
            for (LogupPart& q : f.parts) R0H_REQUIRE(word(&q.ch_kind) && q.ch_kind <= 2 && word(&q.ch_idx) && form(&q.lf), "circuit blob: LOGUP part");
            if (f.table) {
              R0H_REQUIRE(np == 2 && f.parts[1].ch_kind == 0, "circuit blob: a lookup's value is its second part");
              R0H_REQUIRE(f.table <= n_tab, "circuit blob: a lookup names table %u of %u", f.table, n_tab);
              R0H_REQUIRE(a.final_global == 0xffffffffu, "circuit blob: a lookup in an accumulator with a public total can never balance");
              for (const Lf* lf : {&f.num, &f.parts[1].lf})
                for (const LfTerm& t : lf->terms)
                  R0H_REQUIRE(!t.col || ((t.col - 1) >> 28) == R0H_GROUP_DATA, "circuit blob: a lookup's numerator and value read DATA columns, public inputs and constants only");
            }
          }
        }
        R0H_REQUIRE(at == len, "circuit blob: LOGUP length mismatch");
        break;
      }
      default: break;
    }
    pos += 2 + len;
  }
  for (int t = 1; t <= 4; t++) R0H_REQUIRE(seen[t], "circuit blob: section %d missing", t);
  // WITGEN + ACCUM (the synthetic column program) are optional: a circuit imported from risc0 brings its own witness
  const bool any_accum = seen[R0H_SEC_ACCUM] || seen[R0H_SEC_LOGUP];
  c->has_column_program = seen[R0H_SEC_WITGEN] && any_accum;
  R0H_REQUIRE(seen[R0H_SEC_WITGEN] == any_accum && !(seen[R0H_SEC_ACCUM] && seen[R0H_SEC_LOGUP]), "circuit blob: WITGEN comes with exactly one of ACCUM / LOGUP");
  R0H_REQUIRE(c->n_late <= c->n_global, "circuit blob: more late public inputs than public inputs");
  for (const CodeCol& cc : c->code_cols)
    if (cc.kind == 6) R0H_REQUIRE(c->period && (uint64_t)cc.param * c->period + c->period <= c->periodic.size(), "circuit blob: a periodic CODE column names no column of the PERIODIC section");
  if (c->has_sponge)
    R0H_REQUIRE(c->has_column_program && c->period == R0H_SPONGE_PERIOD && (uint64_t)c->sponge_code + R0H_SPONGE_CODE_COLUMNS <= c->group_size[R0H_GROUP_CODE] &&
                    (uint64_t)c->sponge_data + R0H_SPONGE_DATA_COLUMNS <= c->group_size[R0H_GROUP_DATA] && (uint64_t)c->sponge_global + 8 <= c->n_global && c->global_cols.size() == c->n_global,
                "circuit blob: SPONGE names columns or public inputs outside the circuit");
  if (c->has_column_program) {
    R0H_REQUIRE(c->code_cols.size() == c->group_size[R0H_GROUP_CODE] && c->data_cols.size() == c->group_size[R0H_GROUP_DATA],
                "circuit blob: group sizes disagree with the column programs");
    if (seen[R0H_SEC_ACCUM])
      R0H_REQUIRE(4 * c->acc_cols.size() == c->group_size[R0H_GROUP_ACCUM] && c->n_mix == 8 * c->acc_cols.size(), "circuit blob: group sizes disagree with the accumulators");
    else {
      R0H_REQUIRE(4 * c->logup.accs.size() == c->group_size[R0H_GROUP_ACCUM] && c->logup.n_chain >= 1, "circuit blob: group sizes disagree with the log-derivative accumulators");
      auto form_ok = [&](const Lf& lf) {
        for (const LfTerm& t : lf.terms) {
          if (t.global > c->n_global) return false;
          if (t.col) {
            const uint32_t ref = t.col - 1, g = ref >> 28, col = ref & 0xfffffu;
            if ((g != R0H_GROUP_CODE && g != R0H_GROUP_DATA) || col >= c->group_size[g]) return false;
          }
        }
        return true;
      };
      for (const LogupTable& t : c->logup.tables) R0H_REQUIRE(t.data_col < c->group_size[R0H_GROUP_DATA], "circuit blob: LOGUP multiplicity column out of range");
      for (const LogupAcc& a : c->logup.accs) {
        R0H_REQUIRE(a.final_global == 0xffffffffu || (uint64_t)a.final_global + 4 <= c->n_global, "circuit blob: LOGUP total outside the public inputs");
        for (const LogupFraction& f : a.fr) {
          R0H_REQUIRE(form_ok(f.num), "circuit blob: LOGUP numerator refers outside the circuit");
          for (const LogupPart& q : f.parts)
            R0H_REQUIRE(form_ok(q.lf) && (q.ch_kind == 0 || (q.ch_kind == 1 && 4 * (uint64_t)q.ch_idx + 4 <= c->n_mix) || (q.ch_kind == 2 && (uint64_t)q.ch_idx + 4 <= c->n_global)),
                        "circuit blob: LOGUP part refers outside the circuit");
        }
      }
    }
  }
  // taps: sorted, in range, every column owns back 0
  std::vector<std::vector<bool>> has0(3);
  for (int g = 0; g < 3; g++) has0[g].assign(c->group_size[g], false);
  for (size_t t = 0; t < c->taps.size(); t++) {
    const Tap& tp = c->taps[t];
    R0H_REQUIRE(tp.group < 3 && tp.offset < c->group_size[tp.group] && tp.back < 64, "circuit blob: tap %zu out of range", t);
    if (t) {
      const Tap& pv = c->taps[t - 1];
      bool ordered = pv.group < tp.group || (pv.group == tp.group && (pv.offset < tp.offset || (pv.offset == tp.offset && pv.back < tp.back)));
      R0H_REQUIRE(ordered, "circuit blob: taps not strictly sorted at %zu", t);
    }
    if (tp.back == 0) has0[tp.group][tp.offset] = true;
  }
  for (int g = 0; g < 3; g++)
    for (uint32_t k = 0; k < c->group_size[g]; k++) R0H_REQUIRE(has0[g][k], "circuit blob: group %d column %u has no back-0 tap", g, k);
  // registers and combos
  c->combo_begin.assign(1, 0);
  for (int g = 0; g < 4; g++) c->group_tap_begin[g] = (uint32_t)c->taps.size();
  for (uint32_t t = 0; t < c->taps.size();) {
    uint32_t e = t;
    while (e < c->taps.size() && c->taps[e].group == c->taps[t].group && c->taps[e].offset == c->taps[t].offset) e++;
    uint32_t size = e - t, n_combos = (uint32_t)c->combo_begin.size() - 1, combo = n_combos;
    for (uint32_t k = 0; k < n_combos && combo == n_combos; k++) {
      uint32_t b = c->combo_begin[k];
      if (c->combo_begin[k + 1] - b != size) continue;
      bool same = true;
      for (uint32_t i = 0; i < size; i++) same = same && c->combo_backs[b + i] == c->taps[t + i].back;
      if (same) combo = k;
    }
    if (combo == n_combos) {
      for (uint32_t i = 0; i < size; i++) c->combo_backs.push_back(c->taps[t + i].back);
      c->combo_begin.push_back((uint32_t)c->combo_backs.size());
    }
    c->regs.push_back(Reg{c->taps[t].group, c->taps[t].offset, t, size, combo});
    t = e;
  }
  for (uint32_t t = (uint32_t)c->taps.size(); t-- > 0;) c->group_tap_begin[c->taps[t].group] = t;
  for (int g = 2; g >= 0; g--)
    if (c->group_tap_begin[g] == c->taps.size()) c->group_tap_begin[g] = c->group_tap_begin[g + 1];
  // variable numbering + operand validation
  for (uint32_t i = 0; i < c->steps.size(); i++) {
    const Step& s = c->steps[i];
    uint32_t nf = (uint32_t)c->fp_step.size(), nm = (uint32_t)c->mix_step.size();
    switch (s.op) {
      case R0H_OP_CONST: R0H_REQUIRE(s.a < P, "poly step %u: constant not canonical", i); c->fp_step.push_back(i); break;
      case R0H_OP_GET: R0H_REQUIRE(s.a < c->taps.size(), "poly step %u: tap out of range", i); c->fp_step.push_back(i); break;
      case R0H_OP_GET_GLOBAL:
        R0H_REQUIRE(s.a < 2 && s.b < (s.a == 0 ? c->n_global : c->n_mix), "poly step %u: global out of range", i);
        c->fp_step.push_back(i);
        break;
      case R0H_OP_ADD: case R0H_OP_SUB: case R0H_OP_MUL:
        R0H_REQUIRE(s.a < nf && s.b < nf, "poly step %u: operand not yet defined", i);
        c->fp_step.push_back(i);
        break;
      case R0H_OP_TRUE: c->mix_step.push_back(i); break;
      case R0H_OP_AND_EQZ: R0H_REQUIRE(s.a < nm && s.b < nf, "poly step %u: operand not yet defined", i); c->mix_step.push_back(i); break;
      case R0H_OP_AND_COND: R0H_REQUIRE(s.a < nm && s.b < nf && s.c < nm, "poly step %u: operand not yet defined", i); c->mix_step.push_back(i); break;
      default: return make_error("poly step %u: unknown opcode %u", i, s.op);
    }
  }
  R0H_REQUIRE(c->ret < c->mix_step.size(), "circuit blob: ret is not a mix variable");
  for (uint32_t k = 0; k < c->n_global && c->has_column_program; k++)
    R0H_REQUIRE(c->global_cols[k] < c->data_cols.size(), "circuit blob: global column out of range");
  for (size_t k = 0; k < c->data_cols.size(); k++) {
    const DataCol& d = c->data_cols[k];
    R0H_REQUIRE(d.kind <= 2, "witgen: data column %zu has unknown kind", k);
    if (d.kind == 0) continue;
    const uint32_t refs[4] = {d.a, d.b, d.kind == 2 ? d.c : d.a, d.e};
    for (uint32_t r : refs) {
      uint32_t g = r >> 28, col = r & 0xfffffu;
      R0H_REQUIRE((g == R0H_GROUP_CODE && col < c->code_cols.size()) || (g == R0H_GROUP_DATA && col < k), "witgen: data column %zu has a forward or foreign reference", k);
    }
  }
  for (const AccCol& a : c->acc_cols) R0H_REQUIRE(a.a < c->data_cols.size() && a.b < c->data_cols.size(), "accum: column out of range");
  c->blob.assign(w, w + n_words);
  return nullptr;
}

}  // namespace r0h
