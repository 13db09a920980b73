// Stand-alone host check (no GPU, no Python) of the two plain-C++ pieces of the log-derivative kernels, meant for a sanitizer build:
//   1. the lookup list (logup_lookup_list, csrc/logup_host.cpp): the list is walked here as logup_count_kernel walks it -- per table and
//      half of its values, zero and the gated-off slots counted on their own, entry 0 by subtraction -- and the multiplicity columns are
//      compared with r0h_logup_multiplicities_host, which follows the circuit's own description of the lookups;
//   2. fp4_batch_div (csrc/fp.hpp): batches of one to four quotients against top * fp4_inv(den) word for word, over random words and
//      the corners of [0, p), zero denominators among them.
// Build and run: tools/fuzz/run_logup_check.sh (writes a generated circuit and its witness with tests/logup_circuits.py first).
//   logup_host_check BLOB DATA GLOBAL PO2 [N_FIELD_CASES]
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static uint32_t list_form(const std::vector<uint32_t>& list, uint32_t& at, const uint32_t* data, size_t n, size_t r) {
  const uint32_t terms = list.at(at++);
  uint32_t acc = 0;
  for (uint32_t k = 0; k < terms; k++) {
    const uint32_t coef = list.at(at), col = list.at(at + 1);
    at += 2;
    acc = add(acc, col ? mul(coef, data[(size_t)(col - 1) * n + r]) : coef);
  }
  return acc;
}

// the multiplicity columns from the list, as the device counts them; returns the error bits
static uint32_t count_from_list(const r0h_circuit& c, const LookupList& list, uint32_t po2, std::vector<uint32_t>& data) {
  const size_t n = (size_t)1 << po2;
  uint32_t err = 0;
  for (size_t k = 0; k < c.logup.tables.size(); k++) {
    std::vector<uint32_t> hist(65536, 0);
    uint32_t binned = 0, gated = 0;
    for (uint32_t half = 0; half < 2; half++) {
      const uint32_t lo = half * 32768u;
      for (size_t r = 0; r < n; r++) {
        uint32_t at = list.begin[k];
        for (uint32_t e = 0; e < list.entries[k]; e++) {
          const uint32_t num = list_form(list.words, at, data.data(), n, r), value = list_form(list.words, at, data.data(), n, r);
          if (num != ONE) {
            if (num) err |= 1u;
            else if (half == 0) gated++;
            continue;
          }
          uint32_t v = dec(neg(value));
          if (k + 1 == R0H_TABLE_AND) {
            v -= R0H_TAG_AND;
            if (v >> 24 || ((v & 255u) & ((v >> 8) & 255u)) != v >> 16) { err |= 2u; continue; }
            v &= 0xffffu;
          } else if (v >> 16) {
            err |= 2u;
            continue;
          }
          if (v && v - lo < 32768u) { hist.at(lo + (v - lo))++; binned++; }
        }
        if (at != list.begin[k + 1]) { fprintf(stderr, "table %zu: the list's entries end at word %u, not %u\n", k, at, list.begin[k + 1]); exit(1); }
      }
    }
    uint32_t* col = data.data() + (size_t)c.logup.tables[k].data_col * n;
    const uint32_t total = (uint32_t)((uint64_t)list.entries[k] * n);
    for (size_t r = 0; r < n; r++) col[r] = enc(r == 0 ? total - binned - gated : r < 65536 ? hist[r] : 0u);
  }
  return err;
}

static const uint32_t EXTREME[] = {0, 1, 2, P - 1, P - 2, (P - 1) / 2, (P + 1) / 2, 0x78000000u, 0x0FFFFFFFu, 0x70000000u};

template <int NB>
static size_t check_batches(std::mt19937_64& rng, size_t cases) {
  size_t partly_zero = 0;
  for (size_t i = 0; i < cases; i++) {
    Fp4 top[NB], den[NB], want[NB];
    int zeros = 0;
    for (int k = 0; k < NB; k++) {
      const bool extreme = rng() & 1;
      for (int w = 0; w < 4; w++) {
        top[k].e[w] = extreme ? EXTREME[rng() % 10] : (uint32_t)(rng() % P);
        den[k].e[w] = extreme ? EXTREME[rng() % 10] : (uint32_t)(rng() % P);
      }
      if (rng() % 5 == 0) den[k] = fp4_zero();
      zeros += den[k] == fp4_zero();
      want[k] = top[k] * fp4_inv(den[k]);
    }
    partly_zero += zeros > 0 && zeros < NB;
    fp4_batch_div<NB>(top, den);
    for (int k = 0; k < NB; k++)
      if (!(top[k] == want[k])) { fprintf(stderr, "fp4_batch_div<%d>: quotient %d of case %zu differs from top * fp4_inv(den)\n", NB, k, i); exit(1); }
  }
  return partly_zero;
}

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s BLOB DATA GLOBAL PO2 [N_FIELD_CASES]\n", argv[0]); return 2; }
  const std::vector<uint32_t> blob = read_words(argv[1]), data = read_words(argv[2]), global = read_words(argv[3]);
  const uint32_t po2 = (uint32_t)atoi(argv[4]);
  const size_t cases = argc > 5 ? (size_t)atol(argv[5]) : 4000;
  r0h_circuit c;
  const char* e = parse_blob(&c, blob.data(), blob.size());
  if (e) { fprintf(stderr, "%s\n", e); return 1; }
  if (data.size() != (size_t)c.group_size[R0H_GROUP_DATA] << po2 || global.size() < c.n_global) { fprintf(stderr, "witness does not fit the circuit\n"); return 2; }
  LookupList list;
  if ((e = logup_lookup_list(&c, global.data(), &list))) { fprintf(stderr, "%s\n", e); return 1; }
  std::vector<uint32_t> from_list = data, from_host = data;
  const uint32_t err = count_from_list(c, list, po2, from_list);
  e = r0h_logup_multiplicities_host(blob.data(), blob.size(), po2, from_host.data(), global.data());
  if ((err != 0) != (e != nullptr)) { fprintf(stderr, "the list's error bits are %u, the host count says: %s\n", err, e ? e : "no error"); return 1; }
  if (!e && from_list != from_host) { fprintf(stderr, "the multiplicity columns counted from the list differ from the host count's\n"); return 1; }
  printf("lookup list: %u + %u entries over %u columns, 2^%u rows: %s\n", list.entries[0], list.entries[1], list.n_cols, po2,
         e ? "both refuse the witness" : "columns equal to the host count's");
  free((void*)e);
  std::mt19937_64 rng(20);
  const size_t pz = check_batches<1>(rng, cases) + check_batches<2>(rng, cases) + check_batches<3>(rng, cases) + check_batches<4>(rng, cases);
  printf("fp4_batch_div: %zu batches of 1..4 equal to separate inversions (%zu of them partly zero)\n", 4 * cases, pz);
  return 0;
}
