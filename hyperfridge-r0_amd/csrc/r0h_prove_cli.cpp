// r0h_prove: a minimal compiled host over the C ABI (no Python, no torch): load a circuit blob, generate a synthetic
// witness on the device, prove K segments, print throughput and a digest of the seal.
// It stands where hyperfridge's `host prove-camt53` stands relative to risc0 (host/src/main.rs:420-423 obtains a prover and
// calls prove once); everything risc0-specific above the segment prover (executor, receipts) is out of scope.
//   usage: r0h_prove <circuit.r0c> [--code-object file.hsaco] [--po2 N] [--segments K] [--seed S] [--device D] [--contexts C] [--seal-out file] [--verify 1] [--verify-device 1] [--hashfn poseidon2|sha-256]
//                    [--receipt-out file.json | --receipt-dir dir] [--journal text] [--receipts R]
// --hashfn sha-256 proves (and with --verify 1 checks) the segments under the SHA-256 hash suite; receipts name Poseidon2 only, so it is
// refused together with any of the receipt options and with --elf.
// --device-transcript 1 (both modes) turns r0h_ctx_set_device_transcript on: the FRI commitments and the queries of every proof run on a transcript
// on the device, one read-back for both steps; the seals and receipts are the same words.
// --device-finish 1 (both modes) turns r0h_ctx_set_device_finish on: every step of a proof's second half runs on that transcript, one read-back
// for all of them; the seals and receipts are the same words.
// --check-witness 1 (both modes; [--check-code-object file.hsaco] [--term-names file.txt]) turns r0h_ctx_set_check_witness on: every segment's
// witness is checked on the device before its ACCUM group is committed, and a violated segment ends the run with the term, its row count
// and its first row -- and the term's name, from --term-names or <circuit>.terms.txt beside the blob (one name per line, in term
// order: tools/gen_circuit.py --names; the build writes them for the trace and image circuits).
// --check-balance 1 (both modes; [--fraction-names file.txt]) turns r0h_ctx_set_check_balance on: the chain links' fractions of every
// segment's witness must cancel class by class (r0h_logup_check_balance) before its DATA group is committed, and a segment that does not
// balance ends the run with the fraction, the net of its class, its tuples and its first row -- and the fraction's name, from
// --fraction-names or <circuit>.fractions.txt beside the blob (tools/gen_circuit.py --fraction-names; the build writes them for the trace
// and image circuits).  A circuit without a LOGUP section has nothing to check.
// --check-session 1 (--elf mode; [--fraction-names file.txt]) turns r0h_ctx_set_check_session on: before the session challenge is derived,
// the session tuples of all segments must cancel against one another, the ELF's image words and the journal's words
// (r0h_session_balance_*); a session that does not balance ends the run with the lowest class -- fraction, net, tuples, the segment and
// row of its first member, the class's values -- and the fraction's name from the same file (its lines go on past the chain's fractions).
// --session-device-limit-gb G (--elf mode, trace circuit) sets r0h_ctx_set_session_device_limit on every session context: the segments a
// session cannot keep committed within G GiB wait for the challenge as their compact rows and are committed again when it is known; the
// receipt is the one an unlimited run writes, and the result line says how many segments were evicted.
// --session-keep-tree-tops L (with it) sets r0h_ctx_set_session_tree_tops: an evicted segment also keeps the top of its DATA tree, down to
// L levels above the leaves (1..8; 6 is 4 MiB per 2^20-row segment), and is committed again without hashing; the result line says how
// many segments were replayed from their top.
// With --receipt-out / --receipt-dir every segment is proved for a claim (risc0-zkvm `ReceiptClaim`): the session's system states
// are synthetic names (there is no executor here), segment k runs from state k to state k+1, all but the last end in SystemSplit,
// the last halts with the journal's output; the claim's eight naming words are planted as the segment's public inputs.  The image
// id (digest of state 0) and the control root of the trace size are printed for the verifier (`r0h_verify --receipt`).
//
//   usage: r0h_prove <trace.r0c> --elf guest.elf --input words.bin [--code-object file.hsaco] [--po2 N] [--device D] --receipt-out file.json
//                    [--receipts R --contexts C --receipt-dir dir]   R sessions of the guest, C in flight (BASELINE.json configs[3]), each receipt verified with the ELF
//                    [--image-circuit circuits/image.r0c --image-code-object circuits/image.evalcheck.hsaco]   the receipts carry an image proof and are also
//                    verified with the image id alone (r0h_receipt_verify_image: the reference's `receipt.verify(image_id)`)
// `prover.prove(env, ELF)` itself (host/src/main.rs:420-423) as a compiled host: the guest ELF is executed on the u32 input stream
// (the ExecutorEnv frames, little-endian words in a file), every segment is proved (r0h_prove_elf: with circuits/trace.r0c the
// seals are proofs over the segments' own cycles), the receipt is written as JSON, and one line of JSON names the image id in
// the reference's IMAGE_ID.hex form, the control root of every trace size used, the cycle and segment counts and the timing.
//
//   usage: r0h_prove <trace.r0c> --elf circuits/guest_camt53.elf --camt53-response response.xml --pub-bank b.pem --pub-client c.pem --pub-witness w.pem
//                    --tx-key-raw TransactionKeyDecrypt.bin --witness-hex Witness.hex --iban CH.. [--hostinfo text] [--form 1] --receipt-out file.json
// the reference's `host` from its inputs on (host/src/main.rs:389-423): instead of --input, the guest's input words are built from the
// EBICS response, the three public keys, the decrypted transaction key and the witness signature (r0h_camt53_guest_input; r0h_preprocess
// makes the last two from the private keys) -- response.xml to receipt with the compiled hosts alone.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/r0hip.h"

static std::vector<std::string> term_names;  // --check-witness: what a violated term is called (empty: its number is all there is)
static std::vector<std::string> fraction_names;  // --check-balance: likewise for a fraction that does not balance
static void die(const char* what, const char* err) {
  fprintf(stderr, "r0h_prove: %s: %s\n", what, err);
  const char* fr = strstr(err, ": fraction ");
  if (!fr) fr = strstr(err, ": session fraction ");  // --check-session
  if (fr && strstr(fr, " does not balance: net ")) {
    const unsigned long f = strtoul(strstr(fr, "fraction ") + 9, nullptr, 10);
    if (f < fraction_names.size()) fprintf(stderr, "r0h_prove: fraction %lu is \"%s\"\n", f, fraction_names[f].c_str());
  }
  const char* at = strstr(err, "the witness violates");
  if (at && (at = strstr(at, ": term "))) {
    const unsigned long t = strtoul(at + 7, nullptr, 10);
    if (t < term_names.size()) fprintf(stderr, "r0h_prove: term %lu is constraint \"%s\"\n", t, term_names[t].c_str());
  }
  r0h_free_error(err);
  exit(2);
}
#define CHECK(call)                      \
  do {                                   \
    const char* e__ = (call);            \
    if (e__) die(#call, e__);            \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2 || !strcmp(argv[1], "--help") || !strcmp(argv[1], "-h")) {
    printf("usage: r0h_prove <circuit.r0c> [--code-object file.hsaco] [--po2 N] [--segments K] [--seed S] [--device D] [--contexts C] [--seal-out file] [--verify 1] [--verify-device 1] [--hashfn poseidon2|sha-256] [--receipt-out file.json | --receipt-dir dir] [--journal text] [--receipts R]\n"
           "       r0h_prove <trace.r0c> --elf guest.elf --input words.bin [--code-object file.hsaco] [--po2 N] [--device D] --receipt-out file.json\n"
           "       ... --elf guest.elf --compress --recursion-circuit recursion.r0c [--recursion-code-object file.hsaco] [--recursion-po2 N] [--compress-lanes 1..4] --root-out root.bin: "
           "the receipt's segments lifted and joined into one root (wire form) for r0h_verify --root\n"
           "       --check-witness 1 [--check-code-object file.hsaco] [--term-names file.txt]: check every segment's witness on the device before its ACCUM group is committed; "
           "a violated segment ends the run with the constraint term, its name, how many rows violate it and the first of them\n"
           "       --check-balance 1 [--fraction-names file.txt]: check that the log-derivative fractions of every segment's witness cancel before its DATA group is committed; "
           "a segment that does not balance ends the run with the fraction, its name, the net of its class and its first row\n"
           "       --check-session 1 [--fraction-names file.txt]: with --elf, check before the session challenge is derived that the session tuples of all segments cancel against "
           "one another, the program image and the journal; a session that does not balance ends the run with the fraction, its name, the net of its class, the segment and row of its first tuple "
           "and the class's values (single-rank sessions; a diagnostic, not a verifier)\n"
           "       --session-device-limit-gb G: with --elf over the trace circuit, the committed segments of a session keep at most G GiB on the device between its two phases "
           "(a fraction is fine); a segment beyond that is evicted to its compact rows and committed again when the session is finished -- the same receipt; the run reports "
           "how many were (default: no limit)\n"
           "       --session-keep-tree-tops L: with it, an evicted segment also keeps the top of its DATA tree down to L levels above the leaves (1..8) and is committed again "
           "without hashing -- the same receipt; the run reports how many were replayed from their top (default 0: off)\n"
           "       --device-transcript 0|1: with 1 every proof runs its FRI commitments and its queries on a Fiat-Shamir transcript on the device, with one read-back for both steps "
           "instead of one per commitment and per opened tree -- the same seals and receipts (default 0: the transcript stays on the host)\n"
           "       --device-finish 0|1: with 1 every proof runs ALL the steps of its second half -- ACCUM, CHECK, the openings, DEEP, FRI, the queries -- on the transcript on the "
           "device, with one read-back for all of them, whatever --device-transcript says -- the same seals and receipts (default 0)\n"
           "       --session-enqueue 0|1: with --elf over the trace circuit; with 1 the second phase of every session is driven by the calling thread alone: each segment's session sum, "
           "late inputs, accumulation and finish are enqueued on its lane's stream and collected one segment per lane later -- the same receipt (default: R0H_SESSION_ENQUEUE, else 0)\n"
           "       --session-enqueue-begin 0|1: with --elf over the trace circuit; with 1 the calling thread drives the first phase of every session as well -- no lane threads, the DATA "
           "roots read back once per lane, evicted segments committed again without a wait, the image proof enqueued -- and --session-enqueue 1 is implied; the same receipt "
           "(default: R0H_SESSION_ENQUEUE_BEGIN, else 0)\n"
           "       --merkle-fused-tops 0|1: with 1 every Merkle tree is built with its levels of up to 8192 parents in two launches (r0h_hash_fold_top) instead of one launch per level "
           "-- the same trees, seals and receipts (default: R0H_MERKLE_FUSED_TOPS, else 0)\n%s\n", r0h_version());
    return argc < 2 ? 1 : 0;
  }
  // --compress takes no value: it is taken out of the arguments before the "--option value" pairs are read
  bool compress = false;
  for (int i = 2; i < argc; i++)
    if (!strcmp(argv[i], "--compress")) {
      compress = true;
      for (int k = i; k + 1 < argc; k++) argv[k] = argv[k + 1];
      argc--;
      i--;
    }
  std::string recursion_path, recursion_co_path, root_out;
  unsigned recursion_po2 = 18, compress_lanes = 0;
  std::string blob_path = argv[1], co_path, seal_out, receipt_out, receipt_dir, journal_text, elf_path, input_path;
  std::string hashfn = "poseidon2";         // --hashfn: the hash suite of the synthetic-circuit mode (seals only)
  std::map<std::string, std::string> camt;  // --camt53-response and what goes with it
  std::string receipt_prefix;               // --receipt-prefix P: the reference's file name, P-Receipt-<image id>-latest.json (host/src/main.rs:312-316)
  std::string image_circuit_path, image_co_path, check_co_path, term_names_path, fraction_names_path;
  unsigned check_witness = 0, check_balance = 0, check_session = 0;
  unsigned po2 = 16, segments = 1, device = 0, contexts = 1, verify = 0, receipts = 1, verify_device = 0;
  unsigned long long seed = 1;
  double session_device_limit_gb = 0;  // --session-device-limit-gb: r0h_ctx_set_session_device_limit of every session context
  unsigned session_keep_tree_tops = 0;  // --session-keep-tree-tops: r0h_ctx_set_session_tree_tops of every session context
  std::string device_transcript = "0";  // --device-transcript: r0h_ctx_set_device_transcript of every context
  std::string device_finish = "0";      // --device-finish: r0h_ctx_set_device_finish of every context
  std::string session_enqueue_begin;    // --session-enqueue-begin: r0h_ctx_set_session_enqueue_begin of every session context (not given: the library's default)
  std::string session_enqueue;          // --session-enqueue: r0h_ctx_set_session_enqueue of every session context (not given: the library's default)
  bool merkle_fused_given = false;
  std::string merkle_fused_tops;        // --merkle-fused-tops: r0h_ctx_set_merkle_fused_tops of every context (not given: the library's default)
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--code-object")) co_path = argv[i + 1];
    else if (!strcmp(argv[i], "--po2")) po2 = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--segments")) segments = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--seed")) seed = strtoull(argv[i + 1], nullptr, 10);
    else if (!strcmp(argv[i], "--device")) device = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--contexts")) contexts = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--seal-out")) seal_out = argv[i + 1];
    else if (!strcmp(argv[i], "--verify")) verify = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--verify-device")) verify_device = (unsigned)atoi(argv[i + 1]);  // the after-proof verification hashes its Merkle openings on the proving context
    else if (!strcmp(argv[i], "--hashfn")) hashfn = argv[i + 1];
    else if (!strcmp(argv[i], "--check-witness")) check_witness = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--check-code-object")) check_co_path = argv[i + 1];
    else if (!strcmp(argv[i], "--term-names")) term_names_path = argv[i + 1];
    else if (!strcmp(argv[i], "--check-balance")) check_balance = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--check-session")) check_session = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--fraction-names")) fraction_names_path = argv[i + 1];
    else if (!strcmp(argv[i], "--session-device-limit-gb")) session_device_limit_gb = atof(argv[i + 1]);
    else if (!strcmp(argv[i], "--session-keep-tree-tops")) session_keep_tree_tops = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--device-transcript")) device_transcript = argv[i + 1];
    else if (!strcmp(argv[i], "--device-finish")) device_finish = argv[i + 1];
    else if (!strcmp(argv[i], "--session-enqueue")) session_enqueue = argv[i + 1];
    else if (!strcmp(argv[i], "--session-enqueue-begin")) session_enqueue_begin = argv[i + 1];
    else if (!strcmp(argv[i], "--merkle-fused-tops")) { merkle_fused_tops = argv[i + 1]; merkle_fused_given = true; }
    else if (!strcmp(argv[i], "--receipt-out")) receipt_out = argv[i + 1];
    else if (!strcmp(argv[i], "--receipt-dir")) receipt_dir = argv[i + 1];
    else if (!strcmp(argv[i], "--journal")) journal_text = argv[i + 1];
    else if (!strcmp(argv[i], "--receipts")) receipts = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--elf")) elf_path = argv[i + 1];
    else if (!strcmp(argv[i], "--input")) input_path = argv[i + 1];
    else if (!strcmp(argv[i], "--receipt-prefix")) receipt_prefix = argv[i + 1];
    else if (!strcmp(argv[i], "--image-circuit")) image_circuit_path = argv[i + 1];        // circuits/image.r0c: the receipts carry an image proof
    else if (!strcmp(argv[i], "--image-code-object")) image_co_path = argv[i + 1];
    else if (!strcmp(argv[i], "--recursion-circuit")) recursion_path = argv[i + 1];       // with --compress: circuits/recursion.r0c
    else if (!strcmp(argv[i], "--recursion-code-object")) recursion_co_path = argv[i + 1];
    else if (!strcmp(argv[i], "--recursion-po2")) recursion_po2 = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--compress-lanes")) compress_lanes = (unsigned)atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--root-out")) root_out = argv[i + 1];
    else if (!strcmp(argv[i], "--camt53-response")) camt["response"] = argv[i + 1];  // the library's own camt53 guest fed from an EBICS response
    else if (!strcmp(argv[i], "--pub-bank") || !strcmp(argv[i], "--pub-client") || !strcmp(argv[i], "--pub-witness") || !strcmp(argv[i], "--tx-key-raw") ||
             !strcmp(argv[i], "--witness-hex") || !strcmp(argv[i], "--iban") || !strcmp(argv[i], "--hostinfo") || !strcmp(argv[i], "--form"))
      camt[argv[i] + 2] = argv[i + 1];
    else { fprintf(stderr, "r0h_prove: unknown option %s\n", argv[i]); return 1; }
  }
  if ((argc - 2) % 2) { fprintf(stderr, "r0h_prove: option %s needs a value\n", argv[argc - 1]); return 1; }
  if (compress && (elf_path.empty() || recursion_path.empty() || root_out.empty())) {
    fprintf(stderr, "r0h_prove: --compress goes with --elf and needs --recursion-circuit and --root-out (and takes --recursion-code-object, --recursion-po2, --compress-lanes)\n");
    return 1;
  }
  if (session_device_limit_gb < 0 || (session_device_limit_gb > 0 && elf_path.empty())) {
    fprintf(stderr, "r0h_prove: --session-device-limit-gb takes a size of zero or more and goes with --elf\n");
    return 1;
  }
  if (session_keep_tree_tops > R0H_MERKLE_TOP_MAX_LEVELS || (session_keep_tree_tops && elf_path.empty())) {
    fprintf(stderr, "r0h_prove: --session-keep-tree-tops takes 0 .. %u levels and goes with --elf\n", (unsigned)R0H_MERKLE_TOP_MAX_LEVELS);
    return 1;
  }
  if (device_transcript != "0" && device_transcript != "1") {
    fprintf(stderr, "r0h_prove: --device-transcript is 0 or 1, not %s\n", device_transcript.c_str());
    return 2;
  }
  if (device_finish != "0" && device_finish != "1") {
    fprintf(stderr, "r0h_prove: --device-finish is 0 or 1, not %s\n", device_finish.c_str());
    return 2;
  }
  if (!session_enqueue.empty() && ((session_enqueue != "0" && session_enqueue != "1") || elf_path.empty())) {
    fprintf(stderr, "r0h_prove: --session-enqueue is 0 or 1 and goes with --elf, not %s\n", session_enqueue.c_str());
    return 2;
  }
  if (!session_enqueue_begin.empty() && ((session_enqueue_begin != "0" && session_enqueue_begin != "1") || elf_path.empty())) {
    fprintf(stderr, "r0h_prove: --session-enqueue-begin is 0 or 1 and goes with --elf, not %s\n", session_enqueue_begin.c_str());
    return 2;
  }
  if (merkle_fused_given && merkle_fused_tops != "0" && merkle_fused_tops != "1") {
    fprintf(stderr, "r0h_prove: --merkle-fused-tops is 0 or 1, not %s\n", merkle_fused_tops.c_str());
    return 1;
  }
  if (hashfn != "poseidon2" && hashfn != "sha-256") { fprintf(stderr, "r0h_prove: --hashfn is poseidon2 or sha-256, not %s\n", hashfn.c_str()); return 1; }
  if (hashfn != "poseidon2" && (!elf_path.empty() || !receipt_out.empty() || !receipt_dir.empty() || !receipt_prefix.empty() || !camt.empty() || !image_circuit_path.empty())) {
    fprintf(stderr, "r0h_prove: --hashfn %s proves bare seals (--seal-out / --verify); receipts name poseidon2 only, so it does not go with --elf, --receipt-out, "
                    "--receipt-dir, --receipt-prefix, --image-circuit or --camt53-response\n", hashfn.c_str());
    return 1;
  }
  FILE* f = fopen(blob_path.c_str(), "rb");
  if (!f) { fprintf(stderr, "r0h_prove: cannot open %s\n", blob_path.c_str()); return 1; }
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint32_t> blob((size_t)sz / 4);
  if (fread(blob.data(), 4, blob.size(), f) != blob.size()) { fprintf(stderr, "r0h_prove: short read\n"); return 1; }
  fclose(f);
  if (check_witness) {
    std::string names = term_names_path;
    if (names.empty() && blob_path.size() > 4 && blob_path.compare(blob_path.size() - 4, 4, ".r0c") == 0) names = blob_path.substr(0, blob_path.size() - 4) + ".terms.txt";
    FILE* g = names.empty() ? nullptr : fopen(names.c_str(), "rb");
    if (!g && !term_names_path.empty()) { fprintf(stderr, "r0h_prove: cannot open %s\n", names.c_str()); return 1; }
    char line[256];
    while (g && fgets(line, sizeof line, g)) {
      line[strcspn(line, "\r\n")] = 0;
      term_names.push_back(line);
    }
    if (g) fclose(g);
  }
  if (check_balance || check_session) {
    std::string names = fraction_names_path;
    if (names.empty() && blob_path.size() > 4 && blob_path.compare(blob_path.size() - 4, 4, ".r0c") == 0) names = blob_path.substr(0, blob_path.size() - 4) + ".fractions.txt";
    FILE* g = names.empty() ? nullptr : fopen(names.c_str(), "rb");
    if (!g && !fraction_names_path.empty()) { fprintf(stderr, "r0h_prove: cannot open %s\n", names.c_str()); return 1; }
    char line[256];
    while (g && fgets(line, sizeof line, g)) {
      line[strcspn(line, "\r\n")] = 0;
      fraction_names.push_back(line);
    }
    if (g) fclose(g);
  }
  // --check-witness: the context's switch, and the checker's module now (from its code object, else compiled in-process) rather than inside the first proof
  auto arm_checker = [&](r0h_ctx* ctx, r0h_circuit* circ) {
    if (session_device_limit_gb > 0) CHECK(r0h_ctx_set_session_device_limit(ctx, std::max<uint64_t>(1, (uint64_t)(session_device_limit_gb * (double)(1ull << 30)))));
    if (session_keep_tree_tops) CHECK(r0h_ctx_set_session_tree_tops(ctx, session_keep_tree_tops));
    if (device_transcript == "1") CHECK(r0h_ctx_set_device_transcript(ctx, 1));
    if (device_finish == "1") CHECK(r0h_ctx_set_device_finish(ctx, 1));
    if (!session_enqueue.empty()) CHECK(r0h_ctx_set_session_enqueue(ctx, session_enqueue == "1"));
    if (!session_enqueue_begin.empty()) CHECK(r0h_ctx_set_session_enqueue_begin(ctx, session_enqueue_begin == "1"));
    if (merkle_fused_given) CHECK(r0h_ctx_set_merkle_fused_tops(ctx, merkle_fused_tops == "1"));
    if (check_balance) CHECK(r0h_ctx_set_check_balance(ctx, 1));
    if (check_session) CHECK(r0h_ctx_set_check_session(ctx, 1));
    if (!check_witness) return;
    CHECK(r0h_ctx_set_check_witness(ctx, 1));
    CHECK(r0h_circuit_load_check(circ, check_co_path.empty() ? nullptr : check_co_path.c_str()));
  };
  if (!elf_path.empty()) {  // prove(env, elf)
    auto slurp = [](const std::string& path, std::vector<uint8_t>* out) {
      FILE* g = fopen(path.c_str(), "rb");
      if (!g) return false;
      uint8_t buf[65536];
      for (size_t got; (got = fread(buf, 1, sizeof buf, g)) > 0;) out->insert(out->end(), buf, buf + got);
      fclose(g);
      return true;
    };
    std::vector<uint8_t> elf, raw;
    if (!slurp(elf_path, &elf)) { fprintf(stderr, "r0h_prove: cannot open %s\n", elf_path.c_str()); return 1; }
    if (!input_path.empty() && !slurp(input_path, &raw)) { fprintf(stderr, "r0h_prove: cannot open %s\n", input_path.c_str()); return 1; }
    if (raw.size() % 4) { fprintf(stderr, "r0h_prove: --input is a stream of 32-bit words\n"); return 1; }
    if (receipt_out.empty() && receipt_prefix.empty() && receipt_dir.empty()) { fprintf(stderr, "r0h_prove: --elf needs --receipt-out, --receipt-prefix or --receipt-dir\n"); return 1; }
    std::vector<uint32_t> words(raw.size() / 4);
    if (!words.empty()) memcpy(words.data(), raw.data(), raw.size());
    if (camt.count("response")) {
      // what the reference's `host` does between reading the pre-processed files and `prove` (host/src/main.rs:389-417), for this
      // library's camt53 guest: response.xml, the three public keys, the decrypted transaction key block, the witness signature, iban,
      // host info -> the guest's input words (r0h_camt53_guest_input)
      for (const char* need : {"pub-bank", "pub-client", "pub-witness", "tx-key-raw", "witness-hex", "iban"})
        if (!camt.count(need)) { fprintf(stderr, "r0h_prove: --camt53-response needs --%s\n", need); return 1; }
      std::map<std::string, std::vector<uint8_t>> file;
      for (const char* name : {"response", "pub-bank", "pub-client", "pub-witness", "tx-key-raw", "witness-hex"})
        if (!slurp(camt[name], &file[name])) { fprintf(stderr, "r0h_prove: cannot open %s\n", camt[name].c_str()); return 1; }
      r0h_ebics* eb = nullptr;
      CHECK(r0h_ebics_parse((const char*)file["response"].data(), file["response"].size(), &eb));
      uint32_t* stream = nullptr; size_t n_stream = 0;
      auto pem = [&](const char* k) { return (const char*)file[k].data(); };
      CHECK(r0h_camt53_guest_input(eb, pem("pub-bank"), file["pub-bank"].size(), pem("pub-client"), file["pub-client"].size(), pem("pub-witness"), file["pub-witness"].size(),
                                   file["tx-key-raw"].data(), file["tx-key-raw"].size(), pem("witness-hex"), file["witness-hex"].size(), camt["iban"].c_str(),
                                   camt.count("hostinfo") ? camt["hostinfo"].c_str() : "host:main", camt.count("form") ? (uint32_t)atoi(camt["form"].c_str()) : 1u, &stream, &n_stream));
      words.assign(stream, stream + n_stream);
      r0h_free_error((const char*)stream);
      r0h_ebics_free(eb);
    }
    // BASELINE.json configs[3] on the real workload: --receipts R sessions of this guest (host/src/main.rs:389-423 looped by
    // data/watchdog.sh:46-109), --contexts C of them in flight -- each on a context of its own with its own executor thread and
    // prover lanes -- one receipt file each, every receipt verified with the ELF afterwards (outside the timed region)
    if (contexts < 1 || contexts > 8) { fprintf(stderr, "r0h_prove: --contexts must be 1..8 with --elf\n"); return 1; }
    if (receipts > 1 && receipt_dir.empty()) { fprintf(stderr, "r0h_prove: --receipts R > 1 writes one file per receipt: use --receipt-dir\n"); return 1; }
    if (contexts > receipts) contexts = receipts;
    struct Worker { r0h_ctx* ctx = nullptr; r0h_circuit* circ = nullptr; r0h_circuit* image = nullptr; };
    std::vector<Worker> workers(contexts);
    std::vector<uint32_t> image_blob;
    if (!image_circuit_path.empty()) {
      std::vector<uint8_t> bytes;
      if (!slurp(image_circuit_path, &bytes) || bytes.size() % 4) { fprintf(stderr, "r0h_prove: cannot read %s\n", image_circuit_path.c_str()); return 1; }
      image_blob.resize(bytes.size() / 4);
      memcpy(image_blob.data(), bytes.data(), bytes.size());
    }
    for (Worker& w : workers) {
      CHECK(r0h_ctx_create((int)device, &w.ctx));
      CHECK(r0h_circuit_load(w.ctx, blob.data(), blob.size(), co_path.empty() ? nullptr : co_path.c_str(), &w.circ));
      arm_checker(w.ctx, w.circ);
      if (!image_blob.empty()) {  // every receipt then carries an image proof: `receipt.verify(image_id)` needs no ELF
        CHECK(r0h_circuit_load(w.ctx, image_blob.data(), image_blob.size(), image_co_path.empty() ? nullptr : image_co_path.c_str(), &w.image));
        CHECK(r0h_ctx_set_image_circuit(w.ctx, w.image));
      }
    }
    r0h_ctx* ctx = workers[0].ctx;
    r0h_circuit* circ = workers[0].circ;
    std::vector<r0h_receipt*> made(receipts, nullptr);
    uint8_t image_id[32];
    uint64_t cycles = 0;
    std::atomic<unsigned> next_receipt{0};
    auto session_worker = [&](unsigned k) {
      for (unsigned u; (u = next_receipt.fetch_add(1)) < receipts;) {
        uint8_t id[32];
        uint64_t cyc = 0;
        CHECK(r0h_prove_elf(workers[k].ctx, workers[k].circ, elf.data(), elf.size(), words.data(), words.size(), po2, 0, &made[u], id, &cyc));
        if (u == 0) { memcpy(image_id, id, 32); cycles = cyc; }
      }
    };
    const auto t0 = std::chrono::steady_clock::now();
    {
      std::vector<std::thread> threads;
      for (unsigned k = 1; k < contexts; k++) threads.emplace_back(session_worker, k);
      session_worker(0);
      for (auto& t : threads) t.join();
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    r0h_receipt* rc = made[0];
    for (unsigned u = 0; u < receipts; u++) {
      char* text = nullptr;
      CHECK(r0h_receipt_to_json(made[u], &text));
      std::string path = receipt_out;
      if (receipts > 1 || (receipt_out.empty() && receipt_prefix.empty())) {
        char name[64];
        snprintf(name, sizeof name, "/receipt_%04u.json", u);
        path = receipt_dir + name;
      } else if (receipt_out.empty()) {  // where the reference's verifier looks: <camt53 file>-Receipt-<image id>-latest.json
        char id_hex[65];
        CHECK(r0h_image_id_to_hex(image_id, id_hex));
        path = receipt_prefix + "-Receipt-" + id_hex + "-latest.json";
      }
      if (u == 0) receipt_out = path;
      FILE* o = fopen(path.c_str(), "wb");
      if (!o || fwrite(text, 1, strlen(text), o) != strlen(text)) { fprintf(stderr, "r0h_prove: cannot write %s\n", path.c_str()); return 1; }
      fclose(o);
      r0h_free_error(text);
    }
    // the control root of every trace size the segments were proved at: what `r0h_verify --control-root` takes
    const size_t n_seg = r0h_receipt_n_segments(rc);
    std::vector<uint32_t> sizes;
    for (size_t i = 0; i < n_seg; i++) {
      const uint32_t* seal; size_t n_words;
      CHECK(r0h_receipt_segment(rc, i, &seal, &n_words, nullptr));
      int verdict = -1; uint32_t size = 0;
      CHECK(r0h_verify_seal(blob.data(), blob.size(), nullptr, nullptr, seal, n_words, &verdict, &size));
      if (verdict != R0H_VERIFY_OK) { fprintf(stderr, "r0h_prove: the verifier rejects seal %zu: %s\n", i, r0h_verify_reason(verdict)); return 3; }
      if (std::find(sizes.begin(), sizes.end(), size) == sizes.end()) sizes.push_back(size);
    }
    std::vector<uint32_t> root_table;
    for (size_t k = 0; k < sizes.size(); k++) {
      const size_t n = (size_t)1 << sizes[k];
      r0h_buf *code = nullptr, *data = nullptr;
      CHECK(r0h_buf_alloc(ctx, (size_t)r0h_circuit_group_size(circ, R0H_GROUP_CODE) * n * 4, &code));
      CHECK(r0h_buf_alloc(ctx, (size_t)r0h_circuit_group_size(circ, R0H_GROUP_DATA) * n * 4, &data));
      CHECK(r0h_witgen(ctx, circ, sizes[k], 0, code, data, nullptr));  // the circuit's fixed CODE columns
      uint32_t root[8];
      CHECK(r0h_code_root(ctx, code, r0h_circuit_group_size(circ, R0H_GROUP_CODE), sizes[k], root));
      root_table.push_back(sizes[k]);
      root_table.insert(root_table.end(), root, root + 8);
      CHECK(r0h_buf_free(code));
      CHECK(r0h_buf_free(data));
    }
    // every receipt verified the way the reference's verifier would (verifier/src/main.rs:124-126), with the ELF: host threads
    std::atomic<unsigned> next_check{0}, refused{0};
    const auto v0 = std::chrono::steady_clock::now();
    // (--verify-device 1: thread k hashes the seals' Merkle openings on worker k's context, one batch per receipt; every verdict stays the host's)
    auto check_worker = [&](unsigned k) {
      r0h_ctx* on = verify_device ? workers[k].ctx : nullptr;
      for (unsigned u; (u = next_check.fetch_add(1)) < receipts;) {
        int verdict = -1;
        const char* e = on ? r0h_receipt_verify_elf_on(on, made[u], blob.data(), blob.size(), root_table.data(), root_table.size() / 9, elf.data(), elf.size(), &verdict, nullptr, nullptr)
                           : r0h_receipt_verify_elf(made[u], blob.data(), blob.size(), root_table.data(), root_table.size() / 9, elf.data(), elf.size(), &verdict, nullptr, nullptr);
        if (e) { r0h_free_error(e); verdict = -1; }
        if (verdict == R0H_RECEIPT_V_OK && !image_blob.empty()) {  // ... and the way the reference's verifier does: the image id's 32 bytes alone
          e = on ? r0h_receipt_verify_image_on(on, made[u], blob.data(), blob.size(), root_table.data(), root_table.size() / 9, image_blob.data(), image_blob.size(), nullptr, image_id,
                                               &verdict, nullptr, nullptr)
                 : r0h_receipt_verify_image(made[u], blob.data(), blob.size(), root_table.data(), root_table.size() / 9, image_blob.data(), image_blob.size(), nullptr, image_id, &verdict,
                                       nullptr, nullptr);
          if (e) { r0h_free_error(e); verdict = -1; }
        }
        if (verdict != R0H_RECEIPT_V_OK) { fprintf(stderr, "r0h_prove: receipt %u is refused: %s\n", u, r0h_receipt_verify_reason(verdict)); refused++; }
      }
    };
    {
      std::vector<std::thread> threads;
      for (unsigned k = 1; k < std::min(receipts, verify_device ? contexts : 8u); k++) threads.emplace_back(check_worker, k);
      check_worker(0);
      for (auto& t : threads) t.join();
    }
    const double verify_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - v0).count();
    if (refused) return 3;
    // --compress: the first receipt lifted and joined into one root (r0h_compress), written in wire form -- claim words,
    // [n_leaves, seal_words], seal, session words -- for `r0h_verify --root`
    double compress_secs = 0;
    size_t root_leaves = 0;
    if (compress) {
      std::vector<uint8_t> bytes;
      if (!slurp(recursion_path, &bytes) || bytes.size() % 4) { fprintf(stderr, "r0h_prove: cannot read %s\n", recursion_path.c_str()); return 1; }
      std::vector<uint32_t> rec_blob(bytes.size() / 4);
      memcpy(rec_blob.data(), bytes.data(), bytes.size());
      r0h_recursor* recursor = nullptr;
      CHECK(r0h_recursor_new(ctx, rec_blob.data(), rec_blob.size(), recursion_co_path.empty() ? nullptr : recursion_co_path.c_str(), recursion_po2, blob.data(), blob.size(),
                             root_table.data(), root_table.size() / 9, &recursor));
      r0h_node* root = nullptr;
      const auto c0 = std::chrono::steady_clock::now();
      CHECK(r0h_compress(recursor, rc, compress_lanes, &root));
      compress_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
      const uint32_t *seal = nullptr, *session = nullptr;
      size_t seal_words = 0;
      r0h_receipt_claim claim;
      CHECK(r0h_node_seal(root, &seal, &seal_words));
      CHECK(r0h_node_claim(root, &claim));
      CHECK(r0h_node_session(root, &session, &root_leaves));
      const uint32_t head[2] = {(uint32_t)root_leaves, (uint32_t)seal_words};
      FILE* o = fopen(root_out.c_str(), "wb");
      if (!o || fwrite(&claim, 1, sizeof claim, o) != sizeof claim || fwrite(head, 4, 2, o) != 2 || fwrite(seal, 4, seal_words, o) != seal_words ||
          fwrite(session, 4, root_leaves * R0H_NODE_SESSION_WORDS, o) != root_leaves * R0H_NODE_SESSION_WORDS) {
        fprintf(stderr, "r0h_prove: cannot write %s\n", root_out.c_str());
        return 1;
      }
      fclose(o);
      CHECK(r0h_node_free(root));
      CHECK(r0h_recursor_free(recursor));
    }
    char hex[65];
    CHECK(r0h_image_id_to_hex(image_id, hex));
    r0h_session_stats st;
    CHECK(r0h_last_session_stats(ctx, &st));
    uint64_t device[4];  // of the first context's last session
    CHECK(r0h_last_session_device(ctx, device));
    uint64_t tops[3];
    CHECK(r0h_last_session_tree_tops(ctx, tops));
    printf("{\"receipt\": \"%s\", \"image_id\": \"%s\", \"receipts\": %u, \"contexts\": %u, \"segments\": %zu, \"cycles\": %llu, \"seconds\": %.4f, \"segments_per_s\": %.3f, \"receipts_per_s\": %.4f, "
           "\"executor_s\": %.4f, \"evicted_segments\": %llu, \"segments_replayed_from_their_tree_top\": %llu, \"receipts_verified_with_the_elf\": %u, \"receipts_verified_with_the_image_id_alone\": %u, \"verify_seconds\": %.3f, \"control_roots\": [",
           receipt_out.c_str(), hex, receipts, contexts, n_seg, (unsigned long long)cycles, secs, (double)n_seg * receipts / secs, receipts / secs, st.executor_s, (unsigned long long)device[0], (unsigned long long)tops[0], receipts,
           image_blob.empty() ? 0u : receipts, verify_secs);
    for (size_t k = 0; k < sizes.size(); k++) {
      const uint32_t* root = &root_table[9 * k + 1];
      printf("%s\"%u:%u,%u,%u,%u,%u,%u,%u,%u\"", k ? ", " : "", sizes[k], root[0], root[1], root[2], root[3], root[4], root[5], root[6], root[7]);
    }
    printf("]");
    uint64_t phase2[4];  // of the first context's last session
    CHECK(r0h_last_session_phase2(ctx, phase2));
    printf(", \"phase2_host_threads\": %llu, \"phase2_blocking_waits\": %llu", (unsigned long long)phase2[0], (unsigned long long)phase2[1]);
    if (compress) printf(", \"root\": \"%s\", \"root_leaves\": %zu, \"compress_seconds\": %.4f", root_out.c_str(), root_leaves, compress_secs);
    printf("}\n");
    for (r0h_receipt* r : made) CHECK(r0h_receipt_free(r));
    for (Worker& w : workers) {
      CHECK(r0h_circuit_free(w.circ));
      if (w.image) { CHECK(r0h_ctx_set_image_circuit(w.ctx, nullptr)); CHECK(r0h_circuit_free(w.image)); }
      CHECK(r0h_ctx_destroy(w.ctx));
    }
    return 0;
  }
  if (contexts < 1 || contexts > 16) { fprintf(stderr, "r0h_prove: --contexts must be 1..16\n"); return 1; }
  if (receipts < 1 || (receipts > 1 && !receipt_out.empty())) { fprintf(stderr, "r0h_prove: --receipts R > 1 writes one file per receipt: use --receipt-dir\n"); return 1; }
  if (!receipt_out.empty() && !receipt_dir.empty()) { fprintf(stderr, "r0h_prove: --receipt-out and --receipt-dir exclude each other\n"); return 1; }
  const bool with_claims = !receipt_out.empty() || !receipt_dir.empty();
  // BASELINE.json configs[3]: a batch of independent receipts of `segments` segments each -- receipts x segments units on one
  // work queue, every lane takes the next unit when it is free
  const unsigned units = receipts * segments;

  // one context (+ circuit + resident witness) per in-flight lane, each driven by its own host thread: segments are
  // independent, so the lanes never talk to each other
  struct Lane {
    r0h_ctx* ctx = nullptr; r0h_circuit* circ = nullptr; r0h_buf* code = nullptr; r0h_buf* data = nullptr;
    std::vector<uint32_t> global, seal; size_t words = 0; unsigned proved = 0, loaded = 0;  // loaded: unit whose witness the buffers hold
    std::vector<std::pair<unsigned, std::vector<uint32_t>>> kept;  // (unit, seal) when receipts are to be written
  };
  std::vector<Lane> lanes(contexts);
  const size_t n = (size_t)1 << po2;
  for (unsigned k = 0; k < contexts; k++) {
    Lane& ln = lanes[k];
    CHECK(r0h_ctx_create((int)device, &ln.ctx));
    CHECK(r0h_ctx_set_hashfn(ln.ctx, hashfn.c_str()));
    CHECK(r0h_circuit_load(ln.ctx, blob.data(), blob.size(), co_path.empty() ? nullptr : co_path.c_str(), &ln.circ));
    arm_checker(ln.ctx, ln.circ);
    CHECK(r0h_buf_alloc(ln.ctx, (size_t)r0h_circuit_group_size(ln.circ, R0H_GROUP_CODE) * n * 4, &ln.code));
    CHECK(r0h_buf_alloc(ln.ctx, (size_t)r0h_circuit_group_size(ln.circ, R0H_GROUP_DATA) * n * 4, &ln.data));
    ln.global.resize(r0h_circuit_n_global(ln.circ) + 1);
    ln.seal.resize((size_t)1 << 20);
    CHECK(r0h_witgen(ln.ctx, ln.circ, po2, seed + k, ln.code, ln.data, ln.global.data()));
    ln.loaded = k;
  }
  // CODE is the same for every segment of this circuit and size: committed once, read by every lane's proofs
  r0h_code_commit* code_commit = nullptr;
  CHECK(r0h_code_commit_new(lanes[0].ctx, lanes[0].code, r0h_circuit_group_size(lanes[0].circ, R0H_GROUP_CODE), po2, &code_commit));
  // the claims of every unit (receipt r, segment s): unit = r * segments + s
  std::vector<uint8_t> journal(journal_text.size() + 8);
  size_t jn = 0;
  CHECK(r0h_serde_encode_str((const uint8_t*)journal_text.data(), journal_text.size(), journal.data(), journal.size(), &jn));
  journal.resize(jn);
  std::vector<r0h_receipt_claim> claims(units);
  std::vector<std::string> image_ids(receipts);
  if (with_claims) {
    if (r0h_circuit_n_global(lanes[0].circ) < 8) { fprintf(stderr, "r0h_prove: the circuit exposes fewer than 8 public inputs: a claim cannot be bound to its seals\n"); return 1; }
    for (unsigned r = 0; r < receipts; r++) {
      std::vector<r0h_system_state> st(segments + 1);
      for (unsigned k = 0; k <= segments; k++) {
        char name[96];
        int nn = snprintf(name, sizeof name, "r0hip synthetic session %llu/%u/%u", seed, r, k);
        st[k].pc = 0;
        CHECK(r0h_sha256((const uint8_t*)name, (size_t)nn, st[k].merkle_root));
      }
      for (unsigned k = 0; k < segments; k++) {
        r0h_receipt_claim& c = claims[r * segments + k];
        memset(&c, 0, sizeof c);
        c.pre = st[k];
        c.post = st[k + 1];
        const bool last = k + 1 == segments;
        c.exit_system = last ? 0 : 2;  // Halted(0) | SystemSplit
        if (last) CHECK(r0h_output_digest(journal.data(), journal.size(), nullptr, c.output_digest));
      }
      uint8_t id[32];
      CHECK(r0h_system_state_digest(&st[0], id));
      char hex[65];
      CHECK(r0h_image_id_to_hex(id, hex));  // the reference's IMAGE_ID.hex convention: eight {:08x} words
      image_ids[r] = hex;
    }
  }
  std::atomic<unsigned> next_unit{0};
  auto work = [&](unsigned k) {
    Lane& ln = lanes[k];
    for (unsigned u; (u = next_unit.fetch_add(1)) < units;) {
      const unsigned s = u % segments;  // segment index within its receipt
      if (with_claims) {  // the claim's naming words are the segment's public inputs
        uint8_t cd[32];
        CHECK(r0h_claim_digest(&claims[u], cd));
        std::fill(ln.global.begin(), ln.global.end(), 0u);
        CHECK(r0h_claim_globals(cd, ln.global.data()));
        CHECK(r0h_witgen_public(ln.ctx, ln.circ, po2, seed + u, ln.global.data(), ln.code, ln.data));
        ln.loaded = ~0u;
      } else if (u != ln.loaded) {
        CHECK(r0h_witgen(ln.ctx, ln.circ, po2, seed + u, ln.code, ln.data, ln.global.data()));
        ln.loaded = u;
      }
      CHECK(r0h_prove_segment_committed(ln.ctx, ln.circ, po2, code_commit, ln.data, ln.global.data(), ln.seal.data(), ln.seal.size(), &ln.words));
      ln.proved++;
      (void)s;
      if (with_claims) ln.kept.emplace_back(u, std::vector<uint32_t>(ln.seal.begin(), ln.seal.begin() + ln.words));
    }
  };
  auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> threads;
  for (unsigned k = 1; k < contexts; k++) threads.emplace_back(work, k);
  work(0);
  for (auto& t : threads) t.join();
  const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // report the seal lane 0 proved last (with one lane: the last unit; with several, whichever unit the queue handed it)
  const Lane& l0 = lanes[0];
  uint64_t h = 1469598103934665603ull;  // FNV-1a, to compare runs
  for (size_t i = 0; i < l0.words; i++) { h ^= l0.seal[i]; h *= 1099511628211ull; }
  printf("{\"segments\": %u, \"receipts\": %u, \"contexts\": %u, \"po2\": %u, \"seal_words\": %zu, \"seal_fnv1a\": \"%016llx\", \"seconds\": %.6f, "
         "\"segments_per_s\": %.4f, \"receipts_per_s\": %.4f}\n",
         segments, receipts, contexts, po2, l0.words, (unsigned long long)h, total, units / total, receipts / total);
  if (verify) {  // outside the timed region: the host-side verifier on every lane's last seal
    for (const Lane& ln : lanes) {
      if (!ln.proved) continue;
      int verdict = -1;
      if (verify_device) CHECK(r0h_verify_seals_on(ln.ctx, blob.data(), blob.size(), ln.seal.data(), &ln.words, 1, nullptr, &verdict, nullptr, nullptr));
      else CHECK(r0h_verify_seal_hashfn(blob.data(), blob.size(), hashfn.c_str(), ln.seal.data(), ln.words, nullptr, &verdict, nullptr, nullptr));
      if (verdict != R0H_VERIFY_OK) { fprintf(stderr, "r0h_prove: the verifier rejects the seal: %s\n", r0h_verify_reason(verdict)); return 3; }
    }
    fprintf(stderr, "r0h_prove: seals verified\n");
  }
  if (with_claims) {
    // the Receipt JSON `host` writes (host/src/main.rs:251-252, 299-316): all segment seals in order + the journal, which for the
    // hyperfridge guest is the serde word stream of the committed JSON string (host/src/main.rs:258-267)
    uint32_t root[8];
    CHECK(r0h_code_commit_root(code_commit, root));
    printf("{\"control_root\": {\"po2\": %u, \"root\": [%u, %u, %u, %u, %u, %u, %u, %u]}, \"image_ids\": [", po2, root[0], root[1], root[2], root[3], root[4], root[5], root[6], root[7]);
    for (unsigned r = 0; r < receipts; r++) printf("%s\"%s\"", r ? ", " : "", image_ids[r].c_str());
    printf("]}\n");
    for (unsigned r = 0; r < receipts; r++) {
      r0h_receipt* rc = nullptr;
      CHECK(r0h_receipt_new(R0H_RECEIPT_COMPOSITE, journal.data(), journal.size(), &rc));
      for (unsigned k = 0; k < segments; k++)
        for (const Lane& ln : lanes)
          for (const auto& kv : ln.kept)
            if (kv.first == r * segments + k) CHECK(r0h_receipt_add_segment_claim(rc, kv.second.data(), kv.second.size(), k, &claims[kv.first], nullptr));
      if (r0h_receipt_n_segments(rc) != segments) { fprintf(stderr, "r0h_prove: receipt %u is missing segments\n", r); return 3; }
      char* text = nullptr;
      CHECK(r0h_receipt_to_json(rc, &text));
      char name[64];
      snprintf(name, sizeof name, "/receipt_%04u.json", r);
      const std::string path = receipt_out.empty() ? receipt_dir + name : receipt_out;
      FILE* o = fopen(path.c_str(), "wb");
      if (!o || fwrite(text, 1, strlen(text), o) != strlen(text)) { fprintf(stderr, "r0h_prove: cannot write %s\n", path.c_str()); return 1; }
      fclose(o);
      r0h_free_error(text);
      CHECK(r0h_receipt_free(rc));
    }
  }
  if (!seal_out.empty()) {
    FILE* o = fopen(seal_out.c_str(), "wb");
    if (!o || fwrite(l0.seal.data(), 4, l0.words, o) != l0.words) { fprintf(stderr, "r0h_prove: cannot write %s\n", seal_out.c_str()); return 1; }
    fclose(o);
  }
  CHECK(r0h_code_commit_free(code_commit));
  for (Lane& ln : lanes) {
    CHECK(r0h_buf_free(ln.code));
    CHECK(r0h_buf_free(ln.data));
    CHECK(r0h_circuit_free(ln.circ));
    CHECK(r0h_ctx_destroy(ln.ctx));
  }
  return 0;
}
