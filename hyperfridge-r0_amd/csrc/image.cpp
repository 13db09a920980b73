// The image proof: what lets `receipt.verify(image_id)` (verifier/src/main.rs:124-126; risc0-zkvm 3.0.5 `Receipt::verify`) check a
// trace-circuit session WITHOUT the program image in hand.  r0h_receipt_verify_elf completes the session's memory argument by adding
// 1 / fingerprint(address, word) over the ELF's own words; a verifier with the 32 bytes of the image id cannot.  The image circuit
// (tools/image_circuit.py, circuits/image.r0c) proves that sum for it: a Poseidon2 sponge over the image's word list, computed inside
// the proof, gives the digest the image id names as the root of the initial memory state (csrc/rv32im.cpp initial_root), and the same
// rows add every word's fraction under the session's challenge to a running sum whose total is a public input.  The verifier checks
// the seal, takes the digest from the first claim's pre-state (which it holds against the image id) and the total for its balance.
//
// Host: r0h_image_witness (the circuit's DATA group for an ELF: sponge rows + the four validity flags), r0h_image_po2.  Device:
// r0h_prove_image (witness uploaded, total accumulated, proved like any segment; a few milliseconds for a 13 KiB image).
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/r0hip_circuit.h"
#include "circuit.hpp"
#include "receipt_types.hpp"

using namespace r0h;

namespace r0h {
bool is_image_circuit(const r0h_circuit& c) {
  return !memcmp(c.info, "R0HIP_IMAGE:v1__", 16) && c.n_global == R0H_IMAGE_GLOBALS && c.n_late == R0H_IMAGE_LATE_GLOBALS && c.has_sponge &&
         c.group_size[R0H_GROUP_DATA] == R0H_IMAGE_COLUMNS && c.sponge_data == 0 && c.sponge_global == 0;
}
// the DATA group for an image: [R0H_IMAGE_COLUMNS][2^po2] Montgomery words, column-major
const char* image_witness(const std::vector<std::pair<uint32_t, uint32_t>>& image, uint32_t po2, uint32_t* data, uint32_t digest[8]) {
  std::vector<uint32_t> stream;
  image_stream(image, stream);
  const size_t n = (size_t)1 << po2, n_blocks = stream.size() / 16;
  R0H_REQUIRE(n_blocks * R0H_SPONGE_PERIOD < n, "the image's %zu words take %zu rows: the image trace has 2^%u", image.size(), n_blocks * R0H_SPONGE_PERIOD, po2);
  memset(data, 0, (size_t)R0H_IMAGE_COLUMNS * n * 4);
  size_t used = 0;
  p2_sponge_rows_host(p2_default(), stream.data(), stream.size(), data, n, &used);
  for (size_t q = 0; q < n_blocks; q++) {  // the flags: the mask's bits, on the row that absorbs the block
    const size_t there = std::min<size_t>(4, image.size() - std::min<size_t>(image.size(), 4 * q));
    for (size_t j = 0; j < there; j++) data[(R0H_SPONGE_DATA_COLUMNS + j) * n + q * R0H_SPONGE_PERIOD] = ONE;
  }
  if (digest) p2_hash_elems_host(p2_default(), stream.data(), stream.size(), digest);
  return nullptr;
}
}  // namespace r0h

extern "C" {

const char* r0h_image_po2(const uint8_t* elf, size_t elf_len, uint32_t* po2_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(elf && po2_out, "r0h_image_po2: NULL argument");
  std::vector<std::pair<uint32_t, uint32_t>> image;
  uint32_t entry;
  uint8_t id[32];
  R0H_TRY(elf_image(elf, elf_len, image, &entry, id));
  const size_t rows = (image.empty() ? 1 : (image.size() + 3) / 4) * R0H_SPONGE_PERIOD;
  uint32_t po2 = 9;  // the prover's smallest trace
  while (((size_t)1 << po2) <= rows) po2++;
  R0H_REQUIRE(po2 <= R0H_MAX_PO2, "r0h_image_po2: an image of %zu words does not fit a trace", image.size());
  *po2_out = po2;
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_image_witness(const uint8_t* elf, size_t elf_len, uint32_t po2, uint32_t* data_out, uint32_t globals_out[R0H_IMAGE_GLOBALS]) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(elf && data_out && globals_out, "r0h_image_witness: NULL argument");
  R0H_REQUIRE(po2 >= 6 && po2 <= R0H_MAX_PO2, "r0h_image_witness: po2 %u outside [6, %u]", po2, R0H_MAX_PO2);
  std::vector<std::pair<uint32_t, uint32_t>> image;
  uint32_t entry;
  uint8_t id[32];
  R0H_TRY(elf_image(elf, elf_len, image, &entry, id));
  memset(globals_out, 0, R0H_IMAGE_GLOBALS * 4);
  return image_witness(image, po2, data_out, globals_out);
  R0H_GUARD_END
}

// Sessions begun on `ctx` afterwards attach an image proof to their receipts (NULL: stop).  The circuit must be loaded on this context.
const char* r0h_ctx_set_image_circuit(r0h_ctx* ctx, const r0h_circuit* image_circuit) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx, "r0h_ctx_set_image_circuit: ctx is NULL");
  if (image_circuit) {
    R0H_REQUIRE(is_image_circuit(*image_circuit), "r0h_ctx_set_image_circuit: the circuit is not the image circuit (circuits/image.r0c) this library was built for");
    R0H_REQUIRE(image_circuit->ctx == ctx, "r0h_ctx_set_image_circuit: the circuit was loaded on another context");
  }
  ctx->image_circuit = image_circuit;
  return nullptr;
  R0H_GUARD_END
}

// What both forms of the image proof start from: the ELF's image as the circuit's DATA group on the device (the sponge's rows over the
// blocks -- only the rows in use travel --, the flags on the rows that absorb a block) and the public inputs with digest and challenge
// filled in.  `flags` is read by copies on the stream: it lives as long as they may run.  `code` (the blocking form's; nullptr where
// CODE comes from a kept commitment): the CODE columns, allocated and generated in the places r0h_prove_image has always had them.
static const char* image_plant(const char* caller, r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t challenge[16], uint32_t* po2_out,
                               std::vector<uint32_t>& global, DevBuf* code, DevBuf& data, std::vector<uint32_t>& flags) {
  R0H_TRY(require_poseidon2(ctx, caller));
  R0H_REQUIRE(is_image_circuit(*c), "%s: the circuit is not the image circuit (circuits/image.r0c) this library was built for", caller);
  for (int i = 0; i < 16; i++) R0H_REQUIRE(challenge[i] < P, "%s: challenge word %d is not a canonical field word", caller, i);
  R0H_TRY_HIP(hipSetDevice(ctx->device));
  std::vector<std::pair<uint32_t, uint32_t>> image;
  uint32_t entry, po2 = 9;
  uint8_t id[32];
  R0H_TRY(elf_image(elf, elf_len, image, &entry, id));
  std::vector<uint32_t> stream;
  global.assign(R0H_IMAGE_GLOBALS, 0);
  image_stream(image, stream);
  const size_t n_blocks = stream.size() / 16, rows = n_blocks * R0H_SPONGE_PERIOD;
  while (((size_t)1 << po2) <= rows) po2++;
  R0H_REQUIRE(po2 <= R0H_MAX_PO2, "%s: an image of %zu words does not fit a trace", caller, image.size());
  const size_t n = (size_t)1 << po2;
  p2_hash_elems_host(p2_default(), stream.data(), stream.size(), global.data());
  memcpy(&global[R0H_IMAGE_GAMMA], challenge, 64);
  if (code) R0H_TRY(code->alloc(ctx, (size_t)c->group_size[R0H_GROUP_CODE] * n * 4));
  R0H_TRY(data.alloc(ctx, (size_t)R0H_IMAGE_COLUMNS * n * 4));
  if (code) R0H_TRY(witgen_code(ctx, c, po2, code->get()));
  R0H_TRY(sponge_plant(ctx, c, po2, stream.data(), stream.size(), data.get()));
  flags.assign(4 * n_blocks, 0u);  // [flag][block]
  for (size_t k = 0; k < image.size(); k++) flags[(k % 4) * n_blocks + k / 4] = ONE;
  uint32_t* first_flag = (uint32_t*)data->ptr + (size_t)R0H_SPONGE_DATA_COLUMNS * n;
  R0H_TRY_HIP(hipMemsetAsync(first_flag, 0, 4 * n * 4, ctx->stream));
  for (size_t j = 0; j < 4; j++)  // one word every thirty rows
    R0H_TRY_HIP(hipMemcpy2DAsync(first_flag + j * n, (size_t)R0H_SPONGE_PERIOD * 4, flags.data() + j * n_blocks, 4, 4, n_blocks, hipMemcpyHostToDevice, ctx->stream));
  *po2_out = po2;
  return nullptr;
}

// One image proof on `ctx`: the seal's public inputs are the image's digest (8), the challenge given (16), the total (4).
const char* r0h_prove_image(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t challenge[16], uint32_t* seal_out,
                            size_t seal_capacity_words, size_t* seal_words_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && elf && challenge && seal_words_out, "r0h_prove_image: NULL argument");
  uint32_t po2 = 0;
  std::vector<uint32_t> global, flags;
  DevBuf code, data;
  R0H_TRY(image_plant("r0h_prove_image", ctx, c, elf, elf_len, challenge, &po2, global, &code, data, flags));
  R0H_TRY(r0h_logup_totals(ctx, c, po2, code.get(), data.get(), global.data()));
  return r0h_prove_segment(ctx, c, po2, code.get(), data.get(), global.data(), seal_out, seal_capacity_words, seal_words_out);
  R0H_GUARD_END
}

}  // extern "C"

// An image proof between its enqueue and its collect: the proof in flight and what its steps read on the stream until then
struct r0h_image_proof {
  std::shared_ptr<r0h_code_commit> code;  // the circuit's CODE group at this trace size, shared with the context's cache
  DevBuf data, globals, mix, accum;
  std::vector<uint32_t> flags;
  r0h_proof* proof = nullptr;
  ~r0h_image_proof() { r0h_proof_abort(proof); }  // (waits for the stream if the proof is still in flight)
};

extern "C" {

const char* r0h_prove_image_enqueue(r0h_ctx* ctx, const r0h_circuit* c, const uint8_t* elf, size_t elf_len, const uint32_t challenge[16], r0h_image_proof** out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(ctx && c && elf && challenge && out, "r0h_prove_image_enqueue: NULL argument");
  R0H_REQUIRE(ctx->device_finish, "r0h_prove_image_enqueue: the context has r0h_ctx_set_device_finish off: only r0h_prove_image makes this proof");
  std::unique_ptr<r0h_image_proof> h(new r0h_image_proof);
  uint32_t po2 = 0;
  std::vector<uint32_t> global;
  // an error behind the first launch: what was launched runs out before the handle goes (it reads the handle's buffers and `flags`)
  const char* err = [&]() -> const char* {
  R0H_TRY(image_plant("r0h_prove_image_enqueue", ctx, c, elf, elf_len, challenge, &po2, global, nullptr, h->data, h->flags));
  R0H_TRY(ctx_code_commit(ctx, c, po2, &h->code));  // (committed on the first call for this trace size: that one waits)
  const r0h_buf* code = nullptr;
  R0H_TRY(r0h_code_commit_columns(h->code.get(), &code));
  R0H_TRY(h->globals.alloc(ctx, (size_t)R0H_IMAGE_GLOBALS * 4));
  R0H_TRY(stage_h2d(ctx, h->globals->ptr, global.data(), (size_t)R0H_IMAGE_GLOBALS * 4));
  R0H_TRY(r0h_proof_begin_committed_enqueue(ctx, c, po2, h->code.get(), h->data.get(), global.data(), nullptr, &h->proof));
  R0H_TRY(r0h_logup_totals_device(ctx, c, po2, code, h->data.get(), h->globals.get()));
  const r0h_buf late = buf_view(h->globals.get(), (size_t)(R0H_IMAGE_GLOBALS - R0H_IMAGE_LATE_GLOBALS) * 4, (size_t)R0H_IMAGE_LATE_GLOBALS * 4);
  R0H_TRY(h->mix.alloc(ctx, (size_t)(c->n_mix ? c->n_mix : 1) * 4));
  R0H_TRY(r0h_proof_late_device(h->proof, &late, h->mix.get()));
  R0H_TRY(h->accum.alloc(ctx, ((size_t)c->group_size[R0H_GROUP_ACCUM] << po2) * 4));
  R0H_TRY(r0h_accum_public_device(ctx, c, po2, code, h->data.get(), h->globals.get(), h->mix.get(), h->accum.get()));
  r0h_proof* proof = h->proof;
  h->proof = nullptr;  // r0h_proof_finish_enqueue consumes it on an error
  R0H_TRY(r0h_proof_finish_enqueue(proof, h->accum.get()));
  h->proof = proof;
  return nullptr;
  }();
  if (err) {
    if (h->data) (void)ctx_wait(ctx);
    return err;
  }
  *out = h.release();
  return nullptr;
  R0H_GUARD_END
}

const char* r0h_prove_image_collect(r0h_image_proof* handle, uint32_t* seal_out, size_t seal_capacity_words, size_t* seal_words_out) {
  R0H_GUARD_BEGIN
  R0H_REQUIRE(handle && seal_words_out, "r0h_prove_image_collect: NULL argument");
  std::unique_ptr<r0h_image_proof> h(handle);
  r0h_proof* proof = h->proof;
  h->proof = nullptr;  // consumed by the collect either way
  return r0h_proof_finish_collect(proof, seal_out, seal_capacity_words, seal_words_out);
  R0H_GUARD_END
}

const char* r0h_prove_image_abort(r0h_image_proof* handle) {
  delete handle;
  return nullptr;
}

}  // extern "C"
