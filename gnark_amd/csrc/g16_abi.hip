// The Groth16 entry points of the C ABI (include/gnark_amd.h), under abi.hip's rule: an entry point checks the pointers and ranges it
// can judge without the key, and makes ONE call of its driver (g16.hip.h), which lives beside the code it drives -- proofs in
// groth16.hip, keys and the builder in g16_key.hip.h, key files and proof bytes in g16_io.hip.h.  No lock, no device call and no
// curve dispatch is here; a refusal, here or in a driver, names the entry point that was called (current_entry).
#include "g16.hip.h"

using namespace ga;

static Ctx* as_ctx(ga_ctx* h) { return reinterpret_cast<Ctx*>(h); }
static G16Pk* as_pk(ga_g16_pk* p) { return reinterpret_cast<G16Pk*>(p); }
static G16Pk** as_pk_out(ga_g16_pk** out) { return reinterpret_cast<G16Pk**>(out); }
static G16Stage* as_stage(ga_g16_builder* b) { return reinterpret_cast<G16Stage*>(b); }
static bool abi_null_builder(const ga_g16_builder* b) { return abi_bad_argument(!b, "null builder"); }

extern "C" {

// ---- proving keys and the staged builder (g16_key.hip.h) -------------------------------------------------------------------------
int ga_g16_pk_create(ga_ctx* h, const ga_g16_key* key, ga_g16_pk** out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!h || !key || !out)) return GA_ERR_INVALID;
    return pk_create_run(as_ctx(h), key, as_pk_out(out));
} GA_ABI_CATCH

void ga_g16_pk_destroy(ga_g16_pk* p) try {
    GA_ABI_ENTRY();
    pk_destroy(as_pk(p));
} GA_ABI_CATCH_VOID

int ga_g16_builder_create(ga_ctx* h, int curve, uint64_t domain_cardinality, uint64_t nb_wires, uint32_t shard_index, uint32_t shard_count, ga_g16_builder** out) try {
    GA_ABI_ENTRY();
    GA_CHECK(dispatch_check(Scope::FULL, curve, GA_NO_GROUP));   // no Groth16 key on a G1 / Fr curve
    if (abi_bad_argument(!h || !out || domain_cardinality == 0, "bad argument")) return GA_ERR_INVALID;
    return stage_create(as_ctx(h), curve, domain_cardinality, nb_wires, shard_index, shard_count, reinterpret_cast<G16Stage**>(out));
} GA_ABI_CATCH

int ga_g16_builder_reserve(ga_g16_builder* b, int which, uint64_t total_len) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b)) return GA_ERR_INVALID;
    return stage_reserve_run(as_stage(b), which, total_len);
} GA_ABI_CATCH

// (points = null skips `count` points that are none of this shard's business)
int ga_g16_builder_append(ga_g16_builder* b, int which, const void* points, uint64_t count) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b)) return GA_ERR_INVALID;
    return stage_append_run(as_stage(b), which, points, count);
} GA_ABI_CATCH

int ga_g16_builder_set_point(ga_g16_builder* b, int which, const void* affine) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b)) return GA_ERR_INVALID;
    return stage_set_point_run(as_stage(b), which, affine);
} GA_ABI_CATCH

int ga_g16_builder_set_infinity(ga_g16_builder* b, int which, const uint8_t* mask, uint64_t nb_wires) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b)) return GA_ERR_INVALID;
    return stage_set_infinity(as_stage(b), which, mask, nb_wires);
} GA_ABI_CATCH

int ga_g16_builder_add_commitment_key(ga_g16_builder* b, const void* basis, const void* sigma, uint64_t len) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b)) return GA_ERR_INVALID;
    return stage_add_commitment_key_run(as_stage(b), basis, sigma, len);
} GA_ABI_CATCH

int ga_g16_builder_set_k_remove(ga_g16_builder* b, const uint64_t* ids, uint64_t len) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b) || abi_bad_argument(len && !ids, "null pointer")) return GA_ERR_INVALID;
    return stage_set_k_remove(as_stage(b), ids, len);
} GA_ABI_CATCH

int ga_g16_builder_set_window_shard(ga_g16_builder* b, uint32_t index, uint32_t count) try {
    GA_ABI_ENTRY();
    if (abi_null_builder(b)) return GA_ERR_INVALID;
    return stage_set_window_shard(as_stage(b), index, count);
} GA_ABI_CATCH

int ga_g16_builder_finish(ga_g16_builder* b, int32_t precompute, ga_g16_pk** out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!b || !out)) return GA_ERR_INVALID;
    return stage_finish_consume(as_stage(b), precompute, as_pk_out(out));
} GA_ABI_CATCH

void ga_g16_builder_destroy(ga_g16_builder* b) try {
    GA_ABI_ENTRY();
    stage_destroy(as_stage(b));
} GA_ABI_CATCH_VOID

int ga_g16_shard_layout(ga_g16_pk* p, uint64_t* out8) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !out8)) return GA_ERR_INVALID;
    return pk_shard_layout(as_pk(p), out8);
} GA_ABI_CATCH

int ga_g16_table_layout(ga_g16_pk* p, uint64_t* out2) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !out2)) return GA_ERR_INVALID;
    return pk_table_layout(as_pk(p), out2);
} GA_ABI_CATCH

// ---- key files and proof bytes (g16_io.hip.h) ------------------------------------------------------------------------------------
// the _checked forms: ProvingKey.ReadFrom semantics, every point kept is tested for curve and subgroup membership
int ga_g16_pk_read_mem(ga_ctx* h, int curve, const uint8_t* data, size_t len, int32_t precompute, uint32_t shard_index, uint32_t shard_count,
                       const uint64_t* k_remove, uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(!data, "null data") || abi_null_argument(!h || !out || (len_k_remove && !k_remove))) return GA_ERR_INVALID;
    return g16_pk_read_run(as_ctx(h), curve, data, len, -1, precompute, shard_index, shard_count, k_remove, len_k_remove, as_pk_out(out), bytes_read, false, env_u64("GA_KEY_CHUNK", 0));
} GA_ABI_CATCH

int ga_g16_pk_read_fd(ga_ctx* h, int curve, int fd, int32_t precompute, uint32_t shard_index, uint32_t shard_count, const uint64_t* k_remove,
                      uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(fd < 0, "bad file descriptor") || abi_null_argument(!h || !out || (len_k_remove && !k_remove))) return GA_ERR_INVALID;
    return g16_pk_read_run(as_ctx(h), curve, nullptr, 0, fd, precompute, shard_index, shard_count, k_remove, len_k_remove, as_pk_out(out), bytes_read, false, env_u64("GA_KEY_CHUNK", 0));
} GA_ABI_CATCH

int ga_g16_pk_read_mem_checked(ga_ctx* h, int curve, const uint8_t* data, size_t len, int32_t precompute, uint32_t shard_index, uint32_t shard_count,
                               const uint64_t* k_remove, uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(!data, "null data") || abi_null_argument(!h || !out || (len_k_remove && !k_remove))) return GA_ERR_INVALID;
    return g16_pk_read_run(as_ctx(h), curve, data, len, -1, precompute, shard_index, shard_count, k_remove, len_k_remove, as_pk_out(out), bytes_read, true, env_u64("GA_KEY_CHUNK", 0));
} GA_ABI_CATCH

int ga_g16_pk_read_fd_checked(ga_ctx* h, int curve, int fd, int32_t precompute, uint32_t shard_index, uint32_t shard_count, const uint64_t* k_remove,
                              uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(fd < 0, "bad file descriptor") || abi_null_argument(!h || !out || (len_k_remove && !k_remove))) return GA_ERR_INVALID;
    return g16_pk_read_run(as_ctx(h), curve, nullptr, 0, fd, precompute, shard_index, shard_count, k_remove, len_k_remove, as_pk_out(out), bytes_read, true, env_u64("GA_KEY_CHUNK", 0));
} GA_ABI_CATCH

int ga_g16_key_write_fd(ga_ctx* h, const ga_g16_key* key, int format, int fd, uint64_t* bytes_written) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(!h || !key || fd < 0 || format < GA_KEY_FORMAT_COMPRESSED || format > GA_KEY_FORMAT_DUMP, "bad argument")) return GA_ERR_INVALID;
    return g16_key_write_run(as_ctx(h), key, format, fd, bytes_written, env_u64("GA_KEY_CHUNK", 0));
} GA_ABI_CATCH

int ga_g16_proof_unmarshal(int curve, const uint8_t* data, size_t len, void* proof_out, void* commitments_out, uint32_t max_commitments,
                           uint32_t* n_commitments, void* pok_out, size_t* consumed) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!data || !proof_out)) return GA_ERR_INVALID;
    return g16_proof_unmarshal_run(curve, data, len, proof_out, commitments_out, max_commitments, n_commitments, pok_out, consumed);
} GA_ABI_CATCH

int ga_point_unmarshal(int curve, int group, const uint8_t* data, size_t len, void* affine_out, size_t* consumed) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!data || !affine_out)) return GA_ERR_INVALID;
    return g16_point_unmarshal_run(curve, group, data, len, affine_out, consumed);
} GA_ABI_CATCH

int ga_g16_proof_marshal(int curve, const void* proof, uint8_t* out, size_t cap, size_t* len) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!proof || !out || !len)) return GA_ERR_INVALID;
    return g16_marshal_run(curve, proof, nullptr, 0, nullptr, out, cap, len, false);
} GA_ABI_CATCH

int ga_g16_proof_marshal_bsb22(int curve, const void* proof, const void* commitments, uint32_t n, const void* pok, uint8_t* out, size_t cap, size_t* len) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!proof || !out || !len || (n && !commitments))) return GA_ERR_INVALID;
    return g16_marshal_run(curve, proof, commitments, n, pok, out, cap, len, false);
} GA_ABI_CATCH

int ga_g16_proof_marshal_raw(int curve, const void* proof, const void* commitments, uint32_t n, const void* pok, uint8_t* out, size_t cap, size_t* len) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!proof || !out || !len || (n && !commitments))) return GA_ERR_INVALID;
    return g16_marshal_run(curve, proof, commitments, n, pok, out, cap, len, true);
} GA_ABI_CATCH

int ga_g1_marshal_uncompressed(int curve, const void* affine, uint8_t* out, size_t cap, size_t* len) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!affine || !out || !len)) return GA_ERR_INVALID;
    return g16_g1_marshal_uncompressed_run(curve, affine, out, cap, len);
} GA_ABI_CATCH

// ---- proofs (groth16.hip) ---------------------------------------------------------------------------------------------------------
int ga_g16_prove(ga_g16_pk* p, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                 uint64_t nb_public, const void* r, const void* s, void* proof_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !w || !a || !b || !c || !r || !s || !proof_out)) return GA_ERR_INVALID;
    return g16_prove_run(as_pk(p), w, a, b, c, n_constraints, nb_public, r, s, proof_out);
} GA_ABI_CATCH

int ga_g16_prove_batch(ga_g16_pk* p, uint32_t count, const void* const* w, const void* const* a, const void* const* b, const void* const* c,
                       uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proofs_out) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    if (abi_null_argument(!p || !w || !a || !b || !c || !r || !s || !proofs_out)) return GA_ERR_INVALID;
    return g16_prove_batch_run(as_pk(p), count, w, a, b, c, n_constraints, nb_public, r, s, proofs_out);
} GA_ABI_CATCH

int ga_g16_prove_oneshot(ga_ctx* h, const ga_g16_key* key, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                         uint64_t nb_public, const void* r, const void* s, void* proof_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!h || !key || !w || !a || !b || !c || !r || !s || !proof_out)) return GA_ERR_INVALID;
    return g16_prove_oneshot_run(as_ctx(h), key, w, a, b, c, n_constraints, nb_public, r, s, proof_out);
} GA_ABI_CATCH

int ga_g16_prove_partial(ga_g16_pk* p, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints, uint64_t nb_public, void* partials_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !w || !a || !b || !c || !partials_out)) return GA_ERR_INVALID;
    return g16_prove_partial_run(as_pk(p), w, a, b, c, n_constraints, nb_public, partials_out);
} GA_ABI_CATCH

int ga_g16_finish(ga_g16_pk* p, const void* partials_sum, const void* r, const void* s, void* proof_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !partials_sum || !r || !s || !proof_out)) return GA_ERR_INVALID;
    return g16_finish_run(as_pk(p), partials_sum, r, s, proof_out);
} GA_ABI_CATCH

// ---- pieces of a sharded proof (multi-GPU orchestration by the caller: gnark_amd/multigpu.py over RCCL, or ga_g16_prove_multi) ----
int ga_g16_witness_partial(ga_g16_pk* p, const void* w, uint64_t nb_public, void* partials_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !w || !partials_out)) return GA_ERR_INVALID;
    return g16_witness_partial_run(as_pk(p), w, nb_public, partials_out);
} GA_ABI_CATCH

int ga_g16_h_chain(ga_g16_pk* p, const void* v, uint64_t n_constraints, void* out_dev) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !v || !out_dev)) return GA_ERR_INVALID;
    return g16_h_chain_run(as_pk(p), v, out_dev, n_constraints);
} GA_ABI_CATCH

int ga_g16_h_chain_dev(ga_g16_pk* p, void* buf_dev, uint64_t n_constraints) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !buf_dev)) return GA_ERR_INVALID;
    return g16_h_chain_run(as_pk(p), nullptr, buf_dev, n_constraints);
} GA_ABI_CATCH

int ga_g16_h_combine(ga_g16_pk* p, void* a_dev, const void* b_dev, const void* c_dev) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !a_dev || !b_dev || !c_dev)) return GA_ERR_INVALID;
    return g16_h_combine_run(as_pk(p), a_dev, b_dev, c_dev);
} GA_ABI_CATCH

// (h_slice_dev may be null for a shard without a slice of Z: the driver's check)
int ga_g16_z_partial(ga_g16_pk* p, const void* h_slice_dev, void* partial_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || !partial_out)) return GA_ERR_INVALID;
    return g16_z_partial_run(as_pk(p), h_slice_dev, partial_out);
} GA_ABI_CATCH

int ga_g16_prove_multi(ga_g16_pk* const* keys, uint32_t n, const void* w, const void* a, const void* b, const void* c,
                       uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proof_out) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(!keys || n == 0 || n > 64 || !w || !a || !b || !c || !r || !s || !proof_out, "null argument or unsupported device count")) return GA_ERR_INVALID;
    return g16_prove_multi_run(reinterpret_cast<G16Pk* const*>(keys), n, w, a, b, c, n_constraints, nb_public, r, s, proof_out);
} GA_ABI_CATCH

int ga_g16_commit(ga_g16_pk* p, uint32_t index, const void* values, uint64_t n_values, void* commitment_out, void* pok_out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!p || (!values && n_values) || !commitment_out || !pok_out)) return GA_ERR_INVALID;
    return g16_commit_run(as_pk(p), index, values, n_values, commitment_out, pok_out);
} GA_ABI_CATCH

int ga_g16_fold_pok(int curve, const void* poks, uint64_t n, const void* challenge, void* out) try {
    GA_ABI_ENTRY();
    if (abi_null_argument((!poks && n) || !challenge || !out)) return GA_ERR_INVALID;
    return g16_fold_pok_run(curve, poks, n, challenge, out);
} GA_ABI_CATCH

int ga_g16_lane_stats(ga_ctx* h, uint64_t* out6) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!h || !out6)) return GA_ERR_INVALID;
    return g16_lane_stats(as_ctx(h), out6);
} GA_ABI_CATCH

}  // extern "C"
