// What g16_abi.hip sees of Groth16: the key and its builder as opaque types, and the driver of every entry point.  A driver is an
// ordinary function beside the code it drives; it takes its own PkUse, SlotLease and lock, reads the knobs and dispatches on the curve.
// The entry point has checked the pointers it names; a check that needs the key or the builder is the driver's.
#pragma once
#include "common.hip.h"

namespace ga {
struct G16Pk;
struct G16Stage;   // (both: g16_key.hip.h)

// ---- groth16.hip: proofs and their pieces ------------------------------------------------------------------------------------------
int g16_prove_run(G16Pk* pk, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints, uint64_t nb_public, const void* r,
                  const void* s, void* proof_out);
int g16_prove_batch_run(G16Pk* pk, uint32_t count, const void* const* w, const void* const* a, const void* const* b, const void* const* c,
                        uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proofs_out);
int g16_prove_oneshot_run(Ctx* ctx, const ga_g16_key* key, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                          uint64_t nb_public, const void* r, const void* s, void* proof_out);
int g16_prove_multi_run(G16Pk* const* pks, uint32_t n, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                        uint64_t nb_public, const void* r, const void* s, void* proof_out);
int g16_prove_partial_run(G16Pk* pk, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints, uint64_t nb_public, void* partials_out);
int g16_finish_run(G16Pk* pk, const void* partials_sum, const void* r, const void* s, void* proof_out);
int g16_witness_partial_run(G16Pk* pk, const void* w, uint64_t nb_public, void* partials_out);
// host_v: n_constraints elements uploaded into dev_buf first (ga_g16_h_chain); null: they are there already (ga_g16_h_chain_dev)
int g16_h_chain_run(G16Pk* pk, const void* host_v, void* dev_buf, uint64_t n_constraints);
int g16_h_combine_run(G16Pk* pk, void* a_dev, const void* b_dev, const void* c_dev);
int g16_z_partial_run(G16Pk* pk, const void* h_slice_dev, void* partial_out);
int g16_commit_run(G16Pk* pk, uint32_t index, const void* values, uint64_t n_values, void* commitment_out, void* pok_out);
int g16_fold_pok_run(int curve, const void* poks, uint64_t n, const void* challenge, void* out);
int g16_lane_stats(Ctx* ctx, uint64_t* out6);

// ---- g16_key.hip.h: keys and the staged builder (stage_append_run with points = null skips; stage_finish_consume deletes st) ------
int pk_create_run(Ctx* ctx, const ga_g16_key* key, G16Pk** out, bool defer_uploads = false);   // (true: g16_prove_oneshot_run's key)
void pk_destroy(G16Pk* pk);
int pk_shard_layout(const G16Pk* pk, uint64_t* out8);
int pk_table_layout(const G16Pk* pk, uint64_t* out2);
int stage_create(Ctx* ctx, int curve, uint64_t domain_cardinality, uint64_t nb_wires, uint32_t shard_index, uint32_t shard_count, G16Stage** out);
int stage_reserve_run(G16Stage* st, int which, uint64_t total_len);
int stage_append_run(G16Stage* st, int which, const void* points, uint64_t count);
int stage_set_point_run(G16Stage* st, int which, const void* affine);
int stage_set_infinity(G16Stage* st, int which, const uint8_t* mask, uint64_t nb_wires);
int stage_add_commitment_key_run(G16Stage* st, const void* basis, const void* sigma, uint64_t len);
int stage_set_k_remove(G16Stage* st, const uint64_t* ids, uint64_t len);
int stage_set_window_shard(G16Stage* st, uint32_t index, uint32_t count);
int stage_finish_consume(G16Stage* st, int32_t precompute, G16Pk** out);
void stage_destroy(G16Stage* st);

// ---- g16_io.hip.h: key files and proof bytes ---------------------------------------------------------------------------------------
// a key file from memory (data != null) or from fd; checked: ProvingKey.ReadFrom semantics, every kept point tested
// key_chunk: GA_KEY_CHUNK as the entry point read it, the points per staging pass of the reader and the writer (abi.hip has the table)
int g16_pk_read_run(Ctx* ctx, int curve, const uint8_t* data, size_t len, int fd, int32_t precompute, uint32_t shard_index, uint32_t shard_count,
                    const uint64_t* k_remove, uint64_t len_k_remove, G16Pk** out, uint64_t* bytes_read, bool checked, uint64_t key_chunk);
int g16_key_write_run(Ctx* ctx, const ga_g16_key* key, int format, int fd, uint64_t* bytes_written, uint64_t key_chunk);
int g16_proof_unmarshal_run(int curve, const uint8_t* data, size_t len, void* proof_out, void* commitments_out, uint32_t max_commitments,
                            uint32_t* n_commitments, void* pok_out, size_t* consumed);
int g16_point_unmarshal_run(int curve, int group, const uint8_t* data, size_t len, void* affine_out, size_t* consumed);
// Proof.WriteTo (raw: WriteRawTo); without commitments: commitments = pok = null, n = 0
int g16_marshal_run(int curve, const void* proof, const void* commitments, uint32_t n, const void* pok, uint8_t* out, size_t cap, size_t* len, bool raw);
int g16_g1_marshal_uncompressed_run(int curve, const void* affine, uint8_t* out, size_t cap, size_t* len);

}  // namespace ga
