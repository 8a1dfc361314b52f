// Groth16 key files and proof bytes, part of the groth16.hip translation unit -- what backend/groth16/bn254/marshal.go does:
//   ProvingKey.ReadFrom / UnsafeReadFrom / ReadDump    a key file, decoded on the device into the staged builder (g16_key.hip.h)
//   ProvingKey.WriteTo / WriteRawTo / WriteDump        the host description of a key (ga_g16_key) -> key-file bytes
//   Proof.WriteTo / WriteRawTo / ReadFrom              proof bytes; G1Affine.Marshal (the BSB22 commitment hash input)
// The formats and the point codec (point_encode / point_decode, host and device) are in keyio.hip.h; the drivers of the entry points
// (g16.hip.h: g16_pk_read_run, g16_key_write_run, g16_marshal_run, ...) are at the end of this file.
#pragma once
#include <string>
#include <vector>

#include "g16_key.hip.h"
#include "keyio.hip.h"

namespace ga {

// ---- checked reads: ProvingKey.ReadFrom semantics (ga_g16_pk_read_*_checked) ------------------------------------------------------------
// Every point the read keeps is tested for curve and subgroup membership where it first sits on the device (check_points.hip.h,
// declared in common.hip.h): an encoded vector chunk by chunk in the staging buffer, right behind the decode
// kernel and beside the file read of the next chunk; a dumped slice once it is uploaded; a header point from its host image.
// The first bad point of a vector ends the read: GA_ERR_INVALID naming the vector, the index within the FILE's vector and the failure.
static const char* key_vector_name(int which, int commitment_half) {
    static const char* const names[GA_KEY_NB_VECTORS] = {"G1.A", "G1.B", "G1.Z", "G1.K", "G2.B"};
    if (which >= 0 && which < GA_KEY_NB_VECTORS) return names[which];
    return commitment_half ? "a commitment key's BasisExpSigma" : "a commitment key's Basis";
}
static int key_check_verdict(const char* name, const uint64_t* out4, int first_status) {
    if (first_status == GA_POINT_OK) return GA_OK;
    set_error("key file: point %llu of %s is %s (%llu of the points kept are off the curve, %llu outside the subgroup)", (unsigned long long)out4[2], name,
              first_status == GA_POINT_OFF_CURVE ? "not on the curve" : "not in the prime-order subgroup", (unsigned long long)out4[0],
              (unsigned long long)out4[1]);
    return GA_ERR_INVALID;
}
// cnt points on the device whose first is point `base` of the file's vector; drains the stream
template <class C, int G>
static int key_check_resident(Ctx* ctx, const void* d_points, uint64_t cnt, uint64_t base, const char* name) {
    uint64_t out4[4];
    int first = GA_POINT_OK;
    GA_CHECK((check_points_resident<C, G>(ctx, ctx->stream, d_points, cnt, base, 1, check_naive_knob())));
    GA_CHECK((check_points_tally<C, G>(ctx, ctx->stream, out4, &first)));
    return key_check_verdict(name, out4, first);
}
template <class C, int G>
static int key_check_header_point(Ctx* ctx, const std::vector<uint8_t>& image, const char* name) {
    uint64_t out4[4];
    GA_CHECK((check_points_run<C, G>(ctx, image.data(), 1, 0, nullptr, out4, check_naive_knob(), 0)));
    return key_check_verdict(name, out4, out4[0] ? GA_POINT_OFF_CURVE : out4[1] ? GA_POINT_NOT_IN_SUBGROUP : GA_POINT_OK);
}

// ---- key files -> staged key (keyio.hip.h has the formats) --------------------------------------------------------------------------
// `count` encoded points of group G from `src`: decoded on the device, the part inside [keep_lo, keep_lo + keep_cnt) lands at d_dst
template <class C, int G>
static int decode_stream(Ctx* ctx, Staging& sg, ByteSource& src, uint64_t count, bool compressed, void* d_dst, uint64_t keep_lo,
                         uint64_t keep_cnt, const char* check_name = nullptr) {   // check_name: a checked read, and what to call the vector
    typedef typename GroupField<C, G>::F F;
    const size_t enc = compressed ? sizeof(F) : 2 * sizeof(F), psz = sizeof(Affine<F>);
    const uint64_t per_chunk = sg.per_pass(enc);
    GA_HIP_CHECK(hipMemsetAsync(sg.d_bad, 0, 4, ctx->stream));
    const int naive = check_name ? check_naive_knob() : 0;
    int k = 0, tally = 0;
    for (uint64_t done = 0; done < count; k ^= 1) {
        const uint64_t cn = count - done < per_chunk ? count - done : per_chunk;
        GA_HIP_CHECK(hipEventSynchronize(sg.ev[k]));   // the previous copy out of this staging buffer has finished
        GA_CHECK(src.read(sg.h[k], cn * enc));
        GA_HIP_CHECK(hipMemcpyAsync(sg.d_bytes, sg.h[k], cn * enc, hipMemcpyHostToDevice, ctx->stream));
        GA_HIP_CHECK(hipEventRecord(sg.ev[k], ctx->stream));
        hipLaunchKernelGGL((key_decode_kernel<C, G>), dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, ctx->stream, (const uint8_t*)sg.d_bytes, cn,
                           compressed ? 1 : 0, sg.d_points, sg.d_bad);
        GA_KERNEL_CHECK();
        const uint64_t b0 = done > keep_lo ? done : keep_lo;
        const uint64_t e0 = done + cn < keep_lo + keep_cnt ? done + cn : keep_lo + keep_cnt;
        if (e0 > b0) {
            GA_HIP_CHECK(hipMemcpyAsync((char*)d_dst + (b0 - keep_lo) * psz, (const char*)sg.d_points + (b0 - done) * psz, (e0 - b0) * psz,
                                        hipMemcpyDeviceToDevice, ctx->stream));
            if (check_name) {   // the kept part of the staged chunk (a point that does not decode is (0,0) here and counted in d_bad)
                GA_CHECK((check_points_resident<C, G>(ctx, ctx->stream, (const char*)sg.d_points + (b0 - done) * psz, e0 - b0, b0, tally == 0, naive)));
                tally = 1;
            }
        }
        done += cn;
    }
    uint32_t bad = 0;
    GA_HIP_CHECK(hipMemcpyAsync(&bad, sg.d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    GA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (bad) {
        set_error("key file: %u of %llu points do not decode (bad flag bits, coordinate >= p, or not on the curve)", bad,
                  (unsigned long long)count);
        return GA_ERR_INVALID;
    }
    if (tally) {
        uint64_t out4[4];
        int first = GA_POINT_OK;
        GA_CHECK((check_points_tally<C, G>(ctx, ctx->stream, out4, &first)));
        GA_CHECK(key_check_verdict(check_name, out4, first));
    }
    return GA_OK;
}

// a []G1Affine / []G2Affine of the Encoder: u32 BE length, then the points (all compressed or all uncompressed)
// mode: the encoding of the STREAM (1 compressed, 0 raw), fixed once from [alpha]1 -- which is never infinity -- by pk_read; -1 =
// unknown, guess from the first byte of the vector (a vector that starts with a point at infinity is then ambiguous on BN254,
// whose infinity flag is the same in both encodings)
template <class C, int G>
static int read_encoded_vector(G16Stage* st, Staging& sg, ByteSource& src, int which, void** d_plain, uint64_t* len_out, int mode = -1,
                               int commitment_half = 0) {
    typedef typename GroupField<C, G>::F F;
    uint32_t len = 0;
    GA_CHECK(src.u32be(&len));
    bool compressed = mode != 0;
    if (len && mode < 0) {
        uint8_t b0;
        GA_CHECK(src.peek(&b0, 1));
        PointFlags f;
        if (!point_flags<C>(b0, &f)) {
            set_error("key file: malformed flag bits 0x%02x at the head of a point vector", b0);
            return GA_ERR_INVALID;
        }
        compressed = f.compressed || (f.infinity && C::ID == GA_BLS12_381 && (b0 & 0x80));
    }
    if (len_out) *len_out = len;
    GA_CHECK(src.expect(len, compressed ? sizeof(Affine<F>) / 2 : sizeof(Affine<F>), "a point vector"));   // before any allocation
    if (which >= 0) {
        GA_CHECK(stage_reserve(st, which, len));
        G16Stage::Vec& x = st->v[which];
        GA_CHECK((decode_stream<C, G>(st->ctx, sg, src, len, compressed, x.d, x.lo, x.cnt, st->checked ? key_vector_name(which, 0) : nullptr)));
        x.seen = len;
        return GA_OK;
    }
    *d_plain = nullptr;   // a commitment basis: kept whole
    hipError_t e = device_malloc(d_plain, len ? (size_t)len * sizeof(Affine<F>) : 16);
    if (e != hipSuccess) {
        set_error("key file: hipMalloc of a commitment basis failed: %s", hipGetErrorString(e));
        return GA_ERR_NOMEM;
    }
    return decode_stream<C, G>(st->ctx, sg, src, len, compressed, *d_plain, 0, len, st->checked ? key_vector_name(which, commitment_half) : nullptr);
}

// a slice of unsafe.WriteSlice: u64 LE length + gnark's own memory image; no arithmetic, file -> pinned buffer -> HBM
template <class C, int G>
static int read_dumped_vector(G16Stage* st, Staging& sg, ByteSource& src, int which, void** d_plain, uint64_t* len_out, int commitment_half = 0) {
    typedef typename GroupField<C, G>::F F;
    const size_t psz = sizeof(Affine<F>);
    uint64_t len = 0;
    GA_CHECK(src.u64le(&len));
    if (len >= (1ull << 40)) {
        set_error("key dump: implausible slice length %llu", (unsigned long long)len);
        return GA_ERR_INVALID;
    }
    if (len_out) *len_out = len;
    GA_CHECK(src.expect(len, psz, "a dumped slice"));   // before any allocation
    char* plain = nullptr;
    if (which >= 0) GA_CHECK(stage_reserve(st, which, len));
    else {
        hipError_t e = device_malloc((void**)&plain, len ? len * psz : 16);
        if (e != hipSuccess) {
            set_error("key dump: hipMalloc of a commitment basis failed: %s", hipGetErrorString(e));
            return GA_ERR_NOMEM;
        }
        *d_plain = plain;
    }
    const uint64_t per_chunk = sg.per_pass(psz);
    int k = 0;
    for (uint64_t done = 0; done < len; k ^= 1) {
        const uint64_t cn = len - done < per_chunk ? len - done : per_chunk;
        GA_HIP_CHECK(hipEventSynchronize(sg.ev[k]));
        GA_CHECK(src.read(sg.h[k], cn * psz));
        if (which >= 0) GA_CHECK(stage_append(st, which, sg.h[k], cn, /*pinned=*/true));
        else GA_HIP_CHECK(hipMemcpyAsync(plain + done * psz, sg.h[k], cn * psz, hipMemcpyHostToDevice, st->ctx->stream));
        GA_HIP_CHECK(hipEventRecord(sg.ev[k], st->ctx->stream));
        done += cn;
    }
    GA_HIP_CHECK(hipStreamSynchronize(st->ctx->stream));
    if (st->checked) {   // a dump is raw memory: nothing has looked at these bytes yet
        if (len > (1ull << 32)) {
            set_error("key dump: a checked read takes slices of at most 2^32 points, this one has %llu", (unsigned long long)len);
            return GA_ERR_INVALID;
        }
        if (which >= 0) GA_CHECK((key_check_resident<C, G>(st->ctx, st->v[which].d, st->v[which].cnt, st->v[which].lo, key_vector_name(which, 0))));
        else GA_CHECK((key_check_resident<C, G>(st->ctx, plain, len, 0, key_vector_name(which, commitment_half))));
    }
    return GA_OK;
}

// one point of the header (alpha, beta, delta): host arithmetic; advances the source by its encoded length
// *mode: -1 = not known yet, 0 = the stream holds uncompressed points, 1 = compressed; set by the first finite point.  BN254 has
// one flag value (0b01) for infinity in both modes, so an infinity point takes the size of the stream's mode (compressed when the
// mode is still unknown -- the size gnark-crypto's SetBytes consumes for it).
template <class C, int G>
static int read_header_point(ByteSource& src, std::vector<uint8_t>* out_image, int* mode = nullptr) {
    typedef typename GroupField<C, G>::F F;
    uint8_t buf[2 * sizeof(F)];
    GA_CHECK(src.peek(buf, 1));
    PointFlags f;
    if (!point_flags<C>(buf[0], &f)) {
        set_error("key file: malformed flag bits 0x%02x", buf[0]);
        return GA_ERR_INVALID;
    }
    bool compressed = f.compressed;
    if (f.infinity && C::ID == GA_BN254) compressed = !(mode && *mode == 0);
    if (!f.infinity && mode && *mode < 0) *mode = f.compressed ? 1 : 0;
    const size_t len = compressed ? sizeof(F) : 2 * sizeof(F);
    GA_CHECK(src.read(buf, len));
    Affine<F> p;
    if (!point_decode<C, G>(buf, compressed, &p)) {   // (the mode of the bytes consumed: an infinity is all zeros over exactly those)
        set_error("key file: header point does not decode");
        return GA_ERR_INVALID;
    }
    out_image->assign(reinterpret_cast<const uint8_t*>(&p), reinterpret_cast<const uint8_t*>(&p) + sizeof(p));
    return GA_OK;
}

// fft.Domain.WriteTo: cardinality + five fr elements (+ the withPrecompute byte of newer gnark-crypto versions, detected by
// trying to decode [alpha]1 right after it)
template <class C>
static int read_domain(ByteSource& src, uint64_t* cardinality) {
    typedef Fe<typename C::FpP> F1;
    GA_CHECK(src.u64be(cardinality));
    uint8_t skip[5 * 32];
    GA_CHECK(src.read(skip, sizeof skip));
    if (*cardinality == 0 || (*cardinality & (*cardinality - 1)) || *cardinality > (1ull << C::FrP::ADICITY)) {
        set_error("key file: domain cardinality %llu is not a power of two within the field's 2-adicity", (unsigned long long)*cardinality);
        return GA_ERR_INVALID;
    }
    uint8_t win[1 + 2 * sizeof(F1)];
    GA_CHECK(src.peek(win, sizeof win));
    auto decodes = [&](const uint8_t* b) {
        PointFlags f;
        Affine<F1> p;
        return point_flags<C>(b[0], &f) && !f.infinity && point_decode<C, GA_G1>(b, f.compressed, &p);
    };
    if (win[0] <= 1 && decodes(win + 1)) {
        uint8_t flag;
        return src.read(&flag, 1);   // withPrecompute
    }
    if (decodes(win)) return GA_OK;
    set_error("key file: [alpha]1 does not decode after the domain block (neither with nor without the withPrecompute byte)");
    return GA_ERR_INVALID;
}

static bool source_is_dump(ByteSource& src) {
    uint8_t m[8];
    static const uint8_t marker[8] = {0xef, 0xbe, 0xad, 0xde, 0, 0, 0, 0};   // uint64(0xdeadbeef) as this (little-endian) platform stores it
    return src.peek(m, 8) == GA_OK && memcmp(m, marker, 8) == 0;
}

template <class C>
static int pk_read(Ctx* ctx, ByteSource& src, int32_t precompute, uint32_t shard_index, uint32_t shard_count, const uint64_t* k_remove,
                   uint64_t len_k_remove, G16Pk** out, bool checked, uint64_t key_chunk) {
    G16Stage st;
    st.ctx = ctx;
    st.checked = checked;
    st.curve = C::ID;
    st.shard_index = shard_index;
    st.shard_count = shard_count ? shard_count : 1;
    GA_CHECK(check_shard_index(st.shard_index, st.shard_count));
    Staging sg;
    sg.chunk = key_chunk;
    GA_CHECK(sg.init());
    const bool dump = source_is_dump(src);
    if (dump) {
        uint8_t m[8];
        GA_CHECK(src.read(m, 8));
    }
    GA_CHECK(read_domain<C>(src, &st.n));
    auto header_tail = [&]() -> int {   // nbWires, NbInfinityA, NbInfinityB, InfinityA, InfinityB, nbCommitments (marshal.go:263-270,335-349)
        uint64_t nb_wires, nia, nib;
        GA_CHECK(src.u64be(&nb_wires));
        GA_CHECK(src.u64be(&nia));
        GA_CHECK(src.u64be(&nib));
        if (nb_wires >= (1ull << 32)) {
            set_error("key file: %llu wires", (unsigned long long)nb_wires);
            return GA_ERR_INVALID;
        }
        if (nia > nb_wires || nib > nb_wires) {
            set_error("key file: %llu / %llu infinity entries for %llu wires", (unsigned long long)nia, (unsigned long long)nib, (unsigned long long)nb_wires);
            return GA_ERR_INVALID;
        }
        if (src.fd < 0 && 2 * nb_wires > src.mem_len - src.mem_pos) {   // (never size a buffer from an untrusted count alone)
            set_error("key image: unexpected end of input (%llu wires announced, %zu bytes left)", (unsigned long long)nb_wires, src.mem_len - src.mem_pos);
            return GA_ERR_INVALID;
        }
        st.nb_wires = nb_wires;
        for (int k = 0; k < 2; k++) {
            st.inf[k].clear();
            for (uint64_t done = 0; done < nb_wires;) {   // grown as the bytes really arrive
                const uint64_t cn = nb_wires - done < (1u << 20) ? nb_wires - done : (1u << 20);
                st.inf[k].resize(done + cn);
                GA_CHECK(src.read(st.inf[k].data() + done, cn));
                done += cn;
            }
            st.have_inf[k] = true;
            uint64_t ones = 0;
            for (uint8_t b : st.inf[k]) ones += b != 0;
            if (ones != (k == 0 ? nia : nib)) {
                set_error("key file: Infinity%c holds %llu set entries, the header says %llu", k == 0 ? 'A' : 'B', (unsigned long long)ones,
                          (unsigned long long)(k == 0 ? nia : nib));
                return GA_ERR_INVALID;
            }
        }
        return GA_OK;
    };
    uint32_t nb_commitments = 0;
    int mode = -1;   // compressed (1) or raw (0) stream: taken from [alpha]1, the first point, which is never infinity
    if (!dump) {   // ReadFrom order, marshal.go:316-330
        GA_CHECK((read_header_point<C, GA_G1>(src, &st.pts[GA_KEY_G1_ALPHA], &mode)));
        GA_CHECK((read_header_point<C, GA_G1>(src, &st.pts[GA_KEY_G1_BETA], &mode)));
        GA_CHECK((read_header_point<C, GA_G1>(src, &st.pts[GA_KEY_G1_DELTA], &mode)));
        for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_Z, GA_KEY_G1_K}) GA_CHECK((read_encoded_vector<C, GA_G1>(&st, sg, src, w, nullptr, nullptr, mode)));
        GA_CHECK((read_header_point<C, GA_G2>(src, &st.pts[GA_KEY_G2_BETA], &mode)));
        GA_CHECK((read_header_point<C, GA_G2>(src, &st.pts[GA_KEY_G2_DELTA], &mode)));
        GA_CHECK((read_encoded_vector<C, GA_G2>(&st, sg, src, GA_KEY_G2_B, nullptr, nullptr, mode)));
        GA_CHECK(header_tail());
        GA_CHECK(src.u32be(&nb_commitments));
    } else {       // ReadDump order, marshal.go:459-478
        GA_CHECK((read_header_point<C, GA_G1>(src, &st.pts[GA_KEY_G1_ALPHA])));
        GA_CHECK((read_header_point<C, GA_G1>(src, &st.pts[GA_KEY_G1_BETA])));
        GA_CHECK((read_header_point<C, GA_G1>(src, &st.pts[GA_KEY_G1_DELTA])));
        GA_CHECK((read_header_point<C, GA_G2>(src, &st.pts[GA_KEY_G2_BETA])));
        GA_CHECK((read_header_point<C, GA_G2>(src, &st.pts[GA_KEY_G2_DELTA])));
        GA_CHECK(header_tail());
        GA_CHECK(src.u32be(&nb_commitments));
        for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_Z, GA_KEY_G1_K}) GA_CHECK((read_dumped_vector<C, GA_G1>(&st, sg, src, w, nullptr, nullptr)));
        GA_CHECK((read_dumped_vector<C, GA_G2>(&st, sg, src, GA_KEY_G2_B, nullptr, nullptr)));
    }
    if (nb_commitments > 4096) {
        set_error("key file: implausible number of commitment keys %u", nb_commitments);
        return GA_ERR_INVALID;
    }
    if (checked) {   // the header points: decoded on the host (the curve equation) in either format
        GA_CHECK((key_check_header_point<C, GA_G1>(ctx, st.pts[GA_KEY_G1_ALPHA], "[alpha]1")));
        GA_CHECK((key_check_header_point<C, GA_G1>(ctx, st.pts[GA_KEY_G1_BETA], "[beta]1")));
        GA_CHECK((key_check_header_point<C, GA_G1>(ctx, st.pts[GA_KEY_G1_DELTA], "[delta]1")));
        GA_CHECK((key_check_header_point<C, GA_G2>(ctx, st.pts[GA_KEY_G2_BETA], "[beta]2")));
        GA_CHECK((key_check_header_point<C, GA_G2>(ctx, st.pts[GA_KEY_G2_DELTA], "[delta]2")));
    }
    for (uint32_t i = 0; i < nb_commitments; i++) {   // pedersen.ProvingKey: Basis, BasisExpSigma
        void *db = nullptr, *ds = nullptr;
        uint64_t lb = 0, ls = 0;
        int rc = dump ? read_dumped_vector<C, GA_G1>(&st, sg, src, -1, &db, &lb) : read_encoded_vector<C, GA_G1>(&st, sg, src, -1, &db, &lb, mode);
        if (rc == GA_OK) rc = dump ? read_dumped_vector<C, GA_G1>(&st, sg, src, -1, &ds, &ls, 1) : read_encoded_vector<C, GA_G1>(&st, sg, src, -1, &ds, &ls, mode, 1);
        if (rc == GA_OK && lb != ls) {
            set_error("key file: commitment key %u has %llu basis points and %llu sigma points", i, (unsigned long long)lb, (unsigned long long)ls);
            rc = GA_ERR_INVALID;
        }
        if (rc != GA_OK) {
            hipFree(db);
            hipFree(ds);
            return rc;
        }
        st.d_ck_basis.push_back(db);
        st.d_ck_sigma.push_back(ds);
        st.ck_len.push_back(lb);
    }
    if (len_k_remove) st.k_remove.assign(k_remove, k_remove + len_k_remove);
    return stage_finish_any(&st, precompute, out);
}

// ---- key writers: the host description (ga_g16_key) -> WriteTo / WriteRawTo / WriteDump bytes ------------------------------------------
template <class C, int G>
static int write_encoded_vector(Ctx* ctx, Staging& sg, ByteSink& dst, const void* pts, uint64_t len, bool compressed) {
    typedef typename GroupField<C, G>::F F;
    if (len >= (1ull << 32)) {
        set_error("key writer: a vector of %llu points does not fit the u32 length prefix", (unsigned long long)len);
        return GA_ERR_INVALID;
    }
    GA_CHECK(dst.u32be((uint32_t)len));
    const size_t enc = compressed ? sizeof(F) : 2 * sizeof(F), psz = sizeof(Affine<F>);
    const uint64_t per_chunk = sg.per_pass(psz);
    for (uint64_t done = 0; done < len;) {
        const uint64_t cn = len - done < per_chunk ? len - done : per_chunk;
        GA_HIP_CHECK(hipMemcpyAsync(sg.d_points, (const char*)pts + done * psz, cn * psz, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL((key_encode_kernel<C, G>), dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, ctx->stream, (const void*)sg.d_points, cn,
                           compressed ? 1 : 0, sg.d_bytes);
        GA_KERNEL_CHECK();
        GA_HIP_CHECK(hipMemcpyAsync(sg.h[0], sg.d_bytes, cn * enc, hipMemcpyDeviceToHost, ctx->stream));
        GA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        GA_CHECK(dst.write(sg.h[0], cn * enc));
        done += cn;
    }
    return GA_OK;
}
// one point of an affine memory image -> its encoding at `out`; returns the encoded length
template <class C, int G>
static size_t encode_point(const void* affine, bool compressed, uint8_t* out) {
    typedef typename GroupField<C, G>::F F;
    Affine<F> p;
    memcpy(&p, affine, sizeof p);
    point_encode<C, G>(p, compressed, out);
    return compressed ? sizeof(F) : 2 * sizeof(F);
}
template <class C, int G>
static int write_header_point(ByteSink& dst, const void* affine, bool compressed) {
    uint8_t buf[2 * sizeof(typename GroupField<C, G>::F)];
    return dst.write(buf, encode_point<C, G>(affine, compressed, buf));
}
template <class C>
static int write_domain(ByteSink& dst, uint64_t n) {
    typedef typename C::FrP FrP;
    typedef Fe<FrP> F;
    const int logn = ilog2_u64(n);
    if ((1ull << logn) != n || logn > FrP::ADICITY) {
        set_error("key writer: domain cardinality %llu", (unsigned long long)n);
        return GA_ERR_INVALID;
    }
    F w = fe_const<FrP>(FrP::ROOT), wi = fe_const<FrP>(FrP::ROOT_INV);
    for (int k = 0; k < FrP::ADICITY - logn; k++) {
        w = sqr(w);
        wi = sqr(wi);
    }
    F card = fe_zero<FrP>();
    card.l[0] = (uint32_t)n;
    card.l[1] = (uint32_t)(n >> 32);
    const F elems[5] = {inv(to_mont(card)), w, wi, fe_const<FrP>(FrP::GEN), fe_const<FrP>(FrP::GEN_INV)};
    GA_CHECK(dst.u64be(n));
    for (const F& e : elems) {
        uint8_t b[32];
        fe_to_be_bytes(e, b);
        GA_CHECK(dst.write(b, 32));
    }
    const uint8_t with_precompute = 1;
    return dst.write(&with_precompute, 1);
}
template <class C>
static int key_write(Ctx* ctx, const ga_g16_key* key, int format, ByteSink& dst, uint64_t key_chunk) {
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    const bool dump = format == GA_KEY_FORMAT_DUMP, compressed = format == GA_KEY_FORMAT_COMPRESSED;
    Staging sg;
    sg.chunk = key_chunk;
    GA_CHECK(sg.init());
    if (dump) GA_CHECK(dst.u64le(0xdeadbeefull));
    GA_CHECK(write_domain<C>(dst, key->domain_cardinality));
    const bool hc = compressed;   // header points follow the encoder's mode (raw for the dump)
    auto tail = [&]() -> int {
        GA_CHECK(dst.u64be(key->nb_wires));
        GA_CHECK(dst.u64be(key->nb_infinity_a));
        GA_CHECK(dst.u64be(key->nb_infinity_b));
        GA_CHECK(dst.write(key->infinity_a, key->nb_wires));
        GA_CHECK(dst.write(key->infinity_b, key->nb_wires));
        return dst.u32be(key->nb_commitments);
    };
    auto slice = [&](const void* p, uint64_t len, size_t psz) -> int {
        GA_CHECK(dst.u64le(len));
        return dst.write(p, len * psz);
    };
    GA_CHECK((write_header_point<C, GA_G1>(dst, key->g1_alpha, hc)));
    GA_CHECK((write_header_point<C, GA_G1>(dst, key->g1_beta, hc)));
    GA_CHECK((write_header_point<C, GA_G1>(dst, key->g1_delta, hc)));
    if (!dump) {
        GA_CHECK((write_encoded_vector<C, GA_G1>(ctx, sg, dst, key->g1_a, key->len_a, compressed)));
        GA_CHECK((write_encoded_vector<C, GA_G1>(ctx, sg, dst, key->g1_b, key->len_b, compressed)));
        GA_CHECK((write_encoded_vector<C, GA_G1>(ctx, sg, dst, key->g1_z, key->len_z, compressed)));
        GA_CHECK((write_encoded_vector<C, GA_G1>(ctx, sg, dst, key->g1_k, key->len_k, compressed)));
    }
    GA_CHECK((write_header_point<C, GA_G2>(dst, key->g2_beta, hc)));
    GA_CHECK((write_header_point<C, GA_G2>(dst, key->g2_delta, hc)));
    if (!dump) GA_CHECK((write_encoded_vector<C, GA_G2>(ctx, sg, dst, key->g2_b, key->len_b2, compressed)));
    GA_CHECK(tail());
    if (dump) {
        GA_CHECK(slice(key->g1_a, key->len_a, sizeof(Affine<F1>)));
        GA_CHECK(slice(key->g1_b, key->len_b, sizeof(Affine<F1>)));
        GA_CHECK(slice(key->g1_z, key->len_z, sizeof(Affine<F1>)));
        GA_CHECK(slice(key->g1_k, key->len_k, sizeof(Affine<F1>)));
        GA_CHECK(slice(key->g2_b, key->len_b2, sizeof(Affine<F2>)));
    }
    for (uint32_t i = 0; i < key->nb_commitments; i++) {
        if (dump) {
            GA_CHECK(slice(key->ck_basis[i], key->ck_len[i], sizeof(Affine<F1>)));
            GA_CHECK(slice(key->ck_basis_exp_sigma[i], key->ck_len[i], sizeof(Affine<F1>)));
        } else {
            GA_CHECK((write_encoded_vector<C, GA_G1>(ctx, sg, dst, key->ck_basis[i], key->ck_len[i], compressed)));
            GA_CHECK((write_encoded_vector<C, GA_G1>(ctx, sg, dst, key->ck_basis_exp_sigma[i], key->ck_len[i], compressed)));
        }
    }
    return GA_OK;
}

// Proof.ReadFrom (marshal.go:62-86): Ar | Bs | Krs | u32 n | n commitments | CommitmentPok, compressed or uncompressed points
template <class C>
static int proof_unmarshal(const uint8_t* data, size_t len, void* proof_out, void* commitments_out, uint32_t max_commitments,
                           uint32_t* n_commitments, void* pok_out, size_t* consumed) {
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    ByteSource src{data, len};
    std::vector<uint8_t> img;
    int mode = -1;
    char* o = reinterpret_cast<char*>(proof_out);
    GA_CHECK((read_header_point<C, GA_G1>(src, &img, &mode)));
    memcpy(o, img.data(), sizeof(Affine<F1>));
    GA_CHECK((read_header_point<C, GA_G2>(src, &img, &mode)));
    memcpy(o + sizeof(Affine<F1>), img.data(), sizeof(Affine<F2>));
    GA_CHECK((read_header_point<C, GA_G1>(src, &img, &mode)));
    memcpy(o + sizeof(Affine<F1>) + sizeof(Affine<F2>), img.data(), sizeof(Affine<F1>));
    uint32_t n = 0;
    GA_CHECK(src.u32be(&n));
    if (n > max_commitments || (n && !commitments_out)) {
        set_error("proof: %u commitments, room for %u", n, max_commitments);
        return GA_ERR_INVALID;
    }
    for (uint32_t i = 0; i < n; i++) {
        GA_CHECK((read_header_point<C, GA_G1>(src, &img, &mode)));
        memcpy(reinterpret_cast<char*>(commitments_out) + (size_t)i * sizeof(Affine<F1>), img.data(), sizeof(Affine<F1>));
    }
    GA_CHECK((read_header_point<C, GA_G1>(src, &img, &mode)));
    if (pok_out) memcpy(pok_out, img.data(), sizeof(Affine<F1>));
    if (n_commitments) *n_commitments = n;
    if (consumed) *consumed = src.mem_pos;
    return GA_OK;
}
// Proof.WriteTo / WriteRawTo (marshal.go:25-58): Ar | Bs | Krs | u32 BE n | n commitments | CommitmentPok, all compressed or all raw
template <class C>
static int marshal(const void* proof, const void* commitments, uint32_t ncom, const void* pok, uint8_t* out, size_t cap, size_t* len, bool raw) {
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    const size_t nb = C::FpP::N * 4;
    const size_t need = (raw ? 2 : 1) * (nb + 2 * nb + nb + (size_t)ncom * nb + nb) + 4;
    if (cap < need) {
        set_error("proof marshal: buffer too small (%zu < %zu)", cap, need);
        return GA_ERR_INVALID;
    }
    const char* p = reinterpret_cast<const char*>(proof);
    size_t o = 0;
    o += encode_point<C, GA_G1>(p, !raw, out + o);
    o += encode_point<C, GA_G2>(p + sizeof(Affine<F1>), !raw, out + o);
    o += encode_point<C, GA_G1>(p + sizeof(Affine<F1>) + sizeof(Affine<F2>), !raw, out + o);
    out[o] = ncom >> 24;   // uint32 big-endian number of commitments (the slice encoder's length prefix)
    out[o + 1] = ncom >> 16;
    out[o + 2] = ncom >> 8;
    out[o + 3] = ncom;
    o += 4;
    for (uint32_t i = 0; i < ncom; i++) o += encode_point<C, GA_G1>((const char*)commitments + i * sizeof(Affine<F1>), !raw, out + o);
    Affine<F1> inf;
    memset(&inf, 0, sizeof(inf));
    o += encode_point<C, GA_G1>(pok ? pok : &inf, !raw, out + o);   // CommitmentPok (infinity without commitments)
    *len = o;
    return GA_OK;
}

// ---- the drivers of the entry points (g16.hip.h) -----------------------------------------------------------------------------------
int g16_pk_read_run(Ctx* ctx, int curve, const uint8_t* data, size_t len, int fd, int32_t precompute, uint32_t shard_index, uint32_t shard_count,
                    const uint64_t* k_remove, uint64_t len_k_remove, G16Pk** out, uint64_t* bytes_read, bool checked, uint64_t key_chunk) {
    ByteSource src{data, len, 0, fd};   // (the entry point passes fd = -1 with data, data = null with a descriptor)
    CtxLock g(ctx);
    G16Pk* pk = nullptr;
    GA_CHECK(GA_DISPATCH(Scope::FULL, curve, GA_NO_GROUP, return pk_read<C>(ctx, src, precompute, shard_index, shard_count, k_remove, len_k_remove, &pk, checked, key_chunk)));
    *out = pk;
    if (bytes_read) *bytes_read = src.consumed;
    return GA_OK;
}

int g16_key_write_run(Ctx* ctx, const ga_g16_key* key, int format, int fd, uint64_t* bytes_written, uint64_t key_chunk) {
    if (abi_bad_argument(!key_points_present(key) || (key->nb_commitments && (!key->ck_basis || !key->ck_basis_exp_sigma || !key->ck_len)),
                         "null pointer inside ga_g16_key"))
        return GA_ERR_INVALID;
    CtxLock g(ctx);
    ByteSink dst{fd};
    GA_CHECK(GA_DISPATCH(Scope::FULL, key->curve, GA_NO_GROUP, return key_write<C>(ctx, key, format, dst, key_chunk)));
    if (bytes_written) *bytes_written = dst.written;
    return GA_OK;
}

int g16_proof_unmarshal_run(int curve, const uint8_t* data, size_t len, void* proof_out, void* commitments_out, uint32_t max_commitments,
                            uint32_t* n_commitments, void* pok_out, size_t* consumed) {
    return GA_DISPATCH(Scope::FULL, curve, GA_NO_GROUP,
                       return proof_unmarshal<C>(data, len, proof_out, commitments_out, max_commitments, n_commitments, pok_out, consumed));
}

int g16_point_unmarshal_run(int curve, int group, const uint8_t* data, size_t len, void* affine_out, size_t* consumed) {
    ByteSource src{data, len};
    std::vector<uint8_t> img;
    GA_CHECK(GA_DISPATCH(Scope::FULL, curve, group, return (read_header_point<C, G>(src, &img))));
    memcpy(affine_out, img.data(), img.size());
    if (consumed) *consumed = src.mem_pos;
    return GA_OK;
}

int g16_marshal_run(int curve, const void* proof, const void* commitments, uint32_t n, const void* pok, uint8_t* out, size_t cap, size_t* len, bool raw) {
    return GA_DISPATCH(Scope::FULL, curve, GA_NO_GROUP, return marshal<C>(proof, commitments, n, pok, out, cap, len, raw));
}

int g16_g1_marshal_uncompressed_run(int curve, const void* affine, uint8_t* out, size_t cap, size_t* len) {
    return GA_DISPATCH(Scope::FULL, curve, GA_NO_GROUP, {
        if (abi_bad_argument(cap < 2 * sizeof(Fe<typename C::FpP>), "buffer too small")) return GA_ERR_INVALID;
        *len = encode_point<C, GA_G1>(affine, false, out);
    });
}

}  // namespace ga
