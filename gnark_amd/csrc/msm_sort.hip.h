// Stages 1 and 2 of the MSM pipeline (msm.hip.h): scalars -> (key, value) pairs grouped by bucket.  Depends on the scalar field only.
//   1. / 2.  msm_digits_kernel + msm_sort_pairs: the digits, then the library's radix sort (small MSMs)
//   1b / 1c  the same in ONE two-level sort of our own, fused with the digit extraction (msm_fused_sort)
//   msm_sort picks between them.
#pragma once
#include <hipcub/hipcub.hpp>
#include <rocprim/device/device_radix_sort.hpp>

#include <string>

#include "common.hip.h"

namespace ga {

constexpr uint32_t MSM_SIGN = 0x80000000u;   // the value of a pair: point index | sign of the digit << 31

// Onesweep configuration for the bucket keys of large MSMs (17..22 significant bits at c = 18..22): two 11-bit passes instead of
// the library default's three 8-bit ones.  Measured on 12 x 2^24 pairs with 22-bit keys (tools/exp/sortbench.hip,
// profiles/r02_e_sort_configs.txt): default 4.34 ms, 1024 threads x 21 items with 11-bit digits 3.47 ms; 512-thread blocks,
// 12-bit digits (LDS) and more items per thread are slower or do not fit.
typedef rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                   rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 21>, rocprim::kernel_config<1024, 21>, 11,
                                                                       rocprim::block_radix_rank_algorithm::match>>
    MsmSortWide;

// Sort (key, value) pairs on the low end_bit key bits, ping-ponging between the two buffer pairs (no third copy of the data); on
// return keys2/vals2 point at the sorted arrays and keys/vals at the other pair.  The library sort: small MSMs, and whatever the
// fused path (1b / 1c below) does not take.
inline int msm_sort_pairs(Ctx* ctx, const std::string& tmp_name, uint32_t*& keys, uint32_t*& keys2, uint32_t*& vals, uint32_t*& vals2, size_t m,
                          int end_bit, hipStream_t st) {
    rocprim::double_buffer<uint32_t> dk(keys, keys2), dv(vals, vals2);
    const bool wide = (end_bit + 10) / 11 < (end_bit + 7) / 8;   // fewer passes with 11-bit digits than with 8-bit ones
    size_t tmp_bytes = 0;
    void* tmp = nullptr;
    if (wide) GA_HIP_CHECK((rocprim::radix_sort_pairs<MsmSortWide>(nullptr, tmp_bytes, dk, dv, m, 0u, (unsigned)end_bit, st)));
    else GA_HIP_CHECK((rocprim::radix_sort_pairs(nullptr, tmp_bytes, dk, dv, m, 0u, (unsigned)end_bit, st)));
    GA_CHECK(ctx->scratch_get(tmp_name.c_str(), tmp_bytes + 256, &tmp));
    if (wide) GA_HIP_CHECK((rocprim::radix_sort_pairs<MsmSortWide>(tmp, tmp_bytes, dk, dv, m, 0u, (unsigned)end_bit, st)));
    else GA_HIP_CHECK((rocprim::radix_sort_pairs(tmp, tmp_bytes, dk, dv, m, 0u, (unsigned)end_bit, st)));
    keys2 = dk.current();
    keys = dk.alternate();
    vals2 = dv.current();
    vals = dv.alternate();
    return GA_OK;
}

// ---- 1. digits ------------------------------------------------------------------------------------
// The signed c-bit digits of one scalar, least significant window first: (key, value) of window w.
// table mode: every window shares ONE bucket set (bucket set `key_base / half` of a batch of scalar vectors over the same
// table) and the value indexes the precomputed table [window][point]; skip = total bucket count (sorts last)
template <class FrP>
struct DigitWalk {
    Fe<FrP> s;
    uint32_t carry = 0;
    __device__ __forceinline__ void load(const uint32_t* __restrict__ scalars, uint64_t i, int mont) { set(load_fe<FrP>(scalars + i * 8), mont); }
    __device__ __forceinline__ void set(const Fe<FrP>& raw, int mont) {   // (the words may have been loaded ahead of time)
        s = raw;
        if (mont) s = from_mont(s);
        else {
            // canonical input may be any 256-bit integer (a caller's big.Int bytes): bring it below r (canonical_steps, field.hip.h),
            // so that only (BITS mod c) bits are live in the top window as the digit loop assumes
            // (BITS mod c == 0 -- c = 15, 17 for the 255-bit field, c = 11, 23 for BLS12-377's 253 bits -- leaves the top window of
            // BITS / c + 1 with the signed-digit carry alone: digit 0 or 1, never negative, so nothing carries out of it)
#pragma unroll 1
            for (int k = 0; k < canonical_steps<FrP>(); k++) reduce_once<FrP>(s.l);
        }
    }
    __device__ __forceinline__ void next(int c, int w, int win_lo, uint64_t n, uint64_t i, int table, uint32_t key_base, uint32_t skip,
                                         uint32_t& key, uint32_t& val) {
        const uint32_t half = 1u << (c - 1);
        const uint32_t mask = (1u << c) - 1;
        uint32_t d = (s.l[0] & mask) + carry;
        // s >>= c  (c < 32)
#pragma unroll
        for (int k = 0; k < 7; k++) s.l[k] = (s.l[k] >> c) | (s.l[k + 1] << (32 - c));
        s.l[7] >>= c;
        uint32_t neg = 0;
        if (d > half) {
            d = (1u << c) - d;
            neg = MSM_SIGN;
            carry = 1;
        } else {
            carry = 0;
        }
        key = d == 0 ? skip : key_base + (table ? 0u : (uint32_t)(w - win_lo) * half) + (d - 1);
        val = (table ? (uint32_t)((uint64_t)w * n + i) : (uint32_t)i) | neg;
    }
};

template <class FrP>
__global__ void msm_digits_kernel(const uint32_t* __restrict__ scalars, uint64_t n, int mont, int c, int nwin, int win_lo,
                                  int win_hi, int table, uint32_t key_base, uint32_t skip, uint32_t* __restrict__ keys,
                                  uint32_t* __restrict__ vals) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DigitWalk<FrP> D;
    D.load(scalars, i, mont);
    for (int w = 0; w < nwin; w++) {
        uint32_t k, v;
        D.next(c, w, win_lo, n, i, table, key_base, skip, k, v);
        if (w >= win_lo && w < win_hi) {
            uint64_t idx = (uint64_t)(w - win_lo) * n + i;
            keys[idx] = k;
            vals[idx] = v;
        }
    }
}

// ---- 1b. digits fused with the first level of the sort (large bucket sets) ------------------------------------------------------
// The plain sequence writes the (key, value) pairs in scalar order (1.6 GB at 12 x 2^24), reads the keys for the histograms and
// reads / scatters the pairs twice (two 11-bit onesweep passes).  Here the FIRST level -- a partition into at most 2^BITS groups of
// consecutive keys -- is made by the kernel that extracts the digits: a histogram of the groups straight from the scalars (digits
// are cheap to recompute: nothing is written), then a tile of <= 1024 scalars x windows is partitioned in LDS and leaves the CU as
// one run per (tile, group); the second level (1c below) finishes the grouping without the library.
// The order inside a group is not the input order (ranks come from LDS atomics) -- irrelevant for a first level.  Any key distribution
// works: a group's slice of the output is reserved with one global atomic per (tile, group).
// Measured at 12 x 2^24 pairs (tools/exp/partbench.hip, profiles/README.md round 3 batch ZZ2): digits 0.37 + sort 3.62 ms ->
// histogram 0.19 + digits/first pass 1.38 + one library pass for the other bits 1.87 ms (1c replaces that pass).
constexpr int MSM_P1_THREADS = 1024;
constexpr int MSM_P1_MAXW = 16;                       // windows a thread keeps in registers
constexpr uint32_t MSM_P1_ENTRIES = 1024 * 13;        // pairs staged per tile: 104 KB of LDS (+ 16 / 32 KB of bin tables)
constexpr uint32_t MSM_P2_SEG = 16384;                // pairs per second-level segment
constexpr uint32_t MSM_P2_HB = 4104;                  // capacity for the key parts the second level counts in LDS
constexpr uint32_t MSM_XCDS = 8;                      // XCDs of the device: block b is observed to run on XCD b % 8 (a speed assumption only)
// How a key splits between the two levels: the first level groups by key >> low (at most 2^BITS groups), the second level counts the
// 2^low <= 4096 low parts of a group's keys.  A group owns a CONTIGUOUS key range, hence a contiguous slice of the per-key counters,
// of the cursors and of the sorted output: a segment's atomics are consecutive words and its runs land inside the group's own slice.
// (Rounds 3 and 4 split the other way round -- first level on the low 11 / 12 key bits -- which spreads one segment's counters and
// runs 2^BITS keys apart: one memory transaction per (segment, key) three times over.  Same box, 2^24 points,
// profiles/r05_a_sort_ab_2p24.txt: second level 4.06 -> 1.38 ms on the 13 x 2^19 keys of un-pinned bases, 1.44 -> 1.08 ms on a
// table's 2^21 keys; with the XCD placement below 1.15 / 0.98 ms and the first level 1.80 -> 1.44 / 1.73 -> 1.28 ms.)
// BITS = 11 while 2^12 low parts suffice, else 12 (key spaces up to 2^24).
static inline int msm_p1_bits(uint64_t nb) { return (nb >> 12) + 1 <= 2048 ? 11 : 12; }
static inline bool msm_fused_fits(uint64_t nb) {
    const int b = msm_p1_bits(nb);
    return nb >= (1ull << b) && (nb >> 12) + 1 <= (1ull << b);
}
static inline int msm_key_low(uint64_t nb, int bits) {   // smallest low with (nb >> low) + 1 <= 2^bits groups
    int low = 0;
    while ((nb >> low) + 1 > (1ull << bits)) low++;
    return low;
}
static inline uint32_t msm_p1_tile_scalars(int nwl) {
    const uint32_t t = MSM_P1_ENTRIES / (uint32_t)nwl;
    return t < (uint32_t)MSM_P1_THREADS ? t : (uint32_t)MSM_P1_THREADS;
}
// In-place exclusive prefix sums of a[0, count) in LDS by a block of exactly 1024 threads (count <= 5 * 1024); a[count] receives the
// total, which is also returned.  wtot: 16 words of LDS.  The caller has synchronised the block on a[]; the block is synchronised on
// return.  (Round 3 scanned with two ping-pong arrays: 3 x 4 bytes per bin instead of 1 -- what kept 12-bit levels out of 160 KB.)
__device__ __forceinline__ uint32_t msm_block_excl_scan_1024(uint32_t* __restrict__ a, uint32_t count, uint32_t* __restrict__ wtot) {
    GA_REQUIRE_WAVE64();   // 16 waves of 64 lanes: lane 63 publishes the wave total, __shfl_up runs to distance 32
    constexpr int PER = 5;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t v[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const uint32_t idx = t * PER + k;
        const uint32_t x = idx < count ? a[idx] : 0;
        v[k] = s;
        s += x;
    }
    uint32_t inc = s;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) {
        const uint32_t x = wtot[w];
        if (w < wave) base += x;
        total += x;
    }
    base += inc - s;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const uint32_t idx = t * PER + k;
        if (idx < count) a[idx] = base + v[k];
    }
    if (t == 0) a[count] = total;
    __syncthreads();
    return total;
}

// Histogram of the first-level groups straight from the scalars (digits recomputed, nothing written).  A block walks whole TILES of
// the first pass (tile t, t + grid, ...; the grid is a multiple of 8), so that with per-XCD slices (ncls = 8) the counts of class
// t % 8 -- the XCD the first pass's block t is expected on -- are kept apart: ghist[bin * ncls + class].
template <class FrP, int BITS>
__global__ void __launch_bounds__(256)
msm_digit_hist_kernel(const uint32_t* __restrict__ scalars, uint64_t n, int mont, int c, int nwin, int win_lo, int win_hi, int table,
                      uint32_t key_base, uint32_t skip, uint32_t tile_scalars, int low, uint32_t ncls, uint32_t* __restrict__ ghist) {
    constexpr uint32_t BINS = 1u << BITS;
    __shared__ uint32_t h[BINS];
    for (uint32_t b = threadIdx.x; b < BINS; b += blockDim.x) h[b] = 0;
    __syncthreads();
    const uint64_t ntiles = (n + tile_scalars - 1) / tile_scalars;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * tile_scalars;
        const uint64_t i1 = i0 + tile_scalars < n ? i0 + tile_scalars : n;
        for (uint64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            DigitWalk<FrP> D;
            D.load(scalars, i, mont);
            for (int w = 0; w < win_hi; w++) {
                uint32_t k, v;
                D.next(c, w, win_lo, n, i, table, key_base, skip, k, v);
                if (w >= win_lo) atomicAdd(&h[(k >> low)], 1u);
            }
        }
    }
    __syncthreads();
    const uint32_t cls = ncls > 1 ? (blockIdx.x % ncls) : 0;
    for (uint32_t b = threadIdx.x; b < BINS; b += blockDim.x)
        if (h[b]) atomicAdd(&ghist[b * ncls + cls], h[b]);
}

// exclusive scans of the group counts (one block): where each group's slice of the partitioned arrays starts (bin_off: kept, BINS + 1
// entries), where each (group, class) sub-slice starts (cursor: consumed by the first pass) and the number of MSM_P2_SEG-pair
// segments before each group (seg_off)
template <int BITS>
static __global__ void __launch_bounds__(1024) msm_p1_scan_kernel(const uint32_t* __restrict__ ghist, uint32_t ncls, uint32_t* __restrict__ cursor,
                                                                  uint32_t* __restrict__ bin_off, uint32_t* __restrict__ seg_off) {
    constexpr uint32_t BINS = 1u << BITS;
    __shared__ uint32_t a[BINS + 1], g[BINS + 1], wtot[16];
    for (uint32_t b = threadIdx.x; b < BINS; b += blockDim.x) {
        uint32_t tot = 0;
        for (uint32_t k = 0; k < ncls; k++) tot += ghist[b * ncls + k];
        a[b] = tot;
        g[b] = (tot + MSM_P2_SEG - 1) / MSM_P2_SEG;
    }
    __syncthreads();
    msm_block_excl_scan_1024(a, BINS, wtot);
    msm_block_excl_scan_1024(g, BINS, wtot);
    for (uint32_t b = threadIdx.x; b <= BINS; b += blockDim.x) {
        if (b < BINS) {
            uint32_t s = a[b];
            for (uint32_t k = 0; k < ncls; k++) {
                cursor[b * ncls + k] = s;
                s += ghist[b * ncls + k];
            }
        }
        bin_off[b] = a[b];
        seg_off[b] = g[b];
    }
}

// A block walks tiles blockIdx.x, blockIdx.x + grid, ... (the grid is a multiple of 8 whenever a block gets more than one tile, so a
// block's tiles share its XCD class) and loads the NEXT tile's scalars before it writes the current one out: the CU holds one
// workgroup (123 KB of LDS), so nothing else could hide that load.  Same box, 12 x 2^24 pairs (profiles/r05_s_sort_pipelined_ab.txt):
// histogram + first level 1.19 -> 1.13 ms with 256 / 512 / 1024 blocks (one tile per block in this loop form: 1.26).
template <class FrP, int BITS>
__global__ void __launch_bounds__(MSM_P1_THREADS)
msm_digits_pass1_kernel(const uint32_t* __restrict__ scalars, uint64_t n, int mont, int c, int nwin, int win_lo, int win_hi, int table,
                        uint32_t key_base, uint32_t skip, uint32_t tile_scalars, uint64_t ntiles, int low, uint32_t ncls,
                        uint32_t* __restrict__ cursor, uint16_t* __restrict__ out_keys, uint32_t* __restrict__ out_vals) {
    constexpr uint32_t BINS = 1u << BITS;
    __shared__ uint32_t stage_k[MSM_P1_ENTRIES], stage_v[MSM_P1_ENTRIES];
    __shared__ uint32_t start[BINS + 1], delta[BINS], wtot[16];   // start: counts, then (scanned in place) where a bin's run starts in the staging arrays
    const uint32_t t = threadIdx.x;
    const uint32_t cls = ncls > 1 ? (blockIdx.x % ncls) : 0;
    uint64_t i = (uint64_t)blockIdx.x * tile_scalars + t;
    bool live = t < tile_scalars && i < n;
    Fe<FrP> raw;
    if (live) raw = load_fe<FrP>(scalars + i * 8);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (uint32_t b = t; b < BINS; b += blockDim.x) start[b] = 0;
        __syncthreads();
        uint32_t key[MSM_P1_MAXW], val[MSM_P1_MAXW], rank[MSM_P1_MAXW];
        if (live) {
            DigitWalk<FrP> D;
            D.set(raw, mont);
            for (int w = 0; w < win_lo; w++) {   // (windows below this device's share: only their carries matter)
                uint32_t k, v;
                D.next(c, w, win_lo, n, i, table, key_base, skip, k, v);
            }
#pragma unroll
            for (int q = 0; q < MSM_P1_MAXW; q++)
                if (win_lo + q < win_hi) {
                    D.next(c, win_lo + q, win_lo, n, i, table, key_base, skip, key[q], val[q]);
                    rank[q] = atomicAdd(&start[(key[q] >> low)], 1u);
                }
        }
        __syncthreads();
        const uint32_t total = msm_block_excl_scan_1024(start, BINS, wtot);
        // a bin's slice of the output is reserved with one global atomic per (tile, bin) -- with per-XCD slices (ncls = 8) inside the
        // sub-slice of this block's class, so that the runs one XCD's L2 collects are neighbours; delta = where the run goes - where
        // it is staged.  (The reservations are issued here and their results used only after the staging below, so that the atomics'
        // round trips run under the LDS writes: 1.26 -> 1.23 ms at 12 x 2^24 pairs, profiles/r05_n_sort_atomics_ab.txt.)
        constexpr int PER_T = (int)(BINS / MSM_P1_THREADS);
        uint32_t got[PER_T];
#pragma unroll
        for (int u = 0; u < PER_T; u++) {
            const uint32_t b = t + (uint32_t)u * MSM_P1_THREADS;
            const uint32_t cnt = start[b + 1] - start[b];
            got[u] = cnt ? atomicAdd(&cursor[b * ncls + cls], cnt) : 0u;
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < MSM_P1_MAXW; q++)
                if (win_lo + q < win_hi) {
                    const uint32_t at = start[(key[q] >> low)] + rank[q];
                    stage_k[at] = key[q];
                    stage_v[at] = val[q];
                }
        }
        // the next tile's scalars: requested now, needed after the write phase
        i += (uint64_t)gridDim.x * tile_scalars;
        live = tile + gridDim.x < ntiles && t < tile_scalars && i < n;
        if (live) raw = load_fe<FrP>(scalars + i * 8);
#pragma unroll
        for (int u = 0; u < PER_T; u++) {
            const uint32_t b = t + (uint32_t)u * MSM_P1_THREADS;
            delta[b] = got[u] - start[b];   // (bins without pairs: never looked up)
        }
        __syncthreads();
        for (uint32_t p = t; p < total; p += blockDim.x) {   // consecutive lanes write consecutive addresses inside a run
            const uint32_t k = stage_k[p];
            const uint32_t dst = p + delta[(k >> low)];
            out_keys[dst] = (uint16_t)(k & ((1u << low) - 1));   // the second level knows the group from its segment: only the part it counts travels
            out_vals[dst] = stage_v[p];
        }
        __syncthreads();   // (the staging arrays and the bin tables are rewritten by the next tile)
    }
}

// ---- 1c. the second level of the fused sort, in place of the library pass and the binary-search offsets ------------------------
// After the first pass the pairs are grouped; inside a group a pair's final place is off[key] + (any rank among the pairs with the
// same key): no stability is needed, only the per-key counts.  Segments of at most MSM_P2_SEG pairs of ONE group count their key
// parts in LDS and add them to a global per-key histogram (gcount[key]); an exclusive scan of that histogram IS the bucket-offset
// array `off`; then the same segments reserve one run per (segment, key) behind a global atomic and write the VALUES (the sorted
// keys are never materialised), LDS-staged so that a run leaves the CU as consecutive addresses.  Any key distribution works (a
// group of any size is just more segments).
// Measured at 12 x 2^24 pairs (tools/exp/partbench.hip variant C): 1.41 ms against the library pass + offsets kernel's 2.0 ms.
// swz: consecutive segments -- the segments of one group, whose runs are neighbours in the output when the groups are key ranges --
// go to ONE XCD (block b runs on XCD b % 8: it takes segment (b % 8) * ceil(S / 8) + b / 8 of the S the device counted), so that the
// partial lines they write meet in one L2.  Placement is a speed assumption only.
template <int BITS>
__device__ __forceinline__ bool msm_p2_segment(const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ bin_off, int swz, uint32_t& bin,
                                               uint32_t& lo, uint32_t& hi) {
    constexpr uint32_t BINS = 1u << BITS;
    const uint32_t nseg = seg_off[BINS];
    uint32_t sidx = blockIdx.x;
    if (swz) {
        const uint32_t per = (nseg + MSM_XCDS - 1) / MSM_XCDS, j = blockIdx.x / MSM_XCDS;
        if (j >= per) return false;
        sidx = (blockIdx.x % MSM_XCDS) * per + j;
    }
    if (sidx >= nseg) return false;
    uint32_t l = 0, r = BINS;   // the last bin with seg_off[bin] <= sidx
    while (r - l > 1) {
        const uint32_t mid = (l + r) >> 1;
        if (seg_off[mid] <= sidx) l = mid;
        else r = mid;
    }
    bin = l;
    lo = bin_off[bin] + (sidx - seg_off[bin]) * MSM_P2_SEG;
    hi = bin_off[bin + 1];
    if (hi - lo > MSM_P2_SEG) hi = lo + MSM_P2_SEG;
    return true;
}
template <int BITS>
static __global__ void __launch_bounds__(1024)
msm_p2_count_kernel(const uint16_t* __restrict__ keys, const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ bin_off,
                    uint32_t hb, int low, int swz, uint32_t* __restrict__ gcount) {
    __shared__ uint32_t cnt[MSM_P2_HB];
    uint32_t bin, lo, hi;
    if (!msm_p2_segment<BITS>(seg_off, bin_off, swz, bin, lo, hi)) return;   // (uniform per block)
    for (uint32_t h = threadIdx.x; h < hb; h += blockDim.x) cnt[h] = 0;
    __syncthreads();
    constexpr int U = MSM_P2_SEG / 1024;
    uint32_t kk[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t p = lo + u * 1024 + threadIdx.x;
        kk[u] = p < hi ? (uint32_t)keys[p] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (kk[u] != 0xFFFFFFFFu) atomicAdd(&cnt[kk[u]], 1u);
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < hb; h += blockDim.x)
        if (cnt[h]) atomicAdd(&gcount[(bin << low) | h], cnt[h]);
}
template <int BITS>
static __global__ void __launch_bounds__(1024)
msm_p2_scatter_kernel(const uint16_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ seg_off,
                      const uint32_t* __restrict__ bin_off, uint32_t hb, int low, int swz, uint32_t* __restrict__ cursor,
                      uint32_t* __restrict__ out_vals) {
    __shared__ uint32_t stage_v[MSM_P2_SEG];
    __shared__ uint16_t stage_h[MSM_P2_SEG];
    __shared__ uint32_t start[MSM_P2_HB + 1], delta[MSM_P2_HB], wtot[16];
    uint32_t bin, lo, hi;
    if (!msm_p2_segment<BITS>(seg_off, bin_off, swz, bin, lo, hi)) return;
    const uint32_t t = threadIdx.x;
    for (uint32_t h = t; h < hb; h += blockDim.x) start[h] = 0;
    __syncthreads();
    constexpr int U = MSM_P2_SEG / 1024;
    uint32_t kk[U], vv[U], rk[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t p = lo + u * 1024 + t;
        kk[u] = p < hi ? (uint32_t)keys[p] : 0xFFFFFFFFu;
        vv[u] = p < hi ? vals[p] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (kk[u] != 0xFFFFFFFFu) rk[u] = atomicAdd(&start[kk[u]], 1u);
    __syncthreads();
    msm_block_excl_scan_1024(start, hb, wtot);
    // (as in the first level: all of a thread's run reservations are issued before any result is used; no measurable change here,
    // 0.94-0.97 -> 0.94-0.95 ms)
    constexpr int PER_T = 4;   // hb <= 4096 key parts, 1024 threads
    uint32_t got[PER_T];
#pragma unroll
    for (int u = 0; u < PER_T; u++) {
        const uint32_t h = t + (uint32_t)u * 1024u;
        got[u] = 0;
        if (h < hb) {
            const uint32_t cnt = start[h + 1] - start[h];
            if (cnt) got[u] = atomicAdd(&cursor[(bin << low) | h], cnt);
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (kk[u] != 0xFFFFFFFFu) {
            const uint32_t h = kk[u], at = start[h] + rk[u];
            stage_v[at] = vv[u];
            stage_h[at] = (uint16_t)h;
        }
#pragma unroll
    for (int u = 0; u < PER_T; u++) {
        const uint32_t h = t + (uint32_t)u * 1024u;
        if (h < hb) delta[h] = got[u] - start[h];
    }
    __syncthreads();
    const uint32_t total = hi - lo;
    for (uint32_t p = t; p < total; p += blockDim.x) out_vals[p + delta[stage_h[p]]] = stage_v[p];
}

// ---- host: the sort stage ---------------------------------------------------------------------------------------------------
// The scalar input of an MSM: one vector of n scalars, or (batch > 1, table mode only) a host array of `batch` device pointers, one
// scalar vector each, over the SAME table.
struct MsmScalars {
    const void* d;
    size_t n;
    bool mont;
    int batch;
    const uint32_t* vec(int b) const { return batch == 1 ? (const uint32_t*)d : reinterpret_cast<const uint32_t* const*>(d)[b]; }
};

// The fused sort of the scalar vectors' (key, value) pairs, P = the plan of the call (msm_plan_prepare): on return `off` holds the
// bucket offsets (nb + 2 entries) and vals2 the values grouped by key.  keys / vals: the first level's output (scratch).
template <class FrP, int BITS>
int msm_fused_sort(Ctx* ctx, const std::string& sfx, hipStream_t st, const MsmScalars& S, const MsmPrepared& P, uint16_t* keys, uint32_t* vals,
                   uint32_t* vals2, uint32_t* off) {
    // xcd (GA_MSM_XCD, A/B knob): bit 0 per-XCD slices in the first level, bit 1 XCD swizzle of the second level's segments, bit 2
    // the slices at any size (tests)
    const int xcd = ctx->tun.msm_xcd.load(std::memory_order_relaxed);
    constexpr uint32_t BINS = 1u << BITS;
    auto key = [&](const char* k) { return std::string(k) + sfx; };
    const uint64_t n = S.n, m = P.m;
    const int mont = S.mont ? 1 : 0, c = P.c, nwin = P.nwin, win_lo = P.win_lo, win_hi = P.win_hi, table = P.table ? 1 : 0;
    const uint32_t half = P.half, nb = P.nb;
    const int nwl = win_hi - win_lo;
    const int low = msm_key_low(nb, BITS);
    // (per-XCD slices make the histogram and cursor tables 8 x as long: below 2^24 pairs they cost what they save,
    // profiles/r05_b_fuse_min_sweep.txt)
    const uint32_t ncls = ((xcd & 1) && (m >= (1ull << 24) || (xcd & 4))) ? MSM_XCDS : 1;
    const int swz = (xcd & 2) ? 1 : 0;
    uint32_t *ghist, *cursor, *bin_off, *seg_off, *gcount, *kcursor;
    GA_CHECK(ctx->scratch_get(key("msm_p1_hist").c_str(), BINS * MSM_XCDS * 4, (void**)&ghist));
    GA_CHECK(ctx->scratch_get(key("msm_p1_cursor").c_str(), BINS * MSM_XCDS * 4, (void**)&cursor));
    GA_CHECK(ctx->scratch_get(key("msm_p1_bin_off").c_str(), (BINS + 1) * 4, (void**)&bin_off));
    GA_CHECK(ctx->scratch_get(key("msm_p2_seg_off").c_str(), (BINS + 1) * 4, (void**)&seg_off));
    // the key parts the second level counts, and every key a (group, part) pair can form (>= nb + 1)
    const uint32_t hb = 1u << low;   // <= 4096 (msm_fused_fits): msm_p2_scatter_kernel reserves four runs per thread
    const uint64_t nkeys = (((uint64_t)nb >> low) + 1) << low;
    GA_CHECK(ctx->scratch_get(key("msm_p2_count").c_str(), nkeys * 4, (void**)&gcount));
    GA_CHECK(ctx->scratch_get(key("msm_p2_cursor").c_str(), nkeys * 4, (void**)&kcursor));
    {
        StageTimer tm(ctx, "msm_digits_pass1", st);
        const uint32_t tile = msm_p1_tile_scalars(nwl);
        const uint64_t ntiles = (n + tile - 1) / tile;
        uint64_t hist_blocks = (ntiles + MSM_XCDS - 1) / MSM_XCDS * MSM_XCDS;   // a multiple of 8: tile t and the block that counts it agree on t % 8
        if (hist_blocks > 2048) hist_blocks = 2048;
        const uint64_t p1_grid = ctx->tun.msm_p1_grid.load(std::memory_order_relaxed);   // GA_MSM_P1_GRID (A/B knob; tests)
        uint64_t p1_blocks = ntiles <= p1_grid ? ntiles : p1_grid;
        if (ncls > 1 && p1_blocks < ntiles) p1_blocks = (p1_blocks + MSM_XCDS - 1) / MSM_XCDS * MSM_XCDS;   // a block's tiles must share t % 8 (the histogram's classes)
        GA_HIP_CHECK(hipMemsetAsync(ghist, 0, BINS * ncls * 4, st));
        for (int b = 0; b < S.batch; b++)   // (a batch: the vectors' bucket sets are stacked in ONE key space, key_base = b * 2^(c-1))
            hipLaunchKernelGGL((msm_digit_hist_kernel<FrP, BITS>), dim3((unsigned)hist_blocks), dim3(256), 0, st, S.vec(b), n, mont, c, nwin,
                               win_lo, win_hi, table, (uint32_t)b * half, nb, tile, low, ncls, ghist);
        hipLaunchKernelGGL(msm_p1_scan_kernel<BITS>, dim3(1), dim3(1024), 0, st, (const uint32_t*)ghist, ncls, cursor, bin_off, seg_off);
        for (int b = 0; b < S.batch; b++)
            hipLaunchKernelGGL((msm_digits_pass1_kernel<FrP, BITS>), dim3((unsigned)p1_blocks), dim3(MSM_P1_THREADS), 0, st, S.vec(b), n, mont,
                               c, nwin, win_lo, win_hi, table, (uint32_t)b * half, nb, tile, ntiles, low, ncls, cursor, keys, vals);
        GA_KERNEL_CHECK();
    }
    {
        StageTimer tm(ctx, "msm_sort", st);
        unsigned max_seg = (unsigned)(m / MSM_P2_SEG + BINS);
        if (swz) max_seg = (max_seg + MSM_XCDS - 1) / MSM_XCDS * MSM_XCDS + MSM_XCDS;   // ceil(S / 8) blocks per XCD for any S <= max_seg
        GA_HIP_CHECK(hipMemsetAsync(gcount, 0, nkeys * 4, st));
        hipLaunchKernelGGL(msm_p2_count_kernel<BITS>, dim3(max_seg), dim3(1024), 0, st, (const uint16_t*)keys, (const uint32_t*)seg_off,
                           (const uint32_t*)bin_off, hb, low, swz, gcount);
        GA_KERNEL_CHECK();
        size_t sb = 0;
        void* stmp;
        GA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, sb, gcount, off, (int)(nb + 1), st));
        GA_CHECK(ctx->scratch_get(key("msm_p2_scan_tmp").c_str(), sb + 256, &stmp));
        GA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(stmp, sb, gcount, off, (int)(nb + 1), st));   // off[b], b = 0..nb (nb = SKIP)
        GA_HIP_CHECK(hipMemcpyAsync(kcursor, off, ((uint64_t)nb + 1) * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(msm_p2_scatter_kernel<BITS>, dim3(max_seg), dim3(1024), 0, st, (const uint16_t*)keys, (const uint32_t*)vals,
                           (const uint32_t*)seg_off, (const uint32_t*)bin_off, hb, low, swz, kcursor, vals2);
        GA_KERNEL_CHECK();
    }
    return GA_OK;
}

// Stages 1 and 2 of the call planned in P: the pairs of the scalars S, grouped by key, in P->vals.  *off: the bucket-offset array
// (nb + 2 entries).  The fused sort fills it itself and leaves *sorted_keys null; after the library sort *sorted_keys holds the keys
// from which the task stage finds the offsets (msm_offsets_tasks_kernel).
template <class FrP>
int msm_sort(Ctx* ctx, const std::string& sfx, hipStream_t st, const MsmScalars& S, int end_bit, MsmPrepared* P, uint32_t** off,
             const uint32_t** sorted_keys) {
    auto key = [&](const char* k) { return std::string(k) + sfx; };
    const uint64_t m = P->m;
    const int nwl = P->win_hi - P->win_lo;
    uint32_t *keys = nullptr, *keys2 = nullptr, *vals, *vals2;
    GA_CHECK(ctx->scratch_get(key("msm_vals2").c_str(), m * 4, (void**)&vals2));
    GA_CHECK(ctx->scratch_get(key("msm_off").c_str(), ((uint64_t)P->nb + 2) * 4, (void**)off));
    // digits fused with the first sort pass (1b / 1c): key spaces of 2^11 .. 2^24 keys, at most MSM_P1_MAXW windows per scalar, any
    // number of scalar vectors over one table, enough pairs for the saved traffic to matter (GA_MSM_FUSE_MIN)
    const bool fused = msm_fused_fits(P->nb) && nwl <= MSM_P1_MAXW && m >= ctx->tun.msm_fuse_min.load(std::memory_order_relaxed);
    // Scratch of the sort.  Fused: key parts (16 bits) / vals are the first level's output, dead once the second level has run, and
    // the sorted keys are never materialised -- so the two sort slots of a lane SHARE them (stream order separates their uses) and
    // there is no keys2: 14 bytes per pair less per extra slot.  Library sort: ping-pong pairs, the result may live in either.
    // INVARIANT behind the sharing: scratch names are per LANE (Ctx::scratch_get appends "@lane") and a lane has exactly one work
    // stream, so both slots issue on the same stream; a buffer that has to grow is released with hipFree, which waits for the device.
    // A slot prepared on any other stream, or an asynchronous free (hipFreeAsync, a pool), would let one slot's first level overwrite
    // pairs the other slot's second level has not read yet: key these two buffers by stream before doing either.
    if (fused) {
        uint16_t* key_parts;   // what the first level hands to the second per pair besides the value -- the <= 12 low key bits
        GA_CHECK(ctx->scratch_get("msm_keys_level1", m * 2, (void**)&key_parts));
        GA_CHECK(ctx->scratch_get("msm_vals_level1", m * 4, (void**)&vals));
        const auto sort = msm_p1_bits(P->nb) == 11 ? &msm_fused_sort<FrP, 11> : &msm_fused_sort<FrP, 12>;
        GA_CHECK(sort(ctx, sfx, st, S, *P, key_parts, vals, vals2, *off));
    } else {
        GA_CHECK(ctx->scratch_get(key("msm_keys").c_str(), m * 4, (void**)&keys));
        GA_CHECK(ctx->scratch_get(key("msm_vals").c_str(), m * 4, (void**)&vals));
        GA_CHECK(ctx->scratch_get(key("msm_keys2").c_str(), m * 4, (void**)&keys2));
        {
            StageTimer tm(ctx, "msm_digits", st);
            const uint64_t per_vec = (uint64_t)nwl * S.n;
            for (int b = 0; b < S.batch; b++)
                hipLaunchKernelGGL((msm_digits_kernel<FrP>), dim3((unsigned)((S.n + 255) / 256)), dim3(256), 0, st, S.vec(b), (uint64_t)S.n,
                                   S.mont ? 1 : 0, P->c, P->nwin, P->win_lo, P->win_hi, P->table ? 1 : 0, (uint32_t)b * P->half, P->nb,
                                   keys + b * per_vec, vals + b * per_vec);
            GA_KERNEL_CHECK();
        }
        StageTimer tm(ctx, "msm_sort", st);
        GA_CHECK(msm_sort_pairs(ctx, key("msm_sort_tmp"), keys, keys2, vals, vals2, (size_t)m, end_bit, st));
    }
    P->vals = vals2;
    *sorted_keys = keys2;
    return GA_OK;
}

}  // namespace ga
