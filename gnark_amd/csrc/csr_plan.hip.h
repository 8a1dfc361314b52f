// The CSR row planner of the two sparse calls (sparse_sums.hip.h over points, fr_sparse.hip.h over Fr): the validation of row_start
// and of the {cid, col} terms, and the cutting of rows into levels of segments of at most S operands.  Host code, apart from the one
// constant the kernels of both calls read in a segment's destination.
#pragma once
#include <vector>

#include "common.hip.h"

namespace ga {

constexpr uint32_t SPARSE_FINAL = 1u << 31;   // segment destination: the row's sum (else a partial sum of the next level)

struct CsrLevels {
    std::vector<uint32_t> segs;    // 3 words per segment {first operand, operands, destination}, level after level
    struct Level {
        uint64_t first;            // its first segment in `segs`
        uint32_t nseg, nparts;     // segments; partial sums it writes
    };
    std::vector<Level> levels;
    // the partial sums ping-pong between two buffers: level l writes parts[l & 1] and level l + 1 reads it
    void part_sizes(uint64_t parts[2]) const {
        parts[0] = parts[1] = 0;
        for (size_t l = 0; l < levels.size(); l++)
            if (levels[l].nparts > parts[l & 1]) parts[l & 1] = levels[l].nparts;
    }
};

// nothing has been written when it fails; `entry` prefixes the message, `noun` names what a col indexes ("points", "columns")
inline int csr_validate(const char* entry, const char* noun, size_t n_cols, const uint64_t* row_start, size_t n_rows, const uint32_t* terms, size_t n_coeffs) {
    if (row_start[0] != 0) {
        set_error("%s: row_start[0] = %llu, not 0", entry, (unsigned long long)row_start[0]);
        return GA_ERR_INVALID;
    }
    for (size_t r = 0; r < n_rows; r++)
        if (row_start[r + 1] < row_start[r]) {
            set_error("%s: row_start decreases at row %zu (%llu after %llu)", entry, r, (unsigned long long)row_start[r + 1], (unsigned long long)row_start[r]);
            return GA_ERR_INVALID;
        }
    const uint64_t nnz = row_start[n_rows];
    if (nnz >= (1ull << 32)) {
        set_error("%s: row_start[n_rows] = %llu terms, at most 2^32 - 1 per call", entry, (unsigned long long)nnz);
        return GA_ERR_INVALID;
    }
    for (uint64_t k = 0; k < nnz; k++)
        if (terms[2 * k] >= n_coeffs || terms[2 * k + 1] >= n_cols) {
            set_error("%s: term %llu = {cid %u, col %u} outside %zu coefficients, %zu %s", entry, (unsigned long long)k, terms[2 * k], terms[2 * k + 1], n_coeffs,
                      n_cols, noun);
            return GA_ERR_INVALID;
        }
    return GA_OK;
}

// level 0: every row, a row of at most S terms straight to its sum; the levels after it: the rows that are still more than one partial sum
inline void csr_cut_levels(const uint64_t* row_start, size_t n_rows, uint32_t S, CsrLevels& out) {
    struct Long {
        uint32_t row;
        uint64_t first, count;
    };
    std::vector<Long> rows, longer;
    auto cut = [&](uint32_t row, uint64_t first, uint64_t count, uint32_t& nparts) {
        if (count <= S) {
            out.segs.insert(out.segs.end(), {(uint32_t)first, (uint32_t)count, SPARSE_FINAL | row});
            return;
        }
        longer.push_back({row, nparts, (count + S - 1) / S});
        for (uint64_t o = 0; o < count; o += S) out.segs.insert(out.segs.end(), {(uint32_t)(first + o), (uint32_t)(count - o < S ? count - o : S), nparts++});
    };
    {
        CsrLevels::Level lv{0, 0, 0};
        for (size_t r = 0; r < n_rows; r++) cut((uint32_t)r, row_start[r], row_start[r + 1] - row_start[r], lv.nparts);
        lv.nseg = (uint32_t)(out.segs.size() / 3);
        out.levels.push_back(lv);
    }
    while (!longer.empty()) {
        rows.swap(longer);
        longer.clear();
        CsrLevels::Level lv{out.segs.size() / 3, 0, 0};
        for (const Long& w : rows) cut(w.row, w.first, w.count, lv.nparts);
        lv.nseg = (uint32_t)(out.segs.size() / 3 - lv.first);
        out.levels.push_back(lv);
    }
}

}  // namespace ga
