// Host half of the quotient's evaluation form: the column-compressed copy of the R1CS matrix C that the loader's sparse
// combine walks, and the layout of the merged base set Circuit::hl_eval.  Plain C++, no HIP: tests/native/eval_form_host.cpp compiles it
// on its own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace masp {

// a CSR matrix (rowptr: n_rows + 1, col / coef: nnz; coef 32 bytes each) by columns: the entries of column v are
// rowidx / coef [colptr[v], colptr[v + 1]), rows ascending
struct CscMatrix {
    std::vector<uint32_t> colptr, rowidx;
    std::vector<uint8_t> coef;  // 32 bytes per entry, as they came
    uint32_t len(uint32_t v) const { return colptr[v + 1] - colptr[v]; }
};
// false: a column index is >= n_cols (nothing usable in `out` then)
static inline bool csc_from_csr(uint32_t n_rows, uint32_t n_cols, const uint32_t* rowptr, const uint32_t* col, const uint8_t* coef, CscMatrix& out) {
    const uint32_t nnz = rowptr[n_rows];
    out.colptr.assign((size_t)n_cols + 1, 0);
    out.rowidx.assign(nnz, 0);
    out.coef.assign((size_t)32 * nnz, 0);
    for (uint32_t t = 0; t < nnz; ++t) {
        if (col[t] >= n_cols) return false;
        ++out.colptr[col[t] + 1];
    }
    for (uint32_t v = 0; v < n_cols; ++v) out.colptr[v + 1] += out.colptr[v];
    std::vector<uint32_t> fill(out.colptr.begin(), out.colptr.end() - 1);
    for (uint32_t row = 0; row < n_rows; ++row)
        for (uint32_t t = rowptr[row]; t < rowptr[row + 1]; ++t) {
            const uint32_t pos = fill[col[t]]++;
            out.rowidx[pos] = row;
            memcpy(&out.coef[(size_t)32 * pos], coef + (size_t)32 * t, 32);
        }
    return true;
}

// Circuit::hl_eval, point by point: [0, m) the transformed h query T' in the order the forward passes leave the coset evaluations,
// [m, m + n_aux) the folded l query L' (m is a power of two: the subset-row blocks start aligned), then one base per INPUT column
// that C touches (`used_inputs`, ascending; an input C never names gets none).  The scalars of a proof follow the same layout.
struct EvalLayout {
    size_t m = 0;
    uint32_t n_inputs = 0, n_aux = 0;
    std::vector<uint32_t> used_inputs;
    std::vector<uint32_t> long_slots;  // derived slots (see slot_col) whose C column has >= LONG_COL entries: summed by a wave each
    static constexpr uint32_t LONG_COL = 64;
    size_t aux_off() const { return m; }
    size_t in_off() const { return m + n_aux; }
    size_t n() const { return m + n_aux + used_inputs.size(); }
    // the derived (non-T') bases are numbered aux first, then the used inputs: slot o sits at point m + o
    uint32_t n_slots() const { return n_aux + (uint32_t)used_inputs.size(); }
    uint32_t slot_col(uint32_t o) const { return o < n_aux ? n_inputs + o : used_inputs[o - n_aux]; }
};
static inline EvalLayout eval_layout(const CscMatrix& c, uint32_t n_inputs, uint32_t n_aux, size_t m) {
    EvalLayout L;
    L.m = m;
    L.n_inputs = n_inputs;
    L.n_aux = n_aux;
    for (uint32_t v = 0; v < n_inputs; ++v)
        if (c.len(v)) L.used_inputs.push_back(v);
    for (uint32_t o = 0; o < L.n_slots(); ++o)
        if (c.len(L.slot_col(o)) >= EvalLayout::LONG_COL) L.long_slots.push_back(o);
    return L;
}

}  // namespace masp
