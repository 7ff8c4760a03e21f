// The host half of the quotient's evaluation form (masp_amd/csrc/host/eval_form.h) on its own: the column-compressed copy of C and the
// layout of Circuit::hl_eval.  Built with the address and undefined-behaviour sanitizers and run by tests/test_eval_form_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/eval_form.h"

using namespace masp;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

struct Csr {
    std::vector<uint32_t> rowptr{0}, col;
    std::vector<uint8_t> coef;
    void row(std::initializer_list<std::pair<uint32_t, uint8_t>> terms) {
        for (auto& t : terms) {
            col.push_back(t.first);
            std::vector<uint8_t> c(32, 0);
            c[0] = t.second;
            c[31] = (uint8_t)col.size();   // (every entry distinguishable)
            coef.insert(coef.end(), c.begin(), c.end());
        }
        rowptr.push_back((uint32_t)col.size());
    }
};

static int test_csc() {
    // 3 inputs (0 = ONE), 4 aux; 5 rows
    Csr m;
    m.row({{3, 1}, {0, 2}});
    m.row({});
    m.row({{6, 5}, {3, 7}});
    m.row({{0, 9}});
    m.row({{4, 1}});
    CscMatrix c;
    CHECK(csc_from_csr(5, 7, m.rowptr.data(), m.col.data(), m.coef.data(), c));
    const std::vector<uint32_t> want_ptr = {0, 2, 2, 2, 4, 5, 5, 6};
    CHECK(c.colptr == want_ptr);
    const std::vector<uint32_t> want_rows = {0, 3, 0, 2, 4, 2};
    CHECK(c.rowidx == want_rows);
    const uint8_t want_coef[6] = {2, 9, 1, 7, 1, 5}, want_tag[6] = {2, 5, 1, 4, 6, 3};
    for (int t = 0; t < 6; ++t) CHECK(c.coef[32 * t] == want_coef[t] && c.coef[32 * t + 31] == want_tag[t]);
    CHECK(c.len(0) == 2 && c.len(1) == 0 && c.len(3) == 2 && c.len(6) == 1);
    // a column index out of range is refused, not written
    CHECK(!csc_from_csr(5, 6, m.rowptr.data(), m.col.data(), m.coef.data(), c));
    // an empty matrix
    Csr e;
    for (int i = 0; i < 3; ++i) e.row({});
    CHECK(csc_from_csr(3, 4, e.rowptr.data(), e.col.data(), e.coef.data(), c));
    CHECK(c.colptr == std::vector<uint32_t>(5, 0) && c.rowidx.empty() && c.coef.empty());
    // the layout over the first matrix: inputs 0 used, 1 and 2 not
    CHECK(csc_from_csr(5, 7, m.rowptr.data(), m.col.data(), m.coef.data(), c));
    const EvalLayout L = eval_layout(c, 3, 4, 8);
    CHECK(L.used_inputs == std::vector<uint32_t>{0});
    CHECK(L.aux_off() == 8 && L.in_off() == 12 && L.n() == 13 && L.n_slots() == 5);
    CHECK(L.slot_col(0) == 3 && L.slot_col(3) == 6 && L.slot_col(4) == 0);
    CHECK(L.long_slots.empty());
    printf("csc ok\n");
    return 0;
}

static int test_layout_long_columns() {
    // the constant-one input in every row (a long column), one aux column exactly at the threshold, one just below; no input but ONE is used
    const uint32_t n_in = 4, n_aux = 70, rows = 200, LONG = EvalLayout::LONG_COL;
    Csr m;
    for (uint32_t r = 0; r < rows; ++r) {
        if (r < LONG)
            m.row({{0, 1}, {n_in + 5, 1}, {n_in + 69, 1}});
        else if (r == LONG)
            m.row({{0, 1}, {n_in + 5, 1}});
        else
            m.row({{0, 1}});
    }
    CscMatrix c;
    CHECK(csc_from_csr(rows, n_in + n_aux, m.rowptr.data(), m.col.data(), m.coef.data(), c));
    CHECK(c.len(0) == rows && c.len(n_in + 5) == LONG + 1 && c.len(n_in + 69) == LONG);
    for (uint32_t v = 0; v < n_in + n_aux; ++v)
        for (uint32_t t = c.colptr[v]; t + 1 < c.colptr[v + 1]; ++t) CHECK(c.rowidx[t] < c.rowidx[t + 1]);   // rows ascending
    const size_t mm = 256;
    const EvalLayout L = eval_layout(c, n_in, n_aux, mm);
    CHECK(L.used_inputs == std::vector<uint32_t>{0});
    CHECK(L.aux_off() == mm && L.aux_off() % 64 == 0 && L.in_off() == mm + n_aux && L.n() == mm + n_aux + 1);
    const std::vector<uint32_t> want_long = {5, 69, 70};   // slots: aux 5, aux 69, then the used input behind the n_aux aux slots
    CHECK(L.long_slots == want_long);
    CHECK(L.slot_col(70) == 0 && L.slot_col(69) == n_in + 69);
    // every slot's point lies inside the table, every column is named once
    std::vector<int> seen(n_in + n_aux, 0);
    for (uint32_t o = 0; o < L.n_slots(); ++o) {
        CHECK(L.aux_off() + o < L.n());
        ++seen[L.slot_col(o)];
    }
    for (uint32_t v = 0; v < n_in + n_aux; ++v) CHECK(seen[v] == (v >= n_in || v == 0 ? 1 : 0));
    // no input used at all, no aux
    Csr z;
    z.row({});
    CHECK(csc_from_csr(1, 2, z.rowptr.data(), z.col.data(), z.coef.data(), c));
    const EvalLayout Z = eval_layout(c, 2, 0, 2);
    CHECK(Z.used_inputs.empty() && Z.n_slots() == 0 && Z.n() == 2 && Z.in_off() == 2);
    printf("layout ok\n");
    return 0;
}

int main() {
    if (test_csc() || test_layout_long_columns()) return 1;
    printf("all ok\n");
    return 0;
}
