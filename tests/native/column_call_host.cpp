// The per-item wallet calls' layout, driver and ending (masp_amd/csrc/column_call.h) on the CPU: plain arrays stand in for device and
// pinned memory, the device policy copies between them and records every operation, and a fake launch derives every result byte of an
// item from the item's uploaded bytes.  Every buffer is a heap array of exactly the size the layout asks for, the callers' arrays hold
// exactly n items, and an absent array is a null pointer: the address sanitizer is the witness that nothing beyond them is touched.
// One case per line of the output (tests/test_column_call_host.py reads them):
//
//     chunk <configured> <by default> <n> -> <cap> <n_pad>
//     layout <n_pad> <in|out|stage> <total bytes> : <offset>/<width> ...
//     run <secrets> <n> <cap> <fail> -> rc <rc> match <0|1> refused <items> rezeroed <items> ms <a> <b> <c> : <ops> | <ending's ops> | <in> <state> <stage>
//
// <fail>: "none" or <kind><k>@<chunk>: the k-th operation of that kind in that chunk returns 40 + chunk (kinds as in the ops).  <ops>:
// M<k> mark, H<col>:<bytes>@<item> upload from the caller's array at that item (@s<item>: from the column's stage, which holds the
// caller's bytes from that item on; s-1 if it does not), Z<bytes> zero, L<c> launch, D<col>:<bytes>@<item> download, F finish, X drain.
// match: the caller's result arrays equal what the inputs give for every item of a finished chunk, zeros for a refused item, and behind
// a call that succeeded nothing else was written; refused: such items; rezeroed: those of them whose result slots held an accepted
// item's bytes the chunk before.  The last three: whether in, state and stage (-1: none) are all zero after the ending.
#include "column_call.h"

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

using namespace masp;

constexpr ColumnWidths IN_SECRET{{32, 8, 11, 1, 80}, 0b11}, IN_PLAIN{32, 8, 11, 1, 80}, OUT{32, 8, 11, 80, 1};
constexpr size_t STATE = 24;
constexpr int ABSENT_IN = 2, ABSENT_OUT = 1;
static_assert(IN_SECRET.total == 132 && IN_SECRET.stage_total == 40 && IN_PLAIN.stage_total == 0 && OUT.total == 132 && OUT.off[4] == 131, "the layout's sums");

struct Buf {
    std::unique_ptr<uint8_t[]> own;
    uint8_t* p = nullptr;
    size_t cap = 0;
    void reserve(size_t n) {
        own.reset(new uint8_t[n]);
        p = n ? own.get() : nullptr;
        cap = n;
        std::fill(own.get(), own.get() + n, 0xA5);
    }
    bool zero() const { return std::all_of(p, p + cap, [](uint8_t b) { return b == 0; }); }
};
struct Bufs {
    Buf in, state, out, stage;
};

static bool refused(uint8_t first) { return first % 3 == 0; }
// result byte b of column j for an item whose uploaded bytes sum to `sum`: never zero
static uint8_t result(unsigned sum, int j, size_t b) { return (uint8_t)((sum + 31 * j + 7 * b) | 0x80); }

struct Fail {
    char kind = 0;
    int k = 0, chunk = 0;
};

struct Dev {
    const ColumnCall* cc = nullptr;
    Fail fail;
    std::string ops;
    int chunk = 0, seen[128] = {};
    int op(char kind, const std::string& text) {
        ops += " " + std::string(1, kind) + text;
        return kind == fail.kind && chunk == fail.chunk && seen[(int)kind]++ == fail.k ? 40 + chunk : 0;
    }
    int h2d(void* d, const void* h, size_t bytes) {
        int k = 0;
        while (cc->ins[k].dev != d) ++k;
        const ColumnCall::Column& x = cc->ins[k];
        const bool staged = h == x.stage;
        memcpy(d, h, bytes);
        const long item = staged ? (memcmp(h, x.src + x.width * done, bytes) ? -1 : (long)done) : (long)(((const uint8_t*)h - x.src) / x.width);
        return op('H', std::to_string(k) + ":" + std::to_string(bytes) + "@" + (staged ? "s" : "") + std::to_string(item));
    }
    int d2h(void* h, const void* d, size_t bytes) {
        int k = 0;
        while (cc->outs[k].dev != d) ++k;
        memcpy(h, d, bytes);
        return op('D', std::to_string(k) + ":" + std::to_string(bytes) + "@" + std::to_string(((uint8_t*)h - cc->outs[k].dst) / cc->outs[k].width));
    }
    int zero(void* d, size_t bytes) {
        memset(d, 0, bytes);
        return op('Z', std::to_string(bytes));
    }
    int mark(int k) { return op('M', std::to_string(k)); }
    int drain() { return op('X', ""); }
    int finish(double* ms) {
        const int rc = op('F', "");
        if (rc) return rc;
        for (int k = 0; k < 3; ++k) ms[k] += (k + 1) * (chunk + 1) * 0.25;
        done += cc->cap;
        ++chunk;
        std::fill(seen, seen + 128, 0);
        return 0;
    }
    size_t done = 0;   // items of the chunks finished
};

static void run(const ColumnWidths& iw, size_t n, size_t cap, Fail fail) {
    // the caller's arrays: exactly n items each
    std::vector<std::vector<uint8_t>> src(iw.n), dst(OUT.n);
    for (int k = 0; k < iw.n; ++k) {
        src[k].resize(iw.width[k] * n);
        for (size_t b = 0; b < src[k].size(); ++b) src[k][b] = (uint8_t)(b * 37 + k * 11 + b / 251);
    }
    for (int j = 0; j < OUT.n; ++j) dst[j].assign(OUT.width[j] * n, 0xEE);
    ColumnCall cc(iw, OUT, cap);
    Bufs bufs;
    bufs.in.reserve(iw.total * cc.n_pad);
    bufs.state.reserve(STATE * cc.n_pad);
    bufs.out.reserve(OUT.total * cc.n_pad);
    bufs.stage.reserve(iw.stage_total * cc.n_pad);
    cc.d_in = bufs.in.p, cc.d_out = bufs.out.p, cc.stage = bufs.stage.p;
    const uint8_t* d_in[5];
    uint8_t* d_out[5];
    for (int k = 0; k < iw.n; ++k) d_in[k] = cc.in(k == ABSENT_IN ? nullptr : src[k].data());
    for (int j = 0; j < OUT.n; ++j) d_out[j] = cc.out(j == ABSENT_OUT ? nullptr : dst[j].data());
    Dev dev;
    dev.cc = &cc, dev.fail = fail;
    size_t rezeroed = 0;
    std::vector<uint8_t> accepted_before(cc.n_pad, 0);
    auto launch = [&](size_t c) {
        dev.ops += " L" + std::to_string(c);
        for (size_t i = 0; i < c; ++i) {
            unsigned sum = 0;
            for (int k = 0; k < iw.n; ++k)
                for (size_t b = 0; d_in[k] && b < iw.width[k]; ++b) sum += d_in[k][iw.width[k] * i + b];
            const bool no = refused(d_in[0][32 * i]);
            d_out[OUT.n - 1][i] = no ? 9 : 0;
            memset(bufs.state.p + STATE * i, 0x5A, STATE);
            rezeroed += no && accepted_before[i];
            accepted_before[i] = !no;
            for (int j = 0; !no && j + 1 < OUT.n; ++j)
                for (size_t b = 0; b < OUT.width[j]; ++b) d_out[j][OUT.width[j] * i + b] = result(sum, j, b);
        }
    };
    double ms[3] = {0, 0, 0};
    const int rc = run_columns(dev, cc, n, ms, launch);
    // what the inputs give, without the driver: items of finished chunks, nothing behind them
    bool match = d_in[ABSENT_IN] == nullptr && d_out[ABSENT_OUT] != nullptr;
    size_t n_refused = 0;
    const size_t n_done = std::min(n, dev.done);
    for (size_t i = 0; i < n; ++i) {
        unsigned sum = 0;
        for (int k = 0; k < iw.n; ++k)
            for (size_t b = 0; k != ABSENT_IN && b < iw.width[k]; ++b) sum += src[k][iw.width[k] * i + b];
        const bool no = refused(src[0][32 * i]);
        n_refused += no && i < n_done;
        for (int j = 0; j < OUT.n; ++j)
            for (size_t b = 0; j != ABSENT_OUT && b < OUT.width[j]; ++b) {
                const uint8_t want = j + 1 == OUT.n ? (no ? 9 : 0) : no ? 0 : result(sum, j, b);
                const uint8_t got = dst[j][OUT.width[j] * i + b];
                if (i < n_done ? got != want : !rc && got != 0xEE) match = false;   // (a failed call may have copied part of its last chunk)
            }
    }
    std::string work;
    work.swap(dev.ops);
    end_columns(dev, bufs, iw.secrets != 0, rc);
    char f[32] = "none";
    if (fail.kind) snprintf(f, sizeof f, "%c%d@%d", fail.kind, fail.k, fail.chunk);
    printf("run %d %zu %zu %s -> rc %d match %d refused %zu rezeroed %zu ms %.2f %.2f %.2f :%s |%s | %d %d %d\n", iw.secrets != 0, n, cap, f, rc, match, n_refused,
           rezeroed, ms[0], ms[1], ms[2], work.c_str(), dev.ops.c_str(), bufs.in.zero(), bufs.state.zero(), bufs.stage.cap ? bufs.stage.zero() : -1);
}

static void layout(const char* what, size_t n_pad, size_t total, const ColumnCall::Column* cols, int n, const uint8_t* base, bool stage) {
    printf("layout %zu %s %zu :", n_pad, what, total * n_pad);
    for (int k = 0; k < n; ++k)
        if (!stage || cols[k].stage) printf(" %zu/%zu", (size_t)((stage ? cols[k].stage : cols[k].dev) - base), cols[k].width);
    printf("\n");
}

int main() {
    const size_t ns[] = {1, 63, 64, 65, 130};
    for (size_t configured : {(size_t)0, (size_t)1, (size_t)64, (size_t)65})
        for (size_t by_default : {(size_t)128, (size_t)1 << 16, (size_t)1 << 19})
            for (size_t n : ns) {
                const size_t cap = column_chunk(configured, by_default, n);
                printf("chunk %zu %zu %zu -> %zu %zu\n", configured, by_default, n, cap, ColumnCall(IN_SECRET, OUT, cap).n_pad);
            }
    for (size_t cap : {(size_t)1, (size_t)64, (size_t)128, (size_t)192}) {
        ColumnCall cc(IN_SECRET, OUT, cap);
        std::vector<uint8_t> base(IN_SECRET.total * cc.n_pad);   // (only addresses are taken)
        cc.d_in = cc.d_out = cc.stage = base.data();
        for (int k = 0; k < IN_SECRET.n; ++k) cc.in(base.data());
        for (int j = 0; j < OUT.n; ++j) cc.out(base.data());
        layout("in", cc.n_pad, IN_SECRET.total, cc.ins, cc.n_in, base.data(), false);
        layout("stage", cc.n_pad, IN_SECRET.stage_total, cc.ins, cc.n_in, base.data(), true);
        layout("out", cc.n_pad, OUT.total, cc.outs, cc.n_out, base.data(), false);
    }
    for (const ColumnWidths* iw : {&IN_SECRET, &IN_PLAIN})
        for (size_t n : ns)
            for (size_t cap : {(size_t)1, (size_t)64, (size_t)128, column_chunk(0, 1 << 16, n)}) run(*iw, n, cap, Fail());
    for (const ColumnWidths* iw : {&IN_SECRET, &IN_PLAIN})
        for (int chunk : {0, 1})
            for (const char* f : {"M0", "M1", "M2", "M3", "H0", "H3", "Z0", "D0", "D3", "F0"}) run(*iw, 130, 64, Fail{f[0], f[1] - '0', chunk});
    return 0;
}
