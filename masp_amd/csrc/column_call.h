// The body the per-item wallet calls share (k_nullifier.hip, k_output_build.hip, k_spend_build.hip): a call's inputs and results are
// per-item arrays ("columns") side by side in one device buffer each, and the call runs chunk after chunk on one stream: upload the
// columns, zero the results, enqueue the kernels, download, wait.  Plain C++17, no HIP: what a copy, a memset, an event and the wait
// are is the caller's (column_host.h); tests/native/column_call_host.cpp runs layout, driver and ending on the CPU over plain arrays.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace masp {

constexpr int COLUMNS_MAX = 16;

// A buffer's columns at compile time: their widths in bytes per item, in the buffer's order.  off[k] and total are per item too: in a
// buffer for n_pad items column k starts at off[k] * n_pad.  Bit k of `secrets` marks input column k as one that is staged through
// pinned memory: the staging buffer is laid out as the input buffer is and ends behind the last secret column, so the secret columns
// stand first.  The last column of a result buffer is the status bytes.
struct ColumnWidths {
    int n = 0;
    unsigned secrets;
    size_t width[COLUMNS_MAX] = {}, off[COLUMNS_MAX] = {};
    size_t total = 0, stage_total = 0;
    constexpr ColumnWidths(std::initializer_list<size_t> widths, unsigned secrets_ = 0) : secrets(secrets_) {
        for (size_t w : widths) {
            width[n] = w;
            off[n] = total;
            total += w;
            if (secrets >> n++ & 1) stage_total = total;
        }
    }
};

// items per chunk of a call over n >= 1 items: what was configured (0: the call's default), and no more than n in whole waves
inline size_t column_chunk(size_t configured, size_t by_default, size_t n) {
    return std::min(configured ? configured : by_default, (n + 63) / 64 * 64);
}

// One call's columns: the two layouts for chunks of `cap` items, and what each column is bound to.  The buffers hold n_pad items, cap in
// whole waves, so every column starts on a multiple of 64 bytes.  Once the buffers exist (d_in, d_out, stage), the columns are declared
// in the layouts' order, in() and out() taking the next one each and handing back its device pointer.
struct ColumnCall {
    struct Column {
        uint8_t *dev, *stage;   // stage: an input column's pinned staging if it is secret, else null
        const uint8_t* src;     // an input column's source; null: absent, nothing is copied
        uint8_t* dst;           // a result column's destination; null: not downloaded
        size_t width;
    };
    const ColumnWidths &iw, &ow;
    const size_t cap, n_pad;
    uint8_t *d_in = nullptr, *d_out = nullptr, *stage = nullptr;
    Column ins[COLUMNS_MAX], outs[COLUMNS_MAX];
    int n_in = 0, n_out = 0;

    ColumnCall(const ColumnWidths& in_widths, const ColumnWidths& out_widths, size_t cap_) : iw(in_widths), ow(out_widths), cap(cap_), n_pad((cap_ + 63) / 64 * 64) {}

    // the next input column, from src; an absent one (src null) keeps its place and the kernels get a null pointer
    template <class T = uint8_t>
    const T* in(const void* src) {
        const int k = n_in;
        return in_at<T>(d_in + iw.off[k] * n_pad, iw.width[k], src, iw.secrets >> k & 1 ? stage + iw.off[k] * n_pad : nullptr);
    }
    // a further input column with a device base of its own, uploaded behind the layout's
    template <class T = uint8_t>
    const T* in_at(uint8_t* base, size_t width, const void* src, uint8_t* pinned = nullptr) {
        assert(n_in < COLUMNS_MAX);
        ins[n_in++] = {base, pinned, (const uint8_t*)src, nullptr, width};
        return src ? (const T*)base : nullptr;
    }
    // the next result column, to dst; one that is not asked for (dst null) is computed and zeroed all the same
    template <class T = uint8_t>
    T* out(void* dst) {
        assert(n_out < ow.n);
        const int k = n_out++;
        outs[k] = {d_out + ow.off[k] * n_pad, nullptr, nullptr, (uint8_t*)dst, ow.width[k]};
        return (T*)outs[k].dev;
    }
};

// Runs items [0, n) through launch(c) in chunks of cc.cap on the device `dev`: h2d(device, host, bytes), d2h(host, device, bytes),
// zero(device, bytes) and mark(k), each queued and -> rc, and finish(ms) -> rc, which waits for the chunk (the next one overwrites the
// buffers), reports a launch that was refused and adds the times between marks 0 to 3 to ms[0..2]: upload, kernels, download.  Secret
// columns go to the pinned stage first and up from there.  Every result but the status bytes is zeroed before the kernels, so that
// what they skip for a refused item reads zero; the status bytes come down first.  The first non-zero rc ends it and is returned:
// nothing is queued after it (what is queued before it is end_columns' to wait for).
template <class Dev, class Launch>
int run_columns(Dev& dev, const ColumnCall& cc, size_t n, double ms[3], Launch&& launch) {
    assert(cc.n_in >= cc.iw.n && cc.n_out == cc.ow.n);
    const ColumnCall::Column& status = cc.outs[cc.n_out - 1];
    int rc = 0;
    for (size_t o = 0; o < n; o += cc.cap) {
        const size_t c = std::min(cc.cap, n - o);
        for (int k = 0; k < cc.n_in; ++k)
            if (const ColumnCall::Column& x = cc.ins[k]; x.src && x.stage) memcpy(x.stage, x.src + x.width * o, x.width * c);
        if ((rc = dev.mark(0))) return rc;
        for (int k = 0; k < cc.n_in; ++k)
            if (const ColumnCall::Column& x = cc.ins[k]; x.src && (rc = dev.h2d(x.dev, x.stage ? x.stage : x.src + x.width * o, x.width * c))) return rc;
        if ((rc = dev.zero(cc.d_out, (size_t)(status.dev - cc.d_out))) || (rc = dev.mark(1))) return rc;
        launch(c);
        if ((rc = dev.mark(2)) || (rc = dev.d2h(status.dst + status.width * o, status.dev, status.width * c))) return rc;
        for (int k = 0; k + 1 < cc.n_out; ++k)
            if (const ColumnCall::Column& x = cc.outs[k]; x.dst && (rc = dev.d2h(x.dst + x.width * o, x.dev, x.width * c))) return rc;
        if ((rc = dev.mark(3)) || (rc = dev.finish(ms))) return rc;
    }
    return 0;
}

// The end of a call, on success and on every error path, before the wallet lock is released.  bufs: the call's in, state and stage
// buffers (.p, .cap bytes).  A call with secrets leaves nothing of them: the uploaded inputs and the per-item state are zeroed on the
// device, and behind dev.drain(), which waits for the stream, the pinned stage on the host.  A call without secrets waits only if it
// failed (a chunk that succeeded has been waited for): either way nothing of the call stays in flight.  (A memset or a wait that fails
// here is not reported over the call's own result.)
template <class Dev, class Bufs>
void end_columns(Dev& dev, Bufs& bufs, bool secrets, int rc) {
    if (secrets && bufs.in.p) (void)dev.zero(bufs.in.p, bufs.in.cap);
    if (secrets && bufs.state.p) (void)dev.zero(bufs.state.p, bufs.state.cap);
    if (secrets || rc) (void)dev.drain();
    if (secrets && bufs.stage.p) memset(bufs.stage.p, 0, bufs.stage.cap);
}

}  // namespace masp
