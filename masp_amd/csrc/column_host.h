// The HIP half of the per-item wallet calls (column_call.h): the device its driver runs on, a stream with four events, and the steps
// every such call has around its own columns, kernels and tables.  What a call keeps between calls is PerItemCall (internal.h).
#pragma once
#include "internal.h"

namespace masp {

struct HipColumns {
    hipStream_t s;
    Event ev[4];
    int h2d(void* d, const void* h, size_t bytes) { return HIP_RC(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s)); }
    int d2h(void* h, const void* d, size_t bytes) { return HIP_RC(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s)); }
    int zero(void* d, size_t bytes) { return HIP_RC(hipMemsetAsync(d, 0, bytes, s)); }
    int mark(int k) { return HIP_RC(hipEventRecord(ev[k], s)); }
    int drain() { return HIP_RC(hipStreamSynchronize(s)); }
    int finish(double* ms) {
        if (drain()) return MASP_HIP_E_HIP;                          // the next chunk overwrites the buffers
        if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
        return add_elapsed(ev, 3, ms);
    }
};

// n >= 1 items of the call kind k through launch(c) on s, chunk after chunk; a call that succeeds leaves its stage times in k.timing
template <class Launch>
int run_per_item(hipStream_t s, PerItemCall& k, const ColumnCall& cc, size_t n, Launch&& launch) {
    HipColumns dev{s, {}};
    double ms[3] = {0, 0, 0};
    int rc;
    if ((rc = create_events(dev.ev)) || (rc = run_columns(dev, cc, n, ms, launch))) return rc;
    k.timing.store(ms);
    return MASP_HIP_OK;
}

// behind run_per_item and whatever failed in front of it, before WalletCall::done: end_columns, the error text staying the call's own; -> rc
inline int end_per_item(hipStream_t s, PerItemCall& k, const ColumnWidths& in_widths, int rc) {
    const std::string text = last_hip_error();
    HipColumns dev{s, {}};
    end_columns(dev, k, in_widths.secrets != 0, rc);
    last_hip_error() = text;
    return rc;
}

// the bodies of a call kind's configure (items per chunk, 0 = the default, `most` at the most) and last_timing
inline int per_item_configure(masp_hip_ctx* ctx, PerItemCall WalletState::*k, size_t chunk, size_t most) {
    if (!ctx || chunk > most) return MASP_HIP_E_INVALID_ARG;
    (FIRST_DEVICE(ctx)->wallet.*k).chunk.store(chunk);
    return MASP_HIP_OK;
}
inline int per_item_last_timing(masp_hip_ctx* ctx, PerItemCall WalletState::*k, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    (FIRST_DEVICE(ctx)->wallet.*k).timing.load(ms);
    return MASP_HIP_OK;
}

}  // namespace masp
