// The HIP half the three output scans share (k_note_scan.hip, k_note_scan_compact.hip, k_out_recovery.hip) under the chunk pipeline
// (chunk_pipeline.h): what a buffer set keeps on the host, how a chunk's hits come back, how a call's hits go to the caller.  Each unit
// has its own kernels, device buffers and enqueue.
#pragma once
#include "internal.h"

namespace masp {

// a hit as the kernels report it: (output, key) and P bytes of payload (the symmetric key, the ock; plaintext | pk_d of the compact scan)
template <size_t P>
struct ScanHit {
    uint32_t output, key;
    uint8_t data[P];
};

// What a buffer set has on the host for the length of a call: its N_EV timing events, created at the set's first chunk (ev[0] before the
// upload, the others behind the stages), and the vectors its hits are copied into.  They are the set's and not scan_collect's own so that
// a copy that is still queued when scan_collect fails has somewhere to land until the pipeline drains the stream.
template <int N_EV>
struct ScanSetHost {
    Event ev[N_EV];
    std::vector<uint32_t> idx;
    std::vector<uint8_t> data;
};

// Waits for chunk c on its stream s and takes its statuses and hits.  count(nh), called once the chunk's counters are on the host,
// sets the number of hits and says whether the counters are within the chunk's pairs (if not: an error with `beyond` as its text).
// d_status: the chunk's status bytes, copied to epk_status + c.o0 if that is asked for; d_idx, d_data: nh x (output, key) and nh x P
// bytes.  ms[i] += the time between the set's events i and i + 1.
template <size_t P, int N_EV, class Count>
int scan_collect(hipStream_t s, const ChunkInFlight& c, ScanSetHost<N_EV>& h, Count&& count, const char* beyond, uint8_t* epk_status,
                 const uint8_t* d_status, const void* d_idx, const void* d_data, std::vector<ScanHit<P>>& hits, double* ms) {
    HIP_TRY(hipStreamSynchronize(s));
    if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
    size_t nh = 0;
    if (!count(nh)) {
        last_hip_error() = beyond;
        return MASP_HIP_E_HIP;
    }
    if (epk_status) HIP_TRY(hipMemcpyAsync(epk_status + c.o0, d_status, c.n, hipMemcpyDeviceToHost, s));
    h.idx.resize(2 * nh);
    h.data.resize(P * nh);
    if (nh) {
        HIP_TRY(hipMemcpyAsync(h.idx.data(), d_idx, 8 * nh, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.data.data(), d_data, P * nh, hipMemcpyDeviceToHost, s));
    }
    if (epk_status || nh) HIP_TRY(hipStreamSynchronize(s));   // (else nothing was queued behind the first one)
    for (size_t i = 0; i < nh; ++i) {
        ScanHit<P> hit;
        hit.output = h.idx[2 * i];
        hit.key = h.idx[2 * i + 1];
        memcpy(hit.data, &h.data[P * i], P);
        hits.push_back(hit);
    }
    return add_elapsed(h.ev, N_EV - 1, ms);
}

// A call's hits to the caller: sorted by (output, key), the order lanes reached the counter in being no order; *n_hits set; then
// MASP_HIP_E_CAPACITY with nothing written if there are more than `capacity` (the caller comes back with room for *n_hits), else every
// record split into hit_output, hit_key, the first na bytes of its payload to a + na i and the other P - na (if any) to b + (P - na) i.
template <size_t P>
int scan_finish(std::vector<ScanHit<P>>& hits, size_t capacity, uint32_t* hit_output, uint32_t* hit_key, uint8_t* a, size_t na, uint8_t* b,
                size_t* n_hits) {
    std::sort(hits.begin(), hits.end(),
              [](const ScanHit<P>& x, const ScanHit<P>& y) { return x.output != y.output ? x.output < y.output : x.key < y.key; });
    *n_hits = hits.size();
    if (hits.size() > capacity) return MASP_HIP_E_CAPACITY;
    for (size_t i = 0; i < hits.size(); ++i) {
        hit_output[i] = hits[i].output;
        hit_key[i] = hits[i].key;
        memcpy(a + na * i, hits[i].data, na);
        if (na < P) memcpy(b + (P - na) * i, hits[i].data + na, P - na);
    }
    return MASP_HIP_OK;
}

}  // namespace masp
