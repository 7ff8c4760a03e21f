// The chunk pipeline of the three output scans (k_note_scan.hip, k_note_scan_compact.hip, k_out_recovery.hip): a call's outputs are cut
// into chunks that alternate between two buffer sets, each on a stream of its own, so that a chunk's upload runs beside the chunk
// before's kernels.  Plain C++17, no HIP: what a set is, and what enqueueing, collecting and draining one means, is the caller's
// (scan_host.h); tests/native/chunk_pipeline_host.cpp runs the driver on the CPU with recording callbacks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace masp {

constexpr uint32_t NS_BLOCK = 256;                   // lanes per workgroup of the scans' kernels: a chunk is whole workgroups of outputs
constexpr size_t NS_CHUNK_PAIRS = (size_t)1 << 18;   // pairs per launch: one lane each, four waves on every SIMD of the chip

struct ChunkInFlight {
    size_t o0 = 0, n = 0;   // outputs [o0, o0 + n) of the call
    int set = 0;            // the buffer set and stream it runs on
};

// outputs per chunk for n_keys (> 0) keys: NS_CHUNK_PAIRS pairs in whole workgroups, one workgroup at the least
inline size_t chunk_outputs(size_t n_keys) { return std::max<size_t>(NS_BLOCK, NS_CHUNK_PAIRS / n_keys / NS_BLOCK * NS_BLOCK); }

// Runs [0, n_out) in chunks of `per` outputs through enqueue(chunk) -> rc, collect(chunk) -> rc and drain(set).  A set's previous
// chunk (two chunks back) is collected before the set is reused; at the end the pending chunks are collected, the older first.  The
// first non-zero rc ends it and is returned: nothing is enqueued or collected after it, and drain is called for the set it came from
// and for the other one if a chunk is pending there, so that nothing of the call stays in flight.
template <class Enqueue, class Collect, class Drain>
int run_chunks(size_t n_out, size_t per, Enqueue&& enqueue, Collect&& collect, Drain&& drain) {
    ChunkInFlight fly[2];
    bool pending[2] = {false, false};
    int rc = 0, set = 0;   // (set: after an error the one it came from, else the one whose turn is next: it holds the older chunk)
    for (size_t o0 = 0; o0 < n_out; o0 += per, set ^= 1) {
        if (pending[set]) {
            pending[set] = false;
            if ((rc = collect(fly[set]))) break;
        }
        fly[set].o0 = o0;
        fly[set].n = std::min(per, n_out - o0);
        fly[set].set = set;
        if ((rc = enqueue(fly[set]))) break;
        pending[set] = true;
    }
    for (int i = 0; i < 2 && !rc; ++i)
        if (pending[set ^ i]) {
            pending[set ^ i] = false;
            if ((rc = collect(fly[set ^ i]))) set ^= i;
        }
    if (rc) {
        drain(set);
        if (pending[set ^ 1]) drain(set ^ 1);
    }
    return rc;
}

}  // namespace masp
