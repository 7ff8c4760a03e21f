// The chunk pipeline of the output scans (masp_amd/csrc/chunk_pipeline.h) on the CPU: run_chunks over callbacks that only record.
// One case per line of the output (tests/test_chunk_pipeline_host.py reads them):
//
//     run <n> <per> <fail> -> rc <rc> : E<o0>/<n>@<set> C<o0>/<n>@<set> D<set> ...
//
// <fail>: "none", "e<k>" (the k-th enqueue returns 7) or "c<k>" (the k-th collect returns 9), k counted from 0; the trace lists every
// call of enqueue (E), collect (C) and drain (D) in order, the failing one included.  Then the chunk-size rule:
//
//     per <n_keys> <chunk_outputs(n_keys)> <NS_BLOCK> <NS_CHUNK_PAIRS>
#include "chunk_pipeline.h"

#include <cstdio>
#include <string>

static void run(size_t n, size_t per, char kind, int at) {
    std::string trace;
    int n_enq = 0, n_col = 0;
    auto call = [&](char what, const masp::ChunkInFlight& c) {
        char buf[64];
        snprintf(buf, sizeof buf, " %c%zu/%zu@%d", what, c.o0, c.n, c.set);
        trace += buf;
    };
    const int rc = masp::run_chunks(
        n, per,
        [&](const masp::ChunkInFlight& c) {
            call('E', c);
            return kind == 'e' && n_enq++ == at ? 7 : 0;
        },
        [&](const masp::ChunkInFlight& c) {
            call('C', c);
            return kind == 'c' && n_col++ == at ? 9 : 0;
        },
        [&](int set) { trace += " D" + std::to_string(set); });
    if (kind == 'n')
        printf("run %zu %zu none -> rc %d :%s\n", n, per, rc, trace.c_str());
    else
        printf("run %zu %zu %c%d -> rc %d :%s\n", n, per, kind, at, rc, trace.c_str());
}

int main() {
    const size_t per = 4;
    for (size_t n : {(size_t)0, (size_t)1, per, per + 1, 2 * per, 3 * per + 1}) run(n, per, 'n', 0);
    for (char kind : {'e', 'c'})
        for (int at = 0; at < 4; ++at) run(3 * per + 1, per, kind, at);   // four chunks
    for (size_t keys : {(size_t)1, (size_t)32, (size_t)1024, (size_t)1025, (size_t)4096})
        printf("per %zu %zu %u %zu\n", keys, masp::chunk_outputs(keys), masp::NS_BLOCK, masp::NS_CHUNK_PAIRS);
    return 0;
}
