// The pieces of the proving pipeline (prove.hip) that the building blocks and measurement hooks (hooks.hip) drive too.
#pragma once
#include "internal.h"

namespace masp {

// [0, n) cut into ceil(n / cap) groups whose sizes differ by at most one: (first, count) pairs
std::vector<std::pair<size_t, size_t>> even_groups(size_t n, size_t cap);
// x, 32 bytes little-endian, is a canonical element of Fr
bool rs_in_range(const uint8_t* x);
// at least min(want, the context's rows of streams) slots exist (the slot pool; takes slot_mu)
int ensure_slots(masp_hip_ctx* ctx, size_t want);
int enqueue_quotient(Slot& sl, const NttDomain& D, const Fr* const in[3], size_t in_stride, uint32_t nrows, bool mont_in, uint32_t np,
                     Fr* h_out = nullptr, size_t h_stride = 0);
int enqueue_proofs(Slot& sl, Circuit& C, uint32_t np, const Fr* d_w, size_t w_stride, const Fr* const d_abc[3], const uint32_t* d_rs,
                   uint8_t* d_proof, bool aux_montgomery = false);

}  // namespace masp
