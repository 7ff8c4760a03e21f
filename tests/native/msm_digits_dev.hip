// Test-only unit over the sort's digit iterator (masp_amd/csrc/device/msm_sort.hpp: MsmDigitIter), its host instantiation: the very source the
// kernels k_msm_hist, k_msm_partition and k_msm_scatter run per lane, scalar after scalar on the CPU, handed to tests/test_msm_digit_iter.py as
// plain integers.  Needs no device.
#include "../../masp_amd/csrc/device/msm_sort.hpp"

using namespace masp;

extern "C" {

// scalars: n x 8 little-endian words.  out: n x W x 4 words — (table, bucket, neg, non-zero) of window 0, 1, ... as MsmDigitIter::next hands
// them out (bucket is meaningless where non-zero is 0).  twin: the geometry of doubled window rows (msm_geom_twin).  Returns W.
int mdd_digits(const uint32_t* scalars, uint32_t n, int c, int twin, uint32_t* out) {
    const MsmGeom g = twin ? msm_geom_twin(c) : msm_geom(c);
    for (uint32_t i = 0; i < n; ++i) {
        MsmScalar s;
        for (int k = 0; k < 8; ++k) s.w[k] = scalars[(size_t)i * 8 + k];
        MsmDigitIter it(s, g);
        for (int j = 0; j < g.W; ++j) {
            uint32_t table = 0, bucket = 0, neg = 0;
            const bool nz = it.next(table, bucket, neg);
            uint32_t* o = out + ((size_t)i * g.W + j) * 4;
            o[0] = table;
            o[1] = bucket;
            o[2] = neg;
            o[3] = nz ? 1u : 0u;
        }
    }
    return g.W;
}
// the class of a scalar as the kernels take it: 0 zero, 1 one, 2 anything else
int mdd_class(const uint32_t* scalar) {
    MsmScalar s;
    for (int k = 0; k < 8; ++k) s.w[k] = scalar[k];
    return msm_scalar_class(s);
}

}  // extern "C"
