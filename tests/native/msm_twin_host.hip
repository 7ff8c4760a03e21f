// Test-only unit over the geometry of doubled window rows (masp_amd/csrc/device/msm_geom.h: msm_geom_twin, msm_twin_class, msm_twin_bucket),
// host code only: what the kernels and the drivers share, handed to tests/test_msm_twin_rows_host.py as plain integers.  Needs no device.
#include "../../masp_amd/csrc/device/msm_geom.h"

using namespace masp;

extern "C" {

// out: c, W, nb, twin, tables, |B|, classes
void mtw_geom(int c, int twin, uint32_t out[7]) {
    const MsmGeom g = twin ? msm_geom_twin(c) : msm_geom(c);
    out[0] = (uint32_t)g.c;
    out[1] = (uint32_t)g.W;
    out[2] = (uint32_t)g.nb;
    out[3] = (uint32_t)g.twin;
    out[4] = (uint32_t)g.tables();
    out[5] = msm_twin_buckets(c);
    out[6] = msm_twin_classes(c);
}
// out: off, size, weight of class s
void mtw_class(int c, uint32_t s, uint32_t out[3]) {
    const MsmTwinClass k = msm_twin_class(c, s);
    out[0] = k.off;
    out[1] = k.size;
    out[2] = k.weight;
}
// digit magnitude v -> bucket id; *mult: 0 the window's own row, 1 its doubled row
uint32_t mtw_bucket(int c, uint32_t v, uint32_t* mult) { return msm_twin_bucket(c, v, *mult); }

}  // extern "C"
