/* Host hooks for tests/test_drain_paths.py: the two functions the draw-first drain adds to include/ next to the ones they restate, compiled with the
 * oracle's flags (oracle/Makefile: no contraction, explicit fma) into a library of the test's own. */
#include <stdint.h>

#include "hh_envelope.h"

#define API __attribute__((visibility("default")))

/* both forms of the cannon cone's planar stage at n points with the heading vector (he, hn) */
API void dh_cannon_cone(int n, int ac_type, const double *lat1, const double *lon1, const double *lat2, const double *lon2, const double *he,
                        const double *hn, int32_t *full, int32_t *near_form) {
    for (int i = 0; i < n; i++) {
        full[i] = hh_cannon_cone_planar_outside(lat1[i], lon1[i], lat2[i], lon2[i], he[i], hn[i], ac_type);
        near_form[i] = hh_cannon_cone_planar_outside_near(lat1[i], lon1[i], lat2[i], lon2[i], he[i], hn[i], ac_type);
    }
}

/* the range of the mid-latitude estimate from both functions */
API void dh_estimate_range(int n, const double *lat1, const double *lon1, const double *lat2, const double *lon2, double *s_full, double *s_range) {
    for (int i = 0; i < n; i++) {
        double azi;
        hh_geo_inverse_estimate(lat1[i], lon1[i], lat2[i], lon2[i], &s_full[i], &azi);
        hh_geo_inverse_estimate_range(lat1[i], lon1[i], lat2[i], lon2[i], &s_range[i]);
    }
}
