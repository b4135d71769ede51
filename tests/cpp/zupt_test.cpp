// zupt_test.cpp — csrc/host/zupt.h behind a C entry for tests/test_direct_update_reference.py (g++ alone: no HIP, no library).
#include "msckf_stereo_c_amd/csrc/host/zupt.h"

extern "C" int zupt_test_run(const zupt::Point *prev, int n_prev, const zupt::Point *curr, int n_curr, double fx, double fy, int min_features,
                             double max_disparity, int *n_common, double *mean_disparity) {
    const zupt::Disparity d = zupt::disparity(prev, (size_t)n_prev, curr, (size_t)n_curr, fx, fy);
    *n_common = d.n_common;
    *mean_disparity = d.mean_disparity;
    zupt::Config c;
    c.min_features = min_features;
    c.max_disparity = max_disparity;
    return zupt::stationary(d, c) ? 1 : 0;
}
