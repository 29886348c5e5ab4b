// The filter object behind tlab_filter_t, shared by filter.hip (k_filter1d, tlab_filter_create) and filter_stream.hip (the streaming kernels).
#pragma once
#include "../../include/tlab_amd.h"
#include "plan.hpp"

struct tlab_filter {
    int type, n, periodic, bcsmin, bcsmax, ncols;
    tlab::DeviceArray coeffs;      // [ncols][n], column-major like f%coeffs
    tlab::DeviceArray ws;          // two transposed copies of a field: x lines are filtered with the lines made the fastest index (tlab_internal_filter_1d)
};
