// The line algorithms of the streaming filter kernels (tlab_amd/csrc/filter_lines.hpp) on one line of host memory, for
// tests/test_filter_lines_host.py: a serial sweep through a tile of 5 points that loads, steps and stores shifted by the lag as the device stage does.
#include "filter_lines.hpp"
#include <algorithm>
struct HostLine {
    double *f; int n;
    double u(int i) const { return f[i - 1]; }
    template <int S, int LAG, class Step> void sweep(Step &&step) const {
        const int B = 5, nsteps = n + LAG; double tile[B];
        for (int k0 = 0; k0 < nsteps; k0 += B) {
            for (int s = 0; s < B; ++s) { int r = std::min(std::max(S > 0 ? 1 + k0 + s : n - k0 - s, 1), n); tile[s] = f[r - 1]; }
            int m = std::min(B, nsteps - k0);
            for (int s = 0; s < m; ++s) { int r = S > 0 ? 1 + k0 + s : n - k0 - s; tile[s] = step(r - S * LAG, tile[s]); }
            for (int s = 0; s < B; ++s) { int i = (S > 0 ? 1 + k0 + s : n - k0 - s) - S * LAG; if (k0 + s < nsteps && i >= 1 && i <= n) f[i - 1] = tile[s]; }
        }
    }
};
using namespace tlab;
extern "C" void host_filter(int type, int per, int n, int b0, int b1, const double *c, double *f) {
    HostLine g{f, n};
#define RUN(T) (per ? filter_line<T, true>(g, c, n, b0, b1) : filter_line<T, false>(g, c, n, b0, b1))
    if (type == 1) RUN(FLT_COMPACT); else if (type == 2) RUN(FLT_6E); else if (type == 3) RUN(FLT_4E); else RUN(FLT_CUTOFF);
}
