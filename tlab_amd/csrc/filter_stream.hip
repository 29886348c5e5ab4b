// OPR_FILTER's directional branch (operators/opr_filter.f90:283-392) as streaming kernels: in place, several fields a launch, a line swept as often
// as its recursion forces and no more.  The arithmetic is k_filter1d's (filter.hip), written once in filter_lines.hpp: the same expression trees in
// the same order, FP contraction off, true fp64 divisions, one line's recursion in one thread -- every word of a result equals k_filter1d's.
//
// A workgroup is one wave and owns 64 lines.  A sweep walks them B points at a time through an LDS tile: the wave loads the tile with B independent
// coalesced loads per lane (y, z: B = 16, a lane's own column, neighbouring lanes are neighbours in x; x: B = 32, rows of 32 contiguous points, two
// lines an instruction, the tile padded to 33 against bank conflicts), every lane advances its own line through its row of the tile, the wave stores the
// tile.  No transpose, no scratch of field size.  What a step reads beyond the point it writes -- the stencil of a right-hand side -- is a register
// window that the sweep feeds LAG points ahead, so the value written to the tile slot just read belongs LAG points behind it and the tile is stored
// shifted by LAG: a point is written only after every u that is still needed has been loaded.  The end rows of the non-periodic forms and the two
// or three points a periodic form needs from the far end are loaded into registers before the first store.
//
//   explicit4, explicit6   1 sweep                     16 B / point
//   compact                2 sweeps (RHS + forward elimination [+ TRIDPSS's wrk sum] up, back substitution down)          32 B / point
//   compactcutoff          2 sweeps (RHS + PENTADSS2's first recursion down from n, its second up); periodic: a third for dummy1 / dummy2    32 / 48 B
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/tlab_amd.h"
#include "errors.hpp"
#include "filter_lines.hpp"
#include "filter_state.hpp"
#include "internal.hpp"
#include "profile.hpp"

#pragma clang fp contract(off)

using namespace tlab;

namespace {

constexpr int FS_LINES = 64;                                                   // lines of a workgroup = lanes of its one wave
constexpr int FS_MAXF = 8;                                                     // fields of a launch (blockIdx.y)

struct StreamArgs {
    double *f[FS_MAXF];
    const double *c;         // device coeffs, column-major [ncols][n]
    long long nlines, rs, outer_stride;
    int n, lines_inner, bcsmin, bcsmax;
};

template <int B, bool X>
struct Stage;
template <int B, bool X, int S, int LAG, class Step>
__device__ __forceinline__ void stage_sweep(const Stage<B, X> &g, Step &&step);

// one workgroup's 64 lines and the tile they pass through: the G of filter_line
template <int B, bool X>
struct Stage {
    double *tile;            // LDS; X: [64][B + 1] (line, slot), else [B][64] (slot, line)
    double *f;
    long long line0, base, rs;      // first line of the workgroup; first point and point stride of the lane's own line
    int nl, lane, n;                // lines of the workgroup (<= 64)
    bool active;                    // the lane has a line
    __device__ __forceinline__ int at(int slot) const { return X ? lane * (B + 1) + slot : slot * FS_LINES + lane; }
    __device__ __forceinline__ double u(int i) const { return f[base + (long long)(i - 1) * rs]; }
    template <int S, int LAG, class Step>
    __device__ __forceinline__ void sweep(Step &&step) const { stage_sweep<B, X, S, LAG>(*this, step); }
};

// One sweep over the lines of the workgroup: S = +1 upwards from point 1, -1 downwards from point n.  step(i, x) is called for i = 1 - LAG .. n
// (S = -1: n + LAG .. 1) with x = the stored value at point i + S LAG where that is a point of the line (anything otherwise), and returns the new
// value of point i (ignored where i is no point of the line).
template <int B, bool X, int S, int LAG, class Step>
__device__ __forceinline__ void stage_sweep(const Stage<B, X> &g, Step &&step) {
    const int n = g.n, nsteps = n + LAG;
    for (int k0 = 0; k0 < nsteps; k0 += B) {
        // B independent loads per lane, then the tile: no load waits behind a branch (a point or a line beyond the end is read at the nearest valid one
        // and never used)
        double v[B];
        if constexpr (X) {
#pragma unroll
            for (int it = 0; it < B; ++it) {
                const int idx = it * FS_LINES + g.lane, l = min(idx / B, g.nl - 1), slot = idx % B;
                const int r = min(max(S > 0 ? 1 + k0 + slot : n - k0 - slot, 1), n);
                v[it] = g.f[(g.line0 + l) * n + (r - 1)];
            }
#pragma unroll
            for (int it = 0; it < B; ++it) {
                const int idx = it * FS_LINES + g.lane;
                g.tile[(idx / B) * (B + 1) + idx % B] = v[it];
            }
        } else {
#pragma unroll
            for (int slot = 0; slot < B; ++slot) {
                const int r = min(max(S > 0 ? 1 + k0 + slot : n - k0 - slot, 1), n);
                v[slot] = g.f[g.base + (long long)(r - 1) * g.rs];
            }
#pragma unroll
            for (int slot = 0; slot < B; ++slot) g.tile[slot * FS_LINES + g.lane] = v[slot];
        }
        __syncthreads();
        if (g.active) {
            const int m = min(B, nsteps - k0);
            for (int slot = 0; slot < m; ++slot) {
                const int r = S > 0 ? 1 + k0 + slot : n - k0 - slot;
                const int p = g.at(slot);
                g.tile[p] = step(r - S * LAG, g.tile[p]);
            }
        }
        __syncthreads();
        if constexpr (X) {
#pragma unroll
            for (int it = 0; it < B; ++it) {
                const int idx = it * FS_LINES + g.lane, l = idx / B, slot = idx % B;
                const int i = (S > 0 ? 1 + k0 + slot : n - k0 - slot) - S * LAG;
                if (l < g.nl && k0 + slot < nsteps && i >= 1 && i <= n) g.f[(g.line0 + l) * n + (i - 1)] = g.tile[l * (B + 1) + slot];
            }
        } else {
#pragma unroll
            for (int slot = 0; slot < B; ++slot) {
                const int i = (S > 0 ? 1 + k0 + slot : n - k0 - slot) - S * LAG;
                if (g.active && k0 + slot < nsteps && i >= 1 && i <= n) g.f[g.base + (long long)(i - 1) * g.rs] = g.tile[slot * FS_LINES + g.lane];
            }
        }
        __syncthreads();      // the stores are out before the next loads: the following sweep reads what other lanes stored (x), and the tile is free again
    }
}

template <int TYPE, bool PER, bool X>
__global__ void __launch_bounds__(FS_LINES) k_filter_stream(const StreamArgs a) {
#pragma clang fp contract(off)
    constexpr int B = X ? 32 : 16;
    __shared__ double tile[X ? FS_LINES * (B + 1) : FS_LINES * B];
    Stage<B, X> g;
    g.tile = tile; g.f = a.f[blockIdx.y]; g.lane = threadIdx.x; g.n = a.n; g.rs = a.rs;
    g.line0 = (long long)blockIdx.x * FS_LINES;
    const long long line = g.line0 + g.lane;
    g.active = line < a.nlines;
    g.nl = (int)min((long long)FS_LINES, a.nlines - g.line0);
    const long long lv = min(line, a.nlines - 1);      // a lane without a line loads the last line's points and stores nothing
    g.base = (lv / a.lines_inner) * a.outer_stride + lv % a.lines_inner;
    filter_line<TYPE, PER>(g, a.c, a.n, a.bcsmin, a.bcsmax);
}

template <int TYPE, bool PER>
void launch_tp(bool x, dim3 grid, const StreamArgs &a, hipStream_t st) {
    if (x) hipLaunchKernelGGL((k_filter_stream<TYPE, PER, true>), grid, dim3(FS_LINES), 0, st, a);
    else hipLaunchKernelGGL((k_filter_stream<TYPE, PER, false>), grid, dim3(FS_LINES), 0, st, a);
}

// sweeps over a line: what the recursion of the type forces (the header of this file)
int sweeps_of(int type, int periodic) { return type == FLT_COMPACT ? 2 : type == FLT_CUTOFF ? (periodic ? 3 : 2) : 1; }

void launch_filter(int dir, tlab_filter_t f, int nx, int ny, int nz, int nf, double *const *u, hipStream_t st) {
    const LineGeom g = line_geom(dir, nx, ny, nz);
    StreamArgs a;
    a.c = f->coeffs.p; a.nlines = g.nlines; a.rs = g.row_stride; a.outer_stride = g.outer_stride; a.n = g.n; a.lines_inner = g.lines_inner;
    a.bcsmin = f->bcsmin; a.bcsmax = f->bcsmax;
    static const char *const tag[3] = {"k_filter_stream_x", "k_filter_stream_y", "k_filter_stream_z"};
    for (int f0 = 0; f0 < nf; f0 += FS_MAXF) {
        const int m = std::min(FS_MAXF, nf - f0);
        for (int i = 0; i < FS_MAXF; ++i) a.f[i] = i < m ? u[f0 + i] : nullptr;
        const dim3 grid((unsigned)((g.nlines + FS_LINES - 1) / FS_LINES), (unsigned)m);
        ProfScope ps(tag[dir - 1], st, (double)m * g.nlines * g.n * 16.0 * sweeps_of(f->type, f->periodic));
        const bool x = dir == 1, per = f->periodic != 0;
        switch (f->type) {
        case FLT_COMPACT: per ? launch_tp<FLT_COMPACT, true>(x, grid, a, st) : launch_tp<FLT_COMPACT, false>(x, grid, a, st); break;
        case FLT_6E: per ? launch_tp<FLT_6E, true>(x, grid, a, st) : launch_tp<FLT_6E, false>(x, grid, a, st); break;
        case FLT_4E: per ? launch_tp<FLT_4E, true>(x, grid, a, st) : launch_tp<FLT_4E, false>(x, grid, a, st); break;
        case FLT_CUTOFF: per ? launch_tp<FLT_CUTOFF, true>(x, grid, a, st) : launch_tp<FLT_CUTOFF, false>(x, grid, a, st); break;
        default: throw Fail(TLAB_EUNSUPPORTED, "filter type: compact (1), explicit6 (2), explicit4 (3), compactcutoff (9)");
        }
        hk(hipGetLastError(), "k_filter_stream launch");
    }
}

}  // namespace

void tlab_internal_filter_fields(int nx, int ny, int nz, tlab_filter_t const *f, const int *repeat, int nf, double *const *u, hipStream_t st,
                                 const char *who) {
    const std::string w(who);
    if (nx < 1 || ny < 1 || nz < 1 || nf < 0 || (nf > 0 && !u)) throw Fail(TLAB_EINVAL, w + ": bad arguments");
    for (int i = 0; i < nf; ++i) {
        if (!u[i]) throw Fail(TLAB_EINVAL, w + ": bad arguments (null field)");
        for (int j = 0; j < i; ++j)
            if (u[j] == u[i]) throw Fail(TLAB_EINVAL, w + ": bad arguments (the same field twice)");
    }
    const int ext[3] = {nx, ny, nz};
    for (int d = 0; d < 3; ++d) {      // every refusal before the first launch: the fields are filtered in place, a call that fails must leave them as they were
        if (!f[d]) continue;
        if (f[d]->n != ext[d]) throw Fail(TLAB_EINVAL, w + ": filter size does not match the field size along its direction");
        if (repeat && repeat[d] < 1) throw Fail(TLAB_EINVAL, w + ": Filter.Repeat must be positive (opr_filter.f90:198-204)");
    }
    if (nf == 0) return;
    for (int d = 0; d < 3; ++d) {
        if (!f[d]) continue;
        const int rep = repeat ? repeat[d] : 1;
        for (int r = 0; r < rep; ++r) launch_filter(d + 1, f[d], nx, ny, nz, nf, u, st);
    }
}

extern "C" int tlab_opr_filter_fields(int nx, int ny, int nz, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat, int nf,
                                      double *const *u) {
    return guarded([&] {
        const tlab_filter_t f[3] = {fx, fy, fz};
        tlab_internal_filter_fields(nx, ny, nz, f, repeat, nf, u, tlab_current_stream(), "tlab_opr_filter_fields");
    });
}
