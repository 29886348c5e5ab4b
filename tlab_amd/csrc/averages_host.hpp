// Plane statistics (averages.hip, averages.cpp): the programs of k_plane_partial -- which fields a point reads, which plane means it needs and which
// terms it adds up -- written once for the kernel and for the host loop, and the constants a test mirrors.
//
// A program is a type with NFLD fields, NMEAN plane means (mean i belongs to field i), NOUT outputs and add(x, m, acc): acc[o] += term o of one
// point with the field values x and the means m of its plane.  The operation order inside a term is the reference's, left to right as written
// there; nothing is contracted into a fused multiply-add (the pragma below: this header is code of both sides).
//   AvgMeans<NF>   AVG_IK_V (utils/averages.f90:301-327) of NF fields at once
//   AvgPower<IMOM> AVG1V2D_V (:142-167): a**imom as gfortran expands an integer power: a, a*a, (a*a)*a, and a**4 as (a*a)*(a*a)
//   AvgFlow<P>     the incompressible covariances of AVG_FLOW_XZ (statistics/avg_flow_xz.f90:513-553, :597-654) on u, v, w (, p)
//   AvgScal<P>     the moments and fluxes of AVG_SCAL_XZ (statistics/avg_scal_xz.f90:373-455) on s, u, v, w (, p)
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)      // every multiply and add below stays as written

namespace tlab {

constexpr int AVG_ROWS_PER_GROUP = 32;      // rows of k one workgroup of k_plane_partial sums (tests/test_gpu_averages.py mirrors it)
constexpr int AVG_FIELDS_PER_LAUNCH = 8;    // AvgMeans: more fields go in groups
constexpr int AVG_MAX_FIELDS = 8;           // fields of one program (the kernel's argument block)

enum { AVG_PROG_MEANS = 0, AVG_PROG_POWER = 1, AVG_PROG_FLOW = 2, AVG_PROG_SCAL = 3 };

template <int NF>
struct AvgMeans {
    static constexpr int NFLD = NF, NMEAN = 0, NOUT = NF;
    static __host__ __device__ __forceinline__ void add(const double *x, const double *, double *acc) {
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] += x[f];
    }
};

template <int IMOM>
struct AvgPower {
    static constexpr int NFLD = 1, NMEAN = 0, NOUT = 1;
    static __host__ __device__ __forceinline__ void add(const double *x, const double *, double *acc) {
        const double a = x[0], a2 = a * a;
        acc[0] += IMOM == 1 ? a : IMOM == 2 ? a2 : IMOM == 3 ? a2 * a : a2 * a2;
    }
};

// outputs: Rxx Ryy Rzz | Rxy Rxz Ryz | rU3 rU4 rV3 rV4 rW3 rW4 | Txxy Tyyy Tzzy | Txyy Txzy Tyzy | with p: rP2 u'p' v'p' w'p'
template <bool P>
struct AvgFlow {
    static constexpr int NFLD = 3 + (P ? 1 : 0), NMEAN = NFLD, NOUT = 18 + (P ? 4 : 0);
    static __host__ __device__ __forceinline__ void add(const double *x, const double *m, double *acc) {
        const double u = x[0] - m[0], v = x[1] - m[1], w = x[2] - m[2];      // dwdx, dwdy, dwdz (:514-516)
        const double uu = u * u, vv = v * v, ww = w * w, uv = u * v;
        acc[0] += uu; acc[1] += vv; acc[2] += ww;                           // :520-522
        acc[3] += uv; acc[4] += u * w; acc[5] += v * w;                      // :538-540
        const double u3 = uu * u, v3 = vv * v, w3 = ww * w;                  // :597, :602, :607
        acc[6] += u3; acc[7] += u * u3;
        acc[8] += v3; acc[9] += v * v3;
        acc[10] += w3; acc[11] += w * w3;
        acc[12] += uu * v; acc[13] += vv * v; acc[14] += ww * v;             // :613-615
        acc[15] += uv * v; acc[16] += uv * w; acc[17] += vv * w;             // :626-628
        if constexpr (P) {
            const double p = x[3] - m[3];                                    // dvdz (:640)
            acc[18] += p * p; acc[19] += u * p; acc[20] += v * p; acc[21] += w * p;      // :642, :646-648
        }
    }
};

// outputs: rS2 rS3 rS4 | Rsu Rsv Rsw | Tssy1 | Tsuy1 Tsvy1 Tswy1 | with p: Tsvy3
template <bool P>
struct AvgScal {
    static constexpr int NFLD = 4 + (P ? 1 : 0), NMEAN = NFLD, NOUT = 10 + (P ? 1 : 0);
    static __host__ __device__ __forceinline__ void add(const double *x, const double *m, double *acc) {
        const double s = x[0] - m[0], u = x[1] - m[1], v = x[2] - m[2], w = x[3] - m[3];
        const double s2 = s * s, s3 = s * s2;                                // :376, :378
        acc[0] += s2; acc[1] += s3; acc[2] += s * s3;                        // :380
        const double su = s * u, sv = s * v, sw = s * w;                     // :414-416
        acc[3] += su; acc[4] += sv; acc[5] += sw;
        acc[6] += sv * s;                                                    // :432
        acc[7] += su * v; acc[8] += sv * v; acc[9] += sw * v;                // :433-435
        if constexpr (P) acc[10] += (x[4] - m[4]) * s;                       // :450
    }
};

struct AvgInfo { int nfld, nmean, nout; };
// param: the number of fields (MEANS), imom (POWER), 1 with a pressure field (FLOW, SCAL)
inline AvgInfo avg_info(int prog, int param) {
    switch (prog) {
    case AVG_PROG_MEANS: return {param, 0, param};
    case AVG_PROG_POWER: return {1, 0, 1};
    case AVG_PROG_FLOW: return {param ? 4 : 3, param ? 4 : 3, param ? 22 : 18};
    default: return {param ? 5 : 4, param ? 5 : 4, param ? 11 : 10};
    }
}

// Calls fn(P{}) with the program type P of (prog, param); false when there is none.
template <class F>
bool avg_dispatch(int prog, int param, F &&fn) {
    switch (prog) {
    case AVG_PROG_MEANS:
        switch (param) {
        case 1: fn(AvgMeans<1>{}); return true;
        case 2: fn(AvgMeans<2>{}); return true;
        case 3: fn(AvgMeans<3>{}); return true;
        case 4: fn(AvgMeans<4>{}); return true;
        case 5: fn(AvgMeans<5>{}); return true;
        case 6: fn(AvgMeans<6>{}); return true;
        case 7: fn(AvgMeans<7>{}); return true;
        case 8: fn(AvgMeans<8>{}); return true;
        }
        return false;
    case AVG_PROG_POWER:
        switch (param) {
        case 1: fn(AvgPower<1>{}); return true;
        case 2: fn(AvgPower<2>{}); return true;
        case 3: fn(AvgPower<3>{}); return true;
        case 4: fn(AvgPower<4>{}); return true;
        }
        return false;
    case AVG_PROG_FLOW:
        if (param) fn(AvgFlow<true>{}); else fn(AvgFlow<false>{});
        return true;
    case AVG_PROG_SCAL:
        if (param) fn(AvgScal<true>{}); else fn(AvgScal<false>{});
        return true;
    }
    return false;
}

}  // namespace tlab
