// Plane statistics (averages.hip, averages.cpp): the programs of k_plane_partial -- which fields a point reads, which plane means it needs and which
// terms it adds up -- written once for the kernel and for the host loop, and the constants a test mirrors.
//
// A program is a type with NFLD fields, NMEAN plane means (its own table [NMEAN][ny]: a mean need not belong to a field), NOUT outputs and
// add(x, m, acc): acc[o] += term o of one point with the field values x and the means m of its plane.  The operation order inside a term is the
// reference's, left to right as written there; nothing is contracted into a fused multiply-add (the pragma below: this header is code of both
// sides).  ROWS is the number of rows of every field the kernel requests before it uses the first (ROWS NFLD loads in flight per lane); it is
// part of the order of summation, so it belongs to the program.  TAG names the launch in a profile.
//   AvgMeans<NF>   AVG_IK_V (utils/averages.f90:301-327) of NF fields at once
//   AvgPower<IMOM> AVG1V2D_V (:142-167): a**imom as gfortran expands an integer power: a, a*a, (a*a)*a, and a**4 as (a*a)*(a*a)
//   AvgFlow<P>     the incompressible covariances of AVG_FLOW_XZ (statistics/avg_flow_xz.f90:513-553, :597-654) on u, v, w (, p)
//   AvgScal<P>     the moments and fluxes of AVG_SCAL_XZ (statistics/avg_scal_xz.f90:373-455) on s, u, v, w (, p)
// and the groups of the same two routines that need derivative fields, on the nine velocity gradients g[0..8] = dudx dudy dudz dvdx dvdy dvdz dwdx
// dwdy dwdz.  Constant transport: the vis factors of EQNS_TRANS_POWERLAW / SUTHERLAND are not applied.  A profile is RAW: before any visc, diff,
// c23 or 2.0 the reference applies to it on the host.
//   AvgGradFlow1    vorticity and the raw stresses Tau_yy Tau_xy Tau_yz (avg_flow_xz.f90:991-1006, :1181-1197): no means
//   AvgGradFlow2    the derivative moments, U_ii2, vort**2, Phi, Exx .. Eyz (:993-1176): means rU_y rV_y rW_y vortx vorty vortz
//   AvgGradFlow3<P> the viscous transport terms (:1212-1245) and the pressure strain PIxx .. PIyz (:681-699) on g, u, v, w (, p):
//                   means Tau_yy Tau_xy Tau_yz (raw) fU fV fW (, rP)
//   AvgUGradP       u dpdx + v dpdy + w dpdz (:673)
//   AvgGradScal1    Fy, Ess, S_x2 .. S_z4 (avg_scal_xz.f90:607, :714-738) on dsdx dsdy dsdz: mean rS_y
//   AvgGradScal2<P> Tssy2, Tsuy2_d .. Tswy2_d (:742-745) and PIsu PIsv PIsw (:451-453) on dsdy s u v w (, p dsdx dsdz):
//                   means Fy fS fU fV fW (, rP fS_y)
//   AvgCov2         a*b, a*a, b*b of a pair of fields (COV2V2D, utils/averages.f90:244-267): the covariances of tools/statistics/spectra.f90
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)      // every multiply and add below stays as written

namespace tlab {

constexpr int AVG_ROWS_PER_GROUP = 32;      // rows of k one workgroup of k_plane_partial sums (tests/test_gpu_averages.py mirrors it)
constexpr int AVG_FIELDS_PER_LAUNCH = 8;    // AvgMeans: more fields go in groups
constexpr int AVG_MAX_FIELDS = 13;          // fields of one program (the kernel's argument block)

constexpr double AVG_C23 = 2.0 / 3.0;       // c23 of the reference (2.0_wp/3.0_wp)

enum { AVG_PROG_MEANS = 0, AVG_PROG_POWER = 1, AVG_PROG_FLOW = 2, AVG_PROG_SCAL = 3, AVG_PROG_GRAD_FLOW1 = 4, AVG_PROG_GRAD_FLOW2 = 5,
       AVG_PROG_GRAD_FLOW3 = 6, AVG_PROG_UGRADP = 7, AVG_PROG_GRAD_SCAL1 = 8, AVG_PROG_GRAD_SCAL2 = 9, AVG_PROG_COV2 = 10 };

template <int NF>
struct AvgMeans {
    static constexpr int NFLD = NF, NMEAN = 0, NOUT = NF, ROWS = NF <= 4 ? 4 : 16 / NF;
    static constexpr const char *TAG = "k_plane_partial<MEANS>";
    static __host__ __device__ __forceinline__ void add(const double *x, const double *, double *acc) {
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] += x[f];
    }
};

template <int IMOM>
struct AvgPower {
    static constexpr int NFLD = 1, NMEAN = 0, NOUT = 1, ROWS = 4;
    static constexpr const char *TAG = "k_plane_partial<POWER>";
    static __host__ __device__ __forceinline__ void add(const double *x, const double *, double *acc) {
        const double a = x[0], a2 = a * a;
        acc[0] += IMOM == 1 ? a : IMOM == 2 ? a2 : IMOM == 3 ? a2 * a : a2 * a2;
    }
};

// outputs: Rxx Ryy Rzz | Rxy Rxz Ryz | rU3 rU4 rV3 rV4 rW3 rW4 | Txxy Tyyy Tzzy | Txyy Txzy Tyzy | with p: rP2 u'p' v'p' w'p'
template <bool P>
struct AvgFlow {
    static constexpr int NFLD = 3 + (P ? 1 : 0), NMEAN = NFLD, NOUT = 18 + (P ? 4 : 0), ROWS = 4;
    static constexpr const char *TAG = "k_plane_partial<FLOW>";
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
    static constexpr int NFLD = 4 + (P ? 1 : 0), NMEAN = NFLD, NOUT = 10 + (P ? 1 : 0), ROWS = P ? 3 : 4;
    static constexpr const char *TAG = "k_plane_partial<SCAL>";
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

// acc[0], acc[stride], acc[2 stride] += a*a, (a*a)*a, ((a*a)*a)*a: the chain p = a*a; p = p*a; p = p*a of avg_flow_xz.f90:1021-1026
static __host__ __device__ __forceinline__ void avg_chain(double a, double *acc, int stride) {
    double p = a * a;
    acc[0] += p;
    p = p * a;
    acc[stride] += p;
    p = p * a;
    acc[2 * stride] += p;
}

// outputs: vortx vorty vortz | Tau_yy Tau_xy Tau_yz (raw)
struct AvgGradFlow1 {
    static constexpr int NFLD = 9, NMEAN = 0, NOUT = 6, ROWS = 2;
    static constexpr const char *TAG = "k_plane_partial<GRAD_FLOW1>";
    static __host__ __device__ __forceinline__ void add(const double *g, const double *, double *acc) {
        const double dudx = g[0], dudy = g[1], dudz = g[2], dvdx = g[3], dvdy = g[4], dvdz = g[5], dwdx = g[6], dwdy = g[7], dwdz = g[8];
        acc[0] += dwdy - dvdz; acc[1] += dudz - dwdx; acc[2] += dvdx - dudy;      // :991, :998, :1005
        acc[3] += dvdy * 2.0 - dudx - dwdz;                                        // :1181
        acc[4] += dudy + dvdx;                                                      // :1189
        acc[5] += dvdz + dwdy;                                                      // :1197
    }
};

// outputs: U_x2 U_x3 U_x4 | V_y. | W_z. | U_y. | U_z. | V_x. | V_z. | W_x. | W_y. | U_ii2 | vortx2 vorty2 vortz2 | Phi | Exx Eyy Ezz Exy Exz Eyz
struct AvgGradFlow2 {
    static constexpr int NFLD = 9, NMEAN = 6, NOUT = 38, ROWS = 2;
    static constexpr const char *TAG = "k_plane_partial<GRAD_FLOW2>";
    static __host__ __device__ __forceinline__ void add(const double *g, const double *m, double *acc) {
        const double dudx = g[0], dudy = g[1], dudz = g[2], dvdx = g[3], dvdy = g[4], dvdz = g[5], dwdx = g[6], dwdy = g[7], dwdz = g[8];
        avg_chain(dudx, acc + 0, 1);              // :1021-1026
        avg_chain(dvdy - m[1], acc + 3, 1);       // :1028-1039
        avg_chain(dwdz, acc + 6, 1);              // :1041-1046
        avg_chain(dudy - m[0], acc + 9, 1);       // :1050-1061
        avg_chain(dudz, acc + 12, 1);             // :1063-1068
        avg_chain(dvdx, acc + 15, 1);             // :1072-1077
        avg_chain(dvdz, acc + 18, 1);             // :1079-1084
        avg_chain(dwdx, acc + 21, 1);             // :1088-1093
        avg_chain(dwdy - m[2], acc + 24, 1);      // :1095-1106
        const double d = dudx + dvdy + dwdz;                                       // :1110
        acc[27] += (d - m[1]) * (d - m[1]);                                        // :1112
        const double ox = (dwdy - dvdz) - m[3], oy = (dudz - dwdx) - m[4], oz = (dvdx - dudy) - m[5];      // :994, :1001, :1008
        acc[28] += ox * ox; acc[29] += oy * oy; acc[30] += oz * oz;
        const double sxy = dudy + dvdx, sxz = dudz + dwdx, syz = dvdz + dwdy;
        acc[31] += dudx * dudx + dvdy * dvdy + dwdz * dwdz + 0.5 * (sxy * sxy + sxz * sxz + syz * syz) - d * d / 3.0;      // :1136-1137
        const double p = d * AVG_C23;                                              // :1145, :1150, ..
        const double txx = dudx * 2.0 - p, tyy = dvdy * 2.0 - p, tzz = dwdz * 2.0 - p;
        acc[32] += txx * dudx + sxy * dudy + sxz * dudz;                           // :1146
        acc[33] += tyy * dvdy + sxy * dvdx + syz * dvdz;                           // :1151
        acc[34] += tzz * dwdz + syz * dwdy + sxz * dwdx;                           // :1156 (dwdy + dvdz, dwdx + dudz there: the same sums)
        acc[35] += txx * dvdx + sxy * dvdy + sxz * dvdz + tyy * dudy + sxy * dudx + syz * dudz;      // :1161-1162
        acc[36] += txx * dwdx + sxy * dwdy + sxz * dwdz + tzz * dudz + sxz * dudx + syz * dudy;      // :1167-1168
        acc[37] += tyy * dwdy + sxy * dwdx + syz * dwdz + tzz * dvdz + sxz * dvdx + syz * dvdy;      // :1173-1174
    }
};

// fields: the nine gradients, u, v, w (, p).  outputs: Txxy_v Tyyy_v Tzzy_v | Txyy_v Txzy_v Tyzy_v | with p: PIxx PIyy PIzz (raw) | PIxy PIxz PIyz
template <bool P>
struct AvgGradFlow3 {
    static constexpr int NFLD = 12 + (P ? 1 : 0), NMEAN = 6 + (P ? 1 : 0), NOUT = 6 + (P ? 6 : 0), ROWS = 1;
    static constexpr const char *TAG = "k_plane_partial<GRAD_FLOW3>";
    static __host__ __device__ __forceinline__ void add(const double *g, const double *m, double *acc) {
        const double dudx = g[0], dudy = g[1], dvdx = g[3], dvdy = g[4], dvdz = g[5], dwdy = g[7], dwdz = g[8];
        const double t22 = ((dvdy * 2.0 - dudx - dwdz) - m[0]) * AVG_C23;          // :1185
        const double t12 = (dudy + dvdx) - m[1], t23 = (dvdz + dwdy) - m[2];       // :1193, :1201
        const double u = g[9] - m[3], v = g[10] - m[4], w = g[11] - m[5];
        acc[0] += t12 * u; acc[1] += t22 * v; acc[2] += t23 * w;                   // :1212, :1219, :1226
        acc[3] += t22 * u + t12 * v;                                               // :1233
        acc[4] += t23 * u + t12 * w;                                               // :1239
        acc[5] += t23 * v + t22 * w;                                               // :1245
        if constexpr (P) {
            const double dudz = g[2], dwdx = g[6], p = g[12] - m[6];               // dvdz of :640
            acc[6] += p * dudx; acc[7] += p * dvdy; acc[8] += p * dwdz;            // :681-683
            acc[9] += p * (dudy + dvdx); acc[10] += p * (dudz + dwdx); acc[11] += p * (dvdz + dwdy);      // :697-699
        }
    }
};

// fields: u v w dpdx dpdy dpdz
struct AvgUGradP {
    static constexpr int NFLD = 6, NMEAN = 0, NOUT = 1, ROWS = 2;
    static constexpr const char *TAG = "k_plane_partial<UGRADP>";
    static __host__ __device__ __forceinline__ void add(const double *x, const double *, double *acc) {
        acc[0] += x[0] * x[3] + x[1] * x[4] + x[2] * x[5];                         // :673
    }
};

// fields: dsdx dsdy dsdz; mean rS_y.  outputs: Fy Ess (raw) | S_x2 S_y2 S_z2 | S_x3 S_y3 S_z3 | S_x4 S_y4 S_z4
struct AvgGradScal1 {
    static constexpr int NFLD = 3, NMEAN = 1, NOUT = 11, ROWS = 4;
    static constexpr const char *TAG = "k_plane_partial<GRAD_SCAL1>";
    static __host__ __device__ __forceinline__ void add(const double *x, const double *m, double *acc) {
        const double dsdx = x[0], dsdy = x[1], dsdz = x[2];
        acc[0] += dsdy;                                                            // avg_scal_xz.f90:738
        acc[1] += dsdx * dsdx + dsdy * dsdy + dsdz * dsdz;                         // :607
        avg_chain(dsdx, acc + 2, 3);                                               // :714-733
        avg_chain(dsdy - m[0], acc + 3, 3);
        avg_chain(dsdz, acc + 4, 3);
    }
};

// fields: dsdy s u v w (, p dsdx dsdz); means Fy fS fU fV fW (, rP fS_y).  outputs: Tssy2 (raw) | Tsuy2_d Tsvy2_d Tswy2_d | with p: PIsu PIsv PIsw
template <bool P>
struct AvgGradScal2 {
    static constexpr int NFLD = 5 + (P ? 3 : 0), NMEAN = 5 + (P ? 2 : 0), NOUT = 4 + (P ? 3 : 0), ROWS = P ? 2 : 3;
    static constexpr const char *TAG = "k_plane_partial<GRAD_SCAL2>";
    static __host__ __device__ __forceinline__ void add(const double *x, const double *m, double *acc) {
        const double f = x[0] - m[0];
        acc[0] += f * (x[1] - m[1]);                                               // :742
        acc[1] += f * (x[2] - m[2]); acc[2] += f * (x[3] - m[3]); acc[3] += f * (x[4] - m[4]);      // :743-745
        if constexpr (P) {
            const double p = x[5] - m[5];
            acc[4] += p * x[6]; acc[5] += p * (x[0] - m[6]); acc[6] += p * x[7];   // :451-453
        }
    }
};

// fields: a b.  outputs: a*b | a*a | b*b -- the three COV2V2D (utils/averages.f90:244-267) that tools/statistics/spectra.f90:624-628 takes of a pair,
// in one pass over the two fields
struct AvgCov2 {
    static constexpr int NFLD = 2, NMEAN = 0, NOUT = 3, ROWS = 4;
    static constexpr const char *TAG = "k_plane_partial<COV2>";
    static __host__ __device__ __forceinline__ void add(const double *x, const double *, double *acc) {
        acc[0] += x[0] * x[1]; acc[1] += x[0] * x[0]; acc[2] += x[1] * x[1];
    }
};

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
    case AVG_PROG_GRAD_FLOW1: fn(AvgGradFlow1{}); return true;
    case AVG_PROG_GRAD_FLOW2: fn(AvgGradFlow2{}); return true;
    case AVG_PROG_GRAD_FLOW3:
        if (param) fn(AvgGradFlow3<true>{}); else fn(AvgGradFlow3<false>{});
        return true;
    case AVG_PROG_UGRADP: fn(AvgUGradP{}); return true;
    case AVG_PROG_GRAD_SCAL1: fn(AvgGradScal1{}); return true;
    case AVG_PROG_GRAD_SCAL2:
        if (param) fn(AvgGradScal2<true>{}); else fn(AvgGradScal2<false>{});
        return true;
    case AVG_PROG_COV2: fn(AvgCov2{}); return true;
    }
    return false;
}

struct AvgInfo { int nfld, nmean, nout; };
// param: the number of fields (MEANS), imom (POWER), 1 with a pressure field (FLOW, SCAL, GRAD_FLOW3, GRAD_SCAL2), ignored otherwise; zeros when
// there is no such program
inline AvgInfo avg_info(int prog, int param) {
    AvgInfo r{0, 0, 0};
    avg_dispatch(prog, param, [&](auto P) { using T = decltype(P); r = AvgInfo{T::NFLD, T::NMEAN, T::NOUT}; });
    return r;
}

}  // namespace tlab
