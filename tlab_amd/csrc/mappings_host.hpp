// Field mappings (mappings.hip, mappings.cpp): what the kernel k_gradient_maps and the host loop of tlab_gradient_maps share -- the maps, the
// inputs each one reads, its outputs, and the arithmetic of one point, every operation as mappings/fi_vectorcalculus.f90, fi_strain.f90,
// fi_vorticity.f90 and fi_gradient.f90 write it (left-to-right products, no fused multiply-add, IEEE divisions) -- and the launches.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tlab_amd.h"

#pragma clang fp contract(off)      // every operation below stays as written

namespace tlab {

constexpr int MAP_COUNT = 12;       // the TLAB_MAP_* codes of tlab_amd_mappings.h are 0 .. MAP_COUNT - 1
constexpr int MAP_INPUTS = 12;      // u,x u,y u,z v,x v,y v,z w,x w,y w,z s,x s,y s,z
constexpr int MAP_OUTPUTS = 22;     // all maps in one call
enum : int { M_P, M_Q, M_R, M_STRAIN, M_STRAIN_TENSOR, M_CURL, M_VORTICITY, M_VORTICITY_PRODUCTION, M_STRAIN_PRODUCTION, M_GRADIENT,
             M_GRADIENT_PRODUCTION, M_STRAIN_A };

// outputs of a map, the first of them among the 22, and the inputs it reads (bit i: input i)
constexpr int MAP_NOUT[MAP_COUNT] = {1, 1, 1, 1, 6, 4, 1, 1, 1, 1, 1, 3};
constexpr int MAP_FIRST[MAP_COUNT] = {0, 1, 2, 3, 4, 10, 14, 15, 16, 17, 18, 19};
constexpr unsigned MAP_DU = 0x1ffu, MAP_DS = 0xe00u, MAP_OFFDIAG = 0x0eeu, MAP_DIAG = 0x111u;
constexpr unsigned MAP_NEEDS[MAP_COUNT] = {MAP_DIAG, MAP_DU, MAP_DU, MAP_DU, MAP_DU, MAP_OFFDIAG, MAP_OFFDIAG, MAP_DU, MAP_DU, MAP_DS,
                                           MAP_DU | MAP_DS, MAP_DU | MAP_DS};

// One call: in[i] is read only where bit i of `needs` is set, out[MAP_FIRST[m] + k] is written only where bit m of `maps` is set.
struct GradientMapArgs {
    const double *in[MAP_INPUTS];
    double *out[MAP_OUTPUTS];
    unsigned maps, needs;
};

// The maps `maps` of one point: g the twelve gradients (those not needed are not read), o the 22 outputs (those not asked for are not written).
// A map's operations do not depend on which others are computed: no value is shared that the reference computes differently.
__host__ __device__ __forceinline__ void gradient_maps_point(unsigned maps, const double *g, double *o) {
    const double ux = g[0], uy = g[1], uz = g[2], vx = g[3], vy = g[4], vz = g[5], wx = g[6], wy = g[7], wz = g[8];
    const double sx = g[9], sy = g[10], sz = g[11];
    if (maps >> M_P & 1u) o[0] = -((ux + vy) + wz);                                    // fi_vectorcalculus.f90:129-135
    if (maps >> M_Q & 1u) {                                                            // :199-220
        double r = (ux * vy + vy * wz) + wz * ux;
        r = r - vx * uy;
        r = r - wx * uz;
        r = r - wy * vz;
        o[1] = r;
    }
    if (maps >> M_R & 1u) {                                                            // :244-267
        double r = ux * (wz * vy - wy * vz);
        r = r + vx * (wy * uz - wz * uy);
        r = r + wx * (vz * uy - vy * uz);
        o[2] = -r;
    }
    if (maps >> M_STRAIN & 1u) {                                                       // fi_strain.f90:76-96
        double r = ux * ux + vy * vy;
        r = r + wz * wz;
        r = r + (0.5 * (vx + uy)) * (vx + uy);
        r = r + (0.5 * (wx + uz)) * (wx + uz);
        r = r + (0.5 * (wy + vz)) * (wy + vz);
        o[3] = r;
    }
    if (maps >> M_STRAIN_TENSOR & 1u) {                                                // :41-58
        o[4] = ux; o[5] = vy; o[6] = wz;
        o[7] = 0.5 * (uy + vx);
        o[8] = 0.5 * (uz + wx);
        o[9] = 0.5 * (vz + wy);
    }
    const double vort_z = vx - uy, vort_y = uz - wx, vort_x = wy - vz;                 // fi_vorticity.f90:75-87, fi_vectorcalculus.f90:35-47
    if (maps >> M_CURL & 1u) {
        o[10] = vort_x; o[11] = vort_y; o[12] = vort_z;
        o[13] = (vort_x * vort_x + vort_y * vort_y) + vort_z * vort_z;                 // :49
    }
    if (maps >> M_VORTICITY & 1u) o[14] = (vort_z * vort_z + vort_y * vort_y) + vort_x * vort_x;      // fi_vorticity.f90:41-51
    if (maps & (1u << M_VORTICITY_PRODUCTION | 1u << M_STRAIN_PRODUCTION)) {           // :93-113
        double r = (ux * vort_x) * vort_x + (vy * vort_y) * vort_y;
        r = r + (wz * vort_z) * vort_z;
        r = r + ((vx + uy) * vort_x) * vort_y;
        r = r + ((wx + uz) * vort_x) * vort_z;
        r = r + ((wy + vz) * vort_y) * vort_z;
        if (maps >> M_VORTICITY_PRODUCTION & 1u) o[15] = r;
        if (maps >> M_STRAIN_PRODUCTION & 1u) {                                        // fi_strain.f90:124-160
            r = 0.25 * r;
            const double s12 = 0.5 * (vx + uy), s13 = 0.5 * (wx + uz), s23 = 0.5 * (wy + vz);
            r = r + ((2.0 * s12) * s13) * s23;
            r = r + ux * (ux * ux + 3.0 * (s12 * s12 + s13 * s13));
            r = r + vy * (vy * vy + 3.0 * (s12 * s12 + s23 * s23));
            r = r + wz * (wz * wz + 3.0 * (s13 * s13 + s23 * s23));
            o[16] = -r;
        }
    }
    if (maps >> M_GRADIENT & 1u) o[17] = (sx * sx + sy * sy) + sz * sz;                 // fi_gradient.f90:36-40
    if (maps >> M_GRADIENT_PRODUCTION & 1u) {                                          // :71-91
        double r = (ux * sx) * sx + (vy * sy) * sy;
        r = r + (wz * sz) * sz;
        r = r + ((vx + uy) * sx) * sy;
        r = r + ((wx + uz) * sx) * sz;
        o[18] = -(r + ((wy + vz) * sy) * sz);
    }
    if (maps >> M_STRAIN_A & 1u) {                                                     // fi_strain.f90:326-359
        double r = (sx * ux) * sx;
        r = r + (sy * uy) * sx;
        r = r + (sz * uz) * sx;
        r = r + (sx * vx) * sy;
        r = r + (sy * vy) * sy;
        r = r + (sz * vz) * sy;
        r = r + (sx * wx) * sz;
        r = r + (sy * wy) * sz;
        r = r + (sz * wz) * sz;
        const double gg = (sx * sx + sy * sy) + sz * sz;
        o[19] = r;
        o[20] = gg > 0.0 ? r / gg : r;
        o[21] = gg;
    }
}

// mappings.hip.  Nothing is copied or synchronised.
//   launch_gradient_maps  k_gradient_maps on n points; 16-byte accesses when every array of the call is 16-byte aligned
//   launch_acc_prod3      r = [r +] (c f) ((t1 + t2) + t3)       acc != 0: accumulate
//   launch_acc_prod2      r = [r +] a (b [+ c])                  c may be NULL
// gradient_maps_grid: the workgroups of a launch of v points per thread (the grid-stride loop makes a second trip above GRADIENT_MAPS_MAX_BLOCKS)
constexpr int GRADIENT_MAPS_MAX_BLOCKS = 2048, GRADIENT_MAPS_THREADS = 256;
hipError_t launch_gradient_maps(const GradientMapArgs &A, long long n, hipStream_t st);
hipError_t launch_acc_prod3(double *r, double c, const double *f, const double *t1, const double *t2, const double *t3, int acc, long long n,
                            hipStream_t st);
hipError_t launch_acc_prod2(double *r, const double *a, const double *b, const double *c, int acc, long long n, hipStream_t st);

}  // namespace tlab
