// Lagrangian particles of the single-domain driver: TIME_SUBSTEP_PARTICLE (tools/dns/time.f90:906-1070, serial branch :1014-1036) with RHS_PART_1
// (tools/dns/rhs_part_1.f90:43-54, :112-123), FIELD_TO_PARTICLE / Interpolate_Inside_Zones (particles/particle_interpolate.f90:186-332), LOCATE_Y
// (utils/locate_y.f90) and the low-storage scaling of l_hq (time.f90:300-304) as ONE launch per substep, one thread per particle, everything of a
// particle in registers (k_particle_substep); and a permutation of the particle arrays by cell that keeps the gathers of a wave on few cache lines
// (tlab_dns_particle_sort).  Tracers and inertial particles; the bilinear cloud droplets are refused.  With the same weights and corners: the
// sample of any fields (k_particle_sample), the trajectories of the tracked tags (k_particle_trajectories) and the deposit of a particle property
// onto the grid (PARTICLE_TO_FIELD, particles/particle_to_field.f90; k_particle_deposit).
//
// What differs from the reference, and why the values do not:
//   * no halo zones, no Sort_Into_Grid / Sort_Into_Halos: those exist to reach f(1) from the last cell of a periodic direction; here the upper corner
//     of that cell is index 0 (i1 = i0 + 1 == nx ? 0 : i0 + 1).  A particle exactly at x = scale is not wrapped by the reference: its fraction is 0
//     and it takes f(nx) from the halo; here i0 is clamped to nx - 1, which gives the same value and never indexes outside the field.  The same in z.
//   * nz == 1 is the reference's bilinear branch (:291-327): z is neither interpolated nor wrapped, and the third velocity is interpolated in the
//     plane like the others.
//   * l_txc of the inertial particles (the zeroed target of the interpolation) is three registers.
//   * i0, k0 are also clamped from below and nodes(p) to 1 .. ny - 1: no position or node number a host hands over can take a load outside the
//     fields (the reference would read out of bounds there).  On valid input the clamps change nothing.
// Arithmetic: the reference's expressions in its order, multiplies and adds not contracted (the pragma below), so that the numpy restatement
// (tests/particles_oracle.py) gives the same bits.  The divisions are IEEE divisions.
// Access form: per-lane 8-byte loads of the eight corners of three fields; i0 and i1 are neighbours in memory except at the seam.  Unsorted, the 64
// lanes of a wave touch 64 different rows; after tlab_dns_particle_sort they share a few.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "driver_common.hpp"
#include "particles_host.hpp"
#include "plan.hpp"
#include "profile.hpp"

#pragma clang fp contract(off)      // every multiply and add below stays as written

namespace tlab {

// [Particles] of one driver (tlab_dns_set_particles); y: the nodes of the driver's y plan on the device, written when the particles are set
// traj_tags, traj_slot: the tracked tags sorted, and the row j (1-based) of each in l_traj (tlab_dns_set_trajectories)
struct ParticleState {
    int type = TLAB_PART_NONE, bcs = TLAB_PART_BCS_NONE;
    double stokes = 0.0, settling = 0.0;
    double *y = nullptr;
    long long *traj_tags = nullptr;
    int *traj_slot = nullptr;
    int ntraj = 0;
    void drop_trajectories() {
        if (traj_tags) (void)hipFree(traj_tags);
        if (traj_slot) (void)hipFree(traj_slot);
        traj_tags = nullptr; traj_slot = nullptr; ntraj = 0;
    }
    ~ParticleState() {
        if (y) (void)hipFree(y);
        drop_trajectories();
    }
};

namespace {

struct ParticleGrid {
    const double *y;                  // ny nodes
    double dxi, dzi;                  // g(1)%size / g(1)%scale, g(3)%size / g(3)%scale
    double x0, xr, sx, z0, zr, sz;    // x%nodes(1), x%nodes(1) + x%scale, x%scale; the same for z
    double y0, yr;                    // y%nodes(1), y%nodes(1) + y%scale
    int nx, ny, nz;
};
struct ParticleArgs {
    ParticleGrid g;
    const double *q[3];
    double *lq[6], *lh[6];
    int *nodes;
    double dte, kco, ist, sst;        // 1 / stokes, settling / stokes
    int scale;
    unsigned np;
};

// LOCATE_Y (utils/locate_y.f90:13-22), the reference's own bisection with its 1-based jm, jp, jc: the answer for a particle on a node or outside
// [y(1), y(ny)] depends on this path.  jc < jp throughout, so 1 <= jc <= ny - 1 and y(jc + 1) exists; the interval shrinks every turn.
__device__ __forceinline__ int locate_y(double yp, const double *y, int ny) {
    int jp = ny, jm = 1, jc = (jm + jp) / 2;
    while ((yp - y[jc - 1]) * (yp - y[jc]) > 0.0 && jc > jm) {
        if (yp < y[jc - 1]) jp = jc;
        else jm = jc;
        jc = (jm + jp) / 2;
    }
    return jc;
}

// the cell of a position along a periodic direction (particle_interpolate.f90:239-248): 0-based lower corner, clamped into the field, and the
// fraction from the UNclamped floor
__device__ __forceinline__ int cell_of(double xp, double dinv, int n, double &frac) {
    const double a = xp * dinv, fl = floor(a);
    frac = a - fl;
    return fl >= (double)(n - 1) ? n - 1 : (fl > 0.0 ? (int)fl : 0);      // (a NaN compares false twice: cell 0)
}

struct Corners {
    unsigned o00, o01, o11, o10;      // (i0, j0), (i0, j1), (i1, j1), (i1, j0) of plane k0
    unsigned dk;                      // k1 plane - k0 plane as an offset modulo 2^32 (the seam makes it negative)
    double c1, c2, c3, c4, l5, l6;
};
// data_out + A + B of particle_interpolate.f90:277-285 (3-D) and :320-324 (2-D), left to right
template <bool D3>
__device__ __forceinline__ double interpolate(const double *f, const Corners &c, double target) {
    const double a = ((c.c3 * f[c.o00] + c.c4 * f[c.o01]) + c.c1 * f[c.o11]) + c.c2 * f[c.o10];
    if constexpr (!D3) return target + a;
    else {
        const double b = ((c.c3 * f[c.o00 + c.dk] + c.c4 * f[c.o01 + c.dk]) + c.c1 * f[c.o11 + c.dk]) + c.c2 * f[c.o10 + c.dk];
        return (target + a * c.l6) + b * c.l5;
    }
}

// the weights and corners of a particle at (xp, yp, zp) with the node below it (particle_interpolate.f90:239-269; particle_to_field.f90:91-123 forms
// the same numbers); o00 is the number of the cell.  xseam / zseam: the upper corners in x / z are the wrapped ones (index 0).
struct Seam {
    bool x, z;
};
template <bool D3>
__device__ __forceinline__ Seam corners_of(const ParticleGrid &G, double xp, double yp, double zp, int node, Corners &c) {
    double l1, l5 = 0.0;
    const int i0 = cell_of(xp, G.dxi, G.nx, l1);
    const int i1 = i0 + 1 == G.nx ? 0 : i0 + 1;
    const double l2 = 1.0 - l1;
    int k0 = 0, k1 = 0;
    if constexpr (D3) {
        k0 = cell_of(zp, G.dzi, G.nz, l5);
        k1 = k0 + 1 == G.nz ? 0 : k0 + 1;
    }
    c.l5 = l5;
    c.l6 = 1.0 - l5;
    int j0 = node - 1;
    j0 = j0 < 0 ? 0 : (j0 > G.ny - 2 ? G.ny - 2 : j0);
    const double l3 = (yp - G.y[j0]) / (G.y[j0 + 1] - G.y[j0]), l4 = 1.0 - l3;
    c.c1 = l1 * l3; c.c2 = l1 * l4; c.c3 = l4 * l2; c.c4 = l2 * l3;
    const unsigned row0 = ((unsigned)k0 * G.ny + j0) * G.nx, row1 = row0 + G.nx;
    c.o00 = row0 + i0; c.o01 = row1 + i0; c.o11 = row1 + i1; c.o10 = row0 + i1;
    c.dk = ((unsigned)k1 - (unsigned)k0) * ((unsigned)G.ny * G.nx);
    return Seam{i1 == 0, D3 && k1 == 0};
}

// TYPE: TLAB_PART_TRACER / _INERTIA; BCS: TLAB_PART_BCS_*; D3: nz > 1.  Steps 1-7 of the header's list, one particle per thread.
template <int TYPE, int BCS, bool D3>
__global__ void __launch_bounds__(256) k_particle_substep(ParticleArgs A) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.np) return;
    constexpr int NC = TYPE == TLAB_PART_INERTIA ? 6 : 3;
    const ParticleGrid &G = A.g;
    double lq[NC], lh[NC];
    for (int is = 0; is < NC; ++is) { lq[is] = A.lq[is][p]; lh[is] = A.lh[is][p]; }

    // 1. the weights and corners (particle_interpolate.f90:239-269)
    Corners c;
    (void)corners_of<D3>(G, lq[0], lq[1], lq[2], A.nodes[p], c);

    // 2. the equations (rhs_part_1.f90:43-54, :112-123)
    if constexpr (TYPE == TLAB_PART_TRACER) {
        for (int i = 0; i < 3; ++i) lh[i] = interpolate<D3>(A.q[i], c, lh[i]);
    } else {
        double ui[3];
        for (int i = 0; i < 3; ++i) ui[i] = interpolate<D3>(A.q[i], c, 0.0);
        for (int i = 0; i < 3; ++i) lh[i] = lh[i] + lq[3 + i];
        lh[3] = lh[3] + A.ist * (ui[0] - lq[3]);
        lh[4] = lh[4] + A.ist * (ui[1] - lq[4]) - A.sst;
        lh[5] = lh[5] + A.ist * (ui[2] - lq[5]);
    }

    // 3. the update (time.f90:926-928)
    for (int is = 0; is < NC; ++is) lq[is] = lq[is] + A.dte * lh[is];

    // 4. periodic wraps, one at most (time.f90:1019-1036)
    if (lq[0] > G.xr) lq[0] = lq[0] - G.sx;
    else if (lq[0] < G.x0) lq[0] = lq[0] + G.sx;
    if constexpr (D3) {
        if (lq[2] > G.zr) lq[2] = lq[2] - G.sz;
        else if (lq[2] < G.z0) lq[2] = lq[2] + G.sz;
    }

    // 5. the walls (time.f90:1040-1062); a tracer has no fifth column to flip
    if constexpr (BCS == TLAB_PART_BCS_SPECULAR) {
        if (lq[1] > G.yr) {
            lq[1] = 2.0 * G.yr - lq[1];
            if constexpr (NC == 6) lq[4] = -lq[4];
        } else if (lq[1] < G.y0) {
            lq[1] = 2.0 * G.y0 - lq[1];
            if constexpr (NC == 6) lq[4] = -lq[4];
        }
    } else if constexpr (BCS == TLAB_PART_BCS_STICK) {
        if (lq[1] > G.yr) lq[1] = G.yr;
        else if (lq[1] < G.y0) lq[1] = G.y0;
    }

    // 6. the node below (time.f90:1067), 7. the tendencies of the next substep (time.f90:300-304)
    A.nodes[p] = locate_y(lq[1], G.y, G.ny);
    for (int is = 0; is < NC; ++is) {
        A.lq[is][p] = lq[is];
        A.lh[is][p] = A.scale ? lh[is] * A.kco : lh[is];
    }
}

__global__ void __launch_bounds__(256) k_particle_locate(const double *yp, int *nodes, const double *y, int ny, unsigned np) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < np) nodes[p] = locate_y(yp[p], y, ny);
}

// the sort key: the number of the cell, (k0 ny + j0) nx + i0 with the corners of step 1, and the particle's number as the payload
template <bool D3>
__global__ void __launch_bounds__(256) k_particle_keys(const double *xp, const double *zp, const int *nodes, ParticleGrid G, unsigned *keys,
                                                       unsigned *idx, unsigned np) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    double fr;
    const int i0 = cell_of(xp[p], G.dxi, G.nx, fr);
    int k0 = 0;
    if constexpr (D3) k0 = cell_of(zp[p], G.dzi, G.nz, fr);
    int j0 = nodes[p] - 1;
    j0 = j0 < 0 ? 0 : (j0 > G.ny - 2 ? G.ny - 2 : j0);
    keys[p] = ((unsigned)k0 * G.ny + j0) * G.nx + i0;
    idx[p] = p;
}

template <class T>
__global__ void __launch_bounds__(256) k_particle_gather(const T *a, const unsigned *idx, T *out, unsigned np) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < np) out[p] = a[idx[p]];
}

// ---- the transfers between particles and fields: FIELD_TO_PARTICLE of any fields, ParticleTrajectories_Accumulate, PARTICLE_TO_FIELD ----
// what the three kernels share: the grid, the position columns, the nodes
struct TransferArgs {
    ParticleGrid g;
    const double *x, *y, *z;
    const int *nodes;
    unsigned np;
};
struct FieldList {
    const double *f[PARTICLE_FIELDS_PER_LAUNCH];
    int n;
};
struct TargetList {
    double *o[PARTICLE_FIELDS_PER_LAUNCH];
};

// FIELD_TO_PARTICLE (particle_interpolate.f90:186-332) of F.n fields: out = out + A (+ B), the weights formed once per particle
template <bool D3>
__global__ void __launch_bounds__(256) k_particle_sample(TransferArgs A, FieldList F, TargetList O) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.np) return;
    Corners c;
    (void)corners_of<D3>(A.g, A.x[p], A.y[p], A.z[p], A.nodes[p], c);
    for (int v = 0; v < F.n; ++v) O.o[v][p] = interpolate<D3>(F.f[v], c, O.o[v][p]);
}

// ParticleTrajectories_Accumulate (particle_trajectories.f90:205-227) for column `col` of l_traj(rows, nsave, *): the time in row 1, and for a
// particle whose tag is tracked the nq prognostic columns (variables 0 .. nq - 1) and the F.n fields at the particle (variables ivf ..), in fp32.
// The reference's double loop over particles and tags is a bisection in the sorted table; only the lanes that find their tag interpolate.
struct TrajArgs {
    const double *lq[6];
    const long long *tags, *ttags;
    const int *tslot;
    float *traj;
    size_t rows, nsave, col;
    float rtime;
    int nq, ivf, ntraj;
};
template <bool D3>
__global__ void __launch_bounds__(256) k_particle_trajectories(TransferArgs A, TrajArgs R, FieldList F) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    auto at = [&](size_t row, int iv) -> float & { return R.traj[row + R.rows * (R.col + R.nsave * (size_t)iv)]; };
    if (blockIdx.x == 0 && (int)threadIdx.x < R.nq + F.n) {
        const int t = (int)threadIdx.x;
        at(0, t < R.nq ? t : R.ivf + (t - R.nq)) = R.rtime;
    }
    if (p >= A.np) return;
    const long long tag = R.tags[p];
    int lo = 0, hi = R.ntraj;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (R.ttags[mid] < tag) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= R.ntraj || R.ttags[lo] != tag) return;
    const size_t row = (size_t)R.tslot[lo];
    for (int is = 0; is < R.nq; ++is) at(row, is) = (float)R.lq[is][p];
    if (F.n > 0) {
        Corners c;
        (void)corners_of<D3>(A.g, A.x[p], A.y[p], A.z[p], A.nodes[p], c);
        for (int v = 0; v < F.n; ++v) at(row, R.ivf + v) = (float)interpolate<D3>(F.f[v], c, 0.0);
    }
}

// PARTICLE_TO_FIELD_INTERPOLATE (particle_to_field.f90:89-151): property cube length, the products of :131-147 in that order, added to the eight
// (nz == 1: four) corners by no-return fp64 atomic adds at agent scope (global_atomic_add_f64: the fields are plain device allocations).  The
// reference's array has a column nx + 1 and a plane nz + 1 for the upper corners of the seam cells; here those go to index 0 (periodic) or nowhere.
// Particles of adjacent lanes in the same cell (what tlab_dns_particle_sort leaves) are summed in the wave first, a segmented sum by lane shuffles
// over runs of equal cell numbers, and the first lane of a run issues the run's adds.  This reorders the sum, as the atomics do.  Measured against
// the kernel without it (512^3, sorted tracers): 3.7 / 6.0 / 6.6 ms against 4.1 / 11.2 / 25.6 ms at np = 2^24 / 2^26 / 2^27,
// the same time unsorted (a wave without a run of two skips the shuffles).
template <bool D3>
__global__ void __launch_bounds__(256) k_particle_deposit(TransferArgs A, const double *prop, int periodic, double *field) {
    constexpr int NW = D3 ? 8 : 4;
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < A.np;
    Corners c = {};
    Seam s = {false, false};
    double w[NW] = {};
    unsigned key = 0xffffffffu;      // (no cell has this number: at most 2^31 - 1 points)
    if (live) {
        s = corners_of<D3>(A.g, A.x[p], A.y[p], A.z[p], A.nodes[p], c);
        const double pr = prop ? prop[p] : 1.0;
        if constexpr (D3) {
            w[0] = pr * c.c3 * c.l6; w[1] = pr * c.c4 * c.l6; w[2] = pr * c.c1 * c.l6; w[3] = pr * c.c2 * c.l6;
            w[4] = pr * c.c3 * c.l5; w[5] = pr * c.c4 * c.l5; w[6] = pr * c.c1 * c.l5; w[7] = pr * c.c2 * c.l5;
        } else {
            w[0] = pr * c.c3; w[1] = pr * c.c4; w[2] = pr * c.c1; w[3] = pr * c.c2;
        }
        key = c.o00;
    }
    bool issue = live;
    {      // every lane of the wave takes part in the shuffles: nobody has left yet
        const unsigned lane = __lane_id();
        const unsigned before = __shfl_up(key, 1);
        const bool head = lane == 0 || before != key;
        const unsigned long long heads = __ballot(head);
        if (heads != ~0ull) {      // (wave-uniform) some run is longer than one lane
            const unsigned long long above = (((heads >> lane) >> 1) << lane) << 1;      // the heads of the runs after mine
            const unsigned end = above ? (unsigned)__builtin_ctzll(above) - 1u : 63u;    // the last lane of my run
            for (unsigned d = 1; d < 64; d <<= 1) {
                const bool take = lane + d <= end;
                for (int i = 0; i < NW; ++i) {
                    const double o = __shfl_down(w[i], d);
                    if (take) w[i] = w[i] + o;
                }
            }
            issue = live && head;
        }
    }
    if (!issue) return;
    auto add = [&](unsigned o, double v) { (void)__hip_atomic_fetch_add(field + o, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    const bool xs = periodic || !s.x, zs = periodic || !s.z;
    add(c.o00, w[0]);
    add(c.o01, w[1]);
    if (xs) { add(c.o11, w[2]); add(c.o10, w[3]); }
    if constexpr (D3) {
        if (zs) {
            add(c.o00 + c.dk, w[4]);
            add(c.o01 + c.dk, w[5]);
            if (xs) { add(c.o11 + c.dk, w[6]); add(c.o10 + c.dk, w[7]); }
        }
    }
}

// g%scale of FDM_CreatePlan (fdm/fdm.f90:162-167)
double plan_scale(const FdmTables &t) {
    if (t.n <= 1) return 1.0;
    double s = t.nodes[t.n - 1] - t.nodes[0];
    if (t.periodic) s = s * (1.0 + 1.0 / (double)(t.n - 1));
    return s;
}

struct Driver {
    tlab_dns_grid g;
    ParticleState *ps;
};
Driver driver_of(tlab_dns_t d, const char *who) {
    if (!d) throw Fail(TLAB_EINVAL, std::string(who) + ": null handle");
    Driver D;
    tlab_internal_dns_grid(d, &D.g);
    D.ps = *D.g.particles;
    return D;
}

ParticleGrid grid_of(const Driver &D) {
    const FdmTables &tx = D.g.g[0]->t, &ty = D.g.g[1]->t, &tz = D.g.g[2]->t;
    ParticleGrid G;
    G.nx = D.g.nx; G.ny = D.g.ny; G.nz = D.g.nz;
    G.y = D.ps->y;
    G.sx = plan_scale(tx); G.sz = plan_scale(tz);
    G.dxi = (double)tx.n / G.sx; G.dzi = (double)tz.n / G.sz;
    G.x0 = tx.nodes[0]; G.xr = G.x0 + G.sx;
    G.z0 = tz.nodes[0]; G.zr = G.z0 + G.sz;
    G.y0 = ty.nodes[0]; G.yr = G.y0 + plan_scale(ty);
    return G;
}

inline dim3 blocks(long long np) { return dim3((unsigned)((np + 255) / 256)); }

template <int TYPE, int BCS>
void launch_substep_d(bool d3, const ParticleArgs &A, hipStream_t st) {
    if (d3) hipLaunchKernelGGL((k_particle_substep<TYPE, BCS, true>), blocks(A.np), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_particle_substep<TYPE, BCS, false>), blocks(A.np), dim3(256), 0, st, A);
}
template <int TYPE>
void launch_substep_b(int bcs, bool d3, const ParticleArgs &A, hipStream_t st) {
    switch (bcs) {
    case TLAB_PART_BCS_STICK: launch_substep_d<TYPE, TLAB_PART_BCS_STICK>(d3, A, st); break;
    case TLAB_PART_BCS_SPECULAR: launch_substep_d<TYPE, TLAB_PART_BCS_SPECULAR>(d3, A, st); break;
    default: launch_substep_d<TYPE, TLAB_PART_BCS_NONE>(d3, A, st); break;
    }
}

void refuse(int rc, const std::string &why) {
    if (rc != TLAB_OK) throw Fail(rc, why);
}

// a driver with particles, or a null state for the checks to refuse
Driver transfer_driver(tlab_dns_t d, const char *who) {
    Driver D = driver_of(d, who);
    if ((long long)D.g.nx * D.g.ny * D.g.nz > 0x7fffffffLL) throw Fail(TLAB_EINVAL, std::string(who) + ": more than 2^31 - 1 points");
    return D;
}
TransferArgs transfer_args(const Driver &D, double *const *l_q, const int *nodes, long long np) {
    TransferArgs A;
    A.g = grid_of(D);
    A.x = l_q[0]; A.y = l_q[1]; A.z = l_q[2];
    A.nodes = nodes;
    A.np = (unsigned)np;
    return A;
}

}  // namespace
}  // namespace tlab

using namespace tlab;

void tlab_internal_particles_free(tlab::ParticleState *p) { delete p; }

extern "C" {

int tlab_dns_set_particles(tlab_dns_t d, int type, int bcs, double stokes, double settling) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        std::string why;
        int code = TLAB_PART_BCS_NONE;
        refuse(particle_check_settings(type, bcs, stokes, settling, &code, why), why);
        Driver D = driver_of(d, "tlab_dns_set_particles");
        if (type == TLAB_PART_NONE) {
            if (D.ps) hk(hipStreamSynchronize(tlab_current_stream()), "sync");      // a launch that reads the y table may be in flight
            delete D.ps;
            *D.g.particles = nullptr;
            return;
        }
        if (D.g.anelastic) throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_set_particles: particles in an anelastic run are not built on the device");
        const FdmTables &tx = D.g.g[0]->t, &ty = D.g.g[1]->t, &tz = D.g.g[2]->t;
        if (D.g.ny < 2 || (int)ty.nodes.size() < D.g.ny || (int)tx.nodes.size() < tx.n || (int)tz.nodes.size() < tz.n || tx.n != D.g.nx || tz.n != D.g.nz)
            throw Fail(TLAB_EINVAL, "tlab_dns_set_particles: the plans of this driver carry no nodes (tlab_fdm_plan_set_aux), or it is a slab of a larger box");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        if (!D.ps) {
            auto ps = std::make_unique<ParticleState>();
            hk(hipMalloc((void **)&ps->y, (size_t)D.g.ny * sizeof(double)), "hipMalloc");
            hk(hipMemcpy(ps->y, ty.nodes.data(), (size_t)D.g.ny * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
            *D.g.particles = D.ps = ps.release();
        }
        D.ps->type = type; D.ps->bcs = code; D.ps->stokes = stokes; D.ps->settling = settling;
    }, TLAB_EINVAL);
}

int tlab_dns_particle_locate(tlab_dns_t d, long long np, const double *y_part, int *nodes) {
    return guarded([&] {
        const char *who = "tlab_dns_particle_locate";
        Driver D = driver_of(d, who);
        if (!D.ps) throw Fail(TLAB_EINVAL, std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)");
        std::string why;
        refuse(particle_check_count(who, np, why), why);
        if (np == 0) return;
        if (!y_part || !nodes) throw Fail(TLAB_EINVAL, std::string(who) + ": null array");
        hipStream_t st = tlab_current_stream();
        ProfScope ps("k_particle_locate", st, 12.0 * (double)np);
        hipLaunchKernelGGL(k_particle_locate, blocks(np), dim3(256), 0, st, y_part, nodes, D.ps->y, D.g.ny, (unsigned)np);
        hk(hipGetLastError(), "k_particle_locate");
    });
}

int tlab_dns_substep_particle(tlab_dns_t d, double dte, double kco, int scale_tendencies, long long np, double *const *q, double *const *l_q,
                              double *const *l_hq, int *nodes) {
    return guarded([&] {
        Driver D = driver_of(d, "tlab_dns_substep_particle");
        const int nc = D.ps ? particle_columns(D.ps->type) : 0;
        std::string why;
        refuse(particle_check_substep(D.ps != nullptr, nc, dte, kco, np, q, l_q, l_hq, nodes, why), why);
        if (np == 0) return;
        if ((long long)D.g.nx * D.g.ny * D.g.nz > 0x7fffffffLL) throw Fail(TLAB_EINVAL, "tlab_dns_substep_particle: more than 2^31 - 1 points");
        ParticleArgs A;
        A.g = grid_of(D);
        for (int i = 0; i < 3; ++i) A.q[i] = q[i];
        for (int i = 0; i < 6; ++i) { A.lq[i] = i < nc ? l_q[i] : nullptr; A.lh[i] = i < nc ? l_hq[i] : nullptr; }
        A.nodes = nodes;
        A.dte = dte; A.kco = kco; A.scale = scale_tendencies ? 1 : 0;
        A.ist = A.sst = 0.0;
        if (D.ps->type == TLAB_PART_INERTIA) { A.ist = 1.0 / D.ps->stokes; A.sst = D.ps->settling / D.ps->stokes; }      // rhs_part_1.f90:116-117
        A.np = (unsigned)np;
        hipStream_t st = tlab_current_stream();
        // algorithmic bytes: l_q, l_hq read and written, nodes read and written, one pass over the three velocities
        ProfScope ps("k_particle_substep", st, (double)np * (2.0 * 8.0 * 2.0 * nc + 8.0) + 3.0 * 8.0 * (double)D.g.nx * D.g.ny * D.g.nz);
        if (D.ps->type == TLAB_PART_INERTIA) launch_substep_b<TLAB_PART_INERTIA>(D.ps->bcs, D.g.nz > 1, A, st);
        else launch_substep_b<TLAB_PART_TRACER>(D.ps->bcs, D.g.nz > 1, A, st);
        hk(hipGetLastError(), "k_particle_substep");
    });
}

int tlab_dns_particle_sort(tlab_dns_t d, long long np, double *const *l_q, double *const *l_hq, int *nodes, long long *tags, void *scratch,
                           long long scratch_bytes, long long *scratch_needed) {
    return guarded([&] {
        const char *who = "tlab_dns_particle_sort";
        Driver D = driver_of(d, who);
        std::string why;
        refuse(particle_check_count(who, np, why), why);
        const long long ncell = (long long)D.g.nx * D.g.ny * D.g.nz;
        if (ncell > 0x7fffffffLL) throw Fail(TLAB_EINVAL, std::string(who) + ": more than 2^31 - 1 points");
        const unsigned bits = particle_key_bits((unsigned long long)ncell);
        hipStream_t st = tlab_current_stream();
        size_t sort_bytes = 0;
        if (np > 0)
            hk(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr,
                                         (size_t)np, 0u, bits, st), "radix sort (size query)");
        ParticleSortLayout L;
        refuse(particle_sort_layout(np, sort_bytes, &L, why), why);
        if (scratch_needed) *scratch_needed = (long long)L.total;
        if (!scratch) {      // the size query
            if (!scratch_needed) throw Fail(TLAB_EINVAL, std::string(who) + ": scratch and scratch_needed are both null");
            return;
        }
        const int nc = D.ps ? particle_columns(D.ps->type) : 0;
        refuse(particle_check_sort(D.ps != nullptr, nc, np, l_q, l_hq, nodes, tags, scratch, scratch_bytes, L.total, why), why);
        if (np == 0) return;
        char *base = static_cast<char *>(scratch);
        unsigned *keys_in = reinterpret_cast<unsigned *>(base + L.keys_in), *keys_out = reinterpret_cast<unsigned *>(base + L.keys_out);
        unsigned *idx_in = reinterpret_cast<unsigned *>(base + L.idx_in), *idx_out = reinterpret_cast<unsigned *>(base + L.idx_out);
        void *column = base + L.column;
        const unsigned n = (unsigned)np;
        const ParticleGrid G = grid_of(D);
        ProfScope ps("particle_sort", st, (double)np * (16.0 * (2 * nc) + 8.0 + 16.0));
        if (D.g.nz > 1) hipLaunchKernelGGL((k_particle_keys<true>), blocks(np), dim3(256), 0, st, l_q[0], l_q[2], nodes, G, keys_in, idx_in, n);
        else hipLaunchKernelGGL((k_particle_keys<false>), blocks(np), dim3(256), 0, st, l_q[0], l_q[2], nodes, G, keys_in, idx_in, n);
        hk(hipGetLastError(), "k_particle_keys");
        size_t have = sort_bytes;
        hk(rocprim::radix_sort_pairs((void *)(base + L.sort), have, keys_in, keys_out, idx_in, idx_out, (size_t)np, 0u, bits, st), "radix sort");
        auto permute = [&](auto *a) {
            using T = std::remove_pointer_t<decltype(a)>;
            hipLaunchKernelGGL((k_particle_gather<T>), blocks(np), dim3(256), 0, st, (const T *)a, idx_out, (T *)column, n);
            hk(hipGetLastError(), "k_particle_gather");
            hk(hipMemcpyAsync(a, column, (size_t)np * sizeof(T), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
        };
        for (int is = 0; is < nc; ++is) { permute(l_q[is]); permute(l_hq[is]); }
        permute(nodes);
        permute(tags);
    });
}

int tlab_dns_field_to_particle(tlab_dns_t d, int nvar, const double *const *fields, long long np, double *const *l_q, const int *nodes,
                               double *const *out) {
    return guarded([&] {
        const char *who = "tlab_dns_field_to_particle";
        Driver D = transfer_driver(d, who);
        std::string why;
        refuse(particle_check_sample(D.ps != nullptr, nvar, fields, np, l_q, nodes, out, why), why);
        if (np == 0) return;
        const TransferArgs A = transfer_args(D, l_q, nodes, np);
        const double npts = (double)D.g.nx * D.g.ny * D.g.nz;
        hipStream_t st = tlab_current_stream();
        for (int v0 = 0; v0 < nvar; v0 += PARTICLE_FIELDS_PER_LAUNCH) {
            FieldList F = {};
            TargetList O = {};
            F.n = nvar - v0 < PARTICLE_FIELDS_PER_LAUNCH ? nvar - v0 : PARTICLE_FIELDS_PER_LAUNCH;
            for (int v = 0; v < F.n; ++v) { F.f[v] = fields[v0 + v]; O.o[v] = out[v0 + v]; }
            // algorithmic bytes: positions and nodes read, the targets read and written, one pass over the fields
            ProfScope ps("k_particle_sample", st, (double)np * (28.0 + 16.0 * F.n) + 8.0 * F.n * npts);
            if (D.g.nz > 1) hipLaunchKernelGGL((k_particle_sample<true>), blocks(np), dim3(256), 0, st, A, F, O);
            else hipLaunchKernelGGL((k_particle_sample<false>), blocks(np), dim3(256), 0, st, A, F, O);
            hk(hipGetLastError(), "k_particle_sample");
        }
    });
}

int tlab_dns_set_trajectories(tlab_dns_t d, long long ntraj, const long long *tags) {
    (void)tlab_internal_deferred_flush();
    return guarded([&] {
        const char *who = "tlab_dns_set_trajectories";
        Driver D = driver_of(d, who);
        std::string why;
        std::vector<std::pair<long long, int>> table;
        refuse(particle_trajectory_table(D.ps != nullptr, ntraj, tags, &table, why), why);
        std::vector<long long> tt(table.size());
        std::vector<int> ts(table.size());
        for (size_t j = 0; j < table.size(); ++j) { tt[j] = table[j].first; ts[j] = table[j].second; }
        hk(hipStreamSynchronize(tlab_current_stream()), "sync");      // a launch that reads the old table may be in flight
        D.ps->drop_trajectories();
        if (ntraj == 0) return;
        hk(hipMalloc((void **)&D.ps->traj_tags, tt.size() * sizeof(long long)), "hipMalloc");
        hk(hipMalloc((void **)&D.ps->traj_slot, ts.size() * sizeof(int)), "hipMalloc");
        hk(hipMemcpy(D.ps->traj_tags, tt.data(), tt.size() * sizeof(long long), hipMemcpyHostToDevice), "hipMemcpy");
        hk(hipMemcpy(D.ps->traj_slot, ts.data(), ts.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
        D.ps->ntraj = (int)ntraj;
    });
}

int tlab_dns_trajectories_accumulate(tlab_dns_t d, double rtime, long long counter, long long nsave, long long np, double *const *l_q,
                                     const int *nodes, const long long *tags, int nvar, const double *const *fields, float *l_traj) {
    return guarded([&] {
        const char *who = "tlab_dns_trajectories_accumulate";
        Driver D = transfer_driver(d, who);
        const int nc = D.ps ? particle_columns(D.ps->type) : 0;
        std::string why;
        refuse(particle_check_trajectories(D.ps != nullptr, nc, D.ps ? D.ps->ntraj : 0, rtime, counter, nsave, np, l_q, nodes, tags, nvar, fields,
                                           l_traj, why), why);
        if (np == 0) return;
        const TransferArgs A = transfer_args(D, l_q, nodes, np);
        TrajArgs R = {};
        for (int i = 0; i < nc; ++i) R.lq[i] = l_q[i];
        R.tags = tags; R.ttags = D.ps->traj_tags; R.tslot = D.ps->traj_slot; R.ntraj = D.ps->ntraj;
        R.traj = l_traj;
        R.rows = (size_t)D.ps->ntraj + 1; R.nsave = (size_t)nsave; R.col = (size_t)(counter - 1);
        R.rtime = (float)rtime;
        hipStream_t st = tlab_current_stream();
        int v0 = 0;
        do {      // (once without fields: the prognostic columns alone)
            FieldList F = {};
            F.n = nvar - v0 < PARTICLE_FIELDS_PER_LAUNCH ? nvar - v0 : PARTICLE_FIELDS_PER_LAUNCH;
            for (int v = 0; v < F.n; ++v) F.f[v] = fields[v0 + v];
            R.nq = v0 == 0 ? nc : 0;
            R.ivf = nc + v0;
            // algorithmic bytes: every tag read; per tracked particle its columns, position, node and eight corners of each field, and the row written
            ProfScope ps("k_particle_trajectories", st, 8.0 * (double)np + (double)D.ps->ntraj * (12.0 * R.nq + 28.0 + 68.0 * F.n));
            if (D.g.nz > 1) hipLaunchKernelGGL((k_particle_trajectories<true>), blocks(np), dim3(256), 0, st, A, R, F);
            else hipLaunchKernelGGL((k_particle_trajectories<false>), blocks(np), dim3(256), 0, st, A, R, F);
            hk(hipGetLastError(), "k_particle_trajectories");
            v0 += PARTICLE_FIELDS_PER_LAUNCH;
        } while (v0 < nvar);
    });
}

int tlab_dns_particle_to_field(tlab_dns_t d, long long np, double *const *l_q, const int *nodes, const double *property, int periodic,
                               double *field) {
    return guarded([&] {
        const char *who = "tlab_dns_particle_to_field";
        Driver D = transfer_driver(d, who);
        std::string why;
        refuse(particle_check_deposit(D.ps != nullptr, np, l_q, nodes, field, why), why);
        const size_t npts = (size_t)D.g.nx * D.g.ny * D.g.nz;
        hipStream_t st = tlab_current_stream();
        hk(hipMemsetAsync(field, 0, npts * sizeof(double), st), "hipMemsetAsync");      // wrk3d = 0 (particle_to_field.f90:33)
        if (np == 0) return;
        const TransferArgs A = transfer_args(D, l_q, nodes, np);
        const int per = periodic ? 1 : 0;
        // algorithmic bytes: positions, nodes and the property read, eight 8-byte adds per particle
        ProfScope ps("k_particle_deposit", st, (double)np * (28.0 + (property ? 8.0 : 0.0) + (D.g.nz > 1 ? 64.0 : 32.0)));
        if (D.g.nz > 1) hipLaunchKernelGGL((k_particle_deposit<true>), blocks(np), dim3(256), 0, st, A, property, per, field);
        else hipLaunchKernelGGL((k_particle_deposit<false>), blocks(np), dim3(256), 0, st, A, property, per, field);
        hk(hipGetLastError(), "k_particle_deposit");
    });
}

}  // extern "C"
