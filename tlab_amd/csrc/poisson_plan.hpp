// What the translation units of the Poisson solver share on the host side: poisson.hip (plan, transforms, marching-route stages, C entry points),
// poisson_int1.hip (k_int1, k_int1g), poisson_ode.hip (k_ode_nn, k_ode_sing and their tables), poisson_direct.hip (k_int2, k_int2c).  The library is
// built without relocatable device code, so a kernel lives in the file that launches it; this header holds the plan object, the argument structs
// that cross files, the declarations of what those files call in each other, and the small host helpers all of them use.  For these four files only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tlab_amd.h"
#include "errors.hpp"
#include "internal.hpp"
#include "plan.hpp"
#include "fftz.hpp"
#include "poisson_host.hpp"
#include "int1_generic.hpp"
#include "profile.hpp"

namespace tlab {

constexpr int OM = 8;   // rows per thread of the chunked kernels (k_ode_nn, k_ode_sing, k_int2c)

// ------------------------------------------------------------------------------------------------
// device tables
// ------------------------------------------------------------------------------------------------
struct Int1Dev {
    const double *L0, *L1, *R;   // row-major [n][5], [n][5], [n][3]
    double rb[3][4], rt[3][4];
    int n;
};

enum { FS_FIELD = 0, FS_LINEAR = 1, FS_UNIT = 2 };

struct Int1Args {
    Int1Dev T;
    const double *lam;      // [nm] |lambda| of each mode; the kernel applies the sign of its system
    double lam_sign;        // +1 (BCS_MIN system) or -1 (BCS_MAX system)
    long long nm;           // number of modes handled (threads)
    // f source
    const double *fsrc;     // FS_FIELD: complex field (nxh, ny, nz); FS_LINEAR: SoA [(l*n + j)*nm + t]
    int nlf;                // FS_LINEAR: number of stored lines (lines >= nlf are zero)
    int unit_row;           // FS_UNIT: row of the unit entry of line 0
    double fscale;          // FS_FIELD: normalisation 1/(nx*nz) folded into the load (opr_elliptic.f90:295)
    int nxh, ny;            // FS_FIELD layout
    int zero_bsave;         // 1: the f value saved as "opposite boundary value" is zero (f(:,nx)=0 / f(:,1)=0 in the callers)
    // given boundary value per line: constants, or per-mode array [(l*nm) + t] if bv_ptr != NULL
    double bv[3];
    const double *bv_ptr;
    // outputs
    double *scratch;        // SoA [(k*n + j)*nm + t], k < NL + 3
    double *dst;            // SoA [(l*n + j)*nm + t]
    double *du;             // [(l*nm) + t] or NULL
    double *bcs_save;       // FS_FIELD only: [(c*nm + t)], c = 0..3 = Re/Im at the bottom, Re/Im at the top (BC data)
    // LU factors of the modes, SoA [(k*n + j)*nm + t], k = 0..4 = a, b (forward), 1/c, -d, -e (backward), exactly as the elimination of k_int1
    // produces them: fac_out != NULL stores them (plan creation of the low-mode sub-plan), fac != NULL reads them instead of eliminating
    // (its per-call solves: the chain of dependent divisions is what a handful of marching threads spends its time on)
    double *fac_out;
    const double *fac;
    int fpart;              // SPLIT launches of k_int1 (one line per thread): which component of the complex FS_FIELD source this thread takes
    // 3- / 7-diagonal integral systems (int1_generic.cpp): everything factorized on the host, per mode -- g_fac [ndi][n][nm] (rows 2..n-1: the factors
    // of TRIDFS / HEPTADFS; rows 1, n: the reduced boundary rows), g_rb / g_rt [40][nm] (rhs_b(1:5, 0:7), rhs_t(0:4, 1:8)), g_R [n][nri].  g_fac != NULL
    // sends launch_int1 to k_int1g.
    const double *g_fac, *g_rb, *g_rt, *g_R;
    int g_ndi, g_nri;
};

struct OdeSys {                  // Int1Dev without the by-value boundary constants (they would sit in ~100 SGPRs)
    const double *L0, *L1, *R;   // row-major [n][5], [n][5], [n][3]
    const double *pk;            // the same numbers packed per row, [n][16] = L0[5], L1[5], row scale, R[3], 0, 0: one 128-B line and seven 16-B loads
                                 // per row where the separate arrays take 13 loads from four lines (k_ode_nn's per-row loads were a fifth of its time)
    const double *bt;            // [3][4]: rhs_b of the BCS_MIN system / rhs_t of the BCS_MAX system
    int n;
};

// tables of the DIRECT elliptic solver (poisson_direct.hip)
struct Int2Dev {
    const double *Bt, *A5, *s, *R;   // row-major [n][5], [n][5], [n], [n][3] (poisson_host.hpp)
    double rb[3][4], rt[3][4];
    double c1[3], e1, nb[2], cn[3], en, nt[2];
    int n;
};

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
inline void hipc(hipError_t e, const char *what) {
    if (e != hipSuccess) throw Fail(TLAB_EHIP, std::string("HIP ") + what + ": " + hipGetErrorString(e));
}
inline void fftc(rocfft_status s, const char *what) {
    if (s != rocfft_status_success) throw Fail(TLAB_EHIP, std::string("rocFFT ") + what + " failed (status " + std::to_string((int)s) + ")");
}
// an integer switch of the environment; the caller decides when it is read (per call, per plan creation, or once per process through a static)
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// f(std::integral_constant<int, NM>) for NM = modes per workgroup of the chunked kernels (4, 8, 16, 32; anything else: 64)
template <class F>
void dispatch_nm(int NM, F &&f) {
    switch (NM) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
    }
}

// kernel K may ask for up to 160 KiB of dynamic LDS: set once per kernel, before its first launch
template <auto K>
void allow_max_lds() {
    static const bool done = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024));
        (void)hipGetLastError();
        return true;
    }();
    (void)done;
}

struct DBuf {
    double *p = nullptr;
    size_t n = 0;
    void alloc(size_t count) {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = count;
        if (count) hipc(hipMalloc((void **)&p, count * sizeof(double)), "hipMalloc");
    }
    void upload(const std::vector<double> &h) {
        alloc(h.size());
        if (n) hipc(hipMemcpy(p, h.data(), n * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
    }
    ~DBuf() { if (p) (void)hipFree(p); }
};

struct FftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    void *work = nullptr;
    size_t work_bytes = 0;
    ~FftPlan() {
        if (info) rocfft_execution_info_destroy(info);
        if (plan) rocfft_plan_destroy(plan);
        if (work) (void)hipFree(work);
    }
    void finish() {
        fftc(rocfft_plan_get_work_buffer_size(plan, &work_bytes), "work size");
        fftc(rocfft_execution_info_create(&info), "info");
        if (work_bytes) {
            hipc(hipMalloc(&work, work_bytes), "hipMalloc(fft work)");
            fftc(rocfft_execution_info_set_work_buffer(info, work, work_bytes), "set work");
        }
    }
    void exec(void *in, void *out, hipStream_t st, double bytes = 0.0) {
        ProfScope ps("rocfft", st, bytes);
        fftc(rocfft_execution_info_set_stream(info, st), "set stream");
        void *ib[1] = {in}, *ob[1] = {out};
        fftc(rocfft_execute(plan, ib, ob, info), "execute");
    }
};

}  // namespace tlab

using namespace tlab;      // (this header is for the Poisson files only)

struct tlab_poisson_plan {
    int nx = 0, ny = 0, nz = 0, nxh = 0;   // nz = local number of z planes (kmax)
    int nzt = 0, koff = 0, nproc = 1;      // global nz, first global plane of this slab, number of z slabs
    int ioff = 0;                          // first global kx of the local spectral box (kx-pencil plans; nxh is then the local count)
    int fx_nxh = 0, fx_nz = 0;             // x-transform geometry: complex row length nx/2+1 and number of planes it is batched over
    long long nm = 0;                 // local modes = nxh * nz
    double norm = 1.0;
    Int1Tables tmin, tmax;            // host copies
    // SpaceOrder1 with (3, 3) or (5, 7) diagonals: integral systems factorized on the host (int1_generic.cpp), one table set per system and
    // lambda array in use (all modes; the singular modes' zeros), built the first time base_args meets it
    bool generic = false;
    DerTables gder;
    struct GenSet { int which; const double *lam; long long nm; DBuf fac, rb, rt, R; int ndi = 0, nri = 0; };
    mutable std::vector<std::unique_ptr<GenSet>> gen;
    const GenSet &gen_set(int which, const double *lam_dev, long long nm_) const {
        for (const auto &e : gen)
            if (e->which == which && e->lam == lam_dev && e->nm == nm_) return *e;
        std::vector<double> hl((size_t)nm_);
        if (hipMemcpy(hl.data(), lam_dev, (size_t)nm_ * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) throw Fail(TLAB_EHIP, "hipMemcpy (lambda)");
        Int1Gen G;
        int1_generic_build(gder, which == 0 ? 1 : 2, hl.data(), nm_, which == 0 ? 1.0 : -1.0, G);
        auto e = std::make_unique<GenSet>();
        e->which = which; e->lam = lam_dev; e->nm = nm_; e->ndi = G.ndi; e->nri = G.nri;
        e->fac.upload(G.fac); e->rb.upload(G.rb); e->rt.upload(G.rt); e->R.upload(G.R);
        gen.push_back(std::move(e));
        return *gen.back();
    }
    DBuf d_L0[2], d_L1[2], d_R[2];    // [0] BCS_MIN tables, [1] BCS_MAX tables
    DBuf d_pk[2];                     // OdeSys::pk
    DBuf lam;                         // [nm]  sqrt(kx'^2 + kz'^2)
    DBuf hom, der, cst;               // homogeneous solutions [5][ny][nm], their boundary derivatives [3][nm], 3x3 LU [9][nm]
    DBuf scratch, v0, u0, du0, bcs;   // per-call work: [5][ny][nm], [2][ny][nm] x2, [2][nm], [4][nm]
    DBuf cwork;                       // complex work field (nxh*ny*nz complex)
    DBuf d_bt[2], chk[2], chk_s[2], homb;       // chunked ODE kernel: boundary constants [3][4], PENTADFS checkpoints [blk][C][6][NM] of both systems,
                                      // homogeneous solutions re-laid out as [blk][5][ny][NM]
    bool use_chunked = false;
    int ode_nm_per_wg = 0;
    int ode_om = OM;                  // rows per thread of k_ode_nn
    bool ode_pair = false;            // k_ode_nn on mirror pairs (kx, kz), (kx, nz - kz): lambda symmetric to the bit, checked at creation
    // The lowest-lambda modes of a chunked plan go through a marching sub-plan on the side stream (see build_low_modes)
    std::unique_ptr<tlab_poisson_plan> low;
    DBuf fac[2];                      // sub-plan only: stored LU factors of its two systems (Int1Args::fac)
    int *d_low_modes = nullptr;
    int *d_hom_band = nullptr;                  // [2][nm] rows between which the homogeneous solutions of a mode are negligible (k_ode_hom_band)
    int n_low = 0;
    DBuf low_f, low_p, low_dp;
    std::vector<int> sing_modes;      // flat mode indices t = kx + nxh*kz of the singular modes
    int *d_sing = nullptr;
    unsigned char *d_skip = nullptr;
    DBuf s_lam, s_f, s_unit, s_bct, s_v0, s_v1, s_u0, s_u1, s_du0, s_du1, s_scr;
    DBuf dd_v1, dd_u1, dd_du1, dd_sp, dd_ones, dd_bcb;      // BCS_DD: homogeneous solutions of the singular modes (built on first use)
    bool dd_ready = false;
    DBuf cst_dd;                                // [5][nm] constants of the chunked BCS_DD solver (k_dd_constants), built on first use
    FftPlan fx_r2c, fx_c2r, fz_f, fz_b;
    FftPlan f2_fwd, f2_bwd;           // optional fused 2-D (x,z) transforms, batch over y
    std::unique_ptr<FftzPlan> fz_own;  // own strided z-transform (fftz.hip) where its lengths apply; rocFFT's fz_f / fz_b otherwise
    std::unique_ptr<FftxPlan> fx_own;  // own one-pass real-to-complex x-transform (fftz.hip: k_fftx_r2c); rocFFT's two-kernel fx_r2c otherwise
    // one-shot request of the RHS driver (tlab_internal_poisson_arm_v_final): the inverse x-transform of dp^/dy finishes the v equation
    // (FftxPlan::exec_inverse_final) instead of writing dp/dy
    struct VFinal { double *q = nullptr, *h = nullptr; double dte = 0.0, kco = 0.0; int scale = 0; bool armed = false; } vfinal;
    void x_backward_dpdy(void *in, double *dpdy, hipStream_t st, const VFinal &f) {
        if (f.armed && fx_own) fx_own->exec_inverse_final(static_cast<const double *>(in), f.q, f.h, f.dte, f.kco, f.scale, ny, st);
        else fx_c2r.exec(in, dpdy, st);
    }
    // inverse x-transform of p^: rocFFT's c2r runs at the copy rate at 512 points but at 2.1 TB/s from 1024 on (4.06 ms per call on one rank's share of
    // BASELINE configs[4], where the own kernel moves the same bytes at 5.9 TB/s); TLAB_FFTX_C2R_OWN = 0 / 1 forces the choice
    void x_backward_p(void *in, double *p, hipStream_t st) {
        static const int own = env_int("TLAB_FFTX_C2R_OWN", -1);
        if (fx_own && (own == 1 || (own < 0 && nx >= 1024))) fx_own->exec_inverse(static_cast<const double *>(in), p, st);
        else fx_c2r.exec(in, p, st);
    }
    void x_forward(void *in, void *out, hipStream_t st) {
        if (fx_own) fx_own->exec(static_cast<const double *>(in), static_cast<double *>(out), st);
        else fx_r2c.exec(in, out, st);
    }
    // the z-transform: the own one (fftz.hip) where its lengths apply, rocFFT's fz_f / fz_b (out of place) otherwise
    void z_exec(int dir, double *in, double *out, hipStream_t st) {
        if (fz_own) fz_own->exec(dir, in, out, st);
        else (dir > 0 ? fz_f : fz_b).exec(in, out, st);
    }
    // the transforms of a single-device plan (poisson.hip): field -> spectrum in tmp1 (fused 2-D, x then z, or x alone when nz = 1), and the inverse;
    // vf: the field is dp/dy and the inverse x-transform honours the request
    void forward_xz(double *field, double *tmp1, double *tmp2, hipStream_t st);
    void backward_xz(double *hat, double *out, hipStream_t st, const VFinal *vf = nullptr);
    // pack-layout maps of the own x-transforms (tlab_poisson_fft_x_packed), one per distinct block map; a slab driver uses one or two
    struct KxMap { std::vector<long long> key; long long *off = nullptr; int *w = nullptr; };
    std::vector<KxMap> kxmaps;
    const KxMap &kx_map(int nblocks, const int *start, const long long *base) {
        std::vector<long long> key;
        key.reserve((size_t)2 * nblocks);
        for (int b = 0; b < nblocks; ++b) { key.push_back(start[b]); key.push_back(base[b]); }
        for (const KxMap &m : kxmaps) if (m.key == key) return m;
        std::vector<long long> off((size_t)fx_nxh);
        std::vector<int> w((size_t)fx_nxh);
        if (tlab_debug_pack_map(fx_nxh, nblocks, start, base, off.data(), w.data()) != TLAB_OK) throw Fail(TLAB_EINVAL, "pack map: bad block map");
        KxMap m;
        m.key = key;
        hipc(hipMalloc((void **)&m.off, off.size() * sizeof(long long)), "hipMalloc");
        hipc(hipMalloc((void **)&m.w, w.size() * sizeof(int)), "hipMalloc");
        hipc(hipMemcpy(m.off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice), "hipMemcpy");
        hipc(hipMemcpy(m.w, w.data(), w.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
        kxmaps.push_back(m);
        return kxmaps.back();
    }
    bool use_2d = false;
    hipStream_t side = nullptr;       // the <= 4 singular modes are solved beside the regular ones
    // DIRECT elliptic solver (EllipticOrder = CompactDirect6): one second-order integral operator per boundary type, built on first use
    bool direct = false;
    bool exact_mode = false;                  // tlab_poisson_set_exact(1) at creation: marching kernels only (k_int2 instead of k_int2c)
    tlab_fdm_plan_t gy_der = nullptr;         // y plan of the derivatives (dp/dy = OPR_Partial_Y(p), opr_elliptic.f90:447-449); not owned
    // factorized Helmholtz (opr_elliptic.f90:466-557): the per-mode tables depend on alpha, so every alpha in use is a sub-plan of its own
    // (tables only; transforms and work field are the parent's).  The implicit RK cycles through a few alphas: the last 4 are kept.
    tlab_fdm_plan_t g3[3] = {nullptr, nullptr, nullptr};      // x, y, z plans of a single-device factorized plan; not owned
    bool helmholtz = false;
    std::vector<std::pair<double, std::unique_ptr<tlab_poisson_plan>>> helm;
    DerTables ell_der2;                       // second derivative of the elliptic y plan (fdm_loc%der2)
    std::vector<double> ell_nodes;
    struct Int2Set { Int2Tables host; DBuf Bt, A5, s, R, chk; double chk_alpha = 0.0; bool chk_ok = false; };      // chk: checkpoints of k_int2c for one alpha
    std::unique_ptr<Int2Set> int2[4];
    long long sing_direct = -1;               // local index of the mode (1,1), or -1 when another rank owns it
    Int2Dev dev2(int ibc) {
        if (!int2[ibc]) {
            auto e = std::make_unique<Int2Set>();
            int2_build_tables(ell_der2, ell_nodes, ibc, e->host);
            e->Bt.upload(e->host.Bt); e->A5.upload(e->host.A5); e->s.upload(e->host.s); e->R.upload(e->host.R);
            int2[ibc] = std::move(e);
        }
        Int2Set &E = *int2[ibc];
        Int2Dev d;
        d.Bt = E.Bt.p; d.A5 = E.A5.p; d.s = E.s.p; d.R = E.R.p; d.n = ny;
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 4; ++c) { d.rb[j][c] = E.host.rb[j][c]; d.rt[j][c] = E.host.rt[j][c]; }
        for (int q = 0; q < 3; ++q) { d.c1[q] = E.host.c1[q]; d.cn[q] = E.host.cn[q]; }
        d.e1 = E.host.e1; d.en = E.host.en;
        for (int q = 0; q < 2; ++q) { d.nb[q] = E.host.nb[q]; d.nt[q] = E.host.nt[q]; }
        return d;
    }
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t side_low = nullptr;   // the low-mode sub-plan runs beside the singular modes, not behind them
    hipEvent_t ev_join_low = nullptr;
    ~tlab_poisson_plan() {
        if (d_sing) (void)hipFree(d_sing);
        if (d_skip) (void)hipFree(d_skip);
        if (d_low_modes) (void)hipFree(d_low_modes);
        if (d_hom_band) (void)hipFree(d_hom_band);
        if (side) (void)hipStreamDestroy(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (side_low) (void)hipStreamDestroy(side_low);
        if (ev_join_low) (void)hipEventDestroy(ev_join_low);
        for (KxMap &m : kxmaps) { (void)hipFree(m.off); (void)hipFree(m.w); }
    }
    OdeSys sys(int which) const {
        OdeSys d;
        d.L0 = d_L0[which].p; d.L1 = d_L1[which].p; d.R = d_R[which].p; d.bt = d_bt[which].p; d.n = ny;
        d.pk = d_pk[which].p;
        return d;
    }
    Int1Dev dev(int which) const {
        const Int1Tables &T = which == 0 ? tmin : tmax;
        Int1Dev d;
        if (generic) {      // k_int1g reads its own tables (Int1Args::g_*)
            d = Int1Dev{};
            d.n = ny;
            return d;
        }
        d.L0 = d_L0[which].p; d.L1 = d_L1[which].p; d.R = d_R[which].p; d.n = ny;
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 4; ++c) { d.rb[j][c] = T.rb[j][c]; d.rt[j][c] = T.rt[j][c]; }
        return d;
    }
};

// ------------------------------------------------------------------------------------------------
// what the Poisson files call in each other (grouped by defining file)
// ------------------------------------------------------------------------------------------------
namespace tlab {

// ---- poisson_int1.hip ----
// one FDM_Int1_Solve per mode; defined there for the six combinations in use: <1,2,FIELD> <1,2,LINEAR> <2,2,LINEAR> <2,3,LINEAR> <1,2,UNIT> <2,2,UNIT>
template <int BC, int NL, int FS>
void launch_int1(const Int1Args &a, hipStream_t st);

// ---- poisson_ode.hip ----
int ode_modes_per_wg(int C);                                            // modes per workgroup for lines of C chunks, 0: no chunked form
size_t ode_lds_bytes(int C, int NM, int om = OM, int NL = 2);
inline int ode_sing_nm(int C) { return C >= 64 ? 4 : 8; }               // lanes per chunk of k_ode_sing (see launch_ode_sing)
void build_checkpoints(tlab_poisson_plan &P, hipStream_t st);
void build_singular_checkpoints(tlab_poisson_plan &P, hipStream_t st);
void launch_ode(tlab_poisson_plan &P, double *f_hat, double *p_hat, double *dp_hat, hipStream_t st, bool dd = false);
void launch_ode_sing(tlab_poisson_plan &P, double *f_hat, double *p_hat, double *dp_hat, hipStream_t st);

// ---- poisson_direct.hip ----
void poisson_direct_stage(tlab_poisson_plan_t P, int ibc, double *f_hat, double *p_hat, hipStream_t st, bool helmholtz = false, double alpha = 0.0);

}  // namespace tlab
