// C ABI of include/tlab_amd.h: the operators -- which kernel a call takes (dispatch), the fused variants of the drivers, the public operators.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "errors.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "plan.hpp"

using namespace tlab;

namespace {

int g_last_path = 0;
int g_force_path = 0;
DeviceArray *g_ws = nullptr;  // grow-only scratch field

enum { PATH_GENERIC = 1, PATH_XLINE = 2, PATH_RTILE = 3 };

// fusions used by the RHS driver (rhs.cpp): operand = in0 + scale*in0b (P1), result accumulated into the output (P1, Burgers)
struct OpExtra {
    const double *in0b = nullptr;
    double scale = 0.0;
    bool acc = false;
    // MODE_BURGERS with several transported fields and one advecting velocity
    int nf = 0;
    const double *fs[4] = {nullptr, nullptr, nullptr, nullptr};
    double *fo[4] = {nullptr, nullptr, nullptr, nullptr};
    double fnu[4] = {0, 0, 0, 0};
    // MODE_P1 final-update epilogue
    double *fq = nullptr;
    double fdte = 0.0, fkco = 1.0;
    int fscale = 0, fnx = 1, fny = 1;
    const double *fpb = nullptr, *fpt = nullptr;      // ... with given wall tendencies (Neumann walls) instead of zero
    int ffin[4] = {0, 0, 0, 0};
    int fclip[4] = {0, 0, 0, 0};      // k_xline finishing epilogue: scalar bounds (XLineArgs::fclip)
    double flo[4] = {0, 0, 0, 0}, fhi[4] = {0, 0, 0, 0};
    double *fdiv = nullptr;
    double fidte = 0.0;
    unsigned fresh_mask = 0;        // k_htile MODE_BURGERS: fields that overwrite their tendency in an accumulating launch
    const double *ari = nullptr;    // MODE_BURGERS, anelastic: ribackground [ny] on the diffusion term
    int ari_mode = 0, ari_nx = 1, ari_ny = 1;
    bool sub = false;               // MODE_P1: out0 -= value
    int fneu = 0;                   // k_rtile MODE_P1: Neumann-final epilogue (RTileArgs::fneu)
    double fcb[4] = {0, 0, 0, 0}, fct[4] = {0, 0, 0, 0};
};
const OpExtra kNoExtra{};

// Periodic x lines on P chunks whose lane-variant tables the kernel keeps as float differences from chunk 0 (kernels.hip, xcoef): exact only
// while the chunks differ by rounding-level amounts (periodic "uniform" grids), which is checked here once per plan and P on the host tables.
bool xline_wide_ok(tlab_fdm_plan_t g, int P) {
    if (!g || !g->t.periodic || (P != 64 && P != 128 && P != 256) || g->t.n % P != 0) return false;
    int &cache = g->wide_ok[P == 64 ? 0 : P == 128 ? 1 : 2];
    if (cache >= 0) return cache != 0;
    bool ok = true;
    for (int which = 1; which <= 2 && ok; ++which) {
        const SystemEntry *ep = nullptr;
        try { ep = &g->system(which, 0, P); } catch (const std::exception &) { ok = false; break; }      // e.g. no two-level tables
        const SystemEntry &e = *ep;
        if (e.lane_invariant) continue;
        const ChunkedTables &h = e.host;
        const int m = h.m;
        const std::vector<double> *tabs[5] = {&h.Lm, &h.Dinv, &h.Cm, &h.V, &h.W};
        for (int t = 0; t < 5 && ok; ++t)
            for (int l = 0; l < P && ok; ++l)
                for (int p = 0; p < m; ++p) {
                    const double c = (*tabs[t])[(size_t)l * m + p], b = (*tabs[t])[p];
                    const volatile float df = (float)(c - b);
                    const volatile double r = b + (double)df;
                    if (r != c) { ok = false; break; }
                }
    }
    cache = ok ? 1 : 0;
    return ok;
}

}  // namespace

// chunks per x line of the wave-per-line kernel (0: not on that kernel).  Lines of 1024 / 2048 periodic points go on 2 / 4 waves with 8 rows
// per lane (128 / 256 chunks) when their tables allow the float-difference form; TLAB_XLINE_WIDE=0 keeps the one-wave forms (16 / 32 rows per lane).
int xline_chunks(int n, tlab_fdm_plan_t g) {
    static const bool wide = [] { const char *e = getenv("TLAB_XLINE_WIDE"); return !(e && atoi(e) == 0); }();
    if (g && wide && n == 1024 && xline_wide_ok(g, 128)) return 128;
    if (g && wide && n == 2048 && xline_wide_ok(g, 256)) return 256;
    if (n == 2048) return (g && xline_wide_ok(g, 64)) ? 64 : 0;
    return xline_supported(n) ? 64 : 0;
}

namespace {

int choose_path(int dir, int n, tlab_fdm_plan_t g = nullptr) {
    int path = PATH_GENERIC;
    if (g && g->t.der1.ndl == 5) return PATH_GENERIC;      // CompactJacobian6Penta: run_generic sends the first derivative to k_pentatile / k_penta1, nothing is fused
    if (g && g->t.der1.direct && dir == 1) return PATH_GENERIC;      // per-row first-derivative RHS: not in the wave-per-line kernel
    if (dir == 1 && xline_chunks(n, g) > 0) path = PATH_XLINE;
    if (dir != 1 && (rtile_chunk(n) > 0 || htile_chunk(n, MODE_P1) > 0)) path = PATH_RTILE;
    if (g_force_path == PATH_GENERIC) path = PATH_GENERIC;
    if (g_force_path == PATH_RTILE && (rtile_chunk(n) > 0 || htile_chunk(n, MODE_P1) > 0) && dir != 1) path = PATH_RTILE;
    return path;
}

void run_generic(tlab_fdm_plan_t g, const LineGeom &geom, int which, int ibc, const double *in0, const double *d1in,
                 double *out) {
    if (which == 1 && g->t.der1.ndl == 5) {      // CompactJacobian6Penta (fdm_com1_jacobian.f90:136-192)
        const DerTables &d = g->t.der1;
        if (d.ndr != 7 || d.lu.empty()) throw Fail(TLAB_EUNSUPPORTED, "pentadiagonal first derivative: 7 RHS diagonals and the LU factors are required");
        if (!g->penta_rhs) {
            g->penta_rhs = std::make_unique<DeviceArray>();
            g->penta_rhs->upload(d.rhs);
            g->penta_lu = std::make_unique<DeviceArray>();
            g->penta_lu->upload(d.lu);
        }
        PentaArgs a;
        a.in0 = in0; a.out0 = out; a.g = geom; a.rhs = g->penta_rhs->p; a.lu = g->penta_lu->p;
        a.periodic = d.periodic ? 1 : 0; a.ibc = d.periodic ? 0 : ibc;
        std::copy(d.rhs_b, d.rhs_b + 32, a.rb);
        std::copy(d.rhs_t, d.rhs_t + 35, a.rt);
        auto tile = [&](const LineGeom &tg, const double *src, double *dst, bool along_x = false) {      // k_pentatile where the line length allows (32-row chunks, at most 16)
            const int key = d.periodic ? 0 : ibc;
            auto &slot = g->penta_tile[key];
            if (!slot) {
                std::vector<double> rows, blocks, smw;
                pentatile_build(tg.n, tg.n / 32, d.periodic, key, d.lu.data(), rows, blocks, smw);
                slot = std::make_unique<tlab_fdm_plan::PentaTile>();
                slot->rows.upload(rows); slot->blocks.upload(blocks); slot->smw.upload(smw);
            }
            PentaTileArgs t;
            t.in0 = src; t.out0 = dst; t.g = tg; t.rhs = g->penta_rhs->p; t.rows = slot->rows.p; t.blocks = slot->blocks.p; t.smw = slot->smw.p;
            t.r6 = d.rhs[4 + (size_t)tg.n * 5]; t.r7 = d.rhs[4 + (size_t)tg.n * 6];      // rhs(5, 6), rhs(5, 7)
            t.periodic = a.periodic; t.ibc = a.ibc;
            std::copy(d.rhs_b, d.rhs_b + 32, t.rb);
            std::copy(d.rhs_t, d.rhs_t + 35, t.rt);
            if (along_x) hk(launch_pentatile_x(t, tlab_current_stream()), "k_pentatile<x>");
            else hk(launch_pentatile(t, tlab_current_stream()), "k_pentatile");
        };
        if (geom.row_stride == 1 && pentatile_x_ok(geom)) {      // x lines of 64 .. 512 points: the tile kernel through an LDS tile, no transposes
            tile(geom, in0, out, true);
            return;
        }
        if (geom.row_stride == 1 && geom.nlines >= 64) {
            // x lines: one thread per line strides through contiguous memory (64 cache lines per wave access; 243 GB/s at 256^3, measured).  Like the
            // reference (OPR_Partial_X: TLab_Transpose, solve, transpose back, opr_partial.f90:185-195) the lines are made the fastest index first:
            // two transposes at the copy rate + the coalesced solve (the y-direction speed) -- same operations per line, same results
            const size_t N = (size_t)geom.n * geom.nlines;
            if (!g->penta_ws) g->penta_ws = std::make_unique<DeviceArray>();
            double *t1 = g->penta_ws->reserve(2 * N), *t2 = t1 + N;
            hk(launch_transpose(in0, t1, geom.n, (int)geom.nlines, tlab_current_stream()), "transpose");
            a.in0 = t1; a.out0 = t2;
            a.g.row_stride = geom.nlines; a.g.lines_inner = (int)geom.nlines; a.g.outer_stride = 0;
            if (pentatile_ok(a.g)) tile(a.g, t1, t2);
            else hk(launch_penta1(a, tlab_current_stream()), "k_penta1");
            hk(launch_transpose(t2, out, (int)geom.nlines, geom.n, tlab_current_stream()), "transpose");
            return;
        }
        if (pentatile_ok(geom)) tile(geom, in0, out);
        else hk(launch_penta1(a, tlab_current_stream()), "k_penta1");
        return;
    }
    GenericArgs a;
    a.in0 = in0; a.in1 = d1in; a.out0 = out; a.g = geom;
    a.s = g->stencil(which, ibc);
    a.y = g->system(which, ibc, 1).dev();
    a.jc = (which == 2 && d1in) ? g->jaccorr() : JacCorrDev{nullptr};
    hk(launch_generic(which == 2, a, tlab_current_stream()), "k_generic");
}

void run_rtile(tlab_fdm_plan_t g, const LineGeom &geom, int mode, int ibc, const double *in0, const double *in1,
               const double *in2, double *out, double nu, const OpExtra &ex = kNoExtra) {
    const int P = geom.n / rtile_chunk(geom.n);
    RTileArgs a{};
    a.in0 = in0; a.in1 = in1; a.in2 = in2; a.out0 = out; a.out1 = nullptr; a.g = geom; a.nu = nu;
    a.in0b = ex.in0b; a.in0b_scale = ex.scale; a.acc = ex.sub ? 2 : (ex.acc ? 1 : 0);
    a.nf = 0;
    a.fq = ex.fq; a.fdte = ex.fdte; a.fkco = ex.fkco; a.fscale = ex.fscale; a.fnx = ex.fnx; a.fny = ex.fny; a.fpb = ex.fpb; a.fpt = ex.fpt;
    a.fneu = ex.fneu;
    for (int q = 0; q < 4; ++q) { a.fcb[q] = ex.fcb[q]; a.fct[q] = ex.fct[q]; }
    a.s1 = g->stencil(1, ibc);
    a.s2 = g->stencil(2, 0);
    a.y1 = g->system(1, ibc, P).dev();
    a.y2 = g->system(2, 0, P).dev();
    a.jc = (mode == MODE_P2_D1IN || mode == MODE_BURGERS_D1IN) ? g->jaccorr() : JacCorrDev{nullptr};
    hk(launch_rtile(mode, a, tlab_current_stream()), "k_rtile");
}

int g_htile_policy = 0;   // 0 automatic, 1 never (two-launch k_rtile path), 2 always when the size allows

bool htile_ok(int n, int mode) { return g_htile_policy != 1 && htile_chunk(n, mode) > 0; }

void run_htile(tlab_fdm_plan_t g, const LineGeom &geom, int mode, int ibc, const double *in0, const double *vel, double *out0,
               double *out1, double nu, const OpExtra &ex = kNoExtra) {
    const int C = geom.n / htile_chunk(geom.n, mode);
    RTileArgs a{};
    a.in0 = in0; a.in1 = nullptr; a.in2 = vel; a.out0 = out0; a.out1 = out1; a.g = geom; a.nu = nu;
    a.in0b = nullptr; a.in0b_scale = 0.0; a.acc = ex.acc ? 1 : 0;
    a.fq = nullptr; a.fdte = 0.0; a.fkco = 1.0; a.fscale = 0; a.fnx = 1; a.fny = 1; a.fpb = nullptr; a.fpt = nullptr;
    if (mode == MODE_P1) {      // the epilogues of k_rtile<P1> (run_p1_tile)
        a.in0b = ex.in0b; a.in0b_scale = ex.scale; a.acc = ex.sub ? 2 : (ex.acc ? 1 : 0);
        a.fq = ex.fq; a.fdte = ex.fdte; a.fkco = ex.fkco; a.fscale = ex.fscale; a.fnx = ex.fnx; a.fny = ex.fny; a.fpb = ex.fpb; a.fpt = ex.fpt;
    }
    a.nf = ex.nf > 0 ? ex.nf : 1;
    for (int f = 0; f < 4; ++f) { a.fs[f] = ex.nf > 0 ? ex.fs[f] : in0; a.fo[f] = ex.nf > 0 ? ex.fo[f] : out0; a.fnu[f] = ex.nf > 0 ? ex.fnu[f] : nu; }
    a.s1 = g->stencil(1, ibc);
    a.s2 = g->stencil(2, 0);
    a.y1 = g->system(1, ibc, C).dev();
    a.y2 = g->system(2, 0, C).dev();
    a.jc = (mode != MODE_P1) ? g->jaccorr() : JacCorrDev{nullptr};
    a.fresh_mask = ex.fresh_mask; a.fdiv = ex.fdiv; a.fidte = ex.fidte;
    a.ari = ex.ari; a.ari_mode = ex.ari_mode; a.ari_nx = ex.ari_nx; a.ari_ny = ex.ari_ny;
    hk(launch_htile(mode, a, tlab_current_stream()), "k_htile");
}

// One line-set (first derivative, with or without the fused epilogues) along y or z.  k_rtile's 64-line tiles are the best form while a chunk of
// the line fits the 128 VGPRs of its 1024-thread launch (32 rows, lines up to 512 points); at 1024 points its chunks are 64 rows and it spills
// 431 VGPRs (3.0 TB/s for the final z gradient of BASELINE configs[3]) -- those lines take k_htile's 32-line tiles (32 chunks of 32 rows, 126 VGPRs),
// which carries the same epilogues except the Neumann-final one (y lines only).
void run_p1_tile(tlab_fdm_plan_t g, const LineGeom &geom, int ibc, const double *u, double *result, const OpExtra &ex = kNoExtra) {
    static const bool off = [] { const char *e = getenv("TLAB_P1_HTILE"); return e && atoi(e) == 0; }();
    // ... and the final-update epilogue (five passes: p, h, q in; h, q out) at every length: k_rtile's 1024-thread launch spills 43 VGPRs with it,
    // k_htile<32, P1, 512> none -- final z gradient at 512^3 1.24 -> 1.15 ms (A/B on one box); TLAB_P1_HTILE=2: k_htile for every epilogue form
    static const bool always = [] { const char *e = getenv("TLAB_P1_HTILE"); return e && atoi(e) == 2; }();
    const int mr = rtile_chunk(geom.n);
    const bool rtile_spills = mr == 64 && geom.n / 64 > 8;
    const bool lane_offsets_fit = 3.0 * 32.0 * (double)geom.row_stride * 8.0 + 512.0 < 4294967296.0;      // launch_htile's 32-bit lane part of an address
    // ... and y lines (row stride = lines per plane): plain 0.509 -> 0.49 ms at 512^3, with the operand sum of the forcing term 0.114 -> 0.101 ms per 64-plane
    // slab; plain z lines stay on k_rtile (0.536 against 0.585 ms)
    const bool ylines = geom.row_stride == geom.lines_inner && geom.lines_inner != geom.nlines;
    if (!off && (rtile_spills || always || ex.fq != nullptr || ylines) && ex.fneu == 0 && htile_chunk(geom.n, MODE_P1) == 32 && g_htile_policy != 1 && lane_offsets_fit)
        run_htile(g, geom, MODE_P1, ibc, u, nullptr, result, nullptr, 0.0, ex);
    else
        run_rtile(g, geom, MODE_P1, ibc, u, nullptr, nullptr, result, 0.0, ex);
}

void run_xline(tlab_fdm_plan_t g, const LineGeom &geom, int mode, int ibc, const double *in0, const double *in1,
               double *out0, double *out1, double nu, const OpExtra &ex = kNoExtra) {
    XLineArgs a;
    a.in0 = in0; a.in1 = in1; a.out0 = out0; a.out1 = out1; a.nlines = geom.nlines; a.nu = nu;
    a.in0b = ex.in0b; a.in0b_scale = ex.scale; a.acc = ex.sub ? 2 : (ex.acc ? 1 : 0);
    a.fq = ex.fq; a.fdte = ex.fdte; a.fkco = ex.fkco; a.fscale = ex.fscale; a.fnx = ex.fnx; a.fny = ex.fny; a.fpb = ex.fpb; a.fpt = ex.fpt;
    a.nf = ex.nf > 0 ? ex.nf : 1;
    for (int f = 0; f < 4; ++f) { a.fs[f] = ex.nf > 0 ? ex.fs[f] : in0; a.fo[f] = ex.nf > 0 ? ex.fo[f] : out0; a.fnu[f] = ex.nf > 0 ? ex.fnu[f] : nu; a.ffin[f] = ex.ffin[f];
                              a.fclip[f] = ex.fclip[f]; a.flo[f] = ex.flo[f]; a.fhi[f] = ex.fhi[f]; }
    a.fdiv = ex.fdiv; a.fidte = ex.fidte;
    a.ari = ex.ari; a.ari_ny = ex.ari_ny;
    a.s1 = g->stencil(1, ibc);
    a.s2 = g->stencil(2, 0);
    const int P = xline_chunks(geom.n, g);
    SystemEntry &e1 = g->system(1, ibc, P), &e2 = g->system(2, 0, P);
    a.y1 = e1.dev();
    a.y2 = e2.dev();
    const bool lv = !(e1.lane_invariant && e2.lane_invariant);
    static const bool dbg = getenv("TLAB_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[tlab] k_xline mode %d n %d chunks %d lane_variant %d\n", mode, geom.n, P, (int)lv);
    hk(launch_xline(mode, geom.n, P, lv, a, tlab_current_stream()), "k_xline");
}

void check_common(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc) {
    if (!g) throw Fail(TLAB_EINVAL, "null plan");
    if (dir < 1 || dir > 3) throw Fail(TLAB_EINVAL, "dir must be 1, 2 or 3");
    if (nx < 1 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, "bad sizes");
    if ((long long)nx * ny * nz > 2147483647LL) throw Fail(TLAB_EINVAL, "local field exceeds int32 indexing (reference limit, tlab_memory.f90:175)");
    if (ibc < 0 || ibc > 3) throw Fail(TLAB_EINVAL, "ibc must be 0..3");
    const int n = (dir == 1) ? nx : (dir == 2) ? ny : nz;
    if (g->t.n != n) throw Fail(TLAB_EINVAL, "plan size does not match the field size along dir");
    if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
}

}  // namespace

// ---- internal fused variants for the RHS driver; return false when the sizes are not on a fused fast path ----
// result (+)= d/dx_dir (u + scale*ub)
bool tlab_internal_partial_p1_fusable(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz) {
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    const int path = choose_path(dir, geom.n, g);    // with the plan: x lines of 2048 points take k_xline when their tables allow it
    return path == PATH_XLINE || (path == PATH_RTILE && rtile_chunk(geom.n) > 0);
}
bool tlab_internal_partial_p1_fused(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, const double *u, const double *ub,
                                    double scale, double *result, bool acc) {
    check_common(dir, g, nx, ny, nz, ibc);
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    OpExtra ex;
    ex.in0b = ub; ex.scale = scale; ex.acc = acc;
    const int path = choose_path(dir, geom.n, g);
    if (path == PATH_XLINE) {
        run_xline(g, geom, MODE_P1, ibc, u, nullptr, result, nullptr, 0.0, ex);
    } else if (path == PATH_RTILE && rtile_chunk(geom.n) > 0) {
        run_p1_tile(g, geom, ibc, u, result, ex);
    } else {
        return false;
    }
    g_last_path = path;
    return true;
}
// result -= d/dx_dir u  (fused kernels only; the caller falls back to OPR_Partial + a subtraction otherwise)
bool tlab_internal_partial_p1_sub(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, const double *u, double *result) {
    check_common(dir, g, nx, ny, nz, 0);
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    OpExtra ex;
    ex.sub = true;
    const int path = choose_path(dir, geom.n, g);
    if (path == PATH_XLINE) run_xline(g, geom, MODE_P1, 0, u, nullptr, result, nullptr, 0.0, ex);
    else if (path == PATH_RTILE && rtile_chunk(geom.n) > 0) run_p1_tile(g, geom, 0, u, result, ex);
    else return false;
    g_last_path = path;
    return true;
}
// The last pass over a field with Neumann walls (ibc: 1 jmin, 2 jmax, 3 both; the other side Dirichlet): BOUNDARY_BCS_NEUMANN_Y on the finished
// tendency h, its wall planes, q += dte h, h *= kco -- one launch along y instead of OPR_Partial_Y + k_neumann_planes + k_final_update.
bool tlab_internal_neumann_final_ok(tlab_fdm_plan_t g, int nx, int ny, int nz) {
    static const bool on = [] { const char *e = getenv("TLAB_NEUMANN_FINAL"); return !(e && atoi(e) == 0); }();
    if (!on || !g || g->t.periodic || g->t.der1.direct || ny < 8) return false;
    const DerTables &d = g->t.der1;
    if (d.ndl != 3 || (d.ndr != 3 && d.ndr != 5)) return false;
    const LineGeom geom = line_geom(2, nx, ny, nz);
    const int M = rtile_chunk(geom.n);
    return choose_path(2, geom.n, g) == PATH_RTILE && M >= 8 && M % 8 == 0;
}
bool tlab_internal_neumann_final(tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, double *h, double *q, double dte, double kco, int scale) {
    check_common(2, g, nx, ny, nz, ibc);
    if (ibc < 1 || ibc > 3 || !tlab_internal_neumann_final_ok(g, nx, ny, nz)) return false;
    const LineGeom geom = line_geom(2, nx, ny, nz);
    OpExtra ex;
    ex.fq = q; ex.fdte = dte; ex.fkco = kco; ex.fscale = scale; ex.fnx = nx; ex.fny = ny;
    ex.fneu = ibc;
    tlab_internal_neumann_y_coefficients(g, ibc, ny, ex.fcb, ex.fct);
    run_rtile(g, geom, MODE_P1, ibc, h, nullptr, nullptr, h, 0.0, ex);
    g_last_path = PATH_RTILE;
    return true;
}
// h -= d/dx_dir p ; walls ; q += dte h ; h *= kco : the last pass over a velocity component folded into the gradient of the pressure.
// Dirichlet walls only (the tendency is zero on the wall planes); dir = 1 or 3.
// pb, pt (device, [nx][nz]; NULL: zero): the tendencies of the wall planes j = 0 / ny-1 (BOUNDARY_BCS_NEUMANN_Y's values for a Neumann wall)
bool tlab_internal_gradient_final(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, const double *p, double *q, double *h, double dte,
                                  double kco, int scale, const double *pb, const double *pt) {
    check_common(dir, g, nx, ny, nz, 0);
    if (dir == 2) return false;
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    OpExtra ex;
    ex.fq = q; ex.fdte = dte; ex.fkco = kco; ex.fscale = scale; ex.fnx = nx; ex.fny = ny; ex.fpb = pb; ex.fpt = pt;
    const int path = choose_path(dir, geom.n, g);
    if (path == PATH_XLINE) run_xline(g, geom, MODE_P1, 0, p, nullptr, h, nullptr, 0.0, ex);
    else if (path == PATH_RTILE && rtile_chunk(geom.n) > 0) run_p1_tile(g, geom, 0, p, h, ex);
    else return false;
    g_last_path = path;
    return true;
}
// result += nu d2s - vel ds   (only when the fully fused Burgers kernels apply)
bool tlab_internal_burgers_acc(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, double nu, const double *s, const double *vel,
                               double *result) {
    check_common(dir, g, nx, ny, nz, ibc);
    if (tlab_internal_anelastic() || tlab_internal_dealiasing()) return false;      // those branches of OPR_Burgers_1D: the caller's unfused sequence
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    OpExtra ex;
    ex.acc = true;
    const bool corr = g->t.der2.need_1der || g->t.der2.direct;      // (the x-line kernel only knows the constant stencils)
    const int path = choose_path(dir, geom.n, g);
    if (path == PATH_XLINE && !corr) {
        run_xline(g, geom, MODE_BURGERS, ibc, s, vel, result, nullptr, nu, ex);
    } else if (path == PATH_RTILE && htile_ok(geom.n, MODE_BURGERS)) {
        run_htile(g, geom, MODE_BURGERS, ibc, s, vel, result, nullptr, nu, ex);
    } else {
        return false;
    }
    g_last_path = path;
    return true;
}

bool tlab_internal_burgers_fusable(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz) {
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    const int path = choose_path(dir, geom.n, g);
    return (path == PATH_XLINE && !g->t.der2.need_1der && !g->t.der2.direct) || (path == PATH_RTILE && htile_ok(geom.n, MODE_BURGERS));
}
// ... with the anelastic diffusion weight (tlab_internal_burgers_acc_n's ari): it exists in the wave-per-line kernel and in the 32-line tile form of k_htile
bool tlab_internal_burgers_fusable_anelastic(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz) {
    static const bool on = [] { const char *e = getenv("TLAB_ANELASTIC_FUSED"); return !(e && atoi(e) == 0); }();
    if (!on || !tlab_internal_burgers_fusable(dir, g, nx, ny, nz)) return false;
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (choose_path(dir, geom.n, g) == PATH_XLINE) return true;
    return htile_chunk(geom.n, MODE_BURGERS) == 32 && geom.n / 32 <= 16 && !htile_narrow() && (dir == 2 || nx % 32 == 0);
}
// several transported fields, one advecting velocity: result[f] += nu[f] d2 s[f] - vel d s[f]
// x lines of at most 512 points on the wave-per-line kernel: the launch can finish the substep of a transported field in its epilogue
bool tlab_internal_burgers_can_finish(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz) {
    if (dir != 1 || nx / std::max(xline_chunks(nx, g), 1) > 8) return false;      // the epilogue exists in the 8-rows-per-lane forms
    return tlab_internal_burgers_fusable(dir, g, nx, ny, nz) && choose_path(1, nx, g) == PATH_XLINE;
}

// finish (may be NULL): per field, != 0 -> this launch is the last term of that field's tendency and also does its Runge-Kutta update
// (s += dte h, h = scale ? kco h : h, h = 0 on the wall planes); only where tlab_internal_burgers_can_finish says so
// the y / z tile kernel can add its direction's term of the pressure forcing in the epilogue of a one-field launch (RTileArgs::fdiv)
bool tlab_internal_burgers_can_div(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz) {
    if (!g || dir < 2 || dir > 3) return false;
    static const bool on = [] { const char *e = getenv("TLAB_DIV_IN_BURGERS"); return !(e && atoi(e) == 0); }();
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (!on || geom.n == 1 || choose_path(dir, geom.n, g) != PATH_RTILE || !htile_ok(geom.n, MODE_BURGERS)) return false;
    return htile_chunk(geom.n, MODE_BURGERS) == 32 && geom.n / 32 <= 32 && !g->t.der1.direct && !htile_narrow();      // 32 chunks: 1024-point lines on 16-line tiles
}

bool tlab_internal_burgers_acc_n(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, int nf, const double *nu, const double *const *s,
                                 const double *vel, double *const *result, bool overwrite, const int *finish, double dte, double kco,
                                 int scale, double *divx, double idte, unsigned fresh_mask, const double *ari, const int *clip, const double *clip_lo,
                                 const double *clip_hi) {
    check_common(dir, g, nx, ny, nz, ibc);
    if (nf < 1 || nf > 4) throw Fail(TLAB_EINVAL, "1 to 4 fields per call");
    if (tlab_internal_anelastic() && !ari) return false;      // the operator state says anelastic: the plain fused kernels would drop the density weight
    const LineGeom geom = line_geom(dir, nx, ny, nz);
    if (geom.n == 1) return false;
    OpExtra ex;
    ex.acc = !overwrite;        // overwrite: the tendency is known to be zero (start of a Runge-Kutta step): neither zero-filled nor read
    ex.fresh_mask = fresh_mask; // ... or only that of some fields
    if (tlab_internal_dealiasing()) return false;
    if (ari) {      // anelastic: ribackground [ny] (device) on the diffusion term; the epilogues are forms of the incompressible driver
        if (finish || divx || !tlab_internal_burgers_fusable_anelastic(dir, g, nx, ny, nz)) return false;
        ex.ari = ari; ex.ari_mode = dir == 2 ? 1 : 2; ex.ari_nx = nx; ex.ari_ny = ny;
    }
    ex.nf = nf;
    for (int f = 0; f < nf; ++f) { ex.fs[f] = s[f]; ex.fo[f] = result[f]; ex.fnu[f] = nu[f]; }
    if (finish) {
        if (!tlab_internal_burgers_can_finish(dir, g, nx, ny, nz)) throw Fail(TLAB_EINVAL, "internal: this Burgers launch cannot finish a field");
        for (int f = 0; f < nf; ++f) ex.ffin[f] = finish[f];
        ex.fdte = dte; ex.fkco = kco; ex.fscale = scale; ex.fny = ny;
        if (clip)      // scalar bounds of the finished fields (mode 1: every line, 2: interior lines only)
            for (int f = 0; f < nf; ++f)
                if (finish[f] && clip[f]) { ex.fclip[f] = clip[f]; ex.flo[f] = clip_lo[f]; ex.fhi[f] = clip_hi[f]; }
    } else if (clip) {
        for (int f = 0; f < nf; ++f)
            if (clip[f]) throw Fail(TLAB_EINVAL, "internal: bounds without a finishing launch");
    }
    if (divx) {      // divx: the launch also writes (x) / adds (y, z) d/dx (h + idte vel) of the field that is the velocity itself (a term of the pressure forcing)
        if (!(dir == 1 ? tlab_internal_burgers_can_finish(dir, g, nx, ny, nz) : tlab_internal_burgers_can_div(dir, g, nx, ny, nz)))
            throw Fail(TLAB_EINVAL, "internal: this Burgers launch cannot write the forcing term");
        ex.fdiv = divx; ex.fidte = idte;
    }
    const bool corr = g->t.der2.need_1der || g->t.der2.direct;
    const int path = choose_path(dir, geom.n, g);
    if (path == PATH_XLINE && !corr) {
        if (fresh_mask) throw Fail(TLAB_EINVAL, "internal: per-field overwrite is a feature of the y / z tile kernel");
        run_xline(g, geom, MODE_BURGERS, ibc, s[0], vel, result[0], nullptr, nu[0], ex);
    } else if (path == PATH_RTILE && htile_ok(geom.n, MODE_BURGERS)) {
        if (divx && (nf != 1 || s[0] != vel || !tlab_internal_burgers_can_div(dir, g, nx, ny, nz)))
            throw Fail(TLAB_EINVAL, "internal: the forcing term rides on a one-field launch of the velocity component of that direction");
        run_htile(g, geom, MODE_BURGERS, ibc, s[0], vel, result[0], nullptr, nu[0], ex);
    } else {
        return false;
    }
    g_last_path = path;
    return true;
}

// tlab_finalize: the scratch field of tlab_opr_burgers goes back
void tlab_internal_operators_release() {
    delete g_ws;
    g_ws = nullptr;
}

extern "C" {

int tlab_last_kernel_path(void) { return g_last_path; }
int tlab_force_kernel_path(int path) {
    return flushed([&] { g_force_path = path; });      // the recorded substep runs with the state of before
}
int tlab_set_tuning(int key, int value) {
    return flushed([&] {      // the recorded substep runs with the state of before
        if (key == 1) rtile_force_chunk(value);
        else if (key == 2) g_htile_policy = value;
        else if (key == 3 && (value == 16 || value == 32)) htile_set_lines(value);
        else if (key == 4 && value >= 0) ptile_set_grid(value);      // persistent workgroups of k_ptile (0 = one per CU, rounded to a multiple of 8)
        else throw Fail(TLAB_EINVAL, "tlab_set_tuning: unknown key");
    });
}

// Accumulating variants (no counterpart in the reference, which always goes through a temporary and a pointwise loop,
// rhs_global_incompressible_1.f90:106-112, :257-259): fused kernels when the sizes are on a fast path, the reference's sequence otherwise.
int tlab_opr_burgers_add(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, double nu, const double *s, const double *vel,
                         double *result, double *tmp1, double *tmp2) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(dir, g, nx, ny, nz, ibc);
        if (!s || !vel || !result || result == s || result == vel) throw Fail(TLAB_EINVAL, "tlab_opr_burgers_add: null or aliased arrays");
        if (tlab_internal_burgers_acc(dir, g, nx, ny, nz, ibc, nu, s, vel, result)) return;
        if (!tmp1 || !tmp2 || tmp1 == tmp2 || tmp1 == result || tmp2 == result) throw Fail(TLAB_EINVAL, "tlab_opr_burgers_add: the unfused path needs tmp1, tmp2");
        const int rc = tlab_opr_burgers(dir, g, s == vel ? TLAB_OPR_B_SELF : TLAB_OPR_B_U_IN, nx, ny, nz, ibc, nu, s, vel, tmp1, tmp2, 0);
        if (rc != TLAB_OK) throw Fail(TLAB_EINVAL, std::string("tlab_opr_burgers_add: ") + tlab_last_error());
        hk(launch_add1(result, tmp1, (long long)nx * ny * nz, tlab_current_stream()), "k_add1");
    });
}

int tlab_opr_burgers_add_n(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, int nf, const double *nu, const double *const *s,
                           const double *vel, double *const *result, double *tmp1, double *tmp2, int overwrite) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(dir, g, nx, ny, nz, ibc);
        if (nf < 1 || nf > 4 || !nu || !s || !vel || !result) throw Fail(TLAB_EINVAL, "tlab_opr_burgers_add_n: bad arguments (1 to 4 fields)");
        for (int f = 0; f < nf; ++f)
            if (!s[f] || !result[f] || result[f] == s[f] || result[f] == vel) throw Fail(TLAB_EINVAL, "tlab_opr_burgers_add_n: null or aliased arrays");
        if (!tlab_internal_anelastic() &&
            tlab_internal_burgers_acc_n(dir, g, nx, ny, nz, ibc, nf, nu, s, vel, result, overwrite != 0, nullptr, 0.0, 1.0, 0, nullptr, 0.0, 0u, nullptr, nullptr, nullptr, nullptr)) return;
        for (int f = 0; f < nf; ++f) {
            if (overwrite) hk(hipMemsetAsync(result[f], 0, (size_t)nx * ny * nz * sizeof(double), tlab_current_stream()), "memset");
            const int rc = tlab_opr_burgers_add(dir, g, nx, ny, nz, ibc, nu[f], s[f], vel, result[f], tmp1, tmp2);
            if (rc != TLAB_OK) throw Fail(TLAB_EINVAL, std::string("tlab_opr_burgers_add_n: ") + tlab_last_error());
        }
    });
}

int tlab_opr_gradient_final(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, const double *p, double *q, double *h, double dte, double kco,
                            int scale, double *tmp1) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(dir, g, nx, ny, nz, 0);
        if (!p || !q || !h || q == h || p == q || p == h) throw Fail(TLAB_EINVAL, "tlab_opr_gradient_final: null or aliased arrays");
        if (tlab_internal_gradient_final(dir, g, nx, ny, nz, p, q, h, dte, kco, scale, nullptr, nullptr)) return;
        if (!tmp1 || tmp1 == p || tmp1 == q || tmp1 == h) throw Fail(TLAB_EINVAL, "tlab_opr_gradient_final: the unfused path needs tmp1");
        const int rc = tlab_opr_partial(dir, g, TLAB_OPR_P1, nx, ny, nz, 0, p, tmp1, nullptr);
        if (rc != TLAB_OK) throw Fail(TLAB_EINVAL, std::string("tlab_opr_gradient_final: ") + tlab_last_error());
        hk(launch_final_update(q, h, tmp1, nullptr, nullptr, dte, kco, scale, nx, ny, nz, tlab_current_stream()), "k_final_update");
    });
}

int tlab_opr_partial_add(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, const double *u, const double *ub, double scale,
                         double *result, int acc, double *tmp1, double *tmp2) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(dir, g, nx, ny, nz, ibc);
        if (!u || !result || result == u || result == ub) throw Fail(TLAB_EINVAL, "tlab_opr_partial_add: null or aliased arrays");
        if (tlab_internal_partial_p1_fused(dir, g, nx, ny, nz, ibc, u, ub, scale, result, acc != 0)) return;
        if (!tmp1 || !tmp2 || tmp1 == tmp2 || tmp1 == result || tmp2 == result) throw Fail(TLAB_EINVAL, "tlab_opr_partial_add: the unfused path needs tmp1, tmp2");
        const long long n = (long long)nx * ny * nz;
        const double *operand = u;
        if (ub) {
            hk(launch_axpy1(tmp1, u, ub, scale, n, tlab_current_stream()), "k_axpy1");
            operand = tmp1;
        }
        const int rc = tlab_opr_partial(dir, g, TLAB_OPR_P1, nx, ny, nz, ibc, operand, acc ? tmp2 : result, nullptr);
        if (rc != TLAB_OK) throw Fail(TLAB_EINVAL, std::string("tlab_opr_partial_add: ") + tlab_last_error());
        if (acc) hk(launch_add1(result, tmp2, n, tlab_current_stream()), "k_add1");
    });
}

// BOUNDARY_BCS_NEUMANN_Y (tools/dns/boundary_bcs.f90:368-473): the reduced derivative (zero at the chosen walls) is the ordinary
// OPR_Partial_Y under ibc; the wall values follow from the first / last row of the compact scheme in a plane kernel.
int tlab_boundary_bcs_neumann_y(tlab_fdm_plan_t g, int ibc, int nx, int ny, int nz, const double *u, double *bcs_hb, double *bcs_ht,
                                double *tmp1) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(2, g, nx, ny, nz, ibc);
        if (ibc != BCS_ND && ibc != BCS_DN && ibc != BCS_NN) throw Fail(TLAB_EINVAL, "BOUNDARY_BCS_NEUMANN_Y: ibc must be 1 (jmin), 2 (jmax) or 3 (both)");
        if (g->t.periodic) throw Fail(TLAB_EINVAL, "BOUNDARY_BCS_NEUMANN_Y: periodic direction");
        if (!u || !tmp1 || u == tmp1 || !bcs_hb || !bcs_ht) throw Fail(TLAB_EINVAL, "BOUNDARY_BCS_NEUMANN_Y: null or aliased arrays");
        double cb[4], ct[4];
        tlab_internal_neumann_y_coefficients(g, ibc, ny, cb, ct);
        const int rc = tlab_opr_partial(2, g, TLAB_OPR_P1, nx, ny, nz, ibc, u, tmp1, nullptr);
        if (rc != TLAB_OK) throw Fail(TLAB_EINVAL, std::string("BOUNDARY_BCS_NEUMANN_Y: ") + tlab_last_error());
        hk(launch_neumann_planes(u, tmp1, cb, ct, (ibc & 1), (ibc & 2), bcs_hb, bcs_ht, nx, ny, nz, tlab_current_stream()), "k_neumann_planes");
    });
}

int tlab_opr_partial(int dir, tlab_fdm_plan_t g, int type, int nx, int ny, int nz, int ibc, const double *u,
                     double *result, double *tmp1) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(dir, g, nx, ny, nz, ibc);
        if (!u || !result || u == result || (tmp1 && (tmp1 == u || tmp1 == result))) throw Fail(TLAB_EINVAL, "u, result, tmp1 must be distinct");
        if (type >= TLAB_OPR_P1_INT_VP && type <= TLAB_OPR_P0_INT_PV) {
            // interpolatory operators of the staggered pressure grid (opr_partial.f90:110-120, :228-238 -> FDM_Interpol / FDM_Interpol_Der1,
            // fdm_interpolate.f90:98-160): a 4-point right-hand side and the periodic tridiagonal LU of g%intl -- the same shape as the periodic
            // compact FILTER (5-point per-row right-hand side + TRIDPSS), so they run as four such filter objects per plan (k_filter1d)
            if (dir == 2) throw Fail(TLAB_EUNSUPPORTED, "interpolatory operators along y are not built (the RHS staggers x and z only)");
            if (!g->t.stagger) throw Fail(TLAB_EINVAL, "the plan has no interpolation tables: tlab_fdm_plan_set_stagger");
            if ((dir == 1 ? nx : nz) == 1) throw Fail(TLAB_EINVAL, "interpolatory operator along a direction of one point");
            const int k = type - TLAB_OPR_P1_INT_VP;      // 0 P1 VP, 1 P1 PV, 2 P0 VP, 3 P0 PV
            if (!g->interp[k]) {
                const int n = g->t.n;
                const double c0 = 1.0 / 15.0, c1 = 17.0 / 189.0;      // fdm_com0_jacobian.f90:61, :338
                const double st[4][5] = {{0.0, -c1, -1.0, 1.0, c1},       // (u(i+1) - u(i)) + c (u(i+2) - u(i-1))      :347
                                         {-c1, -1.0, 1.0, c1, 0.0},       // (u(i) - u(i-1)) + c (u(i+1) - u(i-2))      :380
                                         {0.0, c0, 1.0, 1.0, c0},         // u(i+1) + u(i) + c (u(i+2) + u(i-1))        :70
                                         {c0, 1.0, 1.0, c0, 0.0}};        // u(i) + u(i-1) + c (u(i+1) + u(i-2))        :102
                std::vector<double> tab((size_t)10 * n);
                for (int q = 0; q < 5; ++q)
                    for (int i = 0; i < n; ++i) tab[(size_t)q * n + i] = st[k][q];
                const std::vector<double> &lu = (k < 2) ? g->t.lu1i : g->t.lu0i;
                std::copy(lu.begin(), lu.end(), tab.begin() + (size_t)5 * n);
                ok(tlab_filter_create(&g->interp[k], TLAB_FILTER_COMPACT, n, 1, 0, 0, 10, tab.data()));
            }
            tlab_internal_filter_1d(dir, g->interp[k], nx, ny, nz, u, result, tlab_current_stream());
            g_last_path = PATH_GENERIC;
            return;
        }
        if (type != TLAB_OPR_P1 && type != TLAB_OPR_P2 && type != TLAB_OPR_P2_P1)
            throw Fail(TLAB_EUNSUPPORTED, "OPR_Partial type not built on the device (the IBM variants stay on the CPU path)");
        const long long ntot = (long long)nx * ny * nz;
        const LineGeom geom = line_geom(dir, nx, ny, nz);
        if (geom.n == 1) {  // 2-D guard (opr_partial.f90:175-177, :287-289)
            hk(launch_fill(result, 0.0, ntot, tlab_current_stream()), "fill");
            if (type == TLAB_OPR_P2_P1 && tmp1) hk(launch_fill(tmp1, 0.0, ntot, tlab_current_stream()), "fill");
            return;
        }
        const bool corr = g->t.der2.need_1der;
        if (type == TLAB_OPR_P2_P1 && !tmp1) throw Fail(TLAB_EINVAL, "OPR_P2_P1 needs tmp1");
        if (type == TLAB_OPR_P2 && corr && !tmp1) throw Fail(TLAB_EINVAL, "OPR_P2 on a non-uniform grid needs tmp1 (opr_partial.f90:96)");
        int path = choose_path(dir, geom.n, g);
        if (path == PATH_XLINE && (corr || g->t.der2.direct) && type != TLAB_OPR_P1) path = PATH_GENERIC;  // non-uniform / direct-scheme x: rare, generic kernel
        g_last_path = path;
        if (path == PATH_XLINE) {
            const int mode = (type == TLAB_OPR_P1) ? MODE_P1 : (type == TLAB_OPR_P2) ? MODE_P2 : MODE_P2_P1;
            run_xline(g, geom, mode, ibc, u, nullptr, result, tmp1, 0.0);
        } else if (path == PATH_RTILE) {
            const bool r64 = rtile_chunk(geom.n) > 0 && g_htile_policy != 2;     // 64-line tiles: best for one line-set
            if (type == TLAB_OPR_P1) {
                if (r64) run_p1_tile(g, geom, ibc, u, result);
                else run_htile(g, geom, MODE_P1, ibc, u, nullptr, result, nullptr, 0.0);
            } else if (type == TLAB_OPR_P2_P1 && htile_ok(geom.n, MODE_P2_P1)) {
                run_htile(g, geom, MODE_P2_P1, ibc, u, nullptr, result, tmp1, 0.0);              // fused, one load of u
            } else if (type == TLAB_OPR_P2 && ((corr && htile_ok(geom.n, MODE_P2)) || !r64)) {
                run_htile(g, geom, MODE_P2, ibc, u, nullptr, result, nullptr, 0.0);              // first derivative stays in registers
            } else {
                const bool need_d1 = corr || type == TLAB_OPR_P2_P1;
                if (need_d1) run_rtile(g, geom, MODE_P1, ibc, u, nullptr, nullptr, tmp1, 0.0);
                if (corr) run_rtile(g, geom, MODE_P2_D1IN, ibc, u, tmp1, nullptr, result, 0.0);
                else run_rtile(g, geom, MODE_P2, ibc, u, nullptr, nullptr, result, 0.0);
            }
        } else {
            if (type == TLAB_OPR_P1) {
                run_generic(g, geom, 1, ibc, u, nullptr, result);
            } else {
                const bool need_d1 = corr || type == TLAB_OPR_P2_P1;
                if (need_d1) run_generic(g, geom, 1, ibc, u, nullptr, tmp1);
                run_generic(g, geom, 2, 0, u, corr ? tmp1 : nullptr, result);
            }
        }
    });
}

// nse_eqns == DNS_EQNS_ANELASTIC: the state OPR_Burgers_Initialize keeps in module variables (rhoinv(1), rhoinv(3), the modified U factors of
// fdmDiffusion(2); physics/opr_burgers.f90:128-183)
static std::unique_ptr<DeviceArray> g_anelastic_ri;
static int g_anelastic_ny = 0;
// the host copies and a change counter: the RHS drivers (rhs.cpp) follow this state instead of keeping one of their own that could disagree with it
static std::vector<double> g_anelastic_rb_host, g_anelastic_ri_host;
static unsigned long g_anelastic_version = 0;
int tlab_opr_burgers_set_anelastic(int ny, const double *rbackground, const double *ribackground) {
    return flushed([&] {      // the recorded substep runs with the state of before
        if (ny <= 0 || !rbackground || !ribackground) {      // back to the incompressible operator
            g_anelastic_ri.reset();
            g_anelastic_ny = 0;
            g_anelastic_rb_host.clear(); g_anelastic_ri_host.clear();
            ++g_anelastic_version;
            return;
        }
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        // along y the reference scales U's inverse diagonal by ribackground(j) and its superdiagonal by rbackground(j+1): x'(j) = x(j) ribackground(j)
        // provided rbackground * ribackground = 1, which is what the profiles of Thermo_Anelastic are; anything else is not the anelastic operator
        for (int j = 0; j < ny; ++j)
            if (std::fabs(rbackground[j] * ribackground[j] - 1.0) > 1e-14) throw Fail(TLAB_EINVAL, "ribackground must be 1 / rbackground");
        g_anelastic_ri = std::make_unique<DeviceArray>();
        g_anelastic_ri->upload(std::vector<double>(ribackground, ribackground + ny));
        g_anelastic_ny = ny;
        g_anelastic_rb_host.assign(rbackground, rbackground + ny);
        g_anelastic_ri_host.assign(ribackground, ribackground + ny);
        ++g_anelastic_version;
    });
}
bool tlab_internal_anelastic() { return g_anelastic_ny > 0; }
// ny of the profiles (0: incompressible), the host copies and the change counter
int tlab_internal_anelastic_state(const double **rb, const double **rib, unsigned long *version) {
    *rb = g_anelastic_rb_host.data(); *rib = g_anelastic_ri_host.data(); *version = g_anelastic_version;
    return g_anelastic_ny;
}

// [Dealiasing] (physics/opr_burgers.f90:33, 71, 118-125): Dealiasing(1:3), one filter per direction (NULL = DNS_FILTER_NONE); NOT owned
static tlab_filter_t g_dealias[3] = {nullptr, nullptr, nullptr};
static DeviceArray *g_wsd[2] = {nullptr, nullptr};      // wrkdea(:, 1:2) (:34, :124): filtered velocity and filtered ds/dx
int tlab_opr_burgers_set_dealiasing(int dir, tlab_filter_t f) {
    return flushed([&] {      // the recorded substep runs with the state of before
        if (dir < 1 || dir > 3) throw Fail(TLAB_EINVAL, "dir must be 1, 2 or 3");
        g_dealias[dir - 1] = f;
    });
}
bool tlab_internal_dealiasing() { return g_dealias[0] || g_dealias[1] || g_dealias[2]; }
// a filter that is being destroyed while still set as Dealiasing(dir) is taken out (tlab_filter_destroy): no dangling pointer in the Burgers operators
void tlab_internal_dealiasing_forget(tlab_filter_t f) {
    for (int i = 0; i < 3; ++i)
        if (g_dealias[i] == f) g_dealias[i] = nullptr;
}
static double *dealias_ws(int k, size_t n) {
    if (!g_wsd[k]) g_wsd[k] = new DeviceArray();
    return g_wsd[k]->reserve(n, "hipMalloc(wrkdea)");
}

int tlab_opr_burgers(int dir, tlab_fdm_plan_t g, int ivel, int nx, int ny, int nz, int ibc, double nu, const double *s,
                     const double *u, double *result, double *tmp1, int write_transposed) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        check_common(dir, g, nx, ny, nz, ibc);
        if (ivel != TLAB_OPR_B_SELF && ivel != TLAB_OPR_B_U_IN) throw Fail(TLAB_EINVAL, "ivel must be OPR_B_SELF or OPR_B_U_IN");
        if (!s || !result || !tmp1 || s == result || tmp1 == s || tmp1 == result) throw Fail(TLAB_EINVAL, "s, result, tmp1 must be distinct");
        const double *vel = (ivel == TLAB_OPR_B_SELF) ? s : u;
        if (!vel || vel == result || vel == tmp1) throw Fail(TLAB_EINVAL, "velocity must not alias result / tmp1");
        const long long ntot = (long long)nx * ny * nz;
        const LineGeom geom = line_geom(dir, nx, ny, nz);
        if (geom.n == 1) {  // opr_burgers.f90:207-210
            hk(launch_fill(result, 0.0, ntot, tlab_current_stream()), "fill");
            return;
        }
        const bool corr = g->t.der2.need_1der;
        const bool wt = write_transposed && ivel == TLAB_OPR_B_SELF && (dir == 1 || (dir == 2 && nz > 1));
        if (wt && !g_ws) g_ws = new DeviceArray();
        double *d1 = wt ? g_ws->reserve((size_t)ntot, "hipMalloc(workspace)") : tmp1;
        int path = choose_path(dir, geom.n, g);
        if (path == PATH_XLINE && (corr || g->t.der2.direct)) path = PATH_GENERIC;
        g_last_path = path;
        if (g_anelastic_ny > 0 || g_dealias[dir - 1]) {      // OPR_Burgers_1D with rhoinv (opr_burgers.f90:504-507) and / or dealiasing (:478-500):
            // the two derivatives unfused, then filter(u) and filter(ds/dx) if asked for, then the (weighted) sum
            if (g_anelastic_ny > 0 && g_anelastic_ny != ny) throw Fail(TLAB_EINVAL, "anelastic profiles were given for another ny");
            ok(tlab_opr_partial(dir, g, TLAB_OPR_P2_P1, nx, ny, nz, ibc, s, result, d1));
            const double *uf = vel, *dsf = d1;
            if (g_dealias[dir - 1]) {
                double *w1 = dealias_ws(0, (size_t)ntot), *w2 = dealias_ws(1, (size_t)ntot);
                tlab_internal_filter_1d(dir, g_dealias[dir - 1], nx, ny, nz, vel, w1, tlab_current_stream());
                tlab_internal_filter_1d(dir, g_dealias[dir - 1], nx, ny, nz, d1, w2, tlab_current_stream());
                uf = w1; dsf = w2;
            }
            if (g_anelastic_ny > 0)
                hk(launch_burgers_epilogue_anelastic(result, uf, dsf, nu, g_anelastic_ri->p, nx, ny, ntot, tlab_current_stream()), "burgers epilogue (anelastic)");
            else
                hk(launch_burgers_epilogue(result, uf, dsf, nu, ntot, tlab_current_stream()), "burgers epilogue");
        } else if (path == PATH_XLINE) {
            run_xline(g, geom, MODE_BURGERS, ibc, s, vel, result, nullptr, nu);
        } else if (path == PATH_RTILE && htile_ok(geom.n, MODE_BURGERS)) {
            run_htile(g, geom, MODE_BURGERS, ibc, s, vel, result, nullptr, nu);                  // fully fused: s and vel read once
        } else if (path == PATH_RTILE) {
            run_rtile(g, geom, MODE_P1, ibc, s, nullptr, nullptr, d1, 0.0);
            run_rtile(g, geom, MODE_BURGERS_D1IN, ibc, s, d1, vel, result, nu);
        } else {
            run_generic(g, geom, 1, ibc, s, nullptr, d1);
            run_generic(g, geom, 2, 0, s, corr ? d1 : nullptr, result);
            hk(launch_burgers_epilogue(result, vel, d1, nu, ntot, tlab_current_stream()), "burgers epilogue");
        }
        if (wt) {  // transposed operand exactly as the reference leaves it in tmp1 (opr_burgers.f90:250, :315)
            if (dir == 1) hk(launch_transpose(s, tmp1, nx, ny * nz, tlab_current_stream()), "transpose");
            else hk(launch_transpose(s, tmp1, nx * ny, nz, tlab_current_stream()), "transpose");
        }
    });
}

int tlab_transpose(const double *a, int nra, int nca, double *b) {
    return flushed([&] {      // a recorded substep runs first (csrc/deferred.cpp)
        if (!a || !b || a == b || nra < 1 || nca < 1) throw Fail(TLAB_EINVAL, "tlab_transpose: bad arguments");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called");
        hk(launch_transpose(a, b, nra, nca, tlab_current_stream()), "transpose");
    });
}

}  // extern "C"
