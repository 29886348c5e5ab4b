// C ABI of the field mappings (tlab_amd_mappings.h): tlab_gradient_maps, the pass k_gradient_maps over gradients that exist (device arrays) or
// the same arithmetic in a host loop (host arrays; a host array never reaches a kernel, a device array is never read by the host); the
// derivatives that feed it on the single-domain driver; and the diffusion and pressure terms of the enstrophy, strain and scalar-gradient
// equations, composed from tlab_opr_partial and the accumulate kernels of mappings.hip in the reference's call order.
#include "tlab_amd_mappings.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "dns_state.hpp"
#include "mappings_host.hpp"
#include "stats_common.hpp"

#pragma clang fp contract(off)      // the host loop keeps every operation as written, like the kernel

using namespace tlab;

static_assert(TLAB_MAP_COUNT == MAP_COUNT && TLAB_MAP_STRAIN_A == M_STRAIN_A && TLAB_MAP_P == M_P, "tlab_amd_mappings.h and mappings_host.hpp");

namespace {

// the selection of a call, checked: the pointers in the kernel's layout, the arrays it reads and writes
struct Selection {
    GradientMapArgs A{};
    std::vector<const void *> used;      // needed inputs, then outputs
};
Selection select(const char *who, long long n, const double *const *du9, const double *const *ds3, const int *maps, int nmaps, double *const *out) {
    if (n < 1 || n > 0x7fffffffLL) throw Fail(TLAB_EINVAL, std::string(who) + ": n must be 1 to 2^31 - 1");
    if (!du9 || !maps || !out || nmaps < 1 || nmaps > MAP_COUNT) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer, or nmaps outside 1 to 12");
    Selection S;
    int o = 0;
    for (int i = 0; i < nmaps; ++i) {
        const int m = maps[i];
        if (m < 0 || m >= MAP_COUNT) throw Fail(TLAB_EINVAL, std::string(who) + ": map " + std::to_string(m) + " is not a TLAB_MAP_* code");
        if (S.A.maps >> m & 1u) throw Fail(TLAB_EINVAL, std::string(who) + ": map " + std::to_string(m) + " is named twice");
        S.A.maps |= 1u << m;
        S.A.needs |= MAP_NEEDS[m];
        for (int k = 0; k < MAP_NOUT[m]; ++k, ++o) {
            if (!out[o]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null output");
            S.A.out[MAP_FIRST[m] + k] = out[o];
        }
    }
    if ((S.A.needs & MAP_DS) && !ds3) throw Fail(TLAB_EINVAL, std::string(who) + ": a requested map needs the scalar gradient ds3");
    std::vector<const double *> given;
    for (int k = 0; k < MAP_INPUTS; ++k) {
        const double *p = k < 9 ? du9[k] : (ds3 ? ds3[k - 9] : nullptr);
        if (p) given.push_back(p);
        if (S.A.needs >> k & 1u) {
            if (!p) throw Fail(TLAB_EINVAL, std::string(who) + ": gradient " + std::to_string(k) + " is needed and null");
            S.A.in[k] = p;
            S.used.push_back(p);
        }
    }
    for (int k = 0; k < MAP_OUTPUTS; ++k)
        if (S.A.out[k]) {
            const double *a = S.A.out[k];
            auto overlaps = [&](const double *b) { return a < b + n && b < a + n; };
            for (const double *b : given)
                if (overlaps(b)) throw Fail(TLAB_EINVAL, std::string(who) + ": an output overlaps an input");
            for (int l = 0; l < k; ++l)
                if (S.A.out[l] && overlaps(S.A.out[l])) throw Fail(TLAB_EINVAL, std::string(who) + ": two outputs overlap");
            S.used.push_back(a);
        }
    return S;
}

// a driver these entry points serve: its own whole box, velocity nodes
void check_driver(const char *who, tlab_dns_t d) {
    if (!d) throw Fail(TLAB_EINVAL, std::string(who) + ": no driver");
    if (d->stagger) throw Fail(TLAB_EUNSUPPORTED, std::string(who) + ": the staggered pressure grid is not built for the mappings");
    if (d->koffset != 0 || (d->nz_total != 0 && d->nz_total != d->nz))
        throw Fail(TLAB_EUNSUPPORTED, std::string(who) + ": a driver that holds a z-slab of a larger box is not built for the mappings");
}
void p1(tlab_dns_t d, int dir, const double *u, double *r) {
    ok(tlab_opr_partial(dir, d->g[dir - 1], TLAB_OPR_P1, d->nx, d->ny, d->nz, 0, u, r, nullptr), "OPR_Partial(OPR_P1)");
}
void p2(tlab_dns_t d, int dir, const double *u, double *r, double *wrk) {
    ok(tlab_opr_partial(dir, d->g[dir - 1], TLAB_OPR_P2, d->nx, d->ny, d->nz, 0, u, r, wrk), "OPR_Partial(OPR_P2)");
}
void velocity_gradients(const char *who, tlab_dns_t d, double *const *q, double *const *txc9) {
    if (!q || !txc9) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
    for (int i = 0; i < 9; ++i)
        if (!txc9[i] || !q[i / 3]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null velocity or txc array");
    for (int c = 0; c < 3; ++c)
        for (int dir = 1; dir <= 3; ++dir) p1(d, dir, q[c], txc9[3 * c + dir - 1]);
}
void scalar_gradient(const char *who, tlab_dns_t d, const double *s, double *const *ds3) {
    if (!s || !ds3 || !ds3[0] || !ds3[1] || !ds3[2]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null scalar or ds3 array");
    for (int dir = 1; dir <= 3; ++dir) p1(d, dir, s, ds3[dir - 1]);
}

}  // namespace

extern "C" {

int tlab_gradient_maps(long long n, const double *const *du9, const double *const *ds3, const int *maps, int nmaps, double *const *out) {
    return flushed([&] {
        const char *who = "tlab_gradient_maps";
        const Selection S = select(who, n, du9, ds3, maps, nmaps, out);
        if (on_device(who, S.used)) {
            hk(launch_gradient_maps(S.A, n, tlab_current_stream()), "k_gradient_maps");
            return;
        }
        for (long long i = 0; i < n; ++i) {
            double g[MAP_INPUTS], o[MAP_OUTPUTS];
            for (int k = 0; k < MAP_INPUTS; ++k) g[k] = (S.A.needs >> k & 1u) ? S.A.in[k][i] : 0.0;
            gradient_maps_point(S.A.maps, g, o);
            for (int m = 0; m < MAP_COUNT; ++m)
                if (S.A.maps >> m & 1u)
                    for (int k = MAP_FIRST[m]; k < MAP_FIRST[m] + MAP_NOUT[m]; ++k) S.A.out[k][i] = o[k];
        }
    });
}

int tlab_dns_velocity_gradients(tlab_dns_t d, double *const *q, double *const *txc9) {
    return flushed([&] {
        const char *who = "tlab_dns_velocity_gradients";
        check_driver(who, d);
        velocity_gradients(who, d, q, txc9);
    });
}

int tlab_dns_scalar_gradient(tlab_dns_t d, const double *s, double *const *ds3) {
    return flushed([&] {
        const char *who = "tlab_dns_scalar_gradient";
        check_driver(who, d);
        scalar_gradient(who, d, s, ds3);
    });
}

int tlab_dns_fi_maps(tlab_dns_t d, double *const *q, const double *s, const int *maps, int nmaps, double *const *txc9, double *const *ds3,
                     double *const *out) {
    return flushed([&] {
        const char *who = "tlab_dns_fi_maps";
        check_driver(who, d);
        if (!txc9) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const long long n = (long long)d->nx * d->ny * d->nz;
        // (the selection is checked before anything is enqueued; every velocity gradient is taken, as the entry point says, whatever the maps read)
        const Selection S = select(who, n, txc9, ds3, maps, nmaps, out);
        if (!on_device(who, S.used)) throw Fail(TLAB_EINVAL, std::string(who) + ": the arrays must be device memory");
        velocity_gradients(who, d, q, txc9);
        if (S.A.needs & MAP_DS) scalar_gradient(who, d, s, ds3);
        hk(launch_gradient_maps(S.A, n, tlab_current_stream()), "k_gradient_maps");
    });
}

int tlab_dns_fi_diffusion(tlab_dns_t d, int kind, double *const *q, const double *f, double *result, double *const *work6) {
    return flushed([&] {
        const char *who = "tlab_dns_fi_diffusion";
        check_driver(who, d);
        if (kind < TLAB_FI_VORTICITY_DIFFUSION || kind > TLAB_FI_STRAIN_PRESSURE) throw Fail(TLAB_EINVAL, std::string(who) + ": kind is not a TLAB_FI_* code");
        const bool needs_q = kind != TLAB_FI_GRADIENT_DIFFUSION, needs_f = kind == TLAB_FI_GRADIENT_DIFFUSION || kind == TLAB_FI_STRAIN_PRESSURE;
        if (!result || !work6 || (needs_q && (!q || !q[0] || !q[1] || !q[2])) || (needs_f && !f))
            throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        for (int i = 0; i < 6; ++i)
            if (!work6[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null work array");
        const long long n = (long long)d->nx * d->ny * d->nz;
        hipStream_t st = tlab_current_stream();
        double *fld = work6[0], *tmp1 = work6[1], *tmp2 = work6[2], *tmp3 = work6[3], *tmp4 = work6[4];
        const double *u = needs_q ? q[0] : nullptr, *v = needs_q ? q[1] : nullptr, *w = needs_q ? q[2] : nullptr;
        int terms = 0;
        // result = [result +] (c fld) (lap fld): the Laplacian in the reference's order, z, y, x
        auto laplacian_term = [&](double c) {
            p2(d, 3, fld, tmp3, tmp4);
            p2(d, 2, fld, tmp2, tmp4);
            p2(d, 1, fld, tmp1, tmp4);
            hk(launch_acc_prod3(result, c, fld, tmp1, tmp2, tmp3, terms++ ? 1 : 0, n, st), "k_acc_prod3");
        };
        // fld = (dir a of fa) + sign (dir b of fb)
        auto pair = [&](int a, const double *fa, int b, const double *fb, double sign) {
            p1(d, a, fa, tmp1);
            p1(d, b, fb, tmp2);
            hk(launch_axpy1(fld, tmp1, tmp2, sign, n, st), "k_axpy1");      // tmp1 + tmp2*(+-1): the bits of tmp1 +- tmp2
        };
        if (kind == TLAB_FI_VORTICITY_DIFFUSION) {
            pair(1, v, 2, u, -1.0); laplacian_term(1.0);
            pair(3, u, 1, w, -1.0); laplacian_term(1.0);
            pair(2, w, 3, v, -1.0); laplacian_term(1.0);
        } else if (kind == TLAB_FI_STRAIN_DIFFUSION) {
            p1(d, 1, u, fld); laplacian_term(1.0);
            p1(d, 2, v, fld); laplacian_term(1.0);
            p1(d, 3, w, fld); laplacian_term(1.0);
            pair(1, v, 2, u, 1.0); laplacian_term(0.5);
            pair(3, u, 1, w, 1.0); laplacian_term(0.5);
            pair(2, w, 3, v, 1.0); laplacian_term(0.5);
        } else if (kind == TLAB_FI_GRADIENT_DIFFUSION) {
            for (int dir = 1; dir <= 3; ++dir) { p1(d, dir, f, fld); laplacian_term(1.0); }
        } else {      // FI_STRAIN_PRESSURE; fld is not used
            for (int dir = 1; dir <= 3; ++dir) {
                p1(d, dir, q[dir - 1], tmp1);
                p2(d, dir, f, tmp2, tmp4);
                hk(launch_acc_prod2(result, tmp1, tmp2, nullptr, terms++ ? 1 : 0, n, st), "k_acc_prod2");
            }
            auto cross = [&](int a, int b, const double *fa, const double *fb) {      // result += p,ab (fa,a + fb,b)
                p1(d, a, f, tmp2);
                p1(d, b, tmp2, tmp1);
                p1(d, a, fa, tmp2);
                p1(d, b, fb, tmp3);
                hk(launch_acc_prod2(result, tmp1, tmp2, tmp3, 1, n, st), "k_acc_prod2");
            };
            cross(1, 2, v, u);
            cross(1, 3, w, u);
            cross(2, 3, w, v);
            hk(launch_negate(result, n, st), "k_negate");
        }
    });
}

}  // extern "C"
