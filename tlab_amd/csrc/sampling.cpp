// C ABI of the sampling between two statistics steps (include/tlab_amd.h): the phase averages tlab_avg_phase_space / _flow / _plane_id, the towers
// tlab_tower_*, the saved planes tlab_planes_gather with tlab_fi_gradient and tlab_log10_small, and tlab_dns_arm_pressure_sampling, whose samples
// rhs.cpp takes between the pressure solve and the pressure gradient.  Device arrays take the kernels of sampling.hip, host arrays the loops below,
// which are the reference's statements; a host array never reaches a kernel, a device array is never read by the host.  Nothing here synchronises
// the stream: the accumulators are the caller's and stay where they are.  From stats_common.hpp: on_device and Scratch.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "averages_host.hpp"
#include "dns_state.hpp"
#include "stats_common.hpp"

#pragma clang fp contract(off)      // every multiply, add and division below stays as written

using namespace tlab;

// DNS_TOWER's module state (dns_tower.f90:36-56): where the towers stand, which slot of the buffer the next call fills
struct tlab_tower {
    int nx, ny, nz, nsave;                  // the box; tower_isize_acc_write = nitera_save
    std::vector<int> ipos, jpos, kpos;      // tower_ipos, tower_jpos, tower_kpos (1-based)
    int *dpos = nullptr;                    // ... on the device (ipos | jpos | kpos), made by the first call on device arrays
    int accumulation = 1, mode_check = 0;   // tower_accumulation, tower_mode_check
    long long acc_field = 0, acc_mean = 0;  // tower_isize_acc_field, tower_isize_acc_mean
    int ti() const { return (int)ipos.size(); }
    int tj() const { return (int)jpos.size(); }
    int tk() const { return (int)kpos.size(); }
    long long bufsize() const { return 5 * acc_field + 5 * acc_mean + 2LL * nsave; }
    ~tlab_tower() { if (dpos) (void)hipFree(dpos); }
};

namespace {

Scratch g_scratch("hipMalloc(tower means)");      // partials and profile of the tower means

// ---- phase averages ----
// the planes of output o of an accumulator avg(nxy, avg_planes + 1, nout): this sample's (plane_id, 1-based) and the running mean (the last one)
double *phase_plane(double *avg, long long nxy, int avg_planes, int o, int plane) {
    return avg + ((long long)o * (avg_planes + 1) + plane) * nxy;
}

// localsum = localsum + field(:,:,k)/g(3)%size (avg_phase.f90:168-174; with g: wrk3d = f*g first, :254-261), then :186, :195 (:273, :282)
void host_phase(long long nxy, int nz, double dz, double dplanes, const double *f, const double *g, double *out, double *last) {
    std::vector<double> localsum((size_t)nxy, 0.0);
    for (int k = 0; k < nz; ++k) {
        const double *a = f + (long long)k * nxy, *b = g ? g + (long long)k * nxy : nullptr;
        for (long long p = 0; p < nxy; ++p) {
            const double x = b ? a[p] * b[p] : a[p];
            localsum[p] = localsum[p] + x / dz;
        }
    }
    for (long long p = 0; p < nxy; ++p) out[p] = localsum[p];
    for (long long p = 0; p < nxy; ++p) last[p] = last[p] + out[p] / dplanes;
}

void check_phase(const std::string &who, int nx, int ny, int nz, int nz_total, int avg_planes, int plane_id) {
    if (nx < 1 || ny < 1 || nz < 1 || nz_total < 1) throw Fail(TLAB_EINVAL, who + ": nx, ny, nz and nz_total must be at least 1");
    if (avg_planes < 1) throw Fail(TLAB_EINVAL, who + ": avg_planes must be at least 1 (the running mean divides by it)");
    if (plane_id < 1 || plane_id > avg_planes) throw Fail(TLAB_EINVAL, who + ": plane_id must be 1 to avg_planes");
}

void phase_space(bool dev, int nx, int ny, int nz, int nz_total, int nf, const double *const *f, int avg_planes, int plane_id, double *avg) {
    const long long nxy = (long long)nx * ny;
    if (!dev) {
        for (int i = 0; i < nf; ++i)
            host_phase(nxy, nz, (double)nz_total, (double)avg_planes, f[i], nullptr, phase_plane(avg, nxy, avg_planes, i, plane_id - 1),
                       phase_plane(avg, nxy, avg_planes, i, avg_planes));
        return;
    }
    for (int f0 = 0; f0 < nf; f0 += 3) {
        const int n = std::min(3, nf - f0);
        double *out[3], *last[3];
        for (int i = 0; i < n; ++i) {
            out[i] = phase_plane(avg, nxy, avg_planes, f0 + i, plane_id - 1);
            last[i] = phase_plane(avg, nxy, avg_planes, f0 + i, avg_planes);
        }
        hk(launch_phase_space(n, false, f + f0, out, last, nxy, nz, nz_total, avg_planes, tlab_current_stream()), "k_phase_space");
    }
}

// ---- towers ----
enum { TOWER_U, TOWER_V, TOWER_W, TOWER_P, TOWER_S };      // the order of the buffer (dns_tower.f90:188-200)

// TOWER_AVG_IK_V (dns_tower.f90:502-546): k outer, i inner, at the planes tower_jpos, divided by a default real
void host_tower_means(const tlab_tower *t, const double *a, double *avg) {
    const int tj = t->tj();
    for (int j = 0; j < tj; ++j) avg[j] = 0.0;
    for (int k = 0; k < t->nz; ++k)
        for (int j = 0; j < tj; ++j) {
            const double *row = a + ((size_t)k * t->ny + (t->jpos[j] - 1)) * t->nx;
            for (int i = 0; i < t->nx; ++i) avg[j] = avg[j] + row[i];
        }
    const double denom = (double)(float)((long long)t->nx * t->nz);
    for (int j = 0; j < tj; ++j) avg[j] = avg[j] / denom;
}

// DNS_TOWER_ACCUMULATE (dns_tower.f90:207-289) on arrays of one kind; the state advances only when every launch is enqueued
void tower_accumulate(tlab_tower *t, bool dev, int index, const double *const *f, int itime, double rtime, double *buf) {
    const char *who = "tlab_tower_accumulate";
    if (t->mode_check + index > 7)
        throw Fail(TLAB_EINVAL, std::string(who) + ": tower_mode_check greater than 7 (each of the indices 4, 1, 2 once per time step)");
    if (t->accumulation > t->nsave) throw Fail(TLAB_EINVAL, std::string(who) + ": the buffer is full (tlab_tower_reset after it has been written)");
    const int nf = index == 1 ? 3 : 1, slot0 = index == 1 ? TOWER_U : index == 2 ? TOWER_S : TOWER_P;
    const int ti = t->ti(), tj = t->tj(), tk = t->tk();
    const long long tip = (long long)ti * tk, acc = t->accumulation - 1;
    double *dst[3], *mean[3], *t_slot = nullptr, *it_slot = nullptr;
    for (int i = 0; i < nf; ++i) {
        dst[i] = buf + (slot0 + i) * t->acc_field + acc * tj * tip;
        mean[i] = buf + 5 * t->acc_field + (slot0 + i) * t->acc_mean + acc * tj;
    }
    if (index == 4) {      // tower_t(tower_accumulation) = rtime, tower_it(tower_accumulation) = itime (:236-237)
        t_slot = buf + 5 * t->acc_field + 5 * t->acc_mean + acc;
        it_slot = t_slot + t->nsave;
    }
    if (dev) {
        hipStream_t st = tlab_current_stream();
        if (!t->dpos) {
            std::vector<int> h(t->ipos);
            h.insert(h.end(), t->jpos.begin(), t->jpos.end());
            h.insert(h.end(), t->kpos.begin(), t->kpos.end());
            hk(hipMalloc((void **)&t->dpos, std::max<size_t>(h.size(), 1) * sizeof(int)), "hipMalloc(tower positions)");
            hk(hipMemcpy(t->dpos, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(tower positions)");
        }
        const int *ipos = t->dpos, *jpos = ipos + ti, *kpos = jpos + tj;
        hk(launch_tower_gather(nf, f, dst, ipos, jpos, kpos, ti, tj, tk, t->nx, t->ny, t_slot, it_slot, rtime, itime, st), "k_tower_gather");
        const size_t npart = (size_t)plane_moments_chunks(t->nz) * t->ny * nf;
        double *partial = g_scratch.doubles(npart + (size_t)nf * t->ny), *prof = partial + npart;
        hk(launch_plane_moments(AVG_PROG_MEANS, nf, t->nx, t->ny, t->nz, f, nullptr, partial, prof, st, (double)(float)((long long)t->nx * t->nz)),
           "k_plane_partial");
        hk(launch_tower_means(prof, t->ny, jpos, tj, nf, mean, st), "k_tower_means");
    } else {
        if (t_slot) { *t_slot = rtime; *it_slot = (double)itime; }
        for (int i = 0; i < nf; ++i) {
            long long ip = 0;
            for (int kk = 0; kk < tk; ++kk)
                for (int ii = 0; ii < ti; ++ii)
                    for (int j = 0; j < tj; ++j)
                        dst[i][ip++] = f[i][((size_t)(t->kpos[kk] - 1) * t->ny + (t->jpos[j] - 1)) * t->nx + (t->ipos[ii] - 1)];
            host_tower_means(t, f[i], mean[i]);
        }
    }
    t->mode_check += index;
    if (t->mode_check == 7) { t->mode_check = 0; t->accumulation += 1; }
}

// the positions of one direction (dns_tower.f90:116-132, :164-186, one rank): counted with mod(i - 1, stride), placed with mod(i, stride)
bool tower_positions(int n, int stride, std::vector<int> &pos) {
    int count = 0;
    for (int i = 0; i < n; ++i) count += (i - 1) % stride == 0 ? 1 : 0;      // (C's % has Fortran mod's sign)
    pos.clear();
    for (int i = 0; i < n; ++i)
        if (i % stride == 0) pos.push_back(i + 1);
    return (int)pos.size() == count;
}

}  // namespace

// the samples of an armed substep (rhs.cpp, between the solve and the gradient): p is the pressure on the velocity nodes, device memory
void tlab::pressure_sampling(tlab_dns *d, const tlab_dns::PressureSampling &ps, const double *p) {
    if (ps.tower) tower_accumulate(ps.tower, true, 4, &p, ps.itime, ps.rtime, ps.tower_buf);
    if (ps.phase_avg) phase_space(true, d->nx, d->ny, d->nz, d->nz_total > 0 ? d->nz_total : d->nz, 1, &p, ps.avg_planes, ps.plane_id, ps.phase_avg);
}

extern "C" {

int tlab_avg_phase_plane_id(int itr, int it_first, int it_save) {
    return it_save != 0 ? ((itr - 1) - it_first) % it_save + 1 : 1;      // avg_phase.f90:142-143 (C's % has Fortran mod's sign)
}

int tlab_avg_phase_space(int nx, int ny, int nz, int nz_total, int nf, const double *const *fields, int avg_planes, int plane_id, double *avg) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_avg_phase_space";
        if (nf < 1 || !fields || !avg) throw Fail(TLAB_EINVAL, std::string(who) + ": nf < 1 or a null pointer");
        check_phase(who, nx, ny, nz, nz_total, avg_planes, plane_id);
        std::vector<const void *> all(fields, fields + nf);
        for (const void *p : all)
            if (!p) throw Fail(TLAB_EINVAL, std::string(who) + ": a null field");
        all.push_back(avg);
        phase_space(on_device(who, all), nx, ny, nz, nz_total, nf, fields, avg_planes, plane_id, avg);
    }, TLAB_EINVAL);
}

int tlab_avg_phase_flow(int nx, int ny, int nz, int nz_total, const double *u, const double *v, const double *w, int avg_planes, int plane_id,
                        double *avg_flow, double *avg_stress) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_avg_phase_flow";
        if (!u || !v || !w || !avg_flow || !avg_stress) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        check_phase(who, nx, ny, nz, nz_total, avg_planes, plane_id);
        const double *f[3] = {u, v, w};
        const long long nxy = (long long)nx * ny;
        double *out[9], *last[9];
        for (int o = 0; o < 9; ++o) {      // stress ids as AvgPhaseStress's calls give them (:230-235): uu 1, uv 2, uw 3, vv 4, vw 5, ww 6
            out[o] = phase_plane(o < 3 ? avg_flow : avg_stress, nxy, avg_planes, o < 3 ? o : o - 3, plane_id - 1);
            last[o] = phase_plane(o < 3 ? avg_flow : avg_stress, nxy, avg_planes, o < 3 ? o : o - 3, avg_planes);
        }
        if (on_device(who, {u, v, w, avg_flow, avg_stress})) {
            hk(launch_phase_space(3, true, f, out, last, nxy, nz, nz_total, avg_planes, tlab_current_stream()), "k_phase_space");
            return;
        }
        static const int pair[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
        for (int o = 0; o < 3; ++o) host_phase(nxy, nz, (double)nz_total, (double)avg_planes, f[o], nullptr, out[o], last[o]);
        for (int o = 0; o < 6; ++o) host_phase(nxy, nz, (double)nz_total, (double)avg_planes, f[pair[o][0]], f[pair[o][1]], out[3 + o], last[3 + o]);
    }, TLAB_EINVAL);
}

int tlab_tower_create(tlab_tower_t *out, int nx, int ny, int nz, const int *stride, int nitera_save) {
    return catch_fail([&] {
        const char *who = "tlab_tower_create";
        if (!out || !stride) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        if (nx < 1 || ny < 1 || nz < 1 || nitera_save < 1 || stride[0] < 1 || stride[1] < 1 || stride[2] < 1)
            throw Fail(TLAB_EINVAL, std::string(who) + ": the box, the strides and nitera_save must be at least 1");
        std::unique_ptr<tlab_tower> t(new tlab_tower());
        t->nx = nx; t->ny = ny; t->nz = nz; t->nsave = nitera_save;
        if (!tower_positions(nx, stride[0], t->ipos) || !tower_positions(ny, stride[1], t->jpos) || !tower_positions(nz, stride[2], t->kpos))
            throw Fail(TLAB_EINVAL, std::string(who) + ": (n - 1) is a multiple of a stride > 1: the reference counts one tower less than it places "
                                                       "(DNS_TOWER_INITIALIZE writes past tower_ipos there)");
        t->acc_field = (long long)nitera_save * t->tj() * t->ti() * t->tk();
        t->acc_mean = (long long)nitera_save * t->tj();
        *out = t.release();
    }, TLAB_EINVAL);
}

int tlab_tower_destroy(tlab_tower_t t) {
    (void)tlab_internal_deferred_flush();      // (a recorded RHS of a driver armed with this tower still samples into it)
    if (t && t->dpos && tlab_device_ready()) (void)hipStreamSynchronize(tlab_current_stream());      // (a gather may still read the positions)
    delete t;
    return TLAB_OK;
}

int tlab_tower_sizes(tlab_tower_t t, long long *sizes) {
    (void)tlab_internal_deferred_flush();      // (tower_accumulation and tower_mode_check are advanced by a recorded RHS that was armed)
    return catch_fail([&] {
        if (!t || !sizes) throw Fail(TLAB_EINVAL, "tlab_tower_sizes: a null pointer");
        const long long s[8] = {t->ti(), t->tj(), t->tk(), t->acc_field, t->acc_mean, t->bufsize(), t->accumulation, t->mode_check};
        std::copy(s, s + 8, sizes);
    }, TLAB_EINVAL);
}

int tlab_tower_positions(tlab_tower_t t, int dir, int *pos) {
    return catch_fail([&] {
        if (!t || !pos || dir < 1 || dir > 3) throw Fail(TLAB_EINVAL, "tlab_tower_positions: a null pointer, or dir outside 1..3");
        const std::vector<int> &p = dir == 1 ? t->ipos : dir == 2 ? t->jpos : t->kpos;
        std::copy(p.begin(), p.end(), pos);
    }, TLAB_EINVAL);
}

int tlab_tower_reset(tlab_tower_t t) {
    (void)tlab_internal_deferred_flush();      // (a recorded RHS that was armed stores its sample in the slot of before)
    return catch_fail([&] {
        if (!t) throw Fail(TLAB_EINVAL, "tlab_tower_reset: a null handle");
        t->accumulation = 1;      // dns_tower.f90:486 (the end of DNS_TOWER_WRITE)
        t->mode_check = 0;
    }, TLAB_EINVAL);
}

int tlab_tower_accumulate(tlab_tower_t t, int index, const double *const *fields, int itime, double rtime, double *tower_buf) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_tower_accumulate";
        if (!t || !fields || !tower_buf) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        if (index != 1 && index != 2 && index != 4) throw Fail(TLAB_EINVAL, std::string(who) + ": index must be 1 (u, v, w), 2 (the first scalar) or 4 (pressure)");
        const int nf = index == 1 ? 3 : 1;
        const void *all[4] = {tower_buf, nullptr, nullptr, nullptr};
        for (int i = 0; i < nf; ++i)
            if (!(all[1 + i] = fields[i])) throw Fail(TLAB_EINVAL, std::string(who) + ": a null field");
        tower_accumulate(t, on_device(who, all, (size_t)nf + 1), index, fields, itime, rtime, tower_buf);
    }, TLAB_EINVAL);
}

int tlab_planes_gather(int nx, int ny, int nz, int nvars, const double *const *fields, int dir, int n, const int *nodes, void *out, int single) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_planes_gather";
        if (nx < 1 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nx, ny, nz must be at least 1");
        if (nvars < 1 || nvars > PLANES_MAX_VARS || n < 1 || n > PLANES_MAX_NODES || dir < 1 || dir > 3 || !fields || !nodes || !out)
            throw Fail(TLAB_EINVAL, std::string(who) + ": 1..16 fields, 1..20 planes, dir 1..3, no null pointer");
        const int len[3] = {nx, ny, nz};
        for (int m = 0; m < n; ++m)      // PLANES_INITIALIZE (planes.f90:145-162)
            if (nodes[m] < 1 || nodes[m] > len[dir - 1]) throw Fail(TLAB_EINVAL, std::string(who) + ": plane nodes deceed / exceed the grid in this direction");
        std::vector<const void *> all(fields, fields + nvars);
        for (const void *p : all)
            if (!p) throw Fail(TLAB_EINVAL, std::string(who) + ": a null field");
        all.push_back(out);
        if (on_device(who, all)) {
            hk(launch_planes_gather(nx, ny, nz, nvars, fields, dir, n, nodes, out, single != 0, tlab_current_stream()), "k_planes_gather");
            return;
        }
        const size_t size = (size_t)nvars * n;
        auto put = [&](size_t o, double x) {
            if (single) ((float *)out)[o] = (float)x;
            else ((double *)out)[o] = x;
        };
        for (int v = 0; v < nvars; ++v)
            for (int m = 0; m < n; ++m) {
                const size_t slot = (size_t)v * n + m, node = (size_t)nodes[m] - 1;
                const double *f = fields[v];
                if (dir == 3) {          // data_k(:, :, slot) = field(:, :, node)  (:288)
                    for (size_t p = 0; p < (size_t)nx * ny; ++p) put(slot * nx * ny + p, f[node * nx * ny + p]);
                } else if (dir == 2) {   // data_j(:, slot, :) = field(:, node, :)  (:306)
                    for (size_t k = 0; k < (size_t)nz; ++k)
                        for (size_t i = 0; i < (size_t)nx; ++i) put((k * size + slot) * nx + i, f[(k * ny + node) * nx + i]);
                } else {                 // data_i(j, slot, k) = field(node, j, k)  (:332-336)
                    for (size_t k = 0; k < (size_t)nz; ++k)
                        for (size_t j = 0; j < (size_t)ny; ++j) put((k * size + slot) * ny + j, f[(k * ny + j) * nx + node]);
                }
            }
    }, TLAB_EINVAL);
}

// FI_GRADIENT (mappings/fi_gradient.f90:26-48): three OPR_Partial(OPR_P1, bcs = 0) with the driver's plans and the two statements between them
int tlab_fi_gradient(tlab_dns_t d, const double *s, double *result, double *tmp) {
    (void)tlab_internal_deferred_flush();
    return guarded([&] {
        if (!d || !s || !result || !tmp) throw Fail(TLAB_EINVAL, "tlab_fi_gradient: bad arguments");
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        const long long n = (long long)nx * ny * nz;
        hipStream_t st = tlab_current_stream();
        ok(tlab_opr_partial(1, d->g[0], TLAB_OPR_P1, nx, ny, nz, 0, s, result, nullptr), "OPR_Partial_X");
        ok(tlab_opr_partial(2, d->g[1], TLAB_OPR_P1, nx, ny, nz, 0, s, tmp, nullptr), "OPR_Partial_Y");
        hk(launch_gradient_magnitude(result, tmp, false, n, st), "k_gradient_magnitude");      // result = result*result + tmp1*tmp1
        ok(tlab_opr_partial(3, d->g[2], TLAB_OPR_P1, nx, ny, nz, 0, s, tmp, nullptr), "OPR_Partial_Z");
        hk(launch_gradient_magnitude(result, tmp, true, n, st), "k_gradient_magnitude");       // result = result + tmp1*tmp1
    });
}

int tlab_log10_small(long long n, double *a) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (n < 1 || !a) throw Fail(TLAB_EINVAL, "tlab_log10_small: n < 1 or a null pointer");
        if (on_device("tlab_log10_small", {a})) hk(launch_log10_small(a, n, tlab_current_stream()), "k_log10_small");
        else
            for (long long i = 0; i < n; ++i) a[i] = std::log10(a[i] + 1.0e-20);
    }, TLAB_EINVAL);
}

int tlab_dns_arm_pressure_sampling(tlab_dns_t d, tlab_tower_t tower, double *tower_buf, int itime, double rtime, double *phase_avg, int avg_planes,
                                   int plane_id) {
    (void)tlab_internal_deferred_flush();
    return guarded([&] {
        const char *who = "tlab_dns_arm_pressure_sampling";
        if (!d) throw Fail(TLAB_EINVAL, std::string(who) + ": null handle");
        d->psample = tlab_dns::PressureSampling();
        if ((tower == nullptr) != (tower_buf == nullptr)) throw Fail(TLAB_EINVAL, std::string(who) + ": tower and tower_buf go together");
        if (tower && (tower->nx != d->nx || tower->ny != d->ny || tower->nz != d->nz)) throw Fail(TLAB_EINVAL, std::string(who) + ": the towers are those of another box");
        if (phase_avg) check_phase(who, d->nx, d->ny, d->nz, 1, avg_planes, plane_id);
        const void *all[2] = {tower_buf, phase_avg};
        for (const void *p : all)
            if (p && tlab_pointer_on_device(p) != 1) throw Fail(TLAB_EINVAL, std::string(who) + ": the accumulators must be device memory");
        if (!tower && !phase_avg) return;      // nothing to sample: nothing armed
        d->psample.armed = true;
        d->psample.tower = tower; d->psample.tower_buf = tower_buf; d->psample.itime = itime; d->psample.rtime = rtime;
        d->psample.phase_avg = phase_avg; d->psample.avg_planes = avg_planes; d->psample.plane_id = plane_id;
    });
}

}  // extern "C"
