// The tail of the Runge-Kutta substep for a host whose time loop is NOT patched (include/tlab_amd.h: tlab_deferred_*).
//
// tools/dns/time.f90 of the reference runs, per substep,
//     call RHS_GLOBAL_INCOMPRESSIBLE_1()                          (:612, link-time replacement: the whole assembly on the device)
//     call DAXPY(n, dte, hq(1,is), 1, q(1,is), 1)   is = 1..3     (:649-660, the -DUSE_BLAS branches)   q += dte hq
//     call DAXPY(n, dte, hs(1,is), 1, s(1,is), 1)   is = 1..ns
//     call DSCAL(n, kco, hq(1,is), 1) ...                         (:279-293, every substep but the last)  hq *= kco
// and `hq = 0 ; hs = 0` at the start of a step (:212-216).  Executed one by one these are 2 (3 + ns) extra passes over the fields per substep
// (4.5 ms of 20.8 at 512^3), because the last kernels of the device RHS that hold each finished tendency in registers cannot know dte's partner
// kco yet.  They CAN when the calls are only recorded: this layer keeps the RHS call and the BLAS calls that follow it as a description, and when
// the description is complete -- or anything else wants the stream -- runs the ONE fused call tlab_time_substep_incompressible_explicit(dte, kco,
// scale) that the patched host of INTEGRATION.md section 3b would have made.  Same kernels, same arguments: the fields are those of the fused
// route to the bit.  A sequence that does not match (other vectors, other factors, another order) is executed literally, in the order it came.
//
// The host's DNS_BOUNDS_LIMIT (time.f90:248-250; tlab_amd/fortran/dns_local_device.sed turns its loop into tlab_deferred_clip) sits between the DAXPYs
// and the DSCALs: a clip of a recorded s after its DAXPY is recorded too and becomes the driver's bounds for the one fused call.
//
// What makes it safe: every launch of the library fetches its stream through tlab_current_stream(), which flushes first -- the stream itself is private
// to that accessor and tlab_set_stream (csrc/runtime.cpp), so no launch can be written that takes it another way.  The public operators, tlab_sync, the
// copies, tlab_free and the *_destroy functions flush as their first statement (before they size a work array or free what a record still names), and
// so do the setters whose state a substep reads (the drivers' tlab_*_set_*, tlab_opr_burgers_set_*, tlab_fdm_plan_set_scheme / _set_stagger,
// tlab_force_kernel_path, tlab_set_tuning): the record runs with the state it was recorded under.  Launches made from INSIDE a replay (the drivers call
// the operators and the tlab_internal_* fused variants) come through the same accessor: g_busy makes the flush return at once there.
// tests/deferred_entry_points.py holds one row per entry point of the header; tests/test_gpu_deferred_entry_points.py runs them with a record pending.
// What it cannot see: a host statement that reads a device array directly (hipMalloc memory is host-addressable on MI355X): such a host calls
// tlab_deferred_flush() or tlab_sync() first, or keeps the layer off (the default).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "driver_common.hpp"

using namespace tlab;

namespace {
struct Range { double *p; long long n; };
// the driver behind a recorded RHS -- tlab_dns (one domain), tlab_slab_dns or tlab_pencil_dns, the same tail behind each of them: its three entry
// points on its handle (and, one domain, on the arrays handed to the RHS), the substep with the tail it is handed
struct Driver {
    std::function<int()> begin_step;
    std::function<int(double dte)> rhs;
    std::function<int(double dte, const SubstepTail &tail)> substep;
    bool has_bounds = false;      // it holds scalar bounds of its own (they cannot change under a record: tlab_*_set_scalar_bounds flushes first)
    // one domain only (empty otherwise): the driver's handle and BOUNDARY_BUFFER_RELAX_SCAL on the recorded arrays
    tlab_dns_t dns = nullptr;
    std::function<int()> relax_scal;
};
struct Pending {
    bool rhs = false;
    Driver drv;
    double dte = 0.0, kco = 1.0;
    int nf = 0;                                   // 3 + nscal
    long long n = 0;
    std::vector<double *> x, y;                   // per field: tendency, state
    std::vector<char> upd, scl;
    int nupd = 0, nscl = 0;
    ScalarBounds clips;                           // per scalar: clipped after its DAXPY (DNS_BOUNDS_LIMIT), and how many are
    int nclp = 0;
    bool relax = false;                           // tlab_deferred_relax_scal recorded straight after the RHS (time.f90:628-630)
    bool sources = false;                         // tlab_deferred_sources_flow came straight before the RHS, same driver and arrays (time.f90:610-612)
    std::function<int()> sources_flow;            // ... and the routine on its own, for a literal run
    std::vector<Range> zeros;                     // `hq = 0` of the start of a step, not yet executed
};
Pending g_p;
bool g_on = false, g_busy = false;
long long g_stat[6] = {0, 0, 0, 0, 0, 0};        // fused substeps, literal flushes, begin_steps, eager axpy, eager scal, eager zero
long long g_clip_stat[2] = {0, 0};                // fused substeps that carried recorded clips, clips executed on their own
long long g_relax_stat[2] = {0, 0};               // fused substeps that carried a recorded scalar relaxation, relaxations executed on their own
long long g_src_stat[2] = {0, 0};                 // fused substeps that carried the sources marker, markers executed on their own
// tlab_deferred_sources_flow not yet followed by anything: the call is kept; a tlab_deferred_rhs of the same driver on the same arrays takes it into
// its record, anything else makes it run literally, in call order
struct Marker {
    bool on = false;
    tlab_dns_t d = nullptr;
    std::vector<double *> q, s, hq;
    int run() const { return tlab_dns_sources_flow(d, q.data(), s.empty() ? nullptr : s.data(), hq.data()); }
};
Marker g_src;
Driver g_last;                                    // the driver of the last tlab_deferred_rhs (a relaxation that meets no record runs on its arrays)

struct Busy {
    bool was;
    Busy() : was(g_busy) { g_busy = true; }
    ~Busy() { g_busy = was; }
};

// the BLAS guard of tlab_deferred_axpy / _scal: 1 both on the device, 0 both on the host, -2 mixed (refused), -1 the query failed
int classify(const char *who, const void *x, const void *y) {
    const int a = tlab_pointer_on_device(x), b = y ? tlab_pointer_on_device(y) : a;
    if (a < 0 || b < 0) return -1;
    if (a != b) {
        tlab_set_error(std::string(who) + ": one array in host memory and one in device memory");
        return -2;
    }
    return a;
}

int run_zeros_eagerly() {
    std::vector<Range> z;
    z.swap(g_p.zeros);
    for (const Range &r : z) {
        ++g_stat[5];
        const int rc = tlab_pw_fill(r.p, 0.0, r.n);
        if (rc != TLAB_OK) return rc;
    }
    return TLAB_OK;
}

// do the pending zero fills cover exactly the tendencies of the pending RHS?  (then they are the `hq = 0 ; hs = 0` of time.f90:212-216 and become
// tlab_dns_begin_step: the first launch of each field overwrites instead of accumulating)
bool zeros_are_the_tendencies(const Pending &p) {
    if (p.zeros.empty()) return false;
    long long total = 0;
    for (const Range &r : p.zeros) total += r.n;
    if (total != (long long)p.nf * p.n) return false;
    for (int f = 0; f < p.nf; ++f) {
        bool in = false;
        for (const Range &r : p.zeros) in = in || (p.x[f] >= r.p && p.x[f] + p.n <= r.p + r.n);
        if (!in) return false;
    }
    return true;
}

// the substep the record describes: its bounds are the recorded clips and nothing else (a driver's own bounds do not belong to RHS + DAXPY), the
// scalar buffer zones of the driver act in it only when the record holds the relaxation, the body forces only when it holds the sources marker
int run_substep(const Pending &p, double kco, int scale) {
    SubstepTail tail{kco, scale, p.nclp ? &p.clips : nullptr, p.relax, p.sources};
    if (!p.drv.dns) {                // a decomposed driver: neither marker can be recorded for it
        tail.scal_zones = true;      // the scalar blocks act in every replay
        tail.forces = false;         // the body forces in none
    }
    return p.drv.substep(p.dte, tail);
}

// a new record: driver, step and the fields (tendency, state) the BLAS calls that follow are matched against; the zero fills recorded so far stay
void record(Driver drv, double dte, int ns, long long n, double *const *q, double *const *s, double *const *hq, double *const *hs) {
    Pending &p = g_p;
    p.rhs = true;
    p.drv = std::move(drv);
    p.dte = dte; p.kco = 1.0;
    p.nf = 3 + ns; p.n = n;
    p.x.clear(); p.y.clear();
    for (int i = 0; i < 3; ++i) { p.x.push_back(hq[i]); p.y.push_back(q[i]); }
    for (int i = 0; i < ns; ++i) { p.x.push_back(hs[i]); p.y.push_back(s[i]); }
    p.upd.assign(p.nf, 0); p.scl.assign(p.nf, 0);
    p.nupd = p.nscl = 0;
    p.clips.on.assign(ns, 0); p.clips.lo.assign(ns, 0.0); p.clips.hi.assign(ns, 0.0);
    p.nclp = 0;
    p.relax = false;
    p.sources = false;
    p.sources_flow = nullptr;
}

// whole_ok = false: the record is cut short by a call that does not belong to the fused substep; it counts as a literal run
int flush_impl(bool whole_ok = true) {
    if (g_busy) return TLAB_OK;
    Busy b;
    if (!g_p.rhs) {                    // zero fills and / or a sources marker that nothing followed: literally, in call order
        int rc = run_zeros_eagerly();
        if (g_src.on) {
            Marker m;
            std::swap(m, g_src);
            ++g_src_stat[1];
            if (rc == TLAB_OK) rc = m.run();
        }
        return rc;
    }
    Pending p;
    std::swap(p, g_p);                 // whatever runs below sees an empty description
    int rc = TLAB_OK;
    const bool fused = whole_ok && p.nupd == p.nf && (p.nscl == 0 || p.nscl == p.nf);
    // (a record with the sources marker that runs literally executes REAL zero fills: the routine on its own adds to what the tendencies hold, and
    // tendencies that only count as zero hold the last step's values)
    if (zeros_are_the_tendencies(p) && !(p.sources && !fused && p.nupd != p.nf)) {
        ++g_stat[2];
        rc = p.drv.begin_step();
    } else {
        for (const Range &r : p.zeros) {
            ++g_stat[5];
            if (rc == TLAB_OK) rc = tlab_pw_fill(r.p, 0.0, r.n);
        }
    }
    if (rc != TLAB_OK) return rc;
    if (fused) {      // the whole substep, as the patched host would have called it
        ++g_stat[0];
        if (p.nclp) ++g_clip_stat[0];
        if (p.relax) ++g_relax_stat[0];
        if (p.sources) ++g_src_stat[0];
        return run_substep(p, p.nscl ? p.kco : 1.0, p.nscl ? 1 : 0);
    }
    ++g_stat[1];
    if (p.nupd == p.nf) {                                           // all updated, some scaled: the substep without scaling (+ clips), then those
        rc = run_substep(p, 1.0, 0);
        for (int f = 0; f < p.nf && rc == TLAB_OK; ++f)
            if (p.scl[f]) rc = tlab_pw_scale(p.x[f], p.kco, p.n);
        return rc;
    }
    if (p.sources) { ++g_src_stat[1]; rc = p.sources_flow(); }      // (the marker stood before the RHS)
    if (rc == TLAB_OK) rc = p.drv.rhs(p.dte);
    if (p.relax && rc == TLAB_OK) { ++g_relax_stat[1]; rc = p.drv.relax_scal(); }      // (recorded before every DAXPY)
    for (int f = 0; f < p.nf && rc == TLAB_OK; ++f)
        if (p.upd[f]) rc = tlab_pw_rk_update(p.y[f], p.x[f], p.dte, 1.0, 0, p.n);
    for (int is = 0; is + 3 < p.nf && rc == TLAB_OK; ++is)          // (a clip was recorded after the DAXPY of its field only)
        if (p.clips.on[is]) { ++g_clip_stat[1]; rc = tlab_pw_clip(p.y[3 + is], p.clips.lo[is], p.clips.hi[is], p.n); }
    return rc;
}
}      // namespace

// every entry point that flushes: tlab_current_stream(), the operators and setters of operators.cpp and fdm_plan.cpp, tlab_sync, the copies, tlab_free, tlab_set_stream, ...
// A recorded substep that runs because some OTHER entry point wanted the stream (the hook in tlab_current_stream()) has no caller to report a failure to:
// the code is kept and handed to the next tlab_sync / tlab_deferred_* call (the error text stays in tlab_last_error()).
static int g_sticky = TLAB_OK;
int tlab_internal_deferred_flush() {
    if (g_busy) return TLAB_OK;
    int rc = TLAB_OK;
    if (g_on && (g_p.rhs || !g_p.zeros.empty() || g_src.on)) rc = flush_impl();
    if (rc != TLAB_OK && g_sticky == TLAB_OK) g_sticky = rc;
    return rc;
}
int tlab_internal_deferred_take_error() {      // runtime.cpp: tlab_sync
    const int rc = g_sticky;
    g_sticky = TLAB_OK;
    return rc;
}

extern "C" {

int tlab_deferred_enable(int on) {
    const int rc = tlab_internal_deferred_flush();
    g_on = on != 0;
    return rc;
}

int tlab_deferred_flush(void) {
    const int rc = tlab_internal_deferred_flush();
    const int old = tlab_internal_deferred_take_error();
    return rc != TLAB_OK ? rc : old;
}

int tlab_deferred_stats(long long *counts) {
    if (!counts) return TLAB_EINVAL;
    for (int i = 0; i < 6; ++i) counts[i] = g_stat[i];
    return TLAB_OK;
}

int tlab_deferred_clip_stats(long long *counts) {
    if (!counts) return TLAB_EINVAL;
    counts[0] = g_clip_stat[0];
    counts[1] = g_clip_stat[1];
    return TLAB_OK;
}

int tlab_deferred_relax_stats(long long *counts) {
    if (!counts) return TLAB_EINVAL;
    counts[0] = g_relax_stat[0];
    counts[1] = g_relax_stat[1];
    return TLAB_OK;
}

// BOUNDARY_BUFFER_RELAX_SCAL of an unchanged host (time.f90:628-630, through tlab_amd/fortran/boundary_buffer_device.sed).  Straight after the recorded
// RHS of this driver, once, with scalar zones set: recorded, and the record runs as the one fused substep with the scalar blocks in it.  After a
// DAXPY, a second time, or without scalar zones: the record runs literally first, then the relaxation on its own, in call order.
int tlab_deferred_relax_scal(tlab_dns_t d) {
    if (!d) { tlab_set_error("tlab_deferred_relax_scal: null handle"); return TLAB_EINVAL; }
    if (g_on && g_p.rhs && g_p.drv.dns == d && !g_p.relax && g_p.nupd == 0 && g_p.nscl == 0 && tlab_internal_dns_has_scal_zones(d)) {
        g_p.relax = true;
        return TLAB_OK;
    }
    Driver drv = (g_p.rhs && g_p.drv.dns == d) ? g_p.drv : g_last;
    if (g_on) {
        const int rc = flush_impl(false);
        if (rc != TLAB_OK) return rc;
    }
    if (drv.dns != d || !drv.relax_scal) {
        tlab_set_error("tlab_deferred_relax_scal: no tlab_deferred_rhs of this driver came before (its arrays are not known)");
        return TLAB_EINVAL;
    }
    ++g_relax_stat[1];
    return drv.relax_scal();
}

int tlab_deferred_sources_stats(long long *counts) {
    if (!counts) return TLAB_EINVAL;
    counts[0] = g_src_stat[0];
    counts[1] = g_src_stat[1];
    return TLAB_OK;
}

// TLab_Sources_Flow of an unchanged host (time.f90:610, through tlab_amd/fortran/tlab_sources_device.sed).  Off: the routine on its own.  On: a pending
// record runs first, then the call is kept as a marker for the tlab_deferred_rhs that follows (see Marker above).
int tlab_deferred_sources_flow(tlab_dns_t d, double *const *q, double *const *s, double *const *hq) {
    if (!g_on) return tlab_dns_sources_flow(d, q, s, hq);
    if (!d || !q || !hq) { tlab_set_error("tlab_deferred_sources_flow: bad arguments"); return TLAB_EINVAL; }
    const int ns = tlab_internal_dns_scal_arrays(d);      // (with a mixture s carries the liquid behind the prognostic scalars)
    if (ns > 0 && !s) { tlab_set_error("tlab_deferred_sources_flow: bad arguments"); return TLAB_EINVAL; }
    if (g_p.rhs || g_src.on) {         // (a marker nothing followed runs literally, after the zero fills that came before it)
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    g_src.on = true; g_src.d = d;
    g_src.q.assign(q, q + 3); g_src.s.assign(s, s + ns); g_src.hq.assign(hq, hq + 3);
    return TLAB_OK;
}

int tlab_deferred_zero(double *a, long long n) {
    if (!a || n < 0) { tlab_set_error("tlab_deferred_zero: bad arguments"); return TLAB_EINVAL; }
    if (!g_on) { ++g_stat[5]; return tlab_pw_fill(a, 0.0, n); }
    if (g_p.rhs || g_src.on) {                       // a substep is still described: it runs first (its fields may be the ones zeroed here)
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    g_p.zeros.push_back({a, n});
    return TLAB_OK;
}

int tlab_deferred_rhs(tlab_dns_t d, double dte, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc) {
    if (!d || !q || !hq || !txc || dte <= 0.0) { tlab_set_error("tlab_deferred_rhs: bad arguments"); return TLAB_EINVAL; }
    const int ns = tlab_internal_dns_nscal(d);
    if (ns > 0 && (!s || !hs)) { tlab_set_error("tlab_deferred_rhs: bad arguments"); return TLAB_EINVAL; }
    // a sources marker belongs to this RHS when it names the same driver and the same arrays; otherwise it runs literally now
    bool sources = false;
    if (g_on && g_src.on) {
        sources = g_src.d == d && std::equal(q, q + 3, g_src.q.begin()) && std::equal(hq, hq + 3, g_src.hq.begin()) && std::equal(s, s + ns, g_src.s.begin());
        if (sources) g_src = Marker();
    }
    if (g_on && (g_p.rhs || g_src.on)) {
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    // the arrays stay with the record: this driver takes them with every call
    const int na = tlab_internal_dns_scal_arrays(d);      // (with a mixture s carries the liquid behind the prognostic scalars)
    const std::vector<double *> Q(q, q + 3), S(s, s + na), HQ(hq, hq + 3), HS(hs, hs + ns), T(txc, txc + 9);
    Driver drv;
    drv.begin_step = [d] { return tlab_dns_begin_step(d); };
    drv.rhs = [=](double dte_) {
        return tlab_rhs_global_incompressible_1(d, dte_, Q.data(), ns ? S.data() : nullptr, HQ.data(), ns ? HS.data() : nullptr, T.data());
    };
    drv.substep = [=](double dte_, const SubstepTail &tail) {
        return catch_fail([&] { tlab_internal_dns_substep(d, dte_, Q.data(), ns ? S.data() : nullptr, HQ.data(), ns ? HS.data() : nullptr, T.data(), tail); }, TLAB_EINVAL);
    };
    drv.has_bounds = tlab_internal_dns_has_bounds(d);
    drv.dns = d;
    drv.relax_scal = [=] { return tlab_dns_buffer_relax_scal(d, ns ? S.data() : nullptr, ns ? HS.data() : nullptr); };
    g_last = drv;
    if (!g_on) return drv.rhs(dte);
    record(std::move(drv), dte, ns, tlab_internal_dns_points(d), q, s, hq, hs);
    g_p.sources = sources;
    if (sources) g_p.sources_flow = [=] { return tlab_dns_sources_flow(d, Q.data(), ns ? S.data() : nullptr, HQ.data()); };
    return TLAB_OK;
}

// the same for the decomposed drivers: their arrays are bound (tlab_slab_dns_bind / tlab_pencil_dns_bind), so the call carries the handle and dte only;
// bound: tlab_internal_{slab,pencil}_bound found the arrays of the one local rank (b)
static int deferred_decomposed(Driver drv, bool bound, const tlab_bound_fields &b, double dte) {
    if (!g_on || !bound || !(dte > 0.0)) {      // off, or nothing to match the BLAS calls against (several local ranks): at once
        if (g_on) { const int rc = flush_impl(); if (rc != TLAB_OK) return rc; }      // (with a sources marker that nothing of its driver followed)
        return drv.rhs(dte);
    }
    if (g_p.rhs || g_src.on) {
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    drv.has_bounds = b.has_bounds;
    record(std::move(drv), dte, b.nscal, b.n, b.q, b.s, b.hq, b.hs);
    return TLAB_OK;
}
int tlab_deferred_slab_rhs(tlab_slab_dns_t d, double dte) {
    if (!d) { tlab_set_error("tlab_deferred_slab_rhs: null handle"); return TLAB_EINVAL; }
    tlab_bound_fields b{};
    const bool bound = tlab_internal_slab_bound(d, &b);
    return deferred_decomposed({[d] { return tlab_slab_dns_begin_step(d); }, [d](double dte_) { return tlab_slab_dns_rhs(d, dte_); },
                                [d](double dte_, const SubstepTail &tail) { return guarded([&] { tlab_internal_slab_substep(d, dte_, tail); }); }},
                               bound, b, dte);
}
int tlab_deferred_pencil_rhs(tlab_pencil_dns_t d, double dte) {
    if (!d) { tlab_set_error("tlab_deferred_pencil_rhs: null handle"); return TLAB_EINVAL; }
    tlab_bound_fields b{};
    const bool bound = tlab_internal_pencil_bound(d, &b);
    return deferred_decomposed({[d] { return tlab_pencil_dns_begin_step(d); }, [d](double dte_) { return tlab_pencil_dns_rhs(d, dte_); },
                                [d](double dte_, const SubstepTail &tail) { return guarded([&] { tlab_internal_pencil_substep(d, dte_, tail); }); }},
                               bound, b, dte);
}

int tlab_deferred_axpy(long long n, double a, const double *x, double *y) {
    if (!x || !y || n < 0) { tlab_set_error("tlab_deferred_axpy: bad arguments"); return TLAB_EINVAL; }
    const int where = classify("tlab_deferred_axpy", x, y);
    if (where < 0) return where == -2 ? TLAB_EINVAL : TLAB_EHIP;
    if (where == 0) {                    // host arrays: the BLAS-1 call of the host itself, at once (a recorded substep is not touched)
        for (long long i = 0; i < n; ++i) y[i] += a * x[i];
        return TLAB_OK;
    }
    if (g_on && g_p.rhs && g_p.nscl == 0 && n == g_p.n && a == g_p.dte) {
        for (int f = 0; f < g_p.nf; ++f)
            if (!g_p.upd[f] && g_p.x[f] == x && g_p.y[f] == y) { g_p.upd[f] = 1; ++g_p.nupd; return TLAB_OK; }
    }
    if (g_on) {
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    ++g_stat[3];
    return tlab_pw_rk_update(y, const_cast<double *>(x), a, 1.0, 0, n);       // y += a x (x is only read when scale = 0)
}

int tlab_deferred_scal(long long n, double a, double *x) {
    if (!x || n < 0) { tlab_set_error("tlab_deferred_scal: bad arguments"); return TLAB_EINVAL; }
    const int where = classify("tlab_deferred_scal", x, nullptr);
    if (where < 0) return where == -2 ? TLAB_EINVAL : TLAB_EHIP;
    if (where == 0) {
        for (long long i = 0; i < n; ++i) x[i] *= a;
        return TLAB_OK;
    }
    if (g_on && g_p.rhs && g_p.nupd == g_p.nf && n == g_p.n && (g_p.nscl == 0 || a == g_p.kco)) {
        for (int f = 0; f < g_p.nf; ++f)
            if (!g_p.scl[f] && g_p.x[f] == x) {
                g_p.scl[f] = 1; ++g_p.nscl; g_p.kco = a;
                return g_p.nscl == g_p.nf ? flush_impl() : TLAB_OK;      // complete: nothing more to wait for
            }
    }
    if (g_on) {
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    ++g_stat[4];
    return tlab_pw_scale(x, a, n);
}

int tlab_deferred_clip(long long n, double lo, double hi, double *x) {
    if (!x || n < 0 || std::isnan(lo) || std::isnan(hi) || lo > hi) {
        tlab_set_error("tlab_deferred_clip: null array, n < 0, NaN bounds or lo > hi");
        return TLAB_EINVAL;
    }
    if (g_on && g_p.rhs && g_p.nscl == 0 && n == g_p.n && !g_p.drv.has_bounds) {
        for (int is = 0; is + 3 < g_p.nf; ++is)
            if (g_p.y[3 + is] == x) {
                if (!g_p.upd[3 + is] || g_p.clips.on[is]) break;       // before its DAXPY, or a second clip: literal
                g_p.clips.on[is] = 1; g_p.clips.lo[is] = lo; g_p.clips.hi[is] = hi; ++g_p.nclp;
                return TLAB_OK;
            }
    }
    if (g_on) {
        const int rc = flush_impl();
        if (rc != TLAB_OK) return rc;
    }
    ++g_clip_stat[1];
    return tlab_pw_clip(x, lo, hi, n);
}

// 1: device memory, 0: host memory, < 0: error.  The allocation ranges of the device pointers seen last are kept (hipMemGetAddressRange), and the host
// pointers seen last: a time loop hands the same arrays over and over, and hipPointerGetAttributes costs a runtime call.
int tlab_pointer_on_device(const void *p) {
    if (!p) { tlab_set_error("tlab_pointer_on_device: null pointer"); return TLAB_EINVAL; }
    struct DevRange { const char *b = nullptr; size_t n = 0; };
    static DevRange dev[16];
    static const void *host[16] = {nullptr};
    static int next_dev = 0, next_host = 0;
    const char *c = static_cast<const char *>(p);
    for (const DevRange &r : dev)
        if (r.b && c >= r.b && c < r.b + r.n) return 1;
    for (const void *h : host)
        if (h == p) return 0;
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e == hipErrorInvalidValue) {      // memory the runtime does not know: host memory; the query leaves a sticky error behind
        (void)hipGetLastError();
        host[next_host] = p; next_host = (next_host + 1) % 16;
        return 0;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        tlab_set_error(std::string("tlab_pointer_on_device: hipPointerGetAttributes: ") + hipGetErrorString(e));
        return TLAB_EHIP;
    }
    if (at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeHost) {
        host[next_host] = p; next_host = (next_host + 1) % 16;
        return 0;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) == hipSuccess && base && size) {
        dev[next_dev].b = static_cast<const char *>(base); dev[next_dev].n = size;
        next_dev = (next_dev + 1) % 16;
    } else {
        (void)hipGetLastError();
    }
    return 1;
}

}      // extern "C"
