// ---- which allocations play q, s, hq, hs, txc (include/tlab_amd.h: tlab_dns_place_arrays) ----
// A kernel that streams many arrays at once runs at a rate that depends on WHICH device allocations they are -- not on any one of them (each alone
// reads / writes at the same rate), on the set: tools/placement_probe measures 4.8 .. 5.9 TB/s for one 13-stream kernel over sets drawn from a pool
// of 1-GiB hipMalloc allocations, reproducibly per set (profiles/r05/placement_*.txt).  It is what made "the slow state of the box" of rounds 3-5:
// the same binary, the same box, 16.0 .. 17.2 ms per substep from process to process.  Neither the virtual alignment nor a skew between the arrays
// of one allocation predicts it, so the assignment is searched: time the substep itself on candidate assignments and keep the fastest.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <utility>
#include <vector>

#include "dns_state.hpp"

using namespace tlab;

extern "C" {      // (the tools of the searches too: `confirm` is in the dynamic symbol table of the library)

namespace {
// the tools of the two placement searches below: one Runge-Kutta step of three substeps (the first on fresh tendencies, the others accumulating and
// scaling: the kernels of a real step) timed by events on the library's stream, after one untimed substep (first touch of the arrays)
struct PlaceTimer {
    tlab_dns_t d;
    double dtime;
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool fresh_on_entry;
    PlaceTimer(tlab_dns_t d_, double dtime_) : d(d_), dtime(dtime_), st(tlab_current_stream()), fresh_on_entry(d_->fresh) {
        hk(hipEventCreate(&e0), "hipEventCreate");
        hk(hipEventCreate(&e1), "hipEventCreate");
    }
    ~PlaceTimer() {      // released on every way out (a failing trial throws); the caller's begin_step flag survives the trial substeps
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        d->fresh = fresh_on_entry;
    }
    double step(double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc, bool first_touch) {
        const double kdt[3] = {1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0}, kco[3] = {-5.0 / 9.0, -153.0 / 128.0, 1.0};
        SubstepTail own{kco[0], 1, &d->bounds, true, true};      // the driver's own settings, as tlab_time_substep_incompressible_explicit passes them
        if (first_touch) {
            d->fresh = true;
            rhs_substep(d, dtime * kdt[0], q, s, hq, hs, txc, &own);
        }
        hk(hipEventRecord(e0, st), "hipEventRecord");
        d->fresh = true;
        for (int k = 0; k < 3; ++k) { own.kco = kco[k]; own.scale = k < 2; rhs_substep(d, dtime * kdt[k], q, s, hq, hs, txc, &own); }
        hk(hipEventRecord(e1, st), "hipEventRecord");
        hk(hipEventSynchronize(e1), "hipEventSynchronize");
        float ms = 0.0f;
        hk(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
        return (double)ms / 3.0;
    }
};
struct XorShift {      // the same sequence everywhere
    unsigned long long x;
    explicit XorShift(unsigned seed) : x(0x9E3779B97F4A7C15ull ^ ((unsigned long long)seed * 0xBF58476D1CE4E5B9ull + 1ull)) {}
    int operator()(int m) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (int)(x % (unsigned long long)m); }
};
// The search keeps the minimum of single timings, which is biased by noise (and the first assignment is timed straight after the warm-up): the
// winner and the first assignment are timed again, back to back, three times each; the winner stays only if its median is below the other's.
// Returns (ms of the first assignment, ms of the assignment kept) from those repeats.
std::pair<double, double> confirm(const std::function<double(const std::vector<int> &)> &trial, const std::vector<int> &ident, std::vector<int> &best) {
    auto med3 = [](double a, double b, double c) { return std::max(std::min(a, b), std::min(std::max(a, b), c)); };
    if (best == ident) {
        const double m = med3(trial(ident), trial(ident), trial(ident));
        return {m, m};
    }
    double a[3], b[3];
    for (int r = 0; r < 3; ++r) { a[r] = trial(ident); b[r] = trial(best); }
    const double mi = med3(a[0], a[1], a[2]), mb = med3(b[0], b[1], b[2]);
    if (!(mb < mi)) { best = ident; return {mi, mi}; }
    return {mi, mb};
}
}      // namespace

int tlab_dns_place_arrays(tlab_dns_t d, int npool, double *const *pool, const double *const *state, double dtime, int random_trials, unsigned seed,
                          int *assignment, double *report) {
    return catch_fail([&] {
        if (!d || !pool || !assignment || dtime <= 0.0 || random_trials < 0) throw Fail(TLAB_EINVAL, "tlab_dns_place_arrays: bad arguments");
        if (d->mixture != TLAB_MIXT_NONE) throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_place_arrays: the search places nscal scalar arrays; a driver with a mixture holds the liquid as well");
        const int ns = d->nscal, nroles = 2 * (3 + ns) + 9;
        if (npool < nroles) throw Fail(TLAB_EINVAL, "tlab_dns_place_arrays: the pool must hold at least 2 (3 + nscal) + 9 arrays");
        for (int i = 0; i < npool; ++i) {
            if (!pool[i]) throw Fail(TLAB_EINVAL, "tlab_dns_place_arrays: null array in the pool");
            for (int j = 0; j < i; ++j)
                if (pool[j] == pool[i]) throw Fail(TLAB_EINVAL, "tlab_dns_place_arrays: the same array twice in the pool");
        }
        PlaceTimer T(d, dtime);
        hipStream_t st = T.st;
        const size_t fbytes = (size_t)d->nx * d->ny * d->nz * sizeof(double);
        auto trial = [&](const std::vector<int> &a) {
            std::vector<double *> q(3), s((size_t)std::max(ns, 1)), hq(3), hs((size_t)std::max(ns, 1)), txc(9);
            int r = 0;
            for (int i = 0; i < 3; ++i) q[i] = pool[a[r++]];
            for (int i = 0; i < ns; ++i) s[i] = pool[a[r++]];
            for (int i = 0; i < 3; ++i) hq[i] = pool[a[r++]];
            for (int i = 0; i < ns; ++i) hs[i] = pool[a[r++]];
            for (int i = 0; i < 9; ++i) txc[i] = pool[a[r++]];
            for (int i = 0; i < 3 + ns; ++i) {
                double *dst = i < 3 ? q[i] : s[i - 3];
                if (state && state[i]) hk(hipMemcpyAsync(dst, state[i], fbytes, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
                else hk(hipMemsetAsync(dst, 0, fbytes, st), "hipMemsetAsync");
            }
            return T.step(q.data(), s.data(), hq.data(), hs.data(), txc.data(), true);
        };
        XorShift rnd(seed);
        std::vector<int> ident((size_t)nroles);
        for (int i = 0; i < nroles; ++i) ident[i] = i;
        std::vector<double> all;
        std::vector<int> best = ident;
        const double first = trial(ident);
        double bestms = first;
        all.push_back(first);
        for (int t = 0; t < random_trials; ++t) {
            std::vector<int> perm((size_t)npool);
            for (int i = 0; i < npool; ++i) perm[i] = i;
            for (int i = npool - 1; i > 0; --i) std::swap(perm[i], perm[rnd(i + 1)]);
            perm.resize((size_t)nroles);
            const double ms = trial(perm);
            all.push_back(ms);
            if (ms < bestms) { bestms = ms; best = perm; }
        }
        // one pass of single-role exchanges against the unused arrays (skipped when the pool has none to spare)
        if (npool > nroles && random_trials > 0) {
            for (int r = 0; r < nroles; ++r) {
                std::vector<char> used((size_t)npool, 0);
                for (int v : best) used[v] = 1;
                int cand = -1;
                for (int tries = 0; tries < 4 * npool && cand < 0; ++tries) { const int c = rnd(npool); if (!used[c]) cand = c; }
                if (cand < 0) continue;
                std::vector<int> a = best;
                a[r] = cand;
                const double ms = trial(a);
                all.push_back(ms);
                if (ms < bestms * 0.999) { bestms = ms; best = a; }
            }
        }
        double ms_first = first, ms_kept = bestms;
        if (random_trials > 0) { auto c = confirm(trial, ident, best); ms_first = c.first; ms_kept = c.second; }
        for (int r = 0; r < nroles; ++r) assignment[r] = best[r];
        if (report) {
            std::vector<double> sorted = all;
            std::sort(sorted.begin(), sorted.end());
            report[0] = ms_first; report[1] = ms_kept; report[2] = sorted[sorted.size() / 2]; report[3] = sorted.back(); report[4] = (double)all.size();
        }
    }, TLAB_EINVAL);
}

// ---- the same question for a Tlab HOST (include/tlab_amd.h: tlab_dns_place_blocks) ----
// The host's arrays are two-dimensional: q(isize_field, 3), s(isize_field, ns), hq, hs, txc(isize_txc_field, 9) (base/tlab_memory.f90:201-207,
// dns_main.f90:103-104) -- the components of a block lie a fixed stride apart and cannot be placed one by one.  What CAN be chosen is which
// allocation plays each block: the host allocates ncand candidates per block (index 0 = the ones it holds), the substep is timed on combinations,
// and the host re-associates its pointers with the winners before any field is read.
int tlab_dns_place_blocks(tlab_dns_t d, int ncand, double *const *cand_q, double *const *cand_s, double *const *cand_hq, double *const *cand_hs,
                          double *const *cand_txc, long long txc_stride, double dtime, int random_trials, unsigned seed, int *choice, double *report) {
    return catch_fail([&] {
        if (!d || ncand < 1 || !cand_q || !cand_hq || !cand_txc || !choice || dtime <= 0.0 || random_trials < 0)
            throw Fail(TLAB_EINVAL, "tlab_dns_place_blocks: bad arguments");
        if (d->mixture != TLAB_MIXT_NONE) throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_place_blocks: the search places blocks of nscal scalar arrays; a driver with a mixture holds the liquid as well");
        const int ns = d->nscal;
        const long long n = (long long)d->nx * d->ny * d->nz;
        if (ns > 0 && (!cand_s || !cand_hs)) throw Fail(TLAB_EINVAL, "tlab_dns_place_blocks: candidates for s, hs are missing");
        if (txc_stride < n) throw Fail(TLAB_EINVAL, "tlab_dns_place_blocks: txc_stride below the field size");
        double *const *cands[5] = {cand_q, ns > 0 ? cand_s : nullptr, cand_hq, ns > 0 ? cand_hs : nullptr, cand_txc};      // (no scalars: whatever stands there is not looked at)
        for (int b = 0; b < 5; ++b) {
            if (!cands[b]) continue;
            for (int i = 0; i < ncand; ++i) {
                if (!cands[b][i]) throw Fail(TLAB_EINVAL, "tlab_dns_place_blocks: null candidate");
                for (int b2 = 0; b2 <= b; ++b2)
                    for (int j = 0; cands[b2] && j < (b2 == b ? i : ncand); ++j)
                        if (cands[b2][j] == cands[b][i]) throw Fail(TLAB_EINVAL, "tlab_dns_place_blocks: the same array twice among the candidates");
            }
        }
        PlaceTimer T(d, dtime);
        hipStream_t st = T.st;
        std::vector<char> touched((size_t)5 * ncand, 0);
        auto trial = [&](const std::vector<int> &a) {
            std::vector<double *> q(3), s((size_t)std::max(ns, 1)), hq(3), hs((size_t)std::max(ns, 1)), txc(9);
            for (int i = 0; i < 3; ++i) { q[i] = cand_q[a[0]] + (long long)i * n; hq[i] = cand_hq[a[2]] + (long long)i * n; }
            for (int i = 0; i < ns; ++i) { s[i] = cand_s[a[1]] + (long long)i * n; hs[i] = cand_hs[a[3]] + (long long)i * n; }
            for (int i = 0; i < 9; ++i) txc[i] = cand_txc[a[4]] + (long long)i * txc_stride;
            // the trial fields are zeros (the host has read nothing yet; the kernels' time does not depend on the values)
            hk(hipMemsetAsync(q[0], 0, (size_t)3 * n * sizeof(double), st), "hipMemsetAsync");
            if (ns > 0) hk(hipMemsetAsync(s[0], 0, (size_t)ns * n * sizeof(double), st), "hipMemsetAsync");
            bool first_touch = false;
            for (int b = 0; b < 5; ++b) { char &t = touched[(size_t)b * ncand + a[b]]; first_touch = first_touch || !t; t = 1; }
            return T.step(q.data(), s.data(), hq.data(), hs.data(), txc.data(), first_touch);
        };
        XorShift rnd(seed);
        const std::vector<int> ident(5, 0);
        std::vector<int> best = ident;
        std::vector<double> all;
        const double first = trial(ident);
        double bestms = first;
        all.push_back(first);
        if (ncand > 1) {
            for (int t = 0; t < random_trials; ++t) {
                std::vector<int> a(5);
                for (int b = 0; b < 5; ++b) a[b] = rnd(ncand);
                const double ms = trial(a);
                all.push_back(ms);
                if (ms < bestms) { bestms = ms; best = a; }
            }
            if (random_trials > 0)      // one pass over the blocks: every other candidate of one block with the rest held
                for (int b = 0; b < 5; ++b) {
                    if (!cands[b]) continue;
                    for (int c = 0; c < ncand; ++c) {
                        if (c == best[b]) continue;
                        std::vector<int> a = best;
                        a[b] = c;
                        const double ms = trial(a);
                        all.push_back(ms);
                        if (ms < bestms * 0.999) { bestms = ms; best = a; }
                    }
                }
        }
        double ms_first = first, ms_kept = bestms;
        if (ncand > 1 && random_trials > 0) { auto c = confirm(trial, ident, best); ms_first = c.first; ms_kept = c.second; }
        for (int b = 0; b < 5; ++b) choice[b] = best[b];
        if (report) {
            std::vector<double> sorted = all;
            std::sort(sorted.begin(), sorted.end());
            report[0] = ms_first; report[1] = ms_kept; report[2] = sorted[sorted.size() / 2]; report[3] = sorted.back(); report[4] = (double)all.size();
        }
    }, TLAB_EINVAL);
}

}  // extern "C"
