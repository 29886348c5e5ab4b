// What the host files of the statistics (averages.cpp, pdfs.cpp, sampling.cpp, spectra.cpp, conditional.cpp) share: the refusal of a mix of host and
// device arrays, the device scratch of a file, and -- pdfs.cpp and conditional.cpp -- the box of a plane walk with its checks, the reference's loop
// over a plane, the groups of fields of a launch, the min / max pass and the two interval passes of the joint statistics.  Header-only, host code.
// Every definition has internal linkage (the unnamed namespace): each file compiles its own copy, none calls into another for them (internal.hpp
// declares nothing of this), and the library exports no symbol for them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "errors.hpp"
#include "kernels.hpp"
#include "pdfs_host.hpp"
#include "plan.hpp"

#pragma clang fp contract(off)      // the host loops below (for_plane, minmax_pass, joint_intervals) stay as written in every file that takes them

namespace tlab {
namespace {

// 1: every array is device memory, 0: every array is host memory (or no tlab_init: no array is the library's); a mix is refused
template <class T>
bool on_device(const char *who, const T *const *p, size_t n) {
    size_t ndev = 0;
    if (tlab_device_ready())
        for (size_t i = 0; i < n; ++i) {
            const int on = tlab_pointer_on_device(p[i]);
            if (on < 0) throw Fail(on, std::string(who) + ": " + tlab_last_error());
            ndev += on ? 1 : 0;
        }
    if (ndev != 0 && ndev != n) throw Fail(TLAB_EINVAL, std::string(who) + ": host and device arrays in one call");
    return ndev != 0;
}
inline bool on_device(const char *who, std::initializer_list<const void *> p) { return on_device(who, p.begin(), p.size()); }
inline bool on_device(const char *who, const std::vector<const void *> &p) { return on_device(who, p.data(), p.size()); }

// The device scratch of ONE file: grown on demand, never shrunk, contents undefined (the calls run on the library's stream one after the other).
// Every file has its own and they must stay apart: a composed entry point holds a pointer into its file's scratch while it calls public entry
// points of another statistics file (spectra.cpp's pairs around tlab_avg_cov2v, tlab_dns_spectra and tlab_dns_gate around tlab_avg_ik_v,
// tlab_fluctuation, tlab_minmax and the gates); with one shared buffer a nested call that grows it would free the memory the outer call still
// uses.  The array lives on the heap and is never deleted: it is the process's, and at exit the runtime that would free it may be gone.
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
class Scratch {
    DeviceArray &a_ = *new DeviceArray;
    const char *what_;      // the text of a refused allocation

public:
    explicit Scratch(const char *what) : what_(what) {}
    double *doubles(size_t n) { return a_.reserve(n, what_); }
    char *bytes(size_t n) { return (char *)a_.reserve((n + 7) / 8, what_); }      // (lay the parts out at multiples of up16)
};

// ---- the planes of a box (pdfs.cpp, conditional.cpp) ---------------------------------------------------------------------------------------------
struct Box {
    bool dev;
    int nx, ny, nz, igate;
    const signed char *gate;      // null: every point takes part
};

// nv fields u, the gate where igate != 0 and -- if there is one -- the array a that is averaged: one box, arrays of one kind
inline Box check_box(const char *who, int nx, int ny, int nz, int nv, const double *const *u, int igate, const signed char *gate,
                     const double *a = nullptr) {
    if (nx < 1 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nx, ny, nz must be at least 1");
    if (nv < 1 || !u) throw Fail(TLAB_EINVAL, std::string(who) + ": nv < 1 or a null pointer");
    if (igate < -128 || igate > 127) throw Fail(TLAB_EINVAL, std::string(who) + ": igate is not a value of an int8 gate");
    if (igate != 0 && !gate) throw Fail(TLAB_EINVAL, std::string(who) + ": igate != 0 needs a gate");
    std::vector<const void *> all;
    for (int v = 0; v < nv; ++v) {
        if (!u[v]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null field");
        all.push_back(u[v]);
    }
    if (a) all.push_back(a);
    if (igate != 0) all.push_back(gate);
    return Box{on_device(who, all), nx, ny, nz, igate, igate != 0 ? gate : nullptr};
}

// the reference's loop (host arrays): plane j of u(nx, ny, nz) is u(:, j, :), k outer, i inner; the volume (j = ny) is the same loop over
// u(nx*ny, 1, nz), that is every point in one flat loop (statistics/pdf.f90:74)
template <class F>
void for_plane(const Box &B, int j, F &&fn) {
    if (j < B.ny) {
        for (int k = 0; k < B.nz; ++k)
            for (int i = 0; i < B.nx; ++i) fn(((size_t)k * B.ny + j) * B.nx + i);
    } else {
        const size_t n = (size_t)B.nx * B.ny * B.nz;
        for (size_t i = 0; i < n; ++i) fn(i);
    }
}

// the fields v0 .. of u[nv] that one launch takes, at most per
inline PdfFields group(const Box &B, const double *const *u, size_t v0, size_t nv, size_t per = PDF_FIELDS_PER_LAUNCH) {
    PdfFields F{};
    F.nv = (int)std::min(per, nv - v0);
    for (int i = 0; i < F.nv; ++i) F.f[i] = u[v0 + i];
    F.gate = B.gate; F.igate = B.igate; F.nx = B.nx; F.ny = B.ny; F.nz = B.nz;
    return F;
}

// utils/pdfs.f90:50-57 (from the first point) and :144-153 (gated: from big_wp) of the planes and of the volume: mm [nv][ny + 1][2].  The ONE
// definition behind tlab_pdf1v_n and tlab_cavg1v_n, which bin on the same intervals.  One synchronisation.
inline void minmax_pass(const Box &B, Scratch &scratch, const double *const *u, size_t nv, std::vector<double> &mm) {
    const size_t np = (size_t)B.ny + 1;
    mm.assign(nv * np * 2, 0.0);
    if (nv == 0) return;
    if (!B.dev) {
        for (size_t v = 0; v < nv; ++v)
            for (int j = 0; j <= B.ny; ++j) {
                double mn, mx;
                if (B.gate) { mn = PDF_BIG; mx = -PDF_BIG; }
                else mn = mx = u[v][j < B.ny ? (size_t)j * B.nx : 0];
                for_plane(B, j, [&](size_t i) {
                    if (B.gate && B.gate[i] != B.igate) return;
                    mn = u[v][i] < mn ? u[v][i] : mn;
                    mx = u[v][i] > mx ? u[v][i] : mx;
                });
                mm[(v * np + j) * 2] = mn; mm[(v * np + j) * 2 + 1] = mx;
            }
        return;
    }
    hipStream_t st = tlab_current_stream();
    const size_t npart = (size_t)PDF_FIELDS_PER_LAUNCH * pdf_chunks(B.nz) * B.ny * 2;
    double *dmm = scratch.doubles(nv * np * 2 + npart), *partial = dmm + nv * np * 2;
    for (size_t v0 = 0; v0 < nv; v0 += PDF_FIELDS_PER_LAUNCH) hk(launch_pdf_minmax(group(B, u, v0, nv), partial, dmm + v0 * np * 2, st), "k_pdf_minmax");
    hk(hipMemcpyAsync(mm.data(), dmm, mm.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(min/max)");
    hk(hipStreamSynchronize(st), "sync");
}

// The two interval passes of the joint statistics of f = (u, v) (PDF2V2D, utils/pdfs.f90:241-268): min / max of u, then of v in every u-bin.
// iv [ny + 1][2] = (umin, ustep) and viv [ny + 1][nb1][2] = (vmin, vstep) of every plane (of the volume as plane ny; plane 0 alone when ny == 1);
// the centres of the first and last bin go to row j of out, rows ld apart, at nb1 * nb2 (u) and at nb1 * nb2 + 2 (v, nb1 firsts, then nb1 lasts).
// Device arrays: two synchronisations, and nothing of the scratch is the caller's afterwards.
inline void joint_intervals(const Box &B, Scratch &scratch, const double *const *f, int nb1, int nb2, double *out, size_t ld, std::vector<double> &iv,
                            std::vector<double> &viv) {
    const size_t np = (size_t)B.ny + 1, npl = B.ny > 1 ? np : 1, nb = (size_t)nb1 * nb2;
    std::vector<double> mm, rng(np * nb1 * 2);
    iv.assign(np * 2, 1.0);
    viv.assign(np * nb1 * 2, 1.0);
    minmax_pass(B, scratch, f, 1, mm);
    for (size_t j = 0; j < npl; ++j) {
        iv[2 * j] = mm[2 * j];
        iv[2 * j + 1] = pdf_step(mm[2 * j], mm[2 * j + 1], nb1, out + j * ld + nb, out + j * ld + nb + 1);
    }
    if (!B.dev) {
        const double *u = f[0], *v = f[1];
        for (size_t j = 0; j < npl; ++j) {
            for (int up = 0; up < nb1; ++up) { rng[(j * nb1 + up) * 2] = PDF_BIG; rng[(j * nb1 + up) * 2 + 1] = -PDF_BIG; }
            for_plane(B, (int)j, [&](size_t i) {
                const int up = pdf_bin(u[i], iv[2 * j], iv[2 * j + 1], nb1, false);
                if (up < 0 || up >= nb1) return;
                double *r = &rng[(j * nb1 + up) * 2];
                r[0] = v[i] < r[0] ? v[i] : r[0];
                r[1] = v[i] > r[1] ? v[i] : r[1];
            });
        }
    } else {
        hipStream_t st = tlab_current_stream();
        const size_t o_rng = up16(iv.size() * 8), o_vp = o_rng + up16(rng.size() * 8), o_part = o_vp + up16((size_t)B.ny * nb1 * 2 * 8);
        char *buf = scratch.bytes(o_part + up16((size_t)pdf_chunks(B.nz) * B.ny * 2 * nb1 * 2 * 8));
        hk(hipMemcpyAsync(buf, iv.data(), iv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(intervals)");
        hk(launch_pdf2v_range(group(B, f, 0, 2), nb1, (double *)buf, (double *)(buf + o_part), (double *)(buf + o_vp), (double *)(buf + o_rng), st),
           "k_pdf2v_range");
        hk(hipMemcpyAsync(rng.data(), buf + o_rng, rng.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(ranges)");
        hk(hipStreamSynchronize(st), "sync");      // (iv lives until here)
    }
    for (size_t j = 0; j < npl; ++j)
        for (int up = 0; up < nb1; ++up) {
            const size_t e = (j * nb1 + up) * 2;
            viv[e] = rng[e];
            viv[e + 1] = pdf_step(rng[e], rng[e + 1], nb2, out + j * ld + nb + 2 + up, out + j * ld + nb + 2 + nb1 + up);
        }
}

}  // namespace
}  // namespace tlab
