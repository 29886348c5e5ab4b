// The host side of the Lagrangian particles (particles.hip) that needs no device: the checks of the entry points' arguments and the layout of the
// sort's scratch array.  Plain C++ without a HIP header, so that a stand-alone program can include it and run under the host sanitizers
// (tools/particles_host_check.cpp).  Every function returns a TLAB_* code and leaves the reason in `why`; none touches memory it is not handed.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tlab_amd.h"

namespace tlab {

// inb_part of Particle_Initialize_Parameters (particle_procs.f90:102-112): the prognostic columns of l_q / l_hq
inline int particle_columns(int type) { return type == TLAB_PART_INERTIA ? 6 : 3; }

// tlab_dns_set_particles.  bcs < 0: the reference's default for the type (particle_procs.f90:65-67); *bcs_out is the code the kernel gets.
// Type 0 reads nothing else (it switches the particles off).
inline int particle_check_settings(int type, int bcs, double stokes, double settling, int *bcs_out, std::string &why) {
    if (type == 4 || type == 5 || type == 6) {
        why = "tlab_dns_set_particles: the bilinear cloud droplets (types 4, 5) and type 6 need Laplacians, FI_GRADIENT and the radiation at the particle: not built on the device";
        return TLAB_EUNSUPPORTED;
    }
    if (type != TLAB_PART_NONE && type != TLAB_PART_TRACER && type != TLAB_PART_INERTIA) { why = "tlab_dns_set_particles: unknown type"; return TLAB_EINVAL; }
    if (type == TLAB_PART_NONE) { *bcs_out = TLAB_PART_BCS_NONE; return TLAB_OK; }
    if (bcs > TLAB_PART_BCS_SPECULAR) { why = "tlab_dns_set_particles: unknown wall condition"; return TLAB_EINVAL; }
    if (!std::isfinite(stokes) || !std::isfinite(settling)) { why = "tlab_dns_set_particles: NaN / infinite values"; return TLAB_EINVAL; }
    if (type == TLAB_PART_INERTIA && !(stokes > 0.0)) { why = "tlab_dns_set_particles: inertial particles need stokes > 0"; return TLAB_EINVAL; }
    *bcs_out = bcs >= 0 ? bcs : (type == TLAB_PART_INERTIA ? TLAB_PART_BCS_SPECULAR : TLAB_PART_BCS_NONE);
    return TLAB_OK;
}

// np of every entry point: the launches index particles with 32 bits, as the project's boxes
constexpr long long PARTICLE_NP_MAX = 0x7fffffffLL;
inline int particle_check_count(const char *who, long long np, std::string &why) {
    if (np < 0) { why = std::string(who) + ": np < 0"; return TLAB_EINVAL; }
    if (np > PARTICLE_NP_MAX) { why = std::string(who) + ": more than 2^31 - 1 particles"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// an array of ncol device pointers, none null (checked only when there are particles)
template <class T>
inline int particle_check_columns(const char *who, const char *name, T *const *cols, int ncol, std::string &why) {
    if (!cols) { why = std::string(who) + ": " + name + " is null"; return TLAB_EINVAL; }
    for (int i = 0; i < ncol; ++i)
        if (!cols[i]) { why = std::string(who) + ": a column of " + name + " is null"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// tlab_dns_substep_particle
inline int particle_check_substep(bool has_particles, int ncol, double dte, double kco, long long np, double *const *q, double *const *l_q,
                                  double *const *l_hq, const int *nodes, std::string &why) {
    const char *who = "tlab_dns_substep_particle";
    if (!has_particles) { why = std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)"; return TLAB_EINVAL; }
    if (int rc = particle_check_count(who, np, why)) return rc;
    if (!std::isfinite(dte) || !std::isfinite(kco)) { why = std::string(who) + ": NaN / infinite dte or kco"; return TLAB_EINVAL; }
    if (np == 0) return TLAB_OK;
    if (int rc = particle_check_columns(who, "q", q, 3, why)) return rc;
    if (int rc = particle_check_columns(who, "l_q", l_q, ncol, why)) return rc;
    if (int rc = particle_check_columns(who, "l_hq", l_hq, ncol, why)) return rc;
    if (!nodes) { why = std::string(who) + ": nodes is null"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// ---- the transfers between particles and fields (k_particle_sample, k_particle_trajectories, k_particle_deposit) ----
// the fields of one launch of the sample and of the trajectories: longer lists go in groups of this many
constexpr int PARTICLE_FIELDS_PER_LAUNCH = 8;

// tlab_dns_field_to_particle: the positions are the first three columns of l_q whatever the type
inline int particle_check_sample(bool has_particles, int nvar, const double *const *fields, long long np, double *const *l_q, const int *nodes,
                                 double *const *out, std::string &why) {
    const char *who = "tlab_dns_field_to_particle";
    if (!has_particles) { why = std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)"; return TLAB_EINVAL; }
    if (int rc = particle_check_count(who, np, why)) return rc;
    if (nvar < 1) { why = std::string(who) + ": nvar < 1"; return TLAB_EINVAL; }
    if (np == 0) return TLAB_OK;
    if (int rc = particle_check_columns(who, "fields", fields, nvar, why)) return rc;
    if (int rc = particle_check_columns(who, "l_q", l_q, 3, why)) return rc;
    if (int rc = particle_check_columns(who, "out", out, nvar, why)) return rc;
    if (!nodes) { why = std::string(who) + ": nodes is null"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// tlab_dns_particle_to_field: the field is zero-filled even without particles, so it is never null
inline int particle_check_deposit(bool has_particles, long long np, double *const *l_q, const int *nodes, const double *field, std::string &why) {
    const char *who = "tlab_dns_particle_to_field";
    if (!has_particles) { why = std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)"; return TLAB_EINVAL; }
    if (int rc = particle_check_count(who, np, why)) return rc;
    if (!field) { why = std::string(who) + ": field is null"; return TLAB_EINVAL; }
    if (np == 0) return TLAB_OK;
    if (int rc = particle_check_columns(who, "l_q", l_q, 3, why)) return rc;
    if (!nodes) { why = std::string(who) + ": nodes is null"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// tlab_dns_set_trajectories: the table of (tag, slot j) sorted by tag, slot 1-based as l_traj_tags(j).  Tags are distinct and >= 1 (the
// reference's tags are 1 .. isize_part_total); nothing is stored in `table` unless the list is good.
constexpr long long PARTICLE_NTRAJ_MAX = 0x7ffffffeLL;      // ntraj + 1 rows are indexed with 32 bits
inline int particle_trajectory_table(bool has_particles, long long ntraj, const long long *tags, std::vector<std::pair<long long, int>> *table,
                                     std::string &why) {
    const char *who = "tlab_dns_set_trajectories";
    if (!has_particles) { why = std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)"; return TLAB_EINVAL; }
    if (ntraj < 0) { why = std::string(who) + ": ntraj < 0"; return TLAB_EINVAL; }
    if (ntraj > PARTICLE_NTRAJ_MAX) { why = std::string(who) + ": more than 2^31 - 2 trajectories"; return TLAB_EINVAL; }
    if (ntraj > 0 && !tags) { why = std::string(who) + ": tags is null"; return TLAB_EINVAL; }
    std::vector<std::pair<long long, int>> t((size_t)ntraj);
    for (long long j = 0; j < ntraj; ++j) {
        if (tags[j] < 1) { why = std::string(who) + ": a tag below 1"; return TLAB_EINVAL; }
        t[(size_t)j] = {tags[j], (int)(j + 1)};
    }
    std::sort(t.begin(), t.end());
    for (size_t j = 1; j < t.size(); ++j)
        if (t[j].first == t[j - 1].first) { why = std::string(who) + ": a tag is listed twice"; return TLAB_EINVAL; }
    table->swap(t);
    return TLAB_OK;
}

// tlab_dns_trajectories_accumulate: ncol = inb_part of the driver's type, ntraj = the rows of its table (0: none was set)
inline int particle_check_trajectories(bool has_particles, int ncol, long long ntraj, double rtime, long long counter, long long nsave,
                                       long long np, double *const *l_q, const int *nodes, const long long *tags, int nvar,
                                       const double *const *fields, const float *l_traj, std::string &why) {
    const char *who = "tlab_dns_trajectories_accumulate";
    if (!has_particles) { why = std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)"; return TLAB_EINVAL; }
    if (ntraj < 1) { why = std::string(who) + ": no tags are tracked on this driver (tlab_dns_set_trajectories)"; return TLAB_EINVAL; }
    if (int rc = particle_check_count(who, np, why)) return rc;
    if (nvar < 0) { why = std::string(who) + ": nvar < 0"; return TLAB_EINVAL; }
    if (nsave < 1 || counter < 1 || counter > nsave) { why = std::string(who) + ": counter outside 1 .. nsave"; return TLAB_EINVAL; }
    if (std::isnan(rtime)) { why = std::string(who) + ": rtime is NaN"; return TLAB_EINVAL; }
    if (np == 0) return TLAB_OK;
    if (int rc = particle_check_columns(who, "l_q", l_q, ncol, why)) return rc;
    if (nvar > 0)
        if (int rc = particle_check_columns(who, "fields", fields, nvar, why)) return rc;
    if (!nodes || !tags || !l_traj) { why = std::string(who) + ": nodes, tags or l_traj is null"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// The scratch of tlab_dns_particle_sort, every part on a 256-byte boundary of the array (the caller's pointer must have that alignment itself):
//   keys_in, keys_out   np 32-bit cell numbers each      idx_in, idx_out   np 32-bit particle numbers each
//   column              np 8-byte values: one array at a time is gathered into it and copied back
//   sort                what the radix sort asks for (sort_bytes: the answer of its size query for np pairs)
struct ParticleSortLayout {
    size_t keys_in = 0, keys_out = 0, idx_in = 0, idx_out = 0, column = 0, sort = 0, total = 0;
};
constexpr size_t PARTICLE_SCRATCH_ALIGN = 256;
inline int particle_sort_layout(long long np, size_t sort_bytes, ParticleSortLayout *L, std::string &why) {
    if (int rc = particle_check_count("tlab_dns_particle_sort", np, why)) return rc;
    if (sort_bytes > ((size_t)1 << 46)) { why = "tlab_dns_particle_sort: the radix sort asks for an absurd amount of scratch"; return TLAB_EINVAL; }
    const size_t n = (size_t)np, A = PARTICLE_SCRATCH_ALIGN;
    auto up = [](size_t b) { return (b + A - 1) / A * A; };      // (np <= 2^31 - 1 and sort_bytes <= 2^46: nothing here can wrap 64 bits)
    size_t at = 0;
    L->keys_in = at; at += up(4 * n);
    L->keys_out = at; at += up(4 * n);
    L->idx_in = at; at += up(4 * n);
    L->idx_out = at; at += up(4 * n);
    L->column = at; at += up(8 * n);
    L->sort = at; at += up(sort_bytes ? sort_bytes : 1);      // never empty: a null pointer there would turn the sort into its size query
    L->total = at;
    return TLAB_OK;
}

// tlab_dns_particle_sort with a scratch array (scratch == NULL is the size query and is answered before this)
inline int particle_check_sort(bool has_particles, int ncol, long long np, double *const *l_q, double *const *l_hq, const int *nodes,
                               const long long *tags, const void *scratch, long long scratch_bytes, size_t needed, std::string &why) {
    const char *who = "tlab_dns_particle_sort";
    if (!has_particles) { why = std::string(who) + ": no particles are set on this driver (tlab_dns_set_particles)"; return TLAB_EINVAL; }
    if (int rc = particle_check_count(who, np, why)) return rc;
    if (np == 0) return TLAB_OK;
    if (int rc = particle_check_columns(who, "l_q", l_q, ncol, why)) return rc;
    if (int rc = particle_check_columns(who, "l_hq", l_hq, ncol, why)) return rc;
    if (!nodes || !tags) { why = std::string(who) + ": nodes or tags is null"; return TLAB_EINVAL; }
    if (scratch_bytes < 0 || (unsigned long long)scratch_bytes < needed) { why = std::string(who) + ": the scratch array is too small (ask with scratch = NULL)"; return TLAB_EINVAL; }
    if (reinterpret_cast<size_t>(scratch) % PARTICLE_SCRATCH_ALIGN != 0) { why = std::string(who) + ": the scratch array must start on a 256-byte boundary"; return TLAB_EINVAL; }
    return TLAB_OK;
}

// bits of the sort key: the cell numbers are below ncell
inline unsigned particle_key_bits(unsigned long long ncell) {
    unsigned b = 1;
    while (b < 32 && ((unsigned long long)1 << b) < ncell) ++b;
    return b;
}

}  // namespace tlab
