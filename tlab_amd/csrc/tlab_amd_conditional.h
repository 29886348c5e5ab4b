/* C ABI of the conditional statistics of libtlab_amd.so: the partition of FI_GATE, the gated moments of AVG_N_XZ and the conditional averages
 * CAVG1V_N / CAVG2V (csrc/conditional.cpp, kernels in csrc/conditional.hip).  The types, the TLAB_* codes and the conventions are those of
 * include/tlab_amd.h, which this header includes.  It lies beside its sources: include/ and the tables of the entry points of include/tlab_amd.h
 * are closed lists that the existing tests hold (tests/test_capi_symbols.py, tests/deferred_entry_points.py); what those tests ask of a symbol of
 * include/tlab_amd.h -- exported by the library, bound in tlab_amd/lib.py, classified against a pending record of the deferred tail and run with
 * one pending -- tests/test_conditional_symbols.py asks of the symbols declared here, with tests/conditional_entry_points.py as their table. */
#ifndef TLAB_AMD_CONDITIONAL_H
#define TLAB_AMD_CONDITIONAL_H

#include "../../include/tlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- conditional statistics: the partition of FI_GATE, the gated moments of AVG_N_XZ, the conditional averages CAVG1V_N / CAVG2V -----------------
 * What tools/statistics/averages.f90 (opt_main 3-18) and pdfs.f90 put between a gate and its statistics, single rank, without their files.  Arrays
 * of a call are classified like tlab_avg_ik_v: all device memory (kernels of csrc/conditional.hip: no atomics on fp64, no global atomics, the
 * order of every sum a function of the shapes and the alignment alone, so a call repeats its bits) or all host memory (or no tlab_init: the
 * reference's loops in the reference's order, bit for bit the reference); a mix: TLAB_EINVAL.  Gates are int8 in the layout of a field.  Every
 * result array is HOST memory, Fortran order.
 *
 * tlab_gate_levels: the loop of mappings/fi_gate.f90:85-90: gate[i] = the first n in 1 .. igate_size - 1 with a[i] < thr[n - 1], else igate_size.
 *   thr: igate_size - 1 ascending absolute thresholds in HOST memory, copied by value; igate_size 1 .. 127.  A NaN gets igate_size.  On the device
 *   the call returns with the kernel enqueued on the library's stream, like tlab_gate_threshold.
 * tlab_gate_flux: the quadrants of :65-71: 1 where a > 0 and v >= 0, 2 where a <= 0 and v > 0, 3 where a < 0 and v <= 0, else 4.
 * tlab_dns_gate: FI_GATE for opt_cond 2 .. 7 on the driver's box, composed from the entry points above and the existing ones.  The indicator is
 *   s[opt_cond_scal - 1] (2) or q[1] (5), read in place and never copied; tlab_fi_vorticity into txc[0] with txc[1..6] as its six work arrays (3);
 *   tlab_fi_gradient into txc[0] with txc[1] as work (4); the fluctuation of s[opt_cond_scal - 1] (tlab_avg_ik_v, tlab_fluctuation) in txc[0]
 *   (6, 7).  7 is the quadrant partition with q[1]; the others classify with the thresholds, with opt_cond_relative == 1 first multiplied by
 *   (umax - umin) of tlab_minmax of the indicator, in fp64 on the host.  q, s, txc: HOST arrays of DEVICE pointers; txc may be NULL for 2 and 5.
 *   opt_cond == 8 (potential vorticity, FI_CURL): TLAB_EUNSUPPORTED; opt_cond == 1 (a gate read from a file) and any other value: TLAB_EINVAL.
 * tlab_avg_n_xz: the calculation of AVG_N_XZ (statistics/avg_xz.f90:10-70) over AVG1V2D / AVG1V2D1G (utils/averages.f90:114-137, :172-209) for
 *   every level at once.  np == 0: ungated, one "level" that holds every point (the gate is not read); np in 1 .. 127: the levels 1 .. np of the
 *   gate, from ONE pass over the gate and the fields (k_gated_moments).  With L = max(np, 1), each output may be NULL but not all three:
 *   avg(ny, nm, nv, L) is what AVG_N_XZ returns for igate = level, RAW_TO_CENTRAL applied (nm > 1); sums(ny, nm, nv, L) the raw undivided sums
 *   of a**m; nsample(ny, L) the counts -- the last two for a decomposed host that reduces over its ranks before it divides.  a**m is the
 *   Fortran runtime's integer power (square and multiply from the low bit) on both sides.  An empty level gives 0.  avg is bit for bit
 *   tlab_raw_to_central of sums / nsample.  nm 1 .. 10.  The call synchronises the stream.
 * tlab_raw_to_central: RAW_TO_CENTRAL (avg_xz.f90:72-102) on moments(nm) in place, host arithmetic.
 * tlab_cavg1v_n: the calculation of CAVG1V_N (statistics/cavg.f90:7-89): avg(nbins+2, ny+1, nv), the first nbins entries of a plane the averages
 *   of a over the bins of u[v] (0 for an empty bin), then the centres of the first and the last bin; the volume as plane ny+1 (zero when
 *   ny == 1).  ibc[v] == 0: the external interval [umin[v], umax[v]] (a point outside is dropped from sum and count alike), anything else: the
 *   local one; PDF_ANALIZE is never called.  igate != 0: only points with gate == igate.  sum, pdf (may be NULL): the same shape, the undivided
 *   sums of a and the counts.  All nv fields share the passes (min/max; the sums).  nbins at most CAVG_MAX_BINS = 1024.
 * tlab_cavg2v: CAVG2V (:93-155) over PDF2V2D, in the layout of tlab_pdf2v with the first nbins[0]*nbins[1] entries of each plane the averages
 *   of a.  nbins[0]*nbins[1] at most CAVG_MAX_BINS.  (The reference hands PDF2V2D work arrays that overlap; here they do not.)
 * On the device a sum per bin differs from the reference's by the order of its terms only: |got - ref| <= 2 (n-1) u sum|a| / n + 2 u |ref| per
 * bin with n its count, u = 2^-53, and likewise per raw moment with sum|a**m|; exactly summable data give the reference's bits.  Counts, nsample
 * and bin coordinates are the reference's. */
int tlab_gate_levels(const double *a, long long n, int igate_size, const double *thr, signed char *gate);
int tlab_gate_flux(const double *a, const double *v, long long n, signed char *gate);
int tlab_dns_gate(tlab_dns_t h, int opt_cond, int opt_cond_relative, int opt_cond_scal, int igate_size, const double *gate_threshold,
                  double *const *q, double *const *s, double *const *txc, signed char *gate);
int tlab_avg_n_xz(int nx, int ny, int nz, int nv, int nm, const double *const *u, int np, const signed char *gate, double *avg, double *sums,
                  long long *nsample);
int tlab_raw_to_central(int nm, double *moments);
int tlab_cavg1v_n(int nx, int ny, int nz, int nv, int nbins, const int *ibc, const double *umin, const double *umax, const double *const *u,
                  int igate, const signed char *gate, const double *a, double *avg, double *sum, double *pdf);
int tlab_cavg2v(int nx, int ny, int nz, const int *nbins, const double *u, const double *v, const double *a, double *avg);

#ifdef __cplusplus
}
#endif

#endif
