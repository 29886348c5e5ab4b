// Kernel argument blocks and host launchers (implemented in kernels.hip, pointwise.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "device_tables.hpp"

namespace tlab {

struct XLineArgs {          // k_xline: derivative along the contiguous index, n = 64*M
    const double *in0;      // field (u or s)
    const double *in1;      // advecting velocity (MODE_BURGERS)
    double *out0, *out1;
    const double *in0b;     // optional: operand = in0 + in0b_scale * in0b   (tmp = hq + q/dte fused into the divergence, P1 only)
    double in0b_scale;
    int acc;                // 1: out0 += value instead of out0 = value (MODE_P1, MODE_BURGERS); 2: out0 -= value (MODE_P1)
    long long nlines;
    StencilDev s1, s2;      // first / second derivative RHS operators
    SystemDev y1, y2;       // first / second derivative chunked systems (P = 64)
    double nu;
    // MODE_BURGERS with several transported fields sharing the advecting velocity in1 (nf >= 1): field f reads fs[f], adds to (acc) or
    // overwrites fo[f] with fnu[f] d2 - in1 d1.  in0 / out0 / nu are ignored then.
    int nf;
    const double *fs[4];
    double *fo[4];
    double fnu[4];
    // MODE_P1 "final update" epilogue (fq != NULL): instead of storing d = D1 u, finish the substep of one velocity component with it:
    //   h = out0 (tendency) ; hv = h - d ; hv = 0 on the wall planes j = 0, fny-1 ; fq += fdte hv ; h = fscale ? fkco hv : hv
    // (rhs_global_incompressible_1.f90:348-352, :373-375 for Dirichlet walls; time.f90:645-664, :272-297)
    double *fq;
    double fdte, fkco;
    int fscale, fnx, fny;
    const double *fpb, *fpt;      // final-update epilogue: wall tendencies of the planes j = 0 / fny-1, [fnx][nz] each (NULL: zero, Dirichlet walls)
    // MODE_BURGERS, 8 rows per lane at most: ffin[f] != 0 finishes the substep of transported field f (a scalar: no pressure term) in the epilogue
    // of this launch, which must be the LAST one that adds to its tendency:  h = fo[f] (+ this term) ; h = 0 on the wall planes ;
    // fs[f] += fdte h ; fo[f] = fscale ? fkco h : h     (time.f90:645-664, :272-297; Dirichlet walls)
    int ffin[4];
    // ... and (k_xline<.., CLIP = true> only) fclip[f] != 0: scalar bounds limiting of the updated field, fs[f] = min(max(fs[f], flo[f]), fhi[f])
    // (DNS_BOUNDS_LIMIT, dns_local.f90:67-90): 1 on every line, 2 on interior lines only (the wall planes are finished and clipped by k_wall_fix)
    int fclip[4];
    double flo[4], fhi[4];
    // ... and fdiv != NULL: for the field whose operand is the advecting velocity itself (u along x) the launch also writes the x term of the
    // pressure forcing, d/dx (h + fidte u) with the finished tendency h (rhs_global_incompressible_1.f90:197-230), into fdiv
    double *fdiv;
    double fidte;
    // MODE_BURGERS, anelastic (opr_burgers.f90:128-183, :504-507): the diffusion term of a line carries ribackground(j), j = line % ari_ny (x lines
    // run over (j, k)); ari == NULL: incompressible
    const double *ari;
    int ari_ny;
    int line_barriers;      // several waves per line and several lines per workgroup: the waves of a line meet at an LDS counter (xline_barrier); 0: workgroup barriers
};

struct RTileArgs {          // k_rtile: derivative along a strided index
    const double *in0;      // field
    const double *in1;      // first derivative (D1IN modes)
    const double *in2;      // advecting velocity (MODE_BURGERS_D1IN)
    double *out0;
    double *out1;           // first derivative (MODE_P2_P1 of k_htile)
    const double *in0b;     // optional second operand term: operand = in0 + in0b_scale * in0b (k_rtile MODE_P1)
    double in0b_scale;
    int acc;                // 1: out0 += value (k_rtile MODE_P1, k_htile MODE_BURGERS); 2: out0 -= value (MODE_P1)
    LineGeom g;
    StencilDev s1, s2;
    SystemDev y1, y2;       // chunked with P = n / rtile_chunk(n)  (k_htile: n / htile_chunk(n, mode))
    JacCorrDev jc;
    double nu;
    int nf;                 // k_htile MODE_BURGERS: as in XLineArgs (velocity = in2)
    const double *fs[4];
    double *fo[4];
    double fnu[4];
    // MODE_P1 "final update" epilogue (fq != NULL): instead of storing d = D1 u, finish the substep of one velocity component with it:
    //   h = out0 (tendency) ; hv = h - d ; hv = 0 on the wall planes j = 0, fny-1 ; fq += fdte hv ; h = fscale ? fkco hv : hv
    // (rhs_global_incompressible_1.f90:348-352, :373-375 for Dirichlet walls; time.f90:645-664, :272-297)
    double *fq;
    double fdte, fkco;
    int fscale, fnx, fny;
    const double *fpb, *fpt;      // final-update epilogue: wall tendencies of the planes j = 0 / fny-1, [fnx][nz] each (NULL: zero, Dirichlet walls)
    // k_htile MODE_BURGERS: bit f of fresh_mask set = field f OVERWRITES its tendency although acc is set (a field whose first term this launch
    // adds, in a launch that accumulates for the others)
    unsigned fresh_mask;
    // k_htile MODE_BURGERS with ONE field that is the advecting velocity itself (v along y, w along z), in the LAST launch that adds to its
    // tendency h: fdiv != NULL also ADDS this direction's term of the pressure forcing, d/dy (h + fidte v) (rhs_global_incompressible_1.f90:197-230),
    // to fdiv -- a third solve on the lines the workgroup holds anyway, instead of a separate pass that re-reads h and v
    double *fdiv;
    double fidte;
    // k_rtile MODE_P1 along y on the FINISHED tendency h (= in0) of a field with Neumann walls (fneu: bit 0 = jmin, bit 1 = jmax): the derivative of
    // the Neumann variant is not stored; its rows 1 / n-2 give the wall tendencies of BOUNDARY_BCS_NEUMANN_Y (boundary_bcs.f90:368-473; fcb / fct =
    // the three stencil coefficients and the LHS coefficient, as k_neumann_planes takes them), a Dirichlet side gets zero, and the final update of
    // k_final_update follows in the same launch: q (= fq) += fdte h, h = fscale ? fkco h : h.
    int fneu;
    double fcb[4], fct[4];
    // k_htile MODE_BURGERS, anelastic: ribackground [ari_ny] on the diffusion term -- ari_mode 1: lines along y, the factor of row j; 2: lines along z,
    // the factor of the tile's y row, j = (first line / ari_nx) % ari_ny (32-line tiles inside one row: ari_nx % 32 == 0)
    const double *ari;
    int ari_mode, ari_nx, ari_ny;
};

struct GenericArgs {        // k_generic: any n
    const double *in0;
    const double *in1;      // first derivative for the Jacobian correction (may be NULL)
    double *out0;
    LineGeom g;
    StencilDev s;
    SystemDev y;            // chunked with P = 1; red[0] = 1 / beta
    JacCorrDev jc;
};

// k_penta1: first derivative of CompactJacobian6Penta (pentadiagonal LHS, 7-diagonal antisymmetric RHS), one thread per line, the
// reference's own operation sequence: MatMul_7d_antisym (fdm_matmul.f90:491-558) + PENTADSS2 / PENTADPSS (utils/linear5.f90:207-411)
struct PentaArgs {
    const double *in0;
    double *out0;
    LineGeom g;
    const double *rhs;      // [7][n] device, column-major g%der1%rhs
    const double *lu;       // [7][n] periodic | [20][n] (4 Neumann variants x 5 columns), exactly g%der1%lu
    int periodic, ibc;
    double rb[4 * 8];       // rhs_b(4,0:7): [(j-1) + 4 c]
    double rt[5 * 7];       // rhs_t(0:4,7): [r + 5 (c-1)]
};
hipError_t launch_penta1(const PentaArgs &a, hipStream_t st);

// k_pentatile (pentatile.hip): the same operator on register tiles; rows / blocks / smw: device copies of what pentatile_build makes
struct PentaTileArgs {
    const double *in0;
    double *out0;
    LineGeom g;
    const double *rhs;      // as PentaArgs
    const double *rows;     // [9][n]
    const double *blocks;   // [2][C][C][4]
    const double *smw;      // [2][n] + 8 (periodic lines)
    double r6, r7;          // interior coefficients rhs(5, 6), rhs(5, 7)
    int periodic, ibc;
    double rb[4 * 8];
    double rt[5 * 7];
};
bool pentatile_ok(const LineGeom &g);
void pentatile_build(int n, int C, bool periodic, int ibc, const double *lu, std::vector<double> &rows, std::vector<double> &blocks, std::vector<double> &smw);
hipError_t launch_pentatile(const PentaTileArgs &a, hipStream_t st);
bool pentatile_x_ok(const LineGeom &g);                                   // lines along x: 16 lines per workgroup through an LDS tile
hipError_t launch_pentatile_x(const PentaTileArgs &a, hipStream_t st);

bool xline_supported(int n);
int rtile_chunk(int n);
void rtile_force_chunk(int m);
hipError_t launch_xline(int mode, int n, int chunks, bool lane_variant, const XLineArgs &a, hipStream_t st);
hipError_t launch_rtile(int mode, const RTileArgs &a, hipStream_t st);
int htile_chunk(int n, int mode);
void ptile_set_grid(int n);       // tests: forced grid of the persistent kernel (0 = default)
void htile_set_lines(int lines);   // tuning: 16 = narrow Burgers tiles (two workgroups per CU)
bool htile_narrow();
hipError_t launch_htile(int mode, const RTileArgs &a, hipStream_t st);
hipError_t launch_generic(bool sym, const GenericArgs &a, hipStream_t st);
hipError_t launch_burgers_epilogue(double *out, const double *vel, const double *d1, double nu, long long ntot, hipStream_t st);
hipError_t launch_fill(double *out, double v, long long ntot, hipStream_t st);
hipError_t launch_transpose(const double *a, double *b, int nra, int nca, hipStream_t st);

// pointwise.hip
hipError_t launch_add3(double *h, const double *a, const double *b, const double *c, long long n, hipStream_t st);
hipError_t launch_axpy3(double *o1, double *o2, double *o3, const double *h1, const double *h2, const double *h3, const double *q1,
                        const double *q2, const double *q3, double s, long long n, hipStream_t st);
hipError_t launch_axpy3w(double *o1, double *o2, double *o3, const double *h1, const double *h2, const double *h3, const double *q1,
                         const double *q2, const double *q3, double s, const double *w, int nx, int ny, long long n, hipStream_t st);
hipError_t launch_minmax_partial(const double *a, const double *v, const double *w, const double *odx, const double *ody, const double *odz,
                                 int mode, int nx, int ny, int nz, int koff, int zon, double *part, int nblocks, hipStream_t st);
hipError_t launch_negate(double *a, long long n, hipStream_t st);
hipError_t launch_scale(double *a, double alpha, long long n, hipStream_t st);
hipError_t launch_surface_flux(double *ref, const double *t, int j, int javg, double sign, double diff, double cpl, double *avg_scratch, int nx, int ny,
                               int nz, hipStream_t st);
hipError_t launch_weight_y(double *out, const double *in, const double *w, int nx, int ny, long long n, int mode, hipStream_t st);
hipError_t launch_burgers_epilogue_anelastic(double *out, const double *vel, const double *d1, double nu, const double *ri, int nx, int ny,
                                             long long n, hipStream_t st);
hipError_t launch_pencil_repack(double *a, double *buf, int nxh, int ny, int kmax, int nproc, const int *ioff, const long long *base, int dir,
                                hipStream_t st);
hipError_t launch_add1(double *h, const double *a, long long n, hipStream_t st);
hipError_t launch_axpy1(double *o, const double *a, const double *b, double s, long long n, hipStream_t st);
hipError_t launch_sum3(double *a, const double *b, const double *c, long long n, hipStream_t st);
// r = ((vx - uy)**2 + (uz - wx)**2) + (wy - vz)**2, unfused (FI_VORTICITY); r aliases no input; at most 2^31 - 1 points
hipError_t launch_vorticity_magnitude(const double *vx, const double *uy, const double *uz, const double *wx, const double *wy, const double *vz,
                                      double *r, long long n, hipStream_t st);
hipError_t launch_sub3(double *h1, double *h2, double *h3, const double *a, const double *b, const double *c, long long n, hipStream_t st);

hipError_t launch_get_wall_planes(const double *f, double *hb, double *ht, int nx, int ny, int nz, hipStream_t st);
hipError_t launch_fill_wall_planes(double *f, double vb, double vt, int nx, int ny, int nz, hipStream_t st);
struct ClipBounds { double lo, hi; };      // scalar bounds limiting (DNS_BOUNDS_LIMIT): s = min(max(s, lo), hi) after the update; NULL: none
hipError_t launch_final_update(double *q, double *h, const double *g, const double *pb, const double *pt, double dte, double kco, int scale,
                               int nx, int ny, int nz, hipStream_t st, const double *gw = nullptr, const ClipBounds *clip = nullptr);
hipError_t launch_clip(double *a, double lo, double hi, long long n, hipStream_t st);
hipError_t launch_rk_update(double *q, double *h, double dte, double kco, int scale, long long n, hipStream_t st, const ClipBounds *clip = nullptr);
hipError_t launch_set_wall_planes(double *f, const double *pb, const double *pt, int nx, int ny, int nz, hipStream_t st);
// RELAX_BLOCK of a J zone (boundary_buffer.f90:463-490) for nf <= 4 fields: h[f] -= tau[f][jloc] (a[f] - ref[f]) on the planes [offset, offset + size);
// ref: device, (nx, size, nz) per field, and tau: device, size doubles per field, both starting at the first field of the launch
hipError_t launch_buffer_relax(int nf, double *const *h, const double *const *a, const double *ref, const double *tau, int nx, int ny, int nz,
                               int offset, int size, hipStream_t st);
// ... and the tail of the substep on the plane jloc of the zone (k_buffer_relax<.., PLANE>): h = bc - tau (s - ref); s = clip(s + dte h); h *= kco.
// bc (may be NULL) / bc[f] NULL: zero; clip (may be NULL) / clip[f] NULL: no bounds
hipError_t launch_buffer_relax_plane(int nf, double *const *h, double *const *s, const double *ref, const double *tau, const double *const *bc,
                                     const ClipBounds *const *clip, double dte, double kco, int scale, int nx, int ny, int nz, int offset, int size,
                                     int jloc, hipStream_t st);
// TLab_Sources_Flow (tlab_sources.f90:36-92) in one launch (k_body_force): Coriolis, then hq_i += g_i b.  cor: 0 off, 1 EQNS_COR_EXPLICIT, 2
// EQNS_COR_NORMALIZED; bod: 0 off, 1 HOMOGENEOUS, 2 LINEAR with 1..3 scalars, 3 LINEAR general branch, 4 BILINEAR, 5 QUADRATIC.  f, g: the vectors;
// c: the coefficients as the kernel takes them; sidx: which scalar feeds slot is (ns slots in use); prof: ny device values (bod >= 2).  Arrays no
// active term needs are not accessed and may be NULL; with nothing active nothing is launched.  At most 2^31 - 1 points.
constexpr int BODY_FORCE_MAX_SCAL = 6;
struct BodyForce {
    int cor = 0, bod = 0, ns = 0;
    double f[3] = {0, 0, 0}, g[3] = {0, 0, 0}, c[BODY_FORCE_MAX_SCAL] = {0, 0, 0, 0, 0, 0}, geo_u = 0.0, geo_w = 0.0;
    int sidx[BODY_FORCE_MAX_SCAL] = {0, 1, 2, 3, 4, 5};
    bool any() const { return (cor == 1 && (f[0] != 0.0 || f[1] != 0.0 || f[2] != 0.0)) || (cor == 2 && f[1] != 0.0) || (bod != 0 && (g[0] != 0.0 || g[1] != 0.0 || g[2] != 0.0)); }
};
hipError_t launch_body_force(const BodyForce &F, double *const *hq, const double *const *q, const double *const *s, const double *prof, int nx, int ny,
                             int nz, hipStream_t st);
// THERMO_AIRWATER_LINEAR (thermo_airwater.f90:483-516), what FI_DIAGNOSTIC calls for imixture = MIXT_TYPE_AIRWATER_LINEAR: the normalized liquid
// l from xi = 1 + p1 s1 [+ p2 s2] (two scalars whenever ns > 1, as the reference), l = max(xi, 0) when |pd| < small_wp, else l = pd log(exp(xi / pd) + 1)
// with 1 / pd formed first and multiplied, unfused.  s2 may be NULL when ns = 1.  At most 2^31 - 1 points.
hipError_t launch_airwater_linear(double *l, const double *s1, const double *s2, int ns, double p1, double p2, double pd, long long n, hipStream_t st);

// radiation.hip: Radiation_Infrared_Y, gray liquid, added to hs (k_infrared_y).  The coefficients every column shares: InfraredCoef by value (the
// boundary rows of the right-hand side, the closure of row 1) and tab, [ny][8] device doubles (infrared_build_tables gives the host copy).
// scr1: one field of scratch; scr2: a second one, read only when flux_bottom != 0.  l, hs and the scratch fields must not alias.
struct InfraredCoef { double rb[3][4], rt[2][4], l0[3]; };
struct DerTables;
void infrared_build_tables(const DerTables &g, std::vector<double> &tab, InfraredCoef &C);
hipError_t launch_infrared_y(const double *l, double *hs, double *scr1, double *scr2, const double *tab, const InfraredCoef &C, double kappa,
                             double flux_top, double flux_bottom, int nx, int ny, int nz, hipStream_t st);

// averages.hip: plane statistics (k_plane_partial + k_plane_final).  prog, param: a program of averages_host.hpp (AVG_PROG_*; param = the number of
// fields, imom, or 1 with a pressure field); f: its fields; means: device, [nmean][ny] (NULL for a program without means); partial: device scratch,
// plane_moments_chunks(nz) * ny * nout doubles; prof: device, [nout][ny], the result.  Nothing is copied or synchronised here.
int plane_moments_chunks(int nz);
// denom: what k_plane_final divides the sums by; 0: real(nx*nz, wp) (the towers divide by a default real, dns_tower.f90:535)
hipError_t launch_plane_moments(int prog, int param, int nx, int ny, int nz, const double *const *f, const double *means, double *partial,
                                double *prof, hipStream_t st, double denom = 0.0);

// sampling.hip: phase averages, towers, saved planes (k_phase_space, k_tower_gather, k_tower_means, k_planes_gather) and the pointwise passes of
// PLANES_LOG.  Nothing is copied or synchronised here.
//   launch_phase_space  nf = 1..3 fields of nxy * nz doubles; stress (nf = 3 only): the six products too; out, last: nf (+ 6) planes of nxy doubles
//                       each, the plane of this sample (overwritten) and the running mean (last += out / avg_planes)
//   launch_tower_gather dst[f][(kk * ti + ii) * tj + j] = f[f](ipos[ii], jpos[j], kpos[kk]); ipos, jpos, kpos: device, 1-based; t_slot, it_slot
//                       (both or neither): take rtime and itime
//   launch_tower_means  dst[f][j] = prof[f * ny + jpos[j] - 1]
//   launch_planes_gather  dir 1: out(ny, nvars * n, nz), 2: out(nx, nvars * n, nz), 3: out(nx, ny, nvars * n), slot v * n + m = plane nodes[m]
//                       (HOST array, 1-based, checked) of field v; single: out is float
constexpr int PLANES_MAX_VARS = 16, PLANES_MAX_NODES = 20;      // vars(16) of PLANES_SAVE, MAX_SAVEPLANES (planes.f90:22, :224)
hipError_t launch_phase_space(int nf, bool stress, const double *const *f, double *const *out, double *const *last, long long nxy, int nz, int nz_total,
                              int avg_planes, hipStream_t st);
hipError_t launch_tower_gather(int nf, const double *const *f, double *const *dst, const int *ipos, const int *jpos, const int *kpos, int ti, int tj, int tk,
                               int nx, int ny, double *t_slot, double *it_slot, double rtime, int itime, hipStream_t st);
hipError_t launch_tower_means(const double *prof, int ny, const int *jpos, int tj, int nf, double *const *dst, hipStream_t st);
hipError_t launch_planes_gather(int nx, int ny, int nz, int nvars, const double *const *f, int dir, int n, const int *nodes, void *out, bool single,
                                hipStream_t st);
hipError_t launch_gradient_magnitude(double *r, const double *t, bool second, long long n, hipStream_t st);      // r = r*r + t*t | r = r + t*t
hipError_t launch_log10_small(double *a, long long n, hipStream_t st);                                            // a = log10(a + small_wp)

// pdfs.hip: plane PDFs (k_pdf_minmax, k_pdf_hist and their final kernels; pdfs_host.hpp holds the bin of a point).  F: at most PDF_FIELDS_PER_LAUNCH
// fields of one box and the gate (igate != 0: only points with gate == igate take part).  Nothing is copied or synchronised here.
//   launch_pdf_minmax  partial: scratch, nv * pdf_chunks(nz) * ny * 2 doubles; mm: [nv][ny + 1][2] = (min, max) of every plane and of the volume
//   launch_pdf_hist    iv: [nv][ny + 1][2] = (umin, ustep) of every plane and of the volume; bit v of ext_mask: field v has an external interval
//                      (a point outside is dropped; otherwise the last point goes to the last bin), of vol_mask: the volume has an interval of its
//                      own and is binned too (otherwise its counts are the sum of the planes'); cnt: scratch, nv * pdf_chunks(nz) * ny * 2 * nbins
//                      32-bit words; volpart: scratch, nv * ny * nbins 64-bit words; pdf: [nv][ny + 1][nbins] counts as doubles (plane ny: the volume,
//                      not written when ny == 1)
//   launch_pdf2v_range per u-bin min / max of v (PDF2V2D, utils/pdfs.f90:259-268), u-bins from iv [ny + 1][2]; partial: scratch,
//                      pdf_chunks(nz) * ny * 2 * nb1 * 2 doubles; volpart: scratch, ny * nb1 * 2 doubles; rng: [ny + 1][nb1][2] = (vmin, vmax)
//   launch_pdf2v_hist  the joint histogram: viv [ny + 1][nb1][2] = (vmin, vstep) of every u-bin; cnt, volpart as above with nbins = nb1 * nb2;
//                      pdf: [ny + 1][nb1 * nb2], bin (up, vp) at vp * nb1 + up
struct PdfFields {
    int nv;
    const double *f[8];
    const signed char *gate;
    int igate, nx, ny, nz;
};
int pdf_chunks(int nz);
hipError_t launch_pdf_minmax(const PdfFields &F, double *partial, double *mm, hipStream_t st);
hipError_t launch_pdf_hist(const PdfFields &F, int nbins, unsigned ext_mask, unsigned vol_mask, const double *iv, unsigned *cnt,
                           unsigned long long *volpart, double *pdf, hipStream_t st);
hipError_t launch_pdf2v_range(const PdfFields &F, int nb1, const double *iv, double *partial, double *volpart, double *rng, hipStream_t st);
hipError_t launch_pdf2v_hist(const PdfFields &F, int nb1, int nb2, const double *iv, const double *viv, unsigned *cnt, unsigned long long *volpart,
                             double *pdf, hipStream_t st);
hipError_t launch_gate_threshold(const double *a, long long n, double thr, signed char *gate, hipStream_t st);
//   launch_gate_count  INTER1V2D of every plane and level 1 .. np (at most GATE_MAX_LEVELS): cnt: scratch, pdf_chunks(nz) * ny * np 32-bit words;
//                      inter: [np][ny] = count / real(nx * nz)
hipError_t launch_gate_count(const signed char *gate, int nx, int ny, int nz, int np, unsigned *cnt, double *inter, hipStream_t st);

// conditional.hip: the partition of FI_GATE, the gated moments and the conditional averages (conditional_host.hpp holds the level of a point, the
// integer power and the limits).  Nothing is copied or synchronised here; F as above (launch_gated_moments: gate null = every point has level 1,
// igate is not read).
//   launch_gate_levels    thr: HOST, igate_size - 1 ascending thresholds, copied by value
//   launch_gated_moments  the levels g0 .. g0 + COND_LEVELS_PER_LAUNCH - 1 (those above L are dropped) and the moments 1 .. nm of the F.nv fields
//                         that are the fields v0 .. of nvt: partial: scratch, F.nv * pdf_chunks(nz) * ny * COND_LEVELS_PER_LAUNCH *
//                         gated_moments_width(nm) doubles; cnt: scratch, pdf_chunks(nz) * ny * COND_LEVELS_PER_LAUNCH 32-bit words; sums
//                         (ny, nm, nvt, L) and nsample (ny, L) in Fortran order: the raw undivided sums and the counts
//   launch_cavg_sum       the sums of a and the counts per bin of every F.f[v] (nb2 == 0: nb1 bins, intervals iv as launch_pdf_hist) or of
//                         (F.f[0], v2) (nb2 > 0: viv as launch_pdf2v_hist, bin (up, vp) at vp * nb1 + up); psum: scratch, F.nv * pdf_chunks(nz) *
//                         ny * 2 * nbins doubles, pcnt: as many 32-bit words; volsum: scratch, F.nv * ny * nbins doubles, volcnt: as many 64-bit
//                         words; sum, cnt: [F.nv][ny + 1][nbins] doubles (plane ny: the volume, written when ny > 1)
int gated_moments_width(int nm);
hipError_t launch_gate_levels(const double *a, long long n, int igate_size, const double *thr, signed char *gate, hipStream_t st);
hipError_t launch_gate_flux(const double *a, const double *v, long long n, signed char *gate, hipStream_t st);
hipError_t launch_gated_moments(const PdfFields &F, int nm, int g0, int L, int v0, int nvt, double *partial, unsigned *cnt, double *sums,
                                long long *nsample, hipStream_t st);
hipError_t launch_cavg_sum(const PdfFields &F, const double *v2, const double *a, int nb1, int nb2, unsigned ext_mask, const double *iv,
                           const double *viv, double *psum, unsigned *pcnt, double *volsum, unsigned long long *volcnt, double *sum, double *cnt,
                           hipStream_t st);

// spectra.hip: plane spectra and correlations (index maps and ring lists: spectra_host.hpp).  Nothing is copied or synchronised here; every array is
// device memory.  a, b: complex (nx/2+1, ny, nz), natural kz; b null: an auto pair.
//   launch_spectrum_reduce     S: scratch, (nx/2) * (ny/nblock) * nz doubles; rowv: scratch, ny * nz doubles; ring_off [kr_total + 1], ring_mode: the
//                              lists of spectrum_rings(nx/2, nz, kr_total); outx (nx/2, ny/nblock), outz (nz/2, ny/nblock), outr (kr_total, ny/nblock)
//                              and out2d (nx/2, ny/nblock, nz; may be null) are accumulated into, variance (ny) is written
//   launch_cross_product       c = b conj(a) for n complex numbers; c may be a or b
//   launch_correlation_reduce  in (nx, ny, nz) real, normj (ny); lists of correlation_rings(nx, nz, nr_total); outx (nx, ny/nblock), outz (nz, ny/nblock),
//                              out2d (nx, ny/nblock, nz; may be null) and outr (nr_total, ny/nblock; null: no radial sums) are accumulated into,
//                              variance2 (ny) is written
//   launch_fluctuation         out = in - mean(j)
hipError_t launch_spectrum_reduce(int nx, int ny, int nz, int nblock, int kr_total, const double *a, const double *b, double *S, double *rowv,
                                  const int *ring_off, const int *ring_mode, double *out2d, double *outx, double *outz, double *outr,
                                  double *variance, hipStream_t st);
hipError_t launch_cross_product(const double *a, const double *b, double *c, long long n, hipStream_t st);
hipError_t launch_correlation_reduce(int nx, int ny, int nz, int nblock, int nr_total, const double *in, const double *normj, const int *ring_off,
                                     const int *ring_mode, double *out2d, double *outx, double *outz, double *outr, double *variance2,
                                     hipStream_t st);
hipError_t launch_fluctuation(int nx, int ny, int nz, const double *in, const double *mean, double *out, hipStream_t st);

hipError_t launch_wall_weighted(const double *a1, const double *a2, const double *wb, const double *wt, int K, double *ob1, double *ot1, double *ob2,
                                double *ot2, int nx, int ny, int nz, hipStream_t st);
hipError_t launch_wall_fix(double *q, double *h, const double *sb, const double *st, double dte, double kco, int scale, int nx, int ny, int nz,
                           hipStream_t stream, const ClipBounds *clip = nullptr);
hipError_t launch_sub2(double *o, const double *a, const double *b, long long n, hipStream_t st);
hipError_t launch_copy_blocks(int n, const double *const *src, double *const *dst, const long long *cnt, hipStream_t st);      // n device copies, batched launches
hipError_t launch_plane_avg(const double *t, int j, int nx, int ny, int nz, double *avg, hipStream_t st);
hipError_t launch_surface_flux_avg(double *ref, const double *t, int j, double sign, double diff, double cpl, double avg, int nx, int ny, int nz,
                                   hipStream_t st);
hipError_t launch_trp_copy(double *S, double *W, long long m, int P, long long c, int to_wire, hipStream_t st);
hipError_t launch_neumann_planes(const double *u, const double *du, const double *cb, const double *ct, int do_b, int do_t, double *hb,
                                 double *ht, int nx, int ny, int nz, hipStream_t st);

}  // namespace tlab
