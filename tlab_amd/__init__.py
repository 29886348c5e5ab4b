"""tlab_amd -- MI355X-native implementation of Tlab's Navier-Stokes RHS hot path.

The compute path is hand-written HIP (tlab_amd/csrc) behind the C ABI of include/tlab_amd.h, loaded here with
ctypes.  There is NO CPU fallback: importing works without a GPU (plan construction is host code), but every
operator raises TlabError unless tlab_init() found an MI355X.
"""
from .lib import TlabError, load, lib_path  # noqa: F401
from .operators import (  # noqa: F401
    FdmPlan, init, sync,
    OPR_P1, OPR_P2, OPR_P2_P1, OPR_B_SELF, OPR_B_U_IN, OPR_P1_INT_VP, OPR_P1_INT_PV, OPR_P0_INT_VP, OPR_P0_INT_PV,
    BCS_DD, BCS_ND, BCS_DN, BCS_NN,
    FDM_COM4_JACOBIAN, FDM_COM6_JACOBIAN_PENTA, FDM_COM6_JACOBIAN, FDM_COM6_JACOBIAN_HYPER, FDM_COM6_DIRECT, FDM_COM4_DIRECT,
    OPR_Partial_X, OPR_Partial_Y, OPR_Partial_Z,
    OPR_Burgers_X, OPR_Burgers_Y, OPR_Burgers_Z, Filter, OPR_FILTER_1D, OPR_FILTER, OPR_FILTER_FIELDS, set_dealiasing,
    TLab_Transpose, PoissonPlan, OPR_Poisson, OPR_Helmholtz, poisson_set_exact, BOUNDARY_BCS_NEUMANN_Y,
    avg_ik_v, avg1v2d_v, avg_moments_flow, avg_moments_scal, avg_gradients_flow, avg_ugradp, avg_gradients_scal,
    pdf1v_n, pdf_minmax_planes, pdf_histogram_planes, pdf_analize, pdf2v, gate_threshold,
    fi_vorticity, vorticity_from_gradients, inter_n_xz,
    avg_phase_space, avg_phase_flow, avg_phase_plane_id, Tower, planes_gather, fi_gradient, log10_small,
    MAPS, FI_DIFFUSION_KINDS, gradient_maps, velocity_gradients, scalar_gradient, fi_maps, fi_diffusion, fi_strain, fi_strain_tensor, fi_curl,
    fi_invariant_q, fi_invariant_r, fi_vorticity_production, fi_strain_production, fi_gradient_production, fi_strain_a,
)
