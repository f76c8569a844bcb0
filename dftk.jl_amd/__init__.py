"""dftk.jl_amd -- MI355X-native plane-wave Kohn-Sham SCF hot path behind DFTK.jl's operator API.

The directory name contains a dot, so import it through the repo-root shim::

    import dftk_jl_amd as dftk

Layout: ``csrc/`` hand-written HIP kernels + the C ABI (include/dftk_mi355x.h),
``_lib.py`` the ctypes binding, and the host-side mirror of the reference interface
(``PlaneWaveBasis``, ``Kpoint``, ``DftHamiltonianBlock`` + ``mul_``, ``lobpcg_hyper``,
``compute_density``, ``self_consistent_field``).
"""
from ._lib import load as load_library, DftkMiError, EXPORTED_SYMBOLS  # noqa: F401
from ._build import build as build_library  # noqa: F401
from .psp import PspHgh, PspUpf, load_psp, parse_psp_hgh, parse_psp_upf  # noqa: F401,E402
from .model import (Model, ElementPsp, model_DFT, model_atomic, create_supercell, silicon_cell,  # noqa: F401,E402
                    MonkhorstPack, ExplicitKpoints, ExactExchange, PBE0, model_HF)
from .exchange import (Coulomb, ShortRangeCoulomb, LongRangeCoulomb, SphericallyTruncatedCoulomb,  # noqa: F401,E402
                       WignerSeitzTruncatedCoulomb, ProbeCharge, ReplaceSingularity, VoxelAveraged, VanillaExx, AceExx,
                       compute_kernel_fourier, apply_exchange)
from .comm import KptComm, split_evenly, distribute_kpoints  # noqa: F401,E402
from .basis import PlaneWaveBasis, Kpoint, compute_fft_size  # noqa: F401,E402
from .hamiltonian import DftHamiltonianBlock, mul_  # noqa: F401,E402
from .terms import energy_hamiltonian, guess_density  # noqa: F401,E402
from .eigen import (lobpcg_hyper, diagonalize_all_kblocks, PreconditionerTPA, random_orbitals,  # noqa: F401,E402
                    columnwise_norms, columnwise_dots, ortho_qr, interpolate_kpoint, lobpcg_residual_history)
from .densities import (compute_density, compute_kinetic_energy_density,  # noqa: F401,E402
                        von_weizsaecker_kinetic_energy_density, guess_kinetic_energy_density)
from .mixing import (SimpleMixing, KerkerMixing, KerkerDosMixing, DielectricMixing, LdosMixing, HybridMixing,  # noqa: F401,E402
                     Chi0Mixing, compute_dos, compute_ldos)
from .scf import (self_consistent_field, next_density, compute_occupation, AdaptiveBands, FixedBands,  # noqa: F401,E402
                  AndersonAcceleration, determine_diagtol, ScfDefaultCallback, ScfStepper)
from .io import scfres_to_dict, save_scfres, load_scfres, basis_to_dict, model_to_dict  # noqa: F401,E402
from .symmetry import (SymOp, symmetry_operations, symmetrize_rho, irreducible_kcoords,  # noqa: F401,E402
                       symmetries_preserving_kgrid, symmetries_preserving_rgrid, check_group)
from .symmetry import symmetrize_forces, find_symmetry_preimage  # noqa: F401,E402
from .terms import energy_forces_ewald  # noqa: F401,E402
from .forces import compute_forces, compute_forces_cart, compute_forces_term  # noqa: F401,E402
from .symmetry import symmetrize_stresses  # noqa: F401,E402
from .terms import stress_ewald  # noqa: F401,E402
from .stresses import (compute_stresses_cart, compute_stresses_term, voigt_stress_to_full,  # noqa: F401,E402
                       full_stress_to_voigt, voigt_strain_to_full, full_strain_to_voigt)
from .memory_usage import estimate_memory_usage, plan_planewave_sharded, MemoryStatistics  # noqa: F401,E402
from .response import (occupation_divided_difference, compute_alpha_mn, is_effective_insulator,  # noqa: F401,E402
                       BandtolBalanced, BandtolGuaranteed, determine_band_tolerances, occupied_empty_masks,
                       compute_delta_occ, sternheimer_solver, apply_chi0_4P, apply_chi0, compute_delta_rho,
                       apply_kernel, solve_OmegaPlusK_split, solve_OmegaPlusK, compute_chi0,
                       multiply_psi_by_potential)
from .terms import dynmat_ewald  # noqa: F401,E402
from .bands import (KPath, kpath_interpolate, compute_bands, default_n_bands_bandstructure,  # noqa: F401,E402
                    atomic_orbital_projectors, atomic_orbital_projections, compute_pdos, sum_pdos)
from .phonon import (compute_dynmat, compute_dynmat_term, compute_delta_H_psi_alpha_s, phonon_modes,  # noqa: F401,E402
                     dynmat_red_to_cart, mass_matrix)
from .hubbard import (OrbitalManifold, Hubbard, resolve_hubbard_manifold, wigner_d_matrix,  # noqa: F401,E402
                      symmetrize_hubbard_n, compute_hubbard_n)
from .transfer import transfer_blochwave_kpt, transfer_blochwave, transfer_density  # noqa: F401,E402
from .refine import (RefinementResult, refine_scfres, refine_energies, refine_forces, invert_refinement_metric,  # noqa: F401,E402
                     select_occupied_orbitals, check_full_occupation, compute_projected_gradient, apply_Omega, apply_K)
from .direct_minimization import direct_minimization, backtracking, LbfgsNative  # noqa: F401,E402
from .newton import newton, solve_OmegaPlusK_cg, TangentSpace, apply_OmegaPlusK, TangentCgNative  # noqa: F401,E402
from .potential_mixing import (scf_potential_mixing, scf_potential_mixing_adaptive, AdaptiveDamping,  # noqa: F401,E402
                               FixedDamping, ScfAcceptStepAll, ScfAcceptImprovingStep, scf_damping_quadratic_model,
                               ensure_damping_within_range, propose_backtrack_damping, trial_damping,
                               total_local_potential, hamiltonian_with_total_potential)
from .unfold import apply_symop, unfold_bz, unfold_mapping, unfold_array  # noqa: F401,E402
from .wannier import (GaussianWannierProjection, HydrogenicWannierProjection, default_wannier_centers,  # noqa: F401,E402
                      radial_hydrogenic, overlap_Mmn_k_kpb, compute_mmn, compute_amn_kpoint, compute_amn, compute_nnkp,
                      complete_nnkp, read_w90_nnkp, write_w90_nnkp, write_w90_win, write_w90_eig, write_w90_amn, write_w90_mmn,
                      write_w90_unk, write_wannier90_files, wannier_spreads, projection_gauge, rotate_mmn)
