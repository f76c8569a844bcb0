/* dftk_mi355x.h -- C ABI of the MI355X-native plane-wave Kohn-Sham hot path.
 *
 * Drop-in boundary for DFTK.jl's SCF hot path.  The reference has no
 * FFI; its seams are Julia-level (the `architecture` kwarg, `HamiltonianBlock` + `mul!`, the
 * `eigensolver=` kwarg of `self_consistent_field`, `compute_density`).  Each entry point below
 * names the reference function it replaces (file:line under the DFTK.jl checkout); the Julia
 * `ccall` shim a maintainer would add is in INTEGRATION.md, the Python (ctypes) binding used
 * by this repo's host mirror is dftk.jl_amd/_lib.py.
 *
 * Conventions
 *  - complex = interleaved (re, im) IEEE fp64 (`dftk_mi_cplx`, 16 B); all arithmetic is fp64.
 *  - matrices are column-major with an explicit leading dimension counted in elements;
 *    orbital blocks psi are n_G x n_bands (one column per band), as in DFTK.
 *  - cubes are (nx, ny, nz) with x fastest: linear index i = ix + nx*(iy + ny*iz) -- exactly
 *    Julia's column-major linear index minus one.  `mapping0` is that 0-based index.
 *  - pointers suffixed `_h` are host pointers, `_d` device pointers (same device as the basis).
 *    Device buffers are owned by the caller; the library never frees them and only keeps the
 *    pointers explicitly documented as "borrowed".
 *  - every call returns an int status: 0 ok; <0 invalid argument / runtime (HIP, RCCL) error;
 *    >0 numerical failure (non-finite values, Cholesky breakdown, eigen-solver not converged).
 *    `dftk_mi_last_error()` gives a thread-local message for the last non-zero status.
 *  - calls are asynchronous on the basis' HIP stream unless they return host data
 *    (`dftk_mi_lobpcg`); `dftk_mi_basis_sync` blocks.
 *  - no call falls back to the CPU: a missing GPU is an error (status -100).
 */
#ifndef DFTK_MI355X_H
#define DFTK_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double re, im; } dftk_mi_cplx;

typedef struct dftk_mi_basis  dftk_mi_basis;   /* FFTGrid + device/stream          */
typedef struct dftk_mi_kblock dftk_mi_kblock;  /* Kpoint + DftHamiltonianBlock     */
typedef struct dftk_mi_comm   dftk_mi_comm;    /* comm_kpts (RCCL communicator)    */

/* ---- status codes -------------------------------------------------------------------------- */
#define DFTK_MI_OK                 0
#define DFTK_MI_EINVAL            (-1)
#define DFTK_MI_EHIP              (-2)
#define DFTK_MI_ERCCL             (-3)
#define DFTK_MI_ENOGPU            (-100)
#define DFTK_MI_NUM_NONFINITE       1   /* NaN/Inf met (reference: @assert !any(isnan, AX))      */
#define DFTK_MI_NUM_CHOLESKY        2   /* ortho!: Cholesky kept failing (reference: SVD fallback)*/
#define DFTK_MI_NUM_NORMALIZATION   3   /* "LOBPCG is badly failing to keep the vectors normalized"*/
#define DFTK_MI_NUM_EIGEN           4   /* dense Hermitian eigensolver did not converge          */
#define DFTK_MI_NUM_TOO_SMALL       5   /* N > 3M violated (lobpcg_hyper_impl.jl:363)            */
#define DFTK_MI_NUM_RANK_DEFICIENT  6   /* linearly dependent columns (ortho.jl:14 @assert)      */

const char* dftk_mi_last_error(void);
/* Library / build identification: "dftk_mi355x <version> gfx950 ..." */
const char* dftk_mi_version(void);

/* ---- basis: replaces FFTGrid(fft_size, unit_cell_volume, arch)  (src/fft.jl:76-98) -----------
 * Holds the 3 one-dimensional mixed-radix plans (radices 2,3,4,5 + generic primes), twiddle
 * tables, the HIP stream and the scratch pool.  `device` is the HIP device ordinal.          */
int dftk_mi_basis_create(int nx, int ny, int nz, double unit_cell_volume, int device,
                         dftk_mi_basis** basis_out);
int dftk_mi_basis_destroy(dftk_mi_basis* basis);
int dftk_mi_basis_sync(dftk_mi_basis* basis);              /* synchronize_device (architecture.jl) */
/* Bands processed per FFT launch group (scratch = n * (T1 + T2) bytes); default 8. */
int dftk_mi_basis_set_fft_batch(dftk_mi_basis* basis, int n_bands_per_batch);
/* HIP stream used by this basis (hipStream_t as void*) -- lets the caller order its own work. */
void* dftk_mi_basis_stream(dftk_mi_basis* basis);

/* ---- k-block: replaces Kpoint(...) (src/Kpoint.jl:20-41) + DftHamiltonianBlock
 *      (src/terms/Hamiltonian.jl:22-57).  `mapping0_h` must be ascending (as Kpoint builds it). */
int dftk_mi_kblock_create(dftk_mi_basis* basis, int64_t n_G, const int64_t* mapping0_h,
                          const double* kinetic_h /* n_G: fourier_op.multiplier, kinetic.jl:31-35 */,
                          dftk_mi_kblock** kb_out);
int dftk_mi_kblock_destroy(dftk_mi_kblock* kb);
/* nonlocal_op (src/terms/operators.jl:119-129): P is n_G x n_p (borrowed device pointer, must
 * outlive the k-block or the next call), D is the dense real n_p x n_p coupling matrix
 * (nonlocal.jl:107-141) on the host; its band structure is detected and exploited. n_p = 0 clears. */
int dftk_mi_kblock_set_projectors(dftk_mi_kblock* kb, int n_p, const dftk_mi_cplx* P_d, int64_t ldP,
                                  const double* D_h);
/* local_op.potential (operators.jl:71-78, :213-222): the SUM of all local terms on the cube,
 * un-normalised (the 1/N of Hamiltonian.jl:152-153 is applied inside).  Copied. NULL clears. */
int dftk_mi_kblock_set_potential(dftk_mi_kblock* kb, const double* V_d);
/* The same potential for n k-blocks (all k-points of a basis apply ONE summed local potential, Hamiltonian.jl:36-57):
 * one call instead of one host round trip per k-block.  V_d must stay unchanged until the blocks' streams have run. */
int dftk_mi_kblocks_set_potential(int n_kblocks, dftk_mi_kblock* const* kbs, const double* V_d);
/* Meta-GGA (DivAgradOperator, src/terms/operators.jl): a second cube, v_tau = de/dtau, bound like the local potential (copied,
 * un-normalised, NULL unbinds; the plural form shares one padded copy among the blocks of a basis).  With one bound,
 * dftk_mi_apply_H_parts(which & 1) adds  -1/2 div(v_tau grad psi) = 1/2 sum_a (G + k)_a fft(v_tau ifft((G + k)_a psi)),
 * (G + k) cartesian: three more transform pairs per band through the local-apply pipeline.  The block must know its k-point
 * first: dftk_mi_kblock_set_kpoint(kb, recip_lattice_h (3x3 column-major), kcoord_h (fractional)).  Un-sharded blocks of
 * complex orbitals only.  A block with a tau potential is refused (DFTK_MI_EINVAL, with a message) by the batched executor
 * (apply_H inside dftk_mi_lobpcg_multi) and by the Gamma-real format, which do not know the term, and never takes the A X
 * handover of dftk_mi_kblock_reuse_AX (binding or unbinding forgets a kept one).  With nothing bound every path runs as
 * before. */
int dftk_mi_kblock_set_kpoint(dftk_mi_kblock* kb, const double* recip_lattice_h, const double* kcoord_h);
int dftk_mi_kblock_set_tau_potential(dftk_mi_kblock* kb, const double* Vtau_d);
int dftk_mi_kblocks_set_tau_potential(int n_kblocks, dftk_mi_kblock* const* kbs, const double* Vtau_d);

/* ---- mul!(Hpsi, H::DftHamiltonianBlock, psi)  (src/terms/Hamiltonian.jl:137-192) ------------- */
int dftk_mi_apply_H(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                    dftk_mi_cplx* Hpsi_d, int64_t ld_Hpsi);
/* Pieces, for tests and profiling: which = 1 local (K1-K5: scatter, iFFT, V, FFT, gather),
 * 2 kinetic (K6), 4 nonlocal (K7-K9); OR-able.  dftk_mi_apply_H == which 7. */
int dftk_mi_apply_H_parts(dftk_mi_kblock* kb, int which, int n_bands, const dftk_mi_cplx* psi_d,
                          int64_t ld_psi, dftk_mi_cplx* Hpsi_d, int64_t ld_Hpsi);

/* ---- basis / term set-up ------------------------------------------------------------------
 * Kpoint(...) sphere enumeration (src/Kpoint.jl:20-41): all cube points with |B (G + k)|^2 / 2 <= Ecut in ascending
 * 0-based x-fastest linear index, their kinetic multipliers (src/terms/kinetic.jl:31-35) and integer G vectors
 * (3 per plane wave).  recip_lattice_h: 3x3 column-major (Julia's `model.recip_lattice`).  Host routine (no GPU
 * needed): call with cap = 0 / NULL buffers to get *n_G, then with buffers of that size. */
int dftk_mi_kpoint_sphere_host(int nx, int ny, int nz, const double* recip_lattice_h, const double* kcoord_h,
                               double Ecut, int64_t cap, int64_t* n_G, int64_t* mapping0_h, double* kinetic_h,
                               int32_t* G_h);
/* build_projection_vectors (src/terms/nonlocal.jl:166-244) for HGH pseudopotentials, written on the device:
 * P[g, c] = f_{l,i}(|q|) Y_lm(q) (-i)^l / sqrt(Omega) exp(-2 pi i (G + k).r_atom), q = B (G + k); columns atom by atom
 * in the order given, within an atom (l, m, i) as nonlocal.jl:228-229.  G_d: 3 ints per row (the rows of this rank's
 * slab for a sharded block); rp_h / n_proj_h: 4 entries (l = 0..3) per species: r_l and the number of radial
 * projectors; positions_h: 3 reduced coordinates per atom.  *n_p = number of columns (P_d may be NULL to query). */
int dftk_mi_build_projectors_hgh(dftk_mi_basis* basis, int64_t n_rows, const int32_t* G_d,
                                 const double* recip_lattice_h, const double* kcoord_h, double unit_cell_volume,
                                 int n_species, const double* rp_h, const int* n_proj_h, int n_atoms,
                                 const int* species_of_atom_h, const double* positions_h, dftk_mi_cplx* P_d,
                                 int64_t ldP, int* n_p);

/* Superposition of atomic form factors on the cube, real-space result:
 *   out(r) = irfft( enforce_real( sum_species ff_s(|G|) sum_{a in s} e^{-2 pi i G.r_a} / sqrt(Omega) ) )
 * kind 0: compute_local_potential (src/terms/local.jl:108-138) with the HGH local form factor
 *         (src/pseudo/PspHgh.jl:110-124); params_h[8 s + 0..5] = rloc, Zion, c1..c4
 * kind 1: Gaussian valence-density superposition of guess_density (src/density_methods.jl:111-125,158-181,236-244,
 *         un-normalised); params_h[8 s + 0..1] = decay length, valence charge.
 * Atoms grouped by species (species_of_atom_h non-decreasing); cube_kb spans the whole cube. */
int dftk_mi_atomic_superposition(dftk_mi_kblock* cube_kb, int kind, const double* recip_lattice_h, int n_species,
                                 const double* params_h, int n_atoms, const int* species_of_atom_h,
                                 const double* positions_h, double* out_d);
/* compute_forces(::TermAtomicLocal) (src/terms/local.jl:142-177): reduced-coordinate forces of the HGH local term,
 * the exact derivative of the local energy this library evaluates (the cube of dftk_mi_atomic_superposition kind 0
 * against the density, unpaired Nyquist entries dropped).  params / species / positions exactly as
 * dftk_mi_atomic_superposition kind 0; rho_d = TOTAL density on the cube (nz x ny x nx, x fastest);
 * forces_h[3 a + alpha] is overwritten.  Deterministic (fixed reduction order, no atomics). */
int dftk_mi_forces_local(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species, const double* params_h,
                         int n_atoms, const int* species_of_atom_h, const double* positions_h, const double* rho_d,
                         double* forces_h);
/* ---- numeric (UPF) norm-conserving pseudopotentials (src/pseudo/PspUpf.jl) -----------------------------------------
 * Radial transform of one channel on the device.  The quadrature rule of the reference (src/common/quadrature.jl) is
 * linear in the integrand: the caller folds it into weights w_i once per mesh and passes wf_h[i] = w_i * r2_f[i], cut at
 * the channel's own length n_r >= 1 (host arrays, read before the call returns), q_d / out_d: n_q device doubles.
 *   kind 0: out[j] = 4 pi sum_i wf_i r_i^l g_l(q_j r_i), g_l(x) = j_l(x) / x^l, l = 0..3: the modified Hankel transform
 *           (src/common/hankel.jl), finite at q = 0 (g_l(0) = 1 / (2l+1)!!).
 *   kind 1: the local potential (PspUpf.jl:229-242) with wf_i = w_i (r_i vloc_i + Zion erf(r_i)):
 *           out[j] = 4 pi (sum_i wf_i sin(q_j r_i) / q_j - Zion / q_j^2 exp(-q_j^2 / 4)); exactly 0 at q_j = 0; l ignored.
 * One lane per q, the sum over i in ascending order in that lane: deterministic.  Asynchronous on the basis' stream.
 * dftk_mi_radial_tile(): the number of mesh points the kernel stages through LDS at a time (host routine). */
int dftk_mi_radial_transform(dftk_mi_basis* basis, int kind, int l, int n_r, const double* r_h, const double* wf_h,
                             double Zion, int64_t n_q, const double* q_d, double* out_d);
int dftk_mi_radial_tile(void);
/* dftk_mi_build_projectors_hgh with tabulated radial parts: R_d[channel * ldR + row] = the kind-0 transform of the
 * channel at |B (G + k)| of the row (ldR >= n_rows); species s owns n_chan_h[4 s + l] channels of angular momentum l
 * (any number), channels first_chan_h[4 s + l] ... of R_d.  Same column order and P layout as the HGH entry. */
int dftk_mi_build_projectors_radial(dftk_mi_basis* basis, int64_t n_rows, const int32_t* G_d,
                                    const double* recip_lattice_h, const double* kcoord_h, double unit_cell_volume,
                                    int n_species, const double* R_d, int64_t ldR, const int* first_chan_h,
                                    const int* n_chan_h, int n_atoms, const int* species_of_atom_h,
                                    const double* positions_h, dftk_mi_cplx* P_d, int64_t ldP, int* n_p);
/* dftk_mi_atomic_superposition / dftk_mi_forces_local with the form factors read from a device table
 * ff_d[species * N + cube index] (N = nx ny nz, x fastest; the value at G = 0 included) instead of closed forms; the
 * unpaired-Nyquist rule, the species grouping and everything else as in those entries.  coeff_h (superposition only; NULL
 * = all 1): one amplitude per atom, as the per-atom coefficients of the spin-density guess
 * (src/density_methods.jl:126-152). */
int dftk_mi_atomic_superposition_table(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species,
                                       const double* ff_d, int n_atoms, const int* species_of_atom_h,
                                       const double* positions_h, const double* coeff_h, double* out_d);
int dftk_mi_forces_local_table(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species, const double* ff_d,
                               int n_atoms, const int* species_of_atom_h, const double* positions_h,
                               const double* rho_d, double* forces_h);
/* compute_forces(::TermAtomicNonlocal) (src/terms/nonlocal.jl:49-98) for ONE k-block, unsymmetrised: the block's P / D
 * (dftk_mi_kblock_set_projectors); kcoord_h = the k-point (reduced); psi_d = n_bands orbitals in the caller's
 * full-sphere layout (leading dimension ld_psi); weight_h[n] = kweight * occupation[n]; atom a owns projector columns
 * col_start_h[a] .. col_start_h[a + 1] (D must not couple atoms: DFTK_MI_EINVAL); forces_h[3 n_atoms] is ACCUMULATED.
 * One product P' [psi | i g_x psi | i g_y psi | i g_z psi] per band chunk (g = G + k reduced), then a per-atom
 * contraction with D.  Gamma-real block: real half-format products.  Sharded block: psi is this rank's row slab, the
 * projections are all-reduced over the block's communicator, every rank gets the full result.  Touches no LOBPCG
 * state of the block (kept A X, start buffers). */
int dftk_mi_forces_nonlocal(dftk_mi_kblock* kb, const double* kcoord_h, int n_bands, const dftk_mi_cplx* psi_d,
                            int64_t ld_psi, const double* weight_h, int n_atoms, const int* col_start_h,
                            double* forces_h);

/* ---- dynamical matrix at q = 0 (src/postprocess/phonon.jl), the explicit pieces (phonon_kernels.hip) ----
 * Reduced coordinates; fp64, fixed reduction order, no atomics: two calls give bitwise identical results.
 *
 * The local part of the perturbation of a displaced atom (compute_dynmat_dH(::TermAtomicLocal), src/terms/local.jl:183-213):
 *   out[alpha](r) = irfft( enforce_real( -2 pi i G_alpha ff_s(|G|) e^{-2 pi i G.R} / sqrt(Omega) ) ),  alpha = 0, 1, 2
 * i.e. the derivative of the cube of dftk_mi_atomic_superposition kind 0 with respect to the position of ONE atom of
 * species `species` at position_h[3] (same G set, same unpaired-Nyquist handling, params_h as there).  out_d: three real
 * cubes, one after the other; all three go through one transform pipeline.  Asynchronous on the basis' stream. */
int dftk_mi_local_potential_displacement(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species,
                                         const double* params_h, int species, const double* position_h, double* out_d);
/* compute_dynmat(::TermAtomicLocal), the explicit term (src/terms/local.jl:183-213): out_h[9 a + 3 beta + alpha] is
 * OVERWRITTEN with d^2 E_loc / dR_{a,beta} dR_{a,alpha}, the exact second derivative of the local energy this library
 * evaluates (of which dftk_mi_forces_local is minus the first).  Arguments as dftk_mi_forces_local.  One forward FFT of
 * the density, then one reduction per atom with the factors G_alpha G_beta. */
int dftk_mi_dynmat_local(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species, const double* params_h,
                         int n_atoms, const int* species_of_atom_h, const double* positions_h, const double* rho_d,
                         double* out_h);
/* compute_dHpsi_alpha_s, the nonlocal part (src/terms/nonlocal.jl:307-383) for ONE k-block and ONE atom: with P_s / D_s the
 * columns col_start_h[atom] .. col_start_h[atom + 1] of the block's bound P / D and g = G + k (reduced),
 *   out[alpha] = -2 pi i [ g_alpha o (P_s D_s P_s' psi) - P_s D_s P_s' (g_alpha o psi) ],  alpha = 0, 1, 2
 * out_d: three blocks of n_bands columns (leading dimension ld_out), one after the other.  One product
 * P_s' [psi | i g_x psi | i g_y psi | i g_z psi] per band chunk (the operands of dftk_mi_forces_nonlocal), the small
 * product with D_s, one back-product, and the row scaling fused into the store.  A Gamma-real block is accepted (the
 * products run in the complex full-sphere layout).  DFTK_MI_EINVAL, with out_d untouched: a plane-wave sharded block, a
 * D that couples this atom to another, a leading dimension below n_G, a call inside a batched multi-k call. */
int dftk_mi_nonlocal_displacement_apply(dftk_mi_kblock* kb, const double* kcoord_h, int atom, int n_atoms,
                                        const int* col_start_h, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                        dftk_mi_cplx* out_d, int64_t ld_out);
/* compute_dynmat(::TermAtomicNonlocal) (src/terms/nonlocal.jl:307-383) for ONE k-block; both outputs are ACCUMULATED.
 * dpsi_d non-NULL: dforces_h[3 a + alpha] += the derivative of what dftk_mi_forces_nonlocal returns along (dpsi, wd):
 *   -4 pi sum_n { wd_n Re[p_n' D_a q_alpha,n] + w_n Re[dp_n' D_a q_alpha,n + p_n' D_a dq_alpha,n] }
 * hess_h non-NULL: hess_h[9 a + 3 beta + alpha] += sum_n w_n <psi_n| d_alpha d_beta (P_a D_a P_a') |psi_n>
 *   = (2 pi)^2 sum_n w_n 2 Re[ c_alpha' D_a c_beta - c_alphabeta' D_a c ]
 * from the ten projected blocks P' [psi | g_alpha psi | g_alpha g_beta psi].  w_h[n] = kweight * occupation[n],
 * wd_h[n] = kweight * d occupation[n]; psi_d / col_start_h as dftk_mi_forces_nonlocal.  Refusals as
 * dftk_mi_nonlocal_displacement_apply (a coupling D of ANY atom), outputs untouched. */
int dftk_mi_dynmat_nonlocal(dftk_mi_kblock* kb, const double* kcoord_h, int n_bands, const dftk_mi_cplx* psi_d,
                            int64_t ld_psi, const dftk_mi_cplx* dpsi_d, int64_t ld_dpsi, const double* w_h,
                            const double* wd_h, int n_atoms, const int* col_start_h, double* dforces_h, double* hess_h);

/* ---- stress tensor (src/postprocess/stresses.jl), term by term at fixed orbital coefficients (stress_kernels.hip) ----
 * All results are Omega * sigma contributions in Cartesian coordinates, six numbers in the order xx, yy, zz, zy, zx, yx
 * (the reference's Voigt order).  fp64, fixed reduction order, no atomics: two calls give bitwise identical results.
 *
 * Kinetic and AtomicNonlocal of ONE k-block, unsymmetrised, ACCUMULATED into stress_h[0..5] (kinetic) and
 * stress_h[6..11] (nonlocal):
 *   kinetic   -sum_n w_n sum_G q_a q_b |psi_n(G)|^2,                         q = B (G + k)
 *   nonlocal   sum_n w_n 2 Re[ (P' psi_n)' D (dP_ab' psi_n) ],  dP_ab = -1/2 delta_ab P - 1/2 (q_a dP/dq_b + q_b dP/dq_a)
 * psi_d / ld_psi / weight_h / col_start_h as dftk_mi_forces_nonlocal; species tables (rp_h, n_proj_h: 4 entries per
 * species), species_of_atom_h and positions_h exactly as they were given to dftk_mi_build_projectors_hgh for this block
 * (atoms WITH projectors only; col_start_h must be the column offsets that table implies and end at the block's n_p,
 * else DFTK_MI_EINVAL).  The six derivative projectors are built on the fly for chunks of whole atoms and multiplied
 * by the library's zgemm (Gamma-real block: real half-format products).  Extra workspace: at most
 * max(512 MiB, 6 rows x the columns of one atom) for the derivative projectors plus (rows + 7 chunk columns) x band chunk
 * complex numbers, never a multiple of the whole P.  A plane-wave sharded block is refused (DFTK_MI_EINVAL). */
int dftk_mi_stress_kinetic_nonlocal(dftk_mi_kblock* kb, const double* recip_lattice_h, const double* kcoord_h,
                                    int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi, const double* weight_h,
                                    int n_species, const double* rp_h, const int* n_proj_h, int n_atoms,
                                    const int* species_of_atom_h, const double* positions_h, const int* col_start_h,
                                    double* stress_h);
/* AtomicLocal and Hartree sums over the cube from the TOTAL density rho_d (one forward FFT shared by both), written to
 * out_h[14]; rho(G) in the normalisation of the energies, unpaired Nyquist entries and G = 0 dropped:
 *   out[0..5]  = -sum_G Re[conj(rho(G)) sum_s S_s(G) ff_s'(|G|) / sqrt(Omega)] G_a G_b / |G|
 *   out[6..11] =  sum_G 4 pi |rho(G)|^2 G_a G_b / |G|^4
 *   out[12]    =  E_AtomicLocal,  out[13] = E_Hartree  (the -delta_ab E parts of both stresses)
 * params / species / positions as dftk_mi_forces_local; n_atoms may be 0 (Hartree only). */
int dftk_mi_stress_cube(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species, const double* params_h,
                        int n_atoms, const int* species_of_atom_h, const double* positions_h, const double* rho_d,
                        double* out_h);
/* Exchange-correlation sums over n grid points (plain sums, the caller multiplies by the volume element):
 *   out[0] = sum e  (0 when e_d is NULL),  out[1] = sum_s sum v_rho,s rho_s,
 *   out[2..7] = sum v_sigma grad_a rho grad_b rho  (0 when vsigma_d is NULL)
 * rho_d / vrho_d: n_spin (1 or 2) arrays of n values; grad_d: 3 arrays of n values (x, y, z; n_spin == 1 only). */
int dftk_mi_stress_xc(dftk_mi_basis* basis, int64_t n, int n_spin, const double* rho_d, const double* vrho_d,
                      const double* e_d, const double* vsigma_d, const double* grad_d, double* out_h);

/* ---- local-potential pipeline of energy_hamiltonian (src/terms/Hamiltonian.jl:200-227) on the cube ----------
 * Hartree (src/terms/hartree.jl:50-59: V_H = irfft(green .* fft(rho)), E_H = 1/2 Re<V_H(G), rho(G)>), LDA exchange-
 * correlation (src/terms/xc.jl:84-160 with lda_x / lda_c_vwn / lda_c_pw, the functionals of `LDA()` and of the
 * reference's pinned tests), the local pseudopotential energy (src/terms/local.jl:15-16) and the summation into ONE
 * potential (src/terms/operators.jl:213-222):  V_out = V_loc + V_H + v_xc.
 * cube_kb: a k-block whose mapping is 0 .. N-1 (the library's cube FFT).  rho_d, V_loc_d, poisson_green_d
 * (4 pi / |G|^2 with the G = 0 and unpaired-G entries zeroed, hartree.jl:29-45), V_out_d: real cubes on the device;
 * V_loc_d / poisson_green_d / V_out_d may be NULL (term absent / energies only).  energies_h[3] = Hartree, Xc,
 * AtomicLocal (host); the call then synchronises the basis' stream.  energies_h may be NULL when V_out_d is not (the
 * Hamiltonian of an SCF step needs the potential only: no fetch, the call is asynchronous); the same holds for the
 * _collinear and _gga entries below. */
#define DFTK_MI_XC_LDA_X     1
#define DFTK_MI_XC_LDA_C_VWN 2
#define DFTK_MI_XC_LDA_C_PW  4
#define DFTK_MI_XC_LDA_XC_TETER93 32
int dftk_mi_local_potential(dftk_mi_kblock* cube_kb, const double* rho_d, const double* V_loc_d,
                            const double* poisson_green_d, int xc_functionals, double* V_out_d, double* energies_h);

/* Collinear spin (model.spin_polarization == :collinear, src/Model.jl:29-39): rho_d and V_out_d hold TWO cubes each,
 * (up, down) = rho[:, :, :, 1:2] of the reference.  V_out[s] = V_loc + V_H[rho_up + rho_down] + v_xc,s(rho_up, rho_down)
 * -- the potential of the k-blocks of spin s (ene_ops picks Vxc[:, :, :, kpt.spin], src/terms/xc.jl:163-175); the energies
 * are those of dftk_mi_local_potential with the total density in the Hartree and local terms.  Spin-polarised closed forms:
 * DFTK_MI_XC_LDA_X, DFTK_MI_XC_LDA_C_PW, DFTK_MI_XC_LDA_XC_TETER93 (anything else: DFTK_MI_EINVAL, nothing written).
 * Density floor: each channel enters the closed forms as max(rho_s, 1e-20) (zero and negative channels included), v_xc,s is
 * the derivative with respect to that clamped variable, and a point with rho_up + rho_down <= 2e-20 contributes e_xc = 0,
 * v_xc,up = v_xc,down = 0.  The unpolarised DFTK_MI_XC_LDA_XC_TETER93 of dftk_mi_local_potential is this form at
 * rho_up = rho_down = rho / 2 and so is zero for rho <= 2e-20; the other unpolarised forms are evaluated for rho > 1e-300. */
int dftk_mi_local_potential_collinear(dftk_mi_kblock* cube_kb, const double* rho_d, const double* V_loc_d,
                                      const double* poisson_green_d, int xc_functionals, double* V_out_d,
                                      double* energies_h);

/* The same pipeline with GGA functionals (PBE() = gga_x_pbe + gga_c_pbe, DFTK_MI_XC_GGA_* bits, may be mixed with the
 * LDA bits): the density gradient and the divergence term of the potential (LibxcDensities src/terms/xc.jl:356-409,
 * xc_potential_real :140-150, divergence_real :576-584) are taken with i G multipliers between the library's cube FFTs,
 *   grad rho = irfft(i G_a fft(rho)),  v_xc = de/drho - 2 div(de/dsigma grad rho),  sigma = |grad rho|^2,
 * G cartesian from recip_lattice_h (3x3 column-major, Julia's model.recip_lattice; required with a GGA bit).  Points
 * with rho <= density_threshold contribute nothing to the GGA part.  Everything else as dftk_mi_local_potential. */
int dftk_mi_local_potential_gga(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, const double* rho_d,
                                const double* V_loc_d, const double* poisson_green_d, int xc_functionals,
                                double density_threshold, double* V_out_d, double* energies_h);

/* The same pipeline with meta-GGA functionals (SCAN: DFTK_MI_XC_MGGA_X_SCAN | DFTK_MI_XC_MGGA_C_SCAN, at least one of them; LDA
 * and GGA bits may be mixed in as above).  tau_d: the kinetic energy density (real cube), one more operand of the point-wise
 * pass; Vtau_out_d = de/dtau (real cube), one more output of it: the cube to bind with dftk_mi_kblocks_set_tau_potential.
 *   V_out = V_loc + V_H + de/drho - 2 div(de/dsigma grad rho)
 * No transform more than dftk_mi_local_potential_gga.  recip_lattice_h is required; Vtau_out_d is required with V_out_d;
 * unpolarised, no core correction.  Point-wise forms and threshold: dftk_mi_xc_mgga. */
int dftk_mi_local_potential_mgga(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, const double* rho_d,
                                 const double* tau_d, const double* V_loc_d, const double* poisson_green_d, int xc_functionals,
                                 double density_threshold, double* V_out_d, double* Vtau_out_d, double* energies_h);

/* Collinear spin with GGA functionals (PBE on a magnetic system, the reference's test/iron_pbe.jl): the semantics of
 * dftk_mi_local_potential_collinear (two cubes in rho_d and V_out_d, Hartree and V_loc on the total density, three
 * energies, energies_h == NULL: asynchronous) with the gradient terms of src/terms/xc.jl:120-137 for two spin components,
 *   grad rho_s = irfft(i G_a fft(rho_s)),  sigma_st = grad rho_s . grad rho_t,
 *   V_out[s] += de/drho_s - 2 div(de/dsigma_ss grad rho_s + 1/2 de/dsigma_ud grad rho_s'),   s' = the other channel,
 * G cartesian from recip_lattice_h (3x3 column-major; required with a GGA bit).  xc_functionals: the spin-polarised LDA
 * bits (LDA_X, LDA_C_PW, LDA_XC_TETER93) and DFTK_MI_XC_GGA_X_PBE, DFTK_MI_XC_GGA_C_PBE in any mix; anything else:
 * DFTK_MI_EINVAL, nothing written.  Without a GGA bit the call is dftk_mi_local_potential_collinear.  Floors of the GGA
 * part: see dftk_mi_xc_gga_spin. */
int dftk_mi_local_potential_collinear_gga(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, const double* rho_d,
                                          const double* V_loc_d, const double* poisson_green_d, int xc_functionals,
                                          double density_threshold, double* V_out_d, double* energies_h);

/* Non-linear core correction (src/terms/xc.jl:35-42, 94-97, 184-187): the four entries above in one, with the core density
 * of the pseudopotentials as one more operand.  n_spin = 1 or 2: rho_d / V_out_d hold that many cubes.  rho_core_d: ONE cube,
 * the TOTAL core density (atomic_total_density(basis, CoreDensity())); each channel sees rho_core / n_spin
 * (rho_from_total, src/densities.jl:158-175).  grad_core_d: three cubes (x, y, z), the gradient of the total core density as
 * dftk_mi_cube_gradient writes it; required with a GGA bit when rho_core_d is given, ignored otherwise.
 *   E_xc, v_xc: those of rho_s + rho_core / n_spin; gradients grad rho_s + grad rho_core / n_spin, sigma and the flux of
 *               the divergence term built from those sums; every floor and threshold applies to the summed argument
 *   Hartree, sum rho V_loc: rho alone
 * The core rides on passes that stream the cube anyway (the final sum, the point-wise GGA pass, the pass that writes the
 * gradients): no transform and no launch more than the entry of the same kind.  Masks and their refusals as that entry
 * (n_spin = 1: LDA bits and TETER93 without a GGA bit, bits 1 .. 16 with one; n_spin = 2: as _collinear_gga);
 * recip_lattice_h (3x3 column-major) is required with a GGA bit; V_loc_d / poisson_green_d / V_out_d may be NULL and
 * energies_h == NULL means asynchronous, as above.  With rho_core_d == NULL the results are bit for bit those of the
 * existing entry.  DFTK_MI_EINVAL, nothing written: n_spin outside {1, 2}, a mask outside the above, a GGA bit with a core
 * but without grad_core_d, a k-block that does not span the cube. */
int dftk_mi_local_potential_core(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_spin, const double* rho_d,
                                 const double* rho_core_d, const double* grad_core_d, const double* V_loc_d,
                                 const double* poisson_green_d, int xc_functionals, double density_threshold,
                                 double* V_out_d, double* energies_h);
/* grad_d[a] = Re irfft(i G_a fft(f_d)), a = x, y, z (three real cubes, one after the other; G cartesian from
 * recip_lattice_h, 3x3 column-major): exactly the operator chain the GGA pipelines apply to the density, so that
 * grad(rho + rho_core) and grad rho + grad rho_core agree to rounding.  Set-up entry, asynchronous on the basis' stream. */
int dftk_mi_cube_gradient(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, const double* f_d, double* grad_d);

/* ---- density-sized operations of the SCF glue ----------------------------------------------
 * symmetrize_rho(basis, rho; symmetries, do_lowpass) for one spin component (src/symmetry.jl:346-357): fft, then
 * accumulate_over_symmetries! (:282-319: out(G) = sum_s e^{-2 pi i G.tau_s} in(S_s^-1 G), terms whose S_s^-1 G leaves
 * the grid dropped) and lowpass_for_symmetry! (:323-343) as ONE kernel over G, / n_sym, irfft.  S_h: n_sym 3x3 integer
 * matrices, column-major (Julia's symop.S = W'); tau_h: 3 doubles each (symop.tau = -W^-1 w).  rho_out_d may alias
 * rho_in_d.  With identity-only symmetries the density is copied (all(isone, symmetries), :292-295).  Any n_sym >= 1: up to
 * 192 operations are one kernel; a larger group (supercells: 384 for 2x2x2 primitive Si) goes through in chunks of 192
 * between the same two FFTs, accumulating first and low-passing once every chunk is in.  DFTK_MI_EINVAL, nothing written:
 * n_sym < 1, a matrix with det S != +-1, a k-block that does not span the cube. */
int dftk_mi_symmetrize_rho(dftk_mi_kblock* cube_kb, int n_sym, const int32_t* S_h, const double* tau_h, int do_lowpass,
                           const double* rho_in_d, double* rho_out_d);
/* mix_density(::KerkerMixing, basis, dF) (src/scf/mixing.jl:61-72, spin-unpolarised):
 *   d_rho = irfft(enforce_real!(G^2 / (kTF^2 + G^2) fft(dF))),  d_rho .+= mean(dF) - mean(d_rho)
 * (the last line = the G = 0 coefficient of dF kept as it is).  Multiplier evaluated on the fly from the integer G of
 * each cube entry and recip_lattice_h (column-major). */
int dftk_mi_mix_kerker(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, double kTF, const double* dF_d,
                       double* drho_d);
/* mix_density(::DielectricMixing, ...) (mixing.jl:161-171): multiplier (kTF^2 - C0 G^2) / (eps_r kTF^2 - C0 G^2),
 * C0 = 1 - eps_r, DC component kept.  (eps_r = 1 and eps_r > 1/sqrt(eps) are the caller's special cases, :163-164.) */
int dftk_mi_mix_dielectric(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, double kTF, double eps_r,
                           const double* dF_d, double* drho_d);
/* apply!(d_rho, ::DielectricModel, dV) kernel part (src/scf/chi0models.jl:66-77, identity localisation):
 *   out = irfft(C0 kTF^2 G^2 / (4 pi (kTF^2 - C0 G^2)) fft(dV)) */
int dftk_mi_chi0_dielectric_apply(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, double kTF, double eps_r,
                                  const double* dV_d, double* out_d);
/* out = irfft(multiplier .* fft(f)) with a real multiplier cube on the device, e.g. apply_kernel(::TermHartree, ...)
 * with the Poisson Green's function (src/terms/hartree.jl:68-81) inside the chi0-mixing GMRES (mixing.jl:255-275). */
int dftk_mi_cube_fourier_filter(dftk_mi_kblock* cube_kb, const double* multiplier_d, const double* f_d, double* out_d);

/* GGA exchange-correlation point by point (the libxc call of src/terms/xc.jl:111 for PBE(): gga_x_pbe + gga_c_pbe):
 * e_d = energy density per volume, vrho_d = de/drho, vsigma_d = de/dsigma (sigma = |grad rho|^2) for n grid points;
 * derivatives by forward-mode differentiation of the closed forms on the device.  Points with rho <= density_threshold
 * give zeros.  The gradient / divergence of xc.jl:356-409,576-584 stay with the caller (cube FFTs). */
#define DFTK_MI_XC_GGA_X_PBE 8
#define DFTK_MI_XC_GGA_C_PBE 16
int dftk_mi_xc_gga(dftk_mi_basis* basis, int64_t n, const double* rho_d, const double* sigma_d, int xc_functionals,
                   double density_threshold, double* e_d, double* vrho_d, double* vsigma_d);

/* The same for two spin components (libxc's polarised gga_x_pbe / gga_c_pbe).  Planar arrays of n values per component:
 * rho_d = (up, down), sigma_d = (uu, ud, dd) with sigma_st = grad rho_s . grad rho_t, e_d = energy density per volume,
 * vrho_d = (de/drho_up, de/drho_down), vsigma_d = (de/dsigma_uu, de/dsigma_ud, de/dsigma_dd) -- the reference's packed
 * order (DftFunctionals.spinindex_sigma).  Each channel enters as max(rho_s, 1e-20) and the derivatives are those of the
 * clamped variables; a point with rho_up + rho_down <= max(density_threshold, 2e-20) gives zeros in all six outputs;
 * sigma_uu, sigma_dd and sigma_uu + 2 sigma_ud + sigma_dd enter as max(., 0). */
int dftk_mi_xc_gga_spin(dftk_mi_basis* basis, int64_t n, const double* rho_d, const double* sigma_d, int xc_functionals,
                        double density_threshold, double* e_d, double* vrho_d, double* vsigma_d);

/* Meta-GGA exchange-correlation point by point (SCAN: libxc's unpolarised mgga_x_scan / mgga_c_scan; Sun, Ruzsinszky, Perdew,
 * PRL 115, 036402 (2015)): e_d = energy density per volume, vrho_d = de/drho, vsigma_d = de/dsigma, vtau_d = de/dtau for n grid
 * points, tau_d = 1/2 sum_n f_n |grad psi_n|^2 the kinetic energy density; derivatives by forward-mode differentiation of the
 * closed forms on the device.  alpha = (tau - sigma / (8 rho)) / tau_unif is not clamped (sigma may exceed 8 rho tau).  Points
 * with rho <= density_threshold give zeros in all four outputs.  xc_functionals: DFTK_MI_XC_MGGA_X_SCAN, DFTK_MI_XC_MGGA_C_SCAN or
 * both; anything else: DFTK_MI_EINVAL, nothing written.  No other entry point accepts these two bits. */
#define DFTK_MI_XC_MGGA_X_SCAN 64
#define DFTK_MI_XC_MGGA_C_SCAN 128
int dftk_mi_xc_mgga(dftk_mi_basis* basis, int64_t n, const double* rho_d, const double* sigma_d, const double* tau_d,
                    int xc_functionals, double density_threshold, double* e_d, double* vrho_d, double* vsigma_d,
                    double* vtau_d);

/* ---- sphere <-> cube transforms  (src/fft.jl:110-122 ifft!, :162-172 fft!; normalize=false) --
 * cube_d is nx*ny*nz complex, x fastest.  Test/diagnostic entry points (the hot path never
 * materialises the full cube in the caller's layout). */
int dftk_mi_ifft_sphere(dftk_mi_kblock* kb, const dftk_mi_cplx* c_d, dftk_mi_cplx* cube_d);
int dftk_mi_fft_sphere(dftk_mi_kblock* kb, const dftk_mi_cplx* cube_d, dftk_mi_cplx* c_d);

/* ---- compute_density inner loop (src/densities.jl:35-43) -------------------------------------
 * rho_d[nx*ny*nz] += sum_n weight_h[n] * |BFFT(pad(psi[:,n]))|^2, weight_h[n] =
 * occupation[n] * kweight * ifft_normalization^2 (bands with weight 0 are skipped). */
int dftk_mi_density_accumulate(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d,
                               int64_t ld_psi, const double* weight_h, double* rho_d);

/* compute_kinetic_energy_density inner loop (src/densities.jl:110-125):
 * tau_d[nx*ny*nz] += sum_n weight_h[n] / 2 * sum_a |BFFT(pad((G + k)_a psi[:,n]))|^2, a = x, y, z cartesian, weights as above.
 * Three transforms per band through the density stages.  Needs dftk_mi_kblock_set_kpoint; un-sharded blocks of complex
 * orbitals outside a batched call only (anything else: DFTK_MI_EINVAL with a message, nothing written). */
int dftk_mi_kinetic_energy_density_accumulate(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d,
                                              int64_t ld_psi, const double* weight_h, double* tau_d);

/* The same with the spin index of the k-block spelled out: rho_d holds n_spin cubes (n_spin = 1 or 2,
 * model.n_spin_components), the bands of this block are added to cube `spin` (0-based: kpt.spin - 1) --
 * `rho[:, :, :, kpt.spin] .+= ...` of src/densities.jl:39; a collinear basis lists all spin-up k-blocks, then all
 * spin-down ones (src/PlaneWaveBasis.jl:50-53, build_kpoints src/Kpoint.jl:58-74). */
int dftk_mi_density_accumulate_spin(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                    const double* weight_h, double* rho_d, int spin, int n_spin);

/* ---- density response (src/response/chi0.jl, src/response/cg.jl, compute_drho of src/densities.jl:60-108; q = 0) --------
 * sternheimer_solver (chi0.jl:115-232) for ONE k-block in one call: solves
 *     Q (H - eps_n) Q dpsi_n = -Q rhs_n,   Q = 1 - psi_occ psi_occ',   n = 0 .. n_occ - 1
 * by the reference's Schur split over the extra bands and its preconditioned block CG (cg.jl:30-128; projections after
 * every update, TPA preconditioner with the mean kinetic energy of the FIRST occupied column, locking of converged columns
 * on a contiguous active range; n_iter counts as the reference does).  psi_occ: n_occ orthonormal columns with
 * psi_occ' H psi_occ = diag(eps_h); psi_extra: n_extra >= 0 further columns, orthonormal to them and Rayleigh-Ritz among
 * themselves (H psi_extra and eps_extra are computed here); rhs: n_occ columns; tol_h[n_occ]: residual-norm tolerance of
 * every column; dpsi0_d (nullable): start vector.  Outputs: dpsi_d (n_G x n_occ), *n_iter, resid_h[n_occ] (norms of the CG
 * residual), *converged.  n_occ = 0 returns at once.  The H of the block's bound potential is applied in the general complex
 * full-sphere layout (a Gamma-real block included).  ONE host synchronisation per CG iteration (the fetch of the residual
 * norms); alpha and beta of the CG stay on the device.  Workspace: (8 n_occ + 2 n_extra) n_G complex numbers of the
 * basis' response workspace; the k-block's LOBPCG state (kept A X, start buffers) is not touched.  A plane-wave sharded
 * block is refused (DFTK_MI_EINVAL). */
int dftk_mi_sternheimer(dftk_mi_kblock* kb, int n_occ, const dftk_mi_cplx* psi_occ_d, int64_t ld_occ, const double* eps_h,
                        int n_extra, const dftk_mi_cplx* psi_extra_d, int64_t ld_extra, const dftk_mi_cplx* rhs_d,
                        int64_t ld_rhs, const double* tol_h, int miniter, int maxiter, const dftk_mi_cplx* dpsi0_d,
                        int64_t ld_dpsi0, dftk_mi_cplx* dpsi_d, int64_t ld_dpsi, int* n_iter, double* resid_h,
                        int* converged);
/* compute_drho's inner loop (densities.jl:86-103) for one k-block:
 *     drho_d[nx*ny*nz] += sum_n 2 w_occ_h[n] Re(conj(psi_n(r)) dpsi_n(r)) + w_docc_h[n] |psi_n(r)|^2
 * with psi_n(r) = BFFT(pad(psi[:, n])) unnormalised: the caller folds kweight * ifft_normalization^2 into both weights
 * (w_occ = occupation * ..., w_docc = d occupation * ...).  Two pruned inverse transforms per band, the product and the
 * accumulation in the last pass; bands with both weights 0 are skipped.  Unsharded blocks only. */
int dftk_mi_density_response_accumulate(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                        const dftk_mi_cplx* dpsi_d, int64_t ld_dpsi, const double* w_occ_h,
                                        const double* w_docc_h, double* drho_d);
/* apply_kernel of TermHartree + TermXc (hartree.jl:68-81, xc.jl:245-330; spin-unpolarised LDA) on the cube:
 *     dV = irfft(poisson_green .* fft(drho)) + f_xc(rho) drho,   f_xc = d^2 (rho eps_xc) / d rho^2
 * in closed form for DFTK_MI_XC_LDA_X, _LDA_C_VWN, _LDA_C_PW (other bits: DFTK_MI_EINVAL).  poisson_green_d NULL: no Hartree
 * part; xc_functionals 0: no XC part (RPA; rho_d may then be NULL).  Asynchronous on the basis' stream. */
int dftk_mi_apply_kernel(dftk_mi_kblock* cube_kb, const double* rho_d, const double* drho_d, const double* poisson_green_d,
                         int xc_functionals, double* dV_d);

/* ---- transfer between two bases of the same lattice (src/transfer.jl) ----------------------------------------------------
 * transfer_blochwave_kpt (transfer.jl:46-124) for all bands of one k-block in ONE launch.  kb_in and kb_out are k-blocks of
 * the same lattice whose k-points differ by the integer vector dG_h[3] = k_out - k_in (0 0 0 for the same k-point); they may
 * belong to two different basis handles (other Ecut, other FFT grid) of the same device.  in_d: n_G(kb_in) x n_bands,
 * out_d: n_G(kb_out) x n_bands, both in the caller's full-sphere complex layout (a Gamma-real block included); they must
 * not overlap.  Row r of the output, carrying the plane wave G, receives the input row that carries G + dG; if G + dG lies
 * outside the input cube or outside the input sphere the row is set to zero, and input rows whose plane wave the output
 * sphere lacks are dropped -- the same rule small -> large and large -> small.  A gather over the output rows through the
 * input block's inverse cube -> row map (built at the first call that reads from the block, kept with it): every entry
 * of the n_G(kb_out) x n_bands output is written exactly once, rows from n_G(kb_out) to ld_out are not touched, no atomics,
 * results are bit-for-bit reproducible and equal to the moved numbers.
 * Streams: the kernel runs on the stream of kb_out's basis after a device-side wait for the work queued on the stream of
 * kb_in's basis, and that stream in turn waits for the kernel; the host does not block (one handle on both sides: one
 * stream, no event).
 * DFTK_MI_EINVAL, outputs untouched: n_bands < 0, a leading dimension below the rows of its sphere, blocks on different
 * devices, a plane-wave sharded block, or a dG that does not fit the blocks -- where both blocks were created with kinetic
 * energies, partners must carry the same |k + G|^2 / 2 (a host pass over the output rows, made once per input block
 * and dG and remembered on the output block). */
int dftk_mi_transfer_blochwave(dftk_mi_kblock* kb_in, dftk_mi_kblock* kb_out, const int* dG_h /* [3] */, int n_bands,
                               const dftk_mi_cplx* in_d, int64_t ld_in, dftk_mi_cplx* out_d, int64_t ld_out);
/* transfer_density (transfer.jl:165-178): rho_out = irfft(basis_out, T fft(basis_in, rho_in)) for n_spin (1 or 2) real cubes
 * stored one after the other.  cube_kb_in / cube_kb_out: full-cube k-blocks (n_G = nx ny nz, identity mapping) of the two
 * bases.  T copies the eight index blocks of transfer_mapping (transfer.jl:10-31) and zeroes the rest: per axis, indices
 * of equal signed frequency correspond over the frequency range of the shorter axis -- the unmatched frequency -n/2 of an
 * even shorter axis is carried to -n/2 of the longer one, whose +n/2 stays zero, so small -> large -> small is not the
 * identity on such a grid (transfer.jl:158-163).  The inverse transform is the library's complex cube transform followed
 * by the real part (as everywhere in this library), where the reference's half-spectrum transform reads the x >= 0
 * half only: the two differ in the contribution of that unmatched plane along x alone, which the density of orbitals
 * on a sphere inside the grid does not populate.  Normalisation: 1 / N_in overall; the integral of the density is preserved
 * small -> large.  Streams: as above (forward transform on the input basis' stream, the rest on the output basis').
 * Asynchronous. */
int dftk_mi_transfer_density(dftk_mi_kblock* cube_kb_in, dftk_mi_kblock* cube_kb_out, int n_spin, const double* rho_in_d,
                             double* rho_out_d);

/* ---- symmetry operations on orbitals and the Wannier90 interface (src/symmetry.jl:229-270, src/external/wannier_shared.jl)
 * apply_symop (symmetry.jl:229-270) for all bands of one k-block in ONE launch:
 *   out(G) = e^{-2 pi i (G + kshift).tau} in(S^-1 (G + kshift))     for every plane wave G of kb_out,
 * kb_in the block of k, kb_out the block of S k reduced to [-0.5, 0.5)^3 by the integer vector kshift_h[3] = reduced - raw.
 * invS_h: the 3x3 integer matrix S^-1, column-major (as S_h of dftk_mi_symmetrize_rho); tau_h: symop.tau.  in_d: n_G(kb_in)
 * x n_bands, out_d: n_G(kb_out) x n_bands, both in the caller's full-sphere complex layout (a Gamma-real block included);
 * they must not overlap.  A gather over the output rows through the input block's inverse cube -> row map (the one
 * dftk_mi_transfer_blochwave keeps): the phase is computed once per row, every entry of the output is written exactly once,
 * rows from n_G(kb_out) to ld_out are not touched, no atomics, results repeat bit for bit; with tau = 0 the numbers are
 * moved, not multiplied.  Streams: as dftk_mi_transfer_blochwave.
 * DFTK_MI_EINVAL, outputs untouched: n_bands < 0, a leading dimension below the rows of its sphere, blocks on different
 * devices, a plane-wave sharded block, det S^-1 != +-1, or an output row whose pre-image lies outside the input cube or
 * sphere -- the operation is then not a symmetry of this discretisation (the reference asserts); a host pass over the output
 * rows, made once per (input block, S^-1, kshift) and remembered on the output block. */
int dftk_mi_apply_symop(dftk_mi_kblock* kb_in, dftk_mi_kblock* kb_out, const int* invS_h /* [9] */,
                        const int* kshift_h /* [3] */, const double* tau_h /* [3] */, int n_bands, const dftk_mi_cplx* in_d,
                        int64_t ld_in, dftk_mi_cplx* out_d, int64_t ld_out);
/* overlap_Mmn_k_kpb (wannier_shared.jl:220-241) of one k-point with all n_nb neighbours:
 *   M_d[m + n_bands (j n_bands + n)] = sum_G conj(psi(G, m)) psi_nb_j(G + dG_j, n),   m, n < n_bands, j < n_nb,
 * the sum over the plane waves G of kb whose partner G + dG_j (dG_h[3 j ..]: the file's G_shift) is a plane wave of
 * kb_nb_h[j]; a neighbour that shares none gives a zero matrix (the identity of the reference is the caller's rule).
 * psi_d: n_G(kb) x n_bands with leading dimension ld; psi_nb_h[j] / ld_nb_h[j]: device block and leading dimension of
 * neighbour j (host arrays of n_nb entries, read before the call returns; a block may be its own neighbour and appear
 * several times).  The neighbours may belong to other basis handles of the same device: this basis' stream waits for
 * theirs and theirs for the kernels (device-side, as dftk_mi_transfer_blochwave).  The partner look-up and the product are
 * one kernel: one launch per 16 neighbours whatever n_bands, no workspace, no host synchronisation; the summation order is
 * fixed, results repeat bit for bit.  Sized for the band counts of a Wannierisation (n_bands of tens at most): a workgroup
 * owns a 4 x 4 tile of one neighbour's matrix and reads both orbital blocks in full, so the blocks are read
 * ceil(n_bands / 4) times each -- once for 4 bands, 9 times for 33; no crossover against a gathered panel and one zgemm has
 * been measured, and hundreds of bands are not what this entry is for.  Asynchronous.  DFTK_MI_EINVAL, M_d untouched:
 * negative counts, a short leading
 * dimension, a null block, a sharded block or another device. */
int dftk_mi_wannier_overlaps(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld, int n_nb,
                             dftk_mi_kblock* const* kb_nb_h, const int* dG_h /* [3 n_nb] */,
                             const dftk_mi_cplx* const* psi_nb_h, const int64_t* ld_nb_h, dftk_mi_cplx* M_d);
/* The guess orbitals of compute_amn_kpoint (wannier_shared.jl:13-22, :38-71, :278-298) at p = k + G for every plane wave of
 * kb, n_cols columns in one launch per 32 columns.  recip_lattice_h: 3x3 column-major; kcoord_h[3]: the k-point, reduced;
 * centers_h[3 c ..]: the centre of column c, reduced.  kind_h[c] = 0: the Gaussian exp(2 pi (-i p.c - |p_cart|^2 / 4));
 * kind_h[c] = 1: e^{-2 pi i p.c} (-i)^l R_lm(p_cart) T_c(|p_cart|) / 4 pi with (l, m) = lm_h[2 c], lm_h[2 c + 1] (l <= 3,
 * R_lm = |p|^l Y_lm the real solid harmonic in the reference's ylm_real convention) and T_c = R_d[chan_h[c] * ldR + row],
 * the kind-0 dftk_mi_radial_transform of the radial function at |p_cart| of every row (n_chan rows of ldR >= n_G values):
 * the reference's sum_r w f j_l(|p| r) is T |p|^l / 4 pi; an exact zero at p = 0 for l > 0.  normalize != 0: every column
 * is divided by its 2-norm (wannier_shared.jl:291).  Asynchronous.  DFTK_MI_EINVAL, out_d untouched: a kind outside
 * {0, 1}, (l, m) or a channel out of range, a short leading dimension, a sharded block. */
int dftk_mi_wannier_guess_columns(dftk_mi_kblock* kb, const double* recip_lattice_h, const double* kcoord_h, int n_cols,
                                  const int* kind_h, const int* lm_h, const int* chan_h, const double* centers_h, int n_chan,
                                  const double* R_d, int64_t ldR, int normalize, dftk_mi_cplx* out_d, int64_t ld_out);

/* ---- refinement metric (src/postprocess/refine.jl:20-84) -----------------------------------------------------------------
 * invert_refinement_metric for ONE k-block, all columns in one call: solves
 *     M_c x_c = P res_c,   M_c = P T_c^{1/2} P T_c^{1/2} P,   T_c = kinetic + mean_kin[c],   P = 1 - psi psi',   c = 0 .. n - 1
 * with mean_kin[c] = sum_G kinetic_G |psi_Gc|^2 (precondprep!, computed here on the device), by conjugate gradients from
 * x = 0 preconditioned with P T_c^{-1} P, until ||r_c|| <= tol (the reference: 100 eps) or maxiter passes (the reference:
 * 20), and projects the result once more: psi' x = 0.  psi_d: n orthonormal columns; res_d: n columns (their components along
 * psi are projected out); out_d: n_G x n.  Every column has its own alpha and beta and is frozen bit for bit once it has
 * converged; iters_h[c] is the reference's n_iter of column c (the pass in which its residual norm was first seen at or
 * below tol; 1 = at the start), or the number of passes made if it never was, and resnorm_h[c] its last residual norm -- a
 * column that did not converge is REPORTED (resnorm_h[c] > tol), the call still returns 0.  Projections are zgemm calls,
 * the scalings one launch for all columns; ONE host synchronisation per CG pass (the fetch of the residual norms).
 * Workspace: 5 n_G n complex numbers of the basis' response workspace.  Unsharded blocks only, not inside a batched
 * multi-k call (DFTK_MI_EINVAL). */
int dftk_mi_refinement_metric_solve(dftk_mi_kblock* kb, int n, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                    const dftk_mi_cplx* res_d, int64_t ld_res, double tol, int maxiter, dftk_mi_cplx* out_d,
                                    int64_t ld_out, int* iters_h, double* resnorm_h);

/* ---- exact exchange at the Gamma point (src/terms/exact_exchange.jl, ExchangeOperator of src/terms/operators.jl:184-210) --
 * The Fock operator built from n_occ orbitals phi (n_G x n_occ) applied to n_bands columns psi:
 *     W_m (+)= - sum_n weight_h[n] FFT[ phi_n(r) IFFT[ K(G) FFT[ conj(phi_n(r)) psi_m(r) ] ] ]
 * in the reference's normalisations (phi_n(r) = ifft(basis, kpt, phi_n), fft / ifft of the k-point: the pair density is
 * taken on the k-block's own sphere).  weight_h[n] = occupation_n / filled_occupation; orbitals with weight 0 are skipped.
 * kernel_d: n_G reals on the block's sphere = scaling_factor * compute_kernel_fourier (src/coulomb.jl).  accumulate = 0
 * overwrites W, otherwise W += ...; rows beyond n_G of a column (ld > n_G) are neither read nor written.  n_bands = 0 does
 * nothing; n_occ = 0 (or all weights 0) zero-fills W when accumulate = 0.  Asynchronous on the basis' stream.
 * Cost: 2 pruned transforms per (orbital, column) pair.  Workspace (the basis' exchange workspace, released with the basis),
 * in complex numbers with N = nx ny nz, g = the FFT launch group, g_phi = min(g, n_occ), g_psi = min(g, n_bands):
 *     (c + 2 g_psi + g_phi) N + (2 g_phi + g_psi) n_G,   c = n_occ while n_occ N 16 B <= 8 GiB (the orbitals' cubes are then
 * transformed once per call), else g_phi (they are transformed again for every group of columns).
 * Refused with DFTK_MI_EINVAL: Gamma-real blocks, plane-wave sharded blocks, null pointers, leading dimensions below n_G.
 * (The library's own batched multi-k drivers never call it: a guard inside refuses that too, unreachable through this ABI.) */
int dftk_mi_exx_apply(dftk_mi_kblock* kb, int n_occ, const dftk_mi_cplx* phi_d, int64_t ld_phi, const double* weight_h,
                      const double* kernel_d, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi, dftk_mi_cplx* W_d,
                      int64_t ld_W, int accumulate);

/* ---- lobpcg_hyper(A, X0; prec=PreconditionerTPA, tol, miniter, maxiter, n_conv_check)
 *      (src/eigen/diag_lobpcg_hyper.jl:5-18 -> LOBPCG, src/eigen/lobpcg_hyper_impl.jl:354-582;
 *       PreconditionerTPA src/eigen/preconditioners.jl:27-78) ----------------------------------
 * X_d: in = guess (need not be orthonormal), out = Ritz vectors (orthonormal), n_G x M.
 * use_tpa: 1 = TPA preconditioner from the block's kinetic vector, 0 = none.
 * n_conv_check <= 0 means M.  seed drives the (rare) re-randomisation of null columns.
 * Outputs (host): lambda_h[M] ascending, resid_h[M] final residual norms, *n_iter, *converged,
 * *n_matvec (the "H psi applies" counter, lobpcg_hyper_impl.jl:377,417). */
int dftk_mi_lobpcg(dftk_mi_kblock* kb, int M, dftk_mi_cplx* X_d, int64_t ldX, double tol,
                   int miniter, int maxiter, int n_conv_check, int use_tpa, uint64_t seed,
                   double* lambda_h, double* resid_h, int* n_iter, int* converged,
                   int64_t* n_matvec);
/* Residual-norm history of the last dftk_mi_lobpcg call on this block (`resid_history` of
 * lobpcg_hyper_impl.jl:368,443-446, rows ordered like the returned eigenpairs): hist_h[i + M * it] for
 * it = 0 .. n_iter; cap = capacity of hist_h in doubles (hist_h may be NULL to query the sizes).
 * *n_svd = how many times ortho! took its SVD fallback (:226-231, :307-314) during the call. */
/* The loop over k-points of diagonalize_all_kblocks (src/eigen/diag.jl:24-48) in ONE call, for workloads of many small
 * k-blocks (k-point meshes of small cells: n_G ~ 1e3, a handful of bands -- launch-latency bound one at a time).  Every
 * k-block runs exactly the iteration of dftk_mi_lobpcg, but in lock-step with its siblings: device operations of the
 * same kind are merged into one launch over all k-blocks (batched small GEMMs / Cholesky / Jacobi kernels, one FFT
 * pipeline over the bands of all k-points), and the host waits once per round instead of once per k-block and
 * operation.  All k-blocks must belong to ONE basis handle.  Arrays of n_kblocks entries; lambda_h / resid_h hold M
 * values per k-block; status[i] = what dftk_mi_lobpcg would have returned for k-block i.  Same eigenpairs as n_kblocks
 * separate calls up to the round-off of the different summation orders. */
int dftk_mi_lobpcg_multi(int n_kblocks, dftk_mi_kblock* const* kbs, int M, dftk_mi_cplx* const* X_d, const int64_t* ldX,
                         double tol, int miniter, int maxiter, int n_conv_check, int use_tpa, const uint64_t* seeds,
                         double* lambda_h, double* resid_h, int* n_iter, int* converged, int64_t* n_matvec, int* status);
/* compute_density's loop over k-points (src/densities.jl:35-43) in ONE call: rho_d += sum_k sum_n weight[k][n]
 * |ifft(psi_k[:, n])|^2 with all bands of all k-blocks in one pipeline (bands of zero weight never enter it).
 * weights_h: the per-band weights (occupation * kweight * ifft_normalization^2) of k-block 0, then of k-block 1, ...
 * One basis handle, unsharded k-blocks.  Asynchronous like dftk_mi_density_accumulate up to the final round. */
int dftk_mi_density_accumulate_multi(int n_kblocks, dftk_mi_kblock* const* kbs, const int* n_bands,
                                     const dftk_mi_cplx* const* psi_d, const int64_t* ld_psi, const double* weights_h,
                                     double* rho_d);
/* The same with a SECOND weight set and a second cube accumulated in the same pass: rho2_d += sum_k sum_n weights2[k][n]
 * |ifft psi_kn|^2 -- compute_density and compute_ldos (src/postprocess/dos.jl:43-62: "compute_density with modified weights")
 * of an SCF step with LdosMixing transform every band once instead of twice.  weights2_h / rho2_d both NULL = the call above. */
int dftk_mi_density_accumulate_multi2(int n_kblocks, dftk_mi_kblock* const* kbs, const int* n_bands,
                                      const dftk_mi_cplx* const* psi_d, const int64_t* ld_psi, const double* weights_h,
                                      double* rho_d, const double* weights2_h, double* rho2_d);
/* Kinetic energy of every band of n k-blocks in one call: out_h = sum_G kin_G |psi_Gn|^2 for the bands of k-block 0,
 * then of k-block 1, ... (the band terms of the Kinetic energy, src/terms/kinetic.jl:49-54).  One basis handle. */
int dftk_mi_band_kinetic_multi(int n_kblocks, dftk_mi_kblock* const* kbs, const int* n_bands,
                               const dftk_mi_cplx* const* psi_d, const int64_t* ld_psi, double* out_h);
/* Counters of the calling thread's last batched call: scheduling rounds (= host synchronisations), recorded
 * operations, merged launches, operations that ran one by one (no batched form). */
int dftk_mi_batch_stats(int64_t* rounds, int64_t* ops, int64_t* merged_launches, int64_t* sequential_ops);
/* Small k-blocks (M <= 8 bands, n_G * M <= 65536, neither sharded nor Gamma-real) run a driver with ONE host
 * synchronisation per LOBPCG iteration: ortho!(X) / ortho!(X, Y) are one kernel each, Ritz values and statuses travel
 * with the residual norms (lobpcg.cpp: lobpcg_run_small; src/eigen/lobpcg_hyper_impl.jl:354-582 unchanged as an
 * algorithm).  Rare branches it only detects (drop_small!, SVD fallbacks) restart the call on the general driver.
 * Process-wide counters: calls that took the small-block driver, and how many of them restarted.
 * DFTK_MI_LOBPCG_SMALL=0 switches the driver off. */
int dftk_mi_lobpcg_small_stats(int64_t* calls, int64_t* restarts);
/* The fused orthogonalisation kernel of that driver on a stand-alone block: ortho!(X, Y) for ny > 0 (X is normalised by
 * norms_d -- its column norms on the device -- or by norms computed here when NULL, projected against the orthonormal Y
 * and orthonormalised, lobpcg_hyper_impl.jl:271-323), plain ortho!(X) for ny = 0 (:216-261); m <= 8, ny <= 16.
 * res4_h = {status (0 done, 1 a host-side branch is needed: X unusable, 2 non-finite), rounds of the ortho!(X, Y) loop,
 * Cholesky factorisations of the last ortho!(X), growth factor}. */
int dftk_mi_ortho_small(dftk_mi_basis* basis, int64_t n, int m, dftk_mi_cplx* X_d, int64_t ldx, int ny, const dftk_mi_cplx* Y_d,
                        int64_t ldy, const double* norms_d, double tol, double* res4_h);
/* The general form of dftk_mi_ortho_small (tests): a TABLE of device operations issued by n_fibers fibers of one batched
 * call, exactly as the k-blocks of dftk_mi_lobpcg_multi issue theirs.  Fiber f issues the rows with fiber == f in table
 * order through the internal entry points the LOBPCG drivers call (which record inside a fiber), and ends with a
 * synchronisation; the recorded queues are merged position by position into the batched kernels.  Field use per type
 * (device pointers unless named host; every leading dimension >= the rows it strides over):
 *   ZGEMM    trans ('N' | 'C'), gm, gn, gk, alpha, A, lda, B, ldb, beta, C, ldc, flags (DFTK_MI_GEMM_*)
 *   COLRED   mode 0 column norms | 1 Re <A, B> | 2 sum_i W[i] |A[i]|^2 | 3 sum |A|^2 | 4 Im <A, B>; n rows, m columns, A, lda,
 *            (B, ldb,) (W,) C = m doubles out
 *   RESIDUAL n, m, A = AX, lda, B = X, ldb, W = lambda (m doubles), C = R, ldc, D = norms out, W2 = kin (n doubles) or NULL,
 *            E = sum kin |x|^2 out (with W2), F = <x, x> out or NULL; W3 != NULL: lambda[c] = W[c] / W3[c] (recorded directly:
 *            the small-block driver's form, which has no one-by-one twin)
 *   TPA      n, m, A = src, lda, C = dst, ldc, W = kin or NULL (plain copy), W2 = mean_kin or NULL (1 / (kin + s0)), D = norms out
 *   SCALE    n, m, C, ldc, W = m factors, flags = 1: divide        COPY  n, m, A, lda, C, ldc        GATHER  the same + W = m ints
 *   FILL0    C, bytes (not a multiple of 16: recorded directly)        SUBID  n rows, m columns, C, ldc, i0: C[i0 + a, a] -= 1 while i0 + a < n
 *   ADDDIAG  m, C, ldc, s0        HERMIT  m, C, ldc        CTRANS  m, A, lda, C, ldc (C = A^H)
 *   H2D      C = destination, host = source, bytes        D2H  A = source, host = destination, bytes; flags = 1: the fiber waits
 *   POTRF    m, C = A in / R out, ldc, D = inv(R), ldb, host = double[2] normests; status = 0 | DFTK_MI_NUM_CHOLESKY
 *   HEEV     m, C = A (destroyed), ldc, D = V, ldb, host = m eigenvalues; status = 0 | DFTK_MI_NUM_*; E != NULL: a device copy
 *            of the eigenvalues as well (recorded directly, no one-by-one twin)
 *   APPLYD   kb, m bands, A = X (n_p x m), C = Y = D X (recorded directly: internal to the batched apply_H)
 *   ORTHO    n, m <= 8, k = ny <= 16, C = X, ldc, A = Y, lda, W = norms or NULL, s0 = tol, host = double[4] as res4_h of
 *            dftk_mi_ortho_small; status = (int)host[0] (recorded directly, batched form only)
 * join_next: the fiber's next row (same type, independent of this one) shares this row's launch.  sync_after: the fiber
 * synchronises after this row, so later rows sit at earlier queue positions of a later round.  A malformed table returns
 * DFTK_MI_EINVAL before anything is launched.  dftk_mi_batch_stats describes the call afterwards. */
enum {
    DFTK_MI_BOP_ZGEMM = 0, DFTK_MI_BOP_COLRED = 1, DFTK_MI_BOP_RESIDUAL = 2, DFTK_MI_BOP_TPA = 3, DFTK_MI_BOP_SCALE = 4,
    DFTK_MI_BOP_COPY = 5, DFTK_MI_BOP_FILL0 = 6, DFTK_MI_BOP_SUBID = 7, DFTK_MI_BOP_GATHER = 8, DFTK_MI_BOP_ADDDIAG = 9,
    DFTK_MI_BOP_HERMIT = 10, DFTK_MI_BOP_CTRANS = 11, DFTK_MI_BOP_H2D = 12, DFTK_MI_BOP_D2H = 13, DFTK_MI_BOP_POTRF = 14,
    DFTK_MI_BOP_HEEV = 15, DFTK_MI_BOP_APPLYD = 18, DFTK_MI_BOP_ORTHO = 19
};
typedef struct dftk_mi_batch_op {
    int32_t type, fiber, trans, m, k, i0, mode, flags, join_next, sync_after;
    int32_t status;                  /* out */
    int32_t reserved;
    int64_t n, gm, gn, gk, lda, ldb, ldc;
    dftk_mi_cplx alpha, beta;
    double s0;
    const void *A, *B, *W, *W2, *W3;
    void *C, *D, *E, *F;
    dftk_mi_kblock* kb;
    void* host;
    uint64_t bytes;
} dftk_mi_batch_op;
int dftk_mi_batch_replay(dftk_mi_basis* basis, int n_fibers, int n_ops, dftk_mi_batch_op* ops);
int dftk_mi_lobpcg_history(dftk_mi_kblock* kb, int* M, int* n_iter, double* hist_h, size_t cap, int* n_svd);
/* One-shot promise for the NEXT dftk_mi_lobpcg call on this block: its X0 IS the X the last call returned (an SCF step
 * hands the orbitals of the previous step back; same number of bands).  The driver then starts from
 * A_new X = (A_old X) inv(R) + (V_new - V_old) X -- the kept A X of its last exit, the Cholesky factor of its own
 * `X = ortho!(copy(X))` and ONE local-only application of the potential difference -- instead of a full H X: the kinetic and
 * nonlocal parts of H do not change between SCF steps (src/scf/self_consistent_field.jl:80-129: only the density-dependent
 * potential does).  Silently ignored (full H X) when nothing is kept, shapes differ, the block is small / batched, or the
 * orthogonalisation needed more than one plain pass.  dftk_mi_kblock_set_projectors drops what is kept. */
int dftk_mi_kblock_reuse_AX(dftk_mi_kblock* kb, int on);
/* number of dftk_mi_lobpcg calls of this process that started from the kept A X (diagnostic / tests) */
int dftk_mi_ax_reuse_count(int64_t* calls);
/* src/densities.jl:39 (compute_density's loop over the bands) and src/scf/self_consistent_field.jl:80-129 (the next_density
 * / diagonalisation hand-over of one SCF step): the density pass transforms the orbitals the last dftk_mi_lobpcg call
 * returned to y-planes, and the kept-A X start of the next call would transform the same orbitals again.  On an un-sharded,
 * un-batched Gamma-real block, dftk_mi_density_accumulate_real over exactly the block the last call returned (pointer,
 * leading dimension, band count) keeps those planes, and a promised dftk_mi_kblock_reuse_AX start applies
 * (V_new - V_old) from them: A_new X = (A_old X_ret + (V_new - V_old) X_ret) inv(R).  Nothing to call: binding a new
 * potential keeps the planes; any other density call, any dftk_mi_lobpcg call, dftk_mi_kblock_set_projectors / _set_shard /
 * _set_gamma_real and a change of dftk_mi_basis_set_fft_batch drop them.  The buffer (one T2 slab per band pair) is allocated
 * on first use if the device has room for it twice over; otherwise the block declines and every call takes the path above.
 * Environment DFTK_MI_PLANES_REUSE=0 (read per call) switches it off.
 * calls = number of dftk_mi_lobpcg calls of this process that started from kept planes (diagnostic / tests) */
int dftk_mi_planes_reuse_count(int64_t* calls);

/* Optional: device pointer to H*X of the last dftk_mi_lobpcg call on this block (n_G x M,
 * leading dimension n_G; valid until the next lobpcg call on the block). */
const dftk_mi_cplx* dftk_mi_lobpcg_last_AX(dftk_mi_kblock* kb);

/* ---- column helpers of LOBPCG as stand-alone calls (results on the host) ------------------------
 * columnwise_norms / columnwise_dots (src/common/linalg.jl:2-15, GPU forms src/gpu/linalg.jl:17-27):
 * X, A, B are n x m column-major device blocks. */
int dftk_mi_columnwise_norms(dftk_mi_basis* basis, int64_t n, int m, const dftk_mi_cplx* X_d, int64_t ldx,
                             double* norms_h /* [m] */);
int dftk_mi_columnwise_dots(dftk_mi_basis* basis, int64_t n, int m, const dftk_mi_cplx* A_d, int64_t lda,
                            const dftk_mi_cplx* B_d, int64_t ldb, dftk_mi_cplx* dots_h /* [m]: dot(A[:,i], B[:,i]) */);
/* ortho_qr (src/common/ortho.jl:1-9) / ortho!(X) (lobpcg_hyper_impl.jl:216-261): orthonormalise the columns of X
 * in place by Cholesky-QR with the reference's shift-and-retry and SVD fallback (same column space as Householder
 * QR; Q differs from LAPACK's by a unitary diagonal).  force_svd = 1 takes the SVD branch (X = U V').  force_svd | 2 (while
 * DFTK_MI_LAND_IN_PLACE is on): the block is first moved to the routine's scratch copy and the passes start from there, as
 * the LOBPCG driver enters them -- an odd number of passes then ends in X without a copy back; same result bit for bit.
 * *n_chol = Cholesky factorizations used (100 after an SVD fallback, as the reference reports). */
int dftk_mi_ortho_qr(dftk_mi_basis* basis, int64_t n, int m, dftk_mi_cplx* X_d, int64_t ldx, int force_svd,
                     int* n_chol, int* used_svd);
/* PreconditionerTPA (src/eigen/preconditioners.jl:27-78; GPU forms src/gpu/linalg.jl:25-43) on the block's kinetic
 * vector: precondprep! -> mean_kin_h[m]; ldiv!(Y, P, R) with mean_kin_h (NULL = not prepared yet: the
 * 1 / (kin + default_shift) form). */
int dftk_mi_tpa_precondprep(dftk_mi_kblock* kb, int m, const dftk_mi_cplx* X_d, int64_t ldx, double* mean_kin_h);
int dftk_mi_tpa_ldiv(dftk_mi_kblock* kb, int m, const dftk_mi_cplx* R_d, int64_t ldr, const double* mean_kin_h,
                     double default_shift, dftk_mi_cplx* Y_d, int64_t ldy);
/* The fused residual pass of one LOBPCG iteration (lobpcg_hyper_impl.jl:441-449): R = AX - X diag(lambda),
 * norms_h = column norms of R, and from the same read of X: mean_kin_h (precondprep!) and xx_h = <x, x>
 * (normalisation check :533); mean_kin_h / xx_h may be NULL. */
int dftk_mi_block_residual(dftk_mi_kblock* kb, int m, const dftk_mi_cplx* AX_d, int64_t lda,
                           const dftk_mi_cplx* X_d, int64_t ldx, const double* lambda_h, dftk_mi_cplx* R_d,
                           int64_t ldr, double* norms_h, double* mean_kin_h, double* xx_h);

/* ---- dense helpers exposed for tests (the LOBPCG building blocks) ----------------------------
 * zgemm: C = alpha*op(A)*B + beta*C, op(A) = A ('N') or A^H ('C'); f64 MFMA, deterministic split-K. */
int dftk_mi_zgemm(dftk_mi_basis* basis, char transA, int64_t m, int64_t n, int64_t k,
                  dftk_mi_cplx alpha, const dftk_mi_cplx* A_d, int64_t lda,
                  const dftk_mi_cplx* B_d, int64_t ldb, dftk_mi_cplx beta,
                  dftk_mi_cplx* C_d, int64_t ldc);
/* Structured variants used by the LOBPCG driver (lobpcg_hyper_impl.jl:141-145 Gram matrices that are
 * hermitised afterwards, :216-261 X*inv(R)); flags (may be combined):
 *   DFTK_MI_GEMM_UPPER     only the tiles of C (128x32 for complex products, 128x64 with DFTK_MI_GEMM_REAL)
 *                          that intersect the upper triangle (i <= j) are computed and written, the rest of C is
 *                          left untouched;
 *   DFTK_MI_GEMM_B_UPPER   B is upper triangular (B[k][j] = 0 for k > j): the k loop stops at the diagonal.  'N' products
 *                          take the entries below the diagonal as zeros whatever the array holds (the call is the dense
 *                          call on triu(B), bit for bit); 'C' products read them inside the diagonal block of a tile
 *                          column and REQUIRE the zeros in the array;
 *   DFTK_MI_GEMM_REAL      the long operands are blocks of real-symmetric vectors in the half-sphere format of
 *                          dftk_mi_kblock_set_gamma_real, i.e. real matrices with two real rows per complex entry:
 *                          'C' computes Re(A^H B) (imaginary part stored as 0), 'N' computes A * Re(B); two real
 *                          matrix-core products per complex entry instead of three;
 *   DFTK_MI_GEMM_SYM_RESULT  'N' products whose result is known to be Hermitian (the Newton-Schulz step X p(X) of
 *                          dftk_mi_heev_lowest): only the tiles of C that hold an entry on or above the diagonal are
 *                          computed and written, the rest of C is left untouched and the caller mirrors the result.
 *                          With DFTK_MI_GEMM_REAL a row of A and C holds two consecutive REAL rows (2 i, 2 i + 1) of
 *                          a real symmetric matrix with 2 m (or 2 m - 1) rows, and the diagonal is counted in those;
 *                          refused with 'C'. */
#define DFTK_MI_GEMM_UPPER 1
#define DFTK_MI_GEMM_B_UPPER 2
#define DFTK_MI_GEMM_REAL 8
#define DFTK_MI_GEMM_SYM_RESULT 32
int dftk_mi_zgemm_ex(dftk_mi_basis* basis, char transA, int64_t m, int64_t n, int64_t k,
                     dftk_mi_cplx alpha, const dftk_mi_cplx* A_d, int64_t lda,
                     const dftk_mi_cplx* B_d, int64_t ldb, dftk_mi_cplx beta,
                     dftk_mi_cplx* C_d, int64_t ldc, int flags);
/* D = alpha * op(A) * B + beta * C with the result in a second array D of C's shape and leading dimension (D == C is
 * dftk_mi_zgemm_ex).  Same flags, same launch plan, same arithmetic in the same order: the result is bit for bit the one the
 * in-place call leaves in C.  C is read only where beta != 0 and never written; with DFTK_MI_GEMM_UPPER /
 * DFTK_MI_GEMM_SYM_RESULT only the computed tiles of D are written. */
int dftk_mi_zgemm_to(dftk_mi_basis* basis, char transA, int64_t m, int64_t n, int64_t k,
                     dftk_mi_cplx alpha, const dftk_mi_cplx* A_d, int64_t lda,
                     const dftk_mi_cplx* B_d, int64_t ldb, dftk_mi_cplx beta,
                     const dftk_mi_cplx* C_d, int64_t ldc, dftk_mi_cplx* D_d, int flags);
/* Hermitian eigen-decomposition (blocked parallel Jacobi): A (n x n, full storage, destroyed),
 * W_h[n] ascending eigenvalues (host), V_d n x n eigenvectors (columns, sorted like W). */
int dftk_mi_heev(dftk_mi_basis* basis, int n, dftk_mi_cplx* A_d, int64_t lda, double* W_h,
                 dftk_mi_cplx* V_d, int64_t ldv);
/* The LOWEST nev eigenpairs only -- what rayleigh_ritz consumes (lobpcg_hyper_impl.jl:141-153: `vectors[:, 1:N]`
 * of the 2N x 2N / 3N x 3N matrix Y'AY): one spectral split by a Newton-Schulz sign iteration on the f64 matrix cores
 * (sigma above the nev-th smallest diagonal entry), an orthonormal basis of the lower invariant subspace by
 * Cholesky-QR, the blocked Jacobi on the k x k projected matrix (nev <= k), one product back.  W_h[0 .. nev) and the
 * first nev columns of V_d are set; A is left intact.  Small problems (n < 384), nev > 0.6 n and inputs on which the
 * split fails its own checks go to dftk_mi_heev (A destroyed, all n pairs returned).  DFTK_MI_HEEV_PARTIAL=0 switches
 * the split off, DFTK_MI_HEEV_PARTIAL_MIN=<n> moves the size threshold. */
int dftk_mi_heev_lowest(dftk_mi_basis* basis, int n, int nev, dftk_mi_cplx* A_d, int64_t lda, double* W_h,
                        dftk_mi_cplx* V_d, int64_t ldv);
/* Exposed for tests: the mirror pass of dftk_mi_heev_lowest's Newton-Schulz step.  X_d is an n x n matrix whose entries on
 * and above the diagonal are valid (the output of a DFTK_MI_GEMM_SYM_RESULT product), ldt rows per column.  real = 0: entry
 * (i, j), i > j, becomes conj(entry (j, i)) and the imaginary part of the diagonal becomes zero.  real = 1: the REAL "tall"
 * layout (complex row i = REAL rows 2 i, 2 i + 1; ldt >= (n + 1) / 2): REAL entry (r, c), r > c, becomes entry (c, r), and
 * every REAL row from n to 2 ldt - 1 (padding) becomes zero.  Plain copies in a fixed order, no atomics. */
int dftk_mi_eig_mirror_tall(dftk_mi_basis* basis, int n, int real, dftk_mi_cplx* X_d, int64_t ldt);
/* Host-only: the shift rule of dftk_mi_heev_lowest on a diagonal (sigma, estimated distance to the nearest
 * eigenvalue) and, for a norm bound of A - sigma I, the number of held iterations (CPU test-suite). */
int dftk_mi_heev_sigma_host(int n, const double* diag_h, int nev, double* sigma, double* gap_guess,
                            int* hold_iterations, double norm_bound);
/* Upper Cholesky A = R^H R in place (strict lower part left untouched) + inverse of R.
 * Returns DFTK_MI_NUM_CHOLESKY when a pivot is not positive / finite. */
int dftk_mi_potrf_trtri(dftk_mi_basis* basis, int n, dftk_mi_cplx* A_d, int64_t lda,
                        dftk_mi_cplx* invR_d, int64_t ldi);
/* The same for a REAL symmetric A stored as complex: the caller vouches that every imaginary part of the upper
 * triangle is exactly zero (the Gram matrices of the real-symmetric Gamma iteration); they are not read. */
int dftk_mi_potrf_trtri_real(dftk_mi_basis* basis, int n, dftk_mi_cplx* A_d, int64_t lda,
                             dftk_mi_cplx* invR_d, int64_t ldi);

/* ---- atomic-orbital projections and the projected density of states (src/postprocess/dos.jl:70-212; pdos_kernels.hip) ----
 * ortho_lowdin (src/common/ortho.jl:11-17) of the n_rows x n_cols block Phi_d (leading dimension ld), in place:
 * S = Phi' Phi by the library's zgemm, S = V diag(lambda) V' by the Hermitian eigensolver behind the heev entry,
 * Phi <- Phi V diag(lambda^-1/2) V' panel by panel (extra workspace: one panel of rows and three n_cols^2 matrices).
 * evals_h (optional, [n_cols]) receives lambda, ascending.  Linearly dependent columns -- min |lambda| <= 2^-52 max |lambda|,
 * the reference's assertion -- return DFTK_MI_NUM_RANK_DEFICIENT with Phi_d untouched; the error text names the ratio.
 * DFTK_MI_EINVAL: n_cols < 1, n_cols > n_rows, ld < n_rows, a call inside a batched multi-k call.  Fixed reduction order:
 * two calls give bitwise identical results. */
int dftk_mi_lowdin_ortho(dftk_mi_basis* basis, int64_t n_rows, int n_cols, dftk_mi_cplx* Phi_d, int64_t ld,
                         double* evals_h);
/* One k-block of atomic_orbital_projections / compute_pdos.  psi_d: n_rows x n_bands, Phi_d: n_rows x n_proj (orthonormal
 * orbitals), both column-major in the caller's full-sphere complex layout (the orbitals of a Gamma-real block included).
 * C = Phi' psi is one zgemm.
 *   proj_d (optional, device, n_proj x n_bands column-major) is OVERWRITTEN with |C_pn|^2, the fat-band weights;
 *   pdos_d (optional, device, n_eps x n_proj column-major) is ACCUMULATED:
 *       pdos[e, p] += weight sum_n g(eps_h[e], eig_h[n]) |C_pn|^2,  g(e, x) = -occupation_derivative((x - e) / T) / T,
 *       weight = filled_occupation * kweight; smearing_kind 1 = Fermi-Dirac, 2 = Gaussian (Smearing.jl:66-92), whose
 *       Fermi-Dirac derivative is written so that |x - e| / T of several hundred gives exactly 0.
 * The accumulation is a tiled real product (a workgroup per tile of energies x projectors, bands in ascending order,
 * |C|^2 staged through LDS), no atomics: reproducible bit for bit.  DFTK_MI_EINVAL, nothing written: both outputs NULL, a
 * leading dimension below n_rows, a size below 1 and, when pdos_d is given, temperature <= 0, an unknown smearing kind or
 * n_eps < 1; a call inside a batched multi-k call. */
int dftk_mi_pdos_accumulate(dftk_mi_basis* basis, int64_t n_rows, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                            int n_proj, const dftk_mi_cplx* Phi_d, int64_t ld_phi, const double* eig_h, double weight,
                            int smearing_kind, double temperature, int n_eps, const double* eps_h, double* proj_d,
                            double* pdos_d);

/* ---- DFT+U: the Hubbard occupation matrix and the rotation of a manifold's orbitals (src/terms/hubbard.jl:149-228;
 *      hubbard_kernels.hip) ----
 * One k-block of compute_hubbard_n.  psi_d: n_rows x n_bands, Phi_d: n_rows x n_proj (orthonormal orbitals), both
 * column-major in the caller's full-sphere complex layout, as for dftk_mi_pdos_accumulate.  C = Phi' psi is one zgemm into
 * basis scratch.  Block b is the s = block_size_h[b] <= 7 consecutive columns of Phi_d that start at block_first_h[b] (the
 * 2 l + 1 orbitals of one atom); blocks may come in any order and need not cover Phi_d.  n_d (device) holds the blocks one
 * after the other, block b as a column-major s x s complex matrix, and is ACCUMULATED:
 *     n_b[m1, m2] += sum_n w_h[n] C[p0 + m1, n] conj(C[p0 + m2, n]),      w_h[n] = kweight occupation_n / filled_occupation
 * (i_projection * diagm(occupation / filled_occ) * j_projection of hubbard.jl:217-222), so that one buffer per spin channel
 * collects every k-block and is fetched once.  One workgroup per block, the bands strided over its threads, a fixed-order
 * tree through LDS, no atomics: reproducible bit for bit.  DFTK_MI_EINVAL, nothing written: a size below 1, a block that
 * is not inside [0, n_proj), a block of more than 7 orbitals, a leading dimension below n_rows, a call inside a batched
 * multi-k call. */
int dftk_mi_hubbard_occupation(dftk_mi_basis* basis, int64_t n_rows, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                               int n_proj, const dftk_mi_cplx* Phi_d, int64_t ld_phi, const double* w_h, int n_blocks,
                               const int* block_first_h, const int* block_size_h, dftk_mi_cplx* n_d);
/* Out[:, block b] = Phi[:, block b] V_b for every block in one launch: V_h (host) holds the column-major s x s complex
 * matrices one after the other, Out_d is laid out like Phi_d (leading dimension ld_out) and may not overlap it; the blocks
 * must be disjoint; columns of Out_d outside every block are left untouched.  With n_b = V nu V' the rotated orbitals carry
 * the Hubbard operator with REAL DIAGONAL couplings, Phi_b (U / 2)(1 - 2 n_b) Phi_b' = (Phi_b V) diag(U / 2 (1 - 2 nu))
 * (Phi_b V)', which is what dftk_mi_kblock_set_projectors takes.  DFTK_MI_EINVAL, nothing written: a size below 1, a block
 * that starts below 0 or holds more than 7 orbitals, two blocks that share a column, a leading dimension below n_rows,
 * overlapping Out_d and Phi_d, a call inside a batched multi-k call. */
int dftk_mi_hubbard_rotate(dftk_mi_basis* basis, int64_t n_rows, int n_blocks, const int* block_first_h,
                           const int* block_size_h, const dftk_mi_cplx* Phi_d, int64_t ld_phi, const dftk_mi_cplx* V_h,
                           dftk_mi_cplx* Out_d, int64_t ld_out);

/* ---- comm_kpts: replaces MPI.Init / mpi_sum!(rho, comm_kpts)
 *      (src/common/mpi.jl:19-32 at src/densities.jl:46) with RCCL over xGMI ---------------------
 * Rank 0 calls get_unique_id and ships the 128 bytes to the other ranks by any side channel. */
int dftk_mi_comm_get_unique_id(char id_out[128]);
int dftk_mi_comm_init_rank(const char id[128], int n_ranks, int rank, int device,
                           dftk_mi_comm** comm_out);
/* Host-staged communicator: the library copies device data to pinned host buffers and calls back -- the hook
 * for MPI (MPI.Allreduce! / MPI.Alltoallv! in a Julia shim) and for running several ranks on one GPU in tests.
 * allreduce: in-place sum of n doubles.  alltoallv: piece i of send_h (offset / count in DOUBLES) goes to rank i,
 * piece i of recv_h comes from rank i (alltoallv may be NULL if no k-block is sharded).  Return 0 on success. */
typedef int (*dftk_mi_allreduce_fn)(void* user, double* buf_h, size_t n);
typedef int (*dftk_mi_alltoallv_fn)(void* user, const double* send_h, const size_t* send_counts,
                                    const size_t* send_offsets, double* recv_h, const size_t* recv_counts,
                                    const size_t* recv_offsets);
int dftk_mi_comm_create_host(int n_ranks, int rank, int device, dftk_mi_allreduce_fn allreduce,
                             dftk_mi_alltoallv_fn alltoallv, void* user, dftk_mi_comm** comm_out);
int dftk_mi_comm_destroy(dftk_mi_comm* comm);
/* What the communicator is: *backend = 0 RCCL / 1 host callbacks; *n_ranks as RCCL itself reports it
 * (ncclCommCount) for an RCCL communicator; *version = ncclGetVersion code (0 for the host back end). */
int dftk_mi_comm_describe(const dftk_mi_comm* comm, int* backend, int* n_ranks, int* version);
int dftk_mi_comm_rank(const dftk_mi_comm* comm);
int dftk_mi_comm_size(const dftk_mi_comm* comm);
/* In-place sum all-reduce of n doubles on `stream` (hipStream_t as void*, NULL = default). */
int dftk_mi_allreduce_sum_f64(dftk_mi_comm* comm, double* buf_d, size_t n, void* stream);

/* ---- plane-wave sharding of ONE k-block over a communicator (Gamma-only cells) ----------
 * The reference can only duplicate a k-point on surplus ranks (src/PlaneWaveBasis.jl:190-203).  Here rank r owns
 * the rows [row_starts_h[r], row_starts_h[r+1]) of the sphere (row_starts_h has n_ranks + 1 entries, 0 .. n_G):
 * after this call every orbital block handed to dftk_mi_apply_H(_parts) / dftk_mi_lobpcg /
 * dftk_mi_density_accumulate is that row slab (packed: leading dimension == local rows for apply_H / density),
 * and dftk_mi_kblock_set_projectors takes the row slab of P.  Inside: products over n_G become local partial
 * sums + one small all-reduce, the small dense factorizations run replicated, and the FFT pipeline is fed by
 * a slab <-> band all-to-all (every rank transforms n_bands / n_ranks whole bands).  dftk_mi_density_accumulate
 * then adds only this rank's bands into rho_d: complete it with dftk_mi_allreduce_sum_f64 over the same
 * communicator.  Call before set_projectors; comm = NULL un-shards.  The communicator is borrowed. */
int dftk_mi_kblock_set_shard(dftk_mi_kblock* kb, dftk_mi_comm* comm, const int64_t* row_starts_h);

/* ---- real-symmetric orbitals of a Gamma-point block (EXTENSION: the reference has no Gamma special case) -------
 * At k = 0 the Hamiltonian of the reference's models (real local potential, projectors of real functions)
 * commutes with complex conjugation in real space: its eigenvectors can be chosen with psi(-G) = conj(psi(G)).
 * After dftk_mi_kblock_set_gamma_real(kb, 1), dftk_mi_lobpcg on this block projects the caller's X onto that
 * invariant subspace, iterates on its HALF-SPHERE image (row 0 = x(G = 0), real; row j > 0 = sqrt(2) x(G_j) for one
 * representative of every pair {G, -G}; n_half = (n_G + 1) / 2 rows), and hands back full-sphere vectors.
 * Eigenvalues, residual norms, density and energies are those of the general complex iteration (same operator,
 * same spectrum and multiplicities); every n_G-long product runs as a REAL matrix product over half the rows
 * (DFTK_MI_GEMM_REAL: a third of the matrix-core flops) and two bands share one FFT pipeline pass (a + i b).
 * Errors (DFTK_MI_EINVAL): sphere without inversion symmetry / with a Nyquist point, kinetic(G) != kinetic(-G)
 * (k != 0), projectors that are not real-symmetric (checked when they are first used).
 * Plane-wave sharded block: call AFTER dftk_mi_kblock_set_shard; the half-format rows are then split evenly over
 * the ranks (dftk_mi_gamma_half_size returns this rank's count; dftk_mi_gamma_compress / _expand / _apply_H become
 * collective and work on packed row slabs), the caller keeps handing full-sphere row slabs to dftk_mi_lobpcg.
 * dftk_mi_apply_H / dftk_mi_density_accumulate on the block keep their general complex semantics.
 * dftk_mi_lobpcg_last_AX returns NULL after a real-mode run. */
int dftk_mi_kblock_set_gamma_real(dftk_mi_kblock* kb, int on);
int dftk_mi_gamma_half_size(dftk_mi_kblock* kb, int64_t* n_half);
/* Host-only pair tables (CPU test-suite): row_h[j] / partner_row_h[j] = sphere rows of G_j / -G_j, j = 0 is G = 0;
 * pairs ascending in row_h.  NULL tables: only count. */
int dftk_mi_gamma_tables_host(int nx, int ny, int nz, int64_t n_G, const int64_t* mapping0_h, int64_t* n_half,
                              int32_t* row_h, int32_t* partner_row_h);
/* full sphere (n_G x m) -> half format (n_half x m): the real-symmetric part (x(G) + conj x(-G)) / 2, scaled; and
 * back (exact inverse on real-symmetric vectors). */
int dftk_mi_gamma_compress(dftk_mi_kblock* kb, int m, const dftk_mi_cplx* X_d, int64_t ldx, dftk_mi_cplx* Xh_d,
                           int64_t ldh);
/* What dftk_mi_lobpcg does with its start vectors on a Gamma-real block: every column is rotated by the global phase
 * exp(-i phi), exp(2 i phi) = s / |s|, s = sum_G x(G) x(-G), that maximises its real-symmetric part, then compressed.
 * A real field times any phase (e.g. an orbital of a complex iteration) keeps all of its norm; a column that is already
 * real-symmetric is compressed bit for bit as by dftk_mi_gamma_compress. */
int dftk_mi_gamma_compress_aligned(dftk_mi_kblock* kb, int m, const dftk_mi_cplx* X_d, int64_t ldx, dftk_mi_cplx* Xh_d,
                                   int64_t ldh);
int dftk_mi_gamma_expand(dftk_mi_kblock* kb, int m, const dftk_mi_cplx* Xh_d, int64_t ldh, dftk_mi_cplx* X_d,
                         int64_t ldx);
/* H psi on half-format blocks (`which` as dftk_mi_apply_H_parts). */
int dftk_mi_gamma_apply_H(dftk_mi_kblock* kb, int which, int n_bands, const dftk_mi_cplx* psih_d, int64_t ld_psi,
                          dftk_mi_cplx* Hpsih_d, int64_t ld_Hpsi);
/* dftk_mi_density_accumulate for REAL-SYMMETRIC columns in the full-sphere layout (what a real-mode dftk_mi_lobpcg
 * returns): bands 2p and 2p + 1 share one transform (rho += w_2p Re^2 + w_2p+1 Im^2).  The caller vouches for the
 * symmetry; general complex columns give a wrong density.  Needs no prior set_gamma_real. */
int dftk_mi_density_accumulate_real(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                    const double* weight_h, double* rho_d);

/* Host-only view of the slab <-> band transposition plan of a sharded block (CPU test-suite): for `rank` of
 * `n_ranks`, an n_bands block: band_starts[s] .. band_starts[s+1] = bands transformed by rank s; slab_off/cnt[s] =
 * piece of the packed n_loc x n_bands slab that goes to rank s; band_off/cnt[r] = piece of the packed band layout that
 * comes from rank r (offsets / counts in complex elements). */
int dftk_mi_shard_plan_host(int n_ranks, int rank, int n_bands, const int64_t* row_starts_h, int* band_starts,
                            int64_t* slab_off, int64_t* slab_cnt, int64_t* band_off, int64_t* band_cnt);

/* ---- per-family kernel timing with HIP events on the basis' stream (used by bench.py) ----------
 * family: 0 UNSTRUCTURED zgemm calls (work = 8mnk flops; 4mnk for a DFTK_MI_GEMM_REAL call = the flops of the
 * equivalent real product), 1..5 FFT stages A..E (work = algorithmic bytes of
 * the pruned pipeline), 6 density z-pass, 7 heev, 8 potrf+trtri, 9 whole apply_H
 * (work = bands), 10 zgemm operand bytes (no time), 11 STRUCTURED zgemm calls (UPPER / B_UPPER; work = flops of
 * the mathematically needed part only), 12 real flops the launched zgemm tiles execute (no time; 6 per complex
 * multiply-add in the 3M kernels, 4 in the REAL ones), 13 collectives of a sharded block (work = bytes), 14 useful
 * flops of all zgemm calls counted as complex products (no time; a REAL call counts twice its flops: what the
 * general complex iteration would need).  enable(1) resets. */
int dftk_mi_prof_enable(dftk_mi_basis* basis, int on);
int dftk_mi_prof_get(dftk_mi_basis* basis, int family, double* total_ms, double* work, int64_t* launches);
/* ---- density-sized solvers of the SCF glue (mix_kernels.hip) -----------------------------
 * Anderson acceleration of the density fixed-point iteration (src/scf/anderson.jl:36-130, ScfAndersonDensitySolver of
 * src/scf/scf_solvers.jl:68-102): history of up to m (iterate, preconditioned residual) pairs of n doubles on the
 * device; a step = one reduction kernel (the inner products with the new residual; the Gram matrix of the history is
 * kept), ONE host synchronisation, the m x m least-squares problem on the host (conditioning test on cond(R) =
 * sqrt(cond(M'M)), entries with error > errorfactor * min dropped, as the reference), one fused update kernel.
 * x_next_d must not alias the inputs.  m = 0, errorfactor <= 1 or maxcond <= 1 (anderson.jl:82): no acceleration, plain
 * damping x + alpha Pf at every call and an empty history. */
typedef struct dftk_mi_anderson dftk_mi_anderson;
int dftk_mi_anderson_create(dftk_mi_basis* basis, int64_t n, int m, double maxcond, double errorfactor,
                            dftk_mi_anderson** out);
int dftk_mi_anderson_destroy(dftk_mi_anderson* acc);
int dftk_mi_anderson_reset(dftk_mi_anderson* acc);
int dftk_mi_anderson_history(const dftk_mi_anderson* acc);   /* entries held */
int dftk_mi_anderson_step(dftk_mi_anderson* acc, const double* x_d, double alpha, const double* Pf_d, double* x_next_d,
                          int* n_history /* may be NULL */);
/* chi0 mixing (src/scf/mixing.jl:228-290, LdosMixing / HybridMixing / Chi0Mixing with RPA = true):
 * d_rho = (1 - chi0 vc)^-1 dF by restarted GMRES in real space (KrylovKit linsolve: krylovdim, tol = max(1e-12,
 * reltol |dF - mean dF|), zero start vector), vc = the Hartree kernel through its multiplier cube poisson_d
 * (src/terms/hartree.jl:68-81; NULL: no Hartree term), chi0 = LdosModel (ldos_d: n_comp cubes = the local density of
 * states at the Fermi level, src/scf/chi0models.jl:21-45; NULL or |ldos| < sqrt(eps) everywhere: term absent) and /
 * or DielectricModel (dielectric != 0: kTF, eps_r, :54-80, needs recip_lattice_h, column-major 3 x 3).  n_comp = 2:
 * collinear spin, vectors are (up, down) stacked, the Hartree kernel sees the total.  With no term alive d_rho = dF
 * (simple mixing, chi0models.jl:32, mixing.jl:264-266).  Every Krylov step is 12 launches and ONE host
 * synchronisation (all inner products of the classical Gram-Schmidt step in one fetch; a second pass, with one more
 * fetch, when the remainder is shorter than |w| / sqrt 2).  *n_applies = applications of the dielectric operator, *converged = 0 if maxiter cycles did not
 * reach the tolerance (d_rho is the last iterate, as the reference's mixing uses it). */
int dftk_mi_chi0_mix(dftk_mi_kblock* cube_kblock, int n_comp, const double* recip_lattice_h, const double* poisson_d,
                     const double* ldos_d, double dvol, int dielectric, double kTF, double eps_r, const double* dF_d,
                     double reltol, int krylovdim, int maxiter, double* drho_d, int* n_applies, int* converged);

/* ---- the optimiser of direct_minimization (dm_kernels.hip; src/scf/direct_minimization.jl, which hands these steps to
 * Optim.jl's L-BFGS on a product of Stiefel manifolds) ---------------------------------------------------------------
 * Optim's project_tangent!(Stiefel(), g, x): G <- G - X (X'G + G'X) / 2 in place, X and G n x m column-major.  One zgemm,
 * one kernel that symmetrises the m x m matrix on the device, one zgemm; no host synchronisation (beyond a first-use
 * growth of the workspace).  DFTK_MI_EINVAL, G untouched: n < 1, m < 1, a leading dimension below n, X_d == G_d, a call
 * inside a batched multi-k call. */
int dftk_mi_stiefel_project_tangent(dftk_mi_basis* basis, int64_t n, int m, const dftk_mi_cplx* X_d, int64_t ldx,
                                    dftk_mi_cplx* G_d, int64_t ldg);
/* L-BFGS on packed vectors.  A packed vector is a list of n_blocks column-major complex blocks, block b of n_rows[b] x
 * n_cols[b] entries with a leading dimension >= n_rows[b], given as HOST arrays of device pointers and of leading
 * dimensions.  The inner product is Optim's: <a, b> = sum over blocks and entries of Re(conj(a) b), no k-weights.
 *
 * The handle holds on the device memory + 1 slots of pairs (s, y), the previous point and the previous gradient, each
 * stored block after block without padding ((2 memory + 4) packed vectors: the spare slot receives the candidate pair of an
 * update, so that a rejected pair leaves a full history as it was), the loop coefficients alpha_i and two buffers of
 * partial sums.  rho_i = 1 / <s_i, y_i> is kept with the history and reaches the kernels through device memory.
 *
 * update: the first call after create / reset only stores (x, g): *kept = 0, *sy_h = 0, no synchronisation.  Every later
 * call is ONE fused pass (reads x, g, x_prev, g_prev; writes s = x - x_prev and y = g - g_prev into the spare slot and the
 * new x_prev, g_prev; block partial sums of <s, y> in a fixed order) and ONE host synchronisation, after which *sy_h =
 * <s, y>.  The pair enters the history (the oldest one leaves when memory pairs are held) only if <s, y> is finite and
 * > 0 -- stricter than Optim, which skips the infinite case only; otherwise the history is unchanged and *kept = 0.
 *
 * direction: d = -H g by the two-loop recursion; g is not modified, d_d must not alias g_d and serves as the work vector.
 *   newest to oldest: alpha_i = rho_i <s_i, q>, q -= alpha_i y_i;
 *   middle step     : r = P^-1 q / scale_b, where P^-1 is the Teter-Payne-Allan ldiv! of the block's kinetic vector with
 *                     mean_kin_h[b][n] for column n, kin-wise mean_kin / (mean_kin + kin) exactly as dftk_mi_tpa_ldiv
 *                     applies it (the reference's DMPreconditioner.ldiv!, the caller passes scale_b = the k-weight);
 *                     kblocks == NULL: r = q / scale_b;
 *   oldest to newest: beta = rho_i <y_i, r>, r += (alpha_i - beta) s_i;     d = -r.
 * Every step is one launch of one kernel body: it sums the partial inner products the previous launch left (fixed order),
 * reads rho_i / alpha_i from device memory, applies its axpy and leaves the partial sums of the next inner product, so that
 * every history vector is read once per loop: 2 k + 1 launches with k pairs held (1 with an empty history, where the result
 * is exactly the middle step, negated), whatever n_blocks (one grid walks a table of work items over all blocks).  No host
 * synchronisation and no host read of a device result, no atomics: two calls give bitwise identical results.  The
 * pointer tables, mean_kin_h and rho travel through two pinned staging buffers used in turn; only a third call while the
 * first is still in flight waits (counted as a host synchronisation).  Runs on the basis' stream.
 *
 * DFTK_MI_EINVAL, every output untouched: sizes below 1, memory < 1, a null pointer or a leading dimension below the rows
 * given at creation, a k-block whose sphere is not n_rows[b] long, scale_b <= 0, a call inside a batched multi-k call. */
typedef struct dftk_mi_lbfgs dftk_mi_lbfgs;
int dftk_mi_lbfgs_create(dftk_mi_basis* basis, int n_blocks, const int64_t* n_rows_h, const int* n_cols_h, int memory,
                         dftk_mi_lbfgs** out);
int dftk_mi_lbfgs_destroy(dftk_mi_lbfgs* acc);
int dftk_mi_lbfgs_reset(dftk_mi_lbfgs* acc);
int dftk_mi_lbfgs_history(const dftk_mi_lbfgs* acc);   /* pairs held */
int dftk_mi_lbfgs_update(dftk_mi_lbfgs* acc, const dftk_mi_cplx* const* x_d, const int64_t* ldx_h,
                         const dftk_mi_cplx* const* g_d, const int64_t* ldg_h, double* sy_h, int* kept);
int dftk_mi_lbfgs_direction(dftk_mi_lbfgs* acc, const dftk_mi_cplx* const* g_d, const int64_t* ldg_h,
                            dftk_mi_kblock* const* kblocks /* or NULL */, const double* const* mean_kin_h /* per block, or NULL */,
                            const double* scale_h /* [n_blocks] */, dftk_mi_cplx* const* d_d, const int64_t* ldd_h);

/* ---- the tangent-space solve of Newton's method (newton_kernels.hip; solve_OmegaPlusK of src/response/hessian.jl:111-176
 * with cg! of src/response/cg.jl) ------------------------------------------------------------------------------------
 * The orbitals are fixed for a whole solve, so their real-space values are transformed ONCE and kept by the caller; an
 * application of K then costs two 3-D transforms per band (the change in, dV psi out) instead of four.  All three entries
 * are fp64, use a fixed reduction order and no atomics (two calls give bitwise identical results), are asynchronous on the
 * block's stream and synchronise with the host only when their workspace grows on first use.  A Gamma-real block is
 * accepted and served in the complex full-sphere layout.  DFTK_MI_EINVAL, every output untouched: a plane-wave sharded
 * block, a leading dimension below n_G, n_bands < 0, a null pointer (with n_bands > 0), a call inside a batched multi-k
 * call.  n_bands = 0 is a no-op.
 *
 * orbitals_realspace: psi_r_d[n] = the UNNORMALISED backward transform of column n, sum_G psi_n(G) e^{+iG.r}, as a complex
 *   cube of nx ny nz entries, x fastest, cube n at offset n nx ny nz (what dftk_mi_ifft_sphere gives per column).
 *   The caller folds ifft_normalization^2 into the weights of tangent_density, as for dftk_mi_density_response_accumulate;
 *   tangent_potential divides by nx ny nz itself, so that its result is that of the H apply.
 * tangent_density: drho(r) += sum_n w_h[n] 2 Re[conj psi_n(r) dpsi_n(r)], the quantity dftk_mi_density_response_accumulate
 *   defines with w_docc = 0.  One backward transform per band (of dpsi), then one streaming kernel per launch group that
 *   reads both cubes once, sums the bands of the group in ascending order per grid point and updates drho once.  A launch
 *   group whose weights are all zero is skipped.
 * tangent_potential: out[:, n] (+)= the sphere rows of FFT(dV psi_n(r)) / (nx ny nz), the quantity
 *   dftk_mi_apply_H_parts(which = 1) defines for a block with dV bound (dV_d: nz x ny x nx doubles, not padded).  One
 *   streaming kernel per launch group forms the products, then one forward transform per band.  The block's bound
 *   potential and its LOBPCG state are not touched. */
int dftk_mi_orbitals_realspace(dftk_mi_kblock* kblock, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                               dftk_mi_cplx* psi_r_d);
int dftk_mi_tangent_density(dftk_mi_kblock* kblock, int n_bands, const dftk_mi_cplx* psi_r_d, const dftk_mi_cplx* dpsi_d,
                            int64_t ld_dpsi, const double* w_h, double* drho_d);
int dftk_mi_tangent_potential(dftk_mi_kblock* kblock, int n_bands, const dftk_mi_cplx* psi_r_d, const double* dV_d,
                              dftk_mi_cplx* out_d, int64_t ld_out, int accumulate);
/* The packed-vector pieces of cg! for one right-hand side.  Packed vectors are those of dftk_mi_lbfgs_* (host arrays of
 * device pointers and leading dimensions, block b of n_rows[b] x n_cols[b] entries); the inner product is
 * <a, b> = sum_b weight[b] Re <a_b, b_b> (the k-weights: Omega + K is self-adjoint with respect to it).
 *
 * dot(slot, a, b): one launch that leaves the per-workgroup partial sums of <a, b> in the slot.  GAMMA receives <r, z>;
 *   the value becomes the current gamma at the next update_p, until then it is the NEXT gamma.  PC receives <p, c>, RR
 *   <r, r>.
 * update_xr(p, c, x, r): sums the partials of the current gamma and of PC itself (fixed order, every workgroup for itself),
 *   alpha = gamma / <p, c>; x += alpha p, r -= alpha c in one launch.
 * update_p(z, p, first): beta = next gamma / current gamma formed the same way, p = z + beta p; first != 0: p = z, p is
 *   not read (the start of cg!).  Either way the next gamma becomes the current one.
 * read(out3_h): out3_h = { <r, r>, current gamma, <p, c> } from the slots; the ONE host synchronisation of an iteration.
 * alpha and beta never visit the host.  No atomics: two runs give bitwise identical results.  The block tables travel
 * through pinned staging buffers used in turn (eight; read frees all of them), so no other entry synchronises.
 *
 * DFTK_MI_EINVAL, every output untouched: sizes below 1, a null table, a null block pointer or a leading dimension below
 * the rows given at creation, an unknown slot, a call inside a batched multi-k call. */
typedef struct dftk_mi_tangent_cg dftk_mi_tangent_cg;
#define DFTK_MI_CG_GAMMA 0
#define DFTK_MI_CG_PC 1
#define DFTK_MI_CG_RR 2
int dftk_mi_tangent_cg_create(dftk_mi_basis* basis, int n_blocks, const int64_t* n_rows_h, const int* n_cols_h,
                              const double* weight_h, dftk_mi_tangent_cg** out);
int dftk_mi_tangent_cg_destroy(dftk_mi_tangent_cg* cg);
int dftk_mi_tangent_cg_dot(dftk_mi_tangent_cg* cg, int slot, const dftk_mi_cplx* const* a_d, const int64_t* lda_h,
                           const dftk_mi_cplx* const* b_d, const int64_t* ldb_h);
int dftk_mi_tangent_cg_update_xr(dftk_mi_tangent_cg* cg, const dftk_mi_cplx* const* p_d, const int64_t* ldp_h,
                                 const dftk_mi_cplx* const* c_d, const int64_t* ldc_h, dftk_mi_cplx* const* x_d,
                                 const int64_t* ldx_h, dftk_mi_cplx* const* r_d, const int64_t* ldr_h);
int dftk_mi_tangent_cg_update_p(dftk_mi_tangent_cg* cg, const dftk_mi_cplx* const* z_d, const int64_t* ldz_h,
                                dftk_mi_cplx* const* p_d, const int64_t* ldp_h, int first);
int dftk_mi_tangent_cg_read(dftk_mi_tangent_cg* cg, double* out3_h);

/* Process-wide counters since load: kernel launches issued by the library and host synchronisations it waited on
 * (stream synchronisations of its drivers, result fetches, scheduling rounds of the batched k-point driver).  For the
 * many-small-k workloads these two ARE the cost model; either pointer may be NULL. */
int dftk_mi_launch_count(int64_t* launches, int64_t* host_syncs);

/* Process-wide: the device allocations the library's handles hold right now and their bytes (every handle owns its
 * buffers by member, so both return to their earlier values when a handle is destroyed; the staging pool of the batched
 * k-point driver is kept for the life of the process and not counted).  Lets a test check releases exactly where the
 * device-wide free memory of a shared machine cannot; either pointer may be NULL. */
int dftk_mi_device_buffers_live(int64_t* count, int64_t* bytes);

/* The two density-sized scalars an SCF step reads on the host besides the term energies, in one kernel and one
 * synchronisation: out_h[0] = sum_i a[i] b[i] (b_d may be NULL: 0), out_h[1] = sum_i (a[i] - c[i])^2 (c_d may be NULL: 0);
 * n doubles each, on the device.  The host mirror passes a = rho_out, b = V_in (the nonlocal energy from the Ritz values:
 * sum f eps - E_kin - int V_in rho_out) and c = rho_in (||rho_out - rho_in||, the convergence criterion of
 * src/scf/self_consistent_field.jl:229-236); the caller multiplies by the volume element. */
int dftk_mi_step_sums(dftk_mi_basis* basis, int64_t n, const double* a_d, const double* b_d, const double* c_d, double* out_h);

/* The cube-sized scalars of one trial step of the potential-mixing SCF (potmix_kernels.hip; slope and curvature of the
 * quadratic model of src/scf/potential_mixing.jl:54-56, ||P^-1 dV||^2 of :14, ||rho_next - rho_in||^2 of :224), all inner
 * products of differences of arrays that exist:
 *   out_h[p] = sum_i (a_p[i] - b_p[i]) * (c_p[i] - d_p[i]),   p < n_pairs, 1 <= n_pairs <= 8,
 * a_d .. d_d host tables of n_pairs device pointers to n doubles each (n: the whole array, both spin channels of a
 * collinear one); an entry of b_d / d_d, or the whole table, may be NULL (= 0).  One launch on the basis' stream, block
 * partials into the pinned landing zone, summed on the host in block order: one synchronisation, no atomics, no
 * temporary, bitwise repeatable.  An operand (x - y) whose two pointers equal those of an earlier operand of the call is
 * read once.  The caller multiplies by the volume element.
 * DFTK_MI_EINVAL, out_h untouched: a null basis, out_h, a_d, c_d, a_d[p] or c_d[p]; n < 1; n_pairs outside [1, 8]. */
int dftk_mi_diff_dots(dftk_mi_basis* basis, int64_t n, int n_pairs, const double* const* a_d, const double* const* b_d,
                      const double* const* c_d, const double* const* d_d, double* out_h);

/* compute_occupation's Fermi-level search (src/occupation.jl:99-132, FermiBisection; host-only, no device call): bisection of
 *   excess(eF) = sum_k kweights[k] sum_n filled * smearing((eig[k][n] - eF) / temperature) - n_electrons
 * on the bracket [lo, hi] (excess(lo) < 0 <= excess(hi)) until the midpoint equals an end point (adjacent doubles; at most
 * 200 halvings), *eF_out = midpoint of the final bracket.  eig: the k-points' eigenvalues behind one another (n_bands[k]
 * each).  smearing: 1 = Fermi-Dirac, 2 = Gaussian (Smearing.jl:66-76, :86-92); temperature > 0.  The host mirror runs this
 * once per SCF step (56 trial levels of a 72-k-point mesh: 0.3 ms of interpreted code in a 4 ms step). */
int dftk_mi_fermi_bisection(int n_k, const int* n_bands, const double* eig, const double* kweights, int smearing,
                            double temperature, double filled, double n_electrons, double lo, double hi, double* eF_out);
/* dftk_mi_prof_enable(basis, 3) also books every zgemm call per SHAPE; this returns (and clears) that table: row i of
 * rows6 = { transA ('N' = 0, 'C' = 1), m, n, k, flags (UPPER | B_UPPER | DFTK_MI_GEMM_REAL; the shape key holds no bit for
 * DFTK_MI_GEMM_SYM_RESULT: such a call is listed with the dense call of the same m, n, k, while its time is booked to the
 * structured family 11), calls }, ms[i] = summed time; *count = shapes seen (<= cap
 * rows are written).  bench.py replays the table at 1 / N of the rows for its sharded-step measurement. */
int dftk_mi_prof_zgemm_shapes(dftk_mi_basis* basis, int cap, int64_t* rows6, double* ms, int* count);

/* Diagnostic: measured issue-rate ceiling of v_mfma_f64_16x16x4_f64 (TFLOP/s, no memory traffic). */
int dftk_mi_diag_mfma_peak(dftk_mi_basis* basis, int waves_per_simd, int iters, double* tflops);

/* ---- host-only introspection (no GPU needed; used by the CPU test-suite) ---------------------
 * Launch plan of dftk_mi_zgemm(_ex) for one shape: out[12] = { column-tile width, full tile rows, full tile
 * columns, right-strip tiles, bottom-strip tiles, interior {K chunks, chunk length, chunk->XCD placement},
 * border {K chunks, chunk length, placement}, shifted }.  shifted = 1: a ragged last tile column is covered by
 * one more FULL tile in the interior launch, shifted left to end at column n (it stores only the new columns),
 * instead of a right-strip launch. */
int dftk_mi_zgemm_plan_host(char transA, int64_t m, int64_t n, int64_t k, int flags, int* out12);
/* Host-only, for the CPU test-suite (not part of the computing ABI; it may change with the launch plan).
 * A DFTK_MI_GEMM_B_UPPER product ('N') whose plan has no K split runs TWO column tiles of a row panel per workgroup
 * (tile gn - 1 - p, then tile p): the tiles of that launch in workgroup order, 4 ints each { tile row, tile column,
 * first k, end k } (at most cap are written), *count = their number, 0 when the shape does not take that launch. */
int dftk_mi_zgemm_fold_host(char transA, int64_t m, int64_t n, int64_t k, int flags, int cap, int* items4, int* count);
/* Host-only, for the CPU test-suite (not part of the computing ABI; it may change with the launch plan).
 * A DFTK_MI_GEMM_UPPER product whose interior launch runs over its LIVE tiles only (dftk_mi_zgemm_plan_host: placement 2):
 * gm row panels x gn column tiles x nsplit K chunks, q = column tiles per row panel (row panel r keeps its column
 * tiles >= r q).  The work items of that launch in workgroup order, 3 ints each { K chunk, tile row, tile column } (at
 * most cap are written), *count = their number. */
int dftk_mi_zgemm_compact_host(int gm, int gn, int q, int nsplit, int cap, int* items3, int* count);
/* Schedule of the blocked Jacobi eigensolver for an n x n matrix: *n_blocks = number of 16-wide blocks (even,
 * padded); for round in [-1, *n_blocks - 2] (pass pairs = where = NULL to query n_blocks only):
 * pairs[2k], pairs[2k+1] = the k-th disjoint block pair of the round (round -1: (2k, 2k+1), then a round-robin
 * tournament); where[2b], where[2b+1] = (pair index, member 0/1) of block b -- the inverse map the look-ahead
 * pair solve uses to find last round's rotations of its two blocks. */
int dftk_mi_jacobi_schedule_host(int n, int round, int* n_blocks, int* pairs /* [n_blocks] */,
                                 int* where /* [2 n_blocks] */);
/*
 * 1-D plan for length n: radices (<= 32 entries) and the in-place permutation `pos[e]` such
 * that a decimation-in-time pass wants input element e at position pos[e] and a
 * decimation-in-frequency pass leaves output frequency k at position pos[k]. */
int dftk_mi_fft_plan_host(int n, int* n_radices, int* radices /* [32] */, int* pos /* [n] */);
/* Sphere pruning tables derived from a mapping: number of non-empty x-lines, number of distinct
 * z planes, and (optionally, may be NULL) the line ids (iy + ny*iz) / first-coefficient offsets. */
int dftk_mi_sphere_tables_host(int nx, int ny, int nz, int64_t n_G, const int64_t* mapping0_h,
                               int64_t* n_lines, int* n_zplanes, int64_t* line_id /* [n_lines] */,
                               int64_t* line_start /* [n_lines+1] */);

#ifdef __cplusplus
}
#endif
#endif /* DFTK_MI355X_H */
