// setup_kernels.hip -- basis / term set-up behind the ABI:
//   Kpoint sphere enumeration      src/Kpoint.jl:20-41 (+ kinetic multipliers, src/terms/kinetic.jl:31-35)
//   build_projection_vectors       src/terms/nonlocal.jl:166-244 for HGH pseudopotentials
//                                  (radial parts src/pseudo/PspHgh.jl:140-164, real solid harmonics
//                                   src/common/spherical_harmonics.jl:31-66)
// The reference runs both as host loops (O(N) and O(n_G n_p), minutes for 1000-electron cells).
// Here the sphere is one pass over the cube in index order on the host (native, no cube-sized temporaries) and the
// projector matrix is written by one device kernel, 16 B per element, straight into the caller's P.
#include "common.h"
#include <cmath>
#include <vector>
// This translation unit contracts floating-point expressions into fused multiply-adds within one statement only
// (sphere_enumerate_host below: not at all), the other kernel files across statements as well (the compiler's default for
// device code).  The shared closed forms are compiled in this file's mode: that is what the projectors and the local
// potential have always been built with, and their last bits depend on it.
#pragma clang fp contract(on)
#include "hgh_forms.h"

// ------------------------------------------------------------------------------------------------ sphere (host)
#pragma clang fp contract(off)
int sphere_enumerate_host(int nx, int ny, int nz, const double* B /* recip_lattice, column-major 3x3 */,
                          const double* k, double Ecut, int64_t cap, int64_t* n_G_out, int64_t* mapping0,
                          double* kinetic, int32_t* G_out) {
    int64_t n = 0;
    for (int iz = 0; iz < nz; ++iz) {
        const double gz = (double)signed_freq(iz, nz) + k[2];
        for (int iy = 0; iy < ny; ++iy) {
            const double gy = (double)signed_freq(iy, ny) + k[1];
            for (int ix = 0; ix < nx; ++ix) {
                const double gx = (double)signed_freq(ix, nx) + k[0];
                // B (G + k) spelled out column by column, the same operation order as the host mirror / the oracle
                double s = 0.0;
                for (int c = 0; c < 3; ++c) {
                    const double q = gx * B[c + 0] + gy * B[c + 3] + gz * B[c + 6];
                    s += q * q;
                }
                const double kin = s / 2;
                if (kin <= Ecut) {
                    if (n < cap) {
                        if (mapping0) mapping0[n] = (int64_t)ix + (int64_t)nx * ((int64_t)iy + (int64_t)ny * iz);
                        if (kinetic) kinetic[n] = kin;
                        if (G_out) {
                            G_out[3 * n + 0] = signed_freq(ix, nx);
                            G_out[3 * n + 1] = signed_freq(iy, ny);
                            G_out[3 * n + 2] = signed_freq(iz, nz);
                        }
                    }
                    n += 1;
                }
            }
        }
    }
    *n_G_out = n;
    if (n > cap && (mapping0 || kinetic || G_out)) {
        dftk_set_error("sphere has %lld plane waves, the buffers hold %lld", (long long)n, (long long)cap);
        return DFTK_MI_EINVAL;
    }
    return 0;
}
#pragma clang fp contract(on)

// ------------------------------------------------------------------------------------------------ projectors (device)
// P[g, c] = radial_{l,i}(|q|) * Y_lm(q) * (-i)^l / sqrt(Omega) * exp(-2 pi i (G + k).r),  q = B (G + k)
// TABLE = false: the HGH closed form of the column's channel; TABLE = true: Rtab[ProjCol::chan][row], the radial
// transform of a numeric channel at |q| of this row (dftk_mi_radial_transform kind 0), everything else the same body
template <bool TABLE>
__global__ __launch_bounds__(256) void k_build_projectors(int64_t n_rows, int n_cols, const int32_t* __restrict__ G,
                                                          Mat3 B, double kx, double ky, double kz, double inv_sqrt_vol,
                                                          const ProjCol* __restrict__ cols,
                                                          const double* __restrict__ Rtab, int64_t ldR,
                                                          cd* __restrict__ P, int64_t ldP) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_rows) return;
    const double px = (double)G[3 * g + 0] + kx, py = (double)G[3 * g + 1] + ky, pz = (double)G[3 * g + 2] + kz;
    double qx, qy, qz;
    recip_times(B, px, py, pz, &qx, &qy, &qz);
    const double qn = sqrt(qx * qx + qy * qy + qz * qz);
    for (int c = blockIdx.y; c < n_cols; c += gridDim.y) {
        const ProjCol pc = cols[c];
        double R, dR, gY[3];
        if (TABLE) {
            R = Rtab[(int64_t)pc.chan * ldR + g];
        } else {
            hgh_radial(pc.l, pc.i, pc.rp, (qn * pc.rp) * (qn * pc.rp), &R, &dR);
        }
        double fr = R * solid_harmonic(pc.l, pc.m, qx, qy, qz, gY) * inv_sqrt_vol, fi = 0.0;
        rotate_minus_i_pow(pc.l, &fr, &fi);
        const double ph = -2.0 * M_PI * (px * pc.rx + py * pc.ry + pz * pc.rz);
        double sn, cs;
        sincos(ph, &sn, &cs);
        P[(int64_t)c * ldP + g] = make_double2(fr * cs - fi * sn, fr * sn + fi * cs);
    }
}

// the columns of P in the order every consumer relies on (build_projectors_hgh, stress_kinetic_nonlocal): see common.h
int list_projector_columns(int n_species, const double* rp_h, const int* nproj_h, int n_atoms,
                           const int* species_of_atom_h, const double* positions_h, std::vector<ProjCol>* cols,
                           std::vector<int>* col_start) {
    cols->clear();
    if (col_start) col_start->assign(1, 0);
    for (int a = 0; a < n_atoms; ++a) {
        const int s = species_of_atom_h[a];
        if (s < 0 || s >= n_species) return DFTK_MI_EINVAL;
        for (int l = 0; l < 4; ++l) {
            const int nl = nproj_h[4 * s + l];
            if (nl < 0 || nl > 3 || (l == 2 && nl > 2) || (l == 3 && nl > 1)) {
                dftk_set_error("HGH projector l=%d with %d radial functions is not tabulated", l, nl);
                return DFTK_MI_EINVAL;
            }
            for (int m = -l; m <= l; ++m)
                for (int i = 1; i <= nl; ++i)
                    cols->push_back(ProjCol{positions_h[3 * a], positions_h[3 * a + 1], positions_h[3 * a + 2],
                                            rp_h[4 * s + l], l, m, i, 0});
        }
        if (col_start) col_start->push_back((int)cols->size());
    }
    return 0;
}

int build_projectors_hgh(dftk_mi_basis* b, int64_t n_rows, const int32_t* G_d, const double* recip_h, const double* k_h,
                         double volume, int n_species, const double* rp_h, const int* nproj_h, int n_atoms,
                         const int* species_of_atom_h, const double* positions_h, cd* P_d, int64_t ldP, int* n_p_out) {
    std::vector<ProjCol> cols;
    CHK(list_projector_columns(n_species, rp_h, nproj_h, n_atoms, species_of_atom_h, positions_h, &cols));
    *n_p_out = (int)cols.size();
    if (cols.empty() || !P_d) return 0;
    if (ldP < n_rows) return DFTK_MI_EINVAL;
    CHK(ensure_ws(b, cols.size() * sizeof(ProjCol)));
    HIPCHK(hipMemcpyAsync(b->ws, cols.data(), cols.size() * sizeof(ProjCol), hipMemcpyHostToDevice, b->stream));
    const unsigned gy = (unsigned)std::min<size_t>(cols.size(), 64);
    hipLaunchKernelGGL(k_build_projectors<false>, dim3((unsigned)((n_rows + 255) / 256), gy), dim3(256), 0, b->stream,
                       n_rows, (int)cols.size(), G_d, make_mat3(recip_h), k_h[0], k_h[1], k_h[2], 1.0 / sqrt(volume),
                       reinterpret_cast<const ProjCol*>(b->ws.get()), (const double*)nullptr, (int64_t)0, P_d, ldP);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));   // cols (host vector) and b->ws are reused by the next call
    return 0;
}

// the same columns with tabulated radial parts: species s owns n_chan_h[4 s + l] channels of angular momentum l, rows
// first_chan_h[4 s + l] ... of R_d (leading dimension ldR >= n_rows); any number of channels per l
int build_projectors_radial(dftk_mi_basis* b, int64_t n_rows, const int32_t* G_d, const double* recip_h,
                            const double* k_h, double volume, int n_species, const double* R_d, int64_t ldR,
                            const int* first_chan_h, const int* n_chan_h, int n_atoms, const int* species_of_atom_h,
                            const double* positions_h, cd* P_d, int64_t ldP, int* n_p_out) {
    std::vector<ProjCol> cols;
    for (int a = 0; a < n_atoms; ++a) {
        const int s = species_of_atom_h[a];
        if (s < 0 || s >= n_species) return DFTK_MI_EINVAL;
        for (int l = 0; l < 4; ++l) {
            const int nl = n_chan_h[4 * s + l], c0 = first_chan_h[4 * s + l];
            if (nl < 0 || (nl > 0 && c0 < 0)) return DFTK_MI_EINVAL;
            for (int m = -l; m <= l; ++m)
                for (int i = 1; i <= nl; ++i)
                    cols.push_back(ProjCol{positions_h[3 * a], positions_h[3 * a + 1], positions_h[3 * a + 2], 0.0, l, m,
                                           i, c0 + i - 1});
        }
    }
    *n_p_out = (int)cols.size();
    if (cols.empty() || !P_d) return 0;
    if (ldP < n_rows || ldR < n_rows || !R_d) return DFTK_MI_EINVAL;
    if (n_rows == 0) return 0;
    CHK(ensure_ws(b, cols.size() * sizeof(ProjCol)));
    HIPCHK(hipMemcpyAsync(b->ws, cols.data(), cols.size() * sizeof(ProjCol), hipMemcpyHostToDevice, b->stream));
    const unsigned gy = (unsigned)std::min<size_t>(cols.size(), 64);
    hipLaunchKernelGGL(k_build_projectors<true>, dim3((unsigned)((n_rows + 255) / 256), gy), dim3(256), 0, b->stream,
                       n_rows, (int)cols.size(), G_d, make_mat3(recip_h), k_h[0], k_h[1], k_h[2], 1.0 / sqrt(volume),
                       reinterpret_cast<const ProjCol*>(b->ws.get()), R_d, ldR, P_d, ldP);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));   // cols (host vector) and b->ws are reused by the next call
    return 0;
}

// ------------------------------------------------------------------------------------------------ atomic superpositions
// f(G) = sum_species ff_s(|G|) sum_{a in s} e^{-2 pi i G.r_a} / sqrt(Omega) on the whole cube, entries whose -G partner
// is not on the grid zeroed (enforce_real!, symmetry.jl:318-337), then the inverse cube FFT:
//   kind 0: compute_local_potential (src/terms/local.jl:108-138) with the HGH local form factor
//           (eval_psp_local_fourier, src/pseudo/PspHgh.jl:110-124); params = {rloc, Zion, c1, c2, c3, c4}
//   kind 1: Gaussian valence-density superposition (src/density_methods.jl:111-125,158-181,236-244);
//           params = {decay length, valence charge}
struct AtomPar {
    double rx, ry, rz;
    int species;
};
// TABLE = true: ff_s(|G|) is read from par[species * N + cube index] (dftk_mi_atomic_superposition_table) instead of
// being evaluated from the 8 parameters of the species, and atom a enters with the amplitude coef[a] (coef may be null: 1)
template <bool TABLE>
__global__ __launch_bounds__(256) void k_atomic_sum(int nx, int ny, int nz, Mat3 B, int kind, int n_atoms,
                                                    const AtomPar* __restrict__ atoms, const double* __restrict__ par,
                                                    const double* __restrict__ coef, double inv_sqrt_vol,
                                                    cd* __restrict__ out) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), iz = (int)(idx / ((int64_t)nx * ny));
    if (unpaired_nyquist(ix, iy, iz, nx, ny, nz)) {
        out[idx] = make_double2(0.0, 0.0);
        return;
    }
    const double gx = (double)signed_freq(ix, nx), gy = (double)signed_freq(iy, ny), gz = (double)signed_freq(iz, nz);
    double qx, qy, qz;
    recip_times(B, gx, gy, gz, &qx, &qy, &qz);
    const double p = sqrt(qx * qx + qy * qy + qz * qz);
    double re = 0.0, im = 0.0;
    int cur = -1;
    double ff = 0.0;
    for (int a = 0; a < n_atoms; ++a) {
        const AtomPar at = atoms[a];
        if (at.species != cur) {      // atoms arrive grouped by species: one form-factor evaluation per species
            cur = at.species;
            const double* q = par + 8 * cur;
            if (TABLE) {
                ff = par[(int64_t)cur * N + idx];
            } else if (kind == 0) {
                ff = hgh_local_ff(q, (p * q[0]) * (p * q[0]));
            } else {
                const double x = p * q[0];
                ff = q[1] * exp(-x * x);
            }
            ff *= inv_sqrt_vol;
        }
        double sn, cs;
        sincos(-2.0 * M_PI * (gx * at.rx + gy * at.ry + gz * at.rz), &sn, &cs);
        if (TABLE && coef) {
            const double f = ff * coef[a];
            re += f * cs;
            im += f * sn;
        } else {
            re += ff * cs;
            im += ff * sn;
        }
    }
    out[idx] = make_double2(re, im);
}

__global__ __launch_bounds__(256) void k_real_part_scaled(int64_t n, const cd* __restrict__ c, double scale,
                                                          double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = scale * c[i].x;
}

int check_species_grouped(const char* who, int n_species, int n_atoms, const int* species_of_atom_h) {
    for (int a = 0; a < n_atoms; ++a) {
        if (species_of_atom_h[a] < 0 || species_of_atom_h[a] >= n_species) return DFTK_MI_EINVAL;
        if (a > 0 && species_of_atom_h[a] < species_of_atom_h[a - 1]) {
            dftk_set_error("%s: atoms must be grouped by species", who);
            return DFTK_MI_EINVAL;
        }
    }
    return 0;
}

std::vector<cd> phase_tables_host(int nx, int ny, int nz, int n_atoms, const double* positions_h) {
    const int dims[3] = {nx, ny, nz};
    std::vector<cd> tab((size_t)n_atoms * ((size_t)nx + ny + nz));
    cd* t = tab.data();
    for (int a = 0; a < n_atoms; ++a)
        for (int d = 0; d < 3; ++d)
            for (int i = 0; i < dims[d]; ++i) {
                const double ph = -2.0 * M_PI * (double)signed_freq(i, dims[d]) * positions_h[3 * a + d];
                *t++ = make_double2(cos(ph), sin(ph));
            }
    return tab;
}

// par_h: 8 parameters per species on the host (kind 0 / 1), or, with ff_d given, nothing: the form factors come from
// the device table ff_d[species][N] and coef_h (nullable) holds one amplitude per atom
static int atomic_superposition_impl(dftk_mi_kblock* cube_kb, int kind, const double* recip_h, int n_species,
                                     const double* par_h, const double* ff_d, const double* coef_h, int n_atoms,
                                     const int* species_of_atom_h, const double* positions_h, double* out_d) {
    dftk_mi_basis* b = cube_kb->basis;
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("atomic_superposition: the k-block must span the whole cube");
        return DFTK_MI_EINVAL;
    }
    CHK(check_species_grouped("atomic_superposition", n_species, n_atoms, species_of_atom_h));
    std::vector<AtomPar> atoms(n_atoms);
    for (int a = 0; a < n_atoms; ++a)
        atoms[a] = AtomPar{positions_h[3 * a], positions_h[3 * a + 1], positions_h[3 * a + 2], species_of_atom_h[a]};
    CHK(scratch_grow(b, b->dense_ws, 2 * (size_t)N * sizeof(cd)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + N;
    const size_t tab = (size_t)n_atoms * sizeof(AtomPar) +
                       std::max((size_t)n_species * 8, (size_t)n_atoms) * sizeof(double);   // parameters or amplitudes
    CHK(ensure_ws(b, tab));
    AtomPar* d_atoms = reinterpret_cast<AtomPar*>(b->ws.get());
    double* d_par = reinterpret_cast<double*>(d_atoms + n_atoms);
    HIPCHK(hipMemcpyAsync(d_atoms, atoms.data(), (size_t)n_atoms * sizeof(AtomPar), hipMemcpyHostToDevice, b->stream));
    if (ff_d) {
        if (coef_h)
            HIPCHK(hipMemcpyAsync(d_par, coef_h, (size_t)n_atoms * sizeof(double), hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_atomic_sum<true>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, b->nx, b->ny,
                           b->nz, make_mat3(recip_h), kind, n_atoms, d_atoms, ff_d,
                           coef_h ? (const double*)d_par : (const double*)nullptr, 1.0 / sqrt(b->volume), c1);
    } else {
        HIPCHK(hipMemcpyAsync(d_par, par_h, (size_t)n_species * 8 * sizeof(double), hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_atomic_sum<false>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, b->nx, b->ny,
                           b->nz, make_mat3(recip_h), kind, n_atoms, d_atoms, d_par, (const double*)nullptr,
                           1.0 / sqrt(b->volume), c1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));      // host tables and b->ws are free again (the FFT below reuses ws-free paths)
    CHK(launch_ifft_to_cube(cube_kb, c1, c2));
    hipLaunchKernelGGL(k_real_part_scaled, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, N, c2,
                       1.0 / sqrt(b->volume), out_d);   // ifft_normalization (fft.jl:87)
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

int atomic_superposition(dftk_mi_kblock* cube_kb, int kind, const double* recip_h, int n_species, const double* par_h,
                         int n_atoms, const int* species_of_atom_h, const double* positions_h, double* out_d) {
    return atomic_superposition_impl(cube_kb, kind, recip_h, n_species, par_h, nullptr, nullptr, n_atoms,
                                     species_of_atom_h, positions_h, out_d);
}

int atomic_superposition_table(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* ff_d,
                               int n_atoms, const int* species_of_atom_h, const double* positions_h,
                               const double* coef_h, double* out_d) {
    return atomic_superposition_impl(cube_kb, 0, recip_h, n_species, nullptr, ff_d, coef_h, n_atoms, species_of_atom_h,
                                     positions_h, out_d);
}
