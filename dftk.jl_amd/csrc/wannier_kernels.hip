// wannier_kernels.hip -- the two n_G-sized passes of the Wannier90 interface (reference: src/external/wannier_shared.jl).
//
//   dftk_mi_wannier_overlaps        overlap_Mmn_k_kpb (:220-241) of one k-point with ALL its neighbours: M^{k,b}[m, n] =
//       sum_G conj(u_mk(G)) u_n,k+b(G + G_shift).  The reference searches the partner of every plane wave with
//       index_G_vectors and then runs a scalar double loop over the bands.  Here the partner look-up goes through the
//       neighbour block's inverse cube -> row map (d_inv, the map of dftk_mi_transfer_blochwave) INSIDE the product kernel:
//       a workgroup owns one WT x WT tile of one neighbour's matrix, a thread finds the partner of its row once, loads WT
//       coefficients of either side and updates WT^2 accumulators; rows are dealt to the threads in a fixed stride and the
//       partial sums are added in a fixed order (wave shuffle tree, then the four waves in order).  The aligned panel of the
//       neighbours is therefore never written to memory, there is one launch per WN_MAX_NB neighbours whatever the number
//       of bands, no workspace, no host synchronisation, and results repeat bit for bit.  (n_bands is the number of
//       Wannierised bands, tens at most: the n_bands x n_bands tiles are far below the 128-row tiles of the matrix-core
//       zgemm, whose launch count also depends on the shape; the kernel is bound by the reads of the orbital blocks.)
//   dftk_mi_wannier_guess_columns   the guess orbitals g_n(k + G) of compute_amn_kpoint (:278-298) for all projections of a
//       k-point in one launch per WN_MAX_COLS columns: centre phase e^{-2 pi i p.c} times either the closed-form Gaussian
//       exp(-pi |p_cart|^2 / 2) (:13-22) or (-i)^l R_lm(p_cart) T(|p_cart|) / 4 pi, where R_lm = |p|^l Y_lm is the real solid
//       harmonic of hgh_forms.h (the reference's ylm_real convention) and T the kind-0 value of dftk_mi_radial_transform of
//       the radial function -- the reference's sum_r w f j_l(|p| r) is T |p|^l / 4 pi, so the product is its :55-70 and is an
//       exact zero at p = 0 for l > 0.  Optionally followed by the column normalisation (:291) with the library's column
//       norms.
#include "common.h"
#include "batch.h"
#include "hgh_forms.h"
#include <cmath>
#include <vector>

namespace dftk_wannier {
const int WN_NT = 256;          // threads of a workgroup
const int WT = 4;               // bands per tile side
const int WN_MAX_NB = 16;       // neighbours per launch (their descriptors travel as kernel arguments)
const int WN_MAX_COLS = 32;     // guess columns per launch (likewise)

struct NbDesc {                 // one neighbour
    const int32_t* inv;         // its inverse cube -> row map
    const cd* psi;              // its orbitals, column-major
    int64_t ld, n_G;
    int nx, ny, nz;
    int dG[3];
};
struct NbList {
    NbDesc d[WN_MAX_NB];
};

// grid (ceil(nb / WT) column tiles, ceil(nb / WT) row tiles, neighbours of this launch)
__global__ __launch_bounds__(WN_NT) void k_wannier_overlaps(int64_t n_G, const int32_t* __restrict__ G3, int nb,
                                                            const cd* __restrict__ psi, int64_t ld, NbList nbs, int j0,
                                                            cd* __restrict__ M) {
    __shared__ double sh[WN_NT / 64];
    const NbDesc& q = nbs.d[blockIdx.z];
    const int n0 = blockIdx.x * WT, m0 = blockIdx.y * WT;
    double ar[WT][WT], ai[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) ar[i][j] = ai[i][j] = 0.0;
    for (int64_t r = threadIdx.x; r < n_G; r += WN_NT) {
        const int g0 = G3[3 * r] + q.dG[0], g1 = G3[3 * r + 1] + q.dG[1], g2 = G3[3 * r + 2] + q.dG[2];
        const int64_t lin = dftk_transfer::cube_index(g0, g1, g2, q.nx, q.ny, q.nz);
        if (lin < 0) continue;
        const int64_t p = q.inv[lin];
        if (p < 0 || p >= q.n_G) continue;
        cd a[WT], c[WT];
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            a[i] = m0 + i < nb ? psi[r + (int64_t)(m0 + i) * ld] : make_double2(0.0, 0.0);
            c[i] = n0 + i < nb ? q.psi[p + (int64_t)(n0 + i) * q.ld] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j) {      // conj(a) c
                ar[i][j] += a[i].x * c[j].x + a[i].y * c[j].y;
                ai[i][j] += a[i].x * c[j].y - a[i].y * c[j].x;
            }
    }
    const int64_t col0 = (int64_t)(j0 + blockIdx.z) * nb;
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const double re = block_sum<WN_NT>(ar[i][j], sh);
            const double im = block_sum<WN_NT>(ai[i][j], sh);
            if (threadIdx.x == 0 && m0 + i < nb && n0 + j < nb) M[(m0 + i) + (int64_t)nb * (col0 + n0 + j)] = make_double2(re, im);
        }
}

struct GuessCol {
    double c[3];                // centre, reduced coordinates
    int kind, l, m, chan;       // kind 0: Gaussian; 1: hydrogenic with the radial values of row `chan` of the table
};
struct GuessList {
    GuessCol d[WN_MAX_COLS];
};

// grid (row blocks, columns of this launch)
__global__ __launch_bounds__(WN_NT) void k_wannier_guess(int64_t n_G, const int32_t* __restrict__ G3, Mat3 B, double k0,
                                                         double k1, double k2, GuessList cols, int c0,
                                                         const double* __restrict__ R, int64_t ldR, cd* __restrict__ out,
                                                         int64_t ld_out) {
    const int64_t r = (int64_t)blockIdx.x * WN_NT + threadIdx.x;
    if (r >= n_G) return;
    const GuessCol& g = cols.d[blockIdx.y];
    const double p0 = G3[3 * r] + k0, p1 = G3[3 * r + 1] + k1, p2 = G3[3 * r + 2] + k2;
    double qx, qy, qz, s, c;
    recip_times(B, p0, p1, p2, &qx, &qy, &qz);
    sincospi(-2.0 * (p0 * g.c[0] + p1 * g.c[1] + p2 * g.c[2]), &s, &c);
    double amp, re, im;
    if (g.kind == 0) {
        amp = exp(-0.5 * M_PI * (qx * qx + qy * qy + qz * qz));
        re = amp * c;
        im = amp * s;
    } else {
        double grad[3];
        amp = solid_harmonic(g.l, g.m, qx, qy, qz, grad) * (R[(int64_t)g.chan * ldR + r] * (0.25 / M_PI));
        re = amp * c;
        im = amp * s;
        rotate_minus_i_pow(g.l, &re, &im);
    }
    out[r + (int64_t)(c0 + blockIdx.y) * ld_out] = make_double2(re, im);
}

int refuse(const char* who, const dftk_mi_kblock* kb) {
    if (kb->sh_comm) {
        dftk_set_error("%s: plane-wave sharded k-blocks are not supported", who);
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("%s: not available inside a batched multi-k call", who);
        return DFTK_MI_EINVAL;
    }
    return 0;
}
}   // namespace dftk_wannier
using namespace dftk_wannier;

extern "C" int dftk_mi_wannier_overlaps(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld, int n_nb,
                                        dftk_mi_kblock* const* kb_nb_h, const int* dG_h, const dftk_mi_cplx* const* psi_nb_h,
                                        const int64_t* ld_nb_h, dftk_mi_cplx* M_d) {
    if (!kb || n_bands < 0 || n_nb < 0 || (n_nb > 0 && (!kb_nb_h || !dG_h || !psi_nb_h || !ld_nb_h))) return DFTK_MI_EINVAL;
    CHK(refuse("wannier_overlaps", kb));
    if (ld < kb->n_G || (n_bands > 0 && n_nb > 0 && (!psi_d || !M_d))) {
        dftk_set_error("wannier_overlaps: null block or leading dimension below the %lld rows of the sphere", (long long)kb->n_G);
        return DFTK_MI_EINVAL;
    }
    for (int j = 0; j < n_nb; ++j) {
        const dftk_mi_kblock* q = kb_nb_h[j];
        if (!q) return DFTK_MI_EINVAL;
        CHK(refuse("wannier_overlaps", q));
        if (q->device != kb->device) {
            dftk_set_error("wannier_overlaps: neighbour %d lives on another device", j);
            return DFTK_MI_EINVAL;
        }
        if (ld_nb_h[j] < q->n_G || (n_bands > 0 && !psi_nb_h[j])) {
            dftk_set_error("wannier_overlaps: null block or short leading dimension of neighbour %d (%lld rows)", j,
                           (long long)q->n_G);
            return DFTK_MI_EINVAL;
        }
    }
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    CHK(ensure_G3(kb));
    for (int j = 0; j < n_nb; ++j) CHK(dftk_transfer::ensure_inverse_map(kb_nb_h[j]));
    if (n_bands == 0 || n_nb == 0) return 0;
    // neighbours on other handles (lanes): this stream waits for theirs before the kernels and theirs for this one after
    std::vector<dftk_mi_basis*> others;
    for (int j = 0; j < n_nb; ++j) {
        dftk_mi_basis* o = kb_nb_h[j]->basis;
        bool seen = o == b;
        for (dftk_mi_basis* s : others) seen = seen || s == o;
        if (!seen) others.push_back(o);
    }
    for (dftk_mi_basis* o : others) CHK(dftk_transfer::order_after(b, o));
    {
        ProfScope prof_scope(b, PROF_EW, kb->n_G >= 4096 ? 16.0 * (double)kb->n_G * n_bands * (1.0 + n_nb) : 0.0);
        const unsigned tiles = (unsigned)((n_bands + WT - 1) / WT);
        for (int j0 = 0; j0 < n_nb; j0 += WN_MAX_NB) {
            const int nj = n_nb - j0 < WN_MAX_NB ? n_nb - j0 : WN_MAX_NB;
            NbList L;
            for (int j = 0; j < nj; ++j) {
                const dftk_mi_kblock* q = kb_nb_h[j0 + j];
                NbDesc& d = L.d[j];
                d.inv = q->d_inv.get();
                d.psi = reinterpret_cast<const cd*>(psi_nb_h[j0 + j]);
                d.ld = ld_nb_h[j0 + j];
                d.n_G = q->n_G;
                d.nx = q->basis->nx; d.ny = q->basis->ny; d.nz = q->basis->nz;
                for (int a = 0; a < 3; ++a) d.dG[a] = dG_h[3 * (j0 + j) + a];
            }
            for (int j = nj; j < WN_MAX_NB; ++j) L.d[j] = L.d[0];
            hipLaunchKernelGGL(k_wannier_overlaps, dim3(tiles, tiles, (unsigned)nj), dim3(WN_NT), 0, b->stream, kb->n_G,
                               kb->d_G3.get(), n_bands, reinterpret_cast<const cd*>(psi_d), ld, L, j0,
                               reinterpret_cast<cd*>(M_d));
            HIPCHK(hipGetLastError());
        }
    }
    for (dftk_mi_basis* o : others) CHK(dftk_transfer::order_after(o, b));
    return 0;
}

extern "C" int dftk_mi_wannier_guess_columns(dftk_mi_kblock* kb, const double* recip_lattice_h, const double* kcoord_h,
                                             int n_cols, const int* kind_h, const int* lm_h, const int* chan_h,
                                             const double* centers_h, int n_chan, const double* R_d, int64_t ldR,
                                             int normalize, dftk_mi_cplx* out_d, int64_t ld_out) {
    if (!kb || !recip_lattice_h || !kcoord_h || n_cols < 0 || n_chan < 0) return DFTK_MI_EINVAL;
    if (n_cols > 0 && (!kind_h || !lm_h || !chan_h || !centers_h || !out_d)) return DFTK_MI_EINVAL;
    CHK(refuse("wannier_guess_columns", kb));
    if (ld_out < kb->n_G || (n_chan > 0 && (!R_d || ldR < kb->n_G))) {
        dftk_set_error("wannier_guess_columns: leading dimension below the %lld rows of the sphere", (long long)kb->n_G);
        return DFTK_MI_EINVAL;
    }
    for (int c = 0; c < n_cols; ++c) {
        const int l = lm_h[2 * c], m = lm_h[2 * c + 1];
        const bool ok = kind_h[c] == 0 || (kind_h[c] == 1 && l >= 0 && l <= 3 && m >= -l && m <= l && chan_h[c] >= 0 && chan_h[c] < n_chan);
        if (!ok) {
            dftk_set_error("wannier_guess_columns: column %d: kind %d, (l, m) = (%d, %d), channel %d of %d", c, kind_h[c], l, m,
                           chan_h[c], n_chan);
            return DFTK_MI_EINVAL;
        }
    }
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    CHK(ensure_G3(kb));
    if (n_cols == 0) return 0;
    if (normalize) CHK(ensure_ws(b, (size_t)n_cols * sizeof(double)));
    const Mat3 B = make_mat3(recip_lattice_h);
    cd* out = reinterpret_cast<cd*>(out_d);
    {
        ProfScope prof_scope(b, PROF_EW, kb->n_G >= 4096 ? 16.0 * (double)kb->n_G * n_cols : 0.0);
        for (int c0 = 0; c0 < n_cols; c0 += WN_MAX_COLS) {
            const int nc = n_cols - c0 < WN_MAX_COLS ? n_cols - c0 : WN_MAX_COLS;
            GuessList L;
            for (int c = 0; c < WN_MAX_COLS; ++c) {
                const int s = c0 + (c < nc ? c : 0);
                GuessCol& g = L.d[c];
                for (int a = 0; a < 3; ++a) g.c[a] = centers_h[3 * s + a];
                g.kind = kind_h[s]; g.l = lm_h[2 * s]; g.m = lm_h[2 * s + 1]; g.chan = chan_h[s];
            }
            hipLaunchKernelGGL(k_wannier_guess, dim3((unsigned)((kb->n_G + WN_NT - 1) / WN_NT), (unsigned)nc), dim3(WN_NT), 0,
                               b->stream, kb->n_G, kb->d_G3.get(), B, kcoord_h[0], kcoord_h[1], kcoord_h[2], L, c0, R_d, ldR, out,
                               ld_out);
            HIPCHK(hipGetLastError());
        }
    }
    if (normalize) {
        double* norms = reinterpret_cast<double*>(b->ws.get());
        CHK(ew_colnorms(b, kb->n_G, n_cols, out, ld_out, norms));
        CHK(ew_scale_cols(b, kb->n_G, n_cols, out, ld_out, norms, true));
    }
    return 0;
}
