// newton_kernels.hip -- the device side of the tangent-space CG of Newton's method (src/scf/newton.jl,
// solve_OmegaPlusK of src/response/hessian.jl:111-176, cg! of src/response/cg.jl) behind the C ABI:
//   dftk_mi_orbitals_realspace   psi_n(r) of every band as full cubes (kept by the caller for a whole solve)
//   dftk_mi_tangent_density      drho += sum_n w_n 2 Re[conj psi_n(r) dpsi_n(r)] from the kept cubes: one transform per band
//   dftk_mi_tangent_potential    out (+)= sphere(FFT(dV psi_n(r))) from the kept cubes: one transform per band
//   dftk_mi_tangent_cg_*         the packed-vector pieces of cg! with alpha and beta formed on the device
//
// psi is fixed for the 10-50 iterations of a solve, so its real-space cubes are transformed once; an application of K then
// costs two 3-D transforms per band (dpsi in, dV psi out) where apply_K of refine.py pays four.  The transforms are the
// k-block's own pruned sphere <-> cube pipelines (launch_ifft_to_cube / launch_fft_from_cube), in launch groups of
// fft_group_size(b) bands; between them run HBM-bound streams in the form of exx_kernels.hip: 256 threads, grid-stride
// loop, one complex fp64 number per 16-byte access, NW_UNR independent loads per operand in flight before the first use.
//
// The CG pieces stand on packed.h (packed vectors, the table of work items, the parameter ring): an inner product leaves
// one partial sum per workgroup in a named slot, and the kernel that needs the scalar sums the partials itself -- alpha and
// beta never visit the host, no atomics.
#include "packed.h"
#include <cmath>

namespace dftk_newton {
const int NW_NT = PACKED_NT;    // threads of a workgroup
const int NW_UNR = 4;
const int NW_MAX_BLOCKS = 4096;
const int NW_RING = 8;          // staging buffers of the CG call parameters, used in turn

// drho[i] += sum_j w[j] 2 Re(conj(psi[j][i]) dpsi[j][i]) over the nb cubes of a launch group (n apart), j ascending: one
// writer per entry, drho read and written once per group
__global__ __launch_bounds__(NW_NT) void k_tangent_density(int64_t n, int nb, const double* __restrict__ w,
                                                           const cd* __restrict__ psi, const cd* __restrict__ dpsi,
                                                           double* __restrict__ drho) {
    const int64_t step = (int64_t)gridDim.x * NW_NT * NW_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * NW_NT * NW_UNR + threadIdx.x; i0 < n; i0 += step) {
        double a[NW_UNR];
#pragma unroll
        for (int u = 0; u < NW_UNR; ++u) a[u] = 0.0;
        for (int j = 0; j < nb; ++j) {
            const cd* p = psi + (int64_t)j * n;
            const cd* d = dpsi + (int64_t)j * n;
            const double wj = 2.0 * w[j];
            cd pv[NW_UNR], dv[NW_UNR];
#pragma unroll
            for (int u = 0; u < NW_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * NW_NT;
                if (i < n) {
                    pv[u] = p[i];
                    dv[u] = d[i];
                }
            }
#pragma unroll
            for (int u = 0; u < NW_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * NW_NT;
                if (i < n) a[u] = fma(wj, fma(pv[u].x, dv[u].x, pv[u].y * dv[u].y), a[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < NW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NW_NT;
            if (i < n) drho[i] += a[u];
        }
    }
}

// prod[j][i] = (scale dV[i]) psi[j][i] for the nb cubes of a launch group: dV is loaded once
__global__ __launch_bounds__(NW_NT) void k_tangent_product(int64_t n, int nb, double scale, const double* __restrict__ dV,
                                                           const cd* __restrict__ psi, cd* __restrict__ prod) {
    const int64_t step = (int64_t)gridDim.x * NW_NT * NW_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * NW_NT * NW_UNR + threadIdx.x; i0 < n; i0 += step) {
        double v[NW_UNR];
#pragma unroll
        for (int u = 0; u < NW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NW_NT;
            v[u] = i < n ? scale * dV[i] : 0.0;
        }
        for (int j = 0; j < nb; ++j) {
            const cd* p = psi + (int64_t)j * n;
            cd* o = prod + (int64_t)j * n;
            cd pv[NW_UNR];
#pragma unroll
            for (int u = 0; u < NW_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * NW_NT;
                if (i < n) pv[u] = p[i];
            }
#pragma unroll
            for (int u = 0; u < NW_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * NW_NT;
                if (i < n) o[i] = make_double2(v[u] * pv[u].x, v[u] * pv[u].y);
            }
        }
    }
}

// W[:, c] = (accumulate ? W[:, c] : 0) + src[:, c]; grid = (row blocks, columns).  Rows beyond n_G of a column (the
// caller's padding) are neither read nor written.
__global__ __launch_bounds__(NW_NT) void k_tangent_store(int64_t n_G, const cd* __restrict__ src, cd* __restrict__ W,
                                                         int64_t ldW, int accumulate) {
    const cd* s = src + (int64_t)blockIdx.y * n_G;
    cd* o = W + (int64_t)blockIdx.y * ldW;
    const int64_t step = (int64_t)gridDim.x * NW_NT * NW_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * NW_NT * NW_UNR + threadIdx.x; i0 < n_G; i0 += step) {
        cd sv[NW_UNR], ov[NW_UNR];
#pragma unroll
        for (int u = 0; u < NW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NW_NT;
            sv[u] = i < n_G ? s[i] : make_double2(0.0, 0.0);
            ov[u] = (accumulate && i < n_G) ? o[i] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < NW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NW_NT;
            if (i < n_G) o[i] = make_double2(ov[u].x + sv[u].x, ov[u].y + sv[u].y);
        }
    }
}

unsigned row_blocks(int64_t n) {
    int64_t rb = (n + (int64_t)NW_NT * NW_UNR - 1) / ((int64_t)NW_NT * NW_UNR);
    return (unsigned)std::min<int64_t>(std::max<int64_t>(rb, 1), NW_MAX_BLOCKS);
}

// the shared refusals of the three transform-side entries
int check_block(const char* who, const dftk_mi_kblock* kb, int n_bands, const void* a, const void* c, int64_t ld) {
    if (!kb || n_bands < 0) {
        dftk_set_error("%s: null k-block or negative band count", who);
        return DFTK_MI_EINVAL;
    }
    if (kb->sh_comm) {
        dftk_set_error("%s: plane-wave sharded k-blocks are not supported", who);
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("%s: not available inside a batched multi-k call", who);
        return DFTK_MI_EINVAL;
    }
    if (n_bands > 0 && (!a || !c)) {
        dftk_set_error("%s: null pointer argument", who);
        return DFTK_MI_EINVAL;
    }
    if (n_bands > 0 && ld < kb->n_G) {
        dftk_set_error("%s: leading dimension below n_G = %lld", who, (long long)kb->n_G);
        return DFTK_MI_EINVAL;
    }
    return 0;
}

// nbb columns of X (ldx apart) to nbb cubes: X itself where it is unpadded, else a copy in `stage` (n_G apart)
int to_cubes(dftk_mi_kblock* kb, const cd* X, int64_t ldx, int nbb, cd* stage, cd* cubes) {
    const cd* c = X;
    if (ldx != kb->n_G) {
        CHK(ew_copy(kb->basis, kb->n_G, nbb, X, ldx, stage, kb->n_G));
        c = stage;
    }
    return launch_ifft_to_cube(kb, c, cubes, nbb);
}
}   // namespace dftk_newton

using namespace dftk_newton;

extern "C" int dftk_mi_orbitals_realspace(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                          dftk_mi_cplx* psi_r_d) {
    CHK(check_block("orbitals_realspace", kb, n_bands, psi_d, psi_r_d, ld_psi));
    if (n_bands == 0) return 0;
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    const int g = std::min(fft_group_size(b), n_bands);
    cd* stage = nullptr;
    WsCarver ws;
    ws.take(&stage, (size_t)g * kb->n_G);
    CHK(scratch_grow(b, b->newton_ws, ws.bytes()));
    ws.bind(b->newton_ws);
    const cd* psi = reinterpret_cast<const cd*>(psi_d);
    cd* out = reinterpret_cast<cd*>(psi_r_d);
    for (int b0 = 0; b0 < n_bands; b0 += g)
        CHK(to_cubes(kb, psi + (int64_t)b0 * ld_psi, ld_psi, std::min(g, n_bands - b0), stage, out + (int64_t)b0 * N));
    return 0;
}

extern "C" int dftk_mi_tangent_density(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_r_d,
                                       const dftk_mi_cplx* dpsi_d, int64_t ld_dpsi, const double* w_h, double* drho_d) {
    CHK(check_block("tangent_density", kb, n_bands, psi_r_d, dpsi_d, ld_dpsi));
    if (n_bands > 0 && (!w_h || !drho_d)) {
        dftk_set_error("tangent_density: null pointer argument");
        return DFTK_MI_EINVAL;
    }
    if (n_bands == 0) return 0;
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    const int g = std::min(fft_group_size(b), n_bands);
    cd *stage = nullptr, *cubes = nullptr;
    double* w_d = nullptr;
    WsCarver ws;
    ws.take(&stage, (size_t)g * kb->n_G);
    ws.take(&cubes, (size_t)g * N);
    ws.take(&w_d, (size_t)n_bands);
    CHK(scratch_grow(b, b->newton_ws, ws.bytes()));
    ws.bind(b->newton_ws);
    // (from the caller's pageable array: staged by the runtime before the call returns)
    HIPCHK(hipMemcpyAsync(w_d, w_h, (size_t)n_bands * sizeof(double), hipMemcpyHostToDevice, b->stream));
    const cd* psi_r = reinterpret_cast<const cd*>(psi_r_d);
    const cd* dpsi = reinterpret_cast<const cd*>(dpsi_d);
    for (int b0 = 0; b0 < n_bands; b0 += g) {
        const int nbb = std::min(g, n_bands - b0);
        bool any = false;
        for (int i = 0; i < nbb && !any; ++i) any = w_h[b0 + i] != 0.0;
        if (!any) continue;         // a group without weight adds nothing: no transform, drho not touched
        CHK(to_cubes(kb, dpsi + (int64_t)b0 * ld_dpsi, ld_dpsi, nbb, stage, cubes));
        hipLaunchKernelGGL(k_tangent_density, dim3(row_blocks(N)), dim3(NW_NT), 0, b->stream, N, nbb,
                           (const double*)(w_d + b0), psi_r + (int64_t)b0 * N, (const cd*)cubes, drho_d);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dftk_mi_tangent_potential(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_r_d, const double* dV_d,
                                         dftk_mi_cplx* out_d, int64_t ld_out, int accumulate) {
    CHK(check_block("tangent_potential", kb, n_bands, psi_r_d, out_d, ld_out));
    if (n_bands > 0 && !dV_d) {
        dftk_set_error("tangent_potential: null pointer argument");
        return DFTK_MI_EINVAL;
    }
    if (n_bands == 0) return 0;
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const int64_t N = (int64_t)b->nx * b->ny * b->nz, n_G = kb->n_G;
    const int g = std::min(fft_group_size(b), n_bands);
    cd *coef = nullptr, *cubes = nullptr;
    WsCarver ws;
    ws.take(&coef, (size_t)g * n_G);
    ws.take(&cubes, (size_t)g * N);
    CHK(scratch_grow(b, b->newton_ws, ws.bytes()));
    ws.bind(b->newton_ws);
    const cd* psi_r = reinterpret_cast<const cd*>(psi_r_d);
    cd* out = reinterpret_cast<cd*>(out_d);
    const double scale = 1.0 / (double)N;       // the potential / N, as the H apply binds it (launch_pad_potential)
    const bool direct = ld_out == n_G && !accumulate;
    for (int b0 = 0; b0 < n_bands; b0 += g) {
        const int nbb = std::min(g, n_bands - b0);
        hipLaunchKernelGGL(k_tangent_product, dim3(row_blocks(N)), dim3(NW_NT), 0, b->stream, N, nbb, scale, dV_d,
                           psi_r + (int64_t)b0 * N, cubes);
        cd* o = out + (int64_t)b0 * ld_out;
        CHK(launch_fft_from_cube(kb, cubes, direct ? o : coef, nbb));
        if (!direct)
            hipLaunchKernelGGL(k_tangent_store, dim3(row_blocks(n_G), (unsigned)nbb), dim3(NW_NT), 0, b->stream, n_G,
                               (const cd*)coef, o, ld_out, accumulate ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ====================================================================================================== packed-vector CG
namespace dftk_newton {
struct CgBlock {              // one block of the caller's vectors for one call (device copy of the call's parameters)
    const cd* a;              // dot: a          update_xr: p          update_p: z
    int64_t lda;
    const cd* c;              // dot: b          update_xr: c
    int64_t ldc;
    cd* x;                    //                 update_xr: x          update_p: p
    int64_t ldx;
    cd* r;                    //                 update_xr: r
    int64_t ldr;
    double w;                 // weight of the block in the inner product
};

// part_out[workgroup] = sum over its items of w_b sum_rows Re(conj(a) b)
__global__ __launch_bounds__(NW_NT) void k_cg_dot(const PackedItem* __restrict__ items, int n_items,
                                                  const CgBlock* __restrict__ blk, double* __restrict__ part_out) {
    __shared__ double sh[NW_NT / 64];
    double acc = 0.0;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const PackedItem item = items[it];
        const CgBlock bk = blk[item.b];
        const cd* a = bk.a + (int64_t)item.col * bk.lda + item.row0;
        const cd* c = bk.c + (int64_t)item.col * bk.ldc + item.row0;
        double s = 0.0;
        for (int r = threadIdx.x; r < item.nrows; r += NW_NT) {
            const cd av = a[r], cv = c[r];
            s += av.x * cv.x + av.y * cv.y;
        }
        acc += bk.w * s;
    }
    const double t = block_sum_all<NW_NT>(acc, sh);
    if (threadIdx.x == 0) part_out[blockIdx.x] = t;
}

// alpha = <r, z> / <p, c> from the partial sums of both; x += alpha p, r -= alpha c
__global__ __launch_bounds__(NW_NT) void k_cg_update_xr(const PackedItem* __restrict__ items, int n_items,
                                                        const CgBlock* __restrict__ blk, const double* __restrict__ part_g,
                                                        const double* __restrict__ part_pc, int n_part) {
    __shared__ double sh[NW_NT / 64];
    const double gamma = sum_partials<NW_NT>(part_g, n_part, sh);
    const double pc = sum_partials<NW_NT>(part_pc, n_part, sh);
    const double alpha = gamma / pc;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const PackedItem item = items[it];
        const CgBlock bk = blk[item.b];
        const cd* p = bk.a + (int64_t)item.col * bk.lda + item.row0;
        const cd* c = bk.c + (int64_t)item.col * bk.ldc + item.row0;
        cd* x = bk.x + (int64_t)item.col * bk.ldx + item.row0;
        cd* rr = bk.r + (int64_t)item.col * bk.ldr + item.row0;
        for (int r = threadIdx.x; r < item.nrows; r += NW_NT) {
            const cd pv = p[r], cv = c[r];
            cd xv = x[r], rv = rr[r];
            xv.x = fma(alpha, pv.x, xv.x);
            xv.y = fma(alpha, pv.y, xv.y);
            rv.x = fma(-alpha, cv.x, rv.x);
            rv.y = fma(-alpha, cv.y, rv.y);
            x[r] = xv;
            rr[r] = rv;
        }
    }
}

// beta = gamma_new / gamma_old from the partial sums of both; p = z + beta p (first: p = z, p is not read)
__global__ __launch_bounds__(NW_NT) void k_cg_update_p(const PackedItem* __restrict__ items, int n_items,
                                                       const CgBlock* __restrict__ blk, const double* __restrict__ part_new,
                                                       const double* __restrict__ part_old, int n_part, int first) {
    __shared__ double sh[NW_NT / 64];
    double beta = 0.0;
    if (!first) {
        const double g_new = sum_partials<NW_NT>(part_new, n_part, sh);
        const double g_old = sum_partials<NW_NT>(part_old, n_part, sh);
        beta = g_new / g_old;
    }
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const PackedItem item = items[it];
        const CgBlock bk = blk[item.b];
        const cd* z = bk.a + (int64_t)item.col * bk.lda + item.row0;
        cd* p = bk.x + (int64_t)item.col * bk.ldx + item.row0;
        for (int r = threadIdx.x; r < item.nrows; r += NW_NT) {
            cd v = z[r];
            if (!first) {
                const cd pv = p[r];
                v.x = fma(beta, pv.x, v.x);
                v.y = fma(beta, pv.y, v.y);
            }
            p[r] = v;
        }
    }
}

// out[0 .. 3) = the sums of three slots of partials (one workgroup; out is the host-visible landing zone)
__global__ __launch_bounds__(NW_NT) void k_cg_read(const double* __restrict__ p0, const double* __restrict__ p1,
                                                   const double* __restrict__ p2, int n_part, double* __restrict__ out) {
    __shared__ double sh[NW_NT / 64];
    const double a = sum_partials<NW_NT>(p0, n_part, sh);
    const double c = sum_partials<NW_NT>(p1, n_part, sh);
    const double d = sum_partials<NW_NT>(p2, n_part, sh);
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = c;
        out[2] = d;
    }
}
}   // namespace dftk_newton

struct dftk_mi_tangent_cg {
    dftk_mi_basis* b = nullptr;          // borrowed
    PackedTable tab;
    std::vector<double> weight;
    // four buffers of PACKED_MAXG partial sums: gamma (two, used in turn: the one a dot of slot GAMMA writes is the NEXT gamma
    // until update_p has used both), <p, c> and <r, r>
    DevTable<double> part;
    int cur = 0;                         // the gamma buffer that holds the current gamma
    ParamRing<NW_RING> ring;             // the parameters of a call: the block table (a _read in between frees every slot)

    double* gamma(int i) const { return part + (size_t)i * PACKED_MAXG; }
    double* pc() const { return part + 2 * (size_t)PACKED_MAXG; }
    double* rr() const { return part + 3 * (size_t)PACKED_MAXG; }
};

namespace dftk_newton {
// the call's block table into the next slot of the ring; *blk_d = its device address
template <class Fill>
int cg_stage(dftk_mi_tangent_cg* a, Fill fill, const CgBlock** blk_d) {
    char *h, *d;
    HIPCHK(hipSetDevice(a->b->device));
    CHK(a->ring.begin(&h, &d));
    CgBlock* blk = reinterpret_cast<CgBlock*>(h);
    for (int i = 0; i < a->tab.n_blocks; ++i) {
        blk[i] = CgBlock{};
        blk[i].w = a->weight[i];
        fill(i, blk[i]);
    }
    CHK(a->ring.commit(a->b->stream));
    *blk_d = reinterpret_cast<const CgBlock*>(d);
    return 0;
}

int cg_check(const char* who, const dftk_mi_tangent_cg* a, int n_vec, const dftk_mi_cplx* const* const* ptr,
             const int64_t* const* ld) {
    if (!a) {
        dftk_set_error("%s: null handle", who);
        return DFTK_MI_EINVAL;
    }
    return packed_check(who, a->tab.n_blocks, a->tab.rows.data(), a->tab.cols.data(), n_vec, ptr, ld);
}
inline const cd* ccd(const dftk_mi_cplx* p) { return reinterpret_cast<const cd*>(p); }
inline cd* mcd(const dftk_mi_cplx* p) { return const_cast<cd*>(reinterpret_cast<const cd*>(p)); }
}   // namespace dftk_newton

extern "C" int dftk_mi_tangent_cg_create(dftk_mi_basis* b, int n_blocks, const int64_t* n_rows_h, const int* n_cols_h,
                                         const double* weight_h, dftk_mi_tangent_cg** out) {
    if (!b || !out || !n_rows_h || !n_cols_h || !weight_h || n_blocks < 1) {
        dftk_set_error("tangent_cg_create: needs n_blocks >= 1, the block sizes and the block weights");
        return DFTK_MI_EINVAL;
    }
    for (int i = 0; i < n_blocks; ++i)
        if (!std::isfinite(weight_h[i])) {
            dftk_set_error("tangent_cg_create: block %d is %lld x %d with weight %g", i, (long long)n_rows_h[i], n_cols_h[i],
                           weight_h[i]);
            return DFTK_MI_EINVAL;
        }
    std::unique_ptr<dftk_mi_tangent_cg> a(new dftk_mi_tangent_cg());
    std::vector<PackedItem> items;
    CHK(a->tab.build("tangent_cg_create", b, n_blocks, n_rows_h, n_cols_h, &items));
    a->b = b;
    a->weight.assign(weight_h, weight_h + n_blocks);
    if (a->tab.items.alloc(items.size() * sizeof(PackedItem)) != hipSuccess ||
        a->part.alloc(4 * (size_t)PACKED_MAXG * sizeof(double)) != hipSuccess ||
        !a->ring.alloc((size_t)n_blocks * sizeof(CgBlock))) {
        dftk_set_error("tangent_cg_create: cannot allocate the tables of %d blocks", n_blocks);
        return DFTK_MI_EHIP;
    }
    HIPCHK(hipMemsetAsync(a->part.get(), 0, 4 * (size_t)PACKED_MAXG * sizeof(double), b->stream));
    CHK(a->tab.upload(b, items));
    *out = a.release();
    return 0;
}

extern "C" int dftk_mi_tangent_cg_destroy(dftk_mi_tangent_cg* a) { return packed_destroy(a); }

extern "C" int dftk_mi_tangent_cg_dot(dftk_mi_tangent_cg* a, int slot, const dftk_mi_cplx* const* a_d, const int64_t* lda_h,
                                      const dftk_mi_cplx* const* b_d, const int64_t* ldb_h) {
    const dftk_mi_cplx* const* ptr[2] = {a_d, b_d};
    const int64_t* ld[2] = {lda_h, ldb_h};
    CHK(cg_check("tangent_cg_dot", a, 2, ptr, ld));
    if (slot < DFTK_MI_CG_GAMMA || slot > DFTK_MI_CG_RR) {
        dftk_set_error("tangent_cg_dot: slot %d is none of GAMMA, PC, RR", slot);
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis* b = a->b;
    const CgBlock* blk_d = nullptr;
    CHK(cg_stage(a, [&](int i, CgBlock& k) {
        k.a = ccd(a_d[i]), k.lda = lda_h[i], k.c = ccd(b_d[i]), k.ldc = ldb_h[i];
    }, &blk_d));
    double* part = slot == DFTK_MI_CG_GAMMA ? a->gamma(a->cur ^ 1) : slot == DFTK_MI_CG_PC ? a->pc() : a->rr();
    hipLaunchKernelGGL(k_cg_dot, dim3(a->tab.grid), dim3(NW_NT), 0, b->stream, (const PackedItem*)a->tab.items.get(),
                       a->tab.n_items, blk_d, part);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dftk_mi_tangent_cg_update_xr(dftk_mi_tangent_cg* a, const dftk_mi_cplx* const* p_d, const int64_t* ldp_h,
                                            const dftk_mi_cplx* const* c_d, const int64_t* ldc_h, dftk_mi_cplx* const* x_d,
                                            const int64_t* ldx_h, dftk_mi_cplx* const* r_d, const int64_t* ldr_h) {
    const dftk_mi_cplx* const* ptr[4] = {p_d, c_d, x_d, r_d};
    const int64_t* ld[4] = {ldp_h, ldc_h, ldx_h, ldr_h};
    CHK(cg_check("tangent_cg_update_xr", a, 4, ptr, ld));
    dftk_mi_basis* b = a->b;
    const CgBlock* blk_d = nullptr;
    CHK(cg_stage(a, [&](int i, CgBlock& k) {
        k.a = ccd(p_d[i]), k.lda = ldp_h[i], k.c = ccd(c_d[i]), k.ldc = ldc_h[i];
        k.x = mcd(x_d[i]), k.ldx = ldx_h[i], k.r = mcd(r_d[i]), k.ldr = ldr_h[i];
    }, &blk_d));
    hipLaunchKernelGGL(k_cg_update_xr, dim3(a->tab.grid), dim3(NW_NT), 0, b->stream, (const PackedItem*)a->tab.items.get(),
                       a->tab.n_items, blk_d, (const double*)a->gamma(a->cur), (const double*)a->pc(), a->tab.grid);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dftk_mi_tangent_cg_update_p(dftk_mi_tangent_cg* a, const dftk_mi_cplx* const* z_d, const int64_t* ldz_h,
                                           dftk_mi_cplx* const* p_d, const int64_t* ldp_h, int first) {
    const dftk_mi_cplx* const* ptr[2] = {z_d, p_d};
    const int64_t* ld[2] = {ldz_h, ldp_h};
    CHK(cg_check("tangent_cg_update_p", a, 2, ptr, ld));
    dftk_mi_basis* b = a->b;
    const CgBlock* blk_d = nullptr;
    CHK(cg_stage(a, [&](int i, CgBlock& k) {
        k.a = ccd(z_d[i]), k.lda = ldz_h[i], k.x = mcd(p_d[i]), k.ldx = ldp_h[i];
    }, &blk_d));
    hipLaunchKernelGGL(k_cg_update_p, dim3(a->tab.grid), dim3(NW_NT), 0, b->stream, (const PackedItem*)a->tab.items.get(),
                       a->tab.n_items, blk_d, (const double*)a->gamma(a->cur ^ 1), (const double*)a->gamma(a->cur), a->tab.grid,
                       first ? 1 : 0);
    HIPCHK(hipGetLastError());
    a->cur ^= 1;                                   // the gamma of the last dot is the current one from here on
    return 0;
}

extern "C" int dftk_mi_tangent_cg_read(dftk_mi_tangent_cg* a, double* out3_h) {
    if (!a || !out3_h) {
        dftk_set_error("tangent_cg_read: null argument");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("tangent_cg_read: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis* b = a->b;
    HIPCHK(hipSetDevice(b->device));
    double* land = reinterpret_cast<double*>(b->h_fetch.get());     // the landing zone: no device -> host blit
    hipLaunchKernelGGL(k_cg_read, dim3(1), dim3(NW_NT), 0, b->stream, (const double*)a->rr(), (const double*)a->gamma(a->cur),
                       (const double*)a->pc(), a->tab.grid, land);
    HIPCHK(hipGetLastError());
    CHK(host_wait(b));
    a->ring.all_idle();                            // the stream is idle: every staging buffer is free
    out3_h[0] = land[0], out3_h[1] = land[1], out3_h[2] = land[2];
    return 0;
}
