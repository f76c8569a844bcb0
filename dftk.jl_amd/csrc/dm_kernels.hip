// dm_kernels.hip -- the optimiser of direct_minimization (src/scf/direct_minimization.jl hands it to Optim.jl: L-BFGS on a
// product of Stiefel manifolds) behind the C ABI:
//   dftk_mi_stiefel_project_tangent   G <- G - X (X'G + G'X) / 2, Optim's project_tangent!(Stiefel(), g, x)
//   dftk_mi_lbfgs_*                   a device-resident history of (s, y) pairs and the two-loop recursion d = -H g
// The inner product of two packed vectors (packed.h) is Optim's, sum over the blocks of Re(conj(a) b).  The history and the
// previous point / gradient are stored block after block without padding.
//
// What counts here is passes over the history and host round trips, so one kernel body (k_dm_step) serves every step of
// both loops: it sums the partial inner products the PREVIOUS launch left (fixed order, every workgroup for itself), forms
// its coefficient from them and from rho on the device, applies the axpy, optionally the preconditioner, and leaves the
// partial sums of the NEXT inner product -- each history vector is read once per loop, 2 k + 1 launches for k pairs, no
// host synchronisation, no atomics.  The item table, the partial sums and the parameter ring are those of packed.h.
#include "packed.h"
#include <cmath>
#include <cstring>

namespace {
const int DM_NT = PACKED_NT;

struct DmBlockArgs {          // one block of the caller's vectors for one call (device copy of the call's parameters)
    const cd* p0;             // direction: g          update: x
    int64_t ld0;
    cd* p1;                   // direction: d          update: g (read only)
    int64_t ld1;
    const double* kin;        // kinetic vector of the block, or null (no preconditioner)
    const double* mk;         // mean kinetic energy per column (device), or null
    double scale;
};
enum { DM_NONE = 0, DM_BACK = 1, DM_FWD = 2 };
struct DmStep {
    const PackedItem* items;
    int n_items;
    const DmBlockArgs* blk;
    int src_out;              // 1: the running vector is read from p1 (d, the work vector); 0: from p0 (g)
    const cd* A;              // axpy vector (packed storage), or null
    const cd* B;              // vector of the next inner product (packed storage), or null
    int has_out;              // write the running vector to p1
    int mode, idx;            // DM_BACK: alpha[idx] = rho[idx] <.,.>, v -= alpha A;  DM_FWD: v += (alpha[idx] - rho[idx] <.,.>) A
    const double* rho;        // device, history order
    double* alpha;            // device, history order
    const double* part_in;    // partial sums of <.,.> left by the previous launch
    int n_part_in;
    double* part_out;         // one partial sum per workgroup of <B, v>
    int precond, negate;
};

__global__ __launch_bounds__(DM_NT) void k_dm_step(DmStep a) {
    __shared__ double sh[DM_NT / 64];
    double coef = 0.0;
    if (a.mode != DM_NONE) {
        const double dot = sum_partials<DM_NT>(a.part_in, a.n_part_in, sh);
        const double rho = a.rho[a.idx];
        if (a.mode == DM_BACK) {
            const double al = rho * dot;
            coef = -al;
            if (blockIdx.x == 0 && threadIdx.x == 0) a.alpha[a.idx] = al;
        } else {
            coef = a.alpha[a.idx] - rho * dot;
        }
    }
    double acc = 0.0;
    for (int it = blockIdx.x; it < a.n_items; it += gridDim.x) {
        const PackedItem item = a.items[it];
        const DmBlockArgs bk = a.blk[item.b];
        const cd* src = a.src_out ? (const cd*)bk.p1 + (int64_t)item.col * bk.ld1 + item.row0
                                  : bk.p0 + (int64_t)item.col * bk.ld0 + item.row0;
        cd* dst = bk.p1 + (int64_t)item.col * bk.ld1 + item.row0;
        const cd* Ap = a.A ? a.A + item.off : nullptr;
        const cd* Bp = a.B ? a.B + item.off : nullptr;
        const double mk = (a.precond && bk.kin) ? bk.mk[item.col] : 0.0;
        for (int r = threadIdx.x; r < item.nrows; r += DM_NT) {
            cd v = src[r];
            cd av = make_double2(0.0, 0.0);
            if (Ap) {
                av = Ap[r];
                v.x += coef * av.x;
                v.y += coef * av.y;
            }
            if (a.precond) {
                if (bk.kin) {
                    const double f = mk / (mk + bk.kin[item.row0 + r]);      // PreconditionerTPA ldiv!
                    v.x *= f;
                    v.y *= f;
                }
                v.x /= bk.scale;
                v.y /= bk.scale;
            }
            if (Bp) {
                const cd bv = (Bp == Ap) ? av : Bp[r];
                acc += bv.x * v.x + bv.y * v.y;
            }
            if (a.has_out) dst[r] = a.negate ? make_double2(-v.x, -v.y) : v;
        }
    }
    if (a.B) {
        const double t = block_sum_all<DM_NT>(acc, sh);
        if (threadIdx.x == 0) a.part_out[blockIdx.x] = t;
    }
}

// the fused pass of an update: s = x - x_prev, y = g - g_prev into a slot, (x_prev, g_prev) <- (x, g), partial sums of
// <s, y>.  S == null: the first call, which only stores the point.
__global__ __launch_bounds__(DM_NT) void k_dm_update(const PackedItem* __restrict__ items, int n_items,
                                                     const DmBlockArgs* __restrict__ blk, cd* __restrict__ xp,
                                                     cd* __restrict__ gp, cd* __restrict__ S, cd* __restrict__ Y,
                                                     double* __restrict__ part_out) {
    __shared__ double sh[DM_NT / 64];
    double acc = 0.0;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const PackedItem item = items[it];
        const DmBlockArgs bk = blk[item.b];
        const cd* x = bk.p0 + (int64_t)item.col * bk.ld0 + item.row0;
        const cd* g = (const cd*)bk.p1 + (int64_t)item.col * bk.ld1 + item.row0;
        for (int r = threadIdx.x; r < item.nrows; r += DM_NT) {
            const cd xv = x[r], gv = g[r];
            if (S) {
                const cd xo = xp[item.off + r], go = gp[item.off + r];
                const cd s = make_double2(xv.x - xo.x, xv.y - xo.y), y = make_double2(gv.x - go.x, gv.y - go.y);
                S[item.off + r] = s;
                Y[item.off + r] = y;
                acc += s.x * y.x + s.y * y.y;
            }
            xp[item.off + r] = xv;
            gp[item.off + r] = gv;
        }
    }
    if (S) {
        const double t = block_sum_all<DM_NT>(acc, sh);
        if (threadIdx.x == 0) part_out[blockIdx.x] = t;
    }
}

// S = (W + W') / 2 for the m x m matrix W (both column-major, leading dimension m)
__global__ __launch_bounds__(DM_NT) void k_dm_symmetrize(int m, const cd* __restrict__ W, cd* __restrict__ S) {
    const int64_t t = (int64_t)blockIdx.x * DM_NT + threadIdx.x;
    if (t >= (int64_t)m * m) return;
    const int i = (int)(t % m), j = (int)(t / m);
    const cd a = W[(int64_t)j * m + i], c = W[(int64_t)i * m + j];
    S[t] = make_double2(0.5 * (a.x + c.x), 0.5 * (a.y - c.y));
}
}   // namespace

extern "C" int dftk_mi_stiefel_project_tangent(dftk_mi_basis* b, int64_t n, int m, const dftk_mi_cplx* X_d, int64_t ldx,
                                               dftk_mi_cplx* G_d, int64_t ldg) {
    if (!b || !X_d || !G_d || n < 1 || m < 1 || ldx < n || ldg < n || (const void*)X_d == (const void*)G_d) {
        dftk_set_error("stiefel_project_tangent: needs n >= 1, m >= 1, leading dimensions >= n and two distinct blocks");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("stiefel_project_tangent: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    const cd* X = reinterpret_cast<const cd*>(X_d);
    cd* G = reinterpret_cast<cd*>(G_d);
    cd *W, *S;
    WsCarver ws;
    ws.take(&W, (size_t)m * m), ws.take(&S, (size_t)m * m);
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0}, minus = {-1.0, 0.0};
    CHK(zgemm(b, 'C', m, m, n, one, X, ldx, G, ldg, zero, W, m));
    hipLaunchKernelGGL(k_dm_symmetrize, dim3((unsigned)(((int64_t)m * m + DM_NT - 1) / DM_NT)), dim3(DM_NT), 0, b->stream, m,
                       (const cd*)W, S);
    HIPCHK(hipGetLastError());
    return zgemm(b, 'N', n, m, m, minus, X, ldx, S, m, one, G, ldg);
}

// ====================================================================================================== L-BFGS history
struct dftk_mi_lbfgs {
    dftk_mi_basis* b = nullptr;          // borrowed
    int memory = 0;
    PackedTable tab;
    // memory + 1 slots of (s, y), then x_prev and g_prev: the spare slot takes the candidate pair of an update, so that a
    // rejected pair leaves a full history as it was
    DevBuf<cd> store;
    DevTable<double> coef;               // alpha[memory + 1], then two buffers of PACKED_MAXG partial sums
    ParamRing<2> ring;                   // the parameters of a call: pointer table, mean kinetic energies, rho
    std::vector<int> slots;              // history order (oldest first) -> slot
    std::vector<int> free_slots;
    std::vector<double> rho;             // history order
    bool have_prev = false;

    cd* slot_s(int s) const { return store + 2 * (size_t)s * tab.total; }
    cd* slot_y(int s) const { return store + (2 * (size_t)s + 1) * tab.total; }
    cd* x_prev() const { return store + 2 * (size_t)(memory + 1) * tab.total; }
    cd* g_prev() const { return store + (2 * (size_t)(memory + 1) + 1) * tab.total; }
    double* alpha() const { return coef; }
    double* part(int i) const { return coef + (memory + 1) + (size_t)i * PACKED_MAXG; }
};

namespace {
size_t dm_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the call's parameters into the next slot of the ring; *blk_d / *rho_d = their device addresses.  fill(blk, mk, mk_d) writes
// the host copy.
template <class Fill>
int dm_stage(dftk_mi_lbfgs* a, Fill fill, const DmBlockArgs** blk_d, const double** rho_d) {
    char *h, *d;
    HIPCHK(hipSetDevice(a->b->device));
    CHK(a->ring.begin(&h, &d));
    const size_t off_mk = dm_align((size_t)a->tab.n_blocks * sizeof(DmBlockArgs));
    const size_t off_rho = off_mk + dm_align((size_t)a->tab.total_cols * sizeof(double));
    double* rho = reinterpret_cast<double*>(h + off_rho);
    fill(reinterpret_cast<DmBlockArgs*>(h), reinterpret_cast<double*>(h + off_mk), reinterpret_cast<const double*>(d + off_mk));
    for (size_t i = 0; i < a->rho.size(); ++i) rho[i] = a->rho[i];
    CHK(a->ring.commit(a->b->stream));
    *blk_d = reinterpret_cast<const DmBlockArgs*>(d);
    if (rho_d) *rho_d = reinterpret_cast<const double*>(d + off_rho);
    return 0;
}
}   // namespace

extern "C" int dftk_mi_lbfgs_create(dftk_mi_basis* b, int n_blocks, const int64_t* n_rows_h, const int* n_cols_h, int memory,
                                    dftk_mi_lbfgs** out) {
    if (!b || !out || !n_rows_h || !n_cols_h || n_blocks < 1 || memory < 1) {
        dftk_set_error("lbfgs_create: needs n_blocks >= 1, memory >= 1 and the block sizes");
        return DFTK_MI_EINVAL;
    }
    std::unique_ptr<dftk_mi_lbfgs> a(new dftk_mi_lbfgs());
    std::vector<PackedItem> items;
    CHK(a->tab.build("lbfgs_create", b, n_blocks, n_rows_h, n_cols_h, &items));
    a->b = b;
    a->memory = memory;
    const size_t param_bytes = dm_align((size_t)n_blocks * sizeof(DmBlockArgs)) +
                               dm_align((size_t)a->tab.total_cols * sizeof(double)) +
                               dm_align((size_t)(memory + 1) * sizeof(double));
    if (a->store.alloc((2 * (size_t)(memory + 1) + 2) * (size_t)a->tab.total * sizeof(cd)) != hipSuccess ||
        a->tab.items.alloc(items.size() * sizeof(PackedItem)) != hipSuccess ||
        a->coef.alloc(((size_t)(memory + 1) + 2 * (size_t)PACKED_MAXG) * sizeof(double)) != hipSuccess ||
        !a->ring.alloc(param_bytes)) {
        dftk_set_error("lbfgs_create: cannot allocate %d pairs of %lld complex entries", memory + 1, (long long)a->tab.total);
        return DFTK_MI_EHIP;
    }
    CHK(a->tab.upload(b, items));
    for (int i = memory; i >= 0; --i) a->free_slots.push_back(i);
    *out = a.release();
    return 0;
}

extern "C" int dftk_mi_lbfgs_destroy(dftk_mi_lbfgs* a) { return packed_destroy(a); }

extern "C" int dftk_mi_lbfgs_reset(dftk_mi_lbfgs* a) {
    if (!a) return DFTK_MI_EINVAL;
    for (int s : a->slots) a->free_slots.push_back(s);
    a->slots.clear();
    a->rho.clear();
    a->have_prev = false;
    return 0;
}

extern "C" int dftk_mi_lbfgs_history(const dftk_mi_lbfgs* a) { return a ? (int)a->slots.size() : -1; }

extern "C" int dftk_mi_lbfgs_update(dftk_mi_lbfgs* a, const dftk_mi_cplx* const* x_d, const int64_t* ldx_h,
                                    const dftk_mi_cplx* const* g_d, const int64_t* ldg_h, double* sy_h, int* kept) {
    if (!a || !x_d || !ldx_h || !g_d || !ldg_h || !sy_h || !kept) return DFTK_MI_EINVAL;
    const PackedTable& tab = a->tab;
    const dftk_mi_cplx* const* ptr[2] = {x_d, g_d};
    const int64_t* ld[2] = {ldx_h, ldg_h};
    CHK(packed_check("lbfgs_update", tab.n_blocks, tab.rows.data(), tab.cols.data(), 2, ptr, ld));
    dftk_mi_basis* b = a->b;
    const DmBlockArgs* blk_d = nullptr;
    CHK(dm_stage(a, [&](DmBlockArgs* blk, double*, const double*) {
        for (int i = 0; i < tab.n_blocks; ++i)
            blk[i] = DmBlockArgs{reinterpret_cast<const cd*>(x_d[i]), ldx_h[i],
                                 const_cast<cd*>(reinterpret_cast<const cd*>(g_d[i])), ldg_h[i], nullptr, nullptr, 1.0};
    }, &blk_d, nullptr));
    if (!a->have_prev) {
        hipLaunchKernelGGL(k_dm_update, dim3(tab.grid), dim3(DM_NT), 0, b->stream, (const PackedItem*)tab.items.get(), tab.n_items,
                           blk_d, a->x_prev(), a->g_prev(), (cd*)nullptr, (cd*)nullptr, (double*)nullptr);
        HIPCHK(hipGetLastError());
        a->have_prev = true;
        *sy_h = 0.0;
        *kept = 0;
        return 0;
    }
    const int s = a->free_slots.back();
    double* hpart = reinterpret_cast<double*>(b->h_fetch.get());     // the landing zone: no device -> host blit
    hipLaunchKernelGGL(k_dm_update, dim3(tab.grid), dim3(DM_NT), 0, b->stream, (const PackedItem*)tab.items.get(), tab.n_items,
                       blk_d, a->x_prev(), a->g_prev(), a->slot_s(s), a->slot_y(s), hpart);
    HIPCHK(hipGetLastError());
    CHK(host_wait(b));
    double sy = 0.0;
    for (int i = 0; i < tab.grid; ++i) sy += hpart[i];
    *sy_h = sy;
    if (!(std::isfinite(sy) && sy > 0.0)) {
        *kept = 0;
        return 0;
    }
    a->free_slots.pop_back();
    a->slots.push_back(s);
    a->rho.push_back(1.0 / sy);
    if ((int)a->slots.size() > a->memory) {          // the oldest pair leaves; its slot is the spare one of the next update
        a->free_slots.push_back(a->slots.front());
        a->slots.erase(a->slots.begin());
        a->rho.erase(a->rho.begin());
    }
    *kept = 1;
    return 0;
}

extern "C" int dftk_mi_lbfgs_direction(dftk_mi_lbfgs* a, const dftk_mi_cplx* const* g_d, const int64_t* ldg_h,
                                       dftk_mi_kblock* const* kblocks, const double* const* mean_kin_h, const double* scale_h,
                                       dftk_mi_cplx* const* d_d, const int64_t* ldd_h) {
    if (!a || !g_d || !ldg_h || !scale_h || !d_d || !ldd_h || (kblocks && !mean_kin_h)) return DFTK_MI_EINVAL;
    const PackedTable& tab = a->tab;
    for (int i = 0; i < tab.n_blocks; ++i) {           // beyond packed_check: no aliasing, the k-block, the scale
        if ((const void*)g_d[i] == (const void*)d_d[i] ||
            (kblocks && (!kblocks[i] || !mean_kin_h[i] || kblocks[i]->n_G != tab.rows[i] ||
                         kblocks[i]->basis->device != a->b->device || kblocks[i]->sh_comm))) {
            dftk_set_error("lbfgs_direction: block %d does not match the %lld x %d block given at creation", i,
                           (long long)tab.rows[i], tab.cols[i]);
            return DFTK_MI_EINVAL;
        }
        if (!(scale_h[i] > 0.0) || !std::isfinite(scale_h[i])) {
            dftk_set_error("lbfgs_direction: scale of block %d is %g", i, scale_h[i]);
            return DFTK_MI_EINVAL;
        }
    }
    const dftk_mi_cplx* const* ptr[2] = {g_d, d_d};
    const int64_t* ld[2] = {ldg_h, ldd_h};
    CHK(packed_check("lbfgs_direction", tab.n_blocks, tab.rows.data(), tab.cols.data(), 2, ptr, ld));
    dftk_mi_basis* b = a->b;
    const DmBlockArgs* blk_d = nullptr;
    const double* rho_d = nullptr;
    CHK(dm_stage(a, [&](DmBlockArgs* blk, double* mk, const double* mk_d) {
        for (int i = 0; i < tab.n_blocks; ++i) {
            blk[i] = DmBlockArgs{reinterpret_cast<const cd*>(g_d[i]), ldg_h[i], reinterpret_cast<cd*>(d_d[i]), ldd_h[i],
                                 kblocks ? kblocks[i]->d_kin.get() : nullptr, kblocks ? mk_d + tab.col0[i] : nullptr,
                                 scale_h[i]};
            if (kblocks) std::memcpy(mk + tab.col0[i], mean_kin_h[i], (size_t)tab.cols[i] * sizeof(double));
        }
    }, &blk_d, &rho_d));
    const int k = (int)a->slots.size();
    DmStep st{};
    st.items = tab.items;
    st.n_items = tab.n_items;
    st.blk = blk_d;
    st.rho = rho_d;
    st.alpha = a->alpha();
    int pp = 0;                                        // the partial-sum buffer the next launch writes
    auto launch = [&](int src_out, const cd* A, const cd* B, int has_out, int mode, int idx, int precond, int negate) {
        st.src_out = src_out, st.A = A, st.B = B, st.has_out = has_out, st.mode = mode, st.idx = idx;
        st.precond = precond, st.negate = negate;
        st.part_in = a->part(pp ^ 1), st.n_part_in = tab.grid, st.part_out = a->part(pp);
        hipLaunchKernelGGL(k_dm_step, dim3(tab.grid), dim3(DM_NT), 0, b->stream, st);
        pp ^= 1;
    };
    if (k == 0) {
        launch(0, nullptr, nullptr, 1, DM_NONE, 0, 1, 1);                       // d = -P^-1 g
    } else {
        launch(0, nullptr, a->slot_s(a->slots[k - 1]), 0, DM_NONE, 0, 0, 0);    // <s_{k-1}, g>
        for (int i = k - 1; i >= 1; --i)                                        // q -= alpha_i y_i, <s_{i-1}, q>
            launch(i < k - 1, a->slot_y(a->slots[i]), a->slot_s(a->slots[i - 1]), 1, DM_BACK, i, 0, 0);
        // q -= alpha_0 y_0, r = P^-1 q, <y_0, r>
        launch(k > 1, a->slot_y(a->slots[0]), a->slot_y(a->slots[0]), 1, DM_BACK, 0, 1, 0);
        for (int i = 0; i < k; ++i)                                             // r += (alpha_i - beta) s_i, <y_{i+1}, r>
            launch(1, a->slot_s(a->slots[i]), i + 1 < k ? a->slot_y(a->slots[i + 1]) : nullptr, 1, DM_FWD, i, 0, i + 1 == k);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
