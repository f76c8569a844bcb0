// dm_kernels.hip -- the optimiser of direct_minimization (src/scf/direct_minimization.jl hands it to Optim.jl: L-BFGS on a
// product of Stiefel manifolds) behind the C ABI:
//   dftk_mi_stiefel_project_tangent   G <- G - X (X'G + G'X) / 2, Optim's project_tangent!(Stiefel(), g, x)
//   dftk_mi_lbfgs_*                   a device-resident history of (s, y) pairs and the two-loop recursion d = -H g
// A "packed vector" is a list of column-major complex blocks (one per k-point), handed over as host arrays of device
// pointers and leading dimensions; the inner product is Optim's, sum over the blocks of Re(conj(a) b).  The history and the
// previous point / gradient are stored block after block without padding.
//
// What counts here is passes over the history and host round trips, so one kernel body (k_dm_step) serves every step of
// both loops: it sums the partial inner products the PREVIOUS launch left (fixed order, every workgroup for itself), forms
// its coefficient from them and from rho on the device, applies the axpy, optionally the preconditioner, and leaves the
// partial sums of the NEXT inner product -- each history vector is read once per loop, 2 k + 1 launches for k pairs, no
// host synchronisation, no atomics.  One grid covers all blocks through a table of work items built at creation.
#include "common.h"
#include "batch.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
const int DM_NT = 256;        // threads of a workgroup
const int DM_CH = 1024;       // rows of one work item (a piece of one column of one block)
const int DM_MAXG = 1024;     // workgroups of a launch at most = partial sums of an inner product

struct DmItem {               // rows [row0, row0 + nrows) of column col of block b; off = position in the packed storage
    int b, col, row0, nrows;
    int64_t off;
};
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
    const DmItem* items;
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

// sum over the workgroup, valid in every thread; two barriers, sh may be reused afterwards
__device__ __forceinline__ double dm_block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(DM_NT) void k_dm_step(DmStep a) {
    __shared__ double sh[DM_NT / 64];
    double coef = 0.0;
    if (a.mode != DM_NONE) {
        double v = 0.0;
        for (int j = threadIdx.x; j < a.n_part_in; j += DM_NT) v += a.part_in[j];
        const double dot = dm_block_sum(v, sh);
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
        const DmItem item = a.items[it];
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
        const double t = dm_block_sum(acc, sh);
        if (threadIdx.x == 0) a.part_out[blockIdx.x] = t;
    }
}

// the fused pass of an update: s = x - x_prev, y = g - g_prev into a slot, (x_prev, g_prev) <- (x, g), partial sums of
// <s, y>.  S == null: the first call, which only stores the point.
__global__ __launch_bounds__(DM_NT) void k_dm_update(const DmItem* __restrict__ items, int n_items,
                                                     const DmBlockArgs* __restrict__ blk, cd* __restrict__ xp,
                                                     cd* __restrict__ gp, cd* __restrict__ S, cd* __restrict__ Y,
                                                     double* __restrict__ part_out) {
    __shared__ double sh[DM_NT / 64];
    double acc = 0.0;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const DmItem item = items[it];
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
        const double t = dm_block_sum(acc, sh);
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
    int n_blocks = 0, memory = 0;
    std::vector<int64_t> rows;
    std::vector<int> cols;
    std::vector<int64_t> col0;           // first column of block b in the list of all columns
    int64_t total = 0, total_cols = 0;   // complex entries / columns of a packed vector
    int n_items = 0, grid = 0;
    // memory + 1 slots of (s, y), then x_prev and g_prev: the spare slot takes the candidate pair of an update, so that a
    // rejected pair leaves a full history as it was
    DevBuf<cd> store;
    DevTable<DmItem> items;
    DevTable<double> coef;               // alpha[memory + 1], then two buffers of DM_MAXG partial sums
    // the parameters of a call (pointer table, mean kinetic energies, rho) travel through pinned memory into a device table;
    // two of each, used in turn, each guarded by an event recorded behind its copy
    PinnedBuf<char> stage[2];
    DevTable<char> params[2];
    EventOwner ev[2];
    bool ev_pending[2] = {false, false};
    int turn = 0;
    size_t param_bytes = 0;
    std::vector<int> slots;              // history order (oldest first) -> slot
    std::vector<int> free_slots;
    std::vector<double> rho;             // history order
    bool have_prev = false;

    cd* slot_s(int s) const { return store + 2 * (size_t)s * total; }
    cd* slot_y(int s) const { return store + (2 * (size_t)s + 1) * total; }
    cd* x_prev() const { return store + 2 * (size_t)(memory + 1) * total; }
    cd* g_prev() const { return store + (2 * (size_t)(memory + 1) + 1) * total; }
    double* alpha() const { return coef; }
    double* part(int i) const { return coef + (memory + 1) + (size_t)i * DM_MAXG; }
};

namespace {
size_t dm_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the call's parameters into the next staging pair; *blk_d / *mk_d / *rho_d = their device addresses.  fill(blk, mk) writes
// the host copy.  No host synchronisation unless the pair is still in flight from two calls ago.
template <class Fill>
int dm_stage(dftk_mi_lbfgs* a, Fill fill, const DmBlockArgs** blk_d, const double** rho_d) {
    dftk_mi_basis* b = a->b;
    const int t = a->turn;
    a->turn ^= 1;
    if (a->ev_pending[t] && hipEventQuery(a->ev[t].e) != hipSuccess) {
        g_dftk_host_syncs.fetch_add(1, std::memory_order_relaxed);
        HIPCHK(hipEventSynchronize(a->ev[t].e));
    }
    a->ev_pending[t] = false;
    char* h = a->stage[t];
    char* d = a->params[t];
    const size_t off_mk = dm_align((size_t)a->n_blocks * sizeof(DmBlockArgs));
    const size_t off_rho = off_mk + dm_align((size_t)a->total_cols * sizeof(double));
    DmBlockArgs* blk = reinterpret_cast<DmBlockArgs*>(h);
    double* mk = reinterpret_cast<double*>(h + off_mk);
    double* rho = reinterpret_cast<double*>(h + off_rho);
    fill(blk, mk, reinterpret_cast<const double*>(d + off_mk));
    for (size_t i = 0; i < a->rho.size(); ++i) rho[i] = a->rho[i];
    HIPCHK(hipMemcpyAsync(d, h, a->param_bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipEventRecord(a->ev[t].e, b->stream));
    a->ev_pending[t] = true;
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
    for (int i = 0; i < n_blocks; ++i)
        if (n_rows_h[i] < 1 || n_rows_h[i] > INT32_MAX - DM_CH || n_cols_h[i] < 1) {
            dftk_set_error("lbfgs_create: block %d is %lld x %d", i, (long long)n_rows_h[i], n_cols_h[i]);
            return DFTK_MI_EINVAL;
        }
    if (batching()) {
        dftk_set_error("lbfgs_create: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    std::unique_ptr<dftk_mi_lbfgs> a(new dftk_mi_lbfgs());
    a->b = b;
    a->n_blocks = n_blocks;
    a->memory = memory;
    a->rows.assign(n_rows_h, n_rows_h + n_blocks);
    a->cols.assign(n_cols_h, n_cols_h + n_blocks);
    std::vector<DmItem> items;
    for (int i = 0; i < n_blocks; ++i) {
        a->col0.push_back(a->total_cols);
        for (int c = 0; c < a->cols[i]; ++c)
            for (int64_t r0 = 0; r0 < a->rows[i]; r0 += DM_CH)
                items.push_back(DmItem{i, c, (int)r0, (int)std::min<int64_t>(DM_CH, a->rows[i] - r0),
                                       a->total + (int64_t)c * a->rows[i] + r0});
        a->total += a->rows[i] * a->cols[i];
        a->total_cols += a->cols[i];
    }
    if (items.size() > (size_t)INT32_MAX) {
        dftk_set_error("lbfgs_create: too many work items");
        return DFTK_MI_EINVAL;
    }
    a->n_items = (int)items.size();
    a->grid = std::min(a->n_items, DM_MAXG);
    a->param_bytes = dm_align((size_t)n_blocks * sizeof(DmBlockArgs)) + dm_align((size_t)a->total_cols * sizeof(double)) +
                     dm_align((size_t)(memory + 1) * sizeof(double));
    bool ok = a->store.alloc((2 * (size_t)(memory + 1) + 2) * (size_t)a->total * sizeof(cd)) == hipSuccess &&
              a->items.alloc(items.size() * sizeof(DmItem)) == hipSuccess &&
              a->coef.alloc(((size_t)(memory + 1) + 2 * (size_t)DM_MAXG) * sizeof(double)) == hipSuccess;
    for (int t = 0; t < 2 && ok; ++t)
        ok = a->stage[t].alloc(a->param_bytes) == hipSuccess && a->params[t].alloc(a->param_bytes) == hipSuccess &&
             hipEventCreateWithFlags(&a->ev[t].e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        dftk_set_error("lbfgs_create: cannot allocate %d pairs of %lld complex entries", memory + 1, (long long)a->total);
        return DFTK_MI_EHIP;
    }
    HIPCHK(hipMemcpyAsync(a->items.get(), items.data(), items.size() * sizeof(DmItem), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));       // (items leaves scope with the call)
    for (int i = memory; i >= 0; --i) a->free_slots.push_back(i);
    *out = a.release();
    return 0;
}

extern "C" int dftk_mi_lbfgs_destroy(dftk_mi_lbfgs* a) {
    if (!a) return 0;
    (void)hipSetDevice(a->b->device);
    (void)hipStreamSynchronize(a->b->stream);
    delete a;
    return 0;
}

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
    for (int i = 0; i < a->n_blocks; ++i)
        if (!x_d[i] || !g_d[i] || ldx_h[i] < a->rows[i] || ldg_h[i] < a->rows[i]) {
            dftk_set_error("lbfgs_update: block %d does not match the %lld x %d block given at creation", i,
                           (long long)a->rows[i], a->cols[i]);
            return DFTK_MI_EINVAL;
        }
    if (batching()) {
        dftk_set_error("lbfgs_update: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis* b = a->b;
    HIPCHK(hipSetDevice(b->device));
    const DmBlockArgs* blk_d = nullptr;
    CHK(dm_stage(a, [&](DmBlockArgs* blk, double*, const double*) {
        for (int i = 0; i < a->n_blocks; ++i)
            blk[i] = DmBlockArgs{reinterpret_cast<const cd*>(x_d[i]), ldx_h[i],
                                 const_cast<cd*>(reinterpret_cast<const cd*>(g_d[i])), ldg_h[i], nullptr, nullptr, 1.0};
    }, &blk_d, nullptr));
    if (!a->have_prev) {
        hipLaunchKernelGGL(k_dm_update, dim3(a->grid), dim3(DM_NT), 0, b->stream, (const DmItem*)a->items.get(), a->n_items,
                           blk_d, a->x_prev(), a->g_prev(), (cd*)nullptr, (cd*)nullptr, (double*)nullptr);
        HIPCHK(hipGetLastError());
        a->have_prev = true;
        *sy_h = 0.0;
        *kept = 0;
        return 0;
    }
    const int s = a->free_slots.back();
    double* hpart = reinterpret_cast<double*>(b->h_fetch.get());     // the landing zone: no device -> host blit
    hipLaunchKernelGGL(k_dm_update, dim3(a->grid), dim3(DM_NT), 0, b->stream, (const DmItem*)a->items.get(), a->n_items, blk_d,
                       a->x_prev(), a->g_prev(), a->slot_s(s), a->slot_y(s), hpart);
    HIPCHK(hipGetLastError());
    CHK(host_wait(b));
    double sy = 0.0;
    for (int i = 0; i < a->grid; ++i) sy += hpart[i];
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
    for (int i = 0; i < a->n_blocks; ++i) {
        if (!g_d[i] || !d_d[i] || (const void*)g_d[i] == (const void*)d_d[i] || ldg_h[i] < a->rows[i] || ldd_h[i] < a->rows[i] ||
            (kblocks && (!kblocks[i] || !mean_kin_h[i] || kblocks[i]->n_G != a->rows[i] || kblocks[i]->basis->device != a->b->device ||
                         kblocks[i]->sh_comm))) {
            dftk_set_error("lbfgs_direction: block %d does not match the %lld x %d block given at creation", i,
                           (long long)a->rows[i], a->cols[i]);
            return DFTK_MI_EINVAL;
        }
        if (!(scale_h[i] > 0.0) || !std::isfinite(scale_h[i])) {
            dftk_set_error("lbfgs_direction: scale of block %d is %g", i, scale_h[i]);
            return DFTK_MI_EINVAL;
        }
    }
    if (batching()) {
        dftk_set_error("lbfgs_direction: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis* b = a->b;
    HIPCHK(hipSetDevice(b->device));
    const DmBlockArgs* blk_d = nullptr;
    const double* rho_d = nullptr;
    CHK(dm_stage(a, [&](DmBlockArgs* blk, double* mk, const double* mk_d) {
        for (int i = 0; i < a->n_blocks; ++i) {
            blk[i] = DmBlockArgs{reinterpret_cast<const cd*>(g_d[i]), ldg_h[i], reinterpret_cast<cd*>(d_d[i]), ldd_h[i],
                                 kblocks ? kblocks[i]->d_kin.get() : nullptr, kblocks ? mk_d + a->col0[i] : nullptr,
                                 scale_h[i]};
            if (kblocks) std::memcpy(mk + a->col0[i], mean_kin_h[i], (size_t)a->cols[i] * sizeof(double));
        }
    }, &blk_d, &rho_d));
    const int k = (int)a->slots.size();
    DmStep st{};
    st.items = a->items;
    st.n_items = a->n_items;
    st.blk = blk_d;
    st.rho = rho_d;
    st.alpha = a->alpha();
    int pp = 0;                                        // the partial-sum buffer the next launch writes
    auto launch = [&](int src_out, const cd* A, const cd* B, int has_out, int mode, int idx, int precond, int negate) {
        st.src_out = src_out, st.A = A, st.B = B, st.has_out = has_out, st.mode = mode, st.idx = idx;
        st.precond = precond, st.negate = negate;
        st.part_in = a->part(pp ^ 1), st.n_part_in = a->grid, st.part_out = a->part(pp);
        hipLaunchKernelGGL(k_dm_step, dim3(a->grid), dim3(DM_NT), 0, b->stream, st);
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
