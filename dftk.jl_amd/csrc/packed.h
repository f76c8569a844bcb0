// packed.h -- the one packed-vector layer under the orbital-space solvers (dm_kernels.hip: L-BFGS, newton_kernels.hip: CG).
//
// A "packed vector" is a list of column-major complex blocks (one per k-point), handed over as host arrays of device
// pointers and leading dimensions.  One grid walks a table of work items over all blocks (built once, at creation), an inner
// product leaves one partial sum per workgroup, and the kernel that needs the scalar sums the partials itself (fixed order,
// every workgroup for itself): no atomics, no host round trip.
// (m_block_sum of mix_kernels.hip, b_block_sum of batch_kernels.hip and block_sum<NT> of common.h associate the wave partials
// differently or return the sum in thread 0 only; repeatability tests pin their bits, so they stay where they are.)
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/dftk_mi355x.h"
#ifndef DFTK_PACKED_HOST_ONLY
#include "common.h"
#include "batch.h"
#endif

void dftk_set_error(const char* fmt, ...);

const int PACKED_NT = 256;        // threads of a workgroup
const int PACKED_CH = 1024;       // rows of one work item (a piece of one column of one block)
const int PACKED_MAXG = 1024;     // workgroups of a launch at most = partial sums of an inner product

struct PackedItem {               // rows [row0, row0 + nrows) of column col of block b; off = position in unpadded packed storage
    int b, col, row0, nrows;
    int64_t off;
};

// The creation-time checks of the block sizes and the item table: block after block, column after column, PACKED_CH rows
// each.  total / total_cols = complex entries / columns of a packed vector, col0[b] = first column of block b in the list
// of all columns.  No HIP call: tools/host_packed_check.cpp compiles this part alone.
inline int packed_items(const char* who, int n_blocks, const int64_t* rows, const int* cols, std::vector<PackedItem>* items,
                        int64_t* total, int64_t* total_cols, std::vector<int64_t>* col0) {
    for (int i = 0; i < n_blocks; ++i)
        if (rows[i] < 1 || rows[i] > INT32_MAX - PACKED_CH || cols[i] < 1) {
            dftk_set_error("%s: block %d is %lld x %d", who, i, (long long)rows[i], cols[i]);
            return DFTK_MI_EINVAL;
        }
    items->clear(), col0->clear();
    *total = *total_cols = 0;
    for (int i = 0; i < n_blocks; ++i) {
        col0->push_back(*total_cols);
        for (int c = 0; c < cols[i]; ++c)
            for (int64_t r0 = 0; r0 < rows[i]; r0 += PACKED_CH)
                items->push_back(PackedItem{i, c, (int)r0, (int)std::min<int64_t>(PACKED_CH, rows[i] - r0),
                                            *total + (int64_t)c * rows[i] + r0});
        *total += rows[i] * cols[i];
        *total_cols += cols[i];
    }
    if (items->size() > (size_t)INT32_MAX) {
        dftk_set_error("%s: too many work items", who);
        return DFTK_MI_EINVAL;
    }
    return 0;
}

#ifndef DFTK_PACKED_HOST_ONLY
// every vector of a call: a non-null pointer table and block pointers, leading dimensions not below the rows of creation
inline int packed_check(const char* who, int n_blocks, const int64_t* rows, const int* cols, int n_vec,
                        const dftk_mi_cplx* const* const* ptr, const int64_t* const* ld) {
    for (int v = 0; v < n_vec; ++v) {
        if (!ptr[v] || !ld[v]) {
            dftk_set_error("%s: null block table", who);
            return DFTK_MI_EINVAL;
        }
        for (int i = 0; i < n_blocks; ++i)
            if (!ptr[v][i] || ld[v][i] < rows[i]) {
                dftk_set_error("%s: block %d does not match the %lld x %d block given at creation", who, i,
                               (long long)rows[i], cols[i]);
                return DFTK_MI_EINVAL;
            }
    }
    if (batching()) {
        dftk_set_error("%s: not available inside a batched multi-k call", who);
        return DFTK_MI_EINVAL;
    }
    return 0;
}

// what a solver handle keeps of its packed vectors: the block sizes and the device copy of the item table
struct PackedTable {
    int n_blocks = 0;
    std::vector<int64_t> rows, col0;
    std::vector<int> cols;
    int64_t total = 0, total_cols = 0;
    int n_items = 0, grid = 0;
    DevTable<PackedItem> items;

    // the first half of a create entry; the caller then allocates `items` with its other buffers and calls upload()
    int build(const char* who, dftk_mi_basis* b, int n, const int64_t* rows_h, const int* cols_h, std::vector<PackedItem>* host) {
        CHK(packed_items(who, n, rows_h, cols_h, host, &total, &total_cols, &col0));
        if (batching()) {
            dftk_set_error("%s: not available inside a batched multi-k call", who);
            return DFTK_MI_EINVAL;
        }
        HIPCHK(hipSetDevice(b->device));
        n_blocks = n;
        rows.assign(rows_h, rows_h + n);
        cols.assign(cols_h, cols_h + n);
        n_items = (int)host->size();
        grid = std::min(n_items, PACKED_MAXG);
        return 0;
    }
    int upload(dftk_mi_basis* b, const std::vector<PackedItem>& host) {
        HIPCHK(hipMemcpyAsync(items.get(), host.data(), host.size() * sizeof(PackedItem), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));       // (host leaves scope with the caller)
        return 0;
    }
};

// the destroy entry of a solver handle (borrowed basis `b`): nothing of the handle is freed under a running kernel
template <class Handle>
int packed_destroy(Handle* a) {
    if (!a) return 0;
    (void)hipSetDevice(a->b->device);
    (void)hipStreamSynchronize(a->b->stream);
    delete a;
    return 0;
}

// The parameters of a call travel through pinned memory into a device table, DEPTH of each, used in turn.  A pinned buffer
// must not be rewritten while its copy is in flight: begin() waits (and counts the wait) if the slot's event is still pending.
template <int DEPTH>
struct ParamRing {
    PinnedBuf<char> stage[DEPTH];
    DevTable<char> params[DEPTH];
    EventOwner ev[DEPTH];
    bool ev_pending[DEPTH] = {};
    int turn = 0, cur = 0;
    size_t bytes = 0;

    bool alloc(size_t n) {
        bytes = n;
        for (int t = 0; t < DEPTH; ++t)
            if (stage[t].alloc(n) != hipSuccess || params[t].alloc(n) != hipSuccess ||
                hipEventCreateWithFlags(&ev[t].e, hipEventDisableTiming) != hipSuccess) return false;
        return true;
    }
    // the next slot: *host to be filled by the caller, *dev where commit() will have put it
    int begin(char** host, char** dev) {
        cur = turn;
        turn = (turn + 1) % DEPTH;
        if (ev_pending[cur] && hipEventQuery(ev[cur].e) != hipSuccess) {
            g_dftk_host_syncs.fetch_add(1, std::memory_order_relaxed);
            HIPCHK(hipEventSynchronize(ev[cur].e));
        }
        ev_pending[cur] = false;
        *host = stage[cur];
        *dev = params[cur];
        return 0;
    }
    int commit(hipStream_t stream) {
        HIPCHK(hipMemcpyAsync(params[cur].get(), stage[cur].get(), bytes, hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(ev[cur].e, stream));
        ev_pending[cur] = true;
        return 0;
    }
    void all_idle() { std::fill(ev_pending, ev_pending + DEPTH, false); }      // the caller has just waited for the stream
};

// sum over a workgroup of NT = 256 threads, valid in every thread; two barriers, sh[NT / 64] may be reused afterwards
template <int NT>
__device__ __forceinline__ double block_sum_all(double v, double* sh) {
    static_assert(NT == 256, "the association below is that of four waves");
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// the partial sums an earlier launch left, summed in a fixed order by every workgroup for itself
template <int NT>
__device__ __forceinline__ double sum_partials(const double* part, int n, double* sh) {
    double v = 0.0;
    for (int j = threadIdx.x; j < n; j += NT) v += part[j];
    return block_sum_all<NT>(v, sh);
}
#endif
