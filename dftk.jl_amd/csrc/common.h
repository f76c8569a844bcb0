// common.h -- shared declarations of the MI355X plane-wave SCF hot-path library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <map>
#include <vector>
#include <memory>
#include "devbuf.h"
#include "handover.h"
#include "../../include/dftk_mi355x.h"

typedef double2 cd;   // complex fp64, (x, y) = (re, im); layout-compatible with dftk_mi_cplx

// Every kernel launch of the library is counted (dftk_mi_launch_count): for the many-small-k workloads launches and
// host synchronisations per SCF step ARE the cost model (bench.py --mode kpoints: roofline.bound = "latency").
#include <atomic>
extern std::atomic<int64_t> g_dftk_launches, g_dftk_host_syncs;
inline hipError_t dftk_counted_stream_sync(hipStream_t s) {
    g_dftk_host_syncs.fetch_add(1, std::memory_order_relaxed);
    return (hipStreamSynchronize)(s);
}
#define hipStreamSynchronize(s) dftk_counted_stream_sync(s)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...)                               \
    do {                                                                  \
        g_dftk_launches.fetch_add(1, std::memory_order_relaxed);          \
        hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__);            \
    } while (0)

void dftk_set_error(const char* fmt, ...);
bool land_in_place();   // api.cpp: the switch DFTK_MI_LAND_IN_PLACE (default on)
// hipMalloc for library-owned scratch (behind DevBuf, devbuf.h); DFTK_MI_POISON=1 fills it with 0xFF bytes (NaN doubles) so
// that any read of scratch that was not written in the current call shows up as a non-finite result (debugging aid)
hipError_t dftk_scratch_malloc(void** p, size_t bytes);

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            dftk_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return DFTK_MI_EHIP;                                                          \
        }                                                                                 \
    } while (0)

#define CHK(expr)                                 \
    do {                                          \
        int _s = (expr);                          \
        if (_s != 0) return _s;                   \
    } while (0)

// 256-byte-aligned pieces of one workspace: take() every piece, grow the buffer to bytes(), then bind() sets the pointers
struct WsCarver {
    void** slot[16];
    size_t at[16];
    int n = 0;
    size_t off = 0;
    template <class T>
    void take(T** p, size_t count) {
        slot[n] = reinterpret_cast<void**>(p);
        at[n++] = off;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
    }
    size_t bytes() const { return off; }
    void bind(void* base) const {
        for (int i = 0; i < n; ++i) *slot[i] = static_cast<char*>(base) + at[i];
    }
};

// sum of K values per thread over a workgroup of 256 (shared-memory tree, fixed order); on return v[0 .. K) of thread 0
// holds the totals
template <int K>
__device__ inline void block_reduce(double* v) {
    __shared__ double sh[K][256];
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = sh[k][0];
}

// sum over the 64 lanes of a wave (shuffle-down tree); result valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// sum over a workgroup of NT threads: wave_sum, then thread 0 adds the NT / 64 wave partials sh[0 .. NT / 64) in wave
// order; result valid in thread 0.  Ends with a barrier: sh may be reused at once.
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) r += sh[i];
    }
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------ 1-D plans
#define DFTK_MAX_RADICES 32
struct FftAxis {            // passed to kernels by value
    int n;                  // transform length
    int nrad;               // number of stages
    int rad[DFTK_MAX_RADICES];
    const cd* tw;           // device: tw[t] = exp(+2 pi i t / n), t in [0, n)
    const int* pos;         // device: in-place permutation (see dftk_mi_fft_plan_host)
};

int  plan_radices(int n, int* nrad, int* rad);          // host: factorise into {5,4,3,2,primes}
void plan_positions(int n, int nrad, const int* rad, int* pos);

// ------------------------------------------------------------------------------------ handles
// Ownership: every device / pinned allocation of a handle is a Buf member (devbuf.h) and every host container a plain
// std::vector, so that deleting the handle releases all of it; members commented "borrowed" are raw pointers into memory of
// the caller or of another handle.
struct StreamOwner {     // the basis' stream: declared before every buffer of the basis, so destroyed after them
    hipStream_t s = nullptr;
    StreamOwner() = default;
    StreamOwner(const StreamOwner&) = delete;
    StreamOwner& operator=(const StreamOwner&) = delete;
    ~StreamOwner() { if (s) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct EventOwner {      // one timing-less event, created on first use (transfer_kernels.hip orders two bases' streams with it)
    hipEvent_t e = nullptr;
    EventOwner() = default;
    EventOwner(const EventOwner&) = delete;
    EventOwner& operator=(const EventOwner&) = delete;
    ~EventOwner() { if (e) hipEventDestroy(e); }
};
struct dftk_mi_basis {
    int nx = 0, ny = 0, nz = 0, nxp = 0;   // nxp = nx rounded up to a multiple of FFT_L (padded x pitch)
    double volume = 0.0;
    int device = 0;
    StreamOwner stream;
    EventOwner order_ev;          // recorded on `stream` when another basis' stream has to wait for this one
    FftAxis ax[3] = {};           // x, y, z (tw / pos point into d_tables)
    DevTable<void> d_tables[6];   // device tw/pos buffers
    int fft_batch = 0;            // bands per launch group
    // scratch pool (grown on demand)
    DevBuf<cd> T1;
    DevBuf<cd> T2;
    // general workspace for dense algebra (split-K slabs, small matrices)
    DevBuf<void> ws;
    DevTable<double> d_scalars;   // small device buffer for reductions (256 doubles)
    PinnedBuf<double> h_scalars;  // pinned host mirror
    Buf<char, Mem::PinnedMapped> h_fetch;   // device-visible landing zone of host_fetch() (zero-copy device -> host results)
    int use_mfma = 0;             // 0 => naive GEMM kernels (env DFTK_MI_GEMM=naive)
    std::unique_ptr<struct Prof> prof;      // per-family HIP-event timing (dftk_mi_prof_*)
    // workspace of the dense factorizations (heev ping-pong copies, rotation buffers); owned by the basis so
    // that several bases / devices in one process never share it
    DevBuf<void> dense_ws;
    // workspace of the partial-spectrum eigensolver (eig_kernels.hip): its iterates live across calls into the routines
    // that use dense_ws (Cholesky, Jacobi on the projected matrix), so it cannot share that buffer
    DevBuf<void> eig_ws;
    struct dftk_mi_comm* comm = nullptr;    // plane-wave (row-slab) communicator of a sharded k-block, or null (borrowed)
    // device copy of the symmetry tables of the last cube_symmetrize call (keyed by a hash of the operations: an SCF
    // symmetrises with the same group every step -- no upload and no host synchronisation after the first call)
    DevTable<void> symm_tab; uint64_t symm_key = 0; int symm_n = 0;
    // workspace of the Sternheimer solver (sternheimer.cpp): its blocks live across calls into the H apply (T1 / T2), the
    // zgemm (ws) and nothing of a k-block's LOBPCG state, so it shares none of those buffers
    DevBuf<void> resp_ws;
    // workspace of the exact-exchange apply (exx_kernels.hip): the cubes of the occupied orbitals, of a group of columns
    // and of a group of pair densities live across calls into the sphere <-> cube pipelines (T1 / T2)
    DevBuf<void> exx_ws;
    // workspace of the tangent-space entries (newton_kernels.hip): the cubes and coefficient vectors of one launch group
    // live across calls into the sphere <-> cube pipelines (T1 / T2)
    DevBuf<void> newton_ws;
};

// ------------------------------------------------------------------------------------ profiling
// Kernel families timed with HIP events on the basis' stream (bench.py roofline numbers).
enum ProfFamily {
    PROF_ZGEMM = 0,      // UNSTRUCTURED zgemm calls: work = 8 m n k flops
    PROF_FFT_A = 1,      // x-lines backward + scatter      (work = algorithmic bytes, dense 3-pass convention)
    PROF_FFT_B = 2,      // y backward
    PROF_FFT_C = 3,      // fused z backward * V * z forward
    PROF_FFT_D = 4,      // y forward
    PROF_FFT_E = 5,      // x forward + gather + kinetic
    PROF_DENS_Z = 6,     // z backward + |psi|^2 accumulate
    PROF_HEEV = 7,       // dense Hermitian eigensolver (whole call)
    PROF_CHOL = 8,       // potrf + trtri (whole call)
    PROF_APPLY_H = 9,    // whole dftk_mi_apply_H call (work = bands)
    PROF_ZGEMM_BYTES = 10,   // no timing: work = algorithmic operand bytes of the zgemm calls (A + B + C [+ C if beta != 0])
    PROF_ZGEMM_STRUCT = 11,  // structured calls (UPPER / B_UPPER), timed apart: work = flops of the part of the product
                             // that is mathematically needed (upper triangle of C; k <= j for triangular B)
    PROF_ZGEMM_EXEC = 12,    // no timing: real flops the launched tiles execute on the matrix pipe, all zgemm calls
                             // (3M kernel: 6 per complex multiply-add, REAL: 4; full tiles incl. shifted/border recompute)
    PROF_COMM = 13,          // collectives of a sharded k-block (work = bytes handed to the communicator)
    PROF_ZGEMM_CPLX = 14,    // no timing: useful flops of all zgemm calls as if none were REAL (a DFTK_MI_GEMM_REAL call
                             // stands for a complex product of twice its flops): what the general complex path needs
    PROF_EW = 15,            // n_G-sized element-wise / column-reduction kernels of the LOBPCG driver and the Gamma-real
                             // pack / unpack passes (work = algorithmic bytes): row-local, i.e. SHARDED work of a
                             // plane-wave-sharded block
    PROF_HOST_WAIT = 16,     // no events: launches = host synchronisations inside the library, ms = wall ms the host waited
    PROF_AR_MODEL = 17,      // no timing: the all-reduces a plane-wave-sharded run of the same calls performs (launches =
                             // calls, work = bytes) -- counted on ONE rank too: the input of bench.py's Amdahl model
    PROF_A2A_MODEL = 18,     // no timing: its slab <-> band transposes (launches, work = bytes of the blocks moved)
    PROF_NFAM = 24
};
struct Prof {
    bool on = false;
    struct Pair { hipEvent_t a, b; int fam; uint64_t tag; double work; };
    struct Shape { double ms = 0, work = 0; int64_t n = 0; };
    std::map<uint64_t, Shape> shapes;   // per-shape zgemm breakdown (env DFTK_MI_GEMM_SHAPES)
    std::vector<Pair> pending;
    std::vector<Pair> pool;
    int open = 0;                       // scopes begun and not yet ended: no flush while > 0 (slots index `pending`)
    int mute = 0;                       // > 0: prof_begin books nothing (inner calls of a routine that is booked as a whole)
    bool shape_tags = false;            // dftk_mi_prof_enable(b, 3): zgemm calls are also booked per shape (dftk_mi_prof_zgemm_shapes)
    double ms[PROF_NFAM] = {0};
    double work[PROF_NFAM] = {0};
    int64_t launches[PROF_NFAM] = {0};
    Prof() = default;
    Prof(const Prof&) = delete;
    Prof& operator=(const Prof&) = delete;
    ~Prof() {                           // (prof_resolve has moved every pair of `pending` into the pool)
        for (auto* v : {&pending, &pool})
            for (auto& pr : *v) {
                hipEventDestroy(pr.a);
                hipEventDestroy(pr.b);
            }
    }
};
int prof_begin(dftk_mi_basis* b, int fam, double work, uint64_t tag = 0);   // returns slot index or -1
void prof_end(dftk_mi_basis* b, int slot);
int prof_resolve(dftk_mi_basis* b);
struct ProfScope {   // RAII pair of prof_begin / prof_end
    dftk_mi_basis* b;
    int slot;
    ProfScope(dftk_mi_basis* basis, int fam, double work) : b(basis), slot(prof_begin(basis, fam, work)) {}
    ~ProfScope() { prof_end(b, slot); }
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
};
void prof_count(dftk_mi_basis* b, int fam, double work);   // count-only families (no events)
// Every host synchronisation of the library's drivers goes through these two (counted in PROF_HOST_WAIT):
// host_wait = hipStreamSynchronize(b->stream); host_fetch = small device -> host result WITHOUT a blit: a copy kernel
// writes into pinned host memory mapped into the device's address space (no __amd_rocclr_copyBuffer dispatch, no staging
// through pageable memory), then one stream synchronisation.
const size_t HOST_FETCH_BYTES = 256 * 1024;
int host_wait(dftk_mi_basis* b);
int host_fetch(dftk_mi_basis* b, void* dst_h, const void* src_d, size_t bytes);

// real-symmetric orbitals of a Gamma-point block (gamma_kernels.hip)
struct GammaReal {
    bool on = false;              // dftk_mi_lobpcg iterates in the half-sphere format
    int64_t n_half = 0;           // (n_G + 1) / 2
    DevTable<int> d_g, d_mg;      // [n_half] sphere rows of G_j and -G_j (j = 0: G = 0)
    DevTable<double> d_kin_half;
    DevTable<cd> P_half;          // n_half x n_p, scaled like the vectors (built on first use)
    const cd* P_src = nullptr;    // borrowed: the kb->P that P_half was built from
    int P_n_p = 0;
    DevBuf<cd> buf;               // pack / unpack scratch
    // plane-wave sharded block: rank r owns the half-format rows [half_rows[r], half_rows[r + 1]) (split evenly);
    // P_half is then this rank's slab of the half-format projectors
    std::vector<int64_t> half_rows;
};

inline std::atomic<uint64_t> g_kblock_serial{0};
struct dftk_mi_kblock {
    dftk_mi_basis* basis = nullptr;   // borrowed
    int device = 0;               // copy of basis->device (destroy must not touch the basis)
    int64_t n_G = 0;
    int64_t n_lines = 0;          // non-empty x-lines (iy, iz)
    int nzx = 0;                  // distinct z planes touched by the sphere
    int z_lo = 0;                 // the sphere planes are {0 .. z_lo-1} u {nz-(nzx-z_lo) .. nz-1} (always so for a sphere
                                  // of G vectors; -1 otherwise: the register-resident z kernels then stay off)
    // device tables
    DevTable<int> d_cpos;         // [n_G]   pos_x[ix] of each coefficient
    DevTable<int> d_line_start;   // [n_lines+1] first coefficient of each line
    DevTable<int> d_line_ypos;    // [n_lines] pos_y[iy] of each line
    DevTable<int> d_zls;          // [nzx+1] first line of each z plane
    DevTable<int> d_zpos;         // [nzx]   pos_z[iz] of each plane
    DevTable<int> d_zval;         // [nzx]   iz of each plane (natural index)
    DevTable<int> d_line_yval;    // [n_lines] iy of each line (natural index)
    DevTable<int> d_cx;           // [n_G]   ix of each coefficient (natural index)
    DevTable<double> d_kin;       // [n_G]
    // [nz*ny*nxp] potential / N, padded pitch: the block's own buffer, or (Vs_shared) the one buffer held by all blocks of a
    // dftk_mi_kblocks_set_potential call; the last holder to let go frees it
    std::shared_ptr<DevTable<double>> Vs_buf;
    bool Vs_shared = false;       // attached by dftk_mi_kblocks_set_potential (stays set when the other holders have left)
    double* d_Vs = nullptr;       // the potential the kernels apply (borrowed: Vs_buf, or ho.dV while the LOBPCG start applies
                                  // V_new - V_old), or null
    // meta-GGA: [nz*ny*nxp] v_tau = de/dtau / N, layout and sharing rule of Vs_buf (dftk_mi_kblock[s]_set_tau_potential); with
    // one bound, H psi gains -1/2 div(v_tau grad psi) (mgga_kernels.hip) and the block stays off the batched executor, the
    // Gamma-real format and the LOBPCG handover, which do not know the term
    std::shared_ptr<DevTable<double>> Vtau_buf;
    bool Vtau_shared = false;
    double* d_Vtau = nullptr;
    // the frame that turns the integer G of a row into (G + k) in cartesian coordinates (dftk_mi_kblock_set_kpoint)
    bool frame_set = false;
    double frame_B[9] = {0};      // recip_lattice, row-major
    double frame_k[3] = {0};      // the k-point, fractional
    DevBuf<cd> mgga_buf;          // n_G x nb scratch of the scaled orbitals (grown on demand)
    // nonlocal
    int n_p = 0;
    const cd* P = nullptr;        // borrowed device pointer, n_G x n_p
    int64_t ldP = 0;
    DevTable<double> d_D;         // [n_p*n_p] dense
    int D_bw = 0;                 // half bandwidth of D
    // LOBPCG workspace (grown on demand)
    DevBuf<cd> lob_buf;
    // what the block keeps between two dftk_mi_lobpcg calls: the A X of the last exit and the y-planes of the density pass
    // over the block it returned (handover.h)
    LobHandover ho;
    // plane-wave (row-slab) sharding of this block over a communicator (dftk_mi_kblock_set_shard): orbital blocks
    // handed to apply_H / lobpcg / density_accumulate and the projector matrix are the rows
    // [sh_rows[rank], sh_rows[rank + 1]) of the sphere; the sphere tables / potential above stay complete
    dftk_mi_comm* sh_comm = nullptr; // borrowed; null = not sharded
    std::vector<int64_t> sh_rows;    // [n_ranks + 1] row offsets
    DevBuf<cd> sh_buf;               // transpose buffers (grown on demand)
    // residual history of the last dftk_mi_lobpcg call: hist[i + M * it], it = 0 .. n_iter (host; empty: no call yet)
    std::vector<double> lob_hist; int lob_hist_M = 0, lob_hist_iters = 0, lob_n_svd = 0;
    // host copies of the sphere (pair tables of the Gamma-real format are built from them on demand)
    std::vector<int64_t> h_mapping;
    std::vector<double> h_kin;
    std::unique_ptr<GammaReal> gr;   // null until dftk_mi_kblock_set_gamma_real / density_accumulate_real
    DevTable<int32_t> d_G3;          // [3 n_G] integer G of every sphere row (built by the first forces call)
    // inverse of the mapping: sphere row of every cube index, -1 where the sphere has none (built by the first
    // dftk_mi_transfer_blochwave call that reads from this block, transfer_kernels.hip)
    DevTable<int32_t> d_inv;
    // every block has its own number (a new block at the address of a destroyed one gets another), and remembers the last
    // (input block, dG) that dftk_mi_transfer_blochwave has checked against it as OUTPUT block: the check runs once per pair
    uint64_t serial = g_kblock_serial.fetch_add(1, std::memory_order_relaxed) + 1;
    uint64_t transfer_in_serial = 0;
    int transfer_dG[3] = {0, 0, 0};
    bool kin_given = false;          // dftk_mi_kblock_create was handed kinetic energies (h_kin is not a row of zeros)
    // the last (input block, S^-1, kshift) that dftk_mi_apply_symop has checked against this block as OUTPUT block
    // (symop_kernels.hip: every output row has its pre-image in the input sphere; the host pass runs once per triple)
    uint64_t symop_in_serial = 0;
    int symop_key[12] = {0};
};

// ------------------------------------------------------------------------------------ internal API
// fft_kernels.hip
int fft_ensure_scratch(dftk_mi_basis* b, dftk_mi_kblock* kb, int nb);
// shift_d (nullable; needs add_kinetic and a bound local potential): out[:, n] -= shift_d[n] psi[:, n] in the gather pass
int launch_local_apply(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, cd* out,
                       int64_t ldout, bool add_kinetic, bool have_local, const double* shift_d = nullptr);
int launch_ifft_to_cube(dftk_mi_kblock* kb, const cd* c, cd* cube, int nb = 1);
int launch_fft_from_cube(dftk_mi_kblock* kb, const cd* cube, cd* c, int nb = 1);
// w_im_h (optional): separate weights for the squared IMAGINARY parts (two real bands packed into one transform)
// keep_planes: stage B of band i writes slot i of kb->ho.planes instead of the scratch, and every launch group that ran is
// marked there (the caller has begun the pass and sized the buffer; never inside a batched call)
int launch_density(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const double* w_h, double* rho,
                   const double* w_im_h = nullptr, const double* w2_h = nullptr, double* rho2 = nullptr,
                   bool keep_planes = false, int pair_nb = 0);
// (pair_nb > 0: psi holds pair_nb FULL-SPHERE columns of real-symmetric orbitals and transform i is column 2 i + i column
//  2 i + 1, formed by stage A itself; nb = ceil(pair_nb / 2), w_h / w_im_h per transform as before.  Single block only.)
int fft_group_size(const dftk_mi_basis* b);      // bands per launch group of the one-slot pipelines
// stages A and B of bands [b0, b0 + nbb) of psi (column 0 = band b0) into slots b0 ... of `planes`
// (pair_nb > 0: column 0 of psi is the first of the pair_nb columns that make up these nbb transforms, as in launch_density)
int launch_planes_fill(dftk_mi_kblock* kb, int b0, int nbb, const cd* psi, int64_t ldpsi, cd* planes, int pair_nb = 0);
// out = V_loc psi for nb bands whose y-planes sit in `planes` (slot = band): stages C (in place: the planes are consumed), D
// and E without the kinetic term; T1 stays scratch
int launch_local_apply_from_planes(dftk_mi_kblock* kb, int nb, cd* planes, cd* out, int64_t ldout);
int launch_density_response(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const cd* dpsi, int64_t lddpsi,
                            const double* wo_h, const double* wd_h, double* drho);
// dst: the padded cube to fill (null: the block's bound local potential)
int launch_pad_potential(dftk_mi_kblock* kb, const double* V, double* dst = nullptr);
// mgga_kernels.hip: tau += sum_n (w_n / 2) sum_a |ifft((G + k)_a psi_n)|^2 and H += -1/2 div(v_tau grad psi) of the bound tau cube
int mgga_tau_accumulate(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const double* w_h, double* tau);
int mgga_div_a_grad(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, cd* H, int64_t ldH);
int launch_kinetic_only(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, cd* out,
                        int64_t ldout, bool accumulate, bool use_kin);

// gemm_kernels.hip
// upper & 1: only the 128x64 tiles that intersect the upper triangle (i <= j) are computed and
//            written; the rest of C is left untouched (Gram matrices that are hermitised afterwards)
// upper & 2: B is upper triangular (B[k][j] = 0 for k > j): the k loop of a tile column stops early
// upper & DFTK_MI_GEMM_SYM_RESULT ('N' products only): the caller knows that A B is Hermitian and needs only its entries
//            on and above the diagonal -- only the tiles that hold one are computed and written, the caller mirrors them.
//            With DFTK_MI_GEMM_REAL the operands are "tall" (a complex row of A and C holds two REAL rows,
//            eig_kernels.hip): the diagonal is met at REAL row 2 i (+ 1) = j, and the tile test uses REAL rows
#define GEMM_SYM_RESULT DFTK_MI_GEMM_SYM_RESULT
bool zgemm_sym_result_pays(int64_t m, int64_t n, int64_t k, bool real);   // (host: does the flag save a round of workgroups?)
int zgemm(dftk_mi_basis* b, char transA, int64_t m, int64_t n, int64_t k, cd alpha, const cd* A,
          int64_t lda, const cd* B, int64_t ldb, cd beta, cd* C, int64_t ldc, int upper = 0);
// D = alpha op(A) B + beta C with D != C allowed (D has C's shape and leading dimension; same flags, same arithmetic: `old`
// is read from C, the store goes to D).  With UPPER / SYM_RESULT only the computed tiles of D are written.  Not recorded
// in a batched call unless D == C.
int zgemm_to(dftk_mi_basis* b, char transA, int64_t m, int64_t n, int64_t k, cd alpha, const cd* A, int64_t lda, const cd* B,
             int64_t ldb, cd beta, const cd* C, int64_t ldc, cd* D, int upper = 0);
int ensure_ws(dftk_mi_basis* b, size_t bytes);
// grow a buffer that work on the basis' stream may still use: if `need` exceeds what it holds, synchronise the stream, then
// reserve (exactly `need` bytes unless `slack` adds some; the contents are not kept; a failure leaves the owner empty)
template <class B>
int scratch_grow(dftk_mi_basis* b, B& buf, size_t need, size_t slack = 0) {
    if (need <= buf.bytes()) return 0;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(buf.reserve(need, slack));
    return 0;
}

// dense_kernels.hip
int dense_potrf_trtri(dftk_mi_basis* b, int n, cd* A, int64_t lda, cd* invR, int64_t ldi,
                      double* normest_R, double* normest_invR, bool real_input = false);   // host outputs
int dense_heev(dftk_mi_basis* b, int n, cd* A, int64_t lda, double* W_h, cd* V, int64_t ldv);
// the blocked Jacobi itself (all n pairs), not booked in any profile family and never redirected
int dense_heev_full(dftk_mi_basis* b, int n, cd* A, int64_t lda, double* W_h, cd* V, int64_t ldv);
// sums over the n x n matrix: squared off-diagonal / diagonal magnitudes and squared imaginary parts (host outputs)
int dense_input_norms(dftk_mi_basis* b, int n, const cd* A, int64_t lda, double* off2, double* dg2, double* im2);
// eig_kernels.hip: the lowest nev eigenpairs only (spectral split on the matrix cores + Jacobi on the projected matrix);
// falls back to dense_heev where the split does not apply
int dense_heev_lowest(dftk_mi_basis* b, int n, int nev, cd* A, int64_t lda, double* W_h, cd* V, int64_t ldv);
int eig_mirror_tall(dftk_mi_basis* b, int n, bool real, cd* X, int64_t ldt);   // eig_kernels.hip
int eig_choose_sigma_host(int n, const double* diag, int nev, double* sigma, double* gap_guess);
int eig_hold_iterations_host(double gap_over_norm);
struct ProfMute {    // RAII: nothing inside is booked (the enclosing scope books the whole routine)
    dftk_mi_basis* b;
    explicit ProfMute(dftk_mi_basis* basis) : b(basis) { if (b->prof) b->prof->mute += 1; }
    ~ProfMute() { if (b->prof) b->prof->mute -= 1; }
    ProfMute(const ProfMute&) = delete;
    ProfMute& operator=(const ProfMute&) = delete;
};
int jacobi_schedule_host(int n, int round, int* nb_out, int* pairs, int* where);
int apply_D(dftk_mi_kblock* kb, int n_bands, const cd* X /*n_p x nb*/, cd* Y);
// elementwise / reductions used by LOBPCG (all on b->stream)
// out[c] of column c, by mode: 0 ||X||, 1 Re <X, Y>, 2 sum w |X|^2, 3 ||X||^2, 4 Im <X, Y>; the five names below are its modes
int ew_colreduce(dftk_mi_basis* b, int mode, int64_t n, int m, const cd* X, int64_t ldx, const cd* Y, int64_t ldy,
                 const double* w, double* out_d);
int ew_colnorms(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, double* out_d);
int ew_coldots(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, const cd* Y, int64_t ldy,
               double* out_re_d);
// out_xy = Re <X, Y> and out_xx = <X, X> per column from one read of X (bit for bit ew_coldots(X, Y) and ew_coldots(X, X))
int ew_coldots2(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, const cd* Y, int64_t ldy, double* out_xy_d,
                double* out_xx_d);
// R = AX - X diag(lam), norms = column norms of R; optionally (kin / xx non-null) mean_kin = sum kin |X|^2 and
// xx = sum |X|^2 per column in the same pass
int ew_residual(dftk_mi_basis* b, int64_t n, int m, const cd* AX, int64_t lda, const cd* X, int64_t ldx,
                const double* lam_d, cd* R, int64_t ldr, double* norms_d, const double* kin, double* mean_kin_d,
                double* xx_d);
// dst = TPA-preconditioned src (kin == null: copy), norms = column norms of dst
// (mean_kin_d == null with kin != null: the default-shift form 1 / (kin + shift), preconditioners.jl:52-53)
int ew_tpa(dftk_mi_basis* b, int64_t n, int m, const cd* src, int64_t lds, cd* dst, int64_t ldd, const double* kin,
           const double* mean_kin_d, double* norms_d, double default_shift = 1.0);
int ew_scale_cols(dftk_mi_basis* b, int64_t n, int m, cd* X, int64_t ldx, const double* s_d, bool invert);
int ew_copy(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, cd* Y, int64_t ldy);
int ew_add(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, cd* Y, int64_t ldy);          // Y += X
int ew_sub_real(dftk_mi_basis* b, int64_t n, const double* a, const double* c, double* out);            // out = a - c
int ew_fill_zero(dftk_mi_basis* b, cd* X, size_t count);
int ew_sub_identity_shifted(dftk_mi_basis* b, int rows, int cols, cd* C, int64_t ldc, int row0);
int ew_gather_cols(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, const int* perm_d,
                   cd* Y, int64_t ldy);
int ew_add_diag(dftk_mi_basis* b, int n, cd* A, int64_t lda, double shift);
int ew_frob2(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, double* out_d);
int ew_hermitize_upper(dftk_mi_basis* b, int n, cd* A, int64_t lda);
int ew_conj_transpose(dftk_mi_basis* b, int n, const cd* A, int64_t lda, cd* B, int64_t ldb);   // B = A^H (n x n)
int ew_square(dftk_mi_basis* b, double* d, size_t n);
int ew_sqrt(dftk_mi_basis* b, double* d, size_t n);
// imaginary parts of the column-wise dots  Im <x_c, y_c>  (ew_coldots gives the real parts)
int ew_coldots_im(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, const cd* Y, int64_t ldy,
                  double* out_im_d);
// mean_kin_c = sum_G kin_G |X_Gc|^2  (precondprep!, preconditioners.jl:75-77)
int ew_weighted_colsums(dftk_mi_basis* b, int64_t n, int m, const cd* X, int64_t ldx, const double* w_d,
                        double* out_d);

// comm.cpp (internal side; all on the basis' stream; null communicator / one rank = no-op)
int comm_size(const dftk_mi_comm* c);
int comm_rank(const dftk_mi_comm* c);
int comm_allreduce(dftk_mi_comm* c, dftk_mi_basis* b, double* d, size_t n);
int comm_allreduce_norms(dftk_mi_comm* c, dftk_mi_basis* b, double* d, size_t n);   // d holds sqrt(local sums)
int comm_alltoallv(dftk_mi_comm* c, dftk_mi_basis* b, const cd* send, const size_t* soff, const size_t* scnt,
                   cd* recv, const size_t* roff, const size_t* rcnt);

// xc_kernels.hip
// (core: the total core density of a non-linear core correction, ONE cube, and grad_core its three gradient cubes; both NULL
// without one.  The XC forms see rho_s + core / n_spin and grad rho_s + grad core / n_spin, every other term rho alone.)
int local_potential_collinear(dftk_mi_kblock* cube_kb, const double* rho, const double* core, const double* vloc,
                              const double* green, int fun_mask, double* V_out, double* energies_h);
int local_potential_lda(dftk_mi_kblock* cube_kb, const double* recip_h, const double* rho, const double* core,
                        const double* grad_core, const double* vloc, const double* green, int fun_mask, double threshold,
                        double* V_out, double* energies_h, const double* tau = nullptr, double* Vtau_out = nullptr);
int local_potential_collinear_gga(dftk_mi_kblock* cube_kb, const double* recip_h, const double* rho, const double* core,
                                  const double* grad_core, const double* vloc, const double* green, int fun_mask,
                                  double threshold, double* V_out, double* energies_h);
int xc_gga_spin_pointwise(dftk_mi_basis* b, int64_t n, const double* rho, const double* sigma, int fun_mask,
                          double threshold, double* e, double* vrho, double* vsigma);

// dV = irfft(green fft(drho)) + f_xc(rho) drho, f_xc = d^2 (rho eps_xc) / d rho^2 of the LDA closed forms (fun_mask bits 1, 2, 4)
int apply_kernel_lda(dftk_mi_kblock* cube_kb, const double* rho, const double* drho, const double* green, int fun_mask,
                     double* dV_out);

// cube_kernels.hip: density-sized operations of the SCF glue (symmetrisation, mixing multipliers) on a full-cube k-block
int cube_symmetrize(dftk_mi_kblock* cube_kb, int n_sym, const int32_t* S_h, const double* tau_h, int do_lowpass,
                    const double* rho_in, double* rho_out);
int cube_fourier_filter(dftk_mi_kblock* cube_kb, int kind, const double* recip_h, double p0, double p1,
                        const double* mult_d, const double* f, double* out);
// grad (three real cubes) = Re irfft(i G_a fft(f)): the operator chain of the GGA pipelines of xc_kernels.hip
int cube_gradient(dftk_mi_kblock* cube_kb, const double* recip_h, const double* f, double* grad);
int xc_gga_pointwise(dftk_mi_basis* b, int64_t n, const double* rho, const double* sigma, int fun_mask,
                     double threshold, double* e, double* vrho, double* vsigma);
int xc_mgga_pointwise(dftk_mi_basis* b, int64_t n, const double* rho, const double* sigma, const double* tau, int fun_mask,
                      double threshold, double* e, double* vrho, double* vsigma, double* vtau);

// setup_kernels.hip
int sphere_enumerate_host(int nx, int ny, int nz, const double* B, const double* k, double Ecut, int64_t cap,
                          int64_t* n_G_out, int64_t* mapping0, double* kinetic, int32_t* G_out);
int build_projectors_hgh(dftk_mi_basis* b, int64_t n_rows, const int32_t* G_d, const double* recip_h, const double* k_h,
                         double volume, int n_species, const double* rp_h, const int* nproj_h, int n_atoms,
                         const int* species_of_atom_h, const double* positions_h, cd* P_d, int64_t ldP, int* n_p_out);

int atomic_superposition(dftk_mi_kblock* cube_kb, int kind, const double* recip_h, int n_species, const double* par_h,
                         int n_atoms, const int* species_of_atom_h, const double* positions_h, double* out_d);
// the table variants (numeric pseudopotentials): tabulated radial parts R_d[channel][row] / form factors ff_d[species][N]
int build_projectors_radial(dftk_mi_basis* b, int64_t n_rows, const int32_t* G_d, const double* recip_h,
                            const double* k_h, double volume, int n_species, const double* R_d, int64_t ldR,
                            const int* first_chan_h, const int* n_chan_h, int n_atoms, const int* species_of_atom_h,
                            const double* positions_h, cd* P_d, int64_t ldP, int* n_p_out);
int atomic_superposition_table(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* ff_d,
                               int n_atoms, const int* species_of_atom_h, const double* positions_h,
                               const double* coef_h, double* out_d);
int forces_local_table(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* ff_d, int n_atoms,
                       const int* species_of_atom_h, const double* positions_h, const double* rho_d, double* forces_h);
// radial_kernels.hip: dftk_mi_radial_transform (asynchronous on the basis' stream)
int radial_transform(dftk_mi_basis* b, int kind, int l, int n_r, const double* r_h, const double* wf_h, double Zion,
                     int64_t n_q, const double* q_d, double* out_d);
// species indices in range and non-decreasing; `who` names the caller in the error text
int check_species_grouped(const char* who, int n_species, int n_atoms, const int* species_of_atom_h);
// per atom [t_x(nx) | t_y(ny) | t_z(nz)], t(i) = exp(-2 pi i g(i) r) with g the signed frequency of index i
std::vector<cd> phase_tables_host(int nx, int ny, int nz, int n_atoms, const double* positions_h);
// the columns of P: atom-major in the caller's order; within an atom (l, m, i): offset_l + n_l (m + l) + (i - 1)
// (nonlocal.jl:205-244).  rp_h / nproj_h: 4 entries per species (l = 0..3).  col_start (optional): n_atoms + 1 offsets.
struct ProjCol;
int list_projector_columns(int n_species, const double* rp_h, const int* nproj_h, int n_atoms,
                           const int* species_of_atom_h, const double* positions_h, std::vector<ProjCol>* cols,
                           std::vector<int>* col_start = nullptr);

// gamma_kernels.hip
int gamma_tables_host(int nx, int ny, int nz, int64_t n_G, const int64_t* mapping, int64_t* n_half_out, int32_t* g,
                      int32_t* mg);
int gamma_enable(dftk_mi_kblock* kb, int on);
int gamma_compress(dftk_mi_kblock* kb, int m, const cd* X, int64_t ldx, cd* H, int64_t ldh);
// ... after rotating every column by the global phase that maximises its real-symmetric part (LOBPCG entry)
int gamma_compress_aligned(dftk_mi_kblock* kb, int m, const cd* X, int64_t ldx, cd* H, int64_t ldh);
int gamma_expand(dftk_mi_kblock* kb, int m, const cd* H, int64_t ldh, cd* X, int64_t ldx);
// add (optional, un-sharded blocks with which == 1 only): Hpsi = add + H psi in the pass that writes Hpsi (add may be Hpsi)
int gamma_apply_H(dftk_mi_kblock* kb, int which, int nb, const cd* psi, int64_t ldpsi, cd* Hpsi, int64_t ldH,
                  const cd* add = nullptr, int64_t ldadd = 0);
int gamma_density(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const double* w_h, double* rho);
// local building blocks (whole bands on this rank)
int gamma_ensure_buf(dftk_mi_kblock* kb, size_t elems);
int gamma_pack_pairs(dftk_mi_kblock* kb, int nb, const cd* H, int64_t ldh, cd* Z, int64_t ldz);
// (add, optional: H = add + unpack(W), one rounding per entry; add may be H itself)
int gamma_unpack_pairs(dftk_mi_kblock* kb, int nb, const cd* W, int64_t ldw, cd* H, int64_t ldh, const cd* add = nullptr,
                       int64_t ldadd = 0);
int gamma_pack_full(dftk_mi_kblock* kb, int nb, const cd* X, int64_t ldx, cd* Z, int64_t ldz);
int gamma_gather_P(dftk_mi_kblock* kb, int ncols, const cd* P, int64_t ldP, cd* Ph, int64_t ldh, double* asym_mag_h);
int gamma_density_bands(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const double* w_h, double* rho);
// y-planes kept by the density pass over the block the general LOBPCG driver returned (kb->ho): may this
// block keep and use them now (DFTK_MI_PLANES_REUSE, Gamma-real format on, un-sharded, outside a batched call)?
bool planes_eligible(const dftk_mi_kblock* kb);
int gamma_apply_local_from_planes(dftk_mi_kblock* kb, int nb, const cd* X, int64_t ldx, cd* Hpsi, int64_t ldH,
                                  const cd* add = nullptr, int64_t ldadd = 0);   // (add: as gamma_unpack_pairs)
int64_t gamma_local_rows(const dftk_mi_kblock* kb);     // half-format rows held by this rank
int64_t gamma_row0(const dftk_mi_kblock* kb);
int gamma_projectors(dftk_mi_kblock* kb);               // half-format projectors of this rank (built on first use)
int gamma_projectors_renew(dftk_mi_kblock* kb, size_t elems);   // shared start of a rebuild: sync, release, allocate
// api.cpp: the plane-wave sharded variants (slab <-> band all-to-alls around the local building blocks) and the
// entry / exit conversions of dftk_mi_lobpcg (caller's full-sphere block <-> half-format block, sharded or not)
int gamma_apply_H_sharded(dftk_mi_kblock* kb, int which, int nb, const cd* psi, int64_t ldpsi, cd* Hpsi, int64_t ldH);
int gamma_projectors_sharded(dftk_mi_kblock* kb);
int gamma_density_sharded(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const double* w_h, double* rho);
int gamma_lobpcg_load(dftk_mi_kblock* kb, int M, const cd* Xuser, int64_t ldX, cd* Xh, int64_t ldh, bool align = false);
int gamma_lobpcg_store(dftk_mi_kblock* kb, int M, const cd* Xh, int64_t ldh, cd* Xuser, int64_t ldX);
// api.cpp: Hpsi (+)= P D P' psi on `rows` rows of projector storage P (leading dimension ldP); gemm_flags is OR-ed
// into the two products (DFTK_MI_GEMM_REAL for half-format blocks); comm (nullable) all-reduces the projections
int apply_nonlocal_rows(dftk_mi_kblock* kb, int nb, const cd* P, int64_t ldP, int64_t rows, const cd* psi,
                        int64_t ldpsi, cd* Hpsi, int64_t ldH, bool accumulate, int gemm_flags, dftk_mi_comm* comm);

// force_kernels.hip: dftk_mi_forces_local / dftk_mi_forces_nonlocal
int forces_local(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* par_h, int n_atoms,
                 const int* species_of_atom_h, const double* positions_h, const double* rho_d, double* forces_h);
int forces_nonlocal(dftk_mi_kblock* kb, const double* kcoord_h, int nb, const cd* psi, int64_t ld_psi,
                    const double* weight_h, int n_atoms, const int* col_start_h, double* forces_h);
int ensure_G3(dftk_mi_kblock* kb);       // kb->d_G3 (integer G of every sphere row), built on first use
// Z[:, n] = psi[:, n], Z[:, (1 + alpha) nb + n] = i g_alpha psi[:, n] for nb columns, g = G + k (reduced) of sphere row row0 + i
int launch_nl_operands_full(dftk_mi_basis* b, int64_t rows, int nb, int64_t row0, const int* G3, const double* kcoord_h,
                            const cd* psi, int64_t ldpsi, cd* Z, int64_t ldz);
// out[r] = scale * sum_i in[r * n + i], one workgroup per row, fixed reduction order
int launch_rowsum(dftk_mi_basis* b, int rows, int64_t n, const double* in, double scale, double* out);
int launch_real_to_cplx(dftk_mi_basis* b, int64_t n, const double* x, cd* y);      // y = x + 0 i

// stress_kernels.hip: dftk_mi_stress_kinetic_nonlocal / dftk_mi_stress_cube / dftk_mi_stress_xc
int stress_kinetic_nonlocal(dftk_mi_kblock* kb, const double* recip_h, const double* kcoord_h, int nb, const cd* psi,
                            int64_t ld_psi, const double* weight_h, int n_species, const double* rp_h, const int* nproj_h,
                            int n_atoms, const int* species_of_atom_h, const double* positions_h, const int* col_start_h,
                            double* stress_h);
int stress_cube(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* par_h, int n_atoms,
                const int* species_of_atom_h, const double* positions_h, const double* rho_d, double* out_h);
int stress_xc(dftk_mi_basis* b, int64_t n, int n_spin, const double* rho_d, const double* vrho_d, const double* e_d,
              const double* vsigma_d, const double* grad_d, double* out_h);

// response_kernels.hip: the n_G-sized element-wise kernels of the Sternheimer solver (all on b->stream; one launch for
// all columns, scalars read from device memory)
// x += p alpha, r -= c alpha with alpha[c] = gamma[c] / pc[c] (0 where pc[c] == 0)
int resp_update_xr(dftk_mi_basis* b, int64_t n, int m, const double* gamma_d, const double* pc_d, const cd* p, int64_t ldp,
                   const cd* c, int64_t ldc, cd* x, int64_t ldx, cd* r, int64_t ldr);
// p = z + p beta with beta[c] = gamma_new[c] / gamma_old[c] (0 where gamma_old[c] == 0)
int resp_update_p(dftk_mi_basis* b, int64_t n, int m, const double* gamma_new_d, const double* gamma_old_d, const cd* z,
                  int64_t ldz, cd* p, int64_t ldp);
// Y = a X + bcoef Y (bcoef == 0: Y is not read); sd (nullable): a is multiplied by sd[column]
int resp_axpby(dftk_mi_basis* b, int64_t n, int m, double a, const double* sd, const cd* X, int64_t ldx, double bcoef, cd* Y,
               int64_t ldy);
// S[i, l] /= (ee[i] - e[l]) for the n_extra x m matrix S
int resp_scale_inv(dftk_mi_basis* b, int n_extra, int m, cd* S, int64_t lds, const double* ee_d, const double* e_d);
int resp_broadcast(dftk_mi_basis* b, int m, const double* src_d, double* dst_d);      // dst[0 .. m) = src[0]

// sternheimer.cpp
int sternheimer_run(dftk_mi_kblock* kb, int n_occ, const cd* psi_occ, int64_t ld_occ, const double* eps_h, int n_extra,
                    const cd* psi_extra, int64_t ld_extra, const cd* rhs, int64_t ld_rhs, const double* tol_h, int miniter,
                    int maxiter, const cd* dpsi0, int64_t ld_dpsi0, cd* dpsi, int64_t ld_dpsi, int* n_iter, double* resid_h,
                    int* converged);

// phonon_kernels.hip: dftk_mi_local_potential_displacement / dftk_mi_dynmat_local / dftk_mi_nonlocal_displacement_apply /
// dftk_mi_dynmat_nonlocal (the entry points are the whole interface: see include/dftk_mi355x.h)

// exx_kernels.hip: dftk_mi_exx_apply (the entry point is the whole interface: see include/dftk_mi355x.h)

// newton_kernels.hip: dftk_mi_orbitals_realspace / dftk_mi_tangent_density / dftk_mi_tangent_potential / dftk_mi_tangent_cg_*
// (the entry points are the whole interface: see include/dftk_mi355x.h)

// transfer_kernels.hip: dftk_mi_transfer_blochwave / dftk_mi_transfer_density; symop_kernels.hip and wannier_kernels.hip share
// the inverse cube -> row map of a block and the ordering of two bases' streams with them
namespace dftk_transfer {
__host__ __device__ inline bool freq_on_axis(int g, int n) { return g >= -((n - 1) - (n - 1) / 2) && g <= (n - 1) / 2; }
__host__ __device__ inline int freq_index(int g, int n) { return g < 0 ? g + n : g; }
// cube index of G on an (nx, ny, nz) grid, -1 if G is not on it
__host__ __device__ inline int64_t cube_index(int g0, int g1, int g2, int nx, int ny, int nz) {
    if (!(freq_on_axis(g0, nx) && freq_on_axis(g1, ny) && freq_on_axis(g2, nz))) return -1;
    return freq_index(g0, nx) + (int64_t)nx * (freq_index(g1, ny) + (int64_t)ny * freq_index(g2, nz));
}
int order_after(dftk_mi_basis* waiter, dftk_mi_basis* producer);
int inverse_map_host(const dftk_mi_kblock* kb, std::vector<int32_t>* inv);
int ensure_inverse_map(dftk_mi_kblock* kb);      // kb->d_inv, built on first use
}

// symop_kernels.hip: dftk_mi_apply_symop; wannier_kernels.hip: dftk_mi_wannier_overlaps / dftk_mi_wannier_guess_columns (the
// entry points are the whole interface: see include/dftk_mi355x.h)

// refine_kernels.hip: the per-column element-wise kernels of the refinement metric (refine.cpp)
// Y[:, c] = f_c(kin) X[:, c] with t = kin + mean_kin[c]: mode 0 f = sqrt(t), mode 1 f = 1 / t   (X == Y allowed)
int refine_scale_T(dftk_mi_basis* b, int64_t n, int m, int mode, const double* kin_d, const double* mean_kin_d, const cd* X,
                   int64_t ldx, cd* Y, int64_t ldy);
// gamma[c] = 0 where res[c] <= tol: the CG kernels of response_kernels.hip then leave x and r of column c as they are
int refine_lock(dftk_mi_basis* b, int m, const double* res_d, double tol, double* gamma_d);
// refine.cpp
int refinement_metric_solve(dftk_mi_kblock* kb, int m, const cd* psi, int64_t ld_psi, const cd* res, int64_t ld_res,
                            double tol, int maxiter, cd* out, int64_t ld_out, int* iters_h, double* resnorm_h);

// lobpcg.cpp
// ortho!(X) (Cholesky-QR with the reference's shift-and-retry and SVD fallback) on a stand-alone block;
// force_svd = 1 takes the SVD branch directly (tests)
int lobpcg_ortho(dftk_mi_basis* b, int64_t n, int m, cd* X, int64_t ldx, int force_svd, int* n_chol, int* used_svd);
int lobpcg_run_multi(int n_kb, dftk_mi_kblock* const* kbs, int M, cd* const* X, const int64_t* ldX, double tol, int miniter,
                     int maxiter, int n_conv_check, int use_tpa, const uint64_t* seeds, double* lambda_h, double* resid_h,
                     int* n_iter, int* converged, int64_t* n_matvec, int* status);
int lobpcg_run(dftk_mi_kblock* kb, int M, cd* X, int64_t ldX, double tol, int miniter, int maxiter,
               int n_conv_check, int use_tpa, uint64_t seed, double* lambda_h, double* resid_h,
               int* n_iter, int* converged, int64_t* n_matvec);
