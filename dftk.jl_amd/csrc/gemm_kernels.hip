// gemm_kernels.hip -- complex fp64 GEMM on the f64 matrix cores (v_mfma_f64_16x16x4_f64, gfx950).
//
// Covers every BLAS3 call of the reference's hot path:
//   P' * psi, P * (D P' psi)                    src/terms/operators.jl:126-128          (K7, K9)
//   mul_hermi(Y', AY), BY' * X                  src/eigen/lobpcg_hyper_impl.jl:90-121,278 (K10, K15)
//   Y * cX, X * invR                            :124-132, 234                           (K12, K14)
// as  C = alpha * op(A) * B + beta * C  with op(A) in {A, A^H}, B never transposed, column-major.
//
// Kernels:
//   k_zgemm_3m     every full and ragged-border tile.  Three real MFMA streams per complex product (Karatsuba) on
//                  128 x 32 workgroup tiles, two per REAL product on 128 x 64 tiles; operands staged through LDS,
//                  software pipeline with one mid-tile barrier.
//   k_zgemm_naive  one thread per C entry, no matrix cores (DFTK_MI_GEMM=naive): debugging reference.
//   k_zgemm_reduce fixed-order sum of the split-K slabs => bitwise reproducible results.
// Host side: tiling into full tiles + ragged border, a cost-model K split that fills the resident
// workgroup slots once, XCD-aware 1-D grids (zgemm(), gemm_tiling(), gemm_plan_split()).
#include "common.h"
#include "batch.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <map>
#include <vector>
#include <cmath>
#include <algorithm>
#include <mutex>

typedef double v4d __attribute__((ext_vector_type(4)));

// lane mapping of v_mfma_f64_16x16x4_f64:
//   A operand: lane l holds A[i = l & 15][k = l >> 4];  B operand: lane l holds B[k = l >> 4][j = l & 15]
//   C/D: 4 values per lane, value r is C[row = (l >> 4) + 4 r][col = l & 15]

// ------------------------------------------------------------------------------------------------
// The complex product with THREE real MFMAs per tile step instead of four (Karatsuba / "3M").  A wave owns a
// 32 x (16 RN) output tile, a workgroup is 4 waves stacked along m: 128 x 32 workgroup tiles for complex
// products (12 accumulator tiles = 96 VGPRs per wave).  15-23 % faster than the classic four-product kernel on
// every LOBPCG / projector shape; the rounding error bound grows by a factor ~2 in the imaginary
// part (still eps * sum |a||b|).
// The K-tile (8 deep) of both operands is staged through LDS:
//   * global reads are fully coalesced (8 lanes x 16 B = one 128-B line per column of a K-major
//     operand; 128 consecutive rows of an M-major one) and each element is fetched ONCE per
//     workgroup instead of once per wave that needs it;
//   * LDS image is [k][column] with a 16-element-aligned pitch, so a wave's MFMA fragment read
//     (16 columns x 2 k per lane group) touches 16 distinct 16-B slots: conflict-free
//     ds_read_b128; K-major operands are stored with the column index XOR (k & 7) so that the
//     transposing ds_write_b128 of 8 consecutive-k lanes also hits 8 distinct slots;
//   * register-staged software pipeline: the global loads of tile t+1 are in flight while the
//     MFMAs of tile t issue; one barrier per tile, two LDS buffers.
#define LT_KT 8
#define GEMM_RM 2
#define GEMM_WAVES 4
#define GEMM_BM (GEMM_WAVES * GEMM_RM * 16)   // 128
#define M3_RN 2
#define M3_BN (16 * M3_RN)
#define M3_RN_REAL 4
#define M3_BN_REAL (16 * M3_RN_REAL)
// workgroups per CU the kernel is compiled for.  3 for the M-major variant (168 VGPRs) is as fast as 2,
// but with 12 instead of 8 row panels in flight per XCD the column tiles of a panel drift apart in k and
// re-fetch their A tiles: FETCH_SIZE 4.0x the operand bytes against 1.55x -> 2.  The K-major variant
// spills at 168 registers (-12 %).
#define M3_MIN_BLOCKS 2
// REAL (flag DFTK_MI_GEMM_REAL of zgemm): the operands are blocks of REAL-SYMMETRIC plane-wave vectors in the
// half-sphere format (gamma_kernels.hip), i.e. really REAL matrices with two real rows per complex entry:
//   conj(A)' B -> Re(A^H B) = Ar' Br + Ai' Bi   (the imaginary part vanishes mathematically; stored as 0)
//   A B        -> A * Re(B): Re = Ar Br, Im = Ai Br   (B is a real coefficient matrix stored as complex)
// TWO real MFMA streams per complex entry instead of three -- exactly the flops of the equivalent dgemm.
// FULL (MODE 1): launched only over tiles that lie entirely inside C -> no per-sub-tile predicates (runtime
// predicates become a branch per MFMA and break the MFMA issue stream).  gm x gn is the tile sub-grid of this
// launch, (rt0, ct0) its origin in tiles (see lsplit below for the border launch).
// FOLD (triangular B, 'N', full tiles, no K split): a workgroup computes TWO column tiles of its row panel back to back, the
// long one gn - 1 - p first and then the short one p (the middle one alone when gn is odd): every workgroup runs gn + 1
// diagonal blocks of k instead of 1 ... gn, half as many workgroups start and drain, and the loads of the second tile's first
// k-tile are in flight while the first tile is stored.  The k order inside a tile is the one of the unfolded kernel.
// Work item of workgroup `id` of a FOLD launch over gm row panels x gn column tiles (grid = 8 ceil(gm / 8) ceil(gn / 2)): the
// items of one row panel sit on the same XCD (id & 7), they share the A panel.  false: no work.  col2 < 0: one tile only.
// (host + device: dftk_mi_zgemm_fold_host lists the items of a launch for the CPU test-suite)
__host__ __device__ inline bool gemm_fold_item(int id, int gm, int gn, int* row_t, int* col1, int* col2) {
    const int xcd = id & 7, slot = id >> 3;
    const int np = (gn + 1) >> 1, p = slot % np;
    *row_t = (slot / np) * 8 + xcd;
    *col1 = gn - 1 - p;
    *col2 = (p != gn - 1 - p) ? p : -1;
    return *row_t < gm;
}

// Work item of workgroup `id` of a compact UPPER launch over gm row panels x gn column tiles x nsplit k-chunks, q = column
// tiles per row panel (grid = 8 ceil(L nsplit / 8), L = live tiles): row panel r keeps its column tiles >= r q; the items
// (k-chunk, row panel, live column tile) in this order are dealt to the XCDs (id & 7) in 8 contiguous blocks.  false: no work.
// (host + device: dftk_mi_zgemm_compact_host lists the items of a launch for the CPU test-suite)
__host__ __device__ inline bool gemm_compact_item(int id, int gm, int gn, int q, int nsplit, int* z, int* row_t, int* col_t) {
    const int xcd = id & 7, slot = id >> 3;
    int L = 0;
    for (int r = 0; r < gm; ++r) L += (gn - r * q > 0) ? gn - r * q : 0;
    const int N = L * nsplit, per = (N + 7) >> 3;
    const int item = xcd * per + slot;
    if (slot >= per || item >= N) return false;
    *z = item / L;
    int t = item - *z * L, r = 0;
    while (t >= gn - r * q) {
        t -= gn - r * q;
        ++r;
    }
    *row_t = r;
    *col_t = r * q + t;
    return true;
}

template <bool CONJA, int MODE, bool REAL, int RN, bool FOLD = false>
__global__ __launch_bounds__(GEMM_WAVES * 64, M3_MIN_BLOCKS) void k_zgemm_3m(int m, int n, int K, int kchunk, int gm, int gn,
                                                               int rt0, int ct0, int lsplit, int upper,
                                                               int shift_ct, int shift_rt, int nsplit, const cd* __restrict__ A, int64_t lda,
                                                               const cd* __restrict__ B, int64_t ldb,
                                                               const cd* C, cd* D, int64_t ldc, cd alpha, cd beta,
                                                               cd* __restrict__ slab) {
    // C, D: the epilogue reads `old` from C and stores to D, entry by entry at the same offset (leading dimension ldc for
    // both).  D == C is the in-place product, so the two are not declared restrict.
    constexpr int BN = 16 * RN;      // column-tile width: 32 (3M complex), 64 (REAL: the third product's registers
                                     // hold a second pair of accumulator columns -> 1.7x the flops per operand byte)
    static_assert(RN == 2 || RN == 4, "B staging handles one or two columns per thread");
    __shared__ cd sA[2][LT_KT][GEMM_BM];
    __shared__ cd sB[2][LT_KT][BN];
    const int id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3;
    int z, row_t, col_t;
    int col2 = -1;   // FOLD: the second tile column of this workgroup
    if (FOLD) {
        if (!gemm_fold_item(id, gm, gn, &row_t, &col_t, &col2)) return;   // whole workgroup
        z = 0;
    } else if (upper & 16) {
        // compact UPPER launch: only the LIVE tiles exist in the grid (row panel r keeps its column tiles >= r BM / BN), the
        // work items (k-chunk, row panel, live column tile) in this order are dealt to the XCDs in 8 contiguous blocks: an
        // XCD sees at most two k-chunks, the column tiles of a row panel sit next to each other, every XCD gets the same
        // number of items and no dead workgroup passes through the dispatcher (with the full grid below 38-44 % of the
        // workgroups of an UPPER launch leave at once; measured: the live ones then spread unevenly over the CUs as soon
        // as an XCD holds more than ~50 of them)
        const int q = (GEMM_BM << ((upper >> 5) & 1)) / BN;   // (upper & 32: two REAL rows per row of C, see below)
        if (!gemm_compact_item(id, gm, gn, q, nsplit, &z, &row_t, &col_t)) return;   // whole workgroup
    } else if (upper & 4) {
        // K-split launches: all tiles of one k-chunk on the SAME XCD, so that both the A chunk and the
        // B chunk are fetched from HBM once and shared through that XCD's L2
        const int per = gm * gn;
        z = (slot / per) * 8 + xcd;
        const int rem = slot % per;
        row_t = rem / gn;
        col_t = rem - row_t * gn;
        if (z >= nsplit) return;   // whole workgroup
    } else {
        // column tiles of one (k-chunk, row panel) on the same XCD (shares the A panel)
        col_t = slot % gn;
        const int R = (slot / gn) * 8 + xcd;
        if (R >= gm * nsplit) return;   // whole workgroup
        z = R / gm;
        row_t = R - z * gm;
        // upper & 8: rotate the row panels by floor(z gcd(8, gm) / 8).  An XCD sees the groups R = xcd + 8 t, i.e. only
        // gm / gcd(8, gm) different row panels; with UPPER the panels hold different numbers of live tiles (8, 6, 4, 2
        // for a 503^2 Gram matrix), so without the rotation XCDs 0 and 4 do four times the work of XCDs 3 and 7
        if (upper & 8) {
            const int g = (gm % 8 == 0) ? 8 : (gm % 4 == 0) ? 4 : (gm % 2 == 0) ? 2 : 1;
            row_t = (row_t + (z * g) / 8) % gm;
        }
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    // rectangle of tiles at (rt0, ct0), or (lsplit >= 0) the L-shaped ragged border as a list:
    // entries < lsplit are the right strip (tile column ct0), the rest the bottom strip (tile row rt0)
    const int tr = lsplit < 0 ? row_t + rt0 : (row_t < lsplit ? row_t : rt0);
    int tcn = lsplit < 0 ? col_t + ct0 : (row_t < lsplit ? ct0 : row_t - lsplit);
    // tile column shift_ct (the one past the last full column) is SHIFTED LEFT to end at column n: it overlaps
    // its neighbour, recomputes up to 31 columns and stores only columns >= jmin.  A ragged n then needs no
    // right-strip launch (which would stream all of A a second time for a handful of columns).
    bool shifted = tcn == shift_ct;
    // likewise tile row shift_rt (the one past the last full row) is SHIFTED UP to end at row m and stores only
    // rows >= imin: a ragged m needs no bottom-strip launch (a second, serialized launch of slow predicated
    // workgroups whose k chains are as long as the interior's)
    const bool rshifted = tr == shift_rt;
    const int I0 = rshifted ? m - GEMM_BM : tr * GEMM_BM, imin = tr * GEMM_BM;
    int J0 = shifted ? n - BN : tcn * BN, jmin = shifted ? tcn * BN : 0;   // (not const: FOLD moves to a second tile column)
    // upper & 32 (with upper & 1): the rows of C are pairs of REAL rows (symmetric result of a "tall" REAL 'N' product,
    // GEMM_SYM_RESULT): the first REAL row of the tile is 2 imin
    if ((upper & 1) && (imin << ((upper >> 5) & 1)) >= J0 + BN) return;   // no needed entry (i <= j) in this tile (whole workgroup)
    const int i0 = I0 + wave * (GEMM_RM * 16);
    const int kbeg = z * kchunk;
    // bit 1 of `upper`: B is upper triangular (B[k][j] = 0 for k > j) -> this tile column stops at k = J0 + BN
    int kend = min(min(K, kbeg + kchunk), (upper & 2) ? J0 + BN : K);
    // MODE 1: every tile of the launch is full (no predicates anywhere).  MODE 0: predicated only.
    constexpr bool FULL = MODE == 1;
    const int rmv = FULL ? GEMM_RM : min(GEMM_RM, max(0, (m - i0 + 15) >> 4));
    const int rnv = FULL ? RN : min(RN, max(0, (n - J0 + 15) >> 4));
    const bool active = FULL || (rmv > 0 && rnv > 0);

    // three real products per complex one (Karatsuba / "3M"):
    //   P1 = sum Ar Br, P2 = sum Ai Bi, P3 = sum (Ar +/- Ai)(Br + Bi)   (- for conj(A))
    //   A B      : Re = P1 - P2, Im = P3 - P1 - P2 ;   conj(A) B: Re = P1 + P2, Im = P3 - P1 + P2
    v4d acc1[GEMM_RM][RN], acc2[GEMM_RM][RN], acc3[GEMM_RM][RN];
#pragma unroll
    for (int a = 0; a < GEMM_RM; ++a)
#pragma unroll
        for (int b = 0; b < RN; ++b) {
            acc1[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
            acc2[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
            acc3[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
        }

    // ---- global -> register staging assignment
    // K-major operand tile (LT_KT x W columns): thread handles k = tid & 7, columns (tid >> 3) + 32 r
    // M-major A tile (LT_KT x 128 rows):        thread handles row = tid & 127, k = (tid >> 7) + 2 r
    const int tk = tid & 7, tc = tid >> 3;
    // running per-thread source pointers (named scalars: arrays captured by lambdas end up in scratch);
    // every load advances them by one k-tile
    const cd *pA0, *pA1, *pA2, *pA3, *pB0, *pB1;
    auto init_ptrs = [&]() {
        auto a_ptr = [&](int r) -> const cd* {
            if (CONJA) {
                int c = I0 + tc + 32 * r;
                if (c > m - 1) c = m - 1;
                return A + (int64_t)c * lda + kbeg + tk;
            } else {
                int i = I0 + (tid & 127);
                if (i > m - 1) i = m - 1;
                return A + i + (int64_t)(kbeg + (tid >> 7) + 2 * r) * lda;
            }
        };
        auto b_ptr = [&](int r) -> const cd* {
            int c = J0 + tc + 32 * r;
            if (c > n - 1) c = n - 1;
            return B + (int64_t)c * ldb + kbeg + tk;
        };
        pA0 = a_ptr(0);
        pA1 = a_ptr(1);
        pA2 = a_ptr(2);
        pA3 = a_ptr(3);
        pB0 = b_ptr(0);
        pB1 = b_ptr(RN == 4 ? 1 : 0);
    };
    init_ptrs();
    const int64_t stepA = CONJA ? (int64_t)LT_KT : (int64_t)LT_KT * lda;
    struct Stage {
        cd a0, a1, a2, a3, b0, b1;
    };
    auto advance = [&]() {
        pA0 += stepA;
        pA1 += stepA;
        pA2 += stepA;
        pA3 += stepA;
        pB0 += LT_KT;
        if (RN == 4) pB1 += LT_KT;
    };
    // tile entirely inside [kbeg, kend): plain loads
    auto load_fast = [&]() -> Stage {
        Stage st;
        st.a0 = *pA0;
        st.a1 = *pA1;
        st.a2 = *pA2;
        st.a3 = *pA3;
        st.b0 = *pB0;
        if (RN == 4) st.b1 = *pB1;
        advance();
        return st;
    };
    // any tile: k indices beyond kend-1 are clamped to kend-1 (and zeroed later by mask_tile)
    auto load_tile = [&](int k0) -> Stage {
        Stage st;
        const int oB = max(0, k0 + tk - (kend - 1));
        if (CONJA) {
            st.a0 = *(pA0 - oB);
            st.a1 = *(pA1 - oB);
            st.a2 = *(pA2 - oB);
            st.a3 = *(pA3 - oB);
        } else {
            const int kk = k0 + (tid >> 7) - (kend - 1);
            st.a0 = *(pA0 - (int64_t)max(0, kk) * lda);
            st.a1 = *(pA1 - (int64_t)max(0, kk + 2) * lda);
            st.a2 = *(pA2 - (int64_t)max(0, kk + 4) * lda);
            st.a3 = *(pA3 - (int64_t)max(0, kk + 6) * lda);
        }
        st.b0 = *(pB0 - oB);
        if (RN == 4) st.b1 = *(pB1 - oB);
        advance();
        return st;
    };
    // zero the entries whose k lies beyond the K range (only the last tile of a chunk needs it)
    auto mask_tile = [&](Stage st, int k0) -> Stage {
        const cd czero = make_double2(0.0, 0.0);
        const bool vB = (k0 + tk) < kend;
        if (CONJA) {
            if (!vB) st.a0 = st.a1 = st.a2 = st.a3 = czero;
        } else {
            const int kk = k0 + (tid >> 7);
            if (kk >= kend) st.a0 = czero;
            if (kk + 2 >= kend) st.a1 = czero;
            if (kk + 4 >= kend) st.a2 = czero;
            if (kk + 6 >= kend) st.a3 = czero;
        }
        if (!vB) st.b0 = st.b1 = czero;
        return st;
    };
    // Triangular B (upper & 2): inside the diagonal block of a tile column (its last BN k) the entries below the diagonal
    // (k > j) are staged as ZEROS, whatever B holds there -- the call equals the dense product with triu(B) bit for bit
    // (the k order of a tile is the same and the dense product adds exact zeros), and the strict lower triangle of B never
    // reaches C.  k0 is the first k of the tile stored; this thread holds the entries (k0 + tk, J0 + tc) and (., J0 + tc + 32).
    int cB0 = (upper & 2) ? J0 + tc - tk : INT32_MAX, cB1 = (upper & 2) ? J0 + tc + 32 - tk : INT32_MAX;
    auto store_tile = [&](int buf, const Stage& st, int k0) {
        if (CONJA) {
            sA[buf][tk][(tc) ^ tk] = st.a0;
            sA[buf][tk][(tc + 32) ^ tk] = st.a1;
            sA[buf][tk][(tc + 64) ^ tk] = st.a2;
            sA[buf][tk][(tc + 96) ^ tk] = st.a3;
        } else {
            const int kk = tid >> 7, ii = tid & 127;
            sA[buf][kk][ii] = st.a0;
            sA[buf][kk + 2][ii] = st.a1;
            sA[buf][kk + 4][ii] = st.a2;
            sA[buf][kk + 6][ii] = st.a3;
        }
        // (selects on the VALUES: a conditional between two cd lvalues becomes a select of addresses and sends st to scratch)
        // 'N' products only (X inv(R)): in the 'C' kernels the extra selects pushed the LDS writes out of their MFMA shadows
        // (Gram products 3-5 % slower, measured); a 'C' call with a triangular B still expects the zeros in B itself
        if (!CONJA) {
            const bool z0 = k0 > cB0, z1 = k0 > cB1;
            sB[buf][tk][(tc) ^ tk] = make_double2(z0 ? 0.0 : st.b0.x, z0 ? 0.0 : st.b0.y);
            if (RN == 4) sB[buf][tk][(tc + 32) ^ tk] = make_double2(z1 ? 0.0 : st.b1.x, z1 ? 0.0 : st.b1.y);
        } else {
            sB[buf][tk][(tc) ^ tk] = st.b0;
            if (RN == 4) sB[buf][tk][(tc + 32) ^ tk] = st.b1;
        }
    };
    // MFMA fragments of one k-half of a tile: half h holds k = 2*lk + h (lk = lane >> 4)
    struct Frag {
        cd a[GEMM_RM], b[RN];
    };
    auto read_frag = [&](int buf, int h) -> Frag {
        Frag f;
        const int kk = 2 * lk + h;
#pragma unroll
        for (int a = 0; a < GEMM_RM; ++a) {
            const int c = wave * (GEMM_RM * 16) + a * 16 + li;
            f.a[a] = sA[buf][kk][CONJA ? (c ^ kk) : c];
        }
#pragma unroll
        for (int b = 0; b < RN; ++b) {
            const int c = b * 16 + li;
            f.b[b] = sB[buf][kk][c ^ kk];
        }
        return f;
    };
    auto mfma_half = [&](const Frag& f, auto nopred_tag) {
        constexpr bool NOPRED = decltype(nopred_tag)::value;
        double bs[RN];
#pragma unroll
        for (int b = 0; b < RN; ++b) bs[b] = f.b[b].x + f.b[b].y;
#pragma unroll
        for (int a = 0; a < GEMM_RM; ++a) {
            if (NOPRED || a < rmv) {
                const double ar = f.a[a].x, ai = f.a[a].y;
                const double as = CONJA ? ar - ai : ar + ai;
#pragma unroll
                for (int b = 0; b < RN; ++b)
                    if (NOPRED || b < rnv) acc1[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, f.b[b].x, acc1[a][b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < RN; ++b)
                    if (NOPRED || b < rnv) {
                        if (REAL && CONJA)   // Re(conj(a) b) = ar br + ai bi: ONE accumulator
                            acc1[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, f.b[b].y, acc1[a][b], 0, 0, 0);
                        else
                            acc2[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, REAL ? f.b[b].x : f.b[b].y, acc2[a][b],
                                                                              0, 0, 0);
                    }
                if (!REAL) {
#pragma unroll
                    for (int b = 0; b < RN; ++b)
                        if (NOPRED || b < rnv) acc3[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(as, bs[b], acc3[a][b], 0, 0, 0);
                }
            }
        }
    };

    // Software pipeline (two LDS buffers, ONE barrier per tile, placed in the middle of the tile's
    // MFMA stream so that nothing waits on a fresh LDS/global access):
    //   iteration t:  read half-1 fragments of tile t | write tile t+1 (registers) to the other buffer,
    //                 issue the global loads of tile t+2 | MFMAs on half 0 | barrier |
    //                 read half-0 fragments of tile t+1 | MFMAs on half 1
    int nt = (kend - kbeg + LT_KT - 1) / LT_KT;
    Stage st;
    if (nt > 0) st = load_tile(kbeg);
    const bool direct = (slab == nullptr);
    cd* sl = direct ? nullptr : slab + (int64_t)z * m * n;
    for (int pass = 0;; ++pass) {
        if (nt > 0) {
            if (nt == 1) st = mask_tile(st, kbeg);
            store_tile(0, st, kbeg);
            if (nt > 1) st = load_tile(kbeg + LT_KT);
            __syncthreads();
            Frag f0 = read_frag(0, 0);
            int t = 0;
            if (FULL) {
                // steady state (tiles t+1, t+2, t+3 exist): one branch-free block, and the
                // scheduler is told to drop one memory instruction into the shadow of each MFMA so that this
                // wave alone keeps the matrix pipe fed (the two workgroups of a CU run in lockstep, so
                // "the other wave covers my memory phase" does not happen by itself).
                for (; t + 3 < nt; ++t) {   // tile t+2 is not the last one: it lies entirely inside the chunk
                    Frag f1 = read_frag(t & 1, 1);
                    store_tile((t + 1) & 1, st, kbeg + (t + 1) * LT_KT);
                    st = load_fast();
                    mfma_half(f0, std::true_type{});
#pragma unroll
                    for (int i = 0; i < GEMM_RM + RN; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // 1 DS read
                    }
#pragma unroll
                    for (int i = 0; i < 4 + RN / 2; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
                        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // 1 DS write
                        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // 1 VMEM read
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);   // pointer advance
                    }
                    __syncthreads();
                    f0 = read_frag((t + 1) & 1, 0);
                    mfma_half(f1, std::true_type{});
#pragma unroll
                    for (int i = 0; i < GEMM_RM + RN; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 2, 1);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
                    }
                }
            }
            for (; t < nt; ++t) {
                const bool more = (t + 1) < nt;
                Frag f1 = read_frag(t & 1, 1);
                if (more) {
                    if (t + 2 == nt) st = mask_tile(st, kbeg + (t + 1) * LT_KT);
                    store_tile((t + 1) & 1, st, kbeg + (t + 1) * LT_KT);
                    if (t + 2 < nt) st = load_tile(kbeg + (t + 2) * LT_KT);
                }
                if (active) mfma_half(f0, std::integral_constant<bool, FULL>{});
                __syncthreads();
                if (more) f0 = read_frag((t + 1) & 1, 0);
                if (active) mfma_half(f1, std::integral_constant<bool, FULL>{});
            }
        }
        if (!active) return;

        // epilogue
        const int j0 = J0, jm = jmin;
        const bool again = FOLD && pass == 0 && col2 >= 0;
        if (again) {
            // the second tile column: its first k-tile is loaded while the stores below drain.  (Every wave is past the last
            // barrier of the first tile and nothing reads LDS after it: the buffers are free.)
            tcn = col2 + ct0;
            shifted = tcn == shift_ct;
            J0 = shifted ? n - BN : tcn * BN;
            jmin = shifted ? tcn * BN : 0;
            kend = min(min(K, kbeg + kchunk), (upper & 2) ? J0 + BN : K);
            nt = (kend - kbeg + LT_KT - 1) / LT_KT;
            cB0 = (upper & 2) ? J0 + tc - tk : INT32_MAX;
            cB1 = (upper & 2) ? J0 + tc + 32 - tk : INT32_MAX;
            init_ptrs();
            if (nt > 0) st = load_tile(kbeg);
        }
#pragma unroll
        for (int a = 0; a < GEMM_RM; ++a)
#pragma unroll
            for (int b = 0; b < RN; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = i0 + a * 16 + lk + 4 * r;
                    const int gj = j0 + b * 16 + li;
                    if (gi < m && gj < n && gj >= jm && gi >= imin) {
                        const double p1 = acc1[a][b][r], p2 = acc2[a][b][r], p3 = acc3[a][b][r];
                        const double vr = REAL ? p1 : (CONJA ? p1 + p2 : p1 - p2);
                        const double vi = REAL ? (CONJA ? 0.0 : p2) : (CONJA ? p3 - p1 + p2 : p3 - p1 - p2);
                        if (direct) {
                            const int64_t off = gi + (int64_t)gj * ldc;
                            cd o = make_double2(alpha.x * vr - alpha.y * vi, alpha.x * vi + alpha.y * vr);
                            if (beta.x != 0.0 || beta.y != 0.0) {
                                const cd old = C[off];
                                o.x += beta.x * old.x - beta.y * old.y;
                                o.y += beta.x * old.y + beta.y * old.x;
                            }
                            D[off] = o;
                        } else {
                            sl[gi + (int64_t)gj * m] = make_double2(vr, vi);
                        }
                    }
                }
        if (!again) break;
#pragma unroll
        for (int a = 0; a < GEMM_RM; ++a)
#pragma unroll
            for (int b = 0; b < RN; ++b) {
                acc1[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
                acc2[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
                acc3[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
            }
    }
}

// C = alpha * sum_z slab[z] + beta * C   (fixed summation order).  The interior (i < mi, j < nj) and
// the ragged border have their own split counts / slabs; a count < 0 means that region was written
// directly by the GEMM kernel and is skipped here.  UPPER: entries of tiles that were not computed are skipped,
// tested on 128 x REDUCE_UPPER_BN blocks; with 128-row tiles that selects the same entries as a test on the
// 128 x 32 tiles of the complex products.
#define REDUCE_UPPER_BN 64
__global__ void k_zgemm_reduce(int m, int n, int mi, int nj, int nsI, const cd* __restrict__ slabI, int nsB,
                               const cd* __restrict__ slabB, const cd* C, cd* D, int64_t ldc, cd alpha, cd beta,
                               int upper) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)m * n) return;
    const int j = (int)(idx / m);
    const int i = (int)(idx - (int64_t)j * m);
    if ((upper & 1) &&
        (((i / GEMM_BM) * GEMM_BM) << ((upper >> 5) & 1)) >= min(n, (j / REDUCE_UPPER_BN) * REDUCE_UPPER_BN + REDUCE_UPPER_BN))
        return;   // tile not computed (a shifted last tile column ends at n: the kernel's own test)
    const bool interior = i < mi && j < nj;
    const int nsplit = interior ? nsI : nsB;
    const cd* slab = interior ? slabI : slabB;
    if (nsplit < 0) return;
    double sr = 0.0, si = 0.0;
    for (int z = 0; z < nsplit; ++z) {
        const cd v = slab[(int64_t)z * m * n + idx];
        sr += v.x;
        si += v.y;
    }
    const int64_t off = i + (int64_t)j * ldc;
    cd o = make_double2(alpha.x * sr - alpha.y * si, alpha.x * si + alpha.y * sr);
    if (beta.x != 0.0 || beta.y != 0.0) {
        const cd old = C[off];
        o.x += beta.x * old.x - beta.y * old.y;
        o.y += beta.x * old.y + beta.y * old.x;
    }
    D[off] = o;
}

// Reference kernel without matrix cores (debug path, env DFTK_MI_GEMM=naive): one thread per C entry.
template <bool CONJA>
__global__ void k_zgemm_naive(int m, int n, int K, const cd* __restrict__ A, int64_t lda,
                              const cd* __restrict__ B, int64_t ldb, const cd* C, cd* D, int64_t ldc, cd alpha,
                              cd beta, int real) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)m * n) return;
    const int j = (int)(idx / m);
    const int i = (int)(idx - (int64_t)j * m);
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < K; ++k) {
        cd a = CONJA ? A[k + (int64_t)i * lda] : A[i + (int64_t)k * lda];
        if (CONJA) a.y = -a.y;
        cd b = B[k + (int64_t)j * ldb];
        if (real && !CONJA) b.y = 0.0;
        sr += a.x * b.x - a.y * b.y;
        si += a.x * b.y + a.y * b.x;
    }
    if (real && CONJA) si = 0.0;
    const int64_t off = i + (int64_t)j * ldc;
    cd o = make_double2(alpha.x * sr - alpha.y * si, alpha.x * si + alpha.y * sr);
    if (beta.x != 0.0 || beta.y != 0.0) {
        const cd old = C[off];
        o.x += beta.x * old.x - beta.y * old.y;
        o.y += beta.x * old.y + beta.y * old.x;
    }
    D[off] = o;
}

// ---- diagnostic: pure v_mfma_f64_16x16x4_f64 issue rate (no memory traffic) -> measured ceiling
__global__ __launch_bounds__(256) void k_mfma_peak(int iters, double* out) {
    v4d acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    double a = 1.0 + threadIdx.x * 1e-9, bb = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[i], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[0] = s;   // keep the chain alive
}

// cycles per MFMA on one wave: out[1] = shader clocks, out[2] = 100 MHz wall ticks for `iters` x 8 MFMAs
template <int NACC>
__global__ __launch_bounds__(256) void k_mfma_cycles(int iters, double* out) {
    v4d acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    double a = 1.0 + threadIdx.x * 1e-9, bb = 1.0 - threadIdx.x * 1e-9;
    const long long c0 = clock64();
    const long long w0 = wall_clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            acc[i % NACC] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[i % NACC], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    const long long c1 = clock64();
    const long long w1 = wall_clock64();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[1] = (double)(c1 - c0);
        out[2] = (double)(w1 - w0);
        out[3] = s;
    }
}

extern "C" int dftk_mi_diag_mfma_peak(dftk_mi_basis* b, int waves_per_simd, int iters, double* tflops) {
    if (!b || !tflops || waves_per_simd < 1 || iters < 1) return DFTK_MI_EINVAL;
    HIPCHK(hipSetDevice(b->device));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const int blocks = 256 * waves_per_simd;       // 256 CUs x (4 waves per block = 1 per SIMD)
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, b->stream, 10, b->d_scalars);
    HIPCHK(hipEventRecord(e0, b->stream));
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, b->stream, iters, b->d_scalars);
    HIPCHK(hipEventRecord(e1, b->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    const double flops = (double)blocks * 4.0 * iters * 8.0 * 2048.0;
    *tflops = flops / (ms * 1e-3) / 1e12;
    for (int nacc : {8, 2, 1}) {
        if (nacc == 8) hipLaunchKernelGGL(k_mfma_cycles<8>, dim3(blocks), dim3(256), 0, b->stream, iters, b->d_scalars);
        if (nacc == 2) hipLaunchKernelGGL(k_mfma_cycles<2>, dim3(blocks), dim3(256), 0, b->stream, iters, b->d_scalars);
        if (nacc == 1) hipLaunchKernelGGL(k_mfma_cycles<1>, dim3(blocks), dim3(256), 0, b->stream, iters, b->d_scalars);
        HIPCHK(hipMemcpyAsync(b->h_scalars, b->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        fprintf(stderr, "[diag] %d wave(s)/SIMD, %d independent accumulators: %.1f shader clocks per MFMA, clock %.0f MHz\n",
                waves_per_simd, nacc, b->h_scalars[1] / (8.0 * iters), b->h_scalars[1] / (b->h_scalars[2] / 100.0));
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return 0;
}

int ensure_ws(dftk_mi_basis* b, size_t bytes) {
    return scratch_grow(b, b->ws, bytes, bytes / 4);
}

// ---------------------------------------------------------------------------------------- planning
// K split: chosen per launch by a small cost model of the actual workgroup -> XCD placement (8 XCDs x
// 64 resident workgroups, 2 per CU).  Candidates: ns chunks with either mapping of the kernel
//   row-major: (chunk, tile row) pairs round-robin over the XCDs, their column tiles together;
//   z-major  : whole chunks round-robin over the XCDs (A and B chunk both shared through one L2).
// cost = (rounds of the fullest XCD) x (chunk length + prologue/epilogue) + slab traffic.
// Short K is latency-bound: chunks of >= 8 tiles.  Plans are cached per shape.  Host-only code
// (dftk_mi_zgemm_plan_host exposes it to the CPU test-suite).
struct Split {
    int nsplit, kchunk;
    bool zmajor;
    cd* slab;
    bool compact = false;   // UPPER interior launch over the live tiles only (k_zgemm_3m, `upper & 16`)
    int live = 0;           // live tiles of the launch (compact: grid = 8 ceil(live nsplit / 8))
};
#define GEMM_SLOTS (256 * M3_MIN_BLOCKS)   // resident workgroups (256 CUs)
// `border`: the plan of a border launch (the plan cache key does not hold `live_rows`, which differ between the
// interior and the border launch of one shape)
static Split gemm_plan_split(int64_t m, int64_t n, int64_t k, int upper, const std::vector<int>& live_rows, bool border,
                             bool compact_ok = false, int rsc = 1) {
    const int64_t slots = GEMM_SLOTS;
    const int64_t plane = (int64_t)m * n * (int64_t)sizeof(cd);
    static std::map<std::vector<int64_t>, std::pair<int, int>> plan_cache;   // key -> (nsplit, zmajor)
    static std::mutex plan_mutex;   // host-only cache shared by every basis / thread of the process
    std::lock_guard<std::mutex> plan_lock(plan_mutex);
    // UPPER launches that cannot take the compact live-tile grid rotate the row panels over the XCDs (k_zgemm_3m,
    // `upper & 8`).  (measured, REAL Gram products of the 1000-electron cell: 503^2 UPPER 2.29 -> 1.90 ms with the
    //  rotation; at 1006^2 / 1509^2 -- 8 / 12 row panels -- the k-major mapping with whole chunks per XCD stays as fast or
    //  faster, so the rotated mapping only competes where an XCD would otherwise see at most 4 different row panels)
    const bool rot_rows = (upper & 1) && (int)live_rows.size() <= 4;
    int64_t total = 0;
    for (int v : live_rows) total += v;
    const int gm_s = (int)live_rows.size();
    // mapping of the launch: 0 row-major, 1 z-major, 2 compact (live tiles only, UPPER interior launches)
    int best_ns = 1, best_zm = compact_ok ? 2 : 0;
    if (k >= 128 && total > 0 && total < slots) {
        const std::vector<int64_t> key = {m, n, k, (int64_t)(upper & 1), (int64_t)border, (int64_t)rot_rows,
                                          (int64_t)compact_ok, (int64_t)rsc};
        auto it = plan_cache.find(key);
        if (it != plan_cache.end()) {
            best_ns = it->second.first;
            best_zm = it->second.second;
        } else {
            int64_t max_ns = k >= 2048 ? k / 256 : k / 64;
            if (max_ns > 1024) max_ns = 1024;
            const int64_t max_by_ws = (int64_t)(1024ull << 20) / plane;   // all slabs of a launch <= 1 GiB
            if (max_ns > max_by_ws) max_ns = max_by_ws;
            if (max_ns > 2 * slots / total + 8) max_ns = 2 * slots / total + 8;
            if (max_ns < 1) max_ns = 1;
            const double per_xcd = (double)slots / 8.0;
            const double slab_cost = 2.0 * (double)plane / 5e12 / 3.7e-6;   // k-tiles of time per extra chunk
            double best = 1e300;
            for (int ns = 1; ns <= max_ns; ++ns) {
                int kc = (int)((k + ns - 1) / ns);
                kc = (kc + 7) & ~7;
                if ((int)((k + kc - 1) / kc) != ns) continue;
                for (int zm = 0; zm < 3; ++zm) {
                    if (zm == 1 && (ns < 8 || k < 2048)) continue;
                    if (zm == 2 && !compact_ok) continue;
                    int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (zm == 2) {
                        load[0] = (total * ns + 7) / 8;   // equal contiguous blocks of work items
                    } else if (zm) {
                        for (int z = 0; z < ns; ++z) load[z & 7] += total;
                    } else {
                        const int64_t R = (int64_t)gm_s * ns;
                        const int g8 = (gm_s % 8 == 0) ? 8 : (gm_s % 4 == 0) ? 4 : (gm_s % 2 == 0) ? 2 : 1;
                        for (int64_t r = 0; r < R; ++r) {
                            const int64_t z = r / gm_s;
                            const int64_t row = rot_rows ? (r % gm_s + (z * g8) / 8) % gm_s : r % gm_s;
                            load[r & 7] += live_rows[row];
                        }
                    }
                    int64_t mx = 0;
                    for (int x = 0; x < 8; ++x) mx = load[x] > mx ? load[x] : mx;
                    const double rounds = std::ceil((double)mx / per_xcd);
                    const double cost = rounds * (kc / 8.0 + 12.0) + (ns > 1 ? slab_cost * ns : 0.0) - 1e-3 * zm;
                    if (cost < best) {
                        best = cost;
                        best_ns = ns;
                        best_zm = zm;
                    }
                }
            }
            if (plan_cache.size() > 4096) plan_cache.clear();
            plan_cache[key] = {best_ns, best_zm};
        }
    }
    int kc = (int)((k + best_ns - 1) / best_ns);
    kc = (kc + 7) & ~7;
    const int ns = (int)((k + kc - 1) / kc);
    Split sp{ns, kc, best_zm == 1 && ns >= 8, nullptr};
    sp.compact = best_zm == 2;
    sp.live = (int)total;
    return sp;
}

// Tiling of one product: interior rectangle of full 128 x BN tiles, ragged border as a list, and the K split of each.
struct GemmTiling {
    int BNt;     // column-tile width: M3_BN (complex products), M3_BN_REAL (REAL products, both operand layouts)
    int gm, gmf, gnf, gnt, nright, nbottom;
    int shift;   // 1: the ragged last tile column is a full tile shifted left, no right strip
    int gnI;     // tile columns of the interior launch = gnf + shift
    int shift_r; // 1: the ragged last tile row is a full tile shifted up, no bottom strip
    int gmI;     // tile rows of the interior launch = gmf + shift_r
    Split I, B;
};
// rsc: REAL rows per row of C in the (upper & 1) tile test -- 2 for the symmetric result of a tall REAL 'N' product
// (GEMM_SYM_RESULT), 1 otherwise
static GemmTiling gemm_tiling(int64_t m, int64_t n, int64_t k, int upper, bool real, int rsc = 1) {
    GemmTiling t;
    t.BNt = real ? M3_BN_REAL : M3_BN;
    t.gm = (int)((m + GEMM_BM - 1) / GEMM_BM);
    t.gnt = (int)((n + t.BNt - 1) / t.BNt);
    t.gmf = (int)(m / GEMM_BM);
    t.gnf = (int)(n / t.BNt);
    t.shift = (t.gnt > t.gnf && t.gnf >= 1) ? 1 : 0;
    t.gnI = t.gnf + t.shift;
    t.shift_r = (t.gm > t.gmf && t.gmf >= 1) ? 1 : 0;
    t.gmI = t.gmf + t.shift_r;
    t.nright = (t.gnt > t.gnf && !t.shift) ? t.gm : 0;
    t.nbottom = (t.gm > t.gmf && !t.shift_r) ? t.gnI : 0;
    // live column tiles per tile row of each launch (upper: only tiles that intersect the upper triangle)
    auto live = [&](int tr, int tc) {
        const int64_t jend = (t.shift && tc == t.gnf) ? n : (int64_t)tc * t.BNt + t.BNt;
        return !(upper & 1) || (int64_t)tr * GEMM_BM * rsc < jend;
    };
    std::vector<int> rowsI(t.gmI, 0), rowsB(t.nright + t.nbottom, 0);
    for (int tr = 0; tr < t.gmI; ++tr)
        for (int tc = 0; tc < t.gnI; ++tc) rowsI[tr] += live(tr, tc) ? 1 : 0;
    for (int e = 0; e < t.nright; ++e) rowsB[e] = live(e, t.gnf) ? 1 : 0;
    for (int e = 0; e < t.nbottom; ++e) rowsB[t.nright + e] = live(t.gmf, e) ? 1 : 0;
    // compact UPPER launches (k_zgemm_3m, `upper & 16`): the kernel rebuilds the live tile list as "row panel r keeps its
    // column tiles >= r BM / BN" -- only used when that is exactly the list above
    bool compact_ok = (upper & 1) && (GEMM_BM * rsc) % t.BNt == 0;
    for (int tr = 0; tr < t.gmI && compact_ok; ++tr)
        compact_ok = rowsI[tr] == std::max(0, t.gnI - tr * (GEMM_BM * rsc / t.BNt));
    t.I = gemm_plan_split(m, n, k, upper, rowsI, false, compact_ok, rsc);
    t.B = gemm_plan_split(m, n, k, upper, rowsB, true, false, rsc);
    return t;
}
// Does GEMM_SYM_RESULT pay for the 'N' product m x n x k?  Only where the FULL product, at the K split its plan chooses, holds
// more workgroups than are resident at once: the flag then saves a whole round of workgroups.  Below that the K split
// already fills the chip in one round, the flag only shortens the chunks a little, and the caller's mirror pass costs more
// (measured, REAL tall: 1006^2 -- 64 tiles x 8 chunks = one round -- heev 5.60 -> 5.99 ms per call with the flag;
// 1509^2 -- 144 tiles x 6 chunks, two rounds -> 84 x 6, one -- 8.55 -> 7.35 and 19.7 -> 17.6 ms)
bool zgemm_sym_result_pays(int64_t m, int64_t n, int64_t k, bool real) {
    if (m <= 0 || n <= 0 || k <= 0) return false;
    const GemmTiling t = gemm_tiling(m, n, k, 0, real);
    return (int64_t)t.gmI * t.gnI * t.I.nsplit > GEMM_SLOTS;
}

// Triangular B ('N', no UPPER) whose interior launch has no K split: two column tiles per workgroup (k_zgemm_3m, FOLD)
static bool gemm_folds(const GemmTiling& t, bool conja, int upper) {
    return !conja && (upper & 3) == 2 && t.I.nsplit == 1 && !t.I.zmajor && t.gmI >= 1 && t.gnI >= 2;
}
// Host-only: the (tile row, tile column, first k, end k) of every tile a FOLD launch runs, in workgroup order, 4 ints per
// tile; *count = 0 when the shape does not take the folded launch (CPU test-suite: every tile of the plan exactly once)
int zgemm_fold_host(char transA, int64_t m, int64_t n, int64_t k, int flags, int cap, int* items4, int* count) {
    if (m <= 0 || n <= 0 || k <= 0 || (flags & ~(3 | DFTK_MI_GEMM_REAL)) || cap < 0 || !count || (cap > 0 && !items4))
        return DFTK_MI_EINVAL;
    const GemmTiling t = gemm_tiling(m, n, k, flags & 3, (flags & DFTK_MI_GEMM_REAL) != 0);
    *count = 0;
    if (!gemm_folds(t, transA == 'C' || transA == 'c', flags & 3)) return 0;
    const int nblk = ((t.gmI + 7) / 8) * 8 * ((t.gnI + 1) / 2);
    for (int id = 0; id < nblk; ++id) {
        int row, c[2];
        if (!gemm_fold_item(id, t.gmI, t.gnI, &row, &c[0], &c[1])) continue;
        for (int i = 0; i < 2; ++i) {
            if (c[i] < 0) continue;
            if (*count < cap) {
                const int64_t j0 = (t.shift && c[i] == t.gnf) ? n - t.BNt : (int64_t)c[i] * t.BNt;
                int* e = items4 + 4 * (int64_t)*count;
                e[0] = row; e[1] = c[i]; e[2] = 0; e[3] = (int)std::min<int64_t>(k, j0 + t.BNt);
            }
            ++*count;
        }
    }
    return 0;
}

// Host-only: the (k-chunk, tile row, tile column) of every workgroup with work of a compact UPPER launch, in workgroup
// order, 3 ints per item (CPU test-suite: every live (chunk, tile) exactly once, no dead one)
int zgemm_compact_host(int gm, int gn, int q, int nsplit, int cap, int* items3, int* count) {
    if (gm <= 0 || gn <= 0 || q <= 0 || nsplit <= 0 || cap < 0 || !count || (cap > 0 && !items3)) return DFTK_MI_EINVAL;
    int64_t live = 0;
    for (int r = 0; r < gm; ++r) live += std::max(0, gn - r * q);
    const int64_t nblk = ((live * nsplit + 7) / 8) * 8;   // the grid of the launch (zgemm_to)
    if (nblk > INT32_MAX) return DFTK_MI_EINVAL;
    *count = 0;
    for (int id = 0; id < (int)nblk; ++id) {
        int z, row, col;
        if (!gemm_compact_item(id, gm, gn, q, nsplit, &z, &row, &col)) continue;
        if (*count < cap) {
            int* e = items3 + 3 * (int64_t)*count;
            e[0] = z; e[1] = row; e[2] = col;
        }
        ++*count;
    }
    return 0;
}

int zgemm_plan_host(char transA, int64_t m, int64_t n, int64_t k, int flags, int* out) {
    if (m <= 0 || n <= 0 || k <= 0 || (flags & ~(3 | DFTK_MI_GEMM_REAL | DFTK_MI_GEMM_SYM_RESULT)) || !out) return DFTK_MI_EINVAL;
    (void)transA;   // both operand layouts share one plan
    const bool real = (flags & DFTK_MI_GEMM_REAL) != 0, sym = (flags & DFTK_MI_GEMM_SYM_RESULT) != 0;
    const GemmTiling t = gemm_tiling(m, n, k, (flags & 3) | (sym ? 1 : 0), real, (sym && real) ? 2 : 1);
    const int v[12] = {t.BNt, t.gmf, t.gnf, t.nright, t.nbottom, t.I.nsplit, t.I.kchunk, t.I.compact ? 2 : t.I.zmajor ? 1 : 0,
                       t.B.nsplit, t.B.kchunk, t.B.zmajor ? 1 : 0, t.shift};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return 0;
}

int zgemm(dftk_mi_basis* b, char transA, int64_t m, int64_t n, int64_t k, cd alpha, const cd* A, int64_t lda,
          const cd* B, int64_t ldb, cd beta, cd* C, int64_t ldc, int upper_in) {
    return zgemm_to(b, transA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, C, upper_in);
}

// D = alpha op(A) B + beta C: the product above with its result in a second array of C's shape and leading dimension.  The
// k order and the epilogue arithmetic are those of the in-place product (D == C); C is only read, and only where beta != 0.
int zgemm_to(dftk_mi_basis* b, char transA, int64_t m, int64_t n, int64_t k, cd alpha, const cd* A, int64_t lda,
             const cd* B, int64_t ldb, cd beta, const cd* C, int64_t ldc, cd* D, int upper_in) {
    const bool real = (upper_in & DFTK_MI_GEMM_REAL) != 0;   // operands are real-symmetric half-sphere blocks
    if (m <= 0 || n <= 0) return 0;
    const bool conja = (transA == 'C' || transA == 'c');
    // GEMM_SYM_RESULT ('N' only): the tile test of UPPER, on REAL rows (two per row of C) for a REAL product
    const bool sym = (upper_in & GEMM_SYM_RESULT) != 0;
    if (sym && conja) {
        dftk_set_error("zgemm: GEMM_SYM_RESULT is a flag of 'N' products");
        return DFTK_MI_EINVAL;
    }
    const int upper = (upper_in & 3) | (sym ? 1 : 0);
    const int rsc = (sym && real) ? 2 : 1;
    if (!conja && !(transA == 'N' || transA == 'n')) {
        dftk_set_error("zgemm: transA must be 'N' or 'C'");
        return DFTK_MI_EINVAL;
    }
    if (m > INT32_MAX || n > INT32_MAX || k > INT32_MAX) return DFTK_MI_EINVAL;
    if (batching()) {   // a fiber of a batched multi-k call: recorded, merged with its siblings' products later
        if (D != C) {
            dftk_set_error("zgemm: a recorded product of a batched call writes its result in place");
            return DFTK_MI_EINVAL;
        }
        BOp o;
        o.b = b;
        o.type = BOP_ZGEMM; o.trans = conja ? 'C' : 'N'; o.gm = m; o.gn = n; o.gk = k; o.alpha = alpha; o.A = A; o.lda = lda;
        o.B = B; o.ldb = ldb; o.beta = beta; o.C = D; o.ldc = ldc;
        o.flags = upper_in & ~GEMM_SYM_RESULT;   // (the merged products know no symmetric result: the full product is computed)
        return batch_record(std::move(o));
    }
    if (k <= 0) {   // C = beta * C : run the reduce kernel over zero slabs
        hipLaunchKernelGGL(k_zgemm_reduce, dim3((unsigned)((m * n + 255) / 256)), dim3(256), 0, b->stream, (int)m,
                           (int)n, (int)m, (int)n, 0, (const cd*)nullptr, 0, (const cd*)nullptr, C, D, ldc, alpha, beta, 0);
        HIPCHK(hipGetLastError());
        return 0;
    }
    static const bool trace = getenv("DFTK_MI_TRACE_GEMM") != nullptr;
    if (trace) fprintf(stderr, "[zgemm] %c %lld %lld %lld\n", transA, (long long)m, (long long)n, (long long)k);
    static const bool shapes_env = getenv("DFTK_MI_GEMM_SHAPES") != nullptr;
    const bool shapes = shapes_env || (b->prof && b->prof->shape_tags);
    const uint64_t tag = !shapes ? 0
                                 // (bit 63 transA, 62 "tagged", 61 REAL, 42..60 m, 40..41 UPPER / B_UPPER, 22..39 n, 0..21 k)
                                 : ((uint64_t)conja << 63) | ((uint64_t)(m & 0x7FFFF) << 42) | ((uint64_t)(real ? 1 : 0) << 61) |
                                       ((uint64_t)(n & 0x3FFFF) << 22) | ((uint64_t)(upper_in & 3) << 40) |
                                       (uint64_t)(k & 0x3FFFFF) | (1ull << 62);
    const GemmTiling til = gemm_tiling(m, n, k, upper, real, rsc);
    // Flop booking (bench.py roofline).  `useful` = the part of the product that is mathematically needed:
    // 8mnk for an unstructured call, only the (i <= j) entries of C for UPPER, only k <= j for a triangular B.
    // `executed` = what the launched tiles really run on the matrix pipe (whole tiles, shifted-tile and border
    // recompute included; 6 real flops per complex multiply-add in the 3M kernel, 4 in a REAL product).
    double useful = 0.0, executed = 0.0;
    if (b->prof && b->prof->on) {
        // a REAL call is a real GEMM with twice the rows (or inner dimension): 2 * (2 m n k) flops, no 3M saving
        const double mac_useful = real ? 4.0 : 8.0;
        if (!(upper & 3)) {
            useful = mac_useful * (double)m * (double)n * (double)k;
        } else {
            for (int64_t j = 0; j < n; ++j) {
                // (symmetric tall REAL result: the j + 1 REAL rows at or above the diagonal are (j + 1) / 2 rows of C)
                const double rows = (upper & 1) ? std::min((double)m, (double)(j + 1) / rsc) : (double)m;
                const double kk = (upper & 2) ? (double)std::min<int64_t>(k, j + 1) : (double)k;
                useful += mac_useful * rows * kk;
            }
        }
        const double per_mac = real ? 4.0 : b->use_mfma ? 6.0 : 8.0;
        const int BNt = til.BNt;
        auto kext = [&](int tc) {   // k range a tile column runs (triangular B stops at the diagonal)
            const int64_t j0 = (til.shift && tc == til.gnf) ? n - BNt : (int64_t)tc * BNt;
            return (double)((upper & 2) ? std::min<int64_t>(k, j0 + BNt) : k);
        };
        auto live = [&](int64_t i0, int tc) {
            const int64_t jend = (til.shift && tc == til.gnf) ? n : std::min<int64_t>(n, (int64_t)tc * BNt + BNt);
            return !(upper & 1) || i0 * rsc < jend;
        };
        for (int tr = 0; tr < til.gmI; ++tr)
            for (int tc = 0; tc < til.gnI; ++tc)
                if (live((int64_t)tr * GEMM_BM, tc)) executed += per_mac * GEMM_BM * BNt * kext(tc);
        const int64_t mrem = m - (int64_t)til.gmf * GEMM_BM;
        const double rows_b = (double)(((mrem + 31) / 32) * 32);   // border: 32-row wave tiles that hold rows run
        for (int tc = 0; tc < til.nbottom; ++tc)
            if (live((int64_t)til.gmf * GEMM_BM, tc)) executed += per_mac * rows_b * BNt * kext(tc);
        for (int tr = 0; tr < til.nright; ++tr) {
            const double rr = tr < til.gmf ? (double)GEMM_BM : rows_b;
            if (live((int64_t)tr * GEMM_BM, til.gnf)) executed += per_mac * rr * BNt * kext(til.gnf);
        }
        if (!b->use_mfma) executed = useful;
    }
    const int slot = prof_begin(b, (upper & 3) ? PROF_ZGEMM_STRUCT : PROF_ZGEMM, useful, tag);
    if (slot >= 0) {
        b->prof->work[PROF_ZGEMM_BYTES] += 16.0 * ((double)m * k + (double)k * n +
                                                   (double)m * n * ((beta.x != 0.0 || beta.y != 0.0) ? 2.0 : 1.0));
        b->prof->work[PROF_ZGEMM_EXEC] += executed;
        b->prof->work[PROF_ZGEMM_CPLX] += real ? 2.0 * useful : useful;
    }
    struct ProfGuard {
        dftk_mi_basis* b;
        int s;
        ~ProfGuard() { prof_end(b, s); }
    } guard{b, slot};
    if (!b->use_mfma) {
        const unsigned blocks = (unsigned)((m * n + 255) / 256);
        if (conja)
            hipLaunchKernelGGL(k_zgemm_naive<true>, dim3(blocks), dim3(256), 0, b->stream, (int)m, (int)n, (int)k, A,
                               lda, B, ldb, C, D, ldc, alpha, beta, real ? 1 : 0);
        else
            hipLaunchKernelGGL(k_zgemm_naive<false>, dim3(blocks), dim3(256), 0, b->stream, (int)m, (int)n, (int)k,
                               A, lda, B, ldb, C, D, ldc, alpha, beta, real ? 1 : 0);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int64_t plane = (int64_t)m * n * (int64_t)sizeof(cd);
    // XCD-aware 1-D grid over a gm_s x gn_s sub-grid of tiles (x nsplit K chunks)
    auto grid_for = [&](int gm_s, int gn_s, int ns) -> int64_t {
        const int64_t rows_total = (int64_t)gm_s * ns;
        return ((rows_total + 7) / 8) * 8 * gn_s;
    };
    // Full tiles run the predicate-free instantiation (a ragged last tile column as one more full tile,
    // shifted left); the remaining ragged strips the predicated one, as ONE list-shaped launch (right strip:
    // all tile rows of the last tile column; bottom strip: the tile columns of the last tile row) with its own
    // K split.  (One mixed launch over all tiles was measured 2-7 % faster on the block updates, but the light
    // border workgroups run ahead of their siblings through k and FETCH_SIZE rose from 2.3x to 3.5x the
    // operand bytes -- dropped.)
    const int BNt = til.BNt, gmf = til.gmf, gnf = til.gnf, nright = til.nright, nbottom = til.nbottom;
    Split spI = til.I, spB = til.B;
    const size_t bytesI = spI.nsplit > 1 ? (size_t)spI.nsplit * plane : 0;
    const size_t bytesB = spB.nsplit > 1 ? (size_t)spB.nsplit * plane : 0;
    if (bytesI + bytesB) CHK(ensure_ws(b, bytesI + bytesB));
    if (bytesI) spI.slab = (cd*)b->ws.get();
    if (bytesB) spB.slab = (cd*)((char*)b->ws.get() + bytesI);
    auto launch = [&](int mode, int gm_s, int gn_s, int rt0, int ct0, int lsplit, const Split& sp) -> int {
        if (gm_s <= 0 || gn_s <= 0) return 0;
        const bool zmajor = sp.zmajor;
        const bool compact = sp.compact && mode == 1 && lsplit < 0;
        // triangular B without a K split: two column tiles per workgroup (k_zgemm_3m, FOLD)
        const bool fold = mode == 1 && lsplit < 0 && gemm_folds(til, conja, upper);
        const int64_t nblk = fold      ? grid_for(gm_s, (gn_s + 1) / 2, 1)
                             : compact ? (((int64_t)sp.live * sp.nsplit + 7) / 8) * 8
                             : zmajor  ? (int64_t)((sp.nsplit + 7) / 8) * 8 * gm_s * gn_s
                                       : grid_for(gm_s, gn_s, sp.nsplit);
        if (nblk > INT32_MAX) return DFTK_MI_EINVAL;
        dim3 grid((unsigned)nblk);
        const int kupper = upper | (compact ? 16 : zmajor ? 4 : 0) | ((!compact && !zmajor && (upper & 1) && gm_s <= 4) ? 8 : 0) |
                           (rsc == 2 ? 32 : 0);
#define DFTK_LAUNCH_3M(CJ, MD)                                                                                         \
    if (real) DFTK_LAUNCH_3M_(CJ, MD, true, M3_RN_REAL, false);                                                        \
    else DFTK_LAUNCH_3M_(CJ, MD, false, M3_RN, false)
#define DFTK_LAUNCH_3M_(CJ, MD, RL, RNN, FD)                                                                           \
    hipLaunchKernelGGL((k_zgemm_3m<CJ, MD, RL, RNN, FD>), grid, dim3(GEMM_WAVES * 64), 0, b->stream, (int)m, (int)n, (int)k,  \
                       sp.kchunk, gm_s, gn_s, rt0, ct0, lsplit, kupper, til.shift ? gnf : -1,                          \
                       (til.shift_r && lsplit < 0) ? gmf : -1, sp.nsplit, A, lda, B, ldb, C, D,                        \
                       ldc, alpha, beta, sp.slab)
        // mode 1 = full tiles, 0 = predicated border
        if (conja) {
            if (mode == 1) { DFTK_LAUNCH_3M(true, 1); }
            else { DFTK_LAUNCH_3M(true, 0); }
        } else if (fold) {
            if (real) DFTK_LAUNCH_3M_(false, 1, true, M3_RN_REAL, true);
            else DFTK_LAUNCH_3M_(false, 1, false, M3_RN, true);
        } else {
            if (mode == 1) { DFTK_LAUNCH_3M(false, 1); }
            else { DFTK_LAUNCH_3M(false, 0); }
        }
#undef DFTK_LAUNCH_3M
#undef DFTK_LAUNCH_3M_
        return 0;
    };
    CHK(launch(1, til.gmI, til.gnI, 0, 0, -1, spI));
    CHK(launch(0, nright + nbottom, 1, gmf, gnf, nright, spB));
    if (spI.slab || spB.slab)
        hipLaunchKernelGGL(k_zgemm_reduce, dim3((unsigned)((m * n + 255) / 256)), dim3(256), 0, b->stream, (int)m,
                           (int)n, til.shift_r ? (int)m : gmf * GEMM_BM, til.shift ? (int)n : gnf * BNt, spI.slab ? spI.nsplit : -1, spI.slab,
                           spB.slab ? spB.nsplit : -1, spB.slab, C, D, ldc, alpha, beta, upper | (rsc == 2 ? 32 : 0));
    HIPCHK(hipGetLastError());
    return 0;
}
