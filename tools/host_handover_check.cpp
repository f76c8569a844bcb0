// host_handover_check -- LobHandover of csrc/handover.h (what a k-block keeps between two dftk_mi_lobpcg calls) on the host,
// without a GPU: the allocate / free macros of csrc/devbuf.h are pointed at fakes that hand out host memory and remember
// what is live, and the transition table at the top of handover.h is walked row by row.  The pointers handed to the object
// are never dereferenced by it; they only have to be distinct.
// exit 0 + "host_handover_check OK" when every case holds.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <set>

enum class Mem;
static int g_allocs = 0, g_frees = 0, g_bad_frees = 0;
static std::set<void*> g_live;
static hipError_t fake_alloc(Mem, void** p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    g_allocs += 1;
    return hipSuccess;
}
static hipError_t fake_free(Mem, void* p) {
    if (g_live.erase(p) != 1) {       // freed twice, or never allocated
        g_bad_frees += 1;
        return hipErrorInvalidValue;
    }
    free(p);
    g_frees += 1;
    return hipSuccess;
}
#define DFTK_DEVBUF_ALLOC fake_alloc
#define DFTK_DEVBUF_FREE fake_free
#include "../dftk.jl_amd/csrc/handover.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            failures += 1;                                             \
            printf("line %d: %s FAILED\n", __LINE__, #cond);           \
        }                                                              \
    } while (0)

// the shapes of the walk: M = 7 bands (4 pairs, the last holds one band), launch groups of 3 pairs (the second ragged)
static const int M = 7, BATCH = 3;
static const int64_t N = 100, LD = 128, LDX = 200;
static cd g_ax[1], g_x[1], g_other[1];
static cd* const AX = g_ax;
static const cd* const X = g_x;

static bool nothing(const LobHandover::Taken& t) { return t.AX == nullptr && !t.planes; }
static bool block_only(const LobHandover::Taken& t) { return t.AX == AX && t.ld == LD && !t.planes; }
static bool block_and_planes(const LobHandover::Taken& t) { return t.AX == AX && t.ld == LD && t.planes; }
static LobHandover::Taken take(LobHandover& h, bool eligible = true) { return h.take(M, N, false, eligible, BATCH); }

// rows "keep + returned", "density pass over the returned X" with every launch group run, "promise" (row 7's state)
// (ret_nb: the band count recorded with the returned X; begin_nb: the one the density pass begins with)
static void kept_with_planes(LobHandover& h, int ret_nb = M, int begin_nb = M) {
    h.keep(AX, LD, M, N);
    h.returned(X, LDX, ret_nb);
    EXPECT(h.pass_keeps_planes(X, LDX, ret_nb));
    if (!h.planes) EXPECT(h.planes.alloc(64) == hipSuccess);
    h.planes_begin(begin_nb, BATCH);
    const int nb2 = (begin_nb + 1) / 2;
    for (int p0 = 0; p0 < nb2; p0 += BATCH) h.planes_mark(p0, nb2 - p0 < BATCH ? nb2 - p0 : BATCH);
    h.promise(true);
}

int main() {
    {   // 1. a fresh object gives nothing
        LobHandover h;
        EXPECT(nothing(take(h)) && h.last_AX() == nullptr && !h.pass_keeps_planes(X, LDX, M));
    }
    {   // 2. keep -> promise -> take returns the block; a second take returns nothing
        LobHandover h;
        h.keep(AX, LD, M, N);
        h.promise(true);
        EXPECT(block_only(take(h)));
        EXPECT(nothing(take(h)));
        h.promise(true);                                   // (nothing is kept any more)
        EXPECT(nothing(take(h)));
    }
    {   // 3. keep -> take without a promise returns nothing, and the block is gone afterwards (a call of the small driver in
        //    between two promised calls: the workspace it lives in has been overwritten)
        LobHandover h;
        h.keep(AX, LD, M, N);
        EXPECT(nothing(take(h)));
        h.promise(true);
        EXPECT(nothing(take(h)));
        h.keep(AX, LD, M, N);                              // promise(0) withdraws
        h.promise(true);
        h.promise(false);
        EXPECT(nothing(take(h)));
    }
    for (int k = 0; k < 3; ++k) {   // 4. promised, but another M, another N, or a moving workspace: nothing, block gone
        LobHandover h;
        h.keep(AX, LD, M, N);
        h.promise(true);
        EXPECT(nothing(h.take(k == 0 ? M + 1 : M, k == 1 ? N + 1 : N, k == 2, true, BATCH)));
        h.promise(true);
        EXPECT(nothing(take(h)));
    }
    {   // 5. promise(1) with nothing kept stays false
        LobHandover h;
        h.promise(true);
        h.keep(AX, LD, M, N);                              // (kept AFTER the promise: that promise was about nothing)
        EXPECT(nothing(take(h)));
    }
    {   // 6. forget() after promise: nothing, and a later promise(1) stays false
        LobHandover h;
        kept_with_planes(h);
        h.forget();
        EXPECT(!h.pass_keeps_planes(X, LDX, M));
        h.promise(true);
        EXPECT(nothing(take(h)));
    }
    {   // 7. keep + returned, begin, all groups marked, promise, eligible take: A X and planes; all of it is spent then
        LobHandover h;
        kept_with_planes(h);
        EXPECT(block_and_planes(take(h)));
        const std::vector<char>& valid = h.planes_consume();
        EXPECT(valid.size() == 4 && valid[0] && valid[1] && valid[2] && valid[3]);
        EXPECT(!h.pass_keeps_planes(X, LDX, M));           // the returned block is forgotten
        h.promise(true);
        EXPECT(nothing(take(h)));
        // a group the density pass skipped stays unmarked: the planes are usable, the consumer fills that group itself
        h.keep(AX, LD, M, N);
        h.returned(X, LDX, M);
        h.planes_begin(M, BATCH);
        h.planes_mark(3, 1);
        h.promise(true);
        EXPECT(block_and_planes(take(h)));
        const std::vector<char>& v2 = h.planes_consume();
        EXPECT(v2.size() == 4 && !v2[0] && !v2[1] && !v2[2] && v2[3]);
    }
    {   // 8. as 7, one condition of the planes missing at a time: A X still returned, planes refused
        LobHandover h;
        kept_with_planes(h);
        EXPECT(block_only(h.take(M, N, false, true, BATCH + 1)));        // another fft_batch
        kept_with_planes(h, M, M - 2);                                   // a valid vector of 3 entries, not 4
        EXPECT(block_only(take(h)));
        kept_with_planes(h, M, M + 2);                                   // ... of 5
        EXPECT(block_only(take(h)));
        kept_with_planes(h, M + 1, M + 1);                               // 8 bands: 4 entries, but not the M of this call
        EXPECT(block_only(take(h)));
        kept_with_planes(h);
        EXPECT(block_only(take(h, /*eligible=*/false)));                 // not eligible
        kept_with_planes(h);
        h.planes_off();                                                  // planes off
        EXPECT(block_only(take(h)));
        kept_with_planes(h);
        (void)h.planes_consume();                                        // ... or spent already
        EXPECT(block_only(take(h)));
        kept_with_planes(h);
        EXPECT(h.planes.reset() == hipSuccess);                          // ... or the buffer is gone
        EXPECT(block_only(take(h)));
    }
    for (int k = 0; k < 4; ++k) {   // 9. planes are never usable when A X was not returned
        LobHandover h;
        kept_with_planes(h);
        if (k == 3) h.promise(false);
        EXPECT(nothing(h.take(k == 0 ? M + 1 : M, k == 1 ? N + 1 : N, k == 2, true, BATCH)));
    }
    {   // 10. a pass that keeps nothing: planes off, returned block remembered; a later pass over it may keep planes again
        LobHandover h;
        kept_with_planes(h);
        EXPECT(!h.pass_keeps_planes(g_other, LDX, M) && !h.pass_keeps_planes(X, LDX + 1, M) && !h.pass_keeps_planes(X, LDX, M - 1));
        h.planes_off();
        EXPECT(h.pass_keeps_planes(X, LDX, M));
        h.planes_begin(M, BATCH);
        h.planes_mark(0, 3);
        h.planes_mark(3, 1);
        EXPECT(block_and_planes(take(h)));
    }
    {   // 11. forget_planes() leaves the kept A X and the promise alone
        LobHandover h;
        kept_with_planes(h);
        h.forget_planes();
        EXPECT(!h.pass_keeps_planes(X, LDX, M));
        EXPECT(block_only(take(h)));
    }
    {   // 12. declined is sticky
        LobHandover h;
        kept_with_planes(h);
        h.planes_decline();
        EXPECT(!h.pass_keeps_planes(X, LDX, M));
        (void)take(h);
        h.forget();
        h.keep(AX, LD, M, N);
        h.returned(X, LDX, M);
        EXPECT(!h.pass_keeps_planes(X, LDX, M));
    }
    {   // last_AX is a plain borrowed pointer: no transition touches it
        LobHandover h;
        h.set_last_AX(AX);
        kept_with_planes(h);
        (void)take(h);
        h.forget();
        EXPECT(h.last_AX() == AX);
    }
    EXPECT(g_live.empty() && g_allocs == g_frees && g_devbuf_live_count.load() == 0 && g_devbuf_live_bytes.load() == 0);
    {   // 13. destruction frees each of the three buffers once, and nothing is live at the end
        const int allocs = g_allocs, frees = g_frees;
        {
            LobHandover h;
            EXPECT(h.V_kept.alloc(800) == hipSuccess && h.dV.alloc(800) == hipSuccess && h.planes.alloc(1600) == hipSuccess);
            EXPECT(g_allocs == allocs + 3 && g_frees == frees && g_live.size() == 3);
            EXPECT(g_devbuf_live_count.load() == 3 && g_devbuf_live_bytes.load() == 3200);   // (dftk_mi_device_buffers_live)
            kept_with_planes(h);
            (void)take(h);
            h.forget();                                    // no transition frees or allocates
            EXPECT(g_allocs == allocs + 3 && g_frees == frees);
        }
        EXPECT(g_frees == frees + 3 && g_live.empty());
    }
    EXPECT(g_bad_frees == 0);
    EXPECT(g_allocs == g_frees && g_devbuf_live_count.load() == 0 && g_devbuf_live_bytes.load() == 0);
    if (failures) {
        printf("host_handover_check: %d checks FAILED\n", failures);
        return 1;
    }
    printf("host_handover_check OK (%d allocations, %d frees)\n", g_allocs, g_frees);
    return 0;
}
