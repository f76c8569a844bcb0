// host_devbuf_check -- the owner type of csrc/devbuf.h on the host, without a GPU: the header's one extension point
// (DFTK_DEVBUF_ALLOC / DFTK_DEVBUF_FREE) is pointed at fakes that hand out host memory, count calls, remember what is live
// and can be told to fail the k-th allocation.  Checked: alloc / reserve / reset / move keep the call counts and the two
// live counters exact; a reserve that fits allocates nothing; a reserve whose allocation fails returns the error and leaves
// an EMPTY owner (null, 0 bytes -- never the old capacity with a null pointer); a struct of several owners whose k-th
// allocation fails frees exactly the k - 1 earlier ones, for every k; nothing is freed twice; nothing is live at the end.
// exit 0 + "host_devbuf_check OK" when every case holds.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

enum class Mem;
static int g_allocs = 0, g_frees = 0, g_fail_at = 0, g_bad_frees = 0;   // g_fail_at: the k-th allocation from now fails
static std::set<void*> g_live;
static hipError_t fake_alloc(Mem, void** p, size_t bytes) {
    if (g_fail_at > 0 && --g_fail_at == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
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
#include "../dftk.jl_amd/csrc/devbuf.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            failures += 1;                                             \
            printf("line %d: %s FAILED\n", __LINE__, #cond);           \
        }                                                              \
    } while (0)

static bool live_is(int64_t count, int64_t bytes) {
    return g_devbuf_live_count.load() == count && g_devbuf_live_bytes.load() == bytes && (int64_t)g_live.size() == count;
}

struct Five {     // a handle-like struct: the members are released in reverse order when it goes out of scope
    DevBuf<double> a;
    DevTable<int> b;
    DevBuf<void> c;
    DevTable<double> d;
    DevBuf<char> e;
    hipError_t build() {
        hipError_t s;
        if ((s = a.alloc(100)) != hipSuccess) return s;
        if ((s = b.alloc(200)) != hipSuccess) return s;
        if ((s = c.alloc(300)) != hipSuccess) return s;
        if ((s = d.alloc(400)) != hipSuccess) return s;
        return e.alloc(500);
    }
};

int main() {
    {   // alloc / reserve / reset
        DevBuf<double> x;
        EXPECT(x.get() == nullptr && x.bytes() == 0 && live_is(0, 0));
        EXPECT(x.alloc(64) == hipSuccess && x.get() != nullptr && x.bytes() == 64 && live_is(1, 64) && g_allocs == 1);
        double* p = x;                                          // implicit conversion
        EXPECT(p == x.get() && (x ? true : false));
        EXPECT(x.reserve(64) == hipSuccess && x.reserve(10) == hipSuccess && g_allocs == 1 && x.get() == p);   // fits
        EXPECT(x.reserve(100, 25) == hipSuccess && x.bytes() == 125 && g_allocs == 2 && g_frees == 1 && live_is(1, 125));
        EXPECT(x.alloc(32) == hipSuccess && x.bytes() == 32 && g_allocs == 3 && g_frees == 2 && live_is(1, 32));   // exact
        EXPECT(x.alloc(0) == hipSuccess && x.get() == nullptr && x.bytes() == 0 && g_frees == 3 && live_is(0, 0));
        EXPECT(x.reset() == hipSuccess && g_frees == 3);        // empty: nothing to free
        EXPECT(x.alloc(8) == hipSuccess && live_is(1, 8));
    }
    EXPECT(g_allocs == 4 && g_frees == 4 && live_is(0, 0));     // the destructor freed
    {   // a grow whose allocation fails: the error comes back and the owner is EMPTY
        DevBuf<double> t1;
        EXPECT(t1.reserve(1000) == hipSuccess && t1.bytes() == 1000);
        g_fail_at = 1;
        EXPECT(t1.reserve(2000) == hipErrorOutOfMemory);
        EXPECT(t1.get() == nullptr && t1.bytes() == 0 && live_is(0, 0));
        EXPECT(t1.reserve(500) == hipSuccess && t1.get() != nullptr && t1.bytes() == 500);   // a smaller request allocates
        g_fail_at = 1;
        EXPECT(t1.alloc(10) == hipErrorOutOfMemory && t1.get() == nullptr && t1.bytes() == 0 && live_is(0, 0));
    }
    EXPECT(live_is(0, 0) && g_allocs == g_frees);
    {   // move construction and move assignment
        DevTable<int> a, b;
        EXPECT(a.alloc(40) == hipSuccess && b.alloc(60) == hipSuccess && live_is(2, 100));
        int* pa = a;
        DevTable<int> c(std::move(a));
        EXPECT(c.get() == pa && c.bytes() == 40 && a.get() == nullptr && a.bytes() == 0 && live_is(2, 100));
        const int frees = g_frees;
        b = std::move(c);                                       // frees b's 60 bytes, takes c's
        EXPECT(g_frees == frees + 1 && b.get() == pa && b.bytes() == 40 && c.get() == nullptr && live_is(1, 40));
        b = std::move(b);                                       // self-move: nothing happens
        EXPECT(b.get() == pa && live_is(1, 40));
    }
    EXPECT(live_is(0, 0) && g_allocs == g_frees);
    {   // pinned memory goes through the same owner and is not counted as device memory
        PinnedBuf<double> h;
        Buf<char, Mem::PinnedMapped> m;
        const int allocs = g_allocs;
        EXPECT(h.reserve(256, 64) == hipSuccess && h.bytes() == 320 && m.alloc(16) == hipSuccess && g_allocs == allocs + 2);
        EXPECT(g_devbuf_live_count.load() == 0 && g_devbuf_live_bytes.load() == 0 && g_live.size() == 2);
    }
    EXPECT(live_is(0, 0) && g_allocs == g_frees);
    for (int k = 1; k <= 6; ++k) {   // the k-th allocation of a struct of five owners fails (k = 6: none does)
        const int allocs = g_allocs, frees = g_frees;
        {
            Five f;
            g_fail_at = k;
            const hipError_t s = f.build();
            g_fail_at = 0;
            EXPECT((s == hipSuccess) == (k == 6));
            EXPECT(g_allocs == allocs + (k <= 5 ? k - 1 : 5) && g_frees == frees);
            EXPECT(g_devbuf_live_count.load() == (k <= 5 ? k - 1 : 5));
        }
        EXPECT(g_frees == frees + (k <= 5 ? k - 1 : 5) && live_is(0, 0));
    }
    EXPECT(g_bad_frees == 0);
    EXPECT(g_allocs == g_frees && live_is(0, 0));
    if (failures) {
        printf("host_devbuf_check: %d checks FAILED\n", failures);
        return 1;
    }
    printf("host_devbuf_check OK (%d allocations, %d frees)\n", g_allocs, g_frees);
    return 0;
}
