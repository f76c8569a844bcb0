// host_packed_check -- packed_items of csrc/packed.h (the table of work items under the packed-vector solvers) on the host,
// without a GPU: the host part of the header is compiled alone (DFTK_PACKED_HOST_ONLY) and no HIP runtime function is called.
// For rows 1, 1023, 1024, 1025, 4097 x cols 1, 3, 33 x 1 to 3 unequal blocks: every (block, column, row) is covered by
// exactly one item, off is the unpadded packed position, total / total_cols / col0 agree with the sizes; and every refusal.
// exit 0 + "host_packed_check OK" when every case holds.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#define DFTK_PACKED_HOST_ONLY
#include "../dftk.jl_amd/csrc/packed.h"

static char g_error[512];
void dftk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            failures += 1;                                             \
            printf("line %d: %s FAILED\n", __LINE__, #cond);           \
        }                                                              \
    } while (0)

// the blocks of a case, unequal in rows and columns (the shapes of the GPU tests)
static void shapes(int64_t rows, int cols, int n_blocks, int64_t* r, int* c) {
    const int64_t rr[3] = {rows, rows / 2 + 1, rows + 7};
    const int cc[3] = {cols, cols + 2, cols > 1 ? cols - 1 : 1};
    for (int i = 0; i < n_blocks; ++i) r[i] = rr[i], c[i] = cc[i];
}

static void check_case(int64_t rows, int cols, int n_blocks) {
    int64_t r[3];
    int c[3];
    shapes(rows, cols, n_blocks, r, c);
    std::vector<PackedItem> items;
    std::vector<int64_t> col0;
    int64_t total = -1, total_cols = -1;
    EXPECT(packed_items("check", n_blocks, r, c, &items, &total, &total_cols, &col0) == 0);
    int64_t want_total = 0, want_cols = 0;
    EXPECT((int)col0.size() == n_blocks);
    for (int i = 0; i < n_blocks; ++i) {
        EXPECT(col0[i] == want_cols);
        want_total += r[i] * c[i];
        want_cols += c[i];
    }
    EXPECT(total == want_total && total_cols == want_cols);
    // seen[packed position] counts the items that cover it; the position of (block, column, row) is recomputed here
    std::vector<int> seen((size_t)want_total, 0);
    std::vector<int64_t> base(n_blocks, 0);
    for (int i = 1; i < n_blocks; ++i) base[i] = base[i - 1] + r[i - 1] * c[i - 1];
    for (const PackedItem& it : items) {
        const bool inside = it.b >= 0 && it.b < n_blocks && it.col >= 0 && it.col < c[it.b] && it.row0 >= 0 && it.nrows >= 1 &&
                            it.nrows <= PACKED_CH && (int64_t)it.row0 + it.nrows <= r[it.b];
        EXPECT(inside);
        if (!inside) return;
        EXPECT(it.row0 % PACKED_CH == 0);
        EXPECT(it.off == base[it.b] + (int64_t)it.col * r[it.b] + it.row0);
        for (int k = 0; k < it.nrows; ++k) seen[(size_t)(base[it.b] + (int64_t)it.col * r[it.b] + it.row0 + k)] += 1;
    }
    int64_t bad = 0;
    for (int v : seen) bad += v != 1;
    EXPECT(bad == 0);
    int64_t want_items = 0;
    for (int i = 0; i < n_blocks; ++i) want_items += c[i] * ((r[i] + PACKED_CH - 1) / PACKED_CH);
    EXPECT((int64_t)items.size() == want_items);
}

static void check_refusal(int64_t rows, int cols, const char* what) {
    for (int at = 0; at < 2; ++at) {                      // the bad block first, then second
        int64_t r[2] = {65, 65};
        int c[2] = {3, 3};
        r[at] = rows, c[at] = cols;
        std::vector<PackedItem> items;
        std::vector<int64_t> col0;
        int64_t total = 0, total_cols = 0;
        g_error[0] = 0;
        EXPECT(packed_items("check", 2, r, c, &items, &total, &total_cols, &col0) == DFTK_MI_EINVAL);
        char want[64];
        snprintf(want, sizeof want, "check: block %d is ", at);
        EXPECT(strncmp(g_error, want, strlen(want)) == 0);
        if (failures) printf("  (%s: \"%s\")\n", what, g_error);
    }
}

int main() {
    const int64_t ROWS[] = {1, 1023, 1024, 1025, 4097};
    const int COLS[] = {1, 3, 33};
    for (int64_t rows : ROWS)
        for (int cols : COLS)
            for (int n_blocks = 1; n_blocks <= 3; ++n_blocks) check_case(rows, cols, n_blocks);
    check_refusal(0, 3, "rows < 1");
    check_refusal(-5, 3, "rows < 1");
    check_refusal(65, 0, "cols < 1");
    check_refusal(65, -2, "cols < 1");
    check_refusal((int64_t)INT32_MAX - PACKED_CH + 1, 1, "rows > INT32_MAX - 1024");
    {   // the largest row count that is accepted: the last item ends at the last row
        int64_t r[1] = {(int64_t)INT32_MAX - PACKED_CH};
        int c[1] = {1};
        std::vector<PackedItem> items;
        std::vector<int64_t> col0;
        int64_t total = 0, total_cols = 0;
        EXPECT(packed_items("check", 1, r, c, &items, &total, &total_cols, &col0) == 0);
        EXPECT(!items.empty() && (int64_t)items.back().row0 + items.back().nrows == r[0] && total == r[0]);
    }
    if (failures) {
        printf("host_packed_check: %d FAILED\n", failures);
        return 1;
    }
    printf("host_packed_check OK\n");
    return 0;
}
