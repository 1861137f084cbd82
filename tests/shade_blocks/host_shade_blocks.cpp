// host_shade_blocks.cpp -- the grid of a k_shade launch (csrc/kernels.h shade_grid_blocks) and the XRT_SHADE_BLOCK switch (csrc/settings.h), checked on the
// host: no device, no scene.  Built by `make hostcheck_shade_blocks` (csrc/Makefile) under ASan and UBSan and run by tests/test_shade_blocks_cpu.py.
//   hostcheck_shade_blocks   -> the checks; prints "host_shade_blocks: ok"
#include <cstdio>
#include <cstdlib>

#include "../../xna-ray-trace_amd/csrc/kernels.h"
#include "../../xna-ray-trace_amd/csrc/settings.h"

using namespace xrt;

static int g_failures = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            g_failures++;                                       \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                           \
            std::printf("\n");                                  \
        }                                                       \
    } while (0)

static int block_with(const char *value) {
    if (value) setenv("XRT_SHADE_BLOCK", value, 1);
    else unsetenv("XRT_SHADE_BLOCK");
    return read_settings().shadeBlock;
}

int main() {
    // the grids the two fixed sizes had: 1024 blocks of 1024, 4096 of 256
    CHECK(shade_grid_blocks(-1, 1024) == 1024 && shade_grid_blocks(-1, 256) == 4096, "%d %d", shade_grid_blocks(-1, 1024), shade_grid_blocks(-1, 256));
    int sizes = 0;
    for (int t = SHADE_BLOCK_MIN; t <= SHADE_BLOCK_MAX; t += 64, sizes++) {
        const long long cap = shade_grid_blocks(-1, t);
        // an unknown generation: the fewest blocks that hold 2^20 threads
        CHECK(cap * t >= SHADE_GRID_THREADS && (cap - 1) * t < SHADE_GRID_THREADS, "threads %d cap %lld", t, cap);
        const long long rays[] = {0, 1, 63, t - 1, t, t + 1, 2LL * t, 36561, 4 * 131072 + 4096, SHADE_GRID_THREADS - 1, SHADE_GRID_THREADS, SHADE_GRID_THREADS + 1,
                                  4LL * 33177600 + 4096, (1LL << 31) + 5, 1LL << 40};
        for (long long n : rays) {
            const long long b = shade_grid_blocks(n, t);
            CHECK(b >= 1 && b <= cap, "threads %d rays %lld blocks %lld", t, n, b);
            // a thread per ray (the hint is in rays, whatever the block size) until the cap; never a block more than that needs
            CHECK(b == cap || b * t >= n, "threads %d rays %lld blocks %lld", t, n, b);
            CHECK(b == 1 || (b - 1) * t < n, "threads %d rays %lld blocks %lld", t, n, b);
        }
    }
    CHECK(sizes == 13, "%d", sizes);
    // the switch: 256 .. 1024 in steps of 64; anything else leaves the default
    const int dflt = block_with(nullptr);
    CHECK(dflt >= SHADE_BLOCK_MIN && dflt <= SHADE_BLOCK_MAX && dflt % 64 == 0, "default %d", dflt);
    for (int t = SHADE_BLOCK_MIN; t <= SHADE_BLOCK_MAX; t += 64) {
        char buf[16];
        std::snprintf(buf, sizeof buf, "%d", t);
        CHECK(block_with(buf) == t, "%d", t);
    }
    for (const char *bad : {"0", "64", "192", "255", "300", "770", "1025", "1088", "2048", "-768", "", "big"})
        CHECK(block_with(bad) == dflt, "XRT_SHADE_BLOCK=%s -> %d", bad, block_with(bad));
    std::printf("default %d\n", dflt);
    if (g_failures) { std::printf("host_shade_blocks: %d FAILED\n", g_failures); return 1; }
    std::printf("host_shade_blocks: ok\n");
    return 0;
}
