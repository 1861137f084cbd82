// host_pixels.cpp -- how xrt_render_pixels splits a centre list into chunks (csrc/pixels_plan.h), checked on the host: no device, no scene.
// Built by `make hostcheck_pixels` (csrc/Makefile) under ASan and UBSan and run by tests/test_pixels_cpu.py; UBSan is what watches the products
// n * samples and entries * bytes, which pass 2^31 and 2^32 below.
//   hostcheck_pixels                                        -> the checks; prints "host_pixels: ok"
//   hostcheck_pixels --plan n mode quality lights budget    -> the boundaries of that one plan, a line of integers
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../xna-ray-trace_amd/csrc/pixels_plan.h"

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

// Every entry once, in order; chunks within the budget and the ray limit; the starts on multiples of 4 entries.
static void check_plan(long long n, int mode, int quality, int lights, uint64_t budget) {
    const std::vector<long long> b = pixel_chunks(n, mode, quality, lights, budget);
    const uint64_t per = pixel_entry_bytes(mode, quality, lights);
    const long long samples = pixel_samples(mode);
    CHECK(!b.empty() && b.front() == 0, "n %lld", n);
    CHECK(b.back() == (n > 0 ? n : 0), "n %lld back %lld", n, b.back());
    CHECK(n > 0 || b.size() == 1, "n %lld", n);
    long long longest = 0;
    for (size_t c = 0; c + 1 < b.size(); c++) {
        const long long m = b[c + 1] - b[c];
        CHECK(m > 0, "n %lld chunk %zu empty", n, c);
        CHECK(b[c] % 4 == 0, "n %lld chunk %zu starts at %lld", n, c, b[c]);
        CHECK(m * samples <= PIXEL_CHUNK_MAX_RAYS, "n %lld chunk %zu has %lld rays", n, c, m * samples);
        if (budget >= 4 * per) CHECK((uint64_t)m * per <= budget, "n %lld chunk %zu: %" PRIu64 " bytes over %" PRIu64, n, c, (uint64_t)m * per, budget);
        else CHECK(m <= 4, "n %lld chunk %zu: %lld entries under a budget below four entries", n, c, m);
        if (m > longest) longest = m;
        CHECK(c + 2 == b.size() || m == b[1] - b[0], "n %lld chunk %zu: %lld entries, the first has %lld", n, c, m, b[1] - b[0]);
    }
    if (n > 0 && (uint64_t)n * per <= budget && n * samples <= PIXEL_CHUNK_MAX_RAYS) CHECK(b.size() == 2, "n %lld fits and is %zu chunks", n, b.size() - 1);
}

int main(int argc, char **argv) {
    if (argc == 7 && !std::strcmp(argv[1], "--plan")) {
        for (long long v : pixel_chunks(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), strtoull(argv[6], nullptr, 10))) std::printf("%lld ", v);
        std::printf("\n");
        return 0;
    }
    const int modes[3] = {XRT_MS_OFF, XRT_MS_ADAPTIVE, XRT_MS_FIXED16};
    const long long ns[] = {0, 1, 3, 4, 5, 63, 64, 65, 4096, 4097, 5184, 1920LL * 1080, 3840LL * 2160, (1LL << 27) + 1, 1LL << 28, (1LL << 31) + 7};
    const uint64_t budgets[] = {1, 1000, 1 << 20, 1ull << 30, 4ull << 30, 1ull << 40, ~0ull};
    int plans = 0;
    for (int mode : modes)
        for (int quality : {0, 2, 6})
            for (int lights : {0, 1, 100})
                for (long long n : ns)
                    for (uint64_t budget : budgets) {
                        if (n / pixel_chunk_entries(mode, quality, lights, budget) > (1 << 20)) continue;   // (more than a million chunks say nothing more)
                        check_plan(n, mode, quality, lights, budget);
                        plans++;
                    }
    // n * samples past 2^31 and 2^32: 2^28 entries of sixteen samples under a budget that holds them all are split by the ray limit alone
    {
        const std::vector<long long> b = pixel_chunks(1LL << 28, XRT_MS_FIXED16, 0, 1, ~0ull);
        CHECK(b.size() == 17, "%zu boundaries", b.size());
        for (size_t c = 0; c + 1 < b.size(); c++) CHECK(b[c + 1] - b[c] == (1LL << 24), "chunk %zu", c);
    }
    // the sizes themselves
    CHECK(pixel_samples(XRT_MS_OFF) == 1 && pixel_samples(XRT_MS_ADAPTIVE) == 4 && pixel_samples(XRT_MS_FIXED16) == 16, "samples");
    CHECK(pixel_entry_bytes(XRT_MS_OFF, 0, 0) == 116 && pixel_entry_bytes(XRT_MS_OFF, 0, 2) == 116 + 168, "entry bytes, one sample");
    CHECK(pixel_entry_bytes(XRT_MS_FIXED16, 0, 1) == 16 * 200, "entry bytes, sixteen samples");
    CHECK(pixel_entry_bytes(XRT_MS_ADAPTIVE, 3, 1) == 4 * 200 + 24, "entry bytes, adaptive");
    CHECK(pixel_entry_bytes(XRT_MS_FIXED16, 0, 0x7fffffff) > (1ull << 40), "entry bytes in 64 bits");
    CHECK(pixel_chunk_entries(XRT_MS_OFF, 0, 1, 200 * 1000 + 199) == 1000, "entries of a budget");
    CHECK(pixel_chunk_entries(XRT_MS_OFF, 0, 1, 200 * 1003) == 1000, "entries are a multiple of 4");
    std::printf("plans %d\n", plans);
    if (g_failures) { std::printf("host_pixels: %d FAILED\n", g_failures); return 1; }
    std::printf("host_pixels: ok\n");
    return 0;
}
