// host_trace.cpp -- how xrt_trace_pixels splits a centre list into chunks (csrc/trace_plan.h), checked on the host: no device, no scene.
// Built by `make hostcheck_trace` (csrc/Makefile) under ASan and UBSan and run by tests/test_trace_pixels_cpu.py; UBSan is what watches the products
// n * samples and entries * bytes, which pass 2^31 and 2^32 below.
//   hostcheck_trace                                -> the checks; prints "host_trace: ok"
//   hostcheck_trace --plan n samples budget hinted -> the boundaries of that one plan, a line of integers
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../xna-ray-trace_amd/csrc/trace_plan.h"

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

// Every entry once, in order; chunks within the budget (with the table where hinted) and the place limit; the starts on multiples of 4 entries.
static void check_plan(long long n, int samples, uint64_t budget, bool hinted) {
    const std::vector<long long> b = trace_chunks(n, samples, budget, hinted);
    const uint64_t per = trace_entry_bytes(samples);
    CHECK(!b.empty() && b.front() == 0, "n %lld", n);
    CHECK(b.back() == (n > 0 ? n : 0), "n %lld back %lld", n, b.back());
    CHECK(n > 0 || b.size() == 1, "n %lld", n);
    const bool roomForFour = trace_chunk_bytes(4, samples, hinted) <= budget;
    for (size_t c = 0; c + 1 < b.size(); c++) {
        const long long m = b[c + 1] - b[c];
        CHECK(m > 0, "n %lld chunk %zu empty", n, c);
        CHECK(b[c] % 4 == 0, "n %lld chunk %zu starts at %lld", n, c, b[c]);
        CHECK(m * samples <= PIXEL_CHUNK_MAX_RAYS, "n %lld chunk %zu has %lld places", n, c, m * samples);
        if (roomForFour) CHECK(trace_chunk_bytes(m, samples, hinted) <= budget, "n %lld samples %d hinted %d chunk %zu: %" PRIu64 " bytes over %" PRIu64, n, samples, (int)hinted, c, trace_chunk_bytes(m, samples, hinted), budget);
        else CHECK(m <= 4, "n %lld chunk %zu: %lld entries under a budget below four entries", n, c, m);
        CHECK(c + 2 == b.size() || m == b[1] - b[0], "n %lld chunk %zu: %lld entries, the first has %lld", n, c, m, b[1] - b[0]);
    }
    if (n > 0 && trace_chunk_bytes(n, samples, hinted) <= budget && (uint64_t)n * per <= budget && n * samples <= PIXEL_CHUNK_MAX_RAYS)
        CHECK(b.size() == 2, "n %lld fits and is %zu chunks", n, b.size() - 1);
}

int main(int argc, char **argv) {
    if (argc == 6 && !std::strcmp(argv[1], "--plan")) {
        for (long long v : trace_chunks(atoll(argv[2]), atoi(argv[3]), strtoull(argv[4], nullptr, 10), atoi(argv[5]) != 0)) std::printf("%lld ", v);
        std::printf("\n");
        return 0;
    }
    const long long ns[] = {0, 1, 3, 4, 5, 63, 64, 65, 4096, 4097, 5184, 1920LL * 1080, 3840LL * 2160, (1LL << 27) + 1, 1LL << 28, (1LL << 31) + 7, (1LL << 32) + 1};
    const uint64_t budgets[] = {1, 35, 36, 143, 144, 576, 1000, 36 * 1000, 36 * 1000 + 1, 1 << 20, 1ull << 30, 4ull << 30, 1ull << 40, ~0ull};
    int plans = 0;
    for (int samples : {1, 16})
        for (bool hinted : {false, true})
            for (long long n : ns)
                for (uint64_t budget : budgets) {
                    if (n / trace_chunk_entries(samples, budget, hinted) > (1 << 20)) continue;   // (more than a million chunks say nothing more)
                    check_plan(n, samples, budget, hinted);
                    plans++;
                }
    // n * samples past 2^31 and 2^32: 2^28 entries of sixteen samples under a budget that holds them all are split by the place limit alone
    for (bool hinted : {false, true}) {
        const std::vector<long long> b = trace_chunks(1LL << 28, 16, ~0ull, hinted);
        CHECK(b.size() == 17, "%zu boundaries", b.size());
        for (size_t c = 0; c + 1 < b.size(); c++) CHECK(b[c + 1] - b[c] == (1LL << 24), "chunk %zu", c);
    }
    {   // more than 2^31 one-sample entries: 2^28 places a chunk
        const std::vector<long long> b = trace_chunks((1LL << 31) + 5, 1, ~0ull, false);
        CHECK(b.size() == 10 && b[8] == (1LL << 31) && b.back() == (1LL << 31) + 5, "%zu boundaries", b.size());
    }
    // the sizes themselves
    CHECK(trace_entry_bytes(1) == 36 && trace_entry_bytes(16) == 576, "entry bytes");
    CHECK(trace_chunk_bytes(1000, 1, false) == 36000 && trace_chunk_bytes(1000, 1, true) == 36000 + 512 + 8 * 16, "chunk bytes, one sample");
    CHECK(trace_chunk_bytes(5, 16, true) == 5 * 576 + 512 + 8 * 2, "chunk bytes, sixteen samples: 80 places are two units");
    CHECK(trace_chunk_entries(1, 36 * 1000 + 35, false) == 1000 && trace_chunk_entries(1, 36 * 1003, false) == 1000, "entries are a multiple of 4");
    CHECK(trace_chunk_entries(1, 36 * 1000, true) < 1000, "the table takes room");
    CHECK(trace_chunk_entries(16, 1, true) == 4 && trace_chunk_entries(1, 0, false) == 4, "never fewer than four entries");
    std::printf("plans %d\n", plans);
    if (g_failures) { std::printf("host_trace: %d FAILED\n", g_failures); return 1; }
    std::printf("host_trace: ok\n");
    return 0;
}
