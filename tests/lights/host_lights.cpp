// host_lights.cpp -- how xrt_light_hits splits a list of hits into chunks (csrc/lights_plan.h), checked on the host: no device, no scene.
// Built by `make hostcheck_lights` (csrc/Makefile) under ASan and UBSan and run by tests/test_lights_cpu.py; UBSan is what watches the products
// entries * lights and entries * bytes, which pass 2^31 and 2^32 below.
//   hostcheck_lights                          -> the checks; prints "host_lights: ok"
//   hostcheck_lights --plan n lights budget   -> the boundaries of that one plan, a line of integers
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../xna-ray-trace_amd/csrc/lights_plan.h"

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

// Every entry once, in order; chunks within the budget (or of one entry), the pair limit and the entry limit; equal but for the last.
static void check_plan(long long n, int lights, uint64_t budget) {
    const std::vector<long long> b = light_chunks(n, lights, budget);
    const uint64_t per = light_entry_bytes(lights);
    CHECK(!b.empty() && b.front() == 0, "n %lld", n);
    CHECK(b.back() == (n > 0 ? n : 0), "n %lld back %lld", n, b.back());
    CHECK(n > 0 || b.size() == 1, "n %lld", n);
    for (size_t c = 0; c + 1 < b.size(); c++) {
        const long long m = b[c + 1] - b[c];
        CHECK(m > 0, "n %lld chunk %zu empty", n, c);
        CHECK(m <= LIGHT_CHUNK_MAX_ENTRIES, "n %lld chunk %zu has %lld entries", n, c, m);
        CHECK(lights <= 0 || m == 1 || m * (long long)lights <= LIGHT_CHUNK_MAX_PAIRS, "n %lld chunk %zu has %lld pairs", n, c, m * (long long)lights);
        if (per > 0 && budget >= per) CHECK((uint64_t)m * per <= budget, "n %lld chunk %zu: %" PRIu64 " bytes over %" PRIu64, n, c, (uint64_t)m * per, budget);
        else if (per > 0) CHECK(m == 1, "n %lld chunk %zu: %lld entries under a budget below one entry", n, c, m);
        CHECK(c + 2 == b.size() || m == b[1] - b[0], "n %lld chunk %zu: %lld entries, the first has %lld", n, c, m, b[1] - b[0]);
        CHECK(m <= b[1] - b[0], "n %lld chunk %zu is longer than the first", n, c);
    }
    const long long fit = light_chunk_entries(lights, budget);
    if (n > 0 && n <= fit) CHECK(b.size() == 2, "n %lld fits and is %zu chunks", n, b.size() - 1);
    if (n > 0) CHECK((long long)b.size() - 1 == (n + fit - 1) / fit, "n %lld: %zu chunks of %lld", n, b.size() - 1, fit);
}

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "--plan")) {
        for (long long v : light_chunks(atoll(argv[2]), atoi(argv[3]), strtoull(argv[4], nullptr, 10))) std::printf("%lld ", v);
        std::printf("\n");
        return 0;
    }
    const long long ns[] = {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 100003, 1920LL * 1080, (1LL << 30) - 1, 1LL << 30, (1LL << 30) + 1, (1LL << 31) + 7, 1LL << 33};
    const uint64_t budgets[] = {1, 87, 88, 89, 175, 176, 1000, 1 << 20, 1ull << 30, 8ull << 30, 1ull << 40, ~0ull};
    int plans = 0;
    for (int lights : {0, 1, 2, 33, 128, 100000, 0x7fffffff})
        for (long long n : ns)
            for (uint64_t budget : budgets) {
                if (n / light_chunk_entries(lights, budget) > (1 << 20)) continue;   // (more than a million chunks say nothing more)
                check_plan(n, lights, budget);
                plans++;
            }
    // the sizes themselves
    CHECK(LIGHT_PAIR_BYTES == 88, "pair bytes");
    CHECK(light_entry_bytes(0) == 0 && light_entry_bytes(-3) == 0 && light_entry_bytes(1) == 88 && light_entry_bytes(128) == 88 * 128, "entry bytes");
    CHECK(light_entry_bytes(0x7fffffff) > (1ull << 37), "entry bytes in 64 bits");
    // one entry; a budget below one entry's bytes; exact multiples
    CHECK(light_chunks(1, 2, 1).size() == 2 && light_chunks(1, 2, 1)[1] == 1, "one entry under any budget");
    CHECK(light_chunk_entries(2, 175) == 1 && light_chunk_entries(2, 176) == 1 && light_chunk_entries(2, 351) == 1 && light_chunk_entries(2, 352) == 2, "entries of a budget");
    CHECK(light_chunks(5, 128, 100).size() == 6, "a budget below one entry: one entry per chunk");
    CHECK(light_chunks(3000, 1, 88 * 1000).size() == 4 && light_chunks(3001, 1, 88 * 1000).size() == 5 && light_chunks(2999, 1, 88 * 1000).size() == 4, "exact multiples");
    CHECK(light_chunks(3001, 1, 88 * 1000).back() == 3001 && light_chunks(3001, 1, 88 * 1000)[3] == 3000, "the last chunk is the shortest");
    // pairs are counted in an int: 2^30 at most, whatever the budget; and without lights only the entry limit splits
    CHECK(light_chunk_entries(128, ~0ull) == (1LL << 30) / 128 && light_chunk_entries(3, ~0ull) == (1LL << 30) / 3, "the pair limit");
    CHECK(light_chunk_entries(0, 1) == (1LL << 30) && light_chunks(1LL << 33, 0, 1).size() == 9, "no lights");
    std::printf("plans %d\n", plans);
    if (g_failures) { std::printf("host_lights: %d FAILED\n", g_failures); return 1; }
    std::printf("host_lights: ok\n");
    return 0;
}
