// lights_plan.h — how xrt_light_hits splits a list of hits into chunks: pure host arithmetic beside pixels_plan.h.  It includes nothing of
// HIP and touches no scene, so a program without a GPU covers it (tests/lights/host_lights.cpp).
//
// A chunk of m entries holds, in this seam's own work buffers, per (entry, light) pair a shadow ray (32 bytes), its hit (48 bytes), its
// hit / miss word (4 bytes) -- the 84 bytes per path and light of a frame context -- and the scatter word of the compact ray list (4 bytes).
// The sum over a chunk's pairs stays within the byte budget (Settings::shadowBytes), and a chunk has at most LIGHT_CHUNK_MAX_PAIRS pairs
// (they are counted in an int) and LIGHT_CHUNK_MAX_ENTRIES entries.  Nothing about the answers depends on the split: every entry is
// answered by the same code whichever chunk it falls into.
#pragma once
#include <cstdint>
#include <vector>

namespace xrt {

constexpr long long LIGHT_CHUNK_MAX_PAIRS = 1LL << 30, LIGHT_CHUNK_MAX_ENTRIES = 1LL << 30;
constexpr uint64_t LIGHT_PAIR_BYTES = 32u + 48u + 4u + 4u;

// Bytes one entry of a chunk accounts for.  64-bit throughout.  (No lights: nothing is traced, an entry holds nothing.)
inline uint64_t light_entry_bytes(int nLights) { return LIGHT_PAIR_BYTES * (uint64_t)(nLights > 0 ? nLights : 0); }

// Most entries of one chunk: at least 1 (an entry is never split, whatever the budget).
inline long long light_chunk_entries(int nLights, uint64_t budgetBytes) {
    uint64_t m = (uint64_t)LIGHT_CHUNK_MAX_ENTRIES;
    if (nLights > 0) {
        const uint64_t byBytes = budgetBytes / light_entry_bytes(nLights), byPairs = (uint64_t)LIGHT_CHUNK_MAX_PAIRS / (uint64_t)nLights;
        if (byBytes < m) m = byBytes;
        if (byPairs < m) m = byPairs;
    }
    if (m < 1) m = 1;
    return (long long)m;
}

// Chunk boundaries b[0] = 0 < b[1] < .. < b[k] = n: chunk c is entries [b[c], b[c + 1]).  n <= 0: {0} (no chunk).  The chunks are equal but for
// the last, which is the shortest.
inline std::vector<long long> light_chunks(long long n, int nLights, uint64_t budgetBytes) {
    std::vector<long long> b;
    b.push_back(0);
    if (n <= 0) return b;
    const long long m = light_chunk_entries(nLights, budgetBytes);
    for (long long at = 0; at < n;) {
        at = (n - at <= m) ? n : at + m;
        b.push_back(at);
    }
    return b;
}

}  // namespace xrt
