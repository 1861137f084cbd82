// pixels_plan.h — how xrt_render_pixels splits a centre list into chunks: pure host arithmetic beside frame_plan.h.  It includes nothing of
// HIP and touches no scene, so a program without a GPU covers it (tests/pixels/host_pixels.cpp).
//
// A chunk of m entries holds, in this seam's own work buffers, m * samples rays (32 bytes) and as many packed sample colours (4 bytes), and the
// pass that traces them (xrt_cast_rays' pipeline) holds per ray of a chunk a hit record (48 bytes), its ray again (32 bytes) and per light a
// shadow ray, its hit and its hit / miss word (84 bytes).  The sum over a chunk's rays stays within the byte budget, and a chunk has at most
// PIXEL_CHUNK_MAX_RAYS rays (one xrt_cast_rays call takes 2^30).  Nothing about the answers depends on the split: every entry is traced by the
// same code whichever chunk it falls into.
//   samples: 1 (XRT_MS_OFF; the colours go straight to the caller's array, the 4 bytes are counted all the same), 16 (XRT_MS_FIXED16), 4
//   (XRT_MS_ADAPTIVE: the level-0 quadrant of an entry.  With quality > 0 an entry also keeps a child base and a child mask per level it may
//   reach, 8 bytes each; how many quadrants the deeper levels have only the device knows, so their buffers are sized by the counts read back
//   and their rays are cast through this same split, as lists of quadrants).
//   A hinted chunk (xrt.h XRT_LIST_COHERENT) whose first launch is a packet launch also has a packet table (kernels.h QuadTable): two count words on
//   256-byte lines of their own, 512 bytes, and one 8-byte entry per 64 places of the chunk -- place r is sample r % samples of entry r / samples, the
//   last unit may be partial.  The accounting includes it for every hinted chunk, whichever kernel the scene's rule picks.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/xrt.h"

namespace xrt {

constexpr long long PIXEL_CHUNK_MAX_RAYS = 1LL << 28;

inline int pixel_samples(int msMode) { return msMode == XRT_MS_FIXED16 ? 16 : (msMode == XRT_MS_ADAPTIVE ? 4 : 1); }

// Bytes one entry of a chunk accounts for (see above).  64-bit throughout: 100 lights and 16 samples are 135 KB per entry.
inline uint64_t pixel_entry_bytes(int msMode, int quality, int nLights) {
    const uint64_t samples = (uint64_t)pixel_samples(msMode);
    const uint64_t perRay = 32u + 4u + 48u + 32u + 84ull * (uint64_t)(nLights > 0 ? nLights : 0);
    uint64_t b = samples * perRay;
    if (msMode == XRT_MS_ADAPTIVE && quality > 0) b += 8ull * (uint64_t)quality;
    return b;
}

// The packet table of a hinted chunk of `rays` places: its entries, and its bytes with the two count lines.
constexpr uint64_t PIXEL_TABLE_HEAD_BYTES = 512, PIXEL_TABLE_ENTRY_BYTES = 8;
inline uint64_t pixel_table_entries(uint64_t rays) { return (rays + 63) / 64; }
inline uint64_t pixel_table_bytes(uint64_t rays) { return PIXEL_TABLE_HEAD_BYTES + PIXEL_TABLE_ENTRY_BYTES * pixel_table_entries(rays); }

// Bytes a chunk of m entries accounts for.
inline uint64_t pixel_chunk_bytes(long long m, int msMode, int quality, int nLights, bool coherent = false) {
    const uint64_t b = (uint64_t)m * pixel_entry_bytes(msMode, quality, nLights);
    return coherent ? b + pixel_table_bytes((uint64_t)m * (uint64_t)pixel_samples(msMode)) : b;
}

// Most entries of one chunk: at least 4 (an entry is never split, whatever the budget), and a multiple of 4, so that every chunk's part of a
// 16-byte aligned array of words, or of float triples, starts 16-byte aligned again.  (coherent: 8 ceil(m samples / 64) <= m samples / 8 + 8, so
// m entries fit where 64 (budget - head - 8) >= m (64 per + 8 samples); a few entries short of the most that fit, never over.)
inline long long pixel_chunk_entries(int msMode, int quality, int nLights, uint64_t budgetBytes, bool coherent = false) {
    const uint64_t per = pixel_entry_bytes(msMode, quality, nLights);
    uint64_t m = budgetBytes / per;
    if (coherent) {
        const uint64_t head = PIXEL_TABLE_HEAD_BYTES + PIXEL_TABLE_ENTRY_BYTES;
        const uint64_t room = budgetBytes > head ? budgetBytes - head : 0;
        const uint64_t per64 = 64u * per + PIXEL_TABLE_ENTRY_BYTES * (uint64_t)pixel_samples(msMode);   // bytes of 64 entries
        m = (room / per64) * 64u + ((room % per64) * 64u) / per64;   // floor(64 room / per64) without the product
    }
    const uint64_t byRays = (uint64_t)(PIXEL_CHUNK_MAX_RAYS / pixel_samples(msMode));
    if (m > byRays) m = byRays;
    m &= ~3ull;
    if (m < 4) m = 4;
    return (long long)m;
}

// Chunk boundaries b[0] = 0 < b[1] < .. < b[k] = n: chunk c is entries [b[c], b[c + 1]).  n <= 0: {0} (no chunk).  The chunks are equal but for
// the last, which is the shortest.
inline std::vector<long long> pixel_chunks(long long n, int msMode, int quality, int nLights, uint64_t budgetBytes, bool coherent = false) {
    std::vector<long long> b;
    b.push_back(0);
    if (n <= 0) return b;
    const long long m = pixel_chunk_entries(msMode, quality, nLights, budgetBytes, coherent);
    const uint64_t fit = budgetBytes / pixel_entry_bytes(msMode, quality, nLights);   // (a list that fits is one chunk, whatever its length modulo 4)
    if ((uint64_t)n <= fit && n * pixel_samples(msMode) <= PIXEL_CHUNK_MAX_RAYS && (!coherent || pixel_chunk_bytes(n, msMode, quality, nLights, true) <= budgetBytes)) { b.push_back(n); return b; }
    for (long long at = 0; at < n;) {
        at = (n - at <= m) ? n : at + m;
        b.push_back(at);
    }
    return b;
}

}  // namespace xrt
