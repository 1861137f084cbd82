// trace_plan.h — how xrt_trace_pixels splits a centre list into chunks: pure host arithmetic beside pixels_plan.h.  It includes nothing of HIP and
// touches no scene, so a program without a GPU covers it (tests/trace/host_trace.cpp).
//
// The outputs are the caller's and cost nothing here.  A chunk of m entries holds, in this seam's own work buffers, per place -- place r is sample
// r % samples of entry r / samples -- a work ray (32 bytes: the compact list of a hinted chunk, the whole list where the caller wants no rays) and a
// word of the index list (4 bytes), and a hinted chunk (xrt.h XRT_LIST_COHERENT) the packet table of pixels_plan.h: two count lines, 512 bytes, and one
// 8-byte entry per 64 places, the last unit may be partial.  The accounting includes the table for every hinted chunk, whichever kernel the scene's rule
// picks, and the index word for every chunk.  The sum stays within the byte budget (XRT_PIXEL_BYTES), and a chunk has at most PIXEL_CHUNK_MAX_RAYS
// places.  An entry is never split and a chunk is a multiple of 4 entries (but for the last), so every chunk's part of the caller's 16-byte aligned
// arrays starts 16-byte aligned and a 16-sample chunk starts on a 64-place unit.  Nothing about the answers depends on the split.
//   samples: 1 (XRT_MS_OFF), 16 (XRT_MS_FIXED16).
#pragma once
#include <cstdint>
#include <vector>

#include "pixels_plan.h"

namespace xrt {

constexpr uint64_t TRACE_PLACE_BYTES = 32u + 4u;

inline uint64_t trace_entry_bytes(int samples) { return (uint64_t)samples * TRACE_PLACE_BYTES; }

// Bytes a chunk of m entries accounts for.
inline uint64_t trace_chunk_bytes(long long m, int samples, bool coherent) {
    const uint64_t b = (uint64_t)m * trace_entry_bytes(samples);
    return coherent ? b + pixel_table_bytes((uint64_t)m * (uint64_t)samples) : b;
}

// Most entries of one chunk: at least 4 (an entry is never split, whatever the budget), and a multiple of 4.  (coherent: as pixel_chunk_entries --
// 8 ceil(m samples / 64) <= m samples / 8 + 8, so m entries fit where 64 (budget - head - 8) >= m (64 per + 8 samples); a few entries short of the most
// that fit, never over.)
inline long long trace_chunk_entries(int samples, uint64_t budgetBytes, bool coherent) {
    const uint64_t per = trace_entry_bytes(samples);
    uint64_t m = budgetBytes / per;
    if (coherent) {
        const uint64_t head = PIXEL_TABLE_HEAD_BYTES + PIXEL_TABLE_ENTRY_BYTES;
        const uint64_t room = budgetBytes > head ? budgetBytes - head : 0;
        const uint64_t per64 = 64u * per + PIXEL_TABLE_ENTRY_BYTES * (uint64_t)samples;   // bytes of 64 entries
        m = (room / per64) * 64u + ((room % per64) * 64u) / per64;   // floor(64 room / per64) without the product
    }
    const uint64_t byRays = (uint64_t)(PIXEL_CHUNK_MAX_RAYS / samples);
    if (m > byRays) m = byRays;
    m &= ~3ull;
    if (m < 4) m = 4;
    return (long long)m;
}

// Chunk boundaries b[0] = 0 < b[1] < .. < b[k] = n: chunk c is entries [b[c], b[c + 1]).  n <= 0: {0} (no chunk).  The chunks are equal but for the
// last, which is the shortest; a list that fits is one chunk, whatever its length modulo 4.
inline std::vector<long long> trace_chunks(long long n, int samples, uint64_t budgetBytes, bool coherent) {
    std::vector<long long> b;
    b.push_back(0);
    if (n <= 0) return b;
    const long long m = trace_chunk_entries(samples, budgetBytes, coherent);
    const uint64_t fit = budgetBytes / trace_entry_bytes(samples);
    if ((uint64_t)n <= fit && (uint64_t)n <= (uint64_t)(PIXEL_CHUNK_MAX_RAYS / samples) && (!coherent || trace_chunk_bytes(n, samples, true) <= budgetBytes)) { b.push_back(n); return b; }
    for (long long at = 0; at < n;) {
        at = (n - at <= m) ? n : at + m;
        b.push_back(at);
    }
    return b;
}

}  // namespace xrt
