// compose.h — launch interface of compose.hip: the return path of CastRay's recursion, one level, on a caller's terms (xrt.h xrt_compose_hits).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/xrt.h"

namespace xrt {

// k_compose_hits takes one entry per thread; a launch has at most COMPOSE_MAX_BLOCKS blocks and walks a longer piece in a grid-stride loop.  The
// tests place their list sizes around COMPOSE_BLOCK and one entry past COMPOSE_MAX_BLOCKS * COMPOSE_BLOCK.
constexpr int COMPOSE_BLOCK = 256;
constexpr int COMPOSE_MAX_BLOCKS = 2048;
// A launch indexes its entries with an int: a longer list is launched in pieces of at most this many entries, each with its base offset.
constexpr long long COMPOSE_PIECE = 1LL << 30;

// One piece of n entries: entry e is record base + e of every array (the records 16-byte aligned, the arrays of floats and colours at their
// natural alignment).  rgbaOut may be reflect or refract itself: a thread reads its entry of both before it writes it.
struct ComposeArgs {
    const xrt_surface *surface = nullptr;   // color, reflectiveness, alpha and two bits of flags are read
    const float *light = nullptr;           // 3 floats per entry: the light sum of RT:534-542
    const uint32_t *reflect = nullptr;      // what the nested CastRay of RT:556-559 returned, or null: RT:726 for every hit
    const uint32_t *refract = nullptr;      // what the nested CastRay of RT:698 returned, or null: RT:586 is skipped for every hit
    size_t base = 0;
    int n = 0;
    // "is this array given": kernel arguments, so every branch on them is wave-uniform
    int haveReflect = 0, haveRefract = 0, wantRgba = 0, wantF32 = 0;
    uint32_t *rgbaOut = nullptr;            // the CALLER's arrays, or null
    float *f32Out = nullptr;
    unsigned long long *hitCount = nullptr;   // the entries with XRT_SURF_HIT (a zeroed word)
};
void launch_compose_hits(const ComposeArgs &A, hipStream_t st);

}  // namespace xrt
