// lights.h — launch interface of lights.hip: CastRay's light loop (RT:534-542) on a caller's hits (xrt.h xrt_light_hits).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/xrt.h"
#include "kernels.h"
#include "traverse.h"

namespace xrt {

// A block of k_light_emit takes LIGHT_EMIT_BLOCK consecutive entries per round, one per thread, and makes one reservation in the compact ray
// list for every LIGHT_EMIT_LIGHTS lights of them (16 waves x 4 lights: the 64 cells one wave scans); the tests place their list sizes
// around LIGHT_EMIT_BLOCK.
constexpr int LIGHT_EMIT_BLOCK = 1024;
constexpr int LIGHT_EMIT_LIGHTS = 4;
static_assert(LIGHT_EMIT_LIGHTS * (LIGHT_EMIT_BLOCK / 64) == 64, "one wave scans the block's cells");
constexpr int LIGHT_FOLD_BLOCK = 256;

// One chunk of n entries: entry e is hits[base + e] of the caller's list (16-byte aligned).  Pair (e, l) is entry e with light l; its number
// e * nLights + l addresses the chunk's flag words and shadow hits.
struct LightEmitArgs {
    const xrt_hit *hits = nullptr;
    long long base = 0;
    int n = 0, nLights = 0;
    const LightRec *lights = nullptr;
    int ae = 0;                 // answer a pair here when the one body's one mesh faces away from its ray (Settings::answerAtEmission)
    xrt_ray *rays = nullptr;    // [cap] the compact list of the shadow rays that have to be traced
    int *scatter = nullptr;     // [cap] the pair of ray i (IntersectArgs::scatter)
    int *flags = nullptr;       // [n * nLights] hit / miss word per pair (IntersectArgs::flags): a pair answered here gets 0
    int *count = nullptr;       // the rays listed (a zeroed word)
    int cap = 0;                // nothing is stored at or behind ray cap
};
void launch_light_emit(const SceneView &S, const LightEmitArgs &A, hipStream_t st);

// The fold over the same entries, behind the trace: flags / shadowHits hold the answer of every pair of a live entry.
struct LightFoldArgs {
    const xrt_hit *hits = nullptr;
    long long base = 0;
    int n = 0;
    const int *flags = nullptr;
    const xrt_hit *shadowHits = nullptr;
    float *lightOut = nullptr;    // the CALLER's arrays (entry base + e): 3 floats per entry, or null
    float *amountOut = nullptr;   // nLights floats per entry, or null
    int *liveCount = nullptr;     // the entries treated as hits (a zeroed word)
};
void launch_light_fold(const SceneView &S, const ShadeView &V, const LightFoldArgs &A, hipStream_t st);

}  // namespace xrt
