// hits.h — launch interface of hits.hip: generation 0 of a pass from a caller's rays AND their closest hits (xrt.h xrt_shade_hits).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/xrt.h"
#include "traverse.h"

namespace xrt {

// A block takes INGEST_HITS_ROUNDS x INGEST_HITS_BLOCK consecutive paths per group and makes one reservation in the live list for all of
// them (the shape of k_ingest, kernels.hip): the tests place their list sizes around INGEST_HITS_SPAN.
constexpr int INGEST_HITS_ROUNDS = 4, INGEST_HITS_BLOCK = 1024;
constexpr int INGEST_HITS_SPAN = 4096;
static_assert(INGEST_HITS_SPAN == INGEST_HITS_ROUNDS * INGEST_HITS_BLOCK && INGEST_HITS_ROUNDS * (INGEST_HITS_BLOCK / 64) == 64, "one wave scans the block's cells");

// One chunk of P paths: path p is (rays[pathBase + p], hits[pathBase + p]) of the caller's lists (each 16-byte aligned).  Everything below
// `raysOut` is the frame context's: what closest-hit launch #0 and k_ingest would have left for part A of k_shade #0 (kernels.h ShadeArgs).
struct IngestHitsArgs {
    const xrt_ray *rays = nullptr;
    const xrt_hit *hits = nullptr;
    long long pathBase = 0;
    int P = 0;
    xrt_ray *raysOut = nullptr;   // [liveCap] the ray of live slot j (ShadeArgs::rays)
    xrt_hit *hitsOut = nullptr;   // [liveCap] its hit (ShadeArgs::hits)
    int *flagsOut = nullptr;      // [liveCap] its hit / miss word (ShadeArgs::hitFlags), or null
    int *index = nullptr;         // [liveCap] its path (ShadeArgs::rayPath)
    int *count = nullptr;         // the live slots taken (a zeroed word of the chunk's counter block)
    f4 *lvlB0 = nullptr;          // [P] generation 0's level records: a path that is not live ends here
    float *refOut = nullptr;      // [liveCap] ray-tree passes: the medium the ray travels in (ShadeArgs::rayRef), or null
    float refIndex = 1.0f;
    int liveCap = 0;              // nothing is stored at or behind slot liveCap
};
void launch_ingest_hits(const SceneView &S, const IngestHitsArgs &A, hipStream_t st, hipEvent_t startEvent = nullptr);

}  // namespace xrt
