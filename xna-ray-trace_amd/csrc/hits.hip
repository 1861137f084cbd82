// hits.hip — generation 0 of a pass from caller-given hits (xrt.h xrt_shade_hits; gfx950, wave64).
// RayTracer.CastRay is a closest-hit query (RT:512) and everything that follows from its IntersectionResult (RT:514-737).  A pass normally
// makes generation 0 with k_ingest (the caller's rays, compacted) and closest-hit launch #0 (their hits); k_ingest_hits makes both from the
// caller's lists, so that part A of k_shade #0 runs on slots it cannot tell from traced ones and launch #0 never happens.  Nothing here
// computes a float: the words of a hit go through as bits.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "hits.h"
#include "shade_math.h"
#include "xrt_core.h"

namespace xrt {

// Path p of the chunk is (rays[pathBase + p], hits[pathBase + p]).  "The query returned hits[p]": hit == 0 is a miss and the path ends as k_ingest
// ends a ray that cannot reach the root box (RT:729-733); so does an entry whose mesh or triangle the scene does not have (shade_math.h
// hit_names_scene) -- it is shaded as a miss and can address nothing.  The others are compacted into the live list with one ballot per round,
// one wave scan of the block's 64 cells and one atomic per block and group (device_util.h reserve_cells), and get what the skipped launch
// would have left at their slot: the ray (CastRay reads its
// direction, RT:549; the origin triangle only entered the query, so the record names none and carries no long-ray mark -- nothing is traced),
// the 48-byte hit with hit = 1 and a zero feedback word, the hit word, the path, and for a ray tree the caller's currentRefIndex (RT:658).
// Two phases, so that a thread keeps 16 bytes per round across the barriers and a miss costs 16 bytes of reads: the first loads the
// (hit, object, mesh, tri) quarter of every record and decides, the second loads the other 64 bytes of the live ones and stores.
__global__ __launch_bounds__(INGEST_HITS_BLOCK) void k_ingest_hits(SceneView S, IngestHitsArgs A) {
    __shared__ int ldsLive[INGEST_HITS_ROUNDS * 16];
    const int span = INGEST_HITS_SPAN;
    const int groups = (A.P + span - 1) / span;
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    for (int grp = (int)blockIdx.x; grp < groups; grp += (int)gridDim.x) {
        int liveAt[INGEST_HITS_ROUNDS];   // rank among the live lanes of the wave, -1: not live
        W4 head[INGEST_HITS_ROUNDS];
#pragma unroll
        for (int r = 0; r < INGEST_HITS_ROUNDS; r++) {
            const int p = grp * span + r * INGEST_HITS_BLOCK + (int)threadIdx.x;
            bool live = false;
            head[r] = W4{0, -1, -1, -1};
            if (p < A.P) {
                const W4 a = reinterpret_cast<const W4 *>(A.hits + (A.pathBase + p))[0];   // hit object mesh tri
                live = hit_names_scene(S.meshes, S.nMeshes, a);
                head[r] = a;
                if (!live) A.lvlB0[p] = f4{0, 0, 0, i2f(FLAG_MISS)};   // generation 0 ends here (RT:729-733)
            }
            const unsigned long long ml = __ballot(live);
            liveAt[r] = live ? lanes_below(ml) : -1;
            if (lane == 0) ldsLive[r * 16 + wave] = (int)__popcll(ml);
        }
        __syncthreads();
        if (wave == 0) reserve_cells(ldsLive, A.count);   // the block's range of the live list (cell r * 16 + w: ascending path order)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < INGEST_HITS_ROUNDS; r++) {
            const int p = grp * span + r * INGEST_HITS_BLOCK + (int)threadIdx.x;
            if (liveAt[r] >= 0) {
                const int slot = ldsLive[r * 16 + wave] + liveAt[r];
                if (slot < A.liveCap) {   // (live paths <= P <= liveCap: the guard is against a wrong bound, not a code path)
                    const W4 *ray = reinterpret_cast<const W4 *>(A.rays + (A.pathBase + p));
                    const W4 *hit = reinterpret_cast<const W4 *>(A.hits + (A.pathBase + p));
                    const W4 ra = ray[0], rb = ray[1];   // o.xyz d.x | d.yz ignore_mesh ignore_tri
                    const W4 hb = hit[1], hc = hit[2];   // leaf u v d | w.xyz reserved
                    A.index[slot] = p;
                    W4 *rdst = reinterpret_cast<W4 *>(A.raysOut + slot);
                    rdst[0] = ra; rdst[1] = W4{rb.x, rb.y, -1, -1};
                    W4 *hdst = reinterpret_cast<W4 *>(A.hitsOut + slot);
                    hdst[0] = W4{1, head[r].y, head[r].z, head[r].w};
                    hdst[1] = hb;
                    hdst[2] = W4{hc.x, hc.y, hc.z, 0};
                    if (A.flagsOut) A.flagsOut[slot] = 1;
                    if (A.refOut) A.refOut[slot] = A.refIndex;
                }
            }
        }
        __syncthreads();   // the cells are reused by the next group
    }
}

void launch_ingest_hits(const SceneView &S, const IngestHitsArgs &A, hipStream_t st, hipEvent_t startEvent) {
    int blocks = (int)(((long long)A.P + INGEST_HITS_SPAN - 1) / INGEST_HITS_SPAN);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipExtLaunchKernelGGL(k_ingest_hits, dim3(blocks), dim3(INGEST_HITS_BLOCK), 0, st, startEvent, nullptr, 0, S, A);
}

}  // namespace xrt
