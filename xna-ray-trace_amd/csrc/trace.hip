// trace.hip — kernels of xrt_trace_pixels (xrt.h): the primary rays and closest hits of a caller's LIST of screen positions, nothing shaded (gfx950).
// An unhinted list needs nothing from this file: k_pixel_rays (pixels.hip) writes the rays and the per-lane kernel traces them, as xrt_scene_intersect does.
// A list the caller calls coherent (xrt.h XRT_LIST_COHERENT) is traced as generation 0 of a frame: k_trace_raygen makes the rays where it compacts them,
// answers the ones that cannot reach the scene's root box itself, and writes the packet table where the traversal launch is a packet launch.  It is
// k_pixel_raygen (pixels.hip) with the sinks of a closest-hit query instead of a pass's: no level record, no reference index, no long-ray list.
// sample_position is pixels.h's, the one k_pixel_raygen calls; the unproject / normalize statements are xrt_core.h's, called in pixels.hip's order: the
// equalities of tests/test_gpu_trace_pixels.py pin the two kernels' rays against each other, bit for bit.
// The arithmetic is xrt_core.h's, compiled with the same flags: contraction off, every addition below its own rounding.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "trace.h"
#include "xrt_core.h"

namespace xrt {

// What lane_result (traverse.h) leaves for a miss: hit 0; object, mesh, tri, leaf -1; u, v, d, wx, wy, wz 0.0f; no scheduling feedback.
__device__ __forceinline__ void store_miss(xrt_hit *dst) {
    Hit16 *p = reinterpret_cast<Hit16 *>(dst);
    p[0] = Hit16{0, -1, -1, -1};
    p[1] = Hit16{-1, 0, 0, 0};
    p[2] = Hit16{0, 0, 0, 0};
}

// A block takes groups of GEN_ROUNDS x 1024 consecutive places; a wave holds 64 consecutive, 64-aligned places of the chunk in every round -- the unit of
// the packet table: 4 entries of a 16-sample list, 64 one-sample entries.  The live rays are kept in registers until the block knows its range of the
// work list: one atomic per block and group, and where a table is written its entries are reserved by the lane next to the one that reserves the slots, in
// the same instruction.
constexpr int GEN_BLOCK = 1024, GEN_ROUNDS = 4;
static_assert(GEN_ROUNDS * (GEN_BLOCK / 64) == 64, "one wave scans the block's cells");
__global__ __launch_bounds__(GEN_BLOCK) void k_trace_raygen(PixelGenArgs G, SceneView S, xrt_ray *raysOut, xrt_hit *hitsOut, xrt_ray *work, int *index, int *count,
                                                            int P, int liveCap, QuadTable Q) {
    __shared__ int ldsLive[GEN_ROUNDS * 16];
    if (Q.table && blockIdx.x == 0 && threadIdx.x == 0) *Q.clear = 0u;   // (the count word of the chunk before the last, kernels.h QuadTable)
    const int shift = G.mode == PIXEL_FIXED16 ? 4 : 0;
    const f4 rlo = S.snodes[0], rhi = S.snodes[1];
    const int span = GEN_ROUNDS * GEN_BLOCK;
    const int groups = (P + span - 1) / span;
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    for (int grp = (int)blockIdx.x; grp < groups; grp += (int)gridDim.x) {
        int liveAt[GEN_ROUNDS];                    // rank among the live lanes of the wave, -1: not live
        v3 keepO[GEN_ROUNDS], keepD[GEN_ROUNDS];   // the live rays of this thread, written once their places in the list are known
#pragma unroll
        for (int r = 0; r < GEN_ROUNDS; r++) {
            const int p = grp * span + r * GEN_BLOCK + (int)threadIdx.x;
            bool live = false;
            keepO[r] = mk(0, 0, 0); keepD[r] = mk(0, 0, 0);
            if (p < P) {
                const size_t e = (size_t)(G.first + (long long)(p >> shift)) * (size_t)G.stride;
                const int s = p & ((1 << shift) - 1);
                float sx = G.cx[e], sy = G.cy[e];
                sample_position<false>(G.mode, G.size, s, sx, sy);   // (this call has no quadrant mode)
                const v3 nearP = unproject(G.cam, sx, sy, 0.0f);   // RT:415
                const v3 farP = unproject(G.cam, sx, sy, 1.0f);    // RT:419
                const v3 dir = normalize(sub(farP, nearP));        // RT:420-421
                const RayPre w = make_ray(nearP, dir);
                float key;
                live = slab(w, rlo.x, rlo.y, rlo.z, rhi.x, rhi.y, rhi.z, key);   // OSM:460 on the root
                keepO[r] = nearP; keepD[r] = dir;
                if (raysOut) store_ray(raysOut + p, nearP, dir, -1, -1);   // the caller's record, in list order: origin null (RT:424), no scheduling mark
                if (!live) store_miss(hitsOut + p);                        // the query ends here: "no intersection" (RT:512 on a ray OSM:460 rejects)
            }
            const unsigned long long ml = __ballot(live);
            liveAt[r] = live ? lanes_below(ml) : -1;
            if (lane == 0) ldsLive[r * 16 + wave] = (int)__popcll(ml);
        }
        __syncthreads();
        int quadLen = 0, quadAt = 0;   // wave 0 of a launch with a packet table: the live rays of this lane's cell and its entry
        // device_util.h's reserve_cells / reserve_cells_and_entries with the scan in front of the branch on Q.table: calling the two helpers moved the scan into both
        // arms and changed this kernel's code and registers, so the one site keeps its own form
        if (wave == 0) {
            const int c = ldsLive[lane];   // cell r * 16 + w: ascending place order
            const int incl = wave_scan_add(c);
            const int total = __builtin_amdgcn_readlane(incl, 63);
            if (Q.table) {
                quadLen = c;
                const unsigned long long mq = __ballot(quadLen > 0);
                int got = 0;   // lane 0 reserves the slots, lane 1 the entries (a word with a 256-byte line of its own): one atomic instruction
                if (lane < 2 && total) got = lane == 0 ? atomicAdd(count, total) : (int)atomicAdd(Q.count, (unsigned)__popcll(mq));
                quadAt = __builtin_amdgcn_readlane(got, 1) + lanes_below(mq);
                ldsLive[lane] = __builtin_amdgcn_readlane(got, 0) + incl - c;
            } else {
                int base = 0;
                if (lane == 0 && total) base = atomicAdd(count, total);
                base = __builtin_amdgcn_readfirstlane(base);
                ldsLive[lane] = base + incl - c;
            }
        }
        __syncthreads();
        // the block's entries, one coalesced store of wave 0 (Q.cap bounds the entries by construction, as liveCap the rays: the guards are against a wrong bound)
        if (quadLen > 0 && quadAt < Q.cap) Q.table[quadAt] = make_uint2((unsigned)ldsLive[lane], (unsigned)quadLen);
#pragma unroll
        for (int r = 0; r < GEN_ROUNDS; r++) {
            const int p = grp * span + r * GEN_BLOCK + (int)threadIdx.x;
            if (liveAt[r] >= 0) {
                const int slot = ldsLive[r * 16 + wave] + liveAt[r];
                if (slot < liveCap) {
                    index[slot] = p;
                    store_ray(work + slot, keepO[r], keepD[r], -1, -1);
                }
            }
        }
        __syncthreads();   // the cells are reused by the next group
    }
}
void launch_trace_raygen(const PixelGenArgs &G, const SceneView &S, xrt_ray *raysOut, xrt_hit *hitsOut, xrt_ray *work, int *index, int *count, int P, int liveCap,
                         const QuadTable &Q, hipStream_t st) {
    int blocks = (int)(((long long)P + GEN_ROUNDS * GEN_BLOCK - 1) / (GEN_ROUNDS * GEN_BLOCK));
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_trace_raygen, dim3(blocks), dim3(GEN_BLOCK), 0, st, G, S, raysOut, hitsOut, work, index, count, P, liveCap, Q);
}

// The hits among n records: one word of every 48-byte record, a count per wave, one atomic per wave that found any.
constexpr int HITS_BLOCK = 256;
__global__ __launch_bounds__(HITS_BLOCK) void k_trace_hits(const xrt_hit *hits, int n, int *count) {
    int mine = 0;
    for (long long i = (long long)blockIdx.x * HITS_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * HITS_BLOCK) mine += hits[i].hit != 0 ? 1 : 0;
    const int total = __builtin_amdgcn_readlane(wave_scan_add(mine), 63);
    if (lane_id() == 0 && total) atomicAdd(count, total);
}
void launch_trace_hits(const xrt_hit *hits, int n, int *count, hipStream_t st) {
    int blocks = (n + HITS_BLOCK - 1) / HITS_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_trace_hits, dim3(blocks < 1 ? 1 : blocks), dim3(HITS_BLOCK), 0, st, hits, n, count);
}

}  // namespace xrt
