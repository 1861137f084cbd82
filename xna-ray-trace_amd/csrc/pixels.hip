// pixels.hip — kernels of xrt_render_pixels (xrt.h): rays, quadrant decisions and the resolve for a caller's LIST of screen positions (gfx950).
// The frame kernels of kernels.hip (k_raygen, k_ms_decide, k_resolve) walk a pixel grid in tiles; these walk a list in the caller's order and
// know nothing of a frame.  The arithmetic is the same functions (xrt_core.h: unproject, normalize, unpack_color / pack_color, divf, length),
// compiled with the same flags: contraction off, every addition below its own rounding.
// An unhinted list is NOT fused -- k_pixel_rays writes 32-byte xrt_ray records and the pass of xrt_cast_rays (k_ingest, iteration 0, currentRefIndex 1.0f)
// reads them back, one round trip through HBM per ray (profiles/pixels/README.md).  A list the caller calls coherent (xrt.h XRT_LIST_COHERENT) is:
// k_pixel_raygen makes the rays where the pass compacts them (profiles/coherent_lists/README.md).
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "pixels.h"
#include "shade_math.h"
#include "xrt_core.h"

#include <hip/hip_ext.h>

namespace xrt {

constexpr int PIXEL_BLOCK = 256;
// Four packed colours -- a quadrant's, or a corner's four sub-samples -- in one 16-byte load: every array of them in this file starts 16-byte
// aligned (device allocations) and holds whole groups of four.
struct alignas(16) Color4 { uint32_t c[4]; };
__device__ __forceinline__ Color4 load4(const uint32_t *p) { return *reinterpret_cast<const Color4 *>(p); }

// (sample_position, where sample s of an entry lies: pixels.h -- trace.hip generates the same rays)

// One thread per ray: ray r of the launch is sample r % samples of entry first + r / samples, so a wave writes 2 KB of consecutive records.
__global__ __launch_bounds__(PIXEL_BLOCK) void k_pixel_rays(RayGenParams g, const float *cx, const float *cy, int stride, long long first, int count,
                                                            float size, int mode, xrt_ray *rays) {
    const int shift = mode == PIXEL_FIXED16 ? 4 : (mode == PIXEL_QUADRANT ? 2 : 0);
    const long long total = (long long)count << shift;
    for (long long r = (long long)blockIdx.x * PIXEL_BLOCK + threadIdx.x; r < total; r += (long long)gridDim.x * PIXEL_BLOCK) {
        const size_t e = (size_t)(first + (r >> shift)) * (size_t)stride;
        const int s = (int)(r & ((1 << shift) - 1));
        float sx = cx[e], sy = cy[e];
        sample_position(mode, size, s, sx, sy);
        const v3 nearP = unproject(g, sx, sy, 0.0f);   // RT:415
        const v3 farP = unproject(g, sx, sy, 1.0f);    // RT:419
        const v3 dir = normalize(sub(farP, nearP));    // RT:420-421
        store_ray(rays + r, nearP, dir, -1, -1);       // origin null (RT:424)
    }
}
void launch_pixel_rays(const RayGenParams &g, const float *cx, const float *cy, int stride, long long first, int count, float size, int mode,
                       xrt_ray *rays, hipStream_t st) {
    const long long total = (long long)count * (mode == PIXEL_FIXED16 ? 16 : (mode == PIXEL_QUADRANT ? 4 : 1));
    long long blocks = (total + PIXEL_BLOCK - 1) / PIXEL_BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_pixel_rays, dim3(blocks < 1 ? 1 : (unsigned)blocks), dim3(PIXEL_BLOCK), 0, st, g, cx, cy, stride, first, count, size, mode, rays);
}

// k_pixel_rays and k_ingest in one (pixels.h): k_raygen's structure (kernels.hip) on a centre list.  A block takes groups of GEN_ROUNDS x 1024 consecutive
// places; a wave holds 64 consecutive, 64-aligned places of the pass in every round -- the unit of the packet table: 4 entries of a 16-sample list, 16
// level-0 quadrants, 64 one-sample entries.  The rays are kept in registers until the block knows its range of the live list: one atomic per list, block
// and group, and where a table is written its entries are reserved by the lane next to the one that reserves the slots, in the same instruction.
constexpr int GEN_BLOCK = 1024, GEN_ROUNDS = 4;
static_assert(GEN_ROUNDS * (GEN_BLOCK / 64) == 64, "one wave scans the block's cells");
__global__ __launch_bounds__(GEN_BLOCK) void k_pixel_raygen(PixelGenArgs G, SceneView S, xrt_ray *rays, f4 *lvlB0, int *index, int *count, int P, long long pathBase,
                                                            HeavyArgs H, int liveCap, float *refOut, float refIndex, QuadTable Q) {
    __shared__ int ldsLive[GEN_ROUNDS * 16], ldsHeavy[GEN_ROUNDS * 16];
    if (Q.table && blockIdx.x == 0 && threadIdx.x == 0) *Q.clear = 0u;   // (the count word of the chunk before the last, kernels.h QuadTable)
    const int shift = G.mode == PIXEL_FIXED16 ? 4 : (G.mode == PIXEL_QUADRANT ? 2 : 0);
    const f4 rlo = S.snodes[0], rhi = S.snodes[1];
    const int span = GEN_ROUNDS * GEN_BLOCK;
    const int groups = (P + span - 1) / span;
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    for (int grp = (int)blockIdx.x; grp < groups; grp += (int)gridDim.x) {
        int liveAt[GEN_ROUNDS], heavyAt[GEN_ROUNDS];   // rank among the flagged lanes of the wave, -1: not flagged
        v3 keepO[GEN_ROUNDS], keepD[GEN_ROUNDS];       // the live rays of this thread, written once their places in the list are known
#pragma unroll
        for (int r = 0; r < GEN_ROUNDS; r++) {
            const int p = grp * span + r * GEN_BLOCK + (int)threadIdx.x;
            bool live = false, heavy = false;
            keepO[r] = mk(0, 0, 0); keepD[r] = mk(0, 0, 0);
            if (p < P) {
                const long long place = pathBase + p;
                const size_t e = (size_t)(G.first + (place >> shift)) * (size_t)G.stride;
                const int s = (int)(place & ((1 << shift) - 1));
                float sx = G.cx[e], sy = G.cy[e];
                sample_position(G.mode, G.size, s, sx, sy);
                const v3 nearP = unproject(G.cam, sx, sy, 0.0f);   // RT:415
                const v3 farP = unproject(G.cam, sx, sy, 1.0f);    // RT:419
                const v3 dir = normalize(sub(farP, nearP));        // RT:420-421
                const RayPre w = make_ray(nearP, dir);
                float key;
                live = slab(w, rlo.x, rlo.y, rlo.z, rhi.x, rhi.y, rhi.z, key);   // OSM:460 on the root
                heavy = live && H.list && long_ray(S, H, p, nearP, dir);
                keepO[r] = nearP; keepD[r] = dir;
                if (!live) lvlB0[p] = f4{0, 0, 0, i2f(FLAG_MISS)};   // generation 0 ends here (RT:729-733): the record k_ingest writes, and no ray
            }
            const unsigned long long ml = __ballot(live), mh = __ballot(heavy);
            liveAt[r] = live ? lanes_below(ml) : -1;
            heavyAt[r] = heavy ? lanes_below(mh) : -1;
            if (lane == 0) { ldsLive[r * 16 + wave] = (int)__popcll(ml); ldsHeavy[r * 16 + wave] = (int)__popcll(mh); }
        }
        __syncthreads();
        int quadLen = 0, quadAt = 0;   // wave 0 of a launch with a packet table: the live rays of this lane's cell and its entry
        // (cell r * 16 + w: ascending place order)
        if (wave == 0 && Q.table) reserve_cells_and_entries(ldsLive, count, Q.count, quadLen, quadAt);   // the live list and the packet table's entries, one atomic instruction
        else if (wave < 2 && (wave == 0 || H.list)) reserve_cells(wave == 0 ? ldsLive : ldsHeavy, wave == 0 ? count : H.count);   // wave 0: the live list, wave 1: the long-ray list
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
                    store_ray(rays + slot, keepO[r], keepD[r], -1, heavyAt[r] >= 0 ? (-1 ^ HEAVY_BIT) : -1);   // origin null (RT:424)
                    if (refOut) refOut[slot] = refIndex;
                    if (heavyAt[r] >= 0) H.list[ldsHeavy[r * 16 + wave] + heavyAt[r]] = slot;
                }
            }
        }
        __syncthreads();   // the cells are reused by the next group
    }
}
void launch_pixel_raygen(const PixelGenArgs &G, const SceneView &S, xrt_ray *rays, f4 *lvlB0, int *index, int *count, int P, long long pathBase, const HeavyArgs &H,
                         int liveCap, float *refOut, float refIndex, const QuadTable &Q, hipStream_t st, hipEvent_t startEvent) {
    int blocks = (int)(((long long)P + GEN_ROUNDS * GEN_BLOCK - 1) / (GEN_ROUNDS * GEN_BLOCK));
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipExtLaunchKernelGGL(k_pixel_raygen, dim3(blocks), dim3(GEN_BLOCK), 0, st, startEvent, nullptr, 0, G, S, rays, lvlB0, index, count, P, pathBase, H, liveCap, refOut, refIndex, Q);
}

// RT:279-306 on listed quadrants.  A corner whose colour-vector length differs from the length of the 4-mean by more than 0.5 (RT:340) is
// subdivided: its child (centre = the corner's sample position, half the size) goes to the next level.  The children of a quadrant must be
// contiguous and in corner order (the fold finds them by base + rank), so a block reserves room by the COUNT of its children: a scan over
// each wave, one over the block's waves, one atomic per block and round.
__global__ __launch_bounds__(PIXEL_BLOCK) void k_pixel_decide(const uint32_t *quadColor, const float *cx, const float *cy, int stride, int n, float size,
                                                              int *childBase, int *childMask, float *nextCx, float *nextCy, int *nextCount) {
    __shared__ int ldsCounts[PIXEL_BLOCK / 64 + 1];
    const int step = (int)(gridDim.x * PIXEL_BLOCK);
    const int rounds = (n + step - 1) / step;   // (every thread of a block takes every round: the barriers below are block-uniform)
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    for (int it = 0; it < rounds; it++) {
        const int q = it * step + (int)(blockIdx.x * PIXEL_BLOCK + threadIdx.x);
        int mask = 0;
        if (q < n) {
            const Color4 k = load4(quadColor + 4 * (size_t)q);
            const v3 c0 = unpack_color(k.c[0]), c1 = unpack_color(k.c[1]), c2 = unpack_color(k.c[2]), c3 = unpack_color(k.c[3]);
            const v3 average = divf(add(add(add(c0, c1), c2), c3), 4.0f);   // RT:285
            const float al = length(average);                               // RT:286
            const float TRESHOLD = 0.5f;                                    // RT:340
            if (fabsf(al - length(c0)) > TRESHOLD) mask |= 1;               // RT:288
            if (fabsf(al - length(c1)) > TRESHOLD) mask |= 2;               // RT:293
            if (fabsf(al - length(c2)) > TRESHOLD) mask |= 4;               // RT:298
            if (fabsf(al - length(c3)) > TRESHOLD) mask |= 8;               // RT:303
        }
        const int cnt = __builtin_popcount((unsigned)mask);
        int incl = cnt;
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
        if (lane == 63) ldsCounts[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            int total = 0;
            for (int w = 0; w < PIXEL_BLOCK / 64; w++) { const int c = ldsCounts[w]; ldsCounts[w] = total; total += c; }
            ldsCounts[PIXEL_BLOCK / 64] = total ? atomicAdd(nextCount, total) : 0;
        }
        __syncthreads();
        const int base = ldsCounts[PIXEL_BLOCK / 64] + ldsCounts[wave] + (incl - cnt);
        __syncthreads();   // the cells are reused by the next round
        if (q < n) {
            childBase[q] = base;
            childMask[q] = mask;
            const float x = cx[(size_t)q * (size_t)stride], y = cy[(size_t)q * (size_t)stride];
            const float quarter = size * 0.25f;
            int o = base;   // (base + cnt <= 4 n: the next level has room for four children of every quadrant)
            for (int j = 0; j < 4; j++)
                if (mask & (1 << j)) {
                    nextCx[o] = (j & 1) ? x + quarter : x - quarter;   // RT:290-305: the corner's sample position
                    nextCy[o] = (j & 2) ? y + quarter : y - quarter;
                    o++;
                }
        }
    }
}
void launch_pixel_decide(const uint32_t *quadColor, const float *cx, const float *cy, int stride, int n, float size, int *childBase, int *childMask,
                         float *nextCx, float *nextCy, int *nextCount, hipStream_t st) {
    int blocks = (n + PIXEL_BLOCK - 1) / PIXEL_BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_pixel_decide, dim3(blocks < 1 ? 1 : blocks), dim3(PIXEL_BLOCK), 0, st, quadColor, cx, cy, stride, n, size, childBase, childMask,
                       nextCx, nextCy, nextCount);
}

// (RT:309, the mean of four quantised colours, re-quantised: mean4, shade_math.h)
__global__ __launch_bounds__(PIXEL_BLOCK) void k_pixel_resolve(const uint32_t *sampleColor, int n, int mode, uint32_t *out, float *outF32) {
    for (int i = (int)(blockIdx.x * PIXEL_BLOCK + threadIdx.x); i < n; i += (int)(gridDim.x * PIXEL_BLOCK)) {
        uint32_t col;
        if (mode == PIXEL_QUADRANT) {   // the entry's level-0 quadrant after all folds
            const Color4 s = load4(sampleColor + (size_t)i * 4);
            col = mean4(s.c);
        } else {                        // PIXEL_FIXED16: four means of four
            Color4 corner;
            for (int q = 0; q < 4; q++) { const Color4 s = load4(sampleColor + (size_t)i * 16 + q * 4); corner.c[q] = mean4(s.c); }
            col = mean4(corner.c);
        }
        out[i] = col;
        if (outF32) { const v3 cv = unpack_color(col); outF32[3 * (size_t)i] = cv.x; outF32[3 * (size_t)i + 1] = cv.y; outF32[3 * (size_t)i + 2] = cv.z; }
    }
}
void launch_pixel_resolve(const uint32_t *sampleColor, int n, int mode, uint32_t *out, float *outF32, hipStream_t st) {
    int blocks = (n + PIXEL_BLOCK - 1) / PIXEL_BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_pixel_resolve, dim3(blocks < 1 ? 1 : blocks), dim3(PIXEL_BLOCK), 0, st, sampleColor, n, mode, out, outF32);
}

}  // namespace xrt
