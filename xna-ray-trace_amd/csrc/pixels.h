// pixels.h — launch interface of pixels.hip: the kernels of xrt_render_pixels (xrt.h), caller-chosen screen positions instead of the pixel grid.
// A LIST here is n centres (cx[i * stride], cy[i * stride]): the caller's interleaved array (stride 2, cy = cx + 1) or a quadrant level's two
// arrays (stride 1).  Nothing in this file knows a frame: no tile, no cull rectangle, no pixel grid.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace xrt {

enum { PIXEL_ONE = 0, PIXEL_QUADRANT = 1, PIXEL_FIXED16 = 2 };   // rays per entry: 1, 4, 16

#ifdef __HIPCC__   // (device code; plain host code includes this header for the launch interface)
// Where sample s of an entry centred at (sx, sy) lies: the one statement of it for the ray generation kernels of a centre list (k_pixel_rays and
// k_pixel_raygen in pixels.hip, k_trace_raygen in trace.hip).  QUADRANT false: a call without a quadrant mode (xrt_trace_pixels) compiles no branch for it.
template <bool QUADRANT = true>
__device__ __forceinline__ void sample_position(int mode, float size, int s, float &sx, float &sy) {
    if (QUADRANT && mode == PIXEL_QUADRANT) {   // RT:223-276: four rays at centre -+ size/4, order UL, UR, LL, LR
        const float quarter = size * 0.25f;
        sx = (s & 1) ? sx + quarter : sx - quarter;
        sy = (s & 2) ? sy + quarter : sy - quarter;
    } else if (mode == PIXEL_FIXED16) {   // corner q = s/4 at +-0.25, sub-sample s%4 at +-0.125, in this association
        const int q = s >> 2, rr = s & 3;
        sx = (sx + ((q & 1) ? 0.25f : -0.25f)) + ((rr & 1) ? 0.125f : -0.125f);
        sy = (sy + ((q & 2) ? 0.25f : -0.25f)) + ((rr & 2) ? 0.125f : -0.125f);
    }
}
#endif

// k_pixel_rays: entries [first, first + count) of a list -> rays[0 .. count * samples), entry-major, as xrt_ray records with a null origin
// (RT:412-421 / RT:223-276 / the sixteen level-1 positions); `size` is the quadrant's (PIXEL_QUADRANT only).  g: camera part only.
void launch_pixel_rays(const RayGenParams &g, const float *cx, const float *cy, int stride, long long first, int count, float size, int mode,
                       xrt_ray *rays, hipStream_t st);

// k_pixel_raygen: k_pixel_rays and generation 0 of the pass that traces them (k_ingest, kernels.hip) in one kernel, for a list the caller calls coherent
// (xrt.h XRT_LIST_COHERENT).  It is k_raygen's structure on a centre list.  Place r = pathBase + p of the list's part -- entries from G.first on -- is sample
// r % samples of entry G.first + r / samples, at k_pixel_rays' position; path p of the pass (p < P) is place pathBase + p.  A ray that cannot reach the scene's
// root box (OSM:460) gets its miss record lvlB0[p] and is never stored; the live ones are compacted into rays[0 .. *count) with index[slot] = p (one
// reservation per block and group of 4096 places), the long ones listed (H), refOut[slot] = refIndex for a ray-tree pass (nullable).  Q.table non-null
// (launch #0 is a packet launch): one entry (first slot, live rays) per 64-aligned unit of the pass's places that has a live ray, reserved with the
// slots in the same atomic instruction; Q.count / Q.clear as k_raygen uses them (kernels.h QuadTable).  Bounds: liveCap slots, Q.cap entries.
struct PixelGenArgs {
    RayGenParams cam;   // camera part only
    const float *cx = nullptr, *cy = nullptr;
    int stride = 1;
    long long first = 0;
    float size = 1.0f;
    int mode = PIXEL_ONE;
};
void launch_pixel_raygen(const PixelGenArgs &G, const SceneView &S, xrt_ray *rays, f4 *lvlB0, int *index, int *count, int P, long long pathBase, const HeavyArgs &H,
                         int liveCap, float *refOut, float refIndex, const QuadTable &Q, hipStream_t st, hipEvent_t startEvent = nullptr);

// k_pixel_decide: RT:279-306 on a list of n quadrants with their four colours -- k_ms_decide for a level whose centres are listed with a
// stride, which is what level 0 of a centre list is.  Children of a quadrant are appended together, in corner order, to nextCx / nextCy (room
// for 4 n); *nextCount (zero before the launch) counts them.
void launch_pixel_decide(const uint32_t *quadColor, const float *cx, const float *cy, int stride, int n, float size, int *childBase, int *childMask,
                         float *nextCx, float *nextCy, int *nextCount, hipStream_t st);

// k_pixel_resolve: out[i] (and outF32[3i..], nullable: ToVector3() of out[i]) for i < n from samples sampleColor[i * samples ..], in list order,
// with the RT:309 arithmetic of k_resolve: the mean of a quadrant's four (PIXEL_QUADRANT) or the mean of four such means (PIXEL_FIXED16).
void launch_pixel_resolve(const uint32_t *sampleColor, int n, int mode, uint32_t *out, float *outF32, hipStream_t st);

}  // namespace xrt
