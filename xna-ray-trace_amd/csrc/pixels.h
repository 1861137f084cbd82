// pixels.h — launch interface of pixels.hip: the kernels of xrt_render_pixels (xrt.h), caller-chosen screen positions instead of the pixel grid.
// A LIST here is n centres (cx[i * stride], cy[i * stride]): the caller's interleaved array (stride 2, cy = cx + 1) or a quadrant level's two
// arrays (stride 1).  Nothing in this file knows a frame: no tile, no cull rectangle, no pixel grid.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace xrt {

enum { PIXEL_ONE = 0, PIXEL_QUADRANT = 1, PIXEL_FIXED16 = 2 };   // rays per entry: 1, 4, 16

// k_pixel_rays: entries [first, first + count) of a list -> rays[0 .. count * samples), entry-major, as xrt_ray records with a null origin
// (RT:412-421 / RT:223-276 / the sixteen level-1 positions); `size` is the quadrant's (PIXEL_QUADRANT only).  g: camera part only.
void launch_pixel_rays(const RayGenParams &g, const float *cx, const float *cy, int stride, long long first, int count, float size, int mode,
                       xrt_ray *rays, hipStream_t st);

// k_pixel_decide: RT:279-306 on a list of n quadrants with their four colours -- k_ms_decide for a level whose centres are listed with a
// stride, which is what level 0 of a centre list is.  Children of a quadrant are appended together, in corner order, to nextCx / nextCy (room
// for 4 n); *nextCount (zero before the launch) counts them.
void launch_pixel_decide(const uint32_t *quadColor, const float *cx, const float *cy, int stride, int n, float size, int *childBase, int *childMask,
                         float *nextCx, float *nextCy, int *nextCount, hipStream_t st);

// k_pixel_resolve: out[i] (and outF32[3i..], nullable: ToVector3() of out[i]) for i < n from samples sampleColor[i * samples ..], in list order,
// with the RT:309 arithmetic of k_resolve: the mean of a quadrant's four (PIXEL_QUADRANT) or the mean of four such means (PIXEL_FIXED16).
void launch_pixel_resolve(const uint32_t *sampleColor, int n, int mode, uint32_t *out, float *outF32, hipStream_t st);

}  // namespace xrt
