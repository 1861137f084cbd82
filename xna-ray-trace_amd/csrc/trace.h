// trace.h — launch interface of trace.hip: the kernels of xrt_trace_pixels (xrt.h), the primary rays and closest hits of caller-chosen screen positions.
// A list is what pixels.h calls one (PixelGenArgs: the caller's interleaved centres, stride 2); place r of a chunk is sample r % samples of entry
// G.first + r / samples, at k_pixel_rays' position.  Nothing is shaded here and nothing of a frame's pass is used: no level records, no path list.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pixels.h"

namespace xrt {

// k_trace_raygen: the rays of a coherent list (xrt.h XRT_LIST_COHERENT) made where they are compacted -- k_pixel_raygen's structure (pixels.hip) with the sinks
// of a closest-hit query.  For every place p < P: the clean ray (ignore_mesh = ignore_tri = -1) goes to raysOut[p] (nullable: not wanted); a ray that cannot
// reach the scene's root box (OSM:460) gets the miss record lane_result leaves (traverse.h) in hitsOut[p] and is never stored in the work list; the live ones
// are compacted into work[0 .. *count) with index[slot] = p, which the traversal launch takes as its scatter list (IntersectArgs / PacketArgs::scatter).
// One reservation per block and group of 4096 places.  Q.table non-null (the launch that follows is a packet launch): one entry (first slot, live rays) per
// 64-aligned unit of the chunk's places that has a live ray, reserved with the slots in the same atomic instruction; Q.count / Q.clear as k_raygen uses
// them (kernels.h QuadTable).  Bounds: P places of raysOut / hitsOut, liveCap slots of work / index, Q.cap entries.
void launch_trace_raygen(const PixelGenArgs &G, const SceneView &S, xrt_ray *raysOut, xrt_hit *hitsOut, xrt_ray *work, int *index, int *count, int P, int liveCap,
                         const QuadTable &Q, hipStream_t st);

// k_trace_hits: *count += the records of hits[0 .. n) whose `hit` word is not zero (xrt_stats.hits_closest of the call).
void launch_trace_hits(const xrt_hit *hits, int n, int *count, hipStream_t st);

}  // namespace xrt
