// surface.h — launch interface of surface.hip: what CastRay computes at a hit without asking the scene anything (xrt.h xrt_surface_hits).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/xrt.h"
#include "kernels.h"

namespace xrt {

// k_surface takes one entry per thread; a launch has at most SURFACE_MAX_BLOCKS blocks and walks a longer piece in a grid-stride loop.  The
// tests place their list sizes around SURFACE_BLOCK and one entry past SURFACE_MAX_BLOCKS * SURFACE_BLOCK.
constexpr int SURFACE_BLOCK = 256;
constexpr int SURFACE_MAX_BLOCKS = 2048;
// A launch indexes its entries with an int: a longer list is launched in pieces of at most this many entries, each with its base offset.
constexpr long long SURFACE_PIECE = 1LL << 30;

// One piece of n entries: entry e is hits[base + e], rays[base + e] and record base + e of every output (all 16-byte aligned).
struct SurfaceArgs {
    const xrt_hit *hits = nullptr;
    const xrt_ray *rays = nullptr;        // read only where a ray output is asked (the direction alone is used)
    size_t base = 0;
    int n = 0;
    int nMeshes = 0;                      // a hit whose mesh or triangle the scene does not have is a miss
    float curRef = 1.0f;                  // currentRefIndex of RT:656-667
    // "is this output asked": kernel arguments, so every branch on them is wave-uniform
    int wantSurface = 0, wantReflect = 0, wantRefract = 0;
    xrt_surface *surfaceOut = nullptr;    // the CALLER's arrays, or null
    xrt_ray *reflectOut = nullptr;
    xrt_ray *refractOut = nullptr;
    unsigned long long *liveCount = nullptr;   // the entries treated as hits (a zeroed word)
};
// V: shade, materials, texels, meshes, addressMode and filtering are read; the lights are not.
void launch_surface(const ShadeView &V, const SurfaceArgs &A, hipStream_t st);

}  // namespace xrt
