// compose.hip — the way back up CastRay's recursion, one level, on a caller's list (xrt.h xrt_compose_hits; gfx950, wave64): from a hit's
// surface record (xrt_surface_hits), its light sum (xrt_light_hits) and the packed colours the two nested CastRay calls returned, the colour
// vector CastRay hands to `new Color` and that colour -- RT:726 at the last level, RT:584 above it, RT:699 behind a Transparent surface, RT:732
// for a miss, RT:705 for the quantisation.  Frames do this inside k_compose / k_compose_tree (kernels.hip) on their own records; here it stands
// alone.  The arithmetic is theirs: the statements of shade_math.h and xrt_core.h, compiled with the same flags: contraction off, every
// operation its own rounding.  (The RT:309 fold of xrt_fold_samples is k_pixel_resolve of pixels.hip.)
#include <hip/hip_runtime.h>

#include "compose.h"
#include "device_util.h"
#include "shade_math.h"
#include "xrt_core.h"

namespace xrt {

// One thread per entry, grid-stride.  Entry e of the piece is record base + e of every array.  A thread reads the (flags, reserved) quarter of
// its surface record first; an entry without XRT_SURF_HIT costs those 16 bytes and gets black (RT:732).  Of a hit the (color, alpha) quarter
// and the light's 12 bytes are read always, the (normal, reflectiveness) quarter and the reflection's colour only where a reflection is given,
// the refraction's colour only where one is given and the entry is Transparent.  The switches are kernel arguments: every branch on them is
// wave-uniform.  None of the pointers is __restrict__: rgbaOut may be reflect or refract, and a thread has read its entry of both before its
// one store to it.
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_hits(ComposeArgs A) {
    __shared__ int ldsHit[COMPOSE_BLOCK / 64];
    int nHit = 0;
    const int step = (int)gridDim.x * COMPOSE_BLOCK;
    // (e + step can pass INT_MAX only behind the last entry of a piece of 2^30: the loop index is kept in 64 bits)
    for (long long e = (long long)blockIdx.x * COMPOSE_BLOCK + (long long)threadIdx.x; e < (long long)A.n; e += step) {
        const size_t at = A.base + (size_t)e;
        const W4 *rec = reinterpret_cast<const W4 *>(A.surface + at);
        const int flags = rec[3].x;   // flags reserved[3]
        v3 cv = mk(0, 0, 0);          // RT:732
        if (flags & XRT_SURF_HIT) {
            nHit++;
            const W4 b = rec[1];      // color alpha
            const v3 surf = mk(i2f(b.x), i2f(b.y), i2f(b.z));
            const float *lp = A.light + 3 * at;
            const v3 light = mk(lp[0], lp[1], lp[2]);
            if (!A.haveReflect) cv = compose_last(light, surf);   // RT:726: iteration >= MaxReflections
            else {
                const W4 a = rec[0];   // normal reflectiveness
                cv = compose_step(A.reflect[at], surf, i2f(a.w), light);   // RT:584
                if (A.haveRefract && (flags & XRT_SURF_TRANSPARENT)) cv = compose_refraction(A.refract[at], cv, i2f(b.w));   // RT:699
            }
        }
        const uint32_t col = pack_color(cv);   // RT:705 (of black: 0xFF000000)
        if (A.wantRgba) A.rgbaOut[at] = col;
        if (A.wantF32) { float *o = A.f32Out + 3 * at; o[0] = cv.x; o[1] = cv.y; o[2] = cv.z; }
    }
    block_count_once<COMPOSE_BLOCK / 64>(A.hitCount, nHit, ldsHit);
}

void launch_compose_hits(const ComposeArgs &A, hipStream_t st) {
    long long blocks = ((long long)A.n + COMPOSE_BLOCK - 1) / COMPOSE_BLOCK;
    if (blocks > COMPOSE_MAX_BLOCKS) blocks = COMPOSE_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_compose_hits, dim3((unsigned)blocks), dim3(COMPOSE_BLOCK), 0, st, A);
}

}  // namespace xrt
