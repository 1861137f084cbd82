// surface.hip — what CastRay computes at a hit without asking the scene anything (xrt.h xrt_surface_hits; gfx950, wave64): the fragment normal
// (RT:520-531), the surface colour with its texture lookup (RT:568-581 == RT:711-724), the material terms of RT:584 / RT:699, and the two rays it
// casts next -- the reflection (RT:547-559) and the Snell refraction (RT:656-694).  Frames do this inside k_shade part A (kernels.hip), where it
// leaves the kernel only inside a colour; here it stands alone on a caller's list.  The arithmetic is k_shade's: the statements of shade_math.h
// and xrt_core.h, compiled with the same flags: contraction off, every operation its own rounding.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "shade_math.h"
#include "surface.h"
#include "xrt_core.h"

namespace xrt {

// One thread per entry, grid-stride.  Entry e of the piece is record base + e of every array.  A thread reads the (hit, object, mesh, tri)
// quarter of its hit first; a miss -- hit == 0, or a mesh / triangle the scene does not have -- costs those 16 bytes and gets the zero record
// and the null rays.  Of a hit the (leaf, u, v, d) quarter is read when u and v are needed (the surface record, an interpolated normal), the
// position quarter and the ray's direction only when a ray output is asked, and of the triangle's six shade words what the asked outputs need:
// the flat normal alone (s5) for the rays of an uninterpolated material, everything for the surface record.  The three switches are kernel
// arguments: every branch on them is wave-uniform.
__global__ __launch_bounds__(SURFACE_BLOCK) void k_surface(ShadeView V, SurfaceArgs A) {
    __shared__ int ldsLive[SURFACE_BLOCK / 64];
    int nLive = 0;
    const bool wantRays = A.wantReflect || A.wantRefract;
    const int step = (int)gridDim.x * SURFACE_BLOCK;
    // (e + step can pass INT_MAX only behind the last entry of a piece of 2^30: the loop index is kept in 64 bits)
    for (long long e = (long long)blockIdx.x * SURFACE_BLOCK + (long long)threadIdx.x; e < (long long)A.n; e += step) {
        const size_t at = A.base + (size_t)e;
        const W4 *rec = reinterpret_cast<const W4 *>(A.hits + at);
        const W4 a = rec[0];   // hit object mesh tri
        const int mesh = a.z, tri = a.w;
        if (!hit_names_scene(V.meshes, A.nMeshes, a)) {
            if (A.wantSurface) {
                W4 *o = reinterpret_cast<W4 *>(A.surfaceOut + at);
                const W4 z = {0, 0, 0, 0};
                o[0] = z; o[1] = z; o[2] = z; o[3] = z;
            }
            if (A.wantReflect) store_ray(A.reflectOut + at, mk(0, 0, 0), mk(0, 0, 0), -1, -1);
            if (A.wantRefract) store_ray(A.refractOut + at, mk(0, 0, 0), mk(0, 0, 0), -1, -1);
            continue;
        }
        nLive++;
        const int gtri = V.meshes[mesh].triBase + tri;
        const MaterialRec M = V.materials[V.meshes[mesh].material];
        const f4 *sr = V.shade + (size_t)gtri * 6;
        float u = 0.0f, v = 0.0f;
        if (A.wantSurface || (M.flags & MAT_INTERP)) {
            const W4 b = rec[1];   // leaf u v d
            u = i2f(b.y); v = i2f(b.z);
        }
        const v3 normal = fragment_normal(V, gtri, M.flags, u, v);
        const bool transparent = (M.flags & MAT_TRANSPARENT) != 0;
        float n1 = 1.0f, n2 = A.curRef;
        if (transparent) refraction_indices(A.curRef, M.refractionIndex, n1, n2);
        if (A.wantSurface) {
            // RT:568-575 interpolatedUV, formed for every hit; the lookup only where the material uses its texture
            float ix, iy;
            interpolated_uv(sr, u, v, ix, iy);
            const f4 s3 = sr[3];   // (colour and alpha)
            v3 surf;
            if (M.flags & MAT_TEXTURE) surf = lookup_uv(V, M, ix, iy);
            else surf = mk(s3.x, s3.y, s3.z);   // RT:577-580
            const int flags = XRT_SURF_HIT | (transparent ? XRT_SURF_TRANSPARENT : 0) | ((M.flags & MAT_INTERP) ? XRT_SURF_INTERPOLATED : 0) |
                              ((M.flags & MAT_TEXTURE) ? XRT_SURF_TEXTURED : 0);
            f4 *o = reinterpret_cast<f4 *>(A.surfaceOut + at);
            o[0] = f4{normal.x, normal.y, normal.z, M.reflectiveness};
            o[1] = f4{surf.x, surf.y, surf.z, s3.w};
            o[2] = f4{ix, iy, M.refractionIndex, n2};
            o[3] = f4{i2f(flags), 0.0f, 0.0f, 0.0f};
        }
        if (wantRays) {
            const W4 c = rec[2];   // w.xyz reserved
            const v3 w = mk(i2f(c.x), i2f(c.y), i2f(c.z));
            const f4 *rp = reinterpret_cast<const f4 *>(A.rays + at);
            const f4 r0 = rp[0], r1 = rp[1];
            const v3 dd = mk(r0.w, r1.x, r1.y);   // ray.Direction
            if (A.wantReflect) store_ray(A.reflectOut + at, w, normalize(reflect(dd, normal)), mesh, tri);   // RT:548-550, origin = result.triangle (RT:559)
            if (A.wantRefract) {
                if (transparent) store_ray(A.refractOut + at, w, refract_dir(dd, normal, n1, n2), mesh, tri);   // RT:692-694
                else store_ray(A.refractOut + at, mk(0, 0, 0), mk(0, 0, 0), -1, -1);
            }
        }
    }
    block_count_once<SURFACE_BLOCK / 64>(A.liveCount, nLive, ldsLive);   // the entries treated as hits are only counted
}

void launch_surface(const ShadeView &V, const SurfaceArgs &A, hipStream_t st) {
    long long blocks = ((long long)A.n + SURFACE_BLOCK - 1) / SURFACE_BLOCK;
    if (blocks > SURFACE_MAX_BLOCKS) blocks = SURFACE_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_surface, dim3((unsigned)blocks), dim3(SURFACE_BLOCK), 0, st, V, A);
}

}  // namespace xrt
