// surface.hip — what CastRay computes at a hit without asking the scene anything (xrt.h xrt_surface_hits; gfx950, wave64): the fragment normal
// (RT:520-531), the surface colour with its texture lookup (RT:568-581 == RT:711-724), the material terms of RT:584 / RT:699, and the two rays it
// casts next -- the reflection (RT:547-559) and the Snell refraction (RT:656-694).  Frames do this inside k_shade part A (kernels.hip), where it
// leaves the kernel only inside a colour; here it stands alone on a caller's list.  The arithmetic is k_shade's, restated (kernels.hip stays as
// it is) and compiled with the same flags: contraction off, every operation its own rounding.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "surface.h"
#include "xrt_core.h"

namespace xrt {

namespace {

// A quarter of a record as four 32-bit words in registers: one 16-byte load / store
typedef int W4 __attribute__((ext_vector_type(4)));

// RT:520-531 fragment normal (kernels.hip fragment_normal)
__device__ __forceinline__ v3 surface_fragment_normal(const f4 *s, int matFlags, float u, float v) {
    if (matFlags & MAT_INTERP) {
        f4 s0 = s[0], s1 = s[1], s2 = s[2];
        v3 n1 = mk(s0.x, s0.y, s0.z), n2 = mk(s1.x, s1.y, s1.z), n3 = mk(s2.x, s2.y, s2.z);
        v3 a = sub(n2, n1), b = sub(n3, n1);
        return normalize(add(add(n1, scale(a, u)), scale(b, v)));
    }
    f4 s5 = s[5];
    return mk(s5.x, s5.y, s5.z);
}

// MAT:71-160 LookupUV: address mode, then point sample or the bilinear filter of MAT:162-232 (kernels.hip lookup_uv)
__device__ __forceinline__ v3 surface_lookup_uv(const ShadeView &V, const MaterialRec &M, float ux, float uy) {
    if (V.addressMode == XRT_ADDRESS_WRAP) {   // MAT:125-136
        if (ux > 1.0f) ux = fmod1(ux);
        if (uy > 1.0f) uy = fmod1(uy);
        if (ux < 0.0f) ux = 1.0f + fmod1(ux);
        if (uy < 0.0f) uy = 1.0f + fmod1(uy);
    } else if (V.addressMode == XRT_ADDRESS_CLAMP) {   // MAT:138-143
        ux = (ux > 1.0f) ? 1.0f : ux; ux = (ux < 0.0f) ? 0.0f : ux;
        uy = (uy > 1.0f) ? 1.0f : uy; uy = (uy < 0.0f) ? 0.0f : uy;
    } else {   // MAT:102-123
        float ox = ux, oy = uy;
        if (ux > 1.0f) ux = fmod1(ux);
        if (uy > 1.0f) uy = fmod1(uy);
        if (ux < 0.0f) ux = 1.0f + fmod1(ux);
        if (uy < 0.0f) uy = 1.0f + fmod1(uy);
        if (cvt_i32(ox - ux) % 2 == 0) ux = 1.0f - ux;
        if (cvt_i32(oy - uy) % 2 == 0) uy = 1.0f - uy;
    }
    if (V.filtering == XRT_FILTER_BILINEAR) {   // MAT:162-232
        // a coordinate that is not a number: the canonical quiet NaN in every channel, as lookup_uv states it (texture lookup)
        if (is_nan(ux) || is_nan(uy)) { const float qnan = i2f(0x7fc00000); return mk(qnan, qnan, qnan); }
        const float tdx = 1.0f / (float)M.texWidth, tdy = 1.0f / (float)M.texHeight;   // MAT:67
        const double remX = remainder((double)ux, (double)tdx), remY = remainder((double)uy, (double)tdy);   // Math.IEEERemainder, exact
        ux -= (float)remX;
        uy -= (float)remY;
        const int bx = (int)(ux * (float)(M.texWidth - 1)), by = (int)(uy * (float)(M.texHeight - 1));
        const int bx2 = (int)((ux + tdx) * (float)(M.texWidth - 1)), by2 = (int)((uy + tdy) * (float)(M.texHeight - 1));
        auto texel = [&](int xx, int yy) {
            long long idx = (long long)M.texWidth * yy + xx;
            if (idx < 0 || idx >= (long long)M.texWidth * M.texHeight) idx = 0;
            uint32_t w = V.texels[M.texOffsetP + idx];   // MAT:186-189: Texture.ColorData
            return mk((float)((w >> 16) & 0xffu), (float)((w >> 8) & 0xffu), (float)(w & 0xffu));
        };
        const v3 c00 = texel(bx, by), c10 = texel(bx2, by), c01 = texel(bx, by2), c11 = texel(bx2, by2);
        const float dx = (float)(remX * (double)M.texWidth) + 0.5f, dy = (float)(remY * (double)M.texHeight) + 0.5f;
        const float ix = 1.0f - dx, iy = 1.0f - dy;
        v3 sum = add(add(add(scale(scale(c00, ix), iy), scale(scale(c01, ix), dy)), scale(scale(c10, dx), iy)), scale(scale(c11, dx), dy));
        return scale(sum, 1.0f / 255.0f);
    }
    int x = cvt_i32(ux * (float)(M.texWidth - 1));    // MAT:147
    int y = cvt_i32(uy * (float)(M.texHeight - 1));   // MAT:148
    long long idx = (long long)M.texWidth * y + x;
    if (idx < 0 || idx >= (long long)M.texWidth * M.texHeight) idx = 0;   // (a NaN uv reads texel 0)
    uint32_t argb = V.texels[M.texOffset + idx];
    const float BYTE_RECIPROCAL = 1.0f / 255.0f;   // MAT:27
    return mk((float)((argb >> 16) & 0xffu) * BYTE_RECIPROCAL, (float)((argb >> 8) & 0xffu) * BYTE_RECIPROCAL, (float)(argb & 0xffu) * BYTE_RECIPROCAL);
}

// RT:656-694 the refracted direction (kernels.hip k_shade part A, `tdir`): Snell's law with the System.Math calls in double; a total internal
// reflection is the square root of a negative number, NaN.  n2 is what the nested CastRay receives as its currentRefIndex (RT:698).
__device__ __forceinline__ void surface_next_index(float curRef, float refractionIndex, float &n1, float &n2) {
    if (curRef == refractionIndex) { n1 = 1.0f; n2 = curRef; }
    else { n1 = refractionIndex; n2 = 1.0f; }
}
__device__ __forceinline__ v3 surface_refract(v3 dd, v3 normal, float n1, float n2) {
    const float cos1 = dot(normal, neg(dd));
    const double ratio = (double)(n1 / n2), c1 = (double)cos1;
    const float cos2 = (float)sqrt(1 - (ratio * ratio) * (1 - (c1 * c1)));   // Math.Pow(x, 2.0) == x*x exactly here
    const float q = n1 / n2;
    const v3 a = scale(dd, q), b = scale(normal, q * cos1 - cos2);
    return normalize(cos1 >= 0 ? add(a, b) : sub(a, b));
}

}  // namespace

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
        bool live = a.x != 0 && mesh >= 0 && mesh < A.nMeshes && tri >= 0;
        if (live) live = tri < V.meshes[mesh].ntri;
        if (!live) {
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
        const v3 normal = surface_fragment_normal(sr, M.flags, u, v);
        const bool transparent = (M.flags & MAT_TRANSPARENT) != 0;
        float n1 = 1.0f, n2 = A.curRef;
        if (transparent) surface_next_index(A.curRef, M.refractionIndex, n1, n2);
        if (A.wantSurface) {
            // RT:568-575 interpolatedUV, formed for every hit; the lookup only where the material uses its texture
            const f4 s0 = sr[0], s1 = sr[1], s2 = sr[2], s3 = sr[3], s4 = sr[4];
            const float uv1x = s0.w, uv1y = s1.w, uv2x = s2.w, uv2y = s4.x, uv3x = s4.y, uv3y = s4.z;
            const float ax = uv2x - uv1x, ay = uv2y - uv1y, bx = uv3x - uv1x, by = uv3y - uv1y;
            const float ix = (uv1x + ax * u) + bx * v, iy = (uv1y + ay * u) + by * v;
            v3 surf;
            if (M.flags & MAT_TEXTURE) surf = surface_lookup_uv(V, M, ix, iy);
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
                if (transparent) store_ray(A.refractOut + at, w, surface_refract(dd, normal, n1, n2), mesh, tri);   // RT:692-694
                else store_ray(A.refractOut + at, mk(0, 0, 0), mk(0, 0, 0), -1, -1);
            }
        }
    }
    // the entries treated as hits are only counted: a wave reduction and one atomic per block (as lights.hip k_light_fold)
    for (int o = 32; o > 0; o >>= 1) nLive += __shfl_xor(nLive, o);
    if (lane_id() == 0) ldsLive[threadIdx.x >> 6] = nLive;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < SURFACE_BLOCK / 64; k++) total += ldsLive[k];
        if (total) atomicAdd(A.liveCount, (unsigned long long)total);
    }
}

void launch_surface(const ShadeView &V, const SurfaceArgs &A, hipStream_t st) {
    long long blocks = ((long long)A.n + SURFACE_BLOCK - 1) / SURFACE_BLOCK;
    if (blocks > SURFACE_MAX_BLOCKS) blocks = SURFACE_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_surface, dim3((unsigned)blocks), dim3(SURFACE_BLOCK), 0, st, V, A);
}

}  // namespace xrt
