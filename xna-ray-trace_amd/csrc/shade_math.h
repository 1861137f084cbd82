// shade_math.h — RayTracer.CastRay's arithmetic at one hit, stated once for every kernel that shades (gfx950, device code only): the fragment normal, the
// way to a light, the texture lookup with its interpolated coordinates, "the one mesh faces away from this ray", Snell's refraction, which hit records
// name something the scene has, and the way back up: one level of the composition and the supersampling mean.  k_shade (kernels.hip) is their first
// user; the list calls -- k_ingest_hits (hits.hip), k_light_emit / k_light_fold (lights.hip), k_surface (surface.hip), k_compose_hits (compose.hip),
// k_pixel_resolve (pixels.hip) -- call the same functions.  Results must be bit-identical to the oracle: the association order, where a double
// is used and which NaN comes out are properties of the statements below, so a fix is made here and nowhere else.  Every user is built with
// -ffp-contract=off: each operation its own rounding.
#pragma once
#include "kernels.h"
#include "traverse.h"
#include "xrt_core.h"
#include "device_util.h"

namespace xrt {

// RT:520-531 fragment normal
__device__ __forceinline__ v3 fragment_normal(const ShadeView &V, int gtri, int matFlags, float u, float v) {
    const f4 *s = V.shade + (size_t)gtri * 6;
    if (matFlags & MAT_INTERP) {
        f4 s0 = s[0], s1 = s[1], s2 = s[2];
        v3 n1 = mk(s0.x, s0.y, s0.z), n2 = mk(s1.x, s1.y, s1.z), n3 = mk(s2.x, s2.y, s2.z);
        v3 a = sub(n2, n1), b = sub(n3, n1);
        return normalize(add(add(n1, scale(a, u)), scale(b, v)));
    }
    f4 s5 = s[5];
    return mk(s5.x, s5.y, s5.z);
}
// RT:469-479 direction and distance towards a light
__device__ __forceinline__ void light_dir(const LightRec &L, v3 world, v3 &dir, float &dist) {
    if (L.kind == 0) {
        v3 t = sub(mk(L.px, L.py, L.pz), world);
        dist = length(t);
        dir = normalize(t);
    } else {
        dir = neg(mk(L.dx, L.dy, L.dz));
        dist = FLT_MAX;
    }
}

// RT:568-575 interpolatedUV of the triangle whose six shade words start at sr, at the hit's (u, v)
__device__ __forceinline__ void interpolated_uv(const f4 *sr, float u, float v, float &ix, float &iy) {
    f4 s0 = sr[0], s1 = sr[1], s2 = sr[2], s4 = sr[4];
    float uv1x = s0.w, uv1y = s1.w, uv2x = s2.w, uv2y = s4.x, uv3x = s4.y, uv3y = s4.z;
    float ax = uv2x - uv1x, ay = uv2y - uv1y, bx = uv3x - uv1x, by = uv3y - uv1y;
    ix = (uv1x + ax * u) + bx * v; iy = (uv1y + ay * u) + by * v;
}
// MAT:71-160 LookupUV: address mode, then point sample or the bilinear filter of MAT:162-232
__device__ __forceinline__ v3 lookup_uv(const ShadeView &V, const MaterialRec &M, float ux, float uy) {
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
        // A coordinate that is not a number (the reference throws: its texel index is 0x80000000) makes every weight below NaN.  Which NaN is no property
        // of the arithmetic: ocml's remainder() returns the canonical one where glibc's hands its argument's on, and a subtraction here flips the sign
        // of a NaN subtrahend where SSE keeps it.  So the answer is stated: the canonical quiet NaN in every channel (texture lookup).
        if (is_nan(ux) || is_nan(uy)) { const float qnan = i2f(0x7fc00000); return mk(qnan, qnan, qnan); }
        const float tdx = 1.0f / (float)M.texWidth, tdy = 1.0f / (float)M.texHeight;   // MAT:67
        const double remX = remainder((double)ux, (double)tdx), remY = remainder((double)uy, (double)tdy);   // Math.IEEERemainder, exact
        ux -= (float)remX;
        uy -= (float)remY;
        const int bx = (int)(ux * (float)(M.texWidth - 1)), by = (int)(uy * (float)(M.texHeight - 1));   // (numbers in [0, W] by now: no cvt_i32)
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
    if (idx < 0 || idx >= (long long)M.texWidth * M.texHeight) idx = 0;   // the C# reads through a raw pointer; a NaN uv (x or y = 0x80000000) reads texel 0
    uint32_t argb = V.texels[M.texOffset + idx];
    const float BYTE_RECIPROCAL = 1.0f / 255.0f;   // MAT:27
    return mk((float)((argb >> 16) & 0xffu) * BYTE_RECIPROCAL, (float)((argb >> 8) & 0xffu) * BYTE_RECIPROCAL, (float)(argb & 0xffu) * BYTE_RECIPROCAL);
}

// ShadeArgs::ae / LightEmitArgs::ae: would the one body's one mesh answer this world-space ray "no intersection" because all its triangles face away from it?
// The object-space direction is formed exactly as the traversal kernels form it (traverse.h lane_begin, OSM:358-364), the test is theirs
// (traverse.h mesh_faces_away: the mesh's normal box and its diagonal box, each with its margin; a NaN anywhere makes it false: such a ray is traced).
__device__ __forceinline__ bool faces_away_single(const SceneView &S, v3 o, v3 d) {
    const ObjRec &ob = S.objects[0];
    const MeshRec &mr = S.meshes[0];
    const v3 v1 = transform(o, ob.invWorld);
    const v3 v2 = transform(add(o, d), ob.invWorld);
    const v3 dir = normalize(sub(v2, v1));
    return mesh_faces_away(mr, dir);
}

// RT:656-694 Snell refraction, the System.Math calls in double; a total internal reflection is the square root of a negative number, NaN.
// n2 is what the nested CastRay receives as its currentRefIndex (RT:698).
__device__ __forceinline__ void refraction_indices(float curRef, float refractionIndex, float &n1, float &n2) {
    if (curRef == refractionIndex) { n1 = 1.0f; n2 = curRef; }
    else { n1 = refractionIndex; n2 = 1.0f; }
}
__device__ __forceinline__ v3 refract_dir(v3 dd, v3 normal, float n1, float n2) {
    const float cos1 = dot(normal, neg(dd));
    const double ratio = (double)(n1 / n2), c1 = (double)cos1;
    const float cos2 = (float)sqrt(1 - (ratio * ratio) * (1 - (c1 * c1)));   // Math.Pow(x, 2.0) == x*x exactly here
    const float q = n1 / n2;
    const v3 a = scale(dd, q), b = scale(normal, q * cos1 - cos2);
    return normalize(cos1 >= 0 ? add(a, b) : sub(a, b));
}

// "The query returned this record": hit != 0 with a mesh and a triangle the scene has (head: the record's hit, object, mesh, tri quarter).  Anything else
// is a miss and addresses nothing.
__device__ __forceinline__ bool hit_names_scene(const MeshRec *meshes, int nMeshes, const W4 head) {
    const int mesh = head.z, tri = head.w;
    bool live = head.x != 0 && mesh >= 0 && mesh < nMeshes && tri >= 0;
    if (live) live = tri < meshes[mesh].ntri;
    return live;
}

// The return path of the CastRay recursion, one level: the deepest hit of a path that reached generation MaxReflections has no reflection term
// (RT:708-727); every other level blends what came back from below -- quantised, RT:705 -- with its surface colour by its Reflectiveness (RT:584),
// and on a Transparent material blends what came back through the surface with that by color.W (RT:699).  The caller quantises the result
// (pack_color).  Users: k_shade, k_compose, k_compose_tree (kernels.hip) and k_compose_hits (compose.hip).
__device__ __forceinline__ v3 compose_last(v3 light, v3 surf) { return mul(light, surf); }
__device__ __forceinline__ v3 compose_step(uint32_t below, v3 surf, float refl, v3 light) { return mul(lerp(unpack_color(below), surf, 1.0f - refl), light); }
__device__ __forceinline__ v3 compose_refraction(uint32_t through, v3 cv, float alpha) { return lerp(unpack_color(through), cv, alpha); }
// RT:309: the mean of four quantised colours, summed left to right, re-quantised.  Users: k_resolve (kernels.hip), k_pixel_resolve (pixels.hip).
__device__ __forceinline__ uint32_t mean4(const uint32_t *s /* four colours */) {
    const v3 sum = add(add(add(unpack_color(s[0]), unpack_color(s[1])), unpack_color(s[2])), unpack_color(s[3]));
    return pack_color(divf(sum, 4.0f));
}

}  // namespace xrt
