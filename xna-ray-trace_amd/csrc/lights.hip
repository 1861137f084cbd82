// lights.hip — CastRay's light loop (RT:534-542) on caller-given hits (xrt.h xrt_light_hits; gfx950, wave64).
// For a hit the reference asks IsLightPathObstructed once per light (RT:465-502: a closest-hit query from the hit towards the light) and sums
// GetLightForFragment scaled by 1 - lightAmount.  Frames do this inside k_shade (kernels.hip: part A emits the shadow rays, part B folds their
// answers); here the same three steps stand alone, on a caller's list: k_light_emit forms the shadow rays, the traversal kernels answer them
// unchanged (IntersectArgs::scatter / flags), k_light_fold turns the answers into the amounts and the fp32 light sum.  The arithmetic is
// k_shade's, restated (kernels.hip stays as it is) and compiled with the same flags: contraction off, every operation its own rounding.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "lights.h"
#include "xrt_core.h"

namespace xrt {

namespace {

// wave64 inclusive scan on the DPP network (row shifts, then the two row broadcasts), as hits.hip's
__device__ __forceinline__ int lights_scan_add(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return v;
}

// A quarter of a record as four 32-bit words in registers: one 16-byte load
typedef int W4 __attribute__((ext_vector_type(4)));

// RT:469-479 direction and distance towards a light (kernels.hip light_dir)
__device__ __forceinline__ void lights_dir(const LightRec &L, v3 world, v3 &dir, float &dist) {
    if (L.kind == 0) {
        v3 t = sub(mk(L.px, L.py, L.pz), world);
        dist = length(t);
        dir = normalize(t);
    } else {
        dir = neg(mk(L.dx, L.dy, L.dz));
        dist = FLT_MAX;
    }
}
// RT:520-531 fragment normal (kernels.hip fragment_normal)
__device__ __forceinline__ v3 lights_fragment_normal(const ShadeView &V, int gtri, int matFlags, float u, float v) {
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
// Would the one body's one mesh answer this world-space ray "no intersection" because all its triangles face away from it (kernels.hip
// faces_away_single: the object-space direction as the traversal kernels form it, OSM:358-364, and their test; a NaN anywhere makes it false)?
__device__ __forceinline__ bool lights_faces_away_single(const SceneView &S, v3 o, v3 d) {
    const ObjRec &ob = S.objects[0];
    const MeshRec &mr = S.meshes[0];
    const v3 v1 = transform(o, ob.invWorld);
    const v3 v2 = transform(add(o, d), ob.invWorld);
    const v3 dir = normalize(sub(v2, v1));
    return mesh_faces_away(mr, dir);
}
// "The query returned this record": hit != 0 with a mesh and a triangle the scene has.  Anything else is a miss and addresses nothing.
__device__ __forceinline__ bool lights_live(const SceneView &S, const W4 head) {
    const int mesh = head.z, tri = head.w;
    bool live = head.x != 0 && mesh >= 0 && mesh < S.nMeshes && tri >= 0;
    if (live) live = tri < S.meshes[mesh].ntri;
    return live;
}

}  // namespace

// Entry e of the chunk is hits[base + e].  A thread reads the (hit, object, mesh, tri) quarter of its entry first and the position only of a
// live one, so a miss costs 16 bytes and no ray.  Then, LIGHT_EMIT_LIGHTS lights at a time: the shadow ray of every (live entry, light) pair
// -- (worldPosition, dirToLight), the query ignores the shaded triangle (RT:482-485) --, one ballot per light, one wave scan of the block's
// 64 cells, one atomic per block and round, and the rays go into the compact list with their scatter word e * nLights + l.  With `ae` a pair
// whose ray the one mesh faces away from gets its answer word here, 0, and is not listed.  A ray is never skipped for what the light would
// contribute: the amount is an output of its own, and 1 - amount must reach the sum as the reference forms it.
__global__ __launch_bounds__(LIGHT_EMIT_BLOCK) void k_light_emit(SceneView S, LightEmitArgs A) {
    __shared__ int ldsCells[64];
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    const int groups = (A.n + LIGHT_EMIT_BLOCK - 1) / LIGHT_EMIT_BLOCK;
    for (int grp = (int)blockIdx.x; grp < groups; grp += (int)gridDim.x) {
        const int e = grp * LIGHT_EMIT_BLOCK + (int)threadIdx.x;
        bool live = false;
        int mesh = -1, tri = -1;
        v3 w = mk(0, 0, 0);
        if (e < A.n) {
            const W4 *rec = reinterpret_cast<const W4 *>(A.hits + (A.base + e));
            const W4 a = rec[0];   // hit object mesh tri
            live = lights_live(S, a);
            if (live) {
                const W4 c = rec[2];   // w.xyz reserved
                mesh = a.z; tri = a.w;
                w = mk(i2f(c.x), i2f(c.y), i2f(c.z));
            }
        }
        for (int l0 = 0; l0 < A.nLights; l0 += LIGHT_EMIT_LIGHTS) {   // (block-uniform)
            v3 dir[LIGHT_EMIT_LIGHTS];
            int rank[LIGHT_EMIT_LIGHTS];   // among the emitting lanes of the wave, -1: no ray
#pragma unroll
            for (int r = 0; r < LIGHT_EMIT_LIGHTS; r++) {
                const int l = l0 + r;
                bool emit = false;
                dir[r] = mk(0, 0, 0);
                if (live && l < A.nLights) {
                    float dist;
                    lights_dir(A.lights[l], w, dir[r], dist);
                    emit = !(A.ae && lights_faces_away_single(S, w, dir[r]));
                    if (!emit) A.flags[(size_t)e * (size_t)A.nLights + (size_t)l] = 0;   // IsLightPathObstructed's query finds nothing (RT:482-485)
                }
                const unsigned long long m = __ballot(emit);
                rank[r] = emit ? lanes_below(m) : -1;
                if (lane == 0) ldsCells[r * 16 + wave] = (int)__popcll(m);
            }
            __syncthreads();
            if (wave == 0) {   // reserves the block's range of the list
                const int c = ldsCells[lane];   // cell r * 16 + w: light by light, ascending entries
                const int incl = lights_scan_add(c);
                const int total = __builtin_amdgcn_readlane(incl, 63);
                int first = 0;
                if (lane == 0 && total) first = atomicAdd(A.count, total);
                first = __builtin_amdgcn_readfirstlane(first);
                ldsCells[lane] = first + incl - c;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < LIGHT_EMIT_LIGHTS; r++) {
                if (rank[r] >= 0) {
                    const int slot = ldsCells[r * 16 + wave] + rank[r];
                    if (slot < A.cap) {   // (rays listed <= n * nLights <= cap: the guard is against a wrong bound, not a code path)
                        store_ray(A.rays + slot, w, dir[r], mesh, tri);   // ignore = shaded triangle (RT:485)
                        A.scatter[slot] = e * A.nLights + l0 + r;
                    }
                }
            }
            __syncthreads();   // the cells are reused by the next round
        }
    }
}

void launch_light_emit(const SceneView &S, const LightEmitArgs &A, hipStream_t st) {
    int blocks = (int)(((long long)A.n + LIGHT_EMIT_BLOCK - 1) / LIGHT_EMIT_BLOCK);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_light_emit, dim3(blocks), dim3(LIGHT_EMIT_BLOCK), 0, st, S, A);
}

// One thread per entry.  A miss -- hit == 0, or a mesh / triangle the scene does not have -- is light (0, 0, 0) and amount 0 for every light.  A
// hit: fragmentNormal (RT:520-531), then for every light in order lightAmount from the pair's answer (RT:485-501: obstructed when the query
// hit and its d, the object-space d of OSM:373,450, is below the world-space distance; color.W of a Transparent blocker's triangle, else 1) and
// lightResult += GetLightForFragment * (1 - lightAmount) when lightAmount != 1 (RT:538-541).  Nothing is quantised.
__global__ __launch_bounds__(LIGHT_FOLD_BLOCK) void k_light_fold(SceneView S, ShadeView V, LightFoldArgs A) {
    __shared__ int ldsLive[LIGHT_FOLD_BLOCK / 64];
    int nLive = 0;
    const int step = (int)gridDim.x * LIGHT_FOLD_BLOCK;
    const size_t nL = (size_t)V.nLights;
    for (int e = (int)blockIdx.x * LIGHT_FOLD_BLOCK + (int)threadIdx.x; e < A.n; e += step) {
        const W4 *rec = reinterpret_cast<const W4 *>(A.hits + (A.base + e));
        const W4 a = rec[0];   // hit object mesh tri
        const bool live = lights_live(S, a);
        v3 w = mk(0, 0, 0), normal = mk(0, 0, 0);
        if (live) {
            const W4 b = rec[1], c = rec[2];   // leaf u v d | w.xyz reserved
            w = mk(i2f(c.x), i2f(c.y), i2f(c.z));
            const int gtri = V.meshes[a.z].triBase + a.w;
            const MaterialRec M = V.materials[V.meshes[a.z].material];
            normal = lights_fragment_normal(V, gtri, M.flags, i2f(b.y), i2f(b.z));
            nLive++;
        }
        v3 lightResult = mk(0, 0, 0);
        const size_t out = (size_t)(A.base + e);
        for (int l = 0; l < V.nLights; l++) {
            float lightAmount = 0.0f;   // RT:485-501
            if (live) {
                const LightRec &Lt = V.lights[l];
                v3 dir; float dist;
                lights_dir(Lt, w, dir, dist);
                const size_t pair = (size_t)e * nL + (size_t)l;
                if (A.flags[pair] != 0) {   // (a miss has no record)
                    const W4 *sh = reinterpret_cast<const W4 *>(A.shadowHits + pair);
                    const W4 sa = sh[0], sb = sh[1];
                    const int smesh = sa.z, stri = sa.w;
                    if (sa.x && i2f(sb.w) < dist) {
                        const MaterialRec SM = V.materials[V.meshes[smesh].material];
                        if (SM.flags & MAT_TRANSPARENT) lightAmount = V.shade[(size_t)(V.meshes[smesh].triBase + stri) * 6 + 3].w;
                        else lightAmount = 1.0f;
                    }
                }
                if (lightAmount != 1.0f) lightResult = add(lightResult, scale(light_for_fragment(Lt, w, normal), 1.0f - lightAmount));   // RT:538-541
            }
            if (A.amountOut) A.amountOut[out * nL + (size_t)l] = lightAmount;
        }
        if (A.lightOut) {
            float *o = A.lightOut + 3 * out;
            o[0] = lightResult.x; o[1] = lightResult.y; o[2] = lightResult.z;
        }
    }
    // the entries treated as hits are only counted: one atomic per block
    for (int o = 32; o > 0; o >>= 1) nLive += __shfl_xor(nLive, o);
    if (lane_id() == 0) ldsLive[threadIdx.x >> 6] = nLive;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < LIGHT_FOLD_BLOCK / 64; k++) total += ldsLive[k];
        if (total) atomicAdd(A.liveCount, total);
    }
}

void launch_light_fold(const SceneView &S, const ShadeView &V, const LightFoldArgs &A, hipStream_t st) {
    int blocks = (int)(((long long)A.n + LIGHT_FOLD_BLOCK - 1) / LIGHT_FOLD_BLOCK);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_light_fold, dim3(blocks), dim3(LIGHT_FOLD_BLOCK), 0, st, S, V, A);
}

}  // namespace xrt
