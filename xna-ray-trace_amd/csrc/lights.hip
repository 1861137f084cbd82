// lights.hip — CastRay's light loop (RT:534-542) on caller-given hits (xrt.h xrt_light_hits; gfx950, wave64).
// For a hit the reference asks IsLightPathObstructed once per light (RT:465-502: a closest-hit query from the hit towards the light) and sums
// GetLightForFragment scaled by 1 - lightAmount.  Frames do this inside k_shade (kernels.hip: part A emits the shadow rays, part B folds their
// answers); here the same three steps stand alone, on a caller's list: k_light_emit forms the shadow rays, the traversal kernels answer them
// unchanged (IntersectArgs::scatter / flags), k_light_fold turns the answers into the amounts and the fp32 light sum.  The arithmetic is
// k_shade's: the statements of shade_math.h and xrt_core.h, compiled with the same flags: contraction off, every operation its own rounding.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "lights.h"
#include "shade_math.h"
#include "xrt_core.h"

namespace xrt {

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
            live = hit_names_scene(S.meshes, S.nMeshes, a);
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
                    light_dir(A.lights[l], w, dir[r], dist);
                    emit = !(A.ae && faces_away_single(S, w, dir[r]));
                    if (!emit) A.flags[(size_t)e * (size_t)A.nLights + (size_t)l] = 0;   // IsLightPathObstructed's query finds nothing (RT:482-485)
                }
                const unsigned long long m = __ballot(emit);
                rank[r] = emit ? lanes_below(m) : -1;
                if (lane == 0) ldsCells[r * 16 + wave] = (int)__popcll(m);
            }
            __syncthreads();
            if (wave == 0) reserve_cells(ldsCells, A.count);   // the block's range of the list (cell r * 16 + w: light by light, ascending entries)
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
        const bool live = hit_names_scene(S.meshes, S.nMeshes, a);
        v3 w = mk(0, 0, 0), normal = mk(0, 0, 0);
        if (live) {
            const W4 b = rec[1], c = rec[2];   // leaf u v d | w.xyz reserved
            w = mk(i2f(c.x), i2f(c.y), i2f(c.z));
            const int gtri = V.meshes[a.z].triBase + a.w;
            const MaterialRec M = V.materials[V.meshes[a.z].material];
            normal = fragment_normal(V, gtri, M.flags, i2f(b.y), i2f(b.z));
            nLive++;
        }
        v3 lightResult = mk(0, 0, 0);
        const size_t out = (size_t)(A.base + e);
        for (int l = 0; l < V.nLights; l++) {
            float lightAmount = 0.0f;   // RT:485-501
            if (live) {
                const LightRec &Lt = V.lights[l];
                v3 dir; float dist;
                light_dir(Lt, w, dir, dist);
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
    block_count_once<LIGHT_FOLD_BLOCK / 64>(A.liveCount, nLive, ldsLive);   // the entries treated as hits are only counted
}

void launch_light_fold(const SceneView &S, const ShadeView &V, const LightFoldArgs &A, hipStream_t st) {
    int blocks = (int)(((long long)A.n + LIGHT_FOLD_BLOCK - 1) / LIGHT_FOLD_BLOCK);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_light_fold, dim3(blocks), dim3(LIGHT_FOLD_BLOCK), 0, st, S, V, A);
}

}  // namespace xrt
