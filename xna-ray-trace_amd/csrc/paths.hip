// paths.hip — RayTracer.points for xrt_cast_rays_paths (gfx950): the line segments every CastRay of a batch appends (RT:543, 701, 740-747) and the
// ray it leaves in its `ref Ray ray` (RT:692-694), as a second product of the pass that computes the colours.  Nothing is traced twice:
//
//   k_paths_capture  once per generation, after k_shade: the world position of every hit (from the slot record part A left) and the direction
//                    of every refraction child among the next generation's rays go to staging records at (node, path), tagged with the number
//                    of this attempt of the chunk -- a generation that is redone leaves nothing of its first attempt behind.
//   k_paths_count    once per chunk: a thread walks its path's recursion depth first (paths.h) and counts its vertices; block-wide exclusive scan.
//   k_paths_scan     one workgroup: the block totals behind what the chunks before needed -> where every block's vertices start.
//   k_paths_emit     the same walk again, writing: vertex_start, the vertices (one 16-byte store each, clipped at the caller's capacity), rays_back.
//
// The recursion is depth first and its output size is unknown before the call; the device works generation by generation.  The records
// are addressed as the level records are (kernels.h ShadeArgs: node * P + path), so the walk needs no sorting.
#include "kernels.h"
#include "device_util.h"
#include "paths.h"

namespace xrt {

__global__ __launch_bounds__(256) void k_paths_capture(PathsCaptureArgs A) {
    const int stride = (int)(gridDim.x * blockDim.x), tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const size_t P = (size_t)A.P;
    int n = *A.scnt;
    if (n > A.slotCap) n = A.slotCap;
    for (int s = tid; s < n; s += stride) {
        const f4 a = reinterpret_cast<const f4 *>(A.slots + s)[0];   // wx wy wz path
        const int node = A.slotNode ? A.slotNode[s] : A.level;
        A.hitRec[(size_t)node * P + (size_t)f2i(a.w)] = f4{a.x, a.y, a.z, i2f((int)A.epoch)};
    }
    if (!A.nextRays) return;
    int m = *A.nextCnt;
    if (m > A.nextCap) m = A.nextCap;
    for (int j = tid; j < m; j += stride) {
        const int node = A.nextNode[j];
        if (!path_is_refraction(node)) continue;
        v3 o, d; int im, it;
        load_ray(A.nextRays + j, o, d, im, it);
        A.dirRec[(size_t)node * P + (size_t)A.nextPath[j]] = f4{path_recorded(d.x), path_recorded(d.y), path_recorded(d.z), i2f((int)A.epoch)};
    }
}
void launch_paths_capture(const PathsCaptureArgs &A, int blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_paths_capture, dim3(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, A);
}

namespace {

struct StagedPath {   // paths.h Src over the staging records of path p
    const f4 *hitRec, *dirRec;
    size_t P, p;
    int epoch;
    XRT_HD bool hit(int node, float w[3]) const {
        const f4 r = hitRec[(size_t)node * P + p];
        w[0] = r.x; w[1] = r.y; w[2] = r.z;
        return f2i(r.w) == epoch;
    }
    XRT_HD bool refracted(int node, float d[3]) const {
        const f4 r = dirRec[(size_t)node * P + p];
        d[0] = r.x; d[1] = r.y; d[2] = r.z;
        return f2i(r.w) == epoch;
    }
};
struct CountSink {
    int n = 0;
    XRT_HD void segment(const float *, const float *, uint32_t) { n += 2; }
};
struct EmitSink {
    xrt_path_vertex *out;
    long long at, cap;   // (cap: whole segments)
    XRT_HD void segment(const float a[3], const float b[3], uint32_t color) {
        if (at + 2 <= cap) {
            f4 *dst = reinterpret_cast<f4 *>(out + at);
            dst[0] = f4{a[0], a[1], a[2], i2f((int)color)};
            dst[1] = f4{b[0], b[1], b[2], i2f((int)color)};
        }
        at += 2;
    }
};
__device__ __forceinline__ StagedPath staged(const PathsEmitArgs &A, int p) { return StagedPath{A.hitRec, A.dirRec, (size_t)A.P, (size_t)p, (int)A.epoch}; }
__device__ __forceinline__ void root_origin(const PathsEmitArgs &A, int p, f4 &a, f4 &b, float o[3]) {
    const f4 *src = reinterpret_cast<const f4 *>(A.batch + (A.pathBase + p));
    a = src[0]; b = src[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
}

}  // namespace

__global__ __launch_bounds__(PATHS_BLOCK) void k_paths_count(PathsEmitArgs A) {
    __shared__ int cells[PATHS_BLOCK];
    const int t = (int)threadIdx.x, p = (int)blockIdx.x * PATHS_BLOCK + t;
    int c = 0;
    if (p < A.Pc) {
        f4 a, b; float o[3];
        root_origin(A, p, a, b, o);
        CountSink sink;
        PathRay back;
        (void)paths_walk(staged(A, p), o, A.depth, A.tree != 0, sink, back);
        c = sink.n;
    }
    cells[t] = c;
    __syncthreads();
    int incl = c;
    for (int d = 1; d < PATHS_BLOCK; d <<= 1) {   // Hillis-Steele over the block
        const int v = t >= d ? cells[t - d] : 0;
        __syncthreads();
        incl += v;
        cells[t] = incl;
        __syncthreads();
    }
    if (p < A.Pc) A.local[p] = incl - c;
    if (t == PATHS_BLOCK - 1) A.blockSum[blockIdx.x] = incl;
}

__global__ __launch_bounds__(1024) void k_paths_scan(PathsEmitArgs A, int nBlocks) {
    __shared__ long long cells[1024];
    __shared__ long long carry;
    const int t = (int)threadIdx.x;
    if (t == 0) carry = A.pathBase > 0 ? A.vertexStart[A.pathBase] : 0;   // what the rays before this chunk need
    __syncthreads();
    for (int base = 0; base < nBlocks; base += 1024) {
        const int i = base + t;
        const long long c = i < nBlocks ? (long long)A.blockSum[i] : 0;
        cells[t] = c;
        __syncthreads();
        long long incl = c;
        for (int d = 1; d < 1024; d <<= 1) {
            const long long v = t >= d ? cells[t - d] : 0;
            __syncthreads();
            incl += v;
            cells[t] = incl;
            __syncthreads();
        }
        const long long before = carry;
        if (i < nBlocks) A.blockBase[i] = before + incl - c;
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    if (t == 0) A.vertexStart[A.pathBase + A.Pc] = carry;
}

__global__ __launch_bounds__(PATHS_BLOCK) void k_paths_emit(PathsEmitArgs A) {
    const int p = (int)blockIdx.x * PATHS_BLOCK + (int)threadIdx.x;
    if (p >= A.Pc) return;
    const long long start = A.blockBase[blockIdx.x] + A.local[p];
    A.vertexStart[A.pathBase + p] = start;
    f4 a, b; float o[3];
    root_origin(A, p, a, b, o);
    EmitSink sink{A.vertices, start, A.capacity & ~1LL};
    PathRay back;
    const bool changed = paths_walk(staged(A, p), o, A.depth, A.tree != 0, sink, back);
    if (A.raysBack) {
        f4 *dst = reinterpret_cast<f4 *>(A.raysBack + (A.pathBase + p));
        if (changed) { a = f4{back.o[0], back.o[1], back.o[2], back.d[0]}; b = f4{back.d[1], back.d[2], b.z, b.w}; }   // (ignore_mesh / ignore_tri: the caller's)
        dst[0] = a; dst[1] = b;
    }
}

void launch_paths_emit(const PathsEmitArgs &A, hipStream_t st) {
    const int blocks = (A.Pc + PATHS_BLOCK - 1) / PATHS_BLOCK;
    if (blocks < 1) return;
    hipLaunchKernelGGL(k_paths_count, dim3(blocks), dim3(PATHS_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_paths_scan, dim3(1), dim3(1024), 0, st, A, blocks);
    hipLaunchKernelGGL(k_paths_emit, dim3(blocks), dim3(PATHS_BLOCK), 0, st, A);
}

}  // namespace xrt
