// screen_rects.hip — k_screen_rects: the per-frame table of screen boxes of a one-body scene's leaf references (screen_rects.h), written in the frame's
// stream in front of the packet launch of its primary rays.  One entry of 8 bytes per reference, in refT order: a leaf's entries are contiguous.
// gfx950; double arithmetic (the entries are compared bit for bit with the host's evaluation of the same functions).
#include "device_util.h"
#include "kernels.h"
#include "screen_rects.h"

namespace xrt {

// The frame's part (make_screen_xf: a 4 x 4 inverse and the error terms, a few thousand dependent double operations) is one thread's work and needs every vector
// register there is; it runs as a kernel of its own so that the table kernel, whose 1.9 million threads (C5) need a fraction of them, keeps its occupancy.
__global__ __launch_bounds__(64) void k_screen_xf(RayGenParams g, const ObjRec *__restrict__ objects, ScreenXf *__restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) make_screen_xf(g, objects[0].invWorld, *out);   // (the frame's pose version: the matrix lane_begin applies)
}

__global__ __launch_bounds__(256) void k_screen_rects(const ScreenXf *__restrict__ xf, const float *__restrict__ refT, int nRefs, uint2 *__restrict__ table) {
    __shared__ ScreenXf X;
    static_assert(sizeof(ScreenXf) % 8 == 0 && sizeof(ScreenXf) / 8 <= 256, "one 8-byte word per thread");
    if (threadIdx.x < sizeof(ScreenXf) / 8) reinterpret_cast<unsigned long long *>(&X)[threadIdx.x] = reinterpret_cast<const unsigned long long *>(xf)[threadIdx.x];
    __syncthreads();
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < (size_t)nRefs; r += (size_t)gridDim.x * blockDim.x) {
        const float *q = refT + r * TRI_REC_WORDS;
        const float v1[3] = {q[4], q[5], q[6]}, e1[3] = {q[7], q[8], q[9]}, e2[3] = {q[10], q[11], q[12]};
        const ScrEntry e = screen_entry(X, v1, e1, e2);
        table[r] = make_uint2(e.x, e.y);
    }
}

// table: nRefs entries and, behind them, SCREEN_XF_SLOTS more that hold the frame's ScreenXf
void launch_screen_rects(const RayGenParams &g, const ObjRec *objects, const float *refT, int nRefs, uint2 *table, hipStream_t st) {
    static_assert(sizeof(ScreenXf) <= SCREEN_XF_SLOTS * sizeof(uint2), "the frame's part fits behind the table");
    if (nRefs <= 0) return;
    ScreenXf *const xf = reinterpret_cast<ScreenXf *>(table + nRefs);
    int blocks = (nRefs + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_screen_xf, dim3(1), dim3(64), 0, st, g, objects, xf);
    hipLaunchKernelGGL(k_screen_rects, dim3(blocks), dim3(256), 0, st, xf, refT, nRefs, table);
}

}  // namespace xrt
