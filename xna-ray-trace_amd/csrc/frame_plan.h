// frame_plan.h — what frame_begin (xrt_api.cpp) decides about a frame before it touches the device: declarations only.  plan_frame is defined in
// xrt_api.cpp, calls no HIP function and writes nothing but its output, so a program without a GPU can walk the whole lattice of decisions
// (tests/frame_plan/host_plan.cpp).  Included by scene_state.h (a frame context keeps the plan of its frame), behind the includer's `using namespace xrt`.
#pragma once
#include "../../include/xrt.h"
#include "kernels.h"

struct xrt_scene;
namespace xrt { struct PixelGenArgs; }   // pixels.h

// A caller's ray list as the ray source of a pass (xrt_cast_rays): n rays in HBM, 16-byte aligned, and generation 0's curRef.
struct BatchSrc {
    const xrt_ray *rays = nullptr;
    long long n = 0;
    float refIndex = 1.0f;
    // xrt_cast_rays_paths: where the ray paths go (HBM; kernels.h PathsEmitArgs), or null
    struct Paths {
        xrt_path_vertex *vertices = nullptr;
        long long capacity = 0;
        long long *vertexStart = nullptr;   // [n + 1], never null
        xrt_ray *raysBack = nullptr;
    };
    const Paths *paths = nullptr;
    // xrt_shade_hits: the closest hits of the rays (n xrt_hit in HBM, 16-byte aligned) -- generation 0 is ingested from them and not traced -- or null
    const xrt_hit *hits = nullptr;
    // xrt_render_opts.list_order == XRT_LIST_COHERENT: consecutive rays are neighbours, the pass picks its kernels as a frame does (FramePlan::pkMask)
    bool coherent = false;
    int samples = 1;   // ... of which sampling: the rays per screen position the list was made with (1, 4, 16; read with `coherent` alone)
    // xrt_render_pixels with that hint: generation 0 comes from a list of screen positions (pixels.h k_pixel_raygen) and `rays` is null -- no ray
    // record exists before the live list -- or null
    const xrt::PixelGenArgs *gen = nullptr;
};

constexpr int ADAPTIVE_LEVEL_WORDS = 16;   // adaptive frames in flight: words in front of the per-pass counters -- lvlCnt[0 .. quality], the overflow word at the end

// Every member holds its final value: nothing is decided again, or differently, once plan_frame has returned.
struct FramePlan {
    xrt::RayGenParams g{};           // the frame's ray generation: camera (or batch), shard, cull rectangle, level map, tileOfSlot
    int R = 0, nL = 0;               // MaxReflections, lights
    int addressMode = 0, filtering = 0;
    // tiles and paths
    bool tabled = false;             // an installed tile table names this rank's tiles (g.tileOfSlot)
    long long totalTiles = 0, myTiles = 0, totalPixels = 0;
    long long framePaths = 0;        // the whole frame (this shard)
    long long partStart = 0, firstPaths = 0;   // this part of it
    long long hintPaths = -1;        // key of the grid hints (-1: parts and adaptive frames have none)
    unsigned long long validPixels = 0;   // pixels of this part that lie inside the image
    size_t nodes = 0;                // level records per path
    long long chunkPaths = 0;
    int P = 0;                       // (int)chunkPaths
    size_t rayCap = 0, liveCap = 0, lvlStride = 0, shadowCap = 0;
    int cntStride = 0, qStride = 0;  // per chunk: counter words, queue words
    bool lvlVerified = false;        // LvlMap::inv was checked against every tile of this geometry: the caller notes it (xrt_scene::lvlChecked*)
    // the pipeline
    bool heap = false;               // Transparent materials: a binary ray tree (RT:586-702)
    bool adaptive = false;           // XRT_MS_ADAPTIVE
    int quality = 0;
    bool batch = false, capturePaths = false;   // the paths are a caller's rays (BatchSrc); ... and their ray paths are recorded
    bool givenHits = false;          // ... and their closest hits are the caller's too (BatchSrc::hits): closest-hit launch #0 and its counting pass do not happen
    bool collect = false;            // the counting pass (xrt_render_opts.collect_stats)
    bool fast = false;               // nothing but kernels on the stream: counters come back with k_compose, the events ride on kernels
    bool heapFast = false;           // a ray-tree frame the optimistic way (fast)
    bool adaptiveFast = false;       // an adaptive frame in flight (fast)
    bool ae = false;                 // answered at emission (ShadeArgs::ae)
    bool finishA = false;            // hits finished in part A (ShadeArgs::finish)
    bool endEarly = false;           // generation-0 paths coloured where they end (EndArgs)
    bool skipTiles = false;          // ... and the tiles outside the level map take no part (EndArgs::skipTiles)
    unsigned long long endSkipped = 0;   // ... their paths
    bool fuseResolve = false;        // k_compose writes the framebuffer itself
    bool wantF32 = false;            // float colours go through the context's sampleF32
    bool wantFeedback = false;       // the long-ray cost map is written and read
    bool listLong = false;           // producers list their long rays
    bool hinted = false;             // launches are sized by the last frame's generations (xrt_scene::gen*)
    bool tileCosts = false;          // packets add their ticks to the scene's tile costs
    bool useStamps = false;          // traversal launches time themselves on the device clock
    int pkMask = 0;                  // which ray populations take the packet kernel
    size_t pkEntries = 0;            // entries of the packet table of the primary rays (kernels.h QuadTable): one per 64 places of a chunk's generation-0 walk; 0: launch #0 takes no table
    size_t scrRefs = 0;              // entries of the frame's table of screen boxes (screen_rects.h): one per leaf reference of the one body; 0: launch #0 takes no such table
    int shadeBlock = 1024;           // threads per block of every k_shade launch over a big or unknown generation (Settings::shadeBlock; a small hinted one takes 256)
    bool ownStream = false;          // no stream given and the frame is worth the context's own
    int cntBase = 0, levelCap = 0;   // adaptive in flight: words in front of the per-pass counters in `pinned`; quadrant capacity of a deeper level
};

// The plan of part `part` of `nParts` of a frame of scene `s` with the materials of version `matVersion`; batch != null: of a pass over a caller's rays
// (cam is not read).  Returns XRT_OK or the code frame_begin reports for the arguments (message in g_err).
int plan_frame(const xrt_scene &s, int matVersion, const xrt_camera *cam, const xrt_light *lights, int nLights, const xrt_render_opts *opts, bool wantsF32,
               bool hasStream, int part, int nParts, bool heapFastAllowed, const BatchSrc *batch, FramePlan &plan);

// What list calls outside a frame share with that decision (pure, beside plan_frame): pkMask of a plain frame or coherent list of `samples` rays per position; the scene's part of `ae`.
int scene_packet_mask(const xrt_scene &s, int samples);
bool scene_answers_at_emission(const xrt_scene &s);
