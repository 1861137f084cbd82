// settings.h — the environment switches of libxrt (INTEGRATION.md "Environment switches"), read once by xrt_scene_create into the scene's
// Settings; the replicas of an n_gpus > 1 render inherit their primary's.  Each member holds its default: a variable that is unset, does
// not parse or is out of range leaves it there.  XRT_ROCTX and XRT_RCCL_LIB are process-wide and read where they are used.
#pragma once

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <string>
#include <type_traits>

namespace xrt {

// Paths in flight per chunk (multiple of 512 * 16).  ~400 bytes of work buffers per path: 1920x1080 at 16 samples per
// pixel (33.2 M paths) is one chunk of 13 GB per frame context -- sized for 288 GB of HBM, so that whole frames take the
// single-chunk path (no host round trips, two frames overlapping).
constexpr int MAX_CHUNK_PATHS = 1 << 25;
constexpr int HEAP_RAY_CAP = 1 << 22;      // rays per generation of a ray-tree chunk
constexpr int MAX_STAMP_ROWS = 256;   // traversal launches of one frame that can time themselves (kernels.h STAMP_*)

struct Settings {
    // Which ray populations take the wave-packet kernel.  -1 (default): all three of a frame with 16 sub-rays per pixel -- a wave
    // then holds 4 pixels x 16 samples, rays that visit the same leaves (measured on the 1M-triangle frame: 7.3 against 11.1 ms);
    // none otherwise (64 pixels of a 1-sample frame fan out over too many leaves: 5 x slower than the per-lane kernel).
    // XRT_PACKET=<mask> forces it: bit 0 primary rays, 1 shadow rays, 2 closest-hit rays of later generations, 3 seam-1 batches,
    // 4 bits 1 and 2 also apply beyond generation 1 (default: the first two generations and the first shadow rays only).
    int packetMask = -1;
    int packetMaskHeap = -1;   // the same for ray-tree frames (XRT_PACKET_HEAP; -1: by image size)
    // Largest guided batch of k_intersect (XRT_BATCH_MAX).  Round 1 let a wave reserve up to 512 rays per atomic; per-wave clocks
    // (make WAVE_TIMES=1, tools/wave_times.py) showed the median wave of a C3 / C4 launch leaving at 57 % of the launch and the
    // tail growing with the frame size -- waves stuck with eight expensive rays per lane while the queue was empty.  64: C3 3.9 ->
    // 3.4 ms, C4 11.4 -> 9.4 ms per blocking frame; 32 and 16 lose to contention on the queue word.
    int batchMax = 64;
    int batchMin = 64;         // XRT_BATCH_MIN (development)
    // A launch of fewer rays than 64 per resident wave is dealt evenly over all waves in multiples of spreadMin instead of 64 to a
    // wave: a batch takes as long as its slowest ray and longer the more rays diverge in it, and idle waves cost nothing -- the ten
    // launches of a ray-tree frame of the reference's default scene: 1.05 -> 0.65 ms (XRT_SPREAD_MIN=64: as before).
    int spreadMin = 4;
    // XRT_TUNE="refill,nodeBurst,leafBurst[,coopMax]": refill threshold (idle lanes), octree-child steps and leaf steps per outer iteration
    // of k_intersect.  tune[0] = 0: the refill threshold is the scene's (xrt_scene::refillMin).
    int tune[4] = {0, 16, 48, 32};
    std::optional<int> heavyShift;   // XRT_HEAVY_SHIFT (unset: the scene's, xrt_scene::heavyShift)
    std::optional<int> firstBatch;   // XRT_FIRST_BATCH (unset: the scene's, xrt_scene::firstBatch)
    bool packetMerge = true;   // the closest-hit and the shadow packets of a step share one launch (XRT_PK_MERGE=0: two launches, as round 2)
    bool answerAtEmission = true;   // XRT_AE=0: k_shade emits every ray (kernels.h ShadeArgs::ae off)
    bool finishInPartA = true;      // XRT_AE_FINISH=0: a hit whose shadow rays were all answered at emission still takes a slot and waits for part B (kernels.h ShadeArgs::finish off)
    bool endEarly = true;           // XRT_END_EARLY=0: every generation-0 path leaves its records and k_compose colours it (kernels.h EndArgs off)
    int packetCullMin = 4;     // XRT_PK_CULL_MIN (development): leaves with fewer references skip the tight-box test
    // Split walks (packet.hip): one-body scenes; a packet / an item that has walked for this many microseconds looks for pending subtrees to hand to other waves
    // (XRT_PK_SPLIT=0: off; XRT_PK_BUDGET / XRT_PK_BUDGET_ITEM in microseconds, XRT_PK_BUDGET=0: a walk looks for pending subtrees at every block it enters;
    // XRT_PK_SPLIT_ITEMS: capacity of a frame context's arena)
    bool packetSplit = false;   // (measured: no gain yet -- profiles/r04/split_walks.txt; XRT_PK_SPLIT=1 switches the split-walk variant of the packet kernel on)
    int packetBudgetUs = 350, packetBudgetItemUs = 150, packetSplitItems = 8192;
    int packetLongUs = 0, packetBudgetLongUs = 8;    // XRT_PK_LONG / XRT_PK_BUDGET_LONG (block entries, whatever the names say): a packet that made more than the first in the context's last frame hands subtrees over every <second> block entries from the start (XRT_PK_LONG=0: no prediction)
    int packetGrabMax = 2;     // XRT_PK_GRAB (development): 8 -> 2 shortened the tail of a launch (C5 blocking 9.0 -> 7.8 ms); 1 loses to contention on the queue word
    int packetStaticDiv = 4;   // XRT_PK_STATIC (development): 1/2 .. 1/8 measured within 2 % of each other on C5
    bool packetQuads = true;   // XRT_PK_QUADS=0: a primary packet is 64 consecutive live rays, as before the packet table (kernels.h QuadTable; scheduling only: the A/B, bisecting)
    bool packetScreen = true;  // XRT_PK_SCREEN=0: the primary packets of a one-body scene's camera frames test every triangle of a run, as before the table of screen boxes (screen_rects.h; work avoided only: the A/B, tests)
    bool levelMap = true;      // XRT_LEVEL_MAP=0: level records for every path of the frame (as before round 4's last build)
    int nodeCull = 1;          // XRT_NODE_CULL: SceneView::nodeCull (tools: a scheduling-free switch, results never change)
    bool noSingle = false;     // XRT_NO_SINGLE: a scene of one SceneObject with one Mesh is still traced as a two-level scene
    int longFracLo = 2, longFracHi = 6;   // percent of a generation's rays the list is steered to (XRT_LONG_FRAC=lo,hi)
    std::optional<float> heavy;   // XRT_HEAVY=<fraction of the box diagonal>: the long-ray estimate in any scene (unset: 0.25, one-body scenes only; xrt_scene::heavyPath)
    long long heapRayCap = HEAP_RAY_CAP;         // XRT_HEAP_RAY_CAP=<n> forces small ray buffers (tests of the overflow / retry path)
    long long shadowBytes = 8LL << 30;   // budget of a frame context's shadow rays / hits / words (XRT_SHADOW_BYTES): many lights shrink the chunk
    long long maxChunkPaths = MAX_CHUNK_PATHS;   // XRT_CHUNK_PATHS=<n> (multiple of 8192) forces smaller chunks (tests of the multi-chunk path)
    long long pixelBytes = 4LL << 30;   // XRT_PIXEL_BYTES=<n>: byte budget of one chunk of an xrt_render_pixels list (pixels_plan.h; tests of the split)
    float overlapMinMs = 0.05f;  // frames at least this long run on per-context streams (XRT_OVERLAP_MS=0: every single-chunk frame gets its context's stream)
    // A launch of persistent waves leaves the machine half empty while its last rays finish; a blocking single frame (what the
    // C# host's RenderInternal asks for) has no other frame to fill the gaps, so it is rendered as two halves of its tiles on
    // two streams.  XRT_SPLIT=0 never, 1 frames nobody else overlaps (default), 2 also pipelined frames.  It paid while a launch's
    // waves were alive 55-60 % of its duration (C4 13.3 -> 10.9 ms), did not in rounds 2 and 3 (the second set of launches cost what the
    // overlap gained: C3 2.74 vs 2.91 ms, C4 7.1 vs 6.9, C5 7.9 vs 8.0), and pays again now that the kernels are faster and a launch's tail
    // is a larger share of it (round 4, one box: C3 1.95 -> 1.72 ms per blocking frame, C4 4.26 -> 4.13, C5 4.48 -> 4.43; three or four
    // bands no better; profiles/r04/frame_split.txt).  By default only two-level scenes: the two extra frame contexts cost a one-body scene like C5
    // 6 GB of work buffers for 1 %.
    std::optional<int> splitMode;   // unset: 1, and only two-level scenes are split (a one-body scene gains 1-2 % for two more frame contexts' work buffers)
    int splitParts = 2;             // XRT_SPLIT_PARTS
    float splitMinMs = 1.0f;        // XRT_SPLIT_MS: frames shorter than this are not split
    bool launchEvents = false;   // XRT_LAUNCH_EVENTS=1: single-chunk frames time their traversal launches with events on the dispatch packets, too
    int maxStampRows = MAX_STAMP_ROWS;   // XRT_STAMP_ROWS=<n> (tests): launches of a frame beyond the n-th carry events instead
    bool adaptiveFast = true;    // adaptive frames are enqueued whole (level buffers sized optimistically) until a level overflows; XRT_ADAPTIVE_FAST=0
    long long adaptiveCap = 0;   // XRT_ADAPTIVE_CAP=<quadrants> (tests): capacity of the deeper levels instead of one quadrant per pixel
    bool heapFast = true;        // single-chunk ray-tree frames go the optimistic way (no host round trip) until one overflows; XRT_HEAP_FAST=0
    bool gridHints = true;       // XRT_GRID_HINTS=0: every launch is sized for the whole chip
    // Threads per block of k_shade over a big generation (XRT_SHADE_BLOCK=<256 .. 1024, a multiple of 64>; scheduling only).  The kernel is compiled for 24 waves
    // per CU and its 16 waves of a 1024-thread block move in lockstep from barrier to barrier, so a CU held one block and waited with it.  Two blocks of 768:
    // k_shade #0 of C5 485 -> 426 us, the pipelined frame 2.962 -> 2.907 ms; three of 512 the same on C5 but C4 +0.03 ms (profiles/shade_blocks).
    int shadeBlock = 768;
    bool launchTiming = true;    // XRT_LAUNCH_TIMING=0: single-chunk frames do not time their traversal launches (xrt_stats.ms_intersect = 0)
    std::string waveTimesPath;   // XRT_WAVE_TIMES=<file>: per-wave clocks of the last frame's launches (development aid, make WAVE_TIMES=1)
    std::string stampDumpPath;   // XRT_STAMP_DUMP=<file>: the stamp rows of the last frame (start, waves, every wave's end) -- how long a launch's waves lived
    bool fakeGpus = false;   // XRT_FAKE_GPUS=1 (test boxes with one GPU): the replicas live on the scene's own device and the exchange is RCCL send-to-self
    bool noRectCull = false, oneStream = false, noFeedback = false;   // XRT_NO_RECT_CULL, XRT_ONE_STREAM, XRT_NO_FEEDBACK (development)
    std::optional<bool> spatialRuns;   // XRT_LEAF_ORDER=0: the references of big leaves in list order (HostScene::spatialRuns; tools: A/B of the storage order, results never change)
#ifdef XRT_DEV   // (make DEV=1) the two margin factors are the only switches that can change a result: below their proven values the skips
                 // are no longer exact.  A shipped library does not read them from the environment of its host process.
    std::optional<double> leafCullSafety;   // XRT_LEAF_CULL: 0 = no tight leaf boxes, 1 = the proven margin (HostScene::leafCullSafety)
    std::optional<double> cullSafety;       // XRT_CULL_SAFETY: factor S of the object pre-cull margin (below 2 the bound is no longer proven)
    bool finishCounts = false;              // XRT_FINISH_COUNTS=1: every single-pass frame prints its generations' hits and how many of them part A finished
#endif
    std::optional<bool> guard;   // XRT_GUARD: process-wide (g_guardMode); unset leaves the mode as it is
};

// One line per switch: an integer (atoi, or atoll for the 64-bit members) in [lo, hi] and a multiple of `step`; a flag (atoi != 0); a
// number (atof); a string; "is it set at all".
template <class T>   // int, std::optional<int> or long long
void env_int(const char *name, T &out, long long lo, long long hi, long long step = 1) {
    const char *e = getenv(name);
    if (!e) return;
    const long long v = std::is_same<T, long long>::value ? atoll(e) : atoi(e);
    if (v >= lo && v <= hi && v % step == 0) out = T(v);
}
template <class T>   // bool or std::optional<bool>
void env_flag(const char *name, T &out) { if (const char *e = getenv(name)) out = atoi(e) != 0; }
template <class T>   // float or std::optional<float>
void env_float(const char *name, T &out) { if (const char *e = getenv(name)) out = (float)atof(e); }
inline void env_str(const char *name, std::string &out) { if (const char *e = getenv(name)) out = e; }
inline bool env_set(const char *name) { return getenv(name) != nullptr; }

// The only reader of the per-scene switches (xrt_scene_create).
inline Settings read_settings() {
    Settings c;
    env_int("XRT_PACKET", c.packetMask, -1, 31);
    env_int("XRT_PACKET_HEAP", c.packetMaskHeap, -1, 31);
    env_int("XRT_BATCH_MAX", c.batchMax, 16, 4096, 16);
    env_int("XRT_BATCH_MIN", c.batchMin, 16, 64, 16);
    env_int("XRT_SPREAD_MIN", c.spreadMin, 4, 64, 4);
    if (const char *t = getenv("XRT_TUNE")) {   // scheduling only, never results
        int v[4] = {0, 0, 0, c.tune[3]};
        if (sscanf(t, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) >= 3 && v[0] >= 1 && v[0] <= 64 && v[1] >= 1 && v[2] >= 1 && v[3] >= 0 && v[3] <= 64)
            for (int i = 0; i < 4; i++) c.tune[i] = v[i];
    }
    env_int("XRT_HEAVY_SHIFT", c.heavyShift, 0, 6);
    env_int("XRT_FIRST_BATCH", c.firstBatch, 64, 4096, 64);
    env_flag("XRT_PK_MERGE", c.packetMerge);
    env_flag("XRT_AE", c.answerAtEmission);
    env_flag("XRT_AE_FINISH", c.finishInPartA);
    env_flag("XRT_END_EARLY", c.endEarly);
    env_int("XRT_PK_CULL_MIN", c.packetCullMin, INT_MIN, INT_MAX);
    env_flag("XRT_PK_SPLIT", c.packetSplit);
    env_int("XRT_PK_BUDGET", c.packetBudgetUs, 0, 1000000);
    env_int("XRT_PK_BUDGET_ITEM", c.packetBudgetItemUs, 0, 1000000);
    env_int("XRT_PK_SPLIT_ITEMS", c.packetSplitItems, 1, 1 << 20);
    env_int("XRT_PK_LONG", c.packetLongUs, 0, 1000000);
    env_int("XRT_PK_BUDGET_LONG", c.packetBudgetLongUs, 0, 1000000);
    env_int("XRT_PK_GRAB", c.packetGrabMax, 1, 64);
    env_int("XRT_PK_STATIC", c.packetStaticDiv, 0, 64);
    env_flag("XRT_PK_QUADS", c.packetQuads);
    env_flag("XRT_PK_SCREEN", c.packetScreen);
    env_flag("XRT_LEVEL_MAP", c.levelMap);
    env_int("XRT_NODE_CULL", c.nodeCull, 0, 2);
    c.noSingle = env_set("XRT_NO_SINGLE");
    if (const char *e = getenv("XRT_LONG_FRAC")) { int lo = 0, hi = 0; if (sscanf(e, "%d,%d", &lo, &hi) == 2 && lo >= 0 && hi > lo && hi <= 100) { c.longFracLo = lo; c.longFracHi = hi; } }
    env_float("XRT_HEAVY", c.heavy);
    env_int("XRT_HEAP_RAY_CAP", c.heapRayCap, 1024, HEAP_RAY_CAP);
    env_int("XRT_SHADOW_BYTES", c.shadowBytes, 1LL << 20, LLONG_MAX);
    env_int("XRT_CHUNK_PATHS", c.maxChunkPaths, 8192, MAX_CHUNK_PATHS, 8192);
    env_int("XRT_PIXEL_BYTES", c.pixelBytes, 1, LLONG_MAX);
    env_float("XRT_OVERLAP_MS", c.overlapMinMs);
    env_int("XRT_SPLIT", c.splitMode, 0, 2);
    env_int("XRT_SPLIT_PARTS", c.splitParts, 2, 4);
    env_float("XRT_SPLIT_MS", c.splitMinMs);
    env_flag("XRT_LAUNCH_EVENTS", c.launchEvents);
    env_int("XRT_STAMP_ROWS", c.maxStampRows, 0, MAX_STAMP_ROWS);
    env_flag("XRT_ADAPTIVE_FAST", c.adaptiveFast);
    env_int("XRT_ADAPTIVE_CAP", c.adaptiveCap, 1, LLONG_MAX);
    env_flag("XRT_HEAP_FAST", c.heapFast);
    env_flag("XRT_GRID_HINTS", c.gridHints);
    env_int("XRT_SHADE_BLOCK", c.shadeBlock, 256, 1024, 64);
    env_flag("XRT_LAUNCH_TIMING", c.launchTiming);
    env_str("XRT_WAVE_TIMES", c.waveTimesPath);
    env_str("XRT_STAMP_DUMP", c.stampDumpPath);
    c.fakeGpus = env_set("XRT_FAKE_GPUS");
    c.noRectCull = env_set("XRT_NO_RECT_CULL"); c.oneStream = env_set("XRT_ONE_STREAM"); c.noFeedback = env_set("XRT_NO_FEEDBACK");
    env_flag("XRT_LEAF_ORDER", c.spatialRuns);
#ifdef XRT_DEV
    if (const char *e = getenv("XRT_LEAF_CULL")) { const double v = atof(e); if (v >= 0.0 && v <= 1e6) c.leafCullSafety = v; }
    if (const char *e = getenv("XRT_CULL_SAFETY")) { const double v = atof(e); if (v >= 0.0 && v <= 1e6) c.cullSafety = v; }
    env_flag("XRT_FINISH_COUNTS", c.finishCounts);
#endif
    env_flag("XRT_GUARD", c.guard);
    return c;
}

}  // namespace xrt
