// scene_state.h — what an xrt_scene is between two calls of include/xrt.h: the host scene, its HBM-resident arrays, the pose versions, the
// work buffers and host state of the frames in flight, the replicas of an n_gpus > 1 render.  Every device resource in here is a member of an
// owner type of device_res.h and is freed by that member's destructor (DESIGN.md "Ownership"); nothing in here decides what a frame launches.
// Included by xrt_api.cpp, the one translation unit that defines the opaque struct of include/xrt.h, behind its `using namespace xrt`.
#pragma once
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <thread>

#include "device_res.h"   // (and <atomic>, <mutex>, <string>, <unordered_map>, <vector>)
#include "frame_plan.h"
#include "kernels.h"
#include "paths.h"
#include "rccl_gather.h"
#include "scene_host.h"
#include "settings.h"

// One host thread per replica device (in-library multi-GPU, xrt_render_opts.n_gpus), created with the replica and parked on a
// condition variable between frames: it has made its device current once and enqueues that device's share of every frame.
// (Round 2 spawned and joined n-1 std::threads per frame: tens of microseconds of host time on a 0.75 ms frame.)
struct RankWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool posted = false, finished = false, quit = false;
    explicit RankWorker(int device) {
        th = std::thread([this, device] {
            (void)hipSetDevice(device);
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                cv.wait(lk, [this] { return posted || quit; });
                if (quit) return;
                posted = false;
                lk.unlock();
                job();
                lk.lock();
                finished = true;
                cv.notify_all();
            }
        });
    }
    void post(std::function<void()> f) {
        { std::lock_guard<std::mutex> lk(m); job = std::move(f); finished = false; posted = true; }
        cv.notify_all();
    }
    void wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [this] { return finished; }); }
    ~RankWorker() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};

struct xrt_scene {
    int device = -1;   // -1: host-only scene (inspection of the built trees; every compute call fails)
    HostScene hs;
    const HostScene *host = &hs;   // what the frame code reads; a replica on another device points at its primary's
    // Declared in front of every stream: members are destroyed in reverse order, so the scene's streams go before the communicators (as they always did).
    RcclGather rccl;
    // HBM-resident scene
    DevBuf<f4> blocks, refN, snodes, shade, leafNB, leafTB, scull, runTB;
    DevBuf<float> refT, pblocks, lrec;
    DevBuf<g3> refG;
    DevBuf<int> childDfs, srefs, objMesh, runBase;
    DevBuf<MeshRec> meshes;
    DevBuf<ObjRec> objects;
    DevBuf<MaterialRec> materials;
    DevBuf<uint32_t> texels;
    SceneView view{};
    // Pose versions (xrt_scene_set_poses): a frame reads the ObjRecs and pre-cull records of ONE version, the one that was current at its
    // begin (FrameCtx::pose).  Version 0 is `objects` / `scull`, versions 1 and 2 are made when a pose update must not overwrite a version
    // an open ticket reads: with at most two tickets open one of the three is always free, so an update never waits for a frame.
    struct PoseVer {
        DevBuf<ObjRec> objects;   // (version 0: the scene's own `objects` / `scull`)
        DevBuf<f4> scull;
        Event ready;                       // recorded behind the version's last write; null while it holds the build's records
        unsigned long long serial = 0;     // which write it holds (a replica copies the primary's version when the serials differ)
        std::vector<std::pair<hipStream_t, Event>> readers;   // the last asynchronous seam-1 read on each stream (xrt_scene_intersect_device)
    } pose[3];
    int poseCur = 0;                       // the version new frames and seam-1 calls read
    int slotPose[2] = {-1, -1};            // the version of the open ticket `slot`
    unsigned long long poseSerial = 0;     // writes since the build
    bool posesOnDevice = false;            // hs's poses are behind: the last update came from device arrays (xrt_scene_set_poses_device)
    Stream poseStream;                     // pose updates run here
    Event poseInput;                       // the caller's stream -> poseStream
    DevBuf<int> scullPosStart, scullPos;   // HostScene scullPosStart / scullPos
    DevBuf<float> wbbDev;                  // WorldBoundingBox of every body, 6 floats (kept by k_pose for the read-back)
    DevBuf<float> poseIn;                  // the host form's arrays on the device: ids | world | inv | wbb
    Pinned<void> posePinned;               // ... and their page-locked staging
    Event poseStaged;                      // the staging copy is done (the staging may be refilled)
    // Material versions (xrt_scene_set_materials), as the pose versions: a frame reads the MaterialRec table and the texel arena of ONE version,
    // the one that was current at its begin (FrameCtx::mat), and takes the plain or the ray-tree pipeline by THAT version's anyTransparent.
    // Version 0 is `materials` / `texels`; versions 1 and 2 are made when an update must not overwrite what an open ticket reads.  Every
    // version holds a whole arena (DESIGN.md "Material versions": at most three copies of every texture).  An update only STAGES what the
    // version lacks, in page-locked memory of the version's own; the copies to the device are enqueued by the first frame or ray batch that
    // reads the version, on ITS stream ahead of its kernels (mat_acquire): an update has no stream and no dispatch of its own that would have
    // to find room among the persistent waves of the frames in flight (profiles/materials).
    struct MatVer {
        DevBuf<MaterialRec> materials;   // (version 0: the scene's own `materials` / `texels`)
        DevBuf<uint32_t> texels;
        Pinned<void> staging;              // MaterialRecs | texels [stagedLo, stagedHi) of the newest write, until its copies have run
        bool pending = false;              // staged, the copies not enqueued yet
        size_t stagedRecBytes = 0, stagedMat = 0, stagedLo = 0, stagedHi = 0;
        hipStream_t owner = nullptr;       // the stream the copies were enqueued on (work on it is behind them anyway) ...
        Event ready;                       // ... and the event recorded behind them there, for readers on other streams; null while it holds the build's records
        unsigned long long serial = 0;     // which write it holds (a replica copies the primary's version when the serials differ)
        bool anyTransparent = false;       // SceneArrays::anyTransparent of the materials it holds
        size_t texCount = 0;               // words of its arena
        bool texFull = false;              // its arena is behind the host's as a whole (never written, or the host's was packed again) ...
        size_t texLo = 0, texHi = 0;       // ... or in these words only
    } mat[3];
    int matCur = 0;                        // the version new frames and ray batches read
    int slotMat[2] = {-1, -1};             // the version of the open ticket `slot`
    unsigned long long matSerial = 0;      // writes since the build
    Stream matStream;                      // (n_gpus > 1: the primary's copies run here when its replicas need the version before its own frame is enqueued)
    std::vector<DevBuf<uint32_t>> matRetired;   // arenas that were outgrown while a ticket was open: freed when none is (hipFree waits for the device)
    // Triangle-shading versions (xrt_scene_set_triangle_shading), as the pose versions: a frame reads the `shade` array of ONE version, the one
    // that was current at its begin (FrameCtx::shade).  Version 0 is `shade`; versions 1 and 2 are allocated when an update must not
    // overwrite what an open ticket reads, and are brought up to date from the current version by a device-to-device copy first.  Every
    // write runs on shadeStream, so the writes of all versions are ordered among themselves; readers wait for the version's event.
    struct ShadeVer {
        DevBuf<f4> shade;                  // (version 0: the scene's own `shade`)
        Event ready;                       // recorded behind the version's last write; null while it holds the upload's records
        unsigned long long serial = 0;     // which write it holds (a replica copies the primary's version when the serials differ)
    } shadeVer[3];
    int shadeCur = 0;                      // the version new frames and ray batches read
    int slotShade[2] = {-1, -1};           // the version of the open ticket `slot`
    unsigned long long shadeSerial = 0;    // writes since `shade` was uploaded
    size_t shadeCount = 0;                 // records of every version: the size `shade` was uploaded with
    bool shadeOnDevice = false;            // hs's n / uv / color are behind: an update came from device arrays (xrt_scene_set_triangle_shading_device)
    Stream shadeStream;                    // the updates run here
    Event shadeInput;                      // the caller's stream -> shadeStream
    DevBuf<uint32_t> shadeIn;              // the host form's arrays on the device: ids | normals | uv | color, each part 16-byte aligned
    Pinned<void> shadePinned;              // ... and their page-locked staging
    Event shadeStaged;                     // the staging copy is done (the staging may be refilled)
    bool resident = false;
    int numCUs = 256;
    int stackNeeded = 2;
    int blocksPerCU = 1, blocksPerCUMesh = 1, blocksPerCUPacket = 1;
    bool packetOk = false;   // the scene's rays can take the wave-packet kernel (one body, one mesh with a real octree)
    Settings cfg;   // the environment switches (settings.h): set once by xrt_scene_create (a replica's by ensure_replicas)
    // Knobs of k_intersect that scene_upload derives from the scene where cfg does not name them (refill threshold: see there)
    int refillMin = 24;
    int heavyShift = 3;        // listed long rays are dealt one in 2^n work items (0: 64 to a wave); scene_upload: 0 for two-level scenes; XRT_HEAVY_SHIFT
    int firstBatch = 64;
    // Sizes of the last finished single-chunk frame's generations (rays of traversal step k, work items of shade step k): the
    // launches of the next frame of the same geometry are sized for four times that instead of for the whole chip -- a generation
    // of a few thousand rays costs its kernels' launch floor (5-6 us each with full grids, C2: 0.119 -> 0.11 ms).  Sizing only.
    long long genKey = -1, genRays[68], genShade[68];
    bool genHeap = false;        // ... made by a ray-tree frame (a frame of the other pipeline takes no hints from them: the counter words mean other things)
    long long genCompose = -1;   // ... and the length of its compose list (kernels.h EndArgs; -1: the frame had none)
    unsigned long long endCounts[3] = {0, 0, 0};   // xrt_debug_end_counts: the last finished frame's paths coloured by k_raygen, by k_shade, and on the compose list
    int quadCtx = -1; unsigned long long quadLive = 0;   // xrt_debug_packet_table: the frame context of the last finished frame if it had one chunk and a packet table (-1: none), its live primary rays
    int lvlCheckedTilesX = 0; long long lvlCheckedTiles = 0;   // (LvlMap::inv verified for this frame geometry)
    unsigned splitSerial = 0;
    std::map<int, std::pair<DevBuf<unsigned>, DevBuf<unsigned>>> apiSplit;   // seam 1 (testing aid, XRT_PACKET & 8): an arena per stream
    int sceneMode = MODE_SCENE;   // MODE_SINGLE when the scene is one SceneObject with one Mesh
    Stream stream;
    // per-frame work buffers
    DevBuf<xrt_ray> apiRays;
    DevBuf<xrt_hit> apiHits;
    DevBuf<xrt_ray> castRays;     // xrt_cast_rays: the host's rays and their colours
    DevBuf<uint32_t> castRGBA;
    DevBuf<float> castF32;
    DevBuf<xrt_hit> castHits;     // xrt_shade_hits: the host's hits (its rays and colours go through castRays / castRGBA / castF32)
    // xrt_light_hits (lights.hip): the work set of one chunk -- the compact shadow-ray list with its scatter words, the pairs' hits and hit / miss
    // words, the two count words, the queue words of its traversal launch, the lights -- and the host form's outputs on the device (its hits go
    // through castHits).  Allocated at the first call, freed with the scene; the work set of frames (WorkBufs) is not touched.
    struct LightWork {
        DevBuf<xrt_ray> rays;
        DevBuf<xrt_hit> hits;
        DevBuf<int> flags, scatter, counts;
        DevBuf<unsigned> queue, splitItems, splitRecs;
        DevBuf<LightRec> lights;
        DevBuf<float> lightOut, amountOut;
        Event ev[4];   // a chunk's start and end, its traversal launch's start and end
    } lightWork;
    // xrt_surface_hits (surface.hip): the counter word of a call, and the host form's outputs on the device (its rays and hits go through
    // castRays / castHits).  Allocated at the first call, freed with the scene; the device form allocates nothing else.
    struct SurfaceWork {
        DevBuf<unsigned long long> count;
        DevBuf<xrt_surface> surfaceOut;
        DevBuf<xrt_ray> reflectOut, refractOut;
        Event ev[2];   // the call's start and end
    } surfaceWork;
    // xrt_compose_hits / xrt_fold_samples (compose.hip; the fold is k_pixel_resolve of pixels.hip): the counter word of a call, and the host
    // forms' inputs and outputs on the device.  Allocated at the first call, freed with the scene; the device forms allocate nothing else.
    struct ComposeWork {
        DevBuf<unsigned long long> count;
        DevBuf<xrt_surface> surfaceIn;
        DevBuf<float> lightIn, f32Out;
        DevBuf<uint32_t> reflectIn, refractIn, samplesIn, rgbaOut;
        Event ev[2];   // the call's start and end
    } composeWork;
    // xrt_trace_pixels (trace.hip): the work set of one chunk -- the work rays (the compact live list of a hinted chunk; the whole list where the caller
    // wants no rays), the whole list again where a hinted call without a ray output counts the reference's work, the count words (live rays, hits), the
    // queue words of its traversal launch -- and the host form's centres and outputs on the device.  The index list and the packet table of a hinted
    // chunk are frame context 0's (WorkBufs::index0 / quadTable: where xrt_debug_packet_table looks; no frame is in flight during the call).
    // Allocated at the first call, freed with the scene.
    struct TraceWork {
        DevBuf<xrt_ray> rays, countRays, raysOut;
        DevBuf<xrt_hit> hitsOut;
        DevBuf<float> centers;
        DevBuf<int> counts;
        DevBuf<unsigned> queue, splitItems, splitRecs;
        Event ev[4];   // a chunk's start and end, its traversal launch's start and end
    } traceWork;
    // xrt_cast_rays_paths (paths.hip): staging records of a chunk -- (hit position, tag) and (refraction direction, tag) per (node, path), allocated
    // only when a paths call is made --, the work arrays of the ordering pass, and the host form's copies of the caller's arrays
    DevBuf<f4> pathHit, pathDir;
    DevBuf<int> pathLocal, pathBlockSum;
    DevBuf<long long> pathBlockBase, pathStart;
    DevBuf<xrt_path_vertex> pathVerts;
    DevBuf<xrt_ray> pathBack;
    unsigned pathEpoch = 0;            // number of the last attempt of a chunk (the tag of its records; 0 is "never written")
    Pinned<long long> pathPinned;      // the batch's vertex count on its way to the host
    // xrt_render_pixels (pixels.hip): the rays and the sample colours of one chunk of the centre list, and the host form's copy of the centres
    // (its colours come back through castRGBA / castF32); the quadrant levels of an adaptive call are the call's own and freed when it returns
    DevBuf<xrt_ray> pixelRays;
    DevBuf<uint32_t> pixelSamples;
    DevBuf<float> pixelCenters;
    DevBuf<unsigned> queues;
    DevBuf<uint32_t> outRGBA;
    DevBuf<float> outF32;
    DevBuf<unsigned long long> counters;
    // Work buffers of one frame in flight.  Two sets (FrameCtx) so that two frames on two streams can overlap: a launch
    // of persistent waves leaves the machine half empty while its last rays finish, and the other frame's launches fill it.
    struct WorkBufs {
        DevBuf<xrt_ray> rays0, rays1, shadowRays;
        DevBuf<xrt_hit> hits, shadowHits;
        DevBuf<int> path0, path1, index0, heavyList, cnts;
        DevBuf<int> composeList;                // kernels.h EndArgs: [0 .. END_WORDS) the count words, [16 ..] the paths k_compose has to walk
        DevBuf<unsigned> quadTable;             // kernels.h QuadTable: the two count words at [0] and [64] (QUAD_HEAD_WORDS in all), then two words per entry
        DevBuf<uint2> scrTable, pkRect;         // screen_rects.h: the frame's screen box per leaf reference (FramePlan::scrRefs), the screen rectangle per entry of quadTable
        int quadWord = 0;                       // ... the count word (0 / 1) the context's last chunk with a table counted into
        DevBuf<int> node0, node1, heapFlag;     // ray-tree frames: heap node of every ray; heapFlag[0]: a generation overflowed its buffers
        DevBuf<float> ref0, ref1, lvlAlpha;     // ... refraction index of the medium a ray travels in; alpha per level record
        DevBuf<int> hitFlags0, shadowFlags;   // hit / miss word per ray of hits, shadowHits (a miss has no record)
        DevBuf<unsigned> splitCost;               // ... what every packet of every packet launch of the context's last plain frame cost (PacketArgs::splitCost)
        size_t splitCostStride = 0;               // (packets a launch may have; a frame of another size starts the memory afresh)
        DevBuf<unsigned> splitItems, splitRecs;   // split walks (kernels.h PacketArgs::splitItems): the arena of this context's packet launches (they run one after the other)
        DevBuf<int> shadowOut;                // ShadeArgs::ae: where the answer of the i-th emitted shadow ray goes (slot * lights + light)
        DevBuf<int> shadowFlags1;             // ShadeArgs::ae: part A of step k answers some shadow queries of generation k ITSELF while part B of the same launch still reads
                                              // generation k-1's words: the generations alternate between shadowFlags and this
        DevBuf<unsigned long long> stamps;      // device-clock stamps of the traversal launches (device_util.h), STAMP_STRIDE per launch
        DevBuf<SlotRec> slot0, slot1;
        DevBuf<int> slotNode0, slotNode1;   // ray-tree frames: the node of a slot's hit
        DevBuf<f4> lvlA, lvlB;
        DevBuf<uint32_t> sampleColor;
        DevBuf<float> sampleF32;
        DevBuf<LightRec> lights;
        // adaptive supersampling in flight (RT:170-311 without host round trips): the quadrant levels' buffers belong to the frame context
        struct Level { DevBuf<uint32_t> color; DevBuf<int> childBase, childMask; DevBuf<float> cx, cy; } levels[8];
        bool levelWordsClean = false;           // the level-count words at the head of cnts are zero (k_resolve cleared them)
        bool heapFlagClean = false;
        bool cntsClean = false;                 // cnts is all zero (the previous frame's epilogue cleared what it counted)
        std::vector<LightRec> lightsOnDevice;   // what `lights` holds
        const void *lightsDevPtr = nullptr;
        Stream stream;                          // the context's own stream (used when the caller passes none)
        hipStream_t lastStream = nullptr;       // the stream the context's last frame ran on
    };
    // cost feedback (kernels.hip long_ray): per path and generation, what the ray cost in the last frames
    DevBuf<unsigned> costMap;
    size_t costMapPaths = 0;
    unsigned epoch = 100;
    int costT[66];            // per generation: rays that cost more than this are started first; steered in frame_finish
    bool deepMeshes = false;  // some mesh has a real octree: rays can be long
    float heavyPath = 0.0f;   // rays longer than this inside the root box are traced first (0: off; cfg.heavy)
    DevBuf<unsigned long long> waveTimes;   // cfg.waveTimesPath
    // Per-frame host state.  Two contexts so that the next frame can be enqueued while the previous one's counters
    // and timings are still on their way back (xrt_render_device_begin / _end).
    struct FrameCtx {
        std::vector<Event> events;
        Pinned<int> pinned;          // host staging for the counter read-back (mapped: k_compose hands the counters over through .dev)
        std::vector<std::pair<size_t, size_t>> pairs;   // (start, stop) event indices of the k_intersect launches
        size_t ev = 0;
        Event done;                  // recorded after the frame's last copy
        std::vector<LightRec> hostLights;
        int pose = 0;                // the pose version the frame reads (xrt_scene::pose)
        int mat = 0;                 // the material version the frame reads (xrt_scene::mat)
        int shade = 0;               // the triangle-shading version the frame reads (xrt_scene::shadeVer)
        bool pending = false;
        FramePlan plan;              // what frame_begin decided about the frame in flight (frame_plan.h): frame_finish and the ticket code read it
        bool redone = false;         // a frame that overflowed on the optimistic way and was rendered again
        xrt_camera redoCam; xrt_render_opts redoOpts; std::vector<xrt_light> redoLights;   // what a redo needs
        uint32_t *redoOut = nullptr; float *redoOutF32 = nullptr; hipStream_t redoSt = nullptr;
        int stampRows = 0;           // traversal launches of the frame that timed themselves (device_util.h)
        Pinned<unsigned long long> stampHost;   // their (start, end) clock pairs: mapped pinned memory and its device view
        // deferred accounting
        int tallyChunks = 0;         // chunks whose counters frame_finish tallies from `pinned` (plan.cntBase words in, plan.cntStride apart)
        unsigned long long answered = 0;   // rays answered at emission (plan.ae): they are not in the ray lists
        unsigned long long shaded = 0, closestDeep = 0, livePaths = 0, live0 = 0, validPixels = 0;
        unsigned long long hcnt[2 * C_COUNT] = {0};
        WorkBufs w;
    } frames[8];   // context of ticket `slot`, part j of its frame: frames[slot + 2 * j] (a frame may be split into up to four bands on as many streams)
    std::vector<Event> events;   // xrt_scene_intersect timing
    float lastFrameMs = 0.0f;    // GPU time of the last finished frame
    bool adaptiveFastOk = true;  // no adaptive frame has overflowed its optimistically sized level buffers (cfg.adaptiveFast)
    bool heapFastOk = true;      // no single-chunk ray-tree frame has overflowed on the optimistic way (cfg.heapFast)
    int wallClockKHz = 0;        // rate of the device clock the launches stamp (hipDeviceAttributeWallClockRate)
    std::atomic<bool> busy{false};
    std::atomic<float> progress{0.0f};
    // Seam 1 (xrt_scene_intersect / xrt_mesh_intersect / xrt_generate_primary_rays) is re-entrant like the reference's
    // ISpatialManager.GetRayIntersection (ISM:15, called from N render threads, RT:105-113): the host-buffer calls share
    // one staging area and are serialised by this mutex; every stream has its own work-queue word.
    // In-library multi-GPU (xrt_render_opts.n_gpus): copies of the scene on devices device+1 .. (owned), the RCCL
    // communicators, and per ticket the buffer the tile shards are gathered into (cfg.fakeGpus: all on the scene's own device).
    std::vector<std::unique_ptr<xrt_scene>> replicas;
    std::vector<std::unique_ptr<RankWorker>> workers;   // workers[i - 1] drives replica i
    int visibleDevices = 0;                             // hipGetDeviceCount at xrt_scene_create
    DevBuf<uint32_t> gathered[2];    // primary: n * tiles_per_rank * 512 pixels, rank-major
    DevBuf<uint32_t> tileOut[2];     // replica: its tiles of the frame in slot 0 / 1
    DevBuf<uint32_t> frameOut[2];    // W*H frame of a host-output ticket
    Event tilesReady[2];   // replica (fake mode): its tiles are rendered
    Event tailDone[2];     // primary: gather + de-tile + host copy of the ticket are done
    // Cost-aware tile assignment (xrt.h xrt_scene_set_tile_table / xrt_scene_tile_costs).  tileTable: the installed table (host copy and device
    // copy) for frames of tableW x tableH pixels with tableCount shards, tableTpr slots per rank; tileCost: ticks per LOCAL tile slot of the
    // frames rendered since the last reset, with the geometry they were rendered under (costKey) and their slots' tiles (costTiles).
    std::vector<int> tileTable;
    DevBuf<int> tileTableDev;
    int tableW = 0, tableH = 0, tableCount = 0, tableTpr = 0;
    DevBuf<unsigned> tileCost;
    std::vector<int> costTiles;      // tile of every local slot the cost words belong to
    int costW = 0, costH = 0;
    std::vector<float> balanceCost;  // n_gpus > 1 with balance_tiles: the last frame's costs by tile (all ranks summed), its size
    int balanceW = 0, balanceH = 0, balanceN = 0;
    struct OpenFrame { int nGpus = 0, nParts = 1; bool tail = false, balance = false; uint32_t *hostOut = nullptr, *devOut = nullptr; size_t px = 0; hipStream_t st0 = nullptr; } open[2];
    std::mutex apiMutex;
    std::unordered_map<hipStream_t, int> queueOfStream;

    // Joins the workers, destroys the replicas (each makes its own device current), makes this scene's device current; then the members free themselves.
    ~xrt_scene() {
        workers.clear();
        replicas.clear();
        if (device >= 0) (void)hipSetDevice(device);
    }
};

struct BusyGuard {
    xrt_scene *s;
    bool owned;
    explicit BusyGuard(xrt_scene *sc) : s(sc) {
        bool expected = false;
        owned = s->busy.compare_exchange_strong(expected, true);
    }
    ~BusyGuard() { if (owned) s->busy.store(false); }
};
