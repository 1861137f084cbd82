/*
 * xrt.h — C-ABI of libxrt, the MI355X (gfx950) ray / octree / triangle hot path that drops in
 * behind the xna-ray-trace C# host (P/Invoke), see INTEGRATION.md.
 *
 * Every entry point names the reference interface it replaces (file:line relative to the reference
 * repository; aliases: RT = RayTraceProject/RayTraceProject/RayTracer.cs,
 * OSM = RayTraceProject/RayTraceProject/Spatial/OctreeSpatialManager.cs,
 * ISM = .../Spatial/ISpatialManager.cs, SO = .../SceneObject.cs, MO = RayTracerTypeLibrary/MeshOctree.cs,
 * MESH = RayTracerTypeLibrary/Mesh.cs, MAT = RayTracerTypeLibrary/Material.cs,
 * TRI = RayTracerTypeLibrary/Triangle.cs, SPOT/DIR = .../SpotLight.cs / DirectionalLight.cs).
 *
 * Conventions
 *   - plain C, cdecl, POD structs with natural alignment, no C++ or torch types;
 *   - every function returns int: XRT_OK (0) or a negative XRT_E_* code; xrt_last_error() gives the
 *     thread-local message (precedent for the style: aviFileWrapper_src/Avi.cs:175-185 int HRESULTs);
 *   - all host arrays are borrowed for the duration of the call and copied; the library owns all
 *     device memory; handles are opaque;
 *   - matrices are XNA row-vector convention (v' = v * M), 16 floats M11,M12,...,M44.
 *   - there is NO CPU fallback: without a HIP device every compute entry point returns
 *     XRT_E_NO_DEVICE.
 */
#ifndef XRT_H
#define XRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XRT_VERSION 203

/* error codes (C# shim: BUSY -> InvalidOperationException (RT:26-27,62-63),
 * INVALID_ARG -> ArgumentException (SO:123-124, MAT:85,97)) */
#define XRT_OK              0
#define XRT_E_INVALID_ARG  -1
#define XRT_E_BUSY         -2
#define XRT_E_NO_DEVICE    -3
#define XRT_E_OOM          -4
#define XRT_E_HIP          -5
#define XRT_E_RCCL         -6
#define XRT_E_INTERNAL     -7
#define XRT_E_UNSUPPORTED  -8
#define XRT_E_NOT_BUILT    -9

/* enums mirror MAT:12-23 */
#define XRT_FILTER_POINT     0
#define XRT_FILTER_BILINEAR  1
#define XRT_ADDRESS_CLAMP    0
#define XRT_ADDRESS_WRAP     1
#define XRT_ADDRESS_MIRROR   2

#define XRT_LIGHT_SPOT         0   /* SPOT: IsPositionable == true  */
#define XRT_LIGHT_DIRECTIONAL  1   /* DIR:  IsPositionable == false */

/* multisampling modes of xrt_render_opts.use_multisampling */
#define XRT_MS_OFF       0   /* RT:103-126 RenderInternal                                       */
#define XRT_MS_ADAPTIVE  1   /* RT:128-168,170-311 RenderInternalWithMultisampling (faithful)   */
#define XRT_MS_FIXED16   2   /* the 16 level-1 positions of RT:218-305, mean of 4 means of 4    */

typedef struct xrt_scene xrt_scene;   /* replaces an OctreeSpatialManager + its SceneObjects (OSM:35, SO:12) */

/* Ray of one ISpatialManager.GetRayIntersection query (ISM:15): Ray{Position,Direction} + the
 * `ignoreTriangle` reference identity expressed as (mesh id, index in Mesh.Triangles[]) — instances
 * of one Model share Triangle objects, so the pair is instance independent (SO:126-127, MO:290).
 * ignore_tri < 0 means null. 32 bytes. */
typedef struct xrt_ray {
    float   o[3];
    float   d[3];
    int32_t ignore_mesh;
    int32_t ignore_tri;
} xrt_ray;

/* IntersectionResult (OSM:11-33) with object / mesh / triangle references turned into indices.
 * tri  = position in Mesh.Triangles[];
 * leaf = DFS pre-order index (root = 0, children in 4i+2j+k order, MO:210-222) of the MeshOctree
 *        leaf in which the winning strict-'<' test happened (MO:294);
 * d    = OBJECT-space distance (OSM:373,450); w = worldPosition (OSM:443). 48 bytes. */
typedef struct xrt_hit {
    int32_t hit;
    int32_t object;
    int32_t mesh;
    int32_t tri;
    int32_t leaf;
    float   u, v, d;
    float   wx, wy, wz;
    int32_t reserved;   /* not part of the answer: scheduling feedback (rounds of the traversal loop the ray was in flight) */
} xrt_hit;

/* Material (MAT:25-69, 234-268). tex_argb = the locked Format32bppArgb bitmap (MAT:65): row-major,
 * top-down, 0xAARRGGBB, tex_width*tex_height words; may be NULL when use_texture == 0.
 * tex_pargb = Material.Texture.ColorData, the Format32bppPArgb (premultiplied) copy RayTracerTexture makes of the same
 * file (TEX:24-33): the bilinear filter reads ITS words (MAT:186-189) while the point sampler reads tex_argb (MAT:150).
 * The host has both arrays; NULL means "same as tex_argb" (true for every image without an alpha channel). */
typedef struct xrt_material {
    float           reflectiveness;
    int32_t         transparent;
    float           refraction_index;
    int32_t         interpolate_normals;
    int32_t         use_texture;
    int32_t         tex_width;
    int32_t         tex_height;
    int32_t         reserved;
    const uint32_t *tex_argb;
    const uint32_t *tex_pargb;
} xrt_material;

/* Inputs of RayTracer.Render ray generation (RT:395-397): Camera.View, Camera.Projection and the
 * GraphicsDevice.Viewport. */
typedef struct xrt_camera {
    float   view[16];
    float   proj[16];
    int32_t vp_x, vp_y, vp_width, vp_height;
    float   vp_min_depth, vp_max_depth;
} xrt_camera;

/* ILight (ILight.cs:9-15) — SpotLight (SPOT:12-35) or DirectionalLight (DIR:10-20). */
typedef struct xrt_light {
    int32_t kind;
    float   position[3];
    float   direction[3];
    float   color[3];
    float   intensity;
    float   spot_angle;       /* SPOT:19-27, radians */
    float   decay_exponent;   /* SPOT:33, default 1.3f */
} xrt_light;

/* The RayTracer properties a frame reads (RT:19-41) + how the frame is spread over GPUs. */
typedef struct xrt_render_opts {
    int32_t max_reflections;      /* RT:33  */
    int32_t use_multisampling;    /* RT:40, XRT_MS_* */
    int32_t multisample_quality;  /* RT:41  */
    int32_t address_mode;         /* RT:37, XRT_ADDRESS_* */
    int32_t filtering;            /* RT:36, XRT_FILTER_*  */
    int32_t shard_rank;           /* one process per GPU: this process renders tiles t with t % shard_count == shard_rank */
    int32_t shard_count;          /* 0 or 1 = whole frame */
    int32_t collect_stats;        /* 1: also run the (untimed) reference-work counting pass */
    /* One process, several GPUs -- the drop-in for the C# host, whose RenderInternal is ONE call on ONE thread
     * (RT:103-126).  0 or 1: the scene's device only.  N > 1: the frame's 64x8 tiles are dealt round-robin to devices
     * d, d+1, .. d+N-1 (d = the scene's device; the scene is replicated on first use), every device renders its
     * tiles, one grouped RCCL send/recv over xGMI gathers the tile buffers on device d, a de-tile kernel writes the
     * W*H frame there.  Needs N visible devices (XRT_E_NO_DEVICE) and shard_count <= 1 (XRT_E_INVALID_ARG); an RCCL
     * failure is XRT_E_RCCL. */
    int32_t n_gpus;
    /* n_gpus > 1 only.  1: cost-aware tile assignment -- every frame leaves the cost of its tiles (xrt_scene_tile_costs), and the next
     * frame of the same size deals the tiles to the devices longest-first (xrt_balance_tiles) instead of round-robin: the reference's only
     * parallel idea is DYNAMIC row stealing (RT:48-52, 105-120), which a static t % N assignment does not reproduce where rows differ in
     * cost (the horizon).  0: round-robin.  Scheduling only: the frame is the same. */
    int32_t balance_tiles;
    /* XRT_LIST_*: what the caller says about the ORDER of a list -- the centres of xrt_render_pixels[_device], the rays of xrt_cast_rays[_device] and
     * xrt_cast_rays_paths[_device].  XRT_LIST_COHERENT: consecutive entries are neighbours on screen / in space (a row-major rectangle, a frame's tile
     * order, the primary rays of a frame), and the list is traced as a frame of the same scene and sampling would be: in every generation the kernel a
     * frame's rule picks -- the wave-packet kernel for the first rays of a two-level scene at any sample count, of a one-body scene with 16 samples --,
     * XRT_PACKET / XRT_PACKET_HEAP overriding as always; xrt_render_pixels then also generates its rays where it compacts them, one kernel instead of
     * two and no ray record for a position that cannot reach the scene.  Scheduling only, the hint never changes a result: rgba_out, rgb_f32_out, the
     * reference work counters, rays_*, hits_*, vertices and rays_back are bit for bit those of the unhinted call.  A hint on a scattered list costs time
     * and nothing else (a packet of scattered rays walks the union of their paths: 4096 random pixels of a two-level scene measured 16-18 % slower
     * hinted), and so can a hint on a list of a few entries (one 16-sample entry of a one-body scene: 0.20 against 0.19 ms; the hint follows the
     * frame's rule whatever the length; profiles/coherent_lists/README.md).  Any other value is XRT_E_INVALID_ARG in those calls.
     * xrt_shade_hits[_device] accept both values and do nothing with them (their first level is not traced); xrt_render* and every other call never read
     * the field.  Added within ABI 203: the first word of what was reserved[2], which callers were told to zero (= XRT_LIST_UNORDERED, the path as it
     * was, launch for launch); size and offsets of the struct are unchanged. */
    int32_t list_order;
    int32_t reserved;             /* zero */
} xrt_render_opts;
#define XRT_LIST_UNORDERED 0   /* as before: nothing is assumed about the order */
#define XRT_LIST_COHERENT  1   /* consecutive entries are neighbours on screen / in space */

/* Exact work counters of the REFERENCE algorithm for the rays of one call and the
 * measured kernel times. Counts are those of the C# code path, not of the pruned GPU traversal. */
typedef struct xrt_stats {
    uint64_t rays_closest;        /* CastRay queries, RT:512 */
    uint64_t rays_shadow;         /* IsLightPathObstructed queries, RT:485 */
    uint64_t hits_closest;
    uint64_t hits_shadow;
    uint64_t scene_node_tests;    /* OSM:460 slab tests */
    uint64_t instance_visits;     /* OSM:349-364 ray transforms */
    uint64_t mesh_aabb_tests;     /* MESH:37 */
    uint64_t mesh_queries;        /* MO:259 calls */
    uint64_t node_tests;          /* MO:331 slab tests */
    uint64_t leaf_refs;           /* MO:288 loop iterations in visited buckets */
    uint64_t tri_tests;           /* RE:42 calls */
    uint64_t shaded_hits;
    uint64_t pixels;
    uint64_t algorithmic_bytes;   /* SURVEY §8d formula over the counters above */
    double   ms_total;            /* device time of the whole call */
    double   ms_intersect;        /* summed durations of the traversal kernel launches: first wave's start to last wave's end on the
                                     device clock for plain single-chunk frames (an event on a dispatch packet costs ~5 us, so those
                                     launches carry none; ~4 us per launch less than a profiler's dispatch-level duration), HIP events
                                     on the launches otherwise, or always with XRT_LAUNCH_EVENTS=1.  The start stamp is the clock of
                                     workgroup 0's first wave, which need not be the first wave of the launch to start (a 1024-block
                                     grid starts first to last within ~0.3-0.7 us): the figure may be short by that much per launch */
    uint32_t intersect_launches;
    uint32_t pieces;              /* the frame was rendered in this many concurrent pieces (halves on two streams, GPUs); 1 otherwise */
    uint64_t rays_traversed;      /* queries (of rays_closest + rays_shadow) that were handed to the traversal kernels: all of them except
                                     the primary rays the ray-generation kernel answers itself because they cannot reach the scene
                                     octree's root box (OSM:318-320 returns false for them before any node is visited).  Not a
                                     counter of the reference: how much of the ray count is real traversal work on this library */
    double   ms_intersect_longest;   /* the longest single traversal launch of the frame (of those ms_intersect sums): on every configuration here
                                     the launch that traces the primary rays -- the launch class a roofline of "the dominant kernel" is about */
    uint64_t mesh_queries_facing_away;   /* with collect_stats: of mesh_queries, those whose ray is inside the mesh octree's root box and meets ONLY back
                                     faces in the whole mesh (the box of the mesh's surface normals says so, with the margin of the leaf
                                     test): RE:48-51 rejects every triangle, the reference walks the octree to find that out, this
                                     library answers "no intersection" from the normal box where the test is made (rays leaving a
                                     surface; the shadow rays and reflections of a terrain seen from above are nearly all of this kind).
                                     Not a counter of the reference either */
} xrt_stats;

/* Flattened octree node for inspection by tests (mirrors the private CubeNode, MO:32-40 / OSM:37-48). */
typedef struct xrt_node_info {
    float   bmin[3];
    float   bmax[3];
    int32_t is_leaf;
    int32_t count;        /* containingObjects.Count */
    int32_t dfs_index;    /* pre-order index */
    int32_t depth;
    int32_t first_ref;    /* offset of this node's list in the ref array returned next to it (leaves only) */
    int32_t reserved;
} xrt_node_info;

/* ---- library ------------------------------------------------------------------------------- */
int         xrt_version(void);
const char *xrt_last_error(void);                      /* thread-local, never NULL */
int         xrt_device_count(int *count_out);          /* number of HIP devices visible */

/* ---- scene upload: replaces SceneObject / Mesh / Triangle / Material graphs (SO:117-134,
 *      MESH:17-32, TRI:14-25, MAT:45-69) -------------------------------------------------------- */
int xrt_scene_create(int device, xrt_scene **scene_out);
int xrt_scene_destroy(xrt_scene *scene);

/* One Mesh (MESH:9-40). v,n: ntri*9 floats (v1,v2,v3 / n1,n2,n3), uv: ntri*6, surf_n: ntri*3
 * (Triangle.surfaceNormal, TMP:199-203), color: ntri*4 (Triangle.color), bbox: Mesh.MeshBoundingBox
 * min xyz max xyz (TMP:244-307). */
int xrt_scene_add_mesh(xrt_scene *scene, const float *v, const float *n, const float *uv,
                       const float *surf_n, const float *color, int32_t ntri,
                       const xrt_material *material, const float bbox[6], int32_t *mesh_id_out);

/* One SceneObject (SO:12): its shared mesh list (SO:126-127), World / InverseWorld (SO:183-199),
 * BoundingBox (SO:131) and the un-normalised WorldBoundingBox (SO:195-196). */
int xrt_scene_add_object(xrt_scene *scene, const int32_t *mesh_ids, int32_t n_meshes,
                         const float world[16], const float inv_world[16],
                         const float bbox[6], const float world_bbox[6], int32_t *object_id_out);

/* Mesh.Init -> MeshOctree.Build for every mesh (MESH:27-32, MO:56-96, 204-236; threshold MO:42) and
 * OctreeSpatialManager.Build (OSM:64-113, 218-248; threshold OSM:50); then uploads to HBM.
 * Pass 0 for the reference defaults (50 / 20). */
int xrt_scene_build(xrt_scene *scene, int32_t mesh_threshold, int32_t scene_threshold);

/* Scene file -- what the reference keeps as .xnb content (the processor's Model.Tag, TMP:113-117: meshes with their materials):
 * xrt_scene_save writes the meshes, materials, texels and bodies of `scene` exactly as they were added (little-endian, version
 * tagged; format in scene_host.cpp); xrt_scene_load is xrt_scene_create followed by the same add_mesh / add_object calls.  The
 * octrees are not stored: call xrt_scene_build after loading (it reproduces them, MO:56-96 / OSM:64-113). */
int xrt_scene_save(const xrt_scene *scene, const char *path);
int xrt_scene_load(int device, const char *path, xrt_scene **scene_out);

/* Inspection of the built trees (test support). mesh_id >= 0: that mesh's MeshOctree; mesh_id == -1:
 * the scene octree (refs are object ids). Call with NULL arrays to get the counts. Nodes are returned
 * in DFS pre-order. */
int xrt_scene_get_tree(const xrt_scene *scene, int32_t mesh_id, xrt_node_info *nodes,
                       int64_t *n_nodes_inout, int32_t *refs, int64_t *n_refs_inout);

/* ---- seam 1: ISpatialManager.GetRayIntersection (ISM:15 = OSM:312-455), batched --------------
 * ignore_object (nullable, n entries) is the dead `Mesh ignoreObject` parameter (OSM:343 compares a
 * Mesh with an ISpatialBody and can never be equal); it is accepted and ignored. Host buffers.
 * Re-entrant like the reference's (its N render threads call it concurrently, RT:105-113): concurrent
 * seam-1 calls on one scene are serialised inside the library and every caller gets its own answers.
 * They may also run while a begin/end ticket is open, except with stats_out (the counters are shared
 * with the frames' counting pass): XRT_E_BUSY.  The scene must not be rebuilt or destroyed meanwhile. */
int xrt_scene_intersect(xrt_scene *scene, const xrt_ray *rays, const int32_t *ignore_object,
                        int64_t n, xrt_hit *hits_out, xrt_stats *stats_out /* nullable */);

/* Same with device pointers (HBM resident rays / hits), asynchronous on `stream` (a hipStream_t,
 * NULL = default stream). Nothing is copied; the caller synchronises. */
int xrt_scene_intersect_device(xrt_scene *scene, const void *d_rays, int64_t n, void *d_hits_out,
                               void *stream);

/* MeshOctree.GetRayIntersection of one mesh in object space (MO:259-326); hit.object = -1,
 * w = objectSpacePosition (MO:310-312). */
int xrt_mesh_intersect(xrt_scene *scene, int32_t mesh_id, const xrt_ray *rays, int64_t n,
                       xrt_hit *hits_out);

/* ---- seam 2: RayTracer.RenderInternal (RT:103-126) / RenderInternalWithMultisampling
 *      (RT:128-168) -------------------------------------------------------------------------------
 * Fills rgba_out[y*W + x] with the packed XNA Color (R in the low byte, RT:425). Blocking.
 * rgb_f32_out (nullable, W*H*3) receives the iteration-0 colorVector before packing (RT:705/726); in the supersampled
 * modes, which average PACKED colours (RT:309), it receives Color.ToVector3() of the pixel's final colour (written by
 * the resolve kernel).  Not available with n_gpus > 1 (XRT_E_UNSUPPORTED).
 * A second concurrent call on the same scene returns XRT_E_BUSY (RT:62-63). */
int xrt_render(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights,
               const xrt_render_opts *opts, uint32_t *rgba_out, float *rgb_f32_out,
               xrt_stats *stats_out /* nullable */);

/* Pipelined form of xrt_render -- RenderAsync / RenderCompleted (RT:59-79, 431-437) with the frame still ending in the
 * host's Color[] (CurrentTarget.SetData, RT:122-123).  _begin enqueues the frame and its device-to-host copy and returns
 * a ticket; _end waits for both and fills stats_out (may be NULL).  Up to two frames may be open (tickets are shared with
 * xrt_render_device_begin), so the copy of frame i runs under the rendering of frame i+1.  rgba_out must stay valid
 * until _end; the copy overlaps only if the buffer is page-locked: xrt_host_register it once (the C# host pins its
 * renderTargetData with GCHandle first), otherwise the runtime stages it. */
int xrt_render_begin(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights,
                     const xrt_render_opts *opts, uint32_t *rgba_out, int32_t *ticket_out);
int xrt_render_end(xrt_scene *scene, int32_t ticket, xrt_stats *stats_out);

/* Page-lock / release a caller-owned host buffer for DMA (hipHostRegister): the host Color[] of xrt_render[_begin]. */
int xrt_host_register(void *host_ptr, uint64_t bytes);
int xrt_host_unregister(void *host_ptr);

/* Same, writing to device memory. With opts->shard_count > 1 only this rank's tiles are rendered and
 * d_rgba_out receives them contiguously, tile after tile (see xrt_shard_layout); otherwise the full
 * W*H frame. The call enqueues on `stream` and synchronises it before returning (stats need it). */
int xrt_render_device(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights,
                      int32_t n_lights, const xrt_render_opts *opts, void *d_rgba_out,
                      void *stream, xrt_stats *stats_out /* nullable */);

/* Pipelined form of xrt_render_device.  _begin enqueues the frame and returns a ticket while the GPU is still working;
 * _end waits for that frame and fills stats_out (may be NULL).  Up to two frames may be in flight, so the host side of
 * frame i+1 (argument marshalling, ~25 launches) overlaps the GPU side of frame i -- the reference's game loop does the
 * same with RenderAsync (RT:92-104) and one frame of latency.  With stream == NULL each of the two frame contexts runs
 * on a stream of its own and the two frames also overlap ON the GPU: a launch of persistent waves leaves the machine
 * half empty while its last rays finish, and the other frame's kernels fill it (a given stream serialises them
 * instead).  d_rgba_out of a frame is complete when its _end returns; give the two frames in flight different output
 * buffers.  Frames that need host decisions between passes (adaptive supersampling, more than one chunk) finish inside
 * _begin and never overlap another frame; a frame with Transparent materials (a ray tree per pixel) of one chunk is enqueued
 * like a plain frame with optimistically sized ray buffers and, should a generation not fit, rendered again inside _end.  While a ticket is open every other call that renders
 * or mutates the scene returns XRT_E_BUSY. */
int xrt_render_device_begin(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights,
                            int32_t n_lights, const xrt_render_opts *opts, void *d_rgba_out, void *stream,
                            int32_t *ticket_out);
int xrt_render_device_end(xrt_scene *scene, int32_t ticket, xrt_stats *stats_out);

/* Image-tile shard geometry: tiles are XRT_TILE_W x XRT_TILE_H pixels, numbered row-major, tile t is
 * owned by rank t % shard_count and stored at slot t / shard_count of that rank's buffer.  Inside a tile's 512 words
 * the pixels are stored as eight 8x8-pixel blocks, left to right, Z-order inside a block (the order the wavefronts
 * trace them in); xrt_detile_device undoes it. */
#define XRT_TILE_W 64
#define XRT_TILE_H 8
int xrt_shard_layout(int32_t width, int32_t height, int32_t shard_count, int32_t *tiles_x_out,
                     int32_t *tiles_y_out, int32_t *tiles_per_rank_out);

/* ---- cost-aware tile assignment (one process per GPU; xrt_render_opts.balance_tiles does the same inside the library) ------------
 * The reference balances its render threads dynamically: each takes the next scanline from a shared counter (RT:48-52, 105-120).
 * Across GPUs the counterpart is a TILE TABLE made from the previous frame's costs, replacing the round-robin default:
 *   tile_of_slot[r * tiles_per_rank + s] = the tile (row-major number, as xrt_shard_layout) rank r renders at slot s of its buffer,
 *                                          or -1 for an unused slot; every tile of the frame appears exactly once.
 * Results never depend on the table (every tile is rendered exactly once, by the same code); only which rank renders it does. */

/* Install (tile_of_slot != NULL) or remove (NULL) the table of frames of width x height pixels rendered with shard_count shards.  The
 * table is copied.  While it is installed, xrt_render_device[_begin] calls of that size and shard count render the tiles of row
 * shard_rank of the table, tiles_per_rank slots (512 pixels each, unused slots zero) -- other sizes and shard counts keep the
 * round-robin layout.  XRT_E_INVALID_ARG unless every tile appears exactly once.  XRT_E_BUSY while a frame is in flight. */
int xrt_scene_set_tile_table(xrt_scene *scene, int32_t width, int32_t height, int32_t shard_count, int32_t tiles_per_rank,
                             const int32_t *tile_of_slot);

/* Cost of every tile (tiles_x * tiles_y floats, row-major tile order) of the frames of width x height pixels this scene object rendered
 * since the last call with reset != 0: device-clock ticks its wave packets spent on the tile's rays, all generations (tiles another
 * rank rendered: 0 -- sum the ranks' arrays).  Frames the per-lane kernel traces (one sample per pixel on one-body scenes, adaptive
 * supersampling, ray trees) report no costs: all zeros, and xrt_balance_tiles then returns the round-robin table.  XRT_E_BUSY while a
 * frame is in flight. */
int xrt_scene_tile_costs(xrt_scene *scene, int32_t width, int32_t height, float *cost_out, int32_t reset);

/* Greedy longest-processing-time-first assignment of the frame's tiles to shard_count ranks: tiles in descending order of cost (ties:
 * ascending tile number), each to the rank with the least cost so far that still has a free slot (ties: the lowest rank); the slots
 * of a rank are then filled in ascending tile order (neighbouring waves work on neighbouring tiles).  tiles_per_rank must be at least
 * ceil(tiles / shard_count) -- the slack above that is what lets a rank take more cheap tiles than another takes expensive ones
 * (xrt_shard_layout's value + 25 % is what bench.py uses).  A cost array without a positive finite entry gives the round-robin
 * table.  Pure host arithmetic, deterministic: every rank computes the same table from the same costs.  tile_of_slot_out:
 * shard_count * tiles_per_rank entries. */
int xrt_balance_tiles(int32_t width, int32_t height, int32_t shard_count, const float *tile_cost, int32_t tiles_per_rank,
                      int32_t *tile_of_slot_out);

/* xrt_detile_device for buffers rendered under a tile table: d_tile_of_slot is the table in DEVICE memory (shard_count *
 * tiles_per_rank int32). */
int xrt_detile_table_device(int32_t width, int32_t height, int32_t shard_count, int32_t tiles_per_rank, const void *d_tile_of_slot,
                            const void *d_gathered, int64_t rank_stride, void *d_rgba_out, void *stream);

/* De-tile the gathered per-rank buffers (rank-major: rank r's tiles_per_rank * 512 pixels start at pixel
 * r * rank_stride; rank_stride 0 = tiles_per_rank * 512, i.e. contiguous) into a W*H frame on the device (used on
 * rank 0 after the RCCL gather; a stride lets one gather carry the tiles of several frames). */
int xrt_detile_device(int32_t width, int32_t height, int32_t shard_count, const void *d_gathered, int64_t rank_stride,
                      void *d_rgba_out, void *stream);

/* Can the in-library multi-GPU path (xrt_render_opts.n_gpus > 1) load RCCL?  XRT_OK, or XRT_E_RCCL with the loader's message in
 * xrt_last_error().  Touches no device: a host can ask before it offers the option (the reference has no counterpart; the call
 * exists so that the failure a C# host would otherwise meet inside RenderInternal, RT:103-126, can be met up front). */
int xrt_rccl_probe(void);

/* Diagnostics of the split walks of long packets (no counterpart in the reference: its scanline threads never share a ray).  The traversal kernel
 * of one-body scenes lets a packet whose octree walk has outlasted its budget hand pending subtrees to other wavefronts; results never depend on it.
 * out[0] subtrees handed over, out[1] taken by another (or, at the end of a launch, the same) wavefront, out[2] packets that were split, out[3] packets
 * whose results were written by a taker -- counted on the scene's device since the library was loaded or since the last call with reset != 0. */
int xrt_split_stats(xrt_scene *scene, uint64_t out[4], int32_t reset);

/* Diagnostics of "end early" (testing aid; XRT_END_EARLY, results never depend on it): plain one-chunk frames of one-body scenes that want no float
 * colours give every path that ends at generation 0 its colour where it ends.  For the last finished frame of the scene: out[0] paths coloured by the
 * ray generation kernel (they cannot reach the scene's root box, or have no pixel), out[1] paths coloured by the shading kernel (misses, and hits with
 * no shadow ray and no reflection to trace), out[2] paths left to the compose kernel's list -- each counted on the device by the kernel that did it.
 * They sum to the frame's paths; all zero: the frame did not take that way.  The output buffer of a frame is written by the frame's last kernel
 * only, on this way as on every other. */
int xrt_debug_end_counts(xrt_scene *scene, uint64_t out[3]);

/* Diagnostics of the primary packets (testing aid; XRT_PK_QUADS, results never depend on it).  The ray generation kernel compacts a frame's live primary
 * rays into slots 0 .. live-1 and, where the packet kernel traces them, writes a table beside them: one entry (first slot, rays) per aligned unit of 64
 * places of the frame that has a live ray; a packet of the first traversal launch is one entry.  For the last finished frame of the scene, if it had
 * one chunk: counts[0] entries of the table, counts[1] live primary rays; up to entries_cap entries go to entries_out (two words each: first slot,
 * rays) and up to paths_cap words of the live list -- the path of the frame whose ray sits in slot j -- to paths_out (either may be null with a capacity
 * of 0).  counts[0] == 0: the frame's first launch took no table (another kernel, a batch, an adaptive frame, XRT_PK_QUADS=0).
 * A list counts as the scene's last frame too.  After xrt_render_pixels[_device] with XRT_LIST_COHERENT whose last pass was one chunk and took a table
 * (the packet kernel traced its first rays) the call reports that table: a unit is 64 aligned places of the pass -- place r is sample r % samples of
 * entry r / samples of the pass's part of the list, so 4 entries with 16 samples, 16 level-0 quadrants, 64 one-sample entries --, counts[1] the live
 * rays and paths_out[j] the place of the ray in slot j.  After any other list call (unhinted, xrt_cast_rays*, xrt_shade_hits) counts[0] == 0. */
int xrt_debug_packet_table(xrt_scene *scene, uint64_t counts[2], uint32_t *entries_out, int64_t entries_cap, int32_t *paths_out, int64_t paths_cap);

/* Diagnostics of the screen boxes (testing aid; XRT_PK_SCREEN, results never depend on it).  A camera frame of a one-body scene whose primary rays the
 * packet kernel traces writes, every frame, one entry per leaf reference of the body's mesh octree: the screen bounding box, in sixteenths of a pixel and
 * rounded outwards, outside which no primary ray of the frame can be accepted by the reference's triangle -- two words, x0 | x1 << 16 and y0 | y1 << 16,
 * each field 16 x + 8 clamped to 0 .. 65534; both words all ones: no box is proven for that triangle.  For the last finished frame of the scene, if it
 * had one chunk: *count entries (0: the frame took no table), up to entries_cap of them to entries_out (null with a capacity of 0) -- the table the
 * device wrote, or with host_eval != 0 the same entries evaluated by the host's build of the same functions from the host's copy of the scene (the two
 * are equal word for word). */
int xrt_debug_screen_table(xrt_scene *scene, int32_t host_eval, uint64_t *count, uint32_t *entries_out, int64_t entries_cap);

/* RayTracer.Progress (RT:43-46): fraction of the frame's ray generations completed; callable from
 * another thread during xrt_render. */
float xrt_progress(const xrt_scene *scene);

/* Primary rays of RayTracer.Render (RT:410-421): two Viewport.Unproject per pixel, row-major. */
int xrt_generate_primary_rays(xrt_scene *scene, const xrt_camera *camera, xrt_ray *rays_out /* W*H */);

/* ---- seam 3: RayTracer.CastRay (RT:506-737) on caller-given rays, batched ----------------------------------------------
 * Added within ABI 203: these two exports are additive; no existing struct, field or entry point changed.
 * For every i: CastRay(ref rays[i], out color, iteration, origin, null, current_ref_index) -- one recursion per ray, with lights,
 * shadow rays, reflections, refraction (a ray tree on Transparent materials) and the RGBA8 quantisation of every level.
 * origin = (rays[i].ignore_mesh, rays[i].ignore_tri), or null when ignore_tri < 0 (the convention of xrt_scene_intersect); a
 * non-negative ignore_tri that names no triangle of the scene is XRT_E_INVALID_ARG here (xrt_cast_rays_device cannot look at the
 * rays: it treats such an origin as null).  ignoreObject is not taken: it is a Mesh compared with ISpatialBodies and never matches
 * (OSM:343).  The ray is used as given: it is not normalised (CastRay does not normalise it).
 * Depth: CastRay from `iteration` reflects while iteration < MaxReflections (RT:545), i.e. a frame's recursion of
 * max(0, max_reflections - iteration) generations; above 64 that is XRT_E_INVALID_ARG, and with Transparent materials above 12
 * XRT_E_UNSUPPORTED, as for frames.  An iteration at or above max_reflections casts no reflection.
 * current_ref_index is the first generation's currentRefIndex (RT:658: equal to a material's RefractionIndex means "inside"); a
 * frame passes 1.0f (RT:424).
 * opts: max_reflections / address_mode / filtering / collect_stats as for a frame; use_multisampling must be XRT_MS_OFF, shard_count
 * and n_gpus 0 or 1 (else XRT_E_INVALID_ARG).
 * rgba_out[i] = the packed Color; rgb_f32_out[i*3 ..] (may be NULL) = the vector handed to `new Color(...)` (RT:705/726/732), as in
 * xrt_render.  stats_out (may be NULL): pixels = n; rays_closest, rays_shadow, hits_closest and shaded_hits always; hits_shadow and
 * the reference work counters with collect_stats (as for frames).  n == 0 does nothing and returns XRT_OK.  Blocking; XRT_E_BUSY under the rule of xrt_render (RT:62-63):
 * while another call renders on the scene or a begin/end ticket is open. */
int xrt_cast_rays(xrt_scene *scene, const xrt_ray *rays, int64_t n, int32_t iteration, float current_ref_index,
                  const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                  uint32_t *rgba_out, float *rgb_f32_out, xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers (d_rays: n xrt_ray, d_rgba_out: n words, d_rgb_f32_out: NULL or 3n floats; each 16-byte aligned, else
 * XRT_E_INVALID_ARG), enqueued on `stream` (a hipStream_t; NULL = the scene's stream) and synchronised before it returns, like
 * xrt_render_device.  The rays must be ready on `stream`. */
int xrt_cast_rays_device(xrt_scene *scene, const void *d_rays, int64_t n, int32_t iteration, float current_ref_index,
                         const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                         void *d_rgba_out, void *d_rgb_f32_out, void *stream, xrt_stats *stats_out /* nullable */);

/* ---- seam 3 without its query: the part of CastRay that follows from an IntersectionResult (RT:514-737), on caller-given hits ----------
 * Added within ABI 203: these two exports are additive; no existing struct, field or entry point changed.
 * CastRay is a closest-hit query (RT:512) and then everything that follows from its result: fragment normal, shadow rays, the reflection
 * and refraction recursion, texture lookup, the RGBA8 quantisation of every level.  xrt_scene_intersect is the first half alone and
 * xrt_cast_rays the two in a row; xrt_shade_hits is the second half alone, for a host that already knows what its rays hit -- a still whose
 * lights, materials or triangle values change from image to image (G1:152-190), or hits taken from a raster G-buffer.
 * For every i: CastRay(ref rays[i], out color, iteration, origin, null, current_ref_index) with RT:512 replaced by "the query returned hits[i]":
 *   hits[i].hit == 0: the query returned false, the path ends as a miss (RT:729-733).
 *   otherwise result.mesh, .triangle, .u, .v, .worldPosition = mesh, tri, u, v, (wx, wy, wz), taken bit for bit (NaN, infinities, -0.0 as given).
 * Of the ray CastRay reads Direction (RT:549 and the refraction).  What it does not read is accepted and ignored: the ray's origin,
 * ignore_mesh / ignore_tri (the origin triangle only enters the query that is skipped), and of a hit d, leaf, reserved and object.  The host
 * form still rejects, as a caller's mistake, an entry with hit != 0 whose mesh is not in [0, n_meshes), whose tri is not in [0, ntri(mesh)),
 * whose object is not in [0, n_bodies) or whose mesh is not one of that body's meshes: XRT_E_INVALID_ARG, the message names the first
 * offending index, nothing is rendered.
 * Hence xrt_shade_hits(R, xrt_scene_intersect(R)) gives the rgba_out and rgb_f32_out of xrt_cast_rays(R) bit for bit for the same iteration,
 * current_ref_index, lights and opts, and with xrt_generate_primary_rays and XRT_MS_OFF the frame of xrt_render.  Every level below the
 * first is traced as xrt_cast_rays traces it.
 * iteration, current_ref_index, lights, opts, the depth limits (above 64 generations XRT_E_INVALID_ARG, Transparent materials above 12
 * XRT_E_UNSUPPORTED), the outputs, n == 0 (XRT_OK), blocking and XRT_E_BUSY: as for xrt_cast_rays, word for word.  Ray trees are supported;
 * poses, materials and triangle values are the latest.  What is wrong with the arguments alone is said first, also on a host-only scene;
 * then XRT_E_NO_DEVICE, XRT_E_NOT_BUILT, XRT_E_BUSY.
 * stats_out (may be NULL): pixels = n.  The n skipped queries are not counted: rays_closest and hits_closest count the queries of the levels
 * below the first (xrt_cast_rays' figures minus n, and minus the entries with hit != 0); rays_shadow and shaded_hits as for xrt_cast_rays;
 * rays_traversed what was handed to the traversal kernels; with collect_stats the reference work counters cover the queries the call made.
 * With n_lights == 0 and max_reflections <= iteration no traversal kernel is launched at all (intersect_launches == 0).
 * There is no form that records ray paths and no begin / end form. */
int xrt_shade_hits(xrt_scene *scene, const xrt_ray *rays, const xrt_hit *hits, int64_t n,
                   int32_t iteration, float current_ref_index,
                   const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                   uint32_t *rgba_out, float *rgb_f32_out /* nullable */, xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers (d_rays: n xrt_ray, d_hits: n xrt_hit, d_rgba_out: n words, d_rgb_f32_out: NULL or 3n floats; each 16-byte
 * aligned, else XRT_E_INVALID_ARG), enqueued on `stream` (a hipStream_t; NULL = the scene's stream) and synchronised before it returns, like
 * xrt_cast_rays_device.  Rays and hits must be ready on `stream`.  Nothing is inspected on the host and `object` is not looked at: the
 * kernel range-checks mesh and tri of every entry, and an entry out of range is shaded as a miss -- it affects no other entry and can
 * never address outside the scene's arrays. */
int xrt_shade_hits_device(xrt_scene *scene, const void *d_rays, const void *d_hits, int64_t n,
                          int32_t iteration, float current_ref_index,
                          const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                          void *d_rgba_out, void *d_rgb_f32_out /* nullable */, void *stream,
                          xrt_stats *stats_out /* nullable */);

/* ---- the light loop of CastRay alone (RT:534-542) on caller-given hits, in fp32 ---------------------------------------------------------
 * Added within ABI 203: these two exports are additive; no existing struct, field or entry point changed.
 * Behind its query CastRay asks IsLightPathObstructed once per light (RT:465-502) and sums ILight.GetLightForFragment (SPOT:37-62, DIR:23-30)
 * scaled by 1 - lightAmount.  xrt_shade_hits hands that sum out only inside a colour -- multiplied by the surface colour, lerped with a
 * reflection, quantised to RGBA8 per level; xrt_light_hits hands out the sum itself and the per-light amounts: for a host that keeps its own
 * CastRay and wants its shadow queries answered in batches, for ray-traced shadow masks over a raster G-buffer, for light baking and probes.
 * For every i, `result` is what RT:512 returned:
 *   hits[i].hit == 0: the query returned false.  The light is (0, 0, 0) and every amount of the entry is 0.0f.
 *   otherwise result.mesh, .triangle, .u, .v, .worldPosition = mesh, tri, u, v, (wx, wy, wz), taken bit for bit (NaN, infinities, -0.0 as given:
 *   computed as the arithmetic gives it, and no other entry is affected).  fragmentNormal follows RT:520-531: with Material.InterpolateNormals
 *   it is interpolated from n1..n3 with u, v and normalised, otherwise it is surfaceNormal as stored (the reference does not transform it).
 *   object, leaf, d and reserved are not read and not checked.
 * amount_out[i * n_lights + l] = IsLightPathObstructed(result, lights[l]): the shadow ray is (worldPosition, dirToLight) -- for a spot light
 * dirToLight = Position - worldPosition, its Length() the distance, then normalised; for a directional light -Direction and float.MaxValue -- and
 * the query ignores (mesh, tri).  The path is obstructed when the query hits and its d is below the distance -- the object-space d of OSM:373,450
 * against a world-space length, as the reference compares them.  An obstructed path gives color.W of the blocker's triangle when the blocker's
 * material is Transparent and 1 otherwise; a free path gives 0.
 * light_f32_out[3i ..] = RT:534-542 from Vector3.Zero: for each light in order, when lightAmount != 1f,
 * += GetLightForFragment(worldPosition, fragmentNormal) * (1 - lightAmount).  Nothing is quantised.  On a mesh that is untextured and whose
 * Triangle.color.XYZ is (1, 1, 1) this is, bit for bit, the rgb_f32_out of xrt_shade_hits and of xrt_cast_rays on the rays that produced the
 * hits with max_reflections <= iteration (RT:726 multiplies the light sum by the surface colour and by nothing else).
 * Poses, materials and triangle values are the latest, as for xrt_cast_rays.  Any light count a frame accepts is accepted; with n_lights == 0
 * every light sum is (0, 0, 0) and no traversal kernel is launched (intersect_launches == 0).  Long lists are split into chunks under the
 * shadow byte budget (XRT_SHADOW_BYTES); nothing about the answers depends on the split.
 * Either output may be NULL, not both.  In this order: XRT_E_INVALID_ARG -- said first, also on a host-only scene -- for n < 0, n_lights < 0,
 * lights NULL with n_lights > 0, both outputs NULL with n > 0, a needed array NULL, and in the host form an entry with hit != 0 whose mesh is
 * not in [0, n_meshes) or whose tri is not in [0, ntri(mesh)) (the message names the first offending index, nothing is computed); n == 0
 * returns XRT_OK; then XRT_E_NO_DEVICE, XRT_E_NOT_BUILT, and XRT_E_BUSY under the rule of xrt_cast_rays.  Blocking.
 * stats_out (may be NULL): pixels = n; shaded_hits the entries treated as hits; rays_shadow = shaded_hits * n_lights; rays_traversed the shadow
 * rays handed to a traversal kernel (on a scene of one body with one mesh the library answers a ray itself when the whole mesh faces away from
 * it); ms_total, ms_intersect and intersect_launches summed over the call's chunks; everything else 0.
 * There is no begin / end form and no form for supersampled lists. */
int xrt_light_hits(xrt_scene *scene, const xrt_hit *hits, int64_t n,
                   const xrt_light *lights, int32_t n_lights,
                   float *light_f32_out /* nullable, 3 n */, float *amount_out /* nullable, n * n_lights */,
                   xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers (d_hits: n xrt_hit, d_light_f32_out: NULL or 3n floats, d_amount_out: NULL or n * n_lights floats; each 16-byte
 * aligned, else XRT_E_INVALID_ARG), enqueued on `stream` (a hipStream_t; NULL = the scene's stream) and synchronised before it returns.  The
 * hits must be ready on `stream`.  Nothing is inspected on the host: the kernels range-check mesh and tri of every entry, and an entry out
 * of range is treated as a miss -- it affects no other entry and can never address outside the scene's arrays. */
int xrt_light_hits_device(xrt_scene *scene, const void *d_hits, int64_t n,
                          const xrt_light *lights, int32_t n_lights,
                          void *d_light_f32_out, void *d_amount_out /* each nullable */, void *stream,
                          xrt_stats *stats_out /* nullable */);

/* ---- what CastRay computes at a hit without asking the scene anything: surface terms and the two rays it casts next ---------------------
 * Added within ABI 203: one struct and two exports, additive; no existing struct, field or entry point changed.
 * Behind its query CastRay forms the fragment normal (RT:520-531), the surface colour with its texture lookup (RT:568-581 == RT:711-724), reads
 * the material terms that weight its composition (Reflectiveness RT:584, color.W RT:699) and builds the reflected ray (RT:547-559) and, on a
 * Transparent material, the Snell refraction (RT:656-694).  xrt_shade_hits hands these out only inside a colour; xrt_surface_hits hands them out
 * themselves: a G-buffer (normal, albedo, alpha, reflectiveness, uv) of given hits, and the rays with which a host drives its own recursion --
 * light with xrt_light_hits, continue with reflect_out / refract_out through xrt_cast_rays or xrt_scene_intersect, compose with xrt_compose_hits (RT:584/699/726).
 * For every i, `result` is what RT:512 returned, as for xrt_light_hits:
 *   hits[i].hit == 0: the query returned false.  The surface record is all zero; both ray records are o = d = 0, ignore_mesh = ignore_tri = -1.
 *   otherwise mesh, tri, u, v are taken bit for bit (NaN, infinities, -0.0 as given; no other entry is affected).  object, leaf, d and reserved
 *   are not read.  (wx, wy, wz) is read only for the ray outputs, whose Position it is (RT:548, 692), and of rays[i] only d is read, only for the
 *   ray outputs (RT:549, 675, 685): `rays` may be NULL when both ray outputs are NULL.
 * surface_out[i]: normal, color and uv exactly as a frame computes them, LookupUV (MAT:71-160) with opts->address_mode and opts->filtering
 * included (bilinear filtering reads the premultiplied words); no other field of opts is read.  uv is formed whether or not the material uses
 * its texture.  next_ref_index is the n2 the nested CastRay of RT:698 receives when the material is Transparent, else current_ref_index.
 * reflect_out[i] of a hit = (worldPosition, Normalize(Reflect(ray.Direction, fragmentNormal))), ignore = (mesh, tri): origin = result.triangle
 * (RT:557/559).  It is formed for every hit; the `iteration < MaxReflections` test of RT:545 is the caller's.
 * refract_out[i] of a hit with XRT_SURF_TRANSPARENT = RT:656-694 with current_ref_index, the System.Math calls in double; a total internal
 * reflection gives a NaN direction, written as it is; ignore = (mesh, tri).  A hit that is not Transparent gets the record of a miss.
 * Materials and triangle shading values are the latest, as for xrt_cast_rays; poses are not read (the reference does not transform the normal).
 * Any output may be NULL, not all three when n > 0; what is not asked for is not loaded or computed.
 * In this order: XRT_E_INVALID_ARG -- said first, also on a host-only scene -- for a NULL scene or opts, n < 0, all outputs NULL with n > 0, a
 * needed array NULL (hits; rays with a ray output), and in the host form an entry with hit != 0 whose mesh is not in [0, n_meshes) or whose tri
 * is not in [0, ntri(mesh)) (the message names the first offending index, nothing is written); n == 0 returns XRT_OK; then XRT_E_NO_DEVICE,
 * XRT_E_NOT_BUILT, and XRT_E_BUSY under the rule of xrt_cast_rays.  Blocking.
 * stats_out (may be NULL): pixels = n; shaded_hits the entries treated as hits; ms_total; intersect_launches = 0; everything else 0.
 * There is no begin / end form, no form for supersampled lists and no view-space depth (it would need a camera). */
#define XRT_SURF_HIT          1   /* the entry was treated as a hit */
#define XRT_SURF_TRANSPARENT  2   /* Material.Transparent: refract_out[i] is a ray */
#define XRT_SURF_INTERPOLATED 4   /* Material.InterpolateNormals */
#define XRT_SURF_TEXTURED     8   /* Material.UseTexture: color came from LookupUV */

typedef struct xrt_surface {      /* 64 bytes, 16-byte aligned quarters */
    float   normal[3];            /* fragmentNormal, RT:520-531 */
    float   reflectiveness;       /* Material.Reflectiveness, RT:584 */
    float   color[3];             /* surfaceColor, RT:568-581 == RT:711-724 */
    float   alpha;                /* result.triangle.color.W, RT:699 / RT:491 */
    float   uv[2];                /* interpolatedUV, RT:570-572, formed whether or not UseTexture */
    float   refraction_index;     /* Material.RefractionIndex */
    float   next_ref_index;       /* n2 of RT:656-667 when TRANSPARENT, else current_ref_index */
    int32_t flags;                /* XRT_SURF_* */
    int32_t reserved[3];          /* written as 0 */
} xrt_surface;

int xrt_surface_hits(xrt_scene *scene, const xrt_ray *rays /* nullable without a ray output */, const xrt_hit *hits, int64_t n,
                     float current_ref_index, const xrt_render_opts *opts,
                     xrt_surface *surface_out /* nullable, n */, xrt_ray *reflect_out /* nullable, n */,
                     xrt_ray *refract_out /* nullable, n */, xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers (d_rays: NULL or n xrt_ray, d_hits: n xrt_hit, the outputs NULL or n records each; each 16-byte aligned, else
 * XRT_E_INVALID_ARG), enqueued on `stream` (a hipStream_t; NULL = the scene's stream) and synchronised once before it returns.  The inputs
 * must be ready on `stream`.  Nothing is inspected on the host: the kernel range-checks mesh and tri of every entry, and an entry out of range
 * is treated as a miss -- it affects no other entry and can never address outside the scene's arrays.  No device memory is allocated per call. */
int xrt_surface_hits_device(xrt_scene *scene, const void *d_rays, const void *d_hits, int64_t n,
                            float current_ref_index, const xrt_render_opts *opts,
                            void *d_surface_out, void *d_reflect_out, void *d_refract_out /* each nullable */, void *stream,
                            xrt_stats *stats_out /* nullable */);

/* ---- the way back up CastRay: one level of its composition, and the RT:309 fold, on caller-given terms ------------------------------------
 * Added within ABI 203: four exports, additive; no existing struct, field or entry point changed.
 * Behind its light loop CastRay either multiplies the light sum by the surface colour (RT:726, iteration >= MaxReflections) or casts the
 * reflected ray, lerps the colour that came back with the surface colour by 1.0f - Reflectiveness and multiplies by the light sum (RT:584),
 * and on a Transparent material casts the refracted ray and lerps what came back with that by color.W (RT:699); the result goes through
 * `new Color(Vector3)` -- clamp, * 255, round half to even (RT:705) -- and what a level hands up is that packed colour, read back with
 * ToVector3() (/ 255).  Every operation is rounded on its own in binary32, once per level: arithmetic a host cannot restate approximately.
 * xrt_compose_hits is those statements as the library's frames execute them, so that a recursion the host drives with xrt_surface_hits,
 * xrt_light_hits and xrt_cast_rays / xrt_scene_intersect ends in the colours the library renders, bit for bit.
 * For every i:
 *   surface[i] is the record xrt_surface_hits writes; only color, reflectiveness, alpha and the bits XRT_SURF_HIT / XRT_SURF_TRANSPARENT of
 *   flags are read.  light_f32[3i ..] is the light sum xrt_light_hits writes.  reflect_rgba[i] / refract_rgba[i] are the packed colours the two
 *   nested CastRay calls returned, as rgba_out of xrt_cast_rays packs them (their alpha byte is ignored).
 *   XRT_SURF_HIT clear: RT:732 -- colour 0xFF000000, vector (0, 0, 0); nothing else of the entry is read.
 *   reflect_rgba == NULL (the caller's `iteration >= MaxReflections`, chosen per call as the reference chooses it per generation): RT:726,
 *   colorVector = lightResult * surfaceColor.  refract_rgba must then be NULL too.
 *   reflect_rgba != NULL: RT:584, Lerp(ToVector3(reflect_rgba[i]), color, 1.0f - reflectiveness) * light; and with refract_rgba != NULL on an
 *   entry with XRT_SURF_TRANSPARENT additionally RT:699, Lerp(ToVector3(refract_rgba[i]), colorVector, alpha).  With refract_rgba == NULL
 *   RT:586 is skipped for every entry.
 * rgb_f32_out[3i ..] is the vector handed to `new Color(...)`, rgba_out[i] that colour (RT:705).  Either may be NULL, not both when n > 0.
 * Values are taken bit for bit: NaN, infinities, -0.0 and colours outside [0, 1] go through the arithmetic as a frame's would (a NaN packs to 0).
 * In this order, also on a host-only scene: XRT_E_INVALID_ARG for a NULL scene, n < 0, both outputs NULL with n > 0, surface or light_f32 NULL
 * with n > 0, refract_rgba without reflect_rgba; n == 0 returns XRT_OK; then XRT_E_NO_DEVICE, XRT_E_NOT_BUILT, and XRT_E_BUSY under the rule of
 * xrt_cast_rays (the scene is read only for its device, its stream and that rule).  Blocking, one synchronisation.
 * stats_out (may be NULL): pixels = n; shaded_hits the entries with XRT_SURF_HIT; ms_total; intersect_launches = 0; everything else 0.
 * Not here: a per-entry current_ref_index for xrt_cast_rays (a host groups refract_out by next_ref_index and casts each group with its index),
 * a begin / end form, and adaptive quadrant trees (xrt_fold_samples with samples == 4 is one level of them). */
int xrt_compose_hits(xrt_scene *scene, const xrt_surface *surface, const float *light_f32 /* 3 n */,
                     const uint32_t *reflect_rgba /* nullable, n */, const uint32_t *refract_rgba /* nullable, n */,
                     int64_t n, uint32_t *rgba_out /* nullable, n */, float *rgb_f32_out /* nullable, 3 n */,
                     xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers, each 16-byte aligned (else XRT_E_INVALID_ARG, stated after the errors above and before n == 0), enqueued on `stream`
 * (a hipStream_t; NULL = the scene's stream) and synchronised once before it returns.  The inputs must be ready on `stream`.  d_rgba_out may be
 * d_reflect_rgba or d_refract_rgba itself -- an entry is read before it is written, so a recursion composes in place --; any other overlap is
 * undefined.  No device memory is allocated per call. */
int xrt_compose_hits_device(xrt_scene *scene, const void *d_surface, const void *d_light_f32,
                            const void *d_reflect_rgba /* nullable */, const void *d_refract_rgba /* nullable */,
                            int64_t n, void *d_rgba_out, void *d_rgb_f32_out /* each nullable */, void *stream,
                            xrt_stats *stats_out /* nullable */);

/* RT:309 on caller-given colours.  samples == 4: rgba_out[i] = new Color((a.ToVector3() + b.ToVector3() + c.ToVector3() + d.ToVector3()) / 4.0f)
 * over rgba_in[4i .. 4i + 3], summed left to right.  samples == 16: four such means over rgba_in[16i + 4q ..], each re-quantised, then their
 * mean -- the record order xrt_trace_pixels and xrt_render_pixels give XRT_MS_FIXED16 (corner q = s / 4, sub-sample s % 4).  rgb_f32_out[3i ..]
 * (nullable) is ToVector3() of the result, as the supersampled modes of xrt_render_pixels report it.  The alpha bytes are ignored; the result's
 * is 0xFF.  Errors in the order of xrt_compose_hits: NULL scene, n < 0, samples neither 4 nor 16, rgba_out NULL with n > 0, rgba_in NULL with
 * n > 0, (device form) alignment -- all XRT_E_INVALID_ARG --; n == 0 returns XRT_OK; XRT_E_NO_DEVICE, XRT_E_NOT_BUILT, XRT_E_BUSY.
 * stats_out: pixels = n, ms_total, everything else 0. */
int xrt_fold_samples(xrt_scene *scene, const uint32_t *rgba_in /* n * samples */, int64_t n, int32_t samples /* 4 or 16 */,
                     uint32_t *rgba_out /* n */, float *rgb_f32_out /* nullable, 3 n */, xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers, each 16-byte aligned; d_rgba_out must not overlap d_rgba_in. */
int xrt_fold_samples_device(xrt_scene *scene, const void *d_rgba_in, int64_t n, int32_t samples,
                            void *d_rgba_out, void *d_rgb_f32_out /* nullable */, void *stream, xrt_stats *stats_out /* nullable */);

/* ---- seam 3, second half: RayTracer.points (RT:504, 543, 701, 740-747) and CastRay's `ref Ray ray` (RT:692-694) ---------------------
 * Added within ABI 203: one struct and two exports, additive; no existing struct, field or entry point changed.
 * Every CastRay appends line segments to the public list RayTracer.points -- the reference's host draws it over its preview (G1:403-413) --
 * and overwrites the ray it was given where it refracts.  For one call C(ray, it), in this order:
 *   miss: nothing.   hit: the segment (ray.Position, hit position) in Color.White, whether or not it < MaxReflections (RT:543);
 *   if it < MaxReflections: the segments of the reflection, cast with a fresh ray (RT:547-559);
 *   if the material is also Transparent: ray = (hit position, refracted direction) (RT:692-694), the segments of C(ray, it + 1) on that
 *   same variable (RT:698), then (ray.Position, ray.Direction * 100) in Color.Red (RT:701) with ray as the nested call left it -- the second
 *   vertex is the direction times 100.0f, a vector, not a point on the ray; every red segment of an unbroken refraction chain therefore
 *   carries the chain's last ray (the deepest one assigned at RT:692-694, whether or not it hit anything).
 * xrt_path_vertex is VertexPositionColor: position, then the colour packed as rgba_out packs colours (White 0xFFFFFFFF, Red 0xFF0000FF);
 * a segment is two consecutive vertices (PrimitiveType.LineList).  Non-finite values (total internal reflection, RT:676) are recorded as they are.
 *
 * xrt_cast_rays_paths is xrt_cast_rays -- every word said there holds, and rgba_out / rgb_f32_out / stats_out are bit for bit what it
 * returns for the same arguments -- and additionally:
 *   vertices[vertex_start[i] .. vertex_start[i + 1]) = the vertices of ray i in the reference's order, rays in the caller's order (as if the
 *   reference had made the n calls one after the other on one thread); vertex_start (may be NULL) has n + 1 entries, vertex_start[n] ==
 *   *n_vertices_out, always even.
 *   *n_vertices_out (not NULL) = the number of vertices the batch NEEDS.  vertices == NULL with vertex_capacity == 0, or a capacity that is
 *   too small, is no error: the first vertex_capacity vertices (rounded down to whole segments) are written, nothing at or behind
 *   vertices[vertex_capacity], vertex_start is complete and the call returns XRT_OK -- compare the count with the capacity.  A call with
 *   vertices == NULL counts; nothing is traced twice within one call.  vertex_capacity < 0, or > 0 with vertices == NULL: XRT_E_INVALID_ARG.
 *   rays_back (may be NULL; may be `rays` itself): rays_back[i].o / .d = the ray as CastRay leaves its `ref ray` -- the last ray of the
 *   refraction chain that starts at the root, or the ray as given when the root misses, is not Transparent or iteration >= max_reflections;
 *   ignore_mesh / ignore_tri are copied from rays[i].
 * n == 0: *n_vertices_out = 0 and vertex_start[0] = 0.
 * Frames record nothing: the reference's Render clears the list (RT:61) and then appends every pixel's segments under one lock, which
 * nobody wants at 1080p; xrt_render* stay as they are. */
typedef struct xrt_path_vertex {
    float    position[3];
    uint32_t color;
} xrt_path_vertex;

int xrt_cast_rays_paths(xrt_scene *scene, const xrt_ray *rays, int64_t n, int32_t iteration, float current_ref_index,
                        const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                        uint32_t *rgba_out, float *rgb_f32_out /* nullable */,
                        xrt_ray *rays_back /* nullable, n */, int64_t *vertex_start /* nullable, n + 1 */,
                        xrt_path_vertex *vertices /* nullable */, int64_t vertex_capacity, int64_t *n_vertices_out,
                        xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers, as xrt_cast_rays_device: d_rays_back (NULL or n xrt_ray; NOT d_rays itself), d_vertex_start (NULL or n + 1
 * int64), d_vertices (NULL or vertex_capacity xrt_path_vertex), each 16-byte aligned, else XRT_E_INVALID_ARG.  Enqueued on `stream` and
 * synchronised once before it returns; n_vertices_out is host memory.  Nothing is written at or behind d_vertices[vertex_capacity]. */
int xrt_cast_rays_paths_device(xrt_scene *scene, const void *d_rays, int64_t n, int32_t iteration, float current_ref_index,
                               const xrt_light *lights, int32_t n_lights, const xrt_render_opts *opts,
                               void *d_rgba_out, void *d_rgb_f32_out /* nullable */,
                               void *d_rays_back /* nullable */, void *d_vertex_start /* nullable */,
                               void *d_vertices /* nullable */, int64_t vertex_capacity, void *stream,
                               int64_t *n_vertices_out /* host */, xrt_stats *stats_out /* nullable */);

/* ---- moving bodies between frames: SceneObject.Position / Rotation / Scale (SO:52-89) ------------------------------------------
 * Added within ABI 203: these three exports are additive; no existing struct, field or entry point changed.
 * The setters of the reference only mark a body dirty; its World, InverseWorld and WorldBoundingBox are recomputed lazily (SO:183-199)
 * and read by the next query (OSM:349-364, 441-443).  xrt_scene_set_poses is that, batched: for i < n, body object_ids[i] takes
 * world[16i..], inv_world[16i..] and world_bbox[6i..] (the arguments xrt_scene_add_object takes; BoundingBox stays as added).  The scene
 * octree is NOT rebuilt: OctreeSpatialManager.Build (OSM:64-99) is the only code of the reference that files bodies into it, so a moved body
 * stays in the nodes of the last xrt_scene_build / xrt_scene_build_tree and the root box keeps its bounds -- as in the reference's own game
 * loop (a body moved out of the root box is not seen until the tree is built again).
 *   - object ids out of range, n < 0, or a NULL array with n > 0: XRT_E_INVALID_ARG; n == 0 does nothing.  A body listed twice takes its
 *     last entry.
 *   - before the first xrt_scene_build the pose is simply what the build uses; on a host-only scene (device -1) the host copy is
 *     updated (xrt_scene_save writes it) and the call returns XRT_OK.
 *   - non-finite or singular transforms are accepted; the body's pre-cull record is then switched off, as at build time.
 *   - xrt_scene_save writes the current poses (the file format is unchanged).
 * Pipelining: the call may be made while one or two begin/end tickets are open, and neither synchronises the device nor waits for the
 * frames in flight.  A frame renders with the poses set before its _begin, never with later ones; seam-1 calls (xrt_scene_intersect,
 * xrt_cast_rays, ...) use the latest poses.  XRT_E_BUSY only while another thread is inside a render call on the scene. */
int xrt_scene_set_poses(xrt_scene *scene, const int32_t *object_ids, int32_t n, const float *world, const float *inv_world,
                        const float *world_bbox);

/* The same with HBM arrays (int32 ids, 16n + 16n + 6n floats), read in order after the work enqueued on `stream` (a hipStream_t; NULL = the
 * scene's stream); work enqueued on `stream` afterwards follows the update.  Every array 16-byte aligned, else XRT_E_INVALID_ARG.  The ids
 * are not looked at on the host: ids out of range are skipped, and the ids of one call must be distinct.  Host-only scene:
 * XRT_E_NO_DEVICE; before xrt_scene_build: XRT_E_NOT_BUILT. */
int xrt_scene_set_poses_device(xrt_scene *scene, const void *d_object_ids, int32_t n, const void *d_world, const void *d_inv_world,
                               const void *d_world_bbox, void *stream);

/* OctreeSpatialManager.Build alone (OSM:64-99, 218-248) over the current poses: the scene octree, its root box and the pre-cull records in
 * scene-leaf order are made again; meshes, mesh octrees, triangles and textures are untouched.  scene_threshold 0 = the reference
 * default (20, OSM:50).  The frame that follows equals that of a scene built from scratch with the same poses.  XRT_E_BUSY while a
 * begin/end ticket is open; XRT_E_NOT_BUILT before xrt_scene_build. */
int xrt_scene_build_tree(xrt_scene *scene, int32_t scene_threshold);

/* ---- changing materials between frames: Material.Reflectiveness / Transparent / RefractionIndex / InterpolateNormals / UseTexture /
 * Texture (MAT:39, 234-268) ----------------------------------------------------------------------------------------------------
 * Added within ABI 203: this export is additive; no existing struct, field or entry point changed.
 * The reference's Material has public setters and CastRay reads them at every hit (RT:515, 520, 568, 584, 586, 658): a host that turns
 * the glass spheres opaque or slides a crate's reflectiveness sees it in the next frame.  xrt_scene_set_materials is that, batched: for
 * i < n, mesh mesh_ids[i] takes materials[i] (the struct xrt_scene_add_mesh takes).
 *   - scalar fields: reflectiveness, transparent, refraction_index, interpolate_normals, use_texture are taken as given.
 *   - texels: use_texture != 0 with tex_argb != NULL replaces the mesh's texels (tex_width, tex_height, tex_pargb as in
 *     xrt_scene_add_mesh; the size may differ from the old one).  use_texture != 0 with tex_argb == NULL keeps the texels the mesh
 *     has: tex_width / tex_height must be 0 or the stored size, and a mesh that never had texels is XRT_E_INVALID_ARG (the reference:
 *     UseTexture = true on a material whose bitmap was never locked, a null dereference).  use_texture == 0 switches the flag only:
 *     the stored texels stay, as the reference's locked bitmap does, and a later use_texture = 1 with NULL texels brings them back;
 *     texels passed with use_texture == 0 are stored.  tex_pargb is read only together with tex_argb.
 *   - what xrt_scene_add_mesh rejects in a material is rejected here with the same code; mesh ids out of range, n < 0, or a NULL array
 *     with n > 0: XRT_E_INVALID_ARG.  A failing call applies nothing.  n == 0 does nothing.  A mesh listed twice takes its last entry.
 *   - before the first xrt_scene_build the call only edits what the build will use; on a host-only scene (device -1) the host copy is
 *     updated and the call returns XRT_OK.
 *   - xrt_scene_save writes the current materials and texels (the file format is unchanged; texels kept while use_texture is 0 are not
 *     part of the file, as they are not part of what xrt_scene_add_mesh is given).
 *   - mesh octrees, triangles, normal boxes, poses, the scene octree, tile tables and the geometry of replicas are not touched; nothing
 *     is rebuilt.
 * Pipelining, exactly as xrt_scene_set_poses: the call may be made while one or two begin/end tickets are open, and neither synchronises
 * the device nor waits for the frames in flight.  A frame renders with the materials set before its _begin, never with later ones --
 * including the choice between the plain and the ray-tree pipeline and the max_reflections <= 12 limit of Transparent materials, which
 * follow the frame's own materials; xrt_cast_rays* use the latest materials.  XRT_E_BUSY only while another thread is inside a render
 * call on the scene. */
int xrt_scene_set_materials(xrt_scene *scene, const int32_t *mesh_ids, int32_t n, const xrt_material *materials);

/* ---- changing which bodies exist: OctreeSpatialManager.Bodies (OSM:54-57) and Build (OSM:64-99) ---------------------------------
 * Added within ABI 203: this export is additive; no existing struct, field or entry point changed.
 * The reference's host fills the public list Bodies and calls Build() (G1:95-109); that only files the bodies into the scene octree,
 * because every Model got its MeshOctree when its SceneObject was constructed (SO:126-132, MESH:27-32).  xrt_scene_set_bodies is that
 * for a built scene: the body list is replaced and the scene octree built, and no mesh octree is built that exists already.
 *   - list replacement: the body list becomes exactly the n_bodies bodies given.  Body i has the meshes
 *     mesh_ids[mesh_start[i] .. mesh_start[i + 1]) and world[16i..], inv_world[16i..], bbox[6i..], world_bbox[6i..] (the arguments
 *     xrt_scene_add_object takes).  Body ids (xrt_hit.object, the ids of xrt_scene_set_poses) are positions in the new list.
 *   - OctreeSpatialManager.Build (OSM:64-99, 218-248) then runs over the new list; scene_threshold 0 = the reference default (20, OSM:50).
 *   - equivalence: the scene equals one made from scratch with the same meshes in the same id order, these bodies, and xrt_scene_build:
 *     frames, hits and xrt_scene_get_tree output are the same.
 *   - mesh ids never change, and (ignore_mesh, ignore_tri) pairs stay valid.  A mesh that no body names any more stays in the scene and
 *     in HBM, as a loaded Model stays in the reference's ContentManager; there is no mesh removal.
 *   - meshes added with xrt_scene_add_mesh since the last build get their MeshOctree.Build now, with the mesh_threshold of the last
 *     xrt_scene_build; no other mesh is built again.  *meshes_built_out (may be NULL) receives the number of mesh octrees the call built:
 *     0 when it only re-lists bodies of known meshes.  The count is this call's own and is written whenever the list was applied, also
 *     when the call then returns XRT_E_UNSUPPORTED (the octrees it built stay built: the repairing call reports 0); a call rejected with
 *     XRT_E_INVALID_ARG, XRT_E_NOT_BUILT or XRT_E_BUSY leaves it untouched.  The new meshes' materials and texels enter as at a build; materials changed with
 *     xrt_scene_set_materials stay, texels kept while use_texture is 0 included.
 *   - poses: the call supplies every pose; poses last set through xrt_scene_set_poses_device are discarded, not read back.
 *   - the pose and material versions start again from 0, as after xrt_scene_build_tree and xrt_scene_build.
 *   - n_bodies == 0 is legal and gives an empty scene (every ray misses); a body without meshes is legal, as in xrt_scene_add_object.
 *   - a NULL array that is needed, n_bodies < 0, mesh_start[0] != 0, a decreasing mesh_start or an unknown mesh id: XRT_E_INVALID_ARG, and
 *     nothing is applied.  Before the first xrt_scene_build: XRT_E_NOT_BUILT.  While a begin/end ticket is open or another thread
 *     renders on the scene: XRT_E_BUSY, as for xrt_scene_build_tree; the frame in flight is not disturbed.  An octree too deep for the
 *     LDS stack, or a scene octree the reference's Build would not finish (OSM:101-113: more bodies than the threshold share a point):
 *     XRT_E_UNSUPPORTED; the scene is then as xrt_scene_build_tree leaves it in that case (the host copy holds the new list,
 *     nothing can be traced), and a later successful call repairs it.
 *   - on a host-only scene (device -1) the host copy is edited and the call returns XRT_OK.
 *   - xrt_scene_save writes the new list (the file format is unchanged).
 * xrt_scene_add_object after a build, and xrt_scene_build, behave as before. */
int xrt_scene_set_bodies(xrt_scene *scene, int32_t n_bodies, const int32_t *mesh_start /* n_bodies + 1 */,
                         const int32_t *mesh_ids /* mesh_start[n_bodies] */, const float *world /* 16 n */, const float *inv_world /* 16 n */,
                         const float *bbox /* 6 n */, const float *world_bbox /* 6 n */, int32_t scene_threshold,
                         int32_t *meshes_built_out /* nullable */);

/* ---- changing triangle normals, texture coordinates and colours between frames: Triangle.n1..n3 / uv1..uv3 / color (TRI:17-23) ------
 * Added within ABI 203: these two exports are additive; no existing struct, field or entry point changed.
 * The reference's Triangle has public fields that CastRay reads at every hit: n1 / n2 / n3 for the fragment normal of an
 * InterpolateNormals material (RT:520-524), uv1 / uv2 / uv3 for the texture lookup (RT:570-572, 713-715), color.XYZ for the surface
 * colour of an untextured material (RT:578-580, 721-723) and color.W for the light a Transparent occluder lets through (RT:491) and the
 * refraction blend (RT:699).  A host that scrolls a texture's coordinates, paints vertex colours, highlights the triangle a click hit
 * (G1:296-325) or fades a glass body's alpha sees it in the next frame; no octree depends on these fields, so nothing is rebuilt.
 * xrt_scene_set_triangle_shading is that, batched, for the triangles of one mesh:
 *   - which triangles: entry i edits triangle tri_ids[i] of mesh mesh_id; indices are positions in Mesh.Triangles[], as in xrt_hit.tri.
 *     With tri_ids == NULL entry i edits triangle first_tri + i; with tri_ids != NULL first_tri must be 0.
 *   - which fields: an entry takes normals[9i..] (n1, n2, n3), uv[6i..] (uv1, uv2, uv3) and color[4i..], the layout of xrt_scene_add_mesh.
 *     A NULL array leaves that field of every listed triangle as it is; all three NULL with n > 0 is XRT_E_INVALID_ARG.  Values are taken
 *     bit for bit: NaN payloads, infinities and -0.0 are stored as given.
 *   - never touched: Triangle.surfaceNormal and the vertices are NOT settable.  The culling test (RE:49) and every conservative
 *     rejection of this library (normal boxes, tight boxes, runs, pre-cull records, answers at emission) are built on them; a host that
 *     changes them gives the mesh its triangles again (xrt_scene_set_mesh_triangles below).  Mesh octrees, runs, normal and tight boxes, poses, the scene
 *     octree, materials, texels and tile tables are not touched either.
 *   - errors: mesh_id out of range, n < 0, first_tri < 0, a range or an id outside [0, ntri), tri_ids != NULL with first_tri != 0:
 *     XRT_E_INVALID_ARG.  A failing call applies nothing.  n == 0 does nothing and returns XRT_OK.  A triangle listed twice takes its
 *     last entry.
 *   - before the first xrt_scene_build the call edits what the build will use; on a host-only scene (device -1) the host copy is
 *     edited and the call returns XRT_OK.
 *   - xrt_scene_save writes the current values (the file format is unchanged), those set through the device variant included: they are
 *     read back first.  Unlike device poses under xrt_scene_set_bodies, triangle values set on the device are never discarded: they
 *     survive xrt_scene_build_tree and xrt_scene_set_bodies (also the call that builds new meshes), are present in the replicas of an
 *     n_gpus > 1 render, and xrt_scene_build starts again from the host copy, which then holds them.
 * xrt_scene_set_triangle_shading_device: the same with the arrays in HBM (each 16-byte aligned, else XRT_E_INVALID_ARG; each nullable as
 * above).  They are read in order after the work already enqueued on `stream` (NULL: the scene's stream), and work enqueued on `stream`
 * afterwards follows the update.  The ids are not inspected on the host: ids outside [0, ntri) are skipped, and the ids of one call
 * must be distinct.  A host-only scene: XRT_E_NO_DEVICE; before xrt_scene_build: XRT_E_NOT_BUILT.
 * Pipelining, exactly as xrt_scene_set_materials: the calls may be made while one or two begin/end tickets are open, and neither
 * synchronise the device nor wait for the frames in flight.  A frame renders with the values set before its _begin, never with later
 * ones; xrt_cast_rays* use the latest values; xrt_scene_intersect* and xrt_mesh_intersect are unaffected.  XRT_E_BUSY only while another
 * thread is inside a render call on the scene. */
int xrt_scene_set_triangle_shading(xrt_scene *scene, int32_t mesh_id, const int32_t *tri_ids /* nullable */, int32_t first_tri, int32_t n,
                                   const float *normals /* nullable, 9 n */, const float *uv /* nullable, 6 n */,
                                   const float *color /* nullable, 4 n */);
int xrt_scene_set_triangle_shading_device(xrt_scene *scene, int32_t mesh_id, const void *d_tri_ids /* nullable */, int32_t first_tri, int32_t n,
                                          const void *d_normals, const void *d_uv, const void *d_color /* each nullable */, void *stream);

/* ---- replacing a mesh's triangles on a built scene: Mesh.Triangles / Mesh.MeshBoundingBox (MESH:12-14) and Mesh.Init() (MESH:27-32) ----
 * Added within ABI 203: this export is additive; no existing struct, field or entry point changed.
 * The reference's Mesh has public setters for Triangles and MeshBoundingBox, Triangle has public v1..v3 and surfaceNormal (TRI:17-23),
 * and Mesh.Init() makes a fresh MeshOctree over whatever Triangles holds (MO:56-96): a host that edits or deforms a mesh and calls
 * Init() traces the new geometry in its next query.  xrt_scene_set_mesh_triangles is that for mesh mesh_id of a built scene: the mesh
 * takes new triangles under the same id, its octree alone is built, and the storage of the old triangles is released.
 *   - arguments: v, n, uv, surf_n, color, ntri and bbox are exactly those of xrt_scene_add_mesh -- the layouts, the NULL defaults of n /
 *     uv / color, values taken bit for bit, bbox = the new Mesh.MeshBoundingBox; surf_n is the caller's, the library does not derive it.
 *     ntri may differ from the old count.  ntri == 0 is legal, as in xrt_scene_add_mesh: the mesh is then empty, every body that names it
 *     is missed through it and its storage is released.  This is what the library offers as mesh removal; mesh ids never change.
 *   - build: MeshOctree.Build (MO:56-96) runs for this mesh alone, with the mesh_threshold of the last xrt_scene_build.  No other mesh
 *     octree is built.
 *   - not touched: the mesh's material and texels (Mesh.MeshMaterial is another property), every other mesh, the body list, the bodies'
 *     BoundingBox / WorldBoundingBox (the reference computes SceneObject.boundingBox once, in the constructor, SO:126-132), the scene
 *     octree (Mesh.Init() does not call OctreeSpatialManager.Build: the bodies stay in the nodes of the last tree build, as after
 *     xrt_scene_set_poses) and tile tables.
 *   - refreshed, and only this: the pre-cull records of the bodies that name the mesh are built on Mesh.MeshBoundingBox; they are made
 *     again from the new box and the body's current pose.
 *   - equivalence: the scene equals the one obtained by starting from scratch with the new triangles in the place of the old ones and
 *     replaying the same calls: the same meshes in id order, the same bodies, xrt_scene_build, then the pose, material and shading edits
 *     made since.  Frames, hits and xrt_scene_get_tree output are equal.
 *   - triangle values set through xrt_scene_set_triangle_shading_device on OTHER meshes survive (they are read back first); those of
 *     the replaced mesh are replaced by what the call gives.  Poses set through xrt_scene_set_poses_device survive: the call supplies no
 *     pose, so they are read back, not discarded.  The pose, material and shading versions start again from 0, as after
 *     xrt_scene_set_bodies with a new mesh; the replicas of an n_gpus > 1 render are dropped and made again on the next such frame.
 *   - ids: xrt_hit.tri and ignore_tri are positions in the new Triangles[].  Hits a host kept from before the call name old triangles;
 *     the host forms of the *_hits calls range-check them as they always do.
 *   - all or nothing: the argument checks of xrt_scene_add_mesh (same codes); a mesh id out of range: XRT_E_INVALID_ARG; an octree the
 *     reference's recursion would not finish, or whose depth no longer fits the LDS stack ((scene depth + 1) + (mesh depth + 1) > 40
 *     words): XRT_E_UNSUPPORTED.  Each is checked before anything is applied: the new octree is built aside and examined before it
 *     takes the old one's place, so a failing call leaves the scene exactly as it was and still traceable.
 *   - before the first xrt_scene_build (and for a mesh added since the last build) the call edits what the build will use.
 *   - on a host-only scene (device -1) the host copy is edited and the call returns XRT_OK.  xrt_scene_save writes the new triangles
 *     (the file format is unchanged).
 *   - while a begin/end ticket is open or another thread renders on the scene: XRT_E_BUSY, as for xrt_scene_set_bodies; the frame in
 *     flight is not disturbed.
 * Not done: a device form with the vertices in HBM (the build is host code); an octree refit (the octree is built anew); an upload of
 * only the changed part (the scene's arrays are sent again, as by xrt_scene_set_bodies with a new mesh); removing a mesh ID. */
int xrt_scene_set_mesh_triangles(xrt_scene *scene, int32_t mesh_id, const float *v /* 9 ntri */, const float *n /* nullable */,
                                 const float *uv /* nullable */, const float *surf_n /* 3 ntri */, const float *color /* nullable */,
                                 int32_t ntri, const float bbox[6]);

/* ---- seam 2 on caller-chosen pixels: GetColorForQuadrant (RT:215-311) and the body of Render's inner loop (RT:412-425), batched ---------
 * Added within ABI 203: these two exports are additive; no existing struct, field or entry point changed.
 * The reference's unit of work is smaller than a frame: both functions take a screen position and produce one colour.  xrt_render_pixels is
 * that for a list: entry i has the centre (cx, cy) = (centers[2i], centers[2i + 1]) in the screen coordinates Viewport.Unproject is given
 * (RT:415), and rgba_out[i] is its colour -- a screen rectangle after an edit, every 16th pixel of a preview, the pixel under the mouse, a
 * random batch of a training step, a frame too large for its work buffers in chunks of the host's choosing.
 *   - XRT_MS_OFF: RT:412-425 with screenSpaceCoord.X = cx, .Y = cy: two Unproject, subtract, normalise,
 *     CastRay(ref ray, out color, 0, null, null, 1.0f).
 *   - XRT_MS_ADAPTIVE: GetColorForQuadrant(cx, cy, 1.0f, 0, out result) with opts->multisample_quality (RT:195, RT:215-311, including
 *     RT:305 writing urColor).
 *   - XRT_MS_FIXED16: the 16 level-1 positions around (cx, cy), as a frame takes them around a pixel: (c + (+-0.25f)) + (+-0.125f) in this
 *     association, corner q = s / 4 in UL, UR, LL, LR order, sub-sample s % 4 in the same order; the result is the RT:309 mean of four
 *     RT:309 means, each re-quantised.
 *   - any float centre is legal: fractional values and positions outside [0, vp_width) x [0, vp_height) are taken as Unproject takes them.
 *     vp_width / vp_height enter only through Unproject: there is no frame size, no tile, no cull rectangle.  Duplicates are legal, every
 *     entry gets its own answer; the order is the caller's.
 *   - equality with frames: an entry whose centre is the integer pixel (x, y) of the viewport receives, bit for bit, what xrt_render writes
 *     for that pixel, in rgba_out and in rgb_f32_out (nullable, 3 n; as for xrt_render: with XRT_MS_OFF the vector before packing, in the
 *     supersampled modes ToVector3() of the final colour), in all three modes.
 *   - opts: max_reflections, use_multisampling, multisample_quality, address_mode, filtering and collect_stats are read as for a frame;
 *     shard_count and n_gpus must be 0 or 1 (XRT_E_INVALID_ARG).  The limits of frames apply with their codes: MultisampleQuality above 6
 *     and Transparent materials above 12 reflections XRT_E_UNSUPPORTED, max_reflections above 64 XRT_E_INVALID_ARG.  Transparent materials
 *     (ray trees) are supported, as xrt_cast_rays supports them.
 *   - poses, materials and triangle values: the latest, as for xrt_cast_rays.
 *   - errors: n < 0, a NULL array that is needed, a non-finite centre (host form; nothing is rendered): XRT_E_INVALID_ARG.  What is wrong
 *     with the arguments alone is said first, also on a host-only scene; then n == 0 does nothing and returns XRT_OK; then XRT_E_NO_DEVICE /
 *     XRT_E_NOT_BUILT, then XRT_E_BUSY under the rule of xrt_render (RT:62-63): while another call renders on the scene or a begin/end
 *     ticket is open.
 *   - stats_out (may be NULL): pixels = n; rays_closest, rays_shadow, hits_closest, shaded_hits and rays_traversed as a frame reports them
 *     for the same work (every quadrant level of an adaptive list included); hits_shadow and the reference work counters with
 *     collect_stats; ms_total, ms_intersect and intersect_launches summed over the passes of the call.
 *   - a long list is split into chunks that fit a byte budget; nothing about the answers depends on the split.
 * Blocking.  There is no begin/end form. */
int xrt_render_pixels(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights,
                      const xrt_render_opts *opts, const float *centers /* 2 n: x0 y0 x1 y1 .. */, int64_t n,
                      uint32_t *rgba_out /* n */, float *rgb_f32_out /* nullable, 3 n */, xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers (d_centers: 2 n floats, d_rgba_out: n words, d_rgb_f32_out: NULL or 3 n floats; each 16-byte aligned, else
 * XRT_E_INVALID_ARG), enqueued on `stream` (a hipStream_t; NULL = the scene's stream) and complete when the call returns, like
 * xrt_cast_rays_device (the stream is synchronised after every pass: the level counts of an adaptive list come back to the host between
 * the levels).  The centres must be ready on `stream`.  They are not inspected: an entry with a non-finite centre gets an unspecified colour and
 * affects no other entry. */
int xrt_render_pixels_device(xrt_scene *scene, const xrt_camera *camera, const xrt_light *lights, int32_t n_lights,
                             const xrt_render_opts *opts, const void *d_centers, int64_t n,
                             void *d_rgba_out, void *d_rgb_f32_out /* nullable */, void *stream, xrt_stats *stats_out /* nullable */);

/* ---- the first level of xrt_render_pixels alone: the ray of RT:412-421 and the IntersectionResult of RT:512 for caller-chosen pixels ------
 * Added within ABI 203: these two exports are additive; no existing struct, field or entry point changed.
 * What turns a camera into hits on the device: the primary hits of a still that is relit afterwards (xrt_shade_hits, xrt_light_hits), a G-buffer,
 * the triangle under the mouse, depth or ids for compositing, a training batch of pixels.  Nothing is shaded and the call takes no lights.
 *   - centres as for xrt_render_pixels: entry i is (centers[2i], centers[2i + 1]), any float is legal, duplicates too.
 *   - opts->use_multisampling: XRT_MS_OFF (samples = 1) or XRT_MS_FIXED16 (samples = 16: the sixteen level-1 positions exactly as
 *     xrt_render_pixels takes them).  Record i * samples + s is sample s of entry i.  XRT_MS_ADAPTIVE is XRT_E_INVALID_ARG: its quadrants
 *     depend on colours -- list the sample positions as centres instead.
 *   - rays_out[r] (nullable, n * samples): o = the unprojected near point, d = the normalised direction, bit for bit the ray xrt_render_pixels
 *     casts; ignore_mesh = ignore_tri = -1.
 *   - hits_out[r] (nullable, n * samples): the record xrt_scene_intersect gives for rays_out[r], field for field; `reserved` is scheduling
 *     feedback and not part of the answer.  A ray that cannot reach the scene's root box gets the miss record: hit 0; object, mesh, tri,
 *     leaf -1; u, v, d, wx, wy, wz 0.0f.
 *   - either output may be NULL, not both.  With hits_out == NULL nothing is traced (intersect_launches == 0): the call is then the list and
 *     device form of xrt_generate_primary_rays.
 *   - opts->list_order: XRT_LIST_COHERENT says consecutive centres are neighbours on screen; the list is then traced as generation 0 of a plain
 *     frame of the same scene and sampling would be -- the rays are generated where they are compacted, rays that cannot reach the root box are
 *     answered there and never traced, the live ones go to the kernel a frame's launch #0 takes (XRT_PACKET overrides as always; materials do not
 *     enter: a closest-hit query has no ray tree), with the packet table a frame writes (xrt_debug_packet_table reports the table of a hinted
 *     one-chunk call).  Scheduling only: both outputs and the counters are bit for bit those of the unhinted call, also for a scrambled list.
 *     A packet is 64 consecutive entries (4 with sixteen samples): a list in compact blocks of the screen (8x8 pixels) costs what a frame's primary
 *     rays cost, a row-major list more (64x1 strips), a scattered one more than the unhinted call.
 *   - opts fields read: use_multisampling, list_order, collect_stats, and shard_count / n_gpus (must be 0 or 1).  Everything else is ignored.
 *     Poses: the latest.  Materials and triangle shading values are not read.
 *   - identities: xrt_shade_hits(rays_out, hits_out, iteration 0, 1.0f) is xrt_render_pixels with XRT_MS_OFF on the same centres, bit for bit in
 *     rgba and rgb_f32; with XRT_MS_FIXED16 the sixteen colours folded by xrt_fold_samples (RT:309) are xrt_render_pixels XRT_MS_FIXED16;
 *     row-major integer centres give xrt_scene_intersect(xrt_generate_primary_rays).
 *   - errors, in this order, also on a host-only scene: NULL scene; n < 0; NULL camera or opts; the opts fields above; a viewport that is not
 *     positive; both outputs NULL with n > 0; NULL centers with n > 0; a non-finite centre (host form: the message names the first one, nothing
 *     is written) -- all XRT_E_INVALID_ARG.  Then n == 0 returns XRT_OK; then XRT_E_NO_DEVICE / XRT_E_NOT_BUILT; then XRT_E_BUSY under the rule
 *     of xrt_render_pixels.
 *   - stats_out (may be NULL): pixels = n; rays_closest = n * samples when hits are asked for; hits_closest; rays_traversed = the rays handed to
 *     a traversal kernel (unhinted: all of them; hinted: the ones that reach the root box); ms_total, ms_intersect, ms_intersect_longest and
 *     intersect_launches over the chunks; with collect_stats the reference work counters (and algorithmic_bytes from them).  Everything else 0.
 *   - a long list is split into chunks under the byte budget of xrt_render_pixels (XRT_PIXEL_BYTES); the answers never depend on the split.
 * Blocking.  There is no begin/end form. */
int xrt_trace_pixels(xrt_scene *scene, const xrt_camera *camera, const xrt_render_opts *opts,
                     const float *centers /* 2 n: x0 y0 x1 y1 .. */, int64_t n,
                     xrt_ray *rays_out /* nullable, n * samples */, xrt_hit *hits_out /* nullable, n * samples */,
                     xrt_stats *stats_out /* nullable */);

/* The same on HBM buffers (d_centers: 2 n floats, d_rays_out: NULL or n * samples xrt_ray, d_hits_out: NULL or n * samples xrt_hit; each 16-byte
 * aligned, else XRT_E_INVALID_ARG -- stated after the errors above), enqueued on `stream` (a hipStream_t; NULL = the scene's stream) and complete
 * when the call returns: the stream is synchronised once per chunk.  Nothing is written at or behind n * samples records.  The centres must be
 * ready on `stream`.  They are not inspected: an entry with a non-finite centre gets unspecified records and affects no other entry. */
int xrt_trace_pixels_device(xrt_scene *scene, const xrt_camera *camera, const xrt_render_opts *opts,
                            const void *d_centers, int64_t n, void *d_rays_out /* nullable */, void *d_hits_out /* nullable */,
                            void *stream, xrt_stats *stats_out /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* XRT_H */
