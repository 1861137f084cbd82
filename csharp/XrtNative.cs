// XrtNative.cs — P/Invoke binding of include/xrt.h for the xna-ray-trace C# host.
// NOT COMPILED HERE: the build image has no .NET toolchain (dotnet / mono / csc absent).  Style follows the
// reference's own native binding precedent (aviFileWrapper_src/Avi.cs:41-185: [StructLayout(Sequential)],
// [DllImport] returning int, wrapper throws on non-zero).
using System;
using System.Runtime.InteropServices;

namespace RayTraceProject.Native
{
    [StructLayout(LayoutKind.Sequential)]
    public struct XrtRay { public float ox, oy, oz, dx, dy, dz; public int ignoreMesh, ignoreTri; }          // 32 B

    [StructLayout(LayoutKind.Sequential)]
    public struct XrtHit { public int hit, obj, mesh, tri, leaf; public float u, v, d, wx, wy, wz; public int reserved; }   // 48 B

    [StructLayout(LayoutKind.Sequential)]
    public struct XrtMaterial
    {
        public float reflectiveness; public int transparent; public float refractionIndex;
        public int interpolateNormals, useTexture, texWidth, texHeight, reserved;
        public IntPtr texArgb;   // BitmapData.Scan0 of the Format32bppArgb lock (Material.cs:65)
        public IntPtr texPArgb;  // Material.Texture.ColorData pinned (RayTracerTexture.cs:24-33: the premultiplied copy GetColorBilinear reads); IntPtr.Zero = same as texArgb
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct XrtCamera
    {
        public fixed float view[16]; public fixed float proj[16];
        public int vpX, vpY, vpWidth, vpHeight; public float vpMinDepth, vpMaxDepth;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct XrtLight
    {
        public int kind; public fixed float position[3]; public fixed float direction[3]; public fixed float color[3];
        public float intensity, spotAngle, decayExponent;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct XrtRenderOpts
    {
        public int maxReflections, useMultisampling, multisampleQuality, addressMode, filtering, shardRank, shardCount, collectStats;
        public int nGpus;                          // > 1: the library spreads the frame's tiles over that many devices and gathers them with RCCL
        public int balanceTiles;                   // with nGpus > 1: 1 = the tiles are dealt by the previous frame's costs (the static counterpart of GetNextScanline, RayTracer.cs:48-52), 0 = round-robin
        public int listOrder;                      // XRT_LIST_*: 0 = nothing is assumed about the order of a list (xrt_render_pixels, xrt_cast_rays*), 1 = consecutive entries are neighbours on screen / in space: traced as a frame would be, same results
        public int reserved;                       // zero
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct XrtNodeInfo                // xrt_scene_get_tree: the private CubeNode (MeshOctree.cs:32-40) flattened, DFS pre-order
    {
        public fixed float bmin[3]; public fixed float bmax[3];
        public int isLeaf, count, dfsIndex, depth, firstRef, reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct XrtPathVertex                     // xrt_path_vertex: VertexPositionColor (Vector3 position, packed Color) -- one end of a segment of RayTracer.points
    {
        public float x, y, z; public uint color;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct XrtSurface                        // xrt_surface, 64 B: what CastRay computes at a hit without asking the scene anything (xrt_surface_hits)
    {
        public float nx, ny, nz;                    // fragmentNormal (RayTracer.cs:520-531)
        public float reflectiveness;                // Material.Reflectiveness (RayTracer.cs:584)
        public float r, g, b;                       // surfaceColor (RayTracer.cs:568-581)
        public float alpha;                         // triangle.color.W (RayTracer.cs:699)
        public float u, v;                          // interpolatedUV (RayTracer.cs:570-572)
        public float refractionIndex, nextRefIndex; // Material.RefractionIndex; n2 of RayTracer.cs:656-667 when Transparent, else currentRefIndex
        public int flags;                           // 1 hit, 2 Transparent, 4 InterpolateNormals, 8 UseTexture
        public int reserved0, reserved1, reserved2;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct XrtStats
    {
        public ulong raysClosest, raysShadow, hitsClosest, hitsShadow, sceneNodeTests, instanceVisits, meshAabbTests, meshQueries,
                     nodeTests, leafRefs, triTests, shadedHits, pixels, algorithmicBytes;
        public double msTotal, msIntersect; public uint intersectLaunches, pieces; public ulong raysTraversed; public double msIntersectLongest; public ulong meshQueriesFacingAway;
    }

    public static class Xrt
    {
        const string Lib = "xrt";   // libxrt.so / xrt.dll
        // include/xrt.h promises cdecl.  The reference builds x86 (RayTraceProject.csproj:47,60), where P/Invoke defaults to StdCall
        // and a cdecl callee would unbalance the stack: every import names its convention.  (The Avi.cs precedent binds Win32
        // stdcall APIs and does not carry over.)
        public const int OK = 0, E_INVALID_ARG = -1, E_BUSY = -2, E_NO_DEVICE = -3;
        public const int LIST_UNORDERED = 0, LIST_COHERENT = 1;   // XrtRenderOpts.listOrder

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_version();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern IntPtr xrt_last_error();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_create(int device, out IntPtr scene);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_destroy(IntPtr scene);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_add_mesh(IntPtr scene, float[] v, float[] n, float[] uv, float[] surfN, float[] color,
                                                                    int ntri, ref XrtMaterial material, float[] bbox, out int meshId);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_add_object(IntPtr scene, int[] meshIds, int nMeshes, float[] world, float[] invWorld,
                                                                      float[] bbox, float[] worldBbox, out int objectId);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_build(IntPtr scene, int meshThreshold, int sceneThreshold);
        // scene file: the content-pipeline step writes it once (instead of .xnb reflection serialisation of Model.Tag), the game loads it
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_save(IntPtr scene, [MarshalAs(UnmanagedType.LPStr)] string path);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_load(int device, [MarshalAs(UnmanagedType.LPStr)] string path, out IntPtr scene);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_intersect(IntPtr scene, [In] XrtRay[] rays, int[] ignoreObject, long n,
                                                                     [Out] XrtHit[] hits, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern unsafe int xrt_render(IntPtr scene, ref XrtCamera camera, XrtLight[] lights, int nLights,
                                                                   ref XrtRenderOpts opts, uint* rgbaOut, float* rgbF32Out, IntPtr stats);
        // pipelined form (two frames in flight; device output): RenderAsync / RenderCompleted without a host round trip
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_render_device_begin(IntPtr scene, ref XrtCamera camera, XrtLight[] lights, int nLights,
                                                                            ref XrtRenderOpts opts, IntPtr dRgbaOut, IntPtr stream, out int ticket);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_render_device_end(IntPtr scene, int ticket, IntPtr statsOut);
        // pipelined form with the frame ending in the host's Color[] (RenderAsync + CurrentTarget.SetData, RayTracer.cs:59-79,122-123):
        // pin renderTargetData (GCHandle.Alloc(.., GCHandleType.Pinned)) and xrt_host_register it once; up to two tickets open
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_render_begin(IntPtr scene, ref XrtCamera camera, XrtLight[] lights, int nLights,
                                                                     ref XrtRenderOpts opts, IntPtr rgbaOut, out int ticket);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_render_end(IntPtr scene, int ticket, IntPtr statsOut);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_host_register(IntPtr hostPtr, ulong bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_host_unregister(IntPtr hostPtr);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern float xrt_progress(IntPtr scene);
        // ---- the rest of include/xrt.h (every export is bound: tests/test_host_logic.py checks this file against the header) ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_device_count(out int count);
        // inspection of the built trees (meshId -1: the scene octree); call with null arrays for the counts
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_get_tree(IntPtr scene, int meshId, [Out] XrtNodeInfo[] nodes, ref long nNodes,
                                                                    [Out] int[] refs, ref long nRefs);
        // seam 1 with HBM-resident rays / hits (device pointers, asynchronous on `stream`), and MeshOctree.GetRayIntersection of one mesh (MeshOctree.cs:259-326)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_intersect_device(IntPtr scene, IntPtr dRays, long n, IntPtr dHitsOut, IntPtr stream);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_mesh_intersect(IntPtr scene, int meshId, [In] XrtRay[] rays, long n, [Out] XrtHit[] hits);
        // blocking frame into device memory (or this process's tile shard)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_render_device(IntPtr scene, ref XrtCamera camera, XrtLight[] lights, int nLights,
                                                                      ref XrtRenderOpts opts, IntPtr dRgbaOut, IntPtr stream, IntPtr statsOut);
        // image-tile shards (one process per GPU): layout, de-tile of the gathered buffers
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_shard_layout(int width, int height, int shardCount, out int tilesX, out int tilesY, out int tilesPerRank);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_detile_device(int width, int height, int shardCount, IntPtr dGathered, long rankStride,
                                                                      IntPtr dRgbaOut, IntPtr stream);
        // cost-aware tile assignment: the previous frame's tile costs -> a longest-first table -> installed for the next frames
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_tile_table(IntPtr scene, int width, int height, int shardCount, int tilesPerRank, int[] tileOfSlot);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_tile_costs(IntPtr scene, int width, int height, [Out] float[] costOut, int reset);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_balance_tiles(int width, int height, int shardCount, float[] tileCost, int tilesPerRank, [Out] int[] tileOfSlotOut);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_detile_table_device(int width, int height, int shardCount, int tilesPerRank, IntPtr dTileOfSlot,
                                                                            IntPtr dGathered, long rankStride, IntPtr dRgbaOut, IntPtr stream);
        // the primary rays of RayTracer.Render (RayTracer.cs:410-421), row-major
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_generate_primary_rays(IntPtr scene, ref XrtCamera camera, [Out] XrtRay[] raysOut);
        // RayTracer.CastRay (RT:506) on caller-given rays, one recursion each (additive within ABI 203); INTEGRATION.md shows the n = 1 forwarding
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern unsafe int xrt_cast_rays(IntPtr scene, [In] XrtRay[] rays, long n, int iteration, float currentRefIndex,
                                                                      XrtLight[] lights, int nLights, ref XrtRenderOpts opts, uint* rgbaOut, float* rgbF32Out, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_cast_rays_device(IntPtr scene, IntPtr dRays, long n, int iteration, float currentRefIndex,
                                                                      XrtLight[] lights, int nLights, ref XrtRenderOpts opts, IntPtr dRgbaOut, IntPtr dRgbF32Out, IntPtr stream, IntPtr stats);
        // ... with RayTracer.points (RT:543, 701: the segments every call appends, vertices[vertexStart[i] .. vertexStart[i + 1]) for ray i) and the ray as CastRay leaves its
        // `ref Ray ray` (RT:692-694).  nVerticesOut is what the batch needs; a capacity that is too small is not an error (the first whole segments are written)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern unsafe int xrt_cast_rays_paths(IntPtr scene, [In] XrtRay[] rays, long n, int iteration, float currentRefIndex,
                                                                      XrtLight[] lights, int nLights, ref XrtRenderOpts opts, uint* rgbaOut, float* rgbF32Out, [Out] XrtRay[] raysBack,
                                                                      [Out] long[] vertexStart, [Out] XrtPathVertex[] vertices, long vertexCapacity, out long nVerticesOut, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_cast_rays_paths_device(IntPtr scene, IntPtr dRays, long n, int iteration, float currentRefIndex,
                                                                      XrtLight[] lights, int nLights, ref XrtRenderOpts opts, IntPtr dRgbaOut, IntPtr dRgbF32Out, IntPtr dRaysBack,
                                                                      IntPtr dVertexStart, IntPtr dVertices, long vertexCapacity, IntPtr stream, out long nVerticesOut, IntPtr stats);
        // what CastRay does with an IntersectionResult (RT:514-737) on caller-given hits: hits[i] stands for the query of rays[i] (RT:512), nothing is traced for the
        // first level -- relighting or re-materialing a still whose hits are known (additive within ABI 203)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern unsafe int xrt_shade_hits(IntPtr scene, [In] XrtRay[] rays, [In] XrtHit[] hits, long n, int iteration, float currentRefIndex,
                                                                      XrtLight[] lights, int nLights, ref XrtRenderOpts opts, uint* rgbaOut, float* rgbF32Out, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_shade_hits_device(IntPtr scene, IntPtr dRays, IntPtr dHits, long n, int iteration, float currentRefIndex,
                                                                      XrtLight[] lights, int nLights, ref XrtRenderOpts opts, IntPtr dRgbaOut, IntPtr dRgbF32Out, IntPtr stream, IntPtr stats);
        // CastRay's light loop alone (RT:534-542) on caller-given hits: per hit the fp32 light sum (3 floats) and / or IsLightPathObstructed's amount per
        // light (RT:465-502), nothing quantised; either output may be null, not both (additive within ABI 203)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_light_hits(IntPtr scene, [In] XrtHit[] hits, long n, XrtLight[] lights, int nLights,
                                                                      [Out] float[] lightF32Out, [Out] float[] amountOut, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_light_hits_device(IntPtr scene, IntPtr dHits, long n, XrtLight[] lights, int nLights,
                                                                      IntPtr dLightF32Out, IntPtr dAmountOut, IntPtr stream, IntPtr stats);
        // What CastRay computes at a hit without asking the scene anything: the surface record, the reflected ray (RT:547-559) and the Snell refraction
        // (RT:656-694) of caller-given hits; rays may be null without a ray output; any output may be null, not all three (additive within ABI 203)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_surface_hits(IntPtr scene, [In] XrtRay[] rays, [In] XrtHit[] hits, long n, float currentRefIndex,
                                                                      ref XrtRenderOpts opts, [Out] XrtSurface[] surfaceOut, [Out] XrtRay[] reflectOut, [Out] XrtRay[] refractOut, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_surface_hits_device(IntPtr scene, IntPtr dRays, IntPtr dHits, long n, float currentRefIndex,
                                                                      ref XrtRenderOpts opts, IntPtr dSurfaceOut, IntPtr dReflectOut, IntPtr dRefractOut, IntPtr stream, IntPtr stats);
        // The way back up CastRay, one level: RT:726 (reflectRgba null), RT:584, RT:699 (refractRgba given, Transparent entries), RT:732 for an entry
        // without XRT_SURF_HIT, RT:705 -- from xrt_surface_hits records, xrt_light_hits sums and the packed colours of the nested calls; either
        // output may be null, not both.  And RT:309: the mean of 4 colours, or of four such means (samples 16).  (additive within ABI 203)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_compose_hits(IntPtr scene, [In] XrtSurface[] surface, [In] float[] lightF32, [In] uint[] reflectRgba,
                                                                      [In] uint[] refractRgba, long n, [Out] uint[] rgbaOut, [Out] float[] rgbF32Out, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_compose_hits_device(IntPtr scene, IntPtr dSurface, IntPtr dLightF32, IntPtr dReflectRgba,
                                                                      IntPtr dRefractRgba, long n, IntPtr dRgbaOut, IntPtr dRgbF32Out, IntPtr stream, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_fold_samples(IntPtr scene, [In] uint[] rgbaIn, long n, int samples, [Out] uint[] rgbaOut,
                                                                      [Out] float[] rgbF32Out, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_fold_samples_device(IntPtr scene, IntPtr dRgbaIn, long n, int samples, IntPtr dRgbaOut,
                                                                      IntPtr dRgbF32Out, IntPtr stream, IntPtr stats);
        // SceneObject.Position / Rotation / Scale (SO:51-88) between frames: the dirty bodies' World / InverseWorld / WorldBoundingBox
        // (16 + 16 + 6 floats per id), also while RenderAsync tickets are open; the scene octree stays until xrt_scene_build_tree
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_poses(IntPtr scene, [In] int[] objectIds, int n,
                                                                     [In] float[] world, [In] float[] invWorld, [In] float[] worldBbox);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_poses_device(IntPtr scene, IntPtr dObjectIds, int n,
                                                                     IntPtr dWorld, IntPtr dInvWorld, IntPtr dWorldBbox, IntPtr stream);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_build_tree(IntPtr scene, int sceneThreshold);
        // Material.Reflectiveness / Transparent / RefractionIndex / InterpolateNormals / UseTexture / Texture (Material.cs:39, 234-268) between frames: mesh
        // meshIds[i] takes materials[i], also while RenderAsync tickets are open; texArgb == IntPtr.Zero keeps the texels the mesh has; nothing is rebuilt
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_materials(IntPtr scene, [In] int[] meshIds, int n,
                                                                     [In] XrtMaterial[] materials);
        // OctreeSpatialManager.Bodies replaced and Build() run on a built scene (OctreeSpatialManager.cs:54-57, 64-99): body i has the meshes
        // meshIds[meshStart[i] .. meshStart[i + 1]) and 16 + 16 + 6 + 6 floats; meshes added since the last build get their octrees (their number
        // comes back in meshesBuilt), no other mesh octree is built again
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_bodies(IntPtr scene, int nBodies, [In] int[] meshStart,
                                                                     [In] int[] meshIds, [In] float[] world, [In] float[] invWorld, [In] float[] bbox,
                                                                     [In] float[] worldBbox, int sceneThreshold, out int meshesBuilt);
        // Triangle.n1..n3 / uv1..uv3 / color (Triangle.cs:17-23) between frames: entry i edits triangle triIds[i] of the mesh (triIds null: firstTri + i)
        // with 9 + 6 + 4 floats; a null array leaves that field; also while RenderAsync tickets are open; surfaceNormal and vertices are not settable
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_triangle_shading(IntPtr scene, int meshId, [In] int[] triIds,
                                                                     int firstTri, int n, [In] float[] normals, [In] float[] uv, [In] float[] color);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_triangle_shading_device(IntPtr scene, int meshId, IntPtr dTriIds,
                                                                     int firstTri, int n, IntPtr dNormals, IntPtr dUv, IntPtr dColor, IntPtr stream);
        // Mesh.Triangles / Mesh.MeshBoundingBox set and Mesh.Init() run on a built scene (Mesh.cs:12-14, 27-32): the mesh takes nTri triangles (the arrays of
        // xrt_scene_add_mesh) under its id and with its material; its MeshOctree alone is built (MeshOctree.cs:56-96); nTri = 0 empties the mesh
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_scene_set_mesh_triangles(IntPtr scene, int meshId, [In] float[] v,
                                                                     [In] float[] n, [In] float[] uv, [In] float[] surfN, [In] float[] color, int nTri, [In] float[] bbox);
        // GetColorForQuadrant / the body of Render's inner loop (RayTracer.cs:215-311, 412-425) on a list of screen positions (centers: x0 y0 x1 y1 ..): the colour
        // of every entry in the caller's order, all three multisampling modes; an integer centre gets the frame's pixel bit for bit
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern unsafe int xrt_render_pixels(IntPtr scene, ref XrtCamera camera, XrtLight[] lights, int nLights,
                                                                     ref XrtRenderOpts opts, [In] float[] centers, long n, uint* rgbaOut, float* rgbF32Out, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_render_pixels_device(IntPtr scene, ref XrtCamera camera, XrtLight[] lights, int nLights,
                                                                     ref XrtRenderOpts opts, IntPtr dCenters, long n, IntPtr dRgbaOut, IntPtr dRgbF32Out, IntPtr stream, IntPtr stats);
        // The first level of xrt_render_pixels alone: per listed screen position the ray of RayTracer.cs:412-421 and the IntersectionResult of RayTracer.cs:512,
        // nothing shaded, no lights; XRT_MS_OFF or XRT_MS_FIXED16 (16 records per centre); either output may be null, not both (additive within ABI 203)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_trace_pixels(IntPtr scene, ref XrtCamera camera, ref XrtRenderOpts opts, [In] float[] centers, long n,
                                                                     [Out] XrtRay[] raysOut, [Out] XrtHit[] hitsOut, IntPtr stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_trace_pixels_device(IntPtr scene, ref XrtCamera camera, ref XrtRenderOpts opts, IntPtr dCenters, long n,
                                                                     IntPtr dRaysOut, IntPtr dHitsOut, IntPtr stream, IntPtr stats);
        // can n_gpus > 1 load RCCL?  OK or E_RCCL (-6) with the loader's message; no device is touched
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_rccl_probe();
        // diagnostics of the split walks of long packets (results never depend on them): subtrees handed over, taken, packets split, packets written by a taker
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_split_stats(IntPtr scene, [Out] ulong[] out4, int reset);
        // diagnostics of "end early" (results never depend on it): the last frame's paths coloured by the ray generation kernel, by the shading kernel, left to the compose list
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_debug_end_counts(IntPtr scene, [Out] ulong[] out3);
        // diagnostics of the primary packets (results never depend on them): the last one-chunk frame's packet table (first slot, rays per packet) and its live list
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_debug_packet_table(IntPtr scene, [Out] ulong[] counts2, [Out] uint[] entriesOut, long entriesCap,
                                                                     [Out] int[] pathsOut, long pathsCap);
        // diagnostics of the screen boxes (results never depend on them): the last one-chunk frame's table, two words per leaf reference (x0 | x1 << 16, y0 | y1 << 16)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int xrt_debug_screen_table(IntPtr scene, int hostEval, out ulong count, [Out] uint[] entriesOut, long entriesCap);

        // error convention of the reference: InvalidOperationException when busy (RayTracer.cs:26-27,62-63),
        // ArgumentException for bad arguments (SceneObject.cs:123-124, Material.cs:85,97)
        public static void Check(int rc)
        {
            if (rc == OK) return;
            string msg = Marshal.PtrToStringAnsi(xrt_last_error());
            if (rc == E_BUSY) throw new InvalidOperationException(msg);
            if (rc == E_INVALID_ARG) throw new ArgumentException(msg);
            throw new Exception("Exception in libxrt: " + rc + " " + msg);
        }
    }
}
