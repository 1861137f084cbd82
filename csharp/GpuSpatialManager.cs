// GpuSpatialManager.cs — ISpatialManager (Spatial/ISpatialManager.cs:10-16) implemented on libxrt.
// NOT COMPILED HERE (no .NET toolchain in the build image).  Drop next to OctreeSpatialManager.cs and assign
// `tracer.CurrentScene = new GpuSpatialManager()` in Game1.LoadContent (Game1.cs:96,123).
using System;
using System.Collections.Generic;
using Microsoft.Xna.Framework;
using RayTracerTypeLibrary;
using RayTraceProject.Native;

namespace RayTraceProject.Spatial
{
    class GpuSpatialManager : ISpatialManager, IDisposable
    {
        readonly List<ISpatialBody> objects = new List<ISpatialBody>();
        readonly Dictionary<Mesh, int> meshIds = new Dictionary<Mesh, int>();
        readonly List<Mesh> meshesById = new List<Mesh>();
        IntPtr scene;

        public List<ISpatialBody> Bodies { get { return this.objects; } }
        public IntPtr Handle { get { return this.scene; } }

        static float[] M(Matrix m)
        {
            return new float[] { m.M11, m.M12, m.M13, m.M14, m.M21, m.M22, m.M23, m.M24, m.M31, m.M32, m.M33, m.M34, m.M41, m.M42, m.M43, m.M44 };
        }
        static float[] B(BoundingBox b) { return new float[] { b.Min.X, b.Min.Y, b.Min.Z, b.Max.X, b.Max.Y, b.Max.Z }; }

        // OctreeSpatialManager.Build (OctreeSpatialManager.cs:64-99) + Mesh.Init of every distinct mesh (SceneObject.cs:132).  The first Build
        // makes the scene; a later one on the scene of this manager's own Build only replaces the body list (xrt_scene_set_bodies): meshes the
        // library has keep their ids and octrees, meshes it has not seen are added and built by the call.  LastBuildMeshes: mesh octrees built.
        public int LastBuildMeshes { get; private set; }
        bool ownBuild;   // the scene was made by Build(), not by Load(): meshIds knows its meshes

        public void Build()
        {
            if (this.scene != IntPtr.Zero && this.ownBuild)
            {
                PushMaterials();
                foreach (SceneObject so in this.objects)
                    foreach (Mesh mesh in so.Meshes)
                        if (!this.meshIds.ContainsKey(mesh)) AddMesh(mesh);
                int n = this.objects.Count, k = 0;
                int[] start = new int[n + 1];
                for (int i = 0; i < n; i++) start[i + 1] = start[i] + ((SceneObject)this.objects[i]).Meshes.Count;
                int[] all = new int[Math.Max(start[n], 1)];
                float[] world = new float[16 * n], inv = new float[16 * n], bbox = new float[6 * n], wbb = new float[6 * n];
                for (int i = 0; i < n; i++)
                {
                    SceneObject so = (SceneObject)this.objects[i];
                    foreach (Mesh mesh in so.Meshes) all[k++] = this.meshIds[mesh];
                    M(so.World).CopyTo(world, 16 * i); M(so.InverseWorld).CopyTo(inv, 16 * i);
                    B(so.BoundingBox).CopyTo(bbox, 6 * i); B(so.WorldBoundingBox).CopyTo(wbb, 6 * i);
                }
                int built;
                Xrt.Check(Xrt.xrt_scene_set_bodies(this.scene, n, start, all, world, inv, bbox, wbb, 0, out built));
                this.LastBuildMeshes = built;
                return;
            }
            if (this.scene != IntPtr.Zero) Xrt.Check(Xrt.xrt_scene_destroy(this.scene));
            Xrt.Check(Xrt.xrt_scene_create(0, out this.scene));
            this.ownBuild = false;
            this.meshIds.Clear(); this.meshesById.Clear();
            foreach (SceneObject so in this.objects)
                foreach (Mesh mesh in so.Meshes)
                    if (!this.meshIds.ContainsKey(mesh)) AddMesh(mesh);          // meshes are shared by reference (SceneObject.cs:126-127)
            foreach (SceneObject so in this.objects)
            {
                int[] ids = new int[so.Meshes.Count];
                for (int i = 0; i < ids.Length; i++) ids[i] = this.meshIds[so.Meshes[i]];
                int oid;
                Xrt.Check(Xrt.xrt_scene_add_object(this.scene, ids, ids.Length, M(so.World), M(so.InverseWorld), B(so.BoundingBox),
                                                   B(so.WorldBoundingBox), out oid));
            }
            Xrt.Check(Xrt.xrt_scene_build(this.scene, 0, 0));   // thresholds 50 / 20 (MeshOctree.cs:42, OctreeSpatialManager.cs:50)
            this.ownBuild = true;
            this.LastBuildMeshes = this.meshesById.Count;
        }

        // xrt_scene_add_mesh for a mesh the library has not seen
        void AddMesh(Mesh mesh)
        {
            Triangle[] t = mesh.Triangles;
            float[] v = new float[t.Length * 9], n = new float[t.Length * 9], uv = new float[t.Length * 6],
                    sn = new float[t.Length * 3], col = new float[t.Length * 4];
            for (int i = 0; i < t.Length; i++)
            {
                Put3(v, i * 9, t[i].v1); Put3(v, i * 9 + 3, t[i].v2); Put3(v, i * 9 + 6, t[i].v3);
                Put3(n, i * 9, t[i].n1); Put3(n, i * 9 + 3, t[i].n2); Put3(n, i * 9 + 6, t[i].n3);
                uv[i * 6] = t[i].uv1.X; uv[i * 6 + 1] = t[i].uv1.Y; uv[i * 6 + 2] = t[i].uv2.X; uv[i * 6 + 3] = t[i].uv2.Y;
                uv[i * 6 + 4] = t[i].uv3.X; uv[i * 6 + 5] = t[i].uv3.Y;
                Put3(sn, i * 3, t[i].surfaceNormal);
                col[i * 4] = t[i].color.X; col[i * 4 + 1] = t[i].color.Y; col[i * 4 + 2] = t[i].color.Z; col[i * 4 + 3] = t[i].color.W;
            }
            Material mat = mesh.MeshMaterial;
            XrtMaterial xm = new XrtMaterial
            {
                reflectiveness = mat.Reflectiveness, transparent = mat.Transparent ? 1 : 0, refractionIndex = mat.RefractionIndex,
                interpolateNormals = mat.InterpolateNormals ? 1 : 0, useTexture = mat.UseTexture ? 1 : 0,
                // Material.Init (Material.cs:59-69) keeps the locked bitmap in private fields; expose Scan0 / Width / Height
                // through three internal getters on Material (one-line additions) and pass them here:
                texWidth = mat.UseTexture ? mat.TextureWidth : 0, texHeight = mat.UseTexture ? mat.TextureHeight : 0,
                texArgb = mat.UseTexture ? mat.TextureScan0 : IntPtr.Zero
            };
            // the bilinear filter reads Material.Texture.ColorData, the premultiplied Format32bppPArgb copy (RayTracerTexture.cs:24-33,
            // Material.cs:186-189): pinned for the call (the library copies it)
            System.Runtime.InteropServices.GCHandle pin = default(System.Runtime.InteropServices.GCHandle);
            if (mat.UseTexture && mat.Texture != null && mat.Texture.ColorData != null)
            {
                pin = System.Runtime.InteropServices.GCHandle.Alloc(mat.Texture.ColorData, System.Runtime.InteropServices.GCHandleType.Pinned);
                xm.texPArgb = pin.AddrOfPinnedObject();
            }
            int id;
            try { Xrt.Check(Xrt.xrt_scene_add_mesh(this.scene, v, n, uv, sn, col, t.Length, ref xm, B(mesh.MeshBoundingBox), out id)); }
            finally { if (pin.IsAllocated) pin.Free(); }
            this.meshIds[mesh] = id; this.meshesById.Add(mesh);
        }

        // Scene file (what the content pipeline would write instead of .xnb reflection data, TracerModelProcessor.cs:113-117):
        // Save after Build(); Load replaces Build() at start-up (Bodies stays as the game filled it: object ids follow its order).
        public void Save(string path) { Xrt.Check(Xrt.xrt_scene_save(this.scene, path)); }
        public void Load(string path)
        {
            if (this.scene != IntPtr.Zero) Xrt.Check(Xrt.xrt_scene_destroy(this.scene));
            Xrt.Check(Xrt.xrt_scene_load(0, path, out this.scene));
            this.ownBuild = false;
            Xrt.Check(Xrt.xrt_scene_build(this.scene, 0, 0));
        }

        // Material's setters (Material.cs:39, 234-268) between frames: the scalar properties of every mesh's material in one xrt_scene_set_materials,
        // before the next RenderAsync (tickets may be open; nothing is rebuilt).  texArgb stays IntPtr.Zero: the library keeps the texels it was given
        // by Build().  A host that assigns Material.Texture passes the new lock's Scan0 / Width / Height (and the pinned ColorData) for that mesh
        // instead, as Build() does.
        public void PushMaterials()
        {
            if (this.scene == IntPtr.Zero || this.meshesById.Count == 0) return;
            int[] ids = new int[this.meshesById.Count];
            XrtMaterial[] mats = new XrtMaterial[ids.Length];
            for (int i = 0; i < ids.Length; i++)
            {
                Material mat = this.meshesById[i].MeshMaterial;
                ids[i] = i;
                mats[i] = new XrtMaterial
                {
                    reflectiveness = mat.Reflectiveness, transparent = mat.Transparent ? 1 : 0, refractionIndex = mat.RefractionIndex,
                    interpolateNormals = mat.InterpolateNormals ? 1 : 0, useTexture = mat.UseTexture ? 1 : 0
                };
            }
            Xrt.Check(Xrt.xrt_scene_set_materials(this.scene, ids, ids.Length, mats));
        }

        // Triangle.n1..n3 / uv1..uv3 / color (Triangle.cs:17-23) between frames: a host that wrote these fields of mesh.Triangles[first .. first + count)
        // -- scrolled UVs, painted colours, the highlight of the triangle a click hit (Game1.cs:296-325), a faded alpha -- calls this before the next
        // RenderAsync (tickets may be open; nothing is rebuilt).  There is no change detection on public fields: nothing is pushed unless the host asks.
        // surfaceNormal and the vertices are not settable this way: a mesh whose geometry changed is pushed with PushMeshTriangles.
        public void PushTriangleShading(Mesh mesh, int first, int count)
        {
            if (this.scene == IntPtr.Zero || count <= 0) return;
            Triangle[] t = mesh.Triangles;
            float[] n = new float[count * 9], uv = new float[count * 6], col = new float[count * 4];
            for (int k = 0; k < count; k++)
            {
                int i = first + k;
                Put3(n, k * 9, t[i].n1); Put3(n, k * 9 + 3, t[i].n2); Put3(n, k * 9 + 6, t[i].n3);
                uv[k * 6] = t[i].uv1.X; uv[k * 6 + 1] = t[i].uv1.Y; uv[k * 6 + 2] = t[i].uv2.X; uv[k * 6 + 3] = t[i].uv2.Y;
                uv[k * 6 + 4] = t[i].uv3.X; uv[k * 6 + 5] = t[i].uv3.Y;
                col[k * 4] = t[i].color.X; col[k * 4 + 1] = t[i].color.Y; col[k * 4 + 2] = t[i].color.Z; col[k * 4 + 3] = t[i].color.W;
            }
            Xrt.Check(Xrt.xrt_scene_set_triangle_shading(this.scene, this.meshIds[mesh], null, first, count, n, uv, col));
        }
        public void PushTriangleShading(Mesh mesh) { PushTriangleShading(mesh, 0, mesh.Triangles.Length); }

        // Mesh.Init() (Mesh.cs:27-32) on a mesh of the built scene: a host that assigned mesh.Triangles (or moved v1..v3 / surfaceNormal of its triangles) and
        // mesh.MeshBoundingBox calls this where the reference calls mesh.Init().  The mesh keeps its id and its material, its MeshOctree alone is built, the
        // body list and the scene octree stay (xrt_scene_set_mesh_triangles).  Not while RenderAsync tickets are open.  No change detection: nothing is pushed
        // unless the host asks.
        public void PushMeshTriangles(Mesh mesh)
        {
            if (this.scene == IntPtr.Zero) return;
            Triangle[] t = mesh.Triangles;
            int count = t.Length;
            float[] v = new float[count * 9 + 1], n = new float[count * 9 + 1], uv = new float[count * 6 + 1], sn = new float[count * 3 + 1], col = new float[count * 4 + 1];
            for (int i = 0; i < count; i++)
            {
                Put3(v, i * 9, t[i].v1); Put3(v, i * 9 + 3, t[i].v2); Put3(v, i * 9 + 6, t[i].v3);
                Put3(n, i * 9, t[i].n1); Put3(n, i * 9 + 3, t[i].n2); Put3(n, i * 9 + 6, t[i].n3);
                uv[i * 6] = t[i].uv1.X; uv[i * 6 + 1] = t[i].uv1.Y; uv[i * 6 + 2] = t[i].uv2.X; uv[i * 6 + 3] = t[i].uv2.Y;
                uv[i * 6 + 4] = t[i].uv3.X; uv[i * 6 + 5] = t[i].uv3.Y;
                Put3(sn, i * 3, t[i].surfaceNormal);
                col[i * 4] = t[i].color.X; col[i * 4 + 1] = t[i].color.Y; col[i * 4 + 2] = t[i].color.Z; col[i * 4 + 3] = t[i].color.W;
            }
            BoundingBox b = mesh.MeshBoundingBox;
            float[] bbox = { b.Min.X, b.Min.Y, b.Min.Z, b.Max.X, b.Max.Y, b.Max.Z };
            Xrt.Check(Xrt.xrt_scene_set_mesh_triangles(this.scene, this.meshIds[mesh], v, n, uv, sn, col, count, bbox));
        }

        static void Put3(float[] a, int o, Vector3 p) { a[o] = p.X; a[o + 1] = p.Y; a[o + 2] = p.Z; }

        // Batched form used by a wavefront renderer.
        public void IntersectBatch(XrtRay[] rays, XrtHit[] hits)
        {
            Xrt.Check(Xrt.xrt_scene_intersect(this.scene, rays, null, rays.Length, hits, IntPtr.Zero));
        }

        // The colours of caller-chosen screen positions (centers: x0 y0 x1 y1 ..) -- GetColorForQuadrant / the body of Render's inner loop
        // (RayTracer.cs:215-311, 412-425) for each, by the camera, lights and options of a frame: the rectangle an edit touched, a progressive
        // preview's every 16th pixel, the pixel under the mouse.  colors[i] is the packed Color of entry i (Color.PackedValue).
        public unsafe void RenderPixels(ref XrtCamera camera, XrtLight[] lights, ref XrtRenderOpts opts, float[] centers, uint[] colors)
        {
            fixed (uint* c = colors)
                Xrt.Check(Xrt.xrt_render_pixels(this.scene, ref camera, lights, lights == null ? 0 : lights.Length, ref opts, centers, colors.Length, c, null, IntPtr.Zero));
        }

        // The primary rays and closest hits of caller-chosen screen positions -- RayTracer.cs:412-421 and the GetRayIntersection of RayTracer.cs:512 for each,
        // nothing shaded: the picking seam (the triangle under the mouse, Game1.cs:296-325, is TracePixels on one centre; hits[0].mesh / .tri name it),
        // the primary hits of a still that is relit afterwards (Game1.cs:152-190: xrt_shade_hits / IsLightPathObstructedBatch on these hits), a G-buffer.
        // rays / hits: either may be null, not both; with opts.useMultisampling = 2 (the fixed sixteen) each holds 16 records per centre.
        public void TracePixels(ref XrtCamera camera, ref XrtRenderOpts opts, float[] centers, XrtRay[] rays, XrtHit[] hits)
        {
            Xrt.Check(Xrt.xrt_trace_pixels(this.scene, ref camera, ref opts, centers, centers.Length / 2, rays, hits, IntPtr.Zero));
        }

        // RayTracer.IsLightPathObstructed (RayTracer.cs:465-502) for every (hit, light) pair of a batch: amounts[i * lights.Length + l] is what the
        // reference returns for hits[i] and lights[l] -- 0 for a free path, 1 for an obstructed one, color.W of a Transparent blocker -- and 0 for an
        // entry whose hit word is 0.  One call and one float per shadow ray, where IntersectBatch on host-formed shadow rays moves an XrtRay in and a
        // 48-byte XrtHit out for each.  lightSums (nullable, 3 floats per hit) receives the unquantised light sum of RayTracer.cs:534-542.
        public void IsLightPathObstructedBatch(XrtHit[] hits, XrtLight[] lights, float[] amounts, float[] lightSums = null)
        {
            Xrt.Check(Xrt.xrt_light_hits(this.scene, hits, hits.Length, lights, lights == null ? 0 : lights.Length, lightSums, amounts, IntPtr.Zero));
        }

        // The single-ray signature of the interface, forwarded as a batch of one (correct, slow: a P/Invoke plus a kernel
        // launch per ray; RayTracer.RenderInternal should call xrt_render instead, see INTEGRATION.md).
        public bool GetRayIntersection(ref Ray ray, out IntersectionResult? result, Triangle ignoreTriangle, Mesh ignoreObject)
        {
            result = null;
            XrtRay[] r = new XrtRay[1];
            r[0].ox = ray.Position.X; r[0].oy = ray.Position.Y; r[0].oz = ray.Position.Z;
            r[0].dx = ray.Direction.X; r[0].dy = ray.Direction.Y; r[0].dz = ray.Direction.Z;
            r[0].ignoreMesh = -1; r[0].ignoreTri = -1;
            if (ignoreTriangle != null)
                foreach (KeyValuePair<Mesh, int> kv in this.meshIds)   // reference identity -> (mesh id, index in Mesh.Triangles[])
                {
                    int idx = Array.IndexOf(kv.Key.Triangles, ignoreTriangle);
                    if (idx >= 0) { r[0].ignoreMesh = kv.Value; r[0].ignoreTri = idx; break; }
                }
            XrtHit[] h = new XrtHit[1];
            IntersectBatch(r, h);
            if (h[0].hit == 0) return false;
            Mesh mesh = this.meshesById[h[0].mesh];
            result = new IntersectionResult(mesh, mesh.Triangles[h[0].tri], h[0].u, h[0].v, h[0].d, new Vector3(h[0].wx, h[0].wy, h[0].wz));
            return true;
        }

        public void Dispose()
        {
            if (this.scene != IntPtr.Zero) { Xrt.xrt_scene_destroy(this.scene); this.scene = IntPtr.Zero; }
        }
    }
}
