// scene_host.h — host representation of one xrt_scene: the uploaded Mesh / SceneObject graph
// (xrt_scene_add_mesh / xrt_scene_add_object) and, after build(), the flat arrays that go to HBM.
// Plain C++ (no HIP).
#pragma once
#include <string>
#include <vector>

#include "scene_build.h"
#include "traverse.h"

namespace xrt {

constexpr int SHADE_F4 = 6;   // f4 per triangle shading record:
//   s0 = (n1.xyz, uv1.x) s1 = (n2.xyz, uv1.y) s2 = (n3.xyz, uv2.x) s3 = color.xyzw
//   s4 = (uv2.y, uv3.x, uv3.y, as_float(material))  s5 = (surfaceNormal.xyz, as_float(mesh))

struct SceneArrays {
    std::vector<f4> blocks, refN, snodes, shade, leafNB;   // leafNB: 2 per node: component-wise min / max of the leaf's surface normals
    std::vector<float> refT;                               // refN + refG as one 13-word record per reference, 16 words of padding at the end
    std::vector<f4> runTB;                                 // 4 per run of LEAF_RUN references of a big leaf: the run's tight box (same record as leafTB)
    std::vector<int> runBase;                              // per node: index of the leaf's first run in runTB / 4, or -1 (small leaf, interior, empty)
    std::vector<f4> scull;                                 // 4 per scene leaf reference (traverse.h SceneView::scull)
    std::vector<int> scullPosStart, scullPos;              // body o's records in scull: positions scullPos[scullPosStart[o] .. scullPosStart[o + 1])
    std::vector<f4> leafTB;                                // 4 per node: the leaf's tight box (xrt_core.h leaf_certainly_missed)
    std::vector<g3> refG;
    // The wave-packet kernel's copies (packet.hip: everything it walks arrives through scalar loads from THREE arrays -- pblocks, lrec, refT):
    std::vector<float> pblocks;                            // PBLOCK_WORDS per block: descriptor (8 words of `blocks`) + the planes of its eight children (traverse.h PBLOCK_*)
    std::vector<float> lrec;                               // LREC_WORDS per node (leafNB, leafTB, first run), then RUN_WORDS per run (runTB): traverse.h LREC_*
    std::vector<int> childDfs, srefs, objMesh;
    std::vector<MeshRec> meshes;
    std::vector<ObjRec> objects;
    std::vector<MaterialRec> materials;
    std::vector<uint32_t> texels;
    int sceneDepth = 0, meshDepth = 0;
    int totalTris = 0;
    bool anyTransparent = false, anyTexture = false;
    size_t bytes() const;
};

struct HostScene {
    std::vector<HostMesh> meshes;
    std::vector<HostObject> objects;
    std::vector<FlatTree> meshTrees;
    FlatTree sceneTree;
    SceneArrays arrays;
    bool built = false;
    int builtMeshes = -1;          // meshes [0, builtMeshes) have their octrees and their part of `arrays` (-1: no build yet; set_bodies builds the others)
    int meshThreshold = 50;        // MeshOctree's threshold of the last build(): what set_bodies builds later meshes with
    bool spatialRuns = true;       // the references of a big leaf are stored in runs of neighbouring triangles (scene_host.cpp spatial_runs; XRT_LEAF_ORDER=0: in list order)
    double leafCullSafety = 1.0;   // factor on the tight-leaf-box margin (xrt_core.h LEAF_CULL_C): 0 switches the skip off, below 1 the bound is no longer proven (tests)
    double cullSafety = 2.0;   // factor S of the object pre-cull margin (scene_host.cpp); tests lower it to see the bound bite

    int add_mesh(const float *v, const float *n, const float *uv, const float *sn, const float *color, int ntri,
                 const xrt_material *m, const float bbox[6], std::string &err);
    int add_object(const int *meshIds, int n, const float *world, const float *invWorld, const float *bbox,
                   const float *worldBbox, std::string &err);
    bool build(int meshThreshold, int sceneThreshold, std::string &err);
    // SceneObject.World / InverseWorld / WorldBoundingBox setters (SO:52-89, 183-199): after a build also the body's ObjRec and its records
    // in scull; the scene octree stays as built (OSM:64-99 runs only in Build).
    bool set_pose(int id, const float *world, const float *invWorld, const float *worldBbox, std::string &err);
    // OctreeSpatialManager.Build alone over the current poses (0 = OSM:50's 20): meshes, their octrees and the ObjRecs are untouched.
    bool build_tree(int sceneThreshold, std::string &err);
    // Material's setters (MAT:39, 234-268), batched: mesh ids[i] takes mats[i] (xrt.h xrt_scene_set_materials: the texel cases, all or
    // nothing, the last entry of a mesh wins).  After a build also the MaterialRecs, the texel arena and anyTransparent / anyTexture of
    // `arrays`; nothing else of it is touched.  texLo / texHi: the words of arrays.texels that changed (texFull: the arena was packed again,
    // every offset may have moved).
    struct MaterialEdit { bool texels = false, texFull = false; size_t texLo = 0, texHi = 0; };
    bool set_materials(const int *ids, int n, const xrt_material *mats, MaterialEdit &edit, std::string &err);
    // Triangle's public fields n1..n3, uv1..uv3 and color (TRI:17-23), batched (xrt.h xrt_scene_set_triangle_shading): entry i edits triangle
    // ids[i] (ids null: first + i) of mesh `mesh`; a null array leaves its field alone.  Everything is checked before anything is applied; of
    // a triangle listed twice the last entry counts.  The words are copied as bits.  Where `arrays` holds the mesh (it is among the built
    // ones) the words of records 0..4 of arrays.shade that the call gives are written too, and nothing else of `arrays` is touched: no tree,
    // box or run depends on these fields.
    bool set_triangle_shading(int mesh, const int *ids, int first, int n, const float *normals, const float *uv, const float *color, std::string &err);
    // ... and the reverse for a whole mesh out of `recs`, the mesh's SHADE_F4 * ntri records as a device version holds them (the values
    // xrt_scene_set_triangle_shading_device left there): the mesh's n / uv / color and records 0..4 of arrays.shade.
    void take_triangle_shading(int mesh, const f4 *recs);
    // OctreeSpatialManager.Bodies replaced and Build() run (xrt.h xrt_scene_set_bodies): the body list becomes the n bodies given, meshes added since
    // the last build get their MeshOctree.Build (meshesBuilt: how many), no other mesh is built again, and `arrays`, sceneTree and meshTrees end byte for
    // byte as build() leaves them for the same meshes and bodies.  Returns XRT_OK, XRT_E_NOT_BUILT (no build yet), XRT_E_INVALID_ARG (nothing was
    // applied) or XRT_E_UNSUPPORTED: the list was applied and a tree could not be built.  When it was the scene tree, meshesBuilt holds what the call
    // built, the arrays of the meshes are whole and another set_bodies (or build()) repairs the scene; when it was a mesh tree (internal errors only),
    // `arrays` is of no use, later calls return XRT_E_NOT_BUILT and only build() repairs it.
    int set_bodies(int n, const int *meshStart, const int *meshIds, const float *world, const float *invWorld, const float *bbox,
                   const float *worldBbox, int sceneThreshold, int &meshesBuilt, std::string &err);
    // Mesh.Triangles (and Mesh.MeshBoundingBox) replaced and Mesh.Init() run (xrt.h xrt_scene_set_mesh_triangles): mesh `mesh` takes the ntri triangles
    // given, arrays as for add_mesh, under its id and with its material.  Where `arrays` holds the mesh (it is among the built ones) its MeshOctree.Build
    // runs with meshThreshold -- for this mesh alone -- into a temporary; the mesh's part of every per-mesh array is replaced by the new one, the parts of
    // the meshes behind it move (their base-relative words take the difference), refT / lrec and the padding are made again, and, on a built scene, the
    // pre-cull records of the bodies that name the mesh are made from the new box and the bodies' current poses.  The body list, the bodies' boxes and the
    // scene octree are not touched.  `arrays` and meshTrees end byte for byte as build() leaves them for the new triangles.  Everything is checked before
    // anything is applied: XRT_E_INVALID_ARG (arguments, mesh id) or XRT_E_UNSUPPORTED (the octree cannot be built, or (scene depth + 1) + (mesh depth + 1)
    // no longer fits a compiled stack) leave the scene as it was.  A mesh that waits for its build (or a scene never built) only takes the new triangles.
    int set_mesh_triangles(int mesh, const float *v, const float *n, const float *uv, const float *sn, const float *color, int ntri, const float bbox[6],
                           std::string &err);
    int meshTreesBuilt = 0;        // MeshOctree.Build runs (build_mesh_tree calls) of this scene so far, whatever came of them
    // Scene file (xrt_scene_save / xrt_scene_load): the meshes, materials, texels and bodies exactly as they were added --
    // what the reference keeps in .xnb files (Model.Tag, TMP:113-117) -- little-endian, no pointers.  The trees are rebuilt on load.
    bool save(const char *path, std::string &err) const;
    bool load(const char *path, std::string &err);
    SceneView host_view() const;
  private:
    // build() in its four parts.  mesh_part builds the octrees of meshes [builtMeshes, meshes.size()) and appends what they add to `arrays` (append_parts:
    // behind what the others left there, the padding of assemble() taken off first -- strip_padding); body_part makes objects / objMesh and the scene octree from `objects`; material_part the material
    // table and the texel arena; assemble() the padding at the arrays' ends and the arrays derived from the whole (refT, lrec).
    struct RawSizes { size_t blocks = 0, refN = 0, shade = 0, leafNB = 0, leafTB = 0, runBase = 0, runTB = 0, childDfs = 0, pblocks = 0, meshes = 0; } raw;   // sizes without the padding
    std::vector<RawSizes> partStart;   // per built mesh: where its part of the per-mesh arrays begins (it ends where the next one's begins, the last one's at `raw`)
    RawSizes sizes_now() const;
    void strip_padding();
    bool mesh_part(std::string &err);
    bool append_parts(size_t first, size_t last, int triBase, std::string &err);
    void refresh_cull(int id);
    bool body_part(int sceneThreshold, std::string &err);
    void material_part();
    void assemble();
    bool scene_part(int sceneThreshold, std::string &err);
  public:   // pointers into `arrays` (CPU single-stepping in tests/emul only)
};

}  // namespace xrt
