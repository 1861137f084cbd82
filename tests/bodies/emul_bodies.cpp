// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  tests/emul (included unmodified) plus the product's host-side body-list edit: the one-lane CPU
// single-stepper of traverse.h on a HostScene whose body list was replaced with HostScene::set_bodies (what xrt_scene_set_bodies runs), and a
// byte-for-byte comparison of two HostScenes: every vector of SceneArrays, its scalars, the scene tree and every mesh tree.
#include "../emul/emul.cpp"

#include <cstdio>

namespace {
template <class T> bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
const char *tree_diff(const FlatTree &a, const FlatTree &b) {
    if (!same(a.blocks, b.blocks)) return "blocks";
    if (!same(a.childDfs, b.childDfs)) return "childDfs";
    if (std::memcmp(a.rootBox, b.rootBox, sizeof(a.rootBox)) != 0) return "rootBox";
    if (a.rootIsLeaf != b.rootIsLeaf || a.rootCount != b.rootCount) return "root";
    if (!same(a.nodes, b.nodes)) return "nodes";
    if (!same(a.nodeDfs, b.nodeDfs)) return "nodeDfs";
    if (!same(a.leafRefs, b.leafRefs)) return "leafRefs";
    if (!same(a.info, b.info)) return "info";
    if (!same(a.infoRefs, b.infoRefs)) return "infoRefs";
    if (a.nodeCount != b.nodeCount || a.leafCount != b.leafCount || a.emptyLeaves != b.emptyLeaves || a.maxDepth != b.maxDepth || a.unsafeNodes != b.unsafeNodes ||
        a.interiors != b.interiors)
        return "counts";
    return nullptr;
}
}  // namespace

extern "C" {
int emu_set_bodies(emu_scene *s, int n, const int *mesh_start, const int *mesh_ids, const float *world, const float *inv_world, const float *bbox,
                   const float *world_bbox, int scene_threshold, int *meshes_built) {
    int built = -1;
    const int rc = s->hs.set_bodies(n, mesh_start, mesh_ids, world, inv_world, bbox, world_bbox, scene_threshold, built, s->err);
    if (meshes_built) *meshes_built = built;
    return rc;
}
int emu_set_materials(emu_scene *s, const int *ids, int n, const xrt_material *mats) {
    HostScene::MaterialEdit edit;
    return s->hs.set_materials(ids, n, mats, edit, s->err) ? 0 : -1;
}
// 0: a and b hold the same bytes; else the name of the first part that differs is written to what[cap]
int emu_compare(const emu_scene *a, const emu_scene *b, char *what, int cap) {
    const SceneArrays &A = a->hs.arrays, &B = b->hs.arrays;
    const char *d = nullptr;
    char buf[64];
#define CMP(f) if (!d && !same(A.f, B.f)) d = "arrays." #f;
    CMP(blocks) CMP(refN) CMP(snodes) CMP(shade) CMP(leafNB) CMP(refT) CMP(runTB) CMP(runBase) CMP(scull) CMP(scullPosStart) CMP(scullPos) CMP(leafTB) CMP(refG)
    CMP(pblocks) CMP(lrec) CMP(childDfs) CMP(srefs) CMP(objMesh) CMP(meshes) CMP(objects) CMP(materials) CMP(texels)
#undef CMP
    if (!d && (A.sceneDepth != B.sceneDepth || A.meshDepth != B.meshDepth || A.totalTris != B.totalTris || A.anyTransparent != B.anyTransparent || A.anyTexture != B.anyTexture))
        d = "arrays scalars";
    if (!d && a->hs.built != b->hs.built) d = "built";
    if (!d && a->hs.objects.size() != b->hs.objects.size()) d = "objects";
    if (!d) if (const char *t = tree_diff(a->hs.sceneTree, b->hs.sceneTree)) { snprintf(buf, sizeof(buf), "sceneTree.%s", t); d = buf; }
    if (!d && a->hs.meshTrees.size() != b->hs.meshTrees.size()) d = "meshTrees";
    for (size_t m = 0; !d && m < a->hs.meshTrees.size(); m++)
        if (const char *t = tree_diff(a->hs.meshTrees[m], b->hs.meshTrees[m])) { snprintf(buf, sizeof(buf), "meshTrees[%zu].%s", m, t); d = buf; }
    if (!d) return 0;
    if (what && cap > 0) snprintf(what, (size_t)cap, "%s", d);
    return 1;
}
}  // extern "C"
