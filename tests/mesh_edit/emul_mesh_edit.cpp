// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  tests/bodies/emul_bodies.cpp (tests/emul, included unmodified, plus emu_set_bodies, emu_set_materials and
// emu_compare) plus the product's host-side replacement of a mesh's triangles: HostScene::set_mesh_triangles (what xrt_scene_set_mesh_triangles runs),
// the other host-side edits a replay needs, the counter of mesh octrees built and the bytes the host arrays hold.
#include "../bodies/emul_bodies.cpp"

extern "C" {
int emu_set_mesh_triangles(emu_scene *s, int mesh, const float *v, const float *n, const float *uv, const float *sn, const float *color, int ntri, const float *bbox) {
    return s->hs.set_mesh_triangles(mesh, v, n, uv, sn, color, ntri, bbox, s->err);
}
int emu_mesh_trees_built(const emu_scene *s) { return s->hs.meshTreesBuilt; }
long long emu_arrays_bytes(const emu_scene *s) { return (long long)s->hs.arrays.bytes(); }
int emu_edit_pose(emu_scene *s, int id, const float *world, const float *inv_world, const float *world_bbox) {
    return s->hs.set_pose(id, world, inv_world, world_bbox, s->err) ? 0 : -1;
}
int emu_edit_triangle_shading(emu_scene *s, int mesh, int first, int n, const float *normals, const float *uv, const float *color) {
    return s->hs.set_triangle_shading(mesh, nullptr, first, n, normals, uv, color, s->err) ? 0 : -1;
}
}  // extern "C"
