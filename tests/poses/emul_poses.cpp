// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  tests/emul (included unmodified) plus the product's host-side pose update: the one-lane CPU
// single-stepper of traverse.h on a HostScene whose bodies were moved with HostScene::set_pose (the ObjRec and pre-cull records
// xrt_scene_set_poses writes) and whose scene octree was made again with HostScene::build_tree (xrt_scene_build_tree).
#include "../emul/emul.cpp"

extern "C" {
int emu_set_pose(emu_scene *s, int id, const float *world, const float *inv_world, const float *world_bbox) {
    return s->hs.set_pose(id, world, inv_world, world_bbox, s->err) ? 0 : -1;
}
int emu_build_tree(emu_scene *s, int scene_threshold) { return s->hs.build_tree(scene_threshold, s->err) ? 0 : -1; }
// the pre-cull record of body id (ObjRec::cullOk, cullMin[4], cullMax[4], cullK2) -> out[10]
void emu_cull_record(emu_scene *s, int id, float *out) {
    const ObjRec &r = s->hs.arrays.objects[(size_t)id];
    out[0] = (float)r.cullOk;
    for (int k = 0; k < 4; k++) { out[1 + k] = r.cullMin[k]; out[5 + k] = r.cullMax[k]; }
    out[9] = r.cullK2;
}
}  // extern "C"
