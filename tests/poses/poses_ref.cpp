// TEST INFRASTRUCTURE -- the checker of xrt_scene_set_poses / xrt_scene_build_tree: the CPU oracle with bodies moved between frames.
// The oracle is included unmodified (through tests/castray).  orc_scene_set_pose is what SceneObject.Position / Rotation / Scale + BuildWorld leave behind
// (SO:51-88, 183-199): new World, InverseWorld and WorldBoundingBox, the scene octree untouched; orc_scene_build_tree is
// OctreeSpatialManager.Build alone (OSM:64-99) over the same bodies.  orc_render / orc_scene_intersect then give the reference's frame.
#include "../castray/castray_ref.cpp"   // (the oracle, included unmodified, and its CastRay entry point)

extern "C" {

int orc_scene_set_pose(orc_scene *s, int32_t id, const float world[16], const float inv_world[16], const float world_bbox[6]) {
    if (id < 0 || id >= (int)s->objects.size()) return -1;
    SceneObject &o = *s->objects[(size_t)id];
    o.World = ToMatrix(world);
    o.InverseWorld = ToMatrix(inv_world);
    o.WorldBoundingBox = BoundingBox{V3(world_bbox[0], world_bbox[1], world_bbox[2]), V3(world_bbox[3], world_bbox[4], world_bbox[5])};
    return 0;
}

int orc_scene_build_tree(orc_scene *s, int32_t scene_threshold) {
    if (!s->built) return -1;
    if (scene_threshold <= 0) scene_threshold = 20;
    s->manager = OctreeSpatialManager();
    s->manager.itemTreshold = scene_threshold;
    for (auto &o : s->objects) s->manager.objects.push_back(o.get());
    s->manager.Build();
    if (s->manager.overflow) { s->error = "scene octree recursion would not terminate"; return -2; }
    return 0;
}

}  // extern "C"
