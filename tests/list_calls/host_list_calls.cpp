// The argument checks of the seven list calls -- xrt_cast_rays, xrt_shade_hits, xrt_light_hits, xrt_surface_hits, xrt_cast_rays_paths, xrt_render_pixels,
// xrt_trace_pixels, each in its host and its _device form -- on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile
// `hostcheck_list_calls`).  The scene of tests/surface/host_surface.cpp: two meshes (3 and 5 triangles) in two bodies, built.
// For every entry point the call with nothing wrong, with n == 0 and with n > 0 -- on a scene without a device XRT_OK or XRT_E_NO_DEVICE --, then a fixed table
// of calls, each wrong in exactly one way, in the order in which the entry point makes its checks.  The pointers of the _device forms are made-up addresses: a host-only scene never follows them.
// One line per call: entry point | case | return code | xrt_last_error() | what became of stats_out (filled with 0xAB before the call).
// tests/test_list_calls_cpu.py compares the output line for line with tests/golden/list_call_errors.txt.  Needs no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../../include/xrt.h"

static const int N = 6;   // entries of a valid list

struct Ctx {
    bool device = false;
    xrt_scene *scene = nullptr;
    // what the pointers below point at in a host form
    xrt_render_opts h_opts;
    xrt_camera h_cam;
    xrt_light h_lights[2];
    std::vector<xrt_ray> h_rays;
    std::vector<xrt_hit> h_hits;
    std::vector<float> h_centers;
    std::vector<unsigned char> h_out[5];
    int64_t h_nv = 0;
    // the arguments
    const void *rays = nullptr, *hits = nullptr, *centers = nullptr;
    int64_t n = 0;
    int32_t iteration = 0, n_lights = 0;
    const xrt_light *lights = nullptr;
    const xrt_render_opts *opts = nullptr;
    const xrt_camera *cam = nullptr;
    void *out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t vertex_capacity = 0;
    int64_t *n_vertices_out = nullptr;
};

static void reset(Ctx &c, xrt_scene *scene, bool device) {
    static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    c.device = device;
    c.scene = scene;
    std::memset(&c.h_opts, 0, sizeof(c.h_opts));
    c.h_opts.max_reflections = 2; c.h_opts.address_mode = XRT_ADDRESS_WRAP; c.h_opts.filtering = XRT_FILTER_POINT;
    std::memset(&c.h_cam, 0, sizeof(c.h_cam));
    std::memcpy(c.h_cam.view, IDENT, sizeof(IDENT)); std::memcpy(c.h_cam.proj, IDENT, sizeof(IDENT));
    c.h_cam.vp_width = 8; c.h_cam.vp_height = 8; c.h_cam.vp_max_depth = 1.0f;
    std::memset(c.h_lights, 0, sizeof(c.h_lights));
    c.h_lights[0].kind = XRT_LIGHT_SPOT; c.h_lights[1].kind = XRT_LIGHT_DIRECTIONAL;
    for (xrt_light &l : c.h_lights) { l.direction[2] = -1.0f; l.color[0] = l.color[1] = l.color[2] = 1.0f; l.intensity = 1.0f; l.spot_angle = 1.0f; l.decay_exponent = 1.3f; }
    c.h_rays.assign(N, xrt_ray());
    c.h_hits.assign(N, xrt_hit());
    c.h_centers.assign(2 * N, 0.0f);
    for (int i = 0; i < N; i++) {
        xrt_ray &r = c.h_rays[i];
        std::memset(&r, 0, sizeof(r));
        r.d[2] = -1.0f; r.ignore_mesh = -1; r.ignore_tri = -1;
        xrt_hit &h = c.h_hits[i];
        std::memset(&h, 0, sizeof(h));
        h.hit = 1; h.object = i & 1; h.mesh = i & 1; h.tri = (i & 1) ? 4 : 2;   // the last triangle of each mesh, in the body that holds the mesh
        h.u = 0.25f; h.v = 0.5f; h.d = 1.0f; h.wx = 1.0f;
        c.h_centers[2 * i] = 0.5f + (float)i; c.h_centers[2 * i + 1] = 0.5f;
    }
    c.h_rays[1].ignore_mesh = 1; c.h_rays[1].ignore_tri = 4;   // an origin that exists
    c.h_hits[2].hit = 0; c.h_hits[2].mesh = 99; c.h_hits[2].tri = -4; c.h_hits[2].object = 55;   // a miss: its other fields are not looked at
    for (auto &o : c.h_out) o.assign(4096, 0xcd);
    c.h_nv = -77;
    if (device) {
        c.rays = (const void *)(uintptr_t)0x10000; c.hits = (const void *)(uintptr_t)0x20000; c.centers = (const void *)(uintptr_t)0x30000;
        for (int k = 0; k < 5; k++) c.out[k] = (void *)(uintptr_t)(0x40000 + 0x10000 * k);
    } else {
        c.rays = c.h_rays.data(); c.hits = c.h_hits.data(); c.centers = c.h_centers.data();
        for (int k = 0; k < 5; k++) c.out[k] = c.h_out[k].data();
    }
    c.n = N; c.iteration = 0; c.n_lights = 2; c.lights = c.h_lights; c.opts = &c.h_opts; c.cam = &c.h_cam;
    c.vertex_capacity = 64; c.n_vertices_out = &c.h_nv;
}

typedef std::function<void(Ctx &)> Mut;
struct Case { std::string name; Mut mut; };
typedef std::vector<Case> Cases;
struct Family {
    const char *name;
    bool device;
    std::function<int(Ctx &, xrt_stats *)> call;
    Cases cases;
};

static void add(Cases &t, const char *name, Mut m) { t.push_back(Case{name, std::move(m)}); }
static void add(Cases &t, const Cases &more) { t.insert(t.end(), more.begin(), more.end()); }

// ---- the single mistakes ---------------------------------------------------------------------------------------------------------------------------
static Cases null_scene() { return {{"null scene", [](Ctx &c) { c.scene = nullptr; }}}; }
static Cases n_negative() { return {{"n < 0", [](Ctx &c) { c.n = -1; }}}; }
static Cases n_above_limit() { return {{"n above the limit", [](Ctx &c) { c.n = (int64_t)(0x7fffffff / 2) + 1; }}}; }
static Cases null_opts() { return {{"null opts", [](Ctx &c) { c.opts = nullptr; }}}; }
static Cases null_camera() { return {{"null camera", [](Ctx &c) { c.cam = nullptr; }}}; }
static Cases null_lights() { return {{"null lights", [](Ctx &c) { c.lights = nullptr; }}}; }
static Cases n_lights_negative() { return {{"n_lights < 0", [](Ctx &c) { c.n_lights = -1; }}}; }
static Cases outputs_null(int count) {
    return {{"every output null", [count](Ctx &c) { for (int k = 0; k < count; k++) c.out[k] = nullptr; }}};
}
static Cases null_output(const char *name, int k) { return {{name, [k](Ctx &c) { c.out[k] = nullptr; }}}; }
static Cases null_rays() { return {{"null rays", [](Ctx &c) { c.rays = nullptr; }}}; }
static Cases null_hits() { return {{"null hits", [](Ctx &c) { c.hits = nullptr; }}}; }
static Cases null_centers() { return {{"null centers", [](Ctx &c) { c.centers = nullptr; }}}; }
// the opts of a ray batch (xrt_cast_rays, xrt_shade_hits, xrt_cast_rays_paths)
static Cases batch_opts() {
    return {
        {"use_multisampling FIXED16", [](Ctx &c) { c.h_opts.use_multisampling = XRT_MS_FIXED16; }},
        {"shard_count 2", [](Ctx &c) { c.h_opts.shard_count = 2; }},
        {"n_gpus 2", [](Ctx &c) { c.h_opts.n_gpus = 2; }},
        {"max_reflections < 0", [](Ctx &c) { c.h_opts.max_reflections = -1; }},
        {"max_reflections - iteration > 64", [](Ctx &c) { c.h_opts.max_reflections = 70; c.iteration = 5; }},
        {"max_reflections - iteration == 64", [](Ctx &c) { c.h_opts.max_reflections = 70; c.iteration = 6; }},
        {"list_order 5", [](Ctx &c) { c.h_opts.list_order = 5; }},
    };
}
static Cases pixels_opts() {
    return {
        {"use_multisampling 7", [](Ctx &c) { c.h_opts.use_multisampling = 7; }},
        {"shard_count 2", [](Ctx &c) { c.h_opts.shard_count = 2; }},
        {"n_gpus 2", [](Ctx &c) { c.h_opts.n_gpus = 2; }},
        {"max_reflections < 0", [](Ctx &c) { c.h_opts.max_reflections = -1; }},
        {"max_reflections 65", [](Ctx &c) { c.h_opts.max_reflections = 65; }},
        {"address_mode 9", [](Ctx &c) { c.h_opts.address_mode = 9; }},
        {"filtering 9", [](Ctx &c) { c.h_opts.filtering = 9; }},
        {"multisample_quality 7, adaptive", [](Ctx &c) { c.h_opts.use_multisampling = XRT_MS_ADAPTIVE; c.h_opts.multisample_quality = 7; }},
        {"viewport width 0", [](Ctx &c) { c.h_cam.vp_width = 0; }},
        {"viewport height -1", [](Ctx &c) { c.h_cam.vp_height = -1; }},
        {"list_order 5", [](Ctx &c) { c.h_opts.list_order = 5; }},
    };
}
static Cases trace_opts() {
    return {
        {"use_multisampling ADAPTIVE", [](Ctx &c) { c.h_opts.use_multisampling = XRT_MS_ADAPTIVE; }},
        {"use_multisampling 7", [](Ctx &c) { c.h_opts.use_multisampling = 7; }},
        {"list_order 5", [](Ctx &c) { c.h_opts.list_order = 5; }},
        {"shard_count 2", [](Ctx &c) { c.h_opts.shard_count = 2; }},
        {"n_gpus 2", [](Ctx &c) { c.h_opts.n_gpus = 2; }},
        {"viewport width 0", [](Ctx &c) { c.h_cam.vp_width = 0; }},
        {"viewport height -1", [](Ctx &c) { c.h_cam.vp_height = -1; }},
    };
}
static Cases light_kind() { return {{"unknown light kind", [](Ctx &c) { c.h_lights[1].kind = 5; }}}; }
// a hit that names something the scene does not have, at index 0 and at index n - 1 (host forms: the device forms do not read the entries)
static Cases bad_hits(bool withBody) {
    Cases t;
    for (int at : {0, N - 1}) {
        const std::string where = at == 0 ? ", index 0" : ", index n-1";
        t.push_back({"hit names mesh -1" + where, [at](Ctx &c) { c.h_hits[at].mesh = -1; }});
        t.push_back({"hit names mesh 2" + where, [at](Ctx &c) { c.h_hits[at].mesh = 2; }});
        t.push_back({"hit names triangle -1" + where, [at](Ctx &c) { c.h_hits[at].tri = -1; }});
        t.push_back({"hit names triangle ntri" + where, [at](Ctx &c) { c.h_hits[at].tri = c.h_hits[at].mesh == 0 ? 3 : 5; }});
        if (withBody) {
            t.push_back({"hit names body -1" + where, [at](Ctx &c) { c.h_hits[at].object = -1; }});
            t.push_back({"hit names body 2" + where, [at](Ctx &c) { c.h_hits[at].object = 2; }});
            t.push_back({"hit names a mesh of another body" + where, [at](Ctx &c) { c.h_hits[at].object ^= 1; }});
        } else {
            t.push_back({"hit names body 2 (not read)" + where, [at](Ctx &c) { c.h_hits[at].object = 2; }});
        }
    }
    return t;
}
static Cases bad_origins() {
    Cases t;
    for (int at : {0, N - 1}) {
        const std::string where = at == 0 ? ", index 0" : ", index n-1";
        t.push_back({"ray names mesh 2" + where, [at](Ctx &c) { c.h_rays[at].ignore_mesh = 2; c.h_rays[at].ignore_tri = 0; }});
        t.push_back({"ray names mesh -1" + where, [at](Ctx &c) { c.h_rays[at].ignore_mesh = -1; c.h_rays[at].ignore_tri = 0; }});
        t.push_back({"ray names triangle ntri" + where, [at](Ctx &c) { c.h_rays[at].ignore_mesh = 0; c.h_rays[at].ignore_tri = 3; }});
    }
    return t;
}
static Cases bad_centers() {
    return {
        {"centre 0 x is NaN", [](Ctx &c) { c.h_centers[0] = std::numeric_limits<float>::quiet_NaN(); }},
        {"centre n-1 y is infinite", [](Ctx &c) { c.h_centers[2 * N - 1] = std::numeric_limits<float>::infinity(); }},
    };
}
static Cases vertex_capacity() {
    return {
        {"vertex_capacity < 0", [](Ctx &c) { c.vertex_capacity = -1; }},
        {"vertex_capacity > 0, null vertices", [](Ctx &c) { c.out[4] = nullptr; }},
        {"null n_vertices_out", [](Ctx &c) { c.n_vertices_out = nullptr; }},
    };
}
// (_device forms) a pointer off by 4 bytes
static Cases misaligned(const char *name, const void *Ctx::*p) {
    return {{std::string("misaligned ") + name, [p](Ctx &c) { c.*p = (const void *)((uintptr_t)(c.*p) + 4); }}};
}
static Cases misaligned_out(const char *name, int k) {
    return {{std::string("misaligned ") + name, [k](Ctx &c) { c.out[k] = (void *)((uintptr_t)c.out[k] + 4); }}};
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------------------------
static std::vector<Family> families() {
    std::vector<Family> F;
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_cast_rays_device" : "xrt_cast_rays", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_cast_rays_device(c.scene, c.rays, c.n, c.iteration, 1.0f, c.lights, c.n_lights, c.opts, c.out[0], c.out[1], nullptr, st);
            };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_cast_rays(c.scene, (const xrt_ray *)c.rays, c.n, c.iteration, 1.0f, c.lights, c.n_lights, c.opts, (uint32_t *)c.out[0], (float *)c.out[1], st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, n_negative()); add(t, n_above_limit()); add(t, null_opts()); add(t, null_rays()); add(t, outputs_null(2));
        add(t, null_output("null rgba", 0)); add(t, null_output("null rgb_f32 (allowed)", 1)); add(t, null_lights()); add(t, n_lights_negative());
        if (dev) { add(t, misaligned("rays", &Ctx::rays)); add(t, misaligned_out("rgba", 0)); add(t, misaligned_out("rgb_f32", 1)); }
        else add(t, bad_origins());
        add(t, batch_opts()); add(t, light_kind());
        F.push_back(f);
    }
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_shade_hits_device" : "xrt_shade_hits", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_shade_hits_device(c.scene, c.rays, c.hits, c.n, c.iteration, 1.0f, c.lights, c.n_lights, c.opts, c.out[0], c.out[1], nullptr, st);
            };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_shade_hits(c.scene, (const xrt_ray *)c.rays, (const xrt_hit *)c.hits, c.n, c.iteration, 1.0f, c.lights, c.n_lights, c.opts, (uint32_t *)c.out[0],
                                      (float *)c.out[1], st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, n_negative()); add(t, n_above_limit()); add(t, null_opts()); add(t, null_rays()); add(t, null_hits()); add(t, outputs_null(2));
        add(t, null_output("null rgba", 0)); add(t, null_output("null rgb_f32 (allowed)", 1)); add(t, null_lights()); add(t, n_lights_negative());
        add(t, batch_opts());
        if (dev) { add(t, misaligned("rays", &Ctx::rays)); add(t, misaligned("hits", &Ctx::hits)); add(t, misaligned_out("rgba", 0)); add(t, misaligned_out("rgb_f32", 1)); }
        else add(t, bad_hits(true));
        add(t, light_kind());
        F.push_back(f);
    }
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_light_hits_device" : "xrt_light_hits", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) { return xrt_light_hits_device(c.scene, c.hits, c.n, c.lights, c.n_lights, c.out[0], c.out[1], nullptr, st); };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_light_hits(c.scene, (const xrt_hit *)c.hits, c.n, c.lights, c.n_lights, (float *)c.out[0], (float *)c.out[1], st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, n_negative()); add(t, n_lights_negative()); add(t, null_lights()); add(t, outputs_null(2));
        add(t, null_output("null light (allowed)", 0)); add(t, null_output("null amount (allowed)", 1)); add(t, null_hits()); add(t, light_kind());
        if (dev) { add(t, misaligned("hits", &Ctx::hits)); add(t, misaligned_out("light", 0)); add(t, misaligned_out("amount", 1)); }
        else add(t, bad_hits(false));
        add(t, "no lights", [](Ctx &c) { c.n_lights = 0; c.lights = nullptr; });
        F.push_back(f);
    }
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_surface_hits_device" : "xrt_surface_hits", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) { return xrt_surface_hits_device(c.scene, c.rays, c.hits, c.n, 1.0f, c.opts, c.out[0], c.out[1], c.out[2], nullptr, st); };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_surface_hits(c.scene, (const xrt_ray *)c.rays, (const xrt_hit *)c.hits, c.n, 1.0f, c.opts, (xrt_surface *)c.out[0], (xrt_ray *)c.out[1],
                                        (xrt_ray *)c.out[2], st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, null_opts()); add(t, n_negative()); add(t, outputs_null(3)); add(t, null_hits()); add(t, null_rays());
        add(t, "null rays, surface alone (allowed)", [](Ctx &c) { c.rays = nullptr; c.out[1] = c.out[2] = nullptr; });
        if (dev) {
            add(t, misaligned("rays", &Ctx::rays)); add(t, misaligned("hits", &Ctx::hits)); add(t, misaligned_out("surface", 0)); add(t, misaligned_out("reflect", 1));
            add(t, misaligned_out("refract", 2));
        } else add(t, bad_hits(false));
        add(t, "opts a frame would refuse (not read)", [](Ctx &c) { c.h_opts.max_reflections = -3; c.h_opts.shard_count = 7; c.h_opts.n_gpus = 9; c.h_opts.list_order = 5; });
        F.push_back(f);
    }
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_cast_rays_paths_device" : "xrt_cast_rays_paths", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_cast_rays_paths_device(c.scene, c.rays, c.n, c.iteration, 1.0f, c.lights, c.n_lights, c.opts, c.out[0], c.out[1], c.out[2], c.out[3], c.out[4],
                                                  c.vertex_capacity, nullptr, c.n_vertices_out, st);
            };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_cast_rays_paths(c.scene, (const xrt_ray *)c.rays, c.n, c.iteration, 1.0f, c.lights, c.n_lights, c.opts, (uint32_t *)c.out[0], (float *)c.out[1],
                                           (xrt_ray *)c.out[2], (int64_t *)c.out[3], (xrt_path_vertex *)c.out[4], c.vertex_capacity, c.n_vertices_out, st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, n_negative()); add(t, n_above_limit()); add(t, null_opts()); add(t, vertex_capacity()); add(t, null_rays()); add(t, outputs_null(5));
        add(t, null_output("null rgba", 0)); add(t, null_output("null rgb_f32 (allowed)", 1)); add(t, null_output("null rays_back (allowed)", 2));
        add(t, null_output("null vertex_start (allowed)", 3)); add(t, null_lights()); add(t, n_lights_negative());
        add(t, "vertex_capacity 0, null vertices (allowed)", [](Ctx &c) { c.vertex_capacity = 0; c.out[4] = nullptr; });
        if (dev) {
            add(t, misaligned("rays", &Ctx::rays)); add(t, misaligned_out("rgba", 0)); add(t, misaligned_out("rgb_f32", 1)); add(t, misaligned_out("rays_back", 2));
            add(t, misaligned_out("vertex_start", 3)); add(t, misaligned_out("vertices", 4));
            add(t, "d_rays_back == d_rays", [](Ctx &c) { c.out[2] = const_cast<void *>(c.rays); });
        } else add(t, bad_origins());
        add(t, batch_opts()); add(t, light_kind());
        F.push_back(f);
    }
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_render_pixels_device" : "xrt_render_pixels", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_render_pixels_device(c.scene, c.cam, c.lights, c.n_lights, c.opts, c.centers, c.n, c.out[0], c.out[1], nullptr, st);
            };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_render_pixels(c.scene, c.cam, c.lights, c.n_lights, c.opts, (const float *)c.centers, c.n, (uint32_t *)c.out[0], (float *)c.out[1], st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, n_negative()); add(t, null_camera()); add(t, null_opts()); add(t, null_lights()); add(t, n_lights_negative()); add(t, pixels_opts());
        add(t, null_centers()); add(t, outputs_null(2)); add(t, null_output("null rgba", 0)); add(t, null_output("null rgb_f32 (allowed)", 1));
        if (dev) { add(t, misaligned("centers", &Ctx::centers)); add(t, misaligned_out("rgba", 0)); add(t, misaligned_out("rgb_f32", 1)); }
        else add(t, bad_centers());
        add(t, light_kind());
        F.push_back(f);
    }
    for (int dev = 0; dev < 2; dev++) {
        Family f{dev ? "xrt_trace_pixels_device" : "xrt_trace_pixels", dev != 0, nullptr, {}};
        if (dev)
            f.call = [](Ctx &c, xrt_stats *st) { return xrt_trace_pixels_device(c.scene, c.cam, c.opts, c.centers, c.n, c.out[0], c.out[1], nullptr, st); };
        else
            f.call = [](Ctx &c, xrt_stats *st) {
                return xrt_trace_pixels(c.scene, c.cam, c.opts, (const float *)c.centers, c.n, (xrt_ray *)c.out[0], (xrt_hit *)c.out[1], st);
            };
        Cases &t = f.cases;
        add(t, null_scene()); add(t, n_negative()); add(t, null_camera()); add(t, null_opts()); add(t, trace_opts()); add(t, outputs_null(2));
        add(t, null_output("null rays_out (allowed)", 0)); add(t, null_output("null hits_out (allowed)", 1)); add(t, null_centers());
        if (dev) { add(t, misaligned("centers", &Ctx::centers)); add(t, misaligned_out("rays_out", 0)); add(t, misaligned_out("hits_out", 1)); }
        else add(t, bad_centers());
        add(t, "use_multisampling FIXED16 (allowed)", [](Ctx &c) { c.h_opts.use_multisampling = XRT_MS_FIXED16; });
        F.push_back(f);
    }
    return F;
}

static int32_t add_mesh(xrt_scene *s, int ntri) {
    std::vector<float> v, n, uv, sn, color;
    for (int t = 0; t < ntri; t++) {
        const float x = (float)t;
        const float tv[9] = {x, 0, 0, x + 1, 0, 0, x, 1, 0};
        v.insert(v.end(), tv, tv + 9);
        for (int k = 0; k < 9; k++) n.push_back(k % 3 == 2 ? 1.0f : 0.0f);
        for (int k = 0; k < 6; k++) uv.push_back(0.125f * (float)(t + k));
        const float nn[3] = {0, 0, 1}, c[4] = {0.5f, 0.5f, 0.25f, 1.0f};
        sn.insert(sn.end(), nn, nn + 3);
        color.insert(color.end(), c, c + 4);
    }
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = 0.25f; mat.refraction_index = 1.0f;
    const float bbox[6] = {0, 0, 0, (float)ntri + 1, 1, 0};
    int32_t id = -1;
    if (xrt_scene_add_mesh(s, v.data(), n.data(), uv.data(), sn.data(), color.data(), ntri, &mat, bbox, &id) != XRT_OK) return -1;
    return id;
}

// One call: the line it prints.  A host form's outputs must be what they were (nothing is written without a device).
static void run(const Family &f, xrt_scene *scene, const std::string &name, const std::vector<const Mut *> &muts, int64_t n) {
    Ctx c;
    reset(c, scene, f.device);
    if (n >= 0) c.n = n;
    for (const Mut *m : muts) (*m)(c);
    xrt_stats st;
    std::memset(&st, 0xab, sizeof(st));
    const int rc = f.call(c, &st);
    const unsigned char *sb = (const unsigned char *)&st;
    size_t zero = 0, kept = 0;
    for (size_t i = 0; i < sizeof(st); i++) { zero += sb[i] == 0; kept += sb[i] == 0xab; }
    const char *stats = zero == sizeof(st) ? "zeroed" : (kept == sizeof(st) ? "kept" : "other");
    bool wrote = c.h_nv != -77;
    for (auto &o : c.h_out)
        for (unsigned char b : o) wrote |= b != 0xcd;
    printf("%s | %s | %d | %s | stats %s%s\n", f.name, name.c_str(), rc, xrt_last_error(), stats, wrote ? " | an output was written" : "");
}

int main() {
    static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    xrt_scene *s = nullptr;
    if (xrt_scene_create(-1, &s) != XRT_OK) { fprintf(stderr, "host_list_calls: xrt_scene_create: %s\n", xrt_last_error()); return 1; }
    const int32_t m0 = add_mesh(s, 3), m1 = add_mesh(s, 5);
    const float box[6] = {0, 0, 0, 8, 1, 0};
    int32_t b0 = -1, b1 = -1;
    if (m0 != 0 || m1 != 1 || xrt_scene_add_object(s, &m0, 1, IDENT, IDENT, box, box, &b0) != XRT_OK || xrt_scene_add_object(s, &m1, 1, IDENT, IDENT, box, box, &b1) != XRT_OK ||
        xrt_scene_build(s, 0, 0) != XRT_OK) {
        fprintf(stderr, "host_list_calls: scene: %s\n", xrt_last_error());
        return 1;
    }
    for (const Family &f : families()) {
        // nothing wrong first, then each mistake alone
        run(f, s, "valid, n == 0", {}, 0);
        run(f, s, "valid, n > 0", {}, -1);
        for (const Case &k : f.cases) run(f, s, k.name, {&k.mut}, -1);
    }
    xrt_scene_destroy(s);
    return 0;
}
