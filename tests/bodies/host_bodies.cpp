// xrt_scene_set_bodies on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile `hostcheck_bodies`): two
// meshes, three bodies, built; then the edits of tests/test_bodies_cpu.py through the C-ABI -- bodies removed from the middle, the list
// reordered, bodies of known meshes added, a body of a new mesh, a new Transparent textured mesh, a list the scene octree cannot hold and its repair, the empty list, the list refilled with a body
// of two meshes and a body of none --, the calls that must be rejected as a whole, and a material change that must survive an edit.  After every
// step the scene file and every tree are compared with those of a scene made from scratch with the same meshes and bodies.  Then save, load,
// build, destroy.  What it checks beyond the return codes: that all of this is clean on the host under AddressSanitizer, UBSan and
// LeakSanitizer.  Needs no GPU; prints "host_bodies: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/xrt.h"

static int failed(const char *what, int rc) {
    fprintf(stderr, "host_bodies: %s returned %d: %s\n", what, rc, xrt_last_error());
    return 1;
}

struct Mesh {
    std::vector<float> v, n, uv, sn, color;
    int ntri = 0;
    float bbox[6] = {0, 0, 0, 0, 0, 0};
    xrt_material mat;
    std::vector<uint32_t> tex;
};
struct Body { std::vector<int32_t> meshes; float x, y, z, s; };

// A bumpy k x k grid of quads over [0, size]^2, enough triangles for a real octree when k is large.
static Mesh grid_mesh(int k, float size, float reflectiveness) {
    Mesh m;
    auto h = [&](int i, int j) { return 0.37f * (float)((i * 7 + j * 13) % 5); };
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            const float x0 = size * i / k, x1 = size * (i + 1) / k, z0 = size * j / k, z1 = size * (j + 1) / k;
            const float tri[2][9] = {{x0, h(i, j), z0, x0, h(i, j + 1), z1, x1, h(i + 1, j), z0}, {x1, h(i + 1, j), z0, x0, h(i, j + 1), z1, x1, h(i + 1, j + 1), z1}};
            for (const auto &t : tri) {
                m.v.insert(m.v.end(), t, t + 9);
                const float e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
                const float nn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                m.sn.insert(m.sn.end(), nn, nn + 3);
                for (int c = 0; c < 3; c++) m.n.insert(m.n.end(), nn, nn + 3);
                const float uv[6] = {0, 0, 1, 0, 0, 1}, col[4] = {1, 0.5f, 0.25f, 1};
                m.uv.insert(m.uv.end(), uv, uv + 6);
                m.color.insert(m.color.end(), col, col + 4);
                m.ntri++;
            }
        }
    m.bbox[3] = size; m.bbox[4] = 2.0f; m.bbox[5] = size;
    std::memset(&m.mat, 0, sizeof(m.mat));
    m.mat.reflectiveness = reflectiveness; m.mat.refraction_index = 1.0f;
    return m;
}

static int add_mesh(xrt_scene *s, const Mesh &m) {
    int32_t id = -1;
    static const float none[9] = {0};
    const bool e = m.ntri == 0;
    return xrt_scene_add_mesh(s, e ? none : m.v.data(), e ? none : m.n.data(), e ? none : m.uv.data(), e ? none : m.sn.data(), e ? none : m.color.data(), m.ntri, &m.mat,
                              m.bbox, &id);
}

struct BodyArrays {
    std::vector<int32_t> start{0}, ids;
    std::vector<float> world, inv, bbox, wbb;
    BodyArrays(const std::vector<Mesh> &meshes, const std::vector<Body> &bodies) {
        for (const Body &b : bodies) {
            ids.insert(ids.end(), b.meshes.begin(), b.meshes.end());
            start.push_back((int32_t)ids.size());
            const float w[16] = {b.s, 0, 0, 0, 0, b.s, 0, 0, 0, 0, b.s, 0, b.x, b.y, b.z, 1};
            const float i[16] = {1 / b.s, 0, 0, 0, 0, 1 / b.s, 0, 0, 0, 0, 1 / b.s, 0, -b.x / b.s, -b.y / b.s, -b.z / b.s, 1};
            float bb[6] = {0, 0, 0, 0, 0, 0};
            for (int32_t m : b.meshes)
                for (int a = 0; a < 3; a++) { bb[a] = bb[a] < meshes[(size_t)m].bbox[a] ? bb[a] : meshes[(size_t)m].bbox[a]; bb[3 + a] = bb[3 + a] > meshes[(size_t)m].bbox[3 + a] ? bb[3 + a] : meshes[(size_t)m].bbox[3 + a]; }
            const float wb[6] = {bb[0] * b.s + b.x, bb[1] * b.s + b.y, bb[2] * b.s + b.z, bb[3] * b.s + b.x, bb[4] * b.s + b.y, bb[5] * b.s + b.z};
            world.insert(world.end(), w, w + 16); inv.insert(inv.end(), i, i + 16); bbox.insert(bbox.end(), bb, bb + 6); wbb.insert(wbb.end(), wb, wb + 6);
        }
        if (ids.empty()) ids.push_back(0);
    }
};

// A scene of `meshes` and `bodies` made from scratch and built.
static xrt_scene *make(const std::vector<Mesh> &meshes, const std::vector<Body> &bodies, int sceneThreshold) {
    xrt_scene *s = nullptr;
    if (xrt_scene_create(-1, &s) != XRT_OK) return nullptr;
    bool ok = true;
    for (const Mesh &m : meshes) ok = ok && add_mesh(s, m) == XRT_OK;
    const BodyArrays a(meshes, bodies);
    for (size_t b = 0; ok && b < bodies.size(); b++) {
        int32_t id = -1;
        ok = xrt_scene_add_object(s, a.ids.data() + a.start[b], a.start[b + 1] - a.start[b], &a.world[16 * b], &a.inv[16 * b], &a.bbox[6 * b], &a.wbb[6 * b], &id) == XRT_OK;
    }
    if (!ok || xrt_scene_build(s, 8, sceneThreshold) != XRT_OK) { xrt_scene_destroy(s); return nullptr; }
    return s;
}

static bool file_bytes(xrt_scene *s, std::string &out) {
    char path[] = "/tmp/xrt_host_bodies_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) return false;
    close(fd);
    const int rc = xrt_scene_save(s, path);
    out.clear();
    if (FILE *f = fopen(path, "rb")) {
        char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) out.append(buf, k);
        fclose(f);
    }
    unlink(path);
    return rc == XRT_OK && !out.empty();
}

static bool trees(xrt_scene *s, int nMeshes, std::string &out) {
    out.clear();
    for (int m = -1; m < nMeshes; m++) {
        int64_t nn = 0, nr = 0;
        if (xrt_scene_get_tree(s, m, nullptr, &nn, nullptr, &nr) != XRT_OK) return false;
        std::vector<xrt_node_info> nodes((size_t)nn + 1);
        std::vector<int32_t> refs((size_t)nr + 1);
        if (xrt_scene_get_tree(s, m, nodes.data(), &nn, refs.data(), &nr) != XRT_OK) return false;
        out.append((const char *)&nn, sizeof(nn)); out.append((const char *)&nr, sizeof(nr));
        out.append((const char *)nodes.data(), (size_t)nn * sizeof(xrt_node_info)); out.append((const char *)refs.data(), (size_t)nr * sizeof(int32_t));
    }
    return true;
}

static bool same_as_fresh(xrt_scene *s, const std::vector<Mesh> &meshes, const std::vector<Body> &bodies, int thr, const char *step) {
    std::string a, b, ta, tb;
    xrt_scene *fresh = make(meshes, bodies, thr);
    const bool ok = fresh && file_bytes(s, a) && file_bytes(fresh, b) && a == b && trees(s, (int)meshes.size(), ta) && trees(fresh, (int)meshes.size(), tb) && ta == tb;
    if (fresh) xrt_scene_destroy(fresh);
    if (!ok) fprintf(stderr, "host_bodies: after '%s' the scene differs from a fresh scene's (file %zu / %zu bytes, trees %zu / %zu): %s\n", step, a.size(), b.size(), ta.size(), tb.size(), xrt_last_error());
    return ok;
}

int main() {
    if (xrt_version() != XRT_VERSION) return failed("xrt_version", xrt_version());
    for (int thr : {2, 20}) {
        std::vector<Mesh> meshes{grid_mesh(6, 10.0f, 0.5f), grid_mesh(1, 4.0f, 0.25f)};
        std::vector<Body> bodies;
        for (int i = 0; i < 5; i++) bodies.push_back(Body{{i % 2}, -40.0f + 20.0f * i, 0.0f, 3.0f * i, 1.0f});
        xrt_scene *s = make(meshes, bodies, thr);
        if (!s) return failed("making the scene", -1);
        int rc;
        size_t known = meshes.size();
        auto step = [&](const char *what, int wantBuilt) -> bool {
            for (; known < meshes.size(); known++)
                if ((rc = add_mesh(s, meshes[known])) != XRT_OK) { failed("xrt_scene_add_mesh", rc); return false; }
            const BodyArrays a(meshes, bodies);
            int32_t built = -1;
            if ((rc = xrt_scene_set_bodies(s, (int32_t)bodies.size(), a.start.data(), a.ids.data(), a.world.data(), a.inv.data(), a.bbox.data(), a.wbb.data(), thr, &built)) != XRT_OK) { failed(what, rc); return false; }
            if (built != wantBuilt) { fprintf(stderr, "host_bodies: '%s' built %d meshes, not %d\n", what, built, wantBuilt); return false; }
            return same_as_fresh(s, meshes, bodies, thr, what);
        };
        bodies.erase(bodies.begin() + 1, bodies.begin() + 3);
        if (!step("bodies removed from the middle", 0)) return 1;
        std::swap(bodies[0], bodies[2]);
        if (!step("reordered", 0)) return 1;
        bodies.push_back(Body{{0}, 5.0f, 12.0f, -30.0f, 1.5f});
        bodies.push_back(Body{{1}, -15.0f, -2.0f, 25.0f, 0.5f});
        if (!step("bodies of known meshes added", 0)) return 1;
        meshes.push_back(grid_mesh(9, 6.0f, 0.7f));
        bodies.push_back(Body{{2}, 0.0f, 20.0f, 0.0f, 1.0f});
        if (!step("a body of a new mesh", 1)) return 1;
        // a material changed on a known mesh: it must survive the edits that follow
        meshes[0].mat.reflectiveness = 0.875f; meshes[0].mat.interpolate_normals = 1;
        const int32_t m0 = 0;
        if ((rc = xrt_scene_set_materials(s, &m0, 1, &meshes[0].mat)) != XRT_OK) return failed("xrt_scene_set_materials", rc);
        Mesh glass = grid_mesh(2, 3.0f, 0.7f);
        glass.tex.assign(6, 0xff204060u);
        glass.mat.transparent = 1; glass.mat.refraction_index = 1.32f; glass.mat.use_texture = 1; glass.mat.tex_width = 3; glass.mat.tex_height = 2;
        meshes.push_back(glass);
        meshes.back().mat.tex_argb = meshes.back().tex.data();
        bodies.insert(bodies.begin() + 1, Body{{3}, 8.0f, 4.0f, 40.0f, 3.0f});
        if (!step("a new Transparent mesh", 1)) return 1;
        // calls that must be rejected as a whole
        std::string before, after;
        if (!file_bytes(s, before)) return failed("xrt_scene_save", -1);
        {
            const BodyArrays a(meshes, bodies);
            const int32_t n = (int32_t)bodies.size();
            std::vector<int32_t> badStart = a.start, badIds = a.ids;
            badStart[0] = 1;
            if ((rc = xrt_scene_set_bodies(s, n, badStart.data(), a.ids.data(), a.world.data(), a.inv.data(), a.bbox.data(), a.wbb.data(), thr, nullptr)) != XRT_E_INVALID_ARG) return failed("mesh_start[0] != 0", rc);
            badStart = a.start; badStart[2] = badStart[1] - 1;
            if ((rc = xrt_scene_set_bodies(s, n, badStart.data(), a.ids.data(), a.world.data(), a.inv.data(), a.bbox.data(), a.wbb.data(), thr, nullptr)) != XRT_E_INVALID_ARG) return failed("a decreasing mesh_start", rc);
            badIds.back() = (int32_t)meshes.size();
            if ((rc = xrt_scene_set_bodies(s, n, a.start.data(), badIds.data(), a.world.data(), a.inv.data(), a.bbox.data(), a.wbb.data(), thr, nullptr)) != XRT_E_INVALID_ARG) return failed("an unknown mesh id", rc);
            if ((rc = xrt_scene_set_bodies(s, -1, a.start.data(), a.ids.data(), a.world.data(), a.inv.data(), a.bbox.data(), a.wbb.data(), thr, nullptr)) != XRT_E_INVALID_ARG) return failed("n_bodies < 0", rc);
            if ((rc = xrt_scene_set_bodies(s, n, a.start.data(), a.ids.data(), nullptr, a.inv.data(), a.bbox.data(), a.wbb.data(), thr, nullptr)) != XRT_E_INVALID_ARG) return failed("a null array", rc);
        }
        if (!file_bytes(s, after) || before != after) { fprintf(stderr, "host_bodies: a rejected call changed the scene\n"); return 1; }
        // a list the scene octree cannot hold (more bodies than the threshold in one place, OSM:101-113), with a new mesh added before it: the call
        // builds and counts the mesh, returns XRT_E_UNSUPPORTED and leaves the scene not built; the next legal call repairs it and builds nothing
        {
            const std::vector<Body> keep = bodies;
            meshes.push_back(grid_mesh(3, 5.0f, 0.3f));
            for (; known < meshes.size(); known++)
                if ((rc = add_mesh(s, meshes[known])) != XRT_OK) return failed("xrt_scene_add_mesh", rc);
            const int32_t fresh = (int32_t)meshes.size() - 1;
            const std::vector<Body> heap((size_t)thr + 1, Body{{fresh}, 1.0f, 2.0f, 3.0f, 1.0f});
            const BodyArrays a(meshes, heap);
            int32_t built = -1;
            rc = xrt_scene_set_bodies(s, (int32_t)heap.size(), a.start.data(), a.ids.data(), a.world.data(), a.inv.data(), a.bbox.data(), a.wbb.data(), thr, &built);
            if (rc != XRT_E_UNSUPPORTED || built != 1) { fprintf(stderr, "host_bodies: a list the scene octree cannot hold built %d meshes\n", built); return failed("a list the scene octree cannot hold", rc); }
            int64_t nn = 0, nr = 0;
            if ((rc = xrt_scene_get_tree(s, -1, nullptr, &nn, nullptr, &nr)) != XRT_E_NOT_BUILT) return failed("xrt_scene_get_tree after the refused list", rc);
            bodies = keep;
            bodies.push_back(Body{{fresh}, 1.0f, 2.0f, 3.0f, 1.0f});
            if (!step("the list repaired", 0)) return 1;
        }
        bodies.clear();
        if (!step("the empty list", 0)) return 1;
        meshes.push_back(grid_mesh(0, 1.0f, 0.1f));   // (a mesh without triangles)
        bodies.push_back(Body{{2, 0}, 0.0f, 0.0f, 0.0f, 1.0f});
        bodies.push_back(Body{{}, 1.0f, 1.0f, 1.0f, 1.0f});
        bodies.push_back(Body{{3, (int32_t)meshes.size() - 1}, -12.0f, 3.0f, 9.0f, 2.0f});
        if (!step("refilled", 1)) return 1;
        // before the first build
        xrt_scene *raw = nullptr;
        if (xrt_scene_create(-1, &raw) != XRT_OK || add_mesh(raw, meshes[0]) != XRT_OK) return failed("xrt_scene_create", -1);
        {
            const BodyArrays a(meshes, bodies);
            if ((rc = xrt_scene_set_bodies(raw, 0, a.start.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr)) != XRT_E_NOT_BUILT) return failed("a call before the build", rc);
        }
        xrt_scene_destroy(raw);
        // save, load, build, destroy
        char path[] = "/tmp/xrt_host_bodies_XXXXXX";
        const int fd = mkstemp(path);
        if (fd < 0) { perror("host_bodies: mkstemp"); return 1; }
        close(fd);
        xrt_scene *loaded = nullptr;
        rc = xrt_scene_save(s, path);
        if (rc == XRT_OK) rc = xrt_scene_load(-1, path, &loaded);
        unlink(path);
        if (rc != XRT_OK) return failed("xrt_scene_save / xrt_scene_load", rc);
        if ((rc = xrt_scene_build(loaded, 8, thr)) != XRT_OK) return failed("xrt_scene_build (loaded scene)", rc);
        if (!same_as_fresh(loaded, meshes, bodies, thr, "load")) return 1;
        if ((rc = xrt_scene_destroy(s)) != XRT_OK) return failed("xrt_scene_destroy", rc);
        if ((rc = xrt_scene_destroy(loaded)) != XRT_OK) return failed("xrt_scene_destroy (loaded scene)", rc);
    }
    printf("host_bodies: ok\n");
    return 0;
}
