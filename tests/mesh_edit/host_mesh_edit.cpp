// xrt_scene_set_mesh_triangles on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile
// `hostcheck_mesh_edit`): three meshes, five bodies, built at scene thresholds 2 and 20; then the first, the middle and the last mesh are
// replaced in turn through the C-ABI -- by a mesh of another kind and another triangle count (a single leaf, a real octree), by the same mesh with its vertices moved, by no triangles at all and by a real mesh again --, a pose, a
// material and triangle values are changed in between, and the calls that must be refused are made.  After every step the scene file and
// every tree are compared with those of a scene made from scratch with the replaced mesh and the same replay; after every refused call
// with those before it.  Then save, load, build, destroy.  What it checks beyond the return codes: that all of this is clean on the host
// under AddressSanitizer, UBSan and LeakSanitizer.  Needs no GPU; prints "host_mesh_edit: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/xrt.h"

static int failed(const char *what, int rc) {
    fprintf(stderr, "host_mesh_edit: %s returned %d: %s\n", what, rc, xrt_last_error());
    return 1;
}

struct Mesh {
    std::vector<float> v, n, uv, sn, color;
    int ntri = 0;
    float bbox[6] = {0, 0, 0, 0, 0, 0};
    xrt_material mat;
};
struct Body { std::vector<int32_t> meshes; float x, y, z, s; };

// A bumpy k x k grid of quads over [0, size]^2 (bump heights below `bump`), enough triangles for a real octree when k is large.  The box is
// [0, size] x [0, 2] x [0, size] whatever k and bump are: the bodies' boxes do not depend on which of these meshes they carry.
static Mesh grid_mesh(int k, float size, float bump, float reflectiveness) {
    Mesh m;
    auto h = [&](int i, int j) { return bump * (float)((i * 7 + j * 13) % 5); };
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

static const float none[9] = {0};   // (an empty vector has no address; the calls reject null arrays)
static int add_mesh(xrt_scene *s, const Mesh &m) {
    int32_t id = -1;
    const bool e = m.ntri == 0;
    return xrt_scene_add_mesh(s, e ? none : m.v.data(), e ? none : m.n.data(), e ? none : m.uv.data(), e ? none : m.sn.data(), e ? none : m.color.data(), m.ntri, &m.mat,
                              m.bbox, &id);
}
static int set_triangles(xrt_scene *s, int32_t id, const Mesh &m) {
    const bool e = m.ntri == 0;
    return xrt_scene_set_mesh_triangles(s, id, e ? none : m.v.data(), e ? none : m.n.data(), e ? none : m.uv.data(), e ? none : m.sn.data(), e ? none : m.color.data(), m.ntri,
                                        m.bbox);
}

struct Pose { float w[16], i[16], wb[6]; };
static Pose pose_of(const Body &b, const float bb[6]) {
    const Pose p = {{b.s, 0, 0, 0, 0, b.s, 0, 0, 0, 0, b.s, 0, b.x, b.y, b.z, 1},
                    {1 / b.s, 0, 0, 0, 0, 1 / b.s, 0, 0, 0, 0, 1 / b.s, 0, -b.x / b.s, -b.y / b.s, -b.z / b.s, 1},
                    {bb[0] * b.s + b.x, bb[1] * b.s + b.y, bb[2] * b.s + b.z, bb[3] * b.s + b.x, bb[4] * b.s + b.y, bb[5] * b.s + b.z}};
    return p;
}
// The bodies' boxes are made from the boxes the meshes had when the scene was FIRST built (the call does not touch them): `boxes`.
static void body_box(const std::vector<Mesh> &boxes, const Body &b, float bb[6]) {
    for (int a = 0; a < 6; a++) bb[a] = 0;
    for (int32_t m : b.meshes)
        for (int a = 0; a < 3; a++) { bb[a] = bb[a] < boxes[(size_t)m].bbox[a] ? bb[a] : boxes[(size_t)m].bbox[a]; bb[3 + a] = bb[3 + a] > boxes[(size_t)m].bbox[3 + a] ? bb[3 + a] : boxes[(size_t)m].bbox[3 + a]; }
}

// What was done to the scene after its build, for the replay on a fresh scene.
struct Replay {
    bool material = false, shading = false;
    xrt_material mat;                 // of mesh 0
    std::vector<float> colors;        // of the first triangles of mesh 2
    std::vector<std::pair<int, Body>> poses;
};

static int replay(xrt_scene *s, const std::vector<Mesh> &boxes, const std::vector<Mesh> &meshes, const Replay &r) {
    int rc;
    for (const auto &p : r.poses) {
        float bb[6];
        body_box(boxes, p.second, bb);
        const Pose q = pose_of(p.second, bb);
        const int32_t id = p.first;
        if ((rc = xrt_scene_set_poses(s, &id, 1, q.w, q.i, q.wb)) != XRT_OK) return rc;
    }
    const int32_t m0 = 0;
    if (r.material && (rc = xrt_scene_set_materials(s, &m0, 1, &r.mat)) != XRT_OK) return rc;
    if (r.shading) {
        const int n = (int)r.colors.size() / 4 < meshes[2].ntri ? (int)r.colors.size() / 4 : meshes[2].ntri;
        if ((rc = xrt_scene_set_triangle_shading(s, 2, nullptr, 0, n, nullptr, nullptr, r.colors.data())) != XRT_OK) return rc;
    }
    return XRT_OK;
}

// A scene of `meshes` and `bodies` (boxes from `boxes`) made from scratch and built, then the replay.
static xrt_scene *make(const std::vector<Mesh> &boxes, const std::vector<Mesh> &meshes, const std::vector<Body> &bodies, int sceneThreshold, const Replay *r) {
    xrt_scene *s = nullptr;
    if (xrt_scene_create(-1, &s) != XRT_OK) return nullptr;
    bool ok = true;
    for (const Mesh &m : meshes) ok = ok && add_mesh(s, m) == XRT_OK;
    for (size_t b = 0; ok && b < bodies.size(); b++) {
        float bb[6];
        body_box(boxes, bodies[b], bb);
        const Pose p = pose_of(bodies[b], bb);
        int32_t id = -1;
        ok = xrt_scene_add_object(s, bodies[b].meshes.data(), (int32_t)bodies[b].meshes.size(), p.w, p.i, bb, p.wb, &id) == XRT_OK;
    }
    if (!ok || xrt_scene_build(s, 8, sceneThreshold) != XRT_OK || (r && replay(s, boxes, meshes, *r) != XRT_OK)) { xrt_scene_destroy(s); return nullptr; }
    return s;
}

static bool file_bytes(xrt_scene *s, std::string &out) {
    char path[] = "/tmp/xrt_host_mesh_edit_XXXXXX";
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

static bool same_as_fresh(xrt_scene *s, const std::vector<Mesh> &boxes, const std::vector<Mesh> &meshes, const std::vector<Body> &bodies, int thr, const Replay &r, const char *step) {
    std::string a, b, ta, tb;
    xrt_scene *fresh = make(boxes, meshes, bodies, thr, &r);
    const bool ok = fresh && file_bytes(s, a) && file_bytes(fresh, b) && a == b && trees(s, (int)meshes.size(), ta) && trees(fresh, (int)meshes.size(), tb) && ta == tb;
    if (fresh) xrt_scene_destroy(fresh);
    if (!ok) fprintf(stderr, "host_mesh_edit: after '%s' the scene differs from a fresh scene's (file %zu / %zu bytes, trees %zu / %zu): %s\n", step, a.size(), b.size(), ta.size(), tb.size(), xrt_last_error());
    return ok;
}

int main() {
    if (xrt_version() != XRT_VERSION) return failed("xrt_version", xrt_version());
    for (int thr : {2, 20}) {
        const std::vector<Mesh> boxes{grid_mesh(6, 10.0f, 0.37f, 0.5f), grid_mesh(1, 10.0f, 0.37f, 0.25f), grid_mesh(9, 10.0f, 0.37f, 0.7f)};
        std::vector<Mesh> meshes = boxes;
        std::vector<Body> bodies;
        for (int i = 0; i < 5; i++) bodies.push_back(Body{{i % 3}, -60.0f + 30.0f * i, 0.0f, 3.0f * i, 1.0f});
        bodies.push_back(Body{{2, 0}, 0.0f, 40.0f, 0.0f, 1.5f});
        Replay r;
        xrt_scene *s = make(boxes, meshes, bodies, thr, nullptr);
        if (!s) return failed("making the scene", -1);
        int rc;
        auto step = [&](int32_t id, const Mesh &m, const char *what) -> bool {
            const xrt_material keep = meshes[(size_t)id].mat;
            meshes[(size_t)id] = m;
            meshes[(size_t)id].mat = keep;   // (the material stays the mesh's)
            if ((rc = set_triangles(s, id, m)) != XRT_OK) { failed(what, rc); return false; }
            return same_as_fresh(s, boxes, meshes, bodies, thr, r, what);
        };
        for (int32_t id : {0, 1, 2}) {
            if (id == 2) r.shading = false;   // (the triangle values of the replaced mesh are what the call gives)
            if (!step(id, grid_mesh(1, 10.0f, 0.2f, 0), "a single leaf")) return 1;
            if (!step(id, grid_mesh(14, 10.0f, 0.1f, 0), "a real octree")) return 1;
            if (!step(id, grid_mesh(14, 10.0f, 0.3f, 0), "the vertices moved")) return 1;
            if (id == 0) {   // edits that must survive the replacements that follow
                r.poses.push_back({3, Body{{0}, 12.0f, 7.0f, -20.0f, 2.0f}});
                r.material = true; r.mat = meshes[0].mat; r.mat.reflectiveness = 0.875f; r.mat.interpolate_normals = 1;
                r.shading = true;
                for (int k = 0; k < 8; k++) r.colors.push_back(0.125f * (float)k);
                if ((rc = replay(s, boxes, meshes, r)) != XRT_OK) return failed("the edits between the replacements", rc);
                meshes[0].mat = r.mat;
            }
            if (!step(id, grid_mesh(0, 10.0f, 0, 0), "no triangles")) return 1;
            if (!step(id, grid_mesh(id == 1 ? 40 : 5, 10.0f, 0.25f, 0), "a real mesh again")) return 1;
        }
        // calls that must be refused as a whole
        std::string before, after, tb, ta;
        if (!file_bytes(s, before) || !trees(s, 3, tb)) return failed("xrt_scene_save", -1);
        {
            const Mesh m = grid_mesh(3, 10.0f, 0.2f, 0);
            if ((rc = xrt_scene_set_mesh_triangles(nullptr, 0, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri, m.bbox)) != XRT_E_INVALID_ARG) return failed("a null scene", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, 3, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri, m.bbox)) != XRT_E_INVALID_ARG) return failed("a mesh id too large", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, -1, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri, m.bbox)) != XRT_E_INVALID_ARG) return failed("a negative mesh id", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, 1, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, -1, m.bbox)) != XRT_E_INVALID_ARG) return failed("ntri < 0", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, 1, nullptr, nullptr, nullptr, m.sn.data(), nullptr, m.ntri, m.bbox)) != XRT_E_INVALID_ARG) return failed("null v", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, 1, m.v.data(), nullptr, nullptr, nullptr, nullptr, m.ntri, m.bbox)) != XRT_E_INVALID_ARG) return failed("null surf_n", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, 1, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri, nullptr)) != XRT_E_INVALID_ARG) return failed("null bbox", rc);
            if ((rc = xrt_scene_set_mesh_triangles(s, 1, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, 1 << 28, m.bbox)) != XRT_E_INVALID_ARG) return failed("too many triangles", rc);
            // nine coincident triangles at mesh threshold 8: MeshOctree.BuildTree would not terminate (MO:84-96)
            Mesh heap = grid_mesh(1, 10.0f, 0.2f, 0);
            for (int k = 0; k < 8; k++) {
                heap.v.insert(heap.v.end(), m.v.begin(), m.v.begin() + 9); heap.n.insert(heap.n.end(), m.n.begin(), m.n.begin() + 9);
                heap.uv.insert(heap.uv.end(), m.uv.begin(), m.uv.begin() + 6); heap.sn.insert(heap.sn.end(), m.sn.begin(), m.sn.begin() + 3);
                heap.color.insert(heap.color.end(), m.color.begin(), m.color.begin() + 4);
                heap.ntri++;
            }
            if ((rc = set_triangles(s, 1, heap)) != XRT_E_UNSUPPORTED) return failed("more coincident triangles than the threshold", rc);
        }
        if (!file_bytes(s, after) || !trees(s, 3, ta) || before != after || tb != ta) { fprintf(stderr, "host_mesh_edit: a refused call changed the scene\n"); return 1; }
        // the defaults of n / uv / color, as in xrt_scene_add_mesh
        {
            Mesh m = grid_mesh(4, 10.0f, 0.2f, 0);
            if ((rc = xrt_scene_set_mesh_triangles(s, 1, m.v.data(), nullptr, nullptr, m.sn.data(), nullptr, m.ntri, m.bbox)) != XRT_OK) return failed("null n / uv / color", rc);
            m.n.assign(m.n.size(), 0.0f); m.uv.assign(m.uv.size(), 0.0f); m.color.assign(m.color.size(), 1.0f);
            const xrt_material keep = meshes[1].mat;
            meshes[1] = m; meshes[1].mat = keep;
            if (!same_as_fresh(s, boxes, meshes, bodies, thr, r, "null n / uv / color")) return 1;
        }
        // before the first build: the call edits what the build will use
        {
            xrt_scene *raw = nullptr;
            if (xrt_scene_create(-1, &raw) != XRT_OK) return failed("xrt_scene_create", -1);
            for (const Mesh &m : boxes) if ((rc = add_mesh(raw, m)) != XRT_OK) return failed("xrt_scene_add_mesh", rc);
            for (int32_t id = 0; id < 3; id++) if ((rc = set_triangles(raw, id, meshes[(size_t)id])) != XRT_OK) return failed("a call before the build", rc);
            std::string fa, fb;
            xrt_scene *fresh = nullptr;
            bool ok = xrt_scene_create(-1, &fresh) == XRT_OK;
            for (size_t k = 0; ok && k < 3; k++) { Mesh m = meshes[k]; m.mat = boxes[k].mat; ok = add_mesh(fresh, m) == XRT_OK; }
            ok = ok && xrt_scene_build(raw, 8, thr) == XRT_OK && xrt_scene_build(fresh, 8, thr) == XRT_OK && file_bytes(raw, fa) && file_bytes(fresh, fb) && fa == fb;
            xrt_scene_destroy(raw);
            if (fresh) xrt_scene_destroy(fresh);
            if (!ok) { fprintf(stderr, "host_mesh_edit: a call before the build did not edit what the build uses\n"); return 1; }
        }
        // save, load, build, destroy
        char path[] = "/tmp/xrt_host_mesh_edit_XXXXXX";
        const int fd = mkstemp(path);
        if (fd < 0) { perror("host_mesh_edit: mkstemp"); return 1; }
        close(fd);
        xrt_scene *loaded = nullptr;
        rc = xrt_scene_save(s, path);
        if (rc == XRT_OK) rc = xrt_scene_load(-1, path, &loaded);
        unlink(path);
        if (rc != XRT_OK) return failed("xrt_scene_save / xrt_scene_load", rc);
        if ((rc = xrt_scene_build(loaded, 8, thr)) != XRT_OK) return failed("xrt_scene_build (loaded scene)", rc);
        std::string fa, fb;
        if (!file_bytes(s, fa) || !file_bytes(loaded, fb) || fa != fb) { fprintf(stderr, "host_mesh_edit: the loaded scene differs\n"); return 1; }
        if ((rc = xrt_scene_destroy(s)) != XRT_OK) return failed("xrt_scene_destroy", rc);
        if ((rc = xrt_scene_destroy(loaded)) != XRT_OK) return failed("xrt_scene_destroy (loaded scene)", rc);
    }
    printf("host_mesh_edit: ok\n");
    return 0;
}
