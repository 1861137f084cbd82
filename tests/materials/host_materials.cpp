// xrt_scene_set_materials on a host-only scene (device -1), as a program of its own for a sanitizer build (csrc/Makefile `hostcheck`): two
// meshes, one textured, built; then every texel case of the header -- texels replaced by the same size and by another size, with and without
// a premultiplied copy, UseTexture off (the texels stay), on again with NULL texels, texels stored while the flag is off --, a duplicate id,
// and one call that must be rejected as a whole.  After every step the scene is saved and the file compared with the file of a scene made
// from scratch with the materials the step should have left.  Then save, load, build, destroy.  What it checks beyond the return codes:
// that all of this is clean on the host under AddressSanitizer, UBSan and LeakSanitizer.  Needs no GPU; prints "host_materials: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/xrt.h"

static int failed(const char *what, int rc) {
    fprintf(stderr, "host_materials: %s returned %d: %s\n", what, rc, xrt_last_error());
    return 1;
}

static const float V[18] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}, N[18] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
static const float UV[12] = {0, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0}, SN[6] = {0, 0, 1, 0, 0, 1}, COLOR[8] = {1, 0.5f, 0.25f, 1, 0.2f, 0.4f, 0.6f, 1};
static const float BBOX[6] = {0, 0, 0, 1, 1, 0}, IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static std::vector<uint32_t> texture(int w, int h, uint32_t seed) {
    std::vector<uint32_t> t((size_t)w * h);
    for (size_t i = 0; i < t.size(); i++) t[i] = 0xff000000u ^ (seed * 2654435761u + (uint32_t)i * 40503u);
    return t;
}

// A scene of the two meshes with materials m0 / m1 and one body of both; built when `build`.
static xrt_scene *make(const xrt_material &m0, const xrt_material &m1, bool build) {
    xrt_scene *s = nullptr;
    int32_t ids[2] = {-1, -1}, body = -1;
    if (xrt_scene_create(-1, &s) != XRT_OK) return nullptr;
    if (xrt_scene_add_mesh(s, V, N, UV, SN, COLOR, 2, &m0, BBOX, &ids[0]) != XRT_OK || xrt_scene_add_mesh(s, V, N, UV, SN, COLOR, 1, &m1, BBOX, &ids[1]) != XRT_OK ||
        xrt_scene_add_object(s, ids, 2, IDENT, IDENT, BBOX, BBOX, &body) != XRT_OK || (build && xrt_scene_build(s, 0, 0) != XRT_OK)) {
        xrt_scene_destroy(s);
        return nullptr;
    }
    return s;
}

static bool file_bytes(xrt_scene *s, std::string &out) {
    char path[] = "/tmp/xrt_host_materials_XXXXXX";
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

// Does `s` save the file a scene made from scratch with m0 / m1 saves?
static bool same_as_fresh(xrt_scene *s, const xrt_material &m0, const xrt_material &m1, const char *step) {
    std::string a, b;
    xrt_scene *fresh = make(m0, m1, true);
    const bool ok = fresh && file_bytes(s, a) && file_bytes(fresh, b) && a == b;
    if (fresh) xrt_scene_destroy(fresh);
    if (!ok) fprintf(stderr, "host_materials: after '%s' the scene file differs from a fresh scene's (%zu / %zu bytes): %s\n", step, a.size(), b.size(), xrt_last_error());
    return ok;
}

int main() {
    if (xrt_version() != XRT_VERSION) return failed("xrt_version", xrt_version());
    const std::vector<uint32_t> t43 = texture(4, 3, 1), t43b = texture(4, 3, 2), t52 = texture(5, 2, 3), p52 = texture(5, 2, 4), t22 = texture(2, 2, 5);
    xrt_material plain, tex;
    std::memset(&plain, 0, sizeof(plain));
    plain.reflectiveness = 0.25f; plain.refraction_index = 1.0f;
    tex = plain;
    tex.use_texture = 1; tex.tex_width = 4; tex.tex_height = 3; tex.tex_argb = t43.data();

    for (int pass = 0; pass < 2; pass++) {   // the updates after the build, and before it
        const bool built = pass == 0;
        xrt_scene *s = make(tex, plain, built);
        if (!s) return failed("making the scene", -1);
        const int32_t m0 = 0, m1 = 1;
        int rc;
        xrt_material a = tex, b = plain;
        auto step = [&](const char *what, const int32_t *ids, int n, const xrt_material *mats, const xrt_material &want0, const xrt_material &want1) -> bool {
            if ((rc = xrt_scene_set_materials(s, ids, n, mats)) != XRT_OK) { failed(what, rc); return false; }
            return !built || same_as_fresh(s, want0, want1, what);
        };
        // scalars
        a.reflectiveness = 0.75f; a.transparent = 1; a.refraction_index = 1.32f; a.interpolate_normals = 1; a.tex_argb = nullptr; a.tex_width = a.tex_height = 0;
        xrt_material want0 = a;
        want0.tex_argb = t43.data(); want0.tex_width = 4; want0.tex_height = 3;
        if (!step("scalars, texels kept", &m0, 1, &a, want0, plain)) return 1;
        // texels of the same size
        a.tex_argb = t43b.data(); a.tex_width = 4; a.tex_height = 3;
        if (!step("texels of the same size", &m0, 1, &a, a, plain)) return 1;
        // texels of another size with a premultiplied copy
        a.tex_argb = t52.data(); a.tex_pargb = p52.data(); a.tex_width = 5; a.tex_height = 2;
        if (!step("texels of another size", &m0, 1, &a, a, plain)) return 1;
        // UseTexture off: the flag only
        xrt_material off = a;
        off.use_texture = 0; off.tex_argb = off.tex_pargb = nullptr; off.tex_width = off.tex_height = 0;
        if (!step("use_texture off", &m0, 1, &off, off, plain)) return 1;
        // ... and on again with NULL texels and the stored size
        xrt_material on = off;
        on.use_texture = 1; on.tex_width = 5; on.tex_height = 2;
        if (!step("use_texture on, texels kept", &m0, 1, &on, a, plain)) return 1;
        // texels stored while the flag is off, on the mesh that had none; then switched on; the same mesh twice in one call: the last entry wins
        b.tex_argb = t22.data(); b.tex_width = b.tex_height = 2;
        if (!step("texels stored with use_texture 0", &m1, 1, &b, a, plain)) return 1;
        xrt_material twice[2] = {plain, plain};
        twice[0].reflectiveness = 0.9f;
        twice[1].use_texture = 1; twice[1].reflectiveness = 0.5f;
        const int32_t both[2] = {1, 1};
        xrt_material want1 = twice[1];
        want1.tex_argb = t22.data(); want1.tex_width = want1.tex_height = 2;
        if (!step("a mesh listed twice", both, 2, twice, a, want1)) return 1;
        // a call that must be rejected as a whole: its third entry asks mesh 0 for kept texels of a size it does not have
        std::string before, after;
        if (built && !file_bytes(s, before)) return failed("xrt_scene_save", -1);
        xrt_material bad[3] = {plain, plain, on};
        bad[0].reflectiveness = 0.1f; bad[1].transparent = 1; bad[2].tex_width = 7;
        const int32_t ids3[3] = {0, 1, 0};
        if ((rc = xrt_scene_set_materials(s, ids3, 3, bad)) != XRT_E_INVALID_ARG) return failed("a call with a bad entry", rc);
        const int32_t outOfRange = 2;
        if ((rc = xrt_scene_set_materials(s, &outOfRange, 1, &plain)) != XRT_E_INVALID_ARG) return failed("a mesh id out of range", rc);
        if ((rc = xrt_scene_set_materials(s, &m0, 0, nullptr)) != XRT_OK) return failed("n == 0", rc);
        if (built && (!file_bytes(s, after) || before != after)) { fprintf(stderr, "host_materials: a rejected call changed the scene\n"); return 1; }
        if (!built) {
            if ((rc = xrt_scene_build(s, 0, 0)) != XRT_OK) return failed("xrt_scene_build", rc);
            if (!same_as_fresh(s, a, want1, "updates before the build")) return 1;
        }
        // save, load, build, destroy
        char path[] = "/tmp/xrt_host_materials_XXXXXX";
        const int fd = mkstemp(path);
        if (fd < 0) { perror("host_materials: mkstemp"); return 1; }
        close(fd);
        xrt_scene *loaded = nullptr;
        rc = xrt_scene_save(s, path);
        if (rc == XRT_OK) rc = xrt_scene_load(-1, path, &loaded);
        unlink(path);
        if (rc != XRT_OK) return failed("xrt_scene_save / xrt_scene_load", rc);
        if ((rc = xrt_scene_build(loaded, 0, 0)) != XRT_OK) return failed("xrt_scene_build (loaded scene)", rc);
        if (!same_as_fresh(loaded, a, want1, "load")) return 1;
        if ((rc = xrt_scene_destroy(s)) != XRT_OK) return failed("xrt_scene_destroy", rc);
        if ((rc = xrt_scene_destroy(loaded)) != XRT_OK) return failed("xrt_scene_destroy (loaded scene)", rc);
    }
    printf("host_materials: ok\n");
    return 0;
}
