// xrt_compose_hits / xrt_fold_samples and their device forms on a host-only scene (device -1), as a program of its own for a sanitizer build
// (csrc/Makefile `hostcheck_compose`): one mesh in one body, built.  What is wrong with the arguments alone is said first and in the header's
// order, each with its message although what follows it is wrong too -- scene, n, the outputs, the needed arrays, refract without reflect
// (samples for the fold), in the device forms the alignment --; n == 0 is XRT_OK; a call with nothing wrong reaches the scene and is
// XRT_E_NO_DEVICE; nothing is written by a call that fails.  Needs no GPU; prints "host_compose: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/xrt.h"

static int g_failed = 0;
static void expect(const char *what, int rc, int want, const char *needle = nullptr) {
    const char *msg = xrt_last_error();
    if (rc != want || (needle && !std::strstr(msg, needle))) {
        fprintf(stderr, "host_compose: %s returned %d (wanted %d%s%s): %s\n", what, rc, want, needle ? ", message with " : "", needle ? needle : "", msg);
        g_failed++;
    }
}

int main() {
    static const float IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    xrt_scene *s = nullptr;
    if (xrt_scene_create(-1, &s) != XRT_OK) { fprintf(stderr, "host_compose: xrt_scene_create: %s\n", xrt_last_error()); return 1; }
    const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, nn[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1}, uv[6] = {0, 0, 1, 0, 0, 1}, sn[3] = {0, 0, 1}, color[4] = {0.5f, 0.5f, 0.25f, 1.0f};
    const float box[6] = {0, 0, 0, 1, 1, 0};
    xrt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = 0.25f; mat.refraction_index = 1.0f;
    int32_t m0 = -1, b0 = -1;
    if (xrt_scene_add_mesh(s, v, nn, uv, sn, color, 1, &mat, box, &m0) != XRT_OK || xrt_scene_add_object(s, &m0, 1, IDENT, IDENT, box, box, &b0) != XRT_OK ||
        xrt_scene_build(s, 0, 0) != XRT_OK) {
        fprintf(stderr, "host_compose: scene: %s\n", xrt_last_error());
        return 1;
    }

    const int N = 5;
    std::vector<xrt_surface> surf(N);
    std::memset(surf.data(), 0, N * sizeof(xrt_surface));
    for (int i = 0; i < N; i++) { surf[i].flags = i == 1 ? 0 : (XRT_SURF_HIT | (i & 2 ? XRT_SURF_TRANSPARENT : 0)); surf[i].color[0] = 0.5f; surf[i].alpha = 0.5f; }
    std::vector<float> light(3 * N, 0.75f);
    std::vector<uint32_t> refl(N, 0xff102030u), refr(N, 0x00405060u), in16(16 * N, 0xff808080u);
    std::vector<uint32_t> rgba(N);
    std::vector<float> f32(3 * N);
    auto paint = [&]() { std::memset(rgba.data(), 0xab, N * sizeof(uint32_t)); std::memset(f32.data(), 0xab, 3 * N * sizeof(float)); };
    auto untouched = [&](const char *what) {
        const unsigned char *p[2] = {(const unsigned char *)rgba.data(), (const unsigned char *)f32.data()};
        const size_t len[2] = {N * sizeof(uint32_t), 3 * N * sizeof(float)};
        for (int k = 0; k < 2; k++)
            for (size_t i = 0; i < len[k]; i++)
                if (p[k][i] != 0xab) { fprintf(stderr, "host_compose: %s wrote output %d\n", what, k); g_failed++; return; }
    };
    xrt_stats st;
    paint();

    // ---- xrt_compose_hits: scene, n, the outputs, surface, light, refract without reflect -- each said although what follows it is wrong too
    expect("compose: null scene", xrt_compose_hits(nullptr, nullptr, nullptr, nullptr, refr.data(), -1, nullptr, nullptr, nullptr), XRT_E_INVALID_ARG, "xrt_compose_hits: null scene");
    expect("compose: n < 0", xrt_compose_hits(s, nullptr, nullptr, nullptr, refr.data(), -1, nullptr, nullptr, &st), XRT_E_INVALID_ARG, "xrt_compose_hits: n = -1");
    expect("compose: both outputs null", xrt_compose_hits(s, nullptr, nullptr, nullptr, refr.data(), N, nullptr, nullptr, &st), XRT_E_INVALID_ARG, "both outputs are null");
    expect("compose: null surface", xrt_compose_hits(s, nullptr, nullptr, nullptr, refr.data(), N, rgba.data(), f32.data(), &st), XRT_E_INVALID_ARG, "null surface");
    expect("compose: null light", xrt_compose_hits(s, surf.data(), nullptr, nullptr, refr.data(), N, rgba.data(), f32.data(), &st), XRT_E_INVALID_ARG, "null light");
    expect("compose: refract without reflect", xrt_compose_hits(s, surf.data(), light.data(), nullptr, refr.data(), N, rgba.data(), f32.data(), &st), XRT_E_INVALID_ARG,
           "refract_rgba without reflect_rgba");
    expect("compose: refract without reflect, n == 0", xrt_compose_hits(s, nullptr, nullptr, nullptr, refr.data(), 0, nullptr, nullptr, &st), XRT_E_INVALID_ARG,
           "refract_rgba without reflect_rgba");
    untouched("xrt_compose_hits with wrong arguments");
    // n == 0: XRT_OK whatever else is missing, nothing read, stats cleared
    std::memset(&st, 0xff, sizeof(st));
    expect("compose: n == 0", xrt_compose_hits(s, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &st), XRT_OK);
    if (st.pixels != 0 || st.shaded_hits != 0 || st.intersect_launches != 0) { fprintf(stderr, "host_compose: n == 0 left the stats alone\n"); g_failed++; }
    expect("compose: n == 0, no stats", xrt_compose_hits(s, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr), XRT_OK);
    // nothing wrong: the scene is looked at, and it has no device -- every branch, each output alone
    expect("compose: RT:726", xrt_compose_hits(s, surf.data(), light.data(), nullptr, nullptr, N, rgba.data(), f32.data(), &st), XRT_E_NO_DEVICE, "host-only");
    expect("compose: RT:584", xrt_compose_hits(s, surf.data(), light.data(), refl.data(), nullptr, N, rgba.data(), nullptr, &st), XRT_E_NO_DEVICE, "host-only");
    expect("compose: RT:699", xrt_compose_hits(s, surf.data(), light.data(), refl.data(), refr.data(), N, nullptr, f32.data(), nullptr), XRT_E_NO_DEVICE, "host-only");
    untouched("xrt_compose_hits without a device");

    // ---- the device form: pointers are only compared and never read on a host-only scene
    void *const S = (void *)(uintptr_t)0x10000, *const L = (void *)(uintptr_t)0x20000, *const R = (void *)(uintptr_t)0x30000, *const T = (void *)(uintptr_t)0x40000,
               *const O = (void *)(uintptr_t)0x50000, *const F = (void *)(uintptr_t)0x60000;
    auto dev = [&](void *a, void *l, void *r, void *t, int64_t n, void *o, void *f) { return xrt_compose_hits_device(s, a, l, r, t, n, o, f, nullptr, nullptr); };
    expect("compose device: null scene", xrt_compose_hits_device(nullptr, S, L, R, T, N, O, F, nullptr, nullptr), XRT_E_INVALID_ARG, "xrt_compose_hits_device: null scene");
    expect("compose device: n < 0", dev(nullptr, nullptr, nullptr, T, -1, nullptr, nullptr), XRT_E_INVALID_ARG, "n = -1");
    expect("compose device: both outputs null", dev(nullptr, nullptr, nullptr, T, N, nullptr, nullptr), XRT_E_INVALID_ARG, "both outputs are null");
    expect("compose device: null surface", dev(nullptr, nullptr, nullptr, T, N, O, nullptr), XRT_E_INVALID_ARG, "null surface");
    expect("compose device: null light", dev(S, nullptr, nullptr, T, N, nullptr, F), XRT_E_INVALID_ARG, "null light");
    expect("compose device: refract without reflect", dev((char *)S + 4, L, nullptr, T, N, O, F), XRT_E_INVALID_ARG, "refract_rgba without reflect_rgba");
    void *const all[6] = {S, L, R, T, O, F};
    for (int k = 0; k < 6; k++) {
        void *p[6];
        for (int j = 0; j < 6; j++) p[j] = j == k ? (void *)((char *)all[j] + (4 << (k % 2))) : all[j];
        expect("compose device: misaligned", dev(p[0], p[1], p[2], p[3], N, p[4], p[5]), XRT_E_INVALID_ARG, "16-byte");
        expect("compose device: misaligned, n == 0", dev(p[0], p[1], p[2], p[3], 0, p[4], p[5]), XRT_E_INVALID_ARG, "16-byte");
    }
    expect("compose device: n == 0", dev(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr), XRT_OK);
    expect("compose device: valid", dev(S, L, R, T, N, O, F), XRT_E_NO_DEVICE, "host-only");
    expect("compose device: valid, in place", dev(S, L, R, T, N, R, nullptr), XRT_E_NO_DEVICE);
    expect("compose device: valid, RT:726", dev(S, L, nullptr, nullptr, N, nullptr, F), XRT_E_NO_DEVICE);

    // ---- xrt_fold_samples: scene, n, samples, rgba_out, rgba_in
    expect("fold: null scene", xrt_fold_samples(nullptr, nullptr, -1, 5, nullptr, nullptr, nullptr), XRT_E_INVALID_ARG, "xrt_fold_samples: null scene");
    expect("fold: n < 0", xrt_fold_samples(s, nullptr, -1, 5, nullptr, nullptr, &st), XRT_E_INVALID_ARG, "xrt_fold_samples: n = -1");
    for (int bad : {0, 1, 5, 8, 15, 17, 64, -4})
        expect("fold: samples", xrt_fold_samples(s, nullptr, N, bad, nullptr, nullptr, &st), XRT_E_INVALID_ARG, "neither 4 nor 16");
    expect("fold: samples, n == 0", xrt_fold_samples(s, nullptr, 0, 1, nullptr, nullptr, &st), XRT_E_INVALID_ARG, "samples = 1");
    expect("fold: null rgba_out", xrt_fold_samples(s, nullptr, N, 16, nullptr, f32.data(), &st), XRT_E_INVALID_ARG, "null rgba_out");
    expect("fold: null rgba_in", xrt_fold_samples(s, nullptr, N, 4, rgba.data(), f32.data(), &st), XRT_E_INVALID_ARG, "null rgba_in");
    untouched("xrt_fold_samples with wrong arguments");
    std::memset(&st, 0xff, sizeof(st));
    expect("fold: n == 0", xrt_fold_samples(s, nullptr, 0, 16, nullptr, nullptr, &st), XRT_OK);
    if (st.pixels != 0 || st.shaded_hits != 0) { fprintf(stderr, "host_compose: fold n == 0 left the stats alone\n"); g_failed++; }
    expect("fold: valid, 16", xrt_fold_samples(s, in16.data(), N, 16, rgba.data(), f32.data(), &st), XRT_E_NO_DEVICE, "host-only");
    expect("fold: valid, 4", xrt_fold_samples(s, in16.data(), N, 4, rgba.data(), nullptr, nullptr), XRT_E_NO_DEVICE, "host-only");
    untouched("xrt_fold_samples without a device");
    auto fdev = [&](void *in, int64_t n, int32_t k, void *o, void *f) { return xrt_fold_samples_device(s, in, n, k, o, f, nullptr, nullptr); };
    expect("fold device: null scene", xrt_fold_samples_device(nullptr, S, N, 16, O, F, nullptr, nullptr), XRT_E_INVALID_ARG, "xrt_fold_samples_device: null scene");
    expect("fold device: n < 0", fdev(nullptr, -1, 3, nullptr, nullptr), XRT_E_INVALID_ARG, "n = -1");
    expect("fold device: samples", fdev(nullptr, N, 3, nullptr, nullptr), XRT_E_INVALID_ARG, "samples = 3");
    expect("fold device: null rgba_out", fdev(nullptr, N, 16, nullptr, F), XRT_E_INVALID_ARG, "null rgba_out");
    expect("fold device: null rgba_in", fdev(nullptr, N, 16, (char *)O + 4, F), XRT_E_INVALID_ARG, "null rgba_in");
    expect("fold device: misaligned in", fdev((char *)S + 8, N, 16, O, F), XRT_E_INVALID_ARG, "16-byte");
    expect("fold device: misaligned out", fdev(S, N, 4, (char *)O + 4, F), XRT_E_INVALID_ARG, "16-byte");
    expect("fold device: misaligned float out", fdev(S, N, 4, O, (char *)F + 12), XRT_E_INVALID_ARG, "16-byte");
    expect("fold device: n == 0", fdev(nullptr, 0, 4, nullptr, nullptr), XRT_OK);
    expect("fold device: valid", fdev(S, N, 16, O, F), XRT_E_NO_DEVICE, "host-only");
    expect("fold device: valid, no floats", fdev(S, N, 4, O, nullptr), XRT_E_NO_DEVICE);

    // a scene that was never built: the arguments first, then the device
    {
        xrt_scene *u = nullptr;
        if (xrt_scene_create(-1, &u) != XRT_OK) { fprintf(stderr, "host_compose: second scene\n"); return 1; }
        expect("unbuilt scene: compose arguments", xrt_compose_hits(u, surf.data(), light.data(), nullptr, refr.data(), N, rgba.data(), nullptr, nullptr), XRT_E_INVALID_ARG, "refract_rgba");
        expect("unbuilt scene: compose", xrt_compose_hits(u, surf.data(), light.data(), nullptr, nullptr, N, rgba.data(), nullptr, nullptr), XRT_E_NO_DEVICE);
        expect("unbuilt scene: fold", xrt_fold_samples(u, in16.data(), N, 16, rgba.data(), nullptr, nullptr), XRT_E_NO_DEVICE);
        xrt_scene_destroy(u);
    }
    untouched("the calls on an unbuilt scene");
    xrt_scene_destroy(s);
    if (g_failed) { fprintf(stderr, "host_compose: %d checks failed\n", g_failed); return 1; }
    printf("host_compose: ok\n");
    return 0;
}
