// host_coherent.cpp -- what xrt_render_opts.list_order == XRT_LIST_COHERENT decides on the host, checked without a device: the byte accounting of a hinted
// chunk of xrt_render_pixels (csrc/pixels_plan.h: the packet table is part of it), the capacity of that table, and the packet mask plan_frame (csrc/frame_plan.h)
// gives a hinted batch -- the mask of a frame of the same scene and sampling -- against the mask of an unhinted one, and scene_packet_mask / scene_answers_at_emission
// (the one statement of both rules, read by plan_frame and by the list calls that trace outside a frame) against plan_frame over every scene kind, packetOk and XRT_PACKET.  The scenes are filled by hand as in
// tests/frame_plan/host_plan.cpp (device -1: no HIP function is called).  Built by `make hostcheck_coherent` (csrc/Makefile) from the library's own sources,
// host code under ASan and UBSan, and run by tests/test_coherent_cpu.py.  Prints "host_coherent: ok".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/xrt.h"
#include "../../xna-ray-trace_amd/csrc/device_res.h"

using namespace xrt;

#include "../../xna-ray-trace_amd/csrc/pixels.h"
#include "../../xna-ray-trace_amd/csrc/pixels_plan.h"
#include "../../xna-ray-trace_amd/csrc/scene_state.h"

static int g_failures = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        if (!(cond)) {                                                   \
            if (g_failures++ < 40) {                                     \
                std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                                \
                std::printf("\n");                                       \
            }                                                            \
        }                                                                \
    } while (0)

// ---- chunks ------------------------------------------------------------------------------------------------------------------------------
// Every entry once, in order, starts on multiples of 4 entries, no chunk over the ray limit; with the table's bytes no chunk over the budget; and the
// unhinted plan is the plan of the five-argument form.
static void check_chunks(long long n, int mode, int quality, int lights, uint64_t budget) {
    const std::vector<long long> plain = pixel_chunks(n, mode, quality, lights, budget), off = pixel_chunks(n, mode, quality, lights, budget, false);
    CHECK(plain == off, "n %lld: coherent = false is not the plan as it was", n);
    CHECK(pixel_chunk_entries(mode, quality, lights, budget) == pixel_chunk_entries(mode, quality, lights, budget, false), "entries, unhinted");
    const std::vector<long long> b = pixel_chunks(n, mode, quality, lights, budget, true);
    const long long samples = pixel_samples(mode);
    const uint64_t per = pixel_entry_bytes(mode, quality, lights);
    CHECK(!b.empty() && b.front() == 0 && b.back() == (n > 0 ? n : 0), "n %lld", n);
    CHECK(b.size() >= plain.size(), "n %lld: %zu hinted chunks, %zu unhinted", n, b.size() - 1, plain.size() - 1);   // (the table only ever takes room)
    const bool roomForFour = budget >= pixel_chunk_bytes(4, mode, quality, lights, true);
    for (size_t c = 0; c + 1 < b.size(); c++) {
        const long long m = b[c + 1] - b[c];
        CHECK(m > 0 && b[c] % 4 == 0, "n %lld chunk %zu: %lld entries from %lld", n, c, m, b[c]);
        CHECK(m * samples <= PIXEL_CHUNK_MAX_RAYS, "n %lld chunk %zu has %lld rays", n, c, m * samples);
        const uint64_t bytes = pixel_chunk_bytes(m, mode, quality, lights, true);
        CHECK(bytes == (uint64_t)m * per + 512u + 8u * (uint64_t)((m * samples + 63) / 64), "n %lld chunk %zu: %" PRIu64 " bytes", n, c, bytes);
        if (roomForFour) CHECK(bytes <= budget, "n %lld chunk %zu: %" PRIu64 " bytes with its table over %" PRIu64, n, c, bytes, budget);
        else CHECK(m <= 4, "n %lld chunk %zu: %lld entries under a budget below four entries", n, c, m);
        CHECK(c + 2 == b.size() || m == b[1] - b[0], "n %lld chunk %zu: %lld entries, the first has %lld", n, c, m, b[1] - b[0]);
    }
    if (n > 0 && pixel_chunk_bytes(n, mode, quality, lights, true) <= budget && n * samples <= PIXEL_CHUNK_MAX_RAYS) CHECK(b.size() == 2, "n %lld fits and is %zu chunks", n, b.size() - 1);
}

// ---- plans -------------------------------------------------------------------------------------------------------------------------------
enum Kind { ONE_BODY = 0, TWO_LEVEL };

static void fill_scene(xrt_scene &s, Kind kind) {   // (tests/frame_plan/host_plan.cpp: what the planner reads of a scene)
    s.device = -1;
    s.cfg = Settings();
    s.hs.arrays.snodes.assign(2, f4{0, 0, 0, 0});
    s.hs.arrays.snodes[0] = f4{-1.0f, -1.0f, -11.0f, 0.0f};
    s.hs.arrays.snodes[1] = f4{1.0f, 1.0f, -9.0f, 0.0f};
    MeshRec m;
    std::memset(&m, 0, sizeof(m));
    m.nbMin[0] = -0.2f; m.nbMax[0] = 0.2f; m.nbMin[1] = 0.9f; m.nbMax[1] = 1.0f; m.nbMin[2] = -0.2f; m.nbMax[2] = 0.2f;
    s.hs.arrays.meshes.assign(1, m);
    s.sceneMode = kind == TWO_LEVEL ? MODE_SCENE : MODE_SINGLE;
    s.packetOk = true;
    s.deepMeshes = true;
    s.view.nodeCull = 1;
    s.heavyPath = kind == TWO_LEVEL ? 0.0f : 0.25f;
    s.mat[0].anyTransparent = false;
    s.lastFrameMs = 1.0f;
    s.wallClockKHz = 100000;
}

static xrt_camera camera(int w, int h) {
    xrt_camera c;
    std::memset(&c, 0, sizeof(c));
    for (int i = 0; i < 4; i++) c.view[5 * i] = 1.0f;
    const float nearZ = 0.1f, farZ = 100.0f, t = 1.0f / std::tan(0.5f * 1.0471976f);
    c.proj[0] = t * (float)h / (float)w; c.proj[5] = t; c.proj[10] = farZ / (nearZ - farZ); c.proj[11] = -1.0f; c.proj[14] = nearZ * farZ / (nearZ - farZ);
    c.vp_width = w; c.vp_height = h; c.vp_min_depth = 0.0f; c.vp_max_depth = 1.0f;
    return c;
}

static xrt_render_opts opts_of(int ms) {
    xrt_render_opts o;
    std::memset(&o, 0, sizeof(o));
    o.max_reflections = 1; o.use_multisampling = ms; o.address_mode = XRT_ADDRESS_WRAP; o.filtering = XRT_FILTER_POINT;
    return o;
}

// The mask of the frame of `ms`, and of a batch of that frame's rays: unhinted, hinted (xrt_cast_rays), hinted with the fused generation (xrt_render_pixels).
static void check_masks(Kind kind, int ms, int packetEnv) {
    xrt_scene s;
    fill_scene(s, kind);
    s.cfg.packetMask = packetEnv;   // XRT_PACKET (-1: not set)
    const int w = 64, h = 27, samples = pixel_samples(ms);
    const xrt_camera cam = camera(w, h);
    xrt_light light;
    std::memset(&light, 0, sizeof(light));
    light.kind = XRT_LIGHT_SPOT; light.direction[1] = -1.0f; light.intensity = 1.0f; light.spot_angle = 1.0f; light.decay_exponent = 1.3f;
    const xrt_render_opts of = opts_of(ms), ob = opts_of(XRT_MS_OFF);
    FramePlan frame, plain, hinted, fused;
    int rc = plan_frame(s, 0, &cam, &light, 1, &of, false, false, 0, 1, true, nullptr, frame);
    CHECK(rc == XRT_OK, "frame: %d", rc);
    xrt_ray dummy;
    std::memset(&dummy, 0, sizeof(dummy));
    BatchSrc b;
    b.rays = &dummy; b.n = (long long)w * h * samples; b.refIndex = 1.0f;
    rc = plan_frame(s, 0, nullptr, &light, 1, &ob, false, false, 0, 1, true, &b, plain);
    CHECK(rc == XRT_OK, "unhinted batch: %d", rc);
    b.coherent = true; b.samples = samples;
    rc = plan_frame(s, 0, nullptr, &light, 1, &ob, false, false, 0, 1, true, &b, hinted);
    CHECK(rc == XRT_OK, "hinted batch: %d", rc);
    PixelGenArgs gen;
    gen.mode = samples == 16 ? PIXEL_FIXED16 : (samples == 4 ? PIXEL_QUADRANT : PIXEL_ONE);
    b.rays = nullptr; b.gen = &gen;
    rc = plan_frame(s, 0, nullptr, &light, 1, &ob, false, false, 0, 1, true, &b, fused);
    CHECK(rc == XRT_OK, "fused batch: %d", rc);
    const char *kn = kind == TWO_LEVEL ? "two-level" : "one-body";
    // the frame's rule: two-level scenes in every generation at any sample count; one-body scenes only with 16 samples
    if (packetEnv < 0) CHECK(frame.pkMask == (kind == TWO_LEVEL ? 23 : (samples == 16 ? 7 : 0)), "%s, %d samples: frame mask %d", kn, samples, frame.pkMask);
    else CHECK(frame.pkMask == packetEnv, "%s, %d samples, XRT_PACKET=%d: frame mask %d", kn, samples, packetEnv, frame.pkMask);
    CHECK(hinted.pkMask == frame.pkMask && fused.pkMask == frame.pkMask, "%s, %d samples: hinted %d fused %d frame %d", kn, samples, hinted.pkMask, fused.pkMask, frame.pkMask);
    if (packetEnv < 0) {
        // an unhinted batch keeps generation 0 away from the packet kernel, and knows nothing of the sampling its rays were made with
        const int asOneSample = kind == TWO_LEVEL ? 23 : 0;
        CHECK(plain.pkMask == (asOneSample & ~1), "%s, %d samples: unhinted mask %d", kn, samples, plain.pkMask);
        CHECK((plain.pkMask & 1) == 0, "%s: an unhinted batch sends generation 0 to the packet kernel", kn);
        CHECK((hinted.pkMask != plain.pkMask) == ((frame.pkMask & 1) != 0), "%s, %d samples: hinted %d unhinted %d", kn, samples, hinted.pkMask, plain.pkMask);
    } else CHECK(plain.pkMask == packetEnv, "XRT_PACKET overrides an unhinted batch too: %d", plain.pkMask);
    // the table: only the fused generation writes one, where launch #0 is a packet launch; one entry per 64 places of the chunk
    CHECK(plain.pkEntries == 0 && hinted.pkEntries == 0, "%s, %d samples: a batch of rays has a table (%zu, %zu)", kn, samples, plain.pkEntries, hinted.pkEntries);
    CHECK(fused.pkEntries == ((fused.pkMask & 1) ? (size_t)pixel_table_entries((uint64_t)fused.P) : 0), "%s, %d samples: %zu entries for %d paths", kn, samples, fused.pkEntries, fused.P);
    CHECK(fused.P == w * h * samples && fused.batch && !fused.fast, "%s: the fused batch is a batch", kn);
    // nothing else of the plan moves with the hint
    CHECK(hinted.P == plain.P && hinted.rayCap == plain.rayCap && hinted.ae == plain.ae && hinted.finishA == plain.finishA && hinted.heap == plain.heap &&
              hinted.cntStride == plain.cntStride && hinted.qStride == plain.qStride && hinted.lvlStride == plain.lvlStride,
          "%s, %d samples: the hint changes more than the mask", kn, samples);
    s.cfg.packetQuads = false;   // XRT_PK_QUADS=0: no table anywhere, the mask as it was
    rc = plan_frame(s, 0, nullptr, &light, 1, &ob, false, false, 0, 1, true, &b, fused);
    CHECK(rc == XRT_OK && fused.pkEntries == 0 && fused.pkMask == frame.pkMask, "%s: XRT_PK_QUADS=0", kn);
}

// scene_packet_mask (csrc/frame_plan.h), the rule the list calls outside a frame read (xrt_trace_pixels bit 0, xrt_light_hits bit 1), is the mask plan_frame gives a
// coherent batch of the same sampling -- and, at one ray per entry and bit 0 cleared, an unordered one where XRT_PACKET is not set -- whatever the scene kind, packetOk and XRT_PACKET; and
// scene_answers_at_emission is the `ae` of a one-chunk batch.  A material version without Transparent materials (no ray tree).
static int check_scene_masks() {
    int n = 0;
    for (Kind kind : {ONE_BODY, TWO_LEVEL})
        for (bool packetOk : {false, true})
            for (int env : {-1, 0, 1, 2, 7, 23, 31})
                for (int samples : {1, 4, 16}) {
                    xrt_scene s;
                    fill_scene(s, kind);
                    s.packetOk = packetOk; s.cfg.packetMask = env;
                    xrt_light light;
                    std::memset(&light, 0, sizeof(light));
                    light.kind = XRT_LIGHT_SPOT; light.direction[1] = -1.0f; light.intensity = 1.0f; light.spot_angle = 1.0f; light.decay_exponent = 1.3f;
                    const xrt_render_opts ob = opts_of(XRT_MS_OFF);
                    xrt_ray dummy;
                    std::memset(&dummy, 0, sizeof(dummy));
                    BatchSrc b;
                    b.rays = &dummy; b.n = 64LL * 27 * samples; b.refIndex = 1.0f;
                    FramePlan plain, hinted;
                    int rc = plan_frame(s, 0, nullptr, &light, 1, &ob, false, false, 0, 1, true, &b, plain);
                    CHECK(rc == XRT_OK, "unordered batch: %d", rc);
                    b.coherent = true; b.samples = samples;
                    rc = plan_frame(s, 0, nullptr, &light, 1, &ob, false, false, 0, 1, true, &b, hinted);
                    CHECK(rc == XRT_OK, "coherent batch: %d", rc);
                    const int mask = scene_packet_mask(s, samples);
                    CHECK(mask == hinted.pkMask, "kind %d packetOk %d XRT_PACKET %d, %d samples: scene_packet_mask %d, the coherent batch's plan %d", (int)kind, (int)packetOk, env, samples, mask, hinted.pkMask);
                    // (an unordered batch knows nothing of the sampling its rays were made with: its own is one ray per entry, so a one-body scene's 16-sample rule does not reach it)
                    if (env < 0) CHECK((scene_packet_mask(s, 1) & ~1) == plain.pkMask, "kind %d packetOk %d, %d samples: scene_packet_mask(1) %d, the unordered batch's plan %d", (int)kind, (int)packetOk, samples, scene_packet_mask(s, 1), plain.pkMask);
                    if (env < 0 && (kind == TWO_LEVEL || samples < 16)) CHECK((mask & ~1) == plain.pkMask, "kind %d, %d samples: %d against %d", (int)kind, samples, mask, plain.pkMask);
                    CHECK(mask == (!packetOk ? 0 : (env >= 0 ? env : (kind == TWO_LEVEL ? 23 : (samples >= 16 ? 7 : 0)))), "kind %d packetOk %d XRT_PACKET %d, %d samples: mask %d", (int)kind, (int)packetOk, env, samples, mask);
                    CHECK(hinted.P == (int)b.n && hinted.ae == scene_answers_at_emission(s) && plain.ae == hinted.ae && hinted.ae == (kind == ONE_BODY),
                          "kind %d: ae %d / %d, scene_answers_at_emission %d", (int)kind, (int)plain.ae, (int)hinted.ae, (int)scene_answers_at_emission(s));
                    n++;
                }
    return n;
}

int main() {
    const int modes[3] = {XRT_MS_OFF, XRT_MS_ADAPTIVE, XRT_MS_FIXED16};
    // chunk sizes with the table included
    const long long ns[] = {0, 1, 3, 4, 5, 63, 64, 65, 4096, 4097, 5184, 1920LL * 1080, 3840LL * 2160, (1LL << 27) + 1, 1LL << 28, (1LL << 31) + 7};
    const uint64_t budgets[] = {1, 600, 1000, 200000, 1 << 20, 1ull << 30, 4ull << 30, 1ull << 40, ~0ull};
    int plans = 0;
    for (int mode : modes)
        for (int quality : {0, 2, 6})
            for (int lights : {0, 1, 100})
                for (long long n : ns)
                    for (uint64_t budget : budgets) {
                        if (n / pixel_chunk_entries(mode, quality, lights, budget, true) > (1 << 20)) continue;   // (more than a million chunks say nothing more)
                        check_chunks(n, mode, quality, lights, budget);
                        plans++;
                    }
    // a 1080p list of 16 samples under the default budget: two chunks unhinted (profiles/pixels), and the table (4 MB of 6.6 GB) does not make it three
    CHECK(pixel_chunks(1920LL * 1080, XRT_MS_FIXED16, 0, 1, 4ull << 30).size() == 3 && pixel_chunks(1920LL * 1080, XRT_MS_FIXED16, 0, 1, 4ull << 30, true).size() == 3, "1080p x 16");
    // a budget that holds exactly m entries unhinted holds fewer with the table
    CHECK(pixel_chunk_entries(XRT_MS_OFF, 0, 1, 200 * 1000) == 1000 && pixel_chunk_entries(XRT_MS_OFF, 0, 1, 200 * 1000, true) == 996, "entries with the table: %lld",
          pixel_chunk_entries(XRT_MS_OFF, 0, 1, 200 * 1000, true));
    CHECK(pixel_chunk_bytes(996, XRT_MS_OFF, 0, 1, true) == 996 * 200 + 512 + 8 * 16, "bytes of 996 one-sample entries");
    // table capacity: one entry per 64 places, the last unit partial
    const struct { uint64_t rays, entries; } caps[] = {{0, 0}, {1, 1}, {63, 1}, {64, 1}, {65, 2}, {4095, 64}, {4096, 64}, {4097, 65}, {16 * 257, 65}, {4 * 17, 2}, {1ull << 28, 1ull << 22}};
    for (const auto &c : caps) {
        CHECK(pixel_table_entries(c.rays) == c.entries, "%" PRIu64 " rays: %" PRIu64 " entries", c.rays, pixel_table_entries(c.rays));
        CHECK(pixel_table_bytes(c.rays) == 512 + 8 * c.entries, "%" PRIu64 " rays: bytes", c.rays);
    }
    static_assert(PIXEL_TABLE_HEAD_BYTES == QUAD_HEAD_WORDS * sizeof(unsigned) && PIXEL_TABLE_ENTRY_BYTES == sizeof(uint2), "the accounting is the table's layout (kernels.h QuadTable)");
    // the unit by sampling: 64 places are 4 entries of 16 samples, 16 quadrants, 64 one-sample entries
    CHECK(64 / pixel_samples(XRT_MS_FIXED16) == 4 && 64 / pixel_samples(XRT_MS_ADAPTIVE) == 16 && 64 / pixel_samples(XRT_MS_OFF) == 64, "units");
    // the masks
    int masks = 0;
    for (Kind kind : {ONE_BODY, TWO_LEVEL})
        for (int mode : modes)
            for (int env : {-1, 0, 1, 6, 7}) { check_masks(kind, mode, env); masks++; }
    // the interface
    static_assert(sizeof(xrt_render_opts) == 48 && offsetof(xrt_render_opts, list_order) == 40 && offsetof(xrt_render_opts, reserved) == 44, "xrt_render_opts keeps its size and offsets");
    static_assert(XRT_LIST_UNORDERED == 0 && XRT_LIST_COHERENT == 1 && XRT_VERSION == 203, "xrt.h");
    std::printf("plans %d masks %d\n", plans, masks);
    std::printf("scene masks %d\n", check_scene_masks());
    if (g_failures) { std::printf("host_coherent: %d FAILED\n", g_failures); return 1; }
    std::printf("host_coherent: ok\n");
    return 0;
}
