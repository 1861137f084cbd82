// scene_host.cpp — see scene_host.h.
#include "scene_host.h"
#include "pose.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace xrt {

size_t SceneArrays::bytes() const {
    return (blocks.size() + refN.size() + snodes.size() + shade.size() + leafNB.size() + leafTB.size() + scull.size() + runTB.size()) * sizeof(f4) + (refT.size() + pblocks.size() + lrec.size()) * sizeof(float) + refG.size() * sizeof(g3) +
           (childDfs.size() + srefs.size() + objMesh.size() + runBase.size()) * sizeof(int) + meshes.size() * sizeof(MeshRec) +
           objects.size() * sizeof(ObjRec) + materials.size() * sizeof(MaterialRec) + texels.size() * sizeof(uint32_t);
}

int HostScene::add_mesh(const float *v, const float *n, const float *uv, const float *sn, const float *color, int ntri,
                        const xrt_material *m, const float bbox[6], std::string &err) {
    if (!v || !sn || !m || !bbox || ntri < 0) { err = "xrt_scene_add_mesh: null argument"; return -1; }
    if (ntri >= (1 << 28)) { err = "xrt_scene_add_mesh: too many triangles"; return -1; }
    HostMesh hm;
    hm.ntri = ntri;
    hm.v.assign(v, v + (size_t)ntri * 9);
    if (n) hm.n.assign(n, n + (size_t)ntri * 9); else hm.n.assign((size_t)ntri * 9, 0.0f);
    if (uv) hm.uv.assign(uv, uv + (size_t)ntri * 6); else hm.uv.assign((size_t)ntri * 6, 0.0f);
    hm.sn.assign(sn, sn + (size_t)ntri * 3);
    if (color) hm.color.assign(color, color + (size_t)ntri * 4); else hm.color.assign((size_t)ntri * 4, 1.0f);
    std::memcpy(hm.bbox, bbox, sizeof(hm.bbox));
    hm.reflectiveness = m->reflectiveness;
    hm.refractionIndex = m->refraction_index;
    hm.transparent = m->transparent != 0;
    hm.interpolateNormals = m->interpolate_normals != 0;
    hm.useTexture = m->use_texture != 0;
    if (hm.useTexture) {
        if (!m->tex_argb || m->tex_width <= 0 || m->tex_height <= 0) { err = "xrt_scene_add_mesh: UseTexture without texels (Bitmap.FromFile would throw, MAT:63)"; return -1; }
        hm.texW = m->tex_width; hm.texH = m->tex_height;
        hm.texels.assign(m->tex_argb, m->tex_argb + (size_t)m->tex_width * m->tex_height);
        if (m->tex_pargb) hm.texelsP.assign(m->tex_pargb, m->tex_pargb + (size_t)m->tex_width * m->tex_height);
    }
    meshes.push_back(std::move(hm));
    built = false;
    return (int)meshes.size() - 1;
}

int HostScene::add_object(const int *meshIds, int n, const float *world, const float *invWorld, const float *bbox,
                          const float *worldBbox, std::string &err) {
    if (!meshIds || n < 0 || !world || !invWorld || !bbox || !worldBbox) { err = "xrt_scene_add_object: null argument"; return -1; }
    HostObject o;
    for (int i = 0; i < n; i++) {
        if (meshIds[i] < 0 || meshIds[i] >= (int)meshes.size()) { err = "xrt_scene_add_object: unknown mesh id"; return -1; }
        o.meshes.push_back(meshIds[i]);
    }
    std::memcpy(o.world, world, 64); std::memcpy(o.invWorld, invWorld, 64);
    std::memcpy(o.bbox, bbox, 24); std::memcpy(o.worldBbox, worldBbox, 24);
    objects.push_back(std::move(o));
    built = false;
    return (int)objects.size() - 1;
}

// The pre-cull record of every body (pose.h object_cull_box): the boxes of its meshes as added.
struct HostMeshBoxes {
    const HostObject &o;
    const std::vector<HostMesh> &meshes;
    void operator()(int k, float bb[6]) const { std::memcpy(bb, meshes[(size_t)o.meshes[(size_t)k]].bbox, 6 * sizeof(float)); }
};
static void object_cull_box(const HostObject &o, const std::vector<HostMesh> &meshes, ObjRec &r, double safety) {
    object_cull_box(o.invWorld, (int)o.meshes.size(), HostMeshBoxes{o, meshes}, r, safety);
}

// Tight-box record of the triangles t.leafRefs[b0 .. b1) of mesh m (xrt_core.h leaf_certainly_missed; DESIGN.md §3 "Tight leaf boxes"):
// [0] = (vertex box min, K = C u0 max_t |E1||E2|/|E1 x E2| * safety), [1] = (vertex box max, longest edge), [2] = (min of the unit geometric
// normals, ok), [3] = (their max, -), all rounded outwards.  The bound behind it holds for ANY set of triangles -- a leaf, or a run of
// consecutive references of a leaf.  rec stays zero (ok = 0: never skipped) when a triangle is outside the magnitudes the analysis assumes.
static void tight_box_record(const HostMesh &m, const std::vector<int> &leafRefs, int b0, int b1, double safety, f4 rec[4]) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, nlo[3] = {2, 2, 2}, nhi[3] = {-2, -2, -2};
    double aMax = 0, eMax = 0;
    bool ok = b1 > b0;
    for (int r = b0; r < b1 && ok; r++) {
        const float *p = &m.v[(size_t)leafRefs[r] * 9];
        const float e1f[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2f[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};   // RE:54-55, as stored in refG
        const double e1[3] = {e1f[0], e1f[1], e1f[2]}, e2[3] = {e2f[0], e2f[1], e2f[2]};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        const double ln = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        // magnitudes the error analysis assumes (no overflow, no subnormal products)
        if (!(l1 >= 1e-9 && l2 >= 1e-9 && l1 <= 1e12 && l2 <= 1e12 && ln > 0 && l1 * l2 / ln <= 1e6)) { ok = false; break; }
        aMax = std::fmax(aMax, l1 * l2 / ln);
        eMax = std::fmax(eMax, std::fmax(l1, l2));
        for (int k = 0; k < 3; k++) {
            const double v[3] = {(double)p[k], (double)p[k] + e1[k], (double)p[k] + e2[k]};
            for (double x : v) { if (!(std::fabs(x) <= 1e12)) ok = false; lo[k] = std::fmin(lo[k], x); hi[k] = std::fmax(hi[k], x); }
            nlo[k] = std::fmin(nlo[k], n[k] / ln); nhi[k] = std::fmax(nhi[k], n[k] / ln);
        }
    }
    if (ok && safety > 0.0) {
        auto down = [](double x) { return std::nextafterf((float)x, -INFINITY); };
        auto up = [](double x) { return std::nextafterf((float)x, INFINITY); };
        rec[0] = f4{down(lo[0]), down(lo[1]), down(lo[2]), up((double)LEAF_CULL_C * std::ldexp(1.0, -24) * aMax * safety)};
        rec[1] = f4{up(hi[0]), up(hi[1]), up(hi[2]), up(eMax)};
        rec[2] = f4{down(nlo[0] - 1e-6), down(nlo[1] - 1e-6), down(nlo[2] - 1e-6), 1.0f};
        rec[3] = f4{up(nhi[0] + 1e-6), up(nhi[1] + 1e-6), up(nhi[2] + 1e-6), 0.0f};
    }
}

// Storage order of a big leaf's references.  The walk tests a leaf of >= LEAF_RUN_MIN references run by run (LEAF_RUN consecutive references, each run with a tight box of
// its own), and a run of consecutive LIST entries is a strip -- the builder hands triangles down in index order (MO:225-233), a heightfield's leaf holds them row by row --
// that a ray crossing the leaf touches whatever its direction.  Here the references of such a leaf are stored in runs of NEIGHBOURS instead: the set is cut at the middle of
// its longest extent (centroids; the cut at a multiple of LEAF_RUN) until a part fits one run.  Order matters to the reference in one place only -- of two triangles of a leaf
// hit at exactly the same distance the EARLIER in the list wins (MO:293-294, strict '<') -- and the list of a leaf is ascending in the triangle index (checked here; a leaf
// that is not keeps its order), so the kernels settle such a tie by the smaller index (traverse.h leaf_candidate, packet.hip pk_candidate) and the answers do not depend on
// the storage order.  xrt_scene_get_tree still shows the reference's order.
// (a leaf keeps its list order where that already gives the smaller runs: the sum of the surface areas of the runs' vertex boxes decides -- the twelve triangles of a
// crate's face pairs lie better in the order they were modelled in)
static double run_boxes_area(const HostMesh &m, const std::vector<int> &lr, int b0, int b1) {
    double sum = 0;
    for (int ra = b0; ra < b1; ra += LEAF_RUN) {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int r = ra; r < ra + LEAF_RUN && r < b1; r++) {
            const float *p = &m.v[(size_t)lr[(size_t)r] * 9];
            for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { const double x = p[3 * j + k]; if (x == x) { lo[k] = std::fmin(lo[k], x); hi[k] = std::fmax(hi[k], x); } }
        }
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx >= 0 && dy >= 0 && dz >= 0) sum += dx * dy + dy * dz + dz * dx;
    }
    return sum;
}
static void spatial_runs_cut(const HostMesh &m, std::vector<int> &lr, int b0, int b1);
static void spatial_runs(const HostMesh &m, std::vector<int> &lr, int b0, int b1) {
    for (int r = b0 + 1; r < b1; r++) if (lr[(size_t)r] <= lr[(size_t)r - 1]) return;
    const std::vector<int> before(lr.begin() + b0, lr.begin() + b1);
    const double a0 = run_boxes_area(m, lr, b0, b1);
    spatial_runs_cut(m, lr, b0, b1);
    if (!(run_boxes_area(m, lr, b0, b1) < a0)) std::copy(before.begin(), before.end(), lr.begin() + b0);
}
static void spatial_runs_cut(const HostMesh &m, std::vector<int> &lr, int b0, int b1) {
    struct Part { int a, b; };
    std::vector<Part> todo{Part{b0, b1}};
    std::vector<std::pair<float, int>> key;
    while (!todo.empty()) {
        const Part q = todo.back();
        todo.pop_back();
        if (q.b - q.a <= LEAF_RUN) { std::sort(lr.begin() + q.a, lr.begin() + q.b); continue; }
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        auto centroid = [&](int tri, int k) { const float *p = &m.v[(size_t)tri * 9]; return (p[k] + p[3 + k]) + p[6 + k]; };
        for (int r = q.a; r < q.b; r++)
            for (int k = 0; k < 3; k++) { const float c = centroid(lr[(size_t)r], k); if (c == c) { lo[k] = std::fmin(lo[k], c); hi[k] = std::fmax(hi[k], c); } }
        int ax = 0;
        for (int k = 1; k < 3; k++) if (hi[k] - lo[k] > hi[ax] - lo[ax]) ax = k;
        key.clear();
        for (int r = q.a; r < q.b; r++) { const float c = centroid(lr[(size_t)r], ax); key.push_back({c == c ? c : FLT_MAX, lr[(size_t)r]}); }
        std::sort(key.begin(), key.end());   // (ties by triangle index: deterministic)
        for (int r = q.a; r < q.b; r++) lr[(size_t)r] = key[(size_t)(r - q.a)].second;
        const int n = q.b - q.a, runs = (n + LEAF_RUN - 1) / LEAF_RUN, left = (runs / 2) * LEAF_RUN;   // (runs >= 2 here)
        todo.push_back(Part{q.a, q.a + left});
        todo.push_back(Part{q.a + left, q.b});
    }
}

// The MaterialRec of mesh m when its texels (and behind them their premultiplied copy) start at word `off` of the arena; off moves past them.  The
// texels a mesh holds have their place whether or not UseTexture is set: the flag alone decides what the kernels read (xrt_scene_set_materials).
static MaterialRec material_record(const HostMesh &m, size_t &off) {
    MaterialRec mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.reflectiveness = m.reflectiveness;
    mat.refractionIndex = m.refractionIndex;
    mat.flags = (m.transparent ? MAT_TRANSPARENT : 0) | (m.interpolateNormals ? MAT_INTERP : 0) | (m.useTexture ? MAT_TEXTURE : 0);
    mat.texOffset = (int)off;
    mat.texWidth = m.texW; mat.texHeight = m.texH;
    off += m.texels.size();
    mat.texOffsetP = mat.texOffset;
    if (!m.texelsP.empty()) { mat.texOffsetP = (int)off; off += m.texelsP.size(); }
    return mat;
}
static void append_material(SceneArrays &A, const HostMesh &m) {
    size_t off = A.texels.size();
    A.materials.push_back(material_record(m, off));
    A.texels.insert(A.texels.end(), m.texels.begin(), m.texels.end());
    A.texels.insert(A.texels.end(), m.texelsP.begin(), m.texelsP.end());
    A.anyTransparent = A.anyTransparent || m.transparent;
    A.anyTexture = A.anyTexture || m.useTexture;
}

// The surface normals sn[3 * tris[i]] bounded in one DIAGONAL frame (traverse.h all_back_facing_diag): for each axis c, with a and b the axes that follow it
// cyclically, the intervals of fl(N_a + N_b) and fl(N_a - N_b), each end moved one float outwards (a sum of two floats is off by at most half an ulp, so
// the interval holds the real sums).  ONE axis is kept.  The rule: a fixed set of 256 directions spread evenly over the sphere is put to the exact bounds
// (in double, no margin); the axis whose diagonal box answers the most directions that the axis-aligned box [nlo, nhi] does NOT answer wins, ties go to the
// smaller (smax - smin) + (dmax - dmin), then to the lower axis.  Widths alone mislead: for a cone of normals about +y the frames about x and z have the
// narrower s and d intervals and answer nothing the axis-aligned box does not, the frame about y answers more than a quarter of what is left.
// Returns 1, 2, 3 = x, y, z and fills dg = (smin, smax, dmin, dmax), or 0: no frame can answer anything (or a normal is not finite).
static int diagonal_normal_box(const float *sn, const int *tris, size_t n, const f4 &nlo, const f4 &nhi, f4 &dg) {
    if (n == 0) return 0;
    const float lo3[3] = {nlo.x, nlo.y, nlo.z}, hi3[3] = {nhi.x, nhi.y, nhi.z};
    float box[3][4];
    bool usable[3];
    for (int c = 0; c < 3; c++) {
        const int a = (c + 1) % 3, b = (c + 2) % 3;
        float smin = FLT_MAX, smax = -FLT_MAX, dmin = FLT_MAX, dmax = -FLT_MAX;
        bool finite = true;
        for (size_t i = 0; i < n; i++) {
            const float *N = sn + 3 * (size_t)tris[i];
            const float s = N[a] + N[b], d = N[a] - N[b];
            if (!(std::fabs(s) <= FLT_MAX && std::fabs(d) <= FLT_MAX)) { finite = false; break; }
            smin = s < smin ? s : smin; smax = s > smax ? s : smax; dmin = d < dmin ? d : dmin; dmax = d > dmax ? d : dmax;
        }
        box[c][0] = std::nextafterf(smin, -INFINITY); box[c][1] = std::nextafterf(smax, INFINITY);
        box[c][2] = std::nextafterf(dmin, -INFINITY); box[c][3] = std::nextafterf(dmax, INFINITY);
        usable[c] = finite && std::fabs(box[c][0]) <= FLT_MAX && std::fabs(box[c][1]) <= FLT_MAX && std::fabs(box[c][2]) <= FLT_MAX && std::fabs(box[c][3]) <= FLT_MAX &&
                    std::fabs(lo3[c]) <= FLT_MAX && std::fabs(hi3[c]) <= FLT_MAX;
        // (a box whose three intervals all hold 0 answers nothing)
        usable[c] = usable[c] && (box[c][0] > 0.0f || box[c][1] < 0.0f || box[c][2] > 0.0f || box[c][3] < 0.0f || lo3[c] > 0.0f || hi3[c] < 0.0f);
    }
    int gained[3] = {0, 0, 0};
    const int K = 256;
    for (int k = 0; k < K; k++) {   // a Fibonacci lattice on the sphere
        const double y = 1.0 - (2.0 * k + 1.0) / K, r = std::sqrt(1.0 - y * y), phi = 2.399963229728653 * k;
        const double D[3] = {r * std::cos(phi), y, r * std::sin(phi)};
        double axisBound = 0.0;
        for (int j = 0; j < 3; j++) axisBound += std::fmin((double)lo3[j] * D[j], (double)hi3[j] * D[j]);
        if (axisBound > 0.0) continue;
        for (int c = 0; c < 3; c++) {
            if (!usable[c]) continue;
            const int a = (c + 1) % 3, b = (c + 2) % 3;
            const double p = D[a] + D[b], q = D[a] - D[b];
            const double bound = std::fmin((double)lo3[c] * D[c], (double)hi3[c] * D[c]) + 0.5 * (std::fmin(box[c][0] * p, box[c][1] * p) + std::fmin(box[c][2] * q, box[c][3] * q));
            if (bound > 0.0) gained[c]++;
        }
    }
    int best = -1;
    double bestWidth = 0.0;
    for (int c = 0; c < 3; c++) {
        if (!usable[c]) continue;
        const double width = ((double)box[c][1] - box[c][0]) + ((double)box[c][3] - box[c][2]);
        if (best < 0 || gained[c] > gained[best] || (gained[c] == gained[best] && width < bestWidth)) { best = c; bestWidth = width; }
    }
    if (best < 0) return 0;
    dg = f4{box[best][0], box[best][1], box[best][2], box[best][3]};
    return best + 1;
}

bool HostScene::build(int meshThreshold, int sceneThreshold, std::string &err) {
    if (meshThreshold <= 0) meshThreshold = 50;    // MO:42
    if (sceneThreshold <= 0) sceneThreshold = 20;  // OSM:50
    built = false;
    builtMeshes = -1;
    arrays = SceneArrays();
    meshTrees.clear();
    raw = RawSizes();
    this->meshThreshold = meshThreshold;
    if (!mesh_part(err)) return false;
    if (!body_part(sceneThreshold, err)) { builtMeshes = -1; return false; }   // (the arrays stay without their padding: nothing may append to them)
    material_part();
    assemble();
    built = true;
    return true;
}

// Meshes [raw.meshes, meshes.size()): Mesh.Init and their part of every per-mesh array, appended.  On failure `arrays` is of no use (builtMeshes -1).
bool HostScene::mesh_part(std::string &err) {
    SceneArrays &A = arrays;
    strip_padding();
    builtMeshes = -1;
    meshTrees.resize(meshes.size());
    const size_t first = raw.meshes;
    for (size_t mi = first; mi < meshes.size(); mi++) {
        meshTreesBuilt++;
        if (!build_mesh_tree(meshes[mi], meshThreshold, meshTrees[mi], err)) return false;   // Mesh.Init (MESH:27-32)
    }
    if (!append_parts(first, meshes.size(), first ? A.totalTris : 0, err)) return false;
    builtMeshes = (int)meshes.size();
    return true;
}

// What assemble() put behind the last mesh's part (padding, the dummies of empty arrays) comes off.
void HostScene::strip_padding() {
    SceneArrays &A = arrays;
    A.blocks.resize(raw.blocks); A.refN.resize(raw.refN); A.refG.resize(3 * raw.refN); A.shade.resize(raw.shade); A.leafNB.resize(raw.leafNB); A.leafTB.resize(raw.leafTB);
    A.runBase.resize(raw.runBase); A.runTB.resize(raw.runTB); A.childDfs.resize(raw.childDfs); A.pblocks.resize(raw.pblocks); A.meshes.resize(raw.meshes);
}

HostScene::RawSizes HostScene::sizes_now() const {
    const SceneArrays &A = arrays;
    RawSizes z;
    z.blocks = A.blocks.size(); z.refN = A.refN.size(); z.shade = A.shade.size(); z.leafNB = A.leafNB.size(); z.leafTB = A.leafTB.size();
    z.runBase = A.runBase.size(); z.runTB = A.runTB.size(); z.childDfs = A.childDfs.size(); z.pblocks = A.pblocks.size(); z.meshes = A.meshes.size();
    return z;
}

// What the kernels' tie rule relies on: every leaf's list is ascending in the triangle index (MO:225-233 hands lists down in order).
static bool leaf_lists_ascending(const FlatTree &t) {
    const std::vector<int> &lr = t.leafRefs;
    for (size_t bi = 0; bi < t.blocks.size() / 2; bi++) {
        const f4 lo = t.blocks[2 * bi], hi = t.blocks[2 * bi + 1];
        const int lref = f2i(lo.y), masks = f2i(lo.z), total = f2i(lo.w);
        const int offw[4] = {f2i(hi.x), f2i(hi.y), f2i(hi.z), f2i(hi.w)};
        auto off = [&](int q) { int w = offw[q >> 1]; return (q & 1) ? (int)((unsigned)w >> 16) : (w & 0xffff); };
        for (int c = 0; c < 8; c++) {
            if ((masks >> c) & 1) continue;
            const int b0 = lref + off(c), b1 = lref + (c == 7 ? total : off(c + 1));
            for (int r = b0 + 1; r < b1; r++) if (lr[(size_t)r] <= lr[(size_t)r - 1]) return false;
        }
    }
    if (t.rootIsLeaf) for (int r = 1; r < t.rootCount; r++) if (lr[(size_t)r] <= lr[(size_t)r - 1]) return false;
    return true;
}

// The parts of meshes [first, last), whose trees are in meshTrees, appended to the per-mesh arrays (which end without padding); the first of them
// numbers its triangles from triBase.  partStart[mi] keeps where mesh mi's part begins, `raw` where the last one ends.
bool HostScene::append_parts(size_t first, size_t last, int triBase, std::string &err) {
    SceneArrays &A = arrays;
    partStart.resize(meshes.size());
    for (size_t mi = first; mi < last; mi++) {
        const HostMesh &m = meshes[mi];
        const FlatTree &t = meshTrees[mi];
        if (!leaf_lists_ascending(t)) { err = "internal: a leaf's triangle list is not ascending"; return false; }
        partStart[mi] = sizes_now();
        std::vector<int> lr = t.leafRefs;   // the references in STORAGE order (spatial_runs)
        if (spatialRuns)
            for (size_t bi = 0; bi < t.blocks.size() / 2; bi++) {
                const f4 lo = t.blocks[2 * bi], hi = t.blocks[2 * bi + 1];
                const int lref = f2i(lo.y), masks = f2i(lo.z), total = f2i(lo.w);
                const int offw[4] = {f2i(hi.x), f2i(hi.y), f2i(hi.z), f2i(hi.w)};
                auto off = [&](int q) { int w = offw[q >> 1]; return (q & 1) ? (int)((unsigned)w >> 16) : (w & 0xffff); };
                for (int c = 0; c < 8; c++) {
                    if ((masks >> c) & 1) continue;
                    const int b0 = lref + off(c), b1 = lref + (c == 7 ? total : off(c + 1));
                    if (b1 - b0 >= LEAF_RUN_MIN) spatial_runs(m, lr, b0, b1);
                }
            }
        const int blockBase = (int)(A.blocks.size() / 2);
        const int refBase = (int)A.refN.size();
        for (size_t bi = 0; bi < t.blocks.size() / 2; bi++) {   // local -> global indices
            f4 lo = t.blocks[2 * bi], hi = t.blocks[2 * bi + 1];
            lo.x = i2f(f2i(lo.x) + blockBase);
            lo.y = i2f(f2i(lo.y) + refBase);
            A.blocks.push_back(lo); A.blocks.push_back(hi);
        }
        A.childDfs.insert(A.childDfs.end(), t.childDfs.begin(), t.childDfs.end());
        // the packet kernel's block records: descriptor + child planes (traverse.h PBLOCK_*), boxes derived from the root box exactly as the
        // builder and the per-lane kernel derive them (child_box / half_of: the same inline functions, compiled without contraction)
        A.pblocks.resize((size_t)(blockBase + t.blocks.size() / 2) * PBLOCK_WORDS, 0.0f);
        if (!t.blocks.empty()) {
            struct Todo { int lb; v3 bmin, half; };
            std::vector<Todo> todo;
            const v3 rmn = mk(t.rootBox[0], t.rootBox[1], t.rootBox[2]);
            todo.push_back(Todo{0, rmn, half_of(rmn, mk(t.rootBox[3], t.rootBox[4], t.rootBox[5]))});   // (local block 0 = the root's children)
            while (!todo.empty()) {
                const Todo w = todo.back();
                todo.pop_back();
                const f4 lo = A.blocks[2 * (size_t)(blockBase + w.lb)], hi = A.blocks[2 * (size_t)(blockBase + w.lb) + 1];
                float *q = &A.pblocks[(size_t)(blockBase + w.lb) * PBLOCK_WORDS];
                q[0] = lo.x; q[1] = lo.y; q[2] = lo.z; q[3] = lo.w; q[4] = hi.x; q[5] = hi.y; q[6] = hi.z; q[7] = hi.w;
                const float bm[3] = {w.bmin.x, w.bmin.y, w.bmin.z}, hf[3] = {w.half.x, w.half.y, w.half.z};
                for (int ax = 0; ax < 3; ax++) {
                    const float p0 = bm[ax] + hf[ax] * 0.0f, p1 = bm[ax] + hf[ax] * 1.0f, p2 = p1 + hf[ax], hp0 = p0 + hf[ax];
                    q[8 + 4 * ax] = p0; q[9 + 4 * ax] = p1; q[10 + 4 * ax] = p2; q[11 + 4 * ax] = hp0;
                }
                const int childBase = f2i(t.blocks[2 * (size_t)w.lb].x), interior = f2i(lo.z) & 0xff;
                for (int c = 0; c < 8; c++)
                    if ((interior >> c) & 1) {
                        v3 cmin, cmax;
                        child_box(w.bmin, w.half, c, cmin, cmax);
                        todo.push_back(Todo{childBase + __builtin_popcount((unsigned)interior & ((1u << c) - 1u)), cmin, half_of(cmin, cmax)});
                    }
            }
        }
        // per leaf: bounds of its triangles' surface normals, so a leaf whose triangles all face away from a ray
        // (RE:48-51 would reject every one of them) can be skipped without reading its references
        for (size_t bi = 0; bi < t.blocks.size() / 2; bi++) {
            const f4 lo = t.blocks[2 * bi], hi = t.blocks[2 * bi + 1];
            const int lref = f2i(lo.y), masks = f2i(lo.z), total = f2i(lo.w);
            const int offw[4] = {f2i(hi.x), f2i(hi.y), f2i(hi.z), f2i(hi.w)};
            auto off = [&](int q) { int w = offw[q >> 1]; return (q & 1) ? (int)((unsigned)w >> 16) : (w & 0xffff); };
            for (int c = 0; c < 8; c++) {
                f4 mn{0, 0, 0, 0}, mx{0, 0, 0, 0};
                if (!((masks >> c) & 1)) {
                    const int b0 = lref + off(c), b1 = lref + (c == 7 ? total : off(c + 1));
                    for (int r = b0; r < b1; r++) {
                        const float *sn = &m.sn[(size_t)lr[(size_t)r] * 3];
                        if (r == b0) { mn = f4{sn[0], sn[1], sn[2], 0}; mx = mn; }
                        else {
                            mn.x = sn[0] < mn.x ? sn[0] : mn.x; mn.y = sn[1] < mn.y ? sn[1] : mn.y; mn.z = sn[2] < mn.z ? sn[2] : mn.z;
                            mx.x = sn[0] > mx.x ? sn[0] : mx.x; mx.y = sn[1] > mx.y ? sn[1] : mx.y; mx.z = sn[2] > mx.z ? sn[2] : mx.z;
                        }
                        if (!(sn[0] == sn[0] && sn[1] == sn[1] && sn[2] == sn[2])) { mn.w = 1.0f; }   // a NaN normal: never skip this leaf
                    }
                }
                A.leafNB.push_back(mn); A.leafNB.push_back(mx);
                // ... and the tight box of the leaf (xrt_core.h leaf_certainly_missed): vertex box, box of the unit geometric normals,
                // K = C u0 max |E1||E2|/|E1 x E2| and the longest edge, all rounded outwards
                f4 rec[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
                int runFirst = -1;
                if (!((masks >> c) & 1)) {
                    const int b0 = lref + off(c), b1 = lref + (c == 7 ? total : off(c + 1));
                    tight_box_record(m, lr, b0, b1, leafCullSafety, rec);
                    // ... and the same record for every run of LEAF_RUN consecutive references of a leaf of at least LEAF_RUN_MIN (the
                    // bound holds for any set of triangles): a ray that reaches the leaf's box still tests only the runs it can reach
                    if (b1 - b0 >= LEAF_RUN_MIN) {
                        runFirst = (int)(A.runTB.size() / 4);
                        for (int ra = b0; ra < b1; ra += LEAF_RUN) {
                            f4 rr[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
                            tight_box_record(m, lr, ra, ra + LEAF_RUN < b1 ? ra + LEAF_RUN : b1, leafCullSafety, rr);
                            for (const f4 &q : rr) A.runTB.push_back(q);
                        }
                    }
                }
                for (const f4 &q : rec) A.leafTB.push_back(q);
                A.runBase.push_back(runFirst);
            }
        }
        // ... and for every INTERIOR node the box of all the surface normals below it (the union of its children's boxes, bottom-up: a child
        // block has a higher index than its parent's), so that a whole subtree RE:48-51 would reject triangle by triangle -- the terrain
        // under a ray that leaves it, the far side of a crate -- is never entered (traverse.h all_back_facing: the same test, the same margin).
        f4 meshNBlo{0, 0, 0, 0}, meshNBhi{0, 0, 0, 0};
        {
            bool meshAny = false;
            const size_t nb = t.blocks.size() / 2;
            for (size_t bi = nb; bi-- > 0;) {
                const int masks = f2i(t.blocks[2 * bi].z), childBase = f2i(t.blocks[2 * bi].x);
                for (int c = 0; c < 8; c++) {
                    if (!((masks >> c) & 1)) continue;   // (a leaf: done above)
                    const size_t cb = (size_t)childBase + (size_t)__builtin_popcount((unsigned)(masks & 0xff) & ((1u << c) - 1u));
                    const int cmasks = f2i(t.blocks[2 * cb].z);
                    f4 mn{0, 0, 0, 0}, mx{0, 0, 0, 0};
                    bool any = false;
                    for (int k = 0; k < 8; k++) {
                        if ((cmasks >> (8 + k)) & 1) continue;   // empty leaf
                        const f4 a = A.leafNB[2 * ((size_t)(blockBase + cb) * 8 + k)], b2 = A.leafNB[2 * ((size_t)(blockBase + cb) * 8 + k) + 1];
                        if (!any) { mn = a; mx = b2; any = true; }
                        else {
                            mn.x = a.x < mn.x ? a.x : mn.x; mn.y = a.y < mn.y ? a.y : mn.y; mn.z = a.z < mn.z ? a.z : mn.z;
                            mx.x = b2.x > mx.x ? b2.x : mx.x; mx.y = b2.y > mx.y ? b2.y : mx.y; mx.z = b2.z > mx.z ? b2.z : mx.z;
                            if (a.w != 0.0f) mn.w = 1.0f;
                        }
                    }
                    if (!any) mn.w = 1.0f;   // (cannot happen: an interior node holds triangles)
                    A.leafNB[2 * ((size_t)(blockBase + bi) * 8 + c)] = mn; A.leafNB[2 * ((size_t)(blockBase + bi) * 8 + c) + 1] = mx;
                    // all_back_facing needs sum_k min(nmin_k d_k, nmax_k d_k) > 0; an axis whose interval holds 0 contributes <= 0 for every d_k, so a box
                    // that holds the origin can never pass: only the other interior children are worth the test (descriptor bits 24..31)
                    const bool canPass = mn.w == 0.0f && (mn.x > 0.0f || mx.x < 0.0f || mn.y > 0.0f || mx.y < 0.0f || mn.z > 0.0f || mx.z < 0.0f);
                    if (canPass) {
                        f4 &lo = A.blocks[2 * (size_t)(blockBase + bi)];
                        lo.z = i2f(f2i(lo.z) | (1 << (24 + c)));
                        A.pblocks[(size_t)(blockBase + bi) * PBLOCK_WORDS + 2] = lo.z;
                    }
                }
            }
            if (nb) {
                const int masks = f2i(t.blocks[0].z);
                for (int k = 0; k < 8; k++) {
                    if ((masks >> (8 + k)) & 1) continue;
                    const f4 a = A.leafNB[2 * ((size_t)blockBase * 8 + k)], b2 = A.leafNB[2 * ((size_t)blockBase * 8 + k) + 1];
                    if (!meshAny) { meshNBlo = a; meshNBhi = b2; meshAny = true; }
                    else {
                        meshNBlo.x = a.x < meshNBlo.x ? a.x : meshNBlo.x; meshNBlo.y = a.y < meshNBlo.y ? a.y : meshNBlo.y; meshNBlo.z = a.z < meshNBlo.z ? a.z : meshNBlo.z;
                        meshNBhi.x = b2.x > meshNBhi.x ? b2.x : meshNBhi.x; meshNBhi.y = b2.y > meshNBhi.y ? b2.y : meshNBhi.y; meshNBhi.z = b2.z > meshNBhi.z ? b2.z : meshNBhi.z;
                        if (a.w != 0.0f) meshNBlo.w = 1.0f;
                    }
                }
            }
            if (!meshAny) meshNBlo.w = 1.0f;   // (a mesh whose root is a leaf, or without triangles: no record, never culled)
        }
        for (int tri : lr) {   // leaf references in storage order: normal stream + geometry stream
            const float *p = &m.v[(size_t)tri * 9];
            const float *sn = &m.sn[(size_t)tri * 3];
            A.refN.push_back(f4{sn[0], sn[1], sn[2], i2f(triBase + tri)});
            A.refG.push_back(g3{p[0], p[1], p[2]});
            A.refG.push_back(g3{p[3] - p[0], p[4] - p[1], p[5] - p[2]});   // Edge1 = v2 - v1 (RE:54)
            A.refG.push_back(g3{p[6] - p[0], p[7] - p[1], p[8] - p[2]});   // Edge2 = v3 - v1 (RE:55)
        }
        for (int i = 0; i < m.ntri; i++) {
            const float *n = &m.n[(size_t)i * 9], *uv = &m.uv[(size_t)i * 6], *c = &m.color[(size_t)i * 4], *sn = &m.sn[(size_t)i * 3];
            A.shade.push_back(f4{n[0], n[1], n[2], uv[0]});
            A.shade.push_back(f4{n[3], n[4], n[5], uv[1]});
            A.shade.push_back(f4{n[6], n[7], n[8], uv[2]});
            A.shade.push_back(f4{c[0], c[1], c[2], c[3]});
            A.shade.push_back(f4{uv[3], uv[4], uv[5], i2f((int)mi)});
            A.shade.push_back(f4{sn[0], sn[1], sn[2], i2f((int)mi)});
        }
        MeshRec mr;
        std::memset(&mr, 0, sizeof(mr));
        for (int a = 0; a < 3; a++) { mr.bmin[a] = m.bbox[a]; mr.bmax[a] = m.bbox[3 + a]; }
        for (int a = 0; a < 3; a++) { mr.rmin[a] = t.rootBox[a]; mr.rmax[a] = t.rootBox[3 + a]; }
        mr.rootBlock = t.rootIsLeaf ? -1 : blockBase;
        mr.rootRef = refBase; mr.rootCount = t.rootIsLeaf ? t.rootCount : 0;
        mr.nbMin[0] = meshNBlo.x; mr.nbMin[1] = meshNBlo.y; mr.nbMin[2] = meshNBlo.z; mr.nbMin[3] = meshNBlo.w;
        mr.nbMax[0] = meshNBhi.x; mr.nbMax[1] = meshNBhi.y; mr.nbMax[2] = meshNBhi.z; mr.nbMax[3] = 0.0f;
        if (meshNBlo.w == 0.0f) {   // ... and the same normals -- those of the leaf references, lr -- bounded in one diagonal frame
            f4 dg;
            const int axis = diagonal_normal_box(m.sn.data(), lr.data(), lr.size(), meshNBlo, meshNBhi, dg);
            if (axis) { mr.nbMax[3] = (float)axis; mr.nbDiag[0] = dg.x; mr.nbDiag[1] = dg.y; mr.nbDiag[2] = dg.z; mr.nbDiag[3] = dg.w; }
        }
        mr.triBase = triBase; mr.ntri = m.ntri; mr.material = (int)mi; mr.maxDepth = t.maxDepth; mr.dfsBase = blockBase * 8;
        A.meshes.push_back(mr);
        if (t.maxDepth > A.meshDepth) A.meshDepth = t.maxDepth;
        triBase += m.ntri;
    }
    A.totalTris = triBase;
    raw = sizes_now();
    return true;
}

// The bodies' records (one ObjRec per body, its mesh ids in objMesh) and OctreeSpatialManager.Build over them.
bool HostScene::body_part(int sceneThreshold, std::string &err) {
    SceneArrays &A = arrays;
    A.objects.clear();
    A.objMesh.clear();
    for (const HostObject &o : objects) {
        ObjRec r;
        std::memset(&r, 0, sizeof(r));
        std::memcpy(r.invWorld, o.invWorld, 64); std::memcpy(r.world, o.world, 64);
        r.meshStart = (int)A.objMesh.size(); r.meshCount = (int)o.meshes.size();
        object_cull_box(o, meshes, r, cullSafety);
        A.objMesh.insert(A.objMesh.end(), o.meshes.begin(), o.meshes.end());
        A.objects.push_back(r);
    }
    if (!scene_part(sceneThreshold, err)) return false;
    if (A.objMesh.empty()) A.objMesh.assign(1, -1);
    if (A.objects.empty()) { ObjRec z; std::memset(&z, 0, sizeof(z)); A.objects.push_back(z); }
    return true;
}

// The material table and the texel arena of ALL meshes as they are now (xrt_scene_set_materials may have changed them since they were added).
void HostScene::material_part() {
    SceneArrays &A = arrays;
    A.materials.clear();
    A.texels.clear();
    A.anyTransparent = A.anyTexture = false;
    for (const HostMesh &m : meshes) append_material(A, m);
    if (A.texels.empty()) A.texels.assign(1, 0u);
    if (A.materials.empty()) { MaterialRec z; std::memset(&z, 0, sizeof(z)); A.materials.push_back(z); }
}

// Behind mesh_part (all meshes built): the padding the kernels rely on, refT and lrec.
void HostScene::assemble() {
    SceneArrays &A = arrays;
    // never hand out empty arrays (a zero-size allocation has no address)
    // two dummy references at the end: the wave-packet kernel requests the next triangle's record before it knows the leaf has ended
    for (int k = 0; k < 2; k++) { A.refN.push_back(f4{0, 0, 0, i2f(-1)}); for (int j = 0; j < 3; j++) A.refG.push_back(g3{0, 0, 0}); }
    A.refT.assign(A.refN.size() * TRI_REC_WORDS + 16, 0.0f);
    for (size_t r = 0; r < A.refN.size(); r++) {
        float *q = &A.refT[r * TRI_REC_WORDS];
        q[0] = A.refN[r].x; q[1] = A.refN[r].y; q[2] = A.refN[r].z; q[3] = A.refN[r].w;
        for (int j = 0; j < 3; j++) { q[4 + 3 * j] = A.refG[3 * r + j].x; q[5 + 3 * j] = A.refG[3 * r + j].y; q[6 + 3 * j] = A.refG[3 * r + j].z; }
    }
    if (A.shade.empty()) A.shade.assign(SHADE_F4, f4{0, 0, 0, 0});
    if (A.meshes.empty()) { MeshRec z; std::memset(&z, 0, sizeof(z)); A.meshes.push_back(z); }
    if (A.blocks.empty()) A.blocks.assign(2, f4{0, 0, 0, 0});
    if (A.leafNB.empty()) A.leafNB.assign(16, f4{0, 0, 0, 0});
    if (A.leafTB.empty()) A.leafTB.assign(32, f4{0, 0, 0, 0});
    if (A.runBase.empty()) A.runBase.assign(8, -1);
    for (int k = 0; k < 8; k++) A.runTB.push_back(f4{0, 0, 0, 0});   // (padding: the packet kernel may request the record after a leaf's last run)
    if (A.childDfs.empty()) A.childDfs.assign(8, -1);
    if (A.pblocks.empty()) A.pblocks.assign(PBLOCK_WORDS, 0.0f);
    {   // the packet kernel's node records (traverse.h LREC_*): leafNB | leafTB | first run, the run records behind them
        const size_t nNodes = A.runBase.size(), nRuns = A.runTB.size() / 4;   // (runTB ends in two records of padding)
        A.lrec.assign(nNodes * LREC_WORDS + nRuns * RUN_WORDS, 0.0f);
        for (size_t nd = 0; nd < nNodes; nd++) {
            float *q = &A.lrec[nd * LREC_WORDS];
            std::memcpy(q, &A.leafNB[2 * nd], 8 * sizeof(float));
            std::memcpy(q + 8, &A.leafTB[4 * nd], 16 * sizeof(float));
            q[24] = i2f(A.runBase[nd] < 0 ? -1 : (int)(nNodes * LREC_WORDS + (size_t)A.runBase[nd] * RUN_WORDS));
        }
        if (nRuns) std::memcpy(&A.lrec[nNodes * LREC_WORDS], A.runTB.data(), nRuns * RUN_WORDS * sizeof(float));
    }
}

int HostScene::set_bodies(int n, const int *meshStart, const int *meshIds, const float *world, const float *invWorld, const float *bbox,
                          const float *worldBbox, int sceneThreshold, int &meshesBuilt, std::string &err) {
    meshesBuilt = 0;
    if (builtMeshes < 0) { err = "xrt_scene_set_bodies: call xrt_scene_build first"; return XRT_E_NOT_BUILT; }
    if (n < 0 || !meshStart || (n > 0 && (!world || !invWorld || !bbox || !worldBbox))) { err = "xrt_scene_set_bodies: null argument"; return XRT_E_INVALID_ARG; }
    if (meshStart[0] != 0) { err = "xrt_scene_set_bodies: mesh_start[0] is not 0"; return XRT_E_INVALID_ARG; }
    for (int i = 0; i < n; i++)
        if (meshStart[i + 1] < meshStart[i]) { err = "xrt_scene_set_bodies: mesh_start decreases at body " + std::to_string(i); return XRT_E_INVALID_ARG; }
    if (meshStart[n] > 0 && !meshIds) { err = "xrt_scene_set_bodies: null argument"; return XRT_E_INVALID_ARG; }
    for (int k = 0; k < meshStart[n]; k++)
        if (meshIds[k] < 0 || meshIds[k] >= (int)meshes.size()) { err = "xrt_scene_set_bodies: unknown mesh id " + std::to_string(meshIds[k]); return XRT_E_INVALID_ARG; }
    if (sceneThreshold <= 0) sceneThreshold = 20;  // OSM:50
    std::vector<HostObject> list((size_t)n);
    for (int i = 0; i < n; i++) {
        HostObject &o = list[(size_t)i];
        o.meshes.assign(meshIds + meshStart[i], meshIds + meshStart[i + 1]);
        std::memcpy(o.world, world + 16 * (size_t)i, 64); std::memcpy(o.invWorld, invWorld + 16 * (size_t)i, 64);
        std::memcpy(o.bbox, bbox + 6 * (size_t)i, 24); std::memcpy(o.worldBbox, worldBbox + 6 * (size_t)i, 24);
    }
    objects = std::move(list);
    built = false;
    const int firstNew = builtMeshes;
    if ((int)meshes.size() > firstNew) {
        if (!mesh_part(err)) return XRT_E_UNSUPPORTED;
        meshesBuilt = (int)meshes.size() - firstNew;
        assemble();
    }
    material_part();   // (also where no mesh is new: materials set while the scene waited for a build are in the meshes alone)
    if (!body_part(sceneThreshold, err)) return XRT_E_UNSUPPORTED;
    built = true;
    return XRT_OK;
}

// OctreeSpatialManager.Build (OSM:64-99) over the current poses and what is made from the scene octree: snodes, srefs, the pre-cull records
// in scene-leaf order (scull) and, per body, the positions of its records there (scullPosStart / scullPos: xrt_scene_set_poses rewrites
// them).  A.objects must hold one record per body.
bool HostScene::scene_part(int sceneThreshold, std::string &err) {
    SceneArrays &A = arrays;
    if (!build_scene_tree(objects, sceneThreshold, sceneTree, err)) return false;   // OSM:64-99
    A.snodes = sceneTree.nodes;
    A.srefs = sceneTree.leafRefs;
    A.sceneDepth = sceneTree.maxDepth;
    A.scull.clear();
    A.scullPosStart.assign(objects.size() + 1, 0);
    for (int o : A.srefs) A.scullPosStart[(size_t)o + 1]++;
    for (size_t o = 0; o < objects.size(); o++) A.scullPosStart[o + 1] += A.scullPosStart[o];
    A.scullPos.assign((size_t)A.scullPosStart.back(), 0);
    std::vector<int> fill(A.scullPosStart.begin(), A.scullPosStart.end() - 1);
    for (size_t i = 0; i < A.srefs.size(); i++) {   // the pre-cull records in scene-leaf order (one 64-byte scalar load per body for the packet kernel)
        const int o = A.srefs[i];
        A.scullPos[(size_t)fill[(size_t)o]++] = (int)i;
        f4 rec[4];
        scull_record(A.objects[(size_t)o], o, rec);
        for (const f4 &q : rec) A.scull.push_back(q);
    }
    for (int k = 0; k < 4; k++) A.scull.push_back(f4{0, 0, 0, 0});   // one record of padding: the packet kernel requests the next record a body ahead
    if (A.srefs.empty()) A.srefs.assign(1, -1);
    if (A.scullPos.empty()) A.scullPos.assign(1, -1);
    return true;
}

bool HostScene::set_pose(int id, const float *world, const float *invWorld, const float *worldBbox, std::string &err) {
    if (id < 0 || id >= (int)objects.size()) { err = "xrt_scene_set_poses: unknown object id"; return false; }
    HostObject &o = objects[(size_t)id];
    std::memcpy(o.world, world, 64); std::memcpy(o.invWorld, invWorld, 64); std::memcpy(o.worldBbox, worldBbox, 24);
    if (!built) return true;   // (the next build reads the pose)
    ObjRec &r = arrays.objects[(size_t)id];
    std::memcpy(r.invWorld, o.invWorld, 64); std::memcpy(r.world, o.world, 64);
    refresh_cull(id);
    return true;
}

// The pre-cull records of body id (its ObjRec's cull box, its records in scull) from its pose and the boxes of its meshes as they are now.
void HostScene::refresh_cull(int id) {
    SceneArrays &A = arrays;
    ObjRec &r = A.objects[(size_t)id];
    object_cull_box(objects[(size_t)id], meshes, r, cullSafety);
    f4 rec[4];
    scull_record(r, id, rec);
    for (int k = A.scullPosStart[(size_t)id]; k < A.scullPosStart[(size_t)id + 1]; k++)
        for (int j = 0; j < 4; j++) A.scull[4 * (size_t)A.scullPos[(size_t)k] + j] = rec[j];
}

int HostScene::set_mesh_triangles(int mesh, const float *v, const float *n, const float *uv, const float *sn, const float *color, int ntri,
                                  const float bbox[6], std::string &err) {
    const std::string fn = "xrt_scene_set_mesh_triangles: ";
    if (!v || !sn || !bbox || ntri < 0) { err = fn + "null argument"; return XRT_E_INVALID_ARG; }   // (the checks of add_mesh)
    if (ntri >= (1 << 28)) { err = fn + "too many triangles"; return XRT_E_INVALID_ARG; }
    if (mesh < 0 || mesh >= (int)meshes.size()) { err = fn + "mesh id " + std::to_string(mesh) + " out of range (" + std::to_string(meshes.size()) + " meshes)"; return XRT_E_INVALID_ARG; }
    const size_t k = (size_t)mesh;
    HostMesh nm;   // the new triangles under the mesh's material and texels (Mesh.MeshMaterial is another property)
    nm.ntri = ntri;
    nm.v.assign(v, v + (size_t)ntri * 9);
    if (n) nm.n.assign(n, n + (size_t)ntri * 9); else nm.n.assign((size_t)ntri * 9, 0.0f);
    if (uv) nm.uv.assign(uv, uv + (size_t)ntri * 6); else nm.uv.assign((size_t)ntri * 6, 0.0f);
    nm.sn.assign(sn, sn + (size_t)ntri * 3);
    if (color) nm.color.assign(color, color + (size_t)ntri * 4); else nm.color.assign((size_t)ntri * 4, 1.0f);
    std::memcpy(nm.bbox, bbox, sizeof(nm.bbox));
    auto take_material = [&]() {
        HostMesh &om = meshes[k];
        nm.reflectiveness = om.reflectiveness; nm.refractionIndex = om.refractionIndex;
        nm.transparent = om.transparent; nm.interpolateNormals = om.interpolateNormals; nm.useTexture = om.useTexture;
        nm.texW = om.texW; nm.texH = om.texH;
        nm.texels.swap(om.texels); nm.texelsP.swap(om.texelsP);
    };
    if (mesh >= builtMeshes) {   // (no build yet, or the mesh waits for its build: the build reads the new triangles)
        take_material();
        meshes[k] = std::move(nm);
        return XRT_OK;
    }
    // Mesh.Init (MESH:27-32) into a temporary; nothing of the scene is touched before every check has passed
    FlatTree nt;
    meshTreesBuilt++;
    if (!build_mesh_tree(nm, meshThreshold, nt, err)) return XRT_E_UNSUPPORTED;
    if (!leaf_lists_ascending(nt)) { err = "internal: a leaf's triangle list is not ascending"; return XRT_E_UNSUPPORTED; }
    int depth = nt.maxDepth;   // the deepest mesh octree afterwards: the replaced one may have been it
    for (size_t mi = 0; mi < (size_t)builtMeshes; mi++) if (mi != k && meshTrees[mi].maxDepth > depth) depth = meshTrees[mi].maxDepth;
    if (built && intersect_stack_capacity((arrays.sceneDepth + 1) + (depth + 1)) < 0) {
        err = fn + "octree too deep for the LDS stack (" + std::to_string((arrays.sceneDepth + 1) + (depth + 1)) + " levels)";
        return XRT_E_UNSUPPORTED;
    }
    SceneArrays &A = arrays;
    // the padding of assemble() comes off, then the parts of the meshes behind k, kept aside
    strip_padding();
    const RawSizes b = partStart[k], e = k + 1 < (size_t)builtMeshes ? partStart[k + 1] : raw;   // mesh k's old part
    SceneArrays T;
    auto cut = [](auto &from, auto &to, size_t at, size_t keep) { to.assign(from.begin() + (std::ptrdiff_t)at, from.end()); from.resize(keep); };
    cut(A.blocks, T.blocks, e.blocks, b.blocks); cut(A.refN, T.refN, e.refN, b.refN); cut(A.refG, T.refG, 3 * e.refN, 3 * b.refN); cut(A.shade, T.shade, e.shade, b.shade);
    cut(A.leafNB, T.leafNB, e.leafNB, b.leafNB); cut(A.leafTB, T.leafTB, e.leafTB, b.leafTB); cut(A.runBase, T.runBase, e.runBase, b.runBase);
    cut(A.runTB, T.runTB, e.runTB, b.runTB); cut(A.childDfs, T.childDfs, e.childDfs, b.childDfs); cut(A.pblocks, T.pblocks, e.pblocks, b.pblocks);
    cut(A.meshes, T.meshes, e.meshes, b.meshes);
    const int triBase = A.meshes.empty() ? 0 : A.meshes.back().triBase + A.meshes.back().ntri, oldTris = meshes[k].ntri, total = A.totalTris;
    take_material();
    meshes[k] = std::move(nm);
    meshTrees[k] = std::move(nt);
    append_parts(k, k + 1, triBase, err);   // (cannot fail: the lists were checked above)
    // ... and the others behind the new part, the words that count from an array's beginning moved by what the part grew: the block and
    // reference bases of `blocks` and `pblocks` (words 0-1), the triangle base in refN.w, runBase, MeshRec's rootBlock / rootRef / triBase / dfsBase
    const RawSizes s = sizes_now();
    const int dBlock = (int)(s.blocks / 2) - (int)(e.blocks / 2), dRef = (int)s.refN - (int)e.refN, dTri = ntri - oldTris, dRun = (int)(s.runTB / 4) - (int)(e.runTB / 4);
    for (size_t i = 0; i + 1 < T.blocks.size(); i += 2) { f4 &lo = T.blocks[i]; lo.x = i2f(f2i(lo.x) + dBlock); lo.y = i2f(f2i(lo.y) + dRef); }
    for (size_t i = 0; i < T.pblocks.size(); i += PBLOCK_WORDS) { T.pblocks[i] = i2f(f2i(T.pblocks[i]) + dBlock); T.pblocks[i + 1] = i2f(f2i(T.pblocks[i + 1]) + dRef); }
    for (f4 &q : T.refN) q.w = i2f(f2i(q.w) + dTri);
    for (int &q : T.runBase) if (q >= 0) q += dRun;
    for (MeshRec &mr : T.meshes) {
        if (mr.rootBlock >= 0) mr.rootBlock += dBlock;
        mr.rootRef += dRef; mr.triBase += dTri; mr.dfsBase += 8 * dBlock;
    }
    auto paste = [](auto &to, const auto &from) { to.insert(to.end(), from.begin(), from.end()); };
    paste(A.blocks, T.blocks); paste(A.refN, T.refN); paste(A.refG, T.refG); paste(A.shade, T.shade); paste(A.leafNB, T.leafNB); paste(A.leafTB, T.leafTB);
    paste(A.runBase, T.runBase); paste(A.runTB, T.runTB); paste(A.childDfs, T.childDfs); paste(A.pblocks, T.pblocks); paste(A.meshes, T.meshes);
    for (size_t mi = k + 1; mi < (size_t)builtMeshes; mi++) {
        RawSizes &p = partStart[mi];
        p.blocks += s.blocks - e.blocks; p.refN += s.refN - e.refN; p.shade += s.shade - e.shade; p.leafNB += s.leafNB - e.leafNB; p.leafTB += s.leafTB - e.leafTB;
        p.runBase += s.runBase - e.runBase; p.runTB += s.runTB - e.runTB; p.childDfs += s.childDfs - e.childDfs; p.pblocks += s.pblocks - e.pblocks; p.meshes += s.meshes - e.meshes;
    }
    raw = sizes_now();
    A.totalTris = total + dTri;
    A.meshDepth = depth;
    assemble();
    material_part();
    if (built)   // the pre-cull records are built on Mesh.MeshBoundingBox: those of the bodies that name the mesh, from the bodies' current poses
        for (size_t o = 0; o < objects.size(); o++)
            if (std::find(objects[o].meshes.begin(), objects[o].meshes.end(), mesh) != objects[o].meshes.end()) refresh_cull((int)o);
    return XRT_OK;
}

bool HostScene::set_materials(const int *ids, int n, const xrt_material *mats, MaterialEdit &edit, std::string &err) {
    edit = MaterialEdit();
    if (n < 0 || (n > 0 && (!ids || !mats))) { err = "xrt_scene_set_materials: null argument"; return false; }
    const int nMesh = (int)meshes.size();
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= nMesh) { err = "xrt_scene_set_materials: mesh id " + std::to_string(ids[i]) + " out of range (" + std::to_string(nMesh) + " meshes)"; return false; }
    // the last entry of a mesh wins (the setters called one after the other); everything is checked before anything is applied
    std::vector<int> last((size_t)nMesh, -1), order;
    for (int i = 0; i < n; i++) last[(size_t)ids[i]] = i;
    for (int i = 0; i < n; i++) if (last[(size_t)ids[i]] == i) order.push_back(i);
    for (int i : order) {
        const xrt_material &m = mats[i];
        const HostMesh &hm = meshes[(size_t)ids[i]];
        if (m.tex_argb) {
            if (m.tex_width <= 0 || m.tex_height <= 0 || (long long)m.tex_width * m.tex_height > (1LL << 30)) { err = "xrt_scene_set_materials: texels of " + std::to_string(m.tex_width) + " x " + std::to_string(m.tex_height); return false; }
        } else if (m.use_texture) {
            if (hm.texels.empty()) { err = "xrt_scene_set_materials: UseTexture without texels on a mesh that has none (the bitmap was never locked, MAT:65)"; return false; }
            if (!((m.tex_width == 0 && m.tex_height == 0) || (m.tex_width == hm.texW && m.tex_height == hm.texH))) { err = "xrt_scene_set_materials: tex_width / tex_height differ from the texels the mesh keeps"; return false; }
        }
    }
    bool repack = false;
    for (int i : order) {
        const xrt_material &m = mats[i];
        HostMesh &hm = meshes[(size_t)ids[i]];
        hm.reflectiveness = m.reflectiveness;
        hm.refractionIndex = m.refraction_index;
        hm.transparent = m.transparent != 0;
        hm.interpolateNormals = m.interpolate_normals != 0;
        hm.useTexture = m.use_texture != 0;
        if (!m.tex_argb) continue;
        const size_t count = (size_t)m.tex_width * (size_t)m.tex_height;
        const bool sameShape = hm.texels.size() == count && hm.texelsP.empty() == (m.tex_pargb == nullptr);
        hm.texW = m.tex_width; hm.texH = m.tex_height;
        hm.texels.assign(m.tex_argb, m.tex_argb + count);
        if (m.tex_pargb) hm.texelsP.assign(m.tex_pargb, m.tex_pargb + count); else hm.texelsP.clear();
        edit.texels = true;
        if (!built || repack) continue;
        if (!sameShape) { repack = true; continue; }
        // texels of the size the mesh had: written over the old ones where they lie in the arena
        const MaterialRec &r = arrays.materials[(size_t)ids[i]];
        std::copy(hm.texels.begin(), hm.texels.end(), arrays.texels.begin() + r.texOffset);
        if (!hm.texelsP.empty()) std::copy(hm.texelsP.begin(), hm.texelsP.end(), arrays.texels.begin() + r.texOffsetP);
        const size_t lo = (size_t)r.texOffset, hi = (size_t)(hm.texelsP.empty() ? r.texOffset : r.texOffsetP) + count;
        if (edit.texHi == edit.texLo) { edit.texLo = lo; edit.texHi = hi; }
        else { edit.texLo = std::min(edit.texLo, lo); edit.texHi = std::max(edit.texHi, hi); }
    }
    if (!built) return true;   // (the next build reads the materials)
    SceneArrays &A = arrays;
    A.anyTransparent = A.anyTexture = false;   // over ALL meshes: turning the last Transparent material opaque clears the flag
    if (repack) {   // some texels changed their size: the arena is packed again, as build packs it
        A.materials.clear();
        A.texels.clear();
        for (const HostMesh &hm : meshes) append_material(A, hm);
        if (A.texels.empty()) A.texels.assign(1, 0u);
        edit.texFull = true;
    } else {        // the records again, the texels where they are
        size_t off = 0;
        for (size_t k = 0; k < meshes.size(); k++) {
            A.materials[k] = material_record(meshes[k], off);
            A.anyTransparent = A.anyTransparent || meshes[k].transparent;
            A.anyTexture = A.anyTexture || meshes[k].useTexture;
        }
    }
    if (edit.texFull) { edit.texLo = 0; edit.texHi = A.texels.size(); }
    return true;
}

bool HostScene::set_triangle_shading(int mesh, const int *ids, int first, int n, const float *normals, const float *uv, const float *color, std::string &err) {
    const std::string fn = "xrt_scene_set_triangle_shading: ";
    if (mesh < 0 || mesh >= (int)meshes.size()) { err = fn + "mesh id " + std::to_string(mesh) + " out of range (" + std::to_string(meshes.size()) + " meshes)"; return false; }
    if (n < 0 || first < 0) { err = fn + "negative count or first triangle"; return false; }
    if (ids && first != 0) { err = fn + "first_tri must be 0 with a list of triangle ids"; return false; }
    if (n > 0 && !normals && !uv && !color) { err = fn + "no field given"; return false; }
    HostMesh &hm = meshes[(size_t)mesh];
    if (!ids && (long long)first + n > (long long)hm.ntri) { err = fn + "triangles " + std::to_string(first) + " .. " + std::to_string((long long)first + n) + " outside the mesh's " + std::to_string(hm.ntri); return false; }
    for (int i = 0; ids && i < n; i++)
        if (ids[i] < 0 || ids[i] >= hm.ntri) { err = fn + "triangle id " + std::to_string(ids[i]) + " outside the mesh's " + std::to_string(hm.ntri); return false; }
    // entries in the order given: a later entry of a triangle overwrites an earlier one
    // (hm.sn -- the surface normals of RE:49, what refN, the node normal boxes and MeshRec's nbMin / nbMax / nbDiag are built from -- is not among the fields:
    // every bound on the normals stays valid, no record of the octree changes)
    f4 *recs = mesh < builtMeshes ? arrays.shade.data() + (size_t)SHADE_F4 * (size_t)arrays.meshes[(size_t)mesh].triBase : nullptr;
    for (int i = 0; i < n; i++) {
        const size_t t = (size_t)(ids ? ids[i] : first + i);
        if (normals) std::memcpy(&hm.n[9 * t], normals + 9 * (size_t)i, 36);
        if (uv) std::memcpy(&hm.uv[6 * t], uv + 6 * (size_t)i, 24);
        if (color) std::memcpy(&hm.color[4 * t], color + 4 * (size_t)i, 16);
        if (!recs) continue;   // (the next build reads the mesh)
        f4 *s = recs + SHADE_F4 * t;
        if (normals) for (int k = 0; k < 3; k++) std::memcpy(&s[k], normals + 9 * (size_t)i + 3 * k, 12);
        if (uv) {
            for (int k = 0; k < 3; k++) std::memcpy(&s[k].w, uv + 6 * (size_t)i + k, 4);
            std::memcpy(&s[4], uv + 6 * (size_t)i + 3, 12);
        }
        if (color) std::memcpy(&s[3], color + 4 * (size_t)i, 16);
    }
    return true;
}

void HostScene::take_triangle_shading(int mesh, const f4 *recs) {
    HostMesh &hm = meshes[(size_t)mesh];
    f4 *own = mesh < builtMeshes ? arrays.shade.data() + (size_t)SHADE_F4 * (size_t)arrays.meshes[(size_t)mesh].triBase : nullptr;
    for (size_t t = 0; t < (size_t)hm.ntri; t++) {
        const f4 *s = recs + SHADE_F4 * t;
        for (int k = 0; k < 3; k++) { std::memcpy(&hm.n[9 * t + 3 * k], &s[k], 12); std::memcpy(&hm.uv[6 * t + k], &s[k].w, 4); }
        std::memcpy(&hm.uv[6 * t + 3], &s[4], 12);
        std::memcpy(&hm.color[4 * t], &s[3], 16);
        if (own) { std::memcpy(own + SHADE_F4 * t, s, 4 * sizeof(f4)); std::memcpy(own + SHADE_F4 * t + 4, &s[4], 12); }
    }
}

bool HostScene::build_tree(int sceneThreshold, std::string &err) {
    if (!built) { err = "xrt_scene_build_tree: call xrt_scene_build first"; return false; }
    if (sceneThreshold <= 0) sceneThreshold = 20;  // OSM:50
    built = false;
    if (!scene_part(sceneThreshold, err)) return false;
    built = true;
    return true;
}

// ---- scene file -----------------------------------------------------------------------------------------------------------
// "XRTSCENE" u32 version=1 u32 nMeshes u32 nObjects, then per mesh: i32 ntri, f32 bbox[6], f32 reflectiveness, f32 refractionIndex,
// i32 flags (1 transparent, 2 interpolateNormals, 4 useTexture, 8 has premultiplied texels), i32 texW, i32 texH, f32 v[9n] n[9n]
// uv[6n] sn[3n] color[4n], u32 texels[texW*texH] (if 4), u32 texelsP[texW*texH] (if 8); per object: i32 nMeshes, i32 ids[],
// f32 world[16] invWorld[16] bbox[6] worldBbox[6].
namespace {
struct FileW {
    FILE *f; bool ok = true;
    template <class T> void put(const T *p, size_t n) { if (ok && n && fwrite(p, sizeof(T), n, f) != n) ok = false; }
    template <class T> void one(T v) { put(&v, 1); }
};
struct FileR {
    FILE *f; bool ok = true;
    long long left = 0;   // bytes of the file not read yet: no array is sized for more than the file can hold
    template <class T> void get(T *p, size_t n) {
        if (!ok || !n) return;
        if ((unsigned long long)n > (unsigned long long)left / sizeof(T) || fread(p, sizeof(T), n, f) != n) { ok = false; return; }
        left -= (long long)(n * sizeof(T));
    }
    template <class T> T one() { T v{}; get(&v, 1); return v; }
    template <class T> void vec(std::vector<T> &v, size_t n) {
        if (!ok) return;
        if ((unsigned long long)n > (unsigned long long)left / sizeof(T)) { ok = false; return; }   // a hostile header cannot ask for more than the file holds
        v.resize(n); get(v.data(), n);
    }
};
}  // namespace

bool HostScene::save(const char *path, std::string &err) const {
    FILE *f = path ? fopen(path, "wb") : nullptr;
    if (!f) { err = "xrt_scene_save: cannot open the file for writing"; return false; }
    FileW w{f};
    w.put("XRTSCENE", 8);
    w.one<uint32_t>(1); w.one<uint32_t>((uint32_t)meshes.size()); w.one<uint32_t>((uint32_t)objects.size());
    for (const HostMesh &m : meshes) {
        w.one<int32_t>(m.ntri); w.put(m.bbox, 6); w.one<float>(m.reflectiveness); w.one<float>(m.refractionIndex);
        // (texels a mesh keeps while UseTexture is off -- xrt_scene_set_materials -- are not part of the file: it holds what add_mesh would be given)
        w.one<int32_t>((m.transparent ? 1 : 0) | (m.interpolateNormals ? 2 : 0) | (m.useTexture ? 4 : 0) | (m.useTexture && !m.texelsP.empty() ? 8 : 0));
        w.one<int32_t>(m.useTexture ? m.texW : 0); w.one<int32_t>(m.useTexture ? m.texH : 0);
        w.put(m.v.data(), m.v.size()); w.put(m.n.data(), m.n.size()); w.put(m.uv.data(), m.uv.size()); w.put(m.sn.data(), m.sn.size());
        w.put(m.color.data(), m.color.size());
        if (m.useTexture) w.put(m.texels.data(), m.texels.size());
        if (m.useTexture && !m.texelsP.empty()) w.put(m.texelsP.data(), m.texelsP.size());
    }
    for (const HostObject &o : objects) {
        w.one<int32_t>((int32_t)o.meshes.size()); w.put(o.meshes.data(), o.meshes.size());
        w.put(o.world, 16); w.put(o.invWorld, 16); w.put(o.bbox, 6); w.put(o.worldBbox, 6);
    }
    const bool ok = w.ok && fclose(f) == 0;
    if (!ok) err = "xrt_scene_save: write failed";
    return ok;
}

bool HostScene::load(const char *path, std::string &err) {
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) { err = "xrt_scene_load: cannot open the file"; return false; }
    FileR r{f};
    if (fseek(f, 0, SEEK_END) == 0) { r.left = ftell(f); if (r.left < 0 || fseek(f, 0, SEEK_SET) != 0) r.ok = false; } else r.ok = false;
    char magic[8] = {0};
    r.get(magic, 8);
    const uint32_t version = r.one<uint32_t>(), nm = r.one<uint32_t>(), no = r.one<uint32_t>();
    if (!r.ok || std::memcmp(magic, "XRTSCENE", 8) != 0 || version != 1 || nm > (1u << 24) || no > (1u << 24)) { fclose(f); err = "xrt_scene_load: not a version-1 xrt scene file"; return false; }
    // The records are read into a scratch scene through add_mesh / add_object -- the very calls (and checks) the header promises a
    // load is equivalent to; the lists grow as records arrive, so the counts of a hostile header allocate nothing.
    HostScene tmp;
    std::string why;
    for (uint32_t i = 0; i < nm && r.ok; i++) {
        HostMesh m;
        m.ntri = r.one<int32_t>(); r.get(m.bbox, 6); m.reflectiveness = r.one<float>(); m.refractionIndex = r.one<float>();
        const int flags = r.one<int32_t>();
        m.texW = r.one<int32_t>(); m.texH = r.one<int32_t>();
        if (!r.ok || m.ntri < 0 || m.ntri >= (1 << 28) || m.texW < 0 || m.texH < 0 || (long long)m.texW * m.texH > (1LL << 30) || (flags & ~15)) { r.ok = false; break; }
        const bool useTexture = (flags & 4) != 0, hasP = (flags & 8) != 0;
        if (hasP && !useTexture) { r.ok = false; why = "premultiplied texels without UseTexture"; break; }
        if (!useTexture && (m.texW != 0 || m.texH != 0)) { r.ok = false; why = "texture size without UseTexture"; break; }
        const size_t n = (size_t)m.ntri;
        r.vec(m.v, n * 9); r.vec(m.n, n * 9); r.vec(m.uv, n * 6); r.vec(m.sn, n * 3); r.vec(m.color, n * 4);
        if (useTexture) r.vec(m.texels, (size_t)m.texW * m.texH);
        if (hasP) r.vec(m.texelsP, (size_t)m.texW * m.texH);
        if (!r.ok) break;
        xrt_material xm;
        std::memset(&xm, 0, sizeof(xm));
        xm.reflectiveness = m.reflectiveness; xm.refraction_index = m.refractionIndex;
        xm.transparent = (flags & 1) ? 1 : 0; xm.interpolate_normals = (flags & 2) ? 1 : 0; xm.use_texture = useTexture ? 1 : 0;
        xm.tex_argb = useTexture ? m.texels.data() : nullptr; xm.tex_pargb = hasP ? m.texelsP.data() : nullptr;
        xm.tex_width = m.texW; xm.tex_height = m.texH;
        static const float none[9] = {0};   // (an empty vector has no address; add_mesh rejects null arrays)
        if (tmp.add_mesh(n ? m.v.data() : none, n ? m.n.data() : none, n ? m.uv.data() : none, n ? m.sn.data() : none, n ? m.color.data() : none, m.ntri, &xm, m.bbox, why) < 0) { r.ok = false; break; }
    }
    for (uint32_t i = 0; i < no && r.ok; i++) {
        HostObject o;
        const int k = r.one<int32_t>();
        if (!r.ok || k < 0 || k > (1 << 20)) { r.ok = false; break; }
        r.vec(o.meshes, (size_t)k);
        r.get(o.world, 16); r.get(o.invWorld, 16); r.get(o.bbox, 6); r.get(o.worldBbox, 6);
        if (!r.ok) break;
        static const int noId[1] = {0};
        if (tmp.add_object(k ? o.meshes.data() : noId, k, o.world, o.invWorld, o.bbox, o.worldBbox, why) < 0) { r.ok = false; break; }
    }
    fclose(f);
    if (!r.ok) { err = "xrt_scene_load: truncated or corrupt scene file" + (why.empty() ? std::string() : " (" + why + ")"); return false; }
    meshes = std::move(tmp.meshes); objects = std::move(tmp.objects);
    built = false;
    builtMeshes = -1;
    return true;
}

SceneView HostScene::host_view() const {
    SceneView S;
    const SceneArrays &A = arrays;
    S.blocks = A.blocks.data(); S.childDfs = A.childDfs.data(); S.leafNB = A.leafNB.data(); S.leafTB = A.leafTB.data(); S.runBase = A.runBase.data(); S.runTB = A.runTB.data(); S.refT = A.refT.data(); S.pblocks = A.pblocks.data(); S.lrec = A.lrec.data();
    S.refN = A.refN.data(); S.refG = A.refG.data(); S.meshes = A.meshes.data();
    S.snodes = A.snodes.data(); S.srefs = A.srefs.data(); S.scull = A.scull.data(); S.objects = A.objects.data(); S.objMesh = A.objMesh.data();
    S.nMeshes = (int)meshes.size(); S.nObjects = (int)objects.size();
    S.sceneDepth = A.sceneDepth + 1; S.meshDepth = A.meshDepth + 1;
    S.nodeCull = 1;
    return S;
}

}  // namespace xrt
