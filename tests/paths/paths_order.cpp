// TEST INFRASTRUCTURE -- the library's ordering rule (csrc/paths.h, the source k_paths_count / k_paths_emit compile) driven on the CPU:
// recursion trees given as node records -- (ray, node, hit position) and (ray, refraction child, direction) -- are walked exactly as the
// device walks its staging records, into vertices, vertex_start and rays_back.
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/xrt.h"
#include "../../xna-ray-trace_amd/csrc/paths.h"

namespace {

struct Rec3 { float v[3]; };
struct TreeSrc {
    const std::unordered_map<int, Rec3> *hits, *dirs;
    bool hit(int node, float w[3]) const { auto it = hits->find(node); if (it == hits->end()) return false; std::memcpy(w, it->second.v, 12); return true; }
    bool refracted(int node, float d[3]) const { auto it = dirs->find(node); if (it == dirs->end()) return false; std::memcpy(d, it->second.v, 12); return true; }
};
struct CountSink { long long n = 0; void segment(const float *, const float *, uint32_t) { n += 2; } };
struct EmitSink {
    xrt_path_vertex *out; long long at, cap;
    void segment(const float a[3], const float b[3], uint32_t color) {
        if (at + 2 <= cap) {
            std::memcpy(out[at].position, a, 12); out[at].color = color;
            std::memcpy(out[at + 1].position, b, 12); out[at + 1].color = color;
        }
        at += 2;
    }
};

}  // namespace

extern "C" {

// count, exclusive scan, emit -- the three steps of paths.hip.  Returns the number of vertices the batch needs.
int64_t xrt_paths_order_cpu(const xrt_ray *rays, int64_t n, int32_t depth, int32_t tree, int64_t n_recs, const int64_t *rec_ray, const int32_t *rec_node,
                            const int32_t *rec_kind, const float *rec_v, xrt_path_vertex *vertices, int64_t capacity, int64_t *vertex_start, xrt_ray *rays_back) {
    std::vector<std::unordered_map<int, Rec3>> hits((size_t)n), dirs((size_t)n);
    for (int64_t i = 0; i < n_recs; i++) {
        Rec3 r; std::memcpy(r.v, rec_v + 3 * i, 12);
        (rec_kind[i] ? dirs : hits)[(size_t)rec_ray[i]][rec_node[i]] = r;
    }
    long long total = 0;
    for (int64_t i = 0; i < n; i++) {
        TreeSrc src{&hits[(size_t)i], &dirs[(size_t)i]};
        CountSink cs; xrt::PathRay back;
        (void)xrt::paths_walk(src, rays[i].o, depth, tree != 0, cs, back);
        vertex_start[i] = total;
        total += cs.n;
    }
    vertex_start[n] = total;
    for (int64_t i = 0; i < n; i++) {
        TreeSrc src{&hits[(size_t)i], &dirs[(size_t)i]};
        EmitSink es{vertices, vertex_start[i], capacity & ~1LL}; xrt::PathRay back;
        const bool changed = xrt::paths_walk(src, rays[i].o, depth, tree != 0, es, back);
        if (rays_back) {
            xrt_ray r = rays[i];
            if (changed) { std::memcpy(r.o, back.o, 12); std::memcpy(r.d, back.d, 12); }
            rays_back[i] = r;
        }
    }
    return total;
}

int32_t xrt_paths_node(int32_t node, int32_t tree, int32_t which) {   // the tree-position arithmetic: 0 reflection, 1 refraction, 2 parent, 3 is-refraction
    switch (which) {
        case 0: return xrt::path_reflection(node, tree != 0);
        case 1: return xrt::path_refraction(node);
        case 2: return xrt::path_parent(node, tree != 0);
        default: return xrt::path_is_refraction(node) ? 1 : 0;
    }
}
int64_t xrt_paths_bound(int32_t depth, int32_t tree) { return xrt::path_vertex_bound(depth, tree != 0); }

}  // extern "C"
