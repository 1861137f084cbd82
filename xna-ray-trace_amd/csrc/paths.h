// paths.h — RayTracer.points (RT:504, 543, 701, 740-747): the order in which one CastRay recursion appends its line segments, and the ray it
// leaves in its `ref Ray ray` (RT:692-694).  XRT_HD: k_paths_count / k_paths_emit (paths.hip) walk the staging records of a pass with it, a CPU
// test walks recursion trees recorded from the oracle with the same source (tests/paths/paths_order.cpp).
//
// A node of the recursion is named as the pass names it (kernels.h ShadeArgs::rayNode): in a ray tree (Transparent materials) the reflection of
// node i is 2i + 1 and its refraction 2i + 2, the root is 0; in a plain reflection chain the node is the generation.  Two facts per node, both
// left by the capture kernel: did its ray hit, and where (the world position; the ray of either child starts there, RT:548 / RT:692), and -- for a
// refraction child -- the direction it was cast with (RT:694), which exists whether or not that ray hits anything.
//
// C(ray, it), RT:506-737:   miss: nothing.   hit: white (ray.Position, hit);  if it < MaxReflections: C(fresh reflection ray, it + 1);  if also
// Transparent: ray = (hit, refracted), C(ray, it + 1) ON THE SAME VARIABLE, then red (ray.Position, ray.Direction * 100) with ray as the nested call
// left it -- so every red segment of an unbroken refraction chain carries the chain's LAST ray, and that ray is what the caller's variable holds.
#pragma once
#include <stdint.h>

#include "xrt_core.h"

namespace xrt {

constexpr uint32_t PATH_WHITE = 0xFFFFFFFFu, PATH_RED = 0xFF0000FFu;   // Color.White / Color.Red as rgba_out packs colours
constexpr int PATH_TREE_DEPTH = 12;                                     // a ray tree is at most this many reflections deep (xrt.h)

XRT_HD int  path_reflection(int node, bool tree) { return tree ? 2 * node + 1 : node + 1; }
XRT_HD int  path_refraction(int node) { return 2 * node + 2; }
XRT_HD bool path_is_refraction(int node) { return node > 0 && (node & 1) == 0; }   // (ray trees only)
XRT_HD int  path_parent(int node, bool tree) { return tree ? (node - 1) >> 1 : node - 1; }
// vertices a recursion of `depth` generations below its root can append at most: two per hit and two per refraction
XRT_HD long long path_vertex_bound(int depth, bool tree) {
    return tree ? 2 * (((1LL << (depth + 1)) - 1) + ((1LL << depth) - 1)) : 2 * ((long long)depth + 1);
}

struct PathRay { float o[3], d[3]; };

// Non-finite values are recorded as they are -- and "as they are" is a bit pattern a host compares.  The reference computes on x86, where
// every invalid operation (the Math.Sqrt of a negative number of RT:676 under total internal reflection) yields the negative quiet NaN
// 0xFFC00000 and every later operation hands that operand on; gfx950 makes 0x7FC00000 of the same square root.  The NaN components of a
// refraction direction the device computed are recorded with the x86 pattern: what the reference's list holds.
XRT_HD float path_recorded(float x) { return x != x ? i2f((int)0xFFC00000u) : x; }

// Walks one root ray's recursion depth first and hands its segments to `sink` in the reference's order.
//   src.hit(node, w)        -> did the node's ray hit; w = world position of the hit
//   src.refracted(node, d)  -> was refraction child `node` cast (its parent is Transparent and may still reflect); d = its direction
//   sink.segment(a, b, colour)
// depth = MaxReflections - iteration (generations below the root that may exist).  Returns whether the root call overwrote its ray; `back` is then
// the ray it left (the last ray of the refraction chain that starts at the root).
template <class Src, class Sink>
XRT_HD bool paths_walk(const Src &src, const float rootO[3], int depth, bool tree, Sink &sink, PathRay &back) {
    if (!tree) {   // a chain: white segments hit to hit until a miss or the depth limit
        float a[3] = {rootO[0], rootO[1], rootO[2]}, w[3];
        for (int k = 0; k <= depth; k++) {
            if (!src.hit(k, w)) break;
            sink.segment(a, w, PATH_WHITE);
            a[0] = w[0]; a[1] = w[1]; a[2] = w[2];
        }
        return false;
    }
    constexpr int MAXD = PATH_TREE_DEPTH + 2;
    int stNode[MAXD], stPhase[MAXD];
    float hp[MAXD][3];   // the hit of the node at every level of the stack: where its children start
    int sp = 0;
    stNode[0] = 0; stPhase[0] = 0;
    bool rootBack = false;
    while (sp >= 0) {
        const int node = stNode[sp];
        const float *pos = sp == 0 ? rootO : hp[sp - 1];
        bool done = false;
        if (stPhase[sp] == 0) {
            if (!src.hit(node, hp[sp])) done = true;   // RT:729-733
            else {
                sink.segment(pos, hp[sp], PATH_WHITE);   // RT:543, before the depth test of RT:545
                if (sp >= depth || sp + 1 >= MAXD) done = true;
                else { stPhase[sp] = 1; sp++; stNode[sp] = path_reflection(node, true); stPhase[sp] = 0; continue; }   // RT:556-559
            }
        } else if (stPhase[sp] == 1) {
            float d[3];
            if (src.refracted(path_refraction(node), d)) { stPhase[sp] = 2; sp++; stNode[sp] = path_refraction(node); stPhase[sp] = 0; continue; }   // RT:692-698
            done = true;
        } else {   // the refraction returned: `back` is the ray the nested calls left (RT:701)
            const float q[3] = {back.d[0] * 100.0f, back.d[1] * 100.0f, back.d[2] * 100.0f};
            sink.segment(back.o, q, PATH_RED);
            if (sp == 0) rootBack = true;
            sp--;   // (this call's ray is the chain's: `back` stays)
            continue;
        }
        if (done) {   // a call that assigns nothing to its ray: where a refraction chain ends
            if (path_is_refraction(node)) {
                back.o[0] = pos[0]; back.o[1] = pos[1]; back.o[2] = pos[2];
                (void)src.refracted(node, back.d);
            }
            sp--;
        }
    }
    return rootBack;
}

}  // namespace xrt
