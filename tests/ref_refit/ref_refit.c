/* ref_refit.c -- TEST INFRASTRUCTURE: the mesh refit of DESIGN.md ("Deforming meshes") restated in plain C,
 * independently of rt_host.cpp and of rt_refit.hip.  A recursive walk from node 0 over whatever tree the caller
 * hands in; IEEE f32, no contraction; min and max in the total order that puts -0 below +0.
 *
 *   triangle in slot t (its original index is indices[t]), per axis:
 *       lo = min(a, min(b, c)), hi = max(a, max(b, c)), p = 0.5f*(lo + hi), r = 0.5f*(hi - lo),
 *       extent [p - r, p + r]
 *   leaf:      (MIN, MAX) = the union of the extents of slots [left_first, left_first + count)
 *   interior:  (MIN, MAX) = the union of its two children's (MIN, MAX)
 *   a node with a triangle below it:  bv_p = 0.5f*(MIN + MAX), bv_r = 0.5f*(MAX - MIN)
 *   every other node keeps its bytes (unreachable ones, the padding entry, a node without triangles)
 *
 * A node is interior when count == 0, left_first != 0 and left_first + 1 < node_count. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_abi.h"

#define EXPORT __attribute__((visibility("default")))

static float min_total(float a, float b) { return (a < b || (a == b && signbit(a))) ? a : b; }
static float max_total(float a, float b) { return (a > b || (a == b && !signbit(a))) ? a : b; }

typedef struct { float mn[3], mx[3]; int any; } box_t;

static box_t no_box(void) {
    box_t b;
    for (int k = 0; k < 3; ++k) { b.mn[k] = INFINITY; b.mx[k] = -INFINITY; }
    b.any = 0;
    return b;
}

static void grow_box(box_t* b, const float* mn, const float* mx) {
    for (int k = 0; k < 3; ++k) { b->mn[k] = min_total(b->mn[k], mn[k]); b->mx[k] = max_total(b->mx[k], mx[k]); }
    b->any = 1;
}

static int is_interior(const rt_bvh_node* nodes, uint32_t node_count, uint32_t i) {
    return nodes[i].count == 0 && nodes[i].left_first != 0 && (uint64_t)nodes[i].left_first + 1 < node_count;
}

/* the extent of the triangle whose vertices are v[0..8] */
static void triangle_extent(const float* v, float* mn, float* mx) {
    for (int k = 0; k < 3; ++k) {
        const float a = v[k], b = v[3 + k], c = v[6 + k];
        const float lo = min_total(a, min_total(b, c)), hi = max_total(a, max_total(b, c));
        const float p = 0.5f*(lo + hi), r = 0.5f*(hi - lo);
        mn[k] = p - r;
        mx[k] = p + r;
    }
}

static box_t walk(const float* tris, const uint32_t* indices, rt_bvh_node* nodes, uint32_t node_count, uint32_t i,
                  uint32_t depth, int* bad) {
    box_t b = no_box();
    if (depth > node_count) { *bad = 1; return b; }          /* not a tree */
    if (nodes[i].count) {
        for (uint32_t t = nodes[i].left_first; t < nodes[i].left_first + nodes[i].count; ++t) {
            float mn[3], mx[3];
            triangle_extent(tris + 9*(size_t)indices[t], mn, mx);
            grow_box(&b, mn, mx);
        }
    } else if (is_interior(nodes, node_count, i)) {
        for (uint32_t g = 0; g < 2; ++g) {
            const box_t c = walk(tris, indices, nodes, node_count, nodes[i].left_first + g, depth + 1, bad);
            if (c.any) grow_box(&b, c.mn, c.mx);
        }
    }
    if (b.any) {
        float* p = &nodes[i].bv_p.x;
        float* r = &nodes[i].bv_r.x;
        for (int k = 0; k < 3; ++k) { p[k] = 0.5f*(b.mn[k] + b.mx[k]); r[k] = 0.5f*(b.mx[k] - b.mn[k]); }
    }
    return b;
}

/* tris: 9 floats per triangle, ORIGINAL order; normals likewise or NULL; indices: slot -> original.
 * nodes: refitted in place.  out_tris: 12 floats per slot (a, 0, b - a, 0, c - a, 0); out_normals: 9 floats per slot
 * (NULL with normals NULL).  Returns 0, or 1 when the nodes are no tree. */
EXPORT int ref_refit(uint32_t triangle_count, const float* tris, const float* normals, const uint32_t* indices,
                     uint32_t node_count, rt_bvh_node* nodes, float* out_tris, float* out_normals) {
    for (uint32_t t = 0; t < triangle_count; ++t) {
        const float* v = tris + 9*(size_t)indices[t];
        float* o = out_tris + 12*(size_t)t;
        for (int k = 0; k < 3; ++k) {
            o[k] = v[k];
            o[4 + k] = v[3 + k] - v[k];
            o[8 + k] = v[6 + k] - v[k];
        }
        o[3] = o[7] = o[11] = 0.0f;
        if (normals) memcpy(out_normals + 9*(size_t)t, normals + 9*(size_t)indices[t], 36);
    }
    int bad = 0;
    if (node_count) walk(tris, indices, nodes, node_count, 0u, 0u, &bad);
    return bad;
}

/* The BVH4 tables of a mesh from its (refitted) BVH2: BVH4 node k was made from BVH2 node src[k]; its child slots
 * are that node's two children, each replaced by its own two children when it is interior (slots 2g, 2g + 1 for
 * child g; a leaf child takes slot 2g alone).  nodes4: 32 floats per BVH4 node, of which rows 0..5 (bv_p.xyz,
 * bv_r.xyz, one float per slot) are written for the slots that hold a child; mid4: 12 floats per BVH4 node, the two
 * children's own boxes (pL.xyz rL.xyz pR.xyz rR.xyz), written when src[k] is interior.  Everything else stays. */
EXPORT void ref_refit_bvh4(uint32_t node_count, const rt_bvh_node* nodes, uint32_t n4, const uint32_t* src, float* nodes4,
                           float* mid4) {
    for (uint32_t k = 0; k < n4; ++k) {
        const uint32_t i = src[k];
        if (!is_interior(nodes, node_count, i)) continue;
        const uint32_t l = nodes[i].left_first;
        for (uint32_t g = 0; g < 2; ++g) {
            const uint32_t c = l + g;
            uint32_t slot[2] = {c, 0xFFFFFFFFu};
            if (is_interior(nodes, node_count, c)) { slot[0] = nodes[c].left_first; slot[1] = nodes[c].left_first + 1; }
            for (uint32_t j = 0; j < 2; ++j) {
                if (slot[j] == 0xFFFFFFFFu) continue;
                const float* p = &nodes[slot[j]].bv_p.x;
                const float* r = &nodes[slot[j]].bv_r.x;
                for (int a = 0; a < 3; ++a) {
                    nodes4[32*(size_t)k + 4*a + 2*g + j] = p[a];
                    nodes4[32*(size_t)k + 4*(3 + a) + 2*g + j] = r[a];
                }
            }
            memcpy(mid4 + 12*(size_t)k + 6*g, &nodes[c].bv_p.x, 12);
            memcpy(mid4 + 12*(size_t)k + 6*g + 3, &nodes[c].bv_r.x, 12);
        }
    }
}
