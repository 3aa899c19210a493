// rt_refit.hip — deforming meshes after upload: new vertices for one mesh of an uploaded scene, its triangle records
// and slot-order normals rewritten and its BVH refitted on the device (rt_scene_update_mesh_device,
// rt_scene_update_mesh), and the read-back of a mesh's table slices for the tests (rt_debug_scene_mesh_table).  Beyond
// the reference, an opt-in: no other entry calls it and no render kernel changes.
//
// The refit is defined operation by operation in DESIGN.md ("Deforming meshes"); tests/ref_refit/ref_refit.c restates
// it in plain C and rth_update_mesh on the host model, and all three agree byte for byte: IEEE f32, no contraction,
// min and max in the total order that puts -0 below +0.
//
// No box passes between workgroups inside a launch (the XCDs' L2s are not coherent and an agent-scope fence per node
// would cost more than the node): a workgroup refits one subtree of the plan in LDS, one __syncthreads() per level, and
// what a later subtree needs of an earlier one crosses a kernel boundary in HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_internal.h"

namespace {

int fail(int code, const std::string& message) { rt_internal_set_error(message.c_str()); return code; }
#define RF_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(RT_ERROR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t SUB_CAP = 1024;          // nodes of one workgroup's subtree: 6 floats each, 24 KB of LDS
constexpr uint32_t SUB_THREADS = 256;
constexpr uint32_t EXTERNAL = 0x80000000u;  // a child reference by node index (its pair is in HBM), not by local index
enum : uint32_t { K_LEAF = 0, K_INTERIOR = 1, K_EMPTY = 2, K_ROOT_BIT = 4 };   // Entry::w
enum { RES_REFUSED = 0, RES_OUTSIDE = 1, RES_BOX = 2, RES_HAS_BOX = 8, RES_WORDS = 16 };   // the result words

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
// the total order: -0 below +0
__device__ __forceinline__ float tmin(float a, float b) { return (a < b || (a == b && (__float_as_uint(a) >> 31))) ? a : b; }
__device__ __forceinline__ float tmax(float a, float b) { return (a > b || (a == b && !(__float_as_uint(a) >> 31))) ? a : b; }
// box_within's expression on one axis
__device__ __forceinline__ bool within_f(float c, float r) { return fabsf(c) + fabsf(r) <= 1099511627776.0f; }

// 1. One thread per BVH slot: the triangle through tri_orig, its extent [p - r, p + r] into ext (6 floats per slot),
// and the refusal flag: a non-finite vertex or a triangle box outside box_within's 2^40.  Writes no scene table.
__global__ void __launch_bounds__(256) k_refit_extents(uint32_t tri_count, const float* __restrict__ tris_in,
                                                       const uint32_t* __restrict__ tri_orig, float* __restrict__ ext,
                                                       uint32_t* __restrict__ res) {
    const uint32_t slot = blockIdx.x*256u + threadIdx.x;
    if (slot >= tri_count) return;
    const float* v = tris_in + 9*(size_t)tri_orig[slot];
    bool ok = true;
    float lo3[3], hi3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = v[k], b = v[3 + k], c = v[6 + k];
        const float lo = tmin(a, tmin(b, c)), hi = tmax(a, tmax(b, c));
        const float p = 0.5f*(lo + hi), r = 0.5f*(hi - lo);
        ok = ok && finite_f(a) && finite_f(b) && finite_f(c) && within_f(p, r);
        lo3[k] = p - r;
        hi3[k] = p + r;
    }
    float* e = ext + 6*(size_t)slot;
    e[0] = lo3[0]; e[1] = lo3[1]; e[2] = lo3[2]; e[3] = hi3[0]; e[4] = hi3[1]; e[5] = hi3[2];
    if (!ok) res[RES_REFUSED] = 1u;
}

// 2. One thread per BVH slot, after the flag has passed: the triangle record (a, b - a, c - a, 0) and the normals
// gathered into slot order (normals_in null: the stored ones stay).
__global__ void __launch_bounds__(256) k_refit_write(uint32_t tri_count, const float* __restrict__ tris_in,
                                                     const float* __restrict__ normals_in, const uint32_t* __restrict__ tri_orig,
                                                     float4* __restrict__ tris, float* __restrict__ normals) {
    const uint32_t slot = blockIdx.x*256u + threadIdx.x;
    if (slot >= tri_count) return;
    const size_t o = tri_orig[slot];
    const float* v = tris_in + 9*o;
    const float ax = v[0], ay = v[1], az = v[2];
    tris[3*(size_t)slot] = make_float4(ax, ay, az, 0.0f);
    tris[3*(size_t)slot + 1] = make_float4(v[3] - ax, v[4] - ay, v[5] - az, 0.0f);
    tris[3*(size_t)slot + 2] = make_float4(v[6] - ax, v[7] - ay, v[8] - az, 0.0f);
    if (normals_in) {
        const float* n = normals_in + 9*o;
        float* d = normals + 9*(size_t)slot;
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = n[k];
    }
}

// One node of a subtree: x = the BVH2 node (mesh-local), w = its kind (| K_ROOT_BIT for the subtree's root); a leaf's
// y, z = its first slot and count; an interior node's y, z = its children, by local index or EXTERNAL | node.
typedef uint4 Entry;
// One subtree: x = its first entry, y = its first level offset (levels[y .. y + z] are entry offsets from x, z levels).
typedef uint4 Subtree;

// 3. One workgroup per subtree of one round of the plan.  The subtree's (MIN, MAX) pairs live in LDS by local index;
// its entries are sorted by level, a level's entries read only lower levels' pairs (LDS), leaves' extents and earlier
// rounds' subtree roots (HBM, written before this launch).  Every node with a triangle below it gets bv_p and bv_r
// from its own pair, in both node tables; the subtree's root leaves its pair in HBM for a later round.
__global__ void __launch_bounds__(SUB_THREADS) k_refit_subtrees(const Entry* __restrict__ entries, const Subtree* __restrict__ subs,
                                                                const uint32_t* __restrict__ levels, uint32_t first_sub,
                                                                const float* __restrict__ ext, float* __restrict__ pairs,
                                                                rt_bvh_node* __restrict__ nodes_src, rt_bvh_node* __restrict__ nodes,
                                                                uint32_t* __restrict__ res) {
    __shared__ float lds[6*SUB_CAP];
    const Subtree sub = subs[first_sub + blockIdx.x];
    const float inf = __uint_as_float(0x7F800000u);
    for (uint32_t lv = 0; lv < sub.z; ++lv) {
        const uint32_t begin = levels[sub.y + lv], end = levels[sub.y + lv + 1];
        for (uint32_t e = begin + threadIdx.x; e < end; e += SUB_THREADS) {
            const Entry en = entries[sub.x + e];
            const uint32_t kind = en.w & 3u;
            float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
            if (kind == K_LEAF) {
                for (uint32_t t = en.y; t < en.y + en.z; ++t) {
                    const float* x = ext + 6*(size_t)t;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { lo[k] = tmin(lo[k], x[k]); hi[k] = tmax(hi[k], x[3 + k]); }
                }
            } else if (kind == K_INTERIOR) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const uint32_t c = g ? en.z : en.y;
                    float cl[3], ch[3];
                    if (c & EXTERNAL) {
                        const float* x = pairs + 6*(size_t)(c & ~EXTERNAL);
#pragma unroll
                        for (int k = 0; k < 3; ++k) { cl[k] = x[k]; ch[k] = x[3 + k]; }
                    } else {
#pragma unroll
                        for (int k = 0; k < 3; ++k) { cl[k] = lds[k*SUB_CAP + c]; ch[k] = lds[(3 + k)*SUB_CAP + c]; }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) { lo[k] = tmin(lo[k], cl[k]); hi[k] = tmax(hi[k], ch[k]); }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { lds[k*SUB_CAP + e] = lo[k]; lds[(3 + k)*SUB_CAP + e] = hi[k]; }
            if (en.w & K_ROOT_BIT) {
                float* x = pairs + 6*(size_t)en.x;
#pragma unroll
                for (int k = 0; k < 3; ++k) { x[k] = lo[k]; x[3 + k] = hi[k]; }
            }
            if (lo[0] <= hi[0]) {                   // a triangle below it: every other node keeps its bytes
                float p[3], r[3];
                bool in = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    p[k] = 0.5f*(lo[k] + hi[k]);
                    r[k] = 0.5f*(hi[k] - lo[k]);
                    in = in && within_f(p[k], r[k]);
                }
                float* a = &nodes_src[en.x].bv_p.x;
                float* b = &nodes[en.x].bv_p.x;
#pragma unroll
                for (int k = 0; k < 3; ++k) { a[k] = p[k]; a[3 + k] = r[k]; b[k] = p[k]; b[3 + k] = r[k]; }
                if (!in) res[RES_OUTSIDE] = 1u;
                if (en.x == 0u) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) { res[RES_BOX + k] = __float_as_uint(p[k]); res[RES_BOX + 3 + k] = __float_as_uint(r[k]); }
                    res[RES_HAS_BOX] = 1u;
                }
            }
        }
        __syncthreads();
    }
}

// 4. One thread per BVH4 node and child slot: rows 0..5 of the node (its children's boxes) from the refitted BVH2,
// and, by slot 0's thread, the node's mid4 entry: the boxes of its BVH2 node's two children.
__global__ void __launch_bounds__(256) k_refit_bvh4(uint32_t n4, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ mid_left,
                                                    const rt_bvh_node* __restrict__ nodes_src, float* __restrict__ nodes4,
                                                    float* __restrict__ mid4) {
    const uint32_t i = blockIdx.x*256u + threadIdx.x;
    if (i >= 4u*n4) return;
    const uint32_t k = i >> 2, j = i & 3u;
    const uint32_t m = slots[i];
    if (m != NONE) {
        const float* c = &nodes_src[m].bv_p.x;
        float* q = nodes4 + 32*(size_t)k + j;
#pragma unroll
        for (int a = 0; a < 6; ++a) q[4*a] = c[a];
    }
    const uint32_t l = mid_left[k];
    if (j == 0u && l != NONE) {
        const float* L = &nodes_src[l].bv_p.x;
        const float* R = &nodes_src[l + 1].bv_p.x;
        float* q = mid4 + 12*(size_t)k;
#pragma unroll
        for (int a = 0; a < 6; ++a) { q[a] = L[a]; q[6 + a] = R[a]; }
    }
}

// ---------------------------------------------------------------- the plan, built on a mesh's first update
struct MeshPlan {
    bool built = false;
    std::vector<void*> allocs;
    Entry* d_entries = nullptr;
    Subtree* d_subs = nullptr;
    uint32_t* d_levels = nullptr;
    uint32_t* d_slots = nullptr;            // BVH4: 4 BVH2 nodes per node
    uint32_t* d_mid_left = nullptr;         // BVH4: the source node's left child, or NONE
    float* d_ext = nullptr;                 // scratch: 6 floats per slot
    float* d_pairs = nullptr;               // scratch: 6 floats per node (subtree roots only)
    std::vector<std::pair<uint32_t, uint32_t>> rounds;   // (first subtree, subtrees): one launch each
    std::vector<uint32_t> src4;             // BVH4 node -> BVH2 node (the read-back's table 6)
    uint32_t counts[8] = {};                // table 7
    bool kept_within = true;                // box_within over the nodes a refit never writes
};
struct RefitState {
    std::vector<MeshPlan> plans;
    uint32_t* d_res = nullptr;
};

void free_state(void* p) {
    RefitState* st = static_cast<RefitState*>(p);
    for (MeshPlan& mp : st->plans)
        for (void* a : mp.allocs) (void)hipFree(a);
    if (st->d_res) (void)hipFree(st->d_res);
    delete st;
}

bool host_within(const rt_bvh_node& n) {
    const float c[3] = {n.bv_p.x, n.bv_p.y, n.bv_p.z}, r[3] = {n.bv_r.x, n.bv_r.y, n.bv_r.z};
    for (int k = 0; k < 3; ++k)
        if (!(fabsf(c[k]) + fabsf(r[k]) <= 1099511627776.0f)) return false;
    return true;
}

template <typename T>
int to_device(MeshPlan& mp, const std::vector<T>& host, T** out) {
    *out = nullptr;
    if (host.empty()) return RT_OK;
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T)*host.size()) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, "rt_scene_update_mesh: hipMalloc (the refit plan)");
    mp.allocs.push_back(p);
    RF_HIP(hipMemcpy(p, host.data(), sizeof(T)*host.size(), hipMemcpyHostToDevice));
    *out = static_cast<T*>(p);
    return RT_OK;
}

// The plan of one mesh from a read-back of its nodes: the tree below node 0 cut into subtrees of at most SUB_CAP nodes,
// in rounds.  A round takes every highest node with at most SUB_CAP unfinished nodes below and including it; what is
// left above is cut the same way in the next round, until node 0 is finished.  A subtree's children outside it are
// roots of earlier rounds' subtrees.
int build_plan(const std::string& e, const RtMeshSlices& ms, MeshPlan& mp) {
    const uint32_t n = ms.node_count;
    std::vector<rt_bvh_node> nodes(n);
    if (n) RF_HIP(hipMemcpy(nodes.data(), ms.nodes_src, sizeof(rt_bvh_node)*(size_t)n, hipMemcpyDeviceToHost));
    auto interior = [&](uint32_t i) { return nodes[i].count == 0 && nodes[i].left_first != 0 && (uint64_t)nodes[i].left_first + 1 < n; };
    std::vector<uint32_t> pre, parent(n, NONE);
    std::vector<uint8_t> seen(n, 0), done(n, 0);
    if (n) {
        std::vector<uint32_t> stack{0u};
        while (!stack.empty()) {
            const uint32_t i = stack.back(); stack.pop_back();
            if (seen[i]) return fail(RT_ERROR_INVALID, e + ": the mesh BVH is not a tree (node " + std::to_string(i) + " has two parents)");
            seen[i] = 1;
            pre.push_back(i);
            if (interior(i))
                for (uint32_t g = 2; g-- > 0;) { parent[nodes[i].left_first + g] = i; stack.push_back(nodes[i].left_first + g); }
        }
    }
    for (uint32_t i = 0; i < n; ++i)
        if (!seen[i] || (!nodes[i].count && !interior(i))) mp.kept_within = mp.kept_within && host_within(nodes[i]);
    std::vector<Entry> entries;
    std::vector<Subtree> subs;
    std::vector<uint32_t> levels;
    std::vector<uint32_t> rsize(n, 0), local(n, 0), level(n, 0), members;
    uint32_t max_nodes = 0, max_levels = 0;
    while (n && !done[0]) {
        for (size_t q = pre.size(); q-- > 0;) {
            const uint32_t i = pre[q];
            rsize[i] = done[i] ? 0u : 1u + (interior(i) ? rsize[nodes[i].left_first] + rsize[nodes[i].left_first + 1] : 0u);
        }
        const uint32_t first_sub = (uint32_t)subs.size();
        for (uint32_t root : pre) {
            if (done[root] || rsize[root] > SUB_CAP || (root != 0u && rsize[parent[root]] <= SUB_CAP)) continue;
            // the unfinished nodes below and including `root`, parents before children
            members.clear();
            std::vector<uint32_t> stack{root};
            while (!stack.empty()) {
                const uint32_t i = stack.back(); stack.pop_back();
                members.push_back(i);
                if (interior(i))
                    for (uint32_t g = 2; g-- > 0;)
                        if (!done[nodes[i].left_first + g]) stack.push_back(nodes[i].left_first + g);
            }
            uint32_t nlev = 0;
            for (size_t q = members.size(); q-- > 0;) {
                const uint32_t i = members[q];
                uint32_t lv = 0;
                if (interior(i))
                    for (uint32_t g = 0; g < 2; ++g) {
                        const uint32_t c = nodes[i].left_first + g;
                        if (!done[c]) lv = std::max(lv, level[c] + 1u);
                    }
                level[i] = lv;
                nlev = std::max(nlev, lv + 1u);
            }
            std::stable_sort(members.begin(), members.end(), [&](uint32_t a, uint32_t b) { return level[a] < level[b]; });
            for (uint32_t q = 0; q < members.size(); ++q) local[members[q]] = q;
            Subtree sb;
            sb.x = (uint32_t)entries.size(); sb.y = (uint32_t)levels.size(); sb.z = nlev; sb.w = (uint32_t)members.size();
            uint32_t at = 0;
            for (uint32_t q = 0; q < members.size(); ++q) {
                const uint32_t i = members[q];
                while (at <= level[i]) { levels.push_back(q); ++at; }
                Entry en;
                en.x = i;
                if (nodes[i].count) { en.y = nodes[i].left_first; en.z = nodes[i].count; en.w = K_LEAF; }
                else if (interior(i)) {
                    const uint32_t l = nodes[i].left_first;
                    en.y = done[l] ? (EXTERNAL | l) : local[l];
                    en.z = done[l + 1] ? (EXTERNAL | (l + 1)) : local[l + 1];
                    en.w = K_INTERIOR;
                } else { en.y = en.z = 0u; en.w = K_EMPTY; }
                if (i == root) en.w |= K_ROOT_BIT;
                entries.push_back(en);
            }
            levels.push_back((uint32_t)members.size());
            subs.push_back(sb);
            max_nodes = std::max(max_nodes, (uint32_t)members.size());
            max_levels = std::max(max_levels, nlev);
            for (uint32_t i : members) done[i] = 2;         // finished once the round is planned
        }
        for (uint32_t i : pre) if (done[i] == 2) done[i] = 1;
        mp.rounds.push_back({first_sub, (uint32_t)subs.size() - first_sub});
        if (subs.size() == first_sub) return fail(RT_ERROR_INVALID, e + ": internal: the refit plan made no progress");
    }
    // the BVH4 as the upload built it
    std::vector<uint32_t> slots, mid_left;
    rt_internal_mesh_bvh4_plan(nodes.data(), n, mp.src4, slots);
    if (mp.src4.size() != ms.n4_count) return fail(RT_ERROR_INVALID, e + ": internal: the BVH4 plan differs from the upload's");
    mid_left.resize(mp.src4.size());
    for (size_t k = 0; k < mp.src4.size(); ++k) mid_left[k] = interior(mp.src4[k]) ? nodes[mp.src4[k]].left_first : NONE;
    for (uint32_t m : slots)
        if (m != NONE && m >= n) return fail(RT_ERROR_INVALID, e + ": internal: a BVH4 slot names no node");
    int err;
    if ((err = to_device(mp, entries, &mp.d_entries)) || (err = to_device(mp, subs, &mp.d_subs)) ||
        (err = to_device(mp, levels, &mp.d_levels)) || (err = to_device(mp, slots, &mp.d_slots)) ||
        (err = to_device(mp, mid_left, &mp.d_mid_left)))
        return err;
    if ((err = to_device(mp, std::vector<float>(6*(size_t)ms.tri_count, 0.0f), &mp.d_ext)) ||
        (err = to_device(mp, std::vector<float>(6*(size_t)n, 0.0f), &mp.d_pairs)))
        return err;
    mp.counts[0] = (uint32_t)mp.rounds.size();
    mp.counts[1] = (uint32_t)subs.size();
    mp.counts[2] = mp.rounds.empty() ? 0u : mp.rounds[0].second;
    mp.counts[3] = (uint32_t)pre.size();
    mp.counts[4] = max_nodes;
    mp.counts[5] = max_levels;
    mp.counts[6] = (uint32_t)mp.src4.size();
    mp.counts[7] = (ms.tri_count ? 2u : 0u) + (uint32_t)mp.rounds.size() + (mp.src4.empty() ? 0u : 1u);
    mp.built = true;
    return RT_OK;
}

// the scene's state and the mesh's plan, built when missing; a failure leaves no half-built plan behind
int plan_of(const std::string& e, rt_scene* s, uint32_t mesh, const RtMeshSlices& ms, RefitState** out_state, MeshPlan** out) {
    void** slot = rt_internal_scene_refit_state(s, free_state);
    if (!*slot) {
        RefitState* st = new RefitState();
        st->plans.resize(rt_internal_scene_mesh_count(s));
        if (hipMalloc(&st->d_res, 4*RES_WORDS) != hipSuccess) { delete st; return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc"); }
        *slot = st;
    }
    RefitState* st = static_cast<RefitState*>(*slot);
    MeshPlan& mp = st->plans[mesh];
    if (!mp.built) {
        const int err = build_plan(e, ms, mp);
        if (err) {
            for (void* a : mp.allocs) (void)hipFree(a);
            mp = MeshPlan();
            return err;
        }
    }
    *out_state = st;
    *out = &mp;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_update_mesh_device(rt_scene* s, uint32_t mesh_index, const float* d_triangles, const float* d_normals,
                                rt_bvh_node* out_root) {
    const std::string e = "rt_scene_update_mesh_device";
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    if (mesh_index >= rt_internal_scene_mesh_count(s))
        return fail(RT_ERROR_INVALID, e + ": mesh_index " + std::to_string(mesh_index) + " is out of range (the scene has " +
                    std::to_string(rt_internal_scene_mesh_count(s)) + " meshes)");
    RtMeshSlices ms;
    rt_internal_scene_mesh(s, mesh_index, &ms);
    if (ms.tri_count && !d_triangles) return fail(RT_ERROR_INVALID, e + ": null d_triangles for a mesh with triangles");
    if (d_normals && !ms.has_normals)
        return fail(RT_ERROR_INVALID, e + ": d_normals for mesh " + std::to_string(mesh_index) + ", which was uploaded without normals");
    int err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    // no frame of the scene may still read a table that changes
    RF_HIP(hipDeviceSynchronize());
    RefitState* st = nullptr;
    MeshPlan* mp = nullptr;
    if ((err = plan_of(e, s, mesh_index, ms, &st, &mp))) return err;
    uint32_t res[RES_WORDS] = {};
    RF_HIP(hipMemsetAsync(st->d_res, 0, sizeof(res), nullptr));
    const uint32_t tri_blocks = (ms.tri_count + 255u) / 256u;
    if (ms.tri_count) {
        k_refit_extents<<<tri_blocks, 256, 0, nullptr>>>(ms.tri_count, d_triangles, ms.tri_orig, mp->d_ext, st->d_res);
        RF_HIP(hipGetLastError());
        // the flag, in one small copy: nothing of the scene is written before it has passed
        RF_HIP(hipMemcpy(res, st->d_res, 4, hipMemcpyDeviceToHost));
        if (res[RES_REFUSED])
            return fail(RT_ERROR_INVALID, e + ": mesh " + std::to_string(mesh_index) +
                        ": a vertex is not finite or a triangle's box is not within 2^40 of the origin");
        k_refit_write<<<tri_blocks, 256, 0, nullptr>>>(ms.tri_count, d_triangles, d_normals, ms.tri_orig,
                                                       reinterpret_cast<float4*>(ms.tris), ms.normals);
        RF_HIP(hipGetLastError());
    }
    for (const auto& r : mp->rounds) {
        k_refit_subtrees<<<r.second, SUB_THREADS, 0, nullptr>>>(mp->d_entries, mp->d_subs, mp->d_levels, r.first, mp->d_ext,
                                                                mp->d_pairs, ms.nodes_src, ms.nodes, st->d_res);
        RF_HIP(hipGetLastError());
    }
    if (ms.n4_count) {
        k_refit_bvh4<<<(4u*ms.n4_count + 255u) / 256u, 256, 0, nullptr>>>(ms.n4_count, mp->d_slots, mp->d_mid_left, ms.nodes_src,
                                                                           ms.nodes4, ms.mid4);
        RF_HIP(hipGetLastError());
    }
    RF_HIP(hipMemcpy(res, st->d_res, sizeof(res), hipMemcpyDeviceToHost));
    float box[6];
    memcpy(box, res + RES_BOX, sizeof(box));
    return rt_internal_scene_mesh_refitted(s, mesh_index, res[RES_HAS_BOX] ? box : nullptr, mp->kept_within && !res[RES_OUTSIDE],
                                           out_root);
}

int rt_scene_update_mesh(rt_scene* s, uint32_t mesh_index, const float* triangles, const float* normals, rt_bvh_node* out_root) {
    const std::string e = "rt_scene_update_mesh";
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    if (mesh_index >= rt_internal_scene_mesh_count(s))
        return fail(RT_ERROR_INVALID, e + ": mesh_index " + std::to_string(mesh_index) + " is out of range (the scene has " +
                    std::to_string(rt_internal_scene_mesh_count(s)) + " meshes)");
    RtMeshSlices ms;
    rt_internal_scene_mesh(s, mesh_index, &ms);
    if (ms.tri_count && !triangles) return fail(RT_ERROR_INVALID, e + ": null triangles for a mesh with triangles");
    if (normals && !ms.has_normals)
        return fail(RT_ERROR_INVALID, e + ": normals for mesh " + std::to_string(mesh_index) + ", which was uploaded without normals");
    int err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t bytes = 36*(size_t)ms.tri_count;
    float* d = nullptr;
    if (bytes && hipMalloc(&d, bytes*(normals ? 2 : 1)) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_n = normals && bytes ? d + 9*(size_t)ms.tri_count : nullptr;
    if (bytes && (hipMemcpy(d, triangles, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                  (d_n && hipMemcpy(d_n, normals, bytes, hipMemcpyHostToDevice) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) {
        err = rt_scene_update_mesh_device(s, mesh_index, d, d_n, out_root);
        if (err) {                                  // the same message under this entry's name
            std::string m = rt_last_error();
            const std::string inner = "rt_scene_update_mesh_device";
            if (m.compare(0, inner.size(), inner) == 0) m = e + m.substr(inner.size());
            rt_internal_set_error(m.c_str());
        }
    }
    if (d) (void)hipFree(d);
    return err;
}

int rt_debug_scene_mesh_table(const rt_scene* scene, uint32_t mesh_index, int which, void* out, size_t cap, size_t* out_bytes) {
    const std::string e = "rt_debug_scene_mesh_table";
    if (!scene) return fail(RT_ERROR_INVALID, e + ": null scene");
    if (!out_bytes) return fail(RT_ERROR_INVALID, e + ": null out_bytes");
    rt_scene* s = const_cast<rt_scene*>(scene);     // the plan tables may build the plan; no scene table changes
    if (mesh_index >= rt_internal_scene_mesh_count(s)) return fail(RT_ERROR_INVALID, e + ": mesh_index out of range");
    if (which < 0 || which >= RT_MESH_TABLE_COUNT) return fail(RT_ERROR_INVALID, e + ": no such table");
    RtMeshSlices ms;
    rt_internal_scene_mesh(s, mesh_index, &ms);
    int err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const void* from = nullptr;
    const void* host = nullptr;
    size_t bytes = 0;
    switch (which) {
        case RT_MESH_TABLE_TRIANGLES: from = ms.tris; bytes = 48*(size_t)ms.tri_count; break;
        case RT_MESH_TABLE_NORMALS: from = ms.normals; bytes = 36*(size_t)ms.tri_count; break;
        case RT_MESH_TABLE_NODES_SRC: from = ms.nodes_src; bytes = 32*(size_t)ms.node_count; break;
        case RT_MESH_TABLE_NODES: from = ms.nodes; bytes = 32*(size_t)ms.node_count; break;
        case RT_MESH_TABLE_NODES4: from = ms.nodes4; bytes = 128*(size_t)ms.n4_count; break;
        case RT_MESH_TABLE_MID4: from = ms.mid4; bytes = 48*(size_t)ms.n4_count; break;
        default: {
            RF_HIP(hipDeviceSynchronize());
            RefitState* st = nullptr;
            MeshPlan* mp = nullptr;
            if ((err = plan_of(e, s, mesh_index, ms, &st, &mp))) return err;
            if (which == RT_MESH_TABLE_BVH4_SOURCES) { host = mp->src4.data(); bytes = 4*mp->src4.size(); }
            else { host = mp->counts; bytes = sizeof(mp->counts); }
        }
    }
    *out_bytes = bytes;
    if (!out) return RT_OK;
    if (cap < bytes) return fail(RT_ERROR_INVALID, e + ": cap is below the table's size");
    if (!bytes) return RT_OK;
    if (host) { memcpy(out, host, bytes); return RT_OK; }
    RF_HIP(hipDeviceSynchronize());
    RF_HIP(hipMemcpy(out, from, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"
