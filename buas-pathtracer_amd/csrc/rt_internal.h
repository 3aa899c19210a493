// Host helpers that rt_kernels.hip exports to the library's other translation units.
// Not part of the C ABI (include/rt_abi.h): C++ linkage, no header outside csrc/ names them.
#ifndef RT_INTERNAL_H
#define RT_INTERNAL_H

#include "rt_abi.h"

void rt_internal_set_error(const char* message);        // the thread's rt_last_error() message
int  rt_internal_bind_device(int device);               // hipSetDevice with the ABI's checks: an rt_status
int  rt_internal_scene_device(const rt_scene* scene);   // the device rt_scene_upload put the scene on
int  rt_internal_scene_cancelled(const rt_scene* scene); // rt_cancel's flag: set until the next frame's loop starts
// rt_gbuffer_specular_device's refusals of its parameters, named after `entry` (the G-buffer's entries and the driver
// over them, rt_specular.hip): an rt_status
int  rt_internal_check_specular_params(const char* entry, const rt_gbuffer_specular_params* params);

// What rt_refit.hip (rt_scene_update_mesh and its kin) needs of a scene.
#include <stdint.h>
#include <vector>
// One mesh's slices of the scene's concatenated mesh tables: device pointers at the mesh's own offsets, null where
// the mesh has nothing of the kind.
struct RtMeshSlices {
    uint32_t tri_count, node_count, n4_first, n4_count, has_normals;
    float* tris;                    // 12 floats per slot: (a, 0), (b - a, 0), (c - a, 0)
    const uint32_t* tri_orig;       // slot -> original triangle
    float* normals;                 // 9 floats per slot
    rt_bvh_node* nodes_src;         // the caller's layout
    rt_bvh_node* nodes;             // the traversal layout: the same boxes, a packed record behind them
    float* nodes4;                  // 32 floats per BVH4 node, rows 0..5 the child boxes
    float* mid4;                    // 12 floats per BVH4 node
};
uint32_t rt_internal_scene_mesh_count(const rt_scene* scene);
void rt_internal_scene_mesh(rt_scene* scene, uint32_t mesh, RtMeshSlices* out);   // mesh < the scene's mesh count
// rt_scene_upload's BVH4 of a mesh BVH2, as a plan: per BVH4 node (in the upload's order, mesh-local) the BVH2 node it
// was made from and its four child slots' BVH2 nodes (0xFFFFFFFF: none).  Empty when the root is a leaf.
void rt_internal_mesh_bvh4_plan(const rt_bvh_node* nodes, uint32_t count, std::vector<uint32_t>& src, std::vector<uint32_t>& slots);
// The scene's slot for rt_refit.hip's state; rt_scene_free hands a non-null state to free_state.
void** rt_internal_scene_refit_state(rt_scene* scene, void (*free_state)(void*));
// After a refit of `mesh`: node 0's new box (bv_p, bv_r: 6 floats; null when the refit wrote none), and whether every
// node box of the mesh is within 2^40 (box_within).  A box whose 24 bytes differ from the kept root's replaces them and
// marks the scene stale until rt_scene_update_instances.  out_root (optional) receives node 0.  An rt_status.
int rt_internal_scene_mesh_refitted(rt_scene* scene, uint32_t mesh, const float* box, bool within, rt_bvh_node* out_root);

#endif
