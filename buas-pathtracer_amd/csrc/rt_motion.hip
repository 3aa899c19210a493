// rt_motion.hip — a temporal history that follows moving instances: the table of per-primitive rigid motions
// (rt_motion_table), the accumulate stage that carries a hit point and its normal through that motion into the
// previous frame (rt_temporal_accumulate_motion_device, rt_temporal_accumulate_motion) and the driver that runs one
// frame of the loop on the public entries (rt_render_temporal_motion_device, rt_render_temporal_motion).  Beyond the
// reference, an opt-in: no other entry calls it.
//
// The stage is defined operation by operation in DESIGN.md ("Moving instances"); tests/ref_motion/ref_motion.c
// restates it in plain C and k_temporal_accumulate_motion matches that checker bit for bit: IEEE f32, no
// contraction, division as /, correctly rounded sqrt, d_expf for the moments, and the additions in the stated orders.
// The kernel's text is rt_temporal_shared.h's one accumulate body with the motion flag on, the moments flag as the
// entry's d_moments says, and no deform table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_temporal_shared.h"   // the accumulate body and what the stage's entries and the drivers share on the host

namespace {

static_assert(sizeof(rt_motion_entry) == 112, "rt_motion_entry is 112 bytes");

template <bool MOMENTS>
__global__ void __launch_bounds__(256) k_temporal_accumulate_motion(
        const float4* __restrict__ current, const rt_gbuffer_texel* __restrict__ gbuffer,
        const float4* __restrict__ prev_history, const float* __restrict__ prev_length,
        const rt_gbuffer_texel* __restrict__ prev_gbuffer, const float2* __restrict__ prev_moments, TaCamera cam,
        uint32_t w, uint32_t h, rt_temporal_params p, const rt_motion_entry* __restrict__ motion, uint32_t motion_count,
        float4* __restrict__ history, float* __restrict__ length, float2* __restrict__ moments,
        float2* __restrict__ velocity) {
    temporal_accumulate_body<MOMENTS, true, false, false>(current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_moments, cam, w, h, p,
                                                   motion, motion_count, nullptr, nullptr, 0u, history, length, moments, velocity, TaClip{});
}

// the driver's workspace: rt_render_temporal_device's 120 bytes per pixel, then the table on a 16-byte boundary
struct Workspace : TaWorkspace {
    rt_motion_entry* motion;
};
Workspace carve(void* d_workspace, size_t n) {
    return {carve_temporal(d_workspace, n),
            reinterpret_cast<rt_motion_entry*>(static_cast<char*>(d_workspace) + motion_table_offset(n))};
}

}  // namespace

extern "C" {

int rt_motion_table(uint32_t count, const rt_m4x4inv* cur, const rt_m4x4inv* prev, rt_motion_entry* out) {
    if (count && !cur) return fail(RT_ERROR_INVALID, "rt_motion_table: null cur");
    if (count && !prev) return fail(RT_ERROR_INVALID, "rt_motion_table: null prev");
    if (count && !out) return fail(RT_ERROR_INVALID, "rt_motion_table: null out");
    for (uint32_t i = 0; i < count; ++i) {
        rt_motion_entry& e = out[i];
        memcpy(e.inv_cur, cur[i].inverse.e, sizeof(e.inv_cur));         // rows 0..2
        memcpy(e.fwd_prev, prev[i].forward.e, sizeof(e.fwd_prev));
        e.moved = (memcmp(cur[i].forward.e, prev[i].forward.e, 48) != 0 || memcmp(cur[i].inverse.e, prev[i].inverse.e, 48) != 0) ? 1u : 0u;
        e.reserved[0] = e.reserved[1] = e.reserved[2] = 0u;
    }
    return RT_OK;
}

int rt_temporal_accumulate_motion_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                         const float* d_prev_history, const float* d_prev_length,
                                         const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                         float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                         float* d_history, float* d_length, void* hip_stream, const rt_motion_entry* d_motion,
                                         uint32_t motion_count, const float* d_prev_moments, float* d_moments,
                                         float* d_velocity) {
    const std::string e = "rt_temporal_accumulate_motion_device";
    const TaArgs a = {d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera, prev_lens_distortion,
                      w, h, p, d_history, d_length, d_motion, motion_count, d_prev_moments, d_moments, d_velocity};
    int err = check_motion(e, "d_", a);
    if (err) return err;
    return launch_accumulate(e, device, d_moments ? k_temporal_accumulate_motion<true> : k_temporal_accumulate_motion<false>, w, h,
                             hip_stream, f4(d_current), d_gbuffer, f4(d_prev_history), d_prev_length, d_prev_gbuffer,
                             f2(d_prev_moments), ta_camera(a), w, h, *p, d_motion, motion_count, f4(d_history), d_length,
                             f2(d_moments), f2(d_velocity));
}

int rt_temporal_accumulate_motion(int device, const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                  const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                                  float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p, float* history,
                                  float* length, const rt_motion_entry* motion, uint32_t motion_count, const float* prev_moments,
                                  float* moments, float* velocity) {
    const std::string e = "rt_temporal_accumulate_motion";
    const TaArgs a = {current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, prev_lens_distortion,
                      w, h, p, history, length, motion, motion_count, prev_moments, moments, velocity};
    int err = check_motion(e, "", a);
    if (err) return err;
    return stage_accumulate(e, device, a, false, [&](const TaArgs& d) {
        return rt_temporal_accumulate_motion_device(device, d.current, d.gbuffer, d.prev_history, d.prev_length, d.prev_gbuffer,
                                                    prev_camera, prev_lens_distortion, w, h, p, d.history, d.length, nullptr,
                                                    d.motion, motion_count, d.prev_moments, d.moments, d.velocity);
    });
}

size_t rt_temporal_motion_workspace_bytes(uint32_t w, uint32_t h, uint32_t primitive_count) {
    return motion_table_offset((size_t)w*h) + sizeof(rt_motion_entry)*(size_t)(primitive_count ? primitive_count : 1u);
}

int rt_render_temporal_motion_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                     const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                                     uint32_t frame_count, const rt_temporal_params* p, rt_temporal_motion_state* state,
                                     float* d_out, float* d_length_out, void* hip_stream, rt_stats* stats) {
    const std::string e = "rt_render_temporal_motion_device";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, d_out, "d_out");
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    const Workspace ws = carve(state->d_workspace, n);
    const uint32_t cur = state->parity, old = state->parity ^ 1u;
    uint32_t count = 0;
    err = rt_scene_primitive_transforms(s, 0, nullptr, &count);
    if (err) return err;
    // a state of another frame size or of another primitive count restarts
    const bool prev = state->frames != 0u && state->w == w && state->h == h && state->primitive_count == count;

    rt_stats fs;
    err = render_current(e, s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    err = rt_gbuffer_device(s, camera, st->lens_distortion, w, h, ws.gbuffer[cur], hip_stream);
    if (err) return err;
    std::vector<rt_m4x4inv> now(count);
    err = rt_scene_primitive_transforms(s, count, now.data(), &count);
    if (err) return err;
    if (prev && count) {
        std::vector<rt_motion_entry> table(count);
        err = rt_motion_table(count, now.data(), state->transforms, table.data());
        if (err) return err;
        // the stage of the frame before has synchronised its stream: nothing reads the table now
        if (hipMemcpy(ws.motion, table.data(), sizeof(rt_motion_entry)*(size_t)count, hipMemcpyHostToDevice) != hipSuccess)
            return fail(RT_ERROR_DEVICE, e + ": table upload");
    }
    err = rt_temporal_accumulate_motion_device(device, ws.current, ws.gbuffer[cur], prev ? ws.history[old] : nullptr,
                                               prev ? ws.length[old] : nullptr, prev ? ws.gbuffer[old] : nullptr, &state->camera,
                                               state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream,
                                               prev && count ? ws.motion : nullptr, prev ? count : 0u, nullptr, nullptr, nullptr);
    if (err) return err;
    err = copy_out_history(e, ws, cur, n, d_out, d_length_out, hip_stream);
    if (err) return err;
    state->primitive_count = count;
    if (count) memcpy(state->transforms, now.data(), sizeof(rt_m4x4inv)*(size_t)count);
    advance_state(state, w, h, camera, st);
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_render_temporal_motion(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                              const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                              const rt_temporal_params* p, rt_temporal_motion_state* state, float* out_pixels, float* out_length,
                              rt_stats* stats) {
    const std::string e = "rt_render_temporal_motion";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, out_pixels, "out_pixels");
    if (err) return err;
    return render_to_host(e, s, w, h, out_pixels, out_length, [&](float* d_out, float* d_length_out) {
        return rt_render_temporal_motion_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, state, d_out,
                                                d_length_out, nullptr, stats);
    });
}

}  // extern "C"
