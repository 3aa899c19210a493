// rt_temporal.hip — temporal accumulation: the stage that reprojects the previous frame's history through the
// primary-hit G-buffer and blends the current frame in (rt_temporal_accumulate_device, rt_temporal_accumulate) and
// the driver that runs one frame of the loop (rt_render_temporal_device, rt_render_temporal).  Beyond the
// reference, an opt-in: no other entry calls it.  The frames are rt_render_device's and the
// G-buffer rt_gbuffer_device's (rt_kernels.hip): nothing here touches a sample or a ray.
//
// The stage is defined operation by operation in DESIGN.md ("Temporal accumulation"); tests/ref_temporal/
// ref_temporal.c restates it in plain C and k_temporal_accumulate matches that checker bit for bit: IEEE f32, no
// contraction, division as /, correctly rounded sqrt, and the additions in the stated orders.  The kernel's text is
// rt_temporal_shared.h's one accumulate body with every flag off: no moments, no motion table, no deform table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_temporal_shared.h"   // the accumulate body and what the stage's entries and the drivers share on the host

namespace {

__global__ void __launch_bounds__(256) k_temporal_accumulate(const float4* __restrict__ current,
                                                             const rt_gbuffer_texel* __restrict__ gbuffer,
                                                             const float4* __restrict__ prev_history,
                                                             const float* __restrict__ prev_length,
                                                             const rt_gbuffer_texel* __restrict__ prev_gbuffer, TaCamera cam,
                                                             uint32_t w, uint32_t h, rt_temporal_params p,
                                                             float4* __restrict__ history, float* __restrict__ length) {
    temporal_accumulate_body<false, false, false, false>(current, gbuffer, prev_history, prev_length, prev_gbuffer, nullptr, cam, w, h, p,
                                                  nullptr, 0u, nullptr, nullptr, 0u, history, length, nullptr, nullptr, TaClip{});
}

}  // namespace

extern "C" {

int rt_temporal_default_params(rt_temporal_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_temporal_default_params: null out");
    *out = {};
    out->max_history = 32.0f;
    out->normal_cos = 0.9f;
    out->plane_tolerance = 0.02f;
    out->snap = 1.0f / 32.0f;
    out->firefly_clamp = 10.0f;
    return RT_OK;
}

size_t rt_temporal_workspace_bytes(uint32_t w, uint32_t h) {
    return (size_t)w*h*(16 + 2*(32 + 16 + 4));
}

int rt_temporal_accumulate_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                  const float* d_prev_history, const float* d_prev_length,
                                  const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                  float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                  float* d_history, float* d_length, void* hip_stream) {
    const std::string e = "rt_temporal_accumulate_device";
    const TaArgs a = {d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera, prev_lens_distortion,
                      w, h, p, d_history, d_length};
    int err = check_accumulate(e, "d_", a);
    if (err) return err;
    return launch_accumulate(e, device, k_temporal_accumulate, w, h, hip_stream, f4(d_current), d_gbuffer, f4(d_prev_history),
                             d_prev_length, d_prev_gbuffer, ta_camera(a), w, h, *p, f4(d_history), d_length);
}

int rt_temporal_accumulate(int device, const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                           const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                           float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p, float* history,
                           float* length) {
    const std::string e = "rt_temporal_accumulate";
    int err = check_accumulate(e, "", {current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, prev_lens_distortion,
                                       w, h, p, history, length});
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    // the driver's layout: current, then the new set [0] and the previous set [1]
    const size_t n = (size_t)w*h;
    void* d_all = nullptr;
    if (hipMalloc(&d_all, rt_temporal_workspace_bytes(w, h)) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    const TaWorkspace ws = carve_temporal(d_all, n);
    const bool prev = prev_history != nullptr;
    if (hipMemcpy(ws.current, current, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ws.gbuffer[0], gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
        (prev && (hipMemcpy(ws.history[1], prev_history, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(ws.length[1], prev_length, 4*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(ws.gbuffer[1], prev_gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_temporal_accumulate_device(device, ws.current, ws.gbuffer[0], prev ? ws.history[1] : nullptr,
                                                  prev ? ws.length[1] : nullptr, prev ? ws.gbuffer[1] : nullptr, prev_camera,
                                                  prev_lens_distortion, w, h, p, ws.history[0], ws.length[0], nullptr);
    if (!err && (hipMemcpy(history, ws.history[0], 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(length, ws.length[0], 4*n, hipMemcpyDeviceToHost) != hipSuccess))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d_all);
    return err;
}

int rt_render_temporal_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                              const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                              uint32_t frame_count, const rt_temporal_params* p, rt_temporal_state* state, float* d_out,
                              float* d_length_out, void* hip_stream, rt_stats* stats) {
    const std::string e = "rt_render_temporal_device";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, d_out, "d_out");
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    const TaWorkspace ws = carve_temporal(state->d_workspace, n);
    const uint32_t cur = state->parity, old = state->parity ^ 1u;
    // a state of another frame size restarts
    const bool prev = state->frames != 0u && state->w == w && state->h == h;

    rt_stats fs;
    err = render_current(e, s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    err = rt_gbuffer_device(s, camera, st->lens_distortion, w, h, ws.gbuffer[cur], hip_stream);
    if (err) return err;
    err = rt_temporal_accumulate_device(device, ws.current, ws.gbuffer[cur], prev ? ws.history[old] : nullptr,
                                        prev ? ws.length[old] : nullptr, prev ? ws.gbuffer[old] : nullptr, &state->camera,
                                        state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream);
    if (err) return err;
    err = copy_out_history(e, ws, cur, n, d_out, d_length_out, hip_stream);
    if (err) return err;
    advance_state(state, w, h, camera, st);
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_render_temporal(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                       const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                       const rt_temporal_params* p, rt_temporal_state* state, float* out_pixels, float* out_length,
                       rt_stats* stats) {
    const std::string e = "rt_render_temporal";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, out_pixels, "out_pixels");
    if (err) return err;
    return render_to_host(e, s, w, h, out_pixels, out_length, [&](float* d_out, float* d_length_out) {
        return rt_render_temporal_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, state, d_out,
                                         d_length_out, nullptr, stats);
    });
}

}  // extern "C"
