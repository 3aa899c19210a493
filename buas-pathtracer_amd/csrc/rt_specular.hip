// rt_specular.hip — the temporal loop over the specular G-buffer: the driver that runs one frame of it on the public
// entries (rt_render_temporal_specular_device, rt_render_temporal_specular).  Beyond the reference, an
// opt-in: no other entry calls it.  The G-buffer is rt_gbuffer_specular_device's (k_gbuffer_specular, rt_kernels.hip),
// the accumulate stage rt_temporal_accumulate_device's or, with clip parameters, rt_temporal_accumulate_clip_device's
// after rt_temporal_neighbourhood_device: no kernel lives here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_temporal_shared.h"   // what the drivers share on the host

namespace {

// the workspace: rt_render_temporal_device's 120 bytes a pixel, then the neighbourhood texels on a 16-byte boundary
size_t texels_offset(size_t n) { return (120*n + 15) & ~(size_t)15; }

int check_specular_driver(const std::string& e, const rt_scene* s, const rt_camera* camera, const rt_settings* st,
                          const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t w, uint32_t h,
                          const rt_temporal_params* p, const rt_temporal_state* state, const rt_gbuffer_specular_params* sp,
                          const rt_temporal_clip_params* cp, const void* out, const char* out_name) {
    int err = rt_internal_check_specular_params(e.c_str(), sp);
    if (err) return err;
    if (cp) {
        err = check_clip_params(e, cp);
        if (err) return err;
    }
    err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, out, out_name);
    if (err) return err;
    if ((uint64_t)w*h >= ((uint64_t)1 << 32)) return fail(RT_ERROR_INVALID, e + ": w*h must be below 2^32");
    return RT_OK;
}

}  // namespace

extern "C" {

size_t rt_temporal_specular_workspace_bytes(uint32_t w, uint32_t h) {
    const size_t n = (size_t)w*h;
    return texels_offset(n) + sizeof(rt_neighbourhood_texel)*n;
}

int rt_render_temporal_specular_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                       const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                                       uint32_t frame_count, const rt_temporal_params* p, rt_temporal_state* state,
                                       const rt_gbuffer_specular_params* sp, const rt_temporal_clip_params* cp, float* d_out,
                                       float* d_length_out, void* hip_stream, rt_stats* stats) {
    const std::string e = "rt_render_temporal_specular_device";
    int err = check_specular_driver(e, s, camera, st, filter, tiles, w, h, p, state, sp, cp, d_out, "d_out");
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    const TaWorkspace ws = carve_temporal(state->d_workspace, n);
    rt_neighbourhood_texel* texels =
        reinterpret_cast<rt_neighbourhood_texel*>(static_cast<char*>(state->d_workspace) + texels_offset(n));
    const uint32_t cur = state->parity, old = state->parity ^ 1u;
    // a state of another frame size restarts
    const bool prev = state->frames != 0u && state->w == w && state->h == h;

    rt_stats fs;
    err = render_current(e, s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    err = rt_gbuffer_specular_device(s, camera, st->lens_distortion, w, h, sp, ws.gbuffer[cur], nullptr, hip_stream);
    if (err) return err;
    const float* ph = prev ? ws.history[old] : nullptr;
    const float* pl = prev ? ws.length[old] : nullptr;
    const rt_gbuffer_texel* pg = prev ? ws.gbuffer[old] : nullptr;
    if (cp) {
        err = rt_temporal_neighbourhood_device(device, ws.current, w, h, cp->radius, p->firefly_clamp, texels, hip_stream);
        if (err) return err;
        err = rt_temporal_accumulate_clip_device(device, ws.current, ws.gbuffer[cur], ph, pl, pg, &state->camera,
                                                 state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream,
                                                 nullptr, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, texels, cp->gamma,
                                                 cp->min_count, nullptr);
    } else {
        err = rt_temporal_accumulate_device(device, ws.current, ws.gbuffer[cur], ph, pl, pg, &state->camera,
                                            state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream);
    }
    if (err) return err;
    err = copy_out_history(e, ws, cur, n, d_out, d_length_out, hip_stream);
    if (err) return err;
    advance_state(state, w, h, camera, st);
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_render_temporal_specular(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                const rt_temporal_params* p, rt_temporal_state* state, const rt_gbuffer_specular_params* sp,
                                const rt_temporal_clip_params* cp, float* out_pixels, float* out_length, rt_stats* stats) {
    const std::string e = "rt_render_temporal_specular";
    int err = check_specular_driver(e, s, camera, st, filter, tiles, w, h, p, state, sp, cp, out_pixels, "out_pixels");
    if (err) return err;
    return render_to_host(e, s, w, h, out_pixels, out_length, [&](float* d_out, float* d_length_out) {
        return rt_render_temporal_specular_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, state, sp,
                                                  cp, d_out, d_length_out, nullptr, stats);
    });
}

}  // extern "C"
