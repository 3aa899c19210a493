// rt_temporal.hip — temporal accumulation: the stage that reprojects the previous frame's history through the
// primary-hit G-buffer and blends the current frame in (rt_temporal_accumulate_device, rt_temporal_accumulate) and
// the driver that runs one frame of the loop (rt_render_temporal_device, rt_render_temporal).  Beyond the
// reference, an opt-in: no other entry calls it.  The frames are rt_render_device's and the
// G-buffer rt_gbuffer_device's (rt_kernels.hip): nothing here touches a sample or a ray.
//
// The stage is defined operation by operation in DESIGN.md ("Temporal accumulation"); tests/ref_temporal/
// ref_temporal.c restates it in plain C and k_temporal_accumulate matches that checker bit for bit: IEEE f32, no
// contraction, division as /, correctly rounded sqrt, and the additions in the stated orders.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_temporal_shared.h"   // the projection, the tap rule and the stage's argument checks (rt_svgf.hip compiles them too)

namespace {

// One thread per pixel; a wave is 64 consecutive pixels of a row (64 x 4 blocks, as k_post): the current frame, the
// texel and both outputs are contiguous runs, and under a small camera motion the taps of a wave are too.  (An 8 x 8
// footprint per wave measured 7 to 11 % slower at 1920x1080: profiles/temporal_frame_cost.txt.)
__global__ void __launch_bounds__(256) k_temporal_accumulate(const float4* __restrict__ current,
                                                             const rt_gbuffer_texel* __restrict__ gbuffer,
                                                             const float4* __restrict__ prev_history,
                                                             const float* __restrict__ prev_length,
                                                             const rt_gbuffer_texel* __restrict__ prev_gbuffer, TaCamera cam,
                                                             uint32_t w, uint32_t h, rt_temporal_params p,
                                                             float4* __restrict__ history, float* __restrict__ length) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    // 1. validity: the denoise stage's rule
    const float4 s = current[i];
    bool valid = s.w > VALID_W;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (valid) {
        cr = s.x / s.w; cg = s.y / s.w; cb = s.z / s.w;
        valid = finite_f(cr) && finite_f(cg) && finite_f(cb);
    }
    if (!valid) {
        history[i] = s;
        length[i] = 0.0f;
        return;
    }
    // 2. clamp
    cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
    if (p.firefly_clamp > 0.0f) {
        cr = cr < p.firefly_clamp ? cr : p.firefly_clamp;
        cg = cg < p.firefly_clamp ? cg : p.firefly_clamp;
        cb = cb < p.firefly_clamp ? cb : p.firefly_clamp;
    }
    TapSum sum = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (prev_history) {
        // 3. the point and its place in the previous frame
        const rt_gbuffer_texel g = gbuffer[i];
        V3f P = v3_of(g.p);
        if (g.primitive == RT_HIT_MISS) P = {cam.p.x + g.p.x, cam.p.y + g.p.y, cam.p.z + g.p.z};
        float fx, fy;
        if (project_prev(cam, P, w, h, fx, fy)) {
            // 4. the taps
            const float plane_limit = p.plane_tolerance*g.t;
            const float rx = rintf(fx), ry = rintf(fy);
            if (fabsf(fx - rx) <= p.snap && fabsf(fy - ry) <= p.snap) {
                add_tap(sum, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
            } else {
                const float x0 = floorf(fx), y0 = floorf(fy);
                const float tx = fx - x0, ty = fy - y0;
                const int ix = (int)x0, iy = (int)y0;
                add_tap(sum, ix, iy, (1.0f - tx)*(1.0f - ty), w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
                add_tap(sum, ix + 1, iy, tx*(1.0f - ty), w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
                add_tap(sum, ix, iy + 1, (1.0f - tx)*ty, w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
                add_tap(sum, ix + 1, iy + 1, tx*ty, w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
            }
        }
    }
    // 5. the blend
    if (sum.W > 0.0f) {
        const float hr = sum.r / sum.W, hg = sum.g / sum.W, hb = sum.b / sum.W;
        const float L = sum.L / sum.W;
        float N = L + 1.0f;
        N = N < p.max_history ? N : p.max_history;
        const float a = 1.0f / N;
        // N = 1 (max_history = 1: a valid tap's length is >= 1) is the current frame itself, not hist + (c - hist)
        if (N == 1.0f) history[i] = make_float4(cr, cg, cb, 1.0f);
        else history[i] = make_float4(hr + (cr - hr)*a, hg + (cg - hg)*a, hb + (cb - hb)*a, 1.0f);
        length[i] = N;
    } else {
        history[i] = make_float4(cr, cg, cb, 1.0f);
        length[i] = 1.0f;
    }
}

// the driver's workspace: the current frame, then two sets of {G-buffer, history, length}
struct Workspace {
    float* current;
    rt_gbuffer_texel* gbuffer[2];
    float* history[2];
    float* length[2];
};
Workspace carve(void* d_workspace, size_t n) {
    char* base = static_cast<char*>(d_workspace);
    Workspace ws;
    ws.current = reinterpret_cast<float*>(base);
    for (int k = 0; k < 2; ++k) {
        ws.gbuffer[k] = reinterpret_cast<rt_gbuffer_texel*>(base + 16*n + (size_t)k*32*n);
        ws.history[k] = reinterpret_cast<float*>(base + 80*n + (size_t)k*16*n);
        ws.length[k] = reinterpret_cast<float*>(base + 112*n + (size_t)k*4*n);
    }
    return ws;
}

int check_driver(const std::string& e, const rt_scene* s, const rt_camera* camera, const rt_settings* st,
                 const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t w, uint32_t h, const rt_temporal_params* p,
                 const rt_temporal_state* state, const void* out, const char* out_name) {
    // the parameters first and the scene last: what needs no scene is refused without one
    int err = check_params(e, p);
    if (err) return err;
    if (!state) return fail(RT_ERROR_INVALID, e + ": null rt_temporal_state");
    if (!state->d_workspace) return fail(RT_ERROR_INVALID, e + ": rt_temporal_state: null d_workspace");
    if (state->parity > 1u) return fail(RT_ERROR_INVALID, e + ": rt_temporal_state: parity must be 0 or 1");
    if (!st) return fail(RT_ERROR_INVALID, e + ": null settings");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if (!camera) return fail(RT_ERROR_INVALID, e + ": null camera");
    if (!filter) return fail(RT_ERROR_INVALID, e + ": null filter");
    if (!tiles) return fail(RT_ERROR_INVALID, e + ": null tiles");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null " + out_name);
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    return RT_OK;
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
    int err = check_accumulate("rt_temporal_accumulate_device", "d_", d_current, d_gbuffer, d_prev_history, d_prev_length,
                               d_prev_gbuffer, prev_camera, w, h, p, d_history, d_length);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    TaCamera cam = {};
    if (d_prev_history) {
        cam.p = {prev_camera->p.x, prev_camera->p.y, prev_camera->p.z};
        cam.x = {prev_camera->x.x, prev_camera->x.y, prev_camera->x.z};
        cam.y = {prev_camera->y.x, prev_camera->y.y, prev_camera->y.z};
        cam.z = {prev_camera->z.x, prev_camera->z.y, prev_camera->z.z};
        cam.film_distance = prev_camera->film_distance;
        cam.half_film_w = prev_camera->half_film_w;
        cam.half_film_h = prev_camera->half_film_h;
        cam.lens_distortion = prev_lens_distortion;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    k_temporal_accumulate<<<grid, 256, 0, stream>>>(reinterpret_cast<const float4*>(d_current), d_gbuffer,
                                                    reinterpret_cast<const float4*>(d_prev_history), d_prev_length,
                                                    d_prev_gbuffer, cam, w, h, *p, reinterpret_cast<float4*>(d_history),
                                                    d_length);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, std::string("rt_temporal_accumulate_device: ") + hipGetErrorString(herr));
    return RT_OK;
}

int rt_temporal_accumulate(int device, const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                           const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                           float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p, float* history,
                           float* length) {
    const std::string e = "rt_temporal_accumulate";
    int err = check_accumulate(e, "", current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, w, h, p, history,
                               length);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    // the driver's layout: current, then the new set [0] and the previous set [1]
    const size_t n = (size_t)w*h;
    void* d_all = nullptr;
    if (hipMalloc(&d_all, rt_temporal_workspace_bytes(w, h)) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    const Workspace ws = carve(d_all, n);
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
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    const Workspace ws = carve(state->d_workspace, n);
    const uint32_t cur = state->parity, old = state->parity ^ 1u;
    // a state of another frame size restarts
    const bool prev = state->frames != 0u && state->w == w && state->h == h;

    if (hipMemsetAsync(ws.current, 0, 16*n, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": hipMemset");
    rt_stats fs;
    err = rt_render_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    // a frame clears the scene's cancel flag when its loop starts: one raised after it is seen here
    if (rt_internal_scene_cancelled(s)) return fail(RT_ERROR_CANCELLED, "render cancelled");
    err = rt_gbuffer_device(s, camera, st->lens_distortion, w, h, ws.gbuffer[cur], hip_stream);
    if (err) return err;
    err = rt_temporal_accumulate_device(device, ws.current, ws.gbuffer[cur], prev ? ws.history[old] : nullptr,
                                        prev ? ws.length[old] : nullptr, prev ? ws.gbuffer[old] : nullptr, &state->camera,
                                        state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream);
    if (err) return err;
    if (hipMemcpyAsync(d_out, ws.history[cur], 16*n, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
        (d_length_out && hipMemcpyAsync(d_length_out, ws.length[cur], 4*n, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": copy out");
    state->w = w; state->h = h;
    state->camera = *camera;
    state->lens_distortion = st->lens_distortion;
    state->parity = old;
    state->frames += 1u;
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
    err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the history, the length
    if (hipMalloc(&d, 20*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_out = reinterpret_cast<float*>(d);
    float* d_len = reinterpret_cast<float*>(d + 16*n);
    err = rt_render_temporal_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, state, d_out,
                                    out_length ? d_len : nullptr, nullptr, stats);
    if (!err && (hipMemcpy(out_pixels, d_out, 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (out_length && hipMemcpy(out_length, d_len, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

}  // extern "C"
