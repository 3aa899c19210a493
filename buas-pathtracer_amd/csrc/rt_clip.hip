// rt_clip.hip — neighbourhood clipping of the temporal history against ghosting: the statistics of the current frame's
// (2r + 1)^2 windows (rt_temporal_neighbourhood_device, rt_temporal_neighbourhood), the accumulate stage that clips the
// history to mean -+ gamma*sigma of them before the blend (rt_temporal_accumulate_clip_device,
// rt_temporal_accumulate_clip) and the driver that runs one frame of the loop on the public entries
// (rt_render_temporal_clipped_device, rt_render_temporal_clipped).  Beyond the reference, an opt-in: no
// other entry calls it.
//
// Both stages are defined operation by operation in DESIGN.md ("Neighbourhood clipping"); tests/ref_clip/ref_clip.c
// restates them in plain C and the two kernels match that checker bit for bit.  The accumulate kernel's text is
// rt_temporal_shared.h's one body with the motion, deform and clip flags on and the moments flag as the entry's
// d_moments says.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_temporal_shared.h"   // the accumulate body and what the stage's entries and the drivers share on the host

namespace {

static_assert(sizeof(rt_neighbourhood_texel) == 32, "rt_neighbourhood_texel is 32 bytes");
static_assert(sizeof(rt_temporal_clip_params) == 16, "rt_temporal_clip_params is 16 bytes");

// The statistics.  A 256-thread block owns 64 x 16 pixels; a wave covers 64 consecutive pixels of a row, as k_post and
// the accumulate kernels do, and four rows below one another.  The block stages its pixels' values with a halo of R
// ({r, g, b, valid ? 1 : 0} as one float4, +0 four times for an invalid pixel and outside the image) in LDS: 70 x 22
// float4 at R = 3, 24 640 bytes, so six blocks fit a CU's 160 KiB.  A lane reads float4 number `lane + d` of a row: 16
// lanes span one 256-byte bank row, which ds_read_b128 serves without a conflict.  Each thread then forms the row sums
// H of the 4 + 2R rows its four pixels need, one after the other in registers, and adds each into the column sums of
// the pixels whose window holds that row, in row order: the separable order of DESIGN.md, with no second LDS buffer
// and one barrier.  A row sum is formed by up to (4 + 2R)/4 threads; that costs LDS reads (70 float4 per thread at
// R = 3 against 49 per pixel unshared) and saves the write, the barrier and the 39 KiB of a row-sum buffer.
constexpr int NB_W = 64, NB_H = 16, NB_ROWS = 4;     // the block's pixels; rows per thread

template <int R>
__global__ void __launch_bounds__(256) k_neighbourhood(const float4* __restrict__ current, uint32_t w, uint32_t h,
                                                       float firefly_clamp, rt_neighbourhood_texel* __restrict__ out) {
    constexpr int TW = NB_W + 2*R, TH = NB_H + 2*R;
    __shared__ float4 tile[TH*TW];
    const int64_t bx = (int64_t)blockIdx.x*NB_W, by = (int64_t)blockIdx.y*NB_H;
    for (int k = threadIdx.x; k < TW*TH; k += 256) {
        const int ty = k / TW, tx = k - ty*TW;
        const int64_t gx = bx + tx - R, gy = by + ty - R;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gy >= 0 && gx < (int64_t)w && gy < (int64_t)h) {
            // the accumulate stage's steps 1 and 2
            const float4 s = current[(size_t)gy*w + (size_t)gx];
            if (s.w > VALID_W) {
                float cr = s.x / s.w, cg = s.y / s.w, cb = s.z / s.w;
                if (finite_f(cr) && finite_f(cg) && finite_f(cb)) {
                    cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
                    if (firefly_clamp > 0.0f) {
                        cr = cr < firefly_clamp ? cr : firefly_clamp;
                        cg = cg < firefly_clamp ? cg : firefly_clamp;
                        cb = cb < firefly_clamp ? cb : firefly_clamp;
                    }
                    v = make_float4(cr, cg, cb, 1.0f);
                }
            }
        }
        tile[k] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float S[NB_ROWS][7];
#pragma unroll
    for (int j = 0; j < NB_ROWS + 2*R; ++j) {
        const float4* row = &tile[(wave*NB_ROWS + j)*TW + lane];
        float4 v = row[0];
        float H[7] = {v.x, v.y, v.z, v.x*v.x, v.y*v.y, v.z*v.z, v.w};
#pragma unroll
        for (int d = 1; d <= 2*R; ++d) {
            v = row[d];
            H[0] = H[0] + v.x; H[1] = H[1] + v.y; H[2] = H[2] + v.z;
            H[3] = H[3] + v.x*v.x; H[4] = H[4] + v.y*v.y; H[5] = H[5] + v.z*v.z;
            H[6] = H[6] + v.w;
        }
#pragma unroll
        for (int k = 0; k < NB_ROWS; ++k) {
            if (j == k) {
#pragma unroll
                for (int c = 0; c < 7; ++c) S[k][c] = H[c];
            } else if (j > k && j <= k + 2*R) {
#pragma unroll
                for (int c = 0; c < 7; ++c) S[k][c] = S[k][c] + H[c];
            }
        }
    }
    const int64_t x = bx + lane;
    if (x >= (int64_t)w) return;
#pragma unroll
    for (int k = 0; k < NB_ROWS; ++k) {
        const int64_t y = by + wave*NB_ROWS + k;
        if (y >= (int64_t)h) break;
        rt_neighbourhood_texel t = {{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};
        const float n = S[k][6];
        if (n > 0.0f) {
            float mean[3], sigma[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mean[c] = S[k][c] / n;
                float var = S[k][3 + c] / n - mean[c]*mean[c];
                var = var > 0.0f ? var : 0.0f;          // NaN goes to 0
                sigma[c] = __builtin_sqrtf(var);
            }
            t.mean = {mean[0], mean[1], mean[2]};
            t.count = n;
            t.sigma = {sigma[0], sigma[1], sigma[2]};
        }
        out[(size_t)y*w + (size_t)x] = t;
    }
}

template <bool MOMENTS>
__global__ void __launch_bounds__(256) k_temporal_accumulate_clip(
        const float4* __restrict__ current, const rt_gbuffer_texel* __restrict__ gbuffer,
        const float4* __restrict__ prev_history, const float* __restrict__ prev_length,
        const rt_gbuffer_texel* __restrict__ prev_gbuffer, const float2* __restrict__ prev_moments, TaCamera cam,
        uint32_t w, uint32_t h, rt_temporal_params p, const rt_motion_entry* __restrict__ motion, uint32_t motion_count,
        const rt_surface_texel* __restrict__ surface, const rt_deform_entry* __restrict__ deform, uint32_t deform_count,
        float4* __restrict__ history, float* __restrict__ length, float2* __restrict__ moments,
        float2* __restrict__ velocity, TaClip clip) {
    temporal_accumulate_body<MOMENTS, true, true, true>(current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_moments, cam, w,
                                                        h, p, motion, motion_count, surface, deform, deform_count, history, length,
                                                        moments, velocity, clip);
}

int check_neighbourhood(const std::string& e, const char* prefix, const float* current, uint32_t w, uint32_t h, uint32_t radius,
                        float firefly_clamp, const rt_neighbourhood_texel* out) {
    const std::string d = prefix;
    if (!current) return fail(RT_ERROR_INVALID, e + ": null " + d + "current");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null " + d + "out");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if ((uint64_t)w*h >= ((uint64_t)1 << 32)) return fail(RT_ERROR_INVALID, e + ": w*h must be below 2^32");
    if (radius < 1u || radius > 3u) return fail(RT_ERROR_INVALID, e + ": radius must be in 1..3");
    if (bad_value(firefly_clamp)) return fail(RT_ERROR_INVALID, e + ": firefly_clamp must be finite and >= 0");
    if (static_cast<const void*>(out) == static_cast<const void*>(current))
        return fail(RT_ERROR_INVALID, e + ": " + d + "out aliases " + d + "current");
    return RT_OK;
}

// the driver's workspace: rt_render_temporal_deform_device's, then the neighbourhood texels on a 16-byte boundary and
// the clip amounts
struct Workspace : TaWorkspace {
    rt_motion_entry* motion;
    rt_surface_texel* surface;
    rt_deform_entry* deform;
    rt_neighbourhood_texel* neighbourhood;
    float* clip_amount;
};
size_t surface_offset(uint32_t w, uint32_t h, uint32_t count) {
    return (rt_temporal_motion_workspace_bytes(w, h, count) + 15) & ~(size_t)15;
}
size_t texels_offset(uint32_t w, uint32_t h, uint32_t count) {
    return (rt_temporal_deform_workspace_bytes(w, h, count) + 15) & ~(size_t)15;
}
Workspace carve(void* d_workspace, uint32_t w, uint32_t h, uint32_t count) {
    const size_t n = (size_t)w*h;
    char* base = static_cast<char*>(d_workspace);
    Workspace ws;
    static_cast<TaWorkspace&>(ws) = carve_temporal(d_workspace, n);
    ws.motion = reinterpret_cast<rt_motion_entry*>(base + motion_table_offset(n));
    ws.surface = reinterpret_cast<rt_surface_texel*>(base + surface_offset(w, h, count));
    ws.deform = reinterpret_cast<rt_deform_entry*>(base + surface_offset(w, h, count) + sizeof(rt_surface_texel)*n);
    ws.neighbourhood = reinterpret_cast<rt_neighbourhood_texel*>(base + texels_offset(w, h, count));
    ws.clip_amount = reinterpret_cast<float*>(base + texels_offset(w, h, count) + sizeof(rt_neighbourhood_texel)*n);
    return ws;
}

}  // namespace

extern "C" {

int rt_temporal_neighbourhood_device(int device, const float* d_current, uint32_t w, uint32_t h, uint32_t radius,
                                     float firefly_clamp, rt_neighbourhood_texel* d_out, void* hip_stream) {
    const std::string e = "rt_temporal_neighbourhood_device";
    int err = check_neighbourhood(e, "d_", d_current, w, h, radius, firefly_clamp, d_out);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((uint32_t)(((uint64_t)w + NB_W - 1) / NB_W), (uint32_t)(((uint64_t)h + NB_H - 1) / NB_H));
    const float4* cur = f4(d_current);
    if (radius == 1u) k_neighbourhood<1><<<grid, 256, 0, stream>>>(cur, w, h, firefly_clamp, d_out);
    else if (radius == 2u) k_neighbourhood<2><<<grid, 256, 0, stream>>>(cur, w, h, firefly_clamp, d_out);
    else k_neighbourhood<3><<<grid, 256, 0, stream>>>(cur, w, h, firefly_clamp, d_out);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, e + ": " + hipGetErrorString(herr));
    return RT_OK;
}

int rt_temporal_neighbourhood(int device, const float* current, uint32_t w, uint32_t h, uint32_t radius, float firefly_clamp,
                              rt_neighbourhood_texel* out) {
    const std::string e = "rt_temporal_neighbourhood";
    int err = check_neighbourhood(e, "", current, w, h, radius, firefly_clamp, out);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the current frame, the texels
    if (hipMalloc(&d, 48*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_cur = reinterpret_cast<float*>(d);
    rt_neighbourhood_texel* d_out = reinterpret_cast<rt_neighbourhood_texel*>(d + 16*n);
    if (hipMemcpy(d_cur, current, 16*n, hipMemcpyHostToDevice) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_temporal_neighbourhood_device(device, d_cur, w, h, radius, firefly_clamp, d_out, nullptr);
    if (!err && hipMemcpy(out, d_out, 32*n, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

int rt_temporal_clip_default_params(rt_temporal_clip_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_temporal_clip_default_params: null out");
    out->radius = 3u;
    out->gamma = 0.5f;         // profiles/clip_quality.txt's sweep
    out->min_count = 2.0f;
    out->reserved = 0u;
    return RT_OK;
}

int rt_temporal_accumulate_clip_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                       const float* d_prev_history, const float* d_prev_length,
                                       const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                       float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                       float* d_history, float* d_length, void* hip_stream, const rt_motion_entry* d_motion,
                                       uint32_t motion_count, const float* d_prev_moments, float* d_moments, float* d_velocity,
                                       const rt_surface_texel* d_surface, const rt_deform_entry* d_deform, uint32_t deform_count,
                                       const rt_neighbourhood_texel* d_neighbourhood, float gamma, float min_count,
                                       float* d_clip_amount) {
    const std::string e = "rt_temporal_accumulate_clip_device";
    const TaArgs a = {d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera, prev_lens_distortion,
                      w, h, p, d_history, d_length, d_motion, motion_count, d_prev_moments, d_moments, d_velocity,
                      d_surface, d_deform, deform_count, d_neighbourhood, gamma, min_count, d_clip_amount};
    int err = check_clip(e, "d_", a);
    if (err) return err;
    const TaClip clip = {d_neighbourhood, gamma, min_count, d_clip_amount};
    return launch_accumulate(e, device, d_moments ? k_temporal_accumulate_clip<true> : k_temporal_accumulate_clip<false>, w, h,
                             hip_stream, f4(d_current), d_gbuffer, f4(d_prev_history), d_prev_length, d_prev_gbuffer,
                             f2(d_prev_moments), ta_camera(a), w, h, *p, d_motion, motion_count, d_surface, d_deform, deform_count,
                             f4(d_history), d_length, f2(d_moments), f2(d_velocity), clip);
}

int rt_temporal_accumulate_clip(int device, const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                                float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p, float* history,
                                float* length, const rt_motion_entry* motion, uint32_t motion_count, const float* prev_moments,
                                float* moments, float* velocity, const rt_surface_texel* surface, const rt_deform_entry* deform,
                                uint32_t deform_count, const rt_neighbourhood_texel* neighbourhood, float gamma, float min_count,
                                float* clip_amount) {
    const std::string e = "rt_temporal_accumulate_clip";
    const TaArgs a = {current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, prev_lens_distortion,
                      w, h, p, history, length, motion, motion_count, prev_moments, moments, velocity, surface, deform, deform_count,
                      neighbourhood, gamma, min_count, clip_amount};
    int err = check_clip(e, "", a);
    if (err) return err;
    return stage_accumulate(e, device, a, true, [&](const TaArgs& d) {
        return rt_temporal_accumulate_clip_device(device, d.current, d.gbuffer, d.prev_history, d.prev_length, d.prev_gbuffer,
                                                  prev_camera, prev_lens_distortion, w, h, p, d.history, d.length, nullptr,
                                                  d.motion, motion_count, d.prev_moments, d.moments, d.velocity, d.surface,
                                                  d.deform, deform_count, d.neighbourhood, gamma, min_count, d.clip_amount);
    });
}

size_t rt_temporal_clipped_workspace_bytes(uint32_t w, uint32_t h, uint32_t primitive_count) {
    return texels_offset(w, h, primitive_count) + (sizeof(rt_neighbourhood_texel) + 4)*(size_t)w*h;
}

int rt_render_temporal_clipped_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                      const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                                      uint32_t frame_count, const rt_temporal_params* p, rt_temporal_motion_state* state,
                                      uint32_t mesh_count, const rt_deform_mesh* meshes, const rt_temporal_clip_params* cp,
                                      float* d_out, float* d_length_out, float* d_clip_amount_out, void* hip_stream,
                                      rt_stats* stats) {
    const std::string e = "rt_render_temporal_clipped_device";
    int err = check_clip_params(e, cp);
    if (err) return err;
    err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, d_out, "d_out");
    if (err) return err;
    if ((uint64_t)w*h >= ((uint64_t)1 << 32)) return fail(RT_ERROR_INVALID, e + ": w*h must be below 2^32");
    uint32_t count = 0;
    err = rt_scene_primitive_transforms(s, 0, nullptr, &count);
    if (err) return err;
    std::vector<rt_m4x4inv> now(count);
    err = rt_scene_primitive_transforms(s, count, now.data(), &count);
    if (err) return err;
    // a state of another frame size or of another primitive count restarts
    const bool prev = state->frames != 0u && state->w == w && state->h == h && state->primitive_count == count;
    // the list is checked on every frame, before anything is rendered; a frame without history uses no entry of it
    std::vector<rt_deform_entry> deform(count);
    err = rt_scene_deform_table(s, mesh_count, meshes, count, prev ? state->transforms : now.data(), deform.data());
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    const Workspace ws = carve(state->d_workspace, w, h, count);
    const uint32_t cur = state->parity, old = state->parity ^ 1u;

    rt_stats fs;
    err = render_current(e, s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    err = rt_gbuffer_surface_device(s, camera, st->lens_distortion, w, h, ws.gbuffer[cur], ws.surface, hip_stream);
    if (err) return err;
    err = rt_temporal_neighbourhood_device(device, ws.current, w, h, cp->radius, p->firefly_clamp, ws.neighbourhood, hip_stream);
    if (err) return err;
    const bool tables = prev && count;
    if (tables) {
        std::vector<rt_motion_entry> table(count);
        err = rt_motion_table(count, now.data(), state->transforms, table.data());
        if (err) return err;
        // the stage of the frame before has synchronised its stream: nothing reads the tables now
        if (hipMemcpy(ws.motion, table.data(), sizeof(rt_motion_entry)*(size_t)count, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(ws.deform, deform.data(), sizeof(rt_deform_entry)*(size_t)count, hipMemcpyHostToDevice) != hipSuccess)
            return fail(RT_ERROR_DEVICE, e + ": table upload");
    }
    err = rt_temporal_accumulate_clip_device(device, ws.current, ws.gbuffer[cur], prev ? ws.history[old] : nullptr,
                                             prev ? ws.length[old] : nullptr, prev ? ws.gbuffer[old] : nullptr, &state->camera,
                                             state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream,
                                             tables ? ws.motion : nullptr, prev ? count : 0u, nullptr, nullptr, nullptr,
                                             ws.surface, tables ? ws.deform : nullptr, prev ? count : 0u, ws.neighbourhood,
                                             cp->gamma, cp->min_count, ws.clip_amount);
    if (err) return err;
    err = copy_out_history(e, ws, cur, n, d_out, d_length_out, hip_stream);
    if (err) return err;
    if (d_clip_amount_out) {
        hipStream_t stream = static_cast<hipStream_t>(hip_stream);
        if (hipMemcpyAsync(d_clip_amount_out, ws.clip_amount, 4*n, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return fail(RT_ERROR_DEVICE, e + ": copy out");
    }
    state->primitive_count = count;
    if (count) memcpy(state->transforms, now.data(), sizeof(rt_m4x4inv)*(size_t)count);
    advance_state(state, w, h, camera, st);
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_render_temporal_clipped(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                               const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                               const rt_temporal_params* p, rt_temporal_motion_state* state, uint32_t mesh_count,
                               const rt_deform_mesh* meshes, const rt_temporal_clip_params* cp, float* out_pixels,
                               float* out_length, float* out_clip_amount, rt_stats* stats) {
    const std::string e = "rt_render_temporal_clipped";
    int err = check_clip_params(e, cp);
    if (err) return err;
    err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, out_pixels, "out_pixels");
    if (err) return err;
    if ((uint64_t)w*h >= ((uint64_t)1 << 32)) return fail(RT_ERROR_INVALID, e + ": w*h must be below 2^32");
    err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the history, the length, the clip amounts
    if (hipMalloc(&d, 24*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_out = reinterpret_cast<float*>(d);
    float* d_len = reinterpret_cast<float*>(d + 16*n);
    float* d_amt = reinterpret_cast<float*>(d + 20*n);
    err = rt_render_temporal_clipped_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, state, mesh_count,
                                            meshes, cp, d_out, out_length ? d_len : nullptr, out_clip_amount ? d_amt : nullptr,
                                            nullptr, stats);
    if (!err && (hipMemcpy(out_pixels, d_out, 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (out_length && hipMemcpy(out_length, d_len, 4*n, hipMemcpyDeviceToHost) != hipSuccess) ||
                 (out_clip_amount && hipMemcpy(out_clip_amount, d_amt, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

}  // extern "C"
