// rt_adaptive.hip — adaptive sampling by tiles: the per-tile error estimate (rt_tile_error_device, rt_tile_error)
// and the driver that loops it with frames over a tile list (rt_render_adaptive_device, rt_render_adaptive).
// Beyond the reference, an opt-in: no other entry calls it.  The frames themselves are
// rt_render_tiles_device's (rt_kernels.hip): nothing here touches a sample.
//
// The estimate is defined operation by operation in DESIGN.md ("Adaptive sampling by tiles"); tests/ref_adaptive/
// ref_adaptive.c restates it in plain C and k_tile_error matches that checker bit for bit: IEEE f32, no
// contraction, division as /, sqrtf correctly rounded, and one fixed order of additions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_internal.h"

namespace {

constexpr float VALID_W = 0.001f;       // k_post's resolve threshold
constexpr int TE_BLOCK = 256;
constexpr uint32_t TE_MAX_GRID = 1u << 20;

int fail(int code, const std::string& message) { rt_internal_set_error(message.c_str()); return code; }

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// One workgroup per listed tile (a grid-stride loop over the list past TE_MAX_GRID tiles).  Thread i adds the
// errors of pixels i, i + 256, ... of the tile's raster order, in that order; the 256 partial sums and counts
// are then added pairwise in LDS, element i += element i + s for s = 128, 64, ..., 1.
__global__ void __launch_bounds__(TE_BLOCK) k_tile_error(const float4* __restrict__ A, const float4* __restrict__ B,
                                                         uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                                                         uint32_t tcx, uint32_t ntiles, const uint32_t* __restrict__ ids,
                                                         uint32_t count, float floor_m, float* __restrict__ out_error,
                                                         uint32_t* __restrict__ out_valid) {
    __shared__ float s_sum[TE_BLOCK];
    __shared__ uint32_t s_cnt[TE_BLOCK];
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < count; k += gridDim.x) {
        const uint32_t t = ids ? ids[k] : k;
        float sum = 0.0f;
        uint32_t cnt = 0;
        if (t < ntiles) {                       // an id out of range owns no pixel: +INFINITY, 0
            const uint32_t min_x = tile_w*(t % tcx), min_y = tile_h*(t / tcx);
            const uint32_t tw = min(w, min_x + tile_w) - min_x, th = min(h, min_y + tile_h) - min_y;
            const uint64_t n = (uint64_t)tw*th;
            for (uint64_t i = tid; i < n; i += TE_BLOCK) {
                const uint32_t x = min_x + (uint32_t)(i % tw), y = min_y + (uint32_t)(i / tw);
                const float4 a4 = A[(size_t)y*w + x], b4 = B[(size_t)y*w + x];
                const bool valid = a4.w > VALID_W && b4.w > VALID_W &&
                                   finite_f(a4.x) && finite_f(a4.y) && finite_f(a4.z) && finite_f(a4.w) &&
                                   finite_f(b4.x) && finite_f(b4.y) && finite_f(b4.z) && finite_f(b4.w);
                if (!valid) continue;
                const float ar = a4.x / a4.w, ag = a4.y / a4.w, ab = a4.z / a4.w;
                const float br = b4.x / b4.w, bg = b4.y / b4.w, bb = b4.z / b4.w;
                const float mw = a4.w + b4.w;
                const float mr = (a4.x + b4.x) / mw, mg = (a4.y + b4.y) / mw, mb = (a4.z + b4.z) / mw;
                const float d = (fabsf(ar - br) + fabsf(ag - bg)) + fabsf(ab - bb);
                const float m = (mr + mg) + mb;
                const float e = d / sqrtf(m > floor_m ? m : floor_m);
                sum = sum + e;
                cnt += 1u;
            }
        }
        s_sum[tid] = sum;
        s_cnt[tid] = cnt;
        __syncthreads();
        for (uint32_t s = TE_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) {
                s_sum[tid] = s_sum[tid] + s_sum[tid + s];
                s_cnt[tid] = s_cnt[tid] + s_cnt[tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const uint32_t nv = s_cnt[0];
            out_error[k] = nv ? s_sum[0] / (float)nv : __uint_as_float(0x7F800000u);
            out_valid[k] = nv;
        }
        __syncthreads();                        // the next tile's partials overwrite s_sum / s_cnt
    }
}

// The driver's last step: samples are added to the caller's buffer, p + (a + b) per float.
__global__ void __launch_bounds__(256) k_add_halves(const float4* __restrict__ A, const float4* __restrict__ B, size_t n,
                                                    float4* __restrict__ pixels) {
    const size_t i = (size_t)blockIdx.x*256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = A[i], b = B[i];
    float4 p = pixels[i];
    p.x = p.x + (a.x + b.x);
    p.y = p.y + (a.y + b.y);
    p.z = p.z + (a.z + b.z);
    p.w = p.w + (a.w + b.w);
    pixels[i] = p;
}

uint64_t tile_count_of(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h) {
    return (uint64_t)((w + tile_w - 1) / tile_w)*((h + tile_h - 1) / tile_h);
}

int check_frame(const std::string& e, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h) {
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if (!tile_w) return fail(RT_ERROR_INVALID, e + ": tile_w is 0");
    if (!tile_h) return fail(RT_ERROR_INVALID, e + ": tile_h is 0");
    if (w > 65535u || h > 65535u) return fail(RT_ERROR_INVALID, e + ": w or h larger than 65535 pixels");
    return RT_OK;
}

int check_error_params(const std::string& e, const rt_tile_error_params* p) {
    if (!p) return fail(RT_ERROR_INVALID, e + ": null rt_tile_error_params");
    if (!(p->floor > 0.0f) || p->floor > 3.402823466e38f)
        return fail(RT_ERROR_INVALID, e + ": rt_tile_error_params: floor must be finite and > 0");
    return RT_OK;
}

// every check of rt_tile_error_device / rt_tile_error that needs no device
int check_tile_error(const std::string& e, const void* a, const void* b, uint32_t w, uint32_t h, uint32_t tile_w,
                     uint32_t tile_h, bool has_ids, uint32_t tile_count, const rt_tile_error_params* p, const void* out_error,
                     const void* out_valid) {
    if (!a) return fail(RT_ERROR_INVALID, e + ": null half_a");
    if (!b) return fail(RT_ERROR_INVALID, e + ": null half_b");
    if (!out_error) return fail(RT_ERROR_INVALID, e + ": null tile_error");
    if (!out_valid) return fail(RT_ERROR_INVALID, e + ": null tile_valid");
    int err = check_frame(e, w, h, tile_w, tile_h);
    if (err) return err;
    err = check_error_params(e, p);
    if (err) return err;
    const uint64_t ntiles = tile_count_of(w, h, tile_w, tile_h);
    if (!tile_count) return fail(RT_ERROR_INVALID, e + ": tile_count is 0");
    if (tile_count > ntiles) return fail(RT_ERROR_INVALID, e + ": tile_count is above the frame's " + std::to_string(ntiles) + " tiles");
    if (!has_ids && tile_count != ntiles)
        return fail(RT_ERROR_INVALID, e + ": null tile_ids means every tile: tile_count must be " + std::to_string(ntiles));
    return RT_OK;
}

int check_adaptive_params(const std::string& e, const rt_adaptive_params* p) {
    if (!p) return fail(RT_ERROR_INVALID, e + ": null rt_adaptive_params");
    if (!p->step_spp || (p->step_spp & 1u)) return fail(RT_ERROR_INVALID, e + ": rt_adaptive_params: step_spp must be even and > 0");
    if (!p->min_spp || p->min_spp % p->step_spp) return fail(RT_ERROR_INVALID, e + ": rt_adaptive_params: min_spp must be a multiple of step_spp and > 0");
    if (!p->max_spp || p->max_spp % p->step_spp) return fail(RT_ERROR_INVALID, e + ": rt_adaptive_params: max_spp must be a multiple of step_spp and > 0");
    if (p->min_spp > p->max_spp) return fail(RT_ERROR_INVALID, e + ": rt_adaptive_params: min_spp is above max_spp");
    if (!(p->threshold >= 0.0f) || p->threshold > 3.402823466e38f)
        return fail(RT_ERROR_INVALID, e + ": rt_adaptive_params: threshold must be finite and >= 0");
    return check_error_params(e, &p->error);
}

void add_stats(rt_stats& sum, const rt_stats& f) {
    sum.closest_hit_rays += f.closest_hit_rays;
    sum.shadow_rays += f.shadow_rays;
    sum.samples += f.samples;
    sum.iterations += f.iterations;
    for (int k = 0; k < RT_KERNEL_COUNT; ++k) { sum.kernel_ms[k] += f.kernel_ms[k]; sum.kernel_launches[k] += f.kernel_launches[k]; }
    for (int k = 0; k < 2; ++k) {
        sum.traced_rays[k] += f.traced_rays[k];
        sum.trace_steps[k] += f.trace_steps[k];
        const rt_traversal_stats* src[2] = {&f.traversal[k], &f.traversal_ref[k]};
        rt_traversal_stats* dst[2] = {&sum.traversal[k], &sum.traversal_ref[k]};
        for (int j = 0; j < 2; ++j) {
            dst[j]->mesh_intersection_count += src[j]->mesh_intersection_count;
            dst[j]->mesh_bvh_traversals += src[j]->mesh_bvh_traversals;
            dst[j]->mesh_node_traversals += src[j]->mesh_node_traversals;
            dst[j]->mesh_leaf_traversals += src[j]->mesh_leaf_traversals;
        }
    }
    sum.splat_mode = f.splat_mode;
    sum.shadow_launch = f.shadow_launch;
}

}  // namespace

extern "C" {

int rt_tile_error_default_params(rt_tile_error_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_tile_error_default_params: null out");
    *out = {};
    out->floor = 1e-4f;
    return RT_OK;
}

int rt_tile_error_device(int device, const float* d_half_a, const float* d_half_b, uint32_t w, uint32_t h,
                         uint32_t tile_w, uint32_t tile_h, const uint32_t* d_tile_ids, uint32_t tile_count,
                         const rt_tile_error_params* p, float* d_tile_error, uint32_t* d_tile_valid, void* hip_stream) {
    int err = check_tile_error("rt_tile_error_device", d_half_a, d_half_b, w, h, tile_w, tile_h, d_tile_ids != nullptr,
                               tile_count, p, d_tile_error, d_tile_valid);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const uint32_t tcx = (w + tile_w - 1) / tile_w;
    const uint32_t ntiles = (uint32_t)tile_count_of(w, h, tile_w, tile_h);      // < 2^32: w, h <= 65535
    const uint32_t grid = tile_count < TE_MAX_GRID ? tile_count : TE_MAX_GRID;
    k_tile_error<<<grid, TE_BLOCK, 0, stream>>>(reinterpret_cast<const float4*>(d_half_a), reinterpret_cast<const float4*>(d_half_b),
                                                w, h, tile_w, tile_h, tcx, ntiles, d_tile_ids, tile_count, p->floor,
                                                d_tile_error, d_tile_valid);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, std::string("rt_tile_error_device: ") + hipGetErrorString(herr));
    return RT_OK;
}

int rt_tile_error(int device, const float* half_a, const float* half_b, uint32_t w, uint32_t h, uint32_t tile_w,
                  uint32_t tile_h, const uint32_t* tile_ids, uint32_t tile_count, const rt_tile_error_params* p,
                  float* tile_error, uint32_t* tile_valid) {
    const std::string e = "rt_tile_error";
    int err = check_tile_error(e, half_a, half_b, w, h, tile_w, tile_h, tile_ids != nullptr, tile_count, p, tile_error, tile_valid);
    if (err) return err;
    if (tile_ids) {
        const uint64_t ntiles = tile_count_of(w, h, tile_w, tile_h);
        for (uint32_t i = 0; i < tile_count; ++i)
            if (tile_ids[i] >= ntiles)
                return fail(RT_ERROR_INVALID, e + ": tile_ids[" + std::to_string(i) + "] = " + std::to_string(tile_ids[i]) +
                                              " is out of range: the frame has " + std::to_string(ntiles) + " tiles");
    }
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t bytes = (size_t)16*w*h, lbytes = (size_t)4*tile_count;
    char* d_all = nullptr;                                  // A, B, ids, errors, counts
    if (hipMalloc(&d_all, 2*bytes + 3*lbytes) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_a = reinterpret_cast<float*>(d_all);
    float* d_b = reinterpret_cast<float*>(d_all + bytes);
    uint32_t* d_ids = reinterpret_cast<uint32_t*>(d_all + 2*bytes);
    float* d_err = reinterpret_cast<float*>(d_all + 2*bytes + lbytes);
    uint32_t* d_val = reinterpret_cast<uint32_t*>(d_all + 2*bytes + 2*lbytes);
    if (hipMemcpy(d_a, half_a, bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_b, half_b, bytes, hipMemcpyHostToDevice) != hipSuccess ||
        (tile_ids && hipMemcpy(d_ids, tile_ids, lbytes, hipMemcpyHostToDevice) != hipSuccess))
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_tile_error_device(device, d_a, d_b, w, h, tile_w, tile_h, tile_ids ? d_ids : nullptr, tile_count, p,
                                         d_err, d_val, nullptr);
    if (!err && (hipMemcpy(tile_error, d_err, lbytes, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(tile_valid, d_val, lbytes, hipMemcpyDeviceToHost) != hipSuccess))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d_all);
    return err;
}

int rt_adaptive_default_params(rt_adaptive_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_adaptive_default_params: null out");
    *out = {};
    out->min_spp = 16;
    out->max_spp = 256;
    out->step_spp = 16;
    // where C3 at 480x270 spends the samples of a 64 to 128 spp uniform frame: a budget, not a
    // quality claim -- at equal samples the uniform frame was as good or better there
    out->threshold = 0.5f;
    out->error.floor = 1e-4f;
    return RT_OK;
}

size_t rt_adaptive_workspace_bytes(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h) {
    if (!w || !h || !tile_w || !tile_h) return 0;
    // the two half buffers; the active list, its errors and its counts
    return (size_t)32*w*h + (size_t)12*tile_count_of(w, h, tile_w, tile_h);
}

int rt_render_adaptive_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                              uint32_t tile_w, uint32_t tile_h, uint32_t total_frame_index, uint32_t w, uint32_t h,
                              uint32_t frame_count, const rt_adaptive_params* p, void* d_workspace, float* d_pixels,
                              uint32_t* out_tile_spp, void* hip_stream, rt_stats* stats) {
    const std::string e = "rt_render_adaptive_device";
    int err = check_adaptive_params(e, p);
    if (err) return err;
    err = check_frame(e, w, h, tile_w, tile_h);
    if (err) return err;
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    if (!camera) return fail(RT_ERROR_INVALID, e + ": null camera");
    if (!st) return fail(RT_ERROR_INVALID, e + ": null settings");
    if (!filter) return fail(RT_ERROR_INVALID, e + ": null filter");
    if (!d_pixels) return fail(RT_ERROR_INVALID, e + ": null d_pixels");
    const auto t0 = std::chrono::steady_clock::now();
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    const uint32_t ntiles = (uint32_t)tile_count_of(w, h, tile_w, tile_h);
    void* own = nullptr;
    if (!d_workspace) {
        if (hipMalloc(&own, rt_adaptive_workspace_bytes(w, h, tile_w, tile_h)) != hipSuccess)
            return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc of the workspace");
        d_workspace = own;
    }
    char* ws = static_cast<char*>(d_workspace);
    float* d_half[2] = {reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws + 16*n)};
    uint32_t* d_ids = reinterpret_cast<uint32_t*>(ws + 32*n);
    float* d_err = reinterpret_cast<float*>(ws + 32*n + (size_t)4*ntiles);
    uint32_t* d_val = reinterpret_cast<uint32_t*>(ws + 32*n + (size_t)8*ntiles);

    std::vector<uint32_t> active(ntiles), spp(ntiles, 0u);
    for (uint32_t t = 0; t < ntiles; ++t) active[t] = t;
    std::vector<float> errors(ntiles);
    rt_stats total;
    memset(&total, 0, sizeof total);
    rt_settings half_st = *st;
    half_st.samples_per_pixel = p->step_spp / 2u;
    auto done = [&](int code) { if (own) (void)hipFree(own); return code; };
    auto hip_fail = [&](const char* what) { return done(fail(RT_ERROR_DEVICE, e + ": " + what)); };
    auto cancelled = [&]() { return done(fail(RT_ERROR_CANCELLED, "render cancelled")); };

    if (hipMemsetAsync(ws, 0, 32*n, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return hip_fail("hipMemset");
    for (uint32_t r = 0; !active.empty() && (uint64_t)r*p->step_spp < p->max_spp; ++r) {
        const uint32_t count = (uint32_t)active.size();
        for (int half = 0; half < 2; ++half) {
            rt_stats fs;
            err = rt_render_tiles_device(s, camera, &half_st, filter, tile_w, tile_h, active.data(), count, total_frame_index,
                                         w, h, frame_count + r*p->step_spp + (uint32_t)half*(p->step_spp / 2u), d_half[half],
                                         hip_stream, &fs);
            if (err) return done(err);
            add_stats(total, fs);
            // a frame clears the scene's cancel flag when its loop starts: one raised between two frames is seen here
            if (rt_internal_scene_cancelled(s)) return cancelled();
        }
        for (uint32_t t : active) spp[t] += p->step_spp;
        if ((uint64_t)(r + 1)*p->step_spp < p->min_spp) continue;
        if (hipMemcpy(d_ids, active.data(), (size_t)4*count, hipMemcpyHostToDevice) != hipSuccess) return hip_fail("copy of the active list");
        err = rt_tile_error_device(device, d_half[0], d_half[1], w, h, tile_w, tile_h, d_ids, count, &p->error, d_err, d_val,
                                   hip_stream);
        if (err) return done(err);
        if (hipMemcpy(errors.data(), d_err, (size_t)4*count, hipMemcpyDeviceToHost) != hipSuccess) return hip_fail("copy of the errors");
        size_t keep = 0;
        for (uint32_t i = 0; i < count; ++i)
            if (!(errors[i] <= p->threshold)) active[keep++] = active[i];      // a NaN error never retires a tile
        active.resize(keep);
        if (rt_internal_scene_cancelled(s)) return cancelled();
    }
    k_add_halves<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(reinterpret_cast<const float4*>(d_half[0]),
                                                                  reinterpret_cast<const float4*>(d_half[1]), n,
                                                                  reinterpret_cast<float4*>(d_pixels));
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return hip_fail(hipGetErrorString(herr));
    if (out_tile_spp) memcpy(out_tile_spp, spp.data(), (size_t)4*ntiles);
    if (stats) {
        total.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *stats = total;
    }
    return done(RT_OK);
}

int rt_render_adaptive(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                       uint32_t tile_w, uint32_t tile_h, uint32_t total_frame_index, const rt_adaptive_params* p,
                       rt_accumulation_buffer* accum, uint32_t* out_tile_spp, rt_stats* stats) {
    const std::string e = "rt_render_adaptive";
    int err = check_adaptive_params(e, p);
    if (err) return err;
    if (!accum || !accum->pixels) return fail(RT_ERROR_INVALID, e + ": null accum");
    err = check_frame(e, accum->w, accum->h, tile_w, tile_h);
    if (err) return err;
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    if (!camera) return fail(RT_ERROR_INVALID, e + ": null camera");
    if (!st) return fail(RT_ERROR_INVALID, e + ": null settings");
    if (!filter) return fail(RT_ERROR_INVALID, e + ": null filter");
    err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t bytes = (size_t)16*accum->w*accum->h;
    float* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    if (hipMemcpy(d, accum->pixels, bytes, hipMemcpyHostToDevice) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_render_adaptive_device(s, camera, st, filter, tile_w, tile_h, total_frame_index, accum->w, accum->h,
                                              accum->frame_count, p, nullptr, d, out_tile_spp, nullptr, stats);
    if (!err && hipMemcpy(accum->pixels, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

}  // extern "C"
