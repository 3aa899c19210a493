// rt_robust.hip — the robust estimator: a Gini-adaptive median of means over a stack of accumulation buffers
// (rt_robust_combine_device, rt_robust_combine), the driver that renders the stack (rt_render_robust_device,
// rt_render_robust) and the picture entry on top of it (rt_render_picture_robust).  Beyond the reference
// (DESIGN.md §9), an opt-in: no other entry calls it.  The frames are rt_render_device's (rt_kernels.hip):
// nothing here touches a sample.
//
// The estimator is defined operation by operation in DESIGN.md ("The robust estimator"); tests/ref_robust/
// ref_robust.c restates it in plain C and k_robust_combine matches that checker bit for bit: IEEE f32, no
// contraction, division as /, and the additions in the stated orders.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"

namespace {

constexpr float VALID_W = 0.001f;       // k_post's resolve threshold
constexpr int RC_BLOCK = 256;
constexpr uint32_t RC_MAX_GRID = 2048;  // 8 blocks a CU; larger frames take the grid-stride loop
constexpr uint32_t RC_MIN_BUFFERS = 2, RC_MAX_BUFFERS = 32;
constexpr uint64_t RC_UNRANKED = ~0ull; // an invalid or padding slot: above every valid word

int fail(int code, const std::string& message) { rt_internal_set_error(message.c_str()); return code; }

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// An order-preserving image of a finite key in 32 bits, -0 as +0: negative keys with all bits flipped, the
// others with the sign bit set.  The largest image is 0xFF7FFFFF, below an unranked slot's all ones.
__device__ __forceinline__ uint32_t key_image(float key) {
    const uint32_t u = key == 0.0f ? 0u : __float_as_uint(key);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// max(key, 0) of an image: only keys > 0 enter the Gini sums
__device__ __forceinline__ float positive_key(uint32_t image) {
    return (image & 0x80000000u) ? __uint_as_float(image ^ 0x80000000u) : 0.0f;
}

__device__ __forceinline__ void compare_exchange(uint64_t& a, uint64_t& b) {
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// A bitonic network of P slots, ascending; every index is a compile-time constant once the loops are unrolled,
// so the words stay in registers.
template <int P>
__device__ __forceinline__ void sort_words(uint64_t (&word)[P]) {
#pragma unroll
    for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    if ((i & k) == 0) compare_exchange(word[i], word[l]);
                    else compare_exchange(word[l], word[i]);
                }
            }
        }
    }
}

// One thread per pixel (a grid-stride loop past RC_MAX_GRID blocks); the lanes of a wave take consecutive pixels, so
// each buffer's read is one contiguous float4 run.  P is the padded size of the ranking network, the smallest of
// {2, 4, 8, 16, 32} that holds `count`.  stack and out may alias (out may be a buffer of the stack): a thread reads
// all of its pixel before it writes it, and neither pointer is __restrict__.
template <int P>
__global__ void __launch_bounds__(RC_BLOCK) k_robust_combine(const float4* stack, uint32_t count, size_t n_pixels,
                                                             float gini_scale, uint32_t max_trim, float4* out,
                                                             float4* info) {
    for (size_t i = (size_t)blockIdx.x*RC_BLOCK + threadIdx.x; i < n_pixels; i += (size_t)gridDim.x*RC_BLOCK) {
        // 1. validity and the words to rank: the key's image above, the buffer index below
        uint64_t word[P];
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            word[k] = RC_UNRANKED;
            if ((uint32_t)k < count) {
                const float4 s = stack[(size_t)k*n_pixels + i];
                bool valid = s.w > VALID_W && finite_f(s.x) && finite_f(s.y) && finite_f(s.z) && finite_f(s.w);
                const float mr = s.x / s.w, mg = s.y / s.w, mb = s.z / s.w;
                const float key = (mr + mg) + mb;
                valid = valid && finite_f(mr) && finite_f(mg) && finite_f(mb) && finite_f(key);
                if (valid) {
                    word[k] = ((uint64_t)key_image(key) << 32) | (uint32_t)k;
                    n += 1u;
                }
            }
        }
        // 2. no valid buffer: buffer 0 as it is
        if (n == 0u) {
            const float4 s0 = stack[i];
            out[i] = s0;
            if (info) info[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        // 3. rank: the valid words come first, ascending by key, equal keys by buffer index
        sort_words<P>(word);
        // 4. the Gini coefficient of max(key, 0), summed in rank order
        float S = 0.0f, T = 0.0f;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            if ((uint32_t)r < n) {
                const float g = positive_key((uint32_t)(word[r] >> 32));
                S = S + g;
                T = T + (float)(r + 1)*g;
            }
        }
        float G = 0.0f;
        if (n >= 3u && finite_f(S) && S > 0.0f) G = (2.0f*T) / ((float)n*S) - (float)(n + 1u) / (float)n;
        if (!(G > 0.0f)) G = 0.0f;
        // 5. the trim count (x is >= 0 or NaN; NaN, from 0*inf, trims nothing)
        const uint32_t half = (n - 1u) / 2u;
        const uint32_t cmax = half < max_trim ? half : max_trim;
        const float x = (gini_scale*G) * ((float)n*0.5f);
        const uint32_t c = x >= (float)cmax ? cmax : (x >= 1.0f ? (uint32_t)floorf(x) : 0u);
        // 6. ranks c .. n-1-c as a mask over buffer indices (an index is < 32: no shift reaches 32)
        uint32_t kept = 0u;
#pragma unroll
        for (int r = 0; r < P; ++r)
            if ((uint32_t)r >= c && (uint32_t)r + c < n) kept |= 1u << ((uint32_t)word[r] & 31u);
        // the kept buffers again, in index order (L2 hits)
        float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if ((uint32_t)k < count && ((kept >> k) & 1u)) {
                const float4 s = stack[(size_t)k*n_pixels + i];
                nr = nr + s.x;
                ng = ng + s.y;
                nb = nb + s.z;
                den = den + s.w;
            }
        }
        out[i] = make_float4(nr / den, ng / den, nb / den, 1.0f);
        if (info) info[i] = make_float4(G, (float)c, (float)n, den);
    }
}

int check_combine(const std::string& e, const void* stack, uint32_t count, uint32_t w, uint32_t h, const rt_robust_params* p,
                  const void* out) {
    if (!stack) return fail(RT_ERROR_INVALID, e + ": null stack");
    if (!p) return fail(RT_ERROR_INVALID, e + ": null rt_robust_params");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null out");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if (count < RC_MIN_BUFFERS || count > RC_MAX_BUFFERS) return fail(RT_ERROR_INVALID, e + ": count must be 2..32");
    if (!(p->gini_scale >= 0.0f) || p->gini_scale > 3.402823466e38f)
        return fail(RT_ERROR_INVALID, e + ": rt_robust_params: gini_scale must be finite and >= 0");
    return RT_OK;
}

// every check of the drivers and the picture entry that needs no device
int check_driver(const std::string& e, const rt_scene* s, const rt_camera* camera, const rt_settings* st,
                 const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t w, uint32_t h, const rt_robust_params* p,
                 const void* out, const char* out_name) {
    // the parameters first and the scene last: what needs no scene is refused without one
    if (!p) return fail(RT_ERROR_INVALID, e + ": null rt_robust_params");
    if (p->buffers < RC_MIN_BUFFERS || p->buffers > RC_MAX_BUFFERS)
        return fail(RT_ERROR_INVALID, e + ": rt_robust_params: buffers must be 2..32");
    if (!(p->gini_scale >= 0.0f) || p->gini_scale > 3.402823466e38f)
        return fail(RT_ERROR_INVALID, e + ": rt_robust_params: gini_scale must be finite and >= 0");
    if (!st) return fail(RT_ERROR_INVALID, e + ": null settings");
    if (!st->samples_per_pixel || st->samples_per_pixel % p->buffers)
        return fail(RT_ERROR_INVALID, e + ": samples_per_pixel must be a multiple of rt_robust_params::buffers and > 0");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if (!camera) return fail(RT_ERROR_INVALID, e + ": null camera");
    if (!filter) return fail(RT_ERROR_INVALID, e + ": null filter");
    if (!tiles) return fail(RT_ERROR_INVALID, e + ": null tiles");
    // the driver shards the frame's sample passes itself (below)
    if (tiles->shard_count != 1u || tiles->shard_index != 0u)
        return fail(RT_ERROR_INVALID, e + ": tiles: shard_index must be 0 and shard_count 1 (the buffers are the frame's pass shards)");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null " + out_name);
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    return RT_OK;
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

template <int P>
void launch(uint32_t grid, hipStream_t stream, const float* d_stack, uint32_t count, size_t n, const rt_robust_params* p,
            float* d_out, float* d_info) {
    k_robust_combine<P><<<grid, RC_BLOCK, 0, stream>>>(reinterpret_cast<const float4*>(d_stack), count, n, p->gini_scale,
                                                       p->max_trim, reinterpret_cast<float4*>(d_out),
                                                       reinterpret_cast<float4*>(d_info));
}

}  // namespace

extern "C" {

int rt_robust_default_params(rt_robust_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_robust_default_params: null out");
    *out = {};
    out->buffers = 8;
    out->gini_scale = 1.0f;
    out->max_trim = 15;
    return RT_OK;
}

size_t rt_robust_workspace_bytes(uint32_t w, uint32_t h, uint32_t buffers) {
    return (size_t)buffers*w*h*16;
}

int rt_robust_combine_device(int device, const float* d_stack, uint32_t count, uint32_t w, uint32_t h,
                             const rt_robust_params* p, float* d_out, float* d_info, void* hip_stream) {
    int err = check_combine("rt_robust_combine_device", d_stack, count, w, h, p, d_out);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    const size_t blocks = (n + RC_BLOCK - 1) / RC_BLOCK;
    const uint32_t grid = blocks < RC_MAX_GRID ? (uint32_t)blocks : RC_MAX_GRID;
    // the smallest network that holds `count`; count itself stays a runtime value
    if (count <= 2u) launch<2>(grid, stream, d_stack, count, n, p, d_out, d_info);
    else if (count <= 4u) launch<4>(grid, stream, d_stack, count, n, p, d_out, d_info);
    else if (count <= 8u) launch<8>(grid, stream, d_stack, count, n, p, d_out, d_info);
    else if (count <= 16u) launch<16>(grid, stream, d_stack, count, n, p, d_out, d_info);
    else launch<32>(grid, stream, d_stack, count, n, p, d_out, d_info);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, std::string("rt_robust_combine_device: ") + hipGetErrorString(herr));
    return RT_OK;
}

int rt_robust_combine(int device, const float* stack, uint32_t count, uint32_t w, uint32_t h, const rt_robust_params* p,
                      float* out, float* info) {
    const std::string e = "rt_robust_combine";
    int err = check_combine(e, stack, count, w, h, p, out);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t bytes = (size_t)16*w*h;
    char* d_all = nullptr;                                  // the stack, the output, the info
    if (hipMalloc(&d_all, (size_t)count*bytes + 2*bytes) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_stack = reinterpret_cast<float*>(d_all);
    float* d_out = reinterpret_cast<float*>(d_all + (size_t)count*bytes);
    float* d_info = reinterpret_cast<float*>(d_all + (size_t)count*bytes + bytes);
    if (hipMemcpy(d_stack, stack, (size_t)count*bytes, hipMemcpyHostToDevice) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_robust_combine_device(device, d_stack, count, w, h, p, d_out, info ? d_info : nullptr, nullptr);
    if (!err && (hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                 (info && hipMemcpy(info, d_info, bytes, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d_all);
    return err;
}

int rt_render_robust_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                            const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                            uint32_t frame_count, const rt_robust_params* p, void* d_workspace, float* d_out, float* d_info,
                            void* hip_stream, rt_stats* stats) {
    const std::string e = "rt_render_robust_device";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, d_out, "d_out");
    if (err) return err;
    const auto t0 = std::chrono::steady_clock::now();
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    const uint32_t K = p->buffers;
    void* own = nullptr;
    if (!d_workspace) {
        if (hipMalloc(&own, rt_robust_workspace_bytes(w, h, K)) != hipSuccess)
            return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc of the workspace");
        d_workspace = own;
    }
    float* d_stack = static_cast<float*>(d_workspace);
    // Buffer k is shard k of K of the frame by sample passes: passes [k*spp/K, (k+1)*spp/K) of every tile, with the
    // frame's own frame_count in every seed.  (A frame of spp/K samples at frame_count + k*spp/K would take the same
    // canonical indices under other random streams: sample_seed hashes the frame's frame_count too.)  The scene's
    // shard mode is set for the call's frames and put back, whatever the outcome.
    rt_scene_config saved, by_pass;
    err = rt_scene_get_config(s, &saved);
    if (err) { if (own) (void)hipFree(own); return err; }
    by_pass = saved;
    by_pass.shard_mode = RT_SHARD_PASSES;
    err = rt_scene_set_config(s, &by_pass);
    if (err) { if (own) (void)hipFree(own); return err; }
    auto done = [&](int code) { (void)rt_scene_set_config(s, &saved); if (own) (void)hipFree(own); return code; };
    rt_stats total;
    memset(&total, 0, sizeof total);

    if (hipMemsetAsync(d_stack, 0, (size_t)K*n*16, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return done(fail(RT_ERROR_DEVICE, e + ": hipMemset"));
    for (uint32_t k = 0; k < K; ++k) {
        rt_stats fs;
        const rt_tile_set shard = {tiles->tile_w, tiles->tile_h, k, K};
        err = rt_render_device(s, camera, st, filter, &shard, total_frame_index, w, h, frame_count,
                               d_stack + (size_t)k*n*4, hip_stream, &fs);
        if (err) return done(err);
        add_stats(total, fs);
        // a frame clears the scene's cancel flag when its loop starts: one raised between two frames is seen here
        if (rt_internal_scene_cancelled(s)) return done(fail(RT_ERROR_CANCELLED, "render cancelled"));
    }
    err = rt_robust_combine_device(device, d_stack, K, w, h, p, d_out, d_info, hip_stream);
    if (err) return done(err);
    if (stats) {
        total.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *stats = total;
    }
    return done(RT_OK);
}

int rt_render_robust(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                     const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                     const rt_robust_params* p, float* out, float* info, rt_stats* stats) {
    const std::string e = "rt_render_robust";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, out, "out");
    if (err) return err;
    err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t bytes = (size_t)16*w*h;
    char* d = nullptr;                                      // the output, the info
    if (hipMalloc(&d, 2*bytes) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_out = reinterpret_cast<float*>(d);
    float* d_info = reinterpret_cast<float*>(d + bytes);
    err = rt_render_robust_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, nullptr, d_out,
                                  info ? d_info : nullptr, nullptr, stats);
    if (!err && (hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                 (info && hipMemcpy(info, d_info, bytes, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

int rt_render_picture_robust(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                             const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                             const rt_post_settings* post, const rt_robust_params* p, const rt_denoise_features_params* dp,
                             uint32_t guide_spp, uint32_t* out_bgra, rt_stats* stats) {
    const std::string e = "rt_render_picture_robust";
    if (!post) return fail(RT_ERROR_INVALID, e + ": null post");
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, out_bgra, "out_bgra");
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    // one allocation: the robust output (denoised in place), the three feature frames, the filter's workspace, the picture
    const size_t ws_bytes = dp ? rt_denoise_features_workspace_bytes(w, h) : 0;
    char* d_all = nullptr;
    if (hipMalloc(&d_all, 64*n + ws_bytes + 4*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_beauty = reinterpret_cast<float*>(d_all);
    float* d_feat[RT_FEATURE_COUNT];
    for (int f = 0; f < RT_FEATURE_COUNT; ++f) d_feat[f] = reinterpret_cast<float*>(d_all + 16*n*(size_t)(f + 1));
    void* d_ws = d_all + 64*n;
    uint32_t* d_pic = reinterpret_cast<uint32_t*>(d_all + 64*n + ws_bytes);
    if (hipMemset(d_all, 0, 64*n) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": hipMemset");
    if (!err) err = rt_render_robust_device(s, camera, st, filter, tiles, total_frame_index, w, h, 0u, p, nullptr, d_beauty,
                                            nullptr, nullptr, stats);
    if (!err && dp) {
        // the feature frames and the stage, as rt_render_picture_features_denoised runs them
        rt_settings gst = *st;
        if (guide_spp) gst.samples_per_pixel = guide_spp;
        rt_stats guide_stats;
        err = rt_render_features_device(s, camera, &gst, filter, tiles, total_frame_index, w, h, 0u, d_feat[RT_FEATURE_NORMAL],
                                        d_feat[RT_FEATURE_DISTANCE], d_feat[RT_FEATURE_ALBEDO], nullptr, &guide_stats);
        if (!err) err = rt_denoise_features_device(device, d_beauty, d_feat[RT_FEATURE_NORMAL], d_feat[RT_FEATURE_DISTANCE],
                                                   d_feat[RT_FEATURE_ALBEDO], w, h, dp, d_ws, d_beauty, nullptr);
    }
    // the dither texture of total_frame_index + 1, as rt_render_picture picks it
    if (!err) err = rt_postprocess_device(device, d_beauty, w, h, post, total_frame_index + 1u, d_pic, nullptr);
    if (!err && hipMemcpy(out_bgra, d_pic, 4*n, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d_all);
    return err;
}

}  // extern "C"
