// rt_svgf.hip — variance-guided filtering of the temporal history (after Schied et al., "Spatiotemporal
// Variance-Guided Filtering", HPG 2017, in this project's terms): the accumulate stage with the first two moments of
// the tonemapped luminance beside it (rt_temporal_accumulate_moments_device), the variance of the history from those
// moments (rt_temporal_variance_device), an à-trous filter whose colour term is scaled by that variance and whose
// edge-stopping terms come from the G-buffer (rt_denoise_variance_device), and the driver that runs one frame of
// the loop (rt_render_temporal_filtered_device).  Beyond the reference, an opt-in: no other entry
// calls it.
//
// The stage is defined operation by operation in DESIGN.md ("Variance-guided filtering"); tests/ref_svgf/
// ref_svgf.c restates it in plain C and the kernels below match that checker bit for bit: IEEE f32, no contraction,
// division as /, correctly rounded sqrt, the exponential d_expf (the oracle's oracle_expf), and the additions in
// the stated orders.  k_temporal_accumulate_moments' text is rt_temporal_shared.h's one accumulate body with the
// moments flag on and neither table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_dmath.h"
#include "rt_temporal_shared.h"   // the accumulate body and what the stage's entries and the drivers share on the host

namespace {

constexpr float INVALID_L = -1.0f;      // the filter's mark of an invalid pixel in {r, g, b, l}; l >= 0 otherwise
constexpr float INVALID_VAR = -1.0f;    // and in the variance buffer beside it; a valid variance is >= 0

// ---- 1. accumulate with moments: the shared body with {m1, m2} beside the history, and neither table

__global__ void __launch_bounds__(256) k_temporal_accumulate_moments(const float4* __restrict__ current,
                                                                     const rt_gbuffer_texel* __restrict__ gbuffer,
                                                                     const float4* __restrict__ prev_history,
                                                                     const float* __restrict__ prev_length,
                                                                     const rt_gbuffer_texel* __restrict__ prev_gbuffer,
                                                                     const float2* __restrict__ prev_moments, TaCamera cam,
                                                                     uint32_t w, uint32_t h, rt_temporal_params p,
                                                                     float4* __restrict__ history, float* __restrict__ length,
                                                                     float2* __restrict__ moments) {
    temporal_accumulate_body<true, false, false, false>(current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_moments, cam, w, h, p,
                                                 nullptr, 0u, nullptr, nullptr, 0u, history, length, moments, nullptr, TaClip{});
}

// ---- 2. the variance of the history

// One thread per pixel in the 64 x 4 block shape.  A pixel whose history is shorter than spatial_below gathers a
// 7 x 7 window of same-surface neighbours: a plain gather (after the first frames a few per cent of the pixels take
// it: DESIGN.md has the measured times of both regimes).
__global__ void __launch_bounds__(256) k_temporal_variance(const float2* __restrict__ moments, const float* __restrict__ length,
                                                           const rt_gbuffer_texel* __restrict__ gbuffer, uint32_t w, uint32_t h,
                                                           float normal_cos, float plane_tolerance, float spatial_below,
                                                           float* __restrict__ variance) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float len = length[i];
    if (!(len >= 1.0f)) { variance[i] = 0.0f; return; }
    float s2;
    if (len >= spatial_below) {
        const float2 m = moments[i];
        s2 = m.y - m.x*m.x;
    } else {
        const rt_gbuffer_texel g = gbuffer[i];
        const V3f n = v3_of(g.n), P = v3_of(g.p);
        const float plane_limit = plane_tolerance*g.t;
        float cnt = 0.0f, A1 = 0.0f, A2 = 0.0f;
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = (int)y + dy;
            if (qy < 0 || qy >= (int)h) continue;
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = (int)x + dx;
                if (qx < 0 || qx >= (int)w) continue;
                const size_t q = (size_t)qy*w + (size_t)qx;
                if (dx != 0 || dy != 0) {                   // the centre always counts
                    if (!(length[q] >= 1.0f)) continue;
                    const rt_gbuffer_texel gq = gbuffer[q];
                    if (gq.primitive != g.primitive) continue;
                    if (g.primitive != RT_HIT_MISS) {
                        if (!(dot3(n, v3_of(gq.n)) >= normal_cos)) continue;
                        const V3f off = {gq.p.x - P.x, gq.p.y - P.y, gq.p.z - P.z};
                        if (!(fabsf(dot3(off, n)) <= plane_limit)) continue;
                    }
                }
                const float2 m = moments[q];
                cnt = cnt + 1.0f;
                A1 = A1 + m.x;
                A2 = A2 + m.y;
            }
        }
        const float M1 = A1 / cnt, M2 = A2 / cnt;
        s2 = M2 - M1*M1;
    }
    s2 = s2 > 0.0f ? s2 : 0.0f;                             // NaN goes to 0
    variance[i] = s2 / len;
}

// ---- 3. the variance-guided filter

// Resolve, validity, clamp: colour -> c0 {r, g, b, l}, variance -> v0 (-1 marks an invalid pixel there; >= 0 otherwise).
__global__ void __launch_bounds__(256) k_svgf_prepare(const float4* __restrict__ color, const float* __restrict__ variance,
                                                      uint32_t w, uint32_t h, float firefly_clamp, float4* __restrict__ c0,
                                                      float* __restrict__ v0) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float4 s = color[i];
    const float var = variance[i];
    bool valid = s.w > VALID_W;
    float4 c = {0.0f, 0.0f, 0.0f, INVALID_L};
    if (valid) {
        c.x = s.x / s.w; c.y = s.y / s.w; c.z = s.z / s.w;
        valid = finite_f(c.x) && finite_f(c.y) && finite_f(c.z);
    }
    valid = valid && var >= 0.0f && finite_f(var);
    if (valid) {
        c.x = rtd::mx(c.x, 0.0f); c.y = rtd::mx(c.y, 0.0f); c.z = rtd::mx(c.z, 0.0f);
        if (firefly_clamp > 0.0f) { c.x = rtd::mn(c.x, firefly_clamp); c.y = rtd::mn(c.y, firefly_clamp); c.z = rtd::mn(c.z, firefly_clamp); }
        c.w = tm_of(c.x, c.y, c.z);
    } else {
        c = {0.0f, 0.0f, 0.0f, INVALID_L};
    }
    c0[i] = c;
    v0[i] = valid ? var : INVALID_VAR;
}

// One iteration at step s, one pixel per thread in the 64 x 4 block shape.  cin, vin -> cout, vout, or on the last
// iteration (out != nullptr) -> the output buffers: {c, 1} and the filtered variance for a valid pixel, the colour
// buffer's own four floats and the variance's own float for an invalid one (out may be the colour buffer and
// var_out the variance buffer: each thread reads only its own pixel of them).  A texel of the G-buffer is read as
// two 16-byte loads: {p, t} and {n, primitive}.  sigma_color, use_normal and use_plane (0: the term is off) are the
// same for every lane.
__global__ void __launch_bounds__(256) k_svgf_iterate(const float4* __restrict__ cin, const float* __restrict__ vin,
                                                      const float4* __restrict__ gbuffer, uint32_t w, uint32_t h, int step,
                                                      float sigma_color, float variance_epsilon, int use_normal, int use_plane,
                                                      float inv_n, float inv_z,
                                                      float4* __restrict__ cout, float* __restrict__ vout, const float4* color,
                                                      const float* variance, float4* out, float* var_out) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float4 cp = cin[i];
    if (cp.w < 0.0f) {                              // invalid: contributes nowhere, passes through unchanged
        if (out) {
            out[i] = color[i];
            if (var_out) var_out[i] = variance[i];
        } else {
            cout[i] = cp;
            vout[i] = INVALID_VAR;
        }
        return;
    }
    // the 3 x 3 Gaussian of the variance around p, at distance 1
    const float gk[3] = {1.0f/4.0f, 1.0f/2.0f, 1.0f/4.0f};
    float gsum = 0.0f, gvar = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)w) continue;
            const size_t q = (size_t)qy*w + (size_t)qx;
            const float vq = vin[q];
            if (vq < 0.0f) continue;
            const float g = gk[dy + 1]*gk[dx + 1];
            gvar += g*vq;
            gsum += g;
        }
    }
    const float gv = gvar / gsum;                   // the centre tap always counts: gsum >= 1/4
    const float inv_l = 1.0f / (sigma_color*__builtin_sqrtf(gv) + variance_epsilon);
    const float4 pa = gbuffer[2*i], pb = gbuffer[2*i + 1];       // {p, t}, {n, primitive}
    const bool p_miss = __float_as_uint(pb.w) == RT_HIT_MISS;
    const float hk[5] = {1.0f/16.0f, 1.0f/4.0f, 3.0f/8.0f, 1.0f/4.0f, 1.0f/16.0f};
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f, vnum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)y + step*dy;
        if (qy < 0 || qy >= (int)h) continue;       // the same for the whole wave: a wave is one row
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)x + step*dx;
            if (qx < 0 || qx >= (int)w) continue;
            const size_t q = (size_t)qy*w + (size_t)qx;
            const float4 cq = cin[q];
            if (cq.w < 0.0f) continue;
            const float4 qb = gbuffer[2*q + 1];
            if (p_miss != (__float_as_uint(qb.w) == RT_HIT_MISS)) continue;
            float e = 0.0f;
            if (sigma_color > 0.0f) e += fabsf(cp.w - cq.w)*inv_l;
            if (!p_miss) {
                if (use_normal) {
                    const float a = pb.x - qb.x, b = pb.y - qb.y, c = pb.z - qb.z;
                    e += ((a*a + b*b) + c*c)*inv_n;
                }
                if (use_plane) {
                    const float4 qa = gbuffer[2*q];
                    const float a = qa.x - pa.x, b = qa.y - pa.y, c = qa.z - pa.z;
                    const float z = ((a*pb.x + b*pb.y) + c*pb.z) / pa.w;
                    e += (z*z)*inv_z;
                }
            }
            const float wt = (hk[dy + 2]*hk[dx + 2])*rtd::d_expf(-e);
            nr += wt*cq.x; ng += wt*cq.y; nb += wt*cq.z;
            den += wt;
            vnum += (wt*wt)*vin[q];
        }
    }
    const float r = nr / den, g = ng / den, b = nb / den;     // the centre tap always counts: den >= 9/64
    const float v = vnum / (den*den);
    if (out) {
        out[i] = {r, g, b, 1.0f};
        if (var_out) var_out[i] = v;
    } else {
        cout[i] = {r, g, b, tm_of(r, g, b)};
        vout[i] = v;
    }
}

// the accumulate stage's checks, then the moments' (mandatory here: another rule than the motion stage's)
int check_moments(const std::string& e, const char* prefix, const TaArgs& a) {
    const std::string d = prefix;
    if (!a.moments) return fail(RT_ERROR_INVALID, e + ": null " + d + "moments");
    // all-or-none with the other three: check_accumulate names the one of those that is missing
    const bool any = a.prev_history || a.prev_length || a.prev_gbuffer || a.prev_moments;
    int err = check_accumulate(e, prefix, a);
    if (err) return err;
    if (any) {
        if (!a.prev_history) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_history beside other previous buffers");
        if (!a.prev_moments) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_moments beside other previous buffers");
        if (a.moments == a.prev_moments) return fail(RT_ERROR_INVALID, e + ": " + d + "moments aliases " + d + "prev_moments");
    }
    return RT_OK;
}

int check_spatial_below(const std::string& e, float spatial_below) {
    if (bad_value(spatial_below)) return fail(RT_ERROR_INVALID, e + ": spatial_below must be finite and >= 0");
    return RT_OK;
}

int check_variance(const std::string& e, const char* prefix, const void* moments, const void* length, const void* gbuffer,
                   uint32_t w, uint32_t h, const rt_temporal_params* p, float spatial_below, const void* variance) {
    const std::string d = prefix;
    if (!moments) return fail(RT_ERROR_INVALID, e + ": null " + d + "moments");
    if (!length) return fail(RT_ERROR_INVALID, e + ": null " + d + "length");
    if (!gbuffer) return fail(RT_ERROR_INVALID, e + ": null " + d + "gbuffer");
    if (!variance) return fail(RT_ERROR_INVALID, e + ": null " + d + "variance");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    int err = check_params(e, p);
    if (err) return err;
    err = check_spatial_below(e, spatial_below);
    if (err) return err;
    // a window reads its neighbours' moments and lengths
    if (variance == moments) return fail(RT_ERROR_INVALID, e + ": " + d + "variance aliases " + d + "moments");
    if (variance == length) return fail(RT_ERROR_INVALID, e + ": " + d + "variance aliases " + d + "length");
    if (variance == gbuffer) return fail(RT_ERROR_INVALID, e + ": " + d + "variance aliases " + d + "gbuffer");
    return RT_OK;
}

int check_filter_params(const std::string& e, const rt_denoise_variance_params* p) {
    if (!p) return fail(RT_ERROR_INVALID, e + ": null rt_denoise_variance_params");
    if (p->iterations < 1 || p->iterations > 8) return fail(RT_ERROR_INVALID, e + ": rt_denoise_variance_params: iterations must be in 1..8");
    if (bad_value(p->sigma_color)) return fail(RT_ERROR_INVALID, e + ": rt_denoise_variance_params: sigma_color must be finite and >= 0");
    if (bad_value(p->sigma_normal)) return fail(RT_ERROR_INVALID, e + ": rt_denoise_variance_params: sigma_normal must be finite and >= 0");
    if (bad_value(p->sigma_plane)) return fail(RT_ERROR_INVALID, e + ": rt_denoise_variance_params: sigma_plane must be finite and >= 0");
    if (bad_value(p->variance_epsilon) || !(p->variance_epsilon > 0.0f))
        return fail(RT_ERROR_INVALID, e + ": rt_denoise_variance_params: variance_epsilon must be finite and > 0");
    if (bad_value(p->firefly_clamp)) return fail(RT_ERROR_INVALID, e + ": rt_denoise_variance_params: firefly_clamp must be finite and >= 0");
    return RT_OK;
}

int check_filter(const std::string& e, const char* prefix, const void* color, const void* variance, const void* gbuffer,
                 uint32_t w, uint32_t h, const rt_denoise_variance_params* p, const void* out, const void* variance_out) {
    const std::string d = prefix;
    if (!color) return fail(RT_ERROR_INVALID, e + ": null " + d + "color");
    if (!variance) return fail(RT_ERROR_INVALID, e + ": null " + d + "variance");
    if (!gbuffer) return fail(RT_ERROR_INVALID, e + ": null " + d + "gbuffer");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null " + d + "out");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    int err = check_filter_params(e, p);
    if (err) return err;
    // out may be the colour and variance_out the variance (a thread reads only its own pixel of them); the G-buffer
    // is read at every tap of every iteration, and an output of one kind over an input of the other has no meaning
    if (out == variance) return fail(RT_ERROR_INVALID, e + ": " + d + "out aliases " + d + "variance");
    if (out == gbuffer) return fail(RT_ERROR_INVALID, e + ": " + d + "out aliases " + d + "gbuffer");
    if (variance_out) {
        if (variance_out == color) return fail(RT_ERROR_INVALID, e + ": " + d + "variance_out aliases " + d + "color");
        if (variance_out == gbuffer) return fail(RT_ERROR_INVALID, e + ": " + d + "variance_out aliases " + d + "gbuffer");
        if (variance_out == out) return fail(RT_ERROR_INVALID, e + ": " + d + "variance_out aliases " + d + "out");
    }
    return RT_OK;
}

// The driver's workspace, 180 bytes per pixel: the current frame, two G-buffers, two histories, the filter's
// workspace (40), two moments, two lengths, the variance.  Every float4 and texel run starts at a multiple of 16 n.
struct Workspace {
    float* current;
    rt_gbuffer_texel* gbuffer[2];
    float* history[2];
    void* filter;
    float* moments[2];
    float* length[2];
    float* variance;
};
Workspace carve(void* d_workspace, size_t n) {
    char* base = static_cast<char*>(d_workspace);
    Workspace ws;
    ws.current = reinterpret_cast<float*>(base);
    ws.filter = base + 112*n;
    for (int k = 0; k < 2; ++k) {
        ws.gbuffer[k] = reinterpret_cast<rt_gbuffer_texel*>(base + 16*n + (size_t)k*32*n);
        ws.history[k] = reinterpret_cast<float*>(base + 80*n + (size_t)k*16*n);
        ws.moments[k] = reinterpret_cast<float*>(base + 152*n + (size_t)k*8*n);
        ws.length[k] = reinterpret_cast<float*>(base + 168*n + (size_t)k*4*n);
    }
    ws.variance = reinterpret_cast<float*>(base + 176*n);
    return ws;
}

int check_driver(const std::string& e, const rt_scene* s, const rt_camera* camera, const rt_settings* st,
                 const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t w, uint32_t h, const rt_temporal_params* p,
                 float spatial_below, const rt_denoise_variance_params* fp, const rt_temporal_filtered_state* state,
                 const void* out, const char* out_name) {
    // the parameters first and the scene last: what needs no scene is refused without one
    int err = check_params(e, p);
    if (err) return err;
    err = check_spatial_below(e, spatial_below);
    if (err) return err;
    err = check_filter_params(e, fp);
    if (err) return err;
    if (!state) return fail(RT_ERROR_INVALID, e + ": null rt_temporal_filtered_state");
    if (!state->d_workspace) return fail(RT_ERROR_INVALID, e + ": rt_temporal_filtered_state: null d_workspace");
    if (state->parity > 1u) return fail(RT_ERROR_INVALID, e + ": rt_temporal_filtered_state: parity must be 0 or 1");
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

int rt_temporal_accumulate_moments_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                          const float* d_prev_history, const float* d_prev_length,
                                          const rt_gbuffer_texel* d_prev_gbuffer, const float* d_prev_moments,
                                          const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                          const rt_temporal_params* p, float* d_history, float* d_length, float* d_moments,
                                          void* hip_stream) {
    const std::string e = "rt_temporal_accumulate_moments_device";
    const TaArgs a = {d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera, prev_lens_distortion,
                      w, h, p, d_history, d_length, nullptr, 0u, d_prev_moments, d_moments};
    int err = check_moments(e, "d_", a);
    if (err) return err;
    return launch_accumulate(e, device, k_temporal_accumulate_moments, w, h, hip_stream, f4(d_current), d_gbuffer,
                             f4(d_prev_history), d_prev_length, d_prev_gbuffer, f2(d_prev_moments), ta_camera(a), w, h, *p,
                             f4(d_history), d_length, f2(d_moments));
}

int rt_temporal_accumulate_moments(int device, const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                   const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const float* prev_moments,
                                   const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                   const rt_temporal_params* p, float* history, float* length, float* moments) {
    const std::string e = "rt_temporal_accumulate_moments";
    int err = check_moments(e, "", {current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, prev_lens_distortion,
                                    w, h, p, history, length, nullptr, 0u, prev_moments, moments});
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    // the driver's layout: current, then the new set [0] and the previous set [1]
    const size_t n = (size_t)w*h;
    void* d_all = nullptr;
    if (hipMalloc(&d_all, rt_temporal_filtered_workspace_bytes(w, h)) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    const Workspace ws = carve(d_all, n);
    const bool prev = prev_history != nullptr;
    if (hipMemcpy(ws.current, current, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ws.gbuffer[0], gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
        (prev && (hipMemcpy(ws.history[1], prev_history, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(ws.length[1], prev_length, 4*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(ws.gbuffer[1], prev_gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(ws.moments[1], prev_moments, 8*n, hipMemcpyHostToDevice) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_temporal_accumulate_moments_device(device, ws.current, ws.gbuffer[0], prev ? ws.history[1] : nullptr,
                                                          prev ? ws.length[1] : nullptr, prev ? ws.gbuffer[1] : nullptr,
                                                          prev ? ws.moments[1] : nullptr, prev_camera, prev_lens_distortion, w, h,
                                                          p, ws.history[0], ws.length[0], ws.moments[0], nullptr);
    if (!err && (hipMemcpy(history, ws.history[0], 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(length, ws.length[0], 4*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(moments, ws.moments[0], 8*n, hipMemcpyDeviceToHost) != hipSuccess))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d_all);
    return err;
}

int rt_temporal_variance_device(int device, const float* d_moments, const float* d_length, const rt_gbuffer_texel* d_gbuffer,
                                uint32_t w, uint32_t h, const rt_temporal_params* p, float spatial_below, float* d_variance,
                                void* hip_stream) {
    int err = check_variance("rt_temporal_variance_device", "d_", d_moments, d_length, d_gbuffer, w, h, p, spatial_below, d_variance);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    k_temporal_variance<<<grid, 256, 0, stream>>>(reinterpret_cast<const float2*>(d_moments), d_length, d_gbuffer, w, h,
                                                  p->normal_cos, p->plane_tolerance, spatial_below, d_variance);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, std::string("rt_temporal_variance_device: ") + hipGetErrorString(herr));
    return RT_OK;
}

int rt_temporal_variance(int device, const float* moments, const float* length, const rt_gbuffer_texel* gbuffer, uint32_t w,
                         uint32_t h, const rt_temporal_params* p, float spatial_below, float* variance) {
    const std::string e = "rt_temporal_variance";
    int err = check_variance(e, "", moments, length, gbuffer, w, h, p, spatial_below, variance);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the G-buffer, the moments, the length, the variance
    if (hipMalloc(&d, 48*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    rt_gbuffer_texel* d_g = reinterpret_cast<rt_gbuffer_texel*>(d);
    float* d_m = reinterpret_cast<float*>(d + 32*n);
    float* d_l = reinterpret_cast<float*>(d + 40*n);
    float* d_v = reinterpret_cast<float*>(d + 44*n);
    if (hipMemcpy(d_g, gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_m, moments, 8*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_l, length, 4*n, hipMemcpyHostToDevice) != hipSuccess)
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_temporal_variance_device(device, d_m, d_l, d_g, w, h, p, spatial_below, d_v, nullptr);
    if (!err && hipMemcpy(variance, d_v, 4*n, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

int rt_denoise_variance_default_params(rt_denoise_variance_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_denoise_variance_default_params: null out");
    *out = {};
    // chosen on the CPU with the checker (DESIGN.md has the sweep; profiles/svgf_defaults.txt the whole of it)
    out->iterations = 4;
    out->sigma_color = 4.0f;
    out->sigma_normal = 0.2f;
    out->sigma_plane = 0.02f;
    out->variance_epsilon = 0.03f;
    out->firefly_clamp = 10.0f;
    return RT_OK;
}

size_t rt_denoise_variance_workspace_bytes(uint32_t w, uint32_t h) { return (size_t)40*w*h; }

int rt_denoise_variance_device(int device, const float* d_color, const float* d_variance, const rt_gbuffer_texel* d_gbuffer,
                               uint32_t w, uint32_t h, const rt_denoise_variance_params* p, void* d_workspace, float* d_out,
                               float* d_variance_out, void* hip_stream) {
    const std::string e = "rt_denoise_variance_device";
    int err = check_filter(e, "d_", d_color, d_variance, d_gbuffer, w, h, p, d_out, d_variance_out);
    if (err) return err;
    if (w > 65535u || h > 65535u) return fail(RT_ERROR_INVALID, e + ": w or h larger than 65535 pixels");
    if ((reinterpret_cast<uintptr_t>(d_gbuffer) & 15u) != 0u) return fail(RT_ERROR_INVALID, e + ": d_gbuffer is not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 15u) != 0u) return fail(RT_ERROR_INVALID, e + ": d_workspace is not 16-byte aligned");
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    void* own = nullptr;
    if (!d_workspace) {
        if (hipMalloc(&own, rt_denoise_variance_workspace_bytes(w, h)) != hipSuccess)
            return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc of the workspace");
        d_workspace = own;
    }
    float4* col[2] = {static_cast<float4*>(d_workspace), static_cast<float4*>(d_workspace) + n};
    float* var[2] = {reinterpret_cast<float*>(col[1] + n), reinterpret_cast<float*>(col[1] + n) + n};
    const float4* color = reinterpret_cast<const float4*>(d_color);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    k_svgf_prepare<<<grid, 256, 0, stream>>>(color, d_variance, w, h, p->firefly_clamp, col[0], var[0]);
    hipError_t herr = hipGetLastError();
    // the constants, in f32 as the checker computes them
    const float sn = p->sigma_normal, sz = p->sigma_plane;
    const float inv_n = sn > 0.0f ? 1.0f / (sn*sn) : 0.0f, inv_z = sz > 0.0f ? 1.0f / (sz*sz) : 0.0f;
    for (int i = 0; i < p->iterations && herr == hipSuccess; ++i) {
        const bool last = i + 1 == p->iterations;
        k_svgf_iterate<<<grid, 256, 0, stream>>>(col[i & 1], var[i & 1], reinterpret_cast<const float4*>(d_gbuffer), w, h, 1 << i,
                                                 p->sigma_color, p->variance_epsilon, sn > 0.0f ? 1 : 0, sz > 0.0f ? 1 : 0, inv_n, inv_z,
                                                 col[(i + 1) & 1],
                                                 var[(i + 1) & 1], color, d_variance,
                                                 last ? reinterpret_cast<float4*>(d_out) : nullptr, last ? d_variance_out : nullptr);
        herr = hipGetLastError();
    }
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (own) (void)hipFree(own);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, e + ": " + hipGetErrorString(herr));
    return RT_OK;
}

int rt_denoise_variance(int device, const float* color, const float* variance, const rt_gbuffer_texel* gbuffer, uint32_t w,
                        uint32_t h, const rt_denoise_variance_params* p, float* out, float* variance_out) {
    const std::string e = "rt_denoise_variance";
    int err = check_filter(e, "", color, variance, gbuffer, w, h, p, out, variance_out);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the colour (and the result, in place), the G-buffer, the variance (the same)
    if (hipMalloc(&d, 52*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_c = reinterpret_cast<float*>(d);
    rt_gbuffer_texel* d_g = reinterpret_cast<rt_gbuffer_texel*>(d + 16*n);
    float* d_v = reinterpret_cast<float*>(d + 48*n);
    if (hipMemcpy(d_c, color, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_g, gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_v, variance, 4*n, hipMemcpyHostToDevice) != hipSuccess)
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_denoise_variance_device(device, d_c, d_v, d_g, w, h, p, nullptr, d_c, variance_out ? d_v : nullptr, nullptr);
    if (!err && (hipMemcpy(out, d_c, 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (variance_out && hipMemcpy(variance_out, d_v, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

size_t rt_temporal_filtered_workspace_bytes(uint32_t w, uint32_t h) { return (size_t)180*w*h; }

int rt_render_temporal_filtered_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                       const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                                       uint32_t frame_count, const rt_temporal_params* p, float spatial_below,
                                       const rt_denoise_variance_params* fp, rt_temporal_filtered_state* state, float* d_out,
                                       float* d_history_out, float* d_length_out, float* d_variance_out, void* hip_stream,
                                       rt_stats* stats) {
    const std::string e = "rt_render_temporal_filtered_device";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, spatial_below, fp, state, d_out, "d_out");
    if (err) return err;
    if (w > 65535u || h > 65535u) return fail(RT_ERROR_INVALID, e + ": w or h larger than 65535 pixels");
    if ((reinterpret_cast<uintptr_t>(state->d_workspace) & 15u) != 0u)
        return fail(RT_ERROR_INVALID, e + ": rt_temporal_filtered_state: d_workspace is not 16-byte aligned");
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    const Workspace ws = carve(state->d_workspace, n);
    const uint32_t cur = state->parity, old = state->parity ^ 1u;
    // a state of another frame size restarts
    const bool prev = state->frames != 0u && state->w == w && state->h == h;

    rt_stats fs;
    err = render_current(e, s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    err = rt_gbuffer_device(s, camera, st->lens_distortion, w, h, ws.gbuffer[cur], hip_stream);
    if (err) return err;
    err = rt_temporal_accumulate_moments_device(device, ws.current, ws.gbuffer[cur], prev ? ws.history[old] : nullptr,
                                                prev ? ws.length[old] : nullptr, prev ? ws.gbuffer[old] : nullptr,
                                                prev ? ws.moments[old] : nullptr, &state->camera, state->lens_distortion, w, h, p,
                                                ws.history[cur], ws.length[cur], ws.moments[cur], hip_stream);
    if (err) return err;
    err = rt_temporal_variance_device(device, ws.moments[cur], ws.length[cur], ws.gbuffer[cur], w, h, p, spatial_below, ws.variance,
                                      hip_stream);
    if (err) return err;
    // the history the next frame reads stays the unfiltered one: the filter writes d_out only
    err = rt_denoise_variance_device(device, ws.history[cur], ws.variance, ws.gbuffer[cur], w, h, fp, ws.filter, d_out, nullptr,
                                     hip_stream);
    if (err) return err;
    if ((d_history_out && hipMemcpyAsync(d_history_out, ws.history[cur], 16*n, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        (d_length_out && hipMemcpyAsync(d_length_out, ws.length[cur], 4*n, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        (d_variance_out && hipMemcpyAsync(d_variance_out, ws.variance, 4*n, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": copy out");
    advance_state(state, w, h, camera, st);
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_render_temporal_filtered(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                                const rt_temporal_params* p, float spatial_below, const rt_denoise_variance_params* fp,
                                rt_temporal_filtered_state* state, float* out_pixels, float* out_history, float* out_length,
                                float* out_variance, rt_stats* stats) {
    const std::string e = "rt_render_temporal_filtered";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, spatial_below, fp, state, out_pixels, "out_pixels");
    if (err) return err;
    err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the picture, the history, the length, the variance
    if (hipMalloc(&d, 40*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_out = reinterpret_cast<float*>(d);
    float* d_hist = reinterpret_cast<float*>(d + 16*n);
    float* d_len = reinterpret_cast<float*>(d + 32*n);
    float* d_var = reinterpret_cast<float*>(d + 36*n);
    err = rt_render_temporal_filtered_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, spatial_below,
                                             fp, state, d_out, out_history ? d_hist : nullptr, out_length ? d_len : nullptr,
                                             out_variance ? d_var : nullptr, nullptr, stats);
    if (!err && (hipMemcpy(out_pixels, d_out, 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (out_history && hipMemcpy(out_history, d_hist, 16*n, hipMemcpyDeviceToHost) != hipSuccess) ||
                 (out_length && hipMemcpy(out_length, d_len, 4*n, hipMemcpyDeviceToHost) != hipSuccess) ||
                 (out_variance && hipMemcpy(out_variance, d_var, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

}  // extern "C"
