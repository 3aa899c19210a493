// rt_denoise.hip — the edge-avoiding à-trous wavelet denoiser (Dammertz, Sewtz, Hanika, Lensch, HPG 2010)
// between the accumulation buffer and the output pass: rt_denoise_device, rt_denoise,
// rt_render_picture_denoised.  Beyond the reference, an opt-in: no other entry calls it.
//
// The filter is defined operation by operation in DESIGN.md ("The denoise stage"); tests/ref_denoise/
// ref_denoise.c restates it in plain C and the kernels below match that checker bit for bit: IEEE f32, no
// contraction, division as /, the exponential d_expf (the oracle's oracle_expf).
//
// Workspace, 64 bytes per pixel: two colour buffers {r, g, b, l} that the iterations ping-pong, where l is
// the tonemapped luminance the colour term compares and l = -1 marks an invalid pixel (l >= 0 otherwise),
// and the two resolved guides {x, y, z, 0}.  A tap is one 16-byte load per buffer it needs; L2 serves the
// re-use between neighbours (DESIGN.md has the measured times).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_dmath.h"

using namespace rtd;

namespace {

constexpr float VALID_W = 0.001f;       // k_post's resolve threshold
constexpr float INVALID_L = -1.0f;

int fail(int code, const std::string& message) { rt_internal_set_error(message.c_str()); return code; }
#define DN_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(RT_ERROR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

RT_D bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
RT_D float luma_l(float r, float g, float b) {
    const float y = 0.2126f*r + 0.7152f*g + 0.0722f*b;
    return 1.0f - d_expf(-y);
}

// Resolve, validity, clamp: beauty -> c0 {r, g, b, l}; guides -> {x, y, z, 0}.
__global__ void __launch_bounds__(256) k_denoise_prepare(const float4* __restrict__ beauty, const float4* __restrict__ guide0,
                                                         const float4* __restrict__ guide1, uint32_t w, uint32_t h,
                                                         float firefly_clamp, float4* __restrict__ c0,
                                                         float4* __restrict__ g0, float4* __restrict__ g1) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float4 s = beauty[i];
    bool valid = s.w > VALID_W;
    float4 c = {0.0f, 0.0f, 0.0f, INVALID_L};
    if (valid) {
        c.x = s.x / s.w; c.y = s.y / s.w; c.z = s.z / s.w;
        valid = finite_f(c.x) && finite_f(c.y) && finite_f(c.z);
    }
    if (guide0) {
        const float4 g = guide0[i];
        float4 r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g.w > VALID_W) {
            r.x = g.x / g.w; r.y = g.y / g.w; r.z = g.z / g.w;
            valid = valid && finite_f(r.x) && finite_f(r.y) && finite_f(r.z);
        } else valid = false;
        g0[i] = r;
    }
    if (guide1) {
        const float4 g = guide1[i];
        float4 r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g.w > VALID_W) {
            r.x = g.x / g.w; r.y = g.y / g.w; r.z = g.z / g.w;
            valid = valid && finite_f(r.x) && finite_f(r.y) && finite_f(r.z);
        } else valid = false;
        g1[i] = r;
    }
    if (valid) {
        c.x = mx(c.x, 0.0f); c.y = mx(c.y, 0.0f); c.z = mx(c.z, 0.0f);
        if (firefly_clamp > 0.0f) { c.x = mn(c.x, firefly_clamp); c.y = mn(c.y, firefly_clamp); c.z = mn(c.z, firefly_clamp); }
        c.w = luma_l(c.x, c.y, c.z);
    } else {
        c = {0.0f, 0.0f, 0.0f, INVALID_L};
    }
    c0[i] = c;
}

// One à-trous iteration at step s, one pixel per thread in k_post's 64 x 4 block shape.  cin -> cout, or on
// the last iteration (out != nullptr) -> the output buffer: {c, 1} for a valid pixel, the beauty pixel's own
// four floats for an invalid one (out may be the beauty buffer: each thread reads only its own pixel of it).
// use_color, g0 and g1 (nullptr: the term is off) are the same for every lane.
__global__ void __launch_bounds__(256) k_denoise_iterate(const float4* __restrict__ cin, const float4* __restrict__ g0,
                                                         const float4* __restrict__ g1, uint32_t w, uint32_t h, int step,
                                                         int use_color, float inv_c, float inv_g0, float inv_g1,
                                                         float4* __restrict__ cout, const float4* beauty, float4* out) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float4 cp = cin[i];
    if (cp.w < 0.0f) {                              // invalid: contributes nowhere, passes through unchanged
        if (out) out[i] = beauty[i];
        else cout[i] = cp;
        return;
    }
    float4 gp0 = {0.0f, 0.0f, 0.0f, 0.0f}, gp1 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (g0) gp0 = g0[i];
    if (g1) gp1 = g1[i];
    const float hk[5] = {1.0f/16.0f, 1.0f/4.0f, 3.0f/8.0f, 1.0f/4.0f, 1.0f/16.0f};
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
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
            float e = 0.0f;
            if (use_color) {
                const float d = cp.w - cq.w;
                e += (d*d)*inv_c;
            }
            if (g0) {
                const float4 gq = g0[q];
                const float a = gp0.x - gq.x, b = gp0.y - gq.y, c = gp0.z - gq.z;
                e += (a*a + b*b + c*c)*inv_g0;
            }
            if (g1) {
                const float4 gq = g1[q];
                const float a = gp1.x - gq.x, b = gp1.y - gq.y, c = gp1.z - gq.z;
                e += (a*a + b*b + c*c)*inv_g1;
            }
            const float wt = (hk[dy + 2]*hk[dx + 2])*d_expf(-e);
            nr += wt*cq.x; ng += wt*cq.y; nb += wt*cq.z;
            den += wt;
        }
    }
    const float r = nr / den, g = ng / den, b = nb / den;     // the centre tap always counts: den >= 9/64
    if (out) out[i] = {r, g, b, 1.0f};
    else cout[i] = {r, g, b, luma_l(r, g, b)};
}

// The stage with feature frames (rt_denoise_features_device): the two kernels above with an albedo buffer.
// Kernels of their own, so rt_denoise_device's keep their code.  The workspace grows by the resolved albedo
// {r, g, b, 0}: 80 bytes per pixel.  With albedo == nullptr and demodulate 0 every operation is the one above.
RT_D float4 resolve_guide(const float4 g, bool& valid) {
    float4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (g.w > VALID_W) {
        r.x = g.x / g.w; r.y = g.y / g.w; r.z = g.z / g.w;
        valid = valid && finite_f(r.x) && finite_f(r.y) && finite_f(r.z);
    } else valid = false;
    return r;
}

__global__ void __launch_bounds__(256) k_denoise_features_prepare(const float4* __restrict__ beauty, const float4* __restrict__ guide0,
                                                                  const float4* __restrict__ guide1, const float4* __restrict__ albedo,
                                                                  uint32_t w, uint32_t h, float firefly_clamp, int demodulate,
                                                                  float albedo_floor, float4* __restrict__ c0, float4* __restrict__ g0,
                                                                  float4* __restrict__ g1, float4* __restrict__ al) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float4 s = beauty[i];
    bool valid = s.w > VALID_W;
    float4 c = {0.0f, 0.0f, 0.0f, INVALID_L};
    if (valid) {
        c.x = s.x / s.w; c.y = s.y / s.w; c.z = s.z / s.w;
        valid = finite_f(c.x) && finite_f(c.y) && finite_f(c.z);
    }
    if (guide0) g0[i] = resolve_guide(guide0[i], valid);
    if (guide1) g1[i] = resolve_guide(guide1[i], valid);
    float4 a = {0.0f, 0.0f, 0.0f, 0.0f};
    if (albedo) { a = resolve_guide(albedo[i], valid); al[i] = a; }
    if (valid) {
        c.x = mx(c.x, 0.0f); c.y = mx(c.y, 0.0f); c.z = mx(c.z, 0.0f);
        if (firefly_clamp > 0.0f) { c.x = mn(c.x, firefly_clamp); c.y = mn(c.y, firefly_clamp); c.z = mn(c.z, firefly_clamp); }
        if (demodulate) {
            c.x = c.x / mx(a.x, albedo_floor); c.y = c.y / mx(a.y, albedo_floor); c.z = c.z / mx(a.z, albedo_floor);
        }
        c.w = luma_l(c.x, c.y, c.z);
    } else {
        c = {0.0f, 0.0f, 0.0f, INVALID_L};
    }
    c0[i] = c;
}

// al: the resolved albedo, compared when use_albedo (sigma_albedo > 0) and multiplied back into the output of the
// last iteration when demodulate; nullptr when neither.
__global__ void __launch_bounds__(256) k_denoise_features_iterate(const float4* __restrict__ cin, const float4* __restrict__ g0,
                                                                  const float4* __restrict__ g1, const float4* __restrict__ al,
                                                                  uint32_t w, uint32_t h, int step, int use_color, int use_albedo,
                                                                  int demodulate, float inv_c, float inv_g0, float inv_g1,
                                                                  float inv_a, float albedo_floor, float4* __restrict__ cout,
                                                                  const float4* beauty, float4* out) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float4 cp = cin[i];
    if (cp.w < 0.0f) {                              // invalid: contributes nowhere, passes through unchanged
        if (out) out[i] = beauty[i];
        else cout[i] = cp;
        return;
    }
    float4 gp0 = {0.0f, 0.0f, 0.0f, 0.0f}, gp1 = {0.0f, 0.0f, 0.0f, 0.0f}, ap = {0.0f, 0.0f, 0.0f, 0.0f};
    if (g0) gp0 = g0[i];
    if (g1) gp1 = g1[i];
    if (al) ap = al[i];
    const float hk[5] = {1.0f/16.0f, 1.0f/4.0f, 3.0f/8.0f, 1.0f/4.0f, 1.0f/16.0f};
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
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
            float e = 0.0f;
            if (use_color) {
                const float d = cp.w - cq.w;
                e += (d*d)*inv_c;
            }
            if (g0) {
                const float4 gq = g0[q];
                const float a = gp0.x - gq.x, b = gp0.y - gq.y, c = gp0.z - gq.z;
                e += (a*a + b*b + c*c)*inv_g0;
            }
            if (g1) {
                const float4 gq = g1[q];
                const float a = gp1.x - gq.x, b = gp1.y - gq.y, c = gp1.z - gq.z;
                e += (a*a + b*b + c*c)*inv_g1;
            }
            if (use_albedo) {
                const float4 aq = al[q];
                const float a = ap.x - aq.x, b = ap.y - aq.y, c = ap.z - aq.z;
                e += (a*a + b*b + c*c)*inv_a;
            }
            const float wt = (hk[dy + 2]*hk[dx + 2])*d_expf(-e);
            nr += wt*cq.x; ng += wt*cq.y; nb += wt*cq.z;
            den += wt;
        }
    }
    float r = nr / den, g = ng / den, b = nb / den;           // the centre tap always counts: den >= 9/64
    if (out) {
        if (demodulate) { r = r*mx(ap.x, albedo_floor); g = g*mx(ap.y, albedo_floor); b = b*mx(ap.z, albedo_floor); }
        out[i] = {r, g, b, 1.0f};
    } else cout[i] = {r, g, b, luma_l(r, g, b)};
}

bool bad_value(float v) { return !(v >= 0.0f) || v > 3.402823466e38f; }   // negative, NaN or infinite

int check_params(const rt_denoise_params* p, bool has_guide0, bool has_guide1) {
    if (!p) return fail(RT_ERROR_INVALID, "rt_denoise: null rt_denoise_params");
    if (p->iterations < 1 || p->iterations > 8) return fail(RT_ERROR_INVALID, "rt_denoise_params: iterations must be in 1..8");
    if (bad_value(p->sigma_color)) return fail(RT_ERROR_INVALID, "rt_denoise_params: sigma_color must be finite and >= 0");
    if (bad_value(p->sigma_guide[0])) return fail(RT_ERROR_INVALID, "rt_denoise_params: sigma_guide[0] must be finite and >= 0");
    if (bad_value(p->sigma_guide[1])) return fail(RT_ERROR_INVALID, "rt_denoise_params: sigma_guide[1] must be finite and >= 0");
    if (bad_value(p->firefly_clamp)) return fail(RT_ERROR_INVALID, "rt_denoise_params: firefly_clamp must be finite and >= 0");
    if (p->sigma_guide[0] > 0.0f && !has_guide0) return fail(RT_ERROR_INVALID, "rt_denoise_params: sigma_guide[0] is set but guide0 is absent");
    if (p->sigma_guide[1] > 0.0f && !has_guide1) return fail(RT_ERROR_INVALID, "rt_denoise_params: sigma_guide[1] is set but guide1 is absent");
    return RT_OK;
}

int check_features_params(const rt_denoise_features_params* p, bool has_normal, bool has_distance, bool has_albedo) {
    if (!p) return fail(RT_ERROR_INVALID, "rt_denoise_features: null rt_denoise_features_params");
    int err = check_params(&p->base, has_normal, has_distance);
    if (err) return err;
    if (bad_value(p->sigma_albedo)) return fail(RT_ERROR_INVALID, "rt_denoise_features_params: sigma_albedo must be finite and >= 0");
    if (p->demodulate != 0 && p->demodulate != 1) return fail(RT_ERROR_INVALID, "rt_denoise_features_params: demodulate must be 0 or 1");
    if (p->demodulate && (bad_value(p->albedo_floor) || !(p->albedo_floor > 0.0f)))
        return fail(RT_ERROR_INVALID, "rt_denoise_features_params: albedo_floor must be finite and > 0 when demodulate is set");
    if (p->sigma_albedo > 0.0f && !has_albedo) return fail(RT_ERROR_INVALID, "rt_denoise_features_params: sigma_albedo is set but the albedo is absent");
    if (p->demodulate && !has_albedo) return fail(RT_ERROR_INVALID, "rt_denoise_features_params: demodulate is set but the albedo is absent");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise_default_params(rt_denoise_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_denoise_default_params: null out");
    *out = {};
    // chosen on the CPU with the checker (DESIGN.md has the error table): guide 0 = normals, guide 1 = distances
    out->iterations = 3;
    out->sigma_color = 1.0f;
    out->sigma_guide[0] = 0.1f;
    out->sigma_guide[1] = 0.05f;
    out->firefly_clamp = 10.0f;
    return RT_OK;
}

size_t rt_denoise_workspace_bytes(uint32_t w, uint32_t h) { return (size_t)64*w*h; }

int rt_denoise_device(int device, const float* d_beauty, const float* d_guide0, const float* d_guide1,
                      uint32_t w, uint32_t h, const rt_denoise_params* p, void* d_workspace, float* d_out,
                      void* hip_stream) {
    if (!d_beauty) return fail(RT_ERROR_INVALID, "rt_denoise_device: null d_beauty");
    if (!d_out) return fail(RT_ERROR_INVALID, "rt_denoise_device: null d_out");
    if (!w) return fail(RT_ERROR_INVALID, "rt_denoise_device: w is 0");
    if (!h) return fail(RT_ERROR_INVALID, "rt_denoise_device: h is 0");
    int err = check_params(p, d_guide0 != nullptr, d_guide1 != nullptr);
    if (err) return err;
    if (w > 65535u || h > 65535u) return fail(RT_ERROR_INVALID, "rt_denoise_device: w or h larger than 65535 pixels");
    err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    void* own = nullptr;
    if (!d_workspace) {
        if (hipMalloc(&own, rt_denoise_workspace_bytes(w, h)) != hipSuccess)
            return fail(RT_ERROR_OUT_OF_MEMORY, "rt_denoise_device: hipMalloc of the workspace");
        d_workspace = own;
    }
    float4* col[2] = {static_cast<float4*>(d_workspace), static_cast<float4*>(d_workspace) + n};
    float4* g0 = d_guide0 ? static_cast<float4*>(d_workspace) + 2*n : nullptr;
    float4* g1 = d_guide1 ? static_cast<float4*>(d_workspace) + 3*n : nullptr;
    const float4* beauty = reinterpret_cast<const float4*>(d_beauty);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    k_denoise_prepare<<<grid, 256, 0, stream>>>(beauty, reinterpret_cast<const float4*>(d_guide0),
                                                reinterpret_cast<const float4*>(d_guide1), w, h, p->firefly_clamp,
                                                col[0], g0, g1);
    hipError_t herr = hipGetLastError();
    // the constants, in f32 as the checker computes them
    const float sg0 = p->sigma_guide[0], sg1 = p->sigma_guide[1];
    const float inv_g0 = sg0 > 0.0f ? 1.0f / (sg0*sg0) : 0.0f, inv_g1 = sg1 > 0.0f ? 1.0f / (sg1*sg1) : 0.0f;
    float scale = 1.0f;                                     // 2^-i
    for (int i = 0; i < p->iterations && herr == hipSuccess; ++i, scale = scale*0.5f) {
        const bool last = i + 1 == p->iterations;
        float inv_c = 0.0f;
        if (p->sigma_color > 0.0f) { const float sc = p->sigma_color*scale; inv_c = 1.0f / (sc*sc); }
        k_denoise_iterate<<<grid, 256, 0, stream>>>(col[i & 1], sg0 > 0.0f ? g0 : nullptr, sg1 > 0.0f ? g1 : nullptr, w, h,
                                                    1 << i, p->sigma_color > 0.0f ? 1 : 0, inv_c, inv_g0, inv_g1,
                                                    col[(i + 1) & 1], beauty, last ? reinterpret_cast<float4*>(d_out) : nullptr);
        herr = hipGetLastError();
    }
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (own) (void)hipFree(own);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, std::string("rt_denoise_device: ") + hipGetErrorString(herr));
    return RT_OK;
}

int rt_denoise(int device, const rt_accumulation_buffer* beauty, const float* guide0, const float* guide1,
               const rt_denoise_params* p, float* out_pixels) {
    if (!beauty || !beauty->pixels) return fail(RT_ERROR_INVALID, "rt_denoise: null beauty");
    if (!out_pixels) return fail(RT_ERROR_INVALID, "rt_denoise: null out_pixels");
    if (!beauty->w) return fail(RT_ERROR_INVALID, "rt_denoise: beauty->w is 0");
    if (!beauty->h) return fail(RT_ERROR_INVALID, "rt_denoise: beauty->h is 0");
    int err = check_params(p, guide0 != nullptr, guide1 != nullptr);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const uint32_t w = beauty->w, h = beauty->h;
    const size_t bytes = (size_t)16*w*h;
    float* d[3] = {nullptr, nullptr, nullptr};              // beauty (and the result, in place), guide 0, guide 1
    const float* src[3] = {beauty->pixels, guide0, guide1};
    for (int k = 0; k < 3 && !err; ++k) {
        if (!src[k]) continue;
        if (hipMalloc(&d[k], bytes) != hipSuccess) err = fail(RT_ERROR_OUT_OF_MEMORY, "rt_denoise: hipMalloc");
        else if (hipMemcpy(d[k], src[k], bytes, hipMemcpyHostToDevice) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_denoise: copy in");
    }
    if (!err) err = rt_denoise_device(device, d[0], d[1], d[2], w, h, p, nullptr, d[0], nullptr);
    if (!err && hipMemcpy(out_pixels, d[0], bytes, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_denoise: copy out");
    for (int k = 0; k < 3; ++k) if (d[k]) (void)hipFree(d[k]);
    return err;
}

int rt_render_picture_denoised(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                               const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                               const rt_post_settings* post, const rt_denoise_params* p, uint32_t guide_spp,
                               uint32_t* out_bgra, rt_stats* stats) {
    if (!s) return fail(RT_ERROR_INVALID, "rt_render_picture_denoised: null scene");
    if (!st) return fail(RT_ERROR_INVALID, "rt_render_picture_denoised: null settings");
    if (!post) return fail(RT_ERROR_INVALID, "rt_render_picture_denoised: null post");
    if (!out_bgra) return fail(RT_ERROR_INVALID, "rt_render_picture_denoised: null out_bgra");
    if (!w) return fail(RT_ERROR_INVALID, "rt_render_picture_denoised: w is 0");
    if (!h) return fail(RT_ERROR_INVALID, "rt_render_picture_denoised: h is 0");
    int err = check_params(p, true, true);
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    // one allocation: beauty (denoised in place), normals, distances, the filter's workspace, the picture
    char* d_all = nullptr;
    const size_t ws_bytes = rt_denoise_workspace_bytes(w, h);
    if (hipMalloc(&d_all, 48*n + ws_bytes + 4*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, "rt_render_picture_denoised: hipMalloc");
    float* d_beauty = reinterpret_cast<float*>(d_all);
    float* d_normals = reinterpret_cast<float*>(d_all + 16*n);
    float* d_distances = reinterpret_cast<float*>(d_all + 32*n);
    void* d_ws = d_all + 48*n;
    uint32_t* d_pic = reinterpret_cast<uint32_t*>(d_all + 48*n + ws_bytes);
    if (hipMemset(d_all, 0, 48*n) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_render_picture_denoised: hipMemset");
    // the beauty frame as rt_render_picture renders it: a fresh buffer, frame_count 0
    if (!err) err = rt_render_device(s, camera, st, filter, tiles, total_frame_index, w, h, 0u, d_beauty, nullptr, stats);
    // the guide frames: the same camera, filter, tiles and frame index, first-hit integrators
    rt_settings gst = *st;
    if (guide_spp) gst.samples_per_pixel = guide_spp;
    rt_stats guide_stats;
    gst.integrator = RT_INTEGRATOR_NORMALS;
    if (!err) err = rt_render_device(s, camera, &gst, filter, tiles, total_frame_index, w, h, 0u, d_normals, nullptr, &guide_stats);
    gst.integrator = RT_INTEGRATOR_DISTANCES;
    if (!err) err = rt_render_device(s, camera, &gst, filter, tiles, total_frame_index, w, h, 0u, d_distances, nullptr, &guide_stats);
    if (!err) err = rt_denoise_device(device, d_beauty, d_normals, d_distances, w, h, p, d_ws, d_beauty, nullptr);
    // the dither texture of total_frame_index + 1, as rt_render_picture picks it
    if (!err) err = rt_postprocess_device(device, d_beauty, w, h, post, total_frame_index + 1u, d_pic, nullptr);
    if (!err && hipMemcpy(out_bgra, d_pic, 4*n, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_render_picture_denoised: copy out");
    (void)hipFree(d_all);
    return err;
}

int rt_denoise_features_default_params(rt_denoise_features_params* out) {
    if (!out) return fail(RT_ERROR_INVALID, "rt_denoise_features_default_params: null out");
    *out = {};
    rt_denoise_default_params(&out->base);
    // chosen on the CPU with the checker (DESIGN.md has the sweep): the albedo as a third edge-stopping term;
    // demodulation lost to it on the three presets' tonemapped error and stays off (its floor is the value a
    // caller who switches it on starts from: the sweep's four floors gave the same figures)
    out->sigma_albedo = 0.2f;
    out->demodulate = 0;
    out->albedo_floor = 0.05f;
    return RT_OK;
}

size_t rt_denoise_features_workspace_bytes(uint32_t w, uint32_t h) { return (size_t)80*w*h; }

int rt_denoise_features_device(int device, const float* d_beauty, const float* d_normal, const float* d_distance,
                               const float* d_albedo, uint32_t w, uint32_t h, const rt_denoise_features_params* fpar,
                               void* d_workspace, float* d_out, void* hip_stream) {
    if (!d_beauty) return fail(RT_ERROR_INVALID, "rt_denoise_features_device: null d_beauty");
    if (!d_out) return fail(RT_ERROR_INVALID, "rt_denoise_features_device: null d_out");
    if (!w) return fail(RT_ERROR_INVALID, "rt_denoise_features_device: w is 0");
    if (!h) return fail(RT_ERROR_INVALID, "rt_denoise_features_device: h is 0");
    int err = check_features_params(fpar, d_normal != nullptr, d_distance != nullptr, d_albedo != nullptr);
    if (err) return err;
    if (w > 65535u || h > 65535u) return fail(RT_ERROR_INVALID, "rt_denoise_features_device: w or h larger than 65535 pixels");
    err = rt_internal_bind_device(device);
    if (err) return err;
    const rt_denoise_params* p = &fpar->base;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    void* own = nullptr;
    if (!d_workspace) {
        if (hipMalloc(&own, rt_denoise_features_workspace_bytes(w, h)) != hipSuccess)
            return fail(RT_ERROR_OUT_OF_MEMORY, "rt_denoise_features_device: hipMalloc of the workspace");
        d_workspace = own;
    }
    float4* col[2] = {static_cast<float4*>(d_workspace), static_cast<float4*>(d_workspace) + n};
    float4* g0 = d_normal ? static_cast<float4*>(d_workspace) + 2*n : nullptr;
    float4* g1 = d_distance ? static_cast<float4*>(d_workspace) + 3*n : nullptr;
    float4* al = d_albedo ? static_cast<float4*>(d_workspace) + 4*n : nullptr;
    const float4* beauty = reinterpret_cast<const float4*>(d_beauty);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    k_denoise_features_prepare<<<grid, 256, 0, stream>>>(beauty, reinterpret_cast<const float4*>(d_normal),
                                                         reinterpret_cast<const float4*>(d_distance),
                                                         reinterpret_cast<const float4*>(d_albedo), w, h, p->firefly_clamp,
                                                         fpar->demodulate, fpar->albedo_floor, col[0], g0, g1, al);
    hipError_t herr = hipGetLastError();
    // the constants, in f32 as the checker computes them
    const float sg0 = p->sigma_guide[0], sg1 = p->sigma_guide[1], sa = fpar->sigma_albedo;
    const float inv_g0 = sg0 > 0.0f ? 1.0f / (sg0*sg0) : 0.0f, inv_g1 = sg1 > 0.0f ? 1.0f / (sg1*sg1) : 0.0f;
    const float inv_a = sa > 0.0f ? 1.0f / (sa*sa) : 0.0f;
    const bool need_al = sa > 0.0f || fpar->demodulate;
    float scale = 1.0f;                                     // 2^-i
    for (int i = 0; i < p->iterations && herr == hipSuccess; ++i, scale = scale*0.5f) {
        const bool last = i + 1 == p->iterations;
        float inv_c = 0.0f;
        if (p->sigma_color > 0.0f) { const float sc = p->sigma_color*scale; inv_c = 1.0f / (sc*sc); }
        k_denoise_features_iterate<<<grid, 256, 0, stream>>>(col[i & 1], sg0 > 0.0f ? g0 : nullptr, sg1 > 0.0f ? g1 : nullptr,
                                                             need_al ? al : nullptr, w, h, 1 << i, p->sigma_color > 0.0f ? 1 : 0,
                                                             sa > 0.0f ? 1 : 0, fpar->demodulate, inv_c, inv_g0, inv_g1, inv_a,
                                                             fpar->albedo_floor, col[(i + 1) & 1], beauty,
                                                             last ? reinterpret_cast<float4*>(d_out) : nullptr);
        herr = hipGetLastError();
    }
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (own) (void)hipFree(own);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, std::string("rt_denoise_features_device: ") + hipGetErrorString(herr));
    return RT_OK;
}

int rt_denoise_features(int device, const rt_accumulation_buffer* beauty, const float* normal, const float* distance,
                        const float* albedo, const rt_denoise_features_params* p, float* out_pixels) {
    if (!beauty || !beauty->pixels) return fail(RT_ERROR_INVALID, "rt_denoise_features: null beauty");
    if (!out_pixels) return fail(RT_ERROR_INVALID, "rt_denoise_features: null out_pixels");
    if (!beauty->w) return fail(RT_ERROR_INVALID, "rt_denoise_features: beauty->w is 0");
    if (!beauty->h) return fail(RT_ERROR_INVALID, "rt_denoise_features: beauty->h is 0");
    int err = check_features_params(p, normal != nullptr, distance != nullptr, albedo != nullptr);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const uint32_t w = beauty->w, h = beauty->h;
    const size_t bytes = (size_t)16*w*h;
    float* d[4] = {nullptr, nullptr, nullptr, nullptr};     // beauty (and the result, in place), normal, distance, albedo
    const float* src[4] = {beauty->pixels, normal, distance, albedo};
    for (int k = 0; k < 4 && !err; ++k) {
        if (!src[k]) continue;
        if (hipMalloc(&d[k], bytes) != hipSuccess) err = fail(RT_ERROR_OUT_OF_MEMORY, "rt_denoise_features: hipMalloc");
        else if (hipMemcpy(d[k], src[k], bytes, hipMemcpyHostToDevice) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_denoise_features: copy in");
    }
    if (!err) err = rt_denoise_features_device(device, d[0], d[1], d[2], d[3], w, h, p, nullptr, d[0], nullptr);
    if (!err && hipMemcpy(out_pixels, d[0], bytes, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_denoise_features: copy out");
    for (int k = 0; k < 4; ++k) if (d[k]) (void)hipFree(d[k]);
    return err;
}

int rt_render_picture_features_denoised(rt_scene* s, const rt_camera* camera, const rt_settings* st,
                                        const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                                        uint32_t w, uint32_t h, const rt_post_settings* post,
                                        const rt_denoise_features_params* p, uint32_t guide_spp, uint32_t* out_bgra,
                                        rt_stats* stats) {
    if (!s) return fail(RT_ERROR_INVALID, "rt_render_picture_features_denoised: null scene");
    if (!st) return fail(RT_ERROR_INVALID, "rt_render_picture_features_denoised: null settings");
    if (!post) return fail(RT_ERROR_INVALID, "rt_render_picture_features_denoised: null post");
    if (!out_bgra) return fail(RT_ERROR_INVALID, "rt_render_picture_features_denoised: null out_bgra");
    if (!w) return fail(RT_ERROR_INVALID, "rt_render_picture_features_denoised: w is 0");
    if (!h) return fail(RT_ERROR_INVALID, "rt_render_picture_features_denoised: h is 0");
    int err = check_features_params(p, true, true, true);
    if (err) return err;
    const int device = rt_internal_scene_device(s);
    err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)w*h;
    // one allocation: beauty (denoised in place), the three feature frames, the filter's workspace, the picture
    char* d_all = nullptr;
    const size_t ws_bytes = rt_denoise_features_workspace_bytes(w, h);
    if (hipMalloc(&d_all, 64*n + ws_bytes + 4*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, "rt_render_picture_features_denoised: hipMalloc");
    float* d_beauty = reinterpret_cast<float*>(d_all);
    float* d_feat[RT_FEATURE_COUNT];
    for (int f = 0; f < RT_FEATURE_COUNT; ++f) d_feat[f] = reinterpret_cast<float*>(d_all + 16*n*(size_t)(f + 1));
    void* d_ws = d_all + 64*n;
    uint32_t* d_pic = reinterpret_cast<uint32_t*>(d_all + 64*n + ws_bytes);
    if (hipMemset(d_all, 0, 64*n) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_render_picture_features_denoised: hipMemset");
    // the beauty frame as rt_render_picture renders it: a fresh buffer, frame_count 0
    if (!err) err = rt_render_device(s, camera, st, filter, tiles, total_frame_index, w, h, 0u, d_beauty, nullptr, stats);
    // the feature frames: the same camera, filter, tiles, frame index and bounce limit
    rt_settings gst = *st;
    if (guide_spp) gst.samples_per_pixel = guide_spp;
    rt_stats guide_stats;
    // (one walk for the three: the buffers are those of three rt_render_feature_device calls, bit for bit)
    if (!err) err = rt_render_features_device(s, camera, &gst, filter, tiles, total_frame_index, w, h, 0u, d_feat[RT_FEATURE_NORMAL],
                                              d_feat[RT_FEATURE_DISTANCE], d_feat[RT_FEATURE_ALBEDO], nullptr, &guide_stats);
    if (!err) err = rt_denoise_features_device(device, d_beauty, d_feat[RT_FEATURE_NORMAL], d_feat[RT_FEATURE_DISTANCE],
                                               d_feat[RT_FEATURE_ALBEDO], w, h, p, d_ws, d_beauty, nullptr);
    // the dither texture of total_frame_index + 1, as rt_render_picture picks it
    if (!err) err = rt_postprocess_device(device, d_beauty, w, h, post, total_frame_index + 1u, d_pic, nullptr);
    if (!err && hipMemcpy(out_bgra, d_pic, 4*n, hipMemcpyDeviceToHost) != hipSuccess) err = fail(RT_ERROR_DEVICE, "rt_render_picture_features_denoised: copy out");
    (void)hipFree(d_all);
    return err;
}

}  // extern "C"
