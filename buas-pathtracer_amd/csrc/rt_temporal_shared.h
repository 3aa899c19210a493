// rt_temporal_shared.h — what rt_temporal.hip and rt_svgf.hip both compile: the projection into the previous
// frame, the rule that says whether a previous pixel counts as a tap, and the argument checks of the accumulate
// stage.  One text for both files, so the history of rt_temporal_accumulate_moments_device cannot drift from
// rt_temporal_accumulate_device's.  Everything is local to the including file (an unnamed namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "rt_abi.h"
#include "rt_internal.h"

namespace {

constexpr float VALID_W = 0.001f;       // k_post's resolve threshold
constexpr int TA_NEWTON_STEPS = 5;      // of the inverse lens distortion (DESIGN.md has the count's reasons)

int fail(int code, const std::string& message) { rt_internal_set_error(message.c_str()); return code; }

struct V3f { float x, y, z; };

// the previous camera and what the projection needs of the frame
struct TaCamera {
    V3f p, x, y, z;
    float film_distance, half_film_w, half_film_h, lens_distortion;
};

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ float dot3(V3f a, V3f b) { return (a.x*b.x + a.y*b.y) + a.z*b.z; }
__device__ __forceinline__ V3f v3_of(rt_v3 a) { return {a.x, a.y, a.z}; }

// The position of world point P in the previous frame, in pixels.  False: no history.
__device__ __forceinline__ bool project_prev(const TaCamera& cam, V3f P, uint32_t w, uint32_t h, float& fx, float& fy) {
    const V3f d = {P.x - cam.p.x, P.y - cam.p.y, P.z - cam.p.z};
    const float z = -dot3(d, cam.z);
    if (!(z > 0.0f)) return false;
    float u = (dot3(d, cam.x)*cam.film_distance) / (z*cam.half_film_w);
    float v = (dot3(d, cam.y)*cam.film_distance) / (z*cam.half_film_h);
    // undo apply_lens_distortion (RT/raytracer.cpp:96-123): the amount > 0 normalisation, then the radial polynomial
    const float amount = cam.lens_distortion;
    const float woh = (float)w / (float)h;
    const float bd1 = 0.1f*amount, bd2 = -0.025f*amount;
    if (amount > 0.0f) {
        // brown_conrady({1, 1}); brown_conrady({0, 0}) is {0, 0}
        const float cy = 1.0f / woh;
        const float c2 = 1.0f*1.0f + cy*cy;
        const float cf = 1.0f + c2*bd1 + c2*c2*bd2;
        u = u*cf;
        v = v*((cy*cf)*woh);
    }
    const float X = u, Y = v / woh;
    const float R = __builtin_sqrtf(X*X + Y*Y);
    const float iw = 1.0f / woh;
    const float rc = __builtin_sqrtf(1.0f + iw*iw);
    // a point beyond the corner's own distorted radius lies outside the previous image
    const float rc2 = rc*rc;
    const float Rc = (rc + bd1*(rc2*rc) + bd2*((rc2*rc2)*rc))*(1.0f + 1.0f/1024.0f);
    if (R > Rc) return false;
    float r = R < rc ? R : rc;
#pragma unroll
    for (int k = 0; k < TA_NEWTON_STEPS; ++k) {
        const float r2 = r*r;
        const float g = (r + bd1*(r2*r) + bd2*((r2*r2)*r)) - R;
        const float dg = 1.0f + (3.0f*bd1)*r2 + (5.0f*bd2)*(r2*r2);
        r = r - g / dg;
        r = r > 0.0f ? r : 0.0f;        // NaN goes to 0
        r = r < rc ? r : rc;
    }
    const float scale = R > 0.0f ? r / R : 1.0f;
    u = u*scale;
    v = v*scale;
    fx = (1.0f - u)*((float)w*0.5f);
    fy = (1.0f - v)*((float)h*0.5f);
    // a position no tap of which can lie in the image (NaN and the infinities among them) has no history either
    return fx >= -1.0f && fx < (float)w && fy >= -1.0f && fy < (float)h;
}

struct TapSum { float W, r, g, b, L; };

// Whether previous pixel (qx, qy) counts as a tap; when it does, its index, length and history.
__device__ __forceinline__ bool tap_counts(int qx, int qy, uint32_t w, uint32_t h, const float4* prev_history,
                                           const float* prev_length, const rt_gbuffer_texel* prev_gbuffer,
                                           const rt_gbuffer_texel& g, V3f P, float normal_cos, float plane_limit, size_t& q,
                                           float& len, float4& ph) {
    if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) return false;
    q = (size_t)qy*w + (size_t)qx;
    len = prev_length[q];
    if (!(len >= 1.0f)) return false;
    const rt_gbuffer_texel pg = prev_gbuffer[q];
    if (pg.primitive != g.primitive) return false;
    if (g.primitive != RT_HIT_MISS) {
        const V3f n = v3_of(g.n);
        if (!(dot3(n, v3_of(pg.n)) >= normal_cos)) return false;
        const V3f off = {pg.p.x - P.x, pg.p.y - P.y, pg.p.z - P.z};
        if (!(fabsf(dot3(off, n)) <= plane_limit)) return false;
    }
    ph = prev_history[q];
    return finite_f(ph.x) && finite_f(ph.y) && finite_f(ph.z);
}

// One tap at previous pixel (qx, qy) with bilinear weight wt, added when it is valid.
__device__ __forceinline__ void add_tap(TapSum& s, int qx, int qy, float wt, uint32_t w, uint32_t h, const float4* prev_history,
                                        const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_gbuffer_texel& g,
                                        V3f P, float normal_cos, float plane_limit) {
    size_t q;
    float len;
    float4 ph;
    if (!tap_counts(qx, qy, w, h, prev_history, prev_length, prev_gbuffer, g, P, normal_cos, plane_limit, q, len, ph)) return;
    s.W = s.W + wt;
    s.r = s.r + wt*ph.x;
    s.g = s.g + wt*ph.y;
    s.b = s.b + wt*ph.z;
    s.L = s.L + wt*len;
}

// The same tap with the previous moments beside it: the tests and the sums of add_tap, then S1 and S2.  The
// moments take no part in the tap's validity.
struct MomentSum { float S1, S2; };
__device__ __forceinline__ void add_tap_moments(TapSum& s, MomentSum& m, int qx, int qy, float wt, uint32_t w, uint32_t h,
                                                const float4* prev_history, const float* prev_length,
                                                const rt_gbuffer_texel* prev_gbuffer, const float2* prev_moments,
                                                const rt_gbuffer_texel& g, V3f P, float normal_cos, float plane_limit) {
    size_t q;
    float len;
    float4 ph;
    if (!tap_counts(qx, qy, w, h, prev_history, prev_length, prev_gbuffer, g, P, normal_cos, plane_limit, q, len, ph)) return;
    s.W = s.W + wt;
    s.r = s.r + wt*ph.x;
    s.g = s.g + wt*ph.y;
    s.b = s.b + wt*ph.z;
    s.L = s.L + wt*len;
    const float2 pm = prev_moments[q];
    m.S1 = m.S1 + wt*pm.x;
    m.S2 = m.S2 + wt*pm.y;
}

bool bad_value(float v) { return !(v >= 0.0f) || v > 3.402823466e38f; }   // negative, NaN or infinite

int check_params(const std::string& e, const rt_temporal_params* p) {
    if (!p) return fail(RT_ERROR_INVALID, e + ": null rt_temporal_params");
    if (!(p->max_history >= 1.0f) || p->max_history > 3.402823466e38f)
        return fail(RT_ERROR_INVALID, e + ": rt_temporal_params: max_history must be finite and >= 1");
    if (!(p->normal_cos >= -1.0f && p->normal_cos <= 1.0f))
        return fail(RT_ERROR_INVALID, e + ": rt_temporal_params: normal_cos must be in [-1, 1]");
    if (bad_value(p->plane_tolerance)) return fail(RT_ERROR_INVALID, e + ": rt_temporal_params: plane_tolerance must be finite and >= 0");
    if (bad_value(p->snap)) return fail(RT_ERROR_INVALID, e + ": rt_temporal_params: snap must be finite and >= 0");
    if (bad_value(p->firefly_clamp)) return fail(RT_ERROR_INVALID, e + ": rt_temporal_params: firefly_clamp must be finite and >= 0");
    return RT_OK;
}

// every check of the stage that needs no device
int check_accumulate(const std::string& e, const char* prefix, const void* current, const void* gbuffer, const void* prev_history,
                     const void* prev_length, const void* prev_gbuffer, const rt_camera* prev_camera, uint32_t w, uint32_t h,
                     const rt_temporal_params* p, const void* history, const void* length) {
    const std::string d = prefix;
    if (!current) return fail(RT_ERROR_INVALID, e + ": null " + d + "current");
    if (!gbuffer) return fail(RT_ERROR_INVALID, e + ": null " + d + "gbuffer");
    if (!history) return fail(RT_ERROR_INVALID, e + ": null " + d + "history");
    if (!length) return fail(RT_ERROR_INVALID, e + ": null " + d + "length");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    int err = check_params(e, p);
    if (err) return err;
    if (prev_history || prev_length || prev_gbuffer) {
        if (!prev_history) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_history beside other previous buffers");
        if (!prev_length) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_length beside other previous buffers");
        if (!prev_gbuffer) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_gbuffer beside other previous buffers");
        if (!prev_camera) return fail(RT_ERROR_INVALID, e + ": null prev_camera with a history");
        if (history == prev_history) return fail(RT_ERROR_INVALID, e + ": " + d + "history aliases " + d + "prev_history");
        if (length == prev_length) return fail(RT_ERROR_INVALID, e + ": " + d + "length aliases " + d + "prev_length");
    }
    return RT_OK;
}

}  // namespace
