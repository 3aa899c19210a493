// rt_deform.hip — a temporal history that follows deforming meshes: the accumulate stage that takes a hit's surface
// point (its triangle and barycentrics, rt_gbuffer_surface_device's record) to where last frame's vertices put it
// (rt_temporal_accumulate_deform_device, rt_temporal_accumulate_deform) and the driver that runs one frame of the loop
// on the public entries (rt_render_temporal_deform_device, rt_render_temporal_deform).  Beyond the reference
// (DESIGN.md §9), an opt-in: no other entry calls it, and rt_motion.hip, rt_temporal.hip and rt_svgf.hip are not touched.
//
// The stage is defined operation by operation in DESIGN.md ("Deforming meshes keep their history");
// tests/ref_deform/ref_deform.c restates it in plain C and k_temporal_accumulate_deform matches that checker bit for
// bit: rt_motion.hip's rules, and for the new case hit_geometry's own expressions (rt_dmath.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_dmath.h"
#include "rt_temporal_shared.h"   // the projection, the tap rule and the accumulate stage's argument checks, as they are

namespace {

static_assert(sizeof(rt_surface_texel) == 16, "rt_surface_texel is 16 bytes");
static_assert(sizeof(rt_deform_entry) == 128, "rt_deform_entry is 128 bytes");
static_assert(sizeof(rt_motion_entry) == 112, "rt_motion_entry is 112 bytes");

// rt_svgf.hip's tm(c) = 1 - expf(-lum(c))
__device__ __forceinline__ float tm_of(float r, float g, float b) {
    const float y = (0.2126f*r + 0.7152f*g) + 0.0722f*b;
    return 1.0f - rtd::d_expf(-y);
}

// a[k] . (v, 1) and a[k] . (v, 0) in the stated order
__device__ __forceinline__ V3f xform_point(const float* a, V3f v) {
    return {((a[0]*v.x + a[1]*v.y) + a[2]*v.z) + a[3], ((a[4]*v.x + a[5]*v.y) + a[6]*v.z) + a[7],
            ((a[8]*v.x + a[9]*v.y) + a[10]*v.z) + a[11]};
}
__device__ __forceinline__ V3f xform_dir(const float* a, V3f v) {
    return {(a[0]*v.x + a[1]*v.y) + a[2]*v.z, (a[4]*v.x + a[5]*v.y) + a[6]*v.z, (a[8]*v.x + a[9]*v.y) + a[10]*v.z};
}

// One thread per pixel, k_temporal_accumulate_motion's layout and text with the deform case in front of the motion
// case.  Last frame's vertices are read by plain gather: 36 B a pixel (72 B with normals) at 9*triangle floats, in
// the caller's original order, so neighbouring pixels of one triangle share their lines and neighbouring triangles
// need not (profiles/deform_frame_cost.txt has what that costs).
template <bool MOMENTS>
__global__ void __launch_bounds__(256) k_temporal_accumulate_deform(
        const float4* __restrict__ current, const rt_gbuffer_texel* __restrict__ gbuffer,
        const float4* __restrict__ prev_history, const float* __restrict__ prev_length,
        const rt_gbuffer_texel* __restrict__ prev_gbuffer, const float2* __restrict__ prev_moments, TaCamera cam,
        uint32_t w, uint32_t h, rt_temporal_params p, const rt_motion_entry* __restrict__ motion, uint32_t motion_count,
        const rt_surface_texel* __restrict__ surface, const rt_deform_entry* __restrict__ deform, uint32_t deform_count,
        float4* __restrict__ history, float* __restrict__ length, float2* __restrict__ moments,
        float2* __restrict__ velocity) {
    const uint32_t x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y*w + x;
    const float qnan = __uint_as_float(0x7FC00000u);
    float2 vel = make_float2(qnan, qnan);
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
        if (MOMENTS) moments[i] = make_float2(0.0f, 0.0f);
        if (velocity) velocity[i] = vel;
        return;
    }
    // 2. clamp
    cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
    if (p.firefly_clamp > 0.0f) {
        cr = cr < p.firefly_clamp ? cr : p.firefly_clamp;
        cg = cg < p.firefly_clamp ? cg : p.firefly_clamp;
        cb = cb < p.firefly_clamp ? cb : p.firefly_clamp;
    }
    float t = 0.0f, t2 = 0.0f;
    if (MOMENTS) { t = tm_of(cr, cg, cb); t2 = t*t; }
    TapSum sum = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    MomentSum ms = {0.0f, 0.0f};
    if (prev_history) {
        // 3. the point and its place in the previous frame
        rt_gbuffer_texel g = gbuffer[i];
        V3f P = v3_of(g.p);
        if (g.primitive == RT_HIT_MISS) P = {cam.p.x + g.p.x, cam.p.y + g.p.y, cam.p.z + g.p.z};
        // 3d. a deformed mesh's surface point and shading normal, as last frame's vertices and transform gave them
        bool deformed = false;
        if (!(g.primitive & RT_HIT_PLANE_BIT) && g.primitive < deform_count) {
            const rt_deform_entry* e = &deform[g.primitive];
            if (e->deformed != 0u) {
                const rt_surface_texel sr = surface[i];
                if (sr.triangle < e->triangle_count) {
                    deformed = true;
                    const float* vt = e->d_prev_triangles + 9*(size_t)sr.triangle;
                    const rtd::V3 a = {vt[0], vt[1], vt[2]};
                    const rtd::V3 e1 = rtd::sub({vt[3], vt[4], vt[5]}, a), e2 = rtd::sub({vt[6], vt[7], vt[8]}, a);
                    const V3f Po = {(a.x + sr.v*e1.x) + sr.w*e2.x, (a.y + sr.v*e1.y) + sr.w*e2.y, (a.z + sr.v*e1.z) + sr.w*e2.z};
                    rtd::M34 inv;
                    float f[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) { inv.e[k >> 2][k & 3] = e->inv_prev[k >> 2][k & 3]; f[k] = e->fwd_prev[k >> 2][k & 3]; }
                    P = xform_point(f, Po);
                    rtd::V3 no;
                    if (e->has_normals != 0u) {
                        const float* nt = e->d_prev_normals + 9*(size_t)sr.triangle;
                        const float u = 1.0f - sr.v - sr.w;
                        no = rtd::add(rtd::add(rtd::smul(u, {nt[0], nt[1], nt[2]}), rtd::smul(sr.v, {nt[3], nt[4], nt[5]})),
                                      rtd::smul(sr.w, {nt[6], nt[7], nt[8]}));
                    } else {
                        no = rtd::cross(rtd::normalize(e1), rtd::normalize(e2));
                    }
                    const rtd::V3 nn = rtd::noz(rtd::xform_normal(inv, no));
                    g.n = {nn.x, nn.y, nn.z};
                }
            }
        }
        // 3m. a moved primitive's point and normal, carried to where they were (a miss has every bit set)
        if (!deformed && !(g.primitive & RT_HIT_PLANE_BIT) && g.primitive < motion_count) {
            const float* e = reinterpret_cast<const float*>(&motion[g.primitive]);
            if (__float_as_uint(e[24]) != 0u) {
                float a[24];
#pragma unroll
                for (int k = 0; k < 24; ++k) a[k] = e[k];
                P = xform_point(a + 12, xform_point(a, P));
                const V3f n = v3_of(g.n);
                const V3f m = xform_dir(a + 12, xform_dir(a, n));
                const float len = __builtin_sqrtf(dot3(m, m));
                if (len > 0.0f) g.n = {m.x / len, m.y / len, m.z / len};
            }
        }
        float fx, fy;
        if (project_prev(cam, P, w, h, fx, fy)) {
            vel = make_float2(fx - (float)x, fy - (float)y);
            // 4. the taps
            const float plane_limit = p.plane_tolerance*g.t;
            const float rx = rintf(fx), ry = rintf(fy);
            if (fabsf(fx - rx) <= p.snap && fabsf(fy - ry) <= p.snap) {
                if (MOMENTS) add_tap_moments(sum, ms, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, prev_moments, g, P, p.normal_cos, plane_limit);
                else add_tap(sum, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
            } else {
                const float x0 = floorf(fx), y0 = floorf(fy);
                const float tx = fx - x0, ty = fy - y0;
                const int ix = (int)x0, iy = (int)y0;
                const float wt[4] = {(1.0f - tx)*(1.0f - ty), tx*(1.0f - ty), (1.0f - tx)*ty, tx*ty};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (MOMENTS) add_tap_moments(sum, ms, ix + (k & 1), iy + (k >> 1), wt[k], w, h, prev_history, prev_length, prev_gbuffer, prev_moments, g, P, p.normal_cos, plane_limit);
                    else add_tap(sum, ix + (k & 1), iy + (k >> 1), wt[k], w, h, prev_history, prev_length, prev_gbuffer, g, P, p.normal_cos, plane_limit);
                }
            }
        }
    }
    if (velocity) velocity[i] = vel;
    // 5. the blend
    if (sum.W > 0.0f) {
        const float hr = sum.r / sum.W, hg = sum.g / sum.W, hb = sum.b / sum.W;
        const float L = sum.L / sum.W;
        float N = L + 1.0f;
        N = N < p.max_history ? N : p.max_history;
        const float a = 1.0f / N;
        // N = 1 (max_history = 1: a valid tap's length is >= 1) is the current frame itself, not hist + (c - hist)
        if (N == 1.0f) {
            history[i] = make_float4(cr, cg, cb, 1.0f);
            if (MOMENTS) moments[i] = make_float2(t, t2);
        } else {
            history[i] = make_float4(hr + (cr - hr)*a, hg + (cg - hg)*a, hb + (cb - hb)*a, 1.0f);
            if (MOMENTS) {
                const float h1 = ms.S1 / sum.W, h2 = ms.S2 / sum.W;
                moments[i] = make_float2(h1 + (t - h1)*a, h2 + (t2 - h2)*a);
            }
        }
        length[i] = N;
    } else {
        history[i] = make_float4(cr, cg, cb, 1.0f);
        length[i] = 1.0f;
        if (MOMENTS) moments[i] = make_float2(t, t2);
    }
}

// the accumulate stage's checks, the motion stage's, then the deform stage's own; all before the device is touched
int check_deform(const std::string& e, const char* prefix, const void* current, const void* gbuffer, const void* prev_history,
                 const void* prev_length, const void* prev_gbuffer, const rt_camera* prev_camera, uint32_t w, uint32_t h,
                 const rt_temporal_params* p, const void* history, const void* length, const void* motion, uint32_t motion_count,
                 const void* prev_moments, const void* moments, const void* surface, const void* deform, uint32_t deform_count) {
    int err = check_accumulate(e, prefix, current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, w, h, p, history,
                               length);
    if (err) return err;
    const std::string d = prefix;
    if (!motion && motion_count) return fail(RT_ERROR_INVALID, e + ": null " + d + "motion with a motion_count");
    if (motion_count & RT_HIT_PLANE_BIT) return fail(RT_ERROR_INVALID, e + ": motion_count must be below 2^31");
    if (!moments) {
        if (prev_moments) return fail(RT_ERROR_INVALID, e + ": " + d + "prev_moments without " + d + "moments");
    } else if (prev_history) {
        if (!prev_moments) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_moments beside other previous buffers");
        if (moments == prev_moments) return fail(RT_ERROR_INVALID, e + ": " + d + "moments aliases " + d + "prev_moments");
    } else if (prev_moments) {
        return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_history beside other previous buffers");
    }
    if (!deform && deform_count) return fail(RT_ERROR_INVALID, e + ": null " + d + "deform with a deform_count");
    if (deform_count & RT_HIT_PLANE_BIT) return fail(RT_ERROR_INVALID, e + ": deform_count must be below 2^31");
    if (deform && !surface) return fail(RT_ERROR_INVALID, e + ": null " + d + "surface with a deform table");
    return RT_OK;
}

// the driver's workspace: rt_render_temporal_motion_device's (120 bytes per pixel, then the motion table on a 16-byte
// boundary), then the surface records and the deform table, each on a 16-byte boundary
struct Workspace {
    float* current;
    rt_gbuffer_texel* gbuffer[2];
    float* history[2];
    float* length[2];
    rt_motion_entry* motion;
    rt_surface_texel* surface;
    rt_deform_entry* deform;
};
size_t motion_table_offset(size_t n) { return (rt_temporal_workspace_bytes(1, 1)*n + 15) & ~(size_t)15; }
size_t surface_offset(uint32_t w, uint32_t h, uint32_t count) {
    return (rt_temporal_motion_workspace_bytes(w, h, count) + 15) & ~(size_t)15;
}
Workspace carve(void* d_workspace, uint32_t w, uint32_t h, uint32_t count) {
    const size_t n = (size_t)w*h;
    char* base = static_cast<char*>(d_workspace);
    Workspace ws;
    ws.current = reinterpret_cast<float*>(base);
    for (int k = 0; k < 2; ++k) {
        ws.gbuffer[k] = reinterpret_cast<rt_gbuffer_texel*>(base + 16*n + (size_t)k*32*n);
        ws.history[k] = reinterpret_cast<float*>(base + 80*n + (size_t)k*16*n);
        ws.length[k] = reinterpret_cast<float*>(base + 112*n + (size_t)k*4*n);
    }
    ws.motion = reinterpret_cast<rt_motion_entry*>(base + motion_table_offset(n));
    ws.surface = reinterpret_cast<rt_surface_texel*>(base + surface_offset(w, h, count));
    ws.deform = reinterpret_cast<rt_deform_entry*>(base + surface_offset(w, h, count) + sizeof(rt_surface_texel)*n);
    return ws;
}

int check_driver(const std::string& e, const rt_scene* s, const rt_camera* camera, const rt_settings* st,
                 const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t w, uint32_t h, const rt_temporal_params* p,
                 const rt_temporal_motion_state* state, const void* out, const char* out_name) {
    // rt_render_temporal_motion_device's checks in its order
    int err = check_params(e, p);
    if (err) return err;
    if (!state) return fail(RT_ERROR_INVALID, e + ": null rt_temporal_motion_state");
    if (!state->d_workspace) return fail(RT_ERROR_INVALID, e + ": rt_temporal_motion_state: null d_workspace");
    if (!state->transforms) return fail(RT_ERROR_INVALID, e + ": rt_temporal_motion_state: null transforms");
    if (state->parity > 1u) return fail(RT_ERROR_INVALID, e + ": rt_temporal_motion_state: parity must be 0 or 1");
    if (!st) return fail(RT_ERROR_INVALID, e + ": null settings");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if (!camera) return fail(RT_ERROR_INVALID, e + ": null camera");
    if (!filter) return fail(RT_ERROR_INVALID, e + ": null filter");
    if (!tiles) return fail(RT_ERROR_INVALID, e + ": null tiles");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null " + out_name);
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    uint32_t count = 0;
    err = rt_scene_primitive_transforms(s, 0, nullptr, &count);
    if (err) return err;
    if (state->transform_cap < count)
        return fail(RT_ERROR_INVALID, e + ": rt_temporal_motion_state: transform_cap is below the scene's primitive count");
    return RT_OK;
}

TaCamera ta_camera(const rt_camera* c, float lens_distortion) {
    TaCamera cam = {};
    cam.p = {c->p.x, c->p.y, c->p.z};
    cam.x = {c->x.x, c->x.y, c->x.z};
    cam.y = {c->y.x, c->y.y, c->y.z};
    cam.z = {c->z.x, c->z.y, c->z.z};
    cam.film_distance = c->film_distance;
    cam.half_film_w = c->half_film_w;
    cam.half_film_h = c->half_film_h;
    cam.lens_distortion = lens_distortion;
    return cam;
}

}  // namespace

extern "C" {

int rt_temporal_accumulate_deform_device(int device, const float* d_current, const rt_gbuffer_texel* d_gbuffer,
                                         const float* d_prev_history, const float* d_prev_length,
                                         const rt_gbuffer_texel* d_prev_gbuffer, const rt_camera* prev_camera,
                                         float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                         float* d_history, float* d_length, void* hip_stream, const rt_motion_entry* d_motion,
                                         uint32_t motion_count, const float* d_prev_moments, float* d_moments,
                                         float* d_velocity, const rt_surface_texel* d_surface, const rt_deform_entry* d_deform,
                                         uint32_t deform_count) {
    const std::string e = "rt_temporal_accumulate_deform_device";
    int err = check_deform(e, "d_", d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera, w, h, p,
                           d_history, d_length, d_motion, motion_count, d_prev_moments, d_moments, d_surface, d_deform, deform_count);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    const TaCamera cam = d_prev_history ? ta_camera(prev_camera, prev_lens_distortion) : TaCamera{};
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    const float4* cur4 = reinterpret_cast<const float4*>(d_current);
    const float4* ph4 = reinterpret_cast<const float4*>(d_prev_history);
    const float2* pm2 = reinterpret_cast<const float2*>(d_prev_moments);
    float4* hist4 = reinterpret_cast<float4*>(d_history);
    float2* mom2 = reinterpret_cast<float2*>(d_moments);
    float2* vel2 = reinterpret_cast<float2*>(d_velocity);
    if (d_moments)
        k_temporal_accumulate_deform<true><<<grid, 256, 0, stream>>>(cur4, d_gbuffer, ph4, d_prev_length, d_prev_gbuffer, pm2, cam, w, h,
                                                                     *p, d_motion, motion_count, d_surface, d_deform, deform_count,
                                                                     hist4, d_length, mom2, vel2);
    else
        k_temporal_accumulate_deform<false><<<grid, 256, 0, stream>>>(cur4, d_gbuffer, ph4, d_prev_length, d_prev_gbuffer, pm2, cam, w, h,
                                                                      *p, d_motion, motion_count, d_surface, d_deform, deform_count,
                                                                      hist4, d_length, mom2, vel2);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, e + ": " + hipGetErrorString(herr));
    return RT_OK;
}

int rt_temporal_accumulate_deform(int device, const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                  const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_camera* prev_camera,
                                  float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p, float* history,
                                  float* length, const rt_motion_entry* motion, uint32_t motion_count, const float* prev_moments,
                                  float* moments, float* velocity, const rt_surface_texel* surface, const rt_deform_entry* deform,
                                  uint32_t deform_count) {
    const std::string e = "rt_temporal_accumulate_deform";
    int err = check_deform(e, "", current, gbuffer, prev_history, prev_length, prev_gbuffer, prev_camera, w, h, p, history, length,
                           motion, motion_count, prev_moments, moments, surface, deform, deform_count);
    if (err) return err;
    err = rt_internal_bind_device(device);
    if (err) return err;
    // rt_temporal_accumulate_motion's 144 bytes per pixel, the surface records (16), the two tables
    const size_t n = (size_t)w*h;
    const size_t motion_at = 160*n;
    const size_t deform_at = motion_at + ((sizeof(rt_motion_entry)*(size_t)(motion_count ? motion_count : 1u) + 15) & ~(size_t)15);
    char* d = nullptr;
    if (hipMalloc(&d, deform_at + sizeof(rt_deform_entry)*(size_t)(deform_count ? deform_count : 1u)) != hipSuccess)
        return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_cur = reinterpret_cast<float*>(d);
    rt_gbuffer_texel* d_g[2] = {reinterpret_cast<rt_gbuffer_texel*>(d + 16*n), reinterpret_cast<rt_gbuffer_texel*>(d + 48*n)};
    float* d_h[2] = {reinterpret_cast<float*>(d + 80*n), reinterpret_cast<float*>(d + 96*n)};
    float* d_m[2] = {reinterpret_cast<float*>(d + 112*n), reinterpret_cast<float*>(d + 120*n)};
    float* d_v = reinterpret_cast<float*>(d + 128*n);
    float* d_l[2] = {reinterpret_cast<float*>(d + 136*n), reinterpret_cast<float*>(d + 140*n)};
    rt_surface_texel* d_s = reinterpret_cast<rt_surface_texel*>(d + 144*n);
    rt_motion_entry* d_t = reinterpret_cast<rt_motion_entry*>(d + motion_at);
    rt_deform_entry* d_e = reinterpret_cast<rt_deform_entry*>(d + deform_at);
    const bool prev = prev_history != nullptr;
    if (hipMemcpy(d_cur, current, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_g[0], gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
        (surface && hipMemcpy(d_s, surface, 16*n, hipMemcpyHostToDevice) != hipSuccess) ||
        (motion_count && hipMemcpy(d_t, motion, sizeof(rt_motion_entry)*(size_t)motion_count, hipMemcpyHostToDevice) != hipSuccess) ||
        (deform_count && hipMemcpy(d_e, deform, sizeof(rt_deform_entry)*(size_t)deform_count, hipMemcpyHostToDevice) != hipSuccess) ||
        (prev && (hipMemcpy(d_h[1], prev_history, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(d_l[1], prev_length, 4*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(d_g[1], prev_gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
                  (prev_moments && hipMemcpy(d_m[1], prev_moments, 8*n, hipMemcpyHostToDevice) != hipSuccess))))
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    if (!err) err = rt_temporal_accumulate_deform_device(device, d_cur, d_g[0], prev ? d_h[1] : nullptr, prev ? d_l[1] : nullptr,
                                                         prev ? d_g[1] : nullptr, prev_camera, prev_lens_distortion, w, h, p, d_h[0],
                                                         d_l[0], nullptr, motion_count ? d_t : nullptr, motion_count,
                                                         prev_moments ? d_m[1] : nullptr, moments ? d_m[0] : nullptr,
                                                         velocity ? d_v : nullptr, surface ? d_s : nullptr,
                                                         deform_count ? d_e : nullptr, deform_count);
    if (!err && (hipMemcpy(history, d_h[0], 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(length, d_l[0], 4*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (moments && hipMemcpy(moments, d_m[0], 8*n, hipMemcpyDeviceToHost) != hipSuccess) ||
                 (velocity && hipMemcpy(velocity, d_v, 8*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

size_t rt_temporal_deform_workspace_bytes(uint32_t w, uint32_t h, uint32_t primitive_count) {
    return surface_offset(w, h, primitive_count) + sizeof(rt_surface_texel)*(size_t)w*h +
           sizeof(rt_deform_entry)*(size_t)(primitive_count ? primitive_count : 1u);
}

int rt_render_temporal_deform_device(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                                     const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h,
                                     uint32_t frame_count, const rt_temporal_params* p, rt_temporal_motion_state* state,
                                     uint32_t mesh_count, const rt_deform_mesh* meshes, float* d_out, float* d_length_out,
                                     void* hip_stream, rt_stats* stats) {
    const std::string e = "rt_render_temporal_deform_device";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, d_out, "d_out");
    if (err) return err;
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
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)w*h;
    const Workspace ws = carve(state->d_workspace, w, h, count);
    const uint32_t cur = state->parity, old = state->parity ^ 1u;

    if (hipMemsetAsync(ws.current, 0, 16*n, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": hipMemset");
    rt_stats fs;
    err = rt_render_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, ws.current, hip_stream, &fs);
    if (err) return err;
    // a frame clears the scene's cancel flag when its loop starts: one raised after it is seen here
    if (rt_internal_scene_cancelled(s)) return fail(RT_ERROR_CANCELLED, "render cancelled");
    err = rt_gbuffer_surface_device(s, camera, st->lens_distortion, w, h, ws.gbuffer[cur], ws.surface, hip_stream);
    if (err) return err;
    if (prev && count) {
        std::vector<rt_motion_entry> table(count);
        err = rt_motion_table(count, now.data(), state->transforms, table.data());
        if (err) return err;
        // the stage of the frame before has synchronised its stream: nothing reads the tables now
        if (hipMemcpy(ws.motion, table.data(), sizeof(rt_motion_entry)*(size_t)count, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(ws.deform, deform.data(), sizeof(rt_deform_entry)*(size_t)count, hipMemcpyHostToDevice) != hipSuccess)
            return fail(RT_ERROR_DEVICE, e + ": table upload");
    }
    const bool tables = prev && count;
    err = rt_temporal_accumulate_deform_device(device, ws.current, ws.gbuffer[cur], prev ? ws.history[old] : nullptr,
                                               prev ? ws.length[old] : nullptr, prev ? ws.gbuffer[old] : nullptr, &state->camera,
                                               state->lens_distortion, w, h, p, ws.history[cur], ws.length[cur], hip_stream,
                                               tables ? ws.motion : nullptr, prev ? count : 0u, nullptr, nullptr, nullptr,
                                               ws.surface, tables ? ws.deform : nullptr, prev ? count : 0u);
    if (err) return err;
    if (hipMemcpyAsync(d_out, ws.history[cur], 16*n, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
        (d_length_out && hipMemcpyAsync(d_length_out, ws.length[cur], 4*n, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": copy out");
    state->w = w; state->h = h;
    state->camera = *camera;
    state->lens_distortion = st->lens_distortion;
    state->primitive_count = count;
    if (count) memcpy(state->transforms, now.data(), sizeof(rt_m4x4inv)*(size_t)count);
    state->parity = old;
    state->frames += 1u;
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_render_temporal_deform(rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                              const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                              const rt_temporal_params* p, rt_temporal_motion_state* state, uint32_t mesh_count,
                              const rt_deform_mesh* meshes, float* out_pixels, float* out_length, rt_stats* stats) {
    const std::string e = "rt_render_temporal_deform";
    int err = check_driver(e, s, camera, st, filter, tiles, w, h, p, state, out_pixels, "out_pixels");
    if (err) return err;
    err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the history, the length
    if (hipMalloc(&d, 20*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_out = reinterpret_cast<float*>(d);
    float* d_len = reinterpret_cast<float*>(d + 16*n);
    err = rt_render_temporal_deform_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, p, state, mesh_count,
                                           meshes, d_out, out_length ? d_len : nullptr, nullptr, stats);
    if (!err && (hipMemcpy(out_pixels, d_out, 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (out_length && hipMemcpy(out_length, d_len, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

}  // extern "C"
