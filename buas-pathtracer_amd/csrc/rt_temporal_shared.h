// rt_temporal_shared.h — the temporal accumulate stage, once, for the five files that launch it: rt_temporal.hip,
// rt_svgf.hip, rt_motion.hip, rt_deform.hip and rt_clip.hip.  The device half is the projection into the previous frame,
// the rule that says whether a previous pixel counts as a tap, and temporal_accumulate_body<MOMENTS, MOTION, DEFORM,
// CLIP>: steps 1 to 5 of DESIGN.md's "Temporal accumulation" with the moments, step 3m, step 3d and step 4c (the
// neighbourhood clip of the history, DESIGN.md's "Neighbourhood clipping") behind the four flags.  Each
// file's __global__ kernel is a call of that body, so a history cannot drift between the entries.  The host half is
// what the entries share: the stage's arguments and their checks as a chain, the launch, the host staging of the
// motion and deform entries, and the drivers' workspace prefix, checks, frame prologue and state epilogue.
// Everything is local to the including file (an unnamed namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <type_traits>

#include "rt_abi.h"
#include "rt_internal.h"
#include "rt_dmath.h"

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

// One tap at previous pixel (qx, qy) with bilinear weight wt, added when it is valid; with MOMENTS the previous
// moments beside it: S1 and S2 after the sums.  The moments take no part in the tap's validity.
struct MomentSum { float S1, S2; };
template <bool MOMENTS>
__device__ __forceinline__ void add_tap(TapSum& s, MomentSum& m, int qx, int qy, float wt, uint32_t w, uint32_t h,
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
    if constexpr (MOMENTS) {
        const float2 pm = prev_moments[q];
        m.S1 = m.S1 + wt*pm.x;
        m.S2 = m.S2 + wt*pm.y;
    }
}

// tm(c) = 1 - expf(-lum(c)): the denoise stage's l, in [0, 1]
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

// what step 4c reads and writes: the current frame's neighbourhood statistics, the box's half width in sigmas, the
// fewest window pixels a texel must hold, and where the clip's size goes (may be null).  All null and 0 without CLIP.
struct TaClip {
    const rt_neighbourhood_texel* neighbourhood;
    float gamma, min_count;
    float* clip_amount;
};

// The accumulate stage of one pixel: the body of k_temporal_accumulate <false, false, false, false>,
// k_temporal_accumulate_moments <true, false, false, false>, k_temporal_accumulate_motion<M> <M, true, false, false>,
// k_temporal_accumulate_deform<M> <M, true, true, false> and k_temporal_accumulate_clip<M> <M, true, true, true>.  One thread per pixel; a wave is 64 consecutive pixels of a row
// (64 x 4 blocks, as k_post): the current frame, the texel and the outputs are contiguous runs, and under a small
// camera motion the taps of a wave are too.  (An 8 x 8 footprint per wave measured 7 to 11 % slower at 1920x1080:
// profiles/temporal_frame_cost.txt.)  A kernel passes null for what it has no parameter for: moments and
// prev_moments without MOMENTS, the motion table and velocity without MOTION, surface and the deform table without
// DEFORM, an empty TaClip without CLIP; velocity may be null with MOTION too, the neighbourhood and the clip amount
// with CLIP.
template <bool MOMENTS, bool MOTION, bool DEFORM, bool CLIP>
__device__ __forceinline__ void temporal_accumulate_body(
        const float4* __restrict__ current, const rt_gbuffer_texel* __restrict__ gbuffer,
        const float4* __restrict__ prev_history, const float* __restrict__ prev_length,
        const rt_gbuffer_texel* __restrict__ prev_gbuffer, const float2* __restrict__ prev_moments, const TaCamera& cam,
        uint32_t w, uint32_t h, const rt_temporal_params& p, const rt_motion_entry* __restrict__ motion, uint32_t motion_count,
        const rt_surface_texel* __restrict__ surface, const rt_deform_entry* __restrict__ deform, uint32_t deform_count,
        float4* __restrict__ history, float* __restrict__ length, float2* __restrict__ moments,
        float2* __restrict__ velocity, const TaClip& clip) {
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
        if (MOTION && velocity) velocity[i] = vel;
        if constexpr (CLIP) { if (clip.clip_amount) clip.clip_amount[i] = 0.0f; }
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
        // 3d. a deformed mesh's surface point and shading normal, as last frame's vertices and transform gave them.
        // Last frame's vertices are read by plain gather: 36 B a pixel (72 B with normals) at 9*triangle floats, in the
        // caller's original order, so neighbouring pixels of one triangle share their lines and neighbouring
        // triangles need not (profiles/deform_frame_cost.txt has what that costs).
        bool deformed = false;
        if constexpr (DEFORM) {
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
        }
        // 3m. a moved primitive's point and normal, carried to where they were (a miss has every bit set).  The table
        // read is a plain gather: a wave's 64 pixels name a handful of primitives, so its 24-word reads fall on one or
        // two entries that stay in L2 and the vector cache.  (Staging the table in LDS per block measured no faster at
        // 1920 x 1080, 60.5 against 60.2 us on C4 and 70.8 against 69.4 us on C3: profiles/motion_frame_cost.txt.)
        if constexpr (MOTION) {
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
        }
        float fx, fy;
        if (project_prev(cam, P, w, h, fx, fy)) {
            vel = make_float2(fx - (float)x, fy - (float)y);
            // 4. the taps
            const float plane_limit = p.plane_tolerance*g.t;
            const float rx = rintf(fx), ry = rintf(fy);
            if (fabsf(fx - rx) <= p.snap && fabsf(fy - ry) <= p.snap) {
                add_tap<MOMENTS>(sum, ms, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, prev_moments, g, P, p.normal_cos, plane_limit);
            } else {
                const float x0 = floorf(fx), y0 = floorf(fy);
                const float tx = fx - x0, ty = fy - y0;
                const int ix = (int)x0, iy = (int)y0;
                const float wt[4] = {(1.0f - tx)*(1.0f - ty), tx*(1.0f - ty), (1.0f - tx)*ty, tx*ty};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    add_tap<MOMENTS>(sum, ms, ix + (k & 1), iy + (k >> 1), wt[k], w, h, prev_history, prev_length, prev_gbuffer, prev_moments, g, P, p.normal_cos, plane_limit);
            }
        }
    }
    if (MOTION && velocity) velocity[i] = vel;
    // 5. the blend
    float clipped = 0.0f;
    if (sum.W > 0.0f) {
        float hr = sum.r / sum.W, hg = sum.g / sum.W, hb = sum.b / sum.W;
        // 4c. the history clipped to the current frame's neighbourhood: mean -+ gamma*sigma per channel.  The
        // comparisons are written so that a NaN bound leaves the value alone.
        if constexpr (CLIP) {
            if (clip.neighbourhood) {
                const rt_neighbourhood_texel nt = clip.neighbourhood[i];
                if (nt.count >= clip.min_count) {
                    const rt_v3 m = nt.mean, sg = nt.sigma;
                    const float br = hr, bg = hg, bb = hb;
                    const float lr = m.x - clip.gamma*sg.x, ur = m.x + clip.gamma*sg.x;
                    const float lg = m.y - clip.gamma*sg.y, ug = m.y + clip.gamma*sg.y;
                    const float lb = m.z - clip.gamma*sg.z, ub = m.z + clip.gamma*sg.z;
                    hr = hr < lr ? lr : hr; hr = hr > ur ? ur : hr;
                    hg = hg < lg ? lg : hg; hg = hg > ug ? ug : hg;
                    hb = hb < lb ? lb : hb; hb = hb > ub ? ub : hb;
                    const float dr = fabsf(br - hr), dg = fabsf(bg - hg), db = fabsf(bb - hb);
                    clipped = dr;
                    clipped = dg > clipped ? dg : clipped;
                    clipped = db > clipped ? db : clipped;
                }
            }
        }
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
    if constexpr (CLIP) { if (clip.clip_amount) clip.clip_amount[i] = clipped; }
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

// The stage's arguments in the order of the widest entry's (rt_temporal_accumulate_deform_device); an entry leaves
// null or 0 what it has no parameter for.  Host or device pointers alike: a check's prefix ("" or "d_") names them.
struct TaArgs {
    const float* current;
    const rt_gbuffer_texel* gbuffer;
    const float* prev_history;
    const float* prev_length;
    const rt_gbuffer_texel* prev_gbuffer;
    const rt_camera* prev_camera;
    float prev_lens_distortion;
    uint32_t w, h;
    const rt_temporal_params* p;
    float* history;
    float* length;
    const rt_motion_entry* motion;
    uint32_t motion_count;
    const float* prev_moments;
    float* moments;
    float* velocity;
    const rt_surface_texel* surface;
    const rt_deform_entry* deform;
    uint32_t deform_count;
    const rt_neighbourhood_texel* neighbourhood;    // the clip entries' four
    float gamma, min_count;
    float* clip_amount;
};

// The checks are a chain, each link before the device is touched: every entry's, then the motion and deform
// entries' (their optional moments among them), then the deform entries' own, then the clip entries' own.
int check_accumulate(const std::string& e, const char* prefix, const TaArgs& a) {
    const std::string d = prefix;
    if (!a.current) return fail(RT_ERROR_INVALID, e + ": null " + d + "current");
    if (!a.gbuffer) return fail(RT_ERROR_INVALID, e + ": null " + d + "gbuffer");
    if (!a.history) return fail(RT_ERROR_INVALID, e + ": null " + d + "history");
    if (!a.length) return fail(RT_ERROR_INVALID, e + ": null " + d + "length");
    if (!a.w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!a.h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    int err = check_params(e, a.p);
    if (err) return err;
    if (a.prev_history || a.prev_length || a.prev_gbuffer) {
        if (!a.prev_history) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_history beside other previous buffers");
        if (!a.prev_length) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_length beside other previous buffers");
        if (!a.prev_gbuffer) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_gbuffer beside other previous buffers");
        if (!a.prev_camera) return fail(RT_ERROR_INVALID, e + ": null prev_camera with a history");
        if (a.history == a.prev_history) return fail(RT_ERROR_INVALID, e + ": " + d + "history aliases " + d + "prev_history");
        if (a.length == a.prev_length) return fail(RT_ERROR_INVALID, e + ": " + d + "length aliases " + d + "prev_length");
    }
    return RT_OK;
}

int check_motion(const std::string& e, const char* prefix, const TaArgs& a) {
    int err = check_accumulate(e, prefix, a);
    if (err) return err;
    const std::string d = prefix;
    if (!a.motion && a.motion_count) return fail(RT_ERROR_INVALID, e + ": null " + d + "motion with a motion_count");
    if (a.motion_count & RT_HIT_PLANE_BIT) return fail(RT_ERROR_INVALID, e + ": motion_count must be below 2^31");
    if (!a.moments) {
        if (a.prev_moments) return fail(RT_ERROR_INVALID, e + ": " + d + "prev_moments without " + d + "moments");
    } else if (a.prev_history) {
        if (!a.prev_moments) return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_moments beside other previous buffers");
        if (a.moments == a.prev_moments) return fail(RT_ERROR_INVALID, e + ": " + d + "moments aliases " + d + "prev_moments");
    } else if (a.prev_moments) {
        return fail(RT_ERROR_INVALID, e + ": null " + d + "prev_history beside other previous buffers");
    }
    return RT_OK;
}

int check_deform(const std::string& e, const char* prefix, const TaArgs& a) {
    int err = check_motion(e, prefix, a);
    if (err) return err;
    const std::string d = prefix;
    if (!a.deform && a.deform_count) return fail(RT_ERROR_INVALID, e + ": null " + d + "deform with a deform_count");
    if (a.deform_count & RT_HIT_PLANE_BIT) return fail(RT_ERROR_INVALID, e + ": deform_count must be below 2^31");
    if (a.deform && !a.surface) return fail(RT_ERROR_INVALID, e + ": null " + d + "surface with a deform table");
    return RT_OK;
}

int check_clip(const std::string& e, const char* prefix, const TaArgs& a) {
    int err = check_deform(e, prefix, a);
    if (err) return err;
    if (bad_value(a.gamma)) return fail(RT_ERROR_INVALID, e + ": gamma must be finite and >= 0");
    if (bad_value(a.min_count)) return fail(RT_ERROR_INVALID, e + ": min_count must be finite and >= 0");
    return RT_OK;
}

// the drivers that clip (rt_clip.hip's and rt_specular.hip's): their rt_temporal_clip_params
int check_clip_params(const std::string& e, const rt_temporal_clip_params* cp) {
    if (!cp) return fail(RT_ERROR_INVALID, e + ": null rt_temporal_clip_params");
    if (cp->radius < 1u || cp->radius > 3u) return fail(RT_ERROR_INVALID, e + ": rt_temporal_clip_params: radius must be in 1..3");
    if (bad_value(cp->gamma)) return fail(RT_ERROR_INVALID, e + ": rt_temporal_clip_params: gamma must be finite and >= 0");
    if (bad_value(cp->min_count)) return fail(RT_ERROR_INVALID, e + ": rt_temporal_clip_params: min_count must be finite and >= 0");
    return RT_OK;
}

// the kernels' view of the previous camera; without a history nothing reads it
TaCamera ta_camera(const TaArgs& a) {
    TaCamera cam = {};
    if (!a.prev_history) return cam;
    const rt_camera* c = a.prev_camera;
    cam.p = {c->p.x, c->p.y, c->p.z};
    cam.x = {c->x.x, c->x.y, c->x.z};
    cam.y = {c->y.x, c->y.y, c->y.z};
    cam.z = {c->z.x, c->z.y, c->z.z};
    cam.film_distance = c->film_distance;
    cam.half_film_w = c->half_film_w;
    cam.half_film_h = c->half_film_h;
    cam.lens_distortion = a.prev_lens_distortion;
    return cam;
}

// the entries' float runs as the kernels read them
const float4* f4(const float* p) { return reinterpret_cast<const float4*>(p); }
float4* f4(float* p) { return reinterpret_cast<float4*>(p); }
const float2* f2(const float* p) { return reinterpret_cast<const float2*>(p); }
float2* f2(float* p) { return reinterpret_cast<float2*>(p); }

// One accumulate kernel over the frame, one thread per pixel in 64 x 4 blocks, and the wait for it.  args are the
// kernel's own parameter list; e names the entry in a device error.
template <class... Params, class... Args>
int launch_accumulate(const std::string& e, int device, void (*kernel)(Params...), uint32_t w, uint32_t h, void* hip_stream,
                      Args... args) {
    int err = rt_internal_bind_device(device);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((w + 63) / 64, (h + 3) / 4);
    kernel<<<grid, 256, 0, stream>>>(args...);
    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess) herr = hipStreamSynchronize(stream);
    if (herr != hipSuccess) return fail(RT_ERROR_DEVICE, e + ": " + hipGetErrorString(herr));
    return RT_OK;
}

// The host entries of the motion and deform stages, after their checks: one device allocation, the copies in, the
// device entry (run, which gets the arguments with device pointers in place of the host's) and the copies out.  Per
// pixel: current 16, two G-buffers 64, two histories 32, two moments 16, velocity 8 and two lengths 8 bytes, then the
// motion table.  with_surface (the deform and clip entries) puts the surface records (16 bytes per pixel) in front of
// the motion table and the deform table behind it on a 16-byte boundary.  The clip entry's neighbourhood texels (32
// bytes per pixel) and clip amounts (4) follow all that, the texels on a 16-byte boundary, when the caller has them.
template <class Run>
int stage_accumulate(const std::string& e, int device, const TaArgs& a, bool with_surface, Run run) {
    int err = rt_internal_bind_device(device);
    if (err) return err;
    const size_t n = (size_t)a.w*a.h;
    const size_t motion_bytes = sizeof(rt_motion_entry)*(size_t)(a.motion_count ? a.motion_count : 1u);
    const size_t motion_at = (with_surface ? 160 : 144)*n;
    const size_t deform_at = motion_at + ((motion_bytes + 15) & ~(size_t)15);
    const size_t tables_end = with_surface ? deform_at + sizeof(rt_deform_entry)*(size_t)(a.deform_count ? a.deform_count : 1u)
                                           : motion_at + motion_bytes;
    const size_t texels_at = (tables_end + 15) & ~(size_t)15;
    const size_t amount_at = texels_at + (a.neighbourhood ? sizeof(rt_neighbourhood_texel)*n : 0);
    const size_t bytes = a.neighbourhood || a.clip_amount ? amount_at + (a.clip_amount ? 4*n : 0) : tables_end;
    char* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_cur = reinterpret_cast<float*>(d);
    rt_gbuffer_texel* d_g[2] = {reinterpret_cast<rt_gbuffer_texel*>(d + 16*n), reinterpret_cast<rt_gbuffer_texel*>(d + 48*n)};
    float* d_h[2] = {reinterpret_cast<float*>(d + 80*n), reinterpret_cast<float*>(d + 96*n)};
    float* d_m[2] = {reinterpret_cast<float*>(d + 112*n), reinterpret_cast<float*>(d + 120*n)};
    float* d_v = reinterpret_cast<float*>(d + 128*n);
    float* d_l[2] = {reinterpret_cast<float*>(d + 136*n), reinterpret_cast<float*>(d + 140*n)};
    rt_surface_texel* d_s = reinterpret_cast<rt_surface_texel*>(d + 144*n);          // with_surface only
    rt_motion_entry* d_t = reinterpret_cast<rt_motion_entry*>(d + motion_at);
    rt_deform_entry* d_e = reinterpret_cast<rt_deform_entry*>(d + deform_at);        // with_surface only
    rt_neighbourhood_texel* d_nb = reinterpret_cast<rt_neighbourhood_texel*>(d + texels_at);     // the clip entry only
    float* d_ca = reinterpret_cast<float*>(d + amount_at);                                       // the clip entry only
    const bool prev = a.prev_history != nullptr;
    if (hipMemcpy(d_cur, a.current, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_g[0], a.gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
        (a.surface && hipMemcpy(d_s, a.surface, 16*n, hipMemcpyHostToDevice) != hipSuccess) ||
        (a.motion_count && hipMemcpy(d_t, a.motion, sizeof(rt_motion_entry)*(size_t)a.motion_count, hipMemcpyHostToDevice) != hipSuccess) ||
        (a.deform_count && hipMemcpy(d_e, a.deform, sizeof(rt_deform_entry)*(size_t)a.deform_count, hipMemcpyHostToDevice) != hipSuccess) ||
        (a.neighbourhood && hipMemcpy(d_nb, a.neighbourhood, sizeof(rt_neighbourhood_texel)*n, hipMemcpyHostToDevice) != hipSuccess) ||
        (prev && (hipMemcpy(d_h[1], a.prev_history, 16*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(d_l[1], a.prev_length, 4*n, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(d_g[1], a.prev_gbuffer, 32*n, hipMemcpyHostToDevice) != hipSuccess ||
                  (a.prev_moments && hipMemcpy(d_m[1], a.prev_moments, 8*n, hipMemcpyHostToDevice) != hipSuccess))))
        err = fail(RT_ERROR_DEVICE, e + ": copy in");
    TaArgs on = a;
    on.current = d_cur; on.gbuffer = d_g[0]; on.history = d_h[0]; on.length = d_l[0];
    on.prev_history = prev ? d_h[1] : nullptr; on.prev_length = prev ? d_l[1] : nullptr; on.prev_gbuffer = prev ? d_g[1] : nullptr;
    on.motion = a.motion_count ? d_t : nullptr;
    on.prev_moments = a.prev_moments ? d_m[1] : nullptr; on.moments = a.moments ? d_m[0] : nullptr;
    on.velocity = a.velocity ? d_v : nullptr;
    on.surface = a.surface ? d_s : nullptr; on.deform = a.deform_count ? d_e : nullptr;
    on.neighbourhood = a.neighbourhood ? d_nb : nullptr; on.clip_amount = a.clip_amount ? d_ca : nullptr;
    if (!err) err = run(on);
    if (!err && (hipMemcpy(a.history, d_h[0], 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(a.length, d_l[0], 4*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (a.moments && hipMemcpy(a.moments, d_m[0], 8*n, hipMemcpyDeviceToHost) != hipSuccess) ||
                 (a.velocity && hipMemcpy(a.velocity, d_v, 8*n, hipMemcpyDeviceToHost) != hipSuccess) ||
                 (a.clip_amount && hipMemcpy(a.clip_amount, d_ca, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

// ---- what the drivers share (rt_render_temporal_device and its motion, deform and filtered kin)

// The first 120 bytes per pixel of the plain, motion and deform drivers' workspaces: the current frame, then two
// sets of {G-buffer, history, length}.  The motion table follows on a 16-byte boundary in the latter two.
struct TaWorkspace {
    float* current;
    rt_gbuffer_texel* gbuffer[2];
    float* history[2];
    float* length[2];
};
TaWorkspace carve_temporal(void* d_workspace, size_t n) {
    char* base = static_cast<char*>(d_workspace);
    TaWorkspace ws;
    ws.current = reinterpret_cast<float*>(base);
    for (int k = 0; k < 2; ++k) {
        ws.gbuffer[k] = reinterpret_cast<rt_gbuffer_texel*>(base + 16*n + (size_t)k*32*n);
        ws.history[k] = reinterpret_cast<float*>(base + 80*n + (size_t)k*16*n);
        ws.length[k] = reinterpret_cast<float*>(base + 112*n + (size_t)k*4*n);
    }
    return ws;
}
size_t motion_table_offset(size_t n) { return (120*n + 15) & ~(size_t)15; }

// The plain, motion and deform drivers' checks.  The parameters first and the scene last: what needs no scene is
// refused without one.  A motion state (the motion and deform drivers') has its transforms checked as well.
template <class State>
int check_driver(const std::string& e, const rt_scene* s, const rt_camera* camera, const rt_settings* st,
                 const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t w, uint32_t h, const rt_temporal_params* p,
                 const State* state, const void* out, const char* out_name) {
    constexpr bool motion = std::is_same<State, rt_temporal_motion_state>::value;
    const std::string sn = motion ? "rt_temporal_motion_state" : "rt_temporal_state";
    int err = check_params(e, p);
    if (err) return err;
    if (!state) return fail(RT_ERROR_INVALID, e + ": null " + sn);
    if (!state->d_workspace) return fail(RT_ERROR_INVALID, e + ": " + sn + ": null d_workspace");
    if constexpr (motion) {
        if (!state->transforms) return fail(RT_ERROR_INVALID, e + ": " + sn + ": null transforms");
    }
    if (state->parity > 1u) return fail(RT_ERROR_INVALID, e + ": " + sn + ": parity must be 0 or 1");
    if (!st) return fail(RT_ERROR_INVALID, e + ": null settings");
    if (!w) return fail(RT_ERROR_INVALID, e + ": w is 0");
    if (!h) return fail(RT_ERROR_INVALID, e + ": h is 0");
    if (!camera) return fail(RT_ERROR_INVALID, e + ": null camera");
    if (!filter) return fail(RT_ERROR_INVALID, e + ": null filter");
    if (!tiles) return fail(RT_ERROR_INVALID, e + ": null tiles");
    if (!out) return fail(RT_ERROR_INVALID, e + ": null " + out_name);
    if (!s) return fail(RT_ERROR_INVALID, e + ": null scene");
    if constexpr (motion) {
        uint32_t count = 0;
        err = rt_scene_primitive_transforms(s, 0, nullptr, &count);
        if (err) return err;
        if (state->transform_cap < count)
            return fail(RT_ERROR_INVALID, e + ": " + sn + ": transform_cap is below the scene's primitive count");
    }
    return RT_OK;
}

// A driver's frame: `current` cleared, rt_render_device into it, and a look at the cancel flag (a frame clears it
// when its loop starts, so one raised after that is seen here).
int render_current(const std::string& e, rt_scene* s, const rt_camera* camera, const rt_settings* st, const rt_filter_cache* filter,
                   const rt_tile_set* tiles, uint32_t total_frame_index, uint32_t w, uint32_t h, uint32_t frame_count,
                   float* d_current, void* hip_stream, rt_stats* stats) {
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (hipMemsetAsync(d_current, 0, 16*(size_t)w*h, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": hipMemset");
    int err = rt_render_device(s, camera, st, filter, tiles, total_frame_index, w, h, frame_count, d_current, hip_stream, stats);
    if (err) return err;
    if (rt_internal_scene_cancelled(s)) return fail(RT_ERROR_CANCELLED, "render cancelled");
    return RT_OK;
}

// the plain, motion and deform drivers' outputs: the new history and, when asked for, its length
int copy_out_history(const std::string& e, const TaWorkspace& ws, uint32_t cur, size_t n, float* d_out, float* d_length_out,
                     void* hip_stream) {
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (hipMemcpyAsync(d_out, ws.history[cur], 16*n, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
        (d_length_out && hipMemcpyAsync(d_length_out, ws.length[cur], 4*n, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail(RT_ERROR_DEVICE, e + ": copy out");
    return RT_OK;
}

// a finished frame becomes the state's previous one
template <class State>
void advance_state(State* state, uint32_t w, uint32_t h, const rt_camera* camera, const rt_settings* st) {
    state->w = w; state->h = h;
    state->camera = *camera;
    state->lens_distortion = st->lens_distortion;
    state->parity ^= 1u;
    state->frames += 1u;
}

// The host twin of the plain, motion or deform driver, after its checks: the device driver (run) into a history and
// a length on the device, copied out.
template <class Run>
int render_to_host(const std::string& e, const rt_scene* s, uint32_t w, uint32_t h, float* out_pixels, float* out_length, Run run) {
    int err = rt_internal_bind_device(rt_internal_scene_device(s));
    if (err) return err;
    const size_t n = (size_t)w*h;
    char* d = nullptr;                                      // the history, the length
    if (hipMalloc(&d, 20*n) != hipSuccess) return fail(RT_ERROR_OUT_OF_MEMORY, e + ": hipMalloc");
    float* d_out = reinterpret_cast<float*>(d);
    float* d_len = reinterpret_cast<float*>(d + 16*n);
    err = run(d_out, out_length ? d_len : nullptr);
    if (!err && (hipMemcpy(out_pixels, d_out, 16*n, hipMemcpyDeviceToHost) != hipSuccess ||
                 (out_length && hipMemcpy(out_length, d_len, 4*n, hipMemcpyDeviceToHost) != hipSuccess)))
        err = fail(RT_ERROR_DEVICE, e + ": copy out");
    (void)hipFree(d);
    return err;
}

}  // namespace
