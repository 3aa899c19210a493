/*
 * ref_temporal.c — CPU checker for temporal accumulation: the primary-hit G-buffer (rt_gbuffer / rt_gbuffer_device)
 * and the accumulate stage (rt_temporal_accumulate / rt_temporal_accumulate_device).  TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over oracle/oracle.c, as tests/ref_features is: the G-buffer half is the camera ray of DESIGN.md
 * ("Temporal accumulation") built from the oracle's cam_setup, apply_lens_distortion and normalize, followed by
 * oracle_debug_intersect.  The stage is restated in plain C in the operation order DESIGN.md defines.  Built with
 * the oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the GPU path.
 */
#include "../../oracle/oracle.c"

#include <stdlib.h>

#define REF_API __attribute__((visibility("default")))

enum { TA_NEWTON_STEPS = 5 };

/* ---- the G-buffer */

/* The ray of pixel (x, y): render_tile's camera ray with jitter 0 and no lens offset. */
static void gbuffer_ray(const CamSetup* c, float lens_distortion, uint32_t w, uint32_t h, uint32_t x, uint32_t y,
                        V3* ray_o, V3* ray_d) {
    float v = 1.0f - 2.0f*(float)y*c->pixel_h;
    float u = 1.0f - 2.0f*(float)x*c->pixel_w;
    apply_lens_distortion(lens_distortion, w, h, &u, &v);
    V3 film_p = c->film_center;
    film_p = add(film_p, smul(u*c->hfw, c->cx));
    film_p = add(film_p, smul(v*c->hfh, c->cy));
    *ray_o = c->cp;
    *ray_d = normalize(sub(film_p, c->cp));
}

/* every pixel's ray direction, row-major (the origin is camera->p) */
REF_API void ref_gbuffer_rays(const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h, float* d) {
    CamSetup c = cam_setup(camera, w, h);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            V3 ro, rd;
            gbuffer_ray(&c, lens_distortion, w, h, x, y, &ro, &rd);
            float* o = &d[3*((size_t)y*w + x)];
            o[0] = rd.x; o[1] = rd.y; o[2] = rd.z;
        }
}

REF_API int ref_gbuffer(const rt_scene_desc* scene, const rt_camera* camera, float lens_distortion, uint32_t w, uint32_t h,
                        rt_gbuffer_texel* out) {
    CamSetup c = cam_setup(camera, w, h);
    for (uint32_t y = 0; y < h; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            rt_ray_query q;
            V3 ro, rd;
            gbuffer_ray(&c, lens_distortion, w, h, x, y, &ro, &rd);
            q.o = ro; q.d = rd; q.max_t = FLT_MAX; q.ignored_primitive = 0;
            rt_hit_record r;
            int err = oracle_debug_intersect(scene, 1, &q, 0, &r);
            if (err) return err;
            rt_gbuffer_texel* g = &out[(size_t)y*w + x];
            if (r.primitive != RT_HIT_MISS) {
                g->p = r.hit_p; g->t = r.t; g->n = r.n; g->primitive = r.primitive;
            } else {
                g->p = rd; g->t = 0.0f; g->n.x = g->n.y = g->n.z = 0.0f; g->primitive = RT_HIT_MISS;
            }
        }
    }
    return RT_OK;
}

/* ---- the accumulate stage */

static int finite_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}
static float dot3(rt_v3 a, rt_v3 b) { return (a.x*b.x + a.y*b.y) + a.z*b.z; }

/* The position of world point P in the previous frame, in pixels.  0: no history. */
static int project_prev(const rt_camera* cam, float amount, rt_v3 P, uint32_t w, uint32_t h, float* fx, float* fy) {
    rt_v3 d = { P.x - cam->p.x, P.y - cam->p.y, P.z - cam->p.z };
    float z = -dot3(d, cam->z);
    if (!(z > 0.0f)) return 0;
    float u = (dot3(d, cam->x)*cam->film_distance) / (z*cam->half_film_w);
    float v = (dot3(d, cam->y)*cam->film_distance) / (z*cam->half_film_h);
    float woh = (float)w / (float)h;
    float bd1 = 0.1f*amount, bd2 = -0.025f*amount;
    if (amount > 0.0f) {
        float cy = 1.0f / woh;
        float c2 = 1.0f*1.0f + cy*cy;
        float cf = 1.0f + c2*bd1 + c2*c2*bd2;
        u = u*cf;
        v = v*((cy*cf)*woh);
    }
    float X = u, Y = v / woh;
    float R = sqrtf(X*X + Y*Y);
    float iw = 1.0f / woh;
    float rc = sqrtf(1.0f + iw*iw);
    /* a point beyond the corner's own distorted radius lies outside the previous image */
    float rc2 = rc*rc;
    float Rc = (rc + bd1*(rc2*rc) + bd2*((rc2*rc2)*rc))*(1.0f + 1.0f/1024.0f);
    if (R > Rc) return 0;
    float r = R < rc ? R : rc;
    for (int k = 0; k < TA_NEWTON_STEPS; ++k) {
        float r2 = r*r;
        float g = (r + bd1*(r2*r) + bd2*((r2*r2)*r)) - R;
        float dg = 1.0f + (3.0f*bd1)*r2 + (5.0f*bd2)*(r2*r2);
        r = r - g / dg;
        r = r > 0.0f ? r : 0.0f;
        r = r < rc ? r : rc;
    }
    float scale = R > 0.0f ? r / R : 1.0f;
    u = u*scale;
    v = v*scale;
    *fx = (1.0f - u)*((float)w*0.5f);
    *fy = (1.0f - v)*((float)h*0.5f);
    return *fx >= -1.0f && *fx < (float)w && *fy >= -1.0f && *fy < (float)h;
}

REF_API int ref_temporal_project(const rt_camera* cam, float lens_distortion, const float* P, uint32_t w, uint32_t h,
                                 float* fx, float* fy) {
    rt_v3 p = { P[0], P[1], P[2] };
    *fx = 0.0f; *fy = 0.0f;
    return project_prev(cam, lens_distortion, p, w, h, fx, fy);
}

REF_API void ref_temporal_project_many(const rt_camera* cam, float lens_distortion, const float* P, uint32_t count,
                                       uint32_t w, uint32_t h, float* fx, float* fy, int32_t* ok) {
    for (uint32_t i = 0; i < count; ++i) {
        rt_v3 p = { P[3*i], P[3*i + 1], P[3*i + 2] };
        fx[i] = 0.0f; fy[i] = 0.0f;
        ok[i] = project_prev(cam, lens_distortion, p, w, h, &fx[i], &fy[i]);
    }
}

typedef struct { float W, r, g, b, L; } TapSum;

static void add_tap(TapSum* s, int qx, int qy, float wt, uint32_t w, uint32_t h, const float* prev_history,
                    const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const rt_gbuffer_texel* g, rt_v3 P,
                    float normal_cos, float plane_limit) {
    if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) return;
    size_t q = (size_t)qy*w + (size_t)qx;
    float len = prev_length[q];
    if (!(len >= 1.0f)) return;
    const rt_gbuffer_texel* pg = &prev_gbuffer[q];
    if (pg->primitive != g->primitive) return;
    if (g->primitive != RT_HIT_MISS) {
        if (!(dot3(g->n, pg->n) >= normal_cos)) return;
        rt_v3 off = { pg->p.x - P.x, pg->p.y - P.y, pg->p.z - P.z };
        if (!(fabsf(dot3(off, g->n)) <= plane_limit)) return;
    }
    const float* ph = &prev_history[4*q];
    if (!(finite_bits(ph[0]) && finite_bits(ph[1]) && finite_bits(ph[2]))) return;
    s->W = s->W + wt;
    s->r = s->r + wt*ph[0];
    s->g = s->g + wt*ph[1];
    s->b = s->b + wt*ph[2];
    s->L = s->L + wt*len;
}

REF_API int ref_temporal_accumulate(const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                    const float* prev_length, const rt_gbuffer_texel* prev_gbuffer,
                                    const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                    const rt_temporal_params* p, float* history, float* length) {
    for (uint32_t y = 0; y < h; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            size_t i = (size_t)y*w + x;
            const float* s = &current[4*i];
            float* out = &history[4*i];
            /* 1. validity */
            int valid = s[3] > 0.001f;
            float cr = 0.0f, cg = 0.0f, cb = 0.0f;
            if (valid) {
                cr = s[0] / s[3]; cg = s[1] / s[3]; cb = s[2] / s[3];
                valid = finite_bits(cr) && finite_bits(cg) && finite_bits(cb);
            }
            if (!valid) {
                memcpy(out, s, 16);
                length[i] = 0.0f;
                continue;
            }
            /* 2. clamp */
            cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
            if (p->firefly_clamp > 0.0f) {
                cr = cr < p->firefly_clamp ? cr : p->firefly_clamp;
                cg = cg < p->firefly_clamp ? cg : p->firefly_clamp;
                cb = cb < p->firefly_clamp ? cb : p->firefly_clamp;
            }
            TapSum sum = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
            if (prev_history) {
                /* 3. the point and its place in the previous frame */
                const rt_gbuffer_texel* g = &gbuffer[i];
                rt_v3 P = g->p;
                if (g->primitive == RT_HIT_MISS) {
                    P.x = prev_camera->p.x + g->p.x; P.y = prev_camera->p.y + g->p.y; P.z = prev_camera->p.z + g->p.z;
                }
                float fx, fy;
                if (project_prev(prev_camera, prev_lens_distortion, P, w, h, &fx, &fy)) {
                    /* 4. the taps */
                    float plane_limit = p->plane_tolerance*g->t;
                    float rx = rintf(fx), ry = rintf(fy);
                    if (fabsf(fx - rx) <= p->snap && fabsf(fy - ry) <= p->snap) {
                        add_tap(&sum, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, g, P,
                                p->normal_cos, plane_limit);
                    } else {
                        float x0 = floorf(fx), y0 = floorf(fy);
                        float tx = fx - x0, ty = fy - y0;
                        int ix = (int)x0, iy = (int)y0;
                        add_tap(&sum, ix, iy, (1.0f - tx)*(1.0f - ty), w, h, prev_history, prev_length, prev_gbuffer, g, P,
                                p->normal_cos, plane_limit);
                        add_tap(&sum, ix + 1, iy, tx*(1.0f - ty), w, h, prev_history, prev_length, prev_gbuffer, g, P,
                                p->normal_cos, plane_limit);
                        add_tap(&sum, ix, iy + 1, (1.0f - tx)*ty, w, h, prev_history, prev_length, prev_gbuffer, g, P,
                                p->normal_cos, plane_limit);
                        add_tap(&sum, ix + 1, iy + 1, tx*ty, w, h, prev_history, prev_length, prev_gbuffer, g, P,
                                p->normal_cos, plane_limit);
                    }
                }
            }
            /* 5. the blend */
            if (sum.W > 0.0f) {
                float hr = sum.r / sum.W, hg = sum.g / sum.W, hb = sum.b / sum.W;
                float L = sum.L / sum.W;
                float N = L + 1.0f;
                N = N < p->max_history ? N : p->max_history;
                float a = 1.0f / N;
                if (N == 1.0f) { out[0] = cr; out[1] = cg; out[2] = cb; }
                else { out[0] = hr + (cr - hr)*a; out[1] = hg + (cg - hg)*a; out[2] = hb + (cb - hb)*a; }
                out[3] = 1.0f;
                length[i] = N;
            } else {
                out[0] = cr; out[1] = cg; out[2] = cb; out[3] = 1.0f;
                length[i] = 1.0f;
            }
        }
    }
    return RT_OK;
}
