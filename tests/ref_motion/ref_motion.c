/*
 * ref_motion.c — CPU checker for the history that follows moving instances: the motion table (rt_motion_table) and
 * the motion-aware accumulate stage (rt_temporal_accumulate_motion / _device).  TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over tests/ref_svgf/ref_svgf.c (itself one over tests/ref_temporal/ref_temporal.c and oracle/
 * oracle.c): the projection is ref_temporal's project_prev, the tonemapped luminance ref_svgf's sv_tm.  The table
 * and the stage are restated in plain C in the operation order DESIGN.md defines ("Moving instances").  Built with
 * the oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the GPU path.
 */
#include "../ref_svgf/ref_svgf.c"

REF_API void ref_motion_table(uint32_t count, const rt_m4x4inv* cur, const rt_m4x4inv* prev, rt_motion_entry* out) {
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t moved = 0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                uint32_t a, b;
                out[i].inv_cur[r][c] = cur[i].inverse.e[r][c];
                out[i].fwd_prev[r][c] = prev[i].forward.e[r][c];
                memcpy(&a, &cur[i].forward.e[r][c], 4); memcpy(&b, &prev[i].forward.e[r][c], 4);
                if (a != b) moved = 1;
                memcpy(&a, &cur[i].inverse.e[r][c], 4); memcpy(&b, &prev[i].inverse.e[r][c], 4);
                if (a != b) moved = 1;
            }
        out[i].moved = moved;
        out[i].reserved[0] = out[i].reserved[1] = out[i].reserved[2] = 0;
    }
}

static rt_v3 mo_point(const float a[3][4], rt_v3 v) {
    rt_v3 o;
    o.x = ((a[0][0]*v.x + a[0][1]*v.y) + a[0][2]*v.z) + a[0][3];
    o.y = ((a[1][0]*v.x + a[1][1]*v.y) + a[1][2]*v.z) + a[1][3];
    o.z = ((a[2][0]*v.x + a[2][1]*v.y) + a[2][2]*v.z) + a[2][3];
    return o;
}
static rt_v3 mo_dir(const float a[3][4], rt_v3 v) {
    rt_v3 o;
    o.x = (a[0][0]*v.x + a[0][1]*v.y) + a[0][2]*v.z;
    o.y = (a[1][0]*v.x + a[1][1]*v.y) + a[1][2]*v.z;
    o.z = (a[2][0]*v.x + a[2][1]*v.y) + a[2][2]*v.z;
    return o;
}

/* Q and the carried normal of `count` points under one entry (the step alone, for the float64 comparison) */
REF_API void ref_motion_carry(const rt_motion_entry* e, uint32_t count, const float* P, const float* n, float* Q, float* m) {
    for (uint32_t i = 0; i < count; ++i) {
        rt_v3 p = { P[3*i], P[3*i + 1], P[3*i + 2] }, nn = { n[3*i], n[3*i + 1], n[3*i + 2] };
        rt_v3 q = mo_point(e->fwd_prev, mo_point(e->inv_cur, p));
        rt_v3 d = mo_dir(e->fwd_prev, mo_dir(e->inv_cur, nn));
        float len = sqrtf(dot3(d, d));
        if (len > 0.0f) { nn.x = d.x / len; nn.y = d.y / len; nn.z = d.z / len; }
        Q[3*i] = q.x; Q[3*i + 1] = q.y; Q[3*i + 2] = q.z;
        m[3*i] = nn.x; m[3*i + 1] = nn.y; m[3*i + 2] = nn.z;
    }
}

/* rt_temporal_accumulate_motion: moments and prev_moments (both or, without history, moments alone) and velocity
 * are optional */
REF_API int ref_temporal_accumulate_motion(const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                           const float* prev_length, const rt_gbuffer_texel* prev_gbuffer,
                                           const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                           const rt_temporal_params* p, float* history, float* length,
                                           const rt_motion_entry* motion, uint32_t motion_count, const float* prev_moments,
                                           float* moments, float* velocity) {
    uint32_t nan_bits = 0x7FC00000u;
    float qnan;
    memcpy(&qnan, &nan_bits, 4);
    for (uint32_t y = 0; y < h; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            size_t i = (size_t)y*w + x;
            const float* s = &current[4*i];
            float* out = &history[4*i];
            float vx = qnan, vy = qnan;
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
                if (moments) { moments[2*i] = 0.0f; moments[2*i + 1] = 0.0f; }
                if (velocity) { velocity[2*i] = vx; velocity[2*i + 1] = vy; }
                continue;
            }
            /* 2. clamp */
            cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
            if (p->firefly_clamp > 0.0f) {
                cr = cr < p->firefly_clamp ? cr : p->firefly_clamp;
                cg = cg < p->firefly_clamp ? cg : p->firefly_clamp;
                cb = cb < p->firefly_clamp ? cb : p->firefly_clamp;
            }
            float t = 0.0f, t2 = 0.0f;
            if (moments) { t = sv_tm(cr, cg, cb); t2 = t*t; }
            SvTapSum sum = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
            if (prev_history) {
                /* 3. the point and its place in the previous frame */
                rt_gbuffer_texel g = gbuffer[i];
                rt_v3 P = g.p;
                if (g.primitive == RT_HIT_MISS) {
                    P.x = prev_camera->p.x + g.p.x; P.y = prev_camera->p.y + g.p.y; P.z = prev_camera->p.z + g.p.z;
                }
                /* 3m. a moved primitive's point and normal, carried to where they were */
                if (motion && !(g.primitive & RT_HIT_PLANE_BIT) && g.primitive < motion_count && motion[g.primitive].moved != 0) {
                    const rt_motion_entry* e = &motion[g.primitive];
                    P = mo_point(e->fwd_prev, mo_point(e->inv_cur, P));
                    rt_v3 d = mo_dir(e->fwd_prev, mo_dir(e->inv_cur, g.n));
                    float len = sqrtf(dot3(d, d));
                    if (len > 0.0f) { g.n.x = d.x / len; g.n.y = d.y / len; g.n.z = d.z / len; }
                }
                float fx, fy;
                if (project_prev(prev_camera, prev_lens_distortion, P, w, h, &fx, &fy)) {
                    vx = fx - (float)x; vy = fy - (float)y;
                    /* 4. the taps */
                    float plane_limit = p->plane_tolerance*g.t;
                    float rx = rintf(fx), ry = rintf(fy);
                    if (fabsf(fx - rx) <= p->snap && fabsf(fy - ry) <= p->snap) {
                        if (moments) sv_add_tap(&sum, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, prev_moments, &g, P, p->normal_cos, plane_limit);
                        else add_tap((TapSum*)&sum, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, &g, P, p->normal_cos, plane_limit);
                    } else {
                        float x0 = floorf(fx), y0 = floorf(fy);
                        float tx = fx - x0, ty = fy - y0;
                        int ix = (int)x0, iy = (int)y0;
                        float wt[4] = { (1.0f - tx)*(1.0f - ty), tx*(1.0f - ty), (1.0f - tx)*ty, tx*ty };
                        for (int k = 0; k < 4; ++k) {
                            if (moments) sv_add_tap(&sum, ix + (k & 1), iy + (k >> 1), wt[k], w, h, prev_history, prev_length, prev_gbuffer, prev_moments, &g, P, p->normal_cos, plane_limit);
                            else add_tap((TapSum*)&sum, ix + (k & 1), iy + (k >> 1), wt[k], w, h, prev_history, prev_length, prev_gbuffer, &g, P, p->normal_cos, plane_limit);
                        }
                    }
                }
            }
            if (velocity) { velocity[2*i] = vx; velocity[2*i + 1] = vy; }
            /* 5. the blend */
            if (sum.W > 0.0f) {
                float hr = sum.r / sum.W, hg = sum.g / sum.W, hb = sum.b / sum.W;
                float L = sum.L / sum.W;
                float h1 = sum.S1 / sum.W, h2 = sum.S2 / sum.W;
                float N = L + 1.0f;
                N = N < p->max_history ? N : p->max_history;
                float a = 1.0f / N;
                if (N == 1.0f) {
                    out[0] = cr; out[1] = cg; out[2] = cb;
                    if (moments) { moments[2*i] = t; moments[2*i + 1] = t2; }
                } else {
                    out[0] = hr + (cr - hr)*a; out[1] = hg + (cg - hg)*a; out[2] = hb + (cb - hb)*a;
                    if (moments) { moments[2*i] = h1 + (t - h1)*a; moments[2*i + 1] = h2 + (t2 - h2)*a; }
                }
                out[3] = 1.0f;
                length[i] = N;
            } else {
                out[0] = cr; out[1] = cg; out[2] = cb; out[3] = 1.0f;
                length[i] = 1.0f;
                if (moments) { moments[2*i] = t; moments[2*i + 1] = t2; }
            }
        }
    }
    return RT_OK;
}
