/*
 * ref_clip.c — CPU checker for neighbourhood clipping of the temporal history: the statistics of the current frame's
 * windows (rt_temporal_neighbourhood / _device) and the accumulate stage with a clip (rt_temporal_accumulate_clip /
 * _device).  TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over tests/ref_deform/ref_deform.c (itself one over ref_motion.c, ref_svgf.c, ref_temporal.c and
 * oracle/oracle.c): the deform case is ref_deform's de_surface, the motion case ref_motion's mo_point and mo_dir.  Both
 * stages are restated in plain C in the operation order DESIGN.md defines ("Neighbourhood clipping").  Built with the
 * oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the GPU path.
 */
#include "../ref_deform/ref_deform.c"

/* a pixel's value: the accumulate stage's steps 1 and 2; {r, g, b, 1} when valid, +0 four times otherwise */
static void cl_value(const float* current, uint32_t w, uint32_t h, int64_t x, int64_t y, float firefly_clamp, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (x < 0 || y < 0 || x >= (int64_t)w || y >= (int64_t)h) return;
    const float* s = &current[4*((size_t)y*w + (size_t)x)];
    if (!(s[3] > 0.001f)) return;
    float cr = s[0] / s[3], cg = s[1] / s[3], cb = s[2] / s[3];
    if (!(finite_bits(cr) && finite_bits(cg) && finite_bits(cb))) return;
    cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
    if (firefly_clamp > 0.0f) {
        cr = cr < firefly_clamp ? cr : firefly_clamp;
        cg = cg < firefly_clamp ? cg : firefly_clamp;
        cb = cb < firefly_clamp ? cb : firefly_clamp;
    }
    v[0] = cr; v[1] = cg; v[2] = cb; v[3] = 1.0f;
}

/* the seven row sums H(x, y) of radius r, in the stated order */
static void cl_row(const float* current, uint32_t w, uint32_t h, int64_t x, int64_t y, int r, float firefly_clamp, float H[7]) {
    float v[4];
    cl_value(current, w, h, x - r, y, firefly_clamp, v);
    H[0] = v[0]; H[1] = v[1]; H[2] = v[2];
    H[3] = v[0]*v[0]; H[4] = v[1]*v[1]; H[5] = v[2]*v[2];
    H[6] = v[3];
    for (int d = 1; d <= 2*r; ++d) {
        cl_value(current, w, h, x - r + d, y, firefly_clamp, v);
        H[0] = H[0] + v[0]; H[1] = H[1] + v[1]; H[2] = H[2] + v[2];
        H[3] = H[3] + v[0]*v[0]; H[4] = H[4] + v[1]*v[1]; H[5] = H[5] + v[2]*v[2];
        H[6] = H[6] + v[3];
    }
}

/* rt_temporal_neighbourhood: out is 8 floats per pixel {mean, count, sigma, reserved} */
REF_API int ref_temporal_neighbourhood(const float* current, uint32_t w, uint32_t h, uint32_t radius, float firefly_clamp,
                                       float* out) {
    int r = (int)radius;
    for (uint32_t y = 0; y < h; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            float S[7], H[7];
            cl_row(current, w, h, x, (int64_t)y - r, r, firefly_clamp, S);
            for (int d = 1; d <= 2*r; ++d) {
                cl_row(current, w, h, x, (int64_t)y - r + d, r, firefly_clamp, H);
                for (int c = 0; c < 7; ++c) S[c] = S[c] + H[c];
            }
            float* t = &out[8*((size_t)y*w + x)];
            for (int c = 0; c < 8; ++c) t[c] = 0.0f;
            float n = S[6];
            if (n > 0.0f) {
                for (int c = 0; c < 3; ++c) {
                    float mean = S[c] / n;
                    float var = S[3 + c] / n - mean*mean;
                    var = var > 0.0f ? var : 0.0f;
                    t[c] = mean;
                    t[4 + c] = sqrtf(var);
                }
                t[3] = n;
            }
        }
    }
    return RT_OK;
}

/* rt_temporal_accumulate_clip: ref_temporal_accumulate_deform's text with step 4c between the taps and the blend.
 * neighbourhood is 8 floats per pixel or NULL; clip_amount one float per pixel or NULL. */
REF_API int ref_temporal_accumulate_clip(const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                         const float* prev_length, const rt_gbuffer_texel* prev_gbuffer,
                                         const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                         const rt_temporal_params* p, float* history, float* length,
                                         const rt_motion_entry* motion, uint32_t motion_count, const float* prev_moments,
                                         float* moments, float* velocity, const rt_surface_texel* surface,
                                         const rt_deform_entry* deform, uint32_t deform_count, const float* neighbourhood,
                                         float gamma, float min_count, float* clip_amount) {
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
                if (clip_amount) clip_amount[i] = 0.0f;
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
                int hit_id = !(g.primitive & RT_HIT_PLANE_BIT);
                /* 3d. a deformed mesh's surface point and normal, as last frame's vertices and transform gave them */
                if (deform && hit_id && g.primitive < deform_count && deform[g.primitive].deformed != 0 &&
                    surface[i].triangle < deform[g.primitive].triangle_count) {
                    const rt_deform_entry* e = &deform[g.primitive];
                    de_surface(e->d_prev_triangles, e->has_normals ? e->d_prev_normals : NULL, e->fwd_prev, e->inv_prev,
                               surface[i].triangle, surface[i].v, surface[i].w, &P, &g.n);
                }
                /* 3m. else a moved primitive's point and normal, carried to where they were */
                else if (motion && hit_id && g.primitive < motion_count && motion[g.primitive].moved != 0) {
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
            float clipped = 0.0f;
            if (sum.W > 0.0f) {
                float hist[3] = { sum.r / sum.W, sum.g / sum.W, sum.b / sum.W };
                /* 4c. the history clipped to the neighbourhood's box */
                if (neighbourhood && neighbourhood[8*i + 3] >= min_count) {
                    const float* nt = &neighbourhood[8*i];
                    float d[3];
                    for (int k = 0; k < 3; ++k) {
                        float before = hist[k];
                        float lo = nt[k] - gamma*nt[4 + k], hi = nt[k] + gamma*nt[4 + k];
                        hist[k] = hist[k] < lo ? lo : hist[k];
                        hist[k] = hist[k] > hi ? hi : hist[k];
                        d[k] = fabsf(before - hist[k]);
                    }
                    clipped = d[0];
                    clipped = d[1] > clipped ? d[1] : clipped;
                    clipped = d[2] > clipped ? d[2] : clipped;
                }
                /* 5. the blend */
                float hr = hist[0], hg = hist[1], hb = hist[2];
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
            if (clip_amount) clip_amount[i] = clipped;
        }
    }
    return RT_OK;
}
