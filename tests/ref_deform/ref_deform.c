/*
 * ref_deform.c — CPU checker for the history that follows deforming meshes: the point and the shading normal of a
 * surface record under given vertices, normals and transform rows (ref_deform_surface) and the deform-aware
 * accumulate stage (rt_temporal_accumulate_deform / _device).  TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over tests/ref_motion/ref_motion.c (itself one over tests/ref_svgf/ref_svgf.c, tests/ref_temporal/
 * ref_temporal.c and oracle/oracle.c): the motion case is ref_motion's mo_point and mo_dir, the normal is the oracle's
 * own normalize, cross, xform_normal and noz in the order of its :NormalCalculation.  The stage is restated in plain C
 * in the operation order DESIGN.md defines ("Deforming meshes keep their history").  Built with the oracle's own
 * flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the GPU path.
 */
#include "../ref_motion/ref_motion.c"

/* One surface record under a mesh's vertices (9 floats a triangle, original order), its normals (likewise, or NULL),
 * forward rows `fwd` and inverse rows `inv`: the world point Q and the shading normal n. */
static void de_surface(const float* triangles, const float* normals, const float fwd[3][4], const float inv[3][4],
                       uint32_t triangle, float v, float w, rt_v3* Q, rt_v3* n) {
    const float* vt = triangles + 9*(size_t)triangle;
    V3 a = v3(vt[0], vt[1], vt[2]);
    V3 e1 = sub(v3(vt[3], vt[4], vt[5]), a), e2 = sub(v3(vt[6], vt[7], vt[8]), a);
    rt_v3 po;
    po.x = (a.x + v*e1.x) + w*e2.x;
    po.y = (a.y + v*e1.y) + w*e2.y;
    po.z = (a.z + v*e1.z) + w*e2.z;
    *Q = mo_point(fwd, po);
    V3 no;
    if (normals) {
        const float* nt = normals + 9*(size_t)triangle;
        float u = 1.0f - v - w;
        no = add(add(smul(u, v3(nt[0], nt[1], nt[2])), smul(v, v3(nt[3], nt[4], nt[5]))), smul(w, v3(nt[6], nt[7], nt[8])));
    } else {
        no = cross(normalize(e1), normalize(e2));
    }
    rt_m4x4 m;
    memset(&m, 0, sizeof(m));
    memcpy(m.e, inv, 48);               /* xform_normal reads rows 0..2 only */
    V3 r = noz(xform_normal(&m, no));
    n->x = r.x; n->y = r.y; n->z = r.z;
}

/* `count` records (triangle[i], vw[2*i], vw[2*i + 1]) -> Q and n, 3 floats each */
REF_API void ref_deform_surface(const float* triangles, const float* normals, const float* fwd, const float* inv, uint32_t count,
                                const uint32_t* triangle, const float* vw, float* Q, float* n) {
    float f[3][4], iv[3][4];
    memcpy(f, fwd, 48); memcpy(iv, inv, 48);
    for (uint32_t i = 0; i < count; ++i) {
        rt_v3 q, nn;
        de_surface(triangles, normals, f, iv, triangle[i], vw[2*i], vw[2*i + 1], &q, &nn);
        Q[3*i] = q.x; Q[3*i + 1] = q.y; Q[3*i + 2] = q.z;
        n[3*i] = nn.x; n[3*i + 1] = nn.y; n[3*i + 2] = nn.z;
    }
}

/* rt_temporal_accumulate_deform: ref_temporal_accumulate_motion's text with the deform case before the motion case.
 * The entries' vertex pointers are host pointers here. */
REF_API int ref_temporal_accumulate_deform(const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                           const float* prev_length, const rt_gbuffer_texel* prev_gbuffer,
                                           const rt_camera* prev_camera, float prev_lens_distortion, uint32_t w, uint32_t h,
                                           const rt_temporal_params* p, float* history, float* length,
                                           const rt_motion_entry* motion, uint32_t motion_count, const float* prev_moments,
                                           float* moments, float* velocity, const rt_surface_texel* surface,
                                           const rt_deform_entry* deform, uint32_t deform_count) {
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
