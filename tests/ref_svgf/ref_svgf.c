/*
 * ref_svgf.c — CPU checker for variance-guided filtering of the temporal history: the accumulate stage with moments
 * (rt_temporal_accumulate_moments / _device), the variance of the history (rt_temporal_variance / _device) and the
 * variance-guided filter (rt_denoise_variance / _device).  TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over tests/ref_temporal/ref_temporal.c (itself one over oracle/oracle.c): the projection into the
 * previous frame is that checker's project_prev, the exponential the oracle's oracle_expf.  The three stages are
 * restated in plain C in the operation order DESIGN.md defines ("Variance-guided filtering").  Built with the
 * oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the GPU path.
 */
#include "../ref_temporal/ref_temporal.c"

static float sv_tm(float r, float g, float b) {
    float y = (0.2126f*r + 0.7152f*g) + 0.0722f*b;
    return 1.0f - oracle_expf(-y);
}
static int sv_bad(float v) { return !(v >= 0.0f) || v > FLT_MAX; }

/* ---- 1. accumulate with moments */

typedef struct { float W, r, g, b, L, S1, S2; } SvTapSum;

/* add_tap's rule and sums (tests/ref_temporal), and the previous moments beside them */
static void sv_add_tap(SvTapSum* s, int qx, int qy, float wt, uint32_t w, uint32_t h, const float* prev_history,
                       const float* prev_length, const rt_gbuffer_texel* prev_gbuffer, const float* prev_moments,
                       const rt_gbuffer_texel* g, rt_v3 P, float normal_cos, float plane_limit) {
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
    s->S1 = s->S1 + wt*prev_moments[2*q];
    s->S2 = s->S2 + wt*prev_moments[2*q + 1];
}

REF_API int ref_temporal_accumulate_moments(const float* current, const rt_gbuffer_texel* gbuffer, const float* prev_history,
                                            const float* prev_length, const rt_gbuffer_texel* prev_gbuffer,
                                            const float* prev_moments, const rt_camera* prev_camera,
                                            float prev_lens_distortion, uint32_t w, uint32_t h, const rt_temporal_params* p,
                                            float* history, float* length, float* moments) {
    for (uint32_t y = 0; y < h; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            size_t i = (size_t)y*w + x;
            const float* s = &current[4*i];
            float* out = &history[4*i];
            float* mo = &moments[2*i];
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
                mo[0] = 0.0f; mo[1] = 0.0f;
                continue;
            }
            /* 2. clamp */
            cr = cr > 0.0f ? cr : 0.0f; cg = cg > 0.0f ? cg : 0.0f; cb = cb > 0.0f ? cb : 0.0f;
            if (p->firefly_clamp > 0.0f) {
                cr = cr < p->firefly_clamp ? cr : p->firefly_clamp;
                cg = cg < p->firefly_clamp ? cg : p->firefly_clamp;
                cb = cb < p->firefly_clamp ? cb : p->firefly_clamp;
            }
            float t = sv_tm(cr, cg, cb), t2 = t*t;
            SvTapSum sum = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
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
                        sv_add_tap(&sum, (int)rx, (int)ry, 1.0f, w, h, prev_history, prev_length, prev_gbuffer, prev_moments, g,
                                   P, p->normal_cos, plane_limit);
                    } else {
                        float x0 = floorf(fx), y0 = floorf(fy);
                        float tx = fx - x0, ty = fy - y0;
                        int ix = (int)x0, iy = (int)y0;
                        sv_add_tap(&sum, ix, iy, (1.0f - tx)*(1.0f - ty), w, h, prev_history, prev_length, prev_gbuffer,
                                   prev_moments, g, P, p->normal_cos, plane_limit);
                        sv_add_tap(&sum, ix + 1, iy, tx*(1.0f - ty), w, h, prev_history, prev_length, prev_gbuffer,
                                   prev_moments, g, P, p->normal_cos, plane_limit);
                        sv_add_tap(&sum, ix, iy + 1, (1.0f - tx)*ty, w, h, prev_history, prev_length, prev_gbuffer,
                                   prev_moments, g, P, p->normal_cos, plane_limit);
                        sv_add_tap(&sum, ix + 1, iy + 1, tx*ty, w, h, prev_history, prev_length, prev_gbuffer,
                                   prev_moments, g, P, p->normal_cos, plane_limit);
                    }
                }
            }
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
                    mo[0] = t; mo[1] = t2;
                } else {
                    out[0] = hr + (cr - hr)*a; out[1] = hg + (cg - hg)*a; out[2] = hb + (cb - hb)*a;
                    mo[0] = h1 + (t - h1)*a; mo[1] = h2 + (t2 - h2)*a;
                }
                out[3] = 1.0f;
                length[i] = N;
            } else {
                out[0] = cr; out[1] = cg; out[2] = cb; out[3] = 1.0f;
                length[i] = 1.0f;
                mo[0] = t; mo[1] = t2;
            }
        }
    }
    return RT_OK;
}

/* ---- 2. the variance of the history */

/* counted[i] (may be NULL): how many taps of pixel i's window counted; 0 where no window was taken */
REF_API int ref_temporal_variance(const float* moments, const float* length, const rt_gbuffer_texel* gbuffer, uint32_t w,
                                  uint32_t h, const rt_temporal_params* p, float spatial_below, float* variance,
                                  uint32_t* counted) {
    for (int y = 0; y < (int)h; ++y) {
        for (int x = 0; x < (int)w; ++x) {
            size_t i = (size_t)y*w + (size_t)x;
            float len = length[i];
            if (counted) counted[i] = 0u;
            if (!(len >= 1.0f)) { variance[i] = 0.0f; continue; }
            float s2;
            if (len >= spatial_below) {
                s2 = moments[2*i + 1] - moments[2*i]*moments[2*i];
            } else {
                const rt_gbuffer_texel* g = &gbuffer[i];
                float plane_limit = p->plane_tolerance*g->t;
                float cnt = 0.0f, A1 = 0.0f, A2 = 0.0f;
                for (int dy = -3; dy <= 3; ++dy) for (int dx = -3; dx <= 3; ++dx) {
                    int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)h) continue;
                    size_t q = (size_t)qy*w + (size_t)qx;
                    if (dx != 0 || dy != 0) {
                        if (!(length[q] >= 1.0f)) continue;
                        const rt_gbuffer_texel* gq = &gbuffer[q];
                        if (gq->primitive != g->primitive) continue;
                        if (g->primitive != RT_HIT_MISS) {
                            if (!(dot3(g->n, gq->n) >= p->normal_cos)) continue;
                            rt_v3 off = { gq->p.x - g->p.x, gq->p.y - g->p.y, gq->p.z - g->p.z };
                            if (!(fabsf(dot3(off, g->n)) <= plane_limit)) continue;
                        }
                    }
                    cnt = cnt + 1.0f;
                    A1 = A1 + moments[2*q];
                    A2 = A2 + moments[2*q + 1];
                    if (counted) counted[i] += 1u;
                }
                float M1 = A1 / cnt, M2 = A2 / cnt;
                s2 = M2 - M1*M1;
            }
            s2 = s2 > 0.0f ? s2 : 0.0f;
            variance[i] = s2 / len;
        }
    }
    return RT_OK;
}

/* ---- 3. the variance-guided filter */

/* The arguments of rt_denoise_variance (`device` is ignored).  Returns RT_OK, or RT_ERROR_INVALID for the arguments
 * rt_denoise_variance refuses. */
REF_API int ref_denoise_variance(int device, const float* color, const float* variance, const rt_gbuffer_texel* gbuffer,
                                 uint32_t uw, uint32_t uh, const rt_denoise_variance_params* p, float* out_pixels,
                                 float* variance_out) {
    (void)device;
    if (!color || !variance || !gbuffer || !out_pixels || !p || !uw || !uh) return RT_ERROR_INVALID;
    if (p->iterations < 1 || p->iterations > 8) return RT_ERROR_INVALID;
    if (sv_bad(p->sigma_color) || sv_bad(p->sigma_normal) || sv_bad(p->sigma_plane) || sv_bad(p->firefly_clamp)) return RT_ERROR_INVALID;
    if (sv_bad(p->variance_epsilon) || !(p->variance_epsilon > 0.0f)) return RT_ERROR_INVALID;
    const int w = (int)uw, h = (int)uh;
    const size_t n = (size_t)w*(size_t)h;
    float* col[2];                              /* {r, g, b, l} per pixel, ping-pong */
    float* var[2];
    unsigned char* valid = (unsigned char*)malloc(n);
    col[0] = (float*)malloc(16*n); col[1] = (float*)malloc(16*n);
    var[0] = (float*)malloc(4*n); var[1] = (float*)malloc(4*n);
    if (!valid || !col[0] || !col[1] || !var[0] || !var[1]) {
        free(valid); free(col[0]); free(col[1]); free(var[0]); free(var[1]);
        return RT_ERROR_OUT_OF_MEMORY;
    }
    /* prepare */
    for (size_t i = 0; i < n; ++i) {
        const float* s = color + 4*i;
        int ok = s[3] > 0.001f;
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (ok) {
            c[0] = s[0] / s[3]; c[1] = s[1] / s[3]; c[2] = s[2] / s[3];
            ok = finite_bits(c[0]) && finite_bits(c[1]) && finite_bits(c[2]);
        }
        ok = ok && variance[i] >= 0.0f && finite_bits(variance[i]);
        valid[i] = (unsigned char)ok;
        float* o = col[0] + 4*i;
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        var[0][i] = 0.0f;
        if (ok) {
            for (int k = 0; k < 3; ++k) {
                c[k] = c[k] > 0.0f ? c[k] : 0.0f;
                if (p->firefly_clamp > 0.0f) c[k] = c[k] < p->firefly_clamp ? c[k] : p->firefly_clamp;
                o[k] = c[k];
            }
            o[3] = sv_tm(c[0], c[1], c[2]);
            var[0][i] = variance[i];
        }
    }
    /* iterations */
    static const float hk[5] = {1.0f/16.0f, 1.0f/4.0f, 3.0f/8.0f, 1.0f/4.0f, 1.0f/16.0f};
    static const float gk[3] = {1.0f/4.0f, 1.0f/2.0f, 1.0f/4.0f};
    float inv_n = 0.0f, inv_z = 0.0f;
    if (p->sigma_normal > 0.0f) inv_n = 1.0f / (p->sigma_normal*p->sigma_normal);
    if (p->sigma_plane > 0.0f) inv_z = 1.0f / (p->sigma_plane*p->sigma_plane);
    for (int it = 0; it < p->iterations; ++it) {
        const int s = 1 << it;
        const float* in = col[it & 1];
        const float* vin = var[it & 1];
        float* out = col[(it + 1) & 1];
        float* vout = var[(it + 1) & 1];
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y*(size_t)w + (size_t)x;
            float* o = out + 4*i;
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            vout[i] = 0.0f;
            if (!valid[i]) continue;
            /* the 3x3 Gaussian of the variance, at distance 1 */
            float gsum = 0.0f, gvar = 0.0f;
            for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const size_t q = (size_t)qy*(size_t)w + (size_t)qx;
                if (!valid[q]) continue;
                float g = gk[dy + 1]*gk[dx + 1];
                gvar += g*vin[q];
                gsum += g;
            }
            float gv = gvar / gsum;
            float inv_l = 1.0f / (p->sigma_color*sqrtf(gv) + p->variance_epsilon);
            const float* cp = in + 4*i;
            const rt_gbuffer_texel* gp = &gbuffer[i];
            const int p_miss = gp->primitive == RT_HIT_MISS;
            float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f, vnum = 0.0f;
            for (int dy = -2; dy <= 2; ++dy) for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + s*dx, qy = y + s*dy;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const size_t q = (size_t)qy*(size_t)w + (size_t)qx;
                if (!valid[q]) continue;
                const rt_gbuffer_texel* gq = &gbuffer[q];
                if (p_miss != (gq->primitive == RT_HIT_MISS)) continue;
                const float* cq = in + 4*q;
                float e = 0.0f;
                if (p->sigma_color > 0.0f) e += fabsf(cp[3] - cq[3])*inv_l;
                if (!p_miss) {
                    if (p->sigma_normal > 0.0f) {
                        rt_v3 d = { gp->n.x - gq->n.x, gp->n.y - gq->n.y, gp->n.z - gq->n.z };
                        e += dot3(d, d)*inv_n;
                    }
                    if (p->sigma_plane > 0.0f) {
                        rt_v3 d = { gq->p.x - gp->p.x, gq->p.y - gp->p.y, gq->p.z - gp->p.z };
                        float z = dot3(d, gp->n) / gp->t;
                        e += (z*z)*inv_z;
                    }
                }
                float wt = (hk[dy + 2]*hk[dx + 2])*oracle_expf(-e);
                num[0] += wt*cq[0]; num[1] += wt*cq[1]; num[2] += wt*cq[2];
                den += wt;
                vnum += (wt*wt)*vin[q];
            }
            o[0] = num[0] / den; o[1] = num[1] / den; o[2] = num[2] / den;
            o[3] = sv_tm(o[0], o[1], o[2]);
            vout[i] = vnum / (den*den);
        }
    }
    /* output */
    const float* res = col[p->iterations & 1];
    const float* vres = var[p->iterations & 1];
    for (size_t i = 0; i < n; ++i) {
        float* o = out_pixels + 4*i;
        if (valid[i]) {
            o[0] = res[4*i]; o[1] = res[4*i + 1]; o[2] = res[4*i + 2]; o[3] = 1.0f;
            if (variance_out) variance_out[i] = vres[i];
        } else {
            memmove(o, color + 4*i, 16);
            if (variance_out) variance_out[i] = variance[i];
        }
    }
    free(valid); free(col[0]); free(col[1]); free(var[0]); free(var[1]);
    return RT_OK;
}
