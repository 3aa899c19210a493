/*
 * ref_denoise.c — CPU checker for the denoise stage (rt_denoise / rt_denoise_device).  TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the filter DESIGN.md defines ("The denoise stage"): resolve, validity, clamp, then
 * `iterations` passes of the 5x5 B3-spline a-trous kernel at step 2^i with edge-stopping weights from the
 * tonemapped luminance and the guide buffers.  Every operation and its order is the definition's: IEEE f32,
 * no contraction (the oracle's flags), division as /, and the exponential is the oracle's oracle_expf, which
 * this file reaches as a unity build over oracle/oracle.c (as tests/ref_integrators does).  The device must
 * match it bit for bit (tests/test_gpu_denoise.py); tests/test_ref_denoise.py pins it to a numpy restatement.
 */
#include "../../oracle/oracle.c"

#include <stdlib.h>

#define REF_API __attribute__((visibility("default")))

static int dn_finite(float x) { return (f_bits(x) & 0x7F800000u) != 0x7F800000u; }
static float dn_max(float a, float b) { return a > b ? a : b; }
static float dn_min(float a, float b) { return a < b ? a : b; }
static float dn_l(float r, float g, float b) {
    float y = 0.2126f*r + 0.7152f*g + 0.0722f*b;
    return 1.0f - oracle_expf(-y);
}
static int dn_bad(float v) { return !(v >= 0.0f) || v > FLT_MAX; }

/* The arguments of rt_denoise (`device` is ignored).  Returns RT_OK, or RT_ERROR_INVALID for the arguments
 * rt_denoise refuses. */
REF_API int ref_denoise(int device, const rt_accumulation_buffer* beauty, const float* guide0, const float* guide1,
                        const rt_denoise_params* p, float* out_pixels) {
    (void)device;
    if (!beauty || !beauty->pixels || !out_pixels || !p || !beauty->w || !beauty->h) return RT_ERROR_INVALID;
    if (p->iterations < 1 || p->iterations > 8) return RT_ERROR_INVALID;
    if (dn_bad(p->sigma_color) || dn_bad(p->sigma_guide[0]) || dn_bad(p->sigma_guide[1]) || dn_bad(p->firefly_clamp))
        return RT_ERROR_INVALID;
    if ((p->sigma_guide[0] > 0.0f && !guide0) || (p->sigma_guide[1] > 0.0f && !guide1)) return RT_ERROR_INVALID;
    const int w = (int)beauty->w, h = (int)beauty->h;
    const size_t n = (size_t)w*(size_t)h;
    const float* guide[2] = {guide0, guide1};
    float* col[2];                              /* {r, g, b, l} per pixel, ping-pong */
    float* g[2];                                /* resolved guides {x, y, z} */
    unsigned char* valid = (unsigned char*)malloc(n);
    col[0] = (float*)malloc(16*n); col[1] = (float*)malloc(16*n);
    g[0] = (float*)calloc(n, 12); g[1] = (float*)calloc(n, 12);
    if (!valid || !col[0] || !col[1] || !g[0] || !g[1]) {
        free(valid); free(col[0]); free(col[1]); free(g[0]); free(g[1]);
        return RT_ERROR_OUT_OF_MEMORY;
    }
    /* prepare */
    for (size_t i = 0; i < n; ++i) {
        const float* s = beauty->pixels + 4*i;
        int ok = s[3] > 0.001f;
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (ok) {
            c[0] = s[0] / s[3]; c[1] = s[1] / s[3]; c[2] = s[2] / s[3];
            ok = dn_finite(c[0]) && dn_finite(c[1]) && dn_finite(c[2]);
        }
        for (int k = 0; k < 2; ++k) {
            if (!guide[k]) continue;
            const float* q = guide[k] + 4*i;
            if (q[3] > 0.001f) {
                float* r = g[k] + 3*i;
                r[0] = q[0] / q[3]; r[1] = q[1] / q[3]; r[2] = q[2] / q[3];
                ok = ok && dn_finite(r[0]) && dn_finite(r[1]) && dn_finite(r[2]);
            } else ok = 0;
        }
        valid[i] = (unsigned char)ok;
        float* o = col[0] + 4*i;
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        if (ok) {
            for (int k = 0; k < 3; ++k) {
                c[k] = dn_max(c[k], 0.0f);
                if (p->firefly_clamp > 0.0f) c[k] = dn_min(c[k], p->firefly_clamp);
                o[k] = c[k];
            }
            o[3] = dn_l(c[0], c[1], c[2]);
        }
    }
    /* iterations */
    static const float hk[5] = {1.0f/16.0f, 1.0f/4.0f, 3.0f/8.0f, 1.0f/4.0f, 1.0f/16.0f};
    float inv_g[2] = {0.0f, 0.0f};
    for (int k = 0; k < 2; ++k)
        if (p->sigma_guide[k] > 0.0f) inv_g[k] = 1.0f / (p->sigma_guide[k]*p->sigma_guide[k]);
    float scale = 1.0f;                         /* 2^-i */
    for (int it = 0; it < p->iterations; ++it, scale = scale*0.5f) {
        const int s = 1 << it;
        float inv_c = 0.0f;
        if (p->sigma_color > 0.0f) { float sc = p->sigma_color*scale; inv_c = 1.0f / (sc*sc); }
        const float* in = col[it & 1];
        float* out = col[(it + 1) & 1];
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y*(size_t)w + (size_t)x;
            float* o = out + 4*i;
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            if (!valid[i]) continue;
            const float* cp = in + 4*i;
            float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
            for (int dy = -2; dy <= 2; ++dy) for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + s*dx, qy = y + s*dy;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const size_t q = (size_t)qy*(size_t)w + (size_t)qx;
                if (!valid[q]) continue;
                const float* cq = in + 4*q;
                float e = 0.0f;
                if (p->sigma_color > 0.0f) {
                    float d = cp[3] - cq[3];
                    e += (d*d)*inv_c;
                }
                for (int k = 0; k < 2; ++k) {
                    if (!guide[k] || !(p->sigma_guide[k] > 0.0f)) continue;
                    const float* gp = g[k] + 3*i;
                    const float* gq = g[k] + 3*q;
                    float a = gp[0] - gq[0], b = gp[1] - gq[1], c = gp[2] - gq[2];
                    e += (a*a + b*b + c*c)*inv_g[k];
                }
                float wt = (hk[dy + 2]*hk[dx + 2])*oracle_expf(-e);
                num[0] += wt*cq[0]; num[1] += wt*cq[1]; num[2] += wt*cq[2];
                den += wt;
            }
            o[0] = num[0] / den; o[1] = num[1] / den; o[2] = num[2] / den;
            o[3] = dn_l(o[0], o[1], o[2]);
        }
    }
    /* output */
    const float* res = col[p->iterations & 1];
    for (size_t i = 0; i < n; ++i) {
        float* o = out_pixels + 4*i;
        if (valid[i]) { o[0] = res[4*i]; o[1] = res[4*i + 1]; o[2] = res[4*i + 2]; o[3] = 1.0f; }
        else memmove(o, beauty->pixels + 4*i, 16);
    }
    free(valid); free(col[0]); free(col[1]); free(g[0]); free(g[1]);
    return RT_OK;
}
