/*
 * ref_robust.c — CPU checker for the robust estimator (rt_robust_combine / rt_robust_combine_device).
 * TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the operation DESIGN.md defines ("The robust estimator"): per pixel a Gini-adaptive
 * median of means over a stack of accumulation buffers.  Every operation and its order is the definition's: IEEE
 * f32, no contraction (the oracle's flags), division as /, the Gini sums added in rank order and the pooled sums
 * in buffer order.  The ranking is an insertion into a list, nothing like the device's network.  The device must
 * match it bit for bit (tests/test_gpu_robust.py); tests/test_ref_robust.py pins it to a numpy restatement.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_abi.h"

#define REF_API __attribute__((visibility("default")))
#define RR_MAX 32

static uint32_t rr_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static int rr_finite(float x) { return (rr_bits(x) & 0x7F800000u) != 0x7F800000u; }

/* The arguments of rt_robust_combine (`device` is ignored; info may be NULL).  Returns RT_OK, or
 * RT_ERROR_INVALID for the arguments rt_robust_combine refuses. */
REF_API int ref_robust_combine(int device, const float* stack, uint32_t count, uint32_t w, uint32_t h,
                               const rt_robust_params* p, float* out, float* info) {
    (void)device;
    if (!stack || !p || !out) return RT_ERROR_INVALID;
    if (!w || !h) return RT_ERROR_INVALID;
    if (count < 2u || count > RR_MAX) return RT_ERROR_INVALID;
    if (!(p->gini_scale >= 0.0f) || !rr_finite(p->gini_scale)) return RT_ERROR_INVALID;
    const size_t n_pixels = (size_t)w*h;
    for (size_t i = 0; i < n_pixels; ++i) {
        /* 1. validity, and 3. the ranking: order[0..n) holds buffer indices by ascending key; a buffer goes in
         * behind every buffer already there whose key is <= its own, so equal keys stay in buffer order */
        float key[RR_MAX];
        uint32_t order[RR_MAX];
        uint32_t n = 0;
        for (uint32_t k = 0; k < count; ++k) {
            const float* S = stack + 4*((size_t)k*n_pixels + i);
            if (!(S[3] > 0.001f)) continue;
            if (!rr_finite(S[0]) || !rr_finite(S[1]) || !rr_finite(S[2]) || !rr_finite(S[3])) continue;
            const float mr = S[0]/S[3], mg = S[1]/S[3], mb = S[2]/S[3];
            if (!rr_finite(mr) || !rr_finite(mg) || !rr_finite(mb)) continue;
            float ky = (mr + mg) + mb;
            if (!rr_finite(ky)) continue;
            if (ky == 0.0f) ky = 0.0f;                 /* -0 counts as +0 */
            key[k] = ky;
            uint32_t at = n;
            while (at > 0 && key[order[at - 1]] > ky) { order[at] = order[at - 1]; --at; }
            order[at] = k;
            n += 1u;
        }
        float* o = out + 4*i;
        /* 2. no valid buffer */
        if (n == 0u) {
            const float* S0 = stack + 4*i;
            float s0[4] = {S0[0], S0[1], S0[2], S0[3]};      /* out may be buffer 0 itself */
            memcpy(o, s0, sizeof s0);
            if (info) { float* f = info + 4*i; f[0] = 0.0f; f[1] = 0.0f; f[2] = 0.0f; f[3] = 0.0f; }
            continue;
        }
        /* 4. the Gini coefficient */
        float Ssum = 0.0f, T = 0.0f;
        for (uint32_t r = 0; r < n; ++r) {
            const float kr = key[order[r]];
            const float g = kr > 0.0f ? kr : 0.0f;
            Ssum = Ssum + g;
            T = T + (float)(r + 1u)*g;
        }
        float G = 0.0f;
        if (n >= 3u && rr_finite(Ssum) && Ssum > 0.0f) G = (2.0f*T)/((float)n*Ssum) - (float)(n + 1u)/(float)n;
        if (!(G > 0.0f)) G = 0.0f;
        /* 5. the trim count; x is >= 0 or NaN (0*inf), and a NaN trims nothing */
        uint32_t cmax = (n - 1u)/2u;
        if (p->max_trim < cmax) cmax = p->max_trim;
        const float x = (p->gini_scale*G)*((float)n*0.5f);
        uint32_t c;
        if (x >= (float)cmax) c = cmax;
        else if (x >= 1.0f) c = (uint32_t)floorf(x);
        else c = 0u;
        /* 6. the kept ranks, pooled in buffer order */
        int kept[RR_MAX];
        for (uint32_t k = 0; k < count; ++k) kept[k] = 0;
        for (uint32_t r = c; r + c < n; ++r) kept[order[r]] = 1;
        float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
        for (uint32_t k = 0; k < count; ++k) {
            if (!kept[k]) continue;
            const float* S = stack + 4*((size_t)k*n_pixels + i);
            num[0] = num[0] + S[0];
            num[1] = num[1] + S[1];
            num[2] = num[2] + S[2];
            den = den + S[3];
        }
        o[0] = num[0]/den;
        o[1] = num[1]/den;
        o[2] = num[2]/den;
        o[3] = 1.0f;
        /* 7. the info */
        if (info) { float* f = info + 4*i; f[0] = G; f[1] = (float)c; f[2] = (float)n; f[3] = den; }
    }
    return RT_OK;
}
