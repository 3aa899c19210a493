/*
 * ref_adaptive.c — CPU checker for the tile error estimate (rt_tile_error / rt_tile_error_device).
 * TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the operation DESIGN.md defines ("Adaptive sampling by tiles"): per pixel of a tile
 * the half-buffer error of Dammertz et al. (HPG 2010), per tile its mean over the valid pixels.  Every
 * operation and its order is the definition's: IEEE f32, no contraction (the oracle's flags), division as /,
 * sqrtf correctly rounded, and the additions in the device's one fixed order -- partial sum i of 256 takes the
 * pixels i, i + 256, ... of the tile's raster order, and the partials are added pairwise, element i +=
 * element i + s for s = 128, 64, ..., 1.  The device must match it bit for bit (tests/test_gpu_adaptive.py);
 * tests/test_ref_adaptive.py pins it to a numpy float64 restatement of the metric.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_abi.h"

#define REF_API __attribute__((visibility("default")))
#define TE_PARTIALS 256

static uint32_t ta_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static int ta_finite(float x) { return (ta_bits(x) & 0x7F800000u) != 0x7F800000u; }
static uint32_t ta_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

/* The arguments of rt_tile_error (`device` is ignored).  Returns RT_OK, or RT_ERROR_INVALID for the arguments
 * rt_tile_error refuses. */
REF_API int ref_tile_error(int device, const float* half_a, const float* half_b, uint32_t w, uint32_t h,
                           uint32_t tile_w, uint32_t tile_h, const uint32_t* tile_ids, uint32_t tile_count,
                           const rt_tile_error_params* p, float* tile_error, uint32_t* tile_valid) {
    (void)device;
    if (!half_a || !half_b || !tile_error || !tile_valid || !p) return RT_ERROR_INVALID;
    if (!w || !h || !tile_w || !tile_h || w > 65535u || h > 65535u) return RT_ERROR_INVALID;
    if (!(p->floor > 0.0f) || !ta_finite(p->floor)) return RT_ERROR_INVALID;
    const uint32_t tcx = (w + tile_w - 1)/tile_w, tcy = (h + tile_h - 1)/tile_h;
    const uint64_t ntiles = (uint64_t)tcx*tcy;
    if (!tile_count || tile_count > ntiles || (!tile_ids && tile_count != ntiles)) return RT_ERROR_INVALID;
    for (uint32_t k = 0; tile_ids && k < tile_count; ++k)
        if (tile_ids[k] >= ntiles) return RT_ERROR_INVALID;
    for (uint32_t k = 0; k < tile_count; ++k) {
        const uint32_t t = tile_ids ? tile_ids[k] : k;
        const uint32_t min_x = tile_w*(t % tcx), min_y = tile_h*(t / tcx);
        const uint32_t tw = ta_min(w, min_x + tile_w) - min_x, th = ta_min(h, min_y + tile_h) - min_y;
        const uint64_t n = (uint64_t)tw*th;
        float sum[TE_PARTIALS];
        uint32_t cnt[TE_PARTIALS];
        for (uint32_t i = 0; i < TE_PARTIALS; ++i) {
            sum[i] = 0.0f;
            cnt[i] = 0;
            for (uint64_t j = i; j < n; j += TE_PARTIALS) {
                const uint32_t x = min_x + (uint32_t)(j % tw), y = min_y + (uint32_t)(j / tw);
                const float* A = half_a + 4*((size_t)y*w + x);
                const float* B = half_b + 4*((size_t)y*w + x);
                int valid = A[3] > 0.001f && B[3] > 0.001f;
                for (int c = 0; c < 4; ++c) valid = valid && ta_finite(A[c]) && ta_finite(B[c]);
                if (!valid) continue;
                const float ar = A[0]/A[3], ag = A[1]/A[3], ab = A[2]/A[3];
                const float br = B[0]/B[3], bg = B[1]/B[3], bb = B[2]/B[3];
                const float mw = A[3] + B[3];
                const float mr = (A[0] + B[0])/mw, mg = (A[1] + B[1])/mw, mb = (A[2] + B[2])/mw;
                const float d = (fabsf(ar - br) + fabsf(ag - bg)) + fabsf(ab - bb);
                const float m = (mr + mg) + mb;
                const float e = d/sqrtf(m > p->floor ? m : p->floor);
                sum[i] = sum[i] + e;
                cnt[i] += 1u;
            }
        }
        for (uint32_t s = TE_PARTIALS/2; s > 0; s >>= 1)
            for (uint32_t i = 0; i < s; ++i) {
                sum[i] = sum[i] + sum[i + s];
                cnt[i] = cnt[i] + cnt[i + s];
            }
        tile_error[k] = cnt[0] ? sum[0]/(float)cnt[0] : INFINITY;
        tile_valid[k] = cnt[0];
    }
    return RT_OK;
}
