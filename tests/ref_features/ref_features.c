/*
 * ref_features.c — CPU checker for the feature frames (rt_render_feature / rt_render_feature_device) and the
 * denoise stage that uses them (rt_denoise_features / rt_denoise_features_device).  TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over oracle/oracle.c, as tests/ref_integrators is: it reaches the oracle's static helpers
 * (intersect_scene_internal, sample_sky, evaluate_material, fresnel_dielectric, reflect, refract,
 * random_in_unit_sphere, the samplers, the camera, the splat, oracle_expf) and adds, in plain C and in the
 * operation order DESIGN.md defines ("Feature frames", "The denoise stage with feature frames"):
 *   feature_walk         advanced_integrator (RT/integrators.cpp:581-821) cut off at its first non-specular
 *                        vertex, recording the surface there;
 *   a frame driver       of its own (camera sample, seed, tiles total-1 .. 0, samples in order, splatted
 *                        straight into the frame: the exact splat order), which tests/test_ref_features.py
 *                        pins to the oracle's with the Advanced integrator in the walk's place;
 *   ref_denoise_features the filter of tests/ref_denoise with the albedo's three additions.
 * Built with the oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the oracle
 * and with the GPU path.
 */
#include "../../oracle/oracle.c"

#include <stdlib.h>

#define REF_API __attribute__((visibility("default")))

enum { REF_FEATURE_ADVANCED = -1 };                     /* the driver pin: advanced_integrator in the walk's place */
enum { END_MISS = 0, END_EMITTER = 1, END_DIFFUSE = 2, END_BOUND = 3 };

typedef struct { V3 value; int end; uint32_t specular_bounces; float T; } WalkResult;

/* The feature walk.  Draws: Sample_Reflectance 1-D at the bounce index, random_in_unit_sphere for a rough
 * reflection; nothing else. */
static WalkResult feature_walk(Ctx* ctx, Sampler* sampler, RandomSeries* entropy, V3 in_o, V3 in_d, int feature) {
    const rt_scene_desc* scene = ctx->scene;
    const rt_settings* st = ctx->settings;
    const uint32_t B = st->max_bounce_count > 1u ? st->max_bounce_count : 1u;
    Ray ray = make_ray(in_o, in_d, FLT_MAX);
    int32_t at = 0;
    uint32_t stack[64];
    stack[0] = 0xFFFFu;
    float T = 0.0f;
    WalkResult r;
    r.value = v3s(1.0f); r.end = END_BOUND; r.specular_bounces = 0; r.T = 0.0f;
    for (uint32_t bounce = 0; bounce < B; ++bounce) {
        Hit h;
        ctx->closest_rays++;
        intersect_scene_internal(scene, &ray, 0, 0, &h, ctx->ts[0]);
        if (!h.hit) {
            r.value = feature == RT_FEATURE_ALBEDO ? v3s(1.0f) : sample_sky(scene, &ray);
            r.end = END_MISS;
            break;
        }
        V3 N = h.n, I = h.hit_p;
        T = T + h.t;
        if (feature == RT_FEATURE_NORMAL) r.value = smul(0.5f, add(v3s(1.0f), N));
        if (feature == RT_FEATURE_DISTANCE) r.value = v3s(1.0f - clampf_(T / 15.0f, 0.0f, 1.0f));
        if (feature == RT_FEATURE_ALBEDO) r.value = v3s(1.0f);
        float cos_i = -dot(ray.d, N);
        int inside = (cos_i < 0.0f);
        uint32_t surf_id = (h.hit == 1) ? scene->planes[h.index].material_id : scene->primitives[h.index].material_id;
        const rt_material* surf = &scene->materials[surf_id];
        const rt_material* mi;
        const rt_material* mt;
        if (inside) {
            mi = surf;
            mt = mat_of(ctx, stack[at - 1 > 0 ? at - 1 : 0]);
            cos_i = -cos_i;
            N = neg(N);
        } else {
            mi = mat_of(ctx, stack[at]);
            mt = surf;
        }
        if (mt->flags & RT_MATERIAL_EMISSIVE) { r.end = END_EMITTER; break; }
        float eta_i = mi->ior, eta_t = mt->ior;
        float eta = eta_i / eta_t;
        float cos_t;
        float refl = fresnel_dielectric(cos_i, eta_i, eta_t, eta, &cos_t);
        float reflect_test = get_next_sample_1d(sampler, Sample_Reflectance, bounce);
        refl = lerpf_(refl, 1.0f, mt->metallic);
        if (reflect_test < refl) {
            V3 rd = reflect(ray.d, N);
            if (mt->roughness > 0.0f) {
                V3 rs = random_in_unit_sphere(entropy);
                rd = normalize(add(smul(1.0f + EPSILON, rd), smul(mt->roughness, rs)));
            }
            ray = make_ray(add(I, smul(EPSILON, rd)), rd, FLT_MAX);
        } else if (mt->is_participating_medium) {
            if (inside) {
                if (at > 0) --at;
            } else if (at < 63) {
                ++at;
                stack[at] = (mt == ctx->air) ? 0xFFFFu : (uint32_t)(mt - scene->materials);
            }
            V3 fd = refract(ray.d, N, cos_i, cos_t, eta);
            ray = make_ray(add(I, muls(fd, EPSILON)), fd, FLT_MAX);
        } else {
            if (feature == RT_FEATURE_ALBEDO) r.value = evaluate_material(mt, I);
            r.end = END_DIFFUSE;
            break;
        }
        if (bounce + 1 < B) r.specular_bounces++;       /* a specular bounce followed: one more ray */
    }
    r.T = T;
    return r;
}

/* One camera sample of render_tile (RT/raytracer.cpp:443-474) with the walk in the integrator's place. */
static V3 feat_render_sample(Ctx* ctx, const CamSetup* c, RandomSeries* entropy, uint32_t x, uint32_t y,
                             float u, float v, uint32_t canonical, int feature, float* jx_out, float* jy_out,
                             WalkResult* walk) {
    const rt_settings* st = ctx->settings;
    Sampler s = { entropy, st->sampling_strategy, canonical, x, y };
    V2 aa = get_next_sample_2d(&s, Sample_AA, 0);
    float jx = aa.x - 0.5f, jy = aa.y - 0.5f;
    V2 dof = get_next_sample_2d(&s, Sample_DOF, 0);
    dof = transform_bokeh_sample(dof, st->f_factor, st->diaphragm_edges, PI_32*st->phi_shutter_max);
    float djx = c->hfw*c->pixel_w*c->lens_radius*dof.x;
    float djy = c->hfh*c->pixel_h*c->lens_radius*dof.y;
    V3 film_p = c->film_center;
    film_p = add(film_p, smul((u + c->pixel_w*jx)*c->hfw, c->cx));
    film_p = add(film_p, smul((v + c->pixel_h*jy)*c->hfh, c->cy));
    V3 jcp = add(add(c->cp, smul(djx, c->cx)), smul(djy, c->cy));
    V3 rd = normalize(sub(film_p, jcp));
    V3 result;
    if (feature == REF_FEATURE_ADVANCED) {
        result = advanced_integrator(ctx, &s, entropy, jcp, rd);
        if (walk) memset(walk, 0, sizeof(*walk));
    } else {
        WalkResult r = feature_walk(ctx, &s, entropy, jcp, rd, feature);
        result = r.value;
        if (walk) *walk = r;
    }
    float vig = dot(rd, c->cz);
    vig = vig*vig*vig*vig;
    vig = lerpf_(1.0f, vig, st->vignette_strength);
    result = muls(result, vig);
    *jx_out = jx; *jy_out = jy;
    return result;
}

static int feat_validate(const rt_scene_desc* scene, const rt_settings* st, const rt_filter_cache* f, int feature) {
    if (!scene || !st || !f) return RT_ERROR_INVALID;
    if (feature != REF_FEATURE_ADVANCED && (feature < 0 || feature >= RT_FEATURE_COUNT)) return RT_ERROR_INVALID;
    if (st->max_bounce_count > 63) return RT_ERROR_INVALID;
    if (f->cache_size && (f->kernel_size == 0 || f->kernel_size > 20 || f->cache_size > 256)) return RT_ERROR_INVALID;
    return RT_OK;
}

static void feat_stats(rt_stats* stats, const Ctx* ctx, uint64_t samples) {
    if (!stats) return;
    memset(stats, 0, sizeof(*stats));
    stats->closest_hit_rays = ctx->closest_rays;
    stats->shadow_rays = ctx->shadow_rays;
    stats->samples = samples;
    set_traversal(stats, ctx->ts);
}

/* One frame, the arguments of rt_render_feature less the device scene: the owned tiles in the order
 * total-1 .. 0 (RT/raytracer.cpp:555), pixels in raster order inside a tile, samples in order, splatted
 * straight into accum.  feature: an rt_feature, or -1 for the Advanced integrator (the driver pin).
 * out_specular_bounces (may be NULL): the frame's count of specular bounces followed. */
REF_API int ref_features_render(const rt_scene_desc* scene, const rt_camera* camera, const rt_settings* settings,
                                const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                                int feature, rt_accumulation_buffer* accum, rt_stats* stats,
                                uint64_t* out_specular_bounces) {
    if (!tiles || !accum || !accum->pixels || !camera || tiles->tile_w == 0 || tiles->tile_h == 0 ||
        tiles->shard_count == 0) return RT_ERROR_INVALID;
    int err = feat_validate(scene, settings, filter, feature);
    if (err) return err;
    const uint32_t w = accum->w, h = accum->h, tw = tiles->tile_w, th = tiles->tile_h;
    const uint32_t tcx = (w + tw - 1) / tw, tcy = (h + th - 1) / th;
    rt_material air;
    init_air(&air);
    Ctx ctx;
    memset(&ctx, 0, sizeof(ctx));
    ctx.scene = scene; ctx.settings = settings; ctx.air = &air;
    CamSetup c = cam_setup(camera, w, h);
    uint64_t samples = 0, spec = 0;
    for (uint32_t tile = tcx*tcy; tile-- > 0;) {
        if (tile % tiles->shard_count != tiles->shard_index) continue;
        uint32_t min_x = tw*(tile % tcx), min_y = th*(tile / tcx);
        uint32_t max_x = min_x + tw < w ? min_x + tw : w;
        uint32_t max_y = min_y + th < h ? min_y + th : h;
        for (uint32_t y = min_y; y < max_y; ++y) {
            for (uint32_t x = min_x; x < max_x; ++x) {
                float u = 1.0f - 2.0f*(float)x*c.pixel_w;
                float v = 1.0f - 2.0f*(float)y*c.pixel_h;
                apply_lens_distortion(settings->lens_distortion, w, h, &u, &v);
                for (uint32_t s = 0; s < settings->samples_per_pixel; ++s) {
                    uint32_t canonical = accum->frame_count + s;
                    RandomSeries e = random_seed(oracle_sample_seed(total_frame_index, accum->frame_count, tile,
                                                                    y*w + x, canonical));
                    float jx, jy;
                    WalkResult wr;
                    V3 r = feat_render_sample(&ctx, &c, &e, x, y, u, v, canonical, feature, &jx, &jy, &wr);
                    spec += wr.specular_bounces;
                    if (filter->cache_size) {
                        splat(filter, accum->pixels, 0, 0, w, w, h, x, y, jx, jy, r);
                    } else {
                        float* px = accum->pixels + 4*((size_t)y*w + x);
                        px[0] += r.x; px[1] += r.y; px[2] += r.z; px[3] += 1.0f;
                    }
                    ++samples;
                }
            }
        }
    }
    feat_stats(stats, &ctx, samples);
    if (out_specular_bounces) *out_specular_bounces = spec;
    return RT_OK;
}

/* Listed samples, the contract of oracle_trace_samples: out[5*i] = {r, g, b, jitter_x, jitter_y}; out_walk
 * (may be NULL) [3*i] = {how the walk ended (0 miss, 1 emitter, 2 diffuse branch, 3 the bound), specular bounces
 * followed, the bits of T}. */
REF_API int ref_features_trace_samples(const rt_scene_desc* scene, const rt_camera* camera, const rt_settings* settings,
                                       uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                                       uint32_t frame_count, uint32_t total_frame_index, int feature,
                                       uint32_t count, const uint32_t* pixel_xy, const uint32_t* sample_offset,
                                       float* out, uint32_t* out_walk, rt_stats* stats) {
    rt_filter_cache box;
    memset(&box, 0, sizeof(box));
    int err = feat_validate(scene, settings, &box, feature);
    if (err) return err;
    if (!camera || !pixel_xy || !sample_offset || !out || !w || !h || !tile_w || !tile_h) return RT_ERROR_INVALID;
    rt_material air;
    init_air(&air);
    Ctx ctx;
    memset(&ctx, 0, sizeof(ctx));
    ctx.scene = scene; ctx.settings = settings; ctx.air = &air;
    CamSetup c = cam_setup(camera, w, h);
    uint32_t tcx = (w + tile_w - 1) / tile_w;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t x = pixel_xy[2*i], y = pixel_xy[2*i + 1];
        uint32_t tile = (y / tile_h)*tcx + (x / tile_w);
        uint32_t canonical = frame_count + sample_offset[i];
        float u = 1.0f - 2.0f*(float)x*c.pixel_w;
        float v = 1.0f - 2.0f*(float)y*c.pixel_h;
        apply_lens_distortion(settings->lens_distortion, w, h, &u, &v);
        RandomSeries e = random_seed(oracle_sample_seed(total_frame_index, frame_count, tile, y*w + x, canonical));
        float jx, jy;
        WalkResult wr;
        V3 r = feat_render_sample(&ctx, &c, &e, x, y, u, v, canonical, feature, &jx, &jy, &wr);
        out[5*i + 0] = r.x; out[5*i + 1] = r.y; out[5*i + 2] = r.z;
        out[5*i + 3] = jx; out[5*i + 4] = jy;
        if (out_walk) {
            out_walk[3*i + 0] = (uint32_t)wr.end;
            out_walk[3*i + 1] = wr.specular_bounces;
            out_walk[3*i + 2] = f_bits(wr.T);
        }
    }
    feat_stats(stats, &ctx, count);
    return RT_OK;
}

/* ---- the denoise stage with feature frames ---- */

static int dn_finite(float x) { return (f_bits(x) & 0x7F800000u) != 0x7F800000u; }
static float dn_max(float a, float b) { return a > b ? a : b; }
static float dn_min(float a, float b) { return a < b ? a : b; }
static float dn_l(float r, float g, float b) {
    float y = 0.2126f*r + 0.7152f*g + 0.0722f*b;
    return 1.0f - oracle_expf(-y);
}
static int dn_bad(float v) { return !(v >= 0.0f) || v > FLT_MAX; }

/* The arguments of rt_denoise_features (`device` is ignored).  RT_OK, or RT_ERROR_INVALID for the arguments
 * rt_denoise_features refuses. */
REF_API int ref_denoise_features(int device, const rt_accumulation_buffer* beauty, const float* normal,
                                 const float* distance, const float* albedo, const rt_denoise_features_params* fp,
                                 float* out_pixels) {
    (void)device;
    if (!beauty || !beauty->pixels || !out_pixels || !fp || !beauty->w || !beauty->h) return RT_ERROR_INVALID;
    const rt_denoise_params* p = &fp->base;
    if (p->iterations < 1 || p->iterations > 8) return RT_ERROR_INVALID;
    if (dn_bad(p->sigma_color) || dn_bad(p->sigma_guide[0]) || dn_bad(p->sigma_guide[1]) || dn_bad(p->firefly_clamp))
        return RT_ERROR_INVALID;
    if ((p->sigma_guide[0] > 0.0f && !normal) || (p->sigma_guide[1] > 0.0f && !distance)) return RT_ERROR_INVALID;
    if (dn_bad(fp->sigma_albedo) || (fp->demodulate != 0 && fp->demodulate != 1)) return RT_ERROR_INVALID;
    if (fp->demodulate && (dn_bad(fp->albedo_floor) || !(fp->albedo_floor > 0.0f))) return RT_ERROR_INVALID;
    if ((fp->sigma_albedo > 0.0f || fp->demodulate) && !albedo) return RT_ERROR_INVALID;
    const int w = (int)beauty->w, h = (int)beauty->h;
    const size_t n = (size_t)w*(size_t)h;
    const float* guide[3] = {normal, distance, albedo};         /* the albedo resolves and validates like a guide */
    float* col[2];
    float* g[3];
    unsigned char* valid = (unsigned char*)malloc(n);
    col[0] = (float*)malloc(16*n); col[1] = (float*)malloc(16*n);
    g[0] = (float*)calloc(n, 12); g[1] = (float*)calloc(n, 12); g[2] = (float*)calloc(n, 12);
    if (!valid || !col[0] || !col[1] || !g[0] || !g[1] || !g[2]) {
        free(valid); free(col[0]); free(col[1]); free(g[0]); free(g[1]); free(g[2]);
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
        for (int k = 0; k < 3; ++k) {
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
                if (fp->demodulate) c[k] = c[k] / dn_max(g[2][3*i + k], fp->albedo_floor);
                o[k] = c[k];
            }
            o[3] = dn_l(c[0], c[1], c[2]);
        }
    }
    /* iterations */
    static const float hk[5] = {1.0f/16.0f, 1.0f/4.0f, 3.0f/8.0f, 1.0f/4.0f, 1.0f/16.0f};
    const float sigma[3] = {p->sigma_guide[0], p->sigma_guide[1], fp->sigma_albedo};
    float inv_g[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; ++k)
        if (sigma[k] > 0.0f) inv_g[k] = 1.0f / (sigma[k]*sigma[k]);
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
                for (int k = 0; k < 3; ++k) {                    /* normal, distance, then the albedo */
                    if (!guide[k] || !(sigma[k] > 0.0f)) continue;
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
    /* output: remodulated, weight 1 */
    const float* res = col[p->iterations & 1];
    for (size_t i = 0; i < n; ++i) {
        float* o = out_pixels + 4*i;
        if (valid[i]) {
            for (int k = 0; k < 3; ++k) {
                float c = res[4*i + k];
                if (fp->demodulate) c = c*dn_max(g[2][3*i + k], fp->albedo_floor);
                o[k] = c;
            }
            o[3] = 1.0f;
        } else memmove(o, beauty->pixels + 4*i, 16);
    }
    free(valid); free(col[0]); free(col[1]); free(g[0]); free(g[1]); free(g[2]);
    return RT_OK;
}

REF_API void ref_features_set_math_mode(int libm) { oracle_set_math_mode(libm); }
