/*
 * ref_integrators.c — CPU checker for the integrators besides the Advanced one.  TEST INFRASTRUCTURE ONLY.
 *
 * The oracle (oracle/oracle.c) restates the reference's advanced_integrator and refuses every other
 * SceneSettings::integrator.  This helper is a unity build over it: it reaches the oracle's static
 * helpers (intersect_scene_internal, sample_sky, evaluate_material, fresnel_dielectric, map_to_hemisphere,
 * reflect, random_unilaterals, the samplers, the camera and the splat) and adds plain-C restatements of
 *   ground_truth_iterative_integrator   RT/integrators.cpp:486-541
 *   normals_integrator                  RT/integrators.cpp:544-560
 *   distances_integrator                RT/integrators.cpp:563-579
 * in the reference's operation order, a render_sample that picks the integrator as
 * scene->settings.integrator->f(&state) does (RT/raytracer.cpp:467), and a single-threaded tile loop in
 * the reference's order (tiles total-1 .. 0, RT/raytracer.cpp:555).  Built with the oracle's own flags
 * (-ffp-contract=off, no fast-math), so it is bit-comparable with the oracle and with the GPU path.
 *
 * tests/test_ref_integrators.py pins the driver restated here (camera, seed, tile loop) to the oracle's
 * with integrator = Advanced, so the three integrators below are the only text the oracle does not pin.
 */
#include "../../oracle/oracle.c"

#define REF_API __attribute__((visibility("default")))

/* RT/integrators.cpp:486-541 */
static V3 ground_truth_iterative_integrator(Ctx* ctx, RandomSeries* entropy, V3 in_o, V3 in_d) {
    const rt_scene_desc* scene = ctx->scene;
    Ray ray = make_ray(in_o, in_d, FLT_MAX);
    V3 throughput = v3s(1.0f);
    V3 total = v3s(0.0f);
    for (uint32_t bounce = 0; bounce < ctx->settings->max_bounce_count; ++bounce) {
        Hit h;
        ctx->closest_rays++;
        intersect_scene_internal(scene, &ray, 0, 0, &h, ctx->ts[0]);
        if (h.hit) {
            V3 I = h.hit_p, N = h.n;
            uint32_t id = (h.hit == 1) ? scene->planes[h.index].material_id : scene->primitives[h.index].material_id;
            const rt_material* m = &scene->materials[id];
            if (m->flags & RT_MATERIAL_EMISSIVE) {                          /* :507-510 */
                total = add(total, mul(throughput, m->emission_color));
                break;
            }
            float r[4];
            random_unilaterals(entropy, r);                                 /* :512 */
            float eta_i = 1.0f;
            float eta_t = m->ior;
            float eta = eta_i / eta_t;
            float cos_i = -dot(ray.d, N);
            float cos_t;
            float reflectance = fresnel_dielectric(cos_i, eta_i, eta_t, eta, &cos_t);
            if (r[0] < reflectance) {                                       /* make_reflected_ray :267-270 */
                V3 rd = reflect(ray.d, N);
                ray = make_ray(add(I, muls(rd, EPSILON)), rd, FLT_MAX);
            } else {                                                        /* :525-532 */
                V3 brdf = muls(evaluate_material(m, I), 1.0f / PI_32);
                throughput = mul(throughput, brdf);
                V2 s2 = { r[1], r[2] };
                V3 R = map_to_hemisphere(N, s2);
                ray = make_ray(add(I, muls(N, EPSILON)), R, FLT_MAX);
                throughput = muls(throughput, dot(ray.d, N));
                throughput = muls(throughput, 2.0f*PI_32);
            }
        } else {
            total = add(total, mul(throughput, sample_sky(scene, &ray)));   /* :535 */
            break;
        }
    }
    return total;
}

/* RT/integrators.cpp:544-560 (normals = 1) and :563-579 (normals = 0): one ray, whatever max_bounce_count */
static V3 first_hit_integrator(Ctx* ctx, V3 in_o, V3 in_d, int normals) {
    Ray ray = make_ray(in_o, in_d, FLT_MAX);
    Hit h;
    ctx->closest_rays++;
    intersect_scene_internal(ctx->scene, &ray, 0, 0, &h, ctx->ts[0]);
    if (!h.hit) return sample_sky(ctx->scene, &ray);
    if (normals) return smul(0.5f, add(v3s(1.0f), h.n));                   /* :556 */
    return v3s(1.0f - clampf_(h.t / 15.0f, 0.0f, 1.0f));                    /* :575, saturate my_math.h:119 */
}

/* One camera sample of render_tile (RT/raytracer.cpp:443-474) with the integrator picked at :467. */
static V3 ref_render_sample(Ctx* ctx, const CamSetup* c, RandomSeries* entropy, uint32_t x, uint32_t y,
                            float u, float v, uint32_t canonical, float* jx_out, float* jy_out) {
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
    switch (st->integrator) {
        case RT_INTEGRATOR_GROUND_TRUTH_ITERATIVE: result = ground_truth_iterative_integrator(ctx, entropy, jcp, rd); break;
        case RT_INTEGRATOR_NORMALS:                result = first_hit_integrator(ctx, jcp, rd, 1); break;
        case RT_INTEGRATOR_DISTANCES:              result = first_hit_integrator(ctx, jcp, rd, 0); break;
        default:                                   result = advanced_integrator(ctx, &s, entropy, jcp, rd); break;
    }
    float vig = dot(rd, c->cz);
    vig = vig*vig*vig*vig;
    vig = lerpf_(1.0f, vig, st->vignette_strength);
    result = muls(result, vig);
    *jx_out = jx; *jy_out = jy;
    return result;
}

static int ref_validate(const rt_scene_desc* scene, const rt_settings* st, const rt_filter_cache* f) {
    if (!scene || !st || !f) return RT_ERROR_INVALID;
    if (st->integrator != RT_INTEGRATOR_ADVANCED && st->integrator != RT_INTEGRATOR_GROUND_TRUTH_ITERATIVE &&
        st->integrator != RT_INTEGRATOR_NORMALS && st->integrator != RT_INTEGRATOR_DISTANCES) return RT_ERROR_INVALID;
    if (st->max_bounce_count > 63) return RT_ERROR_INVALID;
    if (f->cache_size && (f->kernel_size == 0 || f->kernel_size > 20 || f->cache_size > 256)) return RT_ERROR_INVALID;
    return RT_OK;
}

static void ref_stats(rt_stats* stats, const Ctx* ctx, uint64_t samples, double seconds) {
    if (!stats) return;
    memset(stats, 0, sizeof(*stats));
    stats->closest_hit_rays = ctx->closest_rays;
    stats->shadow_rays = ctx->shadow_rays;
    stats->samples = samples;
    stats->seconds = seconds;
    set_traversal(stats, ctx->ts);
}

/* Same contract as oracle_trace_samples; settings->integrator 0, 3, 4 or 5. */
REF_API int ref_trace_samples(const rt_scene_desc* scene, const rt_camera* camera, const rt_settings* settings,
                              uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                              uint32_t frame_count, uint32_t total_frame_index,
                              uint32_t count, const uint32_t* pixel_xy, const uint32_t* sample_offset,
                              float* out, rt_stats* stats) {
    rt_filter_cache box;
    memset(&box, 0, sizeof(box));
    int err = ref_validate(scene, settings, &box);
    if (err) return err;
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
        V3 r = ref_render_sample(&ctx, &c, &e, x, y, u, v, canonical, &jx, &jy);
        out[5*i + 0] = r.x; out[5*i + 1] = r.y; out[5*i + 2] = r.z;
        out[5*i + 3] = jx; out[5*i + 4] = jy;
    }
    ref_stats(stats, &ctx, count, 0.0);
    return RT_OK;
}

/* One frame like oracle_render with RT_RNG_PER_SAMPLE on one thread: the owned tiles in the order
 * total-1 .. 0 (RT/raytracer.cpp:555), pixels in raster order inside a tile, samples in order
 * (render_tile, :409-422), splatted straight into accum. */
REF_API int ref_render(const rt_scene_desc* scene, const rt_camera* camera, const rt_settings* settings,
                       const rt_filter_cache* filter, const rt_tile_set* tiles, uint32_t total_frame_index,
                       rt_accumulation_buffer* accum, rt_stats* stats) {
    if (!tiles || !accum || !accum->pixels || !camera || tiles->tile_w == 0 || tiles->tile_h == 0 ||
        tiles->shard_count == 0) return RT_ERROR_INVALID;
    int err = ref_validate(scene, settings, filter);
    if (err) return err;
    double t0 = now_s();
    const uint32_t w = accum->w, h = accum->h, tw = tiles->tile_w, th = tiles->tile_h;
    const uint32_t tcx = (w + tw - 1) / tw, tcy = (h + th - 1) / th;
    rt_material air;
    init_air(&air);
    Ctx ctx;
    memset(&ctx, 0, sizeof(ctx));
    ctx.scene = scene; ctx.settings = settings; ctx.air = &air;
    CamSetup c = cam_setup(camera, w, h);
    uint64_t samples = 0;
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
                    V3 r = ref_render_sample(&ctx, &c, &e, x, y, u, v, canonical, &jx, &jy);
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
    ref_stats(stats, &ctx, samples, now_s() - t0);
    return RT_OK;
}

/* oracle_set_math_mode of this library's copy of the oracle: 0 = the deterministic transcendentals the
 * HIP kernels share (default), 1 = the C library's. */
REF_API void ref_set_math_mode(int libm) { oracle_set_math_mode(libm); }
