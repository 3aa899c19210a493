/*
 * ref_recursive.c — CPU checker for the two recursive integrators.  TEST INFRASTRUCTURE ONLY.
 *
 * The oracle (oracle/oracle.c) restates advanced_integrator and tests/ref_integrators the three single-chain
 * integrators; both refuse Whitted (1) and Ground Truth Recursive (2).  This helper is a second unity build
 * over the oracle: it reaches the oracle's static helpers (intersect_scene_internal, sample_sky,
 * evaluate_material, fresnel_dielectric, refract, reflect, map_to_hemisphere, random_point_on_light,
 * random_in_unit_sphere, random_unilaterals, the samplers, the camera and the splat) and adds plain-C
 * restatements of
 *   raytrace_recursively / whitted_integrator                     RT/integrators.cpp:310-426
 *   pathtrace_recursively / ground_truth_recursive_integrator     RT/integrators.cpp:428-483
 * as RECURSION, in the reference's operation order (MathLib's operators are component-wise and evaluate
 * left to right: a*b*c is (a*b)*c), a render_sample that picks the integrator as
 * scene->settings.integrator->f(&state) does (RT/raytracer.cpp:467), and a single-threaded tile loop in the
 * reference's order (tiles total-1 .. 0, RT/raytracer.cpp:555) with RT_RNG_PER_SAMPLE keys.  The device runs
 * the same integrators with an explicit frame stack (k_recurse): the comparison is between two formulations.
 * Built with the oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the oracle
 * and with the GPU path.
 *
 * Scene::ambient_light (RT/scene.h:102) is not part of rt_scene_desc: the entries take it as an argument
 * (NULL = the default, 0).
 *
 * tests/test_ref_recursive.py pins the driver restated here to the oracle's with integrator = Advanced.
 */
#include "../../oracle/oracle.c"

#define RR_API __attribute__((visibility("default")))

typedef struct {
    Ctx* ctx;
    Sampler* sampler;
    V3 ambient_light;
} RState;

static const rt_material* hit_material(const rt_scene_desc* scene, const Hit* h) {
    uint32_t id = (h->hit == 1) ? scene->planes[h->index].material_id : scene->primitives[h->index].material_id;
    return &scene->materials[id];
}

/* raytrace_recursively, RT/integrators.cpp:310-414 */
static V3 raytrace_recursively(RState* rs, Ray ray, int32_t recursion, const rt_material* previous_material) {
    Ctx* ctx = rs->ctx;
    const rt_scene_desc* scene = ctx->scene;
    if (recursion > 0) {                                                    /* :312 */
        Hit h;
        ctx->closest_rays++;
        intersect_scene_internal(scene, &ray, 0, 0, &h, ctx->ts[0]);        /* :315 */
        if (h.hit) {
            float t = h.t;
            V3 I = h.hit_p, N = h.n;
            const rt_material* material = hit_material(scene, &h);          /* :318 */
            if (material->flags & RT_MATERIAL_EMISSIVE) {                   /* :320-322 */
                return material->emission_color;
            }
            float cos_theta_i = -dot(ray.d, N);                             /* :324 */
            int ray_hit_inside = (cos_theta_i < 0.0f);
            float eta_i = 1.0f;
            float eta_t = material->ior;
            V3 throughput = v3s(1.0f);
            if (ray_hit_inside) {                                           /* :332-339 */
                N = neg(N);
                cos_theta_i = -cos_theta_i;
                float tmp = eta_i; eta_i = eta_t; eta_t = tmp;
                if (previous_material) {
                    material = previous_material;
                }
            }
            if (ray_hit_inside && material->is_participating_medium) {      /* :341-345 */
                throughput.x *= expf_(-material->absorb.x*t);
                throughput.y *= expf_(-material->absorb.y*t);
                throughput.z *= expf_(-material->absorb.z*t);
            }
            const uint32_t light_sample_count = 1;                          /* :347 */
            V3 illumination = v3s(0.0f);
            for (uint32_t light_index = 0; light_index < scene->light_count; ++light_index) {   /* :350 */
                uint32_t light_id = scene->lights[light_index];
                const rt_primitive* light = &scene->primitives[light_id];
                const rt_material* light_material = &scene->materials[light->material_id];
                for (uint32_t i = 0; i < light_sample_count; ++i) {
                    /* bounce index 0 at every depth (:355) */
                    LightSample ls = random_point_on_light(ctx, light, get_next_sample_2d(rs->sampler, Sample_DirectLighting, 0), I);
                    V3 L = ls.L;
                    V3 Nl = ls.Nl;
                    float N_dot_L = dot(N, L);
                    float neg_Nl_dot_L = -dot(Nl, L);
                    if (N_dot_L > 0.0f && neg_Nl_dot_L > 0.0f) {            /* :363 */
                        Hit sh;
                        Ray sray = make_ray(add(I, muls(L, EPSILON)), L, ls.dist - 2*EPSILON);
                        ctx->shadow_rays++;
                        if (!intersect_scene_internal(scene, &sray, 1, light_id, &sh, ctx->ts[1])) {   /* :364 */
                            /* neg_Nl_dot_L*ls.A*N_dot_L*emission_color / ls.dist_sq (:365) */
                            illumination = add(illumination,
                                               divs(smul(neg_Nl_dot_L*ls.A*N_dot_L, light_material->emission_color), ls.dist_sq));
                        }
                    }
                }
            }
            illumination = muls(illumination, 1.0f / (float)light_sample_count);   /* :370 */
            illumination = add(illumination, rs->ambient_light);                    /* :371 */

            V3 brdf = smul(1.0f / PI_32, evaluate_material(material, I));   /* :373 */
            V3 metallic_color = lerp3(v3s(1.0f), material->albedo, material->metallic);
            float eta_i_over_eta_t = eta_i / eta_t;                         /* :376 */
            float cos_theta_t;
            float reflectance = fresnel_dielectric(cos_theta_i, eta_i, eta_t, eta_i_over_eta_t, &cos_theta_t);
            reflectance = lerpf_(reflectance, 1.0f, material->metallic);    /* :381 */

            if (material->is_participating_medium) {                        /* :383-394 */
                V3 refracted_d = refract(ray.d, N, cos_theta_i, cos_theta_t, eta_i_over_eta_t);
                V3 reflected_d = reflect(ray.d, N);
                if (material->roughness > 0.0f) {
                    reflected_d = normalize(add(smul(1.0f + EPSILON, reflected_d),
                                                smul(material->roughness, random_in_unit_sphere(rs->sampler->entropy))));
                }
                V3 refracted_light = raytrace_recursively(rs, make_ray(add(I, muls(refracted_d, EPSILON)), refracted_d, FLT_MAX),
                                                          recursion - 1, material);
                V3 reflected_light = raytrace_recursively(rs, make_ray(add(I, muls(reflected_d, EPSILON)), reflected_d, FLT_MAX),
                                                          recursion - 1, NULL);
                return lerp3(mul(throughput, refracted_light), reflected_light, reflectance);
            } else if (reflectance > 0.05f) {                               /* :395-404 */
                V3 reflected_d = reflect(ray.d, N);
                if (material->roughness > 0.0f) {
                    reflected_d = normalize(add(smul(1.0f + EPSILON, reflected_d),
                                                smul(material->roughness, random_in_unit_sphere(rs->sampler->entropy))));
                }
                V3 diffuse_light = mul(mul(throughput, brdf), illumination);
                V3 reflected_light = mul(metallic_color,
                                         raytrace_recursively(rs, make_ray(add(I, muls(reflected_d, EPSILON)), reflected_d, FLT_MAX),
                                                              recursion - 1, NULL));
                return lerp3(diffuse_light, reflected_light, reflectance);
            } else {
                return mul(mul(throughput, brdf), illumination);            /* :406 */
            }
        }
        return sample_sky(scene, &ray);                                     /* :410 */
    }
    return v3s(0.0f);                                                       /* :413 */
}

/* pathtrace_recursively, RT/integrators.cpp:428-471 */
static V3 pathtrace_recursively(Ctx* ctx, RandomSeries* entropy, Ray ray, int32_t recursion) {
    const rt_scene_desc* scene = ctx->scene;
    if (recursion > 0) {                                                    /* :430 */
        Hit h;
        ctx->closest_rays++;
        intersect_scene_internal(scene, &ray, 0, 0, &h, ctx->ts[0]);        /* :433 */
        if (h.hit) {
            V3 I = h.hit_p, N = h.n;
            const rt_material* material = hit_material(scene, &h);
            if (material->flags & RT_MATERIAL_EMISSIVE) {                   /* :438-440 */
                return material->emission_color;
            }
            float r[4];
            random_unilaterals(entropy, r);                                 /* :442 */
            float eta_i = 1.0f;
            float eta_t = material->ior;
            float eta_i_over_eta_t = eta_i / eta_t;
            float cos_theta_i = -dot(ray.d, N);
            float cos_theta_t;
            float reflectance = fresnel_dielectric(cos_theta_i, eta_i, eta_t, eta_i_over_eta_t, &cos_theta_t);
            float reflect_test = r[0];
            if (reflect_test < reflectance) {                               /* :452-454, make_reflected_ray :267-270 */
                V3 reflected_d = reflect(ray.d, N);
                return pathtrace_recursively(ctx, entropy, make_ray(add(I, muls(reflected_d, EPSILON)), reflected_d, FLT_MAX),
                                             recursion - 1);
            }
            V3 brdf = muls(evaluate_material(material, I), 1.0f / PI_32);   /* :456 */
            V2 s2 = { r[1], r[2] };
            V3 R = map_to_hemisphere(N, s2);                                /* :460 */
            Ray diffuse_ray = make_ray(add(I, muls(N, EPSILON)), R, FLT_MAX);
            V3 light = pathtrace_recursively(ctx, entropy, diffuse_ray, recursion - 1);   /* :463 */
            light = muls(light, mx(0.0f, dot(N, diffuse_ray.d)));           /* :464 */
            return mul(smul(2.0f*PI_32, light), brdf);                      /* :466 */
        }
    }
    return sample_sky(scene, &ray);                                         /* :470 */
}

/* One camera sample of render_tile (RT/raytracer.cpp:443-474) with the integrator picked at :467. */
static V3 rr_render_sample(Ctx* ctx, const CamSetup* c, RandomSeries* entropy, V3 ambient, uint32_t x, uint32_t y,
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
        case RT_INTEGRATOR_WHITTED: {                                       /* :417-426 */
            RState rs = { ctx, &s, ambient };
            result = raytrace_recursively(&rs, make_ray(jcp, rd, FLT_MAX), (int32_t)st->max_bounce_count, NULL);
        } break;
        case RT_INTEGRATOR_GROUND_TRUTH_RECURSIVE:                          /* :474-483 */
            result = pathtrace_recursively(ctx, entropy, make_ray(jcp, rd, FLT_MAX), (int32_t)st->max_bounce_count);
            break;
        default:
            result = advanced_integrator(ctx, &s, entropy, jcp, rd);
            break;
    }
    float vig = dot(rd, c->cz);
    vig = vig*vig*vig*vig;
    vig = lerpf_(1.0f, vig, st->vignette_strength);
    result = muls(result, vig);
    *jx_out = jx; *jy_out = jy;
    return result;
}

static int rr_validate(const rt_scene_desc* scene, const rt_settings* st, const rt_filter_cache* f) {
    if (!scene || !st || !f) return RT_ERROR_INVALID;
    if (st->integrator != RT_INTEGRATOR_ADVANCED && st->integrator != RT_INTEGRATOR_WHITTED &&
        st->integrator != RT_INTEGRATOR_GROUND_TRUTH_RECURSIVE) return RT_ERROR_INVALID;
    if (st->max_bounce_count > 63) return RT_ERROR_INVALID;
    if (f->cache_size && (f->kernel_size == 0 || f->kernel_size > 20 || f->cache_size > 256)) return RT_ERROR_INVALID;
    return RT_OK;
}

static void rr_stats(rt_stats* stats, const Ctx* ctx, uint64_t samples, double seconds) {
    if (!stats) return;
    memset(stats, 0, sizeof(*stats));
    stats->closest_hit_rays = ctx->closest_rays;
    stats->shadow_rays = ctx->shadow_rays;
    stats->samples = samples;
    stats->seconds = seconds;
    set_traversal(stats, ctx->ts);
}

/* Same contract as oracle_trace_samples; settings->integrator 0, 1 or 2.  ambient: NULL = (0, 0, 0). */
RR_API int rr_trace_samples(const rt_scene_desc* scene, const rt_camera* camera, const rt_settings* settings,
                            const rt_v3* ambient, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                            uint32_t frame_count, uint32_t total_frame_index,
                            uint32_t count, const uint32_t* pixel_xy, const uint32_t* sample_offset,
                            float* out, rt_stats* stats) {
    rt_filter_cache box;
    memset(&box, 0, sizeof(box));
    int err = rr_validate(scene, settings, &box);
    if (err) return err;
    rt_material air;
    init_air(&air);
    Ctx ctx;
    memset(&ctx, 0, sizeof(ctx));
    ctx.scene = scene; ctx.settings = settings; ctx.air = &air;
    const V3 amb = ambient ? v3(ambient->x, ambient->y, ambient->z) : v3s(0.0f);
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
        V3 r = rr_render_sample(&ctx, &c, &e, amb, x, y, u, v, canonical, &jx, &jy);
        out[5*i + 0] = r.x; out[5*i + 1] = r.y; out[5*i + 2] = r.z;
        out[5*i + 3] = jx; out[5*i + 4] = jy;
    }
    rr_stats(stats, &ctx, count, 0.0);
    return RT_OK;
}

typedef struct {
    const rt_scene_desc* scene; const rt_camera* camera; const rt_settings* settings; const rt_filter_cache* filter;
    const rt_tile_set* tiles; uint32_t total_frame_index; rt_accumulation_buffer* accum; V3 ambient;
    uint32_t tile_lo, tile_hi;          /* this worker's tiles [lo, hi), walked hi-1 .. lo */
    float* pixels;                      /* where this worker splats (w*h float4) */
    uint64_t samples, closest, shadow;
    uint64_t ts[2][TS_N];
} RRJob;

/* The owned tiles of [tile_lo, tile_hi) in the order hi-1 .. lo (RT/raytracer.cpp:555), pixels in raster order
 * inside a tile, samples in order (render_tile, :409-422), splatted straight into job->pixels. */
static void rr_run(RRJob* J) {
    const rt_settings* settings = J->settings;
    const rt_filter_cache* filter = J->filter;
    const rt_tile_set* tiles = J->tiles;
    const uint32_t w = J->accum->w, h = J->accum->h, tw = tiles->tile_w, th = tiles->tile_h;
    const uint32_t tcx = (w + tw - 1) / tw;
    rt_material air;
    init_air(&air);
    Ctx ctx;
    memset(&ctx, 0, sizeof(ctx));
    ctx.scene = J->scene; ctx.settings = settings; ctx.air = &air;
    CamSetup c = cam_setup(J->camera, w, h);
    uint64_t samples = 0;
    for (uint32_t tile = J->tile_hi; tile-- > J->tile_lo;) {
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
                    uint32_t canonical = J->accum->frame_count + s;
                    RandomSeries e = random_seed(oracle_sample_seed(J->total_frame_index, J->accum->frame_count, tile,
                                                                    y*w + x, canonical));
                    float jx, jy;
                    V3 r = rr_render_sample(&ctx, &c, &e, J->ambient, x, y, u, v, canonical, &jx, &jy);
                    if (filter->cache_size) {
                        splat(filter, J->pixels, 0, 0, w, w, h, x, y, jx, jy, r);
                    } else {
                        float* px = J->pixels + 4*((size_t)y*w + x);
                        px[0] += r.x; px[1] += r.y; px[2] += r.z; px[3] += 1.0f;
                    }
                    ++samples;
                }
            }
        }
    }
    J->samples = samples; J->closest = ctx.closest_rays; J->shadow = ctx.shadow_rays;
    memcpy(J->ts, ctx.ts, sizeof(J->ts));
}

static void* rr_worker(void* arg) { rr_run((RRJob*)arg); return NULL; }

/* One frame like oracle_render with RT_RNG_PER_SAMPLE.  threads <= 1: one thread, every splat in the
 * reference's single-threaded order (bit-comparable frames).  threads > 1 (timing runs): the tile range is cut
 * into contiguous spans, each worker splats into a buffer of its own and the buffers are added in span order;
 * the samples are the same, the frame's float sums are not. */
RR_API int rr_render(const rt_scene_desc* scene, const rt_camera* camera, const rt_settings* settings,
                     const rt_filter_cache* filter, const rt_tile_set* tiles, const rt_v3* ambient,
                     uint32_t total_frame_index, uint32_t threads, rt_accumulation_buffer* accum, rt_stats* stats) {
    if (!tiles || !accum || !accum->pixels || !camera || tiles->tile_w == 0 || tiles->tile_h == 0 ||
        tiles->shard_count == 0) return RT_ERROR_INVALID;
    int err = rr_validate(scene, settings, filter);
    if (err) return err;
    double t0 = now_s();
    const uint32_t w = accum->w, h = accum->h, tw = tiles->tile_w, th = tiles->tile_h;
    const uint32_t ntiles = ((w + tw - 1) / tw)*((h + th - 1) / th);
    RRJob base;
    memset(&base, 0, sizeof(base));
    base.scene = scene; base.camera = camera; base.settings = settings; base.filter = filter; base.tiles = tiles;
    base.total_frame_index = total_frame_index; base.accum = accum;
    base.ambient = ambient ? v3(ambient->x, ambient->y, ambient->z) : v3s(0.0f);
    Ctx sum;
    memset(&sum, 0, sizeof(sum));
    uint64_t samples = 0;
    if (threads <= 1 || ntiles < 2) {
        base.tile_lo = 0; base.tile_hi = ntiles; base.pixels = accum->pixels;
        rr_run(&base);
        samples = base.samples; sum.closest_rays = base.closest; sum.shadow_rays = base.shadow;
        memcpy(sum.ts, base.ts, sizeof(sum.ts));
    } else {
        if (threads > ntiles) threads = ntiles;
        if (threads > 64) threads = 64;
        RRJob jobs[64];
        pthread_t th_[64];
        const size_t npx = (size_t)w*h*4;
        for (uint32_t k = 0; k < threads; ++k) {
            jobs[k] = base;
            jobs[k].tile_lo = (uint32_t)((uint64_t)ntiles*k / threads);
            jobs[k].tile_hi = (uint32_t)((uint64_t)ntiles*(k + 1) / threads);
            jobs[k].pixels = (float*)calloc(npx, sizeof(float));
            if (!jobs[k].pixels) { for (uint32_t j = 0; j < k; ++j) free(jobs[j].pixels); return RT_ERROR_OUT_OF_MEMORY; }
        }
        for (uint32_t k = 0; k < threads; ++k) pthread_create(&th_[k], NULL, rr_worker, &jobs[k]);
        for (uint32_t k = 0; k < threads; ++k) pthread_join(th_[k], NULL);
        for (uint32_t k = threads; k-- > 0;) {
            for (size_t i = 0; i < npx; ++i) accum->pixels[i] += jobs[k].pixels[i];
            free(jobs[k].pixels);
            samples += jobs[k].samples; sum.closest_rays += jobs[k].closest; sum.shadow_rays += jobs[k].shadow;
            for (int a = 0; a < 2; ++a) for (int i = 0; i < TS_N; ++i) sum.ts[a][i] += jobs[k].ts[a][i];
        }
    }
    rr_stats(stats, &sum, samples, now_s() - t0);
    return RT_OK;
}

/* oracle_set_math_mode of this library's copy of the oracle: 0 = the deterministic transcendentals the
 * HIP kernels share (default), 1 = the C library's. */
RR_API void rr_set_math_mode(int libm) { oracle_set_math_mode(libm); }
