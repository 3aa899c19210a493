/*
 * ref_specular.c — CPU checker for the specular G-buffer (rt_gbuffer_specular / rt_gbuffer_specular_device).
 * TEST INFRASTRUCTURE ONLY.
 *
 * A unity build over oracle/oracle.c, as tests/ref_temporal is: the camera ray is that checker's (cam_setup,
 * apply_lens_distortion and normalize of the oracle, no jitter, no lens offset), every hit is the oracle's
 * intersect_scene_internal, and the walk of DESIGN.md ("A specular G-buffer") is restated in plain C in the operation
 * order it defines, with the oracle's fresnel_dielectric, reflect and refract.  Nothing else is here.  Built with the
 * oracle's own flags (-ffp-contract=off, no fast-math), so it is bit-comparable with the GPU path.
 */
#include "../../oracle/oracle.c"

#include <stdlib.h>

#define REF_API __attribute__((visibility("default")))

enum { SPEC_STACK = 8, SPEC_AIR = 0xFFFFu };

/* what the tests look at beside the texel and the side record; every field is the walk's state when it ended */
typedef struct {
    rt_v3 final_p, final_n;     /* the last hit's point and normal as intersect_scene returns them (0 after a miss) */
    float M[9];                 /* row-major */
    float T;
    uint32_t level, max_level;  /* of the material stack */
} ref_specular_walk;

/* The ray of pixel (x, y): tests/ref_temporal's gbuffer_ray. */
static void specular_ray(const CamSetup* c, float lens_distortion, uint32_t w, uint32_t h, uint32_t x, uint32_t y,
                         V3* ray_o, V3* ray_d) {
    float v = 1.0f - 2.0f*(float)y*c->pixel_h;
    float u = 1.0f - 2.0f*(float)x*c->pixel_w;
    apply_lens_distortion(lens_distortion, w, h, &u, &v);
    V3 film_p = c->film_center;
    film_p = add(film_p, smul(u*c->hfw, c->cx));
    film_p = add(film_p, smul(v*c->hfh, c->cy));
    *ray_o = c->cp;
    *ray_d = normalize(sub(film_p, c->cp));
}

static const rt_material* spec_mat(const rt_scene_desc* scene, const rt_material* air, uint32_t id) {
    return id == SPEC_AIR ? air : &scene->materials[id];
}

static float row_dot(const float* r, V3 n) { return (r[0]*n.x + r[1]*n.y) + r[2]*n.z; }

static void specular_walk(const rt_scene_desc* scene, const rt_material* air, V3 cp, V3 D,
                          const rt_gbuffer_specular_params* sp, rt_gbuffer_texel* g, rt_specular_texel2* c2,
                          ref_specular_walk* wk) {
    Ray ray = make_ray(cp, D, FLT_MAX);
    float T = 0.0f;
    float M[9] = { 1.0f, 0.0f, 0.0f,  0.0f, 1.0f, 0.0f,  0.0f, 0.0f, 1.0f };
    uint32_t stack[SPEC_STACK];
    int32_t at = 0, max_at = 0;
    uint32_t events = 0, bits = 0, end = RT_SPECULAR_END_MISS;
    uint32_t first_code = RT_HIT_MISS;
    float first_t = 0.0f;
    V3 final_p = v3s(0.0f), final_n = v3s(0.0f);
    stack[0] = SPEC_AIR;
    for (;;) {
        Hit h;
        memset(&h, 0, sizeof(h));
        int hit = intersect_scene_internal(scene, &ray, 0, 0, &h, NULL);
        if (!hit) {
            g->p = D; g->t = 0.0f; g->n = v3s(0.0f); g->primitive = RT_HIT_MISS;
            final_p = v3s(0.0f); final_n = v3s(0.0f);
            break;
        }
        uint32_t code = (h.hit == 1) ? (RT_HIT_PLANE_BIT | h.index) : h.index;
        V3 N = h.n, I = h.hit_p;
        final_p = I; final_n = N;
        g->primitive = code;
        if (events == 0) {
            first_code = code; first_t = h.t;
            T = h.t;
            g->p = I; g->t = h.t; g->n = N;
        } else {
            T = (T + EPSILON) + h.t;
            g->p = add(cp, smul(T, D));
            g->t = T;
            g->n = v3(row_dot(&M[0], N), row_dot(&M[3], N), row_dot(&M[6], N));
        }
        float cos_i = -dot(ray.d, N);
        int inside = (cos_i < 0.0f);
        uint32_t surf_id = (h.hit == 1) ? scene->planes[h.index].material_id : scene->primitives[h.index].material_id;
        const rt_material* surf = &scene->materials[surf_id];
        const rt_material* mi;
        const rt_material* mt;
        uint32_t mt_id;
        if (inside) {
            mi = surf;
            mt_id = stack[at - 1 > 0 ? at - 1 : 0];
            mt = spec_mat(scene, air, mt_id);
            cos_i = -cos_i;
            N = neg(N);
        } else {
            mi = spec_mat(scene, air, stack[at]);
            mt = surf;
            mt_id = surf_id;
        }
        if (mt->flags & RT_MATERIAL_EMISSIVE) { end = RT_SPECULAR_END_EMITTER; break; }
        float eta_i = mi->ior, eta_t = mt->ior;
        float eta = eta_i / eta_t;
        float cos_t;
        float refl = fresnel_dielectric(cos_i, eta_i, eta_t, eta, &cos_t);
        refl = lerpf_(refl, 1.0f, mt->metallic);
        V3 nd;
        if (refl >= sp->reflect_threshold) {
            if (mt->roughness > sp->roughness_max) { end = RT_SPECULAR_END_ROUGH; break; }
            if (events == sp->max_events) { end = RT_SPECULAR_END_CAP; break; }
            nd = reflect(ray.d, N);
            /* M = M*(I - 2 N N^T): H[i][i] = 1 - (2 N_i) N_i, H[i][j] = -((2 N_i) N_j) (a negation, so the sign of a
             * zero is the product's, reversed), then rows of M times columns of H */
            float n[3] = { N.x, N.y, N.z };
            float H[9], R[9];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    H[3*i + j] = i == j ? 1.0f - (2.0f*n[i])*n[j] : -((2.0f*n[i])*n[j]);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    R[3*i + j] = (M[3*i]*H[j] + M[3*i + 1]*H[3 + j]) + M[3*i + 2]*H[6 + j];
            memcpy(M, R, sizeof(M));
            bits |= 1u << (8u + events);
        } else if (mt->is_participating_medium) {
            if (!inside && at >= SPEC_STACK - 1) { end = RT_SPECULAR_END_STACK; break; }
            if (events == sp->max_events) { end = RT_SPECULAR_END_CAP; break; }
            if (inside) {
                if (at > 0) --at;
            } else {
                ++at;
                stack[at] = mt_id;
                if (at > max_at) max_at = at;
            }
            nd = refract(ray.d, N, cos_i, cos_t, eta);
        } else {
            end = RT_SPECULAR_END_DIFFUSE;
            break;
        }
        ray = make_ray(add(I, smul(EPSILON, nd)), nd, FLT_MAX);
        ++events;
    }
    if (c2) { c2->first_primitive = first_code; c2->first_t = first_t; c2->chain = events | bits; c2->end = end; }
    if (wk) {
        wk->final_p = final_p; wk->final_n = final_n;
        memcpy(wk->M, M, sizeof(M));
        wk->T = T;
        wk->level = (uint32_t)at; wk->max_level = (uint32_t)max_at;
    }
}

/* The arguments of rt_gbuffer_specular less the device scene; chain and walk may be NULL.  RT_OK, or RT_ERROR_INVALID
 * for the parameters rt_gbuffer_specular refuses. */
REF_API int ref_gbuffer_specular(const rt_scene_desc* scene, const rt_camera* camera, float lens_distortion, uint32_t w,
                                 uint32_t h, const rt_gbuffer_specular_params* sp, rt_gbuffer_texel* out,
                                 rt_specular_texel2* chain, ref_specular_walk* walk) {
    if (!scene || !camera || !sp || !out || !w || !h) return RT_ERROR_INVALID;
    if (sp->max_events > 16u) return RT_ERROR_INVALID;
    if (!(sp->reflect_threshold >= 0.0f) || sp->reflect_threshold > FLT_MAX) return RT_ERROR_INVALID;
    if (!(sp->roughness_max >= 0.0f) || sp->roughness_max > FLT_MAX) return RT_ERROR_INVALID;
    rt_material air;
    init_air(&air);
    CamSetup c = cam_setup(camera, w, h);
    for (uint32_t y = 0; y < h; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            size_t i = (size_t)y*w + x;
            V3 ro, rd;
            specular_ray(&c, lens_distortion, w, h, x, y, &ro, &rd);
            specular_walk(scene, &air, ro, rd, sp, &out[i], chain ? &chain[i] : NULL, walk ? &walk[i] : NULL);
        }
    }
    return RT_OK;
}

/* One ray from anywhere (the TIR test starts inside glass, where the empty stack names the air as the far side): the
 * walk from (o, d).  The texel's p and the unfolding use o as the camera position. */
REF_API int ref_specular_walk_ray(const rt_scene_desc* scene, const float* o, const float* d,
                                  const rt_gbuffer_specular_params* sp, rt_gbuffer_texel* out, rt_specular_texel2* chain,
                                  ref_specular_walk* walk) {
    if (!scene || !o || !d || !sp || !out) return RT_ERROR_INVALID;
    rt_material air;
    init_air(&air);
    specular_walk(scene, &air, v3(o[0], o[1], o[2]), v3(d[0], d[1], d[2]), sp, out, chain, walk);
    return RT_OK;
}
