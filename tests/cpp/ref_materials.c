/*
 * ref_materials.c — CPU restatement of the integrator with material models. TEST INFRASTRUCTURE ONLY.
 *
 * ref_trace_ray (oracle/cpu_ref.c) restated with spt_material_model (include/spt.h "materials"), from the
 * oracle's exported pieces: ref_intersect, ref_bounce_dir, ref_random_float, ref_light_sample,
 * ref_visible, ref_emitter_count, ref_sample_sky, ref_octa_texel. The METAL and DIELECTRIC step below
 * is written from the text of spt.h; it shares no code with the product (csrc/spt_device.h is not
 * included). Compiled with -ffp-contract=off, like the oracle. With models == NULL it is ref_trace_ray,
 * bit for bit (tests/test_materials_host.py asserts that).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/cpu_ref.h"
#include "spt.h"

typedef struct mat_scene {
    const ref_scene* scene;           /* the oracle's scene of the same prims / mats / env */
    const spt_prim* prims;            /* the caller's arrays (the oracle's scene is opaque) */
    const spt_material* mats;
    const spt_material_model* models; /* one per material, or NULL: all DIFFUSE */
    spt_env env;
    const float* env_map;             /* octahedral RGBA texels or NULL */
    uint32_t env_w, env_h;
} mat_scene;

static float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static void cross3(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - b[1] * a[2];
    out[1] = a[2] * b[0] - b[2] * a[0];
    out[2] = a[0] * b[1] - b[0] * a[1];
}
static void normalize3(float v[3]) {
    const float inv = 1.0f / sqrtf(dot3(v, v));
    v[0] = v[0] * inv;
    v[1] = v[1] * inv;
    v[2] = v[2] * inv;
}

/* METAL(f) around nf; returns 1 when absorbed. f == 0 draws nothing. */
static int metal_step(float f, const float d[3], const float nf[3], uint32_t flags, uint32_t* rng, float r[3]) {
    const float c = dot3(d, nf);
    for (int k = 0; k < 3; ++k) r[k] = d[k] - (2.0f * c) * nf[k];
    if (f > 0.0f) {
        float b[3];
        ref_bounce_dir(nf, rng, flags, b);
        for (int k = 0; k < 3; ++k) r[k] = r[k] + f * b[k];
    }
    normalize3(r);
    return !(dot3(r, nf) > 0.0f);
}

/* The scattering step of a METAL or DIELECTRIC model: the new direction, whether it is transmitted;
 * returns 1 when the path is absorbed. */
int mat_scatter(const spt_material_model* m, const float d[3], const float nf[3], int entering, uint32_t flags,
                uint32_t* rng, float out[3], int* transmitted) {
    *transmitted = 0;
    if (m->kind == SPT_MAT_METAL) return metal_step(m->param, d, nf, flags, rng, out);
    const float ior = m->param;
    const float u = ref_random_float(rng);
    const float eta = entering ? 1.0f / ior : ior;
    const float ci = fminf(-dot3(d, nf), 1.0f);
    const float s2 = fmaxf(1.0f - ci * ci, 0.0f);
    const float k = (eta * eta) * s2;
    const float ct = sqrtf(fmaxf(1.0f - k, 0.0f));
    const float q = (1.0f - ior) / (1.0f + ior);
    const float r0 = q * q;
    const float x = 1.0f - (entering ? ci : ct);
    const float x2 = x * x;
    const float R = r0 + (1.0f - r0) * ((x2 * x2) * x);
    if (k > 1.0f || R > u) return metal_step(0.0f, d, nf, flags, rng, out);
    for (int c = 0; c < 3; ++c) out[c] = eta * (d[c] + ci * nf[c]) - ct * nf[c];
    normalize3(out);
    *transmitted = 1;
    return 0;
}

/* spt_bsdf_sample's interface: n the outward normal, nf = entering ? n : -n; DIFFUSE bounces around n. */
void mat_bsdf_sample(const spt_material_model* m, const float d[3], const float n[3], int entering, uint32_t flags,
                     uint32_t* rng, float out[3], int* transmitted, int* absorbed) {
    *transmitted = 0;
    *absorbed = 0;
    if (m->kind == SPT_MAT_DIFFUSE) {
        ref_bounce_dir(n, rng, flags, out);
        return;
    }
    const float nf[3] = {entering ? n[0] : -n[0], entering ? n[1] : -n[1], entering ? n[2] : -n[2]};
    *absorbed = mat_scatter(m, d, nf, entering, flags, rng, out, transmitted);
}

/* whether the ray (direction d, ref_intersect's already flipped normal ng) arrives on the side of the
 * primitive's own normal: the sign of ng against cross(u, v) / cross(v1 - v0, v2 - v0) */
static int entering_flat(const spt_prim* p, const float ng[3]) {
    float e1[3], e2[3], nv[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = p->type == SPT_PRIM_QUAD ? p->p1[k] : p->p1[k] - p->p0[k];
        e2[k] = p->type == SPT_PRIM_QUAD ? p->p2[k] : p->p2[k] - p->p0[k];
    }
    cross3(e1, e2, nv);
    for (int k = 0; k < 3; ++k)
        if (nv[k] != 0.0f) return ng[k] == nv[k];
    return 1;
}

void mat_trace_ray(const mat_scene* ms, const ref_config* cfg, const float ray_origin[3], const float ray_direction[3],
                   uint32_t* rng_state, float out[4]) {
    const ref_scene* s = ms->scene;
    const int max_bounces = (int)cfg->max_bounces;
    const int nee = (cfg->flags & SPT_FLAG_NEE) && ref_emitter_count(s) > 0;
    float L[3] = {0.0f, 0.0f, 0.0f};
    float T[3] = {1.0f, 1.0f, 1.0f};
    float o[3] = {ray_origin[0], ray_origin[1], ray_origin[2]};
    float d[3] = {ray_direction[0], ray_direction[1], ray_direction[2]};
    int bounce_count = 0;
    int spec_prev = 0; /* the previous vertex was METAL or DIELECTRIC */
    while (bounce_count < max_bounces) {
        float hit_t, ng[3];
        uint32_t prim;
        if (!ref_intersect(s, o, d, 0.001f, &hit_t, &prim, ng)) {
            if (ms->env.sky_enabled) {
                float sky[3];
                if (ms->env_map) {
                    const float* e = ms->env_map + 4 * (size_t)ref_octa_texel(d[0], d[1], d[2], ms->env_w, ms->env_h);
                    sky[0] = e[0];
                    sky[1] = e[1];
                    sky[2] = e[2];
                } else {
                    ref_sample_sky(&ms->env, d, sky);
                }
                for (int k = 0; k < 3; ++k) L[k] += T[k] * sky[k];
            }
            break;
        }
        o[0] += hit_t * d[0];
        o[1] += hit_t * d[1];
        o[2] += hit_t * d[2];
        const float inv_len = 1.0f / sqrtf(ng[0] * ng[0] + ng[1] * ng[1] + ng[2] * ng[2]);
        const float n[3] = {ng[0] * inv_len, ng[1] * inv_len, ng[2] * inv_len};
        const spt_prim* p = &ms->prims[prim];
        const spt_material* m = &ms->mats[p->material];
        const spt_material_model diffuse = {SPT_MAT_DIFFUSE, 0.0f, {0, 0}};
        const spt_material_model* model = ms->models ? &ms->models[p->material] : &diffuse;
        const int counted = !nee || bounce_count == 0 || spec_prev;
        if ((m->emission[0] != 0.0f || m->emission[1] != 0.0f || m->emission[2] != 0.0f) && counted)
            for (int k = 0; k < 3; ++k) L[k] += T[k] * m->emission[k];
        for (int k = 0; k < 3; ++k) T[k] *= m->albedo[k];
        bounce_count++;
        const int is_diffuse = model->kind == SPT_MAT_DIFFUSE;
        if (nee && bounce_count < max_bounces && is_diffuse) {
            const float x[3] = {o[0] + n[0] * 1e-4f, o[1] + n[1] * 1e-4f, o[2] + n[2] * 1e-4f};
            float w[3], tmax, add[3];
            if (ref_light_sample(s, x, n, T, rng_state, w, &tmax, add) && ref_visible(s, x, w, tmax))
                for (int k = 0; k < 3; ++k) L[k] += add[k];
        }
        if (bounce_count > (int)cfg->rr_depth) {
            float pmax = T[0];
            if (T[1] > pmax) pmax = T[1];
            if (T[2] > pmax) pmax = T[2];
            if (ref_random_float(rng_state) > pmax) break;
            for (int k = 0; k < 3; ++k) T[k] /= pmax;
        }
        if (is_diffuse) {
            ref_bounce_dir(n, rng_state, cfg->flags, d);
            for (int k = 0; k < 3; ++k) o[k] += n[k] * 1e-4f;
            spec_prev = 0;
            continue;
        }
        int entering;
        float nf[3] = {n[0], n[1], n[2]};
        if (p->type == SPT_PRIM_SPHERE) {
            entering = !(dot3(d, n) > 0.0f);
            if (!entering)
                for (int k = 0; k < 3; ++k) nf[k] = -n[k];
        } else {
            entering = entering_flat(p, ng);
        }
        float nd[3];
        int transmitted;
        if (mat_scatter(model, d, nf, entering, cfg->flags, rng_state, nd, &transmitted)) break; /* absorbed */
        for (int k = 0; k < 3; ++k) {
            o[k] = transmitted ? o[k] - nf[k] * 1e-4f : o[k] + nf[k] * 1e-4f;
            d[k] = nd[k];
        }
        spec_prev = 1;
    }
    out[0] = L[0];
    out[1] = L[1];
    out[2] = L[2];
    out[3] = 1.0f;
}

/* trace_ray's (L, 1) of every pixel of frames [first_frame, first_frame + n_frames) through the
 * reference's camera: frames[f][y][x][4] (not accumulated) */
void mat_render_frames(const mat_scene* ms, const ref_config* cfg, uint32_t first_frame, uint32_t n_frames,
                       float* frames) {
    const float origin[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t f = 0; f < n_frames; ++f)
        for (uint32_t y = 0; y < cfg->height; ++y)
            for (uint32_t x = 0; x < cfg->width; ++x) {
                uint32_t rng = ref_rng_seed(x, y, cfg->width, first_frame + f + 1u);
                float dir[3];
                ref_primary_dir(x, y, cfg->width, cfg->height, dir);
                mat_trace_ray(ms, cfg, origin, dir, &rng, frames + 4 * (((size_t)f * cfg->height + y) * cfg->width + x));
            }
}
