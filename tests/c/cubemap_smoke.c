/* cubemap_smoke.c -- a plain-C caller of the cube map entry points (include/swr.h): dlopen()s libswr_hip.so,
 * uploads a 2 x 2 x 6 cube whose red byte names the face and whose green byte the texel, and checks one lookup per face, a face
 * readback, the face cameras, a depth cube's shadow and one refusal.
 * usage: cubemap_smoke /path/to/libswr_hip.so      exit code 0 = ok.   Built with gcc (tests/c/cubemap_smoke.mk), no HIP headers. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include "swr.h"

#define RESOLVE(name) do { *(void**)(&p_##name) = dlsym(lib, #name); if (!p_##name) { fprintf(stderr, "missing symbol %s\n", #name); return 2; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s libswr_hip.so\n", argv[0]); return 2; }
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    const char* (*p_swr_last_error)(const swr_context*);
    int (*p_swr_create)(int, swr_context**);
    void (*p_swr_destroy)(swr_context*);
    int (*p_swr_texture_create_cube)(swr_context*, const uint8_t*, int, swr_texture**);
    int (*p_swr_texture_create_cube_depth)(swr_context*, const float*, int, swr_texture**);
    int (*p_swr_texture_is_cube)(swr_context*, const swr_texture*, int*);
    int (*p_swr_texture_readback_face)(swr_context*, const swr_texture*, int, int, void*);
    int (*p_swr_cube_face_view)(int, const float*, float*);
    int (*p_swr_texture_cube_face)(swr_context*, const float*, int, int*, float*);
    int (*p_swr_texture_sample_cube)(swr_context*, const swr_texture*, const float*, int, float*);
    int (*p_swr_texture_sample_cube_depth)(swr_context*, const swr_texture*, const float*, int, float*);
    int (*p_swr_texture_update_face_from_frame)(swr_context*, swr_texture*, int, swr_context*, int, int, int);
    int (*p_swr_texture_destroy)(swr_context*, swr_texture*);
    RESOLVE(swr_last_error); RESOLVE(swr_create); RESOLVE(swr_destroy); RESOLVE(swr_texture_create_cube); RESOLVE(swr_texture_create_cube_depth);
    RESOLVE(swr_texture_is_cube); RESOLVE(swr_texture_readback_face); RESOLVE(swr_cube_face_view); RESOLVE(swr_texture_cube_face);
    RESOLVE(swr_texture_sample_cube); RESOLVE(swr_texture_sample_cube_depth); RESOLVE(swr_texture_update_face_from_frame); RESOLVE(swr_texture_destroy);

    int bad = 0;
    /* host only: the -Z camera at (1, 2, 3) is the identity rotation with the eye subtracted */
    const float eye[3] = { 1.0f, 2.0f, 3.0f };
    float view[16];
    bad += p_swr_cube_face_view(5, eye, view) != SWR_OK;
    bad += !(view[0] == 1.0f && view[5] == 1.0f && view[10] == 1.0f && view[12] == -1.0f && view[13] == -2.0f && view[14] == -3.0f && view[15] == 1.0f);
    bad += p_swr_cube_face_view(6, eye, view) != SWR_ERR_INVALID_ARG;

    swr_context* ctx = NULL;
    int rc = p_swr_create(0, &ctx);
    if (rc != SWR_OK) { fprintf(stderr, "swr_create: %d %s\n", rc, p_swr_last_error(NULL)); return 4; }   /* no CPU fallback */
#define CK(call) do { rc = (call); if (rc != SWR_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc, p_swr_last_error(ctx)); return 5; } } while (0)
    uint8_t texels[6 * 4 * 4], got[16];
    for (int f = 0; f < 6; ++f)
        for (int i = 0; i < 4; ++i) { uint8_t* p = texels + (f * 4 + i) * 4; p[0] = (uint8_t)(f * 40); p[1] = (uint8_t)(i * 80); p[2] = 0; p[3] = 255; }
    swr_texture* cube = NULL;
    CK(p_swr_texture_create_cube(ctx, texels, 2, &cube));
    int n = -1;
    CK(p_swr_texture_is_cube(ctx, cube, &n));
    bad += n != 2;
    CK(p_swr_texture_readback_face(ctx, cube, 3, 0, got));
    bad += memcmp(got, texels + 3 * 16, 16) != 0;
    /* the six axes: face f, its centre (0.5, 0.5) -> texel (1, 1) = index 3 under the nearest filter */
    const float axes[6][3] = { { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 } };
    int face[6]; float st[12], dir_lod[24], rgba[24];
    CK(p_swr_texture_cube_face(ctx, &axes[0][0], 6, face, st));
    for (int f = 0; f < 6; ++f) {
        bad += !(face[f] == f && st[2 * f] == 0.5f && st[2 * f + 1] == 0.5f);
        dir_lod[4 * f] = axes[f][0]; dir_lod[4 * f + 1] = axes[f][1]; dir_lod[4 * f + 2] = axes[f][2]; dir_lod[4 * f + 3] = 0.0f;
    }
    CK(p_swr_texture_sample_cube(ctx, cube, dir_lod, 6, rgba));
    for (int f = 0; f < 6; ++f)
        bad += !(rgba[4 * f] == (float)(f * 40) * (1.0f / 255.0f) && rgba[4 * f + 1] == 240.0f * (1.0f / 255.0f) && rgba[4 * f + 3] == 255.0f * (1.0f / 255.0f));
    /* a depth cube: every word -0.5; a reference of -0.25 is nearer (lit, 1), -0.75 is behind (0) */
    float words[6 * 4], dir_ref[8] = { 0, 1, 0, -0.25f, 0, 0, -2, -0.75f }, ds[4];
    for (int i = 0; i < 24; ++i) words[i] = -0.5f;
    swr_texture* shadow = NULL;
    CK(p_swr_texture_create_cube_depth(ctx, words, 2, &shadow));
    CK(p_swr_texture_sample_cube_depth(ctx, shadow, dir_ref, 2, ds));
    bad += !(ds[0] == -0.5f && ds[1] == 1.0f && ds[2] == -0.5f && ds[3] == 0.0f);
    const int refused = p_swr_texture_update_face_from_frame(ctx, cube, 6, NULL, 1, 1, 0);      /* there is no face 6 */
    printf("cubemap_smoke: wrong=%d refused=%d (%s)\n", bad, refused, p_swr_last_error(ctx));
    CK(p_swr_texture_destroy(ctx, shadow));
    CK(p_swr_texture_destroy(ctx, cube));
    p_swr_destroy(ctx);
    return (bad == 0 && refused == SWR_ERR_INVALID_ARG) ? 0 : 7;
}
