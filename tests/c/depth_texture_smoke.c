/* depth_texture_smoke.c -- a plain-C caller of the depth texture entry points (include/swr.h): dlopen()s
 * libswr_hip.so, sets a few depth words of an 8 x 4 frame, reduces it (2, 2) into a 4 x 2 depth texture under MAX, MIN and FIRST and
 * checks the words, one lookup and one refusal.
 * usage: depth_texture_smoke /path/to/libswr_hip.so      exit code 0 = ok.   Built with gcc (tests/c/Makefile), no HIP headers. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include "swr.h"

#define RESOLVE(name) do { *(void**)(&p_##name) = dlsym(lib, #name); if (!p_##name) { fprintf(stderr, "missing symbol %s\n", #name); return 2; } } while (0)
#define MINVALUE (-3.40282347e+38f)

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s libswr_hip.so\n", argv[0]); return 2; }
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    const char* (*p_swr_last_error)(const swr_context*);
    int (*p_swr_create)(int, swr_context**);
    void (*p_swr_destroy)(swr_context*);
    int (*p_swr_resize)(swr_context*, int, int);
    int (*p_swr_clear_depth)(swr_context*);
    int (*p_swr_set_depth)(swr_context*, int, int, float);
    int (*p_swr_texture_create_depth)(swr_context*, const float*, int, int, swr_texture**);
    int (*p_swr_texture_update_from_depth)(swr_context*, swr_texture*, swr_context*, int, int, int);
    int (*p_swr_texture_readback_depth)(swr_context*, const swr_texture*, float*);
    int (*p_swr_texture_sample_depth)(swr_context*, const swr_texture*, const float*, int, float*);
    int (*p_swr_texture_format)(swr_context*, const swr_texture*, int*);
    int (*p_swr_texture_readback)(swr_context*, const swr_texture*, uint8_t*);
    int (*p_swr_texture_destroy)(swr_context*, swr_texture*);
    RESOLVE(swr_last_error); RESOLVE(swr_create); RESOLVE(swr_destroy); RESOLVE(swr_resize); RESOLVE(swr_clear_depth); RESOLVE(swr_set_depth);
    RESOLVE(swr_texture_create_depth); RESOLVE(swr_texture_update_from_depth); RESOLVE(swr_texture_readback_depth);
    RESOLVE(swr_texture_sample_depth); RESOLVE(swr_texture_format); RESOLVE(swr_texture_readback); RESOLVE(swr_texture_destroy);

    swr_context* ctx = NULL;
    int rc = p_swr_create(0, &ctx);
    if (rc != SWR_OK) { fprintf(stderr, "swr_create: %d %s\n", rc, p_swr_last_error(NULL)); return 4; }   /* no CPU fallback */
#define CK(call) do { rc = (call); if (rc != SWR_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc, p_swr_last_error(ctx)); return 5; } } while (0)
    CK(p_swr_resize(ctx, 8, 4));
    CK(p_swr_clear_depth(ctx));
    /* block (0, 0): 0.25 0.75 / 0.5 (cleared)   block (3, 1): only its bottom-right word, -1 */
    CK(p_swr_set_depth(ctx, 0, 0, 0.25f)); CK(p_swr_set_depth(ctx, 1, 0, 0.75f)); CK(p_swr_set_depth(ctx, 0, 1, 0.5f));
    CK(p_swr_set_depth(ctx, 7, 3, -1.0f));
    swr_texture* tex = NULL;
    CK(p_swr_texture_create_depth(ctx, NULL, 4, 2, &tex));
    int format = -1, bad = 0;
    CK(p_swr_texture_format(ctx, tex, &format));
    float t[8];
    CK(p_swr_texture_readback_depth(ctx, tex, t));
    for (int i = 0; i < 8; ++i) bad += t[i] != MINVALUE;
    if (format != SWR_TEXTURE_FORMAT_DEPTH32F || bad) { fprintf(stderr, "a new depth texture: format %d, %d words not float.MinValue\n", format, bad); return 6; }
    const float want[3][2] = { { 0.75f, -1.0f }, { MINVALUE, MINVALUE }, { 0.25f, MINVALUE } };     /* texel 0 and texel 7 under MAX, MIN, FIRST */
    for (int reduce = SWR_DEPTH_REDUCE_MAX; reduce <= SWR_DEPTH_REDUCE_FIRST; ++reduce) {
        CK(p_swr_texture_update_from_depth(ctx, tex, NULL, 2, 2, reduce));
        CK(p_swr_texture_readback_depth(ctx, tex, t));
        for (int i = 0; i < 8; ++i) bad += t[i] != (i == 0 ? want[reduce][0] : i == 7 ? want[reduce][1] : MINVALUE);
    }
    /* FIRST is in the texture now: texel 0 holds 0.25.  Its centre, ref 0.25 (passes) and ref 0.2 (does not) */
    const float uv_ref[6] = { 0.125f, 0.25f, 0.25f, 0.125f, 0.25f, 0.2f };
    float ds[4];
    CK(p_swr_texture_sample_depth(ctx, tex, uv_ref, 2, ds));
    bad += !(ds[0] == 0.25f && ds[1] == 1.0f && ds[2] == 0.25f && ds[3] == 0.0f);
    uint8_t bytes[32];
    memset(bytes, 0, sizeof bytes);
    const int refused = p_swr_texture_readback(ctx, tex, bytes);
    for (int i = 0; i < 32; ++i) bad += bytes[i] != 0;
    printf("depth_texture_smoke: wrong=%d refused=%d (%s)\n", bad, refused, p_swr_last_error(ctx));
    CK(p_swr_texture_destroy(ctx, tex));
    p_swr_destroy(ctx);
    return (bad == 0 && refused == SWR_ERR_INVALID_ARG) ? 0 : 7;
}
