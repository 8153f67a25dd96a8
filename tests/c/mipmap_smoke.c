/* mipmap_smoke.c -- a plain-C caller of the mip chain entry points (include/swr.h): dlopen()s libswr_hip.so,
 * uploads a 4 x 2 texture, generates its chain (4 x 2 -> 2 x 1 -> 1 x 1) and checks the levels' bytes, one lookup by lod, one lod and
 * one refusal.
 * usage: mipmap_smoke /path/to/libswr_hip.so      exit code 0 = ok.   Built with gcc (tests/c/mipmap_smoke.mk), no HIP headers. */
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
    int (*p_swr_texture_create)(swr_context*, const uint8_t*, int, int, swr_texture**);
    int (*p_swr_texture_generate_mipmaps)(swr_context*, swr_texture*);
    int (*p_swr_texture_levels)(swr_context*, const swr_texture*, int*);
    int (*p_swr_texture_level_size)(swr_context*, const swr_texture*, int, int*, int*);
    int (*p_swr_texture_readback_level)(swr_context*, const swr_texture*, int, uint8_t*);
    int (*p_swr_texture_sample_lod)(swr_context*, const swr_texture*, const float*, int, float*);
    int (*p_swr_texture_lod)(swr_context*, const swr_texture*, const float*, int, float*);
    int (*p_swr_texture_destroy)(swr_context*, swr_texture*);
    RESOLVE(swr_last_error); RESOLVE(swr_create); RESOLVE(swr_destroy); RESOLVE(swr_texture_create); RESOLVE(swr_texture_generate_mipmaps);
    RESOLVE(swr_texture_levels); RESOLVE(swr_texture_level_size); RESOLVE(swr_texture_readback_level); RESOLVE(swr_texture_sample_lod);
    RESOLVE(swr_texture_lod); RESOLVE(swr_texture_destroy);

    swr_context* ctx = NULL;
    int rc = p_swr_create(0, &ctx);
    if (rc != SWR_OK) { fprintf(stderr, "swr_create: %d %s\n", rc, p_swr_last_error(NULL)); return 4; }   /* no CPU fallback */
#define CK(call) do { rc = (call); if (rc != SWR_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc, p_swr_last_error(ctx)); return 5; } } while (0)
    /* R of the eight texels, row-major; G = 255 - R, B = 0, A = 255.  Level 1: (0 + 1 + 1 + 1 + 2) >> 2 = 1 and (255 + 255 + 254 + 254 + 2) >> 2 = 255;
     * level 2: the clamp duplicates the row of the 2 x 1 level: (1 + 255 + 1 + 255 + 2) >> 2 = 128 */
    const uint8_t red[8] = { 0, 1, 255, 255, 1, 1, 254, 254 };
    uint8_t texels[32], got[32];
    for (int i = 0; i < 8; ++i) { texels[4 * i] = red[i]; texels[4 * i + 1] = (uint8_t)(255 - red[i]); texels[4 * i + 2] = 0; texels[4 * i + 3] = 255; }
    swr_texture* tex = NULL;
    CK(p_swr_texture_create(ctx, texels, 4, 2, &tex));
    int levels = -1, w = -1, h = -1, bad = 0;
    CK(p_swr_texture_levels(ctx, tex, &levels));
    bad += levels != 1;
    memset(got, 0, sizeof got);
    const int refused = p_swr_texture_readback_level(ctx, tex, 1, got);      /* it has no level 1 yet */
    for (int i = 0; i < 32; ++i) bad += got[i] != 0;
    CK(p_swr_texture_generate_mipmaps(ctx, tex));
    CK(p_swr_texture_levels(ctx, tex, &levels));
    bad += levels != 3;
    CK(p_swr_texture_level_size(ctx, tex, 1, &w, &h));
    bad += !(w == 2 && h == 1);
    CK(p_swr_texture_readback_level(ctx, tex, 0, got));
    bad += memcmp(got, texels, 32) != 0;
    CK(p_swr_texture_readback_level(ctx, tex, 1, got));
    bad += !(got[0] == 1 && got[1] == 254 && got[2] == 0 && got[3] == 255 && got[4] == 255 && got[5] == 1 && got[6] == 0 && got[7] == 255);
    CK(p_swr_texture_readback_level(ctx, tex, 2, got));
    bad += !(got[0] == 128 && got[1] == 128 && got[2] == 0 && got[3] == 255);
    /* lod 2 at any uv is the last level's one texel; the gradient (1, 0, 0, 0) is 4 texels per pixel: lod 2 */
    const float uv_lod[3] = { 0.3f, 0.6f, 2.0f }, grad[4] = { 1.0f, 0.0f, 0.0f, 0.0f };
    float rgba[4], lod = -1.0f;
    CK(p_swr_texture_sample_lod(ctx, tex, uv_lod, 1, rgba));
    bad += !(rgba[0] == 128.0f * (1.0f / 255.0f) && rgba[2] == 0.0f && rgba[3] == 255.0f * (1.0f / 255.0f));
    CK(p_swr_texture_lod(ctx, tex, grad, 1, &lod));
    bad += lod != 2.0f;
    printf("mipmap_smoke: wrong=%d refused=%d (%s)\n", bad, refused, p_swr_last_error(ctx));
    CK(p_swr_texture_destroy(ctx, tex));
    p_swr_destroy(ctx);
    return (bad == 0 && refused == SWR_ERR_INVALID_ARG) ? 0 : 7;
}
