// look_host_check.cpp -- a stand-alone host program for tests/test_look_host.py: the host code of the look (include/mlvfs_amd.h, "a
// look for the rendered frames") -- mlvfs_amd_look_image_size and mlvfs_amd_look_pack against images computed in Python, with buffers
// of exactly the sizes they may touch, every refusal with the image untouched, and the argument checks of the three _look_dev calls,
// of mlvfs_amd_look_apply_dev and of mlvfs_amd_mount_set_look, which happen before any device work and follow no pointer.  It is
// compiled and linked with -fsanitize=address,undefined against the sanitizer build of the library's host code (`make -C
// mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// The file named on the command line: records of {int32 n, uint16 S[4096], uint16 T[3 n^3], the expected image of 8192 + 8 n^3 bytes}.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "look_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: look_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0, refusals = 0;
    for (;; rec++) {
        int32_t n;
        if (fread(&n, sizeof n, 1, f) != 1) break;
        const size_t entries = (size_t)n * n * n, size = 8192 + 8 * entries;
        if (mlvfs_amd_look_image_size(n) != size) return fail("another image size", rec);
        // exactly as long as what may be read and written: a step past any of them is the sanitizer's to see
        std::unique_ptr<uint16_t[]> S(new uint16_t[4096]), T(new uint16_t[3 * entries]);
        std::unique_ptr<uint8_t[]> want(new uint8_t[size]), got(new uint8_t[size]);
        if (fread(S.get(), 2, 4096, f) != 4096 || fread(T.get(), 2, 3 * entries, f) != 3 * entries || fread(want.get(), 1, size, f) != size)
            return fail("a short record", rec);
        memset(got.get(), 0xA5, size);
        if (mlvfs_amd_look_pack(S.get(), n, T.get(), got.get(), size) != MLVFS_AMD_OK) return fail("look_pack refused", rec);
        if (memcmp(got.get(), want.get(), size)) return fail("another image", rec);
        // every refusal leaves the image as it was
        memset(got.get(), 0xA5, size);
        const int rcs[] = { mlvfs_amd_look_pack(nullptr, n, T.get(), got.get(), size), mlvfs_amd_look_pack(S.get(), n, nullptr, got.get(), size),
                            mlvfs_amd_look_pack(S.get(), n, T.get(), nullptr, size), mlvfs_amd_look_pack(S.get(), n, T.get(), got.get(), size - 1),
                            mlvfs_amd_look_pack(S.get(), n, T.get(), got.get(), 0), mlvfs_amd_look_pack(S.get(), 1, T.get(), got.get(), size),
                            mlvfs_amd_look_pack(S.get(), 66, T.get(), got.get(), size), mlvfs_amd_look_pack(S.get(), 0, T.get(), got.get(), size),
                            mlvfs_amd_look_pack(S.get(), -3, T.get(), got.get(), size), mlvfs_amd_look_pack(S.get(), 1 << 30, T.get(), got.get(), size) };
        for (int rc : rcs) {
            if (rc != MLVFS_AMD_ERR_ARG) return fail("a refusal of look_pack did not happen", rec);
            refusals++;
        }
        for (size_t i = 0; i < size; i++) if (got[i] != 0xA5) return fail("a refusal wrote the image", rec);
        if (mlvfs_amd_look_create(nullptr, n, T.get()) || mlvfs_amd_look_create(S.get(), n, nullptr) || mlvfs_amd_look_create(S.get(), 1, T.get()) ||
            mlvfs_amd_look_create(S.get(), 66, T.get()))
            return fail("look_create took what it must refuse", rec);
    }
    fclose(f);
    for (int n : { -1, 0, 1, 66, 1 << 20, (int)0x80000000 })
        if (mlvfs_amd_look_image_size(n) != 0) return fail("an image size for a table that is none", n);
    if (mlvfs_amd_look_image_size(2) != 8192 + 64 || mlvfs_amd_look_image_size(65) != 8192 + 8 * 274625) return fail("another image size", 65);
    mlvfs_amd_look_destroy(nullptr);

    // the three _look_dev calls: a 32 x 8 frame, 512 bytes in; the buffers are host memory; `look` is never followed by a check
    std::unique_ptr<uint16_t[]> px(new uint16_t[3 * 256]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[3 * 1024]);
    std::unique_ptr<int32_t[]> par(new int32_t[3 * 13]);
    memset(px.get(), 7, 3 * 512);
    memset(out.get(), 9, 3 * 1024);
    memset(par.get(), 0, 3 * 13 * sizeof(int32_t));
    uint8_t *s = (uint8_t *)px.get(), *d = out.get();
    int32_t *p = par.get();
    const mlvfs_amd_look_t *lk = (const mlvfs_amd_look_t *)(const void *)out.get();          // any non-null address: no check reads it
    struct Case { const void *src; size_t stride; int w, h; const int32_t *par; void *dst; size_t ostride; int n; const mlvfs_amd_look_t *look; };
    const Case bad[] = {
        { s, 512, 32, 8, p, d, 1024, 1, nullptr }, { nullptr, 512, 32, 8, p, d, 1024, 1, lk }, { s, 512, 32, 8, nullptr, d, 1024, 1, lk },
        { s, 512, 32, 8, p, nullptr, 1024, 1, lk }, { s, 512, 1, 8, p, d, 1024, 1, lk }, { s, 512, 32, 1, p, d, 1024, 1, lk },
        { s, 512, 1 << 14, 1 << 13, p, d, 1024, 1, lk }, { s, 512, -32, 8, p, d, 1024, 1, lk }, { s, 512, 32, 8, p, d, 1024, -1, lk },
        { s, 510, 32, 8, p, d, 1024, 2, lk }, { s, 512, 32, 8, p, d, 40, 2, lk }, { s, 513, 32, 8, p, d, 1024, 2, lk }, { s + 1, 512, 32, 8, p, d, 1024, 1, lk },
        { s, 512, 32, 8, (const int32_t *)((const uint8_t *)p + 2), d, 1024, 1, lk }, { s, 512, 32, 8, p, s, 1024, 1, lk }, { s, 512, 32, 8, p, s + 511, 1024, 1, lk },
        { s, 512, 32, 8, p, p, 1024, 1, lk }, { s, 512, 32, 8, p, (uint8_t *)p + 51, 1024, 1, lk },
    };
    int k = 0;
    for (const Case &c : bad) {
        if (mlvfs_amd_render2_look_dev(c.src, c.stride, c.w, c.h, c.par, c.dst, c.ostride, c.n, c.look, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render2_look_dev did not happen", k);
        if (mlvfs_amd_render1_look_dev(c.src, c.stride, c.w, c.h, c.par, c.dst, c.ostride, c.n, c.look, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render1_look_dev did not happen", k);
        if (mlvfs_amd_render_scaled_look_dev(c.src, c.stride, c.w, c.h, c.par, 7, 3, c.dst, c.ostride, c.n, c.look, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_scaled_look_dev did not happen", k);
        k++;
    }
    for (int ow = 0; ow <= 17; ow += 17)
        if (mlvfs_amd_render_scaled_look_dev(s, 512, 32, 8, p, ow, 3, d, 1024, 1, lk, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a size outside the geometry", ow);
    if (mlvfs_amd_render1_look_dev(s, 512, 2, 2, p, d, 1024, 1, lk, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a full-size rendering below 4x4", 2);
    if (mlvfs_amd_render2_look_dev(s, 512, 32, 8, p, d, 1024, 0, lk, nullptr) != MLVFS_AMD_OK ||
        mlvfs_amd_render1_look_dev(s, 512, 32, 8, p, d, 1024, 0, lk, nullptr) != MLVFS_AMD_OK ||
        mlvfs_amd_render_scaled_look_dev(s, 512, 32, 8, p, 7, 3, d, 1024, 0, lk, nullptr) != MLVFS_AMD_OK)
        return fail("nothing to do is no error", k);
    // mlvfs_amd_look_apply_dev: 8 triples = 48 bytes in, 24 out
    const uint16_t *t = px.get();
    if (mlvfs_amd_look_apply_dev(nullptr, t, 8, d, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_look_apply_dev(lk, nullptr, 8, d, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look_apply_dev(lk, t, 8, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look_apply_dev(lk, (const uint16_t *)(s + 1), 8, d, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look_apply_dev(lk, t, 8, s, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_look_apply_dev(lk, t, 8, s + 47, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look_apply_dev(lk, (const uint16_t *)(s + 24), 8, s + 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look_apply_dev(lk, t, (size_t)-1, d, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of look_apply_dev did not happen", k);
    if (mlvfs_amd_look_apply_dev(lk, t, 0, d, nullptr) != MLVFS_AMD_OK) return fail("nothing to do is no error", k);
    for (int i = 0; i < 3 * 512; i++) if (s[i] != 7) return fail("a refusal wrote the source", i);
    for (int i = 0; i < 3 * 1024; i++) if (d[i] != 9) return fail("a refusal wrote the destination", i);
    if (mlvfs_amd_mount_set_look(nullptr, lk) != MLVFS_AMD_ERR_ARG || mlvfs_amd_mount_set_look(nullptr, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("mount_set_look took a null handle", k);
    printf("look_host_check: %d records, %d + %d refusals\n", rec, refusals, k);
    return rec > 0 ? 0 : 1;
}
