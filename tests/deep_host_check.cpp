// deep_host_check.cpp -- a stand-alone host program for tests/test_deep_host.py: the host code of the 16-bit routes (include/mlvfs_amd.h,
// "rendered frames at 16 bits") -- mlvfs_amd_look16_image_size and mlvfs_amd_look16_pack against images computed in Python, with buffers
// of exactly the sizes they may touch (no table at all where n = 0), every refusal with the image untouched, mlvfs_amd_rgb16_header
// against mlvfs_amd_rgb_header, and the argument checks of the three _deep_dev calls, of mlvfs_amd_look16_apply_dev and of the mount's
// 16-bit calls, which happen before any device work and follow no pointer.  It is compiled and linked with
// -fsanitize=address,undefined against the sanitizer build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run
// directly: no Python, no preloaded runtime, no HIP device.
//
// The file named on the command line: records of {int32 n, uint16 S16[65536], uint16 T[3 n^3], the expected image of 131072 + 8 n^3 bytes}.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "deep_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: deep_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0, refusals = 0;
    for (;; rec++) {
        int32_t n;
        if (fread(&n, sizeof n, 1, f) != 1) break;
        const size_t entries = (size_t)n * n * n, size = 131072 + 8 * entries;
        if (mlvfs_amd_look16_image_size(n) != size) return fail("another image size", rec);
        // exactly as long as what may be read and written: a step past any of them is the sanitizer's to see
        std::unique_ptr<uint16_t[]> S(new uint16_t[65536]), T(entries ? new uint16_t[3 * entries] : nullptr);
        std::unique_ptr<uint8_t[]> want(new uint8_t[size]), got(new uint8_t[size]);
        if (fread(S.get(), 2, 65536, f) != 65536 || (entries && fread(T.get(), 2, 3 * entries, f) != 3 * entries) || fread(want.get(), 1, size, f) != size)
            return fail("a short record", rec);
        memset(got.get(), 0xA5, size);
        if (mlvfs_amd_look16_pack(S.get(), n, T.get(), got.get(), size) != MLVFS_AMD_OK) return fail("look16_pack refused", rec);
        if (memcmp(got.get(), want.get(), size)) return fail("another image", rec);
        // every refusal leaves the image as it was
        memset(got.get(), 0xA5, size);
        const int rcs[] = { mlvfs_amd_look16_pack(nullptr, n, T.get(), got.get(), size), mlvfs_amd_look16_pack(S.get(), n ? n : 2, nullptr, got.get(), size + 64),
                            mlvfs_amd_look16_pack(S.get(), n, T.get(), nullptr, size), mlvfs_amd_look16_pack(S.get(), n, T.get(), got.get(), size - 1),
                            mlvfs_amd_look16_pack(S.get(), n, T.get(), got.get(), 0), mlvfs_amd_look16_pack(S.get(), 1, T.get(), got.get(), size),
                            mlvfs_amd_look16_pack(S.get(), 66, T.get(), got.get(), size), mlvfs_amd_look16_pack(S.get(), -3, T.get(), got.get(), size),
                            mlvfs_amd_look16_pack(S.get(), 1 << 30, T.get(), got.get(), size) };
        for (int rc : rcs) {
            if (rc != MLVFS_AMD_ERR_ARG) return fail("a refusal of look16_pack did not happen", rec);
            refusals++;
        }
        for (size_t i = 0; i < size; i++) if (got[i] != 0xA5) return fail("a refusal wrote the image", rec);
        if (mlvfs_amd_look16_create(nullptr, n, T.get()) || mlvfs_amd_look16_create(S.get(), 2, nullptr) || mlvfs_amd_look16_create(S.get(), 1, T.get()) ||
            mlvfs_amd_look16_create(S.get(), 66, T.get()))
            return fail("look16_create took what it must refuse", rec);
    }
    fclose(f);
    for (int n : { -1, 1, 66, 1 << 20, (int)0x80000000 })
        if (mlvfs_amd_look16_image_size(n) != 0) return fail("an image size for a table that is none", n);
    if (mlvfs_amd_look16_image_size(0) != 131072 || mlvfs_amd_look16_image_size(2) != 131072 + 64 || mlvfs_amd_look16_image_size(65) != 131072 + 8 * 274625)
        return fail("another image size", 65);
    mlvfs_amd_look16_destroy(nullptr);

    // the header: the 8-bit header's bytes but for BitsPerSample (158, 160, 162) and StripByteCounts (126 .. 129)
    {
        std::unique_ptr<uint8_t[]> h8(new uint8_t[256]), h16(new uint8_t[256]);
        memset(h16.get(), 0xA5, 256);
        if (mlvfs_amd_rgb16_header(0, 5, h16.get(), 256) || mlvfs_amd_rgb16_header(7, 5, nullptr, 256) || mlvfs_amd_rgb16_header(7, 5, h16.get(), 255) ||
            mlvfs_amd_rgb16_header(1 << 13, 1 << 12, h16.get(), 256))
            return fail("rgb16_header took what it must refuse", 0);
        for (int i = 0; i < 256; i++) if (h16[i] != 0xA5) return fail("a refusal wrote the header", i);
        if (mlvfs_amd_rgb_header(1792, 660, h8.get(), 256) != 256 || mlvfs_amd_rgb16_header(1792, 660, h16.get(), 256) != 256) return fail("no header", 0);
        for (int i = 0; i < 256; i++) {
            const bool may = i == 158 || i == 160 || i == 162 || (i >= 126 && i < 130);
            if (!may && h8[i] != h16[i]) return fail("the 16-bit header differs where it must not", i);
        }
        uint32_t count;
        memcpy(&count, h16.get() + 126, 4);
        if (count != 6u * 1792 * 660 || h16[158] != 16 || h16[160] != 16 || h16[162] != 16 || h16[159] || h16[161] || h16[163]) return fail("the 16-bit header's own fields", 0);
    }

    // the three _deep_dev calls: a 32 x 8 frame, 512 bytes in; the buffers are host memory; `look` is never followed by a check
    std::unique_ptr<uint16_t[]> px(new uint16_t[3 * 256]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[3 * 2048]);
    std::unique_ptr<int32_t[]> par(new int32_t[3 * 13]);
    memset(px.get(), 7, 3 * 512);
    memset(out.get(), 9, 3 * 2048);
    memset(par.get(), 0, 3 * 13 * sizeof(int32_t));
    uint8_t *s = (uint8_t *)px.get(), *d = out.get();
    int32_t *p = par.get();
    const mlvfs_amd_look16_t *lk = (const mlvfs_amd_look16_t *)(const void *)out.get();      // any non-null address: no check reads it
    struct Case { const void *src; size_t stride; int w, h; const int32_t *par; void *dst; size_t ostride; int n; const mlvfs_amd_look16_t *look; };
    const Case bad[] = {
        { s, 512, 32, 8, p, d, 2048, 1, nullptr }, { nullptr, 512, 32, 8, p, d, 2048, 1, lk }, { s, 512, 32, 8, nullptr, d, 2048, 1, lk },
        { s, 512, 32, 8, p, nullptr, 2048, 1, lk }, { s, 512, 1, 8, p, d, 2048, 1, lk }, { s, 512, 32, 1, p, d, 2048, 1, lk },
        { s, 512, 1 << 14, 1 << 13, p, d, 2048, 1, lk }, { s, 512, -32, 8, p, d, 2048, 1, lk }, { s, 512, 32, 8, p, d, 2048, -1, lk },
        { s, 510, 32, 8, p, d, 2048, 2, lk }, { s, 512, 32, 8, p, d, 100, 2, lk }, { s, 513, 32, 8, p, d, 2048, 2, lk }, { s + 1, 512, 32, 8, p, d, 2048, 1, lk },
        { s, 512, 32, 8, (const int32_t *)((const uint8_t *)p + 2), d, 2048, 1, lk }, { s, 512, 32, 8, p, s, 2048, 1, lk }, { s, 512, 32, 8, p, s + 511, 2048, 1, lk },
        { s, 512, 32, 8, p, p, 2048, 1, lk }, { s, 512, 32, 8, p, (uint8_t *)p + 51, 2048, 1, lk },
    };
    int k = 0;
    for (const Case &c : bad) {
        if (mlvfs_amd_render2_deep_dev(c.src, c.stride, c.w, c.h, c.par, c.dst, c.ostride, c.n, c.look, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render2_deep_dev did not happen", k);
        if (mlvfs_amd_render1_deep_dev(c.src, c.stride, c.w, c.h, c.par, c.dst, c.ostride, c.n, c.look, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render1_deep_dev did not happen", k);
        if (mlvfs_amd_render_scaled_deep_dev(c.src, c.stride, c.w, c.h, c.par, 7, 3, c.dst, c.ostride, c.n, c.look, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_scaled_deep_dev did not happen", k);
        k++;
    }
    // 6 bytes per pixel in the stride checks: one byte short of a rendering, which would hold two 8-bit ones
    if (mlvfs_amd_render2_deep_dev(s, 512, 32, 8, p, d, 383, 2, lk, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render1_deep_dev(s, 512, 32, 8, p, d, 1535, 2, lk, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render_scaled_deep_dev(s, 512, 32, 8, p, 7, 3, d, 125, 2, lk, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a stride one byte short of a 16-bit rendering", k);
    for (int ow = 0; ow <= 17; ow += 17)
        if (mlvfs_amd_render_scaled_deep_dev(s, 512, 32, 8, p, ow, 3, d, 2048, 1, lk, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a size outside the geometry", ow);
    if (mlvfs_amd_render1_deep_dev(s, 512, 2, 2, p, d, 2048, 1, lk, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a full-size rendering below 4x4", 2);
    if (mlvfs_amd_render2_deep_dev(s, 512, 32, 8, p, d, 2048, 0, lk, nullptr) != MLVFS_AMD_OK ||
        mlvfs_amd_render1_deep_dev(s, 512, 32, 8, p, d, 2048, 0, lk, nullptr) != MLVFS_AMD_OK ||
        mlvfs_amd_render_scaled_deep_dev(s, 512, 32, 8, p, 7, 3, d, 2048, 0, lk, nullptr) != MLVFS_AMD_OK)
        return fail("nothing to do is no error", k);
    // mlvfs_amd_look16_apply_dev: 8 triples = 48 bytes in, 48 out
    const uint16_t *t = px.get();
    uint16_t *o = (uint16_t *)d;
    if (mlvfs_amd_look16_apply_dev(nullptr, t, 8, o, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_look16_apply_dev(lk, nullptr, 8, o, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, t, 8, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, (const uint16_t *)(s + 1), 8, o, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, t, 8, (uint16_t *)(d + 1), nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, t, 8, (uint16_t *)s, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, t, 8, (uint16_t *)(s + 46), nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, (const uint16_t *)(s + 46), 8, (uint16_t *)s, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_look16_apply_dev(lk, t, (size_t)-1, o, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of look16_apply_dev did not happen", k);
    if (mlvfs_amd_look16_apply_dev(lk, t, 0, o, nullptr) != MLVFS_AMD_OK) return fail("nothing to do is no error", k);
    // the mount's calls: a null deep look, a null handle, a gain or a size that is none -- before the handle is followed (it is no handle)
    void *m = out.get();
    int res[2] = { 5, 5 };
    if (mlvfs_amd_mount_rgb16(m, 0, 1, d, 2048, 256, nullptr, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_full(m, 0, 1, d, 2048, 256, nullptr, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_scaled(m, 0, 1, d, 2048, 256, 7, 3, nullptr, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16(nullptr, 0, 1, d, 2048, 256, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_full(nullptr, 0, 1, d, 2048, 256, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_scaled(nullptr, 0, 1, d, 2048, 256, 7, 3, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16(m, 0, 1, d, 2048, 0, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_full(m, 0, 1, d, 2048, 65536, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_scaled(m, 0, 1, d, 2048, 256, 0, 3, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_scaled(m, 0, 1, d, 2048, 256, 7, -1, lk, 2, 0, res) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of a mount call did not happen", k);
    if (mlvfs_amd_mount_rgb16_size(nullptr, 0) || mlvfs_amd_mount_rgb16_full_size(nullptr, 0) || mlvfs_amd_mount_rgb16_scaled_size(nullptr, 0, 7, 3))
        return fail("a size from a null handle", k);
    for (int i = 0; i < 3 * 512; i++) if (s[i] != 7) return fail("a refusal wrote the source", i);
    for (int i = 0; i < 3 * 2048; i++) if (d[i] != 9) return fail("a refusal wrote the destination", i);
    if (res[0] != 5 || res[1] != 5) return fail("a refusal wrote results[]", 0);
    printf("deep_host_check: %d records, %d + %d refusals\n", rec, refusals, k);
    return rec > 0 ? 0 : 1;
}
