// demosaic_host_check.cpp -- a stand-alone host program for tests/test_demosaic_host.py: the host code of the full-size rendering
// (include/mlvfs_amd.h, "rendered full-size sRGB frames") -- the geometry, the file's sizes and every argument check of
// mlvfs_amd_render1_dev, which happen before any device work and follow no pointer.  It is compiled and linked with
// -fsanitize=address,undefined against the sanitizer build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run
// directly: no Python, no preloaded runtime, no HIP device.
//
// The file named on the command line: records of {int32 w, h, expected return code, expected pw, expected ph} for mlvfs_amd_rgb_full_geom.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "demosaic_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: demosaic_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        int32_t r[5];
        if (fread(r, sizeof r, 1, f) != 1) break;
        // exactly one int each: a write past either is the sanitizer's to see
        std::unique_ptr<int> pw(new int(-7)), ph(new int(-7));
        if (mlvfs_amd_rgb_full_geom(r[0], r[1], pw.get(), ph.get()) != r[2]) return fail("another return code", rec);
        if (*pw != r[3] || *ph != r[4]) return fail("another geometry", rec);
        // the header the file of that size gets: mlvfs_amd_rgb_header takes every size the geometry takes
        if (r[2] == MLVFS_AMD_OK) {
            const size_t hdr = mlvfs_amd_rgb_header_size();
            std::unique_ptr<uint8_t[]> out(new uint8_t[hdr]);
            if (mlvfs_amd_rgb_header(*pw, *ph, out.get(), hdr) != hdr) return fail("no header for a size the geometry takes", rec);
        }
    }
    fclose(f);
    int one = 5;
    if (mlvfs_amd_rgb_full_geom(16, 16, nullptr, &one) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_full_geom(16, 16, &one, nullptr) != MLVFS_AMD_ERR_ARG || one != 5)
        return fail("a refusal of rgb_full_geom did not happen", rec);
    // mlvfs_amd_render1_dev: a 16 x 8 frame, 256 bytes in, 384 out; the buffers are host memory and exactly that long
    std::unique_ptr<uint16_t[]> px(new uint16_t[3 * 128]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[3 * 384]);
    std::unique_ptr<int32_t[]> par(new int32_t[3 * 13]);
    memset(px.get(), 7, 3 * 256);
    memset(out.get(), 9, 3 * 384);
    memset(par.get(), 0, 3 * 13 * sizeof(int32_t));
    uint8_t *s = (uint8_t *)px.get(), *d = out.get();
    int32_t *p = par.get();
    struct Case { const void *src; size_t stride; int w, h; const int32_t *par; void *dst; size_t ostride; int n; };
    const Case bad[] = {
        { nullptr, 256, 16, 8, p, d, 384, 1 }, { s, 256, 16, 8, nullptr, d, 384, 1 }, { s, 256, 16, 8, p, nullptr, 384, 1 },
        { s, 256, 3, 8, p, d, 384, 1 }, { s, 256, 16, 3, p, d, 384, 1 }, { s, 256, 0, 0, p, d, 384, 1 }, { s, 256, -16, 8, p, d, 384, 1 },
        { s, 256, 1 << 13, 1 << 12, p, d, 384, 1 }, { s, 256, 1 << 30, 1 << 30, p, d, 384, 1 }, { s, 256, 16, 8, p, d, 384, -1 },
        { s, 254, 16, 8, p, d, 384, 2 }, { s, 256, 16, 8, p, d, 383, 2 }, { s, 257, 16, 8, p, d, 384, 2 }, { s + 1, 256, 16, 8, p, d, 384, 1 },
        { s, 256, 16, 8, (const int32_t *)((const uint8_t *)p + 2), d, 384, 1 },
        { s, 256, 16, 8, p, s, 384, 1 }, { s, 256, 16, 8, p, s + 255, 384, 1 }, { s + 384, 256, 16, 8, p, s + 1, 384, 1 },
        { s, 256, 16, 8, p, s + 767, 384, 3 }, { s, 256, 16, 8, p, p, 384, 1 }, { s, 256, 16, 8, p, (uint8_t *)p + 51, 384, 1 },
        { s, 256, 16, 8, p, (uint8_t *)p + 2 * 52 + 51, 384, 3 },
    };
    int k = 0;
    for (const Case &c : bad) {
        if (mlvfs_amd_render1_dev(c.src, c.stride, c.w, c.h, c.par, c.dst, c.ostride, c.n, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a refusal of render1_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_render1_dev(s, 256, 16, 8, p, d, 384, 0, nullptr) != MLVFS_AMD_OK) return fail("nothing to do is no error", k);
    for (int i = 0; i < 3 * 256; i++) if (s[i] != 7) return fail("a refusal wrote the source", i);
    for (int i = 0; i < 3 * 384; i++) if (d[i] != 9) return fail("a refusal wrote the destination", i);
    // the mount's size call follows no null handle
    if (mlvfs_amd_mount_rgb_full_size(nullptr, 0) != 0) return fail("mount_rgb_full_size of a null handle", k);
    uint8_t byte = 0xA5;
    size_t sz = 7;
    int fl = 7;
    if (mlvfs_amd_mount_rgb_full(nullptr, 0, 1, &byte, 1, 256, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_jpeg_full(nullptr, 0, 1, &byte, 1, 256, 90, &sz, &fl, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG || byte != 0xA5 || sz != 7 || fl != 7)
        return fail("a full-size mount call took a null handle", k);
    printf("demosaic_host_check: %d records, %d refusals\n", rec, k);
    return rec > 0 ? 0 : 1;
}
