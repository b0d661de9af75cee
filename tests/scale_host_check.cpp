// scale_host_check.cpp -- a stand-alone host program for tests/test_scale_host.py: the host code of the scaled rendering
// (include/mlvfs_amd.h, "rendered frames at any smaller size") -- mlvfs_amd_rgb_fit, the division and the launch plan behind the test
// hooks, and every argument check of mlvfs_amd_render_scaled_dev and of the mount's scaled calls, which happen before any device work
// and follow no pointer.  It is compiled and linked with -fsanitize=address,undefined against the sanitizer build of the library's
// host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// The file named on the command line: records of {int32 w, h, box_w, box_h, expected return code, expected ow, expected oh} for
// mlvfs_amd_rgb_fit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "scale_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: scale_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        int32_t r[7];
        if (fread(r, sizeof r, 1, f) != 1) break;
        // exactly one int each: a write past either is the sanitizer's to see
        std::unique_ptr<int> ow(new int(-7)), oh(new int(-7));
        if (mlvfs_amd_rgb_fit(r[0], r[1], r[2], r[3], ow.get(), oh.get()) != r[4]) return fail("another return code", rec);
        if (*ow != r[5] || *oh != r[6]) return fail("another size", rec);
        if (r[4] == MLVFS_AMD_OK) {
            // the header the file of that size gets, and the plan of a launch at it
            const size_t hdr = mlvfs_amd_rgb_header_size();
            std::unique_ptr<uint8_t[]> out(new uint8_t[hdr]);
            if (mlvfs_amd_rgb_header(*ow, *oh, out.get(), hdr) != hdr) return fail("no header for a size the fit gives", rec);
            std::unique_ptr<int32_t[]> plan(new int32_t[8]);
            for (int n = 1; n <= 8; n += 7)
                if (mlvfs_amd_test_scale_plan(r[0], r[1], *ow, *oh, n, plan.get()) != MLVFS_AMD_OK || plan[3] < 1 || plan[5] < 1) return fail("no plan for a size the fit gives", rec);
        }
    }
    fclose(f);
    int one = 5;
    if (mlvfs_amd_rgb_fit(64, 48, 10, 10, nullptr, &one) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_fit(64, 48, 10, 10, &one, nullptr) != MLVFS_AMD_ERR_ARG || one != 5)
        return fail("a refusal of rgb_fit did not happen", rec);
    // the division: every shift stays inside its type for the smallest and the largest divisors
    {
        const uint32_t n[4] = { 0u, 1u, 0xFFFFFFFFu, 65535u * 65535u };
        std::unique_ptr<uint32_t[]> q(new uint32_t[4]);
        for (uint32_t d : { 1u, 2u, 3u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFFu }) {
            if (mlvfs_amd_test_scale_div(d, 4, n, q.get()) != MLVFS_AMD_OK) return fail("test_scale_div refused", (int)d);
            for (int k = 0; k < 4; k++) if (q[k] != n[k] / d) return fail("another quotient", (int)d);
        }
        if (mlvfs_amd_test_scale_div(0, 4, n, q.get()) != MLVFS_AMD_ERR_ARG) return fail("a division by 0", 0);
    }
    // mlvfs_amd_render_scaled_dev: a 32 x 8 frame, 512 bytes in, to 7 x 3 = 63 bytes out; the buffers are host memory and exactly that long
    std::unique_ptr<uint16_t[]> px(new uint16_t[3 * 256]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[3 * 64]);
    std::unique_ptr<int32_t[]> par(new int32_t[3 * 13]);
    memset(px.get(), 7, 3 * 512);
    memset(out.get(), 9, 3 * 64);
    memset(par.get(), 0, 3 * 13 * sizeof(int32_t));
    uint8_t *s = (uint8_t *)px.get(), *d = out.get();
    int32_t *p = par.get();
    struct Case { const void *src; size_t stride; int w, h; const int32_t *par; int ow, oh; void *dst; size_t ostride; int n; };
    const Case bad[] = {
        { nullptr, 512, 32, 8, p, 7, 3, d, 64, 1 }, { s, 512, 32, 8, nullptr, 7, 3, d, 64, 1 }, { s, 512, 32, 8, p, 7, 3, nullptr, 64, 1 },
        { s, 512, 1, 8, p, 1, 1, d, 64, 1 }, { s, 512, 32, 1, p, 1, 1, d, 64, 1 }, { s, 512, 0, 0, p, 1, 1, d, 64, 1 }, { s, 512, -32, 8, p, 7, 3, d, 64, 1 },
        { s, 512, 1 << 14, 1 << 13, p, 7, 3, d, 64, 1 }, { s, 512, 1 << 30, 1 << 30, p, 7, 3, d, 64, 1 }, { s, 512, 131072, 2, p, 7, 1, d, 64, 1 },
        { s, 512, 2, 131072, p, 1, 7, d, 64, 1 },
        { s, 512, 32, 8, p, 0, 3, d, 64, 1 }, { s, 512, 32, 8, p, 7, 0, d, 64, 1 }, { s, 512, 32, 8, p, -7, 3, d, 64, 1 }, { s, 512, 32, 8, p, 17, 3, d, 64, 1 },
        { s, 512, 32, 8, p, 7, 5, d, 64, 1 }, { s, 512, 32, 8, p, 1 << 30, 1 << 30, d, 64, 1 }, { s, 512, 32, 8, p, 7, 3, d, 64, -1 },
        { s, 510, 32, 8, p, 7, 3, d, 64, 2 }, { s, 512, 32, 8, p, 7, 3, d, 62, 2 }, { s, 513, 32, 8, p, 7, 3, d, 64, 2 }, { s + 1, 512, 32, 8, p, 7, 3, d, 64, 1 },
        { s, 512, 32, 8, (const int32_t *)((const uint8_t *)p + 2), 7, 3, d, 64, 1 },
        { s, 512, 32, 8, p, 7, 3, s, 64, 1 }, { s, 512, 32, 8, p, 7, 3, s + 511, 64, 1 }, { s + 64, 512, 32, 8, p, 7, 3, s + 2, 64, 1 },
        { s, 512, 32, 8, p, 7, 3, s + 1535, 64, 3 }, { s, 512, 32, 8, p, 7, 3, p, 64, 1 }, { s, 512, 32, 8, p, 7, 3, (uint8_t *)p + 51, 64, 1 },
        { s, 512, 32, 8, p, 7, 3, (uint8_t *)p + 2 * 52 + 51, 64, 3 },
    };
    int k = 0;
    for (const Case &c : bad) {
        if (mlvfs_amd_render_scaled_dev(c.src, c.stride, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.ostride, c.n, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_scaled_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_render_scaled_dev(s, 512, 32, 8, p, 7, 3, d, 64, 0, nullptr) != MLVFS_AMD_OK) return fail("nothing to do is no error", k);
    for (int i = 0; i < 3 * 512; i++) if (s[i] != 7) return fail("a refusal wrote the source", i);
    for (int i = 0; i < 3 * 64; i++) if (d[i] != 9) return fail("a refusal wrote the destination", i);
    // the mount's calls follow no null handle
    if (mlvfs_amd_mount_rgb_scaled_size(nullptr, 0, 7, 3) != 0) return fail("mount_rgb_scaled_size of a null handle", k);
    uint8_t byte = 0xA5;
    size_t sz = 7;
    int fl = 7;
    if (mlvfs_amd_mount_rgb_scaled(nullptr, 0, 1, &byte, 1, 256, 7, 3, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_jpeg_scaled(nullptr, 0, 1, &byte, 1, 256, 90, 7, 3, &sz, &fl, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG || byte != 0xA5 || sz != 7 || fl != 7)
        return fail("a scaled mount call took a null handle", k);
    printf("scale_host_check: %d records, %d refusals\n", rec, k);
    return rec > 0 ? 0 : 1;
}
