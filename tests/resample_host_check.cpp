// resample_host_check.cpp -- a stand-alone host program for tests/test_resample_host.py: the host code of the resampled rendering
// (include/mlvfs_amd.h, "rendered frames resampled from the full-size rendering") -- mlvfs_amd_rgb_fit_full, the launch plan behind the
// test hook, and every argument check of mlvfs_amd_render_resampled_dev, its look and deep forms and the mount's resampled calls, which
// happen before any device work and follow no pointer.  It is compiled and linked with -fsanitize=address,undefined against the
// sanitizer build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime,
// no HIP device.
//
// The file named on the command line: records of {int32 w, h, box_w, box_h, expected return code, expected ow, expected oh} for
// mlvfs_amd_rgb_fit_full.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "resample_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: resample_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        int32_t r[7];
        if (fread(r, sizeof r, 1, f) != 1) break;
        // exactly one int each: a write past either is the sanitizer's to see
        std::unique_ptr<int> ow(new int(-7)), oh(new int(-7));
        if (mlvfs_amd_rgb_fit_full(r[0], r[1], r[2], r[3], ow.get(), oh.get()) != r[4]) return fail("another return code", rec);
        if (*ow != r[5] || *oh != r[6]) return fail("another size", rec);
        if (r[4] == MLVFS_AMD_OK) {
            // the header the file of that size gets, and the plan of a launch at it
            const size_t hdr = mlvfs_amd_rgb_header_size();
            std::unique_ptr<uint8_t[]> out(new uint8_t[hdr]);
            if (mlvfs_amd_rgb_header(*ow, *oh, out.get(), hdr) != hdr || mlvfs_amd_rgb16_header(*ow, *oh, out.get(), hdr) != hdr)
                return fail("no header for a size the fit gives", rec);
            std::unique_ptr<int32_t[]> plan(new int32_t[8]);
            for (int n = 1; n <= 8; n += 7) {
                if (mlvfs_amd_test_resample_plan(r[0], r[1], *ow, *oh, n, plan.get()) != MLVFS_AMD_OK) return fail("no plan for a size the fit gives", rec);
                const bool fast = r[0] % 16 == 0 && 2 * (int64_t)*ow >= r[0];
                if (plan[0] != (fast ? 1 : 0) || (fast && (plan[2] < 1 || plan[2] > plan[1] - 16 || plan[4] < 1 || (int64_t)plan[2] * plan[3] < *ow ||
                                                           (int64_t)plan[4] * plan[5] < *oh)))
                    return fail("a plan that does not cover the size", rec);
            }
        }
    }
    fclose(f);
    int one = 5;
    if (mlvfs_amd_rgb_fit_full(64, 48, 10, 10, nullptr, &one) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_fit_full(64, 48, 10, 10, &one, nullptr) != MLVFS_AMD_ERR_ARG || one != 5)
        return fail("a refusal of rgb_fit_full did not happen", rec);
    {
        std::unique_ptr<int32_t[]> plan(new int32_t[8]);
        const int bad[][5] = { { 3, 8, 1, 1, 1 }, { 32, 8, 33, 8, 1 }, { 32, 8, 32, 9, 1 }, { 32, 8, 0, 1, 1 }, { 65536, 4, 1, 1, 1 }, { 8192, 4096, 1, 1, 1 }, { 32, 8, 4, 4, 0 } };
        for (const auto &b : bad)
            if (mlvfs_amd_test_resample_plan(b[0], b[1], b[2], b[3], b[4], plan.get()) != MLVFS_AMD_ERR_ARG) return fail("a plan for what the route refuses", b[0]);
        if (mlvfs_amd_test_resample_plan(32, 8, 4, 4, 1, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a plan into a null pointer", 0);
        // the widest and the tallest frames: the plan's products stay inside their types
        if (mlvfs_amd_test_resample_plan(65520, 4, 65520, 4, 1, plan.get()) != MLVFS_AMD_OK || plan[0] != 1 || plan[3] != 133) return fail("the widest fast frame", 0);
        if (mlvfs_amd_test_resample_plan(16, 65535, 16, 65535, 8, plan.get()) != MLVFS_AMD_OK || plan[0] != 1) return fail("the tallest frame", 0);
    }
    // mlvfs_amd_render_resampled_dev: a 32 x 8 frame, 512 bytes in, to 20 x 5 = 300 bytes out (600 in the deep form); the buffers are host
    // memory and exactly that long
    std::unique_ptr<uint16_t[]> px(new uint16_t[3 * 256]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[3 * 608]);
    std::unique_ptr<int32_t[]> par(new int32_t[3 * 13]);
    memset(px.get(), 7, 3 * 512);
    memset(out.get(), 9, 3 * 608);
    memset(par.get(), 0, 3 * 13 * sizeof(int32_t));
    uint8_t *s = (uint8_t *)px.get(), *d = out.get();
    int32_t *p = par.get();
    struct Case { const void *src; size_t stride; int w, h; const int32_t *par; int ow, oh; void *dst; size_t ostride; int n; };
    const Case bad[] = {
        { nullptr, 512, 32, 8, p, 20, 5, d, 608, 1 }, { s, 512, 32, 8, nullptr, 20, 5, d, 608, 1 }, { s, 512, 32, 8, p, 20, 5, nullptr, 608, 1 },
        { s, 512, 3, 8, p, 1, 1, d, 608, 1 }, { s, 512, 32, 3, p, 1, 1, d, 608, 1 }, { s, 512, 0, 0, p, 1, 1, d, 608, 1 }, { s, 512, -32, 8, p, 20, 5, d, 608, 1 },
        { s, 512, 1 << 13, 1 << 12, p, 20, 5, d, 608, 1 }, { s, 512, 1 << 30, 1 << 30, p, 20, 5, d, 608, 1 }, { s, 512, 65536, 4, p, 20, 1, d, 608, 1 },
        { s, 512, 4, 65536, p, 1, 5, d, 608, 1 },
        { s, 512, 32, 8, p, 0, 5, d, 608, 1 }, { s, 512, 32, 8, p, 20, 0, d, 608, 1 }, { s, 512, 32, 8, p, -20, 5, d, 608, 1 }, { s, 512, 32, 8, p, 33, 5, d, 608, 1 },
        { s, 512, 32, 8, p, 20, 9, d, 608, 1 }, { s, 512, 32, 8, p, 1 << 30, 1 << 30, d, 608, 1 }, { s, 512, 32, 8, p, 20, 5, d, 608, -1 },
        { s, 510, 32, 8, p, 20, 5, d, 608, 2 }, { s, 512, 32, 8, p, 20, 5, d, 298, 2 }, { s, 513, 32, 8, p, 20, 5, d, 608, 2 }, { s + 1, 512, 32, 8, p, 20, 5, d, 608, 1 },
        { s, 512, 32, 8, (const int32_t *)((const uint8_t *)p + 2), 20, 5, d, 608, 1 },
        { s, 512, 32, 8, p, 20, 5, s, 608, 1 }, { s, 512, 32, 8, p, 20, 5, s + 511, 608, 1 }, { s + 512, 512, 32, 8, p, 20, 5, s + 213, 608, 1 },
        { s, 512, 32, 8, p, 20, 5, s + 1535, 608, 3 }, { s, 512, 32, 8, p, 20, 5, p, 608, 1 }, { s, 512, 32, 8, p, 20, 5, (uint8_t *)p + 51, 608, 1 },
        { s, 512, 32, 8, p, 20, 5, (uint8_t *)p + 2 * 52 + 51, 608, 3 },
    };
    // any non-null pointer stands for a look: the checks that refuse these calls come before a look is read
    const mlvfs_amd_look_t *lk = (const mlvfs_amd_look_t *)d;
    const mlvfs_amd_look16_t *lk16 = (const mlvfs_amd_look16_t *)d;
    int k = 0;
    for (const Case &c : bad) {
        if (mlvfs_amd_render_resampled_dev(c.src, c.stride, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.ostride, c.n, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_resampled_dev did not happen", k);
        if (mlvfs_amd_render_resampled_look_dev(c.src, c.stride, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.ostride, c.n, lk, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_resampled_look_dev did not happen", k);
        if (mlvfs_amd_render_resampled_deep_dev(c.src, c.stride, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.ostride, c.n, lk16, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_resampled_deep_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_render_resampled_look_dev(s, 512, 32, 8, p, 20, 5, d, 608, 1, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render_resampled_deep_dev(s, 512, 32, 8, p, 20, 5, d, 608, 1, nullptr, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a null look", k);
    if (mlvfs_amd_render_resampled_deep_dev(s, 512, 32, 8, p, 20, 5, d, 599, 2, lk16, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a deep stride of 599", k);
    if (mlvfs_amd_render_resampled_dev(s, 512, 32, 8, p, 20, 5, d, 608, 0, nullptr) != MLVFS_AMD_OK ||
        mlvfs_amd_render_resampled_look_dev(s, 512, 32, 8, p, 20, 5, d, 608, 0, lk, nullptr) != MLVFS_AMD_OK ||
        mlvfs_amd_render_resampled_deep_dev(s, 512, 32, 8, p, 20, 5, d, 608, 0, lk16, nullptr) != MLVFS_AMD_OK)
        return fail("nothing to do is no error", k);
    for (int i = 0; i < 3 * 512; i++) if (s[i] != 7) return fail("a refusal wrote the source", i);
    for (int i = 0; i < 3 * 608; i++) if (d[i] != 9) return fail("a refusal wrote the destination", i);
    // the mount's calls follow no null handle
    if (mlvfs_amd_mount_rgb_resampled_size(nullptr, 0, 20, 5) != 0 || mlvfs_amd_mount_rgb16_resampled_size(nullptr, 0, 20, 5) != 0)
        return fail("a size call took a null handle", k);
    uint8_t byte = 0xA5;
    size_t sz = 7;
    int fl = 7;
    if (mlvfs_amd_mount_rgb_resampled(nullptr, 0, 1, &byte, 1, 256, 20, 5, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_jpeg_resampled(nullptr, 0, 1, &byte, 1, 256, 90, 20, 5, &sz, &fl, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_rgb16_resampled(nullptr, 0, 1, &byte, 1, 256, 20, 5, lk16, 1, 1, nullptr) != MLVFS_AMD_ERR_ARG || byte != 0xA5 || sz != 7 || fl != 7)
        return fail("a resampled mount call took a null handle", k);
    printf("resample_host_check: %d records, %d refusals\n", rec, k);
    return rec > 0 ? 0 : 1;
}
