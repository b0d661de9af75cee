// amaze_resample_host_check.cpp -- a stand-alone host program for tests/test_amaze_resample_host.py: the host code of the resampled AMaZE
// rendering (include/mlvfs_amd.h, "resampled rendered frames demosaiced by AMaZE") -- the geometry, the plan of the fast form and every
// argument check of mlvfs_amd_amaze_resample_dev and the three mlvfs_amd_render_resampled_amaze calls, which happen before any device
// work and follow no pointer.  It is compiled and linked with -fsanitize=address,undefined against the sanitizer build of the library's
// host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// GEOM.bin: records of {int32 w, h, ow, oh, expected return code} for mlvfs_amd_rgb_amaze_resample_geom.
// PLAN.bin: records of {int32 w, h, ow, oh, nframes, expected return code, expected out[0 .. 7]} for mlvfs_amd_test_amz_resample_plan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "amaze_resample_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: amaze_resample_host_check GEOM.bin PLAN.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        int32_t r[5];
        if (fread(r, sizeof r, 1, f) != 1) break;
        if (mlvfs_amd_rgb_amaze_resample_geom(r[0], r[1], r[2], r[3]) != r[4]) return fail("another return code", rec);
    }
    fclose(f);

    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    int plans = 0;
    for (;; plans++) {
        int32_t r[14];
        if (fread(r, sizeof r, 1, f) != 1) break;
        std::unique_ptr<int32_t[]> out(new int32_t[8]);              // exactly eight: a write past them is the sanitizer's to see
        for (int i = 0; i < 8; i++) out[i] = -7;
        if (mlvfs_amd_test_amz_resample_plan(r[0], r[1], r[2], r[3], r[4], out.get()) != r[5]) return fail("plan: another return code", plans);
        for (int i = 0; i < 8; i++) if (out[i] != r[6 + i]) return fail("plan: another number", plans);
    }
    fclose(f);
    if (mlvfs_amd_test_amz_resample_plan(64, 64, 40, 40, 1, nullptr) != MLVFS_AMD_ERR_ARG) return fail("plan: a null pointer", plans);

    // a 48 x 36 frame to 30 x 20: 3456 bytes in, 1728 floats a plane, 1800 bytes out (3600 at 16 bits); host memory, exactly that long,
    // for three frames
    const int W = 48, H = 36, OW = 30, OH = 20;
    const size_t IMG = 3456, NP = 1728, OUT = 1800;
    std::unique_ptr<uint16_t[]> px(new uint16_t[3 * NP]);
    std::unique_ptr<float[]> planes(new float[3 * 3 * NP]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[3 * 2 * OUT]);
    std::unique_ptr<int32_t[]> par(new int32_t[3 * 13]);
    memset(px.get(), 7, 3 * IMG);
    memset(planes.get(), 5, 9 * NP * sizeof(float));
    memset(out.get(), 9, 6 * OUT);
    memset(par.get(), 0, 3 * 13 * sizeof(int32_t));
    uint8_t *s = (uint8_t *)px.get(), *d = out.get();
    float *q = planes.get(), *qr = q, *qg = q + 3 * NP, *qb = q + 6 * NP;
    int32_t *p = par.get();
    const int32_t *p2 = (const int32_t *)((const uint8_t *)p + 2);
    int one = 5, k = 0;
    const mlvfs_amd_look_t *lk = (const mlvfs_amd_look_t *)&one;        // never followed: both set is refused first
    const mlvfs_amd_look16_t *lk16 = (const mlvfs_amd_look16_t *)&one;

    struct T { const float *r, *g, *b; size_t ps; int w, h; const int32_t *par; int ow, oh; void *dst; size_t os; int n; const mlvfs_amd_look_t *l; const mlvfs_amd_look16_t *l16; };
    const T bad_t[] = {
        { nullptr, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1, nullptr, nullptr }, { qr, nullptr, qb, NP, W, H, p, OW, OH, d, OUT, 1, nullptr, nullptr },
        { qr, qg, nullptr, NP, W, H, p, OW, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, nullptr, OW, OH, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, OW, OH, nullptr, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1, lk, lk16 },
        { qr, qg, qb, NP, 34, H, p, OW, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, 35, p, OW, OH, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, 50, H, p, OW, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, 1 << 13, 1 << 12, p, OW, OH, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, 36, 65536, p, OW, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, 1 << 30, 1 << 30, p, OW, OH, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, 0, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, OW, 0, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, W + 1, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, OW, H + 1, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, -1, -1, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, 1 << 30, 1 << 30, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, -1, nullptr, nullptr }, { qr, qg, qb, NP - 1, W, H, p, OW, OH, d, OUT, 2, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, OW, OH, d, OUT - 1, 2, nullptr, nullptr }, { (const float *)((const uint8_t *)qr + 2), qg, qb, NP, W, H, p, OW, OH, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p2, OW, OH, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, OW, OH, qr, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, OW, OH, (uint8_t *)qg + 100, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, OW, OH, (uint8_t *)(qb + NP) - 1, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, OW, OH, p, OUT, 1, nullptr, nullptr },
    };
    for (const T &c : bad_t) {
        if (mlvfs_amd_amaze_resample_dev(c.r, c.g, c.b, c.ps, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.os, c.n, c.l, c.l16, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of amaze_resample_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_amaze_resample_dev(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, 0, nullptr, nullptr, nullptr) != MLVFS_AMD_OK) return fail("resample: nothing to do is no error", k);

    struct R { const void *src; size_t stride; int w, h; const int32_t *par; int ow, oh; void *dst; size_t os; int n; };
    const R bad_r[] = {
        { nullptr, IMG, W, H, p, OW, OH, d, OUT, 1 }, { s, IMG, W, H, nullptr, OW, OH, d, OUT, 1 }, { s, IMG, W, H, p, OW, OH, nullptr, OUT, 1 },
        { s, IMG, 34, H, p, OW, OH, d, OUT, 1 }, { s, IMG, W, 35, p, OW, OH, d, OUT, 1 }, { s, IMG, 46, H, p, OW, OH, d, OUT, 1 }, { s, IMG, 16, 8, p, 8, 8, d, OUT, 1 },
        { s, IMG, 1 << 13, 1 << 12, p, OW, OH, d, OUT, 1 }, { s, IMG, 1 << 30, 1 << 30, p, OW, OH, d, OUT, 1 }, { s, IMG, 36, 65536, p, OW, OH, d, OUT, 1 },
        { s, IMG, W, H, p, 0, OH, d, OUT, 1 }, { s, IMG, W, H, p, OW, 0, d, OUT, 1 }, { s, IMG, W, H, p, W + 1, OH, d, OUT, 1 }, { s, IMG, W, H, p, OW, H + 1, d, OUT, 1 },
        { s, IMG, W, H, p, OW, OH, d, OUT, -1 }, { s, IMG - 2, W, H, p, OW, OH, d, OUT, 2 }, { s, IMG, W, H, p, OW, OH, d, OUT - 1, 2 },
        { s, IMG + 1, W, H, p, OW, OH, d, OUT, 2 }, { s + 1, IMG, W, H, p, OW, OH, d, OUT, 1 }, { s, IMG, W, H, p2, OW, OH, d, OUT, 1 },
        { s, IMG, W, H, p, OW, OH, s, OUT, 1 }, { s, IMG, W, H, p, OW, OH, s + IMG - 1, OUT, 1 }, { d + OUT - 1, IMG, W, H, p, OW, OH, d, OUT, 1 },
        { s, IMG, W, H, p, OW, OH, p, OUT, 1 },
    };
    for (const R &c : bad_r) {
        if (mlvfs_amd_render_resampled_amaze_dev(c.src, c.stride, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.os, c.n, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_resampled_amaze_dev did not happen", k);
        if (mlvfs_amd_render_resampled_amaze_look_dev(c.src, c.stride, c.w, c.h, c.par, c.ow, c.oh, c.dst, c.os, c.n, lk, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of render_resampled_amaze_look_dev did not happen", k);
        k++;
    }
    // the look forms want their look, and the deep form's strides are those of 6 bytes per pixel
    if (mlvfs_amd_render_resampled_amaze_look_dev(s, IMG, W, H, p, OW, OH, d, OUT, 1, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render_resampled_amaze_deep_dev(s, IMG, W, H, p, OW, OH, d, 2 * OUT, 1, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render_resampled_amaze_deep_dev(s, IMG, W, H, p, OW, OH, d, 2 * OUT - 1, 2, lk16, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render_resampled_amaze_deep_dev(s, IMG, W, H, p, W + 1, OH, d, 2 * OUT, 1, lk16, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of a look form did not happen", k);
    if (mlvfs_amd_render_resampled_amaze_dev(s, IMG, W, H, p, OW, OH, d, OUT, 0, nullptr) != MLVFS_AMD_OK) return fail("render_resampled_amaze: nothing to do is no error", k);
    for (size_t i = 0; i < 3 * IMG; i++) if (s[i] != 7) return fail("a refusal wrote the source", (int)i);
    for (size_t i = 0; i < 6 * OUT; i++) if (d[i] != 9) return fail("a refusal wrote the destination", (int)i);
    for (size_t i = 0; i < 9 * NP * sizeof(float); i++) if (((uint8_t *)q)[i] != 5) return fail("a refusal wrote the planes", (int)i);
    // the mount's setter follows no null handle
    if (mlvfs_amd_mount_set_resample_demosaic(nullptr, 1) != MLVFS_AMD_ERR_ARG) return fail("mount_set_resample_demosaic of a null handle", k);
    printf("amaze_resample_host_check: %d records, %d plans, %d refusals\n", rec, plans, k);
    return rec > 0 && plans > 0 ? 0 : 1;
}
