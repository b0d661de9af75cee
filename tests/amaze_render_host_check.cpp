// amaze_render_host_check.cpp -- a stand-alone host program for tests/test_amaze_render_host.py: the host code of the AMaZE rendering
// (include/mlvfs_amd.h, "rendered full-size frames demosaiced by AMaZE") -- the geometry, the sub-batch arithmetic and every argument
// check of mlvfs_amd_amaze_balance_dev, mlvfs_amd_amaze_tone_dev and mlvfs_amd_render1_amaze_dev, which happen before any device work
// and follow no pointer.  It is compiled and linked with -fsanitize=address,undefined against the sanitizer build of the library's
// host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// GEOM.bin: records of {int32 w, h, expected return code, expected pw, expected ph} for mlvfs_amd_rgb_amaze_geom.
// PLAN.bin: records of {int64 w, h, nframes, cap_bytes, expected return code, expected out[0 .. 3]} for mlvfs_amd_test_amaze_render_plan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "amaze_render_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: amaze_render_host_check GEOM.bin PLAN.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        int32_t r[5];
        if (fread(r, sizeof r, 1, f) != 1) break;
        // exactly one int each: a write past either is the sanitizer's to see
        std::unique_ptr<int> pw(new int(-7)), ph(new int(-7));
        if (mlvfs_amd_rgb_amaze_geom(r[0], r[1], pw.get(), ph.get()) != r[2]) return fail("another return code", rec);
        if (*pw != r[3] || *ph != r[4]) return fail("another geometry", rec);
    }
    fclose(f);
    int one = 5;
    if (mlvfs_amd_rgb_amaze_geom(64, 64, nullptr, &one) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_amaze_geom(64, 64, &one, nullptr) != MLVFS_AMD_ERR_ARG || one != 5)
        return fail("a refusal of rgb_amaze_geom did not happen", rec);

    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    int plans = 0;
    for (;; plans++) {
        int64_t r[9];
        if (fread(r, sizeof r, 1, f) != 1) break;
        std::unique_ptr<int64_t[]> out(new int64_t[4]);              // exactly four
        for (int i = 0; i < 4; i++) out[i] = -7;
        if (mlvfs_amd_test_amaze_render_plan((int)r[0], (int)r[1], (int)r[2], (size_t)r[3], out.get()) != (int)r[4]) return fail("plan: another return code", plans);
        for (int i = 0; i < 4; i++) if (out[i] != r[5 + i]) return fail("plan: another number", plans);
    }
    fclose(f);
    if (mlvfs_amd_test_amaze_render_plan(64, 64, 1, 0, nullptr) != MLVFS_AMD_ERR_ARG) return fail("plan: a null pointer", plans);

    // a 48 x 36 frame: 3456 bytes in, 1728 floats a plane, 5184 bytes out (10368 at 16 bits); host memory, exactly that long, for three frames
    const int W = 48, H = 36;
    const size_t IMG = 3456, NP = 1728, OUT = 5184;
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
    int k = 0;

    struct B { const void *src; size_t stride; int w, h; const int32_t *par; float *pl; size_t ps; int n; };
    const B bad_b[] = {
        { nullptr, IMG, W, H, p, q, NP, 1 }, { s, IMG, W, H, nullptr, q, NP, 1 }, { s, IMG, W, H, p, nullptr, NP, 1 },
        { s, IMG, 34, H, p, q, NP, 1 }, { s, IMG, W, 35, p, q, NP, 1 }, { s, IMG, 46, H, p, q, NP, 1 }, { s, IMG, 0, 0, p, q, NP, 1 },
        { s, IMG, -48, H, p, q, NP, 1 }, { s, IMG, 1 << 13, 1 << 12, p, q, NP, 1 }, { s, IMG, 1 << 30, 1 << 30, p, q, NP, 1 },
        { s, IMG, W, H, p, q, NP, -1 }, { s, IMG - 2, W, H, p, q, NP, 2 }, { s, IMG, W, H, p, q, NP - 1, 2 }, { s, IMG + 1, W, H, p, q, NP, 2 },
        { s + 1, IMG, W, H, p, q, NP, 1 }, { s, IMG, W, H, p2, q, NP, 1 }, { s, IMG, W, H, p, (float *)((uint8_t *)q + 2), NP, 1 },
        { s, IMG, W, H, p, (float *)s, NP, 1 }, { s, IMG, W, H, p, (float *)(s + IMG - 4), NP, 1 }, { s, IMG, W, H, p, (float *)p, NP, 1 },
        { q, IMG, W, H, p, q + 800, NP, 1 },
    };
    for (const B &c : bad_b) {
        if (mlvfs_amd_amaze_balance_dev(c.src, c.stride, c.w, c.h, c.par, c.pl, c.ps, c.n, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a refusal of amaze_balance_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_amaze_balance_dev(s, IMG, W, H, p, q, NP, 0, nullptr) != MLVFS_AMD_OK) return fail("balance: nothing to do is no error", k);

    const mlvfs_amd_look_t *lk = (const mlvfs_amd_look_t *)&one;        // never followed: both set is refused first
    const mlvfs_amd_look16_t *lk16 = (const mlvfs_amd_look16_t *)&one;
    struct T { const float *r, *g, *b; size_t ps; int w, h; const int32_t *par; void *dst; size_t os; int n; const mlvfs_amd_look_t *l; const mlvfs_amd_look16_t *l16; };
    const T bad_t[] = {
        { nullptr, qg, qb, NP, W, H, p, d, OUT, 1, nullptr, nullptr }, { qr, nullptr, qb, NP, W, H, p, d, OUT, 1, nullptr, nullptr },
        { qr, qg, nullptr, NP, W, H, p, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, nullptr, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, nullptr, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, d, OUT, 1, lk, lk16 },
        { qr, qg, qb, NP, 34, H, p, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, 35, p, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, 50, H, p, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, 1 << 13, 1 << 12, p, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, d, OUT, -1, nullptr, nullptr }, { qr, qg, qb, NP - 1, W, H, p, d, OUT, 2, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, d, OUT - 1, 2, nullptr, nullptr }, { (const float *)((const uint8_t *)qr + 2), qg, qb, NP, W, H, p, d, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p2, d, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, qr, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, (uint8_t *)qg + 100, OUT, 1, nullptr, nullptr }, { qr, qg, qb, NP, W, H, p, (uint8_t *)(qb + NP) - 1, OUT, 1, nullptr, nullptr },
        { qr, qg, qb, NP, W, H, p, p, OUT, 1, nullptr, nullptr },
    };
    for (const T &c : bad_t) {
        if (mlvfs_amd_amaze_tone_dev(c.r, c.g, c.b, c.ps, c.w, c.h, c.par, c.dst, c.os, c.n, c.l, c.l16, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a refusal of amaze_tone_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_amaze_tone_dev(qr, qg, qb, NP, W, H, p, d, OUT, 0, nullptr, nullptr, nullptr) != MLVFS_AMD_OK) return fail("tone: nothing to do is no error", k);

    struct R { const void *src; size_t stride; int w, h; const int32_t *par; void *dst; size_t os; int n; };
    const R bad_r[] = {
        { nullptr, IMG, W, H, p, d, OUT, 1 }, { s, IMG, W, H, nullptr, d, OUT, 1 }, { s, IMG, W, H, p, nullptr, OUT, 1 },
        { s, IMG, 34, H, p, d, OUT, 1 }, { s, IMG, W, 35, p, d, OUT, 1 }, { s, IMG, 46, H, p, d, OUT, 1 }, { s, IMG, 16, 8, p, d, OUT, 1 },
        { s, IMG, 1 << 13, 1 << 12, p, d, OUT, 1 }, { s, IMG, 1 << 30, 1 << 30, p, d, OUT, 1 }, { s, IMG, W, H, p, d, OUT, -1 },
        { s, IMG - 2, W, H, p, d, OUT, 2 }, { s, IMG, W, H, p, d, OUT - 1, 2 }, { s, IMG + 1, W, H, p, d, OUT, 2 }, { s + 1, IMG, W, H, p, d, OUT, 1 },
        { s, IMG, W, H, p2, d, OUT, 1 }, { s, IMG, W, H, p, s, OUT, 1 }, { s, IMG, W, H, p, s + IMG - 1, OUT, 1 }, { d + OUT - 1, IMG, W, H, p, d, OUT, 1 },
        { s, IMG, W, H, p, p, OUT, 1 },
    };
    for (const R &c : bad_r) {
        if (mlvfs_amd_render1_amaze_dev(c.src, c.stride, c.w, c.h, c.par, c.dst, c.os, c.n, nullptr) != MLVFS_AMD_ERR_ARG) return fail("a refusal of render1_amaze_dev did not happen", k);
        k++;
    }
    // the look forms want their look, and the deep form's strides are those of 6 bytes per pixel
    if (mlvfs_amd_render1_amaze_look_dev(s, IMG, W, H, p, d, OUT, 1, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render1_amaze_deep_dev(s, IMG, W, H, p, d, 2 * OUT, 1, nullptr, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render1_amaze_deep_dev(s, IMG, W, H, p, d, 2 * OUT - 1, 2, lk16, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of a look form did not happen", k);
    if (mlvfs_amd_render1_amaze_dev(s, IMG, W, H, p, d, OUT, 0, nullptr) != MLVFS_AMD_OK) return fail("render1_amaze: nothing to do is no error", k);
    for (size_t i = 0; i < 3 * IMG; i++) if (s[i] != 7) return fail("a refusal wrote the source", (int)i);
    for (size_t i = 0; i < 6 * OUT; i++) if (d[i] != 9) return fail("a refusal wrote the destination", (int)i);
    for (size_t i = 0; i < 9 * NP * sizeof(float); i++) if (((uint8_t *)q)[i] != 5) return fail("a refusal wrote the planes", (int)i);
    // the mount's setter follows no null handle and takes two values
    if (mlvfs_amd_mount_set_demosaic(nullptr, 1) != MLVFS_AMD_ERR_ARG) return fail("mount_set_demosaic of a null handle", k);
    printf("amaze_render_host_check: %d records, %d plans, %d refusals\n", rec, plans, k);
    return rec > 0 && plans > 0 ? 0 : 1;
}
