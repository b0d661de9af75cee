// tensor_host_check.cpp -- a stand-alone host program for tests/test_tensor_host.py: the host code of the tensor route
// (include/mlvfs_amd.h, "a clip's frames as device-resident tensors") -- mlvfs_amd_tensor_bayer_params against levels computed in Python,
// every refusal of mlvfs_amd_tensor_rgb_dev, mlvfs_amd_tensor_bayer_dev, mlvfs_amd_mount_tensor and mlvfs_amd_mount_tensor_bytes that
// happens before any device work, with buffers of exactly the sizes a call could touch and nothing written, and the sizes
// mlvfs_amd_mount_tensor_bytes answers for a clip.  It is compiled and linked with -fsanitize=address,undefined against the sanitizer
// build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// Arguments: CASES.bin CLIP.MLV W H.  CASES.bin: records of {int32 black, int32 white, int32 want[4]}; want[1] == 0: the levels are refused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int at)
{
    fprintf(stderr, "tensor_host_check: %d: %s (%s)\n", at, what, mlvfs_amd_last_error());
    return 1;
}

static mlvfs_amd_tensor_spec_t spec_of(int kind, int dtype, int layout, float scale = 1.0f, float bias = 0.0f)
{
    mlvfs_amd_tensor_spec_t s;
    memset(&s, 0, sizeof s);
    s.kind = kind;
    s.dtype = dtype;
    s.layout = layout;
    s.gain_q8 = 256;
    for (int c = 0; c < 4; c++) { s.scale[c] = scale; s.bias[c] = bias; }
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: tensor_host_check CASES.bin CLIP.MLV W H\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int W = atoi(argv[3]), H = atoi(argv[4]);
    int rec = 0, refusals = 0;
    for (;; rec++) {
        int32_t in[6];
        if (fread(in, sizeof(int32_t), 6, f) != 6) break;
        std::unique_ptr<frame_headers> fh(new frame_headers);
        memset(fh.get(), 0, sizeof(frame_headers));
        fh->rawi_hdr.raw_info.black_level = in[0];
        fh->rawi_hdr.raw_info.white_level = in[1];
        std::unique_ptr<int32_t[]> out(new int32_t[4]);                 // exactly what the helper may write
        for (int i = 0; i < 4; i++) out[i] = -7;
        const int rc = mlvfs_amd_tensor_bayer_params(fh.get(), out.get());
        if (in[3] == 0) {
            if (rc != MLVFS_AMD_ERR_ARG) return fail("levels that must be refused were taken", rec);
            for (int i = 0; i < 4; i++) if (out[i] != -7) return fail("a refusal wrote the parameters", rec);
            refusals++;
            continue;
        }
        if (rc != MLVFS_AMD_OK) return fail("tensor_bayer_params refused", rec);
        if (memcmp(out.get(), in + 2, 4 * sizeof(int32_t))) return fail("other parameters", rec);
    }
    fclose(f);
    {
        std::unique_ptr<frame_headers> fh(new frame_headers);
        memset(fh.get(), 0, sizeof(frame_headers));
        int32_t out[4] = { -7, -7, -7, -7 };
        if (mlvfs_amd_tensor_bayer_params(nullptr, out) != MLVFS_AMD_ERR_ARG || mlvfs_amd_tensor_bayer_params(fh.get(), nullptr) != MLVFS_AMD_ERR_ARG || out[0] != -7)
            return fail("tensor_bayer_params took a null pointer", rec);
    }

    // the two device entry points: an 8 x 8 rendering (192 or 384 bytes in) and a 16 x 16 frame (512 bytes in); host memory of exactly
    // the sizes a call of 2 frames could touch; no check follows a pointer
    std::unique_ptr<uint8_t[]> src(new uint8_t[1024]), dst(new uint8_t[1024]);
    std::unique_ptr<int32_t[]> lv(new int32_t[8]);
    memset(src.get(), 7, 1024);
    memset(dst.get(), 9, 1024);
    memset(lv.get(), 0, 8 * sizeof(int32_t));
    uint8_t *s = src.get(), *d = dst.get();
    const int32_t *p = lv.get();
    const int RGB = MLVFS_AMD_TENSOR_RGB, BAYER = MLVFS_AMD_TENSOR_BAYER, F32 = MLVFS_AMD_TENSOR_F32, F16 = MLVFS_AMD_TENSOR_F16, U8 = MLVFS_AMD_TENSOR_U8,
              U16 = MLVFS_AMD_TENSOR_U16, NCHW = MLVFS_AMD_TENSOR_NCHW;
    const mlvfs_amd_tensor_spec_t ok = spec_of(RGB, F16, NCHW), okb = spec_of(BAYER, F16, NCHW);
    const mlvfs_amd_tensor_spec_t bad_specs[] = {
        spec_of(RGB, 5, NCHW), spec_of(RGB, -1, NCHW), spec_of(RGB, F16, 2), spec_of(RGB, F16, -1), spec_of(RGB, U16, NCHW), spec_of(RGB, F32, NCHW, INFINITY),
        spec_of(RGB, F32, NCHW, 1.0f, NAN), spec_of(RGB, F16, NCHW, 0x1p65f), spec_of(RGB, F16, NCHW, 0x1p-65f), spec_of(RGB, F16, NCHW, 1.0f, -0x1p65f),
        spec_of(RGB, F16, NCHW, 1.0f, 0x1p-65f), spec_of(RGB, F16, NCHW, -INFINITY),
    };
    int k = 0;
    for (const mlvfs_amd_tensor_spec_t &b : bad_specs) {
        if (mlvfs_amd_tensor_rgb_dev(s, 192, 8, 8, 8, &b, d, 384, 1, nullptr) != MLVFS_AMD_ERR_ARG) return fail("tensor_rgb_dev took a spec it must refuse", k);
        mlvfs_amd_tensor_spec_t bb = b;
        if (bb.dtype == U16) bb.dtype = U8;                             // the integer dtype a Bayer source does not take
        if (mlvfs_amd_tensor_bayer_dev(s, 512, 16, 16, p, &bb, d, 512, 1, nullptr) != MLVFS_AMD_ERR_ARG) return fail("tensor_bayer_dev took a spec it must refuse", k);
        k++;
    }
    struct RgbCase { const void *src; size_t stride; int pw, ph, bits; const mlvfs_amd_tensor_spec_t *spec; void *dst; size_t ostride; int n; };
    const mlvfs_amd_tensor_spec_t u8 = spec_of(RGB, U8, NCHW);
    const RgbCase bad_rgb[] = {
        { nullptr, 192, 8, 8, 8, &ok, d, 384, 1 }, { s, 192, 8, 8, 8, nullptr, d, 384, 1 }, { s, 192, 8, 8, 8, &ok, nullptr, 384, 1 }, { s, 192, 0, 8, 8, &ok, d, 384, 1 },
        { s, 192, 8, -1, 8, &ok, d, 384, 1 }, { s, 192, 1 << 14, 1 << 14, 8, &ok, d, 384, 1 }, { s, 192, 8, 8, 12, &ok, d, 384, 1 }, { s, 192, 8, 8, 0, &ok, d, 384, 1 },
        { s, 192, 8, 8, 8, &ok, d, 384, -1 }, { s, 191, 8, 8, 8, &ok, d, 384, 2 }, { s, 192, 8, 8, 8, &ok, d, 382, 2 }, { s, 192, 8, 8, 8, &ok, d, 385, 2 },
        { s, 192, 8, 8, 8, &ok, d + 1, 384, 1 }, { s + 1, 384, 8, 8, 16, &ok, d, 384, 1 }, { s, 385, 8, 8, 16, &ok, d, 384, 2 }, { s, 384, 8, 8, 16, &u8, d, 192, 1 },
        { s, 192, 8, 8, 8, &ok, s, 384, 1 }, { s, 192, 8, 8, 8, &ok, s + 190, 384, 1 }, { s + 400, 192, 8, 8, 8, &ok, s + 18, 384, 1 },
    };
    for (const RgbCase &c : bad_rgb) {
        if (mlvfs_amd_tensor_rgb_dev(c.src, c.stride, c.pw, c.ph, c.bits, c.spec, c.dst, c.ostride, c.n, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of tensor_rgb_dev did not happen", k);
        k++;
    }
    struct BayerCase { const void *src; size_t stride; int w, h; const int32_t *lv; const mlvfs_amd_tensor_spec_t *spec; void *dst; size_t ostride; int n; };
    const BayerCase bad_bayer[] = {
        { nullptr, 512, 16, 16, p, &okb, d, 512, 1 }, { s, 512, 16, 16, nullptr, &okb, d, 512, 1 }, { s, 512, 16, 16, p, nullptr, d, 512, 1 },
        { s, 512, 16, 16, p, &okb, nullptr, 512, 1 }, { s, 512, 1, 16, p, &okb, d, 512, 1 }, { s, 512, 16, 1, p, &okb, d, 512, 1 },
        { s, 512, 1 << 14, 1 << 14, p, &okb, d, 512, 1 }, { s, 512, 16, 16, p, &okb, d, 512, -1 }, { s, 510, 16, 16, p, &okb, d, 512, 2 },
        { s, 513, 16, 16, p, &okb, d, 512, 2 }, { s, 512, 16, 16, p, &okb, d, 510, 2 }, { s + 1, 512, 16, 16, p, &okb, d, 512, 1 },
        { s, 512, 16, 16, (const int32_t *)((const uint8_t *)p + 2), &okb, d, 512, 1 }, { s, 512, 16, 16, p, &okb, d + 1, 512, 1 },
        { s, 512, 16, 16, p, &okb, s + 510, 512, 1 }, { s, 512, 16, 16, (const int32_t *)(d + 64), &okb, d, 512, 1 },
    };
    for (const BayerCase &c : bad_bayer) {
        if (mlvfs_amd_tensor_bayer_dev(c.src, c.stride, c.w, c.h, c.lv, c.spec, c.dst, c.ostride, c.n, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of tensor_bayer_dev did not happen", k);
        k++;
    }
    if (mlvfs_amd_tensor_rgb_dev(s, 192, 8, 8, 8, &ok, d, 384, 0, nullptr) != MLVFS_AMD_OK || mlvfs_amd_tensor_bayer_dev(s, 512, 16, 16, p, &okb, d, 512, 0, nullptr) != MLVFS_AMD_OK)
        return fail("nothing to do is no error", k);

    // the mount's two calls on a clip of W x H: the sizes, and every refusal that comes before any device work
    void *reader = mlvfs_amd_mlv_open(argv[2], 0);
    if (!reader) return fail("the clip does not open", 0);
    mlvfs_amd_mount_opts_t opts;
    memset(&opts, 0, sizeof opts);
    void *m = mlvfs_amd_mount_open(reader, &opts, "/T.MLV");
    if (!m) return fail("the mount does not open", 0);
    const size_t pw = W / 2, ph = H / 2;
    mlvfs_amd_tensor_spec_t sp = spec_of(RGB, F16, NCHW);
    if (mlvfs_amd_mount_tensor_bytes(m, 0, &sp) != 3 * pw * ph * 2) return fail("another size of a half-size F16 tensor", 0);
    sp.dtype = F32;
    sp.size = MLVFS_AMD_TENSOR_FULL;
    if (mlvfs_amd_mount_tensor_bytes(m, 0, &sp) != (size_t)3 * W * H * 4) return fail("another size of a full-size F32 tensor", 1);
    sp.dtype = U8;
    sp.size = MLVFS_AMD_TENSOR_SCALED;
    sp.ow = 5;
    sp.oh = 3;
    if (mlvfs_amd_mount_tensor_bytes(m, 0, &sp) != 45) return fail("another size of a scaled U8 tensor", 2);
    sp.size = MLVFS_AMD_TENSOR_RESAMPLED;
    sp.ow = W;
    sp.oh = H - 1;
    if (mlvfs_amd_mount_tensor_bytes(m, 0, &sp) != (size_t)3 * W * (H - 1)) return fail("another size of a resampled U8 tensor", 3);
    mlvfs_amd_tensor_spec_t sb = spec_of(BAYER, U16, MLVFS_AMD_TENSOR_NHWC);
    if (mlvfs_amd_mount_tensor_bytes(m, 0, &sb) != 4 * pw * ph * 2) return fail("another size of a Bayer U16 tensor", 4);
    // refused: nulls, no such frame, specs outside the definition, shapes the route does not take
    mlvfs_amd_tensor_spec_t r1 = spec_of(RGB, F16, NCHW), r2 = r1, r3 = r1, r4 = r1, r5 = r1, r6 = r1, r7 = spec_of(2, F16, NCHW), r8 = spec_of(BAYER, U8, NCHW);
    r1.size = MLVFS_AMD_TENSOR_SCALED; r1.ow = (int)pw + 1; r1.oh = 1;          // wider than the half size
    r2.size = MLVFS_AMD_TENSOR_RESAMPLED; r2.ow = 1; r2.oh = H + 1;
    r3.size = 4;
    r4.gain_q8 = 0;
    r5.size = MLVFS_AMD_TENSOR_SCALED;                                          // ow = oh = 0
    r6.dtype = U16;                                                            // an 8-bit rendering as U16
    const mlvfs_amd_tensor_spec_t *refused[] = { &r1, &r2, &r3, &r4, &r5, &r6, &r7, &r8, &bad_specs[0], &bad_specs[5], &bad_specs[8] };
    for (const mlvfs_amd_tensor_spec_t *r : refused) {
        if (mlvfs_amd_mount_tensor_bytes(m, 0, r) != 0) return fail("mount_tensor_bytes answered for a spec it must refuse", k);
        if (mlvfs_amd_mount_tensor(m, 0, 1, d, 1024, r, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG) return fail("mount_tensor took a spec it must refuse", k);
        k++;
    }
    if (mlvfs_amd_mount_tensor_bytes(nullptr, 0, &ok) || mlvfs_amd_mount_tensor_bytes(m, 0, nullptr) || mlvfs_amd_mount_tensor_bytes(m, -1, &ok) ||
        mlvfs_amd_mount_tensor_bytes(m, 1 << 20, &ok))
        return fail("mount_tensor_bytes answered for a null pointer or a frame that is none", k);
    const size_t need = 3 * pw * ph * 2;
    if (mlvfs_amd_mount_tensor(nullptr, 0, 1, d, need, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_mount_tensor(m, 0, 1, nullptr, need, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_tensor(m, 0, 1, d, need, nullptr, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_mount_tensor(m, 0, -1, d, need, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_tensor(m, 1 << 20, 1, d, need, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_mount_tensor(m, 0, 1, d, need - 2, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_mount_tensor(m, 0, 1, d, need + 1, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_mount_tensor(m, 0, 1, d + 1, need, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of mount_tensor did not happen", k);
    if (mlvfs_amd_mount_tensor(m, 0, 0, d, need, &ok, 2, 0, nullptr) != MLVFS_AMD_OK) return fail("nothing to do is no error", k);
    if (mlvfs_amd_mount_set_proxy(m, 2) != MLVFS_AMD_OK) return fail("the proxy is refused", k);
    if (mlvfs_amd_mount_tensor(m, 0, 1, d, need, &ok, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG || !strstr(mlvfs_amd_last_error(), "prox"))
        return fail("a proxy handle took a tensor call", k);
    if (mlvfs_amd_mount_tensor(m, 0, 1, d, 4 * pw * ph * 2, &okb, 2, 0, nullptr) != MLVFS_AMD_ERR_ARG || !strstr(mlvfs_amd_last_error(), "prox"))
        return fail("a proxy handle took a Bayer tensor call", k);
    mlvfs_amd_mount_close(m);
    mlvfs_amd_mlv_close(reader);
    for (int i = 0; i < 1024; i++) if (s[i] != 7) return fail("a refusal wrote the source", i);
    for (int i = 0; i < 1024; i++) if (d[i] != 9) return fail("a refusal wrote the destination", i);
    for (int i = 0; i < 8; i++) if (p[i] != 0) return fail("a refusal wrote the levels", i);
    printf("tensor_host_check: %d records, %d + %d refusals\n", rec, refusals, k);
    return rec > 0 ? 0 : 1;
}
