// tensor.cpp -- a clip's frames as device-resident tensors on the host (tensor.h; include/mlvfs_amd.h, "a clip's frames as device-resident
// tensors"): what a spec may ask for, the Bayer pass's per-frame parameters from a frame's headers, and the two device entry points
// mlvfs_amd_tensor_rgb_dev and mlvfs_amd_tensor_bayer_dev -- every check before any device work, then the launcher, which picks the
// form.  Nothing here knows a mount (mlvfs_amd_mount_tensor: mount.cpp).
#include "clip.h"
#include "tensor.h"

#include <cstring>

using namespace mlv;

namespace mlv {

bool tensor_spec_ok(const char *who, const mlvfs_amd_tensor_spec_t *spec, int src_bits, int channels)
{
    if (!spec) { set_error("%s: null argument", who); return false; }
    if (!tensor_dtype_ok(spec->dtype) || !tensor_layout_ok(spec->layout)) {
        set_error("%s: a dtype of %d (0: F32, 1: F16, 2: BF16, 3: U8, 4: U16) or a layout of %d (0: NCHW, 1: NHWC)", who, spec->dtype, spec->layout);
        return false;
    }
    if (!tensor_dtype_legal(spec->dtype, src_bits)) {
        set_error("%s: dtype %d is illegal for a %d-bit source (an integer tensor keeps the source's own samples: U8 of 8-bit, U16 of 16-bit ones)", who,
                  spec->dtype, src_bits);
        return false;
    }
    if (tensor_is_int(spec->dtype)) return true;                       // scale and bias are not read
    for (int c = 0; c < channels; c++)
        if (!tensor_factor_ok(spec->scale[c]) || !tensor_factor_ok(spec->bias[c])) {
            set_error("%s: scale %g or bias %g of channel %d outside the range (finite, and zero or of magnitude 2^-64 .. 2^64)", who, (double)spec->scale[c],
                      (double)spec->bias[c], c);
            return false;
        }
    return true;
}

}  // namespace mlv

namespace {

// what both device entry points check alike once the sizes are known: simg, timg bytes of a source frame and of its tensor, sa and
// es the alignment of a source sample and of an element
int check_buffers(const char *who, const void *d_src, size_t src_stride, size_t simg, size_t sa, const void *d_out, size_t out_stride, size_t timg,
                  size_t es, int nframes)
{
    if (((uintptr_t)d_src % sa) || ((uintptr_t)d_out % es)) { set_error("%s: the source or the destination off its element's boundary", who); return MLVFS_AMD_ERR_ARG; }
    if (src_stride < simg || (src_stride % sa) || out_stride < timg || (out_stride % es)) {
        set_error("%s: strides %zu / %zu too small (%zu / %zu), or no multiple of the element", who, src_stride, out_stride, simg, timg);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t a0 = (uintptr_t)d_src, a1 = a0 + (size_t)(nframes - 1) * src_stride + simg;
    const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (size_t)(nframes - 1) * out_stride + timg;
    if (a0 < b1 && b0 < a1) { set_error("%s: the destination overlaps the source (the pass does not work in place)", who); return MLVFS_AMD_ERR_ARG; }
    return MLVFS_AMD_OK;
}

}  // namespace

extern "C" {

int mlvfs_amd_tensor_bayer_params(const struct frame_headers *fh, int32_t out[4])
{
    if (!fh || !out) { set_error("tensor_bayer_params: null argument"); return MLVFS_AMD_ERR_ARG; }
    const int64_t black = fh->rawi_hdr.raw_info.black_level, white = fh->rawi_hdr.raw_info.white_level;
    if (black > (1 << 30) || black < -(1 << 30)) { set_error("tensor_bayer_params: a black level of %lld (|black| <= 2^30)", (long long)black); return MLVFS_AMD_ERR_ARG; }
    const int64_t range = std::max<int64_t>(white - black, 1);
    const float unit = (float)(1.0 / (double)range);                   // divided in double, rounded once
    int32_t bits;
    memcpy(&bits, &unit, sizeof bits);
    const int32_t p[4] = { (int32_t)black, (int32_t)std::min<int64_t>(range, INT32_MAX), bits, 0 };    // (unit is of the range itself)
    memcpy(out, p, sizeof p);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_tensor_rgb_dev(const void *d_src, size_t src_stride, int pw, int ph, int src_bits, const mlvfs_amd_tensor_spec_t *spec, void *d_out,
                             size_t out_stride, int nframes, void *stream)
{
    if (!d_src || !d_out || !spec) { set_error("tensor_rgb: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("tensor_rgb: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (src_bits != 8 && src_bits != 16) { set_error("tensor_rgb: a source of %d bits (8 or 16)", src_bits); return MLVFS_AMD_ERR_ARG; }
    if (pw < 1 || ph < 1 || (uint64_t)pw * (uint64_t)ph >= (1u << 28)) { set_error("tensor_rgb: %dx%d not supported (1x1 up to 2^28 pixels)", pw, ph); return MLVFS_AMD_ERR_ARG; }
    if (!tensor_spec_ok("tensor_rgb", spec, src_bits, 3)) return MLVFS_AMD_ERR_ARG;
    const size_t sa = (size_t)src_bits / 8, es = tensor_elem(spec->dtype), n = (size_t)3 * pw * ph;
    if (const int rc = check_buffers("tensor_rgb", d_src, src_stride, n * sa, sa, d_out, out_stride, n * es, es, nframes)) return rc;
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_tensor_rgb(d_src, src_stride, pw, ph, src_bits, spec->dtype, spec->layout, tensor_affine(*spec), d_out, out_stride, nframes,
                             pick_stream(stream, c));
}

int mlvfs_amd_tensor_bayer_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_levels, const mlvfs_amd_tensor_spec_t *spec,
                               void *d_out, size_t out_stride, int nframes, void *stream)
{
    if (!d_frames || !d_levels || !d_out || !spec) { set_error("tensor_bayer: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("tensor_bayer: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (width < 2 || height < 2 || (uint64_t)width * (uint64_t)height >= (1u << 28)) {
        set_error("tensor_bayer: %dx%d not supported (2x2 up to 2^28 pixels)", width, height);
        return MLVFS_AMD_ERR_ARG;
    }
    if (!tensor_spec_ok("tensor_bayer", spec, 16, 4)) return MLVFS_AMD_ERR_ARG;
    if ((uintptr_t)d_levels & 3) { set_error("tensor_bayer: levels off a 4-byte boundary"); return MLVFS_AMD_ERR_ARG; }
    const size_t es = tensor_elem(spec->dtype), timg = (size_t)4 * (width / 2) * (height / 2) * es;
    if (const int rc = check_buffers("tensor_bayer", d_frames, stride, (size_t)width * height * 2, 2, d_out, out_stride, timg, es, nframes)) return rc;
    if (nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (size_t)(nframes - 1) * out_stride + timg;
    const uintptr_t p0 = (uintptr_t)d_levels, p1 = p0 + (size_t)nframes * TENSOR_LEVELS * sizeof(int32_t);
    if (p0 < b1 && b0 < p1) { set_error("tensor_bayer: the destination overlaps the levels"); return MLVFS_AMD_ERR_ARG; }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_tensor_bayer(d_frames, stride, width, height, d_levels, spec->dtype, spec->layout, tensor_affine(*spec), d_out, out_stride, nframes,
                               pick_stream(stream, c));
}

}  // extern "C"
