// tensor.h -- a clip's frames as device-resident tensors (include/mlvfs_amd.h, "a clip's frames as device-resident tensors"): what the
// host code (tensor.cpp, mount.cpp) and the kernels (k_tensor.hip) share -- the element of a dtype, which dtypes a source takes, the
// range of scale and bias, and the two launchers.  One element-wise pass behind whatever produced the rendering or the final frame.
#pragma once

#include "common.h"

#include <cmath>

namespace mlv {

// mlvfs_amd_tensor_bayer_params' int32 per frame: black, range, the bits of unit, 0 (the pass reads [0] and [2])
constexpr int TENSOR_LEVELS = 4;

// scale_c and bias_c as the kernels take them: by value, so that they are scalar loads
struct TensorAffine {
    float scale[4] = { 1, 1, 1, 1 }, bias[4] = { 0, 0, 0, 0 };
};

inline bool tensor_dtype_ok(int dt) { return dt >= MLVFS_AMD_TENSOR_F32 && dt <= MLVFS_AMD_TENSOR_U16; }
inline bool tensor_layout_ok(int ly) { return ly == MLVFS_AMD_TENSOR_NCHW || ly == MLVFS_AMD_TENSOR_NHWC; }
inline bool tensor_is_int(int dt) { return dt == MLVFS_AMD_TENSOR_U8 || dt == MLVFS_AMD_TENSOR_U16; }
inline size_t tensor_elem(int dt) { return dt == MLVFS_AMD_TENSOR_F32 ? 4 : dt == MLVFS_AMD_TENSOR_U8 ? 1 : 2; }
// the float dtypes for every source; of the integer ones the source's own depth (Bayer: 16)
inline bool tensor_dtype_legal(int dt, int src_bits)
{
    return tensor_dtype_ok(dt) && (!tensor_is_int(dt) || dt == (src_bits == 8 ? MLVFS_AMD_TENSOR_U8 : MLVFS_AMD_TENSOR_U16));
}
// finite, and zero or of magnitude within [2^-64, 2^64]
inline bool tensor_factor_ok(float x) { return std::isfinite(x) && (x == 0.0f || (std::fabs(x) >= 0x1p-64f && std::fabs(x) <= 0x1p64f)); }

// dtype, layout, and for a float dtype the C scales and biases of a spec against a source of src_bits; false with the error set in
// the name of `who`
bool tensor_spec_ok(const char *who, const mlvfs_amd_tensor_spec_t *spec, int src_bits, int channels);
inline TensorAffine tensor_affine(const mlvfs_amd_tensor_spec_t &spec)
{
    TensorAffine a;
    for (int c = 0; c < 4; c++) { a.scale[c] = spec.scale[c]; a.bias[c] = spec.bias[c]; }
    return a;
}

// nframes renderings of pw x ph pixels of three src_bits-bit samples -> their tensors; everything checked by the callers, the form
// picked here (k_tensor.hip)
int launch_tensor_rgb(const void *d_src, size_t src_stride, int pw, int ph, int src_bits, int dtype, int layout, const TensorAffine &a, void *d_out,
                      size_t out_stride, int nframes, hipStream_t stream);
// nframes frames of w x h 16-bit pixels, frame k with d_levels[TENSOR_LEVELS k ..] -> their tensors of 4 x (h / 2) x (w / 2)
int launch_tensor_bayer(const void *d_frames, size_t stride, int w, int h, const int32_t *d_levels, int dtype, int layout, const TensorAffine &a,
                        void *d_out, size_t out_stride, int nframes, hipStream_t stream);

}  // namespace mlv
