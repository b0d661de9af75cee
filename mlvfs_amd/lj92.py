"""LJ92 (lossless JPEG) frame payloads -> 16-bit frames in HBM: ctypes face of csrc/lj92.cpp + csrc/k_lj92.hip
(reference mlvfs/main.c:617-681, mlvfs/lj92.c)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib


def info(stream: bytes) -> dict:
    L = lib.load()
    dims = (C.c_int * 4)()
    buf = np.frombuffer(stream, np.uint8)
    lib.check(L.mlvfs_amd_lj92_info(lib.ptr(buf), buf.size, dims), "lj92_info")
    return dict(width=dims[0], height=dims[1], bits=dims[2], predictor=dims[3])


def decode_frames(streams, xres: int, yres: int, out=None, torch_stream=None):
    """Decode a batch of JPEG streams (bytes-like, host memory) into a (n, yres, xres) int16 CUDA tensor (bit pattern of
    the uint16 pixels), untiled like main.c:646-667 does."""
    import torch
    L = lib.load()
    n = len(streams)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (C.c_size_t * n)(*[b.size for b in bufs])
    if out is None:
        out = torch.empty((n, yres, xres), dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch_stream.cuda_stream) if torch_stream is not None else None
    lib.check(L.mlvfs_amd_lj92_decode_dev(ptrs, sizes, n, xres, yres, C.c_void_p(out.data_ptr()), out.stride(0) * 2, st), "lj92_decode_dev")
    return out


def encode(flat, w: int, h: int, bits: int = 14, read_len: int = 0, skip_len: int = 0, delin=None) -> bytes:
    """lj92_encode of the library (lj92.h:65-68): w x h values read from `flat` (host uint16) in runs of read_len values skip_len
    apart (0: contiguous) -> the JPEG stream.  Raises where the call refuses (what the reference cannot encode inside its arrays)."""
    L = lib.load()
    flat = np.ascontiguousarray(flat, np.uint16).reshape(-1)
    d = None if delin is None else np.ascontiguousarray(delin, np.uint16)
    enc = C.POINTER(C.c_uint8)()
    n = C.c_int(0)
    L.lj92_encode.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_int)]
    rc = L.lj92_encode(flat.ctypes.data, w, h, bits, read_len or w * h, skip_len, None if d is None else d.ctypes.data,
                       0 if d is None else d.size, C.byref(enc), C.byref(n))
    if rc != 0:
        raise lib.MlvfsAmdError(f"lj92_encode failed ({rc}): {L.mlvfs_amd_last_error().decode()}")
    try:
        return C.string_at(enc, n.value)
    finally:
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        libc.free(enc)


STATUS_OK, STATUS_DIFF17, STATUS_TABLE, STATUS_NOFIT = 0, 1, 2, 3           # MLVFS_AMD_LJ92ENC_*


def encode_batch(frames, bits: int = 16, out_stride: int = 0, torch_stream=None):
    """mlvfs_amd_lj92_encode_batch_dev: a batch of frames of one geometry -> (streams, classes, status).

    frames: an (n, h, w) CUDA/HIP tensor of 16-bit values (int16 or uint16 bit patterns; dim 0 may have any even byte stride) or a
    host array / list of arrays, which is uploaded.  streams[f]: the complete JPEG stream as bytes, or None where status[f] is not
    STATUS_OK (what the reference's encoder cannot encode inside its arrays, or a stream longer than out_stride);
    classes[f]: the highest difference class in use.  out_stride: room per stream on the device (0: 4 bytes per pixel, twice the pixels'
    own size; the worst case -- 16-bit codes, 16 value bits, every byte stuffed -- is 8)."""
    import torch
    L = lib.load()
    if not isinstance(frames, torch.Tensor):
        frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f, np.uint16) for f in frames])).view(np.int16)).cuda()
    if frames.dim() != 3 or frames.element_size() != 2 or not frames.is_cuda:
        raise ValueError("frames must be an (n, h, w) tensor of 16-bit values on the GPU")
    n, h, w = frames.shape
    if n and (frames.stride(2) != 1 or frames.stride(1) != w):
        raise ValueError("each frame must be contiguous")
    cap = out_stride or w * h * 4 + 1024
    out = torch.empty((max(n, 1), cap), dtype=torch.uint8, device=frames.device)
    lengths = np.zeros(max(n, 1), np.uint32)
    status = np.zeros(max(n, 1), np.int32)
    classes = np.zeros(max(n, 1), np.int32)
    st = C.c_void_p(torch_stream.cuda_stream) if torch_stream is not None else None
    lib.check(L.mlvfs_amd_lj92_encode_batch_dev(C.c_void_p(frames.data_ptr()), frames.stride(0) * 2 if n > 1 else w * h * 2, n, w, h, bits,
                                                C.c_void_p(out.data_ptr()), cap, lib.ptr(lengths), lib.ptr(status), lib.ptr(classes), st),
              "lj92_encode_batch_dev")
    streams = [out[f, :int(lengths[f])].cpu().numpy().tobytes() if status[f] == STATUS_OK else None for f in range(n)]
    return streams, [int(c) for c in classes[:n]], [int(v) for v in status[:n]]


def encode_table(hist, npix: int):
    """Host-only: the encoder's Huffman table for a class histogram (mlvfs_amd_lj92_encode_table), or None where it refuses."""
    L = lib.load()
    out = (C.c_int * 68)()
    hist = np.ascontiguousarray(hist, np.uint32)
    if L.mlvfs_amd_lj92_encode_table(hist.ctypes.data_as(C.POINTER(C.c_uint32)), npix, out) != 0:
        return None
    o = list(out)
    return dict(bits=o[0:16], nvalues=o[16], values=o[17:34], len=o[34:51], code=o[51:68])


def _frames_3d(frames):
    import torch
    if not isinstance(frames, torch.Tensor):
        frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f, np.uint16) for f in frames])).view(np.int16)).cuda()
    if frames.dim() != 3 or frames.element_size() != 2 or not frames.is_cuda:
        raise ValueError("frames must be an (n, h, w) tensor of 16-bit values on the GPU")
    n, h, w = frames.shape
    if n and (frames.stride(2) != 1 or frames.stride(1) != w):
        raise ValueError("each frame must be contiguous")
    return frames


def _check_out(out, shape, frames):
    """A caller's output tensor: 16-bit values on the frames' device, this shape, every frame (dim 0 may be strided) contiguous."""
    import torch
    if not isinstance(out, torch.Tensor) or out.element_size() != 2 or out.device != frames.device or tuple(out.shape) != tuple(shape):
        raise ValueError(f"out must be a tensor of 16-bit values of shape {tuple(shape)} on {frames.device}")
    inner = 1
    for d in range(out.dim() - 1, 0, -1):
        if shape[d] != 1 and out.stride(d) != inner:
            raise ValueError("each frame of out must be contiguous")
        inner *= shape[d]
    if shape[0] > 1 and out.stride(0) < inner:
        raise ValueError("the frames of out overlap")


def tile_frames(frames, out=None, torch_stream=None):
    """mlvfs_amd_lj92_tile_dev: (n, h, w) 16-bit frames on the GPU (or host arrays, which are uploaded) -> the same shape with the four
    Bayer channels of each frame as its four quadrants, what an MLV writer compresses (the inverse of decode_frames' untiling)."""
    import torch
    L = lib.load()
    frames = _frames_3d(frames)
    n, h, w = frames.shape
    if out is None:
        out = torch.empty((n, h, w), dtype=frames.dtype, device=frames.device)
    _check_out(out, (n, h, w), frames)
    st = C.c_void_p(torch_stream.cuda_stream) if torch_stream is not None else None
    lib.check(L.mlvfs_amd_lj92_tile_dev(C.c_void_p(frames.data_ptr()), frames.stride(0) * 2, C.c_void_p(out.data_ptr()), out.stride(0) * 2,
                                        w, h, n, st), "lj92_tile_dev")
    return out


def pack_frames(frames, bpp: int = 14, out=None, torch_stream=None):
    """mlvfs_amd_pack_dev: (n, h, w) 16-bit frames on the GPU (or host arrays) -> (n, ceil(w * h * bpp / 16)) int16 words of packed
    payload per frame, as an MLV file stores them (the inverse of mlvfs_amd_unpack_dev)."""
    import torch
    L = lib.load()
    frames = _frames_3d(frames)
    n, h, w = frames.shape
    words = (w * h * bpp + 15) // 16
    if out is None:
        out = torch.empty((n, words), dtype=torch.int16, device=frames.device)
    _check_out(out, (n, words), frames)
    geom = lib.Geom(w, h, bpp, 0, 0, 0, 0)
    st = C.c_void_p(torch_stream.cuda_stream) if torch_stream is not None else None
    lib.check(L.mlvfs_amd_pack_dev(C.byref(geom), C.c_void_p(frames.data_ptr()), frames.stride(0) * 2, C.c_void_p(out.data_ptr()),
                                   out.stride(0) * 2, n, st), "pack_dev")
    return out


def repack_frames(packed, w: int, h: int, bpp: int, out_bpp: int, dark=None, out=None, torch_stream=None):
    """mlvfs_amd_repack_dev: (n, ceil(w * h * bpp / 16)) 16-bit words of packed payload per frame on the GPU (or host arrays, which
    are uploaded) -> (n, ceil(w * h * out_bpp / 16)) words at out_bpp bits, every pixel shifted (>> when narrowing, no rounding) after
    `dark` (a mlvfs_amd.dark.Dark of the input's geometry, optional) was subtracted: unpack, subtract, shift and pack in one pass."""
    import torch
    L = lib.load()
    if not isinstance(packed, torch.Tensor):
        packed = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(p, np.uint16) for p in packed])).view(np.int16)).cuda()
    words_in, words = (w * h * bpp + 15) // 16, (w * h * out_bpp + 15) // 16
    if packed.dim() != 2 or packed.element_size() != 2 or not packed.is_cuda or packed.shape[1] != words_in:
        raise ValueError(f"packed must be an (n, {words_in}) tensor of 16-bit words on the GPU")
    n = packed.shape[0]
    if n and packed.stride(1) != 1:
        raise ValueError("each payload must be contiguous")
    if out is None:
        out = torch.empty((n, words), dtype=torch.int16, device=packed.device)
    _check_out(out, (n, words), packed)
    geom = lib.Geom(w, h, bpp, 0, 0, 0, 0)
    st = C.c_void_p(torch_stream.cuda_stream) if torch_stream is not None else None
    lib.check(L.mlvfs_amd_repack_dev(C.byref(geom), out_bpp, None if dark is None else dark.h, C.c_void_p(packed.data_ptr()), packed.stride(0) * 2,
                                     C.c_void_p(out.data_ptr()), out.stride(0) * 2, n, st), "repack_dev")
    return out
