"""The cases of the tensor pass (tests/test_gpu_tensor.py runs them on the GPU against mlvfs_amd/tensor.py; tests/test_tensor_cases.py
proves on the CPU that they reach what they claim and tell the wrong definitions apart).  Everything here is deterministic and small.

A case is a dict: kind, w, h (the rendering's pw x ph, or the Bayer frame's W x H), bits (the source's), dtype, layout, n (frames of the
batch), set (the scale / bias set's name), and how the buffers lie: aligned, src_off, dst_off, and pad bytes added to each stride.
frames(case) gives the source frames, levels(case) a Bayer batch's (black, white) per frame, want(case) the definition's bytes."""
import numpy as np

from mlvfs_amd import tensor as T

RGB_SIZES = [(1, 1), (7, 3), (8, 2), (9, 5), (16, 4), (24, 2), (64, 1), (72, 3), (520, 2), (1032, 3)]
BAYER_SIZES = [(2, 2), (6, 6), (7, 5), (16, 4), (32, 2), (48, 4), (30, 10), (1040, 4)]
FLOATS = (T.F32, T.F16, T.BF16)
f32 = np.float32


def _bits_to_f32(b):
    return np.array([b], np.uint32).view(np.float32)[0]


# values that go through the conversions untouched by any arithmetic (scale 0: the element is the bias): per channel a half tie that
# goes down to even, a half tie that goes up to even, a value above the largest half; and a subnormal half that is no multiple of 2^-24
CONVERT_BIAS = (_bits_to_f32(0x3F801000), _bits_to_f32(0x3F803000), f32(70000.0), f32(2.0 ** -20 * 1.3125 + 2.0 ** -26))
# the same for bfloat16: ties at bit 15 with bit 16 clear and set, a value just above a tie, one just below
CONVERT_BIAS_BF = (_bits_to_f32(0x3F808000), _bits_to_f32(0x3F818000), _bits_to_f32(0x40490FDB), _bits_to_f32(0xC2F6E979))
_MEAN, _STD = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.25)
SETS = {
    "identity": (np.ones(4, f32), np.zeros(4, f32)),
    "imagenet": T.normalisation(_MEAN, _STD, 4),
    "convert": (np.zeros(4, f32), np.array(CONVERT_BIAS, f32)),
    "convert_bf": (np.zeros(4, f32), np.array(CONVERT_BIAS_BF, f32)),
    "small": (np.array([2.0 ** -12, 3 * 2.0 ** -15, 2.0 ** -20, 2.0 ** -10], f32), np.zeros(4, f32)),       # subnormal halves from real samples
    "big": (np.array([70000.0, 2.0 ** 16, 2.0 ** 64, -1e5], f32), np.array([0.0, -3.0, 2.0 ** -64, 1.0], f32)),   # halves that overflow; the range's ends
}
SET_NAMES = list(SETS)
# how the buffers of a case lie: (frames, aligned, source offset and destination offset in elements of 16 bytes or of one sample /
# element, padding of the strides in the same unit)
CONFIGS = [(1, True, 0, 0, 0), (3, True, 1, 2, 2), (3, False, 1, 1, 1), (1, False, 3, 1, 0)]
# a Bayer batch's levels, frame by frame from a rotating start: a clip's own and its x4 levels after a dual-ISO conversion alternate (a
# mixed clip, both parities), a range that is a power of two (exact units: natural ties), levels with pixels below black and above white
LEVELS = [(1024, 5120), (60, 16383), (2048, 15000), (8192, 60000), (2048, 15000), (8192, 60000), (40000, 40000), (-77, 4019)]


def up16(v):
    return (v + 15) // 16 * 16


def _cases(kind, sizes):
    out = []
    for si, (w, h) in enumerate(sizes):
        for bits in ((8, 16) if kind == T.RGB else (16,)):
            for dtype in (T.F32, T.F16, T.BF16, T.U8, T.U16):
                if not T.legal(dtype, bits):
                    continue
                for layout in (T.NCHW, T.NHWC):
                    for ci, (n, aligned, so, do, pad) in enumerate(CONFIGS):
                        # two sets per configuration, rotating so that every set meets every form, dtype and layout somewhere
                        rot = si + dtype + 2 * layout + bits // 8
                        names = [SET_NAMES[(rot + 2 * ci + j) % len(SET_NAMES)] for j in range(2)] if dtype in FLOATS else ["identity"]
                        for name in names:
                            out.append(dict(kind=kind, w=w, h=h, bits=bits, dtype=dtype, layout=layout, n=n, set=name, aligned=aligned, src_off=so,
                                            dst_off=do, pad=pad, seed=len(out)))
    return out


def rgb_cases():
    return _cases(T.RGB, RGB_SIZES)


def bayer_cases():
    return _cases(T.BAYER, BAYER_SIZES)


def frames(case):
    """the n source frames: (ph, pw, 3) uint8 / uint16 renderings, or (H, W) uint16 mosaics"""
    w, h, n, seed = case["w"], case["h"], case["n"], case["seed"]
    out = []
    for k in range(n):
        if case["kind"] == T.RGB:
            i = np.arange(h * w * 3, dtype=np.int64)
            if case["bits"] == 8:
                a = ((i * 37 + 101 * k + 53 * seed) % 256).astype(np.uint8)                 # every byte value within 256 samples
            else:
                a = ((i * 40503 + 977 * k + 7919 * seed) % 65536).astype(np.uint16)
                special = np.array([0, 1, 2, 3, 65535], np.uint16)
                m = min(a.size, 5)
                a[:m] = np.roll(special, -(seed + k))[:m]
            out.append(a.reshape(h, w, 3))
        else:
            black, white = levels(case)[k]
            i = np.arange(h * w, dtype=np.int64)
            a = (i * 40503 + 977 * k + 7919 * seed) % 65536
            # pixels with exact half and bfloat16 ties at a power-of-two range, below black, far above white, and the type's ends
            special = np.clip(np.array([black + 2049, black + 2051, black + 257, black + 259, black - 5, white + 1000, 0, 65535, black, white,
                                        black - 1, black + 1]), 0, 65535)
            m = min(a.size, special.size)
            a[:m] = np.roll(special, -(seed + k))[:m]
            out.append(a.astype(np.uint16).reshape(h, w))
    return out


def levels(case):
    """(black, white) of each frame of a Bayer batch"""
    return [LEVELS[(case["seed"] + k) % len(LEVELS)] for k in range(case["n"])]


def levels_array(case):
    """the device array of a Bayer batch: black, range, the bits of unit, 0 per frame"""
    out = np.zeros((case["n"], 4), np.int32)
    for k, (black, white) in enumerate(levels(case)):
        b, r, u = T.bayer_levels(black, white)
        out[k] = (b, r, int(np.array([u], np.float32).view(np.int32)[0]), 0)
    return out


def scale_bias(case):
    return SETS[case["set"]]


def channels(case):
    return 3 if case["kind"] == T.RGB else 4


def src_bytes(case):
    return case["w"] * case["h"] * (3 * case["bits"] // 8 if case["kind"] == T.RGB else 2)


def out_shape(case):
    h, w = (case["h"], case["w"]) if case["kind"] == T.RGB else (case["h"] // 2, case["w"] // 2)
    return h, w


def out_bytes(case):
    h, w = out_shape(case)
    return channels(case) * h * w * T.ELEM[case["dtype"]]


def placement(case):
    """-> (source stride, source offset, destination stride, destination offset) in bytes"""
    sa = case["bits"] // 8 if case["kind"] == T.RGB else 2
    es = T.ELEM[case["dtype"]]
    if case["aligned"]:
        return up16(src_bytes(case)) + 16 * case["pad"], 16 * case["src_off"], up16(out_bytes(case)) + 16 * case["pad"], 16 * case["dst_off"]
    return src_bytes(case) + sa * case["pad"], sa * case["src_off"], out_bytes(case) + es * case["pad"], es * case["dst_off"]


def takes_fast_form(case):
    """whether the launcher picks the x8 kernel: the width rule, and bases and strides on 16 bytes (the buffers themselves are)"""
    ss, so, ds, do = placement(case)
    wide = case["w"] % (8 if case["kind"] == T.RGB else 16) == 0
    return wide and so % 16 == 0 and do % 16 == 0 and (case["n"] == 1 or (ss % 16 == 0 and ds % 16 == 0))


# ---------------------------------------------------------------- the definition, and the wrong ones
WRONG = ["fma", "folded", "trunc_f16", "trunc_bf16", "flush_f16", "bgr", "g1g2", "layouts", "clamp_black"]


def _trunc_f16(f):
    with np.errstate(over="ignore"):
        hf = f.astype(np.float16)
    over = np.abs(hf.astype(np.float32)) > np.abs(f)                  # rounded away from zero (infinity included): one step back
    return np.where(over, np.nextafter(hf, np.float16(0)), hf).astype(np.float16).view(np.uint16)


def _flush_f16(f):
    b = T.f16_bits(f)
    return np.where(np.abs(f) < np.float32(2.0 ** -14), b & np.uint16(0x8000), b).astype(np.uint16)


def compute(case, k, variant=None):
    """frame k of the case under the definition (variant None: through mlvfs_amd/tensor.py's own entry points) or a wrong one -> bytes"""
    data = frames(case)[k]
    scale, bias = scale_bias(case)
    dtype, layout = case["dtype"], case["layout"]
    if variant is None:
        if case["kind"] == T.RGB:
            return T.rgb(data, case["bits"], dtype, layout, scale, bias).tobytes()
        return T.bayer(data, *levels(case)[k], dtype, layout, scale, bias).tobytes()
    if case["kind"] == T.RGB:
        raw, unit = data, T.unit_of(case["bits"])
        if variant == "bgr":
            raw = raw[..., ::-1]
        v = raw.astype(np.int64)
    else:
        black, _, unit = T.bayer_levels(*levels(case)[k])
        raw = T.bayer_planes(data)
        if variant == "g1g2":
            raw = raw[..., [0, 2, 1, 3]]
        v = raw.astype(np.int64) - black
        if variant == "clamp_black":
            v = np.maximum(v, 0)
    c = v.shape[-1]
    if dtype in (T.U8, T.U16):
        e = raw.astype(T.BITS_DTYPE[dtype])
    else:
        s, b = np.asarray(scale, f32)[:c], np.asarray(bias, f32)[:c]
        x = v.astype(f32)
        if variant == "folded":
            f = x * (f32(unit) * s) + b
        elif variant == "fma":
            f = ((x * f32(unit)).astype(np.float64) * s.astype(np.float64) + b.astype(np.float64)).astype(f32)
        else:
            f = T.f32_value(v, unit, scale, bias)
        if dtype == T.F32:
            e = f.view(np.uint32)
        elif dtype == T.F16:
            e = _trunc_f16(f) if variant == "trunc_f16" else _flush_f16(f) if variant == "flush_f16" else T.f16_bits(f)
        else:
            e = (f.view(np.uint32) >> 16).astype(np.uint16) if variant == "trunc_bf16" else T.bf16_bits(f)
    return T.lay_out(e, (1 - layout) if variant == "layouts" else layout).tobytes()


def want(case):
    return [compute(case, k) for k in range(case["n"])]


def case_id(case):
    return "{}:{}x{}:{}b:dt{}:ly{}:n{}:{}:{}".format("rgb" if case["kind"] == T.RGB else "bayer", case["w"], case["h"], case["bits"], case["dtype"],
                                                     case["layout"], case["n"], case["set"], "a" if case["aligned"] else "m")
