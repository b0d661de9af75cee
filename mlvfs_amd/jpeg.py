"""Baseline JPEG files of a rendering: the definition of include/mlvfs_amd.h ("rendered frames as baseline JPEG files") in numpy, the
yardstick for csrc/jpeg.cpp and csrc/k_jpeg.hip.  Integers only, so the GPU's streams are these bytes exactly.

    qtables(quality)          -> (2, 64) uint8: luminance, chrominance, natural order
    header(pw, ph, quality)   -> the 629 bytes in front of the entropy-coded data
    encode(rgb, quality)      -> the entropy-coded data with its RST markers, then EOI
    split_file(data)          -> (header bytes, stream bytes) of a file as served
    file_sampling(data)       -> the sampling of a file as served: 420, 422 or 444

header + encode is a JFIF file any decoder opens: the Annex K Huffman tables, one restart interval per MCU row.  mcus, header,
coefficients and encode take the chroma sampling as an optional last argument: 420 (the default: MCUs of 16 x 16
pixels, blocks Y00 Y01 Y10 Y11 Cb Cr), 422 (16 x 8, Y0 Y1 Cb Cr, chroma halved along the row only) or 444 (8 x 8, Y Cb Cr).
"""
from __future__ import annotations

import numpy as np

HEADER_BYTES = 629                       # mlvfs_amd_jpeg_header_size()

# sampling -> (MCU width, MCU height, luminance blocks per MCU, the sampling factors of component 1 in SOF0, the C interface's number)
SAMPLINGS = {420: (16, 16, 4, 0x22, 0), 422: (16, 8, 2, 0x21, 1), 444: (8, 8, 1, 0x11, 2)}


def _sampling(sampling: int):
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling {sampling!r} is none of 420, 422, 444")
    return SAMPLINGS[sampling]

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# the forward DCT matrix times 8192, T[u][x]; tests/test_jpeg_cases.py holds it to round(8192 s(u) cos((2x + 1) u pi / 16))
DCT_T = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                  [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                  [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                  [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                  [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                  [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                  [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                  [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], np.int64)

# ZIGZAG[k]: the natural (row-major) index of the k-th coefficient in scan order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63], np.int64)

# the "typical" Huffman tables of Annex K.3 - K.6: 16 counts, then the symbols by code length
DC_LUMA = bytes.fromhex("00010501010101010100000000000000" "000102030405060708090a0b")
DC_CHROMA = bytes.fromhex("00030101010101010101010000000000" "000102030405060708090a0b")
AC_LUMA = bytes.fromhex(
    "0002010303020403050504040000017d"
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
AC_CHROMA = bytes.fromhex(
    "00020102040403040705040400010277"
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)          # the DHT segments' order; their Tc/Th bytes: 00 10 01 11


def huffman_codes(spec: bytes):
    """(length[256], code[256]) of a table given as 16 counts + symbols (Annex C); length 0: no such symbol"""
    length = np.zeros(256, np.int64)
    code = np.zeros(256, np.int64)
    c, k = 0, 16
    for bits in range(1, 17):
        for _ in range(spec[bits - 1]):
            length[spec[k]] = bits
            code[spec[k]] = c
            c += 1
            k += 1
        c <<= 1
    return length, code


def qtables(quality: int) -> np.ndarray:
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} outside 1 .. 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.uint8)


def mcus(pw: int, ph: int, sampling: int = 420):
    mcw, mch = _sampling(sampling)[:2]
    return (pw + mcw - 1) // mcw, (ph + mch - 1) // mch


def header(pw: int, ph: int, quality: int, sampling: int = 420) -> bytes:
    if pw < 1 or ph < 1 or pw > 65535 or ph > 65535 or pw * ph >= 1 << 25:
        raise ValueError(f"{pw}x{ph} pixels not supported")
    q = qtables(quality)
    out = bytearray(b"\xFF\xD8" b"\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xFF\xDB\x00\x43" + bytes([t]) + q[t][ZIGZAG].tobytes()
    out += b"\xFF\xC0\x00\x11\x08" + ph.to_bytes(2, "big") + pw.to_bytes(2, "big") + b"\x03\x01" + bytes([_sampling(sampling)[3]]) + b"\x00\x02\x11\x01\x03\x11\x01"
    for tc_th, spec in zip((0x00, 0x10, 0x01, 0x11), HUFFMAN):
        out += b"\xFF\xC4" + (3 + len(spec)).to_bytes(2, "big") + bytes([tc_th]) + spec
    out += b"\xFF\xDD\x00\x04" + mcus(pw, ph, sampling)[0].to_bytes(2, "big")
    out += b"\xFF\xDA\x00\x0C\x03\x01\x00\x02\x11\x03\x11\x00\x3F\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def ycbcr(rgb: np.ndarray):
    """(H, W, 3) uint8 -> Y, Cb, Cr as int32 planes, and Cb, Cr before their clamps"""
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11058 * r - 21710 * g + 32768 * b + 32768) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128
    return y, np.clip(cb, 0, 255), np.clip(cr, 0, 255), cb, cr


def fdct_quantise(blocks: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(..., 8, 8) samples 0 .. 255, q[64] natural -> (..., 64) quantised coefficients in natural order"""
    p = blocks.astype(np.int64) - 128
    a = (np.einsum("ux,...yx->...yu", DCT_T, p) + 128) >> 8
    b = np.einsum("vy,...yu->...vu", DCT_T, a)
    b = b.reshape(b.shape[:-2] + (64,))
    qq = q.astype(np.int64)
    v = np.sign(b) * (((np.abs(b) + (qq << 17)) >> 18) // qq)
    v[..., 1:] = np.clip(v[..., 1:], -1023, 1023)
    return v


def coefficients(rgb: np.ndarray, quality: int, trace: dict | None = None, sampling: int = 420) -> np.ndarray:
    """(mh, mw, ny + 2, 64): the quantised coefficients in scan (zigzag) order; the ny luminance blocks of an MCU from left to right (at
    420 the top row first: Y00 Y01 Y10 Y11), then Cb, Cr"""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8:
        raise ValueError("a rendering is (H', W', 3) uint8")
    mcw, mch, ny = _sampling(sampling)[:3]
    ph, pw = rgb.shape[:2]
    mw, mh = mcus(pw, ph, sampling)
    q = qtables(quality)
    y, cb, cr, cb0, cr0 = ycbcr(rgb)
    if trace is not None:
        trace.update(cb_range=(int(cb0.min()), int(cb0.max())), cr_range=(int(cr0.min()), int(cr0.max())))     # before the clamps
    pad = ((0, mch * mh - ph), (0, mcw * mw - pw))
    y, cb, cr = (np.pad(p, pad, mode="edge") for p in (y, cb, cr))
    if sampling == 420:
        half = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    elif sampling == 422:
        half = lambda p: (p[:, 0::2] + p[:, 1::2] + 1) >> 1
    else:
        half = lambda p: p
    by, bx = mch // 8, mcw // 8                             # luminance blocks down and across an MCU
    yb = y.reshape(mh, by, 8, mw, bx, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh, mw, ny, 8, 8)
    cbb, crb = (half(p).reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3) for p in (cb, cr))
    out = np.empty((mh, mw, ny + 2, 64), np.int64)
    out[:, :, :ny] = fdct_quantise(yb, q[0])
    out[:, :, ny] = fdct_quantise(cbb, q[1])
    out[:, :, ny + 1] = fdct_quantise(crb, q[1])
    return out[..., ZIGZAG]


def _category(v: np.ndarray) -> np.ndarray:
    a = np.abs(v)
    cat = np.zeros(a.shape, np.int64)
    for k in range(12):
        cat += a >= (1 << k)
    return cat


def encode(rgb: np.ndarray, quality: int, trace: dict | None = None, sampling: int = 420) -> bytes:
    """the entropy-coded data of the rendering rgb, (H', W', 3) uint8, with its RST markers, then EOI.  trace: a dict that receives
    what the stream exercised (for the tests)"""
    co = coefficients(rgb, quality, trace, sampling)
    mh, mw = co.shape[:2]
    ny = co.shape[2] - 2
    tabs = [huffman_codes(s) for s in HUFFMAN]
    # per coefficient: L bits with the value V, in scan order
    L = np.zeros(co.shape, np.int64)
    V = np.zeros(co.shape, np.uint64)
    dc = co[..., 0]
    pred = np.zeros_like(dc)
    pred[:, :, 1:ny] = dc[:, :, 0:ny - 1]
    pred[:, 1:, 0] = dc[:, :-1, ny - 1]
    pred[:, 1:, ny:] = dc[:, :-1, ny:]
    d = dc - pred
    dcat = _category(d)
    dbits = np.where(d >= 0, d, d + (1 << dcat) - 1)
    zrl_count = 0
    for comp, blocks in ((0, slice(0, ny)), (1, slice(ny, ny + 2))):
        dl, dcode = tabs[2 * comp]
        al, acode = tabs[2 * comp + 1]
        c = co[:, :, blocks]
        L[:, :, blocks, 0] = dl[dcat[:, :, blocks]] + dcat[:, :, blocks]
        V[:, :, blocks, 0] = ((dcode[dcat[:, :, blocks]] << dcat[:, :, blocks]) | dbits[:, :, blocks]).astype(np.uint64)
        ac = c[..., 1:]
        nz = ac != 0
        pos = np.arange(1, 64)
        last = np.maximum.accumulate(np.where(nz, pos, 0), axis=-1)                # the last non-zero position up to here
        prev = np.concatenate([np.zeros(last.shape[:-1] + (1,), np.int64), last[..., :-1]], axis=-1)
        run = pos - prev - 1
        cat = _category(ac)
        vbits = np.where(ac >= 0, ac, ac + (1 << cat) - 1)
        sym = ((run & 15) << 4) | cat
        zrls = run >> 4
        ln = zrls * al[0xF0] + al[sym] + cat
        val = np.zeros(ac.shape, np.uint64)
        for k in range(4):
            more = zrls > k
            val = np.where(more, (val << np.uint64(al[0xF0])) | np.uint64(acode[0xF0]), val)
        val = (val << (al[sym] + cat).astype(np.uint64)) | ((acode[sym] << cat) | vbits).astype(np.uint64)
        ln = np.where(nz, ln, 0)
        val = np.where(nz, val, np.uint64(0))
        eob = ~nz[..., 62]
        ln[..., 62] = np.where(eob, al[0], ln[..., 62])
        val[..., 62] = np.where(eob, np.uint64(acode[0]), val[..., 62])
        L[:, :, blocks, 1:] = ln
        V[:, :, blocks, 1:] = val
        zrl_count += int((zrls * nz).sum())
        if trace is not None:
            trace.setdefault("ac_categories", set()).update(int(x) for x in np.unique(cat[nz]))
            trace.setdefault("ac_categories_chroma" if comp else "ac_categories_luma", set()).update(int(x) for x in np.unique(cat[nz]))
            trace["ac_clamped"] = trace.get("ac_clamped", False) or bool((np.abs(ac) == 1023).any())
            trace["eob"] = trace.get("eob", False) or bool(eob.any())
            trace["no_eob"] = trace.get("no_eob", False) or bool((~eob).any())
    out = bytearray()
    pads, stuffed, pad_stuffed = set(), 0, 0
    shifts = np.arange(63, -1, -1, dtype=np.uint64)
    for r in range(mh):
        l, v = L[r].reshape(-1), V[r].reshape(-1)
        keep = l > 0
        l, v = l[keep], v[keep]
        m = ((v[:, None] << (64 - l).astype(np.uint64)[:, None]) >> shifts[None, :]) & np.uint64(1)       # MSB first, left-aligned
        bits = m.astype(np.uint8)[np.arange(64)[None, :] < l[:, None]]
        pad = -len(bits) % 8
        data = np.packbits(np.concatenate([bits, np.ones(pad, np.uint8)]))
        ff = data == 0xFF
        if pad and ff[-1]:                                  # a 0xFF byte that only the padding completed
            pad_stuffed += 1
        pads.add(pad)
        stuffed += int(ff.sum())
        wide = np.zeros((len(data), 2), np.uint8)
        wide[:, 0] = data
        flat = wide.reshape(-1)[np.stack([np.ones(len(data), bool), ff], axis=1).reshape(-1)]
        out += flat.tobytes()
        out += bytes([0xFF, 0xD0 + r % 8]) if r + 1 < mh else b"\xFF\xD9"
    if trace is not None:
        trace.update(dc_categories=set(int(x) for x in np.unique(dcat)), dc_categories_luma=set(int(x) for x in np.unique(dcat[:, :, :ny])),
                     dc_categories_chroma=set(int(x) for x in np.unique(dcat[:, :, ny:])), zrl=zrl_count, pads=pads, stuffed=stuffed,
                     pad_stuffed=pad_stuffed, rows=mh)
    return bytes(out)


def _split(data: bytes):
    data = bytes(data)
    if len(data) < HEADER_BYTES + 2 or data[:2] != b"\xFF\xD8" or data[-2:] != b"\xFF\xD9":
        raise ValueError("not a file of this module")
    head = data[:HEADER_BYTES]
    ph, pw = int.from_bytes(head[163:165], "big"), int.from_bytes(head[165:167], "big")
    q = np.frombuffer(head[25:89], np.uint8)
    for quality in range(1, 101):
        if np.array_equal(qtables(quality)[0][ZIGZAG], q):
            for sampling in SAMPLINGS:
                if header(pw, ph, quality, sampling) == head:
                    return head, data[HEADER_BYTES:], sampling
    raise ValueError("the header is not one of this module's")


def split_file(data: bytes):
    """a file as served -> (header, stream); the header is checked to be the one this module writes for the size it declares, at any of
    the three samplings (which one: file_sampling)"""
    return _split(data)[:2]


def file_sampling(data: bytes) -> int:
    """the sampling of a file as served: 420, 422 or 444; ValueError as split_file"""
    return _split(data)[2]
