"""The baseline JPEG definition of mlvfs_amd/jpeg.py and the cases of tests/jpeg_cases.py (no GPU): the issue's cross-check hashes, every
case decoded by PIL, the PSNR against PIL's own encoder, what the cases reach, and the constants -- the DCT matrix against its formula,
the quantisation tables against PIL's for every quality, the Huffman tables against the DHT segments PIL writes."""
import hashlib
import io

import numpy as np
import pytest
from PIL import Image

from mlvfs_amd import jpeg

import jpeg_cases as jc


def file_of(rgb, quality, trace=None):
    ph, pw = rgb.shape[:2]
    return jpeg.header(pw, ph, quality) + jpeg.encode(rgb, quality, trace)


def decode(data):
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "JPEG" and im.mode == "RGB"
        return np.asarray(im.convert("RGB"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("ph,pw,quality,size,sha,rst", [
    (24, 40, 75, 1275, "a1158804be13a479", None), (24, 40, 100, 2663, "31a75bdb25df0137", None), (24, 40, 1, 701, "71b66ad594278a3c", None),
    (150, 20, 90, 3927, "464c6dbb3166c8fe", [2, 1, 1, 1, 1, 1, 1, 1])])
def test_cross_check_hashes(ph, pw, quality, size, sha, rst):
    data = file_of(jc.formula(pw, ph), quality)
    assert len(data) == size and hashlib.sha256(data).hexdigest().startswith(sha)
    if rst:
        stream = data[jpeg.HEADER_BYTES:]
        assert [stream.count(bytes([0xFF, 0xD0 + k])) for k in range(8)] == rst
    head, stream = jpeg.split_file(data)
    assert len(head) == jpeg.HEADER_BYTES == 629 and head + stream == data


@pytest.fixture(scope="module")
def traces():
    """every case encoded once: [(pw, ph, content, quality, file, trace)]"""
    out = []
    for pw, ph, content, q in jc.all_cases():
        tr = {}
        rgb = content(pw, ph)
        out.append((pw, ph, content, q, file_of(rgb, q, tr), tr))
    return out


def test_pil_decodes_every_case(traces):
    for pw, ph, content, q, data, _ in traces:
        assert decode(data).shape == (ph, pw, 3), (pw, ph, content.__name__, q)


def test_psnr_is_within_half_a_db_of_pils_encoder(traces):
    """at shapes of at least 17 x 17, on the formula, gradient and noise images: decoded by PIL, no more than 0.5 dB below PIL's own
    save(quality=q, subsampling=2) of the same RGB"""
    worst = (0.0, ())
    for pw, ph, content, q, data, _ in traces:
        if content not in jc.SMOOTH or min(pw, ph) < 17:
            continue
        rgb = content(pw, ph)
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=2)
        short = psnr(rgb, decode(b.getvalue())) - psnr(rgb, decode(data))
        print(f"{pw}x{ph} {content.__name__} q{q}: {short:+.3f} dB below PIL, {len(data)} against {len(b.getvalue())} bytes")
        worst = max(worst, (short, (pw, ph, content.__name__, q)))
        assert short <= 0.5, (pw, ph, content.__name__, q, short)
    print("worst shortfall", worst)


def test_what_the_cases_reach(traces):
    tr = [t for *_, t in traces]
    any_ = lambda key: any(t[key] for t in tr)
    union = lambda key: set().union(*(t[key] for t in tr))
    # both ends of Cb and of Cr before their clamps.  The upper clamp is reached (256); the lower one cannot be: the sums are linear in
    # R, G, B, so their extremes lie at the eight corners of the cube, and the lowest corner gives exactly -127 + 128 = 1 for both
    # (32768 = 11058 + 21710 = 27439 + 5329: the rounding term alone remains of 65536 * -127.5 + 32768)
    corners = np.array([[[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]], np.uint8)
    _, _, _, cb0, cr0 = jpeg.ycbcr(corners)
    assert (cb0.min(), cb0.max(), cr0.min(), cr0.max()) == (1, 256, 1, 256)
    for key in ("cb_range", "cr_range"):
        assert min(t[key][0] for t in tr) == 1 and max(t[key][1] for t in tr) == 256, key
    assert {0, 11} <= union("dc_categories")
    # AC category 10 is reached; the clamp to +-1023 is not, and no 8-bit input reaches it: a coefficient is largest for the block of 0
    # and 255 in the sign pattern of its basis function, and the largest of those 2 x 63 blocks gives 1020 at Q = 1
    assert 10 in union("ac_categories") and not any_("ac_clamped")
    sign, extreme = np.sign(jpeg.DCT_T), 0
    for v in range(8):
        for u in range(8):
            for s in (1, -1):
                blk = np.where(s * sign[v][:, None] * sign[u][None, :] > 0, 255, 0)
                got = jpeg.fdct_quantise(blk[None], np.ones(64, np.uint8))[0]
                assert abs(got[v * 8 + u]) == np.abs(got).max()
                if u or v:
                    extreme = max(extreme, int(np.abs(got[1:]).max()))
    assert extreme == 1020
    assert any_("zrl") and any_("eob") and any_("no_eob")
    assert union("pads") == set(range(8))
    assert any_("stuffed") and any_("pad_stuffed")
    assert any(t["rows"] >= 10 for t in tr), "the RST index never wraps"
    # edge replication on both axes: a case whose size is no multiple of 16 either way, and whose last column and row matter
    pw, ph = 17, 17
    rgb = jc.noise(pw, ph)
    grown = np.pad(rgb, ((0, 32 - ph), (0, 32 - pw), (0, 0)), mode="edge")
    assert np.array_equal(jpeg.coefficients(rgb, 90), jpeg.coefficients(grown, 90))
    other = np.pad(rgb, ((0, 32 - ph), (0, 32 - pw), (0, 0)))
    assert not np.array_equal(jpeg.coefficients(rgb, 90), jpeg.coefficients(other, 90))


def test_all_eight_rst_indices_and_the_wrap():
    stream = jpeg.encode(jc.formula(20, 150), 90)
    marks = [stream[k + 1] for k in range(len(stream) - 1) if stream[k] == 0xFF and 0xD0 <= stream[k + 1] <= 0xD7]
    assert marks == [0xD0 + k % 8 for k in range(9)]


def test_the_clamp_of_cb_is_reached_as_the_definition_says():
    y, cb, cr, cb0, cr0 = jpeg.ycbcr(np.array([[[0, 0, 255], [255, 0, 0]]], np.uint8))
    assert cb0[0, 0] == 256 and cb[0, 0] == 255 and cr0[0, 1] == 256 and cr[0, 1] == 255


def test_dct_matrix_is_its_formula():
    t = [[round(8192 * (np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)) for x in range(8)] for u in range(8)]
    assert np.array_equal(jpeg.DCT_T, np.array(t))
    assert list(jpeg.DCT_T[0]) == [2896] * 8 and list(jpeg.DCT_T[1]) == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017]
    assert list(jpeg.DCT_T[4]) == [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896]
    # what the kernel's eight-point pass rests on: T[u][7 - x] = (-1)^u T[u][x]
    sign = np.array([1, -1] * 4)[:, None]
    assert np.array_equal(jpeg.DCT_T[:, ::-1], sign * jpeg.DCT_T)
    # the ranges the definition states: |A| < 2^14, |B| < 2^29
    worst = np.abs(jpeg.DCT_T).sum(axis=1).max()
    a = (worst * 128 + 128) >> 8
    assert a < 1 << 14 and worst * a < 1 << 29


def test_quantisation_tables_are_pils_for_every_quality():
    im = Image.new("RGB", (16, 16))
    for q in range(1, 101):
        b = io.BytesIO()
        im.save(b, "JPEG", quality=q, subsampling=2)
        with Image.open(io.BytesIO(b.getvalue())) as back:
            tabs = back.quantization
        ours = jpeg.qtables(q)
        for t in range(2):
            theirs = np.array(tabs[t])
            # PIL hands the tables out in zigzag or in natural order, depending on its version: one of the two must be ours
            assert np.array_equal(theirs, ours[t]) or np.array_equal(theirs, ours[t][jpeg.ZIGZAG]), (q, t)
        assert b.getvalue()[25:89] == ours[0][jpeg.ZIGZAG].tobytes(), q        # the DQT segment itself: zigzag order in the file


def test_huffman_constants_are_the_dht_segments_pil_writes():
    b = io.BytesIO()
    Image.new("RGB", (16, 16)).save(b, "JPEG", quality=75, subsampling=2)
    d, i, found = b.getvalue(), 2, {}
    while d[i + 1] != 0xDA:
        n = int.from_bytes(d[i + 2:i + 4], "big")
        if d[i + 1] == 0xC4:
            seg, j = d[i + 4:i + 2 + n], 0
            while j < len(seg):
                cnt = sum(seg[j + 1:j + 17])
                found[seg[j]] = bytes(seg[j + 1:j + 17 + cnt])
                j += 17 + cnt
        i += 2 + n
    assert found == {0x00: jpeg.DC_LUMA, 0x10: jpeg.AC_LUMA, 0x01: jpeg.DC_CHROMA, 0x11: jpeg.AC_CHROMA}
    assert [len(s) for s in jpeg.HUFFMAN] == [28, 178, 28, 178]
    for spec in jpeg.HUFFMAN:
        length, code = jpeg.huffman_codes(spec)
        used = length > 0
        assert used.sum() == len(spec) - 16 and length.max() <= 16 and (code[used] < (1 << length[used]) - 1).all()   # no code of all ones


def test_refusals_of_the_oracle():
    with pytest.raises(ValueError):
        jpeg.qtables(0)
    with pytest.raises(ValueError):
        jpeg.qtables(101)
    with pytest.raises(ValueError):
        jpeg.header(0, 4, 90)
    with pytest.raises(ValueError):
        jpeg.header(8192, 4096, 90)
    with pytest.raises(ValueError):
        jpeg.encode(np.zeros((4, 4), np.uint8), 90)
    with pytest.raises(ValueError):
        jpeg.split_file(b"\xFF\xD8" + bytes(700))
