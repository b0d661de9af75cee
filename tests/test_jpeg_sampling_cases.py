"""The chroma samplings of mlvfs_amd/jpeg.py (4:2:2, 4:4:4) and the cases of tests/jpeg_sampling_cases.py (no GPU): the
default is what it was, the issue's cross-check hashes, every case decoded by PIL, the PSNR against PIL's own encoder at the same
sampling, what the cases reach, and that the cases tell wrong definitions from the right one."""
import hashlib
import io

import numpy as np
import pytest
from PIL import Image

from mlvfs_amd import jpeg

import jpeg_cases as jc
import jpeg_sampling_cases as sc

PIL_SUBSAMPLING = {444: 0, 422: 1, 420: 2}
# the worst shortfall against PIL's encoder, measured over the shapes, contents and qualities of test_psnr_against_pils_encoder, and the
# bound it gives: that value rounded up to the next tenth of a dB
#   4:2:2: 1.426 dB, gradient 100 x 83 at quality 100, at 50 dB.  libjpeg's h2v1 mean alternates its rounding term between 0 and 1 from
#          sample to sample; the definition always adds 1, so a ramp's chroma lies a quarter of a step high.  Only the gradient shows
#          it (208 x 132: 0.79 dB at quality 90, 0.56 dB at quality 100); formula and noise stay within 0.02 dB
#   4:4:4: 0.114 dB, gradient 208 x 132 at quality 50
PSNR_BOUND = {422: 1.5, 444: 0.2}


def file_of(rgb, quality, sampling, trace=None):
    ph, pw = rgb.shape[:2]
    return jpeg.header(pw, ph, quality, sampling) + jpeg.encode(rgb, quality, trace, sampling)


def decode(data):
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "JPEG" and im.mode == "RGB"
        return np.asarray(im.convert("RGB"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_shapes_are_what_they_are_derived_to_be():
    assert (sc.GROUP, sc.CHUNK) == ({420: 4, 422: 4, 444: 8}, {420: 16, 422: 24, 444: 32})
    for s in sc.SAMPLINGS:
        nb = jpeg.SAMPLINGS[s][2] + 2
        assert sc.GROUP[s] * nb <= 24 and sc.CHUNK[s] * nb == 96, "the workgroups' LDS is sized for 24 and 96 blocks"
        grid = [jpeg.mcus(pw, ph, s) for pw, ph in sc.shapes(s)]
        g, c = sc.GROUP[s], sc.CHUNK[s]
        assert grid == [(1, 1), (1, 1), (2, 2), (2, 5), (2, 1), (3, 2), (g, 1), (g + 1, 1), (c + 3, 2), (2, 10), (13, 9)], (s, grid)
        assert [jpeg.mcus(pw, ph, s) for pw, ph in sc.LONG[s]] == [(257, 1), (1, 1025)]
        for pw, ph in sc.shapes(s)[2:6] + sc.shapes(s)[8:10]:
            assert pw % sc.mcu(s)[0] or ph % sc.mcu(s)[1], "a shape meant to end in a partly empty MCU"


def test_the_default_is_unchanged():
    """sampling=420 is the call without it, byte for byte, on every case of tests/jpeg_cases.py; the tables of jc.expected are today's"""
    for pw, ph, content, q in jc.all_cases():
        rgb = content(pw, ph)
        assert jpeg.header(pw, ph, q, 420) == jpeg.header(pw, ph, q)
        assert jpeg.encode(rgb, q, None, 420) == jpeg.encode(rgb, q) == jc.expected(pw, ph, jc.CONTENT.index(content), q), (pw, ph, content.__name__, q)
        assert jpeg.coefficients(rgb, q).shape == jpeg.mcus(pw, ph)[::-1] + (6, 64)
    assert jpeg.mcus(300, 20) == jpeg.mcus(300, 20, 420) == (19, 2)
    data = jpeg.header(40, 24, 75) + jpeg.encode(jc.formula(40, 24), 75)
    assert len(data) == 1275 and hashlib.sha256(data).hexdigest().startswith("a1158804be13a479")        # tests/test_jpeg_cases.py's pin
    assert jpeg.split_file(data) == (data[:629], data[629:]) and jpeg.file_sampling(data) == 420


@pytest.mark.parametrize("sampling,pw,ph,quality,size,sha", [
    (444, 17, 9, 90, 798, "55d9e1a9813e8ec9"), (444, 40, 24, 75, 1468, "208405b507dcc371"), (444, 100, 83, 50, 6557, "8d3653335a872cf2"),
    (444, 208, 132, 100, 104185, "137a3a5813fe6be4"), (422, 17, 9, 90, 762, "32204db6360fb4e5"), (422, 40, 24, 75, 1287, "bc42aa3d7f0f7b5e"),
    (422, 100, 83, 50, 4872, "34bc67f851734579"), (422, 208, 132, 100, 68058, "1f5ed2e3fd9ddf2c")])
def test_cross_check_hashes(sampling, pw, ph, quality, size, sha):
    data = file_of(jc.formula(pw, ph), quality, sampling)
    assert len(data) == size and hashlib.sha256(data).hexdigest().startswith(sha)
    head, stream = jpeg.split_file(data)
    assert len(head) == jpeg.HEADER_BYTES == 629 and head + stream == data and jpeg.file_sampling(data) == sampling


def test_the_header_differs_in_three_bytes():
    for pw, ph in ((1, 1), (100, 83), (4112, 8), (65535, 3)):
        heads = {s: jpeg.header(pw, ph, 90, s) for s in (420, 422, 444)}
        assert all(len(h) == 629 for h in heads.values())
        assert [heads[s][169] for s in (420, 422, 444)] == [0x22, 0x21, 0x11]
        for s in (420, 422, 444):
            assert int.from_bytes(heads[s][613:615], "big") == jpeg.mcus(pw, ph, s)[0] and heads[s][609:613] == b"\xFF\xDD\x00\x04"
            assert [k for k in range(629) if heads[s][k] != heads[420][k]] in ([], [169], [169, 614], [169, 613], [169, 613, 614])
    with pytest.raises(ValueError):
        jpeg.header(16, 16, 90, 411)
    with pytest.raises(ValueError):
        jpeg.encode(np.zeros((4, 4, 3), np.uint8), 90, None, 0)
    with pytest.raises(ValueError):
        jpeg.mcus(16, 16, 440)


@pytest.fixture(scope="module")
def traces():
    """every case encoded once: {sampling: [(pw, ph, content, quality, file, trace)]}"""
    out = {}
    for s in sc.SAMPLINGS:
        out[s] = []
        for pw, ph, content, q in sc.all_cases(s):
            tr = {}
            out[s].append((pw, ph, content, q, file_of(content(pw, ph), q, s, tr), tr))
    return out


@pytest.mark.parametrize("sampling", sc.SAMPLINGS)
def test_pil_decodes_every_case(traces, sampling):
    for pw, ph, content, q, data, _ in traces[sampling]:
        with Image.open(io.BytesIO(data)) as im:
            assert im.format == "JPEG" and im.mode == "RGB" and im.size == (pw, ph), (pw, ph, content.__name__, q)
            assert np.asarray(im).shape == (ph, pw, 3)
        assert jpeg.file_sampling(data) == sampling


@pytest.mark.parametrize("sampling", sc.SAMPLINGS)
def test_psnr_against_pils_encoder(sampling):
    """at shapes of at least 17 x 17 among the cases, and the cross-check shapes from 40 x 24 on, on the formula, gradient and noise
    images: decoded by PIL, no more than PSNR_BOUND below PIL's own save(quality=q, subsampling=...) of the same RGB"""
    worst = (-99.0, ())
    todo = [p for p in sc.shapes(sampling) if min(p) >= 17] + sc.PINNED[1:]
    for pw, ph in todo:
        for content in jc.SMOOTH:
            for q in sc.QUALITIES:
                rgb = content(pw, ph)
                b = io.BytesIO()
                Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=PIL_SUBSAMPLING[sampling])
                ours = file_of(rgb, q, sampling)
                short = psnr(rgb, decode(b.getvalue())) - psnr(rgb, decode(ours))
                print(f"{sampling} {pw}x{ph} {content.__name__} q{q}: {short:+.3f} dB below PIL, {len(ours)} against {len(b.getvalue())} bytes")
                worst = max(worst, (short, (pw, ph, content.__name__, q)))
    print("worst shortfall", sampling, worst)
    assert worst[0] <= PSNR_BOUND[sampling], worst


@pytest.mark.parametrize("sampling", sc.SAMPLINGS)
def test_what_the_cases_reach(traces, sampling):
    tr = [t for *_, t in traces[sampling]]
    any_ = lambda key: any(t[key] for t in tr)
    union = lambda key: set().union(*(t[key] for t in tr))
    # both ends of Cb and of Cr before their clamps: 256 above; below, 1 is the lowest value there is (tests/test_jpeg_cases.py)
    for key in ("cb_range", "cr_range"):
        assert min(t[key][0] for t in tr) == 1 and max(t[key][1] for t in tr) == 256, key
    assert union("dc_categories_luma") == set(range(12))
    assert 11 in union("dc_categories_chroma") and 0 in union("dc_categories_chroma")
    # AC category 10 in both tables; the clamp to +-1023 is what no 8-bit block reaches, at any sampling (tests/test_jpeg_cases.py:
    # the largest AC value is 1020), so it stays unreached here as well
    assert 10 in union("ac_categories_luma") and 10 in union("ac_categories_chroma") and not any_("ac_clamped")
    assert any_("zrl") and any_("eob") and any_("no_eob")
    assert union("pads") == set(range(8))
    assert any_("stuffed") and any_("pad_stuffed")
    assert any(t["rows"] >= 10 for t in tr), "the RST index never wraps"
    # edge replication on both axes
    w, h = sc.mcu(sampling)
    pw, ph = w + 1, h + 1
    rgb = jc.noise(pw, ph)
    grown = np.pad(rgb, ((0, 2 * h - ph), (0, 2 * w - pw), (0, 0)), mode="edge")
    assert np.array_equal(jpeg.coefficients(rgb, 90, None, sampling), jpeg.coefficients(grown, 90, None, sampling))
    other = np.pad(rgb, ((0, 2 * h - ph), (0, 2 * w - pw), (0, 0)))
    assert not np.array_equal(jpeg.coefficients(rgb, 90, None, sampling), jpeg.coefficients(other, 90, None, sampling))


def test_rst_indices_wrap_at_every_sampling():
    for s in sc.SAMPLINGS:
        pw, ph = sc.shapes(s)[9]
        stream = jpeg.encode(jc.formula(pw, ph), 90, None, s)
        marks = [stream[k + 1] for k in range(len(stream) - 1) if stream[k] == 0xFF and 0xD0 <= stream[k + 1] <= 0xD7]
        assert marks == [0xD0 + k % 8 for k in range(9)], s


# ------------------------------------------------------------------ wrong definitions
def _coefficients(rgb, quality, sampling, floor=False, chroma_table=1):
    """jpeg.coefficients restated from its parts for 4:2:2 and 4:4:4, with two mistakes to choose from"""
    w, h = sc.mcu(sampling)
    ph, pw = rgb.shape[:2]
    mw, mh = jpeg.mcus(pw, ph, sampling)
    q = jpeg.qtables(quality)
    planes = [np.pad(p, ((0, h * mh - ph), (0, w * mw - pw)), mode="edge") for p in jpeg.ycbcr(rgb)[:3]]
    if sampling == 422:
        planes[1:] = [(p[:, 0::2] + p[:, 1::2] + (0 if floor else 1)) >> 1 for p in planes[1:]]
    blocks = lambda p: p.reshape(mh, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
    y = jpeg.fdct_quantise(blocks(planes[0]), q[0]).reshape(mh, mw, w // 8, 64)
    c = [jpeg.fdct_quantise(blocks(p), q[chroma_table])[:, :, None] for p in planes[1:]]
    return np.concatenate([y] + c, axis=2)[..., jpeg.ZIGZAG]


def _wrong(mp, which, rgb, q, sampling):
    """header + stream of a definition that is wrong in one way"""
    ph, pw = rgb.shape[:2]
    head = jpeg.header(pw, ph, q, sampling)
    right = jpeg.coefficients(rgb, q, None, sampling)
    assert np.array_equal(_coefficients(rgb, q, sampling), right), "the restatement is not the definition"
    ny = right.shape[2] - 2
    if which == "floor":                                   # the 4:2:2 mean without its + 1
        co = _coefficients(rgb, q, sampling, floor=True)
    elif which == "chroma table":                          # chroma quantised with the luminance table
        co = _coefficients(rgb, q, sampling, chroma_table=0)
    elif which == "swap":                                  # Cr in front of Cb
        co = np.concatenate([right[:, :, :ny], right[:, :, ny + 1:], right[:, :, ny:ny + 1]], axis=2)
    elif which == "dri":                                   # the DRI count of 4:2:0
        head = head[:613] + jpeg.header(pw, ph, q, 420)[613:615] + head[615:]
        co = right
    elif which == "y chain":
        # the first Y block of an MCU predicted from the first Y block of the MCU before it, not from the last one: such an encoder
        # writes the differences d'; the right predictor writes exactly those for DC values that are their running sums along the row
        co = right.copy()
        dc = right[:, :, :ny, 0]
        pred = np.zeros_like(dc)
        pred[:, :, 1:] = dc[:, :, :-1]
        pred[:, 1:, 0] = dc[:, :-1, 0]
        co[:, :, :ny, 0] = np.cumsum((dc - pred).reshape(dc.shape[0], -1), axis=1).reshape(dc.shape)
    mp.setattr(jpeg, "coefficients", lambda *a, **k: co)
    return head + jpeg.encode(rgb, q, None, sampling)


@pytest.mark.parametrize("which,samplings", [("floor", (422,)), ("y chain", (422,)), ("swap", (422, 444)), ("dri", (444,)),
                                             ("chroma table", (422, 444))])
def test_wrong_definitions_are_told_apart(monkeypatch, which, samplings):
    """each wrong definition gives other bytes than the right one on at least one case of every sampling it applies to -- so a GPU
    encoder that has the mistake fails tests/test_gpu_jpeg_sampling.py.  (At 4:4:4 an MCU has one Y block: its predictor chains by
    construction, and nothing is averaged.  4:2:2 has the MCU width of 4:2:0 and so its DRI count.)"""
    for s in samplings:
        told = 0
        for pw, ph in sc.shapes(s)[3:6]:
            for ci, content in enumerate(sc.CONTENT[s]):
                rgb = content(pw, ph)
                right = file_of(rgb, 90, s)
                with monkeypatch.context() as mp:
                    wrong = _wrong(mp, which, rgb, 90, s)
                assert file_of(rgb, 90, s) == right, "the definition was not put back"
                told += wrong != right
        assert told >= 3, (which, s, told)


def test_a_wrong_dri_breaks_the_picture():
    """the DRI count of 4:2:0 in a 4:4:4 file: PIL does not give the pixels back"""
    pw, ph, s = 104, 66, 444
    rgb = jc.gradient(pw, ph)
    good = file_of(rgb, 90, s)
    bad = good[:613] + jpeg.header(pw, ph, 90, 420)[613:615] + good[615:]
    assert bad != good and psnr(rgb, decode(good)) > 30
    try:
        broken = psnr(rgb, decode(bad)) < 20
    except OSError:
        broken = True
    assert broken
