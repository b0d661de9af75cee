"""mlvfs_amd_mlv_transcode (csrc/mlvwriter.cpp), the part that needs no GPU: a plain or LZMA clip written again with plain packed
payloads is host code from the container walk to the last write.

What is checked: the output's block sequence per chunk (the source's, in file order, without NULL and XREF blocks), every block
byte for byte except MLVI's video class and VIDF's frameSpace / blockSize, every payload against the frame it was packed from, the
reference's own reader + process_frame text (oracle/_ref/ref_host_ref) serving the output exactly as it serves the source, the
refusals (nothing is overwritten, nothing is left behind), damaged sources, and all of it once more under the address and
undefined-behaviour sanitizers (the pattern of tests/test_hostcheck.py).  The GPU paths: tests/test_gpu_mlv_transcode.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from test_gpu_ref_host import H, W, make_clip, need_hosts, run_host, vpath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "M07-1234.MLV"


def blocks_of(path):
    """[(tag, whole block)] of one chunk file, in file order."""
    data, pos, out = open(path, "rb").read(), 0, []
    while pos + 16 <= len(data):
        size = struct.unpack_from("<I", data, pos + 4)[0]
        assert 16 <= size <= len(data) - pos, (path, pos, size)
        out.append((data[pos:pos + 4], data[pos:pos + size]))
        pos += size
    assert pos == len(data), path
    return out


def chunk_names(first, n):
    return [first] + [first[:-2] + "%02d" % i for i in range(n - 1)]


def video_class(block):
    return struct.unpack_from("<H", block, 32)[0]


def vidf_fields(block):
    frame, _, _, _, _, space = struct.unpack_from("<IHHHHI", block, 16)
    return frame, space


def raw_transcode(reader, out_path, payload, batch=0, io_threads=0, stats=True):
    L = lib.load()
    st = (C.c_longlong * 4)(-1, -1, -1, -1)
    rc = L.mlvfs_amd_mlv_transcode(reader, None if out_path is None else os.fsencode(out_path), payload, batch, io_threads, st if stats else None)
    return rc, list(st), L.mlvfs_amd_last_error().decode()


def check_container(src_first, out_first, nchunks, want_class, payload_of):
    """Block sequence and bytes of every output chunk against its source chunk; payload_of(frame number, payload bytes) checks a VIDF
    payload.  Returns (video frames, payload bytes in the source, payload bytes in the output)."""
    frames = bytes_in = bytes_out = 0
    for s, o in zip(chunk_names(src_first, nchunks), chunk_names(out_first, nchunks)):
        src = [b for b in blocks_of(s) if b[0] not in (b"NULL", b"XREF")]
        out = blocks_of(o)
        assert [t for t, _ in out] == [t for t, _ in src], o
        for (tag, a), (_, b) in zip(src, out):
            if tag == b"MLVI":
                assert video_class(b) == want_class and a[:32] == b[:32] and a[34:] == b[34:], o
            elif tag == b"VIDF":
                (k, space), (k2, space2) = vidf_fields(a), vidf_fields(b)
                assert k2 == k and space2 == 0 and a[8:28] == b[8:28], (o, k)            # timestamp, number, crop and pan
                payload_of(k, b[32:])
                frames += 1
                bytes_in += len(a) - 32 - space
                bytes_out += len(b) - 32
            else:
                assert a == b, (o, tag)
    return frames, bytes_in, bytes_out


@pytest.mark.parametrize("kind", ["plain", "lzma"])
def test_plain_output_of_a_plain_or_lzma_clip(request, tmp_path, kind):
    reference = request.getfixturevalue("reference") if kind == "lzma" else None
    d, frames = make_clip(tmp_path, kind, reference=reference)
    assert any(t == b"NULL" for n in chunk_names(str(d / NAME), 2) for t, _ in blocks_of(n))
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(str(d / NAME)) as r:
        stats = r.transcode(str(out / NAME), lj92=False, batch=2, io_threads=2)
    assert sorted(os.listdir(out)) == [NAME[:-2] + "00", NAME]
    nbytes = (W * H * 14 + 7) // 8

    def payload_of(k, p):
        assert len(p) == (nbytes + 1) // 2 * 2 and p[:nbytes] == synth.pack_bits(frames[k]).tobytes()[:nbytes], k

    seen = check_container(str(d / NAME), str(out / NAME), 2, 1, payload_of)
    assert seen[0] == len(frames)
    assert stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)
    with mlvfile.MlvReader(str(out / NAME)) as r:
        assert r.frame_count == len(frames) and r.chunk_count == 2
        got = r.read_frames(0, len(frames), nbytes + 16)
        for k, f in enumerate(frames):
            assert got[k, :nbytes].tobytes() == synth.pack_bits(f).tobytes()[:nbytes], k


@pytest.mark.parametrize("kind", ["plain", "lzma"])
def test_the_reference_text_serves_the_output_as_it_serves_the_source(request, tmp_path, kind):
    need_hosts()
    reference = request.getfixturevalue("reference") if kind == "lzma" else None
    d, _ = make_clip(tmp_path, kind, reference=reference)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(str(d / NAME)) as r:
        r.transcode(str(out / NAME), lj92=False)
    order = [vpath(2), vpath(0), vpath(4)]
    want, _ = run_host("ref", d, tmp_path / "src", dict(cs=2), order)
    got, _ = run_host("ref", out, tmp_path / "dst", dict(cs=2), order)
    assert got == want


def small_clip(path, w=64, h=48, n=5, **kw):
    frames = [synth.normal_frame(w, h, seed=3, frame=k) for k in range(n)]
    return mlvfile.write_clip(str(path), [synth.pack_bits(f).tobytes() for f in frames], w, h, **kw), frames


def test_refusals_leave_nothing_behind(tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    names, _ = small_clip(src / "A.MLV", chunks=2)
    before = {n: open(n, "rb").read() for n in names}
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(names[0]) as r:
        # nothing is overwritten: the first chunk, a later chunk, an index of whatever clip had this name
        for existing in ("B.MLV", "B.M00", "B.IDX"):
            (out / existing).write_bytes(b"mine")
            rc, stats, err = raw_transcode(r.h, str(out / "B.MLV"), lib.MLV_PLAIN)
            assert rc == lib.ERR_ARG and "exists" in err and stats == [0, 0, 0, 0], existing
            assert os.listdir(out) == [existing] and (out / existing).read_bytes() == b"mine"
            os.remove(out / existing)
        # the source itself, under its own name and under another one
        rc, _, err = raw_transcode(r.h, names[0], lib.MLV_PLAIN)
        assert rc == lib.ERR_ARG and "source" in err
        os.symlink(names[1], out / "C.M00")
        rc, _, err = raw_transcode(r.h, str(out / "C.MLV"), lib.MLV_PLAIN)
        assert rc == lib.ERR_ARG and "source" in err
        os.remove(out / "C.M00")
        for bad in ("B.RAW", "B.MLV.bak", "MLV"):
            assert raw_transcode(r.h, str(out / bad), lib.MLV_PLAIN)[0] == lib.ERR_ARG, bad
        assert raw_transcode(r.h, str(out / "B.mlv"), 7)[0] == lib.ERR_ARG                  # no such payload kind
        assert raw_transcode(None, str(out / "B.MLV"), lib.MLV_PLAIN)[0] == lib.ERR_ARG
        assert raw_transcode(r.h, None, lib.MLV_PLAIN)[0] == lib.ERR_ARG
        assert raw_transcode(r.h, str(out / "B.MLV"), lib.MLV_PLAIN, stats=False)[0] == lib.ERR_ARG
    assert os.listdir(out) == [] and sorted(os.listdir(src)) == ["A.M00", "A.MLV"]
    assert {n: open(n, "rb").read() for n in names} == before
    # LJ92 output of odd sizes: the reference's quadrant map is no bijection there; refused before any device work
    for w, h in ((417, 264), (416, 263)):
        d = tmp_path / f"odd{w}x{h}"
        d.mkdir()
        names, _ = small_clip(d / "O.MLV", w=w, h=h, n=2)
        with mlvfile.MlvReader(names[0]) as r:
            rc, _, err = raw_transcode(r.h, str(out / "O.MLV"), lib.MLV_LJ92)
            assert rc == lib.ERR_ARG and "even" in err, (w, h, err)
            assert os.listdir(out) == []
            assert r.transcode(str(out / "O.MLV"), lj92=False)["frames"] == 2                # plain output takes any size
        os.remove(out / "O.MLV")


def test_other_video_classes_are_refused(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    for vc in (2, 1 | 0x40, 3 | 0x100):                                                     # YUV, raw with DELTA, JPEG
        d = tmp_path / f"vc{vc}"
        d.mkdir()
        names, _ = small_clip(d / "V.MLV", n=2, video_class=vc)
        with mlvfile.MlvReader(names[0]) as r:
            for payload in (lib.MLV_PLAIN, lib.MLV_LJ92):
                rc, _, err = raw_transcode(r.h, str(out / "V.MLV"), payload)
                assert rc == lib.ERR_ARG and "video class" in err, (vc, err)
        assert os.listdir(out) == []


def test_a_source_truncated_inside_a_payload(tmp_path):
    names, _ = small_clip(tmp_path / "T.MLV", chunks=2)
    assert blocks_of(names[0])[-1][0] == b"VIDF"
    data = open(names[0], "rb").read()
    open(names[0], "wb").write(data[:-100])
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(names[0]) as r:
        rc, stats, err = raw_transcode(r.h, str(out / "T.MLV"), lib.MLV_PLAIN)
    assert rc != 0 and err and stats == [0, 0, 0, 0]
    assert os.listdir(out) == []


def test_files_that_cannot_be_read_or_created_are_io_errors(tmp_path):
    """Not argument errors: a block that ends behind the end of its file (the index lists it, the copy cannot read it) and an output
    file that cannot be created."""
    names, _ = small_clip(tmp_path / "S.MLV", chunks=2)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(names[0]) as r:
        rc, stats, err = raw_transcode(r.h, str(tmp_path / "no_such_directory" / "S.MLV"), lib.MLV_PLAIN)
        assert rc == lib.ERR_IO and "cannot create" in err and stats == [0, 0, 0, 0], err
    open(names[1], "ab").write(b"INFO" + struct.pack("<IQ", 64, 10 ** 9) + b"short")
    with mlvfile.MlvReader(names[0]) as r:
        rc, stats, err = raw_transcode(r.h, str(out / "S.MLV"), lib.MLV_PLAIN)
        assert rc == lib.ERR_IO and "short read in the INFO block" in err and stats == [0, 0, 0, 0], err
    assert os.listdir(out) == []                                          # the first chunk had been written in full by then


def test_device_entry_points_check_their_arguments_before_any_device_work():
    """mlvfs_amd_lj92_tile_dev and mlvfs_amd_pack_dev refuse on the host: no HIP device is needed (and under the sanitizer build a
    launcher would abort).  The pointers are never followed."""
    L = lib.load()
    a, b = np.zeros(4096, np.uint16), np.full(4096, 7, np.uint16)
    pa, pb = lib.ptr(a), lib.ptr(b)
    tile = L.mlvfs_amd_lj92_tile_dev
    for w, h in ((3, 2), (2, 3), (5, 5), (417, 264), (416, 263), (0, 2), (2, -2), (1 << 14, 1 << 13)):
        assert tile(pa, 0, pb, 0, w, h, 1, None) == lib.ERR_ARG, (w, h)
    assert b"odd sizes" in L.mlvfs_amd_last_error() or b"not supported" in L.mlvfs_amd_last_error()
    assert tile(pa, 0, pa, 0, 16, 4, 1, None) == lib.ERR_ARG                                  # not in place
    assert tile(None, 0, pb, 0, 16, 4, 1, None) == lib.ERR_ARG and tile(pa, 0, None, 0, 16, 4, 1, None) == lib.ERR_ARG
    assert tile(pa, 64, pb, 256, 16, 4, 2, None) == lib.ERR_ARG and tile(pa, 256, pb, 64, 16, 4, 2, None) == lib.ERR_ARG   # frames that overlap
    assert tile(pa, 129, pb, 128, 16, 4, 2, None) == lib.ERR_ARG                              # an odd stride
    assert tile(C.c_void_p(a.ctypes.data + 1), 0, pb, 0, 16, 4, 1, None) == lib.ERR_ARG
    assert tile(pa, 0, pb, 0, 16, 4, -1, None) == lib.ERR_ARG and tile(pa, 0, pb, 0, 16, 4, 0, None) == 0
    pack = L.mlvfs_amd_pack_dev
    for w, h, bpp in ((16, 4, 0), (16, 4, 17), (16, 4, -3), (0, 4, 14), (16, -1, 14), (1 << 14, 1 << 13, 14)):
        assert pack(C.byref(lib.Geom(w, h, bpp, 0, 0, 0, 0)), pa, 0, pb, 0, 1, None) == lib.ERR_ARG, (w, h, bpp)
    g = C.byref(lib.Geom(16, 4, 14, 0, 0, 0, 0))
    assert pack(None, pa, 0, pb, 0, 1, None) == lib.ERR_ARG and pack(g, None, 0, pb, 0, 1, None) == lib.ERR_ARG
    assert pack(g, pa, 0, None, 0, 1, None) == lib.ERR_ARG
    assert pack(g, pa, 128, pb, 110, 2, None) == lib.ERR_ARG and pack(g, pa, 126, pb, 112, 2, None) == lib.ERR_ARG          # 112 bytes packed, 128 of pixels
    assert pack(g, pa, 128, pb, 113, 2, None) == lib.ERR_ARG
    assert pack(g, pa, 128, pb, 112, -1, None) == lib.ERR_ARG and pack(g, pa, 128, pb, 112, 0, None) == 0
    assert not a.any() and (b == 7).all()


def test_transcode_survives_mutated_sources(tmp_path):
    """Random damage to block headers (the pattern of tests/test_mlv_reader.py): the call answers -- every file it names is there and
    can be walked -- or refuses and leaves nothing."""
    src = tmp_path / "src"
    src.mkdir()
    names, _ = small_clip(src / "F.MLV", n=6, chunks=2, frame_space=16)
    good = [open(n, "rb").read() for n in names]
    rng = np.random.default_rng(5)
    out = tmp_path / "out"
    answered = refused = 0
    for _ in range(120):
        for n, g in zip(names, good):
            b = bytearray(g)
            for _ in range(int(rng.integers(1, 8))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            if rng.integers(0, 4) == 0:
                b = b[: int(rng.integers(16, len(b)))]
            open(n, "wb").write(bytes(b))
        out.mkdir()
        try:
            with mlvfile.MlvReader(names[0]) as r:
                rc, stats, _ = raw_transcode(r.h, str(out / "G.MLV"), lib.MLV_PLAIN, batch=int(rng.integers(1, 5)))
                if rc == 0:
                    answered += 1
                    made = sorted(os.listdir(out))
                    assert len(made) == stats[3] == r.chunk_count and made == sorted(os.path.basename(n) for n in chunk_names(str(out / "G.MLV"), stats[3]))
                    assert sum(t == b"VIDF" for n in made for t, _ in blocks_of(str(out / n))) == stats[0]
                else:
                    refused += 1
                    assert os.listdir(out) == []
        except lib.MlvfsAmdError:
            pass                                                                           # the clip does not open at all
        shutil.rmtree(out)
    assert answered > 10 and refused > 10, (answered, refused)


def _asan():
    r = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True)
    p = r.stdout.strip()
    return p if r.returncode == 0 and os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(os.environ.get("MLVFS_AMD_LIB") is not None, reason="this is the child")
def test_this_file_under_address_and_undefined_behaviour_sanitizers():
    """The tests above once more against libmlvfs_amd_hostcheck.so (g++ -fsanitize=address,undefined, kernel launchers replaced by
    aborting stubs): the writer's host path must neither trip a sanitizer nor reach device code."""
    asan = _asan()
    if asan is None:
        pytest.skip("gcc's libasan.so not found")
    so = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)
    assert b.returncode == 0 and os.path.exists(so), b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, MLVFS_AMD_LIB=so, LD_PRELOAD=asan,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider", "tests/test_mlv_transcode.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert "device code called" not in r.stderr, tail
    assert r.returncode == 0 and " passed" in r.stdout and " failed" not in r.stdout, tail
