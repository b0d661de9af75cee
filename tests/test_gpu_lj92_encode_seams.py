"""The batched LJ92 encoder (csrc/k_lj92enc.hip, csrc/lj92enc.cpp) at the cases of tests/lj92_encode_cases.py, byte for byte against
the reference's own encoder (the oracle's restatement where the stream is longer than the reference's room): block seams at every
bit phase inside a 0xFF byte, last blocks of a few bits, class-0 codes of up to 16 one-bits (k_lje_stuff's LDS at its fullest), narrow
and odd widths, frames at an odd 16-bit offset, 1023 to 2049 blocks, refused frames between good ones, and a room that fits to the
byte.  tests/test_lj92_encode_cases.py shows on the CPU that the cases reach all that.

Every case goes through lj92.encode_batch as a batch of one; the small ones also through the single-frame lj92_encode, whose room is
sized for the worst case and is exact for a stream of 0xFF bytes.  The mixed batch and the room cases call
mlvfs_amd_lj92_encode_batch_dev on a PAD-filled buffer: behind a stream's length, in the whole room of a refused frame and behind the
last room no byte may change."""
import ctypes as C

import numpy as np
import pytest

import lj92_encode_cases as ec
from lossless_cases import max_class
from mlvfs_amd import lib, lj92
from test_gpu_lj92_shapes import decode_raw_batch

pytestmark = pytest.mark.gpu

PAD, GUARD = 0xA5, 256


def device_frames(frames, lead=0, pad=0):
    """An (n, h, w) view of the frames in one device buffer: `lead` 16-bit words in front of the first, `pad` between two"""
    import torch
    n = len(frames)
    h, w = frames[0].shape
    per = w * h + pad
    buf = torch.full((lead + n * per,), 0x5A5A, dtype=torch.int16, device="cuda")
    for k, f in enumerate(frames):
        buf[lead + k * per:lead + k * per + w * h] = torch.from_numpy(np.ascontiguousarray(f).view(np.int16).reshape(-1)).cuda()
    return torch.as_strided(buf, (n, h, w), (per, w, 1), lead)


def encode_into_pad(gpu, frames, bits, room):
    """mlvfs_amd_lj92_encode_batch_dev into a PAD-filled buffer of n rooms and a guard -> lengths, status, classes, the rooms, the guard"""
    import torch
    n, h, w = frames.shape
    out = torch.full((n * room + GUARD,), PAD, dtype=torch.uint8, device="cuda")
    lengths, status, classes = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.check(gpu.mlvfs_amd_lj92_encode_batch_dev(C.c_void_p(frames.data_ptr()), frames.stride(0) * 2, n, w, h, bits, C.c_void_p(out.data_ptr()),
                                                  room, lib.ptr(lengths), lib.ptr(status), lib.ptr(classes), None), "lj92_encode_batch_dev")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return [int(v) for v in lengths], [int(v) for v in status], [int(v) for v in classes], got[:n * room].reshape(n, room), got[n * room:]


def check_rooms(cases, wants, lengths, status, classes, rooms, guard, expect):
    assert status == expect, (status, expect)
    assert (guard == PAD).all(), "written behind the last room"
    for k, c in enumerate(cases):
        if expect[k] != lj92.STATUS_OK:
            assert lengths[k] == 0 and (rooms[k] == PAD).all(), f"{c.name}: a refused frame's room was written to"
            continue
        assert lengths[k] == len(wants[k]) and rooms[k, :lengths[k]].tobytes() == wants[k], (c.name, lengths[k], len(wants[k]))
        assert (rooms[k, lengths[k]:] == PAD).all(), f"{c.name}: written behind the stream's length"
        assert classes[k] == max_class(wants[k]), c.name


@pytest.mark.parametrize("case", ec.CASES, ids=[c.name.replace(" ", "-") for c in ec.CASES])
def test_case_equals_the_reference_encoder(gpu, oracle, reference, case):
    img = ec.image(case)
    want = ec.want(case, oracle, reference)
    assert want is not None
    for lead in ((0,) if case.cls == "blocks" else (0, 1)):                 # 16-byte aligned, and at an odd 16-bit offset
        streams, classes, status = lj92.encode_batch(device_frames([img], lead), bits=case.bits)
        assert status == [lj92.STATUS_OK], (case.name, lead, status)
        assert len(streams[0]) == len(want) and streams[0] == want, (case.name, lead, len(streams[0]), len(want))
        assert classes == [max_class(want)], (case.name, lead)
    if case.cls != "blocks":                                                # the drop-in: a batch of one in a room of the worst case
        got = lj92.encode(img, case.w, case.h, case.bits)
        assert len(got) == len(want) and got == want, (case.name, len(got), len(want))


def test_mixed_batch_refusals_leave_their_neighbours_alone(gpu, oracle, reference):
    cases = ec.MIXED
    wants = [ec.want(c, oracle, reference) for c in cases]
    room = ec.mixed_room([len(s or b"") for s in wants])
    expect = [{None: lj92.STATUS_OK, "diff17": lj92.STATUS_DIFF17, "table": lj92.STATUS_TABLE}[c.refused] for c in cases]
    expect[ec.MIXED_NOFIT] = lj92.STATUS_NOFIT
    assert len(wants[ec.MIXED_NOFIT]) > room
    frames = [ec.image(c) for c in cases]
    for lead, pad in ((0, 0), (1, 49)):
        lengths, status, classes, rooms, guard = encode_into_pad(gpu, device_frames(frames, lead, pad), 16, room)
        check_rooms(cases, wants, lengths, status, classes, rooms, guard, expect)
        assert classes[1] == 17 and classes[4] == 16 and classes[ec.MIXED_NOFIT] == max_class(wants[ec.MIXED_NOFIT])
    # with room for it the frame that did not fit is encoded like the others
    streams, classes, status = lj92.encode_batch(device_frames(frames, 1, 49), bits=16)
    assert status == [lj92.STATUS_OK if c.refused is None else expect[k] for k, c in enumerate(cases)]
    assert streams == wants


def test_a_stream_fits_its_room_to_the_byte(gpu, oracle, reference):
    tight, short = ec.ROOM
    L = len(ec.want(tight, oracle, reference))
    assert L % 4 == 0
    for cases in ([tight, short], [short, tight]):
        wants = [ec.want(c, oracle, reference) for c in cases]
        frames = device_frames([ec.image(c) for c in cases], 0, 8)
        for room, fits in ((L, True), (L - 4, False)):
            expect = [lj92.STATUS_OK if fits or c is short else lj92.STATUS_NOFIT for c in cases]
            lengths, status, classes, rooms, guard = encode_into_pad(gpu, frames, tight.bits, room)
            check_rooms(cases, wants, lengths, status, classes, rooms, guard, expect)


def test_a_deep_stream_decodes_back_on_the_gpu(gpu, oracle, reference):
    """16 one-bits for class 0: the library's own decoder (mlvfs_amd_lj92_decode_dev, the decoder's own order) gives the image back"""
    case = next(c for c in ec.DEEP if c.bits == 16)
    img = ec.image(case)
    streams, _, status = lj92.encode_batch(device_frames([img]), bits=16)
    assert status == [0] and streams[0] == ec.want(case, oracle, reference)
    assert np.array_equal(decode_raw_batch(gpu, [streams[0]], [(case.h, case.w)])[0], img)
