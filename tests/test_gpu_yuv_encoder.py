"""GPU parity (-m gpu) of YUV 4:2:0 input: the unpack kernel (transforms.hip k_unpack_yuv420, fuifgpu_unpack_yuv420) against numpy, and
the writer's two GPU routes (fuifgpu_encode_yuv420 with gpu_forward, and with the frames in device memory).

The yardstick is the reference CLI's bytes (tests/golden/yuv/, written by the unmodified `fuif -I 0 -K 0 -X 0 -Y 0 -y WxH[:b] ...`, see
tests/golden/make_golden_yuv.py) and, for learned trees, the host writer that tests/test_writer_yuv.py pins to the same files.
On a machine without a GPU tests/test_writer_yuv.py runs this file against the wavefront emulator build."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd.synth import yuv420_frame, yuv420_planes

pytestmark = pytest.mark.gpu

EMULATED = ("_emu" in os.path.basename(os.environ.get("FUIF_AMD_LIB", "")))
YUV = os.path.join(GOLDEN, "yuv")
with open(os.path.join(YUV, "manifest_yuv.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
if EMULATED:
    FIXTURES = [e for e in FIXTURES if e["name"] in ("yuv8_97x61_Q80", "yuv8_97x61_R0", "yuv8_200x9_Q0", "yuv8_5x4", "yuv8_6x4", "yuv8_1x1", "yuv8_2x2",
                                                     "yuv12_41x37_Q50", "yuv8_96x60x3_M0_F25_Q70")]
IDS = [e["name"] for e in FIXTURES]
E_ARG = 4
GUARD_BYTE, GUARD_WORD = 0xA5, -123456789


class DevBytes:
    """bytes in device memory through the library's own allocator (host memory under the emulator)"""

    def __init__(self, gpulib, nbytes):
        self.L = gpulib.lib()
        self.n = max(int(nbytes), 16)
        self.ptr = self.L.fuifgpu_dev_alloc(self.n)
        assert self.ptr

    def put(self, arr):
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert a.size <= self.n
        assert self.L.fuifgpu_dev_upload(self.ptr, a.ctypes.data, a.size) == 0
        return self

    def get(self, nbytes, dtype=np.uint8):
        out = np.empty(nbytes, np.uint8)
        assert self.L.fuifgpu_dev_download(out.ctypes.data, self.ptr, nbytes) == 0   # (synchronises with the null stream's kernels)
        return out.view(dtype)

    def free(self):
        self.L.fuifgpu_dev_free(self.ptr)


def raw_frame(planes, bits, layout, pad):
    """(bytes, pitch_y, pitch_c) of one frame whose rows are `pad` bytes longer than their samples (padding: GUARD_BYTE); the frame ends
    with its last sample"""
    y, cb, cr = planes
    dt = np.uint8 if bits <= 8 else np.dtype("<u2")
    parts = [y, cb, cr] if layout == "i420" else [y, np.stack([cb, cr], axis=-1).reshape(cb.shape[0], -1)]
    out, pitches = [], []
    for p in parts:
        rows = np.ascontiguousarray(p.astype(dt)).view(np.uint8).reshape(p.shape[0], -1)
        padded = np.full((rows.shape[0], rows.shape[1] + pad), GUARD_BYTE, np.uint8)
        padded[:, : rows.shape[1]] = rows
        out.append(padded.reshape(-1))
        pitches.append(rows.shape[1] + pad)
    raw = np.concatenate(out)
    return raw[: raw.size - pad], pitches[0], pitches[-1]


WIDTHS = [1, 3, 5, 65, 97] if EMULATED else [1, 2, 3, 4, 5, 63, 64, 65, 97, 255, 256, 257]
HEIGHTS = [1, 3, 18] if EMULATED else [1, 2, 3, 18]      # (18: every one of a wavefront's four rows, and a second block)
PADS = [0, 3] if EMULATED else [0, 1, 3, 6]


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("bits", [8, 10])
def test_unpack_against_numpy(gpulib, bits, layout):
    """every width around the vector, the wavefront and the row segment; rows and frame bases on every byte alignment; the bytes in front of,
    between and behind the rows and the words around every output plane stay what they were; odd sizes: chroma is (w+1)/2 x (h+1)/2"""
    L = gpulib.lib()
    maxval = (1 << bits) - 1
    skews = ([0, 1] if EMULATED else [0, 1, 2, 3]) if bits == 8 else ([0, 2] if EMULATED else [0, 1, 2])
    src = DevBytes(gpulib, 64 + 4 + 3 * 2 * (max(WIDTHS) + 8) * max(HEIGHTS))
    outs = [DevBytes(gpulib, 4 * (max(WIDTHS) * max(HEIGHTS) + 16)) for _ in range(3)]
    flag = DevBytes(gpulib, 4)
    rng = np.random.default_rng(bits * 10 + len(layout))
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                cw, ch = (w + 1) // 2, (h + 1) // 2
                planes = [rng.integers(0, maxval + 1, size=s).astype(np.int32) for s in ((h, w), (ch, cw), (ch, cw))]
                planes[0][-1, -1] = maxval                       # a sample AT the maximum leaves the flag alone
                for pad in PADS:
                    raw, py, pc = raw_frame(planes, bits, layout, pad)
                    for skew in skews:
                        front = 32 + skew
                        buf = np.concatenate([np.full(front, GUARD_BYTE, np.uint8), raw, np.full(32, GUARD_BYTE, np.uint8)])
                        src.put(buf)
                        lead = 4 + (pad & 1)                     # output planes on and off a 16-byte boundary
                        for o, p in zip(outs, planes):
                            o.put(np.full(p.size + lead + 4, GUARD_WORD, np.int32))
                        flag.put(np.zeros(1, np.int32))
                        yuv = gpulib.make_yuv_options(layout, py if pad else 0, pc if pad else 0)
                        rc = L.fuifgpu_unpack_yuv420(src.ptr + front, w, h, bits, C.byref(yuv), outs[0].ptr + 4 * lead, outs[1].ptr + 4 * lead,
                                                     outs[2].ptr + 4 * lead, flag.ptr, None)
                        case = (w, h, bits, layout, pad, skew)
                        assert rc == 0, case
                        for o, p in zip(outs, planes):
                            got = o.get(4 * (p.size + lead + 4), np.int32)
                            assert np.array_equal(got[lead: lead + p.size].reshape(p.shape), p), case
                            assert (got[:lead] == GUARD_WORD).all() and (got[lead + p.size:] == GUARD_WORD).all(), ("words around a plane", case)
                        assert flag.get(4, np.int32)[0] == 0, case
                        assert np.array_equal(src.get(buf.size), buf), ("the frame was written", case)
    finally:
        for d in [src, flag] + outs:
            d.free()


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_unpack_flags_samples_above_the_maximum(gpulib, layout):
    L = gpulib.lib()
    w, h, bits = 70, 5, 10
    cw, ch = 35, 3
    base = [np.full(s, 1023, np.int32) for s in ((h, w), (ch, cw), (ch, cw))]      # every sample AT the maximum: no flag
    src, flag = DevBytes(gpulib, 4096), DevBytes(gpulib, 4)
    outs = [DevBytes(gpulib, 4 * w * h) for _ in range(3)]
    try:
        def run(planes, flag_ptr, pad=0):
            raw, py, pc = raw_frame(planes, bits, layout, pad)
            src.put(raw)
            flag.put(np.zeros(1, np.int32))
            yuv = gpulib.make_yuv_options(layout, py if pad else 0, pc if pad else 0)
            assert L.fuifgpu_unpack_yuv420(src.ptr, w, h, bits, C.byref(yuv), outs[0].ptr, outs[1].ptr, outs[2].ptr, flag_ptr, None) == 0
            return int(flag.get(4, np.int32)[0])

        assert run(base, flag.ptr) == 0
        # one sample above, in each plane: first sample, the last sample of a row (the last lane that has one), the frame's last sample
        for plane in range(3):
            for at in ((0, 0), (1, -1), (-1, -1), (2, 33)):
                for pad in (0, 2, 3):
                    bad = [p.copy() for p in base]
                    bad[plane][at] = 1024
                    assert run(bad, flag.ptr, pad) != 0, (plane, at, pad)
                    assert np.array_equal(outs[plane].get(4 * bad[plane].size, np.int32).reshape(bad[plane].shape), bad[plane])
        bad = [p.copy() for p in base]
        bad[1][0, 0] = 65535
        assert run(bad, None) == 0                     # flag_device = NULL is accepted (and nothing is reported)
        # w * h == 0 touches nothing and needs nothing
        assert L.fuifgpu_unpack_yuv420(None, 0, 5, 8, None, None, None, None, None, None) == 0
        assert L.fuifgpu_unpack_yuv420(None, 5, 0, 8, None, None, None, None, None, None) == 0
        yuv = gpulib.make_yuv_options("i420")
        assert L.fuifgpu_unpack_yuv420(None, 5, 4, 8, C.byref(yuv), outs[0].ptr, outs[1].ptr, outs[2].ptr, None, None) == E_ARG
        assert L.fuifgpu_unpack_yuv420(src.ptr, 5, 4, 15, C.byref(yuv), outs[0].ptr, outs[1].ptr, outs[2].ptr, None, None) == E_ARG
        assert L.fuifgpu_unpack_yuv420(src.ptr, 5, 4, 8, C.byref(gpulib.make_yuv_options("i420", pitch_y=4)), outs[0].ptr, outs[1].ptr, outs[2].ptr, None, None) == E_ARG
    finally:
        for d in [src, flag] + outs:
            d.free()


def fixture_clip(entry, layout="i420", pad=0):
    s = entry["synth"]
    bps = 2 if s["bits"] > 8 else 1
    cw = (s["w"] + 1) // 2
    pitch = None if not pad else (s["w"] * bps + pad, cw * bps * (2 if layout == "nv12" else 1) + pad)
    raw = b"".join(yuv420_frame(s["w"], s["h"], s["bits"], s["seed"] + f, layout=layout, pitch=pitch) for f in range(s["frames"]))
    kw = dict(w=s["w"], h=s["h"], bit_depth=s["bits"], layout=layout)
    if pitch:
        kw.update(pitch_y=pitch[0], pitch_c=pitch[1])
    if s["frames"] > 1:
        kw.update(nb_frames=s["frames"])
    return raw, kw


def encode_on_device(gpulib, raws, skew=0, **kw):
    """the frames in device memory (skew bytes off the allocator's alignment), encoded there; also checks that they were not written"""
    devs = [DevBytes(gpulib, len(r) + skew).put(np.concatenate([np.zeros(skew, np.uint8), np.frombuffer(r, np.uint8)])) for r in raws]
    try:
        blobs = gpulib.encode_yuv420_device([d.ptr + skew for d in devs], **kw)
        for d, r in zip(devs, raws):
            assert d.get(len(r) + skew)[skew:].tobytes() == r, "the caller's frame was written"
        return blobs
    finally:
        for d in devs:
            d.free()


def _same_up_to_the_stray_byte(mine, theirs):
    return mine == theirs[: len(mine)] and 0 <= len(theirs) - len(mine) <= 1


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_gpu_routes_write_the_reference_clis_bytes(gpulib, entry):
    theirs = open(os.path.join(YUV, entry["file"]), "rb").read()
    raw, kw = fixture_clip(entry)
    mine = gpulib.encode_yuv420_batch([raw], tree_mode=0, gpu_forward=True, gpu_entropy=True, **kw, **entry["encode"])[0]
    assert _same_up_to_the_stray_byte(mine, theirs), entry["name"]
    assert encode_on_device(gpulib, [raw], tree_mode=0, **kw, **entry["encode"]) == [mine], entry["name"]
    # the same samples as NV12, and (single frames) in padded rows
    nv, nkw = fixture_clip(entry, "nv12")
    assert encode_on_device(gpulib, [nv], skew=1 if entry["synth"]["bits"] == 8 else 2, tree_mode=0, **nkw, **entry["encode"]) == [mine], entry["name"]
    assert gpulib.encode_yuv420_batch([nv], tree_mode=0, gpu_forward=True, **nkw, **entry["encode"]) == [mine], entry["name"]
    if entry["synth"]["frames"] == 1:
        pad = 5 if entry["synth"]["bits"] == 8 else 6
        pr, pkw = fixture_clip(entry, "i420", pad)
        assert gpulib.encode_yuv420_batch([pr], tree_mode=0, gpu_forward=True, gpu_entropy=True, **pkw, **entry["encode"]) == [mine], entry["name"]
        pn, pnkw = fixture_clip(entry, "nv12", pad)
        assert encode_on_device(gpulib, [pn], tree_mode=0, **pnkw, **entry["encode"]) == [mine], entry["name"]


SHAPES = [(97, 61, 8, {}), (75, 49, 10, {}), (64, 48, 8, dict(quality=80))] if EMULATED else [(97, 61, 8, {}), (75, 49, 10, {}), (256, 192, 8, dict(quality=80))]


@pytest.mark.parametrize("w,h,bits,kw", SHAPES)
def test_host_gpu_forward_and_device_routes_agree_with_learned_trees(gpulib, w, h, bits, kw):
    raw = yuv420_frame(w, h, bits, 9000 + w)
    split = 2 if w * h < 20000 else None       # small pictures: let the learner split at all
    host = gpulib.encode_yuv420(raw, w, h, bits, tree_mode=1, index=True, split_bits=split, **kw)
    if w * h >= 20000:                         # (channels of fewer than 4096 samples learn no tree: the small shapes check the routes, this one the learner's samples)
        assert host != gpulib.encode_yuv420(raw, w, h, bits, tree_mode=0, index=True, **kw)
    for gpu in (dict(gpu_forward=True), dict(gpu_entropy=True), dict(gpu_forward=True, gpu_entropy=True)):
        assert gpulib.encode_yuv420(raw, w, h, bits, tree_mode=1, index=True, split_bits=split, **gpu, **kw) == host, gpu
    assert encode_on_device(gpulib, [raw], w=w, h=h, bit_depth=bits, tree_mode=1, index=True, split_bits=split, **kw) == [host]


def test_a_batch_of_three_frames_in_one_call(gpulib):
    raws = [yuv420_frame(97, 61, 8, 9100 + k) for k in range(3)]
    host = [gpulib.encode_yuv420(r, 97, 61, tree_mode=1, index=True, split_bits=2) for r in raws]
    assert len(set(host)) == 3
    assert gpulib.encode_yuv420_batch(raws, 97, 61, tree_mode=1, index=True, split_bits=2) == host
    assert gpulib.encode_yuv420_batch(raws, 97, 61, tree_mode=1, index=True, split_bits=2, gpu_forward=True, gpu_entropy=True) == host
    assert encode_on_device(gpulib, raws, w=97, h=61, tree_mode=1, index=True, split_bits=2) == host


def test_plane_traffic(gpulib):
    w, h = 97, 61
    raw = yuv420_frame(w, h, 8, 9200)
    assert len(raw) == w * h + 2 * 49 * 31
    gpulib.encode_yuv420(raw, w, h, tree_mode=0, gpu_forward=True)
    up, down = gpulib.encode_plane_traffic()
    assert up == len(raw)                                # the raw frame: 1.5 bytes per pixel, not three int32 planes
    assert down == 4 * (w * h + 2 * 49 * 31)             # (lossless: every transformed channel comes back for the host's pixel loop)
    raw10 = yuv420_frame(w, h, 10, 9201)
    gpulib.encode_yuv420_batch([raw10, raw10], w, h, 10, tree_mode=0, gpu_forward=True)
    assert gpulib.encode_plane_traffic()[0] == 2 * len(raw10)
    encode_on_device(gpulib, [raw], w=w, h=h, tree_mode=0, quality=80)
    assert gpulib.encode_plane_traffic()[0] == 0         # nothing goes up: the frames are there, the channels stay there


def test_an_out_of_range_sample_on_the_gpu_routes(gpulib):
    L = gpulib.lib()
    w, h = 40, 36
    good = np.frombuffer(yuv420_frame(w, h, 10, 9300), "<u2").copy()
    bad = good.copy()
    bad[w * h + 7] = 1024                                # in Cb
    dev_good, dev_bad = DevBytes(gpulib, good.nbytes).put(good), DevBytes(gpulib, bad.nbytes).put(bad)
    try:
        for on_device, ptrs in ((1, [dev_good.ptr, dev_bad.ptr]), (0, [good.ctypes.data, bad.ctypes.data])):
            arr, outs, sizes = (C.c_void_p * 2)(*ptrs), (C.c_void_p * 2)(), (C.c_size_t * 2)()
            outs[0] = outs[1] = 0xDEAD
            opt = gpulib.make_encode_options(0, 1, 12, 0, 4095, 0, 0, 1, 1)
            rc = L.fuifgpu_encode_yuv420(arr, on_device, 2, w, h, 10, None, C.byref(opt), None, outs, sizes)
            assert rc == E_ARG and not outs[0] and not outs[1], on_device
        assert len(gpulib.encode_yuv420_device([dev_good.ptr], w=w, h=h, bit_depth=10, tree_mode=0)) == 1
    finally:
        dev_good.free()
        dev_bad.free()


def test_round_trip_on_the_device(gpulib, port):
    """a lossless stream written from device memory, decoded on the device: without Squeeze the coded channels ARE the unpacked planes;
    with Squeeze the decoded picture is what the oracle makes of the stream"""
    w, h = (41, 37) if EMULATED else (161, 119)
    raw = yuv420_frame(w, h, 8, 9400, layout="nv12")
    planes = yuv420_planes(w, h, 8, 9400)
    src = DevBytes(gpulib, len(raw)).put(np.frombuffer(raw, np.uint8))
    outs = [DevBytes(gpulib, 4 * p.size) for p in planes]
    try:
        gpulib.unpack_yuv420(src.ptr, w, h, outs[0].ptr, outs[1].ptr, outs[2].ptr, layout="nv12")
        unpacked = [o.get(4 * p.size, np.int32).reshape(p.shape) for o, p in zip(outs, planes)]
        assert all(np.array_equal(u, p) for u, p in zip(unpacked, planes))
        flat = gpulib.encode_yuv420_device([src.ptr], w=w, h=h, layout="nv12", tree_mode=1, split_bits=2, squeeze=False, index=True)[0]
        coded, st = gpulib.decode_batch([flat, flat], undo=False)
        assert not st.any()
        for chans in coded:
            assert len(chans) == 3 and all(np.array_equal(c, u) for c, u in zip(chans, unpacked))
        squeezed = gpulib.encode_yuv420_device([src.ptr], w=w, h=h, layout="nv12", tree_mode=1, split_bits=2, index=True)[0]
        want = port.decode(squeezed)
        assert want.ok
        decoded, st = gpulib.decode_batch([squeezed, squeezed])
        assert not st.any() and all(np.array_equal(g, e["data"]) for chans in decoded for g, e in zip(chans, want.channels))
        kept = port.decode(squeezed, keep=2)             # the Squeeze undone, the two recorded transforms kept: Y, Cb, Cr as they went in
        assert all(np.array_equal(c["data"], u) for c, u in zip(kept.channels[:3], unpacked))
    finally:
        for d in [src] + outs:
            d.free()
