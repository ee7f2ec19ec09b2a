"""GPU parity (-m gpu) of the decoder's kept-transform route: Plan(blob, keep) + Batch against the plain-C oracle's undo_transforms(keep) at
every keep, and YUV 4:2:0 frames out -- the pack kernel (transforms.hip k_pack_yuv420, fuifgpu_pack_yuv420) against numpy, and
fuifgpu_batch_pack_yuv420 / _download_yuv420 against the bytes export/write_yuv.h:46-53 gives for the oracle's keep-2 channels, against
the synthetic input frames of the lossless fixtures (which rests on no decoder) and, where oracle/_ref/fuif exists, against the file
`fuif -d x.fuif out.yuv` writes.
On a machine without a GPU tests/test_plan_keep.py runs this file against the wavefront emulator build."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd.synth import photographic, yuv420_frame, yuv420_planes

pytestmark = pytest.mark.gpu

EMULATED = ("_emu" in os.path.basename(os.environ.get("FUIF_AMD_LIB", "")))
YUV = os.path.join(GOLDEN, "yuv")
with open(os.path.join(YUV, "manifest_yuv.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
if EMULATED:
    FIXTURES = [e for e in FIXTURES if e["name"] in ("yuv8_97x61", "yuv8_97x61_Q80", "yuv8_97x61_R0", "yuv8_5x4", "yuv8_6x4", "yuv8_1x1", "yuv8_2x2",
                                                     "yuv10_75x49", "yuv12_41x37_Q50", "yuv8_96x60x3_M0")]
IDS = [e["name"] for e in FIXTURES]
# the streams whose channel tables tests/test_plan_keep.py checks at every keep: here their samples
KEEP_STREAMS = ["yuv/yuv8_97x61.fuif", "yuv/yuv8_5x4.fuif", "yuv/yuv8_1x1.fuif", "yuv/yuv10_75x49_Q60.fuif", "yuv/yuv8_96x60x3_M0.fuif",
                "jpeg420_256x192_q90.fuif", "rgb8_97x61.fuif", "pal_rgb_graphic_120x90.fuif", "animation/rgb_48x8x3_defaults.fuif"]
E_UNSUPPORTED, E_ARG = 3, 4
GUARD_BYTE, GUARD_WORD = 0xA5, -123456789


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


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


def frame_bytes(planes, maxval, layout="i420", pad=0, fill=GUARD_BYTE, whole_last_row=False):
    """write_yuv.h:46-53 in numpy, in any of the layouts: (uint8 array, pitch_y, pitch_c) of one frame of CLAMP(sample, 0, maxval), one
    byte per sample for maxval < 256 else two little-endian, rows `pad` bytes longer than their samples (padding: `fill`).  The frame ends
    with its last sample unless whole_last_row"""
    y, cb, cr = [np.clip(np.asarray(p, np.int64), 0, maxval) for p in planes]
    dt = np.uint8 if maxval < 256 else np.dtype("<u2")
    parts = [y, cb, cr] if layout == "i420" else [y, np.stack([cb, cr], axis=-1).reshape(cb.shape[0], -1)]
    out, pitches = [], []
    for p in parts:
        rows = np.ascontiguousarray(p.astype(dt)).view(np.uint8).reshape(p.shape[0], -1)
        padded = np.full((rows.shape[0], rows.shape[1] + pad), fill, np.uint8)
        padded[:, : rows.shape[1]] = rows
        out.append(padded.reshape(-1))
        pitches.append(rows.shape[1] + pad)
    raw = np.concatenate(out)
    return (raw if whole_last_row else raw[: raw.size - pad]), pitches[0], pitches[-1]


WIDTHS = [1, 3, 5, 65, 97] if EMULATED else [1, 2, 3, 4, 5, 63, 64, 65, 97, 255, 256, 257]
HEIGHTS = [1, 3, 18] if EMULATED else [1, 2, 3, 18]      # (18: every one of a wavefront's four rows, and a second block)
PADS = [0, 3] if EMULATED else [0, 1, 3, 6]
SKEWS = [0, 1, 3] if EMULATED else [0, 1, 2, 3]          # (16-bit rows on odd bytes; NV12 rows whose first aligned word starts inside a pair)


def wild_planes(rng, w, h, maxval):
    """samples in range, below 0, above maxval and at the ends of int16, so that the clamp has work"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    planes = []
    for shape in ((h, w), (ch, cw), (ch, cw)):
        p = rng.integers(0, maxval + 1, size=shape).astype(np.int32)
        wild = rng.integers(0, 6, size=shape)
        p = np.where(wild == 0, rng.integers(-300, 0, size=shape), p)
        p = np.where(wild == 1, rng.integers(maxval + 1, maxval + 300, size=shape), p).astype(np.int32)
        flat = p.reshape(-1)
        for k, v in enumerate((32767, -32767, -32768, maxval, 0)):
            if k < flat.size:
                flat[(k * 7) % flat.size] = v
        planes.append(p)
    return planes


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("bits", [8, 10])
def test_pack_against_numpy(gpulib, bits, layout):
    """every width around the word, the wavefront and the row segment; rows and frame bases on every byte alignment, source planes on and
    off a 16-byte boundary; every byte in front of the frame, in the pitch gaps and behind the last sample stays what it was"""
    L = gpulib.lib()
    maxval = (1 << bits) - 1
    dst = DevBytes(gpulib, 64 + 4 + 3 * 2 * (max(WIDTHS) + 8) * max(HEIGHTS) + 64)
    ins = [DevBytes(gpulib, 4 * (max(WIDTHS) * max(HEIGHTS) + 16)) for _ in range(3)]
    rng = np.random.default_rng(bits * 10 + len(layout))
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                planes = wild_planes(rng, w, h, maxval)
                for pad in PADS:
                    want, py, pc = frame_bytes(planes, maxval, layout, pad)
                    lead = 4 + (pad & 1)                         # source planes on and off a 16-byte boundary
                    for d, p in zip(ins, planes):
                        d.put(np.concatenate([np.full(lead, GUARD_WORD, np.int32), p.reshape(-1)]))
                    for skew in SKEWS:
                        front = 32 + skew
                        dst.put(np.full(front + want.size + 32, GUARD_BYTE, np.uint8))
                        yuv = gpulib.make_yuv_options(layout, py if pad else 0, pc if pad else 0)
                        rc = L.fuifgpu_pack_yuv420(ins[0].ptr + 4 * lead, ins[1].ptr + 4 * lead, ins[2].ptr + 4 * lead, w, h, bits, C.byref(yuv),
                                                   dst.ptr + front, None)
                        case = (w, h, bits, layout, pad, skew)
                        assert rc == 0, case
                        got = dst.get(front + want.size + 32)
                        assert (got[:front] == GUARD_BYTE).all(), ("bytes in front of the frame", case)
                        assert (got[front + want.size:] == GUARD_BYTE).all(), ("bytes behind the last sample", case)
                        assert np.array_equal(got[front: front + want.size], want), case      # (samples, and GUARD_BYTE in every pitch gap)
    finally:
        for d in [dst] + ins:
            d.free()


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_unpack_of_pack_is_the_identity(gpulib, layout):
    L = gpulib.lib()
    for w, h, bits, pad, skew in ((97, 61, 8, 0, 0), (65, 18, 10, 6, 2), (5, 3, 12, 3, 1), (64, 4, 8, 1, 3)):
        planes = yuv420_planes(w, h, bits, 700 + w)
        size = frame_bytes(planes, (1 << bits) - 1, layout, pad)[0].size
        ins = [DevBytes(gpulib, 4 * p.size).put(p) for p in planes]
        outs = [DevBytes(gpulib, 4 * p.size).put(np.full(p.size, GUARD_WORD, np.int32)) for p in planes]
        frame = DevBytes(gpulib, size + 8)
        try:
            bps = 2 if bits > 8 else 1
            pitch = dict(pitch_y=w * bps + pad, pitch_c=((w + 1) // 2) * bps * (2 if layout == "nv12" else 1) + pad) if pad else {}
            gpulib.pack_yuv420(ins[0].ptr, ins[1].ptr, ins[2].ptr, w, h, frame.ptr + skew, bit_depth=bits, layout=layout, **pitch)
            gpulib.unpack_yuv420(frame.ptr + skew, w, h, outs[0].ptr, outs[1].ptr, outs[2].ptr, bit_depth=bits, layout=layout, **pitch)
            for o, p in zip(outs, planes):
                assert np.array_equal(o.get(4 * p.size, np.int32).reshape(p.shape), p), (w, h, bits, layout, pad, skew)
        finally:
            for d in ins + outs + [frame]:
                d.free()
    # w * h == 0 touches nothing and needs nothing; NULL planes, a depth or a pitch the geometry refuses
    assert L.fuifgpu_pack_yuv420(None, None, None, 0, 5, 8, None, None, None) == 0
    yuv = gpulib.make_yuv_options(layout)
    assert L.fuifgpu_pack_yuv420(None, None, None, 5, 4, 8, C.byref(yuv), None, None) == E_ARG
    d = DevBytes(gpulib, 256)
    try:
        assert L.fuifgpu_pack_yuv420(d.ptr, d.ptr, d.ptr, 5, 4, 15, C.byref(yuv), d.ptr, None) == E_ARG
        assert L.fuifgpu_pack_yuv420(d.ptr, d.ptr, d.ptr, 5, 4, 8, C.byref(gpulib.make_yuv_options(layout, pitch_y=4)), d.ptr, None) == E_ARG
    finally:
        d.free()


def decoded_batch(gpulib, blobs, keep, preview=-1):
    """Batch(Plan(blob, keep)) after upload, decode and undo_transforms; the caller closes it"""
    plan = gpulib.Plan(blobs[0], keep)
    batch = gpulib.Batch(plan, len(blobs), sum(len(b) for b in blobs))
    try:
        batch.upload(blobs, preview)
        batch.decode()
        batch.undo_transforms()
        batch.sync()
    except Exception:
        batch.close()
        raise
    return plan, batch


def assert_planes_equal(got, want, what):
    assert len(got) == len(want.channels), what
    for c, (g, e) in enumerate(zip(got, want.channels)):
        assert g.shape == (e["h"], e["w"]), (what, c)
        assert np.array_equal(g.reshape(-1), np.asarray(e["data"]).reshape(-1)), (what, c)


@pytest.mark.parametrize("name", KEEP_STREAMS)
def test_batch_planes_equal_the_oracles_at_every_keep(gpulib, port, name):
    """channel for channel, out-of-range values included (no clamp unless keep == 0); once more with a group index"""
    blob = golden(name)
    indexed = gpulib.index_append(blob, port.decode(blob, undo=False).groups)
    nt = gpulib.Plan(blob).info.nb_transforms
    keeps = range(nt + 1)
    if EMULATED and "jpeg420" in name:
        keeps = (2, 3, 4)       # (the frame route, dequantised coefficient planes as final planes, coded planes as final planes)
    for keep in keeps:
        want = port.decode(blob, keep=keep)
        assert want.ok
        plan, batch = decoded_batch(gpulib, [blob, indexed], keep)
        try:
            assert plan.keep == keep and not batch.status()[0].any()
            for i in range(2):
                assert_planes_equal(batch.out_planes(i), want, (name, keep, i))
        finally:
            batch.close()


@pytest.mark.parametrize("name", ["yuv/yuv8_97x61.fuif", "jpeg420_256x192_q90.fuif"])
def test_preview_at_keep_2(gpulib, port, name):
    blob = golden(name)
    want = port.decode(blob, 2, keep=2)
    plan, batch = decoded_batch(gpulib, [blob], 2, preview=2)
    try:
        assert_planes_equal(batch.out_planes(0), want, name)
    finally:
        batch.close()


def reference_cli_yuv(blob, tmp_path):
    """the bytes `fuif -d x.fuif out.yuv` writes, or None without the reference CLI"""
    from oracle_py import ref_cli, run_ref_cli
    if not ref_cli():
        return None
    src, out = str(tmp_path / "x.fuif"), str(tmp_path / "out.yuv")
    with open(src, "wb") as f:
        f.write(blob)
    r = run_ref_cli(["-d", src, out], timeout=120)
    assert os.path.exists(out), r.stdout + r.stderr
    with open(out, "rb") as f:
        return f.read()


def strip_planes(entry):
    """the synthetic input of a fixture as write_YUV_file sees it: the frames stacked per channel"""
    s = entry["synth"]
    frames = [yuv420_planes(s["w"], s["h"], s["bits"], s["seed"] + f) for f in range(s["frames"])]
    return [np.concatenate([fr[c] for fr in frames], axis=0) for c in range(3)]


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_frames_of_the_yuv_fixtures(gpulib, port, entry, tmp_path):
    blob = golden(os.path.join("yuv", entry["file"]))
    s = entry["synth"]
    maxval = (1 << s["bits"]) - 1
    want = port.decode(blob, keep=2)
    assert want.ok and len(want.channels) == 3
    planes = want.planes()
    tight = frame_bytes(planes, maxval)[0].tobytes()
    plan, batch = decoded_batch(gpulib, [blob], 2)
    try:
        got = batch.download_yuv420(0)
        assert len(got) == plan.yuv420_bytes() == len(tight)
        assert got == tight, entry["name"]
        if "quality" not in entry["encode"] and "chroma_quality" not in entry["encode"]:      # lossless: the input itself, no decoder involved
            assert got == frame_bytes(strip_planes(entry), maxval)[0].tobytes(), entry["name"]
        theirs = reference_cli_yuv(blob, tmp_path)
        if theirs is not None:
            assert got == theirs, entry["name"]
        pad = 5 if s["bits"] == 8 else 6
        assert batch.download_yuv420(0, layout="nv12") == frame_bytes(planes, maxval, "nv12")[0].tobytes()
        for layout in ("i420", "nv12"):
            exp, py, pc = frame_bytes(planes, maxval, layout, pad, fill=0, whole_last_row=True)
            assert batch.download_yuv420(0, layout=layout, pitch_y=py, pitch_c=pc) == exp.tobytes(), (entry["name"], layout)
    finally:
        batch.close()


def test_frame_of_the_jpeg_transcoded_stream(gpulib, port, tmp_path):
    blob = golden("jpeg420_256x192_q90.fuif")
    want = port.decode(blob, keep=2)
    assert [(c["w"], c["h"]) for c in want.channels] == [(256, 192), (128, 96), (128, 96)]
    plan, batch = decoded_batch(gpulib, [blob], 2)
    try:
        got = batch.download_yuv420(0)
        assert got == frame_bytes(want.planes(), 255)[0].tobytes()
        assert batch.download_yuv420(0, layout="nv12") == frame_bytes(want.planes(), 255, "nv12")[0].tobytes()
        theirs = reference_cli_yuv(blob, tmp_path)
        if theirs is not None:
            assert got == theirs
    finally:
        batch.close()


def test_block_padded_planes_are_cropped(gpulib, port):
    from fuif_amd.jpeglike import encode_jpeg_like
    w, h = 97, 61
    blob = encode_jpeg_like(photographic(w, h, 3, 8, seed=77), 90, True, index=True)
    want = port.decode(blob, keep=2)
    assert want.ok and [(c["w"], c["h"]) for c in want.channels] == [(104, 64), (56, 32), (56, 32)]      # iDCT block padding
    cropped = [want.channels[0]["data"][:h, :w], want.channels[1]["data"][:31, :49], want.channels[2]["data"][:31, :49]]
    plan, batch = decoded_batch(gpulib, [blob], 2)
    try:
        assert_planes_equal(batch.out_planes(0), want, "jpeg-like 97x61")
        assert plan.yuv420_bytes() == w * h + 2 * 49 * 31
        assert batch.download_yuv420(0) == frame_bytes(cropped, 255)[0].tobytes()
        exp, py, pc = frame_bytes(cropped, 255, "nv12", 3, fill=0, whole_last_row=True)
        assert batch.download_yuv420(0, layout="nv12", pitch_y=py, pitch_c=pc) == exp.tobytes()
    finally:
        batch.close()


def test_clip_as_frames_and_as_the_strip(gpulib):
    entry = next(e for e in FIXTURES if e["name"] == "yuv8_96x60x3_M0")
    s = entry["synth"]
    clip = b"".join(yuv420_frame(s["w"], s["h"], s["bits"], s["seed"] + f) for f in range(s["frames"]))
    blob = golden(os.path.join("yuv", entry["file"]))
    assert gpulib.encode_yuv420_clip(clip, s["w"], s["h"], s["frames"], tree_mode=0) in (blob, blob[:-1])    # the clip the writer was given
    plan, batch = decoded_batch(gpulib, [blob], 2)
    try:
        assert plan.yuv420_bytes(nb_frames=3) == len(clip) == plan.yuv420_bytes()
        assert batch.download_yuv420(0, nb_frames=3) == clip
        assert batch.download_yuv420(0, nb_frames=1) == frame_bytes(strip_planes(entry), 255)[0].tobytes() != clip
        nv = b"".join(yuv420_frame(s["w"], s["h"], s["bits"], s["seed"] + f, layout="nv12") for f in range(s["frames"]))
        assert batch.download_yuv420(0, layout="nv12", nb_frames=3) == nv
        assert plan.yuv420_bytes(nb_frames=2) == 0
        with pytest.raises(gpulib.FuifGpuError) as e:
            batch.download_yuv420(0, nb_frames=2)
        assert e.value.code == E_ARG
    finally:
        batch.close()


def four_frames(gpulib):
    w, h = 97, 61
    frames = [yuv420_frame(w, h, 8, 8100 + k) for k in range(4)]
    blobs = gpulib.encode_yuv420_batch(frames, w, h, tree_mode=1, index=True, split_bits=2)
    assert len(set(blobs)) == 4
    return frames, blobs


def test_batch_form_strides_siblings_and_streaming(gpulib):
    frames, blobs = four_frames(gpulib)
    size, gap = len(frames[0]), 37
    cap = sum(len(b) for b in blobs)
    plan, batch = decoded_batch(gpulib, blobs, 2)
    dst = DevBytes(gpulib, 4 * (size + gap) + 64)
    sib = stream = slices = None
    try:
        assert plan.yuv420_bytes() == size
        # images 1 and 2 only, a stride wider than the frame: everything else keeps its guard bytes
        dst.put(np.full(dst.n, GUARD_BYTE, np.uint8))
        batch.pack_yuv420(1, 2, dst.ptr + 16, image_stride=size + gap)
        got = dst.get(dst.n)
        assert (got[:16] == GUARD_BYTE).all()
        assert got[16: 16 + size].tobytes() == frames[1] and got[16 + size + gap: 16 + 2 * size + gap].tobytes() == frames[2]
        assert (got[16 + size: 16 + size + gap] == GUARD_BYTE).all() and (got[16 + 2 * size + gap:] == GUARD_BYTE).all()
        # all four, tight
        batch.pack_yuv420(0, 4, dst.ptr)
        assert dst.get(4 * size).tobytes() == b"".join(frames)
        with pytest.raises(gpulib.FuifGpuError) as e:
            batch.pack_yuv420(0, 2, dst.ptr, image_stride=size - 1)
        assert e.value.code == E_ARG
        # the sibling pattern: upload into the sibling (it plans with the primary's keep), decode, pack
        sib = batch.sibling(cap)
        sib.upload(blobs[::-1])
        sib.decode()
        sib.undo_transforms()
        sib.pack_yuv420(0, 4, dst.ptr)
        assert not sib.status()[0].any()
        assert dst.get(4 * size).tobytes() == b"".join(frames[::-1])
        assert sib.download_yuv420(3) == frames[0]
        # a streaming batch: the inverse transforms range by range into caller memory, then the raw pack on the slices
        elems = plan.info.out_elems
        slices = DevBytes(gpulib, 4 * elems * 4)
        stream = gpulib.Batch(plan, 4, cap, streaming=True)
        stream.upload(blobs)
        stream.decode()
        stream.undo_transforms_to(0, 2, slices.ptr)
        stream.undo_transforms_to(2, 2, slices.ptr + 2 * 4 * elems)
        offs = [c["offset"] for c in plan.output_channels]
        for k in range(4):
            base = slices.ptr + 4 * elems * k
            gpulib.pack_yuv420(base + 4 * offs[0], base + 4 * offs[1], base + 4 * offs[2], 97, 61, dst.ptr + k * size)
        assert dst.get(4 * size).tobytes() == b"".join(frames)
        with pytest.raises(gpulib.FuifGpuError) as e:
            stream.pack_yuv420(0, 1, dst.ptr)             # no output slab
        assert e.value.code == E_ARG
    finally:
        for b in (sib, stream, batch):
            if b is not None:
                b.close()
        dst.free()
        if slices is not None:
            slices.free()


def test_decode_yuv420_returns_what_encode_yuv420_batch_was_given(gpulib):
    frames, blobs = four_frames(gpulib)
    assert gpulib.decode_yuv420(blobs) == frames
    nv = [yuv420_frame(97, 61, 8, 8100 + k, layout="nv12") for k in range(4)]
    assert gpulib.decode_yuv420(blobs, layout="nv12") == nv
    raw10 = yuv420_frame(75, 49, 10, 8200)
    assert gpulib.decode_yuv420([gpulib.encode_yuv420(raw10, 75, 49, 10, tree_mode=0)]) == [raw10]


def test_refusals(gpulib):
    yuv = golden("yuv/yuv8_97x61.fuif")
    rgb = golden("rgb8_97x61.fuif")
    dst = DevBytes(gpulib, 97 * 61 * 4)
    try:
        for blob, keep, code in ((yuv, 0, E_ARG), (yuv, 1, E_ARG), (yuv, 3, E_ARG), (rgb, 2, E_UNSUPPORTED), (golden("pal_rgb_graphic_120x90.fuif"), 2, E_UNSUPPORTED),
                                 ) + (() if EMULATED else ((golden("jpeg422_200x104_q88.fuif"), 2, E_UNSUPPORTED),)):
            plan, batch = decoded_batch(gpulib, [blob], keep)
            try:
                assert plan.yuv420_bytes() == 0
                with pytest.raises(gpulib.FuifGpuError) as e:
                    batch.pack_yuv420(0, 1, dst.ptr)
                assert e.value.code == code, (keep, code)
                with pytest.raises(gpulib.FuifGpuError) as e:
                    batch.download_yuv420(0)
                assert e.value.code == code, (keep, code)
            finally:
                batch.close()
        plan, batch = decoded_batch(gpulib, [yuv], 2)
        try:
            with pytest.raises(gpulib.FuifGpuError) as e:
                batch.pack_out(dst.ptr)                   # chroma is smaller than w x h: write_pam.h:50-54 refuses such channels too
            assert e.value.code == E_ARG and batch.packed_bytes() == 0
            with pytest.raises(gpulib.FuifGpuError) as e:
                batch.undo_transforms()                   # once per decode, as ever
            assert e.value.code == E_ARG
        finally:
            batch.close()
        other = gpulib.Batch(plan, 1, len(rgb) + len(yuv))
        try:
            with pytest.raises(gpulib.FuifGpuError) as e:
                other.upload([rgb])                       # planned with the batch's keep, then the signatures are compared
            assert e.value.code == 6                      # FUIFGPU_E_MISMATCH
            other.upload([yuv])                           # (the stream's keep-0 signature differs from the batch's: it is planned with keep 2)
        finally:
            other.close()
    finally:
        dst.free()
