"""CPU: YUV 4:2:0 input of the product's writer (fuifgpu_encode_yuv420, csrc/writer.cpp) against the REAL reference.

The yardstick is the reference CLI's bytes: tests/golden/yuv/ holds what the unmodified `fuif -I 0 -K 0 -X 0 -Y 0 -y WxH[:b] ...` wrote for
seeded frames (tests/golden/make_golden_yuv.py), with the quantisation constant of every channel as the reference's own decoder read it
back.  With single-leaf trees (tree_mode 0) the writer must reproduce those files byte for byte -- which pins the three channels of
unequal geometry, the recorded [YCbCr, ChromaSubsample] pair, the squeeze steps over them, the constants behind the two factors of
fuif.cpp:432-434 and the stacking of a clip's frames."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from fuif_amd.synth import YUV_GUARD, write_yuv, yuv420_frame, yuv420_planes

YUV = os.path.join(GOLDEN, "yuv")
with open(os.path.join(YUV, "manifest_yuv.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
E_ARG, E_HIP = 4, 5


def fixture_clip(entry, layout="i420", pad=0):
    """(raw bytes, keywords of the geometry): the fixture's frames back to back; pad > 0: rows pad bytes longer than their samples"""
    s = entry["synth"]
    bps = 2 if s["bits"] > 8 else 1
    cw = (s["w"] + 1) // 2
    pitch = None if not pad else (s["w"] * bps + pad, cw * bps * (2 if layout == "nv12" else 1) + pad)
    assert pitch is None or s["frames"] == 1, "a pitched frame ends with its last sample: no clips of them here"
    raw = b"".join(yuv420_frame(s["w"], s["h"], s["bits"], s["seed"] + f, layout=layout, pitch=pitch) for f in range(s["frames"]))
    kw = dict(w=s["w"], h=s["h"], bit_depth=s["bits"], layout=layout)
    if pitch:
        kw.update(pitch_y=pitch[0], pitch_c=pitch[1])
    if s["frames"] > 1:
        kw.update(nb_frames=s["frames"])
    return raw, kw


def encode_fixture(gpulib, entry, layout="i420", pad=0, **more):
    raw, kw = fixture_clip(entry, layout, pad)
    return gpulib.encode_yuv420_batch([raw], **kw, **entry["encode"], **more)[0]


def same_up_to_the_stray_byte(mine, theirs):
    """the reference appends one stray byte (BlobIO::bytes_used = seek_pos + 1, fileio.h:252-254): tests/test_writer.py's comparison"""
    return mine == theirs[: len(mine)] and 0 <= len(theirs) - len(mine) <= 1


def test_the_fixture_set_covers_every_rule():
    names = set(IDS)
    assert len(FIXTURES) == 19 and all(os.path.getsize(os.path.join(YUV, e["file"])) == e["nbytes"] for e in FIXTURES)
    assert all(e["nbytes"] < 20000 for e in FIXTURES)
    assert {e["synth"]["bits"] for e in FIXTURES} == {8, 10, 12, 14}
    assert {"yuv8_5x4", "yuv8_5x4_Q80", "yuv8_6x4", "yuv8_1x1", "yuv8_2x2", "yuv8_200x9_Q0", "yuv8_33x130", "yuv8_97x61_Q100_90"} <= names
    assert sum(e["synth"]["frames"] > 1 for e in FIXTURES) == 2
    for e in FIXTURES:   # [YCbCr (0), ChromaSubsample (3)] recorded by the reader, then Squeeze (7) unless too small or off, then Quantize (5)
        want = [0, 3]
        if e["encode"].get("squeeze", True) and e["synth"]["w"] * e["synth"]["h"] * e["synth"]["frames"] > 20:
            want.append(7)
        if e["encode"].get("quality", 100) < 100 or e["encode"].get("chroma_quality", 100) < 100:
            want.append(5)
        assert e["transforms"] == want, e["name"]
    by_name = {e["name"]: e for e in FIXTURES}
    assert by_name["yuv8_5x4"]["nb_coded_channels"] == 3 and by_name["yuv8_6x4"]["transforms"] == [0, 3, 7]


def test_the_synthetic_frames(tmp_path):
    luma, cb, cr = yuv420_planes(97, 61, 8, 5)
    assert luma.shape == (61, 97) and cb.shape == cr.shape == (31, 49)
    assert 85 <= cb.min() and cb.max() <= 171 and 85 <= cr.min() and cr.max() <= 171     # the middle third of the range
    raw = yuv420_frame(97, 61, 8, 5)
    assert len(raw) == 97 * 61 + 2 * 49 * 31 and raw == yuv420_frame(97, 61, 8, 5)
    assert np.array_equal(np.frombuffer(raw, np.uint8)[: 97 * 61].reshape(61, 97), luma)
    nv = np.frombuffer(yuv420_frame(97, 61, 8, 5, layout="nv12"), np.uint8)
    assert np.array_equal(nv[97 * 61:].reshape(31, 49, 2)[..., 0], cb) and np.array_equal(nv[97 * 61:].reshape(31, 49, 2)[..., 1], cr)
    padded = np.frombuffer(yuv420_frame(97, 61, 8, 5, pitch=(102, 54)), np.uint8)
    assert len(padded) == 102 * 61 + 54 * 31 * 2 - 5
    assert (padded[: 102 * 61].reshape(61, 102)[:, 97:] == YUV_GUARD).all() and np.array_equal(padded[: 102 * 61].reshape(61, 102)[:, :97], luma)
    wide = np.frombuffer(yuv420_frame(40, 36, 14, 6), "<u2")
    assert wide.size == 40 * 36 + 2 * 20 * 18 and wide.max() < 1 << 14 and np.array_equal(wide[: 40 * 36].reshape(36, 40), yuv420_planes(40, 36, 14, 6)[0])
    write_yuv(str(tmp_path / "f.yuv"), raw)
    assert open(str(tmp_path / "f.yuv"), "rb").read() == raw


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_quantization_constants_are_the_reference_clis(gpulib, entry):
    kw = entry["encode"]
    assert entry["channels"], "a fixture without a single coded constant pins nothing"
    for ch in entry["channels"]:
        q = gpulib.quantization_constant_yuv(kw.get("quality", 100), kw.get("chroma_quality"), squeeze=kw.get("squeeze", True),
                                             chroma_table=ch["component"] in (1, 2), shift=ch["hcshift"] + ch["vcshift"])
        assert q == ch["q"], (entry["name"], ch)


def test_the_pnm_constants_are_unchanged(gpulib):
    assert gpulib.quantization_constant(50, shift=0) == 58 and gpulib.quantization_constant(50, chroma_table=True, shift=0) == 307
    assert gpulib.quantization_constant_yuv(50, shift=0) == 58          # luma: 3.0 / 3.0 cancel up to rounding at this quality
    assert gpulib.quantization_constant_yuv(50, chroma_table=True, shift=0) == 102
    assert gpulib.quantization_constant_yuv(100) == 1
    for bad in ((float("nan"), 50.0, 0), (-3.0, 50.0, 0), (101.0, 50.0, 0), (50.0, 50.0, -1)):
        assert gpulib.lib().fuifgpu_quantization_constant_yuv(bad[0], bad[1], 1, 0, bad[2]) == -E_ARG


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_writer_writes_the_reference_clis_bytes(gpulib, entry):
    theirs = open(os.path.join(YUV, entry["file"]), "rb").read()
    mine = encode_fixture(gpulib, entry, tree_mode=0)
    assert same_up_to_the_stray_byte(mine, theirs), entry["name"]
    # the same samples as NV12, and (single frames) in rows 5 bytes longer than their samples, planar and NV12
    assert encode_fixture(gpulib, entry, layout="nv12", tree_mode=0) == mine, entry["name"]
    if entry["synth"]["frames"] == 1:
        assert encode_fixture(gpulib, entry, pad=5 if entry["synth"]["bits"] == 8 else 6, tree_mode=0) == mine, entry["name"]
        assert encode_fixture(gpulib, entry, layout="nv12", pad=5 if entry["synth"]["bits"] == 8 else 6, tree_mode=0) == mine, entry["name"]


def test_the_python_entry_points_agree(gpulib):
    e = next(x for x in FIXTURES if x["name"] == "yuv8_97x61_Q80")
    raw, kw = fixture_clip(e)
    one = gpulib.encode_yuv420(raw, 97, 61, quality=80, tree_mode=0)
    assert one == gpulib.encode_yuv420(np.frombuffer(raw, np.uint8), 97, 61, quality=80, tree_mode=0)
    assert gpulib.encode_yuv420_batch([raw, raw], 97, 61, quality=80, tree_mode=0) == [one, one]
    assert gpulib.encode_yuv420_clip(raw, 97, 61, nb_frames=1, quality=80, tree_mode=0) == one      # one frame: "FUIF", the still's bytes
    wide = next(x for x in FIXTURES if x["name"] == "yuv10_75x49")
    raw10, _ = fixture_clip(wide)
    assert gpulib.encode_yuv420(np.frombuffer(raw10, "<u2"), 75, 49, 10, tree_mode=0) == gpulib.encode_yuv420(raw10, 75, 49, 10, tree_mode=0)
    clip = next(x for x in FIXTURES if x["name"] == "yuv8_96x60x3_M0_F25_Q70")
    rawc, _ = fixture_clip(clip)
    theirs = open(os.path.join(YUV, clip["file"]), "rb").read()
    assert same_up_to_the_stray_byte(gpulib.encode_yuv420_clip(rawc, 96, 60, 3, framerate=25, quality=70, tree_mode=0), theirs)
    assert gpulib.yuv420_bytes(96, 60, nb_frames=3) == len(rawc)
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_yuv420(raw[:-1], 97, 61)          # a short buffer is refused before the library reads it
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_yuv420(np.zeros(10000, np.float32), 97, 61)


def input_channels(entry):
    s = entry["synth"]
    per_frame = [yuv420_planes(s["w"], s["h"], s["bits"], s["seed"] + f) for f in range(s["frames"])]
    return [np.concatenate([fr[c] for fr in per_frame], axis=0) for c in range(3)]


@pytest.mark.parametrize("name", ["yuv8_97x61", "yuv10_75x49", "yuv8_6x4", "yuv8_96x60x3_M0"])
def test_learned_tree_streams_decode_the_same_with_port_and_reference(gpulib, port, ref, name):
    entry = next(x for x in FIXTURES if x["name"] == name)
    blob = encode_fixture(gpulib, entry, tree_mode=1, index=True)
    p0, p1 = port.decode_both(blob)
    r0, r1 = ref.decode_both(blob)
    assert p0.ok and r0.ok and p1.ok and r1.ok
    assert [t[0] for t in p0.transforms] == entry["transforms"]
    for a, b in ((p0, r0), (p1, r1)):
        assert len(a.channels) == len(b.channels)
        assert all(np.array_equal(x["data"], y["data"]) for x, y in zip(a.channels, b.channels))
    s = entry["synth"]
    assert p1.channels[0]["data"].shape == (s["h"] * s["frames"], s["w"])


@pytest.mark.parametrize("entry", [e for e in FIXTURES if "quality" not in e["encode"]], ids=[e["name"] for e in FIXTURES if "quality" not in e["encode"]])
def test_lossless_streams_hold_the_input_samples(gpulib, port, entry):
    """the coded channels with only the Squeeze undone (the two recorded transforms kept) are Y, Cb and Cr as they went in"""
    blob = encode_fixture(gpulib, entry, tree_mode=1)
    dec = port.decode(blob, keep=2)
    assert dec.ok and len(dec.channels) >= 3
    for got, want in zip(dec.channels[:3], input_channels(entry)):
        assert np.array_equal(got["data"], want), entry["name"]
    assert [(c["hshift"], c["vshift"]) for c in dec.channels[:3]] == [(0, 0), (1, 1), (1, 1)]


@pytest.mark.parametrize("w,h,bits,seed,extra,kw", [
    (71, 53, 8, 701, ["-Q", "88"], dict(quality=88)),
    (50, 90, 8, 702, ["-Q", "42.25,63"], dict(quality=42.25, chroma_quality=63)),
    (66, 34, 10, 703, ["-Q", "12"], dict(quality=12)),
    (37, 29, 8, 704, ["-R", "0", "-Q", "55"], dict(quality=55, squeeze=False)),
    (23, 7, 12, 705, [], dict()),
])
def test_fresh_frames_against_the_live_reference_cli(gpulib, ref, tmp_path, w, h, bits, seed, extra, kw):
    from oracle_py import ref_cli, run_ref_cli
    if ref_cli() is None:
        pytest.skip("reference CLI not built")
    raw = yuv420_frame(w, h, bits, seed)
    src, out = str(tmp_path / "in.yuv"), str(tmp_path / "ref.fuif")
    write_yuv(src, raw)
    r = run_ref_cli(["-I", "0", "-K", "0", "-X", "0", "-Y", "0", "-y", "%dx%d:%d" % (w, h, bits)] + extra + [src, out])
    assert r.returncode == 0, r.stderr
    mine = gpulib.encode_yuv420(raw, w, h, bits, tree_mode=0, **kw)
    assert same_up_to_the_stray_byte(mine, open(out, "rb").read())


def _call(gpulib, raw, w=24, h=20, bits=8, size=None, layout=0, pitch_y=0, pitch_c=0, nb_frames=1, framerate=0, frames=None, n=1, gpu_forward=0):
    L = gpulib.lib()
    buf = np.frombuffer(raw, np.uint8)
    yuv = gpulib.YuvOptions(C.sizeof(gpulib.YuvOptions) if size is None else size, layout, pitch_y, pitch_c, nb_frames, framerate)
    opt = gpulib.make_encode_options(0, 1, 12, 0, 4095, 0, 0, gpu_forward, 0)
    ptrs = (C.c_void_p * n)(*([buf.ctypes.data] * n if frames is None else frames))
    outs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
    for k in range(n):
        outs[k] = 0xDEAD
    rc = L.fuifgpu_encode_yuv420(ptrs, 0, n, w, h, bits, C.byref(yuv), C.byref(opt), None, outs, sizes)
    if rc == 0:
        for k in range(n):
            L.fuifgpu_free_blob(C.c_void_p(outs[k]))
    else:
        assert all(not outs[k] for k in range(n)), "an error leaves every blob NULL"
    return rc


def test_argument_errors(gpulib):
    raw = yuv420_frame(24, 20, 8, 9) * 2
    raw16 = yuv420_frame(24, 20, 10, 9)
    assert _call(gpulib, raw) == 0
    assert _call(gpulib, raw, size=16) == 0                       # a struct that ends before nb_frames: one frame
    assert _call(gpulib, raw, size=28) == 0                       # a LARGER (later) struct: what this library knows is read
    for size in (0, 2, 6, 10):
        assert _call(gpulib, raw, size=size) == E_ARG, size
    for layout in (-1, 2, 7):
        assert _call(gpulib, raw, layout=layout) == E_ARG, layout
    assert _call(gpulib, raw, pitch_y=23) == E_ARG and _call(gpulib, raw, pitch_c=11) == E_ARG
    assert _call(gpulib, raw, layout=1, pitch_c=23) == E_ARG and _call(gpulib, raw, layout=1, pitch_c=24) == 0
    assert _call(gpulib, raw16, bits=10, pitch_y=47) == E_ARG and _call(gpulib, raw16, bits=10, pitch_y=48) == 0      # two bytes per sample
    for bits in (7, 15, 16, 0):
        assert _call(gpulib, raw16, bits=bits) == E_ARG, bits
    assert _call(gpulib, raw, nb_frames=2) == 0
    assert _call(gpulib, raw, nb_frames=0) == E_ARG and _call(gpulib, raw, nb_frames=-1) == E_ARG
    assert _call(gpulib, raw, framerate=-1) == E_ARG
    assert _call(gpulib, yuv420_frame(24, 21, 8, 9) * 2, h=21, nb_frames=2) == E_ARG      # a clip of odd height
    assert _call(gpulib, yuv420_frame(24, 21, 8, 9), h=21) == 0
    assert _call(gpulib, raw, w=0) == E_ARG and _call(gpulib, raw, h=0) == E_ARG
    assert _call(gpulib, raw, frames=[0]) == E_ARG                                      # NULL frame
    buf = np.frombuffer(raw, np.uint8)
    assert _call(gpulib, raw, frames=[buf.ctypes.data, 0], n=2) == E_ARG
    # a 16-bit sample above maxval, in each plane, on the host route
    for at in (0, 24 * 20 - 1, 24 * 20, 24 * 20 + 12 * 10, 24 * 20 + 2 * 12 * 10 - 1):
        bad = np.frombuffer(raw16, "<u2").copy()
        bad[at] = 1023
        assert _call(gpulib, bad.tobytes(), bits=10) == 0
        bad[at] = 1024
        assert _call(gpulib, bad.tobytes(), bits=10) == E_ARG, at
        assert _call(gpulib, bad.tobytes(), bits=10, layout=1) == E_ARG, at
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.encode_yuv420(raw, 24, 20, layout="yv12")
    assert e.value.code == E_ARG
    L = gpulib.lib()
    assert L.fuifgpu_encode_yuv420(None, 0, 1, 24, 20, 8, None, None, None, None, None) == E_ARG


def test_gpu_forward_fails_loudly_without_a_gpu(gpulib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    raw = yuv420_frame(64, 48, 8, 1)
    for kw in (dict(gpu_forward=True), dict(gpu_forward=True, quality=80), dict(gpu_entropy=True)):
        with pytest.raises(gpulib.FuifGpuError) as e:
            gpulib.encode_yuv420(raw, 64, 48, **kw)
        assert e.value.code == E_HIP and "HIP" in str(e.value)
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.encode_yuv420_batch([raw, raw], 64, 48, gpu_forward=True)
    assert e.value.code == E_HIP


def test_header_declares_the_entry_points(gpulib):
    import re
    hdr = open(os.path.join(ROOT, "include", "fuifgpu.h")).read()
    declared = set(re.findall(r"\b(fuifgpu_[a-z0-9_]+)\s*\(", hdr))
    L = gpulib.lib()
    for s in ("fuifgpu_encode_yuv420", "fuifgpu_unpack_yuv420", "fuifgpu_quantization_constant_yuv"):
        assert s in declared and s in gpulib.ABI_SYMBOLS and hasattr(L, s), s
    assert L.fuifgpu_abi_version() == 3


def test_gpu_yuv_tests_pass_on_the_wavefront_emulator():
    """tests/test_gpu_yuv_encoder.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_unpack_yuv420's lane mapping, its row ends and its de-interleaving, and both GPU routes of the writer, checked without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_yuv_encoder.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
