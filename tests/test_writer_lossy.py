"""CPU: lossy encoding of the product's writer (fuifgpu_encode_image_lossy, csrc/writer.cpp) against the REAL reference.

The yardstick is the reference CLI's bytes: tests/golden/lossy/ holds what the unmodified `fuif -I 0 -K 0 -X 0 -Y 0 -Q ...` wrote for
seeded pictures (tests/golden/make_golden_lossy.py), with the quantisation constant of every channel as the reference's own decoder
read it back.  With single-leaf trees (tree_mode 0) the writer must reproduce those files byte for byte -- which pins the constants
(fuif.cpp:459-503), the truncating division (transform/quantize.h:54-71), the parameterless Quantize entry and the channel headers."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from fuif_amd.synth import photographic, write_pnm

LOSSY = os.path.join(GOLDEN, "lossy")
with open(os.path.join(LOSSY, "manifest_lossy.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]


def fixture_picture(entry):
    s = entry["synth"]
    return photographic(s["w"], s["h"], s["channels"], s["bits"], seed=s["seed"]), s["bits"]


def same_up_to_the_stray_byte(mine, theirs):
    """the reference appends one stray byte (BlobIO::bytes_used = seek_pos + 1, fileio.h:252-254): tests/test_writer.py's comparison"""
    return mine == theirs[: len(mine)] and 0 <= len(theirs) - len(mine) <= 1


def test_the_fixture_set_covers_every_rule():
    names = set(IDS)
    assert len(FIXTURES) == 16 and all(os.path.getsize(os.path.join(LOSSY, e["file"])) == e["nbytes"] for e in FIXTURES)
    kinds = {(e["synth"]["channels"], e["synth"]["bits"]) for e in FIXTURES}
    assert {(3, 8), (1, 8), (4, 14), (2, 8)} <= kinds
    assert any(e["encode"].get("squeeze") is False for e in FIXTURES) and any(e["encode"].get("ycocg") is False for e in FIXTURES)
    assert {"rgb8_5x4_Q80", "rgb8_33x130_Q0", "rgb8_97x61_Q100_90", "rgb8_97x61_Q97p5"} <= names
    for e in FIXTURES:   # Quantize (5) is the last transform, behind Squeeze (7) or YCoCg (1)
        assert e["transforms"][-1] == 5, e["name"]


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_quantization_constants_are_the_reference_clis(gpulib, entry):
    kw = entry["encode"]
    colour = kw.get("ycocg", True)
    assert entry["channels"], "a fixture without a single coded constant pins nothing"
    for ch in entry["channels"]:
        chroma = colour and ch["component"] in (1, 2)
        q = gpulib.quantization_constant(kw["quality"], kw.get("chroma_quality"), squeeze=kw.get("squeeze", True), chroma_table=chroma,
                                         shift=ch["hcshift"] + ch["vcshift"])
        assert q == ch["q"], (entry["name"], ch)


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_writer_writes_the_reference_clis_lossy_bytes(gpulib, entry):
    img, bits = fixture_picture(entry)
    theirs = open(os.path.join(LOSSY, entry["file"]), "rb").read()
    mine = gpulib.encode_image(img, bits, tree_mode=0, **entry["encode"])
    assert same_up_to_the_stray_byte(mine, theirs), entry["name"]


@pytest.mark.parametrize("w,h,c,bits,seed,q_arg,extra,kw", [
    (71, 53, 3, 8, 501, "88", [], dict(quality=88)),
    (50, 90, 3, 8, 502, "42.25,63", [], dict(quality=42.25, chroma_quality=63)),
    (66, 34, 1, 8, 503, "12", [], dict(quality=12)),
    (48, 40, 4, 14, 504, "75,101", [], dict(quality=75, chroma_quality=101)),
    (37, 29, 2, 8, 505, "55", ["-R", "0"], dict(quality=55, squeeze=False)),
])
def test_fresh_pictures_against_the_live_reference_cli(gpulib, ref, tmp_path, w, h, c, bits, seed, q_arg, extra, kw):
    from oracle_py import ref_cli, run_ref_cli
    if ref_cli() is None:
        pytest.skip("reference CLI not built")
    img = photographic(w, h, c, bits, seed=seed)
    src = str(tmp_path / ("in.pam" if c in (2, 4) else "in.ppm" if c == 3 else "in.pgm"))
    write_pnm(src, img, (1 << bits) - 1)
    out = str(tmp_path / "ref.fuif")
    r = run_ref_cli(["-I", "0", "-K", "0", "-X", "0", "-Y", "0", "-Q", q_arg] + extra + [src, out])
    assert r.returncode == 0, r.stderr
    mine = gpulib.encode_image(img, bits, tree_mode=0, **kw)
    assert same_up_to_the_stray_byte(mine, open(out, "rb").read())


def test_quality_100_and_none_write_the_lossless_bytes(gpulib):
    img = photographic(97, 61, 3, 8, seed=2)
    for tree_mode in (0, 1):
        lossless = gpulib.encode_image(img, 8, tree_mode=tree_mode, index=True)
        assert gpulib.encode_image(img, 8, tree_mode=tree_mode, index=True, quality=None, chroma_quality=None) == lossless
        assert gpulib.encode_image(img, 8, tree_mode=tree_mode, index=True, quality=100) == lossless
        assert gpulib.encode_image(img, 8, tree_mode=tree_mode, index=True, quality=100, chroma_quality=100) == lossless
        assert gpulib.encode_image(img, 8, tree_mode=tree_mode, index=True, quality=100, chroma_quality=250) == lossless
        assert gpulib.encode_image(img, 8, tree_mode=tree_mode, index=True, quality=100, chroma_quality=99) != lossless
    # the C entry point with lossy == NULL
    L = gpulib.lib()
    planes = np.ascontiguousarray(img, dtype=np.int32)
    opt = gpulib.make_encode_options(1, 1, 12, 0, 4095, 0, 0, 0, 0)
    out, n = C.c_void_p(), C.c_size_t(0)
    assert L.fuifgpu_encode_image_lossy(planes.ctypes.data, 97, 61, 3, 8, C.byref(opt), None, C.byref(out), C.byref(n)) == 0
    blob = C.string_at(out.value, n.value)
    L.fuifgpu_free_blob(out)
    assert blob == gpulib.encode_image(img, 8, tree_mode=0)


@pytest.mark.parametrize("w,h,c,bits,kw", [(97, 61, 3, 8, dict(quality=80)), (80, 72, 4, 14, dict(quality=35, chroma_quality=70)),
                                           (64, 48, 1, 8, dict(quality=60, squeeze=False)), (40, 36, 2, 8, dict(quality=20))])
def test_learned_tree_lossy_streams_decode_the_same_with_port_and_reference(gpulib, port, ref, w, h, c, bits, kw):
    img = photographic(w, h, c, bits, seed=600 + w)
    blob = gpulib.encode_image(img, bits, tree_mode=1, index=True, **kw)
    p0, p1 = port.decode_both(blob)
    r0, r1 = ref.decode_both(blob)
    assert p0.ok and r0.ok and p1.ok and r1.ok
    assert [t[0] for t in p0.transforms][-1] == 5
    for a, b in ((p0, r0), (p1, r1)):
        assert len(a.channels) == len(b.channels)
        assert all(np.array_equal(x["data"], y["data"]) for x, y in zip(a.channels, b.channels))
    assert all(x["q"] == y["q"] for x, y in zip(p0.channels, r0.channels))
    assert p1.channels[0]["data"].shape == (h, w)


def test_higher_quality_is_larger_and_closer(gpulib, port):
    img = photographic(256, 192, 3, 8, seed=77)
    size, mse = {}, {}
    for q in (90, 50):
        blob = gpulib.encode_image(img, 8, tree_mode=1, quality=q)
        d = port.decode(blob)
        assert d.ok
        rec = np.stack([ch["data"] for ch in d.channels[:3]]).astype(np.float64)
        size[q], mse[q] = len(blob), ((rec - img) ** 2).mean()
    assert size[90] > size[50] and mse[90] < mse[50]
    assert 0 < mse[90]


def _call_lossy(gpulib, struct_size, quality, chroma_quality):
    L = gpulib.lib()
    planes = np.ascontiguousarray(photographic(24, 20, 3, 8, seed=9), dtype=np.int32)
    lossy = gpulib.LossyOptions(struct_size, quality, chroma_quality)
    out, n = C.c_void_p(), C.c_size_t(0)
    rc = L.fuifgpu_encode_image_lossy(planes.ctypes.data, 24, 20, 3, 8, None, C.byref(lossy), C.byref(out), C.byref(n))
    if rc == 0:
        L.fuifgpu_free_blob(out)
    ptrs, outs, sizes = (C.c_void_p * 1)(planes.ctypes.data), (C.c_void_p * 1)(), (C.c_size_t * 1)()
    opt = gpulib.make_encode_options(1, 1, 12, 1, 4095, 0, 0, 0, 0)     # (host pixel loop: an argument error is found before any GPU work)
    rc_batch = L.fuifgpu_encode_images_lossy(ptrs, 1, 24, 20, 3, 8, C.byref(opt), C.byref(lossy), outs, sizes)
    if rc_batch == 0:
        L.fuifgpu_free_blob(C.c_void_p(outs[0]))
    return rc, rc_batch


def test_argument_errors(gpulib):
    E_ARG = 4
    nan = float("nan")
    for size, q, cq in ((12, nan, 50.0), (12, 50.0, nan), (12, -1.0, 50.0), (12, 50.0, -0.5), (12, 100.5, 50.0), (0, 80.0, 80.0), (10, 80.0, 80.0),
                        (6, 80.0, 80.0), (4, 80.0, 80.0)):
        rc, rc_batch = _call_lossy(gpulib, size, q, cq)
        assert rc == E_ARG, (size, q, cq)
        assert rc_batch == E_ARG, (size, q, cq)
    assert _call_lossy(gpulib, 12, 80.0, 101.0)[0] == 0
    assert _call_lossy(gpulib, 8, 80.0, 0.0)[0] == 0          # a caller whose struct ends before chroma_quality: same as quality
    assert _call_lossy(gpulib, 16, 80.0, 60.0)[0] == 0        # a caller with a LARGER (later) struct: what this library knows is read
    for bad in ((nan, 50.0, 0), (50.0, nan, 0), (-3.0, 50.0, 0), (50.0, -3.0, 0), (101.0, 50.0, 0), (50.0, 50.0, -1)):
        assert gpulib.lib().fuifgpu_quantization_constant(bad[0], bad[1], 1, 0, bad[2]) == -E_ARG
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_image(photographic(24, 20, 3, 8, seed=9), 8, quality=-5)
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_images([photographic(24, 20, 3, 8, seed=9)], 8, quality=nan, gpu_forward=False)
    # the helper: 1 without loss, the shift is capped at 15 (fuif.cpp:495), a struct that ends early means the same as chroma > 100
    assert gpulib.quantization_constant(100) == 1 and gpulib.quantization_constant(100, 100, chroma_table=True, shift=0) == 1
    assert gpulib.quantization_constant(50, shift=40) == gpulib.quantization_constant(50, shift=15) == 1
    assert gpulib.quantization_constant(50, shift=0) == 58 and gpulib.quantization_constant(50, chroma_table=True, shift=0) == 307


def test_gpu_forward_with_a_quality_fails_loudly_without_a_gpu(gpulib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    img = photographic(64, 48, 3, 8, seed=1)
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.encode_image(img, 8, gpu_forward=True, quality=80)
    assert "HIP" in str(e.value)
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.encode_images([img], 8, gpu_forward=True, quality=80)
    assert "HIP" in str(e.value)


def test_gpu_lossy_tests_pass_on_the_wavefront_emulator():
    """tests/test_gpu_lossy_encoder.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_fwd_quantize's division and its block reduction, the channel table and the zero-channel shortcut, checked without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_lossy_encoder.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
