"""CPU: animations of the product's writer (fuifgpu_encode_animation, csrc/writer.cpp) against the REAL reference.

The yardstick is the reference CLI's bytes: tests/golden/animation/ holds what the unmodified `fuif -I 0 [...] frame-%02d.ppm` wrote for
seeded film strips (tests/golden/make_golden_animation.py), with the transform list and every coded channel as the reference's own decoder
reports them.  With single-leaf trees (tree_mode 0) the host route must reproduce those files byte for byte -- which pins the FUAF header
(encoding.cpp:458-473), the place of the Matching transform in the chain (fuif.cpp:440-448), its run rule, erode and offset code
(transform/2dmatch.h:303-381), the match channel in front of the palettes, its predictor, and Quantize beside it."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from fuif_amd.synth import filmstrip, from_recipe
from test_writer_palette import same_stream

ANIMATION = os.path.join(GOLDEN, "animation")
with open(os.path.join(ANIMATION, "manifest_animation.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
BY_NAME = {e["name"]: e for e in FIXTURES}
LOSSLESS = [e for e in FIXTURES if e["lossless"]]
NEW_SYMBOLS = ("fuifgpu_encode_animation", "fuifgpu_encode_animations", "fuifgpu_fwd_match_frames")
E_ARG = 4


def golden(entry):
    with open(os.path.join(ANIMATION, entry["file"]), "rb") as f:
        return f.read()


def test_the_fixture_set_covers_every_row():
    assert len(FIXTURES) == 11 and all(os.path.getsize(os.path.join(ANIMATION, e["file"])) == e["nbytes"] <= 16384 for e in FIXTURES)
    ids = {e["name"]: [t[0] for t in e["transforms"]] for e in FIXTURES}
    flags = {e["name"]: e["flags"][2:] for e in FIXTURES}
    assert all(e["flags"][:2] == ["-I", "0"] for e in FIXTURES)
    assert ids["rgb_48x8x3_defaults"] == [1, 6, 6, 8, 7] and flags["rgb_48x8x3_defaults"] == []        # Co and Cg are compacted; the match comes behind
    assert ids["rgb_48x8x3_K0X0Y0"] == [1, 8, 7] and flags["rgb_48x8x3_K0X0Y0"] == ["-K", "0", "-X", "0", "-Y", "0"]
    assert ids["rgb_48x8x3_R0"] == [1, 6, 6, 8] and flags["rgb_48x8x3_R0"] == ["-R", "0"]
    assert ids["rgb_48x8x3_M0"] == [1, 6, 6, 7] and flags["rgb_48x8x3_M0"] == ["-M", "0"]
    assert ids["rgb_48x8x3_F25"] == ids["rgb_48x8x3_defaults"] and flags["rgb_48x8x3_F25"] == ["-F", "25"]
    assert ids["rgb_48x8x3_Q80"] == [1, 8, 7, 5] and flags["rgb_48x8x3_Q80"] == ["-Q", "80"]           # the lossy rule clears the palette options
    assert ids["graphic_48x7x4_palette"] == [1, 6, 8, 7] and BY_NAME["graphic_48x7x4_palette"]["transforms"][1] == [6, 0, 2, 16]
    assert ids["gray_300x7x2"] == [8, 7] and ids["rgba_48x7x2"] == [6, 1, 6, 6, 8, 7]
    assert len({json.dumps(e["input"], sort_keys=True) for e in FIXTURES[:6]}) == 1                      # one strip under six sets of flags
    # shapes: both forms of the offset code, the three values of minmatchcount that matter, 2 to 4 frames
    assert {e["frame_h"] for e in FIXTURES} >= {7, 8} and {e["input"]["w"] for e in FIXTURES} == {48, 300, 2100} and {e["frames"] for e in FIXTURES} == {2, 3, 4}
    for e in FIXTURES:
        if 8 in ids[e["name"]]:
            m = e["channels"][0]   # the match channel leads, in front of every palette
            fh = e["frame_h"]
            assert (m["w"], m["h"], m["hshift"], m["minval"], m["maxval"], m["q"]) == (e["input"]["w"], fh * e["frames"], 0, 0, 1, 2 * fh * fh + (fh & 1)), e["name"]
    m = BY_NAME["graphic_48x7x4_palette"]["channels"]
    assert m[0]["q"] == 99 and (m[1]["w"], m[1]["h"], m[1]["hshift"]) == (16, 3, -1)
    # the conditions on the rows without Squeeze
    r0 = [e for e in FIXTURES if "match_zeroed" in e]
    assert len(r0) == 3 and all(e["match_nonzero"] > e["match_zeroed"] for e in r0)
    for width in (48, 300, 2100):
        assert any(e["input"]["w"] == width and e["match_zeroed"] > 0 for e in r0), width
    assert any(e["a_run_crosses_sample_64"] for e in r0)
    runs = BY_NAME["gray_2100x4x2_R0"]["run_lengths"]
    assert 40 in runs and 39 not in runs                                                                 # the run of 39 is one short of clamp(2100 / 50, 5, 40)
    assert min(BY_NAME["rgb_48x8x3_R0"]["run_lengths"]) >= 5 and min(BY_NAME["rgb_300x8x2_R0"]["run_lengths"]) >= 6


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_host_route_writes_the_reference_clis_bytes(gpulib, port, entry):
    frames = from_recipe(entry["input"])
    mine = gpulib.encode_animation(frames, tree_mode=0, **entry["encode"])
    assert mine[:4] == b"FUAF" and same_stream(port, mine, golden(entry)), entry["name"]


def test_match_previous_false_is_the_M0_file_and_the_frame_rate_is_in_the_header(gpulib, port):
    frames = from_recipe(BY_NAME["rgb_48x8x3_M0"]["input"])
    kw = dict(tree_mode=0, palette_colors=256, compact_post=70, compact_pre=70)
    off = gpulib.encode_animation(frames, match_previous=False, **kw)
    assert same_stream(port, off, golden(BY_NAME["rgb_48x8x3_M0"]))
    on = gpulib.encode_animation(frames, **kw)
    assert on != off and len(on) < len(off)
    f25 = gpulib.encode_animation(frames, framerate=25, **kw)
    assert same_stream(port, f25, golden(BY_NAME["rgb_48x8x3_F25"]))
    assert gpulib.encode_animation(frames, framerate=10, **kw) == on and gpulib.encode_animation(frames, framerate=0, **kw) == on
    differ = [k for k in range(len(on)) if on[k] != f25[k]]
    assert len(on) == len(f25) and differ == [9] and (on[9], f25[9]) == (9, 24)      # FUAF, 4 one-byte varints, frames-2, then den-1


def test_one_frame_is_what_encode_image_writes(gpulib):
    frames = from_recipe(BY_NAME["rgb_48x8x3_defaults"]["input"])
    for kw in (dict(), dict(palette_colors=256, compact_post=70, compact_pre=70), dict(quality=80)):
        still = gpulib.encode_image(frames[1], 8, tree_mode=0, **kw)
        assert still[:4] == b"FUIF"
        assert gpulib.encode_animation(frames[1:2], tree_mode=0, **kw) == still
        assert gpulib.encode_animation(frames[1:2], tree_mode=0, framerate=25, match_previous=False, **kw) == still


def _call(gpulib, frames, struct_size, nb_frames, framerate, match_previous, frame_h=None):
    """return codes of fuifgpu_encode_animation and fuifgpu_encode_animations (host frames; an argument error is found before any GPU work)"""
    L = gpulib.lib()
    frames = np.ascontiguousarray(frames, dtype=np.int32)
    _, c, h, w = frames.shape
    anim = None if struct_size is None else C.byref(gpulib.AnimationOptions(struct_size, nb_frames, framerate, match_previous))
    opt = gpulib.make_encode_options(1, 1, 12, 0, 4095, 0, 0, 0, 0)
    out, n = C.c_void_p(), C.c_size_t(0)
    rc = L.fuifgpu_encode_animation(frames.ctypes.data, w, frame_h or h, c, 8, C.byref(opt), None, None, anim, C.byref(out), C.byref(n))
    if rc == 0:
        L.fuifgpu_free_blob(out)
    ptrs, outs, sizes = (C.c_void_p * 1)(frames.ctypes.data), (C.c_void_p * 1)(), (C.c_size_t * 1)()
    rc_batch = L.fuifgpu_encode_animations(ptrs, 0, 1, w, frame_h or h, c, 8, C.byref(opt), None, None, anim, outs, sizes)
    if rc_batch == 0:
        L.fuifgpu_free_blob(C.c_void_p(outs[0]))
    return rc, rc_batch


def test_argument_errors(gpulib):
    frames = filmstrip(24, 6, frames=2, channels=1, seed=3)
    assert _call(gpulib, frames, 16, 2, 0, 1)[0] == 0 and _call(gpulib, frames, None, 0, 0, 0)[0] == 0
    for size, nf, rate, match in ((16, 0, 0, 1), (16, -1, 0, 1), (16, 2, -1, 1), (16, 2, 0, 2), (16, 2, 0, -1), (16, 2, 0, -2), (0, 2, 0, 1), (8, 2, 0, 1),
                                  (12, 2, 0, 1), (18, 2, 0, 1)):
        assert _call(gpulib, frames, size, nf, rate, match) == (E_ARG, E_ARG), (size, nf, rate, match)
    assert _call(gpulib, frames, 24, 2, 0, 1)[0] == 0                                  # a LARGER (later) struct: what this library knows is read
    # a strip higher than the format holds: more than 2^31-1 samples in a channel, or a frame whose offset code is no int
    assert _call(gpulib, frames, 16, 1 << 27, 0, 1) == (E_ARG, E_ARG)
    assert _call(gpulib, frames, 16, 2, 0, 1, frame_h=32768) == (E_ARG, E_ARG)
    # the deeper distances are refused with a reason
    assert _call(gpulib, frames, 16, 2, 0, 2)[0] == E_ARG
    message = gpulib.lib().fuifgpu_last_error().decode()
    assert "deeper distances" in message and "back-fill" in message
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.encode_animation(frames, match_previous=-2)
    assert e.value.code == E_ARG and "never compared" in str(e.value)
    for bad in (dict(framerate=float("nan")), dict(framerate=float("inf")), dict(framerate=-5), dict(framerate=2.5), dict(quality=float("nan")),
                dict(quality=-1), dict(compact_post=float("nan")), dict(palette_colors=-3)):
        with pytest.raises(gpulib.FuifGpuError) as e:
            gpulib.encode_animation(frames, **bad)
        assert e.value.code == E_ARG, bad
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_animation(frames[:0])                                            # zero frames
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_animation(frames[0])                                             # not (F, C, H, W)
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_animations([frames, frames[:1]])
    # the raw transform: found before any GPU work
    L = gpulib.lib()
    ptrs = (C.c_void_p * 9)(*([8] * 9))
    for nb, w, h, nf, match in ((0, 8, 8, 2, 8), (9, 8, 8, 2, 8), (1, 0, 8, 2, 8), (1, 8, 0, 2, 8), (1, 8, 8, 1, 8), (1, 8, 9, 2, 8), (1, 8, 8, 2, None),
                                (1, 65536, 65536, 2, 8)):
        assert L.fuifgpu_fwd_match_frames(ptrs, nb, w, h, nf, match, None) == E_ARG, (nb, w, h, nf)
    assert L.fuifgpu_fwd_match_frames(None, 1, 8, 8, 2, 8, None) == E_ARG
    assert L.fuifgpu_fwd_match_frames((C.c_void_p * 2)(8, None), 2, 8, 8, 2, 8, None) == E_ARG


def test_gpu_routes_need_a_gpu_and_say_so(gpulib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    frames = filmstrip(24, 6, frames=2, channels=1, seed=3)
    for call in (lambda: gpulib.encode_animation(frames, gpu_forward=True), lambda: gpulib.encode_animations([frames]),
                 lambda: gpulib.encode_animations_device([frames.ctypes.data], 2, 24, 6, 1)):
        with pytest.raises(gpulib.FuifGpuError) as e:
            call()
        assert e.value.code == 5 and "HIP" in str(e.value)     # FUIFGPU_E_HIP: no silent host route behind the kernels


def test_new_entry_points_are_exported_and_declared(gpulib):
    hdr = open(os.path.join(ROOT, "include", "fuifgpu.h")).read()
    declared = set(re.findall(r"\b(fuifgpu_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(os.path.join(ROOT, "fuif_amd", "libfuifgpu.so"))
    for s in NEW_SYMBOLS:
        assert s in declared and s in gpulib.ABI_SYMBOLS and hasattr(L, s), s
    assert "fuifgpu_animation_options" in hdr and C.sizeof(gpulib.AnimationOptions) == 16
    assert gpulib.lib().fuifgpu_abi_version() == 3      # found by symbol lookup: the ABI version stays


@pytest.mark.parametrize("entry", LOSSLESS, ids=[e["name"] for e in LOSSLESS])
def test_learned_tree_streams_decode_to_the_source_with_port_and_reference(gpulib, port, ref, entry):
    frames = from_recipe(entry["input"])
    nf, c, fh, w = frames.shape
    blob = gpulib.encode_animation(frames, tree_mode=1, index=True, split_bits=2, **entry["encode"])
    for dec in (port, ref):
        pre, post = dec.decode_both(blob)
        assert pre.ok and post.ok
        assert [t[0] for t in pre.transforms] == [t[0] for t in entry["transforms"]]
        assert len(pre.channels) == entry["nb_coded_channels"] and len(post.channels) == c
        for k in range(c):
            assert np.array_equal(np.asarray(post.channels[k]["data"]).reshape(nf, fh, w), frames[:, k]), (entry["name"], k)


def test_gpu_animation_tests_pass_on_the_wavefront_emulator():
    """tests/test_gpu_animation_encoder.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_match_frames_runs' ballots and carries, the erode's recursion, the apply pass and the writer's device-only match channel, checked
    without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_animation_encoder.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_route_runs_clean_under_the_address_and_ub_sanitizers(tmp_path, port):
    """tools/animation_host_check.cpp (its own main, no Python in the process) linked against the writer's sources and built with
    -fsanitize=address,undefined encodes the two smallest fixture clips on the host route; its streams are the goldens'.
    The library's sources include the HIP runtime header, so this build takes the wavefront emulator's stand-in for it; the host route
    launches no kernel."""
    from test_emulated_kernels import CSRC, SOURCES
    exe = str(tmp_path / "animation_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFUIF_EMU", "-ffp-contract=off",
           "-Wno-attributes", "-I", os.path.join(ROOT, "tools", "emu"), "-I", os.path.join(ROOT, "include"), "-x", "c++"] + \
          [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "animation_host_check.cpp"),
                                                       "-o", exe]
    subprocess.check_call(cmd)
    smallest = sorted(LOSSLESS, key=lambda e: from_recipe(e["input"]).size)[:2]
    assert [e["name"] for e in smallest] == ["rgba_48x7x2", "rgb_48x8x3_defaults"]
    for entry in smallest:
        frames = np.ascontiguousarray(from_recipe(entry["input"]), dtype="<i4")
        nf, c, fh, w = frames.shape
        src, dst = str(tmp_path / (entry["name"] + ".i32")), str(tmp_path / (entry["name"] + ".fuif"))
        frames.tofile(src)
        kw = entry["encode"]
        r = subprocess.run([exe, src, str(w), str(fh), str(c), str(nf), str(kw.get("framerate", 0)), str(int(kw.get("match_previous", True))),
                            str(kw["palette_colors"]), str(kw["compact_post"]), str(kw["compact_pre"]), str(int(kw.get("squeeze", True))), dst],
                           capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
        assert same_stream(port, open(dst, "rb").read(), golden(entry)), entry["name"]
