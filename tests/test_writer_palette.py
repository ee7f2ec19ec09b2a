"""CPU: Palette and channel compaction of the product's writer (fuifgpu_encode_image_ex, csrc/writer.cpp) against the REAL reference.

The yardstick is the reference CLI's bytes: tests/golden/palette/ holds what the unmodified `fuif -I 0 [...]` wrote for pictures that are
not photographs (tests/golden/make_golden_palette.py), with the transform list and every coded channel as the reference's own decoder
reports them.  With single-leaf trees (tree_mode 0) the host route must reproduce those files byte for byte -- which pins the order of
the attempts (fuif.cpp:374-430), the limit's float arithmetic, the palette order (transform/palette.h:103), the Squeeze test on the
palette (fuif.cpp:453), the predictors (fuif.cpp:580-588), Quantize beside meta-channels and the lossy rule (fuif.cpp:345-350)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from fuif_amd.synth import from_recipe, graphic, photographic

PALETTE = os.path.join(GOLDEN, "palette")
with open(os.path.join(PALETTE, "manifest_palette.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
LOSSLESS = [e for e in FIXTURES if e["lossless"]]
GRAPHIC = [e for e in LOSSLESS if e["input"]["kind"] == "graphic" or e["input"]["kind"] == "stack"]
NEW_SYMBOLS = ("fuifgpu_encode_image_ex", "fuifgpu_encode_images_ex", "fuifgpu_fwd_palette")
E_ARG = 4


def golden(entry):
    with open(os.path.join(PALETTE, entry["file"]), "rb") as f:
        return f.read()


def first_rolled_back_group(port, blob):
    """offset of the first channel group that is stored uncompressed (compress bit 0, encoding.cpp:77) although it is not trivial, or None"""
    d = port.decode(blob, undo=False)
    for channel, offset in d.groups:
        if blob[offset] & 1 == 0 and d.channels[channel]["minval"] < d.channels[channel]["maxval"]:
            return offset
    return None


def same_stream(port, mine, theirs):
    """The reference's BlobIO reports its high-water mark plus one (bytes_used = seek_pos + 1, fileio.h:241-251): one stray byte behind every
    stream (tests/test_writer.py's comparison).  When a group was rolled back to "uncompressed" (encoding.cpp:545-551) the mark is where
    its longer compressed attempt ended, which can lie behind the end of a short stream (a 3x3 palette in front of a 5x4 picture): the
    file then ends with what is left of that attempt.  The writer's stream is everything in front of that."""
    if mine != theirs[: len(mine)]:
        return False
    tail = len(theirs) - len(mine)
    if 0 <= tail <= 1:
        return True
    rolled_back = first_rolled_back_group(port, theirs)
    return rolled_back is not None and port.decode(mine, undo=False).ok and tail < len(theirs) - rolled_back


def test_the_fixture_set_covers_every_row():
    assert len(FIXTURES) == 21 and all(os.path.getsize(os.path.join(PALETTE, e["file"])) == e["nbytes"] <= 16384 for e in FIXTURES)
    chains = {e["name"]: [t[:4] if t[0] == 6 else t[:1] for t in e["transforms"]] for e in FIXTURES}
    assert chains["rgb_120x90_pal35"] == [[1], [6, 0, 2, 35], [7]]
    assert chains["rgba_72x64_pal19"] == [[1], [6, 0, 3, 19], [7]]
    assert chains["gray_100x70_compact19_nosqueeze"] == [[6, 0, 0, 19]]                       # a 19x1 palette switches Squeeze off
    assert chains["rgb_64x48_pal11_R0"] == [[1], [6, 0, 2, 11]]
    assert chains["rgb_96x72_sparse_compact3"] == [[1], [6, 0, 0, 57], [6, 1, 1, 38], [6, 2, 2, 67], [7]]
    assert chains["rgb_96x72_sparse_K0_Q80"] == [[1], [6, 0, 0, 57], [6, 1, 1, 38], [6, 2, 2, 67], [7], [5]]
    assert chains["rgb_96x72_sparse_Q80"] == [[1], [7], [5]]                                  # -K > 0 and a quality: no palettes at all
    assert chains["gray12_24x50_precompact"] == [[6, 0, 0, 755], [7]] and chains["gray14_40x36_precompact"] == [[6, 0, 0, 1247], [7]]
    assert chains["rgb_64x64_precompact_then_pal88"] == [[6, 1, 1, 77], [1], [6, 0, 2, 88], [7]]   # compaction BEFORE YCoCg on a 0..255 channel
    assert chains["rgb_64x64_pal88_C0"] == [[6, 0, 2, 88], [7]]
    assert chains["rgb_64x64_K35_exact"] == [[1], [6, 0, 2, 35], [7]]
    assert chains["rgb_64x64_K34_one_short"] == chains["rgb_64x64_K16"] == [[1], [6, 0, 0, 32], [6, 1, 1, 35], [6, 2, 2, 34], [7]]
    assert chains["rgba_72x64_pal28_photo_alpha"] == [[1], [6, 0, 2, 28], [7]]                # all channels fail, all but the last succeed
    assert chains["graya_40x36_pal9_nosqueeze"] == [[6, 0, 1, 9]]
    assert chains["rgb_30x40_flat77"] == [[1], [6, 0, 2, 1]] and chains["rgb_40x30_two_colours"] == [[1], [6, 0, 2, 2]]
    assert chains["rgb_5x4_pal3"] == [[1], [6, 0, 2, 3]]
    assert chains["gray_30x40_flat9_compaction_fails"] == [[7]]                               # (int)(0.7f * 1) = 0 colours allowed
    e = FIXTURES[0]
    assert e["nb_coded_channels"] == 10 and e["channels"][0] == dict(w=35, h=3, hshift=-1, vshift=0, minval=-233, maxval=233, q=1)


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_host_route_writes_the_reference_clis_bytes(gpulib, port, entry):
    img = from_recipe(entry["input"])
    mine = gpulib.encode_image(img, entry["bits"], tree_mode=0, **entry["encode"])
    assert same_stream(port, mine, golden(entry)), entry["name"]


@pytest.mark.parametrize("entry", LOSSLESS, ids=[e["name"] for e in LOSSLESS])
def test_learned_tree_streams_decode_to_the_source_with_port_and_reference(gpulib, port, ref, entry):
    img = from_recipe(entry["input"])
    blob = gpulib.encode_image(img, entry["bits"], tree_mode=1, index=True, **entry["encode"])
    for dec in (port, ref):
        pre, post = dec.decode_both(blob)
        assert pre.ok and post.ok
        assert [[t[0]] + list(t[1]) for t in pre.transforms] == entry["transforms"]
        assert len(pre.channels) == entry["nb_coded_channels"]
        assert len(post.channels) == img.shape[0]
        for c in range(img.shape[0]):
            assert np.array_equal(post.channels[c]["data"], img[c]), (entry["name"], c)


@pytest.mark.parametrize("entry", GRAPHIC, ids=[e["name"] for e in GRAPHIC])
def test_palette_streams_of_graphics_are_smaller(gpulib, entry):
    img = from_recipe(entry["input"])
    kw = dict(entry["encode"])
    with_options = gpulib.encode_image(img, entry["bits"], tree_mode=1, **kw)
    kw.update(palette_colors=0, compact_post=0, compact_pre=0)
    assert len(with_options) < len(gpulib.encode_image(img, entry["bits"], tree_mode=1, **kw)), entry["name"]


def _call_ex(gpulib, img, bits, struct_size, colors, post, pre, lossy=None, opt=None):
    """(return code, blob) of fuifgpu_encode_image_ex and of fuifgpu_encode_images_ex (host planes, host pixel loop) for one picture"""
    L = gpulib.lib()
    planes = np.ascontiguousarray(img, dtype=np.int32)
    c, h, w = planes.shape
    pal = None if struct_size is None else C.byref(gpulib.PaletteOptions(struct_size, colors, post, pre))
    opt = opt or gpulib.make_encode_options(1, 1, 12, 0, 4095, 0, 0, 0, 0)
    lossy = None if lossy is None else C.byref(gpulib.make_lossy_options(*lossy))
    out, n = C.c_void_p(), C.c_size_t(0)
    rc = L.fuifgpu_encode_image_ex(planes.ctypes.data, w, h, c, bits, C.byref(opt), lossy, pal, C.byref(out), C.byref(n))
    blob = None
    if rc == 0:
        blob = C.string_at(out.value, n.value)
        L.fuifgpu_free_blob(out)
    ptrs, outs, sizes = (C.c_void_p * 1)(planes.ctypes.data), (C.c_void_p * 1)(), (C.c_size_t * 1)()
    rc_batch = L.fuifgpu_encode_images_ex(ptrs, 0, 1, w, h, c, bits, C.byref(opt), lossy, pal, outs, sizes)   # (an argument error is found before any GPU work)
    if rc_batch == 0:
        L.fuifgpu_free_blob(C.c_void_p(outs[0]))
    return rc, rc_batch, blob


def test_null_and_all_zero_options_write_the_bytes_of_the_existing_entry_points(gpulib):
    for img, bits in ((graphic(64, 48, 3, 8, seed=35, colors=12), 8), (photographic(40, 36, 1, 14, seed=4), 14)):
        plain = gpulib.encode_image(img, bits, tree_mode=0)
        assert _call_ex(gpulib, img, bits, None, 0, 0.0, 0.0)[2] == plain
        assert _call_ex(gpulib, img, bits, 16, 0, 0.0, 0.0)[2] == plain
        assert gpulib.encode_image(img, bits, tree_mode=0, palette_colors=0, compact_post=0.0, compact_pre=0.0) == plain
        assert gpulib.encode_image(img, bits, tree_mode=0, palette_colors=256, compact_post=70, compact_pre=70) != plain
        lossy = gpulib.encode_image(img, bits, tree_mode=0, quality=80)
        assert _call_ex(gpulib, img, bits, None, 0, 0.0, 0.0, lossy=(80, None))[2] == lossy
        assert _call_ex(gpulib, img, bits, 16, 0, 0.0, 0.0, lossy=(80, None))[2] == lossy


def test_a_truncated_struct_reads_the_missing_fields_as_zero(gpulib):
    img = from_recipe(dict(kind="photographic", w=96, h=72, channels=3, bits=8, seed=37, floor_to=8))
    full = lambda *a: _call_ex(gpulib, img, 8, *a)[2]
    assert full(4, 256, 70.0, 70.0) == full(16, 0, 0.0, 0.0)             # only struct_size: everything off
    assert full(8, 256, 70.0, 70.0) == full(16, 256, 0.0, 0.0)           # ends behind palette_colors
    assert full(12, 0, 70.0, 70.0) == full(16, 0, 70.0, 0.0)             # ends behind compact_post_percent
    assert full(12, 0, 70.0, 70.0) != full(16, 0, 0.0, 0.0)
    assert full(24, 256, 70.0, 70.0) == full(16, 256, 70.0, 70.0)        # a LARGER (later) struct: what this library knows is read


def test_argument_errors(gpulib):
    img = graphic(24, 20, 3, 8, seed=9, colors=5)
    nan = float("nan")
    for size, colors, post, pre in ((16, -1, 0.0, 0.0), (16, 32768, 0.0, 0.0), (16, 256, nan, 0.0), (16, 256, 0.0, nan), (16, 0, -0.5, 0.0),
                                    (16, 0, 0.0, -1.0), (16, 0, 100.5, 0.0), (16, 0, 0.0, 101.0), (0, 256, 70.0, 70.0), (2, 256, 70.0, 70.0),
                                    (10, 256, 70.0, 70.0)):
        rc, rc_batch, _ = _call_ex(gpulib, img, 8, size, colors, post, pre)
        assert rc == E_ARG and rc_batch == E_ARG, (size, colors, post, pre)
    assert _call_ex(gpulib, img, 8, 16, 32767, 100.0, 100.0)[0] == 0
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_image(img, 8, palette_colors=-3)
    with pytest.raises(gpulib.FuifGpuError):
        gpulib.encode_images([img], 8, compact_post=nan, gpu_forward=False)
    # the raw transform: nb outside 1..4, a negative count, a NULL pointer with work to do (all found before any GPU work)
    L = gpulib.lib()
    count = C.c_int(7)
    ptrs = (C.c_void_p * 5)(8, 8, 8, 8, 8)
    pal = np.zeros(64, np.int32)
    for nb, n, colors, index, palette, cnt in ((0, 10, 4, 8, pal.ctypes.data, C.byref(count)), (5, 10, 4, 8, pal.ctypes.data, C.byref(count)),
                                               (2, -1, 4, 8, pal.ctypes.data, C.byref(count)), (2, 10, -1, 8, pal.ctypes.data, C.byref(count)),
                                               (2, 10, 4, None, pal.ctypes.data, C.byref(count)), (2, 10, 4, 8, None, C.byref(count)),
                                               (2, 10, 4, 8, pal.ctypes.data, None)):
        assert L.fuifgpu_fwd_palette(ptrs, nb, n, colors, index, palette, cnt, None) == E_ARG, (nb, n, colors)
    null_plane = (C.c_void_p * 2)(8, None)
    assert L.fuifgpu_fwd_palette(null_plane, 2, 10, 4, 8, pal.ctypes.data, C.byref(count), None) == E_ARG
    assert L.fuifgpu_fwd_palette(None, 2, 10, 4, 8, pal.ctypes.data, C.byref(count), None) == E_ARG
    assert L.fuifgpu_fwd_palette(None, 2, 0, 4, None, None, C.byref(count), None) == 0 and count.value == 0   # no work: nothing is touched


def test_a_quality_with_a_palette_switches_all_three_options_off(gpulib, port):
    entry = {e["name"]: e for e in FIXTURES}
    img = from_recipe(entry["rgb_96x72_sparse_Q80"]["input"])
    lossy = gpulib.encode_image(img, 8, tree_mode=0, quality=80)
    assert gpulib.encode_image(img, 8, tree_mode=0, quality=80, palette_colors=256, compact_post=70, compact_pre=70) == lossy
    assert gpulib.encode_image(img, 8, tree_mode=0, quality=80, palette_colors=256) == lossy
    assert gpulib.encode_image(img, 8, tree_mode=0, quality=100, chroma_quality=90, palette_colors=256, compact_post=70) != \
        gpulib.encode_image(img, 8, tree_mode=0, quality=100, chroma_quality=90)               # only `quality` is looked at (fuif.cpp:345)
    kept = gpulib.encode_image(img, 8, tree_mode=0, quality=80, palette_colors=0, compact_post=70)
    assert same_stream(port, kept, golden(entry["rgb_96x72_sparse_K0_Q80"]))


def test_batch_writer_on_the_host_planes_needs_a_gpu_and_says_so(gpulib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    img = graphic(64, 48, 3, 8, seed=35, colors=12)
    for call in (lambda: gpulib.encode_image(img, 8, gpu_forward=True, palette_colors=256),
                 lambda: gpulib.encode_images([img], 8, palette_colors=256),
                 lambda: gpulib.encode_images_device([np.ascontiguousarray(img).ctypes.data], 64, 48, 3, 8, palette_colors=256)):
        with pytest.raises(gpulib.FuifGpuError) as e:
            call()
        assert e.value.code == 5 and "HIP" in str(e.value)     # FUIFGPU_E_HIP: no silent host route behind the kernels


def test_new_entry_points_are_exported_and_declared(gpulib):
    hdr = open(os.path.join(ROOT, "include", "fuifgpu.h")).read()
    declared = set(re.findall(r"\b(fuifgpu_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(os.path.join(ROOT, "fuif_amd", "libfuifgpu.so"))
    for s in NEW_SYMBOLS:
        assert s in declared and s in gpulib.ABI_SYMBOLS and hasattr(L, s), s
    assert "fuifgpu_palette_options" in hdr and C.sizeof(gpulib.PaletteOptions) == 16
    assert gpulib.lib().fuifgpu_abi_version() == 3      # found by symbol lookup: the ABI version stays


def test_gpu_palette_tests_pass_on_the_wavefront_emulator():
    """tests/test_gpu_palette_encoder.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_palette_collect's table and its bounded probing, the bitmap form, k_palette_index and the writer's device-only index planes,
    checked without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_palette_encoder.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_route_runs_clean_under_the_address_and_ub_sanitizers(tmp_path, port):
    """tools/palette_host_check.cpp (its own main, no Python in the process) linked against the writer's sources and built with
    -fsanitize=address,undefined encodes the two smallest fixture pictures on the host route; its streams are the goldens'.
    The library's sources include the HIP runtime header, so this build takes the wavefront emulator's stand-in for it; the host route
    launches no kernel."""
    from test_emulated_kernels import CSRC, SOURCES
    exe = str(tmp_path / "palette_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFUIF_EMU", "-ffp-contract=off",
           "-Wno-attributes", "-I", os.path.join(ROOT, "tools", "emu"), "-I", os.path.join(ROOT, "include"), "-x", "c++"] + \
          [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "palette_host_check.cpp"),
                                                       "-o", exe]
    subprocess.check_call(cmd)
    smallest = sorted(FIXTURES, key=lambda e: from_recipe(e["input"]).size)[:2]
    for entry in smallest:
        img = np.ascontiguousarray(from_recipe(entry["input"]), dtype="<i4")
        c, h, w = img.shape
        src, dst = str(tmp_path / (entry["name"] + ".i32")), str(tmp_path / (entry["name"] + ".fuif"))
        img.tofile(src)
        kw = entry["encode"]
        r = subprocess.run([exe, src, str(w), str(h), str(c), str(entry["bits"]), str(kw["palette_colors"]), str(kw["compact_post"]),
                            str(kw["compact_pre"]), dst], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
        assert same_stream(port, open(dst, "rb").read(), golden(entry)), entry["name"]
