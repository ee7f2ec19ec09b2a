"""CPU: the planner's kept-transform schedules (fuifgpu_plan_create_keep, csrc/plan.cpp) against the plain-C oracle's
Image::undo_transforms(keep) (image/image.cpp:94-115), the size rules of the YUV 4:2:0 frame output, the new entry points of the ABI, and
tests/test_gpu_yuv_decode.py run against the wavefront emulator build."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

E_UNSUPPORTED, E_ARG = 3, 4
NEW_SYMBOLS = ["fuifgpu_plan_create_keep", "fuifgpu_plan_keep", "fuifgpu_plan_yuv420_bytes", "fuifgpu_batch_pack_yuv420",
               "fuifgpu_batch_download_yuv420", "fuifgpu_pack_yuv420"]
STREAMS = ["yuv/yuv8_97x61.fuif", "yuv/yuv8_5x4.fuif", "yuv/yuv8_1x1.fuif", "yuv/yuv10_75x49_Q60.fuif", "yuv/yuv8_96x60x3_M0.fuif",
           "jpeg420_256x192_q90.fuif",
           "rgb8_97x61.fuif",                       # YCoCg + Squeeze
           "pal_rgb_graphic_120x90.fuif",           # YCoCg, Palette, Squeeze: a meta-channel stays in front of the list
           "animation/rgb_48x8x3_defaults.fuif"]    # FUAF: YCoCg, two channel palettes, Matching, Squeeze
GEOMETRY = ("w", "h", "hshift", "vshift", "component")


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def test_the_stream_list_is_what_it_says(gpulib):
    ids = {name: [t[0] for t in gpulib.Plan(golden(name)).transforms] for name in STREAMS}
    assert ids["rgb8_97x61.fuif"] == [1, 7] and ids["pal_rgb_graphic_120x90.fuif"] == [1, 6, 7]
    assert ids["animation/rgb_48x8x3_defaults.fuif"] == [1, 6, 6, 8, 7] and golden("animation/rgb_48x8x3_defaults.fuif")[:4] == b"FUAF"
    assert ids["jpeg420_256x192_q90.fuif"] == [0, 3, 4, 5, 7] and ids["yuv/yuv10_75x49_Q60.fuif"] == [0, 3, 7, 5]


@pytest.mark.parametrize("name", STREAMS)
def test_output_channels_are_the_oracles_at_every_keep(gpulib, port, name):
    blob = golden(name)
    base = gpulib.Plan(blob)
    nt = base.info.nb_transforms
    signatures = {0: base.info.signature}
    for keep in range(nt + 1):
        plan = gpulib.Plan(blob, keep)
        want = port.decode(blob, keep=keep, want_data=False)
        assert want.ok and plan.keep == keep
        mine = plan.output_channels
        assert plan.info.nb_output_channels == len(mine) == len(want.channels), (name, keep)
        for c, (m, t) in enumerate(zip(mine, want.channels)):
            assert [m[k] for k in GEOMETRY] == [t[k] for k in GEOMETRY], (name, keep, c)
            if m["w"] * m["h"]:
                assert (m["hcshift"], m["vcshift"]) == (t["hcshift"], t["vcshift"]), (name, keep, c)
        # the planes lie one behind the other in the output slab, and out_elems holds them
        end = 0
        for m in mine:
            if m["w"] * m["h"]:
                assert m["offset"] >= end, (name, keep)
                end = m["offset"] + m["w"] * m["h"]
        assert end <= plan.info.out_elems, (name, keep)
        signatures[keep] = plan.info.signature
    assert len(set(signatures.values())) == nt + 1, name       # keep is part of the signature


def test_the_examples_of_the_shortened_schedules(gpulib):
    shapes = lambda name, keep: [(c["w"], c["h"]) for c in gpulib.Plan(golden(name), keep).output_channels]
    assert shapes("yuv/yuv8_97x61.fuif", 2) == [(97, 61), (49, 31), (49, 31)]
    assert len(shapes("jpeg420_256x192_q90.fuif", 3)) == 192 and len(shapes("jpeg420_256x192_q90.fuif", 5)) == 204
    assert shapes("jpeg420_256x192_q90.fuif", 2) == [(256, 192), (128, 96), (128, 96)]
    assert shapes("yuv/yuv8_96x60x3_M0.fuif", 2) == [(96, 180), (48, 90), (48, 90)]
    pal = gpulib.Plan(golden("pal_rgb_graphic_120x90.fuif"), 2).output_channels       # the palette first, then the index channel
    assert len(pal) == 2 and pal[0]["hshift"] == -1 and (pal[1]["w"], pal[1]["h"]) == (120, 90)
    # a schedule that keeps everything has as many ops as coded channels with samples: plain copies
    full = gpulib.Plan(golden("jpeg420_256x192_q90.fuif"), 5)
    assert full.info.nb_ops == sum(1 for c in full.coded_channels if c["w"] * c["h"]) and full.info.tmp_elems == 0
    # fewer transforms undone: a smaller output slab (no upsampled chroma)
    assert gpulib.Plan(golden("yuv/yuv8_97x61.fuif"), 2).info.out_elems < gpulib.Plan(golden("yuv/yuv8_97x61.fuif")).info.out_elems


@pytest.mark.parametrize("name", STREAMS)
def test_keep_0_is_the_plan_it_always_was(gpulib, name):
    blob = golden(name)
    a, b = gpulib.Plan(blob), gpulib.Plan(blob, 0)
    L = gpulib.lib()
    h = C.c_void_p()
    assert L.fuifgpu_plan_create_keep(blob, len(blob), 0, C.byref(h)) == 0
    try:
        info = gpulib.ImageInfo()
        assert L.fuifgpu_plan_info(h, C.byref(info)) == 0
        assert bytes(info) == bytes(a.info) == bytes(b.info)        # every field, signature and nb_ops among them
        k = C.c_int(-1)
        assert L.fuifgpu_plan_keep(h, C.byref(k)) == 0 and k.value == 0 and a.keep == 0
    finally:
        L.fuifgpu_plan_destroy(h)
    assert a.output_channels == b.output_channels and a.coded_channels == b.coded_channels


def test_keep_out_of_range(gpulib):
    L = gpulib.lib()
    for name in ("yuv/yuv8_97x61.fuif", "yuv/yuv8_1x1.fuif", "gray8_nosqueeze_60x40.fuif"):
        blob = golden(name)
        nt = gpulib.Plan(blob).info.nb_transforms
        for keep in (-1, nt + 1, 1 << 20):
            with pytest.raises(gpulib.FuifGpuError) as e:
                gpulib.Plan(blob, keep)
            assert e.value.code == E_ARG, (name, keep)
            h = C.c_void_p(1)
            assert L.fuifgpu_plan_create_keep(blob, len(blob), keep, C.byref(h)) == E_ARG and not h.value
        assert gpulib.Plan(blob, nt).keep == nt
    assert L.fuifgpu_plan_keep(None, None) == E_ARG


def frame_size(w, h, bits, layout, pitch_y, pitch_c):
    bps = 2 if bits > 8 else 1
    cw, ch = (w + 1) // 2, (h + 1) // 2
    py = pitch_y or w * bps
    pc = pitch_c or cw * bps * (2 if layout == "nv12" else 1)
    return py * h + pc * ch * (1 if layout == "nv12" else 2)


def test_yuv420_bytes(gpulib):
    for name, w, h, bits in (("yuv/yuv8_97x61.fuif", 97, 61, 8), ("yuv/yuv10_75x49_Q60.fuif", 75, 49, 10), ("yuv/yuv8_1x1.fuif", 1, 1, 8),
                             ("jpeg420_256x192_q90.fuif", 256, 192, 8)):
        plan = gpulib.Plan(golden(name), 2)
        bps = 2 if bits > 8 else 1
        for layout in ("i420", "nv12"):
            row_c = ((w + 1) // 2) * bps * (2 if layout == "nv12" else 1)
            for py, pc in ((0, 0), (w * bps + 5, 0), (0, row_c + 3), (w * bps + 6, row_c + 2)):
                assert plan.yuv420_bytes(layout, py, pc) == frame_size(w, h, bits, layout, py, pc), (name, layout, py, pc)
            if w > 1:                                                 # a pitch smaller than the row (0 would be "tight")
                assert plan.yuv420_bytes(layout, w * bps - 1, 0) == 0 and plan.yuv420_bytes(layout, 0, row_c - 1) == 0
        assert plan.yuv420_bytes("i420") == (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * bps
        assert plan.yuv420_bytes(2) == 0                              # no such layout
    # a clip: the strip (one frame of three times the height) or its frames back to back; nothing else
    clip = gpulib.Plan(golden("yuv/yuv8_96x60x3_M0.fuif"), 2)
    assert clip.info.nb_frames == 3 and clip.info.h == 180
    for layout in ("i420", "nv12"):
        assert clip.yuv420_bytes(layout, nb_frames=1) == frame_size(96, 180, 8, layout, 0, 0)
        assert clip.yuv420_bytes(layout, 100, 0, nb_frames=3) == 3 * frame_size(96, 60, 8, layout, 100, 0)
        assert clip.yuv420_bytes(layout, nb_frames=2) == 0 and clip.yuv420_bytes(layout, nb_frames=0) == 0
    assert gpulib.Plan(golden("yuv/yuv8_97x61.fuif"), 2).yuv420_bytes(nb_frames=3) == 0
    # not eligible: another keep, or a keep-2 plan of another shape
    for name in STREAMS:
        nt = gpulib.Plan(golden(name)).info.nb_transforms
        for keep in range(nt + 1):
            if keep != 2 or not (name.startswith("yuv/") or name.startswith("jpeg420")):
                assert gpulib.Plan(golden(name), keep).yuv420_bytes() == 0, (name, keep)
    for name in ("jpeg422_200x104_q88.fuif", "jpeg411_176x72_q85.fuif", "jpeg444_136x120_q85.fuif"):
        assert gpulib.Plan(golden(name), 2).yuv420_bytes() == 0, name
    assert gpulib.lib().fuifgpu_plan_yuv420_bytes(None, None) == 0
    tight = gpulib.Plan(golden("yuv/yuv8_5x4.fuif"), 2)
    assert gpulib.lib().fuifgpu_plan_yuv420_bytes(tight._h, None) == 5 * 4 + 2 * 3 * 2       # NULL options: tight I420, one frame


def test_header_declares_the_entry_points(gpulib):
    hdr = open(os.path.join(ROOT, "include", "fuifgpu.h")).read()
    declared = set(re.findall(r"\b(fuifgpu_[a-z0-9_]+)\s*\(", hdr))
    L = gpulib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and s in gpulib.ABI_SYMBOLS and hasattr(L, s), s
    assert L.fuifgpu_abi_version() == 3
    assert re.search(r"#define\s+FUIFGPU_ABI_VERSION\s+3\b", hdr)


def test_batch_entry_points_without_a_batch(gpulib):
    L = gpulib.lib()
    yuv = gpulib.make_yuv_options("i420")
    assert L.fuifgpu_batch_pack_yuv420(None, 0, 1, C.byref(yuv), None, 0, None) == E_ARG
    assert L.fuifgpu_batch_download_yuv420(None, 0, C.byref(yuv), None, None) == E_ARG
    assert L.fuifgpu_pack_yuv420(None, None, None, -1, 4, 8, None, None, None) == E_ARG


def test_gpu_yuv_decode_passes_on_the_wavefront_emulator():
    """tests/test_gpu_yuv_decode.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_pack_yuv420's lane mapping, its row ends, its interleaving and its clamp, the kept-transform schedules through every inverse kernel,
    and the batch, sibling and streaming forms of the frame output, checked without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_yuv_decode.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
