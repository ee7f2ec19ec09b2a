"""The cases and routes of tests/golden/writer_routes.json: every way a picture can go through the stream writer (csrc/writer.cpp), each on
the smallest picture at which that path exists.  tests/golden/make_writer_routes.py records digests and traffic with this module,
tests/test_gpu_writer_routes.py and tests/test_writer_routes_cpu.py compare against the record.

A case yields routes: (name, streams, device) -- `streams` the byte strings the route wrote, `device` whether it can move planes (its
encode_plane_traffic() and encode_learn_traffic() tuples are part of the record).  The routes of a case without a suffix write the streams
of the case's pictures in order (a route of one picture: the first); routes ending in "_index" write the same streams with the index trailer."""
import hashlib

import numpy as np

from fuif_amd.synth import filmstrip, graphic, photographic, yuv420_frame, yuv420_planes

SPLIT_BITS = 16      # what tests/conftest.py sets for the whole suite: bushy trees on small pictures


class DevBuffer:
    """bytes in device memory through the library's own allocator (host memory under the emulator)"""

    def __init__(self, gpulib, arr):
        self.L = gpulib.lib()
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        self.ptr = self.L.fuifgpu_dev_alloc(max(a.size, 16))
        assert self.ptr
        assert self.L.fuifgpu_dev_upload(self.ptr, a.ctypes.data, a.size) == 0

    def free(self):
        self.L.fuifgpu_dev_free(self.ptr)


def on_device(gpulib, arrays, call):
    devs = [DevBuffer(gpulib, a) for a in arrays]
    try:
        return call([d.ptr for d in devs])
    finally:
        for d in devs:
            d.free()


def _noise(w, h, c, bits, seed):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=(c, h, w)).astype(np.int32)


def _flat(w, h, c, value):
    return np.full((c, h, w), value, np.int32)


def _const_chroma(w, h, seed):
    """an 8-bit I420 frame whose chroma planes are flat: the last channels of its stream are trivial"""
    luma = yuv420_planes(w, h, 8, seed)[0]
    return luma.astype(np.uint8).tobytes() + bytes([128]) * (2 * ((w + 1) // 2) * ((h + 1) // 2))


# name -> (kind, pictures, keywords, what the batch routes do besides)
def cases():
    photo = [photographic(130, 100, 3, 8, seed=4100 + k) for k in range(3)]
    sparse14 = [(photographic(48, 40, 3, 14, seed=4400 + k) // 64 * 64).astype(np.int32) for k in range(3)]
    seven = [graphic(64, 48, 3, 8, seed=4300 + k, colors=7) for k in range(3)]
    clips = [filmstrip(96, 60, frames=3, seed=4500 + k) for k in range(2)]
    nv12_pitch = (33 + 5, 2 * 17 + 5)
    out = {
        "learned_tm1": ("image", photo, dict(bit_depth=8, tree_mode=1), dict(tm2=True)),
        "fixed_tm0": ("image", photo, dict(bit_depth=8, tree_mode=0), {}),
        "rollback_noise14": ("image", [_noise(40, 36, 4, 14, 4200 + k) for k in range(3)], dict(bit_depth=14), {}),
        "flat_16x8": ("image", [_flat(16, 8, 3, 77 + k) for k in range(3)], dict(bit_depth=8), {}),
        "one_pixel": ("image", [_flat(1, 1, 1, 200 + k) for k in range(3)], dict(bit_depth=8), {}),
        "lossy_q50": ("image", photo, dict(bit_depth=8, tree_mode=1, quality=50), dict(tm2=True)),
        "palette_seven": ("image", seven, dict(bit_depth=8, palette_colors=16), {}),
        "palette_compact_post": ("image", seven, dict(bit_depth=8, compact_post=70.0), {}),
        "palette_compact_pre14": ("image", sparse14, dict(bit_depth=14, compact_pre=70.0), {}),
        "animation_match": ("animation", clips, dict(bit_depth=8, match_previous=True), {}),
        "animation_nomatch": ("animation", clips, dict(bit_depth=8, match_previous=False), {}),
        "yuv10_75x49": ("yuv", [yuv420_frame(75, 49, 10, 38 + k) for k in range(2)], dict(w=75, h=49, bit_depth=10, tree_mode=0), {}),
        "yuv10_75x49_q60": ("yuv", [yuv420_frame(75, 49, 10, 38 + k) for k in range(2)], dict(w=75, h=49, bit_depth=10, tree_mode=0, quality=60), {}),
        "yuv8_nv12_pitched": ("yuv", [yuv420_frame(33, 21, 8, 4600 + k, layout="nv12", pitch=nv12_pitch) for k in range(2)],
                              dict(w=33, h=21, bit_depth=8, layout="nv12", pitch_y=nv12_pitch[0], pitch_c=nv12_pitch[1]), dict(tm2=True)),
        "yuv8_clip2_76x48": ("yuv", [b"".join(yuv420_frame(76, 48, 8, 4700 + 2 * k + f) for f in range(2)) for k in range(2)],
                             dict(w=76, h=48, bit_depth=8, nb_frames=2), {}),
        "yuv8_const_chroma": ("yuv", [_const_chroma(40, 28, 4800 + k) for k in range(2)], dict(w=40, h=28, bit_depth=8), {}),
        "jpeglike_64x48": ("channels", [photographic(64, 48, 3, 8, seed=4900)], dict(quality=85), {}),
    }
    return out


CASE_NAMES = ["learned_tm1", "fixed_tm0", "rollback_noise14", "flat_16x8", "one_pixel", "lossy_q50", "palette_seven", "palette_compact_post",
              "palette_compact_pre14", "animation_match", "animation_nomatch", "yuv10_75x49", "yuv10_75x49_q60", "yuv8_nv12_pitched",
              "yuv8_clip2_76x48", "yuv8_const_chroma", "jpeglike_64x48"]


def routes(gpulib, case, host_only=False):
    """generator of (route, streams, device) for one case of cases(); host_only: only the routes that need no device"""
    kind, pics, kw, extra = case
    kw = dict(kw, split_bits=SPLIT_BITS)
    if kind == "channels":
        from fuif_amd.jpeglike import encode_jpeg_like
        yield "channels_host", [encode_jpeg_like(pics[0], kw["quality"])], False
        return
    if kind == "image":
        c, h, w = pics[0].shape
        dev_kw = {k: v for k, v in kw.items() if k != "bit_depth"}
        yield "image", [gpulib.encode_image(pics[0], **kw)], False
        yield "image_index", [gpulib.encode_image(pics[0], index=True, **kw)], False
        if host_only:
            return
        yield "image_gpu_forward", [gpulib.encode_image(pics[0], gpu_forward=True, **kw)], True
        yield "image_gpu_entropy", [gpulib.encode_image(pics[0], gpu_entropy=True, **kw)], True
        yield "image_gpu_both", [gpulib.encode_image(pics[0], gpu_forward=True, gpu_entropy=True, **kw)], True
        yield "images_1", gpulib.encode_images(pics[:1], **kw), True
        yield "images_3", gpulib.encode_images(pics, **kw), True
        yield "images_device", on_device(gpulib, pics, lambda p: gpulib.encode_images_device(p, w, h, c, kw["bit_depth"], **dev_kw)), True
        yield "images_device_index", on_device(gpulib, pics, lambda p: gpulib.encode_images_device(p, w, h, c, kw["bit_depth"], index=True, **dev_kw)), True
        if extra.get("tm2"):
            kw2, dev_kw2 = dict(kw, tree_mode=2), dict(dev_kw, tree_mode=2)
            yield "images_3_tm2", gpulib.encode_images(pics, **kw2), True
            yield "images_device_tm2", on_device(gpulib, pics, lambda p: gpulib.encode_images_device(p, w, h, c, kw["bit_depth"], **dev_kw2)), True
    elif kind == "animation":
        f, c, h, w = pics[0].shape
        yield "animation", [gpulib.encode_animation(pics[0], **kw)], False
        yield "animation_index", [gpulib.encode_animation(pics[0], index=True, **kw)], False
        if host_only:
            return
        yield "animation_gpu_forward", [gpulib.encode_animation(pics[0], gpu_forward=True, **kw)], True
        yield "animation_gpu_both", [gpulib.encode_animation(pics[0], gpu_forward=True, gpu_entropy=True, **kw)], True
        yield "animations_2", gpulib.encode_animations(pics, **kw), True
        yield "animations_device", on_device(gpulib, pics, lambda p: gpulib.encode_animations_device(p, f, w, h, c, **kw)), True
    else:
        yield "yuv", [gpulib.encode_yuv420(pics[0], **kw)], False
        yield "yuv_index", [gpulib.encode_yuv420(pics[0], index=True, **kw)], False
        if host_only:
            return
        raws = [np.frombuffer(p, np.uint8) for p in pics]
        yield "yuv_gpu_forward", [gpulib.encode_yuv420(pics[0], gpu_forward=True, **kw)], True
        yield "yuv_batch_2", gpulib.encode_yuv420_batch(pics, gpu_forward=True, gpu_entropy=True, **kw), True
        yield "yuv_device", on_device(gpulib, raws, lambda p: gpulib.encode_yuv420_device(p, **kw)), True
        yield "yuv_device_index", on_device(gpulib, raws, lambda p: gpulib.encode_yuv420_device(p, index=True, **kw)), True
        if extra.get("tm2"):
            yield "yuv_device_tm2", on_device(gpulib, raws, lambda p: gpulib.encode_yuv420_device(p, **dict(kw, tree_mode=2))), True


def digest(blob):
    return {"sha256": hashlib.sha256(blob).hexdigest(), "bytes": len(blob)}


def check_case(gpulib, name, case, record, host_only=False):
    """every route of the case writes the recorded streams and moves the recorded traffic"""
    for route, streams, device in routes(gpulib, case, host_only):
        want = record["index_streams" if route.endswith("_index") else "streams"]
        assert [digest(b) for b in streams] == want[: len(streams)], (name, route)
        if device:
            moved = {"plane": list(gpulib.encode_plane_traffic()), "learn": list(gpulib.encode_learn_traffic())}
            assert moved == record["traffic"][route], (name, route, moved)
