"""fuif_amd -- MI355X (gfx950) native FUIF decode path.

Python host mirror of the reference's decode interface on top of the C-ABI library
``libfuifgpu.so`` (include/fuifgpu.h):

    reference (C++)                               here
    --------------------------------------------  ---------------------------------------------
    fuif_decode<IO>(io, image, options)           Batch.upload(blobs, preview) + Batch.decode()
      (encoding/encoding.cpp:599-720)
    Image::undo_transforms()                      Batch.undo_transforms()
      (image/image.cpp:94-115)
    Image / Channel geometry after meta_apply     Plan.coded_channels / Plan.output_channels

There is NO CPU fallback: everything that touches pixels runs in HIP kernels, and importing a
Batch without the built extension or without a GPU raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("FUIF_AMD_LIB") or os.path.join(_HERE, "libfuifgpu.so")  # FUIF_AMD_LIB: diagnostic (-DFUIF_PROF) build
_SOURCES = ["plan.cpp", "index.cpp", "writer.cpp", "maniac_decode.hip", "maniac_encode.hip", "transforms.hip", "capi.hip"]
_lib = None


class FuifGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fuifgpu error %d: %s" % (code, msg))
        self.code = code


# -ffp-contract=off: the FP64 paths (iDCT, YCbCr) must round every product and every sum on their own like the reference's
# x86-64 build; hipcc's default fuses them into v_fma_f64 in the BACKEND, which no source pragma switches off
# (tests/test_abi_and_plan.py::test_fp64_kernels_are_not_contracted looks at the ISA)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value"]


def build(force=False, verbose=False):
    """Compile libfuifgpu.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", s) for s in _SOURCES]
    deps = srcs + [os.path.join(_HERE, "csrc", h) for h in ("fuifgpu_internal.h", "maniac_decode.h", "maniac_encode.h", "tree_learn.h", "transforms.h", "squeeze_arith.h")]
    deps.append(os.path.join(_HERE, "..", "include", "fuifgpu.h"))
    if os.environ.get("FUIF_AMD_LIB"):
        return _LIB_PATH
    if not force and os.path.exists(_LIB_PATH) and all(os.path.getmtime(_LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return _LIB_PATH
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fPIC", "-shared", "-o", _LIB_PATH] + srcs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return _LIB_PATH


def build_unit_test(force=False):
    """tests/_bin/test_fast_symbol: the hand-written symbol decoder (inline GCN asm, what ships) against fast_symbol, its C++
    specification (what the wavefront emulator of the CPU suite runs), on the MI355X -- tools/test_fast_symbol.hip includes the
    kernel source itself.  Built here (hipcc cross-compiles) so that the binary travels to the GPU box; tests/test_gpu_fast_symbol.py
    builds it there when it is missing or older than the kernel."""
    root = os.path.dirname(_HERE)
    src = os.path.join(root, "tools", "test_fast_symbol.hip")
    out = os.path.join(root, "tests", "_bin", "test_fast_symbol")
    deps = [src] + [os.path.join(_HERE, "csrc", f) for f in ("maniac_decode.hip", "maniac_decode.h", "fuifgpu_internal.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc"] + HIPCC_FLAGS + ["-I", os.path.join(_HERE, "csrc"), src, "-o", out])
    return out


class ImageInfo(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("bit_depth", C.c_int32), ("maxval", C.c_int32),
                ("nb_channels", C.c_int32), ("colormodel", C.c_int32), ("max_properties", C.c_int32),
                ("nb_frames", C.c_int32), ("nb_transforms", C.c_int32), ("nb_coded_channels", C.c_int32),
                ("nb_output_channels", C.c_int32), ("nb_ops", C.c_int32), ("responsive_offsets", C.c_int32 * 5),
                ("data_start", C.c_int32), ("coef_elems", C.c_int64), ("out_elems", C.c_int64),
                ("tmp_elems", C.c_int64), ("signature", C.c_uint64)]


class ChannelDesc(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("hshift", C.c_int32), ("vshift", C.c_int32),
                ("hcshift", C.c_int32), ("vcshift", C.c_int32), ("component", C.c_int32), ("reserved", C.c_int32),
                ("offset", C.c_int64)]


class EncodeOptions(C.Structure):
    """fuifgpu_encode_options (include/fuifgpu.h): versioned by its first field; make_encode_options() fills it in"""
    _fields_ = [("struct_size", C.c_uint32), ("ycocg", C.c_int32), ("squeeze", C.c_int32), ("max_properties", C.c_int32), ("tree_mode", C.c_int32),
                ("max_tree_nodes", C.c_int32), ("emit_index", C.c_int32), ("split_bits", C.c_int32), ("gpu_forward", C.c_int32), ("gpu_entropy", C.c_int32)]


class LossyOptions(C.Structure):
    """fuifgpu_lossy_options (include/fuifgpu.h): what `fuif -Q quality[,chroma_quality]` sets; versioned by its first field"""
    _fields_ = [("struct_size", C.c_uint32), ("quality", C.c_float), ("chroma_quality", C.c_float)]


class PaletteOptions(C.Structure):
    """fuifgpu_palette_options (include/fuifgpu.h): what `fuif -K colours -X percent -Y percent` sets; versioned by its first field"""
    _fields_ = [("struct_size", C.c_uint32), ("palette_colors", C.c_int32), ("compact_post_percent", C.c_float), ("compact_pre_percent", C.c_float)]


def make_palette_options(palette_colors=0, compact_post=0.0, compact_pre=0.0):
    """PaletteOptions for the three keywords of encode_image / encode_images / encode_images_device, or None when all three are off
    (the callers then use the entry points that have no palette argument)"""
    if not palette_colors and not compact_post and not compact_pre:
        return None
    return PaletteOptions(C.sizeof(PaletteOptions), int(palette_colors), float(compact_post), float(compact_pre))


class AnimationOptions(C.Structure):
    """fuifgpu_animation_options (include/fuifgpu.h): the frames of `fuif frame-%02d.ppm`, `-F framerate` and `-M -1` / `-M 0`"""
    _fields_ = [("struct_size", C.c_uint32), ("nb_frames", C.c_int32), ("framerate", C.c_int32), ("match_previous", C.c_int32)]


def make_animation_options(nb_frames, framerate=None, match_previous=True):
    """AnimationOptions for the keywords of encode_animation / encode_animations / encode_animations_device.  match_previous: True / False
    (or 1 / 0); any other number goes to the library as it is, which refuses it (deeper distances are not offered)"""
    if framerate is None:
        framerate = 0
    elif not np.isfinite(framerate) or framerate < 0 or framerate != int(framerate):
        raise FuifGpuError(4, "encode_animation: the frame rate is a whole number of frames per second, 1 or more (None = the CLI's 10)")
    return AnimationOptions(C.sizeof(AnimationOptions), int(nb_frames), int(framerate), int(match_previous))


class YuvOptions(C.Structure):
    """fuifgpu_yuv_options (include/fuifgpu.h): how the raw 4:2:0 frames of `fuif -y WxH[:b]` lie in memory, how many, and `-F framerate`"""
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_int32), ("pitch_y", C.c_int32), ("pitch_c", C.c_int32), ("nb_frames", C.c_int32),
                ("framerate", C.c_int32)]


YUV_LAYOUTS = {"i420": 0, "nv12": 1}


def make_yuv_options(layout="i420", pitch_y=0, pitch_c=0, nb_frames=1, framerate=None):
    """YuvOptions for the keywords of encode_yuv420 and its siblings.  layout: "i420" / "nv12", or the header's number (which the
    library checks)"""
    if framerate is None:
        framerate = 0
    elif not np.isfinite(framerate) or framerate < 0 or framerate != int(framerate):
        raise FuifGpuError(4, "encode_yuv420_clip: the frame rate is a whole number of frames per second, 1 or more (None = the CLI's 10)")
    code = YUV_LAYOUTS.get(layout.lower(), -1) if isinstance(layout, str) else int(layout)
    return YuvOptions(C.sizeof(YuvOptions), code, int(pitch_y), int(pitch_c), int(nb_frames), int(framerate))


def make_lossy_options(quality=None, chroma_quality=None):
    """LossyOptions for the two keywords of encode_image / encode_images: a missing quality is 100 (lossless luma), a missing
    chroma quality "same as quality" (the CLI's default, 101)"""
    return LossyOptions(C.sizeof(LossyOptions), 100.0 if quality is None else float(quality), 101.0 if chroma_quality is None else float(chroma_quality))


class LearnOptions(C.Structure):
    """fuifgpu_learn_options (include/fuifgpu.h): the tree learner's limits, for learn_tree"""
    _fields_ = [("struct_size", C.c_uint32), ("max_nodes", C.c_int32), ("max_depth", C.c_int32), ("min_leaf", C.c_int32), ("split_bits", C.c_int32),
                ("scale", C.c_double)]


def make_encode_options(*fields):
    """EncodeOptions with struct_size set, the fields behind it in header order"""
    return EncodeOptions(C.sizeof(EncodeOptions), *fields)


# every symbol include/fuifgpu.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = [
    "fuifgpu_strerror", "fuifgpu_last_error", "fuifgpu_abi_version", "fuifgpu_plan_create", "fuifgpu_plan_destroy",
    "fuifgpu_plan_info", "fuifgpu_plan_coded_channel", "fuifgpu_plan_output_channel", "fuifgpu_plan_transform",
    "fuifgpu_build_chance_table", "fuifgpu_batch_create", "fuifgpu_batch_create_sibling", "fuifgpu_dev_mem_info", "fuifgpu_encode_images", "fuifgpu_batch_destroy", "fuifgpu_batch_upload",
    "fuifgpu_batch_decode", "fuifgpu_batch_undo_transforms", "fuifgpu_batch_sync", "fuifgpu_batch_status",
    "fuifgpu_batch_create_streaming", "fuifgpu_batch_undo_transforms_to", "fuifgpu_batch_channel_meta", "fuifgpu_batch_coef_ptr", "fuifgpu_batch_out_ptr", "fuifgpu_batch_download_coef",
    "fuifgpu_batch_download_out", "fuifgpu_batch_last_timing", "fuifgpu_batch_profile", "fuifgpu_batch_tile_log", "fuifgpu_batch_sched_stats", "fuifgpu_inv_hsqueeze", "fuifgpu_inv_vsqueeze",
    "fuifgpu_inv_ycocg", "fuifgpu_inv_ycbcr", "fuifgpu_inv_quantize", "fuifgpu_idct8x8", "fuifgpu_upsample", "fuifgpu_inv_palette", "fuifgpu_inv_approximate", "fuifgpu_inv_match", "fuifgpu_fwd_ycocg", "fuifgpu_fwd_hsqueeze", "fuifgpu_fwd_vsqueeze", "fuifgpu_fwd_quantize", "fuifgpu_encode_image", "fuifgpu_encode_channels", "fuifgpu_free_blob",
    "fuifgpu_index_parse", "fuifgpu_index_append", "fuifgpu_batch_group_index", "fuifgpu_batch_set_group_parallel",
    "fuifgpu_plan_packed_bytes", "fuifgpu_batch_pack_out", "fuifgpu_batch_download_packed",
    "fuifgpu_dev_alloc", "fuifgpu_dev_free", "fuifgpu_dev_upload", "fuifgpu_dev_download",
    "fuifgpu_encode_image_lossy", "fuifgpu_encode_images_lossy", "fuifgpu_quantization_constant",
    "fuifgpu_encode_images_device", "fuifgpu_channel_stats", "fuifgpu_encode_plane_traffic",
    "fuifgpu_encode_image_ex", "fuifgpu_encode_images_ex", "fuifgpu_fwd_palette",
    "fuifgpu_encode_animation", "fuifgpu_encode_animations", "fuifgpu_fwd_match_frames",
    "fuifgpu_encode_yuv420", "fuifgpu_unpack_yuv420", "fuifgpu_quantization_constant_yuv",
    "fuifgpu_plan_create_keep", "fuifgpu_plan_keep", "fuifgpu_plan_yuv420_bytes", "fuifgpu_batch_pack_yuv420", "fuifgpu_batch_download_yuv420", "fuifgpu_pack_yuv420",
    "fuifgpu_learn_tree", "fuifgpu_encode_learn_traffic",
    "fuifgpu_plane_checksums", "fuifgpu_device_count", "fuifgpu_set_device", "fuifgpu_get_device", "fuifgpu_batch_device", "fuifgpu_peer_copy", "fuifgpu_batch_set_in_flight",
]


def _preload_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm ships its own libamdhip64 with the SONAME of
    /opt/rocm's; whichever is loaded first serves both, and with /opt/rocm's first torch's other bundled
    libraries no longer match it (device discovery then fails in this library).  So when torch is
    installed its copy is loaded first -- without importing torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            global _hip_runtime
            _hip_runtime = C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


_hip_runtime = None


def hip_runtime():
    """the HIP runtime this process uses (ctypes handle), for hosts that need a stream or an event of their own without importing torch"""
    lib()
    return _hip_runtime if _hip_runtime is not None else C.CDLL("libamdhip64.so")


def lib():
    """Load libfuifgpu.so; raises if the HIP extension was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError("fuif_amd/libfuifgpu.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _preload_hip_runtime()
    L = C.CDLL(_LIB_PATH)
    vp, i32p, u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.fuifgpu_strerror.restype = C.c_char_p; L.fuifgpu_strerror.argtypes = [C.c_int]
    L.fuifgpu_last_error.restype = C.c_char_p; L.fuifgpu_last_error.argtypes = []
    L.fuifgpu_abi_version.restype = C.c_int
    L.fuifgpu_plan_create.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    L.fuifgpu_plan_destroy.argtypes = [vp]; L.fuifgpu_plan_destroy.restype = None
    L.fuifgpu_plan_info.argtypes = [vp, C.POINTER(ImageInfo)]
    L.fuifgpu_plan_coded_channel.argtypes = [vp, C.c_int, C.POINTER(ChannelDesc)]
    L.fuifgpu_plan_output_channel.argtypes = [vp, C.c_int, C.POINTER(ChannelDesc)]
    L.fuifgpu_plan_transform.argtypes = [vp, C.c_int, i32p, vp, C.c_int, i32p]
    L.fuifgpu_build_chance_table.argtypes = [vp, C.c_uint32, C.c_int]; L.fuifgpu_build_chance_table.restype = None
    L.fuifgpu_batch_create.argtypes = [vp, C.c_int, C.c_size_t, vp, vp, C.c_int, C.POINTER(vp)]
    L.fuifgpu_batch_create_sibling.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.fuifgpu_batch_destroy.argtypes = [vp]; L.fuifgpu_batch_destroy.restype = None
    L.fuifgpu_batch_upload.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, vp]
    L.fuifgpu_batch_decode.argtypes = [vp, vp]
    L.fuifgpu_batch_undo_transforms.argtypes = [vp, vp]
    L.fuifgpu_batch_create_streaming.argtypes = [vp, C.c_int, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.fuifgpu_batch_undo_transforms_to.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.fuifgpu_batch_sync.argtypes = [vp, vp]
    L.fuifgpu_batch_status.argtypes = [vp, vp, vp]
    L.fuifgpu_batch_channel_meta.argtypes = [vp, C.c_int, vp]
    L.fuifgpu_batch_coef_ptr.argtypes = [vp, C.c_int]; L.fuifgpu_batch_coef_ptr.restype = vp
    L.fuifgpu_batch_out_ptr.argtypes = [vp, C.c_int]; L.fuifgpu_batch_out_ptr.restype = vp
    L.fuifgpu_batch_download_coef.argtypes = [vp, C.c_int, vp, vp]
    L.fuifgpu_batch_download_out.argtypes = [vp, C.c_int, vp, vp]
    L.fuifgpu_device_count.argtypes = [C.POINTER(C.c_int)]
    L.fuifgpu_set_device.argtypes = [C.c_int]
    L.fuifgpu_get_device.argtypes = [C.POINTER(C.c_int)]
    L.fuifgpu_batch_device.argtypes = [vp, C.POINTER(C.c_int)]
    L.fuifgpu_peer_copy.argtypes = [vp, C.c_int, vp, C.c_int, C.c_size_t, vp]
    L.fuifgpu_plane_checksums.argtypes = [vp, C.c_int64, C.c_int64, C.c_int, vp, vp]
    L.fuifgpu_batch_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.fuifgpu_batch_profile.argtypes = [vp, vp]
    L.fuifgpu_batch_tile_log.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.fuifgpu_batch_sched_stats.argtypes = [vp, vp]
    L.fuifgpu_inv_hsqueeze.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, vp]
    L.fuifgpu_inv_vsqueeze.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, vp]
    L.fuifgpu_inv_ycocg.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.fuifgpu_inv_ycbcr.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.fuifgpu_inv_quantize.argtypes = [vp, C.c_int64, C.c_int, vp]
    L.fuifgpu_idct8x8.argtypes = [C.POINTER(vp), C.c_int, C.c_int, vp, C.c_int, vp]
    L.fuifgpu_upsample.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.fuifgpu_inv_palette.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    L.fuifgpu_inv_approximate.argtypes = [vp, vp, C.c_int64, C.c_int, vp]
    L.fuifgpu_inv_match.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.fuifgpu_fwd_ycocg.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    L.fuifgpu_fwd_hsqueeze.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.fuifgpu_fwd_vsqueeze.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.fuifgpu_dev_alloc.argtypes = [C.c_size_t]; L.fuifgpu_dev_alloc.restype = vp
    L.fuifgpu_dev_free.argtypes = [vp]; L.fuifgpu_dev_free.restype = None
    L.fuifgpu_dev_upload.argtypes = [vp, vp, C.c_size_t]
    L.fuifgpu_dev_download.argtypes = [vp, vp, C.c_size_t]
    L.fuifgpu_fwd_quantize.argtypes = [vp, C.c_int64, C.c_int, vp, vp]
    L.fuifgpu_encode_image_lossy.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_encode_images_lossy.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_encode_images_device.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_channel_stats.argtypes = [vp, C.c_int64, vp, vp]
    L.fuifgpu_encode_image_ex.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(PaletteOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_encode_images_ex.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(PaletteOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_fwd_palette.argtypes = [C.POINTER(vp), C.c_int, C.c_int64, C.c_int, vp, vp, C.POINTER(C.c_int), vp]
    L.fuifgpu_encode_animation.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(PaletteOptions), C.POINTER(AnimationOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_encode_animations.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(PaletteOptions), C.POINTER(AnimationOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_fwd_match_frames.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.fuifgpu_encode_yuv420.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(YuvOptions), C.POINTER(EncodeOptions), C.POINTER(LossyOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_unpack_yuv420.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(YuvOptions), vp, vp, vp, vp, vp]
    L.fuifgpu_quantization_constant_yuv.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    L.fuifgpu_plan_create_keep.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.fuifgpu_plan_keep.argtypes = [vp, C.POINTER(C.c_int)]
    L.fuifgpu_plan_yuv420_bytes.argtypes = [vp, C.POINTER(YuvOptions)]; L.fuifgpu_plan_yuv420_bytes.restype = C.c_size_t
    L.fuifgpu_batch_pack_yuv420.argtypes = [vp, C.c_int, C.c_int, C.POINTER(YuvOptions), vp, C.c_int64, vp]
    L.fuifgpu_batch_download_yuv420.argtypes = [vp, C.c_int, C.POINTER(YuvOptions), vp, vp]
    L.fuifgpu_pack_yuv420.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(YuvOptions), vp, vp]
    L.fuifgpu_encode_plane_traffic.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fuifgpu_encode_learn_traffic.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fuifgpu_learn_tree.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(LearnOptions), C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    L.fuifgpu_quantization_constant.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    L.fuifgpu_encode_image.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_encode_images.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EncodeOptions), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_free_blob.argtypes = [vp]; L.fuifgpu_free_blob.restype = None
    L.fuifgpu_index_parse.argtypes = [C.c_char_p, C.c_size_t, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.fuifgpu_index_append.argtypes = [C.c_char_p, C.c_size_t, vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fuifgpu_batch_group_index.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.fuifgpu_batch_set_group_parallel.argtypes = [vp, C.c_int]
    L.fuifgpu_batch_set_in_flight.argtypes = [vp, C.c_int]
    L.fuifgpu_plan_packed_bytes.argtypes = [vp, C.c_int]; L.fuifgpu_plan_packed_bytes.restype = C.c_size_t
    L.fuifgpu_batch_pack_out.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.fuifgpu_batch_download_packed.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    _lib = L
    return L


def _check(code):
    if code != 0:
        L = lib()
        msg = L.fuifgpu_strerror(code).decode()
        last = L.fuifgpu_last_error().decode()
        raise FuifGpuError(code, msg + (" (" + last + ")" if last else ""))


class Plan:
    """Parsed header + channel table + inverse schedule of one stream (host only).  keep: transforms the schedule leaves standing
    (fuifgpu_plan_create_keep, Image::undo_transforms(keep)); 2 on a `fuif -y` stream leaves Y, Cb, Cr as they were coded."""

    def __init__(self, blob, keep=0):
        L = lib()
        self._h = C.c_void_p()
        head = bytes(blob[:65536]) if len(blob) > 65536 else bytes(blob)
        if keep:
            _check(L.fuifgpu_plan_create_keep(head, len(head), int(keep), C.byref(self._h)))
        else:
            _check(L.fuifgpu_plan_create(head, len(head), C.byref(self._h)))
        self.info = ImageInfo()
        _check(L.fuifgpu_plan_info(self._h, C.byref(self.info)))

    @property
    def keep(self):
        k = C.c_int(0)
        _check(lib().fuifgpu_plan_keep(self._h, C.byref(k)))
        return k.value

    def yuv420_bytes(self, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1):
        """bytes of one image's raw 4:2:0 frame(s) in that layout (fuifgpu_plan_yuv420_bytes); 0: this plan cannot be written as such"""
        yuv = make_yuv_options(layout, pitch_y, pitch_c, nb_frames)
        return int(lib().fuifgpu_plan_yuv420_bytes(self._h, C.byref(yuv)))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.fuifgpu_plan_destroy(self._h)
            self._h = None

    def _channels(self, fn, n):
        out = []
        for i in range(n):
            d = ChannelDesc()
            _check(fn(self._h, i, C.byref(d)))
            out.append({k: int(getattr(d, k)) for k, _ in ChannelDesc._fields_ if k != "reserved"})
        return out

    @property
    def coded_channels(self):
        return self._channels(lib().fuifgpu_plan_coded_channel, self.info.nb_coded_channels)

    @property
    def output_channels(self):
        return self._channels(lib().fuifgpu_plan_output_channel, self.info.nb_output_channels)

    @property
    def transforms(self):
        out = []
        for i in range(self.info.nb_transforms):
            tid, n = C.c_int32(), C.c_int32()
            buf = np.zeros(1024, np.int32)
            _check(lib().fuifgpu_plan_transform(self._h, i, C.byref(tid), buf.ctypes.data, 1024, C.byref(n)))
            out.append((int(tid.value), [int(v) for v in buf[: n.value]]))
        return out


class Batch:
    """Device state for ``n_images`` streams sharing one plan (geometry + transform chain)."""

    def __init__(self, plan, n_images, blob_capacity, coef_ptr=None, out_ptr=None, tmp_images=0, streaming=False):
        L = lib()
        self.plan = plan
        self.n = n_images
        self._h = C.c_void_p()
        if streaming:
            # no output slab: the inverse transforms run range by range into caller memory (undo_transforms_to)
            _check(L.fuifgpu_batch_create_streaming(plan._h, n_images, blob_capacity, tmp_images, C.byref(self._h)))
        else:
            _check(L.fuifgpu_batch_create(plan._h, n_images, blob_capacity, coef_ptr, out_ptr, tmp_images, C.byref(self._h)))
        self._keep = None

    def undo_transforms_to(self, first_image, n_images, out_device_ptr, stream=None):
        """inverse transforms of images [first, first + n) of the current decode into DEVICE memory (n * out_elems int32)"""
        _check(lib().fuifgpu_batch_undo_transforms_to(self._h, first_image, n_images, out_device_ptr, stream))

    def sibling(self, blob_capacity):
        """a second set of stream buffers over this Batch's slabs, scratch and arenas (fuifgpu_batch_create_sibling): upload
        into one while the other decodes.  Creating a sibling freezes the launch resources the two share (ABI 2), so either may be
        loaded first; close the sibling before the primary."""
        other = Batch.__new__(Batch)
        other.plan, other.n, other._keep = self.plan, self.n, None
        other._h = C.c_void_p()
        other._primary = self          # keeps the primary alive as long as the sibling
        _check(lib().fuifgpu_batch_create_sibling(self._h, blob_capacity, C.byref(other._h)))
        return other

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.fuifgpu_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def upload(self, blobs, preview=-1, stream=None):
        n = len(blobs)
        arr = (C.c_char_p * n)(*[C.c_char_p(b) for b in blobs])
        sizes = (C.c_size_t * n)(*[len(b) for b in blobs])
        self._keep = (blobs, arr, sizes)
        _check(lib().fuifgpu_batch_upload(self._h, arr, sizes, n, preview, stream))
        self.n_loaded = n

    def decode(self, stream=None):
        _check(lib().fuifgpu_batch_decode(self._h, stream))

    def undo_transforms(self, stream=None):
        _check(lib().fuifgpu_batch_undo_transforms(self._h, stream))

    def sync(self, stream=None):
        _check(lib().fuifgpu_batch_sync(self._h, stream))

    def status(self):
        st = np.zeros(self.n_loaded, np.int32)
        used = np.zeros(self.n_loaded, np.uint32)
        _check(lib().fuifgpu_batch_status(self._h, st.ctypes.data, used.ctypes.data))
        return st, used

    @property
    def device(self):
        d = C.c_int(0)
        _check(lib().fuifgpu_batch_device(self._h, C.byref(d)))
        return d.value

    def set_group_parallel(self, enable):
        """False: ignore group indices (one wavefront per image, as for streams that carry none); applies to the next upload"""
        _check(lib().fuifgpu_batch_set_group_parallel(self._h, int(bool(enable))))

    def set_in_flight(self, n_batches):
        """how many batches the host keeps in flight on this device (fuifgpu_batch_set_in_flight); applies to the next upload"""
        _check(lib().fuifgpu_batch_set_in_flight(self._h, int(n_batches)))

    def group_index(self, image):
        """[(first_channel, byte_offset)] of every channel group the last decode of `image` went through"""
        nch = self.plan.info.nb_coded_channels
        fc, st, n = np.zeros(max(nch, 1), np.int32), np.zeros(max(nch, 1), np.uint32), C.c_int(0)
        _check(lib().fuifgpu_batch_group_index(self._h, image, fc.ctypes.data, st.ctypes.data, nch, C.byref(n)))
        return [(int(fc[i]), int(st[i])) for i in range(n.value)]

    def channel_meta(self, image):
        m = np.zeros((self.plan.info.nb_coded_channels, 4), np.int32)
        _check(lib().fuifgpu_batch_channel_meta(self._h, image, m.ctypes.data))
        return m

    def coef_ptr(self, image=0):
        return lib().fuifgpu_batch_coef_ptr(self._h, image)

    def out_ptr(self, image=0):
        return lib().fuifgpu_batch_out_ptr(self._h, image)

    def timing(self):
        a, b = C.c_float(), C.c_float()
        _check(lib().fuifgpu_batch_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def profile(self):
        """(n_loaded, 8) uint64 phase cycle counters of the last decode (diagnostic builds only)"""
        out = np.zeros((self.n_loaded, 8), np.uint64)
        _check(lib().fuifgpu_batch_profile(self._h, out.ctypes.data))
        return out

    def tile_log(self):
        """(n_tiles, 4) uint64 schedule of the last decode launch (see fuifgpu_batch_tile_log); the first call arms logging"""
        n = C.c_int(0)
        _check(lib().fuifgpu_batch_tile_log(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.uint64)
        if n.value:
            _check(lib().fuifgpu_batch_tile_log(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def sched_stats(self):
        out = np.zeros(8, np.uint64)
        _check(lib().fuifgpu_batch_sched_stats(self._h, out.ctypes.data))
        return out

    def coef_planes(self, image):
        """coded channel planes of one image as a list of (h,w) int32 arrays (device -> host)"""
        slab = np.zeros(max(self.plan.info.coef_elems, 1), np.int32)
        _check(lib().fuifgpu_batch_download_coef(self._h, image, slab.ctypes.data, None))
        return [slab[c["offset"]: c["offset"] + c["w"] * c["h"]].reshape(c["h"], c["w"]).copy() for c in self.plan.coded_channels]

    def packed(self, image, components=0):
        """(h, w, components) uint8 / uint16 samples of one decoded image, interleaved and clamped on the GPU
        (the payload export/write_pam.h would write); call after undo_transforms()"""
        info = self.plan.info
        n = lib().fuifgpu_plan_packed_bytes(self.plan._h, components)
        if not n:
            raise FuifGpuError(4, "these output channels cannot be packed")
        buf = np.zeros(n, np.uint8)
        _check(lib().fuifgpu_batch_download_packed(self._h, image, components, buf.ctypes.data, None))
        bps = 2 if info.maxval > 255 else 1
        comps = n // (info.w * info.h * bps)
        if bps == 2:
            return buf.view(">u2").astype(np.uint16).reshape(info.h, info.w, comps)
        return buf.reshape(info.h, info.w, comps)

    def packed_bytes(self, components=0):
        return int(lib().fuifgpu_plan_packed_bytes(self.plan._h, components))

    def pack_out(self, dst_device_ptr, first_image=0, n_images=None, components=0, stream=None):
        """interleaved clamped 8 / 16-bit samples of images [first, first+n) into DEVICE memory (n * packed_bytes bytes):
        the payload of the final gather (dist.gather_packed) and of a PNM/PAM file; call after undo_transforms()"""
        n = self.n_loaded - first_image if n_images is None else n_images
        _check(lib().fuifgpu_batch_pack_out(self._h, first_image, n, components, dst_device_ptr, stream))

    def pack_yuv420(self, first_image, n_images, dst_device_ptr, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1, image_stride=0, stream=None):
        """raw YUV 4:2:0 frames of images [first, first+n) of a keep = 2 batch into DEVICE memory, image_stride bytes apart (0 = tight,
        plan.yuv420_bytes(...)), in one launch (fuifgpu_batch_pack_yuv420); call after undo_transforms().  nb_frames: 1 = the stacked strip
        of a clip, the stream's frame count = its frames back to back, the layout encode_yuv420_clip reads"""
        yuv = make_yuv_options(layout, pitch_y, pitch_c, nb_frames)
        _check(lib().fuifgpu_batch_pack_yuv420(self._h, int(first_image), int(n_images), C.byref(yuv), dst_device_ptr, int(image_stride), stream))

    def download_yuv420(self, image, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1):
        """the raw YUV 4:2:0 frame(s) of one image of a keep = 2 batch as bytes -- for tight I420 the .yuv file `fuif -d x.fuif out.yuv`
        writes (fuifgpu_batch_download_yuv420; padding bytes of pitched rows are 0); call after undo_transforms()"""
        yuv = make_yuv_options(layout, pitch_y, pitch_c, nb_frames)
        n = int(lib().fuifgpu_plan_yuv420_bytes(self.plan._h, C.byref(yuv)))
        buf = np.zeros(max(n, 1), np.uint8)
        _check(lib().fuifgpu_batch_download_yuv420(self._h, int(image), C.byref(yuv), buf.ctypes.data, None))
        return buf[:n].tobytes()

    def out_planes(self, image):
        """the output channels of one image as (h, w) int32 arrays, each with its own shape (a keep plan's channels differ in size)"""
        slab = np.zeros(max(self.plan.info.out_elems, 1), np.int32)
        _check(lib().fuifgpu_batch_download_out(self._h, image, slab.ctypes.data, None))
        return [slab[c["offset"]: c["offset"] + c["w"] * c["h"]].reshape(c["h"], c["w"]).copy() for c in self.plan.output_channels]


def device_count():
    n = C.c_int(0)
    _check(lib().fuifgpu_device_count(C.byref(n)))
    return n.value


def set_device(device):
    """the calling thread's current device (fuifgpu_set_device): batches created afterwards live there"""
    _check(lib().fuifgpu_set_device(int(device)))


def get_device():
    d = C.c_int(0)
    _check(lib().fuifgpu_get_device(C.byref(d)))
    return d.value


def plane_checksums(planes_device_ptr, elems_per_image, n_images, sums_device_ptr, stream=None, image_stride=None):
    """fuifgpu_plane_checksums: one position-weighted 64-bit sum per image of a device slab of int32 planes into DEVICE memory
    (n_images x uint64), asynchronous on `stream`"""
    _check(lib().fuifgpu_plane_checksums(planes_device_ptr, elems_per_image, elems_per_image if image_stride is None else image_stride,
                                        n_images, sums_device_ptr, stream))


def decode_batch(blobs, preview=-1, undo=True):
    """Decode same-geometry streams on the GPU; returns (list of per-image output planes, status)."""
    plan = Plan(blobs[0])
    cap = sum(len(b) for b in blobs)
    batch = Batch(plan, len(blobs), cap)
    try:
        batch.upload(blobs, preview)
        batch.decode()
        if undo:
            batch.undo_transforms()
        batch.sync()
        st, used = batch.status()
        outs = [batch.out_planes(i) if undo else batch.coef_planes(i) for i in range(len(blobs))]
        return outs, st
    finally:
        batch.close()


# learned trees: 0 = the writer's default rule (description length of the extra leaf), > 0 = flat bits a split must save.
# The test suite sets 16 (bushy trees on small pictures: coverage of the context-tree walk).
DEFAULT_SPLIT_BITS = 0


def encode_image(planes, bit_depth=8, ycocg=True, squeeze=True, max_properties=12, tree_mode=1, max_tree_nodes=4095, index=False,
                 split_bits=None, gpu_forward=False, gpu_entropy=False, quality=None, chroma_quality=None, palette_colors=0, compact_post=0.0,
                 compact_pre=0.0):
    """(C,H,W) int32 planes -> .fuif bytes (host C++ writer, csrc/writer.cpp); lossless unless a quality is given.
    palette_colors / compact_post / compact_pre: `fuif -K / -X / -Y` (the CLI's defaults are 256, 70, 70; 0 = off, the default here): the
    whole-picture Palette and the per-channel compaction the CLI tries for PNM input (fuifgpu_encode_image_ex).
    quality / chroma_quality: the two numbers of `fuif -Q` (0..100; chroma_quality None or > 100 = same as quality): the channels are
    quantised after YCoCg and Squeeze with the reference CLI's constants (fuifgpu_encode_image_lossy); 100 writes the lossless bytes.
    index=True appends the group index trailer (csrc/index.cpp) that unlocks one-wavefront-per-group decoding.
    gpu_forward=True runs the forward YCoCg and Squeeze on the GPU (fuifgpu_fwd_*), gpu_entropy=True the MANIAC pixel loop of
    every compressed group (csrc/maniac_encode.hip): same bytes either way."""
    split_bits = DEFAULT_SPLIT_BITS if split_bits is None else split_bits
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    c, h, w = planes.shape
    opt = make_encode_options(int(ycocg), int(squeeze), max_properties, tree_mode, max_tree_nodes, int(index), int(split_bits), int(gpu_forward), int(gpu_entropy))
    out = C.c_void_p()
    n = C.c_size_t(0)
    pal = make_palette_options(palette_colors, compact_post, compact_pre)
    if pal is not None:
        lossy = None if quality is None and chroma_quality is None else C.byref(make_lossy_options(quality, chroma_quality))
        _check(lib().fuifgpu_encode_image_ex(planes.ctypes.data, w, h, c, bit_depth, C.byref(opt), lossy, C.byref(pal), C.byref(out), C.byref(n)))
    elif quality is None and chroma_quality is None:
        _check(lib().fuifgpu_encode_image(planes.ctypes.data, w, h, c, bit_depth, C.byref(opt), C.byref(out), C.byref(n)))
    else:
        lossy = make_lossy_options(quality, chroma_quality)
        _check(lib().fuifgpu_encode_image_lossy(planes.ctypes.data, w, h, c, bit_depth, C.byref(opt), C.byref(lossy), C.byref(out), C.byref(n)))
    blob = C.string_at(out.value, n.value)
    lib().fuifgpu_free_blob(out)
    return blob


def encode_images(images, bit_depth=8, ycocg=True, squeeze=True, max_properties=12, tree_mode=1, max_tree_nodes=4095, index=False,
                  split_bits=None, gpu_forward=False, quality=None, chroma_quality=None, palette_colors=0, compact_post=0.0, compact_pre=0.0):
    """a batch of equally sized (C,H,W) pictures -> list of .fuif byte strings, what encode_image writes for each of them; the
    MANIAC pixel loops of ALL their channel groups run in one launch pair on the GPU (fuifgpu_encode_images; with a quality,
    fuifgpu_encode_images_lossy)"""
    split_bits = DEFAULT_SPLIT_BITS if split_bits is None else split_bits
    arrs = [np.ascontiguousarray(im, dtype=np.int32) for im in images]
    c, h, w = arrs[0].shape
    if any(a.shape != (c, h, w) for a in arrs):
        raise FuifGpuError(4, "encode_images: all pictures of a batch must have one shape")
    n = len(arrs)
    opt = make_encode_options(int(ycocg), int(squeeze), max_properties, tree_mode, max_tree_nodes, int(index), int(split_bits), int(gpu_forward), 1)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    outs = (C.c_void_p * n)()
    sizes = (C.c_size_t * n)()
    pal = make_palette_options(palette_colors, compact_post, compact_pre)
    if pal is not None:   # (pictures of one batch may end up with different transform chains)
        lossy = None if quality is None and chroma_quality is None else C.byref(make_lossy_options(quality, chroma_quality))
        _check(lib().fuifgpu_encode_images_ex(ptrs, 0, n, w, h, c, bit_depth, C.byref(opt), lossy, C.byref(pal), outs, sizes))
    elif quality is None and chroma_quality is None:
        _check(lib().fuifgpu_encode_images(ptrs, n, w, h, c, bit_depth, C.byref(opt), outs, sizes))
    else:
        lossy = make_lossy_options(quality, chroma_quality)
        _check(lib().fuifgpu_encode_images_lossy(ptrs, n, w, h, c, bit_depth, C.byref(opt), C.byref(lossy), outs, sizes))
    blobs = []
    for k in range(n):
        blobs.append(C.string_at(outs[k], sizes[k]))
        lib().fuifgpu_free_blob(C.c_void_p(outs[k]))
    return blobs


def encode_images_device(planes, w=None, h=None, nch=None, bit_depth=8, ycocg=True, squeeze=True, max_properties=12, tree_mode=1, max_tree_nodes=4095,
                         index=False, split_bits=None, quality=None, chroma_quality=None, palette_colors=0, compact_post=0.0, compact_pre=0.0):
    """pictures that already live in DEVICE memory -> list of .fuif byte strings, the bytes encode_images writes for the same samples
    (fuifgpu_encode_images_device: the planes are read, never written, and no channel crosses to the host unless its group is rolled
    back to "uncompressed").  planes: a list of integer device pointers (each nch planes of w*h int32; w, h, nch given), or an object
    with data_ptr(), shape == (N, C, H, W), an int32 dtype and contiguous layout -- e.g. a torch tensor on the current device."""
    split_bits = DEFAULT_SPLIT_BITS if split_bits is None else split_bits
    if hasattr(planes, "data_ptr"):
        shape = tuple(int(v) for v in planes.shape)
        if len(shape) != 4 or "int32" not in str(planes.dtype) or (hasattr(planes, "is_contiguous") and not planes.is_contiguous()):
            raise FuifGpuError(4, "encode_images_device: a tensor must be contiguous int32 of shape (N, C, H, W)")
        n, nch, h, w = shape
        ptrs = [planes.data_ptr() + 4 * k * nch * h * w for k in range(n)]
    else:
        ptrs = [int(p) if p else 0 for p in planes]
        if w is None or h is None or nch is None:
            raise FuifGpuError(4, "encode_images_device: w, h and nch go with a list of device pointers")
    n = len(ptrs)
    opt = make_encode_options(int(ycocg), int(squeeze), max_properties, tree_mode, max_tree_nodes, int(index), int(split_bits), 1, 1)
    lossy = None if quality is None and chroma_quality is None else C.byref(make_lossy_options(quality, chroma_quality))
    arr = (C.c_void_p * max(n, 1))(*ptrs)
    outs = (C.c_void_p * max(n, 1))()
    sizes = (C.c_size_t * max(n, 1))()
    pal = make_palette_options(palette_colors, compact_post, compact_pre)
    if pal is not None:   # (the index planes stay on the device like every other channel; the palettes are small host tables)
        _check(lib().fuifgpu_encode_images_ex(arr, 1, n, int(w), int(h), int(nch), bit_depth, C.byref(opt), lossy, C.byref(pal), outs, sizes))
    else:
        _check(lib().fuifgpu_encode_images_device(arr, n, int(w), int(h), int(nch), bit_depth, C.byref(opt), lossy, outs, sizes))
    blobs = []
    for k in range(n):
        blobs.append(C.string_at(outs[k], sizes[k]))
        lib().fuifgpu_free_blob(C.c_void_p(outs[k]))
    return blobs


def _encode_options_from_keywords(gpu_forward, gpu_entropy, bit_depth=8, ycocg=True, squeeze=True, max_properties=12, tree_mode=1, max_tree_nodes=4095,
                                  index=False, split_bits=None, quality=None, chroma_quality=None, palette_colors=0, compact_post=0.0, compact_pre=0.0):
    """the keywords encode_image has besides the two routes -> (bit_depth, EncodeOptions, LossyOptions or None, PaletteOptions or None)"""
    split_bits = DEFAULT_SPLIT_BITS if split_bits is None else split_bits
    opt = make_encode_options(int(ycocg), int(squeeze), max_properties, tree_mode, max_tree_nodes, int(index), int(split_bits), int(gpu_forward), int(gpu_entropy))
    lossy = None if quality is None and chroma_quality is None else make_lossy_options(quality, chroma_quality)
    return bit_depth, opt, lossy, make_palette_options(palette_colors, compact_post, compact_pre)


def _byref_or_none(struct):
    return None if struct is None else C.byref(struct)


def _take_blobs(outs, sizes, n):
    blobs = []
    for k in range(n):
        blobs.append(C.string_at(outs[k], sizes[k]))
        lib().fuifgpu_free_blob(C.c_void_p(outs[k]))
    return blobs


def encode_animation(frames, framerate=None, match_previous=True, gpu_forward=False, gpu_entropy=False, **keywords):
    """(F,C,H,W) int32 frames -> the bytes `fuif frame-%02d.ppm out.fuif` writes for them: one strip under the magic FUAF and, with
    match_previous (the CLI's `-M -1`; False = `-M 0`), the Matching transform against the frame above (fuifgpu_encode_animation).
    framerate: `-F` (None = 10).  The other keywords are encode_image's.  One frame writes what encode_image writes."""
    frames = np.ascontiguousarray(frames, dtype=np.int32)
    if frames.ndim != 4:
        raise FuifGpuError(4, "encode_animation: frames of shape (F, C, H, W)")
    f, c, h, w = frames.shape
    bit_depth, opt, lossy, pal = _encode_options_from_keywords(gpu_forward, gpu_entropy, **keywords)
    anim = make_animation_options(f, framerate, match_previous)
    out, n = C.c_void_p(), C.c_size_t(0)
    _check(lib().fuifgpu_encode_animation(frames.ctypes.data, w, h, c, bit_depth, C.byref(opt), _byref_or_none(lossy), _byref_or_none(pal), C.byref(anim),
                                          C.byref(out), C.byref(n)))
    blob = C.string_at(out.value, n.value)
    lib().fuifgpu_free_blob(out)
    return blob


def encode_animations(clips, framerate=None, match_previous=True, gpu_forward=False, **keywords):
    """a batch of equally shaped (F,C,H,W) clips -> list of byte strings, what encode_animation writes for each; the pixel loops of all
    their channel groups run in one launch pair (fuifgpu_encode_animations, the batch writer of encode_images)"""
    arrs = [np.ascontiguousarray(cl, dtype=np.int32) for cl in clips]
    if not arrs or arrs[0].ndim != 4 or any(a.shape != arrs[0].shape for a in arrs):
        raise FuifGpuError(4, "encode_animations: all clips of a batch have one shape (F, C, H, W)")
    f, c, h, w = arrs[0].shape
    n = len(arrs)
    bit_depth, opt, lossy, pal = _encode_options_from_keywords(gpu_forward, 1, **keywords)
    anim = make_animation_options(f, framerate, match_previous)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    outs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
    _check(lib().fuifgpu_encode_animations(ptrs, 0, n, w, h, c, bit_depth, C.byref(opt), _byref_or_none(lossy), _byref_or_none(pal), C.byref(anim), outs, sizes))
    return _take_blobs(outs, sizes, n)


def encode_animations_device(clips, nb_frames=None, w=None, h=None, nch=None, framerate=None, match_previous=True, **keywords):
    """clips that already live in DEVICE memory -> list of byte strings, the bytes encode_animations writes for the same samples.  The
    frames are read, never written; no channel and no match channel crosses to the host unless its group is rolled back to
    "uncompressed" (encode_plane_traffic).  clips: a list of integer device pointers (each nb_frames x nch planes of w*h int32, frame
    after frame; nb_frames, w, h, nch given), or an object with data_ptr(), shape == (N, F, C, H, W), an int32 dtype and contiguous layout"""
    if hasattr(clips, "data_ptr"):
        shape = tuple(int(v) for v in clips.shape)
        if len(shape) != 5 or "int32" not in str(clips.dtype) or (hasattr(clips, "is_contiguous") and not clips.is_contiguous()):
            raise FuifGpuError(4, "encode_animations_device: a tensor must be contiguous int32 of shape (N, F, C, H, W)")
        n, nb_frames, nch, h, w = shape
        ptrs = [clips.data_ptr() + 4 * k * nb_frames * nch * h * w for k in range(n)]
    else:
        ptrs = [int(p) if p else 0 for p in clips]
        if nb_frames is None or w is None or h is None or nch is None:
            raise FuifGpuError(4, "encode_animations_device: nb_frames, w, h and nch go with a list of device pointers")
    n = len(ptrs)
    bit_depth, opt, lossy, pal = _encode_options_from_keywords(1, 1, **keywords)
    anim = make_animation_options(nb_frames, framerate, match_previous)
    arr = (C.c_void_p * max(n, 1))(*ptrs)
    outs, sizes = (C.c_void_p * max(n, 1))(), (C.c_size_t * max(n, 1))()
    _check(lib().fuifgpu_encode_animations(arr, 1, n, int(w), int(h), int(nch), bit_depth, C.byref(opt), _byref_or_none(lossy), _byref_or_none(pal), C.byref(anim),
                                           outs, sizes))
    return _take_blobs(outs, sizes, n)


def fwd_match_frames(plane_device_ptrs, w, h, nb_frames, match_device_ptr, stream=None):
    """fuifgpu_fwd_match_frames: the forward Matching against the previous frame (transform/2dmatch.h:303-381, distance -1) of up to eight
    planes of a w x h strip of nb_frames frames in DEVICE memory: the match channel goes to match_device_ptr (w*h int32) and the matched
    samples of the planes become 0 IN PLACE; asynchronous on `stream`"""
    nb = len(plane_device_ptrs)
    ptrs = (C.c_void_p * max(nb, 1))(*[int(p) if p else 0 for p in plane_device_ptrs])
    _check(lib().fuifgpu_fwd_match_frames(ptrs, nb, int(w), int(h), int(nb_frames), match_device_ptr, stream))


def yuv420_bytes(w, h, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1):
    """bytes from the first sample of a raw 4:2:0 clip to its last one (the last row of the last plane carries no padding)"""
    bps = 2 if bit_depth > 8 else 1
    nv12 = make_yuv_options(layout).layout == 1
    cw, ch = (w + 1) // 2, (h + 1) // 2
    row_c = cw * bps * (2 if nv12 else 1)
    py, pc = pitch_y or w * bps, pitch_c or row_c
    frame = py * h + pc * ch * (1 if nv12 else 2)
    last_plane = py * h + (0 if nv12 else pc * ch)
    return (nb_frames - 1) * frame + last_plane + (ch - 1) * pc + row_c


def _yuv_raw(frame, need):
    """bytes, or a uint8 / 16-bit unsigned array (stored little-endian) -> contiguous uint8 array of at least `need` bytes"""
    if isinstance(frame, (bytes, bytearray, memoryview)):
        a = np.frombuffer(frame, dtype=np.uint8)
    else:
        a = np.asarray(frame)
        if a.dtype.kind != "u" or a.dtype.itemsize > 2:
            raise FuifGpuError(4, "encode_yuv420: a frame is bytes, or a uint8 / uint16 array")
        a = np.ascontiguousarray(a.astype("<u2", copy=False) if a.dtype.itemsize == 2 else a).reshape(-1).view(np.uint8)
    if a.size < need:
        raise FuifGpuError(4, "encode_yuv420: the frame holds %d bytes, its geometry needs %d" % (a.size, need))
    return a


def _yuv_keywords(gpu_forward, gpu_entropy, squeeze=True, max_properties=12, tree_mode=1, max_tree_nodes=4095, index=False, split_bits=None,
                  quality=None, chroma_quality=None):
    """encode_image's keywords minus the colour and palette ones -> (EncodeOptions, LossyOptions or None)"""
    split_bits = DEFAULT_SPLIT_BITS if split_bits is None else split_bits
    opt = make_encode_options(0, int(squeeze), max_properties, tree_mode, max_tree_nodes, int(index), int(split_bits), int(gpu_forward), int(gpu_entropy))
    return opt, (None if quality is None and chroma_quality is None else make_lossy_options(quality, chroma_quality))


def _encode_yuv420_call(ptrs, on_device, w, h, bit_depth, yuv, opt, lossy):
    n = len(ptrs)
    arr = (C.c_void_p * max(n, 1))(*ptrs)
    outs, sizes = (C.c_void_p * max(n, 1))(), (C.c_size_t * max(n, 1))()
    _check(lib().fuifgpu_encode_yuv420(arr, int(on_device), n, int(w), int(h), int(bit_depth), C.byref(yuv), C.byref(opt), _byref_or_none(lossy), outs, sizes))
    return _take_blobs(outs, sizes, n)


def encode_yuv420_batch(frames, w, h, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1, framerate=None, gpu_forward=False,
                        gpu_entropy=False, **keywords):
    """raw YUV 4:2:0 pictures (or clips of nb_frames frames back to back) of one shape -> list of .fuif byte strings, the bytes
    `fuif -y WxH[:b]` writes for each (fuifgpu_encode_yuv420).  A picture is bytes, or a uint8 / uint16 array: the Y plane, then Cb and Cr of
    ((w+1)/2) x ((h+1)/2) samples (layout "i420") or one plane of Cb, Cr pairs ("nv12"); one byte per sample at 8 bits, two little-endian
    above; pitch_y / pitch_c: bytes from row to row (0 = tight).  The other keywords are encode_image's minus the colour and palette ones.
    gpu_forward: the raw frames are uploaded and unpacked on the GPU (one launch), forward Squeeze and Quantize run there;
    with gpu_entropy a batch's pixel loops run in one launch pair.  Same bytes on every route."""
    need = yuv420_bytes(w, h, bit_depth, layout, pitch_y, pitch_c, nb_frames)
    raws = [_yuv_raw(f, need) for f in frames]
    opt, lossy = _yuv_keywords(gpu_forward, gpu_entropy, **keywords)
    yuv = make_yuv_options(layout, pitch_y, pitch_c, nb_frames, framerate)
    return _encode_yuv420_call([a.ctypes.data for a in raws], 0, w, h, bit_depth, yuv, opt, lossy)


def encode_yuv420(frame, w, h, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0, **keywords):
    """one raw YUV 4:2:0 frame -> .fuif bytes: encode_yuv420_batch of one picture"""
    return encode_yuv420_batch([frame], w, h, bit_depth, layout, pitch_y, pitch_c, **keywords)[0]


def encode_yuv420_clip(clip, w, h, nb_frames, framerate=None, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0, **keywords):
    """nb_frames raw frames back to back -> the bytes `fuif -M 0 [-F framerate] -y WxH[:b] v-%02d.yuv` writes: the frames stacked per channel
    under the magic FUAF, no Matching transform (the reference's previous-frame matcher reads outside the chroma planes).  h must be even."""
    return encode_yuv420_batch([clip], w, h, bit_depth, layout, pitch_y, pitch_c, nb_frames=nb_frames, framerate=framerate, **keywords)[0]


def encode_yuv420_device(frames, w=None, h=None, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1, framerate=None, **keywords):
    """raw frames that already live in DEVICE memory (a hardware decoder's surfaces) -> list of .fuif byte strings, the bytes
    encode_yuv420_batch writes for the same samples.  The frames are read, never written; the unpacked channels stay on the device until
    the last coded byte (encode_plane_traffic: nothing goes up).  frames: a list of integer device pointers, or an object with data_ptr(),
    a uint8 or 16-bit dtype, contiguous layout and shape (N, bytes or samples per picture) -- e.g. a torch uint8 / int16 tensor on the GPU."""
    if hasattr(frames, "data_ptr"):
        shape = tuple(int(v) for v in frames.shape)
        item = 2 if "int16" in str(frames.dtype) else 1 if "uint8" in str(frames.dtype) else 0
        if len(shape) != 2 or not item or (hasattr(frames, "is_contiguous") and not frames.is_contiguous()):
            raise FuifGpuError(4, "encode_yuv420_device: a tensor must be contiguous uint8 / int16 of shape (N, elements per picture)")
        if shape[1] * item < yuv420_bytes(w, h, bit_depth, layout, pitch_y, pitch_c, nb_frames):
            raise FuifGpuError(4, "encode_yuv420_device: the tensor's rows are shorter than a picture")
        ptrs = [frames.data_ptr() + k * shape[1] * item for k in range(shape[0])]
    else:
        ptrs = [int(p) if p else 0 for p in frames]
    if w is None or h is None:
        raise FuifGpuError(4, "encode_yuv420_device: w and h are needed")
    opt, lossy = _yuv_keywords(1, 1, **keywords)
    yuv = make_yuv_options(layout, pitch_y, pitch_c, nb_frames, framerate)
    return _encode_yuv420_call(ptrs, 1, w, h, bit_depth, yuv, opt, lossy)


def unpack_yuv420(frame_device_ptr, w, h, y_device_ptr, cb_device_ptr, cr_device_ptr, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0,
                  flag_device_ptr=None, stream=None):
    """fuifgpu_unpack_yuv420: one raw 4:2:0 frame in DEVICE memory -> three tight int32 planes in device memory (w*h, and twice
    ((w+1)/2) * ((h+1)/2) samples); flag_device_ptr: an int32 that becomes non-zero if a sample exceeds 2^bit_depth - 1; asynchronous on `stream`"""
    yuv = make_yuv_options(layout, pitch_y, pitch_c)
    _check(lib().fuifgpu_unpack_yuv420(frame_device_ptr, int(w), int(h), int(bit_depth), C.byref(yuv), y_device_ptr, cb_device_ptr, cr_device_ptr,
                                      flag_device_ptr, stream))


def pack_yuv420(y_device_ptr, cb_device_ptr, cr_device_ptr, w, h, frame_device_ptr, bit_depth=8, layout="i420", pitch_y=0, pitch_c=0, stream=None):
    """fuifgpu_pack_yuv420, the inverse of unpack_yuv420: three tight int32 planes in DEVICE memory (w*h, and twice ((w+1)/2) * ((h+1)/2)
    samples) -> one raw 4:2:0 frame in device memory, every sample clamped to [0, 2^bit_depth - 1]; asynchronous on `stream`"""
    yuv = make_yuv_options(layout, pitch_y, pitch_c)
    _check(lib().fuifgpu_pack_yuv420(y_device_ptr, cb_device_ptr, cr_device_ptr, int(w), int(h), int(bit_depth), C.byref(yuv), frame_device_ptr, stream))


def decode_yuv420(blobs, layout="i420", pitch_y=0, pitch_c=0, nb_frames=1, preview=-1):
    """same-geometry `fuif -y` streams -> list of raw YUV 4:2:0 frames (bytes), the counterpart of encode_yuv420_batch: one batch whose
    inverse schedule keeps the recorded [YCbCr, ChromaSubsample] pair (keep = 2), one pack launch, one copy to the host.  An image whose
    status says corrupt or unsupported raises"""
    plan = Plan(blobs[0], keep=2)
    size = plan.yuv420_bytes(layout, pitch_y, pitch_c, nb_frames)
    batch = Batch(plan, len(blobs), sum(len(b) for b in blobs))
    L = lib()
    dev = None
    try:
        batch.upload(blobs, preview)
        batch.decode()
        batch.undo_transforms()
        dev = L.fuifgpu_dev_alloc(max(size * len(blobs), 16))
        if not dev:
            raise FuifGpuError(7, "decode_yuv420: no device memory for the frames")
        batch.pack_yuv420(0, len(blobs), dev, layout, pitch_y, pitch_c, nb_frames)   # (refuses a plan that is no 4:2:0 picture)
        st, _ = batch.status()
        if (st & ~1).any():                  # (bit 0, truncated, is what a preview asks for)
            raise FuifGpuError(2, "decode_yuv420: image status %s" % [int(v) for v in st])
        host = np.zeros(max(size * len(blobs), 1), np.uint8)
        _check(L.fuifgpu_dev_download(host.ctypes.data, dev, size * len(blobs)))
        return [host[k * size: (k + 1) * size].tobytes() for k in range(len(blobs))]
    finally:
        if dev:
            L.fuifgpu_dev_free(dev)
        batch.close()


def quantization_constant_yuv(quality, chroma_quality=None, squeeze=True, chroma_table=False, shift=0):
    """quantization_constant for `fuif -y` input (fuifgpu_quantization_constant_yuv: fuif.cpp:432-434 triples the luma factor and
    divides the quality factor by three)"""
    q = lib().fuifgpu_quantization_constant_yuv(float(quality), 101.0 if chroma_quality is None else float(chroma_quality), int(bool(squeeze)),
                                                int(bool(chroma_table)), int(shift))
    if q < 1:
        _check(-q)
    return q


def channel_stats(plane_device_ptr, n_samples, stats_device_ptr, stream=None):
    """fuifgpu_channel_stats: {min, max, zero samples} of n int32 samples in DEVICE memory accumulated into three int32 of device
    memory the caller has preset; asynchronous on `stream`"""
    _check(lib().fuifgpu_channel_stats(plane_device_ptr, int(n_samples), stats_device_ptr, stream))


def encode_plane_traffic():
    """(host->device, device->host) bytes of whole planes / channels the last encode call of this thread moved (fuifgpu_encode_plane_traffic)"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _check(lib().fuifgpu_encode_plane_traffic(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def encode_learn_traffic():
    """(sample bytes, statistic bytes) the tree learner of the last encode call of this thread copied device->host
    (fuifgpu_encode_learn_traffic): tree_mode 1 brings the samples of device-only channels, tree_mode 2 shortlists and record slices"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _check(lib().fuifgpu_encode_learn_traffic(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


LEARN_WHERE = {"host": 0, "gpu": 1, "levelwise": 2}


def learn_tree(props, bucket, n_samples=None, nprops=None, where="host", max_nodes=4095, max_depth=14, min_leaf=48, split_bits=0, scale=1.0, cap=None):
    """The writer's tree learner on one sample set (fuifgpu_learn_tree) -> (n_nodes, 4) int32 array of {prop, split, gt, le}, prop -1 a leaf.
    where: "host" (0, the recursive learner of tree_mode 1), "levelwise" (2, level by level with plain C++ statistics) -- props an
    (n_samples, nprops) int32 array, bucket n_samples uint8 classes 0..16 -- or "gpu" (1, level by level with the kernels of tree_mode 2):
    props and bucket are device addresses (ints) of the same two arrays, with n_samples and nprops given"""
    code = LEARN_WHERE.get(where, -1) if isinstance(where, str) else int(where)
    if code == 1:
        p_ptr, b_ptr = int(props), int(bucket)
        n, k = int(n_samples), int(nprops)
    else:
        p = np.ascontiguousarray(props, dtype=np.int32)
        b = np.ascontiguousarray(bucket, dtype=np.uint8)
        if p.ndim != 2 or b.ndim != 1 or b.shape[0] != p.shape[0]:
            raise FuifGpuError(4, "learn_tree: props is (n_samples, nprops), bucket n_samples classes")
        n, k = p.shape
        p_ptr, b_ptr = p.ctypes.data, b.ctypes.data
    if cap is None:
        cap = max(1, min(int(max_nodes), 2 * max(n, 0) + 1)) if max_nodes >= 1 else 1
    out = np.zeros((max(int(cap), 1), 4), np.int32)
    count = C.c_int(0)
    opt = LearnOptions(C.sizeof(LearnOptions), int(max_nodes), int(max_depth), int(min_leaf), int(split_bits), float(scale))
    _check(lib().fuifgpu_learn_tree(p_ptr, b_ptr, n, k, C.byref(opt), code, out.ctypes.data, int(cap), C.byref(count)))
    return out[: count.value].copy()


def quantization_constant(quality, chroma_quality=None, squeeze=True, chroma_table=False, shift=0):
    """the constant `fuif -Q quality[,chroma_quality]` gives a channel of hcshift + vcshift = shift (fuifgpu_quantization_constant)"""
    q = lib().fuifgpu_quantization_constant(float(quality), 101.0 if chroma_quality is None else float(chroma_quality), int(bool(squeeze)), int(bool(chroma_table)), int(shift))
    if q < 1:
        _check(-q)
    return q


def fwd_quantize(plane_device_ptr, n_samples, q, minmax_device_ptr=None, stream=None):
    """fuifgpu_fwd_quantize: n int32 samples in DEVICE memory divided by q in place (truncating); their {min, max} accumulated
    into two int32 of device memory when a pointer is given"""
    _check(lib().fuifgpu_fwd_quantize(plane_device_ptr, int(n_samples), int(q), minmax_device_ptr, stream))


def fwd_palette(plane_device_ptrs, n_samples, max_colors, index_device_ptr, stream=None):
    """fuifgpu_fwd_palette: the forward Palette (transform/palette.h:92-142) of up to four planes of n int32 samples in DEVICE memory.
    Returns None when they hold more than max_colors distinct tuples (nothing is written); otherwise the palette as a (planes, colours)
    int32 array in the reference's order, with every sample's colour number written to index_device_ptr (which may be the first plane)."""
    nb = len(plane_device_ptrs)
    ptrs = (C.c_void_p * max(nb, 1))(*[int(p) if p else 0 for p in plane_device_ptrs])
    pal = np.zeros((max(nb, 1), max(int(max_colors), 1)), dtype=np.int32)
    count = C.c_int(0)
    _check(lib().fuifgpu_fwd_palette(ptrs, nb, int(n_samples), int(max_colors), index_device_ptr, pal.ctypes.data, C.byref(count), stream))
    if count.value < 0:
        return None
    return np.ascontiguousarray(pal[:nb, :count.value])


def index_parse(blob):
    """[(first_channel, byte_offset)] from the stream's group index trailer (csrc/index.cpp); [] when it has none"""
    fc, st, n = np.zeros(4096, np.int32), np.zeros(4096, np.uint32), C.c_int(0)
    _check(lib().fuifgpu_index_parse(blob, len(blob), fc.ctypes.data, st.ctypes.data, 4096, C.byref(n)))
    return [(int(fc[i]), int(st[i])) for i in range(min(n.value, 4096))]


def index_append(blob, groups):
    """the stream with a group index trailer built from [(first_channel, byte_offset)] (an existing trailer is replaced)"""
    fc = np.array([g[0] for g in groups], np.int32)
    st = np.array([g[1] for g in groups], np.uint32)
    out, n = C.c_void_p(), C.c_size_t(0)
    _check(lib().fuifgpu_index_append(blob, len(blob), fc.ctypes.data, st.ctypes.data, len(groups), C.byref(out), C.byref(n)))
    res = C.string_at(out.value, n.value)
    lib().fuifgpu_free_blob(out)
    return res


def add_group_index(blobs, hbm_budget_bytes=200 << 30):
    """Existing streams (as the reference encoder writes them) -> the same bytes + the group index trailer, in the caller's order:
    one entropy-decode launch per geometry (a streaming batch: no output slab, no inverse transforms), the group starts the kernel
    went through (fuifgpu_batch_group_index) appended with index_append.  A stream that already has a valid trailer, or whose decode
    is flagged (truncated / corrupt: its group starts are not those of the whole file), or which the planner refuses (out of scope,
    corrupt header), comes back unchanged.  The Python form of
    fuif_amd/boundary/fuif_index_main.cpp."""
    out = list(blobs)
    todo = []
    for i, b in enumerate(blobs):
        try:
            if not index_parse(b):
                Plan(b)                     # a stream the planner refuses (out of scope, corrupt header) is copied through, like a flagged decode
                todo.append(i)
        except FuifGpuError:
            pass
    for sig, (plan, idx) in group_by_signature([blobs[i] for i in todo]).items():
        idx = [todo[k] for k in idx]
        per = 2 * plan.info.coef_elems + 19 * (1 << 20) + max(len(blobs[i]) for i in idx)
        chunk = max(1, min(len(idx), int(hbm_budget_bytes // per), 65535))
        for c0 in range(0, len(idx), chunk):
            part = idx[c0:c0 + chunk]
            sub = [blobs[i] for i in part]
            # (tmp_images = 1: an entropy-only run needs no transform arena; the default would reserve one for a whole chunk of images)
            batch = Batch(plan, len(sub), sum(len(b) for b in sub) + 4096 * len(sub), streaming=True, tmp_images=1)
            try:
                batch.upload(sub)
                batch.decode()
                batch.sync()
                st, _ = batch.status()
                for k, i in enumerate(part):
                    if st[k] == 0:
                        out[i] = index_append(blobs[i], batch.group_index(k))
            finally:
                batch.close()
    return out


def group_by_signature(blobs):
    """host-side batch scheduler, step 1: streams that share geometry + transform chain (equal
    fuifgpu_image_info::signature) can share a launch.  Returns {signature: (Plan, [indices])} in
    first-seen order.  Pure host code (no GPU)."""
    groups = {}
    for i, b in enumerate(blobs):
        p = Plan(b)
        sig = int(p.info.signature)
        if sig not in groups:
            groups[sig] = (p, [])
        groups[sig][1].append(i)
    return groups


def plan_bytes_per_image(plan, avg_blob_bytes=0):
    """HBM bytes one in-flight image needs: coefficient + output slabs + decoder scratch + its stream"""
    return 2 * plan.info.coef_elems + 4 * plan.info.out_elems + 19 * (1 << 20) + int(avg_blob_bytes)   # int16 coefficients, int32 outputs


def decode_mixed(blobs, preview=-1, hbm_budget_bytes=200 << 30):
    """Decode an arbitrary list of streams (mixed sizes / Squeeze and DCT chains, BASELINE config C5's
    shape): group by signature, run one batch per group in chunks that fit `hbm_budget_bytes`, and
    return the per-image output planes in the caller's order plus the status words."""
    outs = [None] * len(blobs)
    status = np.zeros(len(blobs), np.int32)
    for sig, (plan, idx) in group_by_signature(blobs).items():
        per = plan_bytes_per_image(plan, sum(len(blobs[i]) for i in idx) / len(idx))
        chunk = max(1, min(len(idx), int(hbm_budget_bytes // per), 65535))
        for c0 in range(0, len(idx), chunk):
            part = idx[c0:c0 + chunk]
            sub = [blobs[i] for i in part]
            batch = Batch(plan, len(sub), sum(len(b) for b in sub))
            try:
                batch.upload(sub, preview)
                batch.decode()
                batch.undo_transforms()
                batch.sync()
                st, _ = batch.status()
                for k, i in enumerate(part):
                    outs[i] = batch.out_planes(k)
                    status[i] = st[k]
            finally:
                batch.close()
    return outs, status
