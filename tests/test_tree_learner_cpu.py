"""CPU: tree_mode 2 (MANIAC trees learned with the statistics kernels of csrc/maniac_encode.hip) without a GPU: its -m gpu tests against the
wavefront emulator build, the two new symbols in the library and the header, the loud failure without a HIP device, and the one entry
point that refuses the mode."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("fuifgpu_learn_tree", "fuifgpu_encode_learn_traffic")


def test_gpu_tree_learner_tests_pass_on_the_wavefront_emulator():
    """tests/test_gpu_tree_learner.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_learn_samples_cols_jobs, k_learn_transpose, k_learn_root_hist, k_learn_stats (staged and unstaged nodes, one to four digit passes),
    k_learn_shortlist, k_learn_partition and the batch writer's tree_mode 2 route, checked without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_tree_learner.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_new_entry_points_are_exported_and_declared(gpulib):
    hdr = open(os.path.join(ROOT, "include", "fuifgpu.h")).read()
    declared = set(re.findall(r"\b(fuifgpu_[a-z0-9_]+)\s*\(", hdr))
    L = C.CDLL(os.path.join(ROOT, "fuif_amd", "libfuifgpu.so"))
    for s in NEW_SYMBOLS:
        assert s in declared and s in gpulib.ABI_SYMBOLS and hasattr(L, s), s
    assert gpulib.lib().fuifgpu_abi_version() == 3      # found by symbol lookup: the ABI version stays
    assert C.sizeof(gpulib.EncodeOptions) == 40         # the mode is a value of an existing field
    assert C.sizeof(gpulib.LearnOptions) == 32
    assert "tree_mode 0" in hdr and "2 = learned exactly as 1" in hdr


def test_tree_mode_2_fails_loudly_without_a_gpu(gpulib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from fuif_amd.synth import photographic
    big = photographic(97, 61, 3, 8, seed=1)            # without Squeeze its groups learn
    flat = np.full((3, 8, 16), 5, np.int32)              # nothing to learn, nothing to code: still no host route
    for img, kw in ((big, dict(squeeze=False)), (big, dict(quality=80)), (flat, dict())):
        for call in (lambda: gpulib.encode_image(img, 8, tree_mode=2, **kw), lambda: gpulib.encode_images([img, img], 8, tree_mode=2, **kw),
                     lambda: gpulib.encode_animation(np.stack([img, img]), tree_mode=2, **kw)):
            with pytest.raises(gpulib.FuifGpuError) as e:
                call()
            assert e.value.code == 5, kw                  # FUIFGPU_E_HIP
    raw = np.zeros(128 * 96 * 3 // 2, np.uint8)
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.encode_yuv420(raw, 128, 96, tree_mode=2, squeeze=False)
    assert e.value.code == 5
    props = np.zeros((200, 3), np.int32)
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.learn_tree(props.ctypes.data, props.ctypes.data, 200, 3, where="gpu")     # (never read: the first device allocation fails)
    assert e.value.code == 5
    assert len(gpulib.encode_image(big, 8, tree_mode=1, squeeze=False)) > 0               # the host learner needs no device


def test_encode_channels_refuses_tree_mode_2(gpulib):
    from fuif_amd.edgecases import _RawChannel
    L = gpulib.lib()
    plane = np.arange(64, dtype=np.int32).reshape(8, 8)
    raw = (_RawChannel * 1)(_RawChannel(8, 8, 0, 0, 0, 0, 0, 1, plane.ctypes.data))
    out, size = C.c_void_p(), C.c_size_t(0)
    L.fuifgpu_encode_channels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.POINTER(gpulib.EncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    for mode, want in ((1, 0), (2, 3)):                   # 3: FUIFGPU_E_UNSUPPORTED
        opt = gpulib.make_encode_options(0, 0, 12, mode, 4095, 0, 0, 0, 0)
        assert L.fuifgpu_encode_channels(raw, 1, 8, 8, 1, 8, None, 0, C.byref(opt), C.byref(out), C.byref(size)) == want
        if want == 0:
            L.fuifgpu_free_blob(out)
