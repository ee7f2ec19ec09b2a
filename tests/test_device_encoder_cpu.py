"""CPU: the device-resident encode route (fuifgpu_encode_images_device, fuifgpu_channel_stats, fuifgpu_encode_plane_traffic) without a GPU:
its -m gpu tests against the wavefront emulator build, the three symbols in the library and the header, and the loud failure without
a HIP device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("fuifgpu_encode_images_device", "fuifgpu_channel_stats", "fuifgpu_encode_plane_traffic")


def test_gpu_device_encoder_tests_pass_on_the_wavefront_emulator():
    """tests/test_gpu_device_encoder.py against the kernels' own sources compiled for the wavefront emulator (tests/test_emulated_kernels.py):
    k_channel_stats' head / quads / tail and its wavefront reduction, k_learn_samples_jobs against the host learner's sampling loop, and the
    writer's device-only channels, checked without a GPU"""
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_device_encoder.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_new_entry_points_are_exported_and_declared(gpulib):
    hdr = open(os.path.join(ROOT, "include", "fuifgpu.h")).read()
    declared = set(re.findall(r"\b(fuifgpu_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(os.path.join(ROOT, "fuif_amd", "libfuifgpu.so"))
    for s in NEW_SYMBOLS:
        assert s in declared and s in gpulib.ABI_SYMBOLS and hasattr(L, s), s
    assert gpulib.lib().fuifgpu_abi_version() == 3      # found by symbol lookup: the ABI version stays


def test_device_route_fails_loudly_without_a_gpu(gpulib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    planes = np.zeros((3, 8, 16), np.int32)     # (never read: the first device allocation fails)
    for kw in (dict(), dict(quality=80)):
        with pytest.raises(gpulib.FuifGpuError) as e:
            gpulib.encode_images_device([planes.ctypes.data], 16, 8, 3, 8, **kw)
        assert e.value.code == 5 and "HIP" in str(e.value)     # FUIFGPU_E_HIP: there is no host route
    assert gpulib.encode_plane_traffic() == (0, 0)
