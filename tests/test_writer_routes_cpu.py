"""CPU: the record of tests/golden/writer_routes.json without a GPU: tests/test_gpu_writer_routes.py against the wavefront emulator build,
and the routes that need no device (the host writer of every case, with and without the index trailer) directly."""
import json
import os
import subprocess
import sys

import pytest

import writer_routes
from conftest import GOLDEN, ROOT

with open(os.path.join(GOLDEN, "writer_routes.json")) as _f:
    RECORD = json.load(_f)["cases"]


def test_gpu_writer_routes_pass_on_the_wavefront_emulator():
    if sys.platform != "linux" or os.uname().machine != "x86_64":
        pytest.skip("the emulator's context switch is x86-64 SysV assembly")
    from test_emulated_kernels import build_emulated_library
    env = dict(os.environ, FUIF_AMD_LIB=build_emulated_library(), EMU_ALARM="900")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_writer_routes.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def cases():
    return writer_routes.cases()


@pytest.mark.parametrize("name", writer_routes.CASE_NAMES)
def test_host_routes_write_the_recorded_bytes(gpulib, cases, name):
    writer_routes.check_case(gpulib, name, cases[name], RECORD[name], host_only=True)


@pytest.mark.parametrize("name", ["yuv10_75x49", "yuv10_75x49_q60"])
def test_the_yuv_cases_are_the_reference_clis_files(name):
    """the two cases that reproduce the reference's stale tail: the recorded stream is the file of tests/golden/yuv (whose last byte, a stray
    one of the reference's buffer, the writer does not produce: tests/test_writer_yuv.py)"""
    import hashlib
    theirs = open(os.path.join(GOLDEN, "yuv", name.replace("_q", "_Q") + ".fuif"), "rb").read()
    want = RECORD[name]["streams"][0]
    assert 0 <= len(theirs) - want["bytes"] <= 1 and hashlib.sha256(theirs[: want["bytes"]]).hexdigest() == want["sha256"]
