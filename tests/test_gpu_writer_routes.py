"""GPU (-m gpu): every route through the stream writer (fuif_amd/csrc/writer.cpp) writes the bytes and moves the planes that
tests/golden/writer_routes.json records (tests/golden/make_writer_routes.py: taken once, from the commit named in the file, before the
writer's host code was restructured).  Cases and routes: tests/writer_routes.py.  On a machine without a GPU
tests/test_writer_routes_cpu.py runs this file against the wavefront emulator build."""
import json
import os

import pytest

import writer_routes
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "writer_routes.json")) as _f:
    RECORD = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def cases():
    return writer_routes.cases()


def test_the_record_holds_every_case():
    assert sorted(RECORD) == sorted(writer_routes.CASE_NAMES)
    assert RECORD["learned_tm1"]["streams"] != RECORD["fixed_tm0"]["streams"]            # a tree was learned
    assert RECORD["learned_tm1"]["traffic"]["images_device_tm2"]["learn"][1] > 0          # ... and, tree_mode 2, with the kernels' statistics
    lossy = RECORD["lossy_q50"]["traffic"]["image_gpu_forward"]["plane"]
    assert 0 < lossy[1] < lossy[0]                                                        # channels that quantise to all zero stay on the device


@pytest.mark.parametrize("name", writer_routes.CASE_NAMES)
def test_every_route_writes_the_recorded_bytes_and_moves_the_recorded_traffic(gpulib, cases, name):
    writer_routes.check_case(gpulib, name, cases[name], RECORD[name])


def test_the_noise_picture_has_a_group_that_is_rolled_back(gpulib, port, cases):
    from test_gpu_device_encoder import rolled_back_bytes
    kind, pics, kw, _ = cases["rollback_noise14"]
    blob = gpulib.encode_image(pics[0], split_bits=writer_routes.SPLIT_BITS, **kw)
    assert writer_routes.digest(blob) == RECORD["rollback_noise14"]["streams"][0]
    assert rolled_back_bytes(port, blob) > 0, "no non-trivial group has its compress bit off: the case checks nothing"
