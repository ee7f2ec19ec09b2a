"""GPU parity (-m gpu) of lossy encoding: the forward Quantize kernel (transforms.hip k_fwd_quantize, fuifgpu_fwd_quantize) and the
writer's GPU options with a quality (fuifgpu_encode_image_lossy / fuifgpu_encode_images_lossy).

The yardstick is the reference CLI's bytes (tests/golden/lossy/, written by the unmodified `fuif -I 0 -K 0 -X 0 -Y 0 -Q ...`, see
tests/golden/make_golden_lossy.py) and, for learned trees, the host writer that tests/test_writer_lossy.py pins to the same files.
On a machine without a GPU tests/test_writer_lossy.py runs this file against the wavefront emulator build."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd.synth import photographic

pytestmark = pytest.mark.gpu

EMULATED = ("_emu" in os.path.basename(os.environ.get("FUIF_AMD_LIB", "")))
LOSSY = os.path.join(GOLDEN, "lossy")
with open(os.path.join(LOSSY, "manifest_lossy.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class DevInts:
    """int32 values in device memory through the library's own allocator (host memory under the emulator)"""

    def __init__(self, gpulib, arr):
        self.L = gpulib.lib()
        self.a = np.ascontiguousarray(arr, dtype=np.int32)
        self.ptr = self.L.fuifgpu_dev_alloc(max(self.a.nbytes, 4))
        assert self.ptr
        assert self.L.fuifgpu_dev_upload(self.ptr, self.a.ctypes.data, self.a.nbytes) == 0

    def get(self):
        out = np.empty_like(self.a)
        assert self.L.fuifgpu_dev_download(out.ctypes.data, self.ptr, out.nbytes) == 0   # (synchronises with the null stream's kernels)
        return out

    def free(self):
        self.L.fuifgpu_dev_free(self.ptr)


def quantize_on_device(gpulib, values, q, skew=0):
    """skew: samples in front of the plane, so that it does not start on a 16-byte boundary (the kernel's one-by-one path)"""
    guard = 12345
    plane = DevInts(gpulib, np.concatenate([np.full(skew, guard, np.int32), values, np.full(3, guard, np.int32)]))
    mm = DevInts(gpulib, [INT32_MAX, INT32_MIN])
    try:
        rc = gpulib.lib().fuifgpu_fwd_quantize(plane.ptr + 4 * skew, len(values), q, mm.ptr, None)
        assert rc == 0
        got = plane.get()
        assert (got[:skew] == guard).all() and (got[skew + len(values):] == guard).all(), "samples outside the plane were touched"
        return got[skew: skew + len(values)], mm.get()
    finally:
        plane.free()
        mm.free()


def c_division(v, q):
    return np.fix(v.astype(np.float64) / q).astype(np.int32)   # exact: |v| < 2^15, the quotient's fraction is at least 1/q away from an integer


QS = [1, 61, 32767] if EMULATED else [1, 2, 3, 5, 7, 61, 122, 255, 1024, 2764, 32767]


@pytest.mark.parametrize("q", QS)
def test_every_int16_value_divides_like_c(gpulib, q):
    v = np.arange(-32768, 32768, dtype=np.int32)
    if EMULATED:
        v = np.concatenate([v[:100], v[32768 - 70: 32768 + 70], v[-17:]])[:257]
    got, mm = quantize_on_device(gpulib, v, q)
    want = c_division(v, q)
    assert np.array_equal(got, want)
    assert (mm[0], mm[1]) == (want.min(), want.max())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257] + ([] if EMULATED else [65537]))
def test_lengths_around_the_wavefront_and_the_block(gpulib, n):
    rng = np.random.default_rng(n)
    v = rng.integers(-32768, 32768, size=n).astype(np.int32)
    v[-1] = 32767 if n & 1 else -32768          # the extreme sits in the last (partial) wavefront
    for q in QS[:3] if EMULATED else (1, 3, 61, 2764):
        for skew in (0, 1, 3):
            got, mm = quantize_on_device(gpulib, v, q, skew)
            want = c_division(v, q)
            assert np.array_equal(got, want), (n, q, skew)
            assert (mm[0], mm[1]) == (want.min(), want.max()), (n, q, skew)


def test_ranges_accumulate_and_edge_arguments(gpulib):
    L = gpulib.lib()
    v = np.array([-700, 5, 699, -3, 0, 12], np.int32)
    plane, mm = DevInts(gpulib, v), DevInts(gpulib, [-1000, 7])
    try:
        # n == 0 leaves a preset pair alone (and needs no plane); the caller's preset values take part in the range
        assert L.fuifgpu_fwd_quantize(plane.ptr, 0, 3, mm.ptr, None) == 0
        assert L.fuifgpu_fwd_quantize(None, 0, 3, mm.ptr, None) == 0
        assert list(mm.get()) == [-1000, 7] and np.array_equal(plane.get(), v)
        assert L.fuifgpu_fwd_quantize(plane.ptr, len(v), 7, mm.ptr, None) == 0
        assert np.array_equal(plane.get(), [-100, 0, 99, 0, 0, 1]) and list(mm.get()) == [-1000, 99]
        # no range wanted
        assert L.fuifgpu_fwd_quantize(plane.ptr, len(v), 10, None, None) == 0
        assert np.array_equal(plane.get(), [-10, 0, 9, 0, 0, 0]) and list(mm.get()) == [-1000, 99]
        for bad_q in (0, -1):
            assert L.fuifgpu_fwd_quantize(plane.ptr, len(v), bad_q, mm.ptr, None) == 4
        assert L.fuifgpu_fwd_quantize(plane.ptr, -1, 2, mm.ptr, None) == 4
        assert L.fuifgpu_fwd_quantize(None, 6, 2, mm.ptr, None) == 4
        assert np.array_equal(plane.get(), [-10, 0, 9, 0, 0, 0])
    finally:
        plane.free()
        mm.free()


def _same_up_to_the_stray_byte(mine, theirs):
    return mine == theirs[: len(mine)] and 0 <= len(theirs) - len(mine) <= 1


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_gpu_path_writes_the_reference_clis_lossy_bytes(gpulib, entry):
    s = entry["synth"]
    img = photographic(s["w"], s["h"], s["channels"], s["bits"], seed=s["seed"])
    theirs = open(os.path.join(LOSSY, entry["file"]), "rb").read()
    mine = gpulib.encode_image(img, s["bits"], tree_mode=0, gpu_forward=True, gpu_entropy=True, **entry["encode"])
    assert _same_up_to_the_stray_byte(mine, theirs), entry["name"]
    batch = gpulib.encode_images([img, img], s["bits"], tree_mode=0, gpu_forward=True, **entry["encode"])
    assert len(batch) == 2 and all(_same_up_to_the_stray_byte(b, theirs) for b in batch), entry["name"]


SHAPES = [(97, 61, 3, 8), (64, 48, 1, 12), (40, 30, 4, 14)] if EMULATED else [(97, 61, 3, 8), (333, 200, 1, 12), (256, 256, 4, 14)]


@pytest.mark.parametrize("w,h,c,bits", SHAPES)
@pytest.mark.parametrize("kw", [dict(quality=80), dict(quality=35, chroma_quality=70)], ids=["Q80", "Q35_70"])
def test_host_and_gpu_agree_with_learned_trees(gpulib, w, h, c, bits, kw):
    img = photographic(w, h, c, bits, seed=8000 + w)
    split = 2 if w * h < 20000 else None       # small pictures: let the learner split at all
    host = gpulib.encode_image(img, bits, tree_mode=1, index=True, split_bits=split, **kw)
    assert host != gpulib.encode_image(img, bits, tree_mode=1, index=True, split_bits=split)
    for gpu in (dict(gpu_forward=True), dict(gpu_entropy=True), dict(gpu_forward=True, gpu_entropy=True)):
        assert gpulib.encode_image(img, bits, tree_mode=1, index=True, split_bits=split, **gpu, **kw) == host, gpu
    for gpu_forward in (False, True):
        assert gpulib.encode_images([img, img], bits, tree_mode=1, index=True, split_bits=split, gpu_forward=gpu_forward, **kw) == [host, host]


def test_channels_that_vanish(gpulib, port):
    """a low-contrast picture at quality 20 -- every residual channel quantises to all zero, so the GPU path downloads none of them --
    and a flat picture: the same bytes as the host route, and streams that decode"""
    rng = np.random.default_rng(5)
    w, h = 72, 56        # (a larger picture of +-3 noise keeps +-1 in its coarsest residuals, whose constant is 1)
    low = (128 + rng.integers(-3, 4, size=(3, h, w))).astype(np.int32)
    flat = np.full((3, h, w), 77, np.int32)
    for img in (low, flat):
        host = gpulib.encode_image(img, 8, tree_mode=1, quality=20)
        assert gpulib.encode_image(img, 8, tree_mode=1, quality=20, gpu_forward=True, gpu_entropy=True) == host
        assert gpulib.encode_images([img, img], 8, tree_mode=1, quality=20, gpu_forward=True) == [host, host]
        pre, post = port.decode_both(host)
        assert pre.ok and post.ok
        n_base = 3
        assert all(ch["minval"] == 0 and ch["maxval"] == 0 for ch in pre.channels[n_base:]), "a residual channel survived"
        assert post.channels[0]["data"].shape == (h, w)


def test_lossy_streams_round_trip_on_the_device(gpulib, port):
    w, h = (72, 56) if EMULATED else (160, 120)
    img = photographic(w, h, 3, 8, seed=8100)
    split = 2
    plain = gpulib.encode_image(img, 8, tree_mode=1, index=False, split_bits=split, quality=80)
    for index in (True, False):
        blob = gpulib.encode_images([img], 8, tree_mode=1, index=index, split_bits=split, gpu_forward=True, quality=80)[0]
        assert blob == gpulib.encode_image(img, 8, tree_mode=1, index=index, split_bits=split, quality=80)
        assert blob[: len(plain)] == plain and (len(blob) > len(plain)) == index   # the index is a trailer behind the stream
        want = port.decode(blob)
        assert want.ok
        plan = gpulib.Plan(blob)
        batch = gpulib.Batch(plan, 3, 3 * len(blob))
        try:
            batch.upload([blob] * 3)
            batch.decode()
            batch.undo_transforms()
            batch.sync()
            st, used = batch.status()
            assert not st.any() and [int(u) for u in used] == [len(plain)] * 3   # bytes consumed: the stream, not its index trailer
            for k in range(3):
                planes = batch.out_planes(k)
                assert len(planes) == len(want.channels)
                assert all(np.array_equal(g, e["data"]) for g, e in zip(planes, want.channels))
        finally:
            batch.close()
        outs, st = gpulib.decode_batch([blob, blob])
        assert not st.any() and all(np.array_equal(g, e["data"]) for planes in outs for g, e in zip(planes, want.channels))
