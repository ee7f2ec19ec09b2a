"""GPU parity (-m gpu) of tree_mode 2: the writer's MANIAC trees learned level by level with the statistics kernels of
csrc/maniac_encode.hip (k_learn_stats, k_learn_shortlist, k_learn_partition) write the bytes of tree_mode 1, whose trees the recursive
host learner builds.  fuifgpu_learn_tree runs the learner on its own: where=1 (device rows, the kernels) against where=0 (the host learner).
On a machine without a GPU tests/test_tree_learner_cpu.py runs this file against the wavefront emulator build."""
import os

import numpy as np
import pytest

from fuif_amd.synth import photographic
from test_tree_learner_levelwise import correlated

pytestmark = pytest.mark.gpu

EMULATED = ("_emu" in os.path.basename(os.environ.get("FUIF_AMD_LIB", "")))


class Dev:
    """an array in device memory through the library's own allocator (host memory under the emulator)"""

    def __init__(self, gpulib, arr):
        self.L = gpulib.lib()
        self.a = np.ascontiguousarray(arr)
        self.ptr = self.L.fuifgpu_dev_alloc(max(self.a.nbytes, 4))
        assert self.ptr
        assert self.L.fuifgpu_dev_upload(self.ptr, self.a.ctypes.data, self.a.nbytes) == 0

    def unchanged(self):
        out = np.empty_like(self.a)
        assert self.L.fuifgpu_dev_download(out.ctypes.data, self.ptr, out.nbytes) == 0
        return np.array_equal(out, self.a)

    def free(self):
        self.L.fuifgpu_dev_free(self.ptr)


def same_on_device(gpulib, props, bucket, **kw):
    props = np.ascontiguousarray(props, dtype=np.int32)
    bucket = np.ascontiguousarray(bucket, dtype=np.uint8)
    want = gpulib.learn_tree(props, bucket, where="host", **kw)
    dp, db = Dev(gpulib, props), Dev(gpulib, bucket)
    try:
        got = gpulib.learn_tree(dp.ptr, db.ptr, props.shape[0], props.shape[1], where="gpu", cap=max(len(want), 1) + 2, **kw)
        assert dp.unchanged() and db.unchanged(), "the caller's rows were written"
    finally:
        dp.free()
        db.free()
    assert got.shape == want.shape and np.array_equal(got, want), (kw, want[:8], got[:8])
    return want


# ---- 1. the learner on its own --------------------------------------------------------------------------------------------------------
def test_smallest_node_that_splits(gpulib):
    for n, nodes in ((95, 1), (96, 3)):
        props = np.zeros((n, 3), np.int32)
        props[:, 1] = np.arange(n) >= n - 48
        bucket = (np.arange(n) >= n - 48).astype(np.uint8) * 9
        assert len(same_on_device(gpulib, props, bucket, min_leaf=48, split_bits=1)) == nodes


def test_constant_two_valued_negative_and_wide_properties(gpulib):
    rng = np.random.default_rng(3)
    n = 1500
    props = np.zeros((n, 4), np.int32)
    props[:, 0] = 7
    props[:, 1] = rng.integers(0, 2, size=n) * 5 + 10
    props[:, 2] = rng.integers(-50, 50, size=n)
    props[:, 3] = 7
    bucket = (props[:, 1] > 10).astype(np.uint8) * 6 + rng.integers(0, 2, size=n).astype(np.uint8)
    assert same_on_device(gpulib, props, bucket, split_bits=1)[0][0] == 1
    props[:, 1] = (np.arange(n) >= n - 60) * 5 + 10
    same_on_device(gpulib, props, (props[:, 1] > 10).astype(np.uint8) * 6, split_bits=1)
    n = 3000
    props = rng.integers(-2 ** 17, 2 ** 17 + 1, size=(n, 5)).astype(np.int32)
    props[:3, 0] = [-2 ** 17, 2 ** 17, 0]
    props[:, 4] = -rng.integers(1, 9, size=n)
    bucket = np.clip((props[:, 0] // 2 ** 14) + 8 + (props[:, 4] < -4) * 2, 0, 16).astype(np.uint8)
    assert len(same_on_device(gpulib, props, bucket, split_bits=2)) > 3
    props[:, 1] = rng.choice([-2 ** 31, 2 ** 31 - 1, -1, 0, 12345], size=n)      # max - min needs all 32 bits: four digit passes
    same_on_device(gpulib, props, bucket, split_bits=2)


def test_identical_columns(gpulib):
    rng = np.random.default_rng(5)
    drive = rng.integers(-100, 100, size=3000).astype(np.int32)
    bucket = np.clip((drive + 100) // 13, 0, 16).astype(np.uint8)
    two = np.stack([rng.integers(0, 4, size=3000).astype(np.int32), drive, drive], axis=1)
    tree = same_on_device(gpulib, two, bucket, split_bits=1)
    assert len(tree) > 1 and 2 not in set(tree[:, 0])
    tree = same_on_device(gpulib, np.repeat(drive[:, None], 10, axis=1), bucket, split_bits=1)     # 30 exact ties: the shortlist overflows
    assert len(tree) > 1 and set(tree[:, 0]) <= {-1, 0}


@pytest.mark.parametrize("kw", [dict(max_depth=2), dict(split_bits=0), dict(split_bits=5, scale=3.0), dict(min_leaf=20, split_bits=1, max_nodes=7),
                                dict(min_leaf=20, split_bits=1, max_nodes=15), dict(min_leaf=6, max_depth=40, max_nodes=8000, split_bits=1)], ids=str)
def test_limits_bars_and_the_node_cap(gpulib, kw):
    props, bucket = correlated(8, 6000, 6)      # (6000 samples: above the 4096 a block stages in LDS at the root, below it from level 1 on)
    tree = same_on_device(gpulib, props, bucket, **kw)
    if "max_nodes" in kw and kw["max_nodes"] < 100:
        full = gpulib.learn_tree(props, bucket, **dict(kw, max_nodes=4095))
        assert len(full) > 15 and len(tree) == kw["max_nodes"], "the uncapped tree is no larger: the case checks nothing"


@pytest.mark.parametrize("n,nprops", [(4096, 13), (4097, 3)] + ([] if EMULATED else [(20000, 37)]))
def test_sample_sets_of_the_writers_sizes(gpulib, n, nprops):
    props, bucket = correlated(n, n, nprops, lo=-2000, hi=2000)
    assert len(same_on_device(gpulib, props, bucket, min_leaf=48 if n > 5000 else 12)) > 7


def test_empty_set_and_argument_errors(gpulib):
    L = gpulib.lib()
    d = Dev(gpulib, np.zeros(8, np.int32))
    try:
        assert len(gpulib.learn_tree(d.ptr, d.ptr, 0, 3, where="gpu")) == 1
        with pytest.raises(gpulib.FuifGpuError) as e:
            gpulib.learn_tree(d.ptr, d.ptr, 2, 0, where="gpu")
        assert e.value.code == 4
        with pytest.raises(gpulib.FuifGpuError) as e:
            gpulib.learn_tree(d.ptr, d.ptr, -1, 3, where="gpu")
        assert e.value.code == 4
    finally:
        d.free()


# ---- 2. tree_mode 2 writes the bytes of tree_mode 1 ------------------------------------------------------------------------------------
LOSSY = [dict(), dict(quality=80)]
LOSSY_IDS = ["lossless", "Q80"]
# (w, h, channels, bits, options, whether any group reaches the 4096 pixels from which the writer learns a tree): tests/test_gpu_device_encoder.py's list
SHAPES = [(97, 61, 3, 8, dict(split_bits=2), False), (97, 61, 3, 8, dict(split_bits=2, squeeze=False), True)]
if not EMULATED:
    SHAPES += [(256, 256, 4, 14, dict(split_bits=2), True), (400, 301, 1, 8, dict(squeeze=False), True),
               (256, 256, 1, 8, dict(squeeze=False, max_tree_nodes=8000), True)]     # the last: min_leaf 6, depth 40, the node cap may bind


def pictures(w, h, c, bits):
    return [photographic(w, h, c, bits, seed=8000 + w), photographic(w, h, c, bits, seed=8001 + w)]


def device_encode(gpulib, imgs, bits, **kw):
    devs = [Dev(gpulib, np.ascontiguousarray(im, dtype=np.int32)) for im in imgs]
    try:
        c, h, w = devs[0].a.shape
        blobs = gpulib.encode_images_device([d.ptr for d in devs], w, h, c, bits, **kw)
        traffic = gpulib.encode_plane_traffic(), gpulib.encode_learn_traffic()
        assert all(d.unchanged() for d in devs), "the caller's planes were written"
        return blobs, traffic
    finally:
        for d in devs:
            d.free()


@pytest.mark.parametrize("w,h,c,bits,kw,learns", SHAPES, ids=["%dx%dx%d_%d_%s" % (t[:4] + ("_".join("%s%s" % kv for kv in sorted(t[4].items())),)) for t in SHAPES])
@pytest.mark.parametrize("lossy", LOSSY, ids=LOSSY_IDS)
def test_batch_routes_write_the_bytes_of_tree_mode_1(gpulib, w, h, c, bits, kw, learns, lossy):
    """two different pictures per batch: learning groups of unequal content share every round"""
    imgs = pictures(w, h, c, bits)
    host = gpulib.encode_images(imgs, bits, tree_mode=1, index=True, **kw, **lossy)
    if learns:
        fixed = gpulib.encode_images(imgs, bits, tree_mode=0, index=True, **{k: v for k, v in kw.items() if k != "split_bits"}, **lossy)
        assert host[0] != fixed[0] and host[1] != fixed[1], "no tree was learned: the case checks nothing"
    assert gpulib.encode_images(imgs, bits, tree_mode=2, index=True, **kw, **lossy) == host
    blobs, _ = device_encode(gpulib, imgs, bits, tree_mode=2, index=True, **kw, **lossy)
    assert blobs == host


@pytest.mark.parametrize("lossy", LOSSY, ids=LOSSY_IDS)
def test_single_picture_animation_and_yuv_routes(gpulib, lossy):
    w, h = 97, 61
    img = photographic(w, h, 3, 8, seed=8000 + w)
    kw = dict(split_bits=2, squeeze=False)
    one = gpulib.encode_image(img, 8, tree_mode=1, **kw, **lossy)
    assert one != gpulib.encode_image(img, 8, tree_mode=0, squeeze=False, **lossy)
    assert gpulib.encode_image(img, 8, tree_mode=2, **kw, **lossy) == one
    assert gpulib.encode_image(img, 8, tree_mode=2, gpu_forward=True, gpu_entropy=True, **kw, **lossy) == one
    frames = np.stack([img, np.roll(img, 3, axis=2)])
    clip = gpulib.encode_animation(frames, tree_mode=1, **kw, **lossy)
    assert clip != gpulib.encode_animation(frames, tree_mode=0, squeeze=False, **lossy)
    assert gpulib.encode_animation(frames, tree_mode=2, **kw, **lossy) == clip
    assert gpulib.encode_animations([frames, frames[::-1]], tree_mode=2, **kw, **lossy) == gpulib.encode_animations([frames, frames[::-1]], tree_mode=1, **kw, **lossy)
    # a 128 x 96 4:2:0 frame without Squeeze: luma (12 288 samples) learns, chroma (3072) does not
    yw, yh = 128, 96
    luma = photographic(yw, yh, 1, 8, seed=77)[0].astype(np.uint8)
    chroma = photographic(yw // 2, yh // 2, 2, 8, seed=78).astype(np.uint8)
    raw = np.concatenate([luma.ravel(), chroma.ravel()])
    raw2 = np.concatenate([np.roll(luma, 5, axis=1).ravel(), chroma.ravel()])
    want = gpulib.encode_yuv420_batch([raw, raw2], yw, yh, tree_mode=1, squeeze=False, split_bits=2, **lossy)
    assert want[0] != gpulib.encode_yuv420(raw, yw, yh, tree_mode=0, squeeze=False, **lossy)
    assert gpulib.encode_yuv420_batch([raw, raw2], yw, yh, tree_mode=2, squeeze=False, split_bits=2, **lossy) == want
    assert gpulib.encode_yuv420(raw, yw, yh, tree_mode=2, squeeze=False, split_bits=2, **lossy) == want[0]
    devs = [Dev(gpulib, raw), Dev(gpulib, raw2)]
    try:
        assert gpulib.encode_yuv420_device([d.ptr for d in devs], yw, yh, tree_mode=2, squeeze=False, split_bits=2, **lossy) == want
        assert all(d.unchanged() for d in devs)
    finally:
        for d in devs:
            d.free()


# ---- 3. what crosses to the host -------------------------------------------------------------------------------------------------------
def test_samples_stay_on_the_device(gpulib):
    imgs = pictures(97, 61, 3, 8)
    kw = dict(split_bits=2, squeeze=False)
    one, (planes1, learn1) = device_encode(gpulib, imgs, 8, tree_mode=1, **kw)
    two, (planes2, learn2) = device_encode(gpulib, imgs, 8, tree_mode=2, **kw)
    assert one == two
    assert learn2[0] == 0 and learn2[1] > 0
    assert planes2 == planes1
    assert learn1[0] >= 2 * 3 * 97 * 61 * (4 * 13 + 1) and learn1[1] == 0, "the counter does not count"
    assert learn2[1] < learn1[0]
    gpulib.encode_images(imgs, 8, tree_mode=0)
    assert gpulib.encode_learn_traffic() == (0, 0)


# ---- 4. nothing to learn ---------------------------------------------------------------------------------------------------------------
def test_flat_single_pixel_and_small_pictures(gpulib):
    flat = np.full((3, 56, 72), 77, np.int32)
    one = np.full((3, 1, 1), 200, np.int32)
    small = photographic(60, 40, 3, 8, seed=4)          # 2400 pixels per group: below the 4096 from which a tree is learned
    for img in (flat, one, small):
        for lossy in LOSSY:
            want = gpulib.encode_image(img, 8, tree_mode=1, **lossy)
            assert want == gpulib.encode_image(img, 8, tree_mode=0, **lossy)
            assert gpulib.encode_image(img, 8, tree_mode=2, **lossy) == want
            assert gpulib.encode_images([img, img], 8, tree_mode=2, **lossy) == [want, want]
            blobs, (_, learn) = device_encode(gpulib, [img, img], 8, tree_mode=2, **lossy)
            assert blobs == [want, want] and learn == (0, 0)
