"""GPU parity (-m gpu) of the device-resident encode route: fuifgpu_encode_images_device takes pictures that already live in device
memory, keeps the transformed channels there until the last coded byte, and brings back only their statistics (transforms.hip
k_channel_stats, fuifgpu_channel_stats) and the tree learner's samples (maniac_encode.hip k_learn_samples_jobs).

The yardstick is the bytes of the host-pointer route: the reference CLI's files (tests/golden/lossy/, and the lossless `-I 0 -K 0 -X 0
-Y 0` cases of tests/test_writer.py) with fixed trees, fuif_amd.encode_images on the host planes with learned ones.  "Device-resident" is
what fuifgpu_encode_plane_traffic reports.  On a machine without a GPU tests/test_device_encoder_cpu.py runs this file against the
wavefront emulator build."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd.synth import photographic, write_pnm

pytestmark = pytest.mark.gpu

EMULATED = ("_emu" in os.path.basename(os.environ.get("FUIF_AMD_LIB", "")))
LOSSY = os.path.join(GOLDEN, "lossy")
with open(os.path.join(LOSSY, "manifest_lossy.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
LOSSLESS = [(97, 61, 3, 8, 2), (64, 48, 1, 8, 3), (80, 72, 4, 14, 4)]   # the cases tests/test_writer.py compares with the reference CLI byte for byte
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
E_ARG = 4


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


def rolled_back_bytes(port, blob):
    """bytes of the channels `blob` stores uncompressed although they are not trivial, read off the stream itself: the groups the
    writer rolled back (encoding.cpp:545-551: the compressed form was no smaller) -- the only samples the device route may bring
    to the host.  A group header starts with the byte (predictor << 1) + compress."""
    d = port.decode(blob, undo=False)
    assert d.ok
    total = 0
    for channel, start in d.groups:
        ch = d.channels[channel]
        if not (blob[start] & 1) and ch["minval"] < ch["maxval"]:
            total += 4 * ch["data"].size
    return total


def device_encode(gpulib, imgs, bits, port=None, **kw):
    """encode_images_device on uploaded copies of `imgs`; the device planes must come back as they went in.  With `port`: the plane
    traffic of the call must be no upload at all and the download of exactly the groups that were rolled back"""
    devs = [DevInts(gpulib, im) for im in imgs]
    try:
        c, h, w = devs[0].a.shape
        blobs = gpulib.encode_images_device([d.ptr for d in devs], w, h, c, bits, **kw)
        traffic = gpulib.encode_plane_traffic()
        for d in devs:
            assert np.array_equal(d.get(), d.a), "the caller's planes were written"
        if port is not None:
            assert traffic == (0, sum(rolled_back_bytes(port, b) for b in blobs))
        return blobs, traffic
    finally:
        for d in devs:
            d.free()


# ---- 1. the statistics kernel ------------------------------------------------------------------------------------------------------
def stats_on_device(gpulib, values, skew=0, preset=(INT32_MAX, INT32_MIN, 0)):
    """skew: samples in front of the plane, so that it does not start on a 16-byte boundary (the kernel's one-by-one head)"""
    guard = 0            # a zero next to the plane: a read outside it would show in the count
    plane = DevInts(gpulib, np.concatenate([np.full(skew, guard, np.int32), values, np.full(5, guard, np.int32)]))
    st = DevInts(gpulib, list(preset))
    try:
        gpulib.channel_stats(plane.ptr + 4 * skew, len(values), st.ptr)
        got = st.get()
        assert np.array_equal(plane.get(), plane.a), "the plane or its guard words were written"
        return tuple(int(v) for v in got)
    finally:
        plane.free()
        st.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257] + ([] if EMULATED else [65537]))
def test_stats_lengths_around_the_wavefront_and_the_block(gpulib, n):
    rng = np.random.default_rng(n)
    v = rng.integers(-32768, 32768, size=n).astype(np.int32)
    v[v == 0] = 7
    for extreme in (32767, -32768):
        w = v.copy()
        w[-1] = extreme                       # the extreme value and a zero sit in the last (partial) wavefront
        if n > 1:
            w[-2] = 0
        if n > 40:
            w[5] = 0
            w[n // 2] = 0
        want = (int(w.min()), int(w.max()), int((w == 0).sum()))
        for skew in (0, 1, 3):
            assert stats_on_device(gpulib, w, skew) == want, (n, extreme, skew)


def test_stats_accumulate_and_edge_arguments(gpulib):
    L = gpulib.lib()
    v = np.array([-700, 5, 699, 0, 0, 12], np.int32)
    assert stats_on_device(gpulib, v, preset=(-1000, 7, 40)) == (-1000, 699, 42)     # preset values take part: min / max accumulate, zeros add
    assert stats_on_device(gpulib, v, preset=(3, 100000, -2)) == (-700, 100000, 0)
    plane, st = DevInts(gpulib, v), DevInts(gpulib, [-1000, 7, 40])
    try:
        assert L.fuifgpu_channel_stats(plane.ptr, 0, st.ptr, None) == 0              # n == 0 leaves the triple alone (and needs no plane)
        assert L.fuifgpu_channel_stats(None, 0, st.ptr, None) == 0
        assert list(st.get()) == [-1000, 7, 40]
        assert L.fuifgpu_channel_stats(plane.ptr, -1, st.ptr, None) == E_ARG
        assert L.fuifgpu_channel_stats(None, 6, st.ptr, None) == E_ARG
        assert L.fuifgpu_channel_stats(plane.ptr, 6, None, None) == E_ARG
        assert L.fuifgpu_channel_stats(plane.ptr, 2 ** 31, st.ptr, None) == E_ARG    # the zero count is an int32
        assert list(st.get()) == [-1000, 7, 40] and np.array_equal(plane.get(), v)
    finally:
        plane.free()
        st.free()


# ---- 2. the reference CLI's bytes --------------------------------------------------------------------------------------------------
def _same_up_to_the_stray_byte(mine, theirs):
    return mine == theirs[: len(mine)] and 0 <= len(theirs) - len(mine) <= 1


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_device_route_writes_the_reference_clis_lossy_bytes(gpulib, port, entry):
    s = entry["synth"]
    img = photographic(s["w"], s["h"], s["channels"], s["bits"], seed=s["seed"])
    theirs = open(os.path.join(LOSSY, entry["file"]), "rb").read()
    blobs, _ = device_encode(gpulib, [img, img], s["bits"], port, tree_mode=0, **entry["encode"])
    assert len(blobs) == 2 and all(_same_up_to_the_stray_byte(b, theirs) for b in blobs), entry["name"]


@pytest.mark.parametrize("w,h,c,bits,seed", LOSSLESS)
def test_device_route_writes_the_reference_clis_lossless_bytes(gpulib, port, tmp_path, w, h, c, bits, seed):
    from oracle_py import ref_cli, run_ref_cli
    img = photographic(w, h, c, bits, seed=seed)
    blobs, _ = device_encode(gpulib, [img, img], bits, port, tree_mode=0)
    assert blobs == [gpulib.encode_image(img, bits, tree_mode=0)] * 2     # what tests/test_writer.py pins to the CLI
    if ref_cli() is not None:                                               # ... and, where the reference CLI is built, its bytes directly
        src = str(tmp_path / ("in.pam" if c in (2, 4) else "in.ppm" if c == 3 else "in.pgm"))
        write_pnm(src, img, (1 << bits) - 1)
        out = str(tmp_path / "ref.fuif")
        r = run_ref_cli(["-I", "0", "-K", "0", "-X", "0", "-Y", "0", src, out])
        assert r.returncode == 0, r.stderr
        theirs = open(out, "rb").read()
        assert all(_same_up_to_the_stray_byte(b, theirs) for b in blobs)


# ---- 3. learned trees: the learner's samples come from the device --------------------------------------------------------------------
# (w, h, channels, bits, options, whether any group reaches the 4096 pixels from which the writer learns a tree at all)
# 97x61 and 64x48 squeezed: every group is smaller, the route must still agree; 97x61 without Squeeze: 5917 pixels per group, sample stride 1;
# 400x301 without Squeeze: 120 400 pixels per group -> stride 2 bumped to 3, the smallest case of the strided sample path
LEARNED = [(97, 61, 3, 8, dict(split_bits=2), False), (97, 61, 3, 8, dict(split_bits=2, squeeze=False), True)]
if EMULATED:
    LEARNED += [(64, 48, 1, 12, dict(split_bits=2), False)]
else:
    LEARNED += [(256, 256, 4, 14, dict(split_bits=2), True), (400, 301, 1, 8, dict(squeeze=False), True), (400, 301, 3, 8, dict(squeeze=False), True)]


@pytest.mark.parametrize("w,h,c,bits,kw,learns", LEARNED, ids=["%dx%dx%d_%d%s" % (t[:4] + ("_R0" if "squeeze" in t[4] else "",)) for t in LEARNED])
@pytest.mark.parametrize("lossy", [dict(), dict(quality=80)], ids=["lossless", "Q80"])
def test_learned_trees_equal_the_host_route(gpulib, port, w, h, c, bits, kw, learns, lossy):
    img = photographic(w, h, c, bits, seed=8000 + w)
    img2 = photographic(w, h, c, bits, seed=8001 + w)
    host = gpulib.encode_images([img, img2], bits, tree_mode=1, index=True, **kw, **lossy)
    if learns:
        fixed = gpulib.encode_images([img], bits, tree_mode=0, index=True, **{k: v for k, v in kw.items() if k != "split_bits"}, **lossy)[0]
        assert host[0] != fixed, "no tree was learned: the case checks nothing"
    blobs, _ = device_encode(gpulib, [img, img2], bits, port, tree_mode=1, index=True, **kw, **lossy)
    assert blobs == host


# ---- 4. planes stay on the device --------------------------------------------------------------------------------------------------
def test_planes_stay_on_the_device(gpulib, port):
    """RGB 97x61: nothing goes up, and what comes down is exactly the groups the stream stores uncompressed.  Squeezed, those are the
    pyramid's smallest channels (a few dozen samples each code no smaller than their raw bits: 492 of the picture's 17 751 samples,
    1968 bytes); without Squeeze no group is rolled back and the call moves no plane at all.  The host-pointer route with gpu_forward
    moves every plane both ways, so the counters are known to count."""
    img = photographic(97, 61, 3, 8, seed=2)
    planes = 3 * 97 * 61 * 4
    _, traffic = device_encode(gpulib, [img, img], 8, port, tree_mode=0)
    assert traffic[0] == 0 and traffic[1] <= 2 * planes // 8
    _, traffic = device_encode(gpulib, [img, img], 8, port, tree_mode=0, squeeze=False)
    assert traffic == (0, 0)
    gpulib.encode_images([img, img], 8, tree_mode=0, gpu_forward=True)
    up, down = gpulib.encode_plane_traffic()
    assert up >= 2 * planes and down >= 2 * planes, "the counters do not count"


def test_rolled_back_groups_are_the_only_download(gpulib, port):
    """8-bit uniform noise without transforms: every group codes larger than its raw bits and is rolled back to "uncompressed"
    (encoding.cpp:545-551) -- the one case in which a device-only channel comes to the host"""
    w, h = 64, 48
    noise = np.random.default_rng(11).integers(0, 256, size=(3, h, w)).astype(np.int32)
    host = gpulib.encode_images([noise], 8, squeeze=False, ycocg=False)
    blobs, traffic = device_encode(gpulib, [noise], 8, port, squeeze=False, ycocg=False)
    assert blobs == host
    assert traffic == (0, 3 * w * h * 4)


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------------
def test_device_encoded_streams_round_trip_on_the_device(gpulib, port):
    w, h = (72, 56) if EMULATED else (160, 120)
    img = photographic(w, h, 3, 8, seed=8100)
    plain = gpulib.encode_image(img, 8, tree_mode=1, index=False, split_bits=2, quality=80)
    for index in (True, False):
        blob = device_encode(gpulib, [img], 8, port, tree_mode=1, index=index, split_bits=2, quality=80)[0][0]
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
            assert not st.any() and [int(u) for u in used] == [len(plain)] * 3
            for k in range(3):
                planes = batch.out_planes(k)
                assert len(planes) == len(want.channels)
                assert all(np.array_equal(g, e["data"]) for g, e in zip(planes, want.channels))
        finally:
            batch.close()


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------
def test_flat_vanishing_and_single_pixel_pictures(gpulib, port):
    rng = np.random.default_rng(5)
    w, h = 72, 56
    low = (128 + rng.integers(-3, 4, size=(3, h, w))).astype(np.int32)    # at quality 20 every residual channel quantises to all zero
    flat = np.full((3, h, w), 77, np.int32)                                # every channel trivial
    for img in (low, flat):
        host = gpulib.encode_image(img, 8, tree_mode=1, quality=20)
        blobs, traffic = device_encode(gpulib, [img, img], 8, port, tree_mode=1, quality=20)
        assert blobs == [host, host] and (traffic == (0, 0) or img is low)   # (low: its 8x7 base channels are rolled back)
    blobs, traffic = device_encode(gpulib, [flat], 8)
    assert blobs == [gpulib.encode_image(flat, 8)] and traffic == (0, 0)
    for c in (1, 3):
        one = np.full((c, 1, 1), 200, np.int32)
        assert device_encode(gpulib, [one], 8)[0] == [gpulib.encode_image(one, 8)]
        assert device_encode(gpulib, [one], 8, quality=50)[0] == [gpulib.encode_image(one, 8, quality=50)]


def test_a_null_plane_pointer_is_refused(gpulib):
    L = gpulib.lib()
    img = DevInts(gpulib, photographic(16, 8, 3, 8, seed=1))
    try:
        ptrs = (C.c_void_p * 3)(img.ptr, None, img.ptr)
        outs = (C.c_void_p * 3)(1, 2, 3)
        sizes = (C.c_size_t * 3)(9, 9, 9)
        assert L.fuifgpu_encode_images_device(ptrs, 3, 16, 8, 3, 8, None, None, outs, sizes) == E_ARG
        assert [outs[k] for k in range(3)] == [None] * 3 and [sizes[k] for k in range(3)] == [0] * 3
        assert L.fuifgpu_encode_images_device(None, 3, 16, 8, 3, 8, None, None, outs, sizes) == E_ARG
        assert L.fuifgpu_encode_images_device(ptrs, 0, 16, 8, 3, 8, None, None, outs, sizes) == E_ARG
        with pytest.raises(gpulib.FuifGpuError) as e:
            gpulib.encode_images_device([img.ptr, 0], 16, 8, 3, 8)
        assert e.value.code == E_ARG
    finally:
        img.free()


def test_a_tensor_like_object_is_taken_as_it_is(gpulib):
    """an object with data_ptr(), shape (N, C, H, W), an int32 dtype and contiguous layout (a torch tensor on the current device qualifies)"""
    imgs = np.stack([photographic(40, 24, 3, 8, seed=k) for k in (1, 2)])
    dev = DevInts(gpulib, imgs)

    class Slab:
        shape, dtype = imgs.shape, "int32"

        def data_ptr(self):
            return dev.ptr

        def is_contiguous(self):
            return True
    try:
        assert gpulib.encode_images_device(Slab(), bit_depth=8) == gpulib.encode_images(list(imgs), 8)
        Slab.dtype = "float32"
        with pytest.raises(gpulib.FuifGpuError):
            gpulib.encode_images_device(Slab(), bit_depth=8)
    finally:
        dev.free()
