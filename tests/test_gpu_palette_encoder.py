"""GPU parity (-m gpu) of the forward Palette kernels (transforms.hip k_palette_collect / k_palette_index and their one-channel forms,
fuifgpu_fwd_palette) and of the writer's routes that use them: gpu_forward, the batch writer, and pictures that live in device memory.

The raw transform is checked against numpy (np.unique(tuples, axis=0) IS the reference's std::set order: lexicographic, signed, component 0
most significant); the routes against the reference CLI's files (tests/golden/palette/) and against the host route byte for byte.
On a machine without a GPU tests/test_writer_palette.py runs this file against the wavefront emulator build."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd.synth import from_recipe, graphic, photographic
from test_gpu_device_encoder import DevInts
from test_writer_palette import same_stream

pytestmark = pytest.mark.gpu

PALETTE = os.path.join(GOLDEN, "palette")
with open(os.path.join(PALETTE, "manifest_palette.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
CLI_DEFAULTS = dict(palette_colors=256, compact_post=70, compact_pre=70)
UNTOUCHED = -7     # what the index buffer holds before a call


def fwd_palette_on_device(gpulib, planes, max_colors, in_place=False):
    """(palette or None, index buffer afterwards, planes afterwards) of fuifgpu_fwd_palette on uploaded copies of planes[nb][n]"""
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    devs = [DevInts(gpulib, p) for p in planes]
    index = None if in_place else DevInts(gpulib, np.full(planes.shape[1], UNTOUCHED, np.int32))
    try:
        pal = gpulib.fwd_palette([d.ptr for d in devs], planes.shape[1], max_colors, devs[0].ptr if in_place else index.ptr)
        after = np.stack([d.get() for d in devs])
        return pal, (after[0] if in_place else index.get()), after
    finally:
        for d in devs + ([] if in_place else [index]):
            d.free()


def check_against_numpy(gpulib, planes, max_colors):
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    uniq, inverse = np.unique(planes.T, axis=0, return_inverse=True)
    pal, index, after = fwd_palette_on_device(gpulib, planes, max_colors)
    assert np.array_equal(after, planes), "the planes were written"
    if len(uniq) > max_colors:
        assert pal is None and (index == UNTOUCHED).all(), "too many colours: nothing may be written"
        return None
    assert pal is not None and pal.shape == (planes.shape[0], len(uniq))
    assert np.array_equal(pal, uniq.T), "palette order"
    assert np.array_equal(index, inverse.ravel()), "indices"
    return pal


def from_table(table, n, seed):
    """n samples drawn from the rows of `table` (colours x nb), every row at least once when n allows"""
    table = np.asarray(table, dtype=np.int32)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(table), size=n)
    k = min(n, len(table))
    pick[rng.permutation(n)[:k]] = np.arange(k)
    return table[pick].T


# colours that are close in every way a packed key can confuse: one component apart (the last one), one sign apart, the key of all zero
# bits and the key of all one bits, and the int16 extremes
def awkward_table(nb):
    rows = [[0] * nb, [-1] * nb, [5] * nb, [5] * (nb - 1) + [6], [5] * (nb - 1) + [-5], [-5] + [5] * (nb - 1), [32767] * nb, [-32768] * nb,
            [0] * (nb - 1) + [1], [0] * (nb - 1) + [-1], [1] + [0] * (nb - 1), [-1] + [0] * (nb - 1), [-233, 166, 15, -46][:nb], [255, 0, 255, 0][:nb]]
    return np.unique(np.array(rows, dtype=np.int32), axis=0)


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(67, 5), (300, 200)], ids=["67x5", "300x200"])
def test_fwd_palette_against_numpy(gpulib, nb, shape):
    """67x5: not a multiple of a wavefront; 300x200: more than one pass of the grid (30 blocks of 256 lanes for 60 000 samples)"""
    table = awkward_table(nb)
    planes = from_table(table, shape[0] * shape[1], seed=10 * nb + shape[0])
    pal = check_against_numpy(gpulib, planes, 256)
    assert pal.shape[1] == len(table)
    assert check_against_numpy(gpulib, planes, len(table)) is not None           # exactly max_colors colours: a palette
    assert check_against_numpy(gpulib, planes, len(table) - 1) is None           # one more than max_colors: -1, the index buffer untouched
    assert check_against_numpy(gpulib, planes, 1) is None


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_one_colour_and_the_two_special_keys_alone(gpulib, nb):
    for value in (77, 0, -1):       # 0 / -1 in every component: the packed key of all zero bits / all one bits (for nb = 4, all 64 of them)
        planes = np.full((nb, 130), value, np.int32)
        pal = check_against_numpy(gpulib, planes, 1)
        assert pal.tolist() == [[value]] * nb
    both = from_table([[0] * nb, [-1] * nb], 333, seed=nb)
    assert check_against_numpy(gpulib, both, 2).tolist() == [[-1, 0]] * nb


@pytest.mark.parametrize("nb", [3, 4])
def test_many_colours_fill_and_collide_in_the_table(gpulib, nb):
    """4096 pixels drawn from 3000 random colours with max_colors = 4096 (the table is built directly: synth.graphic realises far fewer
    colours than it is asked for); then one colour too many"""
    rng = np.random.default_rng(77 + nb)
    table = np.unique(rng.integers(-300, 300, size=(3000, nb)), axis=0)
    planes = from_table(table, 4096, seed=5)
    pal = check_against_numpy(gpulib, planes, 4096)
    assert pal.shape[1] > 2000
    assert check_against_numpy(gpulib, planes, pal.shape[1]) is not None
    assert check_against_numpy(gpulib, planes, pal.shape[1] - 1) is None
    assert check_against_numpy(gpulib, planes, 100) is None                      # far too many: the kernel stops early, same answer


def test_one_channel_with_wide_ranges(gpulib):
    rng = np.random.default_rng(14)
    used = rng.choice(16384, size=1200, replace=False)                           # 14 bits, about 1200 values in use
    pal = check_against_numpy(gpulib, from_table(used[:, None], 40 * 36 * 4, seed=1), int(np.float32(0.7) * 16384))
    assert pal.shape == (1, 1200)
    wide = rng.integers(-32768, 32768, size=(1, 70000))                          # the whole int16 range, limit (int)(0.7f * 65536) = 45875
    wide[0, :2] = (-32768, 32767)
    pal = check_against_numpy(gpulib, wide, 45875)
    assert pal is not None and 40000 < pal.shape[1] <= 45875 and pal[0, 0] == -32768 and pal[0, -1] == 32767
    assert check_against_numpy(gpulib, rng.integers(-32768, 32768, size=(1, 110000)), 45875) is None


def test_two_calls_give_identical_outputs_and_the_index_may_replace_the_first_plane(gpulib):
    planes = from_table(np.unique(np.random.default_rng(3).integers(-40, 40, size=(500, 3)), axis=0), 300 * 200, seed=8)
    a = fwd_palette_on_device(gpulib, planes, 1000)
    b = fwd_palette_on_device(gpulib, planes, 1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])             # insertion order must not show
    pal, index, after = fwd_palette_on_device(gpulib, planes, 1000, in_place=True)
    assert np.array_equal(pal, a[0]) and np.array_equal(index, a[1]) and np.array_equal(after[1:], planes[1:])
    one = fwd_palette_on_device(gpulib, planes[:1], 1000, in_place=True)
    assert np.array_equal(one[0][0], np.unique(planes[0])) and np.array_equal(one[1], np.searchsorted(np.unique(planes[0]), planes[0]))


def test_a_sample_outside_the_int16_range_is_refused(gpulib):
    planes = np.array([[1, 2, 40000, 4], [1, 2, 3, 4]], np.int32)
    for sub in (planes, planes[:1]):
        with pytest.raises(gpulib.FuifGpuError) as e:
            fwd_palette_on_device(gpulib, sub, 10)
        assert e.value.code == 4


# ---- the writer's routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_gpu_forward_writes_the_reference_clis_bytes(gpulib, port, entry):
    img = from_recipe(entry["input"])
    mine = gpulib.encode_image(img, entry["bits"], tree_mode=0, gpu_forward=True, **entry["encode"])
    assert same_stream(port, mine, open(os.path.join(PALETTE, entry["file"]), "rb").read()), entry["name"]


def rolled_back_plane_bytes(port, blob):
    """tests/test_gpu_device_encoder.py's accounting (the groups the stream stores uncompressed although they are not trivial) over the
    channels that are planes: a palette (hshift < 0) is a table the host made, it never was on the device"""
    d = port.decode(blob, undo=False)
    assert d.ok
    return sum(4 * d.channels[c]["data"].size for c, start in d.groups
               if not (blob[start] & 1) and d.channels[c]["minval"] < d.channels[c]["maxval"] and d.channels[c]["hshift"] >= 0)


MIXED = [graphic(96, 72, 3, 8, seed=51, colors=20), from_recipe(dict(kind="photographic", w=96, h=72, channels=3, bits=8, seed=37, floor_to=8)),
         photographic(96, 72, 3, 8, seed=52)]


@pytest.mark.parametrize("tree_mode", [0, 1])
def test_a_batch_that_mixes_three_transform_chains(gpulib, port, tree_mode):
    """a palettised, a compacted and a photographic picture of one size in one batch: the host route picture by picture, the batch writer
    on host planes, and the device-resident route write the same bytes; the device route uploads no plane and downloads the rolled-back
    groups alone -- the palettes add no plane traffic"""
    kw = dict(tree_mode=tree_mode, index=True, split_bits=2, **CLI_DEFAULTS)
    host = [gpulib.encode_image(im, 8, **kw) for im in MIXED]
    chains = [[t[0] for t in port.decode(b, undo=False).transforms] for b in host]
    assert chains == [[1, 6, 7], [1, 6, 6, 6, 7], [1, 7]]
    assert gpulib.encode_images(MIXED, 8, **kw) == host
    assert gpulib.encode_images(MIXED, 8, gpu_forward=True, **kw) == host
    devs = [DevInts(gpulib, im) for im in MIXED]
    try:
        blobs = gpulib.encode_images_device([d.ptr for d in devs], 96, 72, 3, 8, **kw)
        traffic = gpulib.encode_plane_traffic()
        assert all(np.array_equal(d.get(), d.a) for d in devs), "the caller's planes were written"
    finally:
        for d in devs:
            d.free()
    assert blobs == host
    assert traffic == (0, sum(rolled_back_plane_bytes(port, b) for b in blobs))


@pytest.mark.parametrize("entry", [e for e in FIXTURES if e["lossless"]], ids=[e["name"] for e in FIXTURES if e["lossless"]])
def test_device_route_equals_the_host_route_and_round_trips_through_the_decoder(gpulib, port, entry):
    """every lossless fixture: encode_images_device writes the host route's bytes, and decode_batch of the tree_mode 1, index=True stream
    returns the source pixels"""
    img = from_recipe(entry["input"])
    kw = dict(tree_mode=1, index=True, split_bits=2, **entry["encode"])
    host = gpulib.encode_image(img, entry["bits"], **kw)
    dev = DevInts(gpulib, img)
    try:
        c, h, w = img.shape
        blobs = gpulib.encode_images_device([dev.ptr, dev.ptr], w, h, c, entry["bits"], **kw)
        traffic = gpulib.encode_plane_traffic()
    finally:
        dev.free()
    assert blobs == [host, host]
    assert traffic == (0, 2 * rolled_back_plane_bytes(port, host))
    outs, st = gpulib.decode_batch([host, host])
    assert not st.any()
    for planes in outs:
        assert len(planes) == c and all(np.array_equal(planes[k], img[k]) for k in range(c)), entry["name"]
