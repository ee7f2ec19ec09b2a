"""GPU parity (-m gpu) of the forward Matching kernels (transforms.hip k_match_frames_runs / _erode / _apply, fuifgpu_fwd_match_frames) and
of the writer's animation routes that use them: gpu_forward, the batch writer, and clips that live in device memory.

The raw transform is checked against the reference's own match channel (coded channel 0 of the -R 0 files of tests/golden/animation/) and
against a numpy statement of the rule (match_rule below); the routes against the reference CLI's files and against the host route byte for
byte.  On a machine without a GPU tests/test_writer_animation.py runs this file against the wavefront emulator build."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd.synth import from_recipe
from test_gpu_device_encoder import DevInts
from test_gpu_palette_encoder import rolled_back_plane_bytes
from test_writer_palette import same_stream

pytestmark = pytest.mark.gpu

ANIMATION = os.path.join(GOLDEN, "animation")
with open(os.path.join(ANIMATION, "manifest_animation.json")) as _f:
    FIXTURES = json.load(_f)["fixtures"]
IDS = [e["name"] for e in FIXTURES]
LOSSLESS = [e for e in FIXTURES if e["lossless"]]
R0 = [e for e in FIXTURES if "match_zeroed" in e]
UNTOUCHED = -7     # what the match buffer holds before a call


def golden(entry):
    with open(os.path.join(ANIMATION, entry["file"]), "rb") as f:
        return f.read()


def match_rule(planes, fh):
    """(match channel, mask of the samples that are set to zero) of a (C, H, W) strip of frames fh rows high: transform/2dmatch.h:303-381
    with maxdist = -1.  A sample of row y >= fh equals when every plane holds what it holds fh rows up; maximal horizontal runs of at
    least clamp(w / 50, 5, 40) equal samples are matched; each of three sweeps flags the matched samples that have a never-matched
    sample above or to the left, or a never-matched or already flagged one below or to the right (the picture's edges do not count);
    what is matched and not flagged is set to zero."""
    _, h, w = planes.shape
    shortest = min(40, max(5, w // 50))
    m = np.zeros((h, w), dtype=bool)
    equal = (planes[:, fh:] == planes[:, :-fh]).all(axis=0)
    for y in range(fh, h):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], equal[y - fh].astype(np.int8), [0]))))
        for a, b in zip(edges[::2], edges[1::2]):
            m[y, a:b] = b - a >= shortest
    flagged = np.zeros_like(m)
    for _ in range(3):
        gone = ~m | flagged
        near = np.zeros_like(m)
        near[1:] |= ~m[:-1]
        near[:, 1:] |= ~m[:, :-1]
        near[:-1] |= gone[1:]
        near[:, :-1] |= gone[:, 1:]
        flagged = flagged | (m & near)
    return m.astype(np.int32), m & ~flagged


def fwd_match_on_device(gpulib, strip, nb_frames):
    """(match channel, planes afterwards) of fuifgpu_fwd_match_frames on uploaded copies of the (C, H, W) strip"""
    strip = np.ascontiguousarray(strip, dtype=np.int32)
    c, h, w = strip.shape
    devs = [DevInts(gpulib, p) for p in strip]
    match = DevInts(gpulib, np.full((h, w), UNTOUCHED, np.int32))
    try:
        gpulib.fwd_match_frames([d.ptr for d in devs], w, h, nb_frames, match.ptr)
        return match.get(), np.stack([d.get() for d in devs])
    finally:
        for d in devs + [match]:
            d.free()


def check_against_the_rule(gpulib, strip, nb_frames):
    strip = np.ascontiguousarray(strip, dtype=np.int32)
    m, zeroed = match_rule(strip, strip.shape[1] // nb_frames)
    got_m, got_planes = fwd_match_on_device(gpulib, strip, nb_frames)
    assert np.array_equal(got_m, m), "match channel"
    expect = strip.copy()
    expect[:, zeroed] = 0
    assert np.array_equal(got_planes, expect), "the planes: zero exactly where a matched sample kept its mark, untouched elsewhere"
    return m, zeroed


def strip_of(w, fh, nb_frames, channels=2, seed=1):
    """frames that differ in EVERY sample from the frame above (values 1.. so that a zeroed sample shows), as a (C, H, W) strip; the tests
    copy the spans that are to match from the row fh above"""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 50, size=(channels, fh, w))
    return np.concatenate([base + 50 * f for f in range(nb_frames)], axis=1).astype(np.int32)


def keep(strip, fh, y0, y1, x0, x1):
    """rows y0..y1-1, samples x0..x1-1 become what is fh rows above them (after the rows above have been made)"""
    for y in range(y0, y1):
        strip[:, y, x0:x1] = strip[:, y - fh, x0:x1]


# ---- the raw transform -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", R0, ids=[e["name"] for e in R0])
def test_fwd_match_frames_gives_the_references_match_channel(gpulib, ref, entry):
    """the channels as they stand in front of the match are what the reference decodes when only the match is undone: its own coded
    channels with every matched sample copied down from the frame above"""
    d = ref.decode(golden(entry), undo=False)
    assert d.ok
    metas = sum(1 for t in entry["transforms"] if t[0] in (6, 8))
    fh, nf = entry["frame_h"], entry["frames"]
    their_m = np.asarray(d.channels[0]["data"]).reshape(fh * nf, -1)
    coded = np.stack([np.asarray(ch["data"]).reshape(their_m.shape) for ch in d.channels[metas:]])
    before = coded.copy()
    for y in range(fh, fh * nf):
        before[:, y] = np.where(their_m[y] != 0, before[:, y - fh], before[:, y])
    got_m, got_planes = fwd_match_on_device(gpulib, before, nf)
    assert np.array_equal(got_m, their_m) and int((got_m != 0).sum()) == entry["match_nonzero"]
    assert np.array_equal(got_planes, coded) and int((got_planes != before).any(axis=0).sum()) <= entry["match_zeroed"]
    m, zeroed = check_against_the_rule(gpulib, before, nf)
    assert int(zeroed.sum()) == entry["match_zeroed"]


def test_a_row_that_is_one_run_of_exactly_the_shortest_length_and_one_that_is_too_narrow(gpulib):
    five = strip_of(5, 3, 2)
    keep(five, 3, 3, 6, 0, 5)                                   # 5x3x2, all equal: every row one run of 5
    m, zeroed = check_against_the_rule(gpulib, five, 2)
    assert m[3:].all() and not m[:3].any() and zeroed[4:].all() and not zeroed[3].any()     # the first row of frame 1 is always flagged
    four = strip_of(4, 3, 2)
    keep(four, 3, 3, 6, 0, 4)                                   # 4x3x2: all equal, and never matched
    m, zeroed = check_against_the_rule(gpulib, four, 2)
    assert not m.any() and not zeroed.any()


def test_runs_across_the_64_sample_chunks_and_up_to_the_last_sample(gpulib):
    s = strip_of(70, 7, 3, channels=3)
    keep(s, 7, 8, 12, 60, 70)                                   # a run over samples 60..69: crosses sample 64 and ends at the row's last sample
    keep(s, 7, 9, 10, 0, 4)                                     # too short
    keep(s, 7, 15, 21, 0, 70)                                   # frame 2: whole rows, 70 = one full chunk and six samples
    s[:, 17, 63] += 1                                          # ... split at the chunk's last sample
    s[:, 18, 64] += 1                                           # ... and at the next chunk's first
    m, zeroed = check_against_the_rule(gpulib, s, 3)
    assert m[8, 60:].all() and not m[8, :60].any() and not m[9, :4].any() and m[15].all() and m[17].sum() == 69 and m[18].sum() == 69
    assert zeroed.any()


@pytest.mark.parametrize("w,short,long_", [(300, 5, 6), (2100, 39, 40)], ids=["300_runs_5_6", "2100_runs_39_40"])
def test_runs_one_short_of_the_shortest_length_are_not_matched(gpulib, w, short, long_):
    fh = 8 if w == 300 else 4
    s = strip_of(w, fh, 2, channels=1)
    keep(s, fh, fh + 1, fh + 2, 10, 10 + short)
    keep(s, fh, fh + 1, fh + 2, 100, 100 + long_)
    keep(s, fh, fh + 2, fh + 3, 64 - short, 64)                 # ends at a chunk's last sample
    keep(s, fh, fh + 2, fh + 3, 128 - long_ + 1, 129)           # ends at a chunk's first sample
    keep(s, fh, fh + 3, fh + 4, w - long_, w)                   # ends with the row
    m, _ = check_against_the_rule(gpulib, s, 2)
    assert m[fh + 1].sum() == long_ and m[fh + 1, 100:100 + long_].all()
    assert m[fh + 2].sum() == long_ and m[fh + 2, 128 - long_ + 1:129].all()
    assert m[fh + 3].sum() == long_ and m[fh + 3, w - long_:].all()


def test_the_erode_leaves_the_interior_of_a_large_block_and_nothing_of_a_small_one(gpulib):
    s = strip_of(24, 10, 4, channels=3)
    keep(s, 10, 11, 19, 2, 14)                                  # 12 wide, 8 high, in frame 1
    keep(s, 10, 31, 35, 16, 20)                                 # 4 x 4 in frame 3: runs shorter than 5, never matched
    keep(s, 10, 21, 25, 15, 20)                                 # 5 x 4 in frame 2: matched, nothing survives three sweeps
    m, zeroed = check_against_the_rule(gpulib, s, 4)
    assert m[11:19, 2:14].all() and m.sum() == 12 * 8 + 5 * 4
    inside = np.zeros_like(zeroed)
    inside[12:16, 3:11] = True                                  # one sample off the top and left, three off the bottom and right
    assert np.array_equal(zeroed, inside)


def test_a_region_that_stays_equal_over_three_frames(gpulib):
    """frame 2 matches frame 1 where frame 1 matched frame 0: the samples above a matched sample are themselves zeroed in the output, and
    between two matched frames only the left and right rims go"""
    s = strip_of(40, 8, 3, channels=1)
    keep(s, 8, 8, 24, 4, 30)
    m, zeroed = check_against_the_rule(gpulib, s, 3)
    assert m[8:, 4:30].all() and zeroed[9:, 5:27].all() and not zeroed[8].any() and zeroed.sum() == 15 * 22


# ---- the writer's routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_gpu_forward_and_the_batch_writer_write_the_reference_clis_bytes(gpulib, port, entry):
    frames = from_recipe(entry["input"])
    theirs = golden(entry)
    forward = gpulib.encode_animation(frames, tree_mode=0, gpu_forward=True, **entry["encode"])
    assert same_stream(port, forward, theirs), entry["name"]
    assert forward == gpulib.encode_animation(frames, tree_mode=0, **entry["encode"])
    assert gpulib.encode_animations([frames], tree_mode=0, **entry["encode"]) == [forward]
    assert gpulib.encode_animations([frames], tree_mode=0, gpu_forward=True, **entry["encode"]) == [forward]


def device_encode(gpulib, port, clips, **kw):
    """encode_animations_device on uploaded copies of the clips: the caller's frames must come back as they went in, nothing is uploaded,
    and what is downloaded is exactly the groups the streams store uncompressed"""
    devs = [DevInts(gpulib, cl) for cl in clips]
    try:
        nf, c, h, w = devs[0].a.shape
        blobs = gpulib.encode_animations_device([d.ptr for d in devs], nf, w, h, c, **kw)
        traffic = gpulib.encode_plane_traffic()
        assert all(np.array_equal(d.get(), d.a) for d in devs), "the caller's frames were written"
    finally:
        for d in devs:
            d.free()
    assert traffic == (0, sum(rolled_back_plane_bytes(port, b) for b in blobs))
    return blobs, traffic


@pytest.mark.parametrize("entry", FIXTURES, ids=IDS)
def test_device_route_writes_the_reference_clis_bytes(gpulib, port, entry):
    frames = from_recipe(entry["input"])
    blobs, _ = device_encode(gpulib, port, [frames], tree_mode=0, **entry["encode"])
    assert same_stream(port, blobs[0], golden(entry)), entry["name"]


def test_no_plane_and_no_match_channel_leaves_the_device(gpulib, port):
    """learned trees on a clip none of whose groups is rolled back: the plane traffic of the whole call is zero"""
    entry = next(e for e in FIXTURES if e["name"] == "gray_2100x4x2_R0")
    frames = from_recipe(entry["input"])
    host = gpulib.encode_animation(frames, tree_mode=1, split_bits=2, **entry["encode"])
    assert rolled_back_plane_bytes(port, host) == 0
    blobs, traffic = device_encode(gpulib, port, [frames], tree_mode=1, split_bits=2, **entry["encode"])
    assert blobs == [host] and traffic == (0, 0)


def test_a_batch_of_three_clips_equals_three_single_calls(gpulib, port):
    clips = [from_recipe(dict(kind="filmstrip", w=48, h=8, frames=3, channels=3, bits=8, seed=seed, background=back, colors=9, noise=noise))
             for seed, back, noise in ((21, "photographic", 0.25), (22, "graphic", 0.0), (23, "photographic", 0.0))]
    kw = dict(tree_mode=1, index=True, split_bits=2, palette_colors=256, compact_post=70, compact_pre=70)
    single = [gpulib.encode_animation(cl, **kw) for cl in clips]
    chains = [[t[0] for t in port.decode(b, undo=False).transforms] for b in single]
    assert all(8 in ch for ch in chains) and len({tuple(ch) for ch in chains}) > 1          # clips of one batch with different chains
    assert gpulib.encode_animations(clips, **kw) == single
    assert gpulib.encode_animations(clips, gpu_forward=True, **kw) == single
    blobs, _ = device_encode(gpulib, port, clips, **kw)
    assert blobs == single

    class Tensor:       # what encode_animations_device reads of a torch tensor
        def __init__(self, dev):
            self.shape, self.dtype, self.dev = (3,) + clips[0].shape, "torch.int32", dev

        def data_ptr(self):
            return self.dev.ptr

        def is_contiguous(self):
            return True
    dev = DevInts(gpulib, np.stack(clips))
    try:
        assert gpulib.encode_animations_device(Tensor(dev), **kw) == single
    finally:
        dev.free()


@pytest.mark.parametrize("entry", LOSSLESS, ids=[e["name"] for e in LOSSLESS])
def test_lossless_streams_round_trip_through_the_products_decoder(gpulib, port, entry):
    frames = from_recipe(entry["input"])
    nf, c, fh, w = frames.shape
    kw = dict(tree_mode=1, index=True, split_bits=2, **entry["encode"])
    blobs, _ = device_encode(gpulib, port, [frames], **kw)
    assert blobs == [gpulib.encode_animation(frames, **kw)]
    outs, st = gpulib.decode_batch([blobs[0], blobs[0]])
    assert not st.any()
    for planes in outs:
        assert len(planes) == c and all(np.array_equal(np.asarray(planes[k]).reshape(nf, fh, w), frames[:, k]) for k in range(c)), entry["name"]
