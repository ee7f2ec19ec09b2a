"""Predictors 1, 4..7, channel groups of more than one channel, and the median predictor's gradient beyond int16.

The fixtures are reference-written streams in tests/golden/manifest.json (tests/golden/make_golden.py, PREDICTOR_SPECS), so the parity
tests over the manifest decode them on the oracle, the kernels and the emulator without further code.  The tests here show that the
fixtures do what they are for -- conditions on the streams themselves, which hold for the reference alone -- and cover what a stream
file cannot: the reference ENCODER with every predictor (CPU, needs oracle/_ref), and the product's writer on a picture whose
gradient leaves int16 (host route on the CPU, the GPU routes under -m gpu).

The reference takes the median of (pixel_type)(left + top - topleft), left, top (context_predict.h:160,165; pixel_type = int16_t):
the gradient is narrowed, the context property left + top - topleft (:146) is not."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fuif_amd import edgecases
from fuif_amd.edgecases import WRAP_FIXTURES, count_gradient_wraps, group_headers

META = ("w", "h", "minval", "maxval", "q", "hshift", "vshift", "hcshift", "vcshift", "component", "size")

# fixture -> the predictor it is named for (a mixed -P string: the digit of the channel the fixture is about)
PREDICTOR_FIXTURES = dict([("rgb8_65x34_P%d_nosqueeze" % p, p) for p in (1, 4, 5, 6, 7)] + [
    ("gray8_1x9_P541_nosqueeze", 5), ("gray8_9x1_P541_nosqueeze", 5), ("gray8_2x7_P541_nosqueeze", 5),
    ("rgb8_97x61_P1", 1), ("rgb8_97x61_P5", 5), ("rgb8_97x61_P2461", 1), ("rgba14_40x36_P6", 6), ("rgba14_40x36_P1", 1),
    ("rgb8_65x34_E24_P5", 5), ("rgb8_61x47_G2_P5", 5), ("ga8_70x66_G2_P5", 5)])
# (-G 3 writes the bytes of -G 2 on this picture: the reference encoder finds no three neighbouring channels of one size, so only -G 2 is kept)
GROUP_FIXTURES = ("rgb8_61x47_G2", "rgb8_61x47_G2_P5", "rgb8_61x47_G3_flat_second_channel", "ga8_70x66_G2_P5")
CLI_QUADRANTS = "grad16_rgb14_quadrants_24x40_cli_I0"     # `fuif -I 0 -R 0 -K 0 -X 0 -Y 0` on edgecases.quadrants_14bit(24, 40)


def fixture_blob(name):
    with open(os.path.join(GOLDEN, name + ".fuif"), "rb") as f:
        return f.read()


def same(a, b):
    assert a.ok and b.ok
    assert a.transforms == b.transforms
    assert len(a.channels) == len(b.channels)
    for i, (x, y) in enumerate(zip(a.channels, b.channels)):
        assert {k: x[k] for k in META} == {k: y[k] for k in META}, i
        assert np.array_equal(x["data"], y["data"]), "channel %d: %d of %d samples differ" % (i, int((x["data"] != y["data"]).sum()), x["data"].size)


@pytest.mark.parametrize("name", sorted(PREDICTOR_FIXTURES))
def test_predictor_fixture_codes_a_compressed_group_with_its_predictor(port, name):
    """an uncompressed group carries the predictor in its header but never uses it (encoding.cpp:153-165,334-350)"""
    groups, _ = group_headers(fixture_blob(name), port)
    assert any(predictor == PREDICTOR_FIXTURES[name] and compress for _, _, predictor, compress in groups), groups


def test_mixed_predictor_string_is_one_digit_per_channel(port):
    """-P 2461 with Squeeze: channels 0, 1, 2 get 2, 4, 6 and every later channel the last digit (fuif.cpp:136, encoding.cpp:503)"""
    groups, _ = group_headers(fixture_blob("rgb8_97x61_P2461"), port)
    assert [g[2] for g in groups[:4]] == [2, 4, 6, 1] and all(g[2] == 1 for g in groups[3:])


def test_more_than_31_properties_with_a_predictor(port):
    """-E 24: up to twelve earlier channels give two properties each (context_predict.h:69-82: those with a range and hshift >= 0), 13 more are
    the channel's own; a compressed predictor-5 group with at least ten of them has 2 * 10 + 13 = 33 properties or more -- the 65-word
    property rows and half-length chunks of the entropy kernel"""
    groups, d = group_headers(fixture_blob("rgb8_65x34_E24_P5"), port)
    def properties(first):
        refs = sum(1 for c in d.channels[:first] if c["minval"] != c["maxval"] and c["hshift"] >= 0)
        return 2 * min(refs, 12) + 13
    assert any(predictor == 5 and compress and properties(first) > 31 for first, _, predictor, compress in groups), [(g, properties(g[0])) for g in groups]


def test_previews_cut_a_stream_with_a_predictor(port, manifest):
    """the preview cases of ga8_70x66_G2_P5 stop at a preview size: channels behind it are never decoded (size 0), and at least one
    compressed group in front of it has predictor 5 and is decoded"""
    entry = next(e for e in manifest["fixtures"] if e["name"] == "ga8_70x66_G2_P5")
    previews = [c for c in entry["cases"] if c["preview"] >= 0]
    assert len(previews) >= 2
    blob = fixture_blob("ga8_70x66_G2_P5")
    groups, _ = group_headers(blob, port)
    for c in previews:
        assert any(ch["size"] == 0 for ch in c["pre"]) and any(ch["size"] for ch in c["pre"]), c["case"]
        d = port.decode(blob, preview=c["preview"], undo=False)
        assert [ch["size"] for ch in d.channels] == [ch["size"] for ch in c["pre"]], c["case"]
        assert any(predictor == 5 and compress and d.channels[first]["size"] for first, _, predictor, compress in groups), c["case"]


def test_four_samples_are_always_stored_uncompressed(port):
    """gray8_2x2: uncompressed it costs 4 * 8 + 16 bits, which no compressed form of four samples undercuts (encoding.cpp:531-551), so this
    fixture pins the header and the uncompressed path of a 2x2 channel; gray8_2x7 beside it is the smallest two-column picture whose
    group stays compressed"""
    groups, _ = group_headers(fixture_blob("gray8_2x2_P541_nosqueeze"), port)
    assert groups == [(0, 0, 5, 0)]


@pytest.mark.parametrize("name", GROUP_FIXTURES)
def test_group_fixture_has_a_group_of_several_channels(port, name):
    groups, d = group_headers(fixture_blob(name), port)
    several = [g for g in groups if g[1] > 0]
    assert several and any(g[3] for g in several), groups
    if name.endswith("_P5"):
        assert any(g[2] == 5 and g[3] for g in several), groups
    if "flat" in name:
        # a channel with minval == maxval in front of a coded one, in a compressed group (encoding.cpp:300-303: filled, no symbols)
        assert any(g[3] and d.channels[g[0]]["minval"] == d.channels[g[0]]["maxval"] and
                   any(d.channels[c]["minval"] < d.channels[c]["maxval"] for c in range(g[0] + 1, g[0] + g[1] + 1)) for g in several), groups


@pytest.mark.parametrize("name", WRAP_FIXTURES)
def test_wrap_fixture_has_a_gradient_beyond_int16_in_a_compressed_median_group(port, ref, manifest, name):
    """counted on the REFERENCE's coded planes (a decoder that takes the median of the int gradient loses the stream at the first such
    sample); the manifest entry records the count"""
    blob = fixture_blob(name)
    groups, _ = group_headers(blob, port)
    assert any(compress and predictor in (2, 7) for _, _, predictor, compress in groups), groups
    coded = ref.decode(blob, undo=False)
    n = 0
    for first, more, predictor, compress in groups:
        if compress and predictor in (2, 7):
            n += sum(edgecases.gradient_wraps(coded.channels[c]["data"], coded.channels[c]["zero"]) for c in range(first, first + more + 1))
    entry = next(e for e in manifest["fixtures"] if e["name"] == name)
    assert n > 0 and n == entry["gradient_wraps"]


def test_wrap_fixtures_through_the_oracle_alone(port, manifest):
    """the same count from the oracle's planes, for a machine without the reference"""
    for name in WRAP_FIXTURES:
        entry = next(e for e in manifest["fixtures"] if e["name"] == name)
        assert count_gradient_wraps(fixture_blob(name), port) == entry["gradient_wraps"] > 0, name


def _pictures():
    from fuif_amd.synth import photographic
    return [("rgb8_33x17", photographic(33, 17, 3, 8, seed=96), 255), ("quadrants14_24x40", edgecases.quadrants_14bit(24, 40), 16383)]


@pytest.mark.parametrize("squeeze", [0, 1])
@pytest.mark.parametrize("predictor", range(8))
def test_reference_encoder_with_every_predictor(port, ref, predictor, squeeze):
    """one predictor for every channel (oracle/ref_driver.cpp), Squeeze residuals included: oracle == reference before and after undo_transforms,
    and the picture comes back"""
    for name, img, maxval in _pictures():
        blob = ref.encode(img, maxval=maxval, squeeze=squeeze, predictor=predictor)
        a0, a1 = ref.decode_both(blob)
        b0, b1 = port.decode_both(blob)
        same(a0, b0)
        same(a1, b1)
        assert all(np.array_equal(a1.channels[c]["data"], img[c]) for c in range(img.shape[0])), name


def test_predicted_15bit_channel_through_the_writer_stays_compressed(gpulib, port):
    """the case of edgecases.CASES that tests/test_oracle_vs_ref.py and tests/test_gpu_int16_edges.py decode: its one group must be
    compressed with the median predictor and hold a gradient beyond int16, or those tests say nothing about the predictor"""
    case = next(c for c in edgecases.CASES if c["name"] == "predicted_blocks_15bit_70x45")
    blob = edgecases.build(case)
    groups, d = group_headers(blob, port)
    assert groups == [(0, 0, 2, 1)]
    assert edgecases.gradient_wraps(edgecases.blocks_15bit(70, 45)[0]) > 0


def _check_writer_bytes(mine, refblob):
    # the reference appends one stray byte (BlobIO::bytes_used = seek_pos+1, fileio.h:252-254)
    assert mine == refblob[: len(mine)] and len(refblob) - len(mine) <= 1, (len(mine), len(refblob))


def test_writer_on_a_gradient_beyond_int16_host_route(gpulib, port, ref):
    """the 14-bit quadrants: Co = R - B steps -16383, 9000, 16383 and the gradient at the centre is 41 766.  Fixed trees: the bytes the
    reference CLI writes.  Learned trees: the reference decodes the stream to the source."""
    img = edgecases.quadrants_14bit(24, 40)
    _check_writer_bytes(gpulib.encode_image(img, 14, tree_mode=0, squeeze=False), fixture_blob(CLI_QUADRANTS))
    for squeeze in (False, True):
        blob = gpulib.encode_image(img, 14, tree_mode=1, squeeze=squeeze)
        for dec in (ref, port):
            d = dec.decode(blob)
            assert d.ok and all(np.array_equal(d.channels[c]["data"], img[c]) for c in range(3)), squeeze


@pytest.mark.gpu
def test_writer_on_a_gradient_beyond_int16_gpu_routes(gpulib, port):
    """k_enc_model / k_enc_model_jobs / k_learn_samples_jobs all predict through enc_props_and_guess (csrc/maniac_encode.hip): the
    GPU entropy route, the GPU forward route and the device-resident route write the reference CLI's bytes with fixed trees, and with
    learned trees a stream that the oracle (and the reference, where it is built) decodes to the source"""
    from oracle_py import Ref
    from test_gpu_device_encoder import device_encode
    img = edgecases.quadrants_14bit(24, 40)
    want = fixture_blob(CLI_QUADRANTS)
    decoders = [port] + ([Ref()] if Ref.available() else [])
    for route, kw in (("gpu_entropy", dict(gpu_entropy=True)), ("gpu_forward", dict(gpu_forward=True)), ("both", dict(gpu_forward=True, gpu_entropy=True))):
        _check_writer_bytes(gpulib.encode_image(img, 14, tree_mode=0, squeeze=False, **kw), want)
        blob = gpulib.encode_image(img, 14, tree_mode=1, squeeze=False, **kw)
        for dec in decoders:
            d = dec.decode(blob)
            assert d.ok and all(np.array_equal(d.channels[c]["data"], img[c]) for c in range(3)), route
    _check_writer_bytes(gpulib.encode_images([img, img], 14, tree_mode=0, squeeze=False)[1], want)
    blobs, _ = device_encode(gpulib, [img, img], 14, tree_mode=0, squeeze=False)
    for b in blobs:
        _check_writer_bytes(b, want)
    blobs, _ = device_encode(gpulib, [img], 14, tree_mode=1, squeeze=False)
    for dec in decoders:
        d = dec.decode(blobs[0])
        assert d.ok and all(np.array_equal(d.channels[c]["data"], img[c]) for c in range(3))


@pytest.mark.gpu
def test_kernels_decode_every_new_fixture(gpulib, port):
    """the planner refuses no -P / -G stream (a refusal would raise here): every fixture plans, decodes with status 0 and gives the oracle's coded
    and output planes, per image and -- with a group index, where a resumed tile carries the predictor in its record -- per group"""
    for name in sorted(set(PREDICTOR_FIXTURES) | set(GROUP_FIXTURES) | set(WRAP_FIXTURES)):
        blob = fixture_blob(name)
        pre, post = port.decode_both(blob)
        indexed = gpulib.index_append(blob, port.decode(blob, undo=False).groups)
        for stream in (blob, indexed):
            plan = gpulib.Plan(stream)
            batch = gpulib.Batch(plan, 1, len(stream))
            try:
                batch.upload([stream])
                batch.decode()
                batch.sync()
                st, _ = batch.status()
                assert not st.any(), (name, st)
                coded = batch.coef_planes(0)
                batch.undo_transforms()
                batch.sync()
                out = batch.out_planes(0)
            finally:
                batch.close()
            for i, (g, e) in enumerate(zip(coded, pre.channels)):
                if e["size"] == e["w"] * e["h"]:
                    assert np.array_equal(np.asarray(g).reshape(e["h"], e["w"]), e["data"]), (name, "coded plane", i)
            assert len(out) == len(post.channels)
            for i, (g, e) in enumerate(zip(out, post.channels)):
                assert np.array_equal(np.asarray(g).reshape(e["data"].shape), e["data"]), (name, "output plane", i)
