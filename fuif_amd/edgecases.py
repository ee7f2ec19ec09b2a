"""Seeded hand-made FUIF streams at the edges of the reference's 16-bit sample type.

The reference keeps every sample in pixel_type = int16_t (image/image.h:35) and narrows whatever its inverse transforms compute when they
store it (squeeze.h:92-107,189-213; quantize.h:41,44-45; approximate.h:53-55; 2dmatch.h:129,155).  Streams a real encoder writes from pictures of at most 14 bits never reach
that edge, so the streams here are written directly in the transform domain: raw channels with explicit transform words through the
product's writer (fuifgpu_encode_channels, squeeze = 0 in the options unless a case says otherwise), the way fuif_amd/jpeglike.py
does.  The writer takes each channel's range from its data, so the ranges below are the coded ranges; every coded channel stays inside
what check_bit_depth (encoding.cpp:61-72) accepts: 15 bits of magnitude, maxval - minval <= 32767 where the predictor is not 0 (the
writer gives the first nb_channels channels predictor 2 and every other channel -- the residuals, the AC coefficients -- predictor 0).
Every stream is valid: the reference decodes it with `ok`, and its arithmetic on it is defined (int sums, modular narrowing).

CASES is the list the CPU test (oracle == real reference) and the GPU test (kernels == oracle == real reference) share; a case is a
pure function of its entry.  `wraps` says whether the case is meant to leave 16 bits.  The number beside each wrapping case is the
count of post-transform samples on which a decoder that keeps the inverse chain in int32 (this repository before the int16 stores were
matched) differed from the real reference, measured once on the CPU; each is at least 0.5 % of the case's samples.
"""
import ctypes as C

import numpy as np

from .jpeglike import DCT_CSHIFTS, ZIGZAG, _dct_matrix

TR_YCOCG, TR_DCT, TR_QUANTIZE, TR_SQUEEZE, TR_2DMATCH, TR_APPROXIMATE = 1, 4, 5, 7, 8, 10   # transform ids of the format (transform/transform.h)


class _RawChannel(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("hshift", C.c_int32), ("vshift", C.c_int32), ("hcshift", C.c_int32),
                ("vcshift", C.c_int32), ("component", C.c_int32), ("q", C.c_int32), ("data", C.c_void_p)]


def encode_channels(chans, w, h, nb_channels, bit_depth, words, squeeze=0):
    """chans: [dict(w, h, hshift, vshift, hcshift, vcshift, component, q, data=int array h x w)] -> .fuif bytes"""
    import fuif_amd
    L = fuif_amd.lib()
    keep = [np.ascontiguousarray(c["data"], dtype=np.int32).reshape(c["h"], c["w"]) for c in chans]
    for c, d in zip(chans, keep):
        if d.size:
            lo, hi = int(d.min()), int(d.max())
            assert max(abs(lo), abs(hi)) <= 32767, "coded channel outside 15 bits of magnitude"
            assert c.get("predictor0", False) or hi - lo <= 32767, "range of a predicted channel beyond check_bit_depth"
    arr = (_RawChannel * len(chans))(*[_RawChannel(c["w"], c["h"], c["hshift"], c["vshift"], c["hcshift"], c["vcshift"], c["component"], c.get("q", 1),
                                                   d.ctypes.data) for c, d in zip(chans, keep)])
    tw = np.array(words, np.int32)
    opt = fuif_amd.make_encode_options(0, int(squeeze), 12, 1, 4095, 0, int(fuif_amd.DEFAULT_SPLIT_BITS), 0, 0)
    out, n = C.c_void_p(), C.c_size_t(0)
    L.fuifgpu_encode_channels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.POINTER(fuif_amd.EncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    fuif_amd._check(L.fuifgpu_encode_channels(arr, len(chans), w, h, nb_channels, bit_depth, tw.ctypes.data, len(words), C.byref(opt), C.byref(out), C.byref(n)))
    blob = C.string_at(out.value, n.value)
    L.fuifgpu_free_blob(out)
    return blob


def _picture_channels(w, h, n):
    return [dict(w=w, h=h, hshift=0, vshift=0, hcshift=0, vcshift=0, component=c, q=1) for c in range(n)]


def squeeze_layout(chans, params, nb_channels):
    """the channel list after the Squeeze steps `params` (triples type, beginc, endc): geometry and shifts as the decoder derives
    them (squeeze.h:323-360); `base` marks a channel that is an average (not inserted as a residual by one of the steps)"""
    chans = [dict(c, base=True) for c in chans]
    for i in range(0, len(params), 3):
        horizontal, in_place = params[i] & 1, not (params[i] & 2)
        beginc, endc = params[i + 1], params[i + 2]
        offset = endc + 1 if in_place else nb_channels
        for c in range(beginc, endc + 1):
            a = chans[c]
            d = dict(hcshift=a["hcshift"], vcshift=a["vcshift"], component=a["component"], q=1, base=False)
            if horizontal:
                w = a["w"]
                a["w"] = (w + 1) // 2; a["hshift"] += 1; a["hcshift"] += 1
                d["w"], d["h"] = w - (w + 1) // 2, a["h"]
            else:
                h = a["h"]
                a["h"] = (h + 1) // 2; a["vshift"] += 1; a["vcshift"] += 1
                d["h"], d["w"] = h - (h + 1) // 2, a["w"]
            d["hshift"], d["vshift"] = a["hshift"], a["vshift"]
            chans.insert(offset + c - beginc, d)
    return chans


def _fill(rng, ch, lo, hi):
    """uniform over lo..hi, then every other sample (at random) redrawn from the outer eighths of the range: sums leave 16 bits where
    large averages meet large residuals, and uniform samples alone rarely do in a 14-bit case"""
    shape = (ch["h"], ch["w"])
    d = rng.integers(lo, hi + 1, shape, dtype=np.int32)
    eighth = max(1, (hi - lo) // 8)
    outer = np.where(rng.integers(0, 2, shape) == 1, hi - rng.integers(0, eighth + 1, shape), lo + rng.integers(0, eighth + 1, shape)).astype(np.int32)
    ch["data"] = np.where(rng.integers(0, 2, shape) == 1, outer, d)
    if ch["data"].size >= 2:                      # both ends of the range are present: the coded range is exactly lo..hi
        ch["data"].flat[0], ch["data"].flat[-1] = lo, hi


def squeeze_only(w, h, avg_max, res_max, seed):
    """one channel, three Squeeze levels h, v, h with explicit parameters; average 0..avg_max, residuals -res_max..res_max"""
    rng = np.random.default_rng(seed)
    params = [1, 0, 0, 0, 0, 0, 1, 0, 0]
    chans = squeeze_layout(_picture_channels(w, h, 1), params, 1)
    for c in chans:
        if c["base"]:
            _fill(rng, c, 0, avg_max)
        else:
            c["predictor0"] = True
            _fill(rng, c, -res_max, res_max)
    return encode_channels(chans, w, h, 1, 14, [TR_SQUEEZE, len(params)] + params)


def ycocg_squeeze(w, h, seed):
    """three channels, YCoCg, then the chroma planes squeezed horizontally and vertically the way the default parameters start
    (squeeze.h:277-280: not in place, residuals behind the picture's channels): the chain whose last two unsqueezes and colour
    transform the planner fuses into OP_HSQ2_YCOCG.  Chroma averages -16383..16383, chroma residuals -32767..32767."""
    rng = np.random.default_rng(seed)
    params = [3, 1, 2, 2, 1, 2]
    chans = squeeze_layout(_picture_channels(w, h, 3), params, 3)
    for i, c in enumerate(chans):
        if i == 0:
            _fill(rng, c, 0, 16383)
        elif c["base"]:
            _fill(rng, c, -16383, 16383)
        else:
            c["predictor0"] = True
            _fill(rng, c, -32767, 32767)
    return encode_channels(chans, w, h, 3, 14, [TR_YCOCG, 0, TR_SQUEEZE, len(params)] + params)


def quantize_only(w, h, q, amp, seed):
    """one channel of samples -amp..amp with quantisation constant q and the transform list [Quantize]"""
    rng = np.random.default_rng(seed)
    c = _picture_channels(w, h, 1)[0]
    c["q"] = q
    _fill(rng, c, -amp, amp)
    return encode_channels([c], w, h, 1, 14, [TR_QUANTIZE, 0])


def approximate(w, h, q, amp, rem, seed):
    """one channel of quotients -amp..amp with the transform list [Approximate(q)] and its remainder channel -rem..rem behind it
    (approximate.h:62-78): the inverse is quotient * q, stored, then + remainder, stored (:53-55)"""
    rng = np.random.default_rng(seed)
    c, r = _picture_channels(w, h, 1)[0], _picture_channels(w, h, 1)[0]
    _fill(rng, c, -amp, amp)
    r["predictor0"] = True
    _fill(rng, r, -rem, rem)
    return encode_channels([c, r], w, h, 1, 14, [TR_APPROXIMATE, 3, 0, 0, q - 1])


def soft_match(w, h, amp, seed, chain=False):
    """one channel -amp..amp behind a match meta-channel of free offsets 0..4 (0 = unmatched; 1..4 = the left, upper left, upper and
    upper right neighbour, 2dmatch.h:50-78) with the transform list [2DMatch(soft)]: a matched sample is its coded value + its source's
    final value, stored (2dmatch.h:129) -- chains of sums that leave 16 bits.  chain: every sample but the first is matched to its
    left neighbour (in linear order, so across the rows as well) and the coded values are -40..299 -- the planes of
    tests/test_gpu_transform_exports.py::test_inv_match_free_offsets_export at density 1.0: one chain through the whole plane, a running
    sum that passes 2^16 several times"""
    rng = np.random.default_rng(seed)
    m, c = _picture_channels(w, h, 1)[0], _picture_channels(w, h, 1)[0]
    m["data"] = rng.integers(0, 5, (h, w), dtype=np.int32)
    m["data"].flat[0], m["data"].flat[-1] = 0, 4
    c["predictor0"] = True
    if chain:
        m["data"][:] = 1
        m["data"].flat[0] = 0
        c["data"] = rng.integers(-40, 300, (h, w), dtype=np.int32)
    else:
        _fill(rng, c, -amp, amp)
    return encode_channels([m, c], w, h, 1, 14, [TR_2DMATCH, 4, 0, 0, 1, 1000000])


def idct_outputs(dc, ac, qdc, qac, maxval):
    """float64 outputs of the reference's inverse DCT (dct.h:281-289) for blocks whose dequantised coefficients are the int16 the
    reference stores: dc [bh, bw], ac [63, bh, bw] in channel order (zig-zag rank 1..63), q per channel"""
    K = _dct_matrix()
    nat_of_pos = np.argsort(ZIGZAG)
    bh, bw = dc.shape
    blocks = np.zeros((bh, bw, 64), np.float64)
    blocks[:, :, 0] = (dc.astype(np.int64) * qdc).astype(np.int16).astype(np.float64) + np.float32((maxval + 1.0) * 4.0)
    for k in range(1, 64):
        blocks[:, :, int(nat_of_pos[k])] = (ac[k - 1].astype(np.int64) * int(qac[k - 1])).astype(np.int16).astype(np.float64)
    return np.einsum("ux,abuv,vy->abxy", K, blocks.reshape(bh, bw, 8, 8), K)


def jpeg_like_wrapping(bw, bh, seed, bit_depth=10, squeeze=1):
    """the JPEG-transcode chain [DCT, Quantize] of a one-component picture (squeeze = 1: the writer adds the default Squeeze of the DC
    plane like the CLI, so the DC plane reaches the dequantisation as an int32 product of the unsqueeze chain; squeeze = 0: all 64
    planes reach it as untouched coded planes, the int16 form of k_dequant) whose coefficient * q leaves int16: DC samples -3000..3000 with q = 16, and in every block three AC coefficients of
    -2000..2000 on channels with q = 20..60.  The inverse DCT's own store, round(double) into pixel_type (dct.h:289), is undefined
    for a value outside int16, so the float64 outputs of every block -- computed from the int16 products the reference stores --
    are asserted to stay inside +-32000 (two-dimensional basis functions are at most 0.2405: three wrapped AC products and the DC
    term give at most 3 * 0.2405 * 32768 + (32767 + 4096) / 8 = 28 250)."""
    rng = np.random.default_rng(seed)
    maxval = (1 << bit_depth) - 1
    qdc, qac = 16, rng.integers(20, 61, 63)
    dc = rng.integers(-3000, 3001, (bh, bw), dtype=np.int32)
    ac = np.zeros((63, bh, bw), np.int32)
    for by in range(bh):
        for bx in range(bw):
            for k in rng.choice(63, 3, replace=False):
                ac[k, by, bx] = rng.integers(-2000, 2001)
    out = idct_outputs(dc, ac, qdc, qac, maxval)
    assert np.abs(out).max() <= 32000.0, "a block leaves the range in which the reference's iDCT store is defined"
    assert (np.abs(ac.astype(np.int64) * qac[:, None, None]) > 32767).any() and (np.abs(dc.astype(np.int64) * qdc) > 32767).any()
    chans = [dict(w=bw, h=bh, hshift=3, vshift=3, hcshift=int(DCT_CSHIFTS[0]), vcshift=int(DCT_CSHIFTS[0]), component=0, q=qdc, data=dc)]
    for k in range(1, 64):
        chans.append(dict(w=bw, h=bh, hshift=3, vshift=3, hcshift=int(DCT_CSHIFTS[k]), vcshift=int(DCT_CSHIFTS[k]), component=0, q=int(qac[k - 1]),
                          data=ac[k - 1], predictor0=True))
    return encode_channels(chans, bw * 8, bh * 8, 1, bit_depth, [TR_DCT, 0, TR_QUANTIZE, 0], squeeze=squeeze)


def blocks_15bit(w, h, seed=7701):
    """(1, h, w): 8x8 blocks, each one of {0, 1000, 20000, 30000, 32767} (seeded), and every fifth sample of the main diagonal large.
    At the corners where three different blocks meet, left + top - topleft leaves int16 with left != top: the median predictor's
    first argument, which the reference narrows to pixel_type (context_predict.h:160,165).  Flat blocks compress, so an encoder keeps
    the group compressed -- random 15-bit data is rolled back to the uncompressed form, which uses no predictor."""
    levels = np.array([0, 1000, 20000, 30000, 32767], np.int32)
    pick = np.random.default_rng(seed).integers(0, 5, ((h + 7) // 8, (w + 7) // 8))
    img = np.kron(levels[pick], np.ones((8, 8), np.int32))[:h, :w].copy()
    for i in range(0, min(w, h), 5):
        img[i, i] = 32767 - (i * 37) % 500
    return img[None].astype(np.int32)


def quadrants_15bit(w, h):
    """(1, h, w) gray: four flat quadrants 0 | 20000 over 30000 | 32767.  Squeeze keeps flat quadrants flat, so the averages that are left
    after every Squeeze step meet in the same corner: 30000 + 20000 - 0 = 50 000 in the one median-predicted channel, which stays compressed"""
    img = np.zeros((1, h, w), np.int32)
    img[0, : h // 2, w // 2:], img[0, h // 2:, : w // 2], img[0, h // 2:, w // 2:] = 20000, 30000, 32767
    return img


def quadrants_14bit(w, h):
    """(3, h, w) RGB: four flat quadrants whose Co plane (R - B, -16383..16383 after YCoCg) steps from -16383 to 9000 to 16383: at the
    centre left + top - topleft = 16383 + 9000 + 16383 = 41 766 on the Co plane of a picture of only 14 bits"""
    img = np.empty((3, h, w), np.int32)
    img[1] = 8000
    hy, hx = h // 2, w // 2
    for (ys, xs), (r, b) in zip(((slice(0, hy), slice(0, hx)), (slice(0, hy), slice(hx, w)), (slice(hy, h), slice(0, hx)), (slice(hy, h), slice(hx, w))),
                                ((0, 16383), (9000, 0), (16383, 0), (12000, 3000))):
        img[0][ys, xs], img[2][ys, xs] = r, b
    return img


def gradient_wraps(plane, zero=0):
    """samples of a coded plane at which left + top - topleft is outside int16 and left != top, with the neighbour rules of
    context_predict.h:126-128: where the median of the narrowed gradient is not the median of the int gradient"""
    p = np.asarray(plane, np.int64)
    left = np.concatenate([np.full((p.shape[0], 1), zero, np.int64), p[:, :-1]], axis=1)
    top = np.concatenate([np.full((1, p.shape[1]), zero, np.int64), p[:-1]], axis=0)
    topleft = np.concatenate([np.full((1, p.shape[1]), zero, np.int64), left[:-1]], axis=0)
    topleft[0] = left[0]          # y == 0: topleft = left
    topleft[1:, 0] = left[1:, 0]  # x == 0: topleft = left
    g = left + top - topleft
    return int((((g > 32767) | (g < -32768)) & (left != top)).sum())


# the golden fixtures (tests/golden/make_golden.py) whose manifest entry records `gradient_wraps`
WRAP_FIXTURES = ("grad16_gray15_48x64_nosqueeze", "grad16_gray15_quadrants_48x64", "grad16_rgb14_quadrants_24x40_nosqueeze",
                 "grad16_rgb14_quadrants_24x40_cli_I0")


def group_headers(blob, port):
    """([(first channel, channels - 1, predictor, compress)], the oracle's Decoded before undo_transforms): a channel group starts with
    the big-endian varint count << 4 | predictor << 1 | compress (encoding.cpp:77,266-268), at the positions the oracle's parse recorded
    (port: oracle_py.Port)"""
    d = port.decode(blob, undo=False)
    out = []
    for first, pos in d.groups:
        v = 0
        while True:
            b = blob[pos]
            pos += 1
            v = (v << 7) | (b & 127)
            if b < 128:
                break
        out.append((first, v >> 4, (v >> 1) & 7, v & 1))
    return out, d


def count_gradient_wraps(blob, port, coded=None):
    """gradient_wraps summed over the compressed groups with the median predictor (2, or 7 = the `default:` branch), on the coded planes
    of `coded` (a Decoded before undo_transforms, e.g. the real reference's; default: the oracle's own)"""
    groups, d = group_headers(blob, port)
    coded = coded or d
    n = 0
    for first, more, predictor, compress in groups:
        if compress and predictor in (2, 7):
            n += sum(gradient_wraps(coded.channels[c]["data"], coded.channels[c]["zero"]) for c in range(first, first + more + 1) if coded.channels[c]["size"])
    return n


def predicted_blocks(w, h):
    """one untransformed 15-bit channel of blocks_15bit through the writer, which gives a picture channel the median predictor: the
    group stays compressed, so the predictor really runs (tests/test_predictors_and_groups.py asserts the header's compress bit)"""
    c = _picture_channels(w, h, 1)[0]
    c["data"] = blocks_15bit(w, h)[0]
    return encode_channels([c], w, h, 1, 14, [])   # (the writer's headers stop at 14 bits; the coded range is the data's, 0..32767)


# `ycocg` / `dct`: the planner switches that apply to the case (FUIFGPU_FUSE_YCOCG; FUIFGPU_FUSE_DEQUANT).
# The comment beside a wrapping case = post-transform samples on which the int32 inverse chain (the oracle before the int16 stores were
# matched) differed from the real reference, of the case's post-transform samples.
CASES = [
    # three levels h, v, h; 40x24: k_inv_hsqueeze_rows and the tail loops of the vertical kernel
    dict(name="squeeze3_14bit_40x24", make=squeeze_only, args=dict(w=40, h=24, avg_max=16383, res_max=16383, seed=7101), wraps=True),        # 45 of 960 (4.7 %)
    dict(name="squeeze3_15bit_40x24", make=squeeze_only, args=dict(w=40, h=24, avg_max=32767, res_max=16383, seed=7102), wraps=True),        # 461 of 960 (48.0 %)
    # 262x140: k_inv_hsqueeze_tiles with three row tiles (the last of 12 rows), 131 residual columns (4 tiles of 32 pairs + a tail), 65 columns at
    # the third level (k_inv_hsqueeze_rows, one step + a tail), a vertical step of 70 row pairs (8 steps of VS_STEP + a tail)
    dict(name="squeeze3_14bit_262x140", make=squeeze_only, args=dict(w=262, h=140, avg_max=16383, res_max=16383, seed=7103), wraps=True),    # 1655 of 36 680 (4.5 %)
    dict(name="squeeze3_15bit_262x140", make=squeeze_only, args=dict(w=262, h=140, avg_max=32767, res_max=16383, seed=7104), wraps=True),    # 17 268 of 36 680 (47.1 %)
    # k_inv_hsq2_ycocg: 35 and 67 residual columns (2 and 4 tiles of 16 pairs + a tail of 3), 66 and 70 rows (two row tiles, the second of 2 and 6 rows)
    dict(name="ycocg_squeeze_70x66", make=ycocg_squeeze, args=dict(w=70, h=66, seed=7201), wraps=True, ycocg=True),                          # 6847 of 13 860 (49.4 %)
    dict(name="ycocg_squeeze_134x70", make=ycocg_squeeze, args=dict(w=134, h=70, seed=7202), wraps=True, ycocg=True),                        # 13 913 of 28 140 (49.4 %)
    dict(name="quantize_q9_5000_40x24", make=quantize_only, args=dict(w=40, h=24, q=9, amp=5000, seed=7301), wraps=True),                    # 604 of 960 (62.9 %)
    dict(name="quantize_q9_3640_40x24", make=quantize_only, args=dict(w=40, h=24, q=9, amp=3640, seed=7302), wraps=False),                   # 9 * 3640 = 32 760: the control, 0 of 960
    dict(name="approximate_q9_5000_40x24", make=approximate, args=dict(w=40, h=24, q=9, amp=5000, rem=16383, seed=7501), wraps=True),   # 403 of 960 (42.0 %)
    dict(name="soft_match_40x24", make=soft_match, args=dict(w=40, h=24, amp=16383, seed=7601), wraps=True),                                 # 168 of 960 (17.5 %)
    dict(name="soft_match_chain_33x50", make=soft_match, args=dict(w=33, h=50, amp=0, seed=7602, chain=True), wraps=True),                      # 1139 of 1650 (69.0 %)
    dict(name="jpeg_like_wrapping_12x10_blocks", make=jpeg_like_wrapping, args=dict(bw=12, bh=10, seed=7401), wraps=True, dct=True),         # 3972 of 7680 (51.7 %)
    dict(name="jpeg_like_wrapping_6x5_blocks_dc_coded", make=jpeg_like_wrapping, args=dict(bw=6, bh=5, seed=7402, squeeze=0), wraps=True, dct=True),  # 1236 of 1920 (64.4 %)
    # no transform at all: the narrowing is in the entropy stage, the median predictor's gradient (context_predict.h:160); 70x45 = one 64-pixel chunk + 6
    # (a decoder that takes the median of the int gradient loses the stream at the first such sample: every sample behind it differs)
    dict(name="predicted_blocks_15bit_70x45", make=predicted_blocks, args=dict(w=70, h=45), wraps=True),
]


def build(case):
    return case["make"](**case["args"])


# ---- streams whose every prefix is decoded (tests/test_gpu_prefixes.py on the kernels, tests/test_oracle_vs_ref.py on the oracle) ----------
# Small on purpose: a sweep decodes one prefix per byte.  `length` = the range the test asserts for a stream the product's writer makes from
# a seeded picture (the bytes follow the writer, the seed is fixed); golden files have the length the manifest records.
# The writer learns no MANIAC tree for a channel below 4096 pixels (writer.cpp, plan_learner), so at 40 x 30 tree_mode 1 and 0 write the same
# bytes, single-leaf trees throughout -- and a predictor-0 group with a single-leaf tree takes the kernel's "fast track" (leaf_symbol on every
# symbol), not the chunk-fast / fast_symbol_hw / leaf_symbol hand-overs.  Those run where a predictor-0 group has a tree: in the writer's
# 128 x 64 stream below (the smallest picture whose last Squeeze residual has 4096 pixels; its tree has over 100 nodes) and in the reference
# encoder's gray8_64x48 (3 nodes).  Both were checked once against a library whose window reload was edited away (188u -> 260u): it decodes
# the large channels of exactly these streams wrongly, and every other stream of the list as before.
def golden_stream(name):
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", name + ".fuif"), "rb") as f:
        return f.read()


def _written(w, h, channels, bits, sigma=None, **keywords):
    import fuif_amd
    from .synth import photographic
    keywords.setdefault("split_bits", 2)
    return fuif_amd.encode_image(photographic(w, h, channels, bits, sigma=sigma), bits, **keywords)


def rolled_back_picture(w=40, h=30, seed=5):
    """uniform noise in the even columns, a constant in the odd ones: the residuals of the first horizontal Squeeze steps are uniform over a
    power-of-two range, which MANIAC codes in more bits than the flat code of an "uncompressed" group, so the writer rolls the largest
    groups back (encoding.cpp:545-551) -- the shape `fuif -U` forces"""
    a = np.random.default_rng(seed).integers(0, 256, size=(3, h, w)).astype(np.int32)
    a[:, :, 1::2] = 128
    return a


def _rolled_back():
    import fuif_amd
    return fuif_amd.encode_image(rolled_back_picture(), 8, ycocg=False, tree_mode=1, split_bits=2)


def _jpeg420(w, h):
    from .jpeglike import encode_jpeg_like
    from .synth import photographic
    return encode_jpeg_like(photographic(w, h, 3, 8, seed=77, sigma=1.0), 90, True)


PREFIX_STREAMS = [
    # YCoCg + Squeeze, lossless, predictor 0 in every residual group, 22 groups
    dict(name="writer_trees_40x30", make=lambda: _written(40, 30, 3, 8, tree_mode=1), length=(2900, 3300)),
    dict(name="writer_notrees_40x30", make=lambda: _written(40, 30, 3, 8, tree_mode=0), length=(2900, 3300)),
    # learned trees from the product's writer in front of predictor-0 symbols: one channel, Squeeze, the 64 x 64 residual learns
    dict(name="writer_trees_128x64", make=lambda: _written(128, 64, 1, 8, tree_mode=1, sigma=0.3), length=(3300, 3700)),
    # groups of 300 and 600 pixels stored "uncompressed" between compressed ones
    dict(name="writer_rolled_back_40x30", make=_rolled_back, length=(3500, 3900)),
    # a non-zero predictor in every group (reference CLI, -P 7 -R 0): no fast path at all.  The smallest -P fixture with more than 9 pixels
    dict(name="rgb8_65x34_P7_nosqueeze", make=lambda: golden_stream("rgb8_65x34_P7_nosqueeze"), length=(5334, 5334)),
    # 14 bits without YCoCg: 31-chance leaves, the wide context format
    dict(name="writer_wide14_32x24", make=lambda: _written(32, 24, 4, 14, ycocg=False, tree_mode=1), length=(4600, 5200)),
    # more than 31 properties: kPropPitchWide, half chunks
    dict(name="writer_props24_40x30", make=lambda: _written(40, 30, 4, 8, max_properties=24, tree_mode=1), length=(3800, 4300)),
    # the DCT shape: 192 channels.  8 x 8 is the smallest picture the transcode-like writer takes (one pixel per channel, every group
    # "uncompressed": a group start and a rac_init every four bytes); 64 x 48 has compressed groups among them
    dict(name="jpeg420_8x8", make=lambda: _jpeg420(8, 8), length=(650, 800)),
    dict(name="jpeg420_64x48", make=lambda: _jpeg420(64, 48), length=(1800, 2200)),
    # written by the real reference, with its learned trees: Squeeze only, and YCoCg + Squeeze + Quantization + Approximate
    dict(name="gray8_64x48", make=lambda: golden_stream("gray8_64x48"), length=(2066, 2066)),
    dict(name="approx_quant_rgb8_40x30", make=lambda: golden_stream("approx_quant_rgb8_40x30"), length=(484, 484)),
    # YCoCg without Squeeze: three groups of one channel, the median predictor, each channel a property of the next (the bare form of
    # PREFIX_INDEXED_WAITING below)
    dict(name="writer_nosqueeze_40x30", make=lambda: _written(40, 30, 3, 8, squeeze=False, tree_mode=1), length=(2800, 3250)),
]
# the stream of the group-parallel sweep: the first one, written with the group index
PREFIX_INDEXED = dict(name="writer_trees_40x30_indexed", make=lambda: _written(40, 30, 3, 8, tree_mode=1, index=True), length=(2950, 3400))
# Its single-leaf predictor-0 groups take the kernel's fast track, which never looks at another channel's rows: its tiles never wait and
# are never suspended, and the fast symbol decoders do not run in them.  Two more streams with the index:
# * the 128 x 64 stream: the fast symbol decoders and their hand-overs inside tiles.  Its tiles look at the rows of the channels they refer
#   to, but every such channel is half the size of the tile's own and started no later: it stays ahead, and no suspension was ever counted;
# * the 40 x 30 picture without Squeeze: three tiles of one channel each, all of one size, channel k a property of channel k + 1, so a
#   tile runs into the rows its neighbour has not finished, and is suspended and resumed (the position travels in the tile record).  How
#   often depends on which wavefront gets there first: 7 to 20 suspensions per sweep were counted on the emulator with four wavefronts
PREFIX_INDEXED_TREES = dict(name="writer_trees_128x64_indexed", make=lambda: _written(128, 64, 1, 8, tree_mode=1, sigma=0.3, index=True), length=(3330, 3760))
PREFIX_INDEXED_WAITING = dict(name="writer_nosqueeze_40x30_indexed", make=lambda: _written(40, 30, 3, 8, squeeze=False, tree_mode=1, index=True), length=(2820, 3290))
# (indexed stream, the same stream without the trailer)
PREFIX_SIDE_INDEX = [(PREFIX_INDEXED, PREFIX_STREAMS[0]), (PREFIX_INDEXED_TREES, PREFIX_STREAMS[2]), (PREFIX_INDEXED_WAITING, PREFIX_STREAMS[-1])]
assert PREFIX_STREAMS[2]["name"] == "writer_trees_128x64" and PREFIX_STREAMS[-1]["name"] == "writer_nosqueeze_40x30"
# (golden fixture, preview): the preview's byte limit lies inside the stream.  approx_quant_rgb8_40x30 is the smallest fixture whose previews the
# manifest lists; only its preview 0 has a limit of its own (byte 75).  pal_rgb_graphic_120x90 (Palette + Squeeze, 2438 bytes) has limits at
# 271, 515 and 1171 for previews 2, 3 and 4.  rgb8_97x61 has 11 322 bytes: too many for a sweep of every byte
PREFIX_PREVIEWS = [("approx_quant_rgb8_40x30", 0), ("pal_rgb_graphic_120x90", 3)]

# (stream name, prefix length, reason): prefixes the real reference itself fails on, left out of both tests.  None: it decodes them all
PREFIX_REFERENCE_FAILS = []

_prefix_blobs = {}


def prefix_stream(entry):
    """the bytes of one PREFIX_STREAMS entry (made once per process), its length inside the entry's range"""
    name = entry["name"]
    if name not in _prefix_blobs:
        blob = entry["make"]()
        lo, hi = entry["length"]
        assert lo <= len(blob) <= hi, (name, len(blob))
        _prefix_blobs[name] = blob
    return _prefix_blobs[name]


def first_planned_length(blob, limit=64):
    """the shortest prefix fuif_amd.Plan accepts (found by trying)"""
    import fuif_amd
    for n in range(1, limit + 1):
        try:
            fuif_amd.Plan(blob[:n])
            return n
        except fuif_amd.FuifGpuError:
            pass
    raise AssertionError("no prefix of up to %d bytes makes a plan" % limit)


def side_indexed(blob, groups, n):
    """blob[:n] with a group index of the groups that start inside it behind the cut (n beyond the first group's start).  To the reference,
    which knows no trailer, those bytes are stream data for the group that contains the cut; to the product the stream ends at the cut"""
    import fuif_amd
    return fuif_amd.index_append(blob[:n], [g for g in groups if g[1] < n])
