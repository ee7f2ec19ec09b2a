"""GPU parity (-m gpu): every prefix of a stream decodes like the oracle decodes the same bytes.

The entropy kernel chooses per chunk and per symbol, from the bytes that are left, between the hand-written decoders (which have no
end-of-stream case) and leaf_symbol / s_getc (which has).  A whole stream leaves the fast paths in its last few hundred bytes only, so the
suite's handful of fractional cuts exercises each hand-over once; here the cut moves through a small stream byte by byte.  All prefixes of
one stream share a plan, so a sweep is ONE batch and one launch: image k of the batch is blob[:n0 + k].

Per prefix: status, bytes consumed, coded planes, channel ranges and output planes against the oracle on the same bytes
(tests/test_oracle_vs_ref.py pins the oracle to the real reference on the same prefixes), and the same results again with the images of
the batch in reversed order -- a read past a prefix's end would show as a dependence on the neighbour in the blob slab.

FUIF_TEST_PREFIX_STRIDE (set by tests/test_emulated_kernels.py only): the step between two cuts on the wavefront emulator, where a decode
takes milliseconds instead of microseconds.  On the GPU it is one byte."""
import os

import numpy as np
import pytest

from fuif_amd import edgecases

pytestmark = pytest.mark.gpu

STRIDE = max(1, int(os.environ.get("FUIF_TEST_PREFIX_STRIDE", "1")))
ST_TRUNCATED = 1   # FUIFGPU_ST_TRUNCATED (include/fuifgpu.h)
_oracle_cache = {}


def _cut_lengths(blob, name=None):
    n0 = edgecases.first_planned_length(blob)
    assert n0 < 64
    left_out = {n for stream, n, reason in edgecases.PREFIX_REFERENCE_FAILS if stream == name}   # (where the real reference itself fails: none)
    ns = [n for n in range(n0, len(blob) + 1, STRIDE) if n not in left_out]
    if ns[-1] != len(blob):
        ns.append(len(blob))      # the whole stream is always the last image
    return ns


def _oracle(port, name, blob, ns, preview=-1):
    """{n: (coded Decoded, output Decoded, bytes consumed)} of the oracle, computed once per stream and preview and shared"""
    key = (name, preview)
    have = _oracle_cache.setdefault(key, {})
    for n in ns:
        if n not in have:
            cut = blob[:n]
            pre, post = port.decode_both(cut, preview=preview, io_kind=0)
            have[n] = (pre, post, port.decode(cut, preview=preview, undo=False, want_data=False).stats["bytes"])
    return have


def _decode(batch, cuts, preview=-1):
    batch.upload(cuts, preview)
    batch.decode()
    batch.sync()
    st, used = batch.status()
    pre = [batch.coef_planes(i) for i in range(len(cuts))]
    meta = [batch.channel_meta(i) for i in range(len(cuts))]
    batch.undo_transforms()
    batch.sync()
    post = [batch.out_planes(i) for i in range(len(cuts))]
    return [dict(st=int(st[i]), used=int(used[i]), pre=pre[i], meta=meta[i], post=post[i]) for i in range(len(cuts))]


def _same_result(a, b):
    return (a["st"] == b["st"] and a["used"] == b["used"] and np.array_equal(a["meta"], b["meta"]) and
            all(np.array_equal(x, y) for x, y in zip(a["pre"], b["pre"])) and all(np.array_equal(x, y) for x, y in zip(a["post"], b["post"])))


def _against_oracle(n, got, want, untouched):
    """what differs between the kernels' decode of one prefix and the oracle's, as a list of words; (pairs, skipped) counts the channels.
    untouched: the oracle's channels for the shortest prefix, where no group has been read.  The oracle has no "decoded" mark, so a channel
    counts as decoded by it when its range or q is no longer what it was there -- or when the kernels say that they decoded it."""
    pre, post, used = want
    bad, skipped = [], 0
    if got["st"] & ~ST_TRUNCATED:
        bad.append("status %d" % got["st"])
    if pre.status != 1 or post.status != 1:
        bad.append("oracle refuses")
    if got["used"] != used:
        bad.append("bytes consumed %d, oracle %d" % (got["used"], used))
    assert len(got["pre"]) == len(pre.channels)
    for i, (g, ch) in enumerate(zip(got["pre"], pre.channels)):
        if ch["size"] == 0:
            ok = not g.any()              # undecoded channel reads as zeros
        elif ch["size"] != ch["w"] * ch["h"]:
            skipped += 1                  # constructor-sized plane the stream never reached
            continue
        else:
            ok = g.shape == ch["data"].shape and np.array_equal(g, ch["data"])
        if not ok:
            bad.append("coded channel %d" % i)
    for i, (ch, was) in enumerate(zip(pre.channels, untouched.channels)):
        ranges = (ch["minval"], ch["maxval"], ch["q"])
        if (ranges != (was["minval"], was["maxval"], was["q"]) or got["meta"][i][3]) and tuple(int(v) for v in got["meta"][i][:3]) != ranges:
            bad.append("meta of channel %d" % i)
    if len(got["post"]) != len(post.channels):
        bad.append("%d output planes, oracle %d" % (len(got["post"]), len(post.channels)))
    for i, (g, ch) in enumerate(zip(got["post"], post.channels)):
        if g.shape != np.shape(ch["data"]) or not np.array_equal(g, ch["data"]):
            bad.append("output channel %d" % i)
    return bad, len(pre.channels), skipped


def _report(name, failures):
    assert not failures, "%s: %d failing prefixes, the first: %s" % (name, len(failures), failures[:10])


def _sweep(gpulib, port, name, blob, preview=-1):
    ns = _cut_lengths(blob, name)
    cuts = [blob[:n] for n in ns]
    want = _oracle(port, name, blob, ns, preview)
    batch = gpulib.Batch(gpulib.Plan(blob), len(cuts), sum(ns))
    try:
        forward = _decode(batch, cuts, preview)
        backward = _decode(batch, cuts[::-1], preview)[::-1]
    finally:
        batch.close()
    failures, pairs, skipped, truncated = [], 0, 0, 0
    full = forward[-1]
    for n, got, again in zip(ns, forward, backward):
        bad, p, s = _against_oracle(n, got, want[n], want[ns[0]][0])
        pairs += p
        skipped += s
        truncated += got["st"] & ST_TRUNCATED
        if n == len(blob) and preview < 0 and got["st"] != 0:      # (a preview that stops at its byte limit is marked like a cut stream)
            bad.append("the whole stream has status %d" % got["st"])
        if not (got["st"] & ST_TRUNCATED) and not all(np.array_equal(x, y) for x, y in zip(got["pre"], full["pre"])):
            bad.append("differs from the whole stream without the truncated bit")
        if not _same_result(got, again):
            bad.append("depends on its neighbours in the batch")
        if bad:
            failures.append((n, bad))
    print("%s%s: %d bytes, %d prefixes from %d, %d with the truncated bit, %d of %d (prefix, channel) pairs constructor-sized (%.2f %%)" % (
        name, "" if preview < 0 else " preview %d" % preview, len(blob), len(ns), ns[0], truncated, skipped, pairs, 100.0 * skipped / pairs))
    assert 4 * skipped <= pairs, (name, skipped, pairs)
    _report(name, failures)


@pytest.mark.parametrize("entry", edgecases.PREFIX_STREAMS, ids=lambda e: e["name"])
def test_every_prefix_decodes_like_the_oracle(gpulib, port, entry):
    _sweep(gpulib, port, entry["name"], edgecases.prefix_stream(entry))


def test_the_streams_are_what_their_sweeps_are_for(gpulib, port):
    """the properties the list in fuif_amd/edgecases.py claims, read from the streams: compressed predictor-0 groups of more than two chunks,
    trees in front of them where the fast symbol decoders are meant to run, rolled-back groups of 300 and more pixels between compressed
    ones, a non-zero predictor in every group of the -P stream, 14 bits, 192 groups in the DCT shape"""
    by = {e["name"]: edgecases.prefix_stream(e) for e in edgecases.PREFIX_STREAMS}

    def groups(name):
        heads, d = edgecases.group_headers(by[name], port)
        return [(first, predictor, compress, d.channels[first]["w"] * d.channels[first]["h"]) for first, more, predictor, compress in heads], d

    for name in ("writer_trees_40x30", "writer_trees_128x64", "writer_wide14_32x24", "writer_props24_40x30", "gray8_64x48"):
        g, d = groups(name)
        assert sum(1 for first, predictor, compress, pixels in g if predictor == 0 and compress and pixels >= 128) >= 3, name
    # no channel of 40 x 30 has the 4096 pixels from which the writer learns a tree: one stream under two names, cut at different places
    # where a stride applies (tests/test_emulated_kernels.py)
    assert by["writer_trees_40x30"] == by["writer_notrees_40x30"] and groups("writer_trees_40x30")[1].stats["max_tree_nodes"] == 1
    g, d = groups("writer_trees_128x64")
    assert d.stats["max_tree_nodes"] >= 51 and (g[-1][1], g[-1][2], g[-1][3]) == (0, 1, 4096)
    assert groups("gray8_64x48")[1].stats["max_tree_nodes"] > 1
    g, d = groups("writer_rolled_back_40x30")
    assert sum(1 for first, predictor, compress, pixels in g if not compress and pixels >= 300) >= 3
    assert sum(1 for first, predictor, compress, pixels in g if compress and pixels >= 300) >= 3
    g, d = groups("rgb8_65x34_P7_nosqueeze")
    assert all(predictor != 0 and compress for first, predictor, compress, pixels in g) and d.stats["max_tree_nodes"] > 1
    g, d = groups("writer_nosqueeze_40x30")
    assert [(first, compress, pixels) for first, predictor, compress, pixels in g] == [(k, 1, 1200) for k in range(3)] and all(p != 0 for first, p, c, n in g)
    assert gpulib.Plan(by["writer_wide14_32x24"]).info.maxval == 16383
    assert len(groups("jpeg420_8x8")[0]) == len(groups("jpeg420_64x48")[0]) == 192
    assert any(compress for first, predictor, compress, pixels in groups("jpeg420_64x48")[0])


def _without_trailer(gpulib, pair):
    """the stream in front of its group index, and the index: the writer's trailer is the one index_append puts behind the bare stream"""
    indexed, bare = edgecases.prefix_stream(pair[0]), edgecases.prefix_stream(pair[1])
    groups = gpulib.index_parse(indexed)
    assert len(groups) >= 3
    assert indexed[: len(bare)] == bare and gpulib.index_append(bare, groups) == indexed
    return bare, groups


_side_index_cache = {}


def _side_index_decodes(gpulib, monkeypatch, pair, ctx_kb):
    """every prefix of one stream three times (computed once per stream and arena setting, shared by the tests below): the bare prefix
    sequentially, the prefix + the side index of the groups that start inside it group-parallel, and those same bytes sequentially.
    `suspensions`: how often a tile of the group-parallel launch was suspended, where the library counts that (-DFUIF_STATS builds,
    fuifgpu_batch_sched_stats; the release build carries no statistics: None)"""
    if ctx_kb is not None:
        monkeypatch.setenv("FUIFGPU_CTX_KB", ctx_kb)
    key = (pair[0]["name"], ctx_kb)
    if key not in _side_index_cache:
        blob, groups = _without_trailer(gpulib, pair)
        ns = [n for n in _cut_lengths(blob) if n > groups[0][1]]    # (a prefix that ends at the first group's start has no group to index)
        plan = gpulib.Plan(blob)
        cuts = [blob[:n] for n in ns]
        parts = [[g for g in groups if g[1] < n] for n in ns]
        side = [edgecases.side_indexed(blob, groups, n) for n in ns]
        assert all(gpulib.index_parse(s) == p for s, p in zip(side, parts))
        runs, suspensions = [], None
        for streams, parallel in ((cuts, False), (side, True), (side, False)):
            batch = gpulib.Batch(plan, len(streams), sum(len(s) for s in streams))
            try:
                batch.set_group_parallel(parallel)
                runs.append(_decode(batch, streams))
                if parallel:
                    try:
                        suspensions = int(batch.sched_stats()[2])
                    except gpulib.FuifGpuError:
                        pass
            finally:
                batch.close()
        _side_index_cache[key] = dict(blob=blob, ns=ns, parts=parts, side=side, bare=runs[0], par=runs[1], same_bytes=runs[2], suspensions=suspensions)
    return _side_index_cache[key]


ARENAS = pytest.mark.parametrize("ctx_kb", [None, "0"], ids=["arenas", "pinned"])
SIDE_INDEX = pytest.mark.parametrize("pair", edgecases.PREFIX_SIDE_INDEX, ids=lambda p: p[0]["name"])


@SIDE_INDEX
@ARENAS
def test_every_prefix_group_parallel_equals_sequential(gpulib, port, monkeypatch, pair, ctx_kb):
    """the same prefixes with a side index of the groups that start inside them, one wavefront per group, against the sequential decode
    of the bare prefix.  FUIFGPU_CTX_KB=0: no context arena, a suspendable tile is pinned to its wavefront.

    Three streams (fuif_amd/edgecases.py).  writer_trees_40x30_indexed has 22 groups, so many group starts lie near a cut; its groups have
    single-leaf trees and take the kernel's fast track, which never looks at the rows of other channels: its tiles never wait and are never
    suspended.  writer_trees_128x64_indexed runs the fast symbol decoders and their hand-overs inside tiles.  writer_nosqueeze_40x30_indexed
    is the one whose tiles are suspended and resumed, so that the coder state and the position come back from the tile record (rec->pos;
    rec->flags bit 8, the end-of-stream flag, is 0 in every record a tile can write: a tile yields at the start of a row, behind the test
    that ends the channel once the flag is set).  Whether a tile is suspended depends on which wavefront runs first: where the library
    counts suspensions (-DFUIF_STATS; the emulator run of tests/test_emulated_kernels.py, four wavefronts at once) the count of that stream
    must not be 0; the release build on the GPU has no counter, and there this sweep shows the results only.

    A valid trailer stands behind the stream and the stream ends where it begins (capi.hip, stage_streams), so the group that contains the
    cut meets the end of the stream at the cut, with or without the index: the two decodes agree in EVERYTHING -- every coded plane (those
    in front of the group that contains the cut, which the issue of this sweep asks for, and the ones behind it), ranges, output planes,
    status and bytes consumed -- and so does the sequential decode of the bytes with the trailer, and all three equal the oracle on the
    bare prefix.  (Until the stream ended there, the cut group went on into the trailer's bytes: 427 of the 3076 prefixes of the 40 x 30
    stream came out FUIFGPU_ST_CORRUPT, a channel range beyond the picture or an invalid tree spelled by the index.)"""
    r = _side_index_decodes(gpulib, monkeypatch, pair, ctx_kb)
    name, blob, ns = pair[0]["name"], r["blob"], r["ns"]
    want = _oracle(port, pair[1]["name"], blob, ns + [edgecases.first_planned_length(blob)])
    untouched = want[edgecases.first_planned_length(blob)][0]
    failures, compared = [], 0
    for n, part, a, b, c in zip(ns, r["parts"], r["bare"], r["par"], r["same_bytes"]):
        bad = []
        first_cut_channel = part[-1][0] if n < len(blob) else len(a["pre"])
        for i in range(first_cut_channel):
            compared += 1
            if not np.array_equal(a["pre"][i], b["pre"][i]):
                bad.append("coded channel %d in front of the cut" % i)
        if n == len(blob) and b["st"] != 0:
            bad.append("the whole stream has status %d" % b["st"])
        if not _same_result(a, b):
            bad.append("group-parallel with the index differs from the bare prefix")
        if not _same_result(b, c):
            bad.append("group-parallel and sequential differ on the same bytes")
        bad += _against_oracle(n, b, want[n], untouched)[0]
        if bad:
            failures.append((n, bad))
    print("%s: %d bytes, %d prefixes, %d coded planes in front of the cut, suspensions: %s" % (
        name, len(blob), len(ns), compared, "not counted by this build" if r["suspensions"] is None else r["suspensions"]))
    assert 4 * compared > len(r["bare"][0]["pre"]) * len(ns)
    _report(name, failures)
    if r["suspensions"] is not None and pair[0] is edgecases.PREFIX_INDEXED_WAITING and len(ns) >= 16:
        assert r["suspensions"] > 0, "no tile of %s was suspended" % name


@SIDE_INDEX
@ARENAS
def test_no_status_bit_but_truncated_with_a_side_index(gpulib, monkeypatch, pair, ctx_kb):
    """no status bit other than TRUNCATED on either side of the sweep above: not on the sequential decode of a bare prefix, not on the
    group-parallel decode of the prefix with its side index"""
    r = _side_index_decodes(gpulib, monkeypatch, pair, ctx_kb)
    failures = []
    for n, a, b in zip(r["ns"], r["bare"], r["par"]):
        bad = ["sequential status %d" % a["st"]] if a["st"] & ~ST_TRUNCATED else []
        if b["st"] & ~ST_TRUNCATED:
            bad.append("group-parallel status %d" % b["st"])
        if bad:
            failures.append((n, bad))
    _report(pair[0]["name"], failures)


@pytest.mark.parametrize("name,preview", edgecases.PREFIX_PREVIEWS)
def test_every_prefix_of_a_preview(gpulib, port, name, preview):
    """a preview's byte limit and the end of the stream compete in s_limit_hit (the two streams: fuif_amd/edgecases.py, PREFIX_PREVIEWS);
    every byte, no stride: the decode stops at the limit, so the sweeps are short"""
    blob = edgecases.golden_stream(name)
    limit = port.decode(blob, preview=preview, undo=False, want_data=False).stats["bytes"]
    assert 64 < limit < len(blob) // 2
    _sweep(gpulib, port, name, blob, preview)
