#!/usr/bin/env python3
"""Generate tests/golden/animation/: what the REAL reference CLI writes for `fuif frame-%02d.ppm out.fuif` (run on the build machine only).

  inputs  : fuif_amd.synth.filmstrip recipes (a static background, a moving sprite, a share of per-frame noise, exact runs placed by
            `edits`) written as frame-00, frame-01, ... PNM / PAM files
  encoder : the unmodified reference CLI oracle/_ref/fuif with `-I 0` (single-leaf trees: the mode in which the product's writer is
            byte-identical) and otherwise the flags of the row -- by default none, so -K 256 -X 70 -Y 70 -M -1 -F 10 are in force
  recorded: animation/manifest_animation.json -- the recipe, the CLI flags, the keywords of fuif_amd.encode_animation that mean the same,
            the transform list, every coded channel's geometry, range and q as the reference's own decoder reports them and, for the
            rows without Squeeze (-R 0), the number of non-zero samples of the match channel and of samples the match set to zero

The numbers of the -R 0 rows come from a numpy statement of the rule (match_rule below) that is first checked, sample by sample, against
the reference's own match channel and coded channels; the conditions the test suite relies on are asserted at the end.
Nothing here is reference source; the .fuif files and the manifest are data.
Re-run: python tests/golden/make_golden_animation.py   (does not touch the other generators' files or manifests)
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "animation")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fuif_amd.synth import from_recipe, write_pnm  # noqa: E402
from oracle_py import Ref, ref_cli, run_ref_cli  # noqa: E402

DEFAULTS = dict(palette_colors=256, compact_post=70, compact_pre=70)   # what the CLI does when no -K / -X / -Y is given


def strip(w, h, frames, c, seed, **kw):
    return dict(kind="filmstrip", w=w, h=h, frames=frames, channels=c, bits=8, seed=seed, **kw)


RGB = strip(48, 8, 3, 3, 11)
# row 1 of frame 1: everything changes but [10, 49) and [100, 140): runs of 39 (one short) and 40
GRAY2100 = strip(2100, 4, 2, 1, 17, noise=0.0, edits=[[1, 1, 2, 0, 2100, 1], [1, 1, 2, 10, 49, 0], [1, 1, 2, 100, 140, 0]])
# name, recipe, further CLI flags, the same as keywords of encode_animation
SPECS = [
    ("rgb_48x8x3_defaults", RGB, [], dict(DEFAULTS)),
    ("rgb_48x8x3_K0X0Y0", RGB, ["-K", "0", "-X", "0", "-Y", "0"], dict()),
    ("rgb_48x8x3_R0", RGB, ["-R", "0"], dict(DEFAULTS, squeeze=False)),
    ("rgb_48x8x3_M0", RGB, ["-M", "0"], dict(DEFAULTS, match_previous=False)),
    ("rgb_48x8x3_F25", RGB, ["-F", "25"], dict(DEFAULTS, framerate=25)),
    ("rgb_48x8x3_Q80", RGB, ["-Q", "80"], dict(DEFAULTS, quality=80)),
    ("graphic_48x7x4_palette", strip(48, 7, 4, 3, 12, background="graphic", colors=9, noise=0.0, speckles=2), [], dict(DEFAULTS)),
    ("gray_300x7x2", strip(300, 7, 2, 1, 13, speckles=3), [], dict(DEFAULTS)),
    ("rgba_48x7x2", strip(48, 7, 2, 4, 14), [], dict(DEFAULTS)),
    ("rgb_300x8x2_R0", strip(300, 8, 2, 3, 15, noise=0.1, speckles=4), ["-R", "0"], dict(DEFAULTS, squeeze=False)),
    ("gray_2100x4x2_R0", GRAY2100, ["-R", "0"], dict(DEFAULTS, squeeze=False)),
]


def match_rule(planes, fh):
    """(match channel, mask of the samples that are set to zero) of a (C, H, W) strip of frames fh rows high: transform/2dmatch.h:303-381
    with maxdist = -1, the three in-place erode sweeps written as three data-parallel steps"""
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
        gone = ~m | flagged                      # below and to the right: never matched, or flagged by an earlier sweep
        near = np.zeros_like(m)
        near[1:] |= ~m[:-1]                      # above and to the left: never matched (the picture's edges do not count)
        near[:, 1:] |= ~m[:, :-1]
        near[:-1] |= gone[1:]
        near[:, :-1] |= gone[:, 1:]
        flagged = flagged | (m & near)
    return m.astype(np.int32), m & ~flagged


def fwd_ycocg(p):
    r, g, b = p[0], p[1], p[2]
    out = p.copy()
    out[0], out[1], out[2] = (((r + b) >> 1) + g) >> 1, r - b, g - ((r + b) >> 1)
    return out


def main():
    if ref_cli() is None or not Ref.available():
        sys.exit("oracle/_ref is not built (make -C oracle ref cli)")
    os.makedirs(OUT, exist_ok=True)
    ref = Ref()
    fixtures = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, recipe, extra, kwargs in SPECS:
            frames = from_recipe(recipe)
            nf, c, fh, w = frames.shape
            ext = ".pam" if c in (2, 4) else ".ppm" if c == 3 else ".pgm"
            os.makedirs(os.path.join(tmp, name))
            for f in range(nf):
                write_pnm(os.path.join(tmp, name, "frame-%02d%s" % (f, ext)), frames[f], 255)
            dst = os.path.join(OUT, name + ".fuif")
            flags = ["-I", "0"] + extra
            r = run_ref_cli(flags + [os.path.join(tmp, name, "frame-%02d" + ext), dst])
            if r.returncode != 0:
                sys.exit("%s: the reference CLI failed\n%s" % (name, r.stderr))
            blob = open(dst, "rb").read()
            again = dst + ".again"
            run_ref_cli(flags + [os.path.join(tmp, name, "frame-%02d" + ext), again])
            assert open(again, "rb").read() == blob, name + ": the reference CLI is not deterministic here"
            os.remove(again)
            dec = ref.decode(blob, undo=False)
            back = ref.decode(blob)
            assert dec.ok and back.ok, name
            source = np.concatenate(list(frames), axis=1)   # (C, F*H, W): the strip
            if "quality" not in kwargs:
                assert all(np.array_equal(back.channels[k]["data"], source[k]) for k in range(c)), name
            channels = [dict(w=ch["w"], h=ch["h"], hshift=ch["hshift"], vshift=ch["vshift"], minval=ch["minval"], maxval=ch["maxval"], q=ch["q"])
                        for ch in dec.channels]
            entry = dict(name=name, file=name + ".fuif", nbytes=len(blob), input=recipe, frames=nf, frame_h=fh, flags=flags, encode=kwargs,
                         lossless="quality" not in kwargs, transforms=[[t[0]] + list(t[1]) for t in dec.transforms],
                         nb_coded_channels=len(dec.channels), channels=channels)
            if "-R" in extra:
                # the chain in front of the match: YCoCg, then the CLI's default channel compaction (a photograph's Co and Cg use less than
                # 70 % of their range): a compacted channel holds the ranks of its values, its palette is one more meta-channel
                transformed = fwd_ycocg(source) if c >= 3 else source.copy()
                compacted = [t for t in entry["transforms"] if t[0] == 6]
                assert [t[0] for t in entry["transforms"]] == ([1] if c >= 3 else []) + [6] * len(compacted) + [8], (name, entry["transforms"])
                for t in compacted:
                    assert t[1] == t[2], name
                    transformed[t[1]] = np.unique(transformed[t[1]], return_inverse=True)[1].reshape(transformed[t[1]].shape)
                m, zeroed = match_rule(transformed, fh)
                assert np.array_equal(np.asarray(dec.channels[0]["data"]).reshape(m.shape), m), name + ": the rule and the reference's match channel differ"
                expect = transformed.copy()
                expect[:, zeroed] = 0
                for k in range(c):
                    assert np.array_equal(np.asarray(dec.channels[1 + len(compacted) + k]["data"]).reshape(m.shape), expect[k]), (name, k)
                runs = np.flatnonzero(np.diff(np.concatenate((np.zeros((m.shape[0], 1), np.int32), m, np.zeros((m.shape[0], 1), np.int32)), axis=1).ravel()))
                entry.update(match_nonzero=int(m.sum()), match_zeroed=int(zeroed.sum()), a_run_crosses_sample_64=bool((m[:, 63] & m[:, 64]).any()) if w > 64 else False,
                             run_lengths=sorted(set(int(b - a) for a, b in zip(runs[::2], runs[1::2]))))
            fixtures.append(entry)
            print("%-28s %6d bytes, %2d channels, transforms %s %s" % (name, len(blob), len(dec.channels), entry["transforms"],
                                                                       {k: entry[k] for k in ("match_nonzero", "match_zeroed") if k in entry}))
    r0 = [e for e in fixtures if "match_zeroed" in e]
    for width in (48, 300, 2100):
        assert any(e["input"]["w"] == width and e["match_zeroed"] > 0 for e in r0), "no -R 0 fixture of width %d has a sample set to zero" % width
    assert any(e["a_run_crosses_sample_64"] for e in r0)
    assert all(e["nbytes"] <= 16384 for e in fixtures)
    with open(os.path.join(OUT, "manifest_animation.json"), "w") as f:
        json.dump(dict(fixtures=fixtures), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
