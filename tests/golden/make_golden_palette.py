#!/usr/bin/env python3
"""Generate tests/golden/palette/: streams of the REAL reference CLI for input it does not treat as a photograph (run on the build machine only).

  inputs  : fuif_amd.synth.from_recipe pictures (seeded graphics, photographs with sparse histograms, flat pictures, colour + alpha)
            written as PNM / PAM
  encoder : the unmodified reference CLI oracle/_ref/fuif with `-I 0` (single-leaf trees: the mode in which the product's writer is
            byte-identical) and otherwise the flags of the row -- by default none, so -K 256 -X 70 -Y 70 are in force
  recorded: palette/manifest_palette.json -- the recipe, the CLI flags, the keywords of fuif_amd.encode_image that mean the same, the
            transform list with its parameters, and every coded channel's geometry and range as the reference's own decoder reports them

One file per row of the rules of fuif.cpp:345-350, 374-430, 453: a whole-picture palette with and without alpha, a palette so small that
Squeeze is switched off, per-channel compaction after and BEFORE the colour transform, the lossy rule that clears all three options
only when -K is on, -K at and below the number of colours, a palette beside a photographic alpha, flat pictures, and a one-colour gray
picture on which compaction fails.  Nothing here is reference source; the .fuif files and the manifest are data.
Re-run: python tests/golden/make_golden_palette.py   (does not touch the other generators' files or manifests)
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "palette")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fuif_amd.synth import from_recipe, write_pnm  # noqa: E402
from oracle_py import Ref, ref_cli, run_ref_cli  # noqa: E402

DEFAULTS = dict(palette_colors=256, compact_post=70, compact_pre=70)   # what the CLI does when no -K / -X / -Y is given


def graphic(w, h, c, bits, seed, **kw):
    return dict(kind="graphic", w=w, h=h, channels=c, bits=bits, seed=seed, **kw)


def photo(w, h, c, bits, seed, **kw):
    return dict(kind="photographic", w=w, h=h, channels=c, bits=bits, seed=seed, **kw)


SPARSE_PHOTO = photo(96, 72, 3, 8, 37, floor_to=8)
G257, G40 = graphic(64, 64, 3, 8, 5, colors=257), graphic(64, 64, 3, 8, 5, colors=40)
# name, recipe, bits, further CLI flags, the same as keywords of encode_image
SPECS = [
    ("rgb_120x90_pal35", graphic(120, 90, 3, 8, 31, colors=40), 8, [], dict(DEFAULTS)),
    ("rgba_72x64_pal19", graphic(72, 64, 4, 8, 32, colors=20), 8, [], dict(DEFAULTS)),
    ("gray_100x70_compact19_nosqueeze", graphic(100, 70, 1, 8, 33, colors=24, step=5), 8, [], dict(DEFAULTS)),
    ("rgb_128x96_pal94", graphic(128, 96, 3, 8, 34, colors=700, step=8), 8, [], dict(DEFAULTS)),
    ("rgb_64x48_pal11_R0", graphic(64, 48, 3, 8, 35, colors=12), 8, ["-R", "0"], dict(DEFAULTS, squeeze=False)),
    ("rgb_96x72_sparse_compact3", SPARSE_PHOTO, 8, [], dict(DEFAULTS)),
    ("rgb_96x72_sparse_K0_Q80", SPARSE_PHOTO, 8, ["-K", "0", "-Q", "80"], dict(DEFAULTS, palette_colors=0, quality=80)),
    ("rgb_96x72_sparse_Q80", SPARSE_PHOTO, 8, ["-Q", "80"], dict(DEFAULTS, quality=80)),
    ("gray12_24x50_precompact", photo(24, 50, 1, 12, 15), 12, [], dict(DEFAULTS)),
    ("gray14_40x36_precompact", photo(40, 36, 1, 14, 4), 14, [], dict(DEFAULTS)),
    ("rgb_64x64_precompact_then_pal88", G257, 8, [], dict(DEFAULTS)),
    ("rgb_64x64_pal88_C0", G257, 8, ["-C", "0"], dict(DEFAULTS, ycocg=False)),
    ("rgb_64x64_K35_exact", G40, 8, ["-K", "35"], dict(DEFAULTS, palette_colors=35)),
    ("rgb_64x64_K34_one_short", G40, 8, ["-K", "34"], dict(DEFAULTS, palette_colors=34)),
    ("rgb_64x64_K16", G40, 8, ["-K", "16"], dict(DEFAULTS, palette_colors=16)),
    ("rgba_72x64_pal28_photo_alpha", dict(kind="stack", parts=[graphic(72, 64, 3, 8, 41, colors=30), photo(72, 64, 1, 8, 9)]), 8, [], dict(DEFAULTS)),
    ("graya_40x36_pal9_nosqueeze", graphic(40, 36, 2, 8, 8, colors=9), 8, [], dict(DEFAULTS)),
    ("rgb_30x40_flat77", dict(kind="full", shape=[3, 40, 30], value=77), 8, [], dict(DEFAULTS)),
    ("rgb_40x30_two_colours", graphic(40, 30, 3, 8, 3, colors=2), 8, [], dict(DEFAULTS)),
    ("rgb_5x4_pal3", graphic(5, 4, 3, 8, 6, colors=3), 8, [], dict(DEFAULTS)),
    ("gray_30x40_flat9_compaction_fails", dict(kind="full", shape=[1, 40, 30], value=9), 8, [], dict(DEFAULTS)),
]


def main():
    if ref_cli() is None or not Ref.available():
        sys.exit("oracle/_ref is not built (make -C oracle ref cli)")
    os.makedirs(OUT, exist_ok=True)
    ref = Ref()
    fixtures = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, recipe, bits, extra, kwargs in SPECS:
            img = from_recipe(recipe)
            c = img.shape[0]
            src = os.path.join(tmp, name + (".pam" if c in (2, 4) else ".ppm" if c == 3 else ".pgm"))
            write_pnm(src, img, (1 << bits) - 1)
            dst = os.path.join(OUT, name + ".fuif")
            flags = ["-I", "0"] + extra
            r = run_ref_cli(flags + [src, dst])
            if r.returncode != 0:
                sys.exit("%s: the reference CLI failed\n%s" % (name, r.stderr))
            blob = open(dst, "rb").read()
            again = dst + ".again"
            run_ref_cli(flags + [src, again])
            assert open(again, "rb").read() == blob, name + ": the reference CLI is not deterministic here"
            os.remove(again)
            dec = ref.decode(blob, undo=False)
            assert dec.ok, name
            channels = [dict(w=ch["w"], h=ch["h"], hshift=ch["hshift"], vshift=ch["vshift"], minval=ch["minval"], maxval=ch["maxval"], q=ch["q"])
                        for ch in dec.channels]
            fixtures.append(dict(name=name, file=name + ".fuif", nbytes=len(blob), input=recipe, bits=bits, flags=flags, encode=kwargs,
                                 lossless="quality" not in kwargs, transforms=[[t[0]] + list(t[1]) for t in dec.transforms],
                                 nb_coded_channels=len(dec.channels), channels=channels))
            print("%-40s %6d bytes, %2d channels, transforms %s" % (name, len(blob), len(dec.channels), fixtures[-1]["transforms"]))
    with open(os.path.join(OUT, "manifest_palette.json"), "w") as f:
        json.dump(dict(fixtures=fixtures), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
