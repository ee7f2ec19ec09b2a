#!/usr/bin/env python3
"""Generate tests/golden/lossy/: lossy Squeeze streams written by the REAL reference CLI (run on the build machine only).

  inputs  : seeded fuif_amd.synth.photographic pictures written as PNM / PAM
  encoder : the unmodified reference CLI oracle/_ref/fuif with `-I 0 -K 0 -X 0 -Y 0 -Q ...` (single-leaf trees, no palette,
            no 2D match: the mode in which the product's writer is byte-identical, tests/test_writer.py)
  recorded: lossy/manifest_lossy.json -- the synth arguments, the CLI flags, the keywords of fuif_amd.encode_image that mean the same,
            and per channel that is not all zero its hcshift, vcshift, component and the quantisation constant q the reference's
            own decoder reads back from the stream (an all-zero channel carries no q, encoding.cpp:490)

One file per rule of fuif.cpp:459-503: integer and fractional quality, a separate chroma quality, the <= 50 branch, luma lossless
with lossy chroma (100,90), quality 0, the remap without Squeeze (-R 0), 14-bit RGBA, gray, gray + alpha (whose alpha gets the
CHROMA table: component 1), a 5x4 picture (too small for Squeeze, yet no remap: the remap follows the option), -C 0 (luma table
for every channel).  Nothing here is reference source; the .fuif files and the manifest are data.
Re-run: python tests/golden/make_golden_lossy.py   (does not touch make_golden.py's files or manifest.json)
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "lossy")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fuif_amd.synth import photographic, write_pnm  # noqa: E402
from oracle_py import Ref, ref_cli, run_ref_cli  # noqa: E402

BASE_FLAGS = ["-I", "0", "-K", "0", "-X", "0", "-Y", "0"]
RGB, GRAY, RGBA14, GRAYA, TINY, WIDE, TALL = ((97, 61, 3, 8, 2), (64, 48, 1, 8, 3), (80, 72, 4, 14, 4), (40, 36, 2, 8, 5), (5, 4, 3, 8, 6),
                                              (200, 9, 3, 8, 13), (33, 130, 3, 8, 12))
# name, (w, h, channels, bits, seed), the -Q argument, further flags, the same as keywords of encode_image
SPECS = [
    ("rgb8_97x61_Q80", RGB, "80", [], dict(quality=80)),
    ("rgb8_97x61_Q35_70", RGB, "35,70", [], dict(quality=35, chroma_quality=70)),
    ("rgb8_97x61_Q97p5", RGB, "97.5", [], dict(quality=97.5)),
    ("rgb8_97x61_Q60_R0", RGB, "60", ["-R", "0"], dict(quality=60, squeeze=False)),
    ("rgb8_97x61_Q100_90", RGB, "100,90", [], dict(quality=100, chroma_quality=90)),
    ("rgb8_97x61_Q80_C0", RGB, "80", ["-C", "0"], dict(quality=80, ycocg=False)),
    ("rgb8_33x130_Q0", TALL, "0", [], dict(quality=0)),
    ("rgb8_200x9_Q50", WIDE, "50", [], dict(quality=50)),
    ("gray8_64x48_Q80", GRAY, "80", [], dict(quality=80)),
    ("gray8_64x48_Q60_R0", GRAY, "60", ["-R", "0"], dict(quality=60, squeeze=False)),
    ("rgba14_80x72_Q80", RGBA14, "80", [], dict(quality=80)),
    ("rgba14_80x72_Q35_70", RGBA14, "35,70", [], dict(quality=35, chroma_quality=70)),
    ("graya8_40x36_Q80", GRAYA, "80", [], dict(quality=80)),
    ("graya8_40x36_Q35_70", GRAYA, "35,70", [], dict(quality=35, chroma_quality=70)),
    ("rgb8_5x4_Q80", TINY, "80", [], dict(quality=80)),
    ("rgb8_5x4_Q50", TINY, "50", [], dict(quality=50)),
]


def main():
    if ref_cli() is None or not Ref.available():
        sys.exit("oracle/_ref is not built (make -C oracle ref cli)")
    os.makedirs(OUT, exist_ok=True)
    ref = Ref()
    fixtures = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (w, h, c, bits, seed), q_arg, extra, kwargs in SPECS:
            img = photographic(w, h, c, bits, seed=seed)
            src = os.path.join(tmp, name + (".pam" if c in (2, 4) else ".ppm" if c == 3 else ".pgm"))
            write_pnm(src, img, (1 << bits) - 1)
            dst = os.path.join(OUT, name + ".fuif")
            flags = BASE_FLAGS + ["-Q", q_arg] + extra
            r = run_ref_cli(flags + [src, dst])
            if r.returncode != 0:
                sys.exit("%s: the reference CLI failed\n%s" % (name, r.stderr))
            blob = open(dst, "rb").read()
            dec = ref.decode(blob, undo=False)
            assert dec.ok, name
            channels = [dict(index=i, hcshift=ch["hcshift"], vcshift=ch["vcshift"], component=ch["component"], q=ch["q"])
                        for i, ch in enumerate(dec.channels) if not (ch["minval"] == 0 and ch["maxval"] == 0)]
            fixtures.append(dict(name=name, file=name + ".fuif", nbytes=len(blob), synth=dict(w=w, h=h, channels=c, bits=bits, seed=seed),
                                 flags=flags, encode=kwargs, transforms=[t[0] for t in dec.transforms], nb_coded_channels=len(dec.channels),
                                 channels=channels))
            print("%-24s %6d bytes, %2d of %2d channels carry a q" % (name, len(blob), len(channels), len(dec.channels)))
    with open(os.path.join(OUT, "manifest_lossy.json"), "w") as f:
        json.dump(dict(fixtures=fixtures), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
