#!/usr/bin/env python3
"""Generate tests/golden/yuv/: streams the REAL reference CLI writes for raw YUV 4:2:0 input (run on the build machine only).

  inputs  : seeded fuif_amd.synth.yuv420_frame frames written as tight I420 .yuv files (a clip: v-00.yuv, v-01.yuv, ... of seeds
            seed, seed + 1, ...)
  encoder : the unmodified reference CLI oracle/_ref/fuif with `-I 0 -K 0 -X 0 -Y 0 -y WxH[:b] ...` (single-leaf trees: the mode in
            which the product's writer is byte-identical, tests/test_writer.py); clips with `-M 0`, the only distance the reference can
            match .yuv frames with (2dmatch.h:321-322 indexes the chroma planes with luma coordinates)
  recorded: yuv/manifest_yuv.json -- the synth arguments, the CLI flags, the keywords of fuif_amd.encode_yuv420 / encode_yuv420_clip
            that mean the same, the transform ids, and per channel that is not all zero its hcshift, vcshift, component and the
            quantisation constant q the reference's own decoder reads back from the stream

One file per rule of the `-y` route: lossless, the qualities of fuif.cpp:459-503 behind the factors of fuif.cpp:432-434, the remap without
Squeeze (-R 0), wide and tall frames (the order of the squeeze steps), 5x4 (too small for Squeeze) and 6x4 (squeezed), 1x1 and 2x2, 10 / 12 /
14 bits, clips.  Nothing here is reference source; the .fuif files and the manifest are data.
Re-run: python tests/golden/make_golden_yuv.py   (does not touch the other generators' files)
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "yuv")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fuif_amd.synth import write_yuv, yuv420_frame  # noqa: E402
from oracle_py import Ref, ref_cli, run_ref_cli  # noqa: E402

BASE_FLAGS = ["-I", "0", "-K", "0", "-X", "0", "-Y", "0"]
# name, (w, h, bits, seed, frames), further flags, the same as keywords of encode_yuv420 (a clip: of encode_yuv420_clip)
SPECS = [
    ("yuv8_97x61", (97, 61, 8, 31, 1), [], dict()),
    ("yuv8_97x61_Q80", (97, 61, 8, 31, 1), ["-Q", "80"], dict(quality=80)),
    ("yuv8_97x61_Q35_70", (97, 61, 8, 31, 1), ["-Q", "35,70"], dict(quality=35, chroma_quality=70)),
    ("yuv8_97x61_Q100_90", (97, 61, 8, 31, 1), ["-Q", "100,90"], dict(quality=100, chroma_quality=90)),
    ("yuv8_97x61_R0", (97, 61, 8, 31, 1), ["-R", "0"], dict(squeeze=False)),
    ("yuv8_97x61_R0_Q60", (97, 61, 8, 31, 1), ["-R", "0", "-Q", "60"], dict(squeeze=False, quality=60)),
    ("yuv8_200x9_Q0", (200, 9, 8, 32, 1), ["-Q", "0"], dict(quality=0)),
    ("yuv8_33x130", (33, 130, 8, 33, 1), [], dict()),
    ("yuv8_5x4", (5, 4, 8, 34, 1), [], dict()),
    ("yuv8_5x4_Q80", (5, 4, 8, 34, 1), ["-Q", "80"], dict(quality=80)),
    ("yuv8_6x4", (6, 4, 8, 35, 1), [], dict()),
    ("yuv8_1x1", (1, 1, 8, 36, 1), [], dict()),
    ("yuv8_2x2", (2, 2, 8, 37, 1), [], dict()),
    ("yuv10_75x49", (75, 49, 10, 38, 1), [], dict()),
    ("yuv10_75x49_Q60", (75, 49, 10, 38, 1), ["-Q", "60"], dict(quality=60)),
    ("yuv12_41x37_Q50", (41, 37, 12, 39, 1), ["-Q", "50"], dict(quality=50)),
    ("yuv14_40x36", (40, 36, 14, 40, 1), [], dict()),
    ("yuv8_96x60x3_M0", (96, 60, 8, 41, 3), ["-M", "0"], dict()),
    ("yuv8_96x60x3_M0_F25_Q70", (96, 60, 8, 41, 3), ["-M", "0", "-F", "25", "-Q", "70"], dict(framerate=25, quality=70)),
]


def main():
    if ref_cli() is None or not Ref.available():
        sys.exit("oracle/_ref is not built (make -C oracle ref cli)")
    os.makedirs(OUT, exist_ok=True)
    ref = Ref()
    fixtures, dropped = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (w, h, bits, seed, frames), extra, kwargs in SPECS:
            work = os.path.join(tmp, name)
            os.makedirs(work)
            for f in range(frames):
                write_yuv(os.path.join(work, "v-%02d.yuv" % f), yuv420_frame(w, h, bits, seed + f))
            src = os.path.join(work, "v-%02d.yuv" if frames > 1 else "v-00.yuv")
            dst = os.path.join(OUT, name + ".fuif")
            flags = BASE_FLAGS + ["-y", "%dx%d" % (w, h) + (":%d" % bits if bits != 8 else "")] + extra
            r = run_ref_cli(flags + [src, dst])
            if r.returncode != 0 or not os.path.exists(dst):
                dropped.append(name)
                print("%-28s DROPPED: the reference CLI failed (exit %s)\n%s" % (name, r.returncode, r.stderr[-400:]))
                continue
            blob = open(dst, "rb").read()
            dec = ref.decode(blob, undo=False)
            assert dec.ok, name
            channels = [dict(index=i, hcshift=ch["hcshift"], vcshift=ch["vcshift"], component=ch["component"], q=ch["q"])
                        for i, ch in enumerate(dec.channels) if not (ch["minval"] == 0 and ch["maxval"] == 0)]
            fixtures.append(dict(name=name, file=name + ".fuif", nbytes=len(blob), synth=dict(w=w, h=h, bits=bits, seed=seed, frames=frames),
                                 flags=flags, encode=kwargs, transforms=[t[0] for t in dec.transforms], nb_coded_channels=len(dec.channels),
                                 channels=channels))
            print("%-28s %6d bytes, %2d of %2d channels carry a q" % (name, len(blob), len(channels), len(dec.channels)))
    with open(os.path.join(OUT, "manifest_yuv.json"), "w") as f:
        json.dump(dict(fixtures=fixtures, dropped=dropped), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
