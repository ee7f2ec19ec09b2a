"""Times the two routes from decoded `-y` streams to frame bytes on one MI355X (profiles/yuv_decode.txt):

  keep 2:  Plan(blob, keep=2): inverse transforms up to the recorded [YCbCr, ChromaSubsample] pair, then k_pack_yuv420 (raw 4:2:0 frames)
  full:    Plan(blob): the whole chain (chroma upsampled, YCbCr -> RGB, clamp), then fuifgpu_batch_pack_out (interleaved RGB bytes)

Both batches live in one process and take turns, repeat after repeat.  transform_ms is fuifgpu_batch_last_timing's (device events around
the schedule); the pack launches are timed with device events of this script's own around one call on the null stream.  Bytes are
computed from the shapes: what the kernel has to read and write, not what a counter saw.

    python tools/yuv_decode_time.py [--images 64] [--w 3840] [--h 2160] [--bits 8] [--distinct 4] [--repeats 9] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fuif_amd  # noqa: E402
from fuif_amd.synth import yuv420_frame  # noqa: E402


class Events:
    def __init__(self):
        self.hip = fuif_amd.hip_runtime()
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time(self, fn):
        """milliseconds of what fn queues on the null stream"""
        assert self.hip.hipEventRecord(self.a, None) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value


def med(v):
    return "%.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, n = a.w, a.h, a.images
    bps = 2 if a.bits > 8 else 1
    frames = [yuv420_frame(w, h, a.bits, 3 + k) for k in range(a.distinct)]
    distinct = fuif_amd.encode_yuv420_batch(frames, w, h, a.bits, tree_mode=0, index=True, gpu_forward=True, gpu_entropy=True)
    blobs = [distinct[k % a.distinct] for k in range(n)]        # (the same host object: uploaded once, replicated on the device)
    cap = sum(len(b) for b in blobs)
    L = fuif_amd.lib()
    ev = Events()
    routes = {"keep2": fuif_amd.Plan(blobs[0], keep=2), "full": fuif_amd.Plan(blobs[0])}
    batches = {k: fuif_amd.Batch(p, n, cap) for k, p in routes.items()}
    frame_size = routes["keep2"].yuv420_bytes()
    assert frame_size == len(frames[0])
    pitch_y = (w * bps + 255) // 256 * 256 + 256
    pitch_c_i420 = (((w + 1) // 2) * bps + 255) // 256 * 256 + 256
    forms = {"i420 tight": dict(), "nv12 tight": dict(layout="nv12"),
             "i420 pitch %d / %d" % (pitch_y, pitch_c_i420): dict(pitch_y=pitch_y, pitch_c=pitch_c_i420),
             "nv12 pitch %d / %d" % (pitch_y, pitch_y): dict(layout="nv12", pitch_y=pitch_y, pitch_c=pitch_y)}
    dst_bytes = max([routes["keep2"].yuv420_bytes(**kw) for kw in forms.values()] + [batches["full"].packed_bytes()]) * n
    dst = L.fuifgpu_dev_alloc(dst_bytes)
    assert dst
    res = {"transform_ms": {k: [] for k in routes}, "pack_ms": {k: [] for k in list(forms) + ["full pack_out"]}}
    try:
        for b in batches.values():
            b.upload(blobs)
        for rep in range(a.repeats + 1):                        # repeat 0 warms every launch up and is left out
            for k, b in batches.items():
                b.decode()
                b.undo_transforms()
                b.sync()
                assert not b.status()[0].any()
                t = b.timing()[1]
                packs = {}
                if k == "keep2":
                    for name, kw in forms.items():
                        packs[name] = ev.time(lambda: b.pack_yuv420(0, n, dst, **kw))
                else:
                    packs["full pack_out"] = ev.time(lambda: b.pack_out(dst))
                if rep:
                    res["transform_ms"][k].append(t)
                    for name, ms in packs.items():
                        res["pack_ms"][name].append(ms)
        got = [batches["keep2"].download_yuv420(k) for k in range(a.distinct)]
        assert got == frames, "the keep-2 route does not give the input frames back"
    finally:
        L.fuifgpu_dev_free(dst)
        for b in batches.values():
            b.close()
    samples = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    pack_bytes = n * samples * (4 + bps)                        # int32 in, 1 or 2 bytes out
    packout_bytes = n * w * h * 3 * (4 + bps)
    lines = ["%d x %dx%d %d-bit -y streams with the group index (%d distinct frames, lossless, %.1f MB per stream), %d repeats after a warm-up; median (min - max)"
             % (n, w, h, a.bits, a.distinct, len(distinct[0]) / 1e6, a.repeats),
             "inverse schedule: keep 2: %d ops, out slab %.1f MB per image;  full: %d ops, out slab %.1f MB per image"
             % (routes["keep2"].info.nb_ops, routes["keep2"].info.out_elems * 4 / 1e6, routes["full"].info.nb_ops, routes["full"].info.out_elems * 4 / 1e6)]
    for k in routes:
        lines.append("transform_ms  %-6s %s ms" % (k, med(res["transform_ms"][k])))
    for name in forms:
        v = res["pack_ms"][name]
        lines.append("k_pack_yuv420 %-24s %s ms   %.2f TB/s of %.1f MB" % (name, med(v), pack_bytes / statistics.median(v) / 1e9, pack_bytes / 1e6))
    v = res["pack_ms"]["full pack_out"]
    lines.append("pack_out      %-24s %s ms   %.2f TB/s of %.1f MB" % ("RGB interleaved", med(v), packout_bytes / statistics.median(v) / 1e9, packout_bytes / 1e6))
    k2 = statistics.median(res["transform_ms"]["keep2"]) + statistics.median(res["pack_ms"]["i420 tight"])
    fu = statistics.median(res["transform_ms"]["full"]) + statistics.median(v)
    lines.append("route totals (medians): keep 2 + k_pack_yuv420 %.3f ms, full + pack_out %.3f ms, ratio %.2f" % (k2, fu, fu / k2))
    print("\n".join(lines))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
