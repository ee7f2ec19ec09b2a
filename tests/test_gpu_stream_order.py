"""GPU tests (-m gpu) of the stream contract of include/fuifgpu.h: every entry point that takes a `void *stream` does ALL its device work
on that stream.  The streams here are made with hipStreamNonBlocking (tests/hipstreams.py): nothing orders them against the null stream, so
a memset, a table upload or a kernel that slipped onto the null stream shows as a wrong result instead of being ordered by the runtime, as
it would be on the blocking streams of torch.cuda.Stream().

How a case catches a step that left its stream S:
  * S starts with a gate (a chain of device-to-device copies that ends by itself), and everything the call depends on is queued BEHIND
    it on S: the inputs X start as zeros and get their real values by copies on S, the output slabs of a batch get their 0x5A fill on S.
    A step that runs as soon as it is issued reads zeros (a valid input of every kernel here), and what it writes is overwritten.
  * the null stream gets a gate of its own, NULL_GATE_FACTOR times as long.  A step that was issued to the null stream runs after
    everything on S has finished: the snapshots that are taken on S do not hold its effect, and a late memset wipes what S computed
    (status words, bytes consumed, channel metadata, checksums).
  * the only wait is hipStreamSynchronize(S); results are snapshot copies queued on S behind the call.
  * directly after the calls have returned hipStreamQuery(S) must say not-ready.  If it says ready, the gate was too short (or a call
    that is listed as enqueue-only waited) and the case has proved nothing: it fails.
Each Part 1 case also shows that the zero input gives another result than the real one, so reading X too early cannot pass.

Gate length.  Host-side time of the calls under test (time to return, not to finish), measured on an MI355X with this module:
  single-transform exports, one launch each                    0.02 - 0.04 ms  (1.8 ms for the very first launch of the process,
                                                                                which loads the code object)
  fuifgpu_batch_decode (seven fills, two events, one launch)   0.03 - 0.06 ms
  fuifgpu_batch_undo_transforms (the slowest: ~20-50 launches) 0.05 - 0.11 ms
  fuifgpu_batch_pack_out / fuifgpu_plane_checksums             0.005 - 0.02 ms
  a whole Part 2 region (four calls and four snapshot copies)  0.11 - 0.22 ms
One 256 MiB device-to-device copy takes 0.10 ms (Gate measures it again at every run and sizes the chain from it: 500 copies).
GATE_MS = 50 is 25 times the slowest call there will ever be (the cold first launch) and over 200 times a whole warm region; every case
prints what it measured (pytest -s).  The entry points of the WAITS table take the length of the gates instead (150 - 185 ms).

Part 1: the single-transform and helper exports, one small shape each (stream order does not depend on the shape), against the references
the suite already has (the oracle's fo_kat_* restatements and the numpy formulas of the other test_gpu_* files).
Part 2: the batch pipeline on one stream, byte for byte over the whole caller-owned slabs against a run on the null stream.
Part 3: two batches on two streams with nothing waiting on the host, three rounds, against the oracle's planes.

Not run under the wavefront emulator (it has one "stream") and not in its file lists (tests/test_emulated_kernels.py)."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from conftest import ROOT, golden_blob

pytestmark = pytest.mark.gpu

if "_emu" in os.environ.get("FUIF_AMD_LIB", ""):
    pytest.skip("the wavefront emulator has one stream", allow_module_level=True)

from fuif_amd.synth import photographic  # noqa: E402
from hipstreams import Buf, Gate, Hip  # noqa: E402
from test_gpu_animation_encoder import keep as keep_span, match_rule, strip_of  # noqa: E402
from test_gpu_lossy_encoder import c_division  # noqa: E402
from test_gpu_palette_encoder import awkward_table, from_table  # noqa: E402
from test_gpu_transform_exports import _match_case, _zigzag, ref_squeeze  # noqa: E402
from test_gpu_yuv_decode import frame_bytes, golden as golden_file, wild_planes  # noqa: E402
from test_gpu_yuv_encoder import raw_frame  # noqa: E402

# ---- the two tables: every entry point of include/fuifgpu.h that takes a stream is in exactly one ------------------------------------
# only queue work on the stream and return (checked: the stream is still busy with its gate when they have returned)
ENQUEUE_ONLY = {
    "fuifgpu_batch_decode", "fuifgpu_batch_undo_transforms", "fuifgpu_batch_undo_transforms_to", "fuifgpu_batch_pack_out",
    "fuifgpu_batch_pack_yuv420", "fuifgpu_plane_checksums", "fuifgpu_peer_copy",
    "fuifgpu_inv_hsqueeze", "fuifgpu_inv_vsqueeze", "fuifgpu_inv_ycocg", "fuifgpu_inv_ycbcr", "fuifgpu_inv_quantize", "fuifgpu_upsample",
    "fuifgpu_inv_palette", "fuifgpu_inv_approximate",
    "fuifgpu_fwd_ycocg", "fuifgpu_fwd_hsqueeze", "fuifgpu_fwd_vsqueeze", "fuifgpu_fwd_quantize", "fuifgpu_channel_stats",
    "fuifgpu_fwd_match_frames", "fuifgpu_unpack_yuv420", "fuifgpu_pack_yuv420",
}
# wait for the stream before they return (checked: the stream is idle when they have returned)
WAITS = {
    "fuifgpu_batch_upload", "fuifgpu_batch_sync",
    "fuifgpu_batch_download_coef", "fuifgpu_batch_download_out", "fuifgpu_batch_download_packed", "fuifgpu_batch_download_yuv420",
    "fuifgpu_idct8x8", "fuifgpu_inv_match", "fuifgpu_fwd_palette",
}


def stream_entry_points():
    with open(os.path.join(ROOT, "include", "fuifgpu.h")) as f:
        text = f.read()
    return {m.group(1) for m in re.finditer(r"\b(fuifgpu_\w+)\s*\(([^()]*)\)\s*;", text) if "void *stream" in m.group(2)}


_DECLARED = stream_entry_points()
assert len(_DECLARED) >= 30, "include/fuifgpu.h was not understood"
assert not (ENQUEUE_ONLY & WAITS), sorted(ENQUEUE_ONLY & WAITS)
assert _DECLARED == ENQUEUE_ONLY | WAITS, ("in neither table: %s; in a table, not in the header: %s"
                                          % (sorted(_DECLARED - ENQUEUE_ONLY - WAITS), sorted((ENQUEUE_ONLY | WAITS) - _DECLARED)))

GATE_MS = 50.0
NULL_GATE_FACTOR = 3
FILL = 0x5A
UNTOUCHED = -7
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
GATE_TOO_SHORT = "%s: the stream was idle when the call(s) had returned (%.3f ms on the host): the gate was too short, or the call waited -- nothing is proved"


class Env:
    def __init__(self, gpulib, port, manifest):
        self.gpulib, self.port, self.manifest = gpulib, port, manifest
        self.L = gpulib.lib()
        self.olib = port.lib
        self.hip = Hip()
        self.gate = Gate(self.hip)
        self.references = {}
        print("\n[stream order] one %d MiB copy: %.3f ms; gate %.0f ms on the stream, %.0f ms on the null stream"
              % (self.gate.nbytes >> 20, self.gate.copy_ms, GATE_MS, NULL_GATE_FACTOR * GATE_MS))

    def gates(self, *streams):
        """the long gate on the null stream first, then the gate on every stream under test"""
        self.gate.queue(None, NULL_GATE_FACTOR * GATE_MS)
        for s in streams:
            self.gate.queue(s, GATE_MS)

    def note(self, what, **ms):
        print("[stream order] %-40s host ms: %s" % (what, "  ".join("%s %.3f" % kv for kv in ms.items())))


@pytest.fixture(scope="module")
def env(gpulib, port, manifest):
    e = Env(gpulib, port, manifest)
    yield e
    e.hip.device_sync()
    e.gate.free()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


# ==== Part 1: single-transform and helper exports under a gate ==========================================================================
def run_gated(env, entry, real, outs, call):
    """real: the arrays the call reads (or rewrites in place); outs: what its output-only buffers hold before.  call(x, o, S) gets the
    device addresses and returns the entry point's code.  -> (snapshots of x, snapshots of o), taken on S behind the call"""
    assert (entry in ENQUEUE_ONLY) != (entry in WAITS), entry
    hip = env.hip
    real = [np.ascontiguousarray(a) for a in real]
    outs = [np.ascontiguousarray(a) for a in outs]
    B = [Buf(hip, a) for a in real]
    X = [Buf(hip, np.zeros(a.nbytes, np.uint8)) for a in real]
    O = [Buf(hip, a) for a in outs]
    snaps = [Buf(hip, np.full(a.nbytes, 0xEE, np.uint8)) for a in real + outs]
    S = hip.stream()
    try:
        env.gates(S)
        for b, x in zip(B, X):
            hip.copy(x.ptr, b.ptr, b.nbytes, S)
        rc, ms = timed(lambda: call([x.ptr for x in X], [o.ptr for o in O], S))
        busy_on_return = hip.busy(S)
        for s, d in zip(snaps, X + O):
            hip.copy(s.ptr, d.ptr, d.nbytes, S)
        busy = hip.busy(S)
        hip.sync(S)
        env.note(entry, call=ms)
        assert rc == 0, (entry, rc, env.L.fuifgpu_last_error())
        if entry in ENQUEUE_ONLY:
            assert busy_on_return and busy, GATE_TOO_SHORT % (entry, ms)
        else:
            assert not busy_on_return, "%s is listed as waiting for its stream, which was still busy when it had returned" % entry
        got = [s.get(a.dtype).reshape(a.shape) for s, a in zip(snaps, real + outs)]
        return got[: len(real)], got[len(real):]
    finally:
        hip.sync(S)
        hip.destroy(S)
        for b in B + X + O + snaps:
            b.free()


def zeros_like_all(arrays):
    return [np.zeros_like(a) for a in arrays]


def differ(want, idle):
    """the reference result of the all-zero input is not the expected result: a call that read its inputs before they arrived shows"""
    want, idle = [np.asarray(a) for a in want], [np.asarray(a) for a in idle]
    return any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(want, idle))


def test_inv_hsqueeze(env):
    w1, w2, h, n = 65, 64, 130, 3
    rng = np.random.default_rng(1)
    real = [rng.integers(-3000, 3000, (n, h, w1), dtype=np.int32), rng.integers(-700, 700, (n, h, w2), dtype=np.int32)]
    ref = lambda a: [np.stack([ref_squeeze(env.olib, True, a[0][p], a[1][p]) for p in range(n)])]   # noqa: E731
    want = ref(real)
    assert differ(want, ref(zeros_like_all(real)))
    _, got = run_gated(env, "fuifgpu_inv_hsqueeze", real, [np.zeros((n, h, w1 + w2), np.int32)],
                       lambda x, o, S: env.L.fuifgpu_inv_hsqueeze(x[0], w1, x[1], w2, h, o[0], n, h * w1, h * w2, h * (w1 + w2), S))
    assert np.array_equal(got[0], want[0])


def test_inv_vsqueeze(env):
    h1, h2, w, n = 65, 64, 300, 2
    rng = np.random.default_rng(2)
    real = [rng.integers(-3000, 3000, (n, h1, w), dtype=np.int32), rng.integers(-700, 700, (n, h2, w), dtype=np.int32)]
    ref = lambda a: [np.stack([ref_squeeze(env.olib, False, a[0][p], a[1][p]) for p in range(n)])]   # noqa: E731
    want = ref(real)
    assert differ(want, ref(zeros_like_all(real)))
    _, got = run_gated(env, "fuifgpu_inv_vsqueeze", real, [np.zeros((n, h1 + h2, w), np.int32)],
                       lambda x, o, S: env.L.fuifgpu_inv_vsqueeze(x[0], h1, x[1], h2, w, o[0], n, h1 * w, h2 * w, (h1 + h2) * w, S))
    assert np.array_equal(got[0], want[0])


@pytest.mark.parametrize("ycbcr", [0, 1], ids=["ycocg", "ycbcr"])
def test_inv_color(env, ycbcr):
    w, h, maxval = 130, 33, 255
    rng = np.random.default_rng(3 + ycbcr)
    lo, hi = (-maxval - 10, 2 * maxval) if not ycbcr else (-20, maxval + 20)
    real = [rng.integers(lo, hi, (h, w), dtype=np.int32) for _ in range(3)]

    def ref(planes):
        out = [p.copy() for p in planes]
        assert env.olib.fo_kat_inv_color(ycbcr, *[p.ctypes.data_as(C.c_void_p) for p in out], w, h, 0, maxval)
        return out
    want = ref(real)
    assert differ(want, ref(zeros_like_all(real)))
    if ycbcr:
        got, _ = run_gated(env, "fuifgpu_inv_ycbcr", real, [], lambda x, o, S: env.L.fuifgpu_inv_ycbcr(x[0], x[1], x[2], w, h, w, w, w, 0, maxval, S))
    else:
        got, _ = run_gated(env, "fuifgpu_inv_ycocg", real, [], lambda x, o, S: env.L.fuifgpu_inv_ycocg(x[0], x[1], x[2], w, h, w, w, w, maxval, S))
    for g, e in zip(got, want):
        assert np.array_equal(g, e)


def test_inv_quantize(env):
    n, q = 257 * 33, 16
    a = np.random.default_rng(4).integers(-2000, 2000, n).astype(np.int32)
    want = a * q
    assert differ([want], [np.zeros_like(a) * q])
    got, _ = run_gated(env, "fuifgpu_inv_quantize", [a], [], lambda x, o, S: env.L.fuifgpu_inv_quantize(x[0], n, q, S))
    assert np.array_equal(got[0], want)


def test_idct8x8(env):
    bw, bh, maxval = 3, 2, 255
    rng = np.random.default_rng(5)
    planes = rng.integers(-60, 60, (64, bh, bw), dtype=np.int32)
    planes[0] = rng.integers(-4 * (maxval + 1), 4 * (maxval + 1), (bh, bw), dtype=np.int32)

    def ref(p):
        out = np.zeros((bh * 8, bw * 8), np.int32)
        assert env.olib.fo_kat_inv_dct(p.ctypes.data_as(C.c_void_p), bw, bh, maxval, out.ctypes.data_as(C.c_void_p))
        return out
    want = ref(planes)
    assert differ([want], [ref(np.zeros_like(planes))])
    z = _zigzag(env.olib)

    def call(x, o, S):
        ptrs = (C.c_void_p * 64)(*[x[0] + int(z[i]) * bh * bw * 4 for i in range(64)])
        return env.L.fuifgpu_idct8x8(ptrs, bw, bh, o[0], maxval, S)
    _, got = run_gated(env, "fuifgpu_idct8x8", [planes], [np.zeros((bh * 8, bw * 8), np.int32)], call)
    assert np.array_equal(got[0], want)


def test_upsample(env):
    w, h, srh, srv = 5, 3, 2, 2
    src = np.random.default_rng(6).integers(-50, 300, (h, w), dtype=np.int32)

    def ref(a):
        out = np.zeros((h * srv, w * srh), np.int32)
        assert env.olib.fo_kat_upsample(a.ctypes.data_as(C.c_void_p), w, h, srh, srv, out.ctypes.data_as(C.c_void_p))
        return out
    want = ref(src)
    assert differ([want], [ref(np.zeros_like(src))])
    _, got = run_gated(env, "fuifgpu_upsample", [src], [np.zeros((h * srv, w * srh), np.int32)],
                       lambda x, o, S: env.L.fuifgpu_upsample(x[0], w, h, srh, srv, o[0], S))
    assert np.array_equal(got[0], want)


def test_inv_palette(env):
    w, h, colours = 64, 33, 200
    rng = np.random.default_rng(7)
    idx = rng.integers(-3, colours + 4, (h, w), dtype=np.int32)
    row = rng.integers(-500, 1500, colours, dtype=np.int32)
    ref = lambda i, r: r[np.clip(i, 0, colours - 1)]   # noqa: E731
    want = ref(idx, row)
    assert differ([want], [ref(np.zeros_like(idx), np.zeros_like(row))])
    _, got = run_gated(env, "fuifgpu_inv_palette", [idx, row], [np.full((h, w), UNTOUCHED, np.int32)],
                       lambda x, o, S: env.L.fuifgpu_inv_palette(x[0], w, h, x[1], colours, o[0], S))
    assert np.array_equal(got[0], want)


def test_inv_approximate(env):
    n, q = 1000, 4
    rng = np.random.default_rng(8)
    a, r = rng.integers(-700, 700, n).astype(np.int32), rng.integers(0, q, n).astype(np.int32)
    want = a * q + r
    assert differ([want], [np.zeros_like(a)])
    got, _ = run_gated(env, "fuifgpu_inv_approximate", [a, r], [], lambda x, o, S: env.L.fuifgpu_inv_approximate(x[0], x[1], n, q, S))
    assert np.array_equal(got[0], want) and np.array_equal(got[1], r)


@pytest.mark.parametrize("mode", ["free_offsets", "previous_frames"])
def test_inv_match(env, mode):
    rng = np.random.default_rng(9)
    if mode == "free_offsets":
        w, h, n_planes, maxz, q, frames = 40, 30, 3, 24, 1, 1
        z, planes = _match_case(rng, w, h, n_planes, maxz, 0.5)
    else:
        w, fh, frames, n_planes = 24, 10, 4, 3
        h, q, maxz = fh * frames, 2 * fh * fh + (fh & 1), 1
        z, planes = _match_case(rng, w, h, n_planes, frames, 0.6)

    def ref(zz, pp):
        out = pp.copy()
        assert env.olib.fo_kat_inv_match(zz.ctypes.data_as(C.c_void_p), w, h, out.ctypes.data_as(C.c_void_p), n_planes, 0, q, maxz, frames)
        return out
    want = ref(z, planes)
    assert differ([want], [ref(np.zeros_like(z), np.zeros_like(planes))]) and differ([want], [planes])

    def call(x, o, S):
        ptrs = (C.c_void_p * n_planes)(*[x[1] + k * w * h * 4 for k in range(n_planes)])
        return env.L.fuifgpu_inv_match(x[0], w, h, ptrs, n_planes, 0, q, maxz, frames, S)
    got, _ = run_gated(env, "fuifgpu_inv_match", [z, planes], [], call)
    assert np.array_equal(got[1], want) and np.array_equal(got[0], z)


def test_fwd_ycocg(env):
    w, h, maxval = 130, 33, 255
    rng = np.random.default_rng(10)
    rgb = [rng.integers(0, maxval + 1, size=(h, w)).astype(np.int32) for _ in range(3)]
    ref = lambda c: [(((c[0] + c[2]) >> 1) + c[1]) >> 1, c[0] - c[2], c[1] - ((c[0] + c[2]) >> 1)]   # noqa: E731  (transform/ycocg.h:65-95)
    want = ref(rgb)
    assert differ(want, ref(zeros_like_all(rgb)))
    got, _ = run_gated(env, "fuifgpu_fwd_ycocg", rgb, [], lambda x, o, S: env.L.fuifgpu_fwd_ycocg(x[0], x[1], x[2], w, h, S))
    for g, e in zip(got, want):
        assert np.array_equal(g, e)


@pytest.mark.parametrize("horizontal", [True, False], ids=["hsqueeze", "vsqueeze"])
def test_fwd_squeeze(env, horizontal):
    """as in tests/test_gpu_transform_exports.py: a plane has exactly one (average, residual) pair, so the reference's inverse of what the
    kernel wrote must be the plane; the pair of the zero plane is zero"""
    w, h = 33, 17
    rng = np.random.default_rng(11 + int(horizontal))
    plane = rng.integers(-300, 1024, size=(h, w)).astype(np.int32)
    plane[: h // 2] = rng.integers(0, 4, size=(h // 2, w))
    aw, ah = ((w + 1) // 2, h) if horizontal else (w, (h + 1) // 2)
    rw, rh = (w - aw, h) if horizontal else (w, h - ah)
    idle = ref_squeeze(env.olib, horizontal, np.zeros((ah, aw), np.int32), np.zeros((rh, rw), np.int32))
    assert not idle.any() and differ([plane], [idle])
    entry = "fuifgpu_fwd_hsqueeze" if horizontal else "fuifgpu_fwd_vsqueeze"
    fn = getattr(env.L, entry)
    got_in, got = run_gated(env, entry, [plane], [np.full((ah, aw), UNTOUCHED, np.int32), np.full((rh, rw), UNTOUCHED, np.int32)],
                            lambda x, o, S: fn(x[0], w, h, o[0], o[1], S))
    assert np.array_equal(got_in[0], plane)
    assert np.array_equal(ref_squeeze(env.olib, horizontal, got[0], got[1]), plane)


def test_fwd_quantize_with_its_range_words(env):
    n, q = 65 * 4 + 1, 61
    v = np.random.default_rng(13).integers(-32768, 32768, size=n).astype(np.int32)
    v[-1] = -32768
    mm = np.array([INT32_MAX, INT32_MIN], np.int32)

    def ref(vals, preset):
        d = c_division(vals, q)
        return [d, np.array([min(int(preset[0]), int(d.min())), max(int(preset[1]), int(d.max()))], np.int32)]
    want = ref(v, mm)
    assert differ(want, ref(np.zeros_like(v), np.zeros_like(mm)))
    got, _ = run_gated(env, "fuifgpu_fwd_quantize", [v, mm], [], lambda x, o, S: env.L.fuifgpu_fwd_quantize(x[0], n, q, x[1], S))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_channel_stats(env):
    n = 257
    v = np.random.default_rng(14).integers(-32768, 32768, size=n).astype(np.int32)
    v[v == 0] = 7
    v[[5, n // 2, n - 2]] = 0
    preset = np.array([INT32_MAX, INT32_MIN, 0], np.int32)
    ref = lambda vals, p: np.array([min(int(p[0]), int(vals.min())), max(int(p[1]), int(vals.max())), int(p[2]) + int((vals == 0).sum())], np.int32)   # noqa: E731
    want = ref(v, preset)
    assert differ([want], [ref(np.zeros_like(v), np.zeros_like(preset))])
    got, _ = run_gated(env, "fuifgpu_channel_stats", [v, preset], [], lambda x, o, S: env.L.fuifgpu_channel_stats(x[0], n, x[1], S))
    assert np.array_equal(got[1], want) and np.array_equal(got[0], v)


@pytest.mark.parametrize("nb", [1, 3])
def test_fwd_palette(env, nb):
    n, max_colors = 67 * 5, 256
    planes = np.ascontiguousarray(from_table(awkward_table(nb), n, seed=10 * nb), dtype=np.int32)

    def ref(p):
        uniq, inverse = np.unique(p.T, axis=0, return_inverse=True)
        return [uniq.T, inverse.ravel().astype(np.int32)]
    want = ref(planes)
    assert differ(want, ref(np.zeros_like(planes)))
    pal = np.zeros((nb, max_colors), np.int32)
    count = C.c_int(0)

    def call(x, o, S):
        ptrs = (C.c_void_p * nb)(*x)
        return env.L.fuifgpu_fwd_palette(ptrs, nb, n, max_colors, o[0], pal.ctypes.data, C.byref(count), S)
    got_in, got = run_gated(env, "fuifgpu_fwd_palette", list(planes), [np.full(n, UNTOUCHED, np.int32)], call)
    assert count.value == want[0].shape[1]
    assert np.array_equal(pal[:, : count.value], want[0]) and np.array_equal(got[0], want[1])
    assert np.array_equal(np.stack(got_in), planes)


def test_fwd_match_frames(env):
    w, fh, frames = 24, 10, 4
    strip = strip_of(w, fh, frames, channels=3)
    keep_span(strip, fh, 11, 19, 2, 14)
    keep_span(strip, fh, 21, 25, 15, 20)
    c, h, _ = strip.shape

    def ref(s):
        m, zeroed = match_rule(s, fh)
        out = s.copy()
        out[:, zeroed] = 0
        return [m, out]
    want = ref(strip)
    assert want[0].any() and differ(want, ref(np.zeros_like(strip))) and differ([want[1]], [strip])

    def call(x, o, S):
        ptrs = (C.c_void_p * c)(*x)
        return env.L.fuifgpu_fwd_match_frames(ptrs, c, w, h, frames, o[0], S)
    got_planes, got = run_gated(env, "fuifgpu_fwd_match_frames", list(strip), [np.full((h, w), UNTOUCHED, np.int32)], call)
    assert np.array_equal(got[0], want[0]) and np.array_equal(np.stack(got_planes), want[1])


def test_unpack_yuv420(env):
    w, h, bits = 65, 18, 8
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rng = np.random.default_rng(15)
    planes = [rng.integers(1, 256, size=s).astype(np.int32) for s in ((h, w), (ch, cw), (ch, cw))]
    raw = raw_frame(planes, bits, "i420", 0)[0]
    assert differ(planes, zeros_like_all(planes))                 # (a frame of zero bytes unpacks to zero planes)
    yuv = env.gpulib.make_yuv_options("i420")
    outs = [np.full(p.shape, UNTOUCHED, np.int32) for p in planes] + [np.zeros(4, np.int32)]
    _, got = run_gated(env, "fuifgpu_unpack_yuv420", [raw], outs,
                       lambda x, o, S: env.L.fuifgpu_unpack_yuv420(x[0], w, h, bits, C.byref(yuv), o[0], o[1], o[2], o[3], S))
    for g, p in zip(got, planes):
        assert np.array_equal(g, p)
    assert not got[3].any()                                       # no sample above the maximum


def test_pack_yuv420(env):
    w, h, bits = 65, 18, 8
    planes = wild_planes(np.random.default_rng(16), w, h, 255)
    want = frame_bytes(planes, 255)[0]
    assert differ([want], [frame_bytes(zeros_like_all(planes), 255)[0]])
    yuv = env.gpulib.make_yuv_options("i420")
    got_in, got = run_gated(env, "fuifgpu_pack_yuv420", planes, [np.full(want.size, 0xA5, np.uint8)],
                            lambda x, o, S: env.L.fuifgpu_pack_yuv420(x[0], x[1], x[2], w, h, bits, C.byref(yuv), o[0], S))
    assert np.array_equal(got[0], want)


def numpy_checksums(slab, elems):
    """sum v[i] * (i mod 65521 + 1) per image in wrapping uint64 arithmetic (tests/test_gpu_transform_exports.py::test_plane_checksums_export)"""
    w = (np.arange(elems, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return np.array([(row[:elems].astype(np.int64).view(np.uint64) * w).sum(dtype=np.uint64) for row in slab], np.uint64)


def test_plane_checksums(env):
    elems, stride, n = 64 * 3 + 2, 196, 2
    slab = np.random.default_rng(17).integers(-(1 << 31), 1 << 31, size=(n, stride), dtype=np.int64).astype(np.int32)
    want = numpy_checksums(slab, elems)
    assert differ([want], [numpy_checksums(np.zeros_like(slab), elems)])
    _, got = run_gated(env, "fuifgpu_plane_checksums", [slab], [np.full(2 * n, -1, np.int32)],         # (the call zeroes the sums on the stream)
                       lambda x, o, S: env.L.fuifgpu_plane_checksums(x[0], elems, stride, n, o[0], S))
    assert np.array_equal(got[0].view(np.uint64), want)


def test_peer_copy_on_one_device(env):
    a = np.arange(1, 1001, dtype=np.int32)
    dev = env.gpulib.get_device()
    _, got = run_gated(env, "fuifgpu_peer_copy", [a], [np.zeros_like(a)], lambda x, o, S: env.L.fuifgpu_peer_copy(o[0], dev, x[0], dev, a.nbytes, S))
    assert np.array_equal(got[0], a)


# ==== Part 2: the batch pipeline on one non-blocking stream ============================================================================
PIPELINE_FIXTURES = ["rgb8_97x61", "rgb8_128x128_I0", "jpeg420_256x192_q90", "rgba14_80x72", "indexed_photographic_256x256"]


def fixture_blobs(env, name):
    """three streams of one plan: the whole file, a byte-truncated copy where the fixture has one (its status word is not 0), the file"""
    if name == "indexed_photographic_256x256":
        blob = env.gpulib.encode_image(photographic(256, 256, 3, 8, seed=5), 8, index=True)
        assert env.gpulib.index_parse(blob)
        return [blob, blob, blob]
    e = next(x for x in env.manifest["fixtures"] if x["name"] == name)
    full = golden_blob(e, next(c for c in e["cases"] if c["case"] == "full"))
    cut = [c for c in e["cases"] if c["case"].startswith("trunc") and c["preview"] == -1]
    return [full, golden_blob(e, cut[len(cut) // 2]) if cut else full, full]


class Slabs:
    """the caller-owned memory of one run: coefficient and output slab, the destination of pack_out and the checksum table"""

    def __init__(self, env, plan, n):
        info = plan.info
        packed = int(env.L.fuifgpu_plan_packed_bytes(plan._h, 0))
        assert packed
        sizes = dict(coef=2 * n * max(info.coef_elems, 1), out=4 * n * max(info.out_elems, 1), packed=n * packed, sums=8 * n)
        self.names = list(sizes)
        self.buf = {k: Buf(env.hip, np.zeros(v, np.uint8)) for k, v in sizes.items()}

    def __getitem__(self, k):
        return self.buf[k]

    def read(self):
        return {k: self.buf[k].get() for k in self.names}

    def free(self):
        for b in self.buf.values():
            b.free()


def out_planes_of(plan, out_bytes, image):
    slab = out_bytes.view(np.int32)[image * plan.info.out_elems: (image + 1) * plan.info.out_elems]
    return [slab[c["offset"]: c["offset"] + c["w"] * c["h"]].reshape(c["h"], c["w"]) for c in plan.output_channels]


def reference_run(env, name):
    """upload, decode, undo_transforms, pack_out and plane_checksums on the null stream with a device synchronise between the steps, every
    slab pre-filled with 0x5A; the planes are checked against the oracle as tests/test_gpu_parity.py does.  Computed once per fixture"""
    if name in env.references:
        return env.references[name]
    gpulib, hip = env.gpulib, env.hip
    blobs = fixture_blobs(env, name)
    n = len(blobs)
    plan = gpulib.Plan(blobs[0])
    slabs = Slabs(env, plan, n)
    batch = None
    try:
        for k in slabs.names:
            slabs[k].put(np.full(slabs[k].nbytes, FILL, np.uint8))
        batch = gpulib.Batch(plan, n, sum(len(b) for b in blobs), coef_ptr=slabs["coef"].ptr, out_ptr=slabs["out"].ptr)
        for step in (lambda: batch.upload(blobs), batch.decode, batch.undo_transforms, lambda: batch.pack_out(slabs["packed"].ptr),
                     lambda: gpulib.plane_checksums(slabs["out"].ptr, plan.info.out_elems, n, slabs["sums"].ptr)):
            step()
            hip.device_sync()
        data = slabs.read()
        st, used = batch.status()
        metas = [batch.channel_meta(i) for i in range(n)]
    finally:
        if batch is not None:
            batch.close()
        slabs.free()
    oracle = {}
    for i, blob in enumerate(blobs):
        if blob not in oracle:
            oracle[blob] = env.port.decode(blob)
        want = oracle[blob]
        got = out_planes_of(plan, data["out"], i)
        assert len(got) == len(want.channels), name
        for g, e in zip(got, want.channels):
            assert np.array_equal(g.reshape(-1), np.asarray(e["data"]).reshape(-1)), (name, i)
        if st[i] == 0:
            assert used[i] == want.stats["bytes"], (name, i)
    assert not (st & 2).any() and used.all() and st[0] == 0, name
    assert np.array_equal(data["sums"].view(np.uint64), numpy_checksums(data["out"].view(np.int32).reshape(n, -1), plan.info.out_elems))
    ref = dict(blobs=blobs, plan=plan, data=data, status=st, used=used, metas=metas)
    env.references[name] = ref
    return ref


@pytest.mark.parametrize("name", PIPELINE_FIXTURES)
def test_batch_pipeline_on_one_stream(env, name):
    gpulib, hip = env.gpulib, env.hip
    ref = reference_run(env, name)
    blobs, plan = ref["blobs"], ref["plan"]
    n = len(blobs)
    slabs, snaps = Slabs(env, plan, n), Slabs(env, plan, n)
    S = hip.stream()
    batch = None
    try:
        batch = gpulib.Batch(plan, n, sum(len(b) for b in blobs), coef_ptr=slabs["coef"].ptr, out_ptr=slabs["out"].ptr)
        batch.upload(blobs, stream=S)                         # (synchronises S itself: WAITS)
        assert not hip.busy(S)
        env.gates(S)
        for k in slabs.names:
            hip.fill(slabs[k].ptr, FILL, slabs[k].nbytes, S)
        t0 = time.perf_counter()
        _, t_decode = timed(lambda: batch.decode(S))
        _, t_undo = timed(lambda: batch.undo_transforms(S))
        _, t_pack = timed(lambda: batch.pack_out(slabs["packed"].ptr, stream=S))
        _, t_sums = timed(lambda: gpulib.plane_checksums(slabs["out"].ptr, plan.info.out_elems, n, slabs["sums"].ptr, S))
        for k in slabs.names:
            hip.copy(snaps[k].ptr, slabs[k].ptr, slabs[k].nbytes, S)
        region = (time.perf_counter() - t0) * 1e3
        busy = hip.busy(S)
        hip.sync(S)
        env.note("batch pipeline " + name, decode=t_decode, undo_transforms=t_undo, pack_out=t_pack, plane_checksums=t_sums, region=region)
        assert busy, GATE_TOO_SHORT % ("batch pipeline " + name, region)
        got = snaps.read()
        for k in slabs.names:
            assert np.array_equal(got[k], ref["data"][k]), "%s: the %s slab as S left it differs from the null-stream run's" % (name, k)
        st, used = batch.status()                             # (synchronises the device: the null stream's gate has ended too)
        assert np.array_equal(st, ref["status"]) and np.array_equal(used, ref["used"]), (name, st, used)
        for i in range(n):
            assert np.array_equal(batch.channel_meta(i), ref["metas"][i]), (name, i)
        live = slabs.read()
        for k in slabs.names:
            assert np.array_equal(live[k], ref["data"][k]), "%s: the %s slab was written after S had finished" % (name, k)
    finally:
        hip.device_sync()
        if batch is not None:
            batch.close()
        hip.destroy(S)
        slabs.free()
        snaps.free()


def test_streaming_batch_ranges_out_of_order(env):
    """streaming=True: no output slab; image 2 first, then images 0..1, through undo_transforms_to into a caller buffer"""
    gpulib, hip = env.gpulib, env.hip
    name = "rgb8_128x128_I0"
    ref = reference_run(env, name)
    blobs, plan = ref["blobs"], ref["plan"]
    n, image_bytes = len(blobs), 4 * plan.info.out_elems
    out, snap = Buf(hip, np.zeros(n * image_bytes, np.uint8)), Buf(hip, np.zeros(n * image_bytes, np.uint8))
    S = hip.stream()
    batch = None
    try:
        batch = gpulib.Batch(plan, n, sum(len(b) for b in blobs), streaming=True)
        batch.upload(blobs, stream=S)
        env.gates(S)
        hip.fill(out.ptr, FILL, out.nbytes, S)
        t0 = time.perf_counter()
        batch.decode(S)
        batch.undo_transforms_to(2, 1, out.ptr + 2 * image_bytes, S)
        batch.undo_transforms_to(0, 2, out.ptr, S)
        hip.copy(snap.ptr, out.ptr, out.nbytes, S)
        region = (time.perf_counter() - t0) * 1e3
        busy = hip.busy(S)
        hip.sync(S)
        env.note("streaming batch " + name, region=region)
        assert busy, GATE_TOO_SHORT % ("streaming batch", region)
        assert np.array_equal(snap.get(), ref["data"]["out"])
        st, used = batch.status()
        assert np.array_equal(st, ref["status"]) and np.array_equal(used, ref["used"])
        assert np.array_equal(out.get(), ref["data"]["out"])
    finally:
        hip.device_sync()
        if batch is not None:
            batch.close()
        hip.destroy(S)
        out.free()
        snap.free()


def test_keep_2_plan_to_yuv420_frames(env):
    """Plan(blob, keep=2) of the yuv420p_97x61 fixture: fuifgpu_batch_pack_yuv420 on S, then fuifgpu_batch_download_yuv420 directly behind
    it; the frame bytes are what tests/test_gpu_yuv_decode.py derives from the oracle's keep-2 channels"""
    gpulib, hip = env.gpulib, env.hip
    blob = golden_file("yuv420p_97x61.fuif")
    want = frame_bytes(env.port.decode(blob, keep=2).planes(), 255)[0]
    plan = gpulib.Plan(blob, keep=2)
    size, n = plan.yuv420_bytes(), 3
    assert size == want.size
    dst, snap = Buf(hip, np.zeros(n * size, np.uint8)), Buf(hip, np.zeros(n * size, np.uint8))
    yuv = gpulib.make_yuv_options("i420")
    S = hip.stream()
    batch = None
    try:
        batch = gpulib.Batch(plan, n, n * len(blob))
        batch.upload([blob] * n, stream=S)
        env.gates(S)
        hip.fill(dst.ptr, FILL, dst.nbytes, S)
        t0 = time.perf_counter()
        batch.decode(S)
        batch.undo_transforms(S)
        _, t_pack = timed(lambda: batch.pack_yuv420(0, n, dst.ptr, stream=S))
        hip.copy(snap.ptr, dst.ptr, dst.nbytes, S)
        region = (time.perf_counter() - t0) * 1e3
        busy = hip.busy(S)
        host = np.zeros(size, np.uint8)
        assert env.L.fuifgpu_batch_download_yuv420(batch._h, 1, C.byref(yuv), host.ctypes.data, S) == 0     # no sync in between: it waits
        assert not hip.busy(S), "fuifgpu_batch_download_yuv420 is listed as waiting for its stream"
        hip.sync(S)
        env.note("keep-2 batch to yuv420", pack_yuv420=t_pack, region=region)
        assert busy, GATE_TOO_SHORT % ("keep-2 batch", region)
        assert np.array_equal(host, want)
        assert np.array_equal(snap.get().reshape(n, size), np.stack([want] * n))
        assert not batch.status()[0].any()
    finally:
        hip.device_sync()
        if batch is not None:
            batch.close()
        hip.destroy(S)
        dst.free()
        snap.free()


def test_downloads_wait_for_the_work_in_front_of_them(env):
    """download_coef, download_out and download_packed with stream = S, each called directly behind a gate and queued work, with no
    synchronisation in between: each returns the finished data and leaves S idle"""
    gpulib, hip, L = env.gpulib, env.hip, env.L
    name = "rgb8_97x61"
    ref = reference_run(env, name)
    blobs, plan = ref["blobs"], ref["plan"]
    n, info = len(blobs), plan.info
    packed = len(ref["data"]["packed"]) // n
    S = hip.stream()
    batch = None
    try:
        batch = gpulib.Batch(plan, n, sum(len(b) for b in blobs))
        batch.upload(blobs, stream=S)
        env.gates(S)
        batch.decode(S)
        coef = np.full(max(info.coef_elems, 1), UNTOUCHED, np.int32)
        assert L.fuifgpu_batch_download_coef(batch._h, 0, coef.ctypes.data, S) == 0      # (image 0: the whole file, every channel decoded)
        assert not hip.busy(S)
        want = ref["data"]["coef"].view(np.int16).reshape(n, -1)[0].astype(np.int32)
        for c in plan.coded_channels:                            # (the planes: the gaps between them belong to nobody in a slab of the library's own)
            span = slice(c["offset"], c["offset"] + c["w"] * c["h"])
            assert np.array_equal(coef[span], want[span]), c

        env.gates(S)
        batch.undo_transforms(S)
        out = np.full(info.out_elems, UNTOUCHED, np.int32)
        assert L.fuifgpu_batch_download_out(batch._h, 2, out.ctypes.data, S) == 0
        assert not hip.busy(S)
        want = ref["data"]["out"].view(np.int32).reshape(n, -1)[2]
        for c in plan.output_channels:
            span = slice(c["offset"], c["offset"] + c["w"] * c["h"])
            assert np.array_equal(out[span], want[span]), c

        env.gates(S)
        batch.decode(S)
        batch.undo_transforms(S)
        host = np.zeros(packed, np.uint8)
        assert L.fuifgpu_batch_download_packed(batch._h, 1, 0, host.ctypes.data, S) == 0
        assert not hip.busy(S)
        assert np.array_equal(host, ref["data"]["packed"].reshape(n, -1)[1])

        env.gates(S)
        batch.decode(S)
        assert L.fuifgpu_batch_sync(batch._h, S) == 0
        assert not hip.busy(S)
        st, used = batch.status()
        assert np.array_equal(st, ref["status"]) and np.array_equal(used, ref["used"])
    finally:
        hip.device_sync()
        if batch is not None:
            batch.close()
        hip.destroy(S)


# ==== Part 3: two batches on two non-blocking streams ==================================================================================
ROUNDS = 3


class Side:
    """one of the two batches of a pairing: a streaming batch, the caller's output buffer (zeros: the gaps between the planes take part in
    the checksum), a checksum table of ROUNDS rows, and what the oracle says both must hold"""

    def __init__(self, env, blob, planes, n, wide_without_index):
        gpulib = env.gpulib
        self.n, self.plan = n, gpulib.Plan(blob)
        elems = self.plan.info.out_elems
        image = np.zeros(elems, np.int32)
        chans = self.plan.output_channels
        assert len(chans) == len(planes)
        for c, p in zip(chans, planes):
            image[c["offset"]: c["offset"] + c["w"] * c["h"]] = np.asarray(p["data"]).reshape(-1)
        self.want = np.stack([image] * n)
        self.want_sums = numpy_checksums(self.want, elems)
        assert self.want_sums.all()
        self.out = Buf(env.hip, np.zeros(4 * n * elems, np.uint8))
        self.sums = Buf(env.hip, np.full(8 * ROUNDS * n, 0xFF, np.uint8))
        self.batch = gpulib.Batch(self.plan, n, n * len(blob), streaming=True)
        self.batch.set_in_flight(2)
        if wide_without_index:
            self.batch.set_group_parallel(False)
        self.stream = env.hip.stream()
        self.batch.upload([blob] * n, stream=self.stream)
        self.begin = [env.hip.event() for _ in range(ROUNDS)]
        self.end = [env.hip.event() for _ in range(ROUNDS)]

    def decode(self, env, r):
        env.hip.record(self.begin[r], self.stream)
        self.batch.decode(self.stream)
        env.hip.record(self.end[r], self.stream)

    def finish(self, env, r):
        self.batch.undo_transforms_to(0, self.n, self.out.ptr, self.stream)
        env.gpulib.plane_checksums(self.out.ptr, self.plan.info.out_elems, self.n, self.sums.ptr + 8 * r * self.n, self.stream)

    def close(self, env):
        self.batch.close()
        env.hip.destroy(self.stream)
        for e in self.begin + self.end:
            env.hip.event_destroy(e)
        self.out.free()
        self.sums.free()


def indexed_bigtrees(env):
    e = next(x for x in env.manifest["fixtures"] if x["name"] == "rgb8_512x384_I16_bigtrees")
    blob = golden_blob(e, e["cases"][0])
    d = env.port.decode(blob)
    indexed = env.gpulib.index_append(blob, d.groups)
    assert env.gpulib.index_parse(indexed)
    return indexed, d.channels


def golden_with_planes(env, name):
    e = next(x for x in env.manifest["fixtures"] if x["name"] == name)
    blob = golden_blob(e, e["cases"][0])
    return blob, env.port.decode(blob).channels


@pytest.mark.parametrize("pairing", ["same_plan_wide", "different_plans"])
def test_two_batches_on_two_streams(env, pairing):
    """three rounds of decode, undo_transforms_to and plane_checksums for two batches, the host calls interleaved and nothing waiting on
    the host until both streams are synchronised at the end.  same_plan_wide: two streaming batches of 8 x c1_rgb8_512x512 with
    set_in_flight(2) and set_group_parallel(False), what bench.py's overlapped steps run; different_plans: rgb8_512x384_I16_bigtrees
    with its group index beside jpeg420_256x192_q90.  Whether the two decode launches of a round overlapped is printed, not asserted:
    the test makes the overlap possible, the runtime decides"""
    hip = env.hip
    if pairing == "same_plan_wide":
        blob, planes = golden_with_planes(env, "c1_rgb8_512x512")
        specs = [(blob, planes, 8, True), (blob, planes, 8, True)]
    else:
        specs = [indexed_bigtrees(env) + (3, False), golden_with_planes(env, "jpeg420_256x192_q90") + (3, False)]
    sides = []
    try:
        for spec in specs:
            sides.append(Side(env, *spec))
        a, b = sides
        env.gate.queue(None, NULL_GATE_FACTOR * GATE_MS)         # (whatever left its stream for the null stream runs late)
        for r in range(ROUNDS):
            a.decode(env, r)
            b.decode(env, r)
            a.finish(env, r)
            b.finish(env, r)
        hip.sync(a.stream)
        hip.sync(b.stream)
        overlapped = []
        for r in range(ROUNDS):
            a_ms, b_ms = hip.elapsed_ms(a.begin[r], a.end[r]), hip.elapsed_ms(b.begin[r], b.end[r])
            b_after_a = hip.elapsed_ms(a.begin[r], b.begin[r])
            overlapped.append(b_after_a < a_ms and b_after_a + b_ms > 0)
            print("[stream order] %s round %d: decode A %.3f ms, decode B %.3f ms, B began %.3f ms after A: %s"
                  % (pairing, r, a_ms, b_ms, b_after_a, "overlapped" if overlapped[-1] else "one after the other"))
        print("[stream order] %s: decode intervals overlapped in %d of %d rounds" % (pairing, sum(overlapped), ROUNDS))
        for which, s in zip("AB", sides):
            got = s.sums.get(np.uint64).reshape(ROUNDS, s.n)
            for r in range(ROUNDS):
                assert np.array_equal(got[r], s.want_sums), (pairing, which, r)
            assert np.array_equal(s.out.get(np.int32).reshape(s.n, -1), s.want), (pairing, which)
            st, used = s.batch.status()
            assert not st.any() and (used == used[0]).all() and used[0], (pairing, which)
    finally:
        hip.device_sync()
        for s in sides:
            s.close(env)
