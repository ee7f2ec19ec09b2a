"""Seeded synthetic "photographic" images.

Per channel: sum of 6 sinusoids A*sin(2*pi*fx*x/w+p1)*cos(2*pi*fy*y/h+p2), A~U(10,40), f~U(0.5,8),
+128 + N(0, sigma), clipped to [0,255]; the 14-bit variant uses A~U(300,1500), +8192 + N(0,40),
clip [0,16383].  numpy.random.default_rng(seed) makes the image a pure function of
(seed, w, h, channels, bits, sigma) so the same pixels exist here and on the GPU box.
"""
import numpy as np


def photographic(w, h, channels=3, bits=8, seed=1, sigma=None):
    rng = np.random.default_rng(seed)
    if bits <= 8:
        amp, mid, sig, maxval = (10.0, 40.0), 128.0, 3.0, 255
    else:
        amp, mid, sig, maxval = (300.0, 1500.0), 8192.0, 40.0, (1 << bits) - 1
        scale = maxval / 16383.0
        amp, mid, sig = (amp[0] * scale, amp[1] * scale), mid * scale, sig * scale
    if sigma is not None:
        sig = sigma
    x = np.arange(w, dtype=np.float64)[None, :] / w
    y = np.arange(h, dtype=np.float64)[:, None] / h
    out = np.empty((channels, h, w), dtype=np.int32)
    for c in range(channels):
        acc = np.full((h, w), mid, dtype=np.float64)
        for _ in range(6):
            a = rng.uniform(*amp)
            fx, fy = rng.uniform(0.5, 8.0, size=2)
            p1, p2 = rng.uniform(0, 2 * np.pi, size=2)
            acc += a * np.sin(2 * np.pi * fx * x + p1) * np.cos(2 * np.pi * fy * y + p2)
        if sig > 0:
            acc += rng.normal(0.0, sig, size=(h, w))
        out[c] = np.clip(np.rint(acc), 0, maxval).astype(np.int32)
    return out


def graphic(w, h, channels=3, bits=8, seed=1, colors=32, step=1):
    """Seeded "screen content": a few dozen flat colours in overlapping rectangles and diagonal bands
    (what makes the reference CLI choose its Palette transform, transform/palette.h).  colors = size of the
    colour set; step > 1 additionally restricts every sample to multiples of `step` (sparse channel histograms:
    the per-channel palette heuristic of fuif.cpp:413-427)."""
    rng = np.random.default_rng(seed)
    maxval = (1 << bits) - 1
    table = rng.integers(0, maxval // step + 1, size=(colors, channels)) * step
    idx = np.zeros((h, w), dtype=np.int64)
    for _ in range(3 * colors):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = min(w, x0 + int(rng.integers(2, max(3, w // 2)))), min(h, y0 + int(rng.integers(2, max(3, h // 2))))
        idx[y0:y1, x0:x1] = int(rng.integers(0, colors))
    yy, xx = np.mgrid[0:h, 0:w]
    band = ((xx + 2 * yy) // 7) % 11 == 0
    idx[band] = (idx[band] + 1) % colors
    out = np.empty((channels, h, w), dtype=np.int32)
    for c in range(channels):
        out[c] = table[idx, c]
    return out


def filmstrip(w, h, frames=3, channels=3, bits=8, seed=1, background="photographic", colors=24, noise=0.25, speckles=0, edits=()):
    """Seeded animation, (F,C,H,W): what the Matching transform against the previous frame (transform/2dmatch.h:303-381) is made for.
    A static background (photographic() or graphic() of the same seed) in every frame; a flat sprite of about w/6 x h/2 that moves
    right by two samples per frame (wrapping); fresh noise in every frame over the rightmost `noise` share of the columns; `speckles`
    single samples per frame changed at seeded places (short runs); then `edits`, rows [frame, y0, y1, x0, x1, d]: that region of that
    frame becomes (background + d) mod 2^bits -- d = 0 puts the background back, which is how a test places runs of an exact length."""
    rng = np.random.default_rng(seed)
    maxval = (1 << bits) - 1
    back = photographic(w, h, channels, bits, seed) if background == "photographic" else graphic(w, h, channels, bits, seed, colors=colors)
    out = np.repeat(back[None], frames, axis=0)
    sw, sh = max(3, w // 6), max(2, h // 2)
    sx, sy = int(rng.integers(0, max(1, w - sw))), int(rng.integers(0, max(1, h - sh + 1)))
    colour = rng.integers(0, maxval + 1, size=channels)
    nw = int(round(noise * w))
    for f in range(frames):
        x0 = (sx + 2 * f) % max(1, w - sw)
        out[f, :, sy:sy + sh, x0:x0 + sw] = colour[:, None, None]
        if nw:
            out[f, :, :, w - nw:] = rng.integers(0, maxval + 1, size=(channels, h, nw))
        for _ in range(speckles):
            out[f, :, int(rng.integers(0, h)), int(rng.integers(0, w))] = rng.integers(0, maxval + 1, size=channels)
    for f, y0, y1, x0, x1, d in edits:
        out[f, :, y0:y1, x0:x1] = (back[:, y0:y1, x0:x1] + d) % (maxval + 1)
    return out.astype(np.int32)


def from_recipe(recipe):
    """A picture from a description that fits in a JSON manifest (tests/golden/palette/manifest_palette.json), for inputs that are not one
    call of the generators above ("filmstrip": the (F,C,H,W) frames of filmstrip() with the recipe's keywords):
      {"kind": "graphic" | "photographic", "w":, "h":, "channels":, "bits":, "seed":, ...their keywords, "floor_to": k}
          floor_to: every sample rounded down to a multiple of k (a sparse histogram on a photograph)
      {"kind": "full", "shape": [c, h, w], "value": v}            one flat value
      {"kind": "stack", "parts": [recipe, ...]}                     the parts' channels one behind the other (colour + alpha)"""
    kind = recipe["kind"]
    if kind == "full":
        return np.full(tuple(recipe["shape"]), recipe["value"], dtype=np.int32)
    if kind == "stack":
        return np.concatenate([from_recipe(p) for p in recipe["parts"]], axis=0)
    kw = {k: v for k, v in recipe.items() if k not in ("kind", "floor_to")}
    if kind == "filmstrip":
        return filmstrip(**kw)
    img = {"graphic": graphic, "photographic": photographic}[kind](**kw)
    k = recipe.get("floor_to", 1)
    return (img // k * k).astype(np.int32)


YUV_GUARD = 0xA5   # what yuv420_frame puts into the padding bytes of a pitched frame


def yuv420_planes(w, h, bits=8, seed=1):
    """the samples of yuv420_frame: (Y (h,w), Cb, Cr ((h+1)//2, (w+1)//2)) int32 -- smooth luma plus noise (photographic()'s first
    channel), chroma in the middle third of the range (smooth, a little noise)"""
    maxval = (1 << bits) - 1
    luma = photographic(w, h, 1, bits, seed=seed)[0]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rng = np.random.default_rng(seed + 7919)
    x = np.arange(cw, dtype=np.float64)[None, :] / cw
    y = np.arange(ch, dtype=np.float64)[:, None] / ch
    third = (maxval + 1) / 3.0
    chroma = []
    for _ in range(2):
        fx, fy = rng.uniform(0.5, 3.0, size=2)
        p1, p2 = rng.uniform(0, 2 * np.pi, size=2)
        acc = 1.5 * third + 0.4 * third * np.sin(2 * np.pi * fx * x + p1) * np.cos(2 * np.pi * fy * y + p2) + rng.normal(0.0, third / 80.0, size=(ch, cw))
        chroma.append(np.clip(np.rint(acc), np.ceil(third), np.floor(2 * third)).astype(np.int32))
    return luma, chroma[0], chroma[1]


def yuv420_frame(w, h, bits=8, seed=1, layout="i420", pitch=None):
    """A seeded raw YUV 4:2:0 frame as bytes, what `fuif -y WxH[:bits]` reads: the Y plane, then Cb and Cr (layout "i420") or one plane of
    Cb, Cr pairs ("nv12", the same samples); one byte per sample up to 8 bits, two little-endian above.  pitch: None = tight rows, else
    (pitch_y, pitch_c) in bytes -- the padding behind every row but the frame's last is filled with YUV_GUARD."""
    luma, cb, cr = yuv420_planes(w, h, bits, seed)
    dt = np.uint8 if bits <= 8 else np.dtype("<u2")
    planes = [luma, cb, cr] if layout == "i420" else [luma, np.stack([cb, cr], axis=-1).reshape(cb.shape[0], -1)]
    out = []
    for k, p in enumerate(planes):
        rows = np.ascontiguousarray(p.astype(dt)).view(np.uint8).reshape(p.shape[0], -1)
        want = rows.shape[1] if pitch is None else pitch[0 if k == 0 else 1]
        if want < rows.shape[1]:
            raise ValueError("a pitch smaller than the row")
        padded = np.full((rows.shape[0], want), YUV_GUARD, np.uint8)
        padded[:, : rows.shape[1]] = rows
        out.append(padded.reshape(-1))
    raw = np.concatenate(out)
    last_row = planes[-1].shape[1] * np.dtype(dt).itemsize
    tail = (0 if pitch is None else pitch[1]) - last_row
    return raw[: raw.size - tail].tobytes() if pitch is not None and tail > 0 else raw.tobytes()


def write_yuv(path, frame_bytes):
    """a raw .yuv file for the reference's import/read_yuv.h (tight I420 frames only)"""
    with open(path, "wb") as f:
        f.write(frame_bytes)


def write_pnm(path, planes, maxval=255):
    """planes: (C,H,W) int32 -> P5/P6/P7 file readable by the reference's import/read_pam.h."""
    c, h, w = planes.shape
    dt = np.uint8 if maxval < 256 else np.dtype(">u2")
    inter = np.ascontiguousarray(np.moveaxis(planes, 0, -1)).astype(dt)
    with open(path, "wb") as f:
        if c == 1:
            f.write(b"P5\n%d %d\n%d\n" % (w, h, maxval))
        elif c == 3:
            f.write(b"P6\n%d %d\n%d\n" % (w, h, maxval))
        else:
            tt = {2: b"GRAYSCALE_ALPHA", 4: b"RGB_ALPHA"}[c]
            f.write(b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH %d\nMAXVAL %d\nTUPLTYPE %s\nENDHDR\n" % (w, h, c, maxval, tt))
        f.write(inter.tobytes())
