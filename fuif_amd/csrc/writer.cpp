// fuif_amd/csrc/writer.cpp -- FUIF stream writer (host C++), the input generator of the decode path.
//
// the reference encoder needs ~19 s per 4K image and does not exist on
// the GPU box, so the build carries its own writer.  It produces streams the REAL reference
// decoder accepts (tests/test_writer.py decodes them with oracle/_ref and compares pixels) using
// the same format decisions as the reference CLI for PNM input:
//   [with fuifgpu_palette_options, what the CLI tries by default for everything that is not a photograph: channel compaction before the
//    colour transform, a Palette over all channels (or all but the last) behind it, channel compaction again (fuif.cpp:345-350, 374-430;
//    transform/palette.h:92-142); palettes are meta-channels in front of the channel list, coded with predictor 3]
//   YCoCg (transform/ycocg.h:65-95) -> default Squeeze (transform/squeeze.h:135-170,227-321)
//   -> one channel per group (fuif.cpp:455), predictor 2 for the base channels and 0 for residuals
//   (fuif.cpp:580-588), tight ranges (image/image.h:127), responsive offsets (image.cpp:124-136,
//   encoding.cpp:552-565), compressed-vs-uncompressed fallback (encoding.cpp:529-551).
// The bit-level coding mirrors the decoder side it must agree with: RAC (maniac/rac_enc.h:28-100),
// symbol binarisation (maniac/symbol.h:154-185 read side), pre-order tree serialisation
// (maniac/compound.h:277-308 read side), context properties (encoding/context_predict.h).
// Lossy streams (`fuif -Q`): the CLI's quantisation constants and the truncating division of transform/quantize.h:54-71 behind Squeeze.
// With tree_mode 0 (single-leaf trees, what `fuif -I 0` produces) the output is byte-identical to
// the reference encoder's, which pins the arithmetic; tree_mode 1 learns MANIAC trees with the
// writer's OWN greedy top-down learner (bucket-entropy gain on sampled pixels), not the
// reference's two-pass virtual-chance learner (maniac/compound_enc.h), so those files are valid
// FUIF with realistic tree sizes but not byte-identical to the reference's.
// fuifgpu_encode_images_device: the pictures are in device memory and the transformed channels stay there (Chan::resident); the host sees
// three integers per channel (k_channel_stats) and the learner's samples (k_learn_samples_jobs), and writes the same bytes.
// With a palette the colours are collected and the pixels indexed there too (k_palette_collect / k_palette_index): the index plane stays on
// the device like any channel; the palette itself is a table the host sorts, not a plane, and fuifgpu_encode_plane_traffic does not count it.
// Animations (fuifgpu_encode_animation, `fuif frame-%02d.ppm out.fuif`): the frames are one strip under the magic FUAF (encoding.cpp:458-473)
// and, by default, Matching against the previous frame runs between the palettes and Squeeze (fuif.cpp:440-448; transform/2dmatch.h:303-381
// with maxdist = -1); on the GPU routes k_match_frames_runs / _erode / _apply do it.  Only that distance and "off" are offered: from the
// second distance on the reference's back-fill (2dmatch.h:327-329) counts positions, not unmatched samples, and overwrites samples an
// earlier distance matched with an offset that was never compared -- a lossless mode that loses pixels, which is not reproduced.
// Raw YUV 4:2:0 frames (fuifgpu_encode_yuv420, `fuif -y WxH[:b]`; import/read_yuv.h:29-63, fuif.cpp:431-435): three channels of unequal geometry
// under a recorded [YCbCr, ChromaSubsample] pair, no colour transform, no palettes, no Matching; on the GPU routes k_unpack_yuv420 unpacks the
// raw bytes of every frame of a call in one launch.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/fuifgpu.h"
#include "fuifgpu_internal.h"
#include "maniac_encode.h"

namespace fuifgpu {
namespace {

constexpr int CH_ZERO = 0, CH_SIGN = 1, CH_EXP = 2, CH_MANT = 16, CH_N = 31;

inline int ilog2u(uint32_t l) { return l == 0 ? 0 : 31 - __builtin_clz(l); }
inline int slog(int x) {
    if (x == 0) return 0;
    if (x > 0) return 32 - __builtin_clz((unsigned)x);
    return -(32 - __builtin_clz((unsigned)(-x)));
}
inline int iabs(int x) { return x < 0 ? -x : x; }
inline int median3(int a, int b, int c) {
    if (a < b) { if (b < c) return b; return a < c ? c : a; }
    if (a < c) return a;
    return b < c ? c : b;
}

// a device buffer that goes with its owner (move-only)
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() { if (p) fuifgpu_dev_free(p); p = nullptr; }   // (frees are ordered behind the kernels of the null stream)
    bool alloc(size_t bytes) { reset(); p = fuifgpu_dev_alloc(bytes); return p != nullptr; }
    int32_t *i32() const { return static_cast<int32_t *>(p); }
    explicit operator bool() const { return p != nullptr; }
};

// everything of a channel but its samples
struct ChanGeom {
    int w = 0, h = 0, minval = 0, maxval = 0, zero = 0, q = 1;
    int hshift = 0, vshift = 0, hcshift = 0, vcshift = 0, component = -1;
    int64_t zeros = -1;               // device-only channels: the number of zero samples, counted by the statistics launch (channel_ranges)
};
struct Chan : ChanGeom {
    std::vector<int32_t> data;
    mutable DevBuf dev;               // gpu_forward: the samples live here (w x h, contiguous) until every transform has run; gpu_entropy: a device copy of `data` (ensure_dev)
    // device-only: `dev` is set and `data` is empty -- the samples never come to the host (fuifgpu_encode_images_device)
    bool resident() const { return dev && data.empty(); }
    // a channel of the same geometry, ranges and q, without samples
    Chan like() const { Chan g; static_cast<ChanGeom &>(g) = *this; return g; }
    void setzero() { zero = minval > 0 ? minval : (maxval < 0 ? maxval : 0); }
    void minmax() {
        int mn = 0x7FFFFFFF, mx = (int)0x80000001;
        for (int32_t v : data) { if (v < mn) mn = v; if (v > mx) mx = v; }
        minval = mn; maxval = mx;
    }
};

struct Bytes {
    std::vector<uint8_t> b;
    void put(int c) { b.push_back((uint8_t)c); }
    // encoding/encoding.cpp:32-43
    void varint(size_t number, bool done = true) {
        if (number < 128) put((int)(done ? number : number + 128));
        else { size_t lsb = number & 127; varint(number >> 7, false); varint(lsb, done); }
    }
};

// Range encoder matching RacInput24 (maniac/rac.h); carry handling by delayed byte + pending 0xFF run.  `st` is what travels to the GPU
// pixel loop and back (maniac_encode.h)
struct RacEnc {
    Bytes &out;
    RacEncState st{1u << 24, 0, -1, 0};
    explicit RacEnc(Bytes &o) : out(o) {}
    RacEnc(Bytes &o, const RacEncState &behind) : out(o), st(behind) {}
    void shift() {
        uint32_t byte = st.low >> 16;  // bit 8 = carry into the bytes already generated
        if (st.delayed < 0) st.delayed = (int)byte;
        else if (byte < 0xFF) { out.put(st.delayed); for (; st.pending; st.pending--) out.put(0xFF); st.delayed = (int)byte; }
        else if (byte > 0xFF) { out.put(st.delayed + 1); for (; st.pending; st.pending--) out.put(0x00); st.delayed = (int)(byte & 0xFF); }
        else st.pending++;
        st.low = (st.low & 0xFFFF) << 8;
        st.range <<= 8;
    }
    void put(uint32_t chance, int bit) {
        if (bit) { st.low += st.range - chance; st.range = chance; }
        else st.range -= chance;
        while (st.range <= 0x10000u) shift();
    }
    void put12(uint32_t b12, int bit) { put((((st.range & 0xFFFu) * b12 + 0x800u) >> 12) + ((st.range >> 12) * b12), bit); }
    void putbit(int bit) { put(st.range >> 1, bit); }
    // rac_enc.h:87-99: the decoder is three bytes ahead; four generated bytes, the last stays delayed
    void flush() {
        st.low += 0xFFFF;
        for (int k = 0; k < 4; k++) { st.range = 0xFFFF; shift(); }
    }
};

void chance_init(uint16_t *ch, int zero_chance) {  // maniac/symbol.h:115-138
    uint32_t rp = 0x1000 - zero_chance;
    ch[CH_ZERO] = (uint16_t)zero_chance;
    ch[CH_SIGN] = 0x800;
    for (int i = 0; i < kMaxBitDepth - 1; i++) {
        if (rp < 0x100) rp = 0x100;
        if (rp > 0xf00) rp = 0xf00;
        ch[CH_EXP + i] = (uint16_t)(0x1000 - rp);
        rp = (rp * rp + 0x800) >> 12;
    }
    for (int i = 0; i < kMaxBitDepth; i++) ch[CH_MANT + i] = 1024;
}

inline void coder_write(RacEnc &r, uint16_t *ch, int idx, const uint16_t *table, int bit) {
    uint32_t c = ch[idx];
    r.put12(c, bit);
    ch[idx] = table[c * 2 + bit];
}

// write side of maniac/symbol.h:154-185
void write_symbol(RacEnc &r, uint16_t *ch, const uint16_t *table, int min, int max, int value) {
    if (min == max) return;
    if (value == 0) { coder_write(r, ch, CH_ZERO, table, 1); return; }
    coder_write(r, ch, CH_ZERO, table, 0);
    const int sign = value > 0;
    if (min < 0 && max > 0) coder_write(r, ch, CH_SIGN, table, sign);
    const int a = iabs(value);
    const int e = ilog2u((uint32_t)a);
    const int amax = sign ? max : -min;
    const int emax = ilog2u((uint32_t)amax);
    for (int i = 0; i < emax; i++) {
        coder_write(r, ch, CH_EXP + i, table, i == e);
        if (i == e) break;
    }
    int have = 1 << e;
    for (int pos = e; pos > 0;) {
        pos--;
        int minabs1 = have | (1 << pos);
        if (minabs1 > amax) continue;
        int bit = (a >> pos) & 1;
        coder_write(r, ch, CH_MANT + pos, table, bit);
        if (bit) have = minabs1;
    }
}
void write_symbol2(RacEnc &r, uint16_t *ch, const uint16_t *table, int min, int max, int value) {  // symbol.h:235-239
    if (min > 0) write_symbol(r, ch, table, 0, max - min, value - min);
    else if (max < 0) write_symbol(r, ch, table, min - max, 0, value - max);
    else write_symbol(r, ch, table, min, max, value);
}
// write side of maniac/symbol.h:44-57
void uniform_write(RacEnc &r, int min, int len, int value) {
    while (len != 0) {
        int med = len / 2;
        if (value > min + med) { r.putbit(1); min = min + med + 1; len = len - (med + 1); }
        else { r.putbit(0); len = med; }
    }
}

struct Range { int lo, hi; };

struct Image {
    std::vector<Chan> ch;
    int w = 0, h = 0, maxval = 0, nb_channels = 0, nb_meta = 0;
    int nb_frames = 1, den = 10;   // an animation: h = nb_frames frames one above the other; den: frames per second (image.h `den`)
    std::vector<TransformDesc> transforms;
    int downscales[6];
    bool squeezed = false;     // the default Squeeze ran (default_squeeze)
    bool dct_style = false;    // the caller's channels were in a transform domain already (fuifgpu_encode_channels)
    bool stale_tail = false;  // write what the reference's buffer holds behind the last group (StaleTail below); the .yuv route sets it
};

// The reference codes every group compressed first and, when that does not pay, seeks back and writes it again uncompressed
// (encoding.cpp:545-551) -- but its BlobIO never shrinks (fileio.h:236-263: bytes_used is a high-water mark), so where the shorter
// second form of the LAST groups ends before the first one did, the file goes on with the abandoned form's bytes.  No decoder reads
// them.  A .yuv stream ends with its smallest channels (the chroma residuals, or 3 x 2 chroma planes), where this is common, so that
// route reproduces them: `shadow` is the reference's buffer as far as abandoned forms reached.
struct StaleTail {
    std::vector<uint8_t> shadow;
    void abandoned(size_t at, const uint8_t *bytes, size_t n) {
        if (shadow.size() < at + n) shadow.resize(at + n, 0);
        memcpy(shadow.data() + at, bytes, n);
    }
    // what lies behind a stream of `end` bytes
    std::vector<uint8_t> behind(size_t end) const { return end < shadow.size() ? std::vector<uint8_t>(shadow.begin() + end, shadow.end()) : std::vector<uint8_t>(); }
};

// bytes of whole planes / channels the current encode call of this thread has moved (fuifgpu_encode_plane_traffic): every copy of
// channel samples between host and device goes through plane_upload / plane_download
thread_local uint64_t g_plane_h2d = 0, g_plane_d2h = 0;
// what the tree learner of the current encode call has brought to the host (fuifgpu_encode_learn_traffic): sample rows and buckets
// (tree_mode 1 on device-only channels), shortlists and record slices of the level statistics (tree_mode 2)
thread_local uint64_t g_learn_sample_d2h = 0, g_learn_stat_d2h = 0;
int plane_upload(int32_t *dev, const int32_t *host, size_t samples) {
    g_plane_h2d += sizeof(int32_t) * samples;
    return fuifgpu_dev_upload(dev, host, sizeof(int32_t) * samples);
}
int plane_download(int32_t *host, const int32_t *dev, size_t samples) {
    g_plane_d2h += sizeof(int32_t) * samples;
    return fuifgpu_dev_download(host, dev, sizeof(int32_t) * samples);
}

// a device copy of a channel's samples for the GPU pixel loop (kept until the stream is written)
int ensure_dev(const Chan &c) {
    if (c.dev || c.data.empty()) return FUIFGPU_OK;
    if (!c.dev.alloc(sizeof(int32_t) * c.data.size())) return FUIFGPU_E_HIP;
    if (c.hshift < 0) return fuifgpu_dev_upload(c.dev.p, c.data.data(), sizeof(int32_t) * c.data.size());   // a palette is a table, not a plane: not counted
    return plane_upload(c.dev.i32(), c.data.data(), c.data.size());
}

// one k_channel_stats launch over the device planes of `who`: every channel's range and its number of zero samples
int device_ranges(const std::vector<Chan *> &who) {
    std::vector<StatsRec> recs;
    for (const Chan *c : who) recs.push_back(StatsRec{c->dev.i32(), (int64_t)c->w * c->h, 0, 0});
    std::vector<int32_t> stats(3 * recs.size());
    const int rc = channel_stats_gpu(recs.data(), (int)recs.size(), stats.data());
    for (size_t k = 0; k < who.size() && rc == FUIFGPU_OK; k++) { who[k]->minval = stats[3 * k]; who[k]->maxval = stats[3 * k + 1]; who[k]->zeros = stats[3 * k + 2]; }
    return rc;
}

// ---- forward transforms ------------------------------------------------------------------------
int smooth_tendency(int B, int a, int n) {  // transform/squeeze.h:61-77
    int diff = 0;
    if (B >= a && a >= n) {
        diff = (4 * B - 3 * n - a + 6) / 12;
        if (diff - (diff & 1) > 2 * (B - a)) diff = 2 * (B - a) + 1;
        if (diff + (diff & 1) > 2 * (a - n)) diff = 2 * (a - n);
    } else if (B <= a && a <= n) {
        diff = (4 * B - 3 * n - a - 6) / 12;
        if (diff + (diff & 1) < 2 * (B - a)) diff = 2 * (B - a) - 1;
        if (diff - (diff & 1) < 2 * (a - n)) diff = 2 * (a - n);
    }
    return diff;
}

void fwd_ycocg(Image &img) {  // transform/ycocg.h:65-95
    const int m = img.nb_meta;
    Chan &c0 = img.ch[m], &c1 = img.ch[m + 1], &c2 = img.ch[m + 2];
    size_t n = c0.data.size();
    for (size_t i = 0; i < n; i++) {
        int R = c0.data[i], G = c1.data[i], B = c2.data[i];
        c0.data[i] = (((R + B) >> 1) + G) >> 1;
        c1.data[i] = R - B;
        c2.data[i] = G - ((R + B) >> 1);
    }
}

// what one Squeeze step makes of channel `in` (squeeze.h:135-146 / 227-238): the averages and the residuals, no samples yet
void squeeze_geometry(const Chan &in, bool horizontal, Chan &avg, Chan &res) {
    avg = in.like(); res = in.like();
    res.q = 1;
    if (horizontal) {
        avg.w = (in.w + 1) / 2; avg.h = in.h; res.w = in.w - avg.w; res.h = in.h;
        avg.hshift = in.hshift + 1; avg.hcshift = in.hcshift + 1; res.hshift = in.hshift + 1; res.hcshift = in.hcshift;
    } else {
        avg.w = in.w; avg.h = (in.h + 1) / 2; res.w = in.w; res.h = in.h - avg.h;
        avg.vshift = in.vshift + 1; avg.vcshift = in.vcshift + 1; res.vshift = in.vshift + 1; res.vcshift = in.vcshift;
    }
}

// the samples of that step on the host: transform/squeeze.h:147-170 (horizontal) / 239-263 (vertical)
void squeeze_samples_host(const Chan &in, bool horizontal, Chan &avg, Chan &res) {
    avg.data.assign((size_t)avg.w * avg.h, 0); res.data.assign((size_t)res.w * res.h, 0);
    if (horizontal) {
        for (int y = 0; y < in.h; y++) {
            const int32_t *row = &in.data[(size_t)y * in.w];
            for (int x = 0; x < res.w; x++) {
                int A = row[2 * x], B = row[2 * x + 1];
                int a = (A + B + (A > B)) >> 1;
                avg.data[(size_t)y * avg.w + x] = a;
                int next = a;
                if (x + 1 < res.w) next = (row[2 * x + 2] + row[2 * x + 3] + (row[2 * x + 2] > row[2 * x + 3])) >> 1;
                else if (in.w & 1) next = row[2 * x + 2];
                int left = x > 0 ? row[2 * x - 1] : a;
                res.data[(size_t)y * res.w + x] = (A - B) - smooth_tendency(left, a, next);
            }
            if (in.w & 1) avg.data[(size_t)y * avg.w + avg.w - 1] = row[2 * (avg.w - 1)];
        }
    } else {
        const int w = in.w;
        for (int y = 0; y < res.h; y++) {
            for (int x = 0; x < w; x++) {
                int A = in.data[(size_t)(2 * y) * w + x], B = in.data[(size_t)(2 * y + 1) * w + x];
                int a = (A + B + (A > B)) >> 1;
                avg.data[(size_t)y * w + x] = a;
                int next = a;
                if (y + 1 < res.h) {
                    int C = in.data[(size_t)(2 * y + 2) * w + x], D = in.data[(size_t)(2 * y + 3) * w + x];
                    next = (C + D + (C > D)) >> 1;
                } else if (in.h & 1) next = in.data[(size_t)(2 * y + 2) * w + x];
                int top = y > 0 ? in.data[(size_t)(2 * y - 1) * w + x] : a;
                res.data[(size_t)y * w + x] = (A - B) - smooth_tendency(top, a, next);
            }
        }
        if (in.h & 1) for (int x = 0; x < w; x++) avg.data[(size_t)(avg.h - 1) * w + x] = in.data[(size_t)(2 * (avg.h - 1)) * w + x];
    }
}
// ... and on the GPU (fuifgpu_fwd_hsqueeze / fuifgpu_fwd_vsqueeze)
int squeeze_samples_gpu(const Chan &in, bool horizontal, Chan &avg, Chan &res) {
    const bool have = avg.dev.alloc(sizeof(int32_t) * std::max<size_t>((size_t)avg.w * avg.h, 1));
    if (!res.dev.alloc(sizeof(int32_t) * std::max<size_t>((size_t)res.w * res.h, 1)) || !have) return FUIFGPU_E_HIP;
    return horizontal ? fuifgpu_fwd_hsqueeze(in.dev.i32(), in.w, in.h, avg.dev.i32(), res.dev.i32(), nullptr)
                      : fuifgpu_fwd_vsqueeze(in.dev.i32(), in.w, in.h, avg.dev.i32(), res.dev.i32(), nullptr);
}
// one Squeeze step of channel c: the averages take its place, the residuals go to position rc; the input, samples and device plane, goes
// right behind the step
int fwd_squeeze_one(Image &img, int c, int rc, bool horizontal, bool on_gpu) {
    const Chan in = std::move(img.ch[c]);
    Chan avg, res;
    squeeze_geometry(in, horizontal, avg, res);
    int err = FUIFGPU_OK;
    if (on_gpu) err = squeeze_samples_gpu(in, horizontal, avg, res);
    else squeeze_samples_host(in, horizontal, avg, res);
    img.ch[c] = std::move(avg);
    img.ch.insert(img.ch.begin() + rc, std::move(res));
    return err;
}

std::vector<int> default_squeeze_params(const Image &img) {  // transform/squeeze.h:266-321
    std::vector<int> p;
    int nb = img.nb_channels, m = img.nb_meta;
    int w = img.ch[m].w, h = img.ch[m].h;
    bool wide = w > h;
    if (nb > 2 && img.ch[m + 1].w == w && img.ch[m + 1].h == h) {
        p.insert(p.end(), {3, m + 1, m + 2});
        p.insert(p.end(), {2, m + 1, m + 2});
    }
    if (!wide && h > 8) { p.insert(p.end(), {0, m, m + nb - 1}); h = (h + 1) / 2; }
    while (w > 8 || h > 8) {
        if (w > 8) { p.insert(p.end(), {1, m, m + nb - 1}); w = (w + 1) / 2; }
        if (h > 8) { p.insert(p.end(), {0, m, m + nb - 1}); h = (h + 1) / 2; }
    }
    return p;
}

int fwd_squeeze(Image &img, const std::vector<int> &params, bool on_gpu) {  // transform/squeeze.h:389-408
    for (size_t i = 0; i + 2 < params.size(); i += 3) {
        bool horizontal = params[i] & 1;
        bool in_place = !(params[i] & 2);
        int beginc = params[i + 1], endc = params[i + 2];
        int offset = in_place ? endc + 1 : img.nb_meta + img.nb_channels;
        for (int c = beginc; c <= endc; c++) {
            const int rc = fwd_squeeze_one(img, c, offset + c - beginc, horizontal, on_gpu);
            if (rc != FUIFGPU_OK) return rc;
        }
    }
    return FUIFGPU_OK;
}
// fuif.cpp:450-455, 576-578: the default Squeeze, unless channel[0] -- the match channel or a palette, once there is one -- is too small
int default_squeeze(Image &img, bool on_gpu) {
    if ((int64_t)img.ch[0].w * img.ch[0].h <= 20) return FUIFGPU_OK;
    const int rc = fwd_squeeze(img, default_squeeze_params(img), on_gpu);
    img.transforms.push_back({TR_SQUEEZE, {}});  // empty parameter list = "default" in the stream
    img.squeezed = true;
    return rc;
}

// ---- forward Palette (transform/palette.h:92-142) and the three options of the CLI that try it (fuif.cpp:374-430) -----------------
// colors: -K, the whole-picture palette; post / pre: -X / -Y as the CLI holds them, a float fraction of a channel's range (0.01 * percent,
// computed in double and stored to float like `channel_colors = 0.01*atof(optarg)`); 0 = off
struct PaletteOpts {
    int colors = 0;
    float post = 0.f, pre = 0.f;
};
// a tuple as one integer whose order is the order of std::set<std::vector<pixel_type>>: component 0 most significant, signed
inline uint64_t tuple_order_key(const Chan *chans, int nb, size_t i) {
    uint64_t k = 0;
    for (int c = 0; c < nb; c++) k = (k << 16) | (uint16_t)(chans[c].data[i] + 32768);
    return k;
}
// the host's collect + index: `rows` gets the palette (row c = component c, colours in the reference's order) and channel `chans[0]` the
// indices; false (nothing touched) with more than `limit` colours
bool fwd_palette_host(Chan *chans, int nb, int limit, std::vector<int32_t> &rows, int &n_colors) {
    const size_t n = chans[0].data.size();
    std::vector<uint64_t> keys;   // the distinct tuples, kept sorted; a run of equal pixels costs one comparison each
    uint64_t last = 0;
    bool have = false;
    for (size_t i = 0; i < n; i++) {
        const uint64_t k = tuple_order_key(chans, nb, i);
        if (have && k == last) continue;
        last = k; have = true;
        auto at = std::lower_bound(keys.begin(), keys.end(), k);
        if (at != keys.end() && *at == k) continue;
        if (keys.size() >= (size_t)limit) return false;   // palette.h:109: one more than the limit
        keys.insert(at, k);
    }
    n_colors = (int)keys.size();
    rows.assign((size_t)n_colors * nb, 0);
    for (int k = 0; k < n_colors; k++)
        for (int c = 0; c < nb; c++) rows[(size_t)c * n_colors + k] = (int32_t)((keys[(size_t)k] >> (16 * (nb - 1 - c))) & 0xFFFF) - 32768;
    have = false;
    int32_t last_index = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t k = tuple_order_key(chans, nb, i);
        if (!have || k != last) { last_index = (int32_t)(std::lower_bound(keys.begin(), keys.end(), k) - keys.begin()); last = k; have = true; }
        chans[0].data[i] = last_index;
    }
    return true;
}
// Image::do_transform of one Palette attempt over channels begin..end (numbered from the first non-meta channel) with at most `limit`
// colours: on success the index replaces channel `begin`, the others go (with their device planes), the palette (colours x nb, hshift -1)
// goes in FRONT of the channel list and the transform is recorded with the number of colours found; on failure nothing changes and nothing
// is recorded.  on_gpu: the samples are on the device (Chan::dev); the palette itself is a small table and lives on the host either way
int try_palette(Image &img, int begin, int end, int limit, bool on_gpu) {
    const int bc = img.nb_meta + begin, nb = end - begin + 1;
    if (limit < 1 || nb < 1 || !img.ch[bc].w || !img.ch[bc].h) return FUIFGPU_OK;   // (the first pixel is already one colour too many)
    std::vector<int32_t> rows;
    int n_colors = -1;
    if (on_gpu) {
        const int32_t *planes[4] = {nullptr, nullptr, nullptr, nullptr};
        if (nb > 4) return FUIFGPU_E_ARG;
        for (int c = 0; c < nb; c++) planes[c] = img.ch[bc + c].dev.i32();
        const int rc = fwd_palette_gpu(planes, nb, (int64_t)img.ch[bc].w * img.ch[bc].h, limit, img.ch[bc].dev.i32(), rows, &n_colors);
        if (rc != FUIFGPU_OK) return rc;
    } else if (!fwd_palette_host(&img.ch[bc], nb, limit, rows, n_colors)) n_colors = -1;
    if (n_colors < 0) return FUIFGPU_OK;
    img.ch.erase(img.ch.begin() + bc + 1, img.ch.begin() + bc + nb);
    Chan pal;   // Channel pch(nb_colors, nb, 0, 1); pch.hshift = -1
    pal.w = n_colors; pal.h = nb; pal.minval = 0; pal.maxval = 1; pal.hshift = -1;
    pal.data = std::move(rows);
    img.ch.insert(img.ch.begin(), std::move(pal));
    img.nb_meta++;
    img.nb_channels -= nb - 1;
    img.transforms.push_back({TR_PALETTE, {begin, end, n_colors}});
    return FUIFGPU_OK;
}
// Image::recompute_minmax for the channels the compaction heuristic looks at (the non-meta ones): host scan, or one k_channel_stats launch
int current_ranges(Image &img, bool on_gpu) {
    if (!on_gpu) { for (int i = img.nb_meta; i < (int)img.ch.size(); i++) img.ch[i].minmax(); return FUIFGPU_OK; }
    std::vector<Chan *> who;
    for (int i = img.nb_meta; i < (int)img.ch.size(); i++) who.push_back(&img.ch[i]);
    return device_ranges(who);
}
// fuif.cpp:374-388 (pre: before the colour transform, ranges of 256 values and more only) and :418-430 (after it): every channel whose
// samples use less than `fraction` of its range is compacted to the ranks of the values that occur
int compact_channels(Image &img, float fraction, bool pre, bool on_gpu) {
    int rc = current_ranges(img, on_gpu);
    for (int i = 0; i < img.nb_channels && rc == FUIFGPU_OK; i++) {
        const Chan &c = img.ch[img.nb_meta + i];
        const int colors = c.maxval - c.minval + 1;
        if (pre && colors < 256) continue;
        rc = try_palette(img, i, i, (int)(fraction * colors), on_gpu);
    }
    return rc;
}

// ---- animations: forward Matching against the previous frame (transform/2dmatch.h:245-262, 303-381 with maxdist = -1) -------------
struct AnimOpts {
    int nb_frames = 1, den = 10;
    bool match = true;
};
// the host's form is the reference's loop nest as it stands, in-place erode included (the kernels' data-parallel form is checked against it)
void fwd_match_frames_host(Chan *chans, int nb, int fh, Chan &m) {
    const int w = m.w, h = m.h;
    const int minmatchcount = std::max(5, std::min(40, w / 50));
    auto M = [&](int y, int x) -> int32_t & { return m.data[(size_t)y * w + x]; };
    for (int y = fh; y < h; y++) {
        int matchcount = 0;
        bool firstmatch = true;
        for (int x = 0; x < w; x++) {
            bool nomatch = false;
            for (int c = 0; c < nb; c++) nomatch |= chans[c].data[(size_t)y * w + x] != chans[c].data[(size_t)(y - fh) * w + x];
            if (nomatch) { matchcount = 0; firstmatch = true; continue; }
            matchcount++;
            if (matchcount >= minmatchcount) {
                if (firstmatch) for (int prev_x = x - matchcount + 1; prev_x < x; prev_x++) M(y, prev_x) = 1;
                firstmatch = false;
                M(y, x) = 1;
            }
        }
    }
    for (int it = 0; it < 3; it++)   // 2dmatch.h:355-369
        for (int y = fh; y < h; y++)
            for (int x = 0; x < w; x++)
                if (M(y, x) > 0 && (M(y - 1, x) == 0 || (x > 0 && M(y, x - 1) == 0) || (y + 1 < h && M(y + 1, x) <= 0) || (x + 1 < w && M(y, x + 1) <= 0)))
                    M(y, x) = -M(y, x);
    for (int y = fh; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (M(y, x) > 0) for (int c = 0; c < nb; c++) chans[c].data[(size_t)y * w + x] = 0;
            else if (M(y, x) < 0) M(y, x) *= -1;
        }
}
// Image::do_transform of the Matching: the meta-channel goes in FRONT of the channel list (meta_match, 2dmatch.h:191-193), the transform is
// recorded without parameters (:256: channels 0..nb_channels-1, no soft match)
int fwd_match_frames(Image &img, bool on_gpu) {
    const int bc = img.nb_meta, nb = img.nb_channels;
    if (nb > 8) return FUIFGPU_E_ARG;
    Chan m;   // Channel mch(w, h, 0, 1)
    m.w = img.ch[bc].w; m.h = img.ch[bc].h; m.minval = 0; m.maxval = 1;
    const int fh = m.h / img.nb_frames;
    m.q = 2 * fh * fh + (fh & 1);   // the code of the offset "exactly one frame up" (:310)
    int rc = FUIFGPU_OK;
    if (on_gpu) {
        const int32_t *planes[8];
        for (int c = 0; c < nb; c++) planes[c] = img.ch[bc + c].dev.i32();
        rc = m.dev.alloc(sizeof(int32_t) * (size_t)m.w * m.h) ? fuifgpu_fwd_match_frames(planes, nb, m.w, m.h, img.nb_frames, m.dev.i32(), nullptr) : FUIFGPU_E_HIP;
    } else {
        m.data.assign((size_t)m.w * m.h, 0);
        fwd_match_frames_host(&img.ch[bc], nb, fh, m);
    }
    img.ch.insert(img.ch.begin(), std::move(m));
    img.nb_meta++;
    img.transforms.push_back({TR_2DMATCH, {}});
    return rc;
}

// ---- lossy: the CLI's quantisation constants for Squeeze channels (fuif.cpp:459-503) ---------------------------------------------
// Everything below is float arithmetic whose roundings decide an integer: the variables are floats initialised from double literals,
// the quality mapping is evaluated in double and stored to float, the products run left to right in float (no contraction: the
// library is built with -ffp-contract=off and without -ffast-math).
struct Lossy {
    bool active = false;               // fuif.cpp:459: quality < 100 || cquality < 100
    float quality = 100.f, cquality = 100.f;
    bool yuv = false;                  // .yuv input (image_type == 2): the two factors of fuif.cpp:432-434
};
const float squeeze_quality_factor = 0.3, squeeze_luma_factor = 1.2;   // fuif.cpp:70-71
// fuif.cpp:432-434, "make chroma more important" for .yuv input: `squeeze_luma_factor *= 3.0; squeeze_quality_factor /= 3.0;` -- the float
// variables above, each updated through a double expression and stored back to float
const float yuv_squeeze_quality_factor = (float)((double)squeeze_quality_factor / 3.0), yuv_squeeze_luma_factor = (float)((double)squeeze_luma_factor * 3.0);
const float squeeze_luma_qtable[16] = {163.84, 81.92, 40.96, 20.48, 10.24, 5.12, 2.56, 1.28, 0.64, 0.32, 0.16, 0.08, 0.04, 0.02, 0.01, 0.005};   // fuif.cpp:74
const float squeeze_chroma_qtable[16] = {1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1, 0.5, 0.5, 0.5, 0.5, 0.5};                                  // fuif.cpp:76

// -Q's number -> the factor on the tables (fuif.cpp:461-477); squeeze_option: the OPTION ("responsive"), not whether Squeeze ran
float quality_to_scale(float x, bool squeeze_option) {
    if (!squeeze_option) x = (400 + x) / 5;
    if (x > 50) x = 200.0 - x * 2.0;
    else x = 900.0 - x * 16.0;
    x *= 0.01f;
    return x;
}
int quantization_constant(const Lossy &l, bool squeeze_option, bool chroma_table, int shift) {  // fuif.cpp:492-500
    if (shift > 15) shift = 15;
    int q;
    const float quality_factor = l.yuv ? yuv_squeeze_quality_factor : squeeze_quality_factor, luma_factor = l.yuv ? yuv_squeeze_luma_factor : squeeze_luma_factor;
    if (chroma_table) q = (int)(quality_to_scale(l.cquality, squeeze_option) * quality_factor * squeeze_chroma_qtable[shift]);
    else q = (int)(quality_to_scale(l.quality, squeeze_option) * quality_factor * luma_factor * squeeze_luma_qtable[shift]);
    return q < 1 ? 1 : q;
}
// the caller's two numbers -> Lossy; false: NaN, negative, or a quality above 100 (only the chroma quality may be: "same as quality", fuif.cpp:247)
bool read_qualities(float quality, float chroma_quality, Lossy &l) {
    if (!(quality >= 0.f && quality <= 100.f) || !(chroma_quality >= 0.f)) return false;
    l.quality = quality;
    l.cquality = chroma_quality > 100.f ? quality : chroma_quality;
    l.active = l.quality < 100.f || l.cquality < 100.f;
    return true;
}

// transform/quantize.h:54-71 over every channel with the constants above; the ranges are recomputed from the samples when the stream
// is written (encoding.cpp:737-739).  on_gpu: the samples are on the device (Chan::dev) -- one launch divides every channel and
// finds its range, one copy brings the ranges back, and only channels that are not all zero are downloaded afterwards.
int fwd_quantize(Image &img, const Lossy &l, bool squeeze_option, bool colour_option, bool on_gpu, std::vector<char> &all_zero) {
    const int n = (int)img.ch.size();
    all_zero.assign((size_t)n, 0);
    for (int i = img.nb_meta; i < n; i++) {
        Chan &c = img.ch[i];
        c.q = quantization_constant(l, squeeze_option, colour_option && c.component > 0 && c.component < 3, c.hcshift + c.vcshift);
        if (!on_gpu) for (int32_t &v : c.data) v = v / c.q;
    }
    img.transforms.push_back({TR_QUANTIZE, {}});   // no parameters in the stream: Transform::has_parameters() (transform.h:85)
    if (!on_gpu) return FUIFGPU_OK;
    std::vector<QuantChan> table;
    for (int i = img.nb_meta; i < n; i++) {
        Chan &c = img.ch[i];
        table.push_back(QuantChan{c.dev.i32(), (int64_t)c.w * c.h, c.q, (int32_t)table.size(), 0, 0});
    }
    std::vector<int32_t> minmax(2 * table.size());
    const int rc = fwd_quantize_channels_gpu(table.data(), (int)table.size(), minmax.data());
    if (rc != FUIFGPU_OK) return rc;
    for (size_t k = 0; k < table.size(); k++) all_zero[(size_t)img.nb_meta + k] = minmax[2 * k] == 0 && minmax[2 * k + 1] == 0;
    return FUIFGPU_OK;
}

void recompute_downscales(Image &img) {  // image/image.cpp:124-136, RESPONSIVE_SIZE(n) = 32>>n
    int n = (int)img.ch.size();
    img.downscales[0] = img.nb_meta + img.nb_channels - 1;
    for (int s = 1; s < 6; s++) {
        img.downscales[s] = n - 1;
        int rs = 32 >> s;
        for (int k = img.downscales[s - 1]; k < n; k++) {
            if ((1 << img.ch[k].hcshift) < rs || (1 << img.ch[k].vcshift) < rs) break;
            if ((1 << img.ch[k].hcshift) == rs && (1 << img.ch[k].vcshift) == rs) img.downscales[s] = k;
        }
    }
}

// ---- context model (same arithmetic as the decoder) --------------------------------------------
struct RefInfo { const Chan *c; };

int init_properties(std::vector<Range> &pr, std::vector<RefInfo> &refs, const Image &img, int beginc, int endc, int max_properties) {
    pr.clear(); refs.clear();
    int offset = 0;
    for (int j = beginc - 1; j >= 0 && offset < max_properties; j--) {  // context_predict.h:69-82
        const Chan &c = img.ch[j];
        if (c.minval == c.maxval) continue;
        if (c.hshift < 0) continue;
        int mn = c.minval > 0 ? 0 : c.minval, mx = c.maxval < 0 ? 0 : c.maxval;
        pr.push_back({0, iabs(mx > -mn ? mx : mn)});
        pr.push_back({slog(mn), slog(mx)});
        offset += 2;
        refs.push_back({&c});
    }
    int mn = 0x7FFFFFFF, mx = (int)0x80000001, maxh = 0, maxw = 0;
    for (int j = beginc; j <= endc; j++) {
        const Chan &c = img.ch[j];
        mn = std::min(mn, c.minval); mx = std::max(mx, c.maxval); maxh = std::max(maxh, c.h); maxw = std::max(maxw, c.w);
    }
    if (mn > 0) mn = 0;
    if (mx < 0) mx = 0;
    int amax = std::max(iabs(mn), iabs(mx));
    pr.push_back({0, amax}); pr.push_back({0, amax});
    pr.push_back({slog(mn), slog(mx)}); pr.push_back({slog(mn), slog(mx)});
    pr.push_back({0, maxh - 1}); pr.push_back({0, maxw - 1});
    pr.push_back({mn + mn - mx, mx + mx - mn}); pr.push_back({mn + mn - mx, mx + mx - mn});
    for (int k = 0; k < 5; k++) pr.push_back({slog(mn - mx), slog(mx - mn)});
    return (int)pr.size();
}

// properties + prediction of pixel (x,y): context_predict.h:124-168 and :233-289 (per-pixel form)
inline int props_and_guess(int32_t *p, const Chan &c, const std::vector<RefInfo> &refs, int x, int y, int predictor) {
    int o = 0;
    for (const RefInfo &r : refs) {
        const Chan &rc = *r.c;
        int ry = (y << c.vshift) >> rc.vshift; if (ry >= rc.h) ry = rc.h - 1;
        // a palette (hshift -1) coded behind the match channel: the reference's step size is (1 << rc.hshift) >> -1, 0 on its x86 build,
        // and every sample reads the reference row's last sample (context_predict.h:248-276)
        int rx = c.hshift < 0 ? rc.w - 1 : (x << c.hshift) >> rc.hshift; if (rx >= rc.w) rx = rc.w - 1;
        int v = rc.data[(size_t)ry * rc.w + rx];
        p[o++] = iabs(v); p[o++] = slog(v);
    }
    const int32_t *d = c.data.data();
    const int w = c.w;
    int left = x ? d[(size_t)y * w + x - 1] : c.zero;
    int top = y ? d[(size_t)(y - 1) * w + x] : c.zero;
    int topleft = (x && y) ? d[(size_t)(y - 1) * w + x - 1] : left;
    int topright = (x + 1 < w && y) ? d[(size_t)(y - 1) * w + x + 1] : top;
    int leftleft = x > 1 ? d[(size_t)y * w + x - 2] : left;
    int toptop = y > 1 ? d[(size_t)(y - 2) * w + x] : top;
    p[o++] = iabs(top); p[o++] = iabs(left); p[o++] = slog(top); p[o++] = slog(left);
    p[o++] = y; p[o++] = x;
    p[o++] = left + top - topleft; p[o++] = topleft + topright - top;
    p[o++] = slog(left - topleft); p[o++] = slog(topleft - top); p[o++] = slog(top - topright);
    p[o++] = slog(top - toptop); p[o++] = slog(left - leftleft);
    switch (predictor) {
        case 0: return c.zero;
        case 1: return (left + top) / 2;
        case 2: return median3((int16_t)(left + top - topleft), left, top);   // :160 narrows the gradient to pixel_type (the property above stays an int)
        case 3: return left;
        case 4: return top;
        case 5: return (left + topleft + top + topright) / 4;
        case 6: { int t = left + top - topleft; return t < c.minval ? c.minval : (t > c.maxval ? c.maxval : t); }
        default: return median3((int16_t)(left + top - topleft), left, top);
    }
}

// ---- one group (encoding/encoding.cpp:74-207 for a single-channel group), step by step ---------------------------------------------
// The tree learner is csrc/tree_learn.h: Learner, the recursive host learner of tree_mode 1, and learn_levelwise, the level-wise one of
// tree_mode 2 whose statistics come from the kernels of maniac_encode.hip.

// what the groups of a call are coded with: the two chance transition tables, the options that bear on a group, and where the learner's
// input comes from when it is not the channel's own samples
struct GroupCoder {
    std::vector<uint16_t> tables;   // the tree coder's table, then the pixel coder's
    const uint16_t *tree_table, *pixel_table;
    int max_properties, tree_mode, max_tree_nodes, split_bits;
    bool gpu_entropy = false;       // write_stream: the pixel loop of compressed groups runs in maniac_encode.hip
    EncScratch *scratch = nullptr;  // its device buffers, reused from group to group
    // device-only channels: the learner's samples of the picture's groups as k_learn_samples_jobs computed them, sample_job[channel] = job or -1
    const LearnSamples *samples = nullptr;
    const std::vector<int> *sample_job = nullptr;
    // tree_mode 2: the trees of the picture's groups as the level-wise learner left them (learn_trees_device), learned[channel]; a channel
    // that learns nothing has no entry
    const std::vector<std::vector<LearnNode>> *learned = nullptr;
    explicit GroupCoder(const fuifgpu_encode_options &o)
        : tables(16384), tree_table(tables.data()), pixel_table(tables.data() + 8192), max_properties(o.max_properties), tree_mode(o.tree_mode),
          max_tree_nodes(o.max_tree_nodes), split_bits(o.split_bits > 0 ? o.split_bits : 0) {
        build_chance_table(tables.data(), 0xFFFFFFFFu / 19, 2);
        build_chance_table(tables.data() + 8192, 0x0d000000u, 6);
    }
    GroupCoder(const GroupCoder &) = delete;
};

// what the learner samples of a group: every stride-th pixel, none for small groups or fixed trees
struct LearnPlan {
    size_t stride = 0, n_samples = 0;   // stride 0: no learned tree
    int max_depth = 14, min_leaf = 48;
};
LearnPlan plan_learner(const Chan &c, int tree_mode, int max_tree_nodes) {
    LearnPlan lp;
    const size_t npix = (size_t)c.w * c.h;
    if ((tree_mode != 1 && tree_mode != 2) || npix < 4096) return lp;   // 2: learned exactly as 1, the statistics on the GPU
    // sample pixels on a coprime stride so every row/column phase is seen
    size_t target = 60000;
    if (max_tree_nodes > 4095) {
        // a caller who lifts the node cap above the default wants trees of that size (the reference encoder's reach 19 000 nodes
        // with `-I 16`; the format allows 65 535, compound.h:46): 60 000 samples in leaves of >= 48 stop near 2 500 nodes, so the
        // sample, the depth and the smallest leaf scale with the cap.  The default cap keeps the default rule and its bytes.
        target = (size_t)max_tree_nodes * 16;
        lp.max_depth = 40; lp.min_leaf = 6;
    }
    lp.stride = std::max<size_t>(1, npix / target);
    if (lp.stride > 1 && lp.stride % 2 == 0) lp.stride++;
    lp.n_samples = (npix + lp.stride - 1) / lp.stride;
    return lp;
}

// the group as the GPU pixel loop sees it: device copies of its plane and of its reference channels
int build_enc_group(const Chan &c, const std::vector<RefInfo> &refs, int predictor, EncGroup &g) {
    int rc = ensure_dev(c);
    g = EncGroup{};
    g.w = c.w; g.h = c.h; g.hshift = c.hshift; g.vshift = c.vshift;
    g.minval = c.minval; g.maxval = c.maxval; g.zero = c.zero; g.predictor = predictor;
    g.nrefs = (int)refs.size();
    if (g.nrefs > kMaxRefs) rc = FUIFGPU_E_ARG;
    for (int k = 0; k < g.nrefs && rc == FUIFGPU_OK; k++) {
        const Chan &r = *refs[k].c;
        rc = ensure_dev(r);
        g.refs[k] = EncRef{r.dev.i32(), r.w, r.h, r.hshift, r.vshift};
    }
    g.plane = c.dev.i32();
    return rc;
}

// a group in its compressed form as far as it is coded: header, zero chance, tree and (behind a pixel coder) the pixels; `state` is the
// coder behind the last of them, not flushed
struct CodedGroup {
    Bytes bytes;
    size_t header_len = 0;
    bool trivial = false;           // minval == maxval: the header is all there is, no coder runs
    RacEncState state{};
};
// ... and what the pixel coders need besides: the context model, the tree in the decoder's layout, the chances every leaf starts with
struct GroupDraft {
    CodedGroup coded;
    std::vector<Range> ranges;
    std::vector<RefInfo> refs;
    int nprops = 0;
    std::vector<EncNode> tree;
    std::vector<uint16_t> leaves;   // n_leaves x CH_N
    int n_leaves() const { return ((int)tree.size() + 1) / 2; }
};

// the group header (encoding.cpp:529-540): predictor and compress bit, the channel's range, its q unless the channel is all zero
void group_header(Bytes &io, Chan &c, int predictor, bool compress) {
    io.varint((size_t)((0 << 4) + (predictor << 1) + (compress ? 1 : 0)));
    if (c.minval <= 0) io.varint((size_t)(1 - c.minval));
    else { io.varint(0); io.varint((size_t)c.minval); }
    io.varint((size_t)(c.maxval - c.minval));
    if (!(c.minval == 0 && c.maxval == 0)) io.varint((size_t)c.q);
    c.setzero();
}

// the group in its uncompressed form: the header and, unless the channel is trivial, every sample in a uniform code of its own coder.
// A device-only channel comes to the host for this one loop
int write_uncompressed(Bytes &io, Chan &c, int predictor) {
    group_header(io, c, predictor, false);
    if (c.minval == c.maxval) return FUIFGPU_OK;
    int rc = FUIFGPU_OK;
    std::vector<int32_t> fetched;
    if (c.resident()) {
        fetched.resize((size_t)c.w * c.h);
        rc = plane_download(fetched.data(), c.dev.i32(), fetched.size());
    }
    RacEnc rac(io);
    for (int32_t v : c.resident() ? fetched : c.data) uniform_write(rac, c.minval, c.maxval - c.minval, v);
    rac.flush();
    return rc;
}

// the tree of a group: learned from the host samples, from the rows k_learn_samples_jobs computed (device-only channels), or taken from
// the level-wise learner's result (tree_mode 2); a single node in L.nodes where nothing is learned
int group_tree(const Image &img, int ci, int predictor, const GroupCoder &gc, const GroupDraft &d, Learner &L) {
    const Chan &c = img.ch[ci];
    L.nodes.assign(1, Learner::LNode());
    const LearnPlan lp = plan_learner(c, gc.tree_mode, gc.max_tree_nodes);
    if (!lp.stride) return FUIFGPU_OK;
    L.max_depth = lp.max_depth; L.min_leaf = lp.min_leaf;
    L.nprops = d.nprops; L.scale = (double)lp.stride; L.max_nodes = gc.max_tree_nodes;
    L.threshold_bits = (double)gc.split_bits;
    if (gc.tree_mode == 2) {   // learned before the pictures' groups were written, all groups of the call in the same rounds
        if (!gc.learned || (size_t)ci >= gc.learned->size() || (*gc.learned)[(size_t)ci].empty()) return FUIFGPU_E_HIP;   // (no host route behind it)
        L.nodes = (*gc.learned)[(size_t)ci];
        return FUIFGPU_OK;
    }
    if (c.resident()) {   // the same rows, in the same order, from the device
        const int job = gc.samples && gc.sample_job ? (*gc.sample_job)[(size_t)ci] : -1;
        if (job < 0) return FUIFGPU_E_HIP;
        L.props.assign(gc.samples->props((size_t)job), gc.samples->props((size_t)job) + lp.n_samples * (size_t)d.nprops);
        L.bucket.assign(gc.samples->bucket((size_t)job), gc.samples->bucket((size_t)job) + lp.n_samples);
    } else {
        std::vector<int32_t> props(d.nprops);
        const size_t npix = (size_t)c.w * c.h;
        for (size_t i = 0; i < npix; i += lp.stride) {
            int y = (int)(i / c.w), x = (int)(i % c.w);
            int guess = props_and_guess(props.data(), c, d.refs, x, y, predictor);
            int diff = c.data[i] - guess;
            L.props.insert(L.props.end(), props.begin(), props.end());
            L.bucket.push_back((uint8_t)(diff == 0 ? 0 : ilog2u((uint32_t)iabs(diff)) + 1));
        }
    }
    std::vector<int> idx(L.bucket.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (int)i;
    L.build(idx, 0, (int)idx.size(), 0, 0);
    return FUIFGPU_OK;
}

// serialise a learned tree in pre-order (write side of compound.h:277-308) and build the
// decoder-layout node array (children appended pairwise when the parent is parsed)
void write_tree(RacEnc &rac, const Learner *L, std::vector<Range> ranges, const uint16_t *table, std::vector<EncNode> &out) {
    uint16_t ctx[3][CH_N];
    for (int k = 0; k < 3; k++) chance_init(ctx[k], 1024);
    const int nprops = (int)ranges.size();
    static constexpr EncNode leaf_node{-1, 0, 0, 0};
    out.assign(1, leaf_node);
    struct Rec {
        RacEnc &rac; const Learner *L; std::vector<Range> &rg; const uint16_t *table; std::vector<EncNode> &out; uint16_t (*ctx)[CH_N]; int nprops;
        void go(int lnode, int pos) {
            int p = (L && lnode >= 0) ? L->nodes[lnode].prop : -1;
            write_symbol2(rac, ctx[0], table, 0, nprops, p + 1);
            out[pos].prop = p;
            if (p < 0) return;
            int oldmin = rg[p].lo, oldmax = rg[p].hi;
            int s = L->nodes[lnode].split;
            write_symbol2(rac, ctx[2], table, oldmin, oldmax - 1, s);
            out[pos].split = s;
            int child = (int)out.size();
            out[pos].child = child;
            out.push_back(leaf_node); out.push_back(leaf_node);
            rg[p].lo = s + 1;
            go(L->nodes[lnode].gt, child);
            rg[p].lo = oldmin; rg[p].hi = s;
            go(L->nodes[lnode].le, child + 1);
            rg[p].hi = oldmax;
        }
    } rec{rac, L, ranges, table, out, ctx, nprops};
    rec.go(L ? 0 : -1, 0);
    int leaf = 0;
    for (auto &n : out) if (n.prop < 0) n.leaf = leaf++;
}

// the prefix of a group's compressed form: header, zero chance ("predictability" of a predictor-0 group), tree; d.leaves gets the chances
// of every leaf and d.coded.state the coder behind the tree.  A trivial channel has its header only
int group_prefix(Image &img, int ci, int predictor, const GroupCoder &gc, GroupDraft &d) {
    Chan &c = img.ch[ci];
    Bytes &io = d.coded.bytes;
    group_header(io, c, predictor, true);
    d.coded.header_len = io.b.size();
    d.coded.trivial = c.minval == c.maxval;
    if (d.coded.trivial) return FUIFGPU_OK;   // no RAC stream
    d.nprops = init_properties(d.ranges, d.refs, img, ci, ci, gc.max_properties);
    int predictability = 2048;
    if (predictor == 0) {
        uint64_t zeroes = 0, pixels = (uint64_t)c.w * c.h;
        if (c.resident()) zeroes = (uint64_t)c.zeros;
        else for (int32_t v : c.data) zeroes += (v == 0);
        int rounded = (int)(zeroes * 128 / pixels);
        rounded = std::max(1, std::min(127, rounded));
        io.varint((size_t)rounded);
        predictability = rounded * 32;
    }
    Learner L;
    const int rc = group_tree(img, ci, predictor, gc, d, L);
    if (rc != FUIFGPU_OK) return rc;
    RacEnc rac(io);
    write_tree(rac, L.nodes.size() > 1 ? &L : nullptr, d.ranges, gc.tree_table, d.tree);
    d.leaves.resize((size_t)d.n_leaves() * CH_N);
    chance_init(d.leaves.data(), predictability);
    for (int l = 1; l < d.n_leaves(); l++) memcpy(&d.leaves[(size_t)l * CH_N], d.leaves.data(), sizeof(uint16_t) * CH_N);
    d.coded.state = rac.st;
    return FUIFGPU_OK;
}

// the pixels of a group behind its prefix, three ways.  1: the host loop
void code_pixels_host(const Chan &c, int predictor, const GroupCoder &gc, GroupDraft &d) {
    RacEnc rac(d.coded.bytes, d.coded.state);
    const std::vector<EncNode> &tree = d.tree;
    if (tree.size() == 1 && predictor == 0 && c.zero == 0) {
        for (int32_t v : c.data) write_symbol(rac, d.leaves.data(), gc.pixel_table, c.minval, c.maxval, v);  // fast track
    } else {
        std::vector<int32_t> props(d.nprops);
        for (int y = 0; y < c.h; y++)
            for (int x = 0; x < c.w; x++) {
                int guess = props_and_guess(props.data(), c, d.refs, x, y, predictor);
                int mn = c.minval - guess, mx = c.maxval - guess;
                if (mn == mx) continue;
                int pos = 0;
                while (tree[pos].prop >= 0) pos = (props[tree[pos].prop] > tree[pos].split) ? tree[pos].child : tree[pos].child + 1;
                write_symbol(rac, &d.leaves[(size_t)tree[pos].leaf * CH_N], gc.pixel_table, mn, mx, c.data[(size_t)y * c.w + x] - guess);
            }
    }
    d.coded.state = rac.st;
}
// 2: every sample is known, so the context model of all pixels runs in parallel and one wavefront then codes them in order into THIS
// range coder (its state goes to the device and comes back; the tree is already in it)
int code_pixels_gpu(const Chan &c, int predictor, const GroupCoder &gc, GroupDraft &d) {
    EncGroup g{};
    const int rc = build_enc_group(c, d.refs, predictor, g);
    if (rc != FUIFGPU_OK) return rc;
    return maniac_encode_group_gpu(g, d.tree.data(), (int)d.tree.size(), d.n_leaves(), d.leaves.data(), gc.pixel_table, &d.coded.state, d.coded.bytes.b, *gc.scratch);
}
// 3: a job of maniac_encode_jobs_gpu, which codes the groups of a whole batch in one launch pair (the caller takes job.body and job.state back)
int make_enc_job(const Chan &c, int predictor, GroupDraft &d, EncJob &job) {
    const int rc = build_enc_group(c, d.refs, predictor, job.g);
    job.n_leaves = d.n_leaves();
    job.tree = std::move(d.tree);
    memcpy(job.leaf_init, d.leaves.data(), sizeof(uint16_t) * CH_N);
    job.state = d.coded.state;
    return rc;
}

// a stream as it is assembled: the fixed header fields, everything behind them, and what is noted on the way
struct StreamOut {
    Bytes head, io;
    int responsive[5] = {-1, -1, -1, -1, -1};
    std::vector<GroupEntry> group_at;  // group starts relative to `io` (made absolute by finish_stream)
    StaleTail stale;
};

// The end of every group, for both stream writers: flush the coder behind the last symbol; keep the compressed form if it is smaller than
// the samples' raw bits, else (encoding.cpp:545-551) roll back and store the group uncompressed -- a trivial channel always: the reference
// re-encodes it "uncompressed" too (compress bit = 0); tell StaleTail what was abandoned; note where the group starts and the responsive
// offset it ends
int settle_group(StreamOut &out, Image &img, int i, int predictor, CodedGroup &cg) {
    Chan &c = img.ch[i];
    Bytes &io = out.io;
    const size_t before = io.b.size();
    out.group_at.push_back(GroupEntry{(uint32_t)before, i});
    if (!cg.trivial) RacEnc(cg.bytes, cg.state).flush();
    const size_t body = cg.bytes.b.size() - cg.header_len;
    float bits = body * 8.0f, pixels = (float)c.w * c.h, ubits = 0.0f;
    if (c.maxval > c.minval) ubits = pixels * (ilog2u((uint32_t)(c.maxval - c.minval)) + 1) + 16;
    int rc = FUIFGPU_OK;
    if (bits >= ubits) {
        if (img.stale_tail) out.stale.abandoned(before, cg.bytes.b.data(), cg.bytes.b.size());
        rc = write_uncompressed(io, c, predictor);
    } else io.b.insert(io.b.end(), cg.bytes.b.begin(), cg.bytes.b.end());
    for (int s = 0; s < 5; s++) if (img.downscales[s] == i) out.responsive[s] = (int)io.b.size();
    return rc;
}

// ---- what write_stream and write_streams_batch share besides -------------------------------------------------------------------------
// fuif_prepare_encode (encoding.cpp:737-743): every channel's range from its samples.  Host channels are scanned here; device-only ones
// (of all pictures) go through ONE k_channel_stats launch, which also counts their zeros for the "predictability" byte
int channel_ranges(Image *imgs, size_t n_images) {
    std::vector<Chan *> who;
    for (size_t m = 0; m < n_images; m++)
        for (Chan &c : imgs[m].ch) {
            if (c.resident()) who.push_back(&c);
            else c.minmax();
        }
    return device_ranges(who);
}
int group_predictor(const Image &img, int i) {  // fuif.cpp:580-588
    if (i < img.nb_meta) return 3;   // "left" for the palettes
    if (!img.squeezed && !img.dct_style) return 2;
    return i < img.nb_meta + img.nb_channels ? 2 : 0;
}
void responsive_downscales(Image &img) {
    recompute_downscales(img);
    if (!img.squeezed && !img.dct_style) for (int s = 0; s < 6; s++) img.downscales[s] = (int)img.ch.size() - 1;
}
// what to sample of channel i's group on the device, if the group learns a tree at all (else lp.stride stays 0)
int learn_job(Image &img, int i, const GroupCoder &gc, LearnPlan &lp, LearnJob &job) {
    Chan &c = img.ch[i];
    if (!c.w || !c.h || c.minval == c.maxval) return FUIFGPU_OK;
    lp = plan_learner(c, gc.tree_mode, gc.max_tree_nodes);
    if (!lp.stride) return FUIFGPU_OK;
    c.setzero();
    std::vector<Range> ranges; std::vector<RefInfo> refs;
    job.nprops = init_properties(ranges, refs, img, i, i, gc.max_properties);
    job.n_samples = (int64_t)lp.n_samples; job.stride = (int64_t)lp.stride;
    return build_enc_group(c, refs, group_predictor(img, i), job.g);
}
// the learner's samples of a picture's device-only groups (what group_tree's sampling loop computes for host channels), in one launch:
// sample_job[channel] = its job in `out`, -1 for channels that learn nothing or have their samples on the host
int learn_samples_device(Image &img, const GroupCoder &gc, LearnSamples &out, std::vector<int> &sample_job) {
    std::vector<LearnJob> jobs;
    sample_job.assign(img.ch.size(), -1);
    for (int i = 0; i < (int)img.ch.size(); i++) {
        LearnPlan lp;
        LearnJob job;
        const int rc = img.ch[i].resident() ? learn_job(img, i, gc, lp, job) : FUIFGPU_OK;
        if (rc != FUIFGPU_OK) return rc;
        if (!lp.stride) continue;
        sample_job[(size_t)i] = (int)jobs.size();
        jobs.push_back(job);
    }
    const int rc = learn_samples_jobs_gpu(jobs, out);
    g_learn_sample_d2h += out.raw.size() * sizeof(int32_t);
    return rc;
}
// tree_mode 2: the trees of every learning group of every picture of the call.  Host-resident channels go to the device here, one phase
// earlier than for the GPU pixel loop (the same copies); the samples are computed there and stay there.  learned[m][channel]
int learn_trees_device(std::vector<Image> &imgs, const GroupCoder &gc, std::vector<std::vector<std::vector<LearnNode>>> &learned) {
    std::vector<LearnTreeJob> jobs;
    std::vector<std::pair<size_t, int>> where;
    learned.assign(imgs.size(), std::vector<std::vector<LearnNode>>());
    for (size_t m = 0; m < imgs.size(); m++) {
        Image &img = imgs[m];
        learned[m].resize(img.ch.size());
        for (int i = 0; i < (int)img.ch.size(); i++) {
            LearnPlan lp;
            LearnTreeJob job;
            const int rc = learn_job(img, i, gc, lp, job.sample);
            if (rc != FUIFGPU_OK) return rc;
            if (!lp.stride) continue;
            job.prm.max_nodes = gc.max_tree_nodes; job.prm.max_depth = lp.max_depth; job.prm.min_leaf = lp.min_leaf;
            job.prm.threshold_bits = (double)gc.split_bits; job.prm.scale = (double)lp.stride;
            where.push_back(std::make_pair(m, i));
            jobs.push_back(std::move(job));
        }
    }
    uint64_t stat_bytes = 0;
    const int rc = learn_trees_gpu(jobs, &stat_bytes);
    g_learn_stat_d2h += stat_bytes;
    for (size_t k = 0; k < jobs.size() && rc == FUIFGPU_OK; k++) learned[where[k].first][(size_t)where[k].second].swap(jobs[k].nodes);
    return rc;
}
// encoding/encoding.cpp:455-470: the fixed header fields into `head`, the transform list into `io`
void begin_stream(const Image &img, int nch, int bit_depth, const fuifgpu_encode_options &o, StreamOut &out) {
    Bytes &head = out.head;
    for (const char *m = img.nb_frames > 1 ? "FUAF" : "FUIF"; *m; m++) head.put(*m);
    head.varint((size_t)(nch + '0'));
    head.varint((size_t)(bit_depth + '&'));
    head.varint((size_t)(img.w - 1));
    head.varint((size_t)(img.h - 1));
    if (img.nb_frames > 1) {   // encoding.cpp:467-473: no per-frame numerators, no loop count
        head.varint((size_t)(img.nb_frames - 2));
        head.varint((size_t)(img.den - 1));
        head.varint(0);
        head.varint(0);
    }
    head.varint(0);  // colormodel
    head.varint((size_t)o.max_properties);
    out.io.varint(img.transforms.size());
    for (auto &t : img.transforms) {
        out.io.varint((size_t)((t.params.size() << 4) + t.id));
        for (int v : t.params) out.io.varint((size_t)v);
    }
}
// encoding.cpp:552-573: the responsive offsets behind the header, the groups, what the reference's buffer holds behind them
// (Image::stale_tail), the optional index trailer -> one malloc'ed blob
int finish_stream(StreamOut &out, bool emit_index, uint8_t **blob_out, size_t *size_out) {
    Bytes &head = out.head;
    const Bytes &io = out.io;
    int rel = 0;
    for (int s = 0; s < 5; s++) {
        if (out.responsive[s] < 0) out.responsive[s] = (int)io.b.size();
        head.varint((size_t)(out.responsive[s] - rel));
        rel = out.responsive[s];
    }
    const std::vector<uint8_t> stale = out.stale.behind(io.b.size());
    std::vector<uint8_t> trailer;
    if (emit_index && !out.group_at.empty()) {
        // the transform list sits between the header and the first group: offsets become absolute here
        for (GroupEntry &g : out.group_at) g.start += (uint32_t)head.b.size();
        build_index_trailer(out.group_at, trailer);
    }
    const size_t total = head.b.size() + io.b.size() + stale.size() + trailer.size();
    uint8_t *blob = (uint8_t *)malloc(total ? total : 1);
    if (!blob) return FUIFGPU_E_NOMEM;
    memcpy(blob, head.b.data(), head.b.size());
    memcpy(blob + head.b.size(), io.b.data(), io.b.size());
    if (!stale.empty()) memcpy(blob + head.b.size() + io.b.size(), stale.data(), stale.size());
    if (!trailer.empty()) memcpy(blob + head.b.size() + io.b.size() + stale.size(), trailer.data(), trailer.size());
    *blob_out = blob;
    *size_out = total;
    return FUIFGPU_OK;
}

// ---- one picture: group by group, the pixel loops on the host or (gpu_entropy) one launch pair per group -----------------------------
// encoding/encoding.cpp:455-573.  The picture is taken over: its device copies and the coder's buffers live as long as this call.
// There is no host route behind the GPU pixel loop: the caller asked for it
int write_stream(Image img, int nch, int bit_depth, const fuifgpu_encode_options &o, uint8_t **blob_out, size_t *size_out) {
    if (o.tree_mode == 2)   // (fuifgpu_encode_channels; every other entry point takes tree_mode 2 to the batch writer)
        return fail_with_message(FUIFGPU_E_UNSUPPORTED, "tree_mode 2 (trees learned with GPU statistics) is not offered for channels in a transform domain: use tree_mode 1");
    EncScratch enc_scratch;
    int rc = channel_ranges(&img, 1);
    if (rc != FUIFGPU_OK) return rc;
    responsive_downscales(img);
    GroupCoder gc(o);
    gc.gpu_entropy = o.gpu_entropy != 0; gc.scratch = &enc_scratch;
    StreamOut out;
    begin_stream(img, nch, bit_depth, o, out);
    for (int i = 0; i < (int)img.ch.size(); i++) {
        Chan &c = img.ch[i];
        if (!c.w || !c.h) continue;
        const int predictor = group_predictor(img, i);
        GroupDraft d;
        rc = group_prefix(img, i, predictor, gc, d);
        if (rc == FUIFGPU_OK && !d.coded.trivial) {
            if (gc.gpu_entropy) rc = code_pixels_gpu(c, predictor, gc, d);
            else code_pixels_host(c, predictor, gc, d);
        }
        if (rc == FUIFGPU_OK) rc = settle_group(out, img, i, predictor, d.coded);
        if (rc != FUIFGPU_OK) return rc;
    }
    return finish_stream(out, o.emit_index != 0, blob_out, size_out);
}

// ---- a batch of pictures: every compressed group's pixel loop in ONE launch pair ------------------------------------------------
// Phase 1 (host, per picture): per group the prefix (header + zero chance + learned tree) into its own byte buffer, the coder's
// state behind the tree, and a job.  Phase 2 (GPU): maniac_encode_jobs_gpu -- the context model of every pixel of every group in
// one launch, then one wavefront per group.  Phase 3 (host, per picture): header fields, settle_group for every group, group index.
// Same bytes as write_stream picture by picture.
// Device-only channels (fuifgpu_encode_images_device) take the same three phases: their ranges and zero counts come from one
// statistics launch, the learner's samples of a picture from one k_learn_samples_jobs launch, and build_enc_group hands their
// buffers to the coder as they are; only a group that is rolled back comes to the host.
struct PendingGroup {
    int channel = 0, predictor = 0, job = -1;   // job -1: a trivial channel (no coder)
    CodedGroup coded;
};
int write_streams_batch(std::vector<Image> &imgs, int nch, int bit_depth, const fuifgpu_encode_options &o, uint8_t **blobs_out, size_t *sizes_out) {
    GroupCoder gc(o);
    if (o.tree_mode == 2) {   // no silent host route: without a device the call fails whatever the pictures hold
        int n_devices = 0;
        const int rc = fuifgpu_device_count(&n_devices);
        if (rc != FUIFGPU_OK) return rc;
    }
    int rc = channel_ranges(imgs.data(), imgs.size());
    if (rc != FUIFGPU_OK) return rc;
    std::vector<std::vector<std::vector<LearnNode>>> learned;
    if (gc.tree_mode == 2) {
        rc = learn_trees_device(imgs, gc, learned);
        if (rc != FUIFGPU_OK) return rc;
    }
    std::vector<EncJob> jobs;
    std::vector<std::vector<PendingGroup>> pending(imgs.size());
    for (size_t m = 0; m < imgs.size(); m++) {
        Image &img = imgs[m];
        responsive_downscales(img);
        LearnSamples samples;
        std::vector<int> sample_job;
        rc = gc.tree_mode == 2 ? FUIFGPU_OK : learn_samples_device(img, gc, samples, sample_job);
        if (rc != FUIFGPU_OK) return rc;
        gc.samples = &samples; gc.sample_job = &sample_job;
        gc.learned = gc.tree_mode == 2 ? &learned[m] : nullptr;
        for (int i = 0; i < (int)img.ch.size(); i++) {
            Chan &c = img.ch[i];
            if (!c.w || !c.h) continue;
            PendingGroup pg;
            pg.channel = i;
            pg.predictor = group_predictor(img, i);
            GroupDraft d;
            rc = group_prefix(img, i, pg.predictor, gc, d);
            if (rc == FUIFGPU_OK && !d.coded.trivial) {
                EncJob job;
                rc = make_enc_job(c, pg.predictor, d, job);
                pg.job = (int)jobs.size();
                jobs.push_back(std::move(job));
            }
            if (rc != FUIFGPU_OK) return rc;
            pg.coded = std::move(d.coded);
            pending[m].push_back(std::move(pg));
        }
        gc.samples = nullptr; gc.sample_job = nullptr; gc.learned = nullptr;
    }
    rc = maniac_encode_jobs_gpu(jobs, gc.pixel_table);
    if (rc != FUIFGPU_OK) return rc;
    for (size_t m = 0; m < imgs.size(); m++) {
        StreamOut out;
        begin_stream(imgs[m], nch, bit_depth, o, out);
        for (PendingGroup &pg : pending[m]) {
            if (pg.job >= 0) {
                const EncJob &job = jobs[(size_t)pg.job];
                pg.coded.bytes.b.insert(pg.coded.bytes.b.end(), job.body.begin(), job.body.end());
                pg.coded.state = job.state;
            }
            rc = settle_group(out, imgs[m], pg.channel, pg.predictor, pg.coded);   // (a device-only channel that is rolled back comes to the host here)
            if (rc != FUIFGPU_OK) return rc;
        }
        rc = finish_stream(out, o.emit_index != 0, &blobs_out[m], &sizes_out[m]);
        if (rc != FUIFGPU_OK) return rc;
    }
    return FUIFGPU_OK;
}

// ---- the input routes: planes -> transformed Image ------------------------------------------------------------------------------------
// the end of every input route (fuif.cpp:450-503): default Squeeze, Quantize, and the transformed channels back from the GPU unless they
// stay there (keep_resident).  The channels may differ in geometry from the start (.yuv input).  colour_option: `colorspace != 0`, components
// 1 and 2 take the chroma table.  rc: what the steps before have come to -- after a failure only the device buffers are released
int squeeze_quantize_and_fetch(Image &img, const fuifgpu_encode_options &o, const Lossy &lossy, bool colour_option, bool on_gpu, bool keep_resident, int rc) {
    if (rc == FUIFGPU_OK && o.squeeze) rc = default_squeeze(img, on_gpu);
    std::vector<char> all_zero(img.ch.size(), 0);   // gpu_forward + lossy: channels whose quotients are all 0 stay on the device
    if (rc == FUIFGPU_OK && lossy.active) rc = fwd_quantize(img, lossy, o.squeeze != 0, colour_option, on_gpu, all_zero);   // fuif.cpp:459-503
    if (on_gpu && (!keep_resident || rc != FUIFGPU_OK)) {
        for (size_t k = 0; k < img.ch.size(); k++) {
            Chan &ch = img.ch[k];
            if (rc == FUIFGPU_OK && ch.dev) {
                ch.data.assign((size_t)ch.w * ch.h, 0);
                if (!ch.data.empty() && !all_zero[k]) rc = plane_download(ch.data.data(), ch.dev.i32(), ch.data.size());
            }
            ch.dev.reset();
        }
    }
    return rc;   // (no host route behind a failed GPU transform: the caller asked for the GPU)
}

// planes -> Image with the CLI's default forward transforms applied (fuif.cpp:380-455) and, with a quality, its Quantize (fuif.cpp:459-503),
// on the host or on the GPU.  device_input: `planes` is device memory -- the forward transforms run on working copies there (gpu_forward is
// implied) and the transformed channels STAY there, device-only (Chan::resident), for write_streams_batch
// An animation (anim.nb_frames > 1): `planes` holds the frames one after the other, each nch planes of w x frame_h; channel c of the strip
// is plane c of every frame, one above the other (fuif.cpp:319-327)
int build_transformed_image(const int32_t *planes, int w, int frame_h, int nch, int bit_depth, const fuifgpu_encode_options &o, const Lossy &lossy,
                            PaletteOpts pal, const AnimOpts &anim, Image &img, bool device_input = false) {
    if (lossy.quality < 100.f && pal.colors > 0) pal = PaletteOpts();   // fuif.cpp:345-350: `quality` alone is read, and only -K > 0 clears the other two
    const int h = frame_h * anim.nb_frames;
    const size_t frame_samples = (size_t)w * frame_h;
    img.w = w; img.h = h; img.maxval = (1 << bit_depth) - 1; img.nb_channels = nch;
    img.nb_frames = anim.nb_frames; img.den = anim.den;
    img.ch.resize(nch);
    for (int c = 0; c < nch; c++) {
        Chan &ch = img.ch[c];
        ch.w = w; ch.h = h; ch.component = c; ch.minval = 0; ch.maxval = img.maxval;
        if (device_input) continue;
        ch.data.reserve((size_t)w * h);
        for (int f = 0; f < anim.nb_frames; f++) {
            const int32_t *src = planes + ((size_t)f * nch + c) * frame_samples;
            ch.data.insert(ch.data.end(), src, src + frame_samples);
        }
    }
    const bool on_gpu = o.gpu_forward != 0 || device_input;
    int rc = FUIFGPU_OK;
    if (on_gpu) {
        // the planes go to the GPU once, every forward transform runs there, the transformed channels come back for the entropy coder
        for (int c = 0; c < nch && rc == FUIFGPU_OK; c++) {
            Chan &ch = img.ch[c];
            if (!ch.dev.alloc(sizeof(int32_t) * (size_t)w * h)) rc = FUIFGPU_E_HIP;
            else if (device_input)   // the caller's planes are never written
                for (int f = 0; f < anim.nb_frames && rc == FUIFGPU_OK; f++)
                    rc = dev_copy(ch.dev.i32() + (size_t)f * frame_samples, planes + ((size_t)f * nch + c) * frame_samples, sizeof(int32_t) * frame_samples);
            else rc = plane_upload(ch.dev.i32(), ch.data.data(), (size_t)w * h);
            ch.data.clear();
        }
    }
    if (rc == FUIFGPU_OK && pal.pre > 0.f && o.ycocg) rc = compact_channels(img, pal.pre, true, on_gpu);   // fuif.cpp:374-388
    if (rc == FUIFGPU_OK && o.ycocg && nch >= 3) {
        const int m = img.nb_meta;
        if (on_gpu) rc = fuifgpu_fwd_ycocg(img.ch[m].dev.i32(), img.ch[m + 1].dev.i32(), img.ch[m + 2].dev.i32(), w, h, nullptr);
        else fwd_ycocg(img);
        img.transforms.push_back({TR_YCOCG, {}});
    }
    if (rc == FUIFGPU_OK && pal.colors > 0) {   // fuif.cpp:400-417: every channel, then (still more than three) all but the last
        if (img.nb_channels > 1) rc = try_palette(img, 0, img.nb_channels - 1, pal.colors, on_gpu);
        if (rc == FUIFGPU_OK && img.nb_channels > 3) rc = try_palette(img, 0, img.nb_channels - 2, pal.colors, on_gpu);
    }
    if (rc == FUIFGPU_OK && pal.post > 0.f) rc = compact_channels(img, pal.post, false, on_gpu);   // fuif.cpp:418-430
    if (rc == FUIFGPU_OK && anim.nb_frames > 1 && anim.match) rc = fwd_match_frames(img, on_gpu);   // fuif.cpp:440-448
    return squeeze_quantize_and_fetch(img, o, lossy, o.ycocg != 0, on_gpu, device_input, rc);
}

// ---- what every entry point starts with -----------------------------------------------------------------------------------------------
// fuifgpu_encode_options is versioned by its first field (include/fuifgpu.h): copy what the caller's header knows, zero the rest.  Then
// the entry point's other argument checks (`others`, in the place they have always had: a refused call reports the same code and message),
// max_properties, the clamp of max_tree_nodes, and the traffic counters of the call start at zero
template <class OtherChecks>
int begin_encode_call(const fuifgpu_encode_options *opt, int gpu_entropy_default, fuifgpu_encode_options &o, OtherChecks others) {
    memset(&o, 0, sizeof(o));
    if (!opt) {
        o.ycocg = 1; o.squeeze = 1; o.max_properties = 12; o.tree_mode = 1; o.max_tree_nodes = 4095; o.gpu_entropy = gpu_entropy_default;
    } else {
        const uint32_t sz = opt->struct_size;
        if (sz < 2 * sizeof(uint32_t) || (sz & 3u)) return FUIFGPU_E_ARG;
        memcpy(&o, opt, sz < sizeof(o) ? sz : sizeof(o));
    }
    o.struct_size = (uint32_t)sizeof(o);
    if (const int rc = others()) return rc;
    if (o.max_properties < 0 || o.max_properties > 2 * kMaxRefs) return FUIFGPU_E_ARG;
    if (o.max_tree_nodes < 1) o.max_tree_nodes = 4095;
    if (o.max_tree_nodes > kMaxNodes) o.max_tree_nodes = kMaxNodes;
    g_plane_h2d = g_plane_d2h = 0;
    g_learn_sample_d2h = g_learn_stat_d2h = 0;
    return FUIFGPU_OK;
}

// fuifgpu_lossy_options is versioned like fuifgpu_encode_options; NULL = lossless.  A struct that ends before chroma_quality: same as quality
bool read_lossy_options(const fuifgpu_lossy_options *lossy, Lossy &l) {
    l = Lossy();
    if (!lossy) return true;
    const uint32_t sz = lossy->struct_size;
    if (sz < sizeof(uint32_t) + sizeof(float) || (sz & 3u)) return false;
    return read_qualities(lossy->quality, sz >= sizeof(fuifgpu_lossy_options) ? lossy->chroma_quality : 101.f, l);
}

// fuifgpu_palette_options is versioned like the other two; NULL, or fields the caller's struct ends before, = 0 = off
bool read_palette_options(const fuifgpu_palette_options *palette, int nch, PaletteOpts &p) {
    p = PaletteOpts();
    if (!palette) return true;
    const uint32_t sz = palette->struct_size;
    if (sz < sizeof(uint32_t) || (sz & 3u)) return false;
    fuifgpu_palette_options v;
    memset(&v, 0, sizeof(v));
    memcpy(&v, palette, sz < sizeof(v) ? sz : sizeof(v));
    if (v.palette_colors < 0 || v.palette_colors > 32767) return false;   // an index is an int16 sample
    if (!(v.compact_post_percent >= 0.f && v.compact_post_percent <= 100.f) || !(v.compact_pre_percent >= 0.f && v.compact_pre_percent <= 100.f)) return false;
    if (v.palette_colors > 0 && nch > 4) return false;   // the colour tuples are keys of at most four int16 (no PNM has more channels)
    p.colors = v.palette_colors;
    p.post = 0.01 * (double)v.compact_post_percent;   // fuif.cpp:143-144
    p.pre = 0.01 * (double)v.compact_pre_percent;
    return true;
}

// fuifgpu_animation_options: NULL = one frame; the strip must fit the format (h an int, a channel at most 2^31-1 samples) and the offset
// code 2*fh*fh + 1 an int
int read_animation_options(const fuifgpu_animation_options *anim, int w, int frame_h, AnimOpts &a) {
    a = AnimOpts();
    if (anim) {
        if (anim->struct_size < sizeof(fuifgpu_animation_options) || (anim->struct_size & 3u)) return FUIFGPU_E_ARG;
        if (anim->nb_frames < 1) return fail_with_message(FUIFGPU_E_ARG, "encode_animation: an animation has at least one frame");
        if (anim->framerate < 0) return fail_with_message(FUIFGPU_E_ARG, "encode_animation: a negative frame rate");
        if (anim->match_previous != 0 && anim->match_previous != 1)
            return fail_with_message(FUIFGPU_E_ARG, "encode_animation: match_previous is 1 (fuif -M -1, the previous frame) or 0 (-M 0); deeper distances are not "
                                                    "offered: the reference's back-fill overwrites samples an earlier distance matched with an offset it never compared");
        a.nb_frames = anim->nb_frames;
        a.den = anim->framerate > 0 ? anim->framerate : 10;   // fuif.cpp:335; image.h: den = 10
        a.match = anim->match_previous != 0;
    }
    if (w < 1 || frame_h < 1) return FUIFGPU_E_ARG;
    if ((int64_t)frame_h * a.nb_frames * w > INT32_MAX || (a.nb_frames > 1 && frame_h > 32767))
        return fail_with_message(FUIFGPU_E_ARG, "encode_animation: the strip of frames is higher than the format's h holds");
    return FUIFGPU_OK;
}
// the option structs of the PNM routes, in the order the entry points have always read them
int read_picture_options(const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette, const fuifgpu_animation_options *anim_options,
                         int w, int h, int nch, Lossy &l, PaletteOpts &pal, AnimOpts &anim) {
    if (!read_lossy_options(lossy, l) || !read_palette_options(palette, nch, pal)) return FUIFGPU_E_ARG;
    return read_animation_options(anim_options, w, h, anim);
}

void drop_blobs(uint8_t **blobs_out, size_t *sizes_out, int n) {
    for (int m = 0; m < n; m++) { free(blobs_out[m]); blobs_out[m] = nullptr; sizes_out[m] = 0; }
}

// the batch entry points: planes[m] on the host, or (device_input) in device memory
int encode_images_common(const int32_t *const *planes, int n_images, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                         const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette, uint8_t **blobs_out, size_t *sizes_out,
                         bool device_input, const fuifgpu_animation_options *anim_options) {
    if (!planes || !blobs_out || !sizes_out || n_images < 1 || w < 1 || h < 1 || nch < 1 || nch > 8 || bit_depth < 1 || bit_depth > 14) return FUIFGPU_E_ARG;
    fuifgpu_encode_options o;
    Lossy l;
    PaletteOpts pal;
    AnimOpts anim;
    if (const int rc = begin_encode_call(opt, 1, o, [&] { return read_picture_options(lossy, palette, anim_options, w, h, nch, l, pal, anim); })) return rc;
    for (int m = 0; m < n_images; m++) { blobs_out[m] = nullptr; sizes_out[m] = 0; }
    for (int m = 0; m < n_images; m++) if (!planes[m]) return FUIFGPU_E_ARG;
    std::vector<Image> imgs((size_t)n_images);   // (after a failure the pictures before the failed one may hold device-only channels: they go with `imgs`)
    int rc = FUIFGPU_OK;
    for (int m = 0; m < n_images && rc == FUIFGPU_OK; m++) rc = build_transformed_image(planes[m], w, h, nch, bit_depth, o, l, pal, anim, imgs[(size_t)m], device_input);
    if (rc != FUIFGPU_OK) return rc;
    rc = write_streams_batch(imgs, nch, bit_depth, o, blobs_out, sizes_out);
    if (rc != FUIFGPU_OK) drop_blobs(blobs_out, sizes_out, n_images);
    return rc;
}

// ---- YUV 4:2:0 video frames: what `fuif -y WxH[:b]` writes (import/read_yuv.h:29-63, fuif.cpp:277-283, 309-329, 431-435) ------------------
// Three channels of unequal geometry from the start -- Y w x h, Cb and Cr (w+1)/2 x (h+1)/2 with hshift = vshift = 1 -- under a transform
// list that begins [YCbCr, ChromaSubsample{0}] (recorded, not computed); no colour transform, no palettes, no Matching (2dmatch.h:321-322
// indexes the chroma planes with luma coordinates); from Squeeze on, the end of every input route (squeeze_quantize_and_fetch).

// where plane p (0 Y, 1 Cb, 2 Cr; NV12: 1 = 2 = the plane of pairs) of a frame starts, and the bytes of a clip up to its last sample
int64_t yuv_plane_at(const YuvGeom &g, int p) { return p == 0 ? 0 : g.pitch_y * g.h + (p == 2 && !g.nv12 ? g.pitch_c * g.ch : 0); }
int64_t yuv_clip_bytes(const YuvGeom &g) {
    return (g.nb_frames - 1) * g.frame_bytes + yuv_plane_at(g, 2) + (int64_t)(g.ch - 1) * g.pitch_c + g.row_bytes(true);
}
// the three channels as Image(w, h, maxval, 3) + read_YUV_file leave them, frames stacked (fuif.cpp:319-327); no samples yet
void yuv_image_shell(const YuvGeom &g, int den, Image &img) {
    img.w = g.w; img.h = g.h * g.nb_frames; img.maxval = g.maxval; img.nb_channels = 3;
    img.nb_frames = g.nb_frames; img.den = den;
    img.ch.resize(3);
    for (int c = 0; c < 3; c++) {
        Chan &ch = img.ch[c];
        ch.w = c ? g.cw : g.w; ch.h = (c ? g.ch : g.h) * g.nb_frames;
        ch.hshift = ch.vshift = c ? 1 : 0;
        ch.component = c; ch.minval = 0; ch.maxval = g.maxval;
    }
    img.transforms.push_back({TR_YCBCR, {}});
    img.transforms.push_back({TR_SUBSAMPLE, {0}});   // 4:2:0
    img.stale_tail = true;
}
// the host route: read_YUV_file's loops over memory; false: a sample above maxval
bool unpack_yuv_host(const uint8_t *src, const YuvGeom &g, Image &img) {
    bool in_range = true;
    for (int c = 0; c < 3; c++) {
        Chan &ch = img.ch[c];
        const int pw = c ? g.cw : g.w, ph = c ? g.ch : g.h;
        const int64_t pitch = c ? g.pitch_c : g.pitch_y, step = (int64_t)g.bytes * (c && g.nv12 ? 2 : 1), first = c == 2 && g.nv12 ? g.bytes : 0;
        ch.data.resize((size_t)pw * ph * g.nb_frames);
        int32_t *dst = ch.data.data();
        for (int f = 0; f < g.nb_frames; f++)
            for (int y = 0; y < ph; y++) {
                const uint8_t *row = src + f * g.frame_bytes + yuv_plane_at(g, c) + y * pitch + first;
                for (int x = 0; x < pw; x++) {
                    int32_t v = row[x * step];
                    if (g.bytes > 1) v += row[x * step + 1] << 8;
                    in_range &= v <= g.maxval;
                    *dst++ = v;
                }
            }
    }
    return in_range;
}
// the GPU routes: the raw frames go to the device as they are (or are there already), ONE launch unpacks every plane of every frame of the
// call into the channels' own buffers, and the staging copies go behind it
int unpack_yuv_gpu(const void *const *frames, bool on_device, const YuvGeom &g, std::vector<Image> &imgs, bool &in_range) {
    const int n = (int)imgs.size();
    std::vector<YuvJob> jobs((size_t)n);
    std::vector<DevBuf> staged;
    const size_t clip_bytes = (size_t)yuv_clip_bytes(g);
    int rc = FUIFGPU_OK;
    for (int m = 0; m < n && rc == FUIFGPU_OK; m++) {
        YuvJob &job = jobs[(size_t)m];
        job.src = static_cast<const uint8_t *>(frames[m]);
        if (!on_device) {
            DevBuf dev;
            if (!dev.alloc(clip_bytes)) { rc = FUIFGPU_E_HIP; break; }
            g_plane_h2d += clip_bytes;
            rc = fuifgpu_dev_upload(dev.p, frames[m], clip_bytes);
            job.src = static_cast<const uint8_t *>(dev.p);
            staged.push_back(std::move(dev));
        }
        for (int c = 0; c < 3 && rc == FUIFGPU_OK; c++) {
            Chan &ch = imgs[(size_t)m].ch[c];
            if (!ch.dev.alloc(sizeof(int32_t) * (size_t)ch.w * ch.h)) rc = FUIFGPU_E_HIP;
            job.out[c] = ch.dev.i32();
        }
    }
    int flag = 0;
    if (rc == FUIFGPU_OK) rc = unpack_yuv420_gpu(jobs.data(), n, g, &flag);   // (synchronous: the staging copies can go)
    in_range = flag == 0;
    return rc;
}

}  // namespace

int yuv_geometry(const void *yuv_options, int w, int h, int bit_depth, bool one_frame, YuvGeom &g, int *framerate) {
    fuifgpu_yuv_options y;
    memset(&y, 0, sizeof(y));
    if (yuv_options) {
        const uint32_t sz = static_cast<const fuifgpu_yuv_options *>(yuv_options)->struct_size;
        if (sz < sizeof(uint32_t) || (sz & 3u)) return fail_with_message(FUIFGPU_E_ARG, "yuv420: struct_size of fuifgpu_yuv_options");
        memcpy(&y, yuv_options, sz < sizeof(y) ? sz : sizeof(y));
        if (sz <= offsetof(fuifgpu_yuv_options, nb_frames)) y.nb_frames = 1;   // a struct that ends before the field
    } else y.nb_frames = 1;
    if (one_frame) y.nb_frames = 1;
    if (w < 1 || h < 1 || bit_depth < 8 || bit_depth > 14) return fail_with_message(FUIFGPU_E_ARG, "yuv420: a frame of at least 1 x 1 samples of 8 to 14 bits");
    if (y.layout != 0 && y.layout != 1) return fail_with_message(FUIFGPU_E_ARG, "yuv420: layout is 0 (I420) or 1 (NV12)");
    if (y.nb_frames < 1 || y.nb_frames > 65535 || y.framerate < 0) return fail_with_message(FUIFGPU_E_ARG, "yuv420: 1 to 65535 frames, a frame rate of 0 or more");
    if (y.nb_frames > 1 && (h & 1))
        return fail_with_message(FUIFGPU_E_ARG, "yuv420: a clip needs an even frame height (the stacked chroma planes would not be (H+1)/2 rows of the strip)");
    if ((int64_t)w * h * y.nb_frames > INT32_MAX || (int64_t)h * y.nb_frames > INT32_MAX) return fail_with_message(FUIFGPU_E_ARG, "yuv420: more than 2^31-1 samples in a channel");
    g = YuvGeom{};
    g.w = w; g.h = h; g.cw = (w + 1) / 2; g.ch = (h + 1) / 2;
    g.bytes = bit_depth > 8 ? 2 : 1; g.nv12 = y.layout; g.maxval = (1 << bit_depth) - 1; g.nb_frames = y.nb_frames;
    g.pitch_y = y.pitch_y ? y.pitch_y : g.row_bytes(false);
    g.pitch_c = y.pitch_c ? y.pitch_c : g.row_bytes(true);
    if (g.pitch_y < g.row_bytes(false) || g.pitch_c < g.row_bytes(true)) return fail_with_message(FUIFGPU_E_ARG, "yuv420: a row pitch smaller than the row");
    g.frame_bytes = g.pitch_y * g.h + g.pitch_c * g.ch * (g.nv12 ? 1 : 2);
    if (framerate) *framerate = y.framerate;
    return FUIFGPU_OK;
}

}  // namespace fuifgpu

using namespace fuifgpu;

extern "C" {

void fuifgpu_free_blob(uint8_t *p) { free(p); }

int fuifgpu_encode_plane_traffic(uint64_t *h2d_bytes, uint64_t *d2h_bytes) {
    if (h2d_bytes) *h2d_bytes = g_plane_h2d;
    if (d2h_bytes) *d2h_bytes = g_plane_d2h;
    return FUIFGPU_OK;
}

int fuifgpu_encode_learn_traffic(uint64_t *sample_bytes_d2h, uint64_t *stat_bytes_d2h) {
    if (sample_bytes_d2h) *sample_bytes_d2h = g_learn_sample_d2h;
    if (stat_bytes_d2h) *stat_bytes_d2h = g_learn_stat_d2h;
    return FUIFGPU_OK;
}

// the tree learner on its own: one sample set through the recursive host learner, the level-wise learner with the kernels' statistics, or
// the level-wise learner with the plain C++ statistics
int fuifgpu_learn_tree(const int32_t *props, const uint8_t *bucket, int64_t n_samples, int nprops, const fuifgpu_learn_options *opt, int where,
                       fuifgpu_learn_node *nodes_out, int cap, int *n_nodes) {
    if (n_samples < 0 || n_samples > INT32_MAX || nprops < 1 || nprops >= kMaxProps || where < 0 || where > 2 || !nodes_out || cap < 1 || !n_nodes ||
        (n_samples > 0 && (!props || !bucket)))
        return FUIFGPU_E_ARG;
    LearnParams q;
    if (opt) {
        if (opt->struct_size < sizeof(fuifgpu_learn_options)) return FUIFGPU_E_ARG;
        q.max_nodes = opt->max_nodes; q.max_depth = opt->max_depth; q.min_leaf = opt->min_leaf;
        q.threshold_bits = (double)(opt->split_bits > 0 ? opt->split_bits : 0); q.scale = opt->scale;
    }
    if (q.max_nodes < 1 || q.max_depth < 0 || q.min_leaf < 1 || !(q.scale > 0.0) || !std::isfinite(q.scale)) return FUIFGPU_E_ARG;
    if (where != 1)
        for (int64_t i = 0; i < n_samples; i++) if (bucket[i] > 16) return fail_with_message(FUIFGPU_E_ARG, "learn_tree: a residual class above 16");
    std::vector<LearnNode> nodes;
    int rc = FUIFGPU_OK;
    if (where == 0) learn_tree_recursive(props, bucket, n_samples, nprops, q, nodes);
    else if (where == 2) rc = learn_tree_levelwise_host(props, bucket, n_samples, nprops, q, nodes);
    else rc = learn_tree_rows_gpu(props, bucket, n_samples, nprops, q, nodes);
    if (rc != FUIFGPU_OK) return rc;
    if (nodes.size() > (size_t)cap) return fail_with_message(FUIFGPU_E_ARG, "learn_tree: the tree has more nodes than nodes_out holds");
    for (size_t k = 0; k < nodes.size(); k++) nodes_out[k] = fuifgpu_learn_node{nodes[k].prop, nodes[k].split, nodes[k].gt, nodes[k].le};
    *n_nodes = (int)nodes.size();
    return FUIFGPU_OK;
}

int fuifgpu_quantization_constant(float quality, float chroma_quality, int squeeze_option, int chroma_table, int shift) {
    Lossy l;
    if (shift < 0 || !read_qualities(quality, chroma_quality, l)) return -FUIFGPU_E_ARG;
    return l.active ? quantization_constant(l, squeeze_option != 0, chroma_table != 0, shift) : 1;
}
int fuifgpu_quantization_constant_yuv(float quality, float chroma_quality, int squeeze_option, int chroma_table, int shift) {
    Lossy l;
    if (shift < 0 || !read_qualities(quality, chroma_quality, l)) return -FUIFGPU_E_ARG;
    l.yuv = true;
    return l.active ? quantization_constant(l, squeeze_option != 0, chroma_table != 0, shift) : 1;
}

// planes: nch planes of w*h int32 in [0, 2^bit_depth-1].
int fuifgpu_encode_animation(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                             const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette, const fuifgpu_animation_options *anim_options,
                             uint8_t **blob_out, size_t *size_out) {
    if (!planes || !blob_out || !size_out || w < 1 || h < 1 || nch < 1 || nch > 8 || bit_depth < 1 || bit_depth > 14) return FUIFGPU_E_ARG;
    fuifgpu_encode_options o;
    Lossy l;
    PaletteOpts pal;
    AnimOpts anim;
    if (const int rc = begin_encode_call(opt, 0, o, [&] { return read_picture_options(lossy, palette, anim_options, w, h, nch, l, pal, anim); })) return rc;
    // tree_mode 2 learns with the batch writer's rounds: a batch of one picture, which writes the same bytes (include/fuifgpu.h)
    if (o.tree_mode == 2) return encode_images_common(&planes, 1, w, h, nch, bit_depth, opt, lossy, palette, blob_out, size_out, false, anim_options);
    Image img;
    const int rc = build_transformed_image(planes, w, h, nch, bit_depth, o, l, pal, anim, img);
    if (rc != FUIFGPU_OK) return rc;
    return write_stream(std::move(img), nch, bit_depth, o, blob_out, size_out);
}
int fuifgpu_encode_image_ex(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                            const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette, uint8_t **blob_out, size_t *size_out) {
    return fuifgpu_encode_animation(planes, w, h, nch, bit_depth, opt, lossy, palette, nullptr, blob_out, size_out);
}
int fuifgpu_encode_image_lossy(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                               const fuifgpu_lossy_options *lossy, uint8_t **blob_out, size_t *size_out) {
    return fuifgpu_encode_image_ex(planes, w, h, nch, bit_depth, opt, lossy, nullptr, blob_out, size_out);
}
int fuifgpu_encode_image(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt, uint8_t **blob_out,
                         size_t *size_out) {
    return fuifgpu_encode_image_lossy(planes, w, h, nch, bit_depth, opt, nullptr, blob_out, size_out);
}

// Same writer for channels that are ALREADY in a transform domain (e.g. quantised 8x8 DCT
// coefficient planes of a JPEG-like image: what import/read_jpeg.h:56-184 builds).  The caller
// supplies the channel list (geometry, q, samples) and the transform list that produced it; with
// opt->squeeze the default Squeeze of the first `nb_channels` channels is applied on top
// (fuif.cpp:576-578).  Predictors follow fuif.cpp:580-588, groups are single-channel.
int fuifgpu_encode_channels(const fuifgpu_raw_channel *channels, int n_channels, int w, int h, int nb_channels, int bit_depth,
                            const int32_t *transforms, int n_transform_words, const fuifgpu_encode_options *opt, uint8_t **blob_out,
                            size_t *size_out) {
    if (!channels || !blob_out || !size_out || n_channels < 1 || nb_channels < 1 || nb_channels > n_channels || w < 1 || h < 1 ||
        bit_depth < 1 || bit_depth > 14 || (n_transform_words && !transforms))
        return FUIFGPU_E_ARG;
    fuifgpu_encode_options o;
    if (const int rc = begin_encode_call(opt, 0, o, [] { return (int)FUIFGPU_OK; })) return rc;
    Image img;
    img.w = w; img.h = h; img.maxval = (1 << bit_depth) - 1; img.nb_channels = nb_channels;
    img.ch.resize(n_channels);
    for (int c = 0; c < n_channels; c++) {
        const fuifgpu_raw_channel &rc = channels[c];
        if (rc.w < 0 || rc.h < 0 || (!rc.data && (int64_t)rc.w * rc.h > 0)) return FUIFGPU_E_ARG;
        Chan &ch = img.ch[c];
        ch.w = rc.w; ch.h = rc.h; ch.hshift = rc.hshift; ch.vshift = rc.vshift; ch.hcshift = rc.hcshift; ch.vcshift = rc.vcshift;
        ch.component = rc.component; ch.q = rc.q < 1 ? 1 : rc.q;
        ch.data.assign(rc.data, rc.data + (size_t)rc.w * rc.h);
    }
    // transforms: flat words {id, nparams, params...}
    for (int k = 0; k < n_transform_words;) {
        if (k + 2 > n_transform_words) return FUIFGPU_E_ARG;
        TransformDesc t;
        t.id = transforms[k];
        const int np = transforms[k + 1];
        if (np < 0 || k + 2 + np > n_transform_words) return FUIFGPU_E_ARG;
        t.params.assign(transforms + k + 2, transforms + k + 2 + np);
        img.transforms.push_back(t);
        k += 2 + np;
    }
    img.dct_style = true;
    if (o.squeeze) default_squeeze(img, false);
    return write_stream(std::move(img), nb_channels, bit_depth, o, blob_out, size_out);
}

int fuifgpu_encode_images_lossy(const int32_t *const *planes, int n_images, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                                const fuifgpu_lossy_options *lossy, uint8_t **blobs_out, size_t *sizes_out) {
    return encode_images_common(planes, n_images, w, h, nch, bit_depth, opt, lossy, nullptr, blobs_out, sizes_out, false, nullptr);
}
int fuifgpu_encode_images_ex(const int32_t *const *planes, int planes_on_device, int n_images, int w, int h, int nch, int bit_depth,
                             const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette,
                             uint8_t **blobs_out, size_t *sizes_out) {
    return encode_images_common(planes, n_images, w, h, nch, bit_depth, opt, lossy, palette, blobs_out, sizes_out, planes_on_device != 0, nullptr);
}
int fuifgpu_encode_animations(const int32_t *const *frames, int on_device, int n_clips, int w, int frame_h, int nch, int bit_depth,
                              const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette,
                              const fuifgpu_animation_options *anim, uint8_t **blobs_out, size_t *sizes_out) {
    return encode_images_common(frames, n_clips, w, frame_h, nch, bit_depth, opt, lossy, palette, blobs_out, sizes_out, on_device != 0, anim);
}
int fuifgpu_encode_images(const int32_t *const *planes, int n_images, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                          uint8_t **blobs_out, size_t *sizes_out) {
    return fuifgpu_encode_images_lossy(planes, n_images, w, h, nch, bit_depth, opt, nullptr, blobs_out, sizes_out);
}
int fuifgpu_encode_images_device(const int32_t *const *planes_device, int n_images, int w, int h, int nch, int bit_depth,
                                 const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, uint8_t **blobs_out, size_t *sizes_out) {
    return encode_images_common(planes_device, n_images, w, h, nch, bit_depth, opt, lossy, nullptr, blobs_out, sizes_out, true, nullptr);
}

int fuifgpu_encode_yuv420(const void *const *frames, int on_device, int n, int w, int h, int bit_depth, const fuifgpu_yuv_options *yuv,
                          const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, uint8_t **blobs_out, size_t *sizes_out) {
    if (!frames || !blobs_out || !sizes_out || n < 1) return FUIFGPU_E_ARG;
    for (int m = 0; m < n; m++) { blobs_out[m] = nullptr; sizes_out[m] = 0; }
    fuifgpu_encode_options o;
    Lossy l;
    YuvGeom g;
    int framerate = 0;
    if (const int rc = begin_encode_call(opt, on_device ? 1 : 0, o, [&] {
            if (!read_lossy_options(lossy, l)) return (int)FUIFGPU_E_ARG;
            return yuv_geometry(yuv, w, h, bit_depth, false, g, &framerate);
        }))
        return rc;
    l.yuv = true;
    for (int m = 0; m < n; m++)
        if (!frames[m]) return fail_with_message(FUIFGPU_E_ARG, "yuv420: a NULL frame");
    const bool on_gpu = on_device != 0 || o.gpu_forward != 0;
    const int den = framerate > 0 ? framerate : 10;   // fuif.cpp:335; image.h: den = 10
    std::vector<Image> imgs((size_t)n);
    int rc = FUIFGPU_OK;
    bool in_range = true;
    for (Image &im : imgs) yuv_image_shell(g, den, im);
    if (on_gpu) rc = unpack_yuv_gpu(frames, on_device != 0, g, imgs, in_range);
    else for (int m = 0; m < n; m++) in_range &= unpack_yuv_host(static_cast<const uint8_t *>(frames[m]), g, imgs[(size_t)m]);
    if (rc == FUIFGPU_OK && !in_range) rc = fail_with_message(FUIFGPU_E_ARG, "yuv420: a sample above 2^bit_depth - 1");
    for (int m = 0; m < n && rc == FUIFGPU_OK; m++) rc = squeeze_quantize_and_fetch(imgs[(size_t)m], o, l, true, on_gpu, on_device != 0, rc);
    if (rc != FUIFGPU_OK) return rc;
    // pictures in device memory stay there until their last coded byte: the batch writer; so does a batch whose pixel loops run on the
    // GPU (one launch pair for all of them); else picture by picture through the stream writer of fuifgpu_encode_image
    if (on_device || (o.gpu_entropy && n > 1) || o.tree_mode == 2) rc = write_streams_batch(imgs, 3, bit_depth, o, blobs_out, sizes_out);
    else for (int m = 0; m < n && rc == FUIFGPU_OK; m++) rc = write_stream(std::move(imgs[(size_t)m]), 3, bit_depth, o, &blobs_out[m], &sizes_out[m]);
    if (rc != FUIFGPU_OK) drop_blobs(blobs_out, sizes_out, n);
    return rc;
}

}  // extern "C"
