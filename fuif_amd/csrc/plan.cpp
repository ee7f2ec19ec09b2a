// fuif_amd/csrc/plan.cpp -- host planner of the MI355X FUIF decode path.
//
// Turns the first ~100 bytes of a .fuif stream into everything the device needs that does NOT
// depend on pixel data:
//   1. header fields                       (reference: encoding/encoding.cpp:599-657)
//   2. transform list + meta transforms    (encoding.cpp:673-693, transform/transform.cpp:66-81,
//                                           squeeze.h:266-360, dct.h:209-246, subsample.h:33-69,135-157)
//      -> the coded channel table (w,h,shifts, slab offsets) the entropy kernel fills
//   3. a flat schedule of inverse-transform kernel launches equivalent to
//      Image::undo_transforms(0)           (image/image.cpp:94-115, squeeze.h:363-388,
//                                           quantize.h:32-49, dct.h:249-296, subsample.h:73-127)
//      with plane lifetimes resolved to three per-image slabs: COEF (entropy output), OUT (final
//      planes) and TMP (short-lived intermediates, first-fit with reuse).
//
// The planner is geometry only: two streams with the same header produce the same plan, which is
// what lets one kernel launch process a whole batch of images (grid.z = image).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../include/fuifgpu.h"
#include "fuifgpu_internal.h"

namespace fuifgpu {

namespace {

struct ByteReader {
    const uint8_t *p;
    size_t n, pos;
    bool eof;
    int get() {
        if (pos >= n) { eof = true; return -1; }
        return p[pos++];
    }
    // big-endian base-128 varint, at most 10 bytes, -1 on EOF (encoding/encoding.cpp:45-59)
    int varint() {
        uint32_t result = 0;
        for (int k = 0; k < 10; k++) {
            int b = get();
            if (b < 0) return -1;
            if (b < 128) return (int)(result + (uint32_t)b);
            result = (result + (uint32_t)(b - 128)) << 7;
        }
        return -1;
    }
};

struct PlaneInfo {
    int w = 0, h = 0, qsrc = -1;
    int buf = BUF_COEF;
    int64_t off = 0;
    int birth = -1;   // op index that creates the plane (-1: coded plane living in COEF)
    int death = -1;   // last op index that reads it
    bool is_final = false;
};

struct LiveChannel {
    int plane;
    int w, h, hshift, vshift, hcshift, vcshift, component;
    bool ctor_data;   // the reference's Channel owns w*h samples before any decoding (constructor planes: image.h:64-65)
};

struct ProtoOp {
    int kind = 0;
    int src[3] = {-1, -1, -1};
    int dst[3] = {-1, -1, -1};
    int p0 = 0, p1 = 0;
    std::vector<int> list;    // OP_IDCT: 64 source planes; OP_QUANT: planes to scale
    std::vector<int> list_q;  // OP_QUANT: Channel::q source of each listed plane at the time of the op
    int src_q[3] = {-2, -2, -2};  // Channel::q source of src[k] AT THE TIME OF THE OP (-2: whatever the plane carries at the end);
                                  // a later Quantize inverse resets q (quantize.h:47), which must not leak back into earlier ops
};

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// first-fit allocator with coalescing free list for the TMP slab
struct Arena {
    std::map<int64_t, int64_t> free_blocks;  // off -> size
    int64_t top = 0, peak = 0;
    int64_t alloc(int64_t size) {
        size = align_up(std::max<int64_t>(size, 1), kPlaneAlign);
        for (auto it = free_blocks.begin(); it != free_blocks.end(); ++it) {
            if (it->second >= size) {
                int64_t off = it->first, rest = it->second - size;
                free_blocks.erase(it);
                if (rest) free_blocks[off + size] = rest;
                return off;
            }
        }
        // grow: if the last free block touches the top, extend it
        if (!free_blocks.empty()) {
            auto last = std::prev(free_blocks.end());
            if (last->first + last->second == top) {
                int64_t off = last->first;
                top = off + size;
                free_blocks.erase(last);
                peak = std::max(peak, top);
                return off;
            }
        }
        int64_t off = top;
        top += size;
        peak = std::max(peak, top);
        return off;
    }
    void release(int64_t off, int64_t size) {
        size = align_up(std::max<int64_t>(size, 1), kPlaneAlign);
        auto it = free_blocks.emplace(off, size).first;
        auto next = std::next(it);
        if (next != free_blocks.end() && it->first + it->second == next->first) {
            it->second += next->second;
            free_blocks.erase(next);
        }
        if (it != free_blocks.begin()) {
            auto prev = std::prev(it);
            if (prev->first + prev->second == it->first) {
                prev->second += it->second;
                free_blocks.erase(it);
            }
        }
    }
};

// reference zig-zag variant (transform/dct.h:120-129) and cumulative shifts (dct.h:159-171)
const int kZigzag[64] = {0,  1,  4,  15, 16, 35, 36, 63, 2,  3,  5,  14, 17, 34, 37, 62, 8,  7,  6,  13, 18, 33,
                         38, 61, 9,  10, 11, 12, 19, 32, 39, 60, 24, 23, 22, 21, 20, 31, 40, 59, 25, 26, 27, 28,
                         29, 30, 41, 58, 48, 47, 46, 45, 44, 43, 42, 57, 49, 50, 51, 52, 53, 54, 55, 56};
const int kDctCshift[64] = {3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

bool has_parameters(int id) {  // transform/transform.h:85-102
    switch (id) {
        case TR_SUBSAMPLE: case TR_PALETTE: case TR_SQUEEZE: case TR_DCT: case TR_2DMATCH: case TR_PERMUTE: case TR_APPROXIMATE:
            return true;
        default:
            return false;
    }
}

// transform/subsample.h:33-69
std::vector<int> expand_subsample(const std::vector<int> &in) {
    std::vector<int> p = in;
    if (p.size() == 1) {
        switch (p[0]) {
            case 0: p = {1, 2, 2, 2}; break;
            case 1: p = {1, 2, 2, 1}; break;
            case 2: p = {1, 2, 1, 2}; break;
            case 3: p = {1, 2, 4, 1}; break;
            default: break;
        }
    }
    if (p.size() % 4) p.clear();
    return p;
}

struct Builder {
    Plan &plan;
    std::vector<LiveChannel> live;
    std::vector<PlaneInfo> planes;
    std::vector<ProtoOp> ops;
    int nb_meta = 0;  // Image::nb_meta_channels (palettes live in front of the channel list)
    bool permute_is_last = false;   // the transform list ends with a parameter-less Permute (encoding.cpp:712)
    std::vector<int> permute_labels;   // component labels of the channels a parameter-less Permute covers, in natural order
    int nbc = 0;      // Image::nb_channels: shrinks/grows with Palette (palette.h:88,66)

    explicit Builder(Plan &p) : plan(p), nbc(p.nb_channels) {}

    bool fail(int code, const std::string &msg) {
        plan.error = code;
        plan.message = msg;
        return false;
    }

    // ---- forward geometry (meta_apply) ------------------------------------------------------
    // transform/squeeze.h:266-321
    void default_squeeze(std::vector<int> &params) {
        params.clear();
        int nb = nbc;
        int w = live[nb_meta].w, h = live[nb_meta].h;
        bool wide = w > h;
        if (nb > 2 && live[nb_meta + 1].w == w && live[nb_meta + 1].h == h) {
            params.insert(params.end(), {3, nb_meta + 1, nb_meta + 2});
            params.insert(params.end(), {2, nb_meta + 1, nb_meta + 2});
        }
        if (!wide && h > 8) {
            params.insert(params.end(), {0, nb_meta, nb_meta + nb - 1});
            h = (h + 1) / 2;
        }
        while (w > 8 || h > 8) {
            if (w > 8) { params.insert(params.end(), {1, nb_meta, nb_meta + nb - 1}); w = (w + 1) / 2; }
            if (h > 8) { params.insert(params.end(), {0, nb_meta, nb_meta + nb - 1}); h = (h + 1) / 2; }
        }
    }

    // transform/squeeze.h:323-360
    bool meta_squeeze(std::vector<int> &params) {
        if (params.empty()) default_squeeze(params);
        for (size_t i = 0; i + 2 < params.size(); i += 3) {
            bool horizontal = params[i] & 1;
            bool in_place = !(params[i] & 2);
            int beginc = params[i + 1], endc = params[i + 2];
            int offset = in_place ? endc + 1 : nb_meta + nbc;
            if (beginc < 0 || endc < beginc || endc >= (int)live.size() || offset > (int)live.size())
                return fail(FUIFGPU_E_CORRUPT, "squeeze parameters address a missing channel");
            for (int c = beginc; c <= endc; c++) {
                LiveChannel d{};
                d.plane = -1;
                d.hcshift = live[c].hcshift; d.vcshift = live[c].vcshift; d.component = live[c].component;
                if (horizontal) {
                    int w = live[c].w;
                    live[c].w = (w + 1) / 2; live[c].hshift++; live[c].hcshift++;
                    d.w = w - (w + 1) / 2; d.h = live[c].h;
                } else {
                    int h = live[c].h;
                    live[c].h = (h + 1) / 2; live[c].vshift++; live[c].vcshift++;
                    d.h = h - (h + 1) / 2; d.w = live[c].w;
                }
                d.hshift = live[c].hshift; d.vshift = live[c].vshift;
                int at = offset + c - beginc;
                if (at > (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "squeeze residual position out of range");
                live.insert(live.begin() + at, d);
            }
        }
        return true;
    }

    // transform/dct.h:209-246 (scan script dct.h:173-207: position p -> component p%nb, coefficient p/nb)
    bool meta_dct(std::vector<int> &params) {
        if (params.empty()) params = {0, nbc - 1};
        if (params.size() < 2) return fail(FUIFGPU_E_CORRUPT, "DCT needs two parameters");
        int beginc = nb_meta + params[0], endc = nb_meta + params[1];
        int nb = endc - beginc + 1;
        if (beginc < 0 || nb < 1 || endc >= (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "DCT channel range invalid");
        for (int c = beginc; c <= endc; c++) {
            live[c].w = (live[c].w + 7) / 8; live[c].h = (live[c].h + 7) / 8;
            live[c].hshift += 3; live[c].vshift += 3; live[c].hcshift += 3; live[c].vcshift += 3;
        }
        for (int i = nb; i < 64 * nb; i++) {
            int c = beginc + (i % nb), coeff = i / nb;
            LiveChannel d{};
            d.plane = -1;
            d.w = live[c].w; d.h = live[c].h; d.hshift = live[c].hshift; d.vshift = live[c].vshift;
            d.hcshift = kDctCshift[coeff] + live[c].hcshift - 3;
            d.vcshift = kDctCshift[coeff] + live[c].vcshift - 3;
            d.component = live[c].component;
            live.push_back(d);
        }
        return true;
    }

    // transform/subsample.h:135-157
    bool meta_subsample(const std::vector<int> &params) {
        std::vector<int> p = expand_subsample(params);
        for (size_t i = 0; i < p.size(); i += 4) {
            int c1 = p[i], c2 = p[i + 1], srh = p[i + 2], srv = p[i + 3];
            // (the reference asserts ratios of 1 or 2 here, subsample.h:143-144, but its release build has no asserts and 4:1:1 -- ratio 4,
            // subsample.h:54-59 -- goes through: the shift is 1 for every ratio above 1, the inverse is the box filter of :116-126)
            if (c1 < 0 || c2 >= (int)live.size() || srh < 1 || srh > 8 || srv < 1 || srv > 8)
                return fail(FUIFGPU_E_UNSUPPORTED, "subsampling ratio above 8");
            for (int c = c1; c <= c2; c++) {
                live[c].w = (live[c].w + srh - 1) / srh;
                live[c].h = (live[c].h + srv - 1) / srv;
                live[c].hshift += (srh == 1 ? 0 : 1);
                live[c].vshift += (srv == 1 ? 0 : 1);
            }
        }
        return true;
    }

    // transform/palette.h:76-96
    bool meta_palette(const std::vector<int> &params) {
        if (params.size() != 3) return fail(FUIFGPU_E_CORRUPT, "Palette needs three parameters");
        int begin_c = nb_meta + params[0], end_c = nb_meta + params[1];
        if (begin_c < 0 || begin_c > end_c || end_c >= (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "Palette channel range invalid");
        int nb = end_c - begin_c + 1, nb_colors = params[2];
        if (nb_colors < 0 || (int64_t)nb_colors * nb > (1LL << 28)) return fail(FUIFGPU_E_CORRUPT, "implausible palette size");
        nb_meta++;
        nbc -= nb - 1;
        live.erase(live.begin() + begin_c + 1, live.begin() + end_c + 1);
        LiveChannel pch{};
        pch.plane = -1; pch.w = nb_colors; pch.h = nb; pch.hshift = -1; pch.component = -1; pch.ctor_data = true;
        live.insert(live.begin(), pch);
        return true;
    }

    // transform/approximate.h:62-78
    static int approx_q(const std::vector<int> &params, int c) {
        size_t k = (size_t)(c + 2 - params[0]);
        return k < params.size() ? params[k] : params.back();
    }
    bool meta_approximate(const std::vector<int> &params) {
        if (params.size() < 3) return fail(FUIFGPU_E_CORRUPT, "Approximate needs at least three parameters");
        int nb = params[1] - params[0] + 1;
        if (nb < 1 || params[0] < 0 || params[1] >= (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "Approximate channel range invalid");
        for (int c = params[0]; c <= params[1]; c++)
            if (approx_q(params, c)) { LiveChannel copy = live[c]; copy.plane = -1; live.push_back(copy); }
        return true;
    }

    // transform/2dmatch.h:115-121,179-194
    bool meta_match(std::vector<int> &params) {
        if (params.empty()) params = {0, nbc - 1, 0, 1000000};
        if (params.size() < 3) return fail(FUIFGPU_E_CORRUPT, "match transform with incorrect parameters");
        int begin_c = nb_meta + params[0], end_c = nb_meta + params[1];
        if (begin_c < 0 || begin_c > end_c || end_c >= (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "match channel range invalid");
        nb_meta++;
        LiveChannel mch{};
        mch.plane = -1; mch.w = live[begin_c].w; mch.h = live[begin_c].h; mch.component = -1; mch.ctor_data = true;
        live.insert(live.begin(), mch);
        return true;
    }

    // transform/permute.h:56-84.  With parameters the permutation is static: only the channel table moves.  Without, it is
    // the content of a 1-row meta-channel in front of the list -- stream DATA, while this planner is geometry only; so the
    // permuted channels must all have the same geometry (then neither the decode-time inv_permute_meta of
    // encoding.cpp:576-596,712 nor the inverse changes the channel table, and the inverse is a per-image plane gather).
    bool meta_permute(const std::vector<int> &params) {
        const int nb = (int)live.size() - nb_meta;
        if (params.empty()) {
            if (nb < 1) return fail(FUIFGPU_E_CORRUPT, "Permute on an image without channels");
            for (int i = 1; i < nb; i++) {
                const LiveChannel &a = live[nb_meta], &c = live[nb_meta + i];
                if (a.w != c.w || a.h != c.h || a.hshift != c.hshift || a.vshift != c.vshift || a.hcshift != c.hcshift || a.vcshift != c.vcshift)
                    return fail(FUIFGPU_E_UNSUPPORTED, "Permute from a meta-channel over channels of different geometry (the channel table would depend on stream data)");
            }
            permute_labels.clear();
            for (int i = 0; i < nb; i++) permute_labels.push_back(live[nb_meta + i].component);
            nb_meta++;
            LiveChannel pch{};
            pch.plane = -1; pch.w = nb; pch.h = 1; pch.hshift = -1; pch.component = -1; pch.ctor_data = true;
            live.insert(live.begin(), pch);
            return true;
        }
        if ((int)params.size() > nb) return fail(FUIFGPU_E_CORRUPT, "Incorrect number of parameters in Permute transform");
        const std::vector<LiveChannel> in = live;
        for (size_t i = 0; i < params.size(); i++) {
            const int c = params[i];
            if (c < 0 || c >= (int)params.size()) return fail(FUIFGPU_E_CORRUPT, "Invalid permutation: a channel is lost");
            for (size_t j = 0; j < i; j++) if (params[i] == params[j]) return fail(FUIFGPU_E_CORRUPT, "Invalid permutation: two channels map to one");
            live[nb_meta + c] = in[nb_meta + i];
        }
        return true;
    }

    // ---- inverse schedule -------------------------------------------------------------------
    int new_plane(int w, int h, int qsrc, int birth) {
        PlaneInfo pi;
        pi.w = w; pi.h = h; pi.qsrc = qsrc; pi.birth = birth; pi.buf = BUF_TMP;
        planes.push_back(pi);
        return (int)planes.size() - 1;
    }
    void touch(int plane, int op) { planes[plane].death = std::max(planes[plane].death, op); }

    // transform/squeeze.h:363-388
    bool inv_squeeze(const std::vector<int> &params) {
        for (int i = (int)params.size() - 3; i >= 0; i -= 3) {
            bool horizontal = params[i] & 1;
            bool in_place = !(params[i] & 2);
            int beginc = params[i + 1], endc = params[i + 2];
            int offset = in_place ? endc + 1 : nb_meta + nbc;
            if (beginc < 0 || endc < beginc || offset + (endc - beginc) >= (int)live.size())
                return fail(FUIFGPU_E_CORRUPT, "inverse squeeze: residual channels missing");
            for (int c = beginc; c <= endc; c++) {
                LiveChannel &a = live[c];
                const LiveChannel &r = live[offset + c - beginc];
                ProtoOp op;
                op.kind = horizontal ? OP_HSQUEEZE : OP_VSQUEEZE;
                int idx = (int)ops.size();
                int nw = horizontal ? a.w + r.w : a.w, nh = horizontal ? a.h : a.h + r.h;
                if (horizontal ? (a.h != r.h && r.w > 0) || (a.w - r.w < 0 || a.w - r.w > 1)
                               : (a.w != r.w && r.h > 0) || (a.h - r.h < 0 || a.h - r.h > 1))
                    return fail(FUIFGPU_E_UNSUPPORTED, "inverse squeeze: residual geometry not produced by meta_squeeze");
                op.src[0] = a.plane; op.src[1] = r.plane;
                op.dst[0] = new_plane(nw, nh, planes[a.plane].qsrc, idx);
                touch(a.plane, idx); touch(r.plane, idx);
                ops.push_back(op);
                a.plane = op.dst[0];
                a.w = nw; a.h = nh;
                if (horizontal) { a.hshift--; a.hcshift--; } else { a.vshift--; a.vcshift--; }
            }
            live.erase(live.begin() + offset, live.begin() + offset + (endc - beginc + 1));
        }
        return true;
    }

    // transform/quantize.h:32-49 : one batched in-place op over every plane that still carries a q
    bool inv_quantize() {
        ProtoOp op;
        op.kind = OP_QUANT;
        int idx = (int)ops.size();
        for (size_t c = nb_meta; c < live.size(); c++) {
            int pl = live[c].plane;
            if (planes[pl].qsrc < 0 || (int64_t)planes[pl].w * planes[pl].h == 0) continue;
            op.list.push_back(pl);
            op.list_q.push_back(planes[pl].qsrc);
            touch(pl, idx);
        }
        if (!op.list.empty()) ops.push_back(op);
        // Channel::q becomes 1 (quantize.h:47); recorded AFTER the op list captured the q source
        if (!op.list.empty()) pending_q_clear = op.list;
        return true;
    }
    std::vector<int> pending_q_clear;

    // transform/dct.h:249-296
    bool inv_dct(std::vector<int> &params) {
        if (params.empty()) params = {0, nbc - 1};
        int beginc = nb_meta + params[0], endc = nb_meta + params[1];
        int nb = endc - beginc + 1;
        int offset = (int)live.size() - 63 * nb;
        if (offset <= endc || nb < 1 || beginc < 0) return fail(FUIFGPU_E_CORRUPT, "invalid number of channels for inverse DCT");
        for (int c = beginc; c <= endc; c++) {
            LiveChannel &dc = live[c];
            int bw = live[c - beginc + offset].w, bh = live[c - beginc + offset].h;
            if (dc.w < bw) bw = dc.w;
            if (dc.h < bh) bh = dc.h;
            ProtoOp op;
            op.kind = OP_IDCT;
            int idx = (int)ops.size();
            op.list.resize(64);
            op.list[0] = dc.plane;
            for (int i = 1; i < 64; i++) {
                int ci = offset - nb + kZigzag[i] * nb + (c - beginc);  // ordering[c-beginc][zigzag[i]]
                if (ci < 0 || ci >= (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "inverse DCT: coefficient channel missing");
                op.list[i] = live[ci].plane;
            }
            for (int i = 0; i < 64; i++) {
                const PlaneInfo &pi = planes[op.list[i]];
                if (pi.w < bw || pi.h < bh) return fail(FUIFGPU_E_UNSUPPORTED, "inverse DCT: coefficient planes smaller than the block grid");
                touch(op.list[i], idx);
            }
            op.p0 = bw; op.p1 = bh;
            op.dst[0] = new_plane(bw * 8, bh * 8, -1, idx);
            ops.push_back(op);
            int old_hc = dc.hcshift;
            dc.plane = op.dst[0];
            dc.w = bw * 8; dc.h = bh * 8;
            dc.hshift -= 3; dc.vshift -= 3; dc.hcshift = old_hc - 3; dc.vcshift = old_hc - 3;  // sic, dct.h:280
        }
        live.erase(live.begin() + offset, live.begin() + offset + nb * 63);
        return true;
    }

    // transform/subsample.h:73-127
    bool inv_subsample(const std::vector<int> &params) {
        std::vector<int> p = expand_subsample(params);
        for (size_t i = 0; i < p.size(); i += 4) {
            int c1 = p[i], c2 = p[i + 1], srh = p[i + 2], srv = p[i + 3];
            for (int c = c1; c <= c2 && c < (int)live.size(); c++) {
                LiveChannel &ch = live[c];
                if (ch.w >= live[nb_meta].w && ch.h >= live[nb_meta].h) continue;  // subsample.h:87-91
                ProtoOp op;
                op.kind = OP_UPSAMPLE;
                int idx = (int)ops.size();
                op.src[0] = ch.plane;
                op.p0 = srh; op.p1 = srv;
                op.dst[0] = new_plane(ch.w * srh, ch.h * srv, -1, idx);
                touch(ch.plane, idx);
                ops.push_back(op);
                ch.plane = op.dst[0];
                ch.w *= srh; ch.h *= srv;
                ch.hshift = ch.vshift = ch.hcshift = ch.vcshift = 0;  // Channel(w,h,min,max) ctor defaults
                ch.component = -1;
            }
        }
        return true;
    }

    bool inv_color(int kind) {
        // transform/ycocg.h:33-48 / ycbcr.h:33-47 preconditions
        int m = (kind == OP_YCOCG) ? nb_meta : 0;
        int have = (kind == OP_YCOCG) ? nbc : (int)live.size();
        if (have < 3 || (int)live.size() < m + 3) return fail(FUIFGPU_E_CORRUPT, "colour transform needs three channels");
        int w = live[m].w, h = live[m].h;
        if (live[m + 1].w < w || live[m + 1].h < h || live[m + 2].w < w || live[m + 2].h < h)
            return fail(FUIFGPU_E_CORRUPT, "colour transform on subsampled chroma");
        ProtoOp op;
        op.kind = kind;
        int idx = (int)ops.size();
        for (int k = 0; k < 3; k++) { op.src[k] = op.dst[k] = live[m + k].plane; touch(live[m + k].plane, idx); }
        op.p0 = w; op.p1 = h;
        ops.push_back(op);
        return true;
    }

    // transform/palette.h:32-68: one gather per component; the index plane is replaced by component 0
    bool inv_palette(const std::vector<int> &params) {
        if (nb_meta < 1 || params.size() != 3) return fail(FUIFGPU_E_CORRUPT, "Palette transform without palette");
        const LiveChannel pal = live[0];
        int nb = pal.h;
        int c0 = nb_meta + params[0];
        if (c0 >= (int)live.size() || nb < 1) return fail(FUIFGPU_E_CORRUPT, "Palette transform with incorrect parameters");
        const LiveChannel index = live[c0];
        std::vector<int> outp(nb);
        for (int c = 0; c < nb; c++) {
            ProtoOp op;
            op.kind = OP_PALETTE;
            int idx = (int)ops.size();
            op.src[0] = index.plane; op.src[1] = pal.plane;
            op.p0 = c; op.p1 = pal.w;
            op.dst[0] = new_plane(index.w, index.h, c == 0 ? planes[index.plane].qsrc : -1, idx);
            touch(index.plane, idx); touch(pal.plane, idx);
            ops.push_back(op);
            outp[c] = op.dst[0];
        }
        live[c0].plane = outp[0];
        for (int i = 1; i < nb; i++) {
            // Channel(w,h,0,1) inserted at c0+1, then channel[c0+i] is labelled (palette.h:52-55): only the
            // channel that ends up last carries a component
            LiveChannel n{};
            n.w = index.w; n.h = index.h; n.component = -1; n.ctor_data = true; n.plane = -1;
            live.insert(live.begin() + c0 + 1, n);
            live[c0 + i].component = params[0] + i;
        }
        for (int i = 1; i < nb; i++) live[c0 + i].plane = outp[i];
        nbc += nb - 1;
        nb_meta--;
        live.erase(live.begin());
        return true;
    }

    // transform/permute.h:31-54
    bool inv_permute(const std::vector<int> &params) {
        if (!params.empty()) {
            if (nb_meta + (int)params.size() > (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "Permute: channels missing");
            const std::vector<LiveChannel> tmp = live;
            for (size_t i = 0; i < params.size(); i++) live[nb_meta + i] = tmp[nb_meta + params[i]];
            return true;
        }
        if (nb_meta < 1) return fail(FUIFGPU_E_CORRUPT, "Permute without its meta-channel");
        const LiveChannel perm = live[0];
        const int nb = perm.w;
        if (nb_meta + nb > (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "Permute: channels missing");
        std::vector<int> cand(nb), outp(nb);
        for (int k = 0; k < nb; k++) {
            cand[k] = live[nb_meta + k].plane;
            if (live[nb_meta + k].w != live[nb_meta].w || live[nb_meta + k].h != live[nb_meta].h)
                return fail(FUIFGPU_E_UNSUPPORTED, "Permute from a meta-channel over planes of different size");
        }
        for (int i = 0; i < nb; i++) {
            ProtoOp op;
            op.kind = OP_PERMUTE;
            const int idx = (int)ops.size();
            op.src[0] = perm.plane;
            op.list = cand;
            op.p0 = i; op.p1 = nb;
            op.dst[0] = new_plane(live[nb_meta].w, live[nb_meta].h, -1, idx);
            touch(perm.plane, idx);
            for (int pl : cand) touch(pl, idx);
            ops.push_back(op);
            outp[i] = op.dst[0];
        }
        // The reference moves whole Channel objects, so the component LABEL of output i is the one coded position perm[i]
        // carried: stream data again.  When Permute is the last transform the decode-time metadata permutation
        // (encoding.cpp:576-596) has put the labels in coded order first and the two cancel: labels end up natural.
        // Otherwise the label is not knowable from the header: reported as -1.
        for (int i = 0; i < nb; i++) {
            live[nb_meta + i].plane = outp[i];
            live[nb_meta + i].component = permute_is_last && i < (int)permute_labels.size() ? permute_labels[i] : -1;
        }
        nb_meta--;
        live.erase(live.begin());
        return true;
    }

    // transform/approximate.h:32-60
    bool inv_approximate(const std::vector<int> &params) {
        int beginc = params[0], endc = params[1];
        int offset = (int)live.size() - (endc - beginc + 1);
        for (int c = beginc; c <= endc; c++) if (!approx_q(params, c)) offset++;
        if (beginc < 0 || endc < beginc || offset <= endc || offset > (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "Approximate: remainder channels missing");
        int i = 0;
        for (int c = beginc; c <= endc; c++) {
            int q = approx_q(params, c) + 1;
            if (q == 1) continue;
            LiveChannel &ch = live[c];
            const LiveChannel &chr = live[offset + i];
            i++;
            if ((int64_t)ch.w * ch.h == 0) continue;
            if (chr.w != ch.w || chr.h != ch.h) return fail(FUIFGPU_E_UNSUPPORTED, "Approximate: remainder geometry differs");
            ProtoOp op;
            op.kind = OP_APPROX;
            int idx = (int)ops.size();
            op.src[0] = op.dst[0] = ch.plane; op.src[1] = chr.plane;
            op.p0 = q; op.p1 = chr.ctor_data ? 1 : 0;
            op.src_q[0] = planes[ch.plane].qsrc; op.src_q[1] = planes[chr.plane].qsrc;
            touch(ch.plane, idx); touch(chr.plane, idx);
            ops.push_back(op);
        }
        live.erase(live.begin() + offset, live.end());
        return true;
    }

    // transform/2dmatch.h:123-177.  Which of the two modes a stream uses is DATA (the match channel's q,
    // :147-149), so the op carries both pieces of geometry and the kernel decides per image; only the
    // previous-frame mode (what the CLI picks for animations, fuif.cpp:440) runs on the GPU.
    bool inv_match(const std::vector<int> &params) {
        if (nb_meta < 1 || params.size() < 3) return fail(FUIFGPU_E_CORRUPT, "match transform without match channel");
        int c0 = nb_meta + params[0], cn = nb_meta + params[1];
        if (c0 < 1 || cn < c0 || cn >= (int)live.size()) return fail(FUIFGPU_E_CORRUPT, "match transform with incorrect parameters");
        const LiveChannel &m = live[0];
        int w = live[c0].w, h = live[c0].h;
        ProtoOp op;
        op.kind = OP_MATCH;
        int idx = (int)ops.size();
        op.src[0] = m.plane;
        op.src_q[0] = planes[m.plane].qsrc;
        touch(m.plane, idx);
        for (int c = c0; c <= cn; c++) {
            if (live[c].w != w || live[c].h != h) return fail(FUIFGPU_E_UNSUPPORTED, "match over channels of different sizes");
            op.list.push_back(live[c].plane);
            touch(live[c].plane, idx);
        }
        if (m.w != w || m.h != h) return fail(FUIFGPU_E_UNSUPPORTED, "match channel geometry differs from the matched channels");
        op.p0 = params[2] ? 1 : 0;
        op.p1 = h / std::max(1, plan.nb_frames);
        if ((int64_t)w * h > 0) {
            ops.push_back(op);
            // free-offset mode (match channel q == 1): every sample copies from an EARLIER sample in scan order, which may
            // itself be a copy.  The chains are resolved with pointer jumping on a map of linear source indices:
            // ceil(log2(samples)) doubling steps, then one gather per matched plane.  In the other mode these ops return at once.
            // A soft match (value += source) carries one accumulator per matched plane along the chains, in two copies (a doubling
            // step reads one and writes the other): transforms.hip, k_match_*.
            const std::vector<int> channel_planes = op.list;
            const int mq = op.src_q[0];
            const bool soft = op.p0 != 0;
            int steps = 1;
            while ((1LL << steps) < (int64_t)w * h) steps++;
            ProtoOp init;
            init.kind = OP_MATCH_INIT;
            int k = (int)ops.size();
            init.src[0] = m.plane; init.src_q[0] = mq; init.p0 = op.p0;
            int cur = new_plane(w, h, -1, k);
            init.dst[0] = cur;
            touch(m.plane, k);
            std::vector<int> soft_list;   // [planes, accumulators copy 0, accumulators copy 1]
            if (soft) {
                soft_list = channel_planes;
                for (size_t c = 0; c < 2 * channel_planes.size(); c++) soft_list.push_back(new_plane(w, h, -1, k));
                init.list = soft_list;
                for (int pl : soft_list) touch(pl, k);
            }
            ops.push_back(init);
            int other = -1;
            for (int sidx = 0; sidx < steps; sidx++) {
                ProtoOp j;
                j.kind = OP_MATCH_JUMP;
                k = (int)ops.size();
                if (other < 0) other = new_plane(w, h, -1, k);
                j.src[0] = cur; j.src[1] = m.plane; j.src_q[1] = mq; j.dst[0] = other;
                j.p0 = op.p0; j.p1 = sidx & 1; j.list = soft_list;
                touch(cur, k); touch(other, k); touch(m.plane, k);
                for (int pl : soft_list) touch(pl, k);
                ops.push_back(j);
                std::swap(cur, other);
            }
            ProtoOp ap;
            ap.kind = OP_MATCH_APPLY;
            k = (int)ops.size();
            ap.src[0] = cur; ap.src[1] = m.plane; ap.src_q[1] = mq; ap.list = soft ? soft_list : channel_planes;
            ap.p0 = op.p0; ap.p1 = steps & 1;
            touch(cur, k); if (other >= 0) touch(other, k); touch(m.plane, k);
            for (int pl : ap.list) touch(pl, k);
            ops.push_back(ap);
        }
        nb_meta--;
        live.erase(live.begin());
        return true;
    }

    // Peephole on the flat schedule: [HSQUEEZE -> Co, HSQUEEZE -> Cg, YCOCG(Y, Co, Cg)] of equal geometry, the way every default
    // `fuif` encode (YCoCg, then Squeeze whose first step halves the chroma planes horizontally, squeeze.h:272-281) ends its
    // inverse chain, becomes ONE op: the full-size Co and Cg planes are never written and read back, and the YCoCg pass over
    // six planes disappears (C2: 331 -> 198 MB of plane traffic per 4K image for these three ops).
    void fuse_chroma_hsqueeze_ycocg() {
        const char *e = getenv("FUIFGPU_FUSE_YCOCG");   // read per plan: A/B measurements and tests switch it inside one process
        if (e && atoi(e) == 0) return;
        std::vector<Op> &ops = plan.ops;
        for (size_t k = 2; k < ops.size(); k++) {
            const Op &c = ops[k], &h1 = ops[k - 2], &h2 = ops[k - 1];
            if (c.kind != OP_YCOCG || h1.kind != OP_HSQUEEZE || h2.kind != OP_HSQUEEZE) continue;
            auto same = [](const PlaneRef &a, const PlaneRef &b) { return a.buf == b.buf && a.off == b.off && a.w == b.w && a.h == b.h; };
            if (!same(h1.dst[0], c.src[1]) || !same(h2.dst[0], c.src[2]) || h1.clamp_out || h2.clamp_out) continue;
            if (h1.src[0].w != h2.src[0].w || h1.src[1].w != h2.src[1].w || h1.src[0].h != h2.src[0].h) continue;
            const int wo = h1.src[0].w + h1.src[1].w, h = h1.src[0].h;
            if (c.p0 != wo || c.p1 != h || c.src[0].w != wo || c.src[0].h != h || h1.dst[0].w != wo || h2.dst[0].w != wo) continue;
            if (h1.src[1].w < 1 || h1.src[0].buf < 0 || h1.src[1].buf < 0 || h2.src[1].buf < 0) continue;
            // The fused kernel reads its four chroma inputs tile by tile while other blocks already write R, G, B: no input
            // range may overlap an output range (first-fit TMP planes can land on a plane released just before -- ADVICE r3).
            // In-place on Y alone is fine: a block reads the Y samples of its own tile before it writes them.
            auto overlaps = [](const PlaneRef &a, const PlaneRef &b) {
                return a.buf == b.buf && a.off < b.off + (int64_t)b.w * b.h && b.off < a.off + (int64_t)a.w * a.h;
            };
            const PlaneRef ins[4] = {h1.src[0], h1.src[1], h2.src[0], h2.src[1]}, outs[3] = {c.src[0], c.src[1], c.src[2]};
            bool alias = false;
            for (const PlaneRef &i : ins) for (const PlaneRef &o : outs) alias = alias || overlaps(i, o);
            for (int a = 0; a < 3; a++) for (int b2 = a + 1; b2 < 3; b2++) alias = alias || overlaps(outs[a], outs[b2]);
            if (alias) continue;
            Op f{};
            f.kind = OP_HSQ2_YCOCG;
            f.lo = c.lo; f.hi = c.hi; f.p0 = wo; f.p1 = h;
            f.src[0] = h1.src[0]; f.src[1] = h1.src[1]; f.src[2] = h2.src[0]; f.ext[0] = h2.src[1];
            f.dst[0] = c.src[0]; f.dst[1] = c.src[1]; f.dst[2] = c.src[2];
            f.idct_first = c.idct_first; f.pad = 0;
            ops[k - 2] = f;
            ops.erase(ops.begin() + (k - 1), ops.begin() + (k + 1));
            if (getenv("FUIFGPU_VERBOSE")) fprintf(stderr, "fuifgpu: plan %dx%d: chroma unsqueeze + YCoCg fused into one op (%zu ops)\n", plan.w, plan.h, ops.size());
            return;   // one YCoCg per chain
        }
    }

    // Peephole on the flat schedule: the dequantisation of a JPEG-transcoded stream (quantize.h:32-49: every coefficient plane times its q)
    // runs over 192 planes, 189 of which -- the AC coefficient planes -- are coded planes nobody touches before and that exactly one iDCT reads
    // afterwards.  For those the product is folded into the iDCT's load: the iDCT's source entry becomes BUF_COEF16Q (the int16 sample in the
    // coefficient slab times ChannelMeta::q of the plane's channel) and the plane leaves the QUANT op's list -- no widened int32 copy, no in-place
    // scaling pass, no int32 re-read (18 -> 2 bytes of traffic per AC coefficient).  The DC planes (products of the unsqueeze chain) stay in the QUANT op.
    void fuse_dequant_into_idct() {
        const char *e = getenv("FUIFGPU_FUSE_DEQUANT");      // read per plan: A/B measurements and tests switch it inside one process
        if (e && atoi(e) == 0) return;
        const char *e16 = getenv("FUIFGPU_INT16_RESIDUALS");
        if (e16 && atoi(e16) == 0) return;
        std::vector<Op> &ops = plan.ops;
        auto list_of = [&](const Op &op, int *n) -> PlaneRef * {
            *n = op.pad > 0 && (size_t)op.idct_first + (size_t)op.pad <= plan.idct_src.size() ? op.pad : 0;
            return plan.idct_src.data() + op.idct_first;
        };
        // (an Op's unused PlaneRef slots are value-initialised -- buf 0 = BUF_COEF, off 0, w = h = 0 -- and must not pass for the coded plane at offset 0: ADVICE r5)
        auto same_plane = [](const PlaneRef &a, const PlaneRef &b) { return a.buf == b.buf && a.off == b.off && (int64_t)a.w * a.h > 0 && (int64_t)b.w * b.h > 0; };
        for (size_t qk = 0; qk < ops.size(); qk++) {
            if (ops[qk].kind != OP_QUANT) continue;
            int nq = 0;
            list_of(ops[qk], &nq);
            // which planes of the QUANT list qualify: coded planes nothing else reads or writes, consumed by exactly one iDCT behind the dequantisation
            std::vector<char> cand((size_t)nq, 0);
            for (int li = 0; li < nq; li++) {
                const PlaneRef pl = plan.idct_src[(size_t)ops[qk].idct_first + (size_t)li];
                bool ok = pl.buf == BUF_COEF && (int64_t)pl.w * pl.h > 0 && pl.qsrc >= 0;
                int uses = 0;
                for (size_t k = 0; k < ops.size() && ok; k++) {
                    const Op &op = ops[k];
                    for (int d = 0; d < 3; d++) if (same_plane(op.src[d], pl) || same_plane(op.dst[d], pl)) ok = false;
                    if (same_plane(op.ext[0], pl)) ok = false;
                    int n = 0;
                    const PlaneRef *l = list_of(op, &n);
                    for (int m = 0; m < n; m++) {
                        if (!same_plane(l[m], pl)) continue;
                        if (k == qk) { if (m != li) ok = false; }                      // listed twice in the QUANT op
                        else if (op.kind == OP_IDCT && k > qk) uses++;                 // the one reader we fold into
                        else ok = false;                                               // any other op, or an iDCT BEFORE the dequantisation
                    }
                }
                cand[(size_t)li] = ok && uses == 1;
            }
            auto cand_index = [&](const PlaneRef &r) { for (int li = 0; li < nq; li++) if (cand[(size_t)li] && same_plane(plan.idct_src[(size_t)ops[qk].idct_first + (size_t)li], r)) return li; return -1; };
            // An iDCT takes the fold only when ALL of its 63 AC planes qualify: its kernel is then the instantiation whose AC loads are int16 loads at
            // compile time (a per-plane test inside the load loop keeps the loads from being issued together: measured, the iDCT doubled).  The DC plane
            // (entry 0) is its own case -- a product of the unsqueeze chain in a default stream, a coded plane when the DC was not squeezed -- and is tested at run time.
            std::vector<char> folded((size_t)nq, 0);
            bool changed = false;
            for (size_t k = qk + 1; k < ops.size(); k++) {
                if (ops[k].kind != OP_IDCT) continue;
                int n = 0;
                PlaneRef *l = list_of(ops[k], &n);
                if (n != 64) continue;
                bool all_ac = true;
                for (int m = 1; m < 64; m++) all_ac = all_ac && cand_index(l[m]) >= 0;
                if (!all_ac) continue;
                for (int m = 0; m < 64; m++) {
                    const int li = cand_index(l[m]);
                    if (li < 0) continue;
                    const int qsrc = plan.idct_src[(size_t)ops[qk].idct_first + (size_t)li].qsrc;
                    l[m].buf = BUF_COEF16Q; l[m].qsrc = qsrc;
                    folded[(size_t)li] = 1;
                }
                ops[k].pad2 = 1;      // OP_IDCT: the AC planes (entries 1..63) are BUF_COEF16Q
                changed = true;
            }
            if (!changed) continue;
            std::vector<PlaneRef> keep;
            for (int li = 0; li < nq; li++) if (!folded[(size_t)li]) keep.push_back(plan.idct_src[(size_t)ops[qk].idct_first + (size_t)li]);
            if (getenv("FUIFGPU_VERBOSE")) fprintf(stderr, "fuifgpu: plan %dx%d: dequantisation of %d of %d planes folded into the iDCT loads\n", plan.w, plan.h, nq - (int)keep.size(), nq);
            for (int li = 0; li < nq; li++) plan.idct_src[(size_t)ops[qk].idct_first + (size_t)li].buf = -1;   // the old list is dead: nobody may widen its planes on its account
            ops[qk].idct_first = (int)plan.idct_src.size();
            ops[qk].pad = (int)keep.size();
            for (const PlaneRef &r : keep) plan.idct_src.push_back(r);
            if (keep.empty()) { ops.erase(ops.begin() + (long)qk); qk--; }
        }
    }

    // Peephole on the flat schedule: [UPSAMPLE 2x2 -> Cb, UPSAMPLE 2x2 -> Cr, YCBCR(Y, Cb, Cr)], the way every 4:2:0 JPEG-transcoded chain
    // ends (subsample.h:90-115, ycbcr.h:49-60), becomes ONE op: the full-size Cb / Cr planes are never written and read back (283 -> 150 MB of plane
    // traffic per 4K picture for these three ops).  The chroma planes may be larger than the Y plane (block padding): their samples outside the
    // colour transform's region get the upsampled value and the final clamp, as the separate ops + image.cpp:107-113 leave them.
    void fuse_upsample_ycbcr() {
        const char *e = getenv("FUIFGPU_FUSE_YCBCR");
        if (e && atoi(e) == 0) return;
        std::vector<Op> &ops = plan.ops;
        for (size_t k = 2; k < ops.size(); k++) {
            const Op &c = ops[k], &u1 = ops[k - 2], &u2 = ops[k - 1];
            if (c.kind != OP_YCBCR || u1.kind != OP_UPSAMPLE || u2.kind != OP_UPSAMPLE) continue;
            if (u1.p0 != 2 || u1.p1 != 2 || u2.p0 != 2 || u2.p1 != 2 || u1.clamp_out || u2.clamp_out) continue;
            auto same = [](const PlaneRef &a, const PlaneRef &b) { return a.buf == b.buf && a.off == b.off && a.w == b.w && a.h == b.h; };
            if (!same(u1.dst[0], c.src[1]) || !same(u2.dst[0], c.src[2])) continue;
            if (u1.src[0].w != u2.src[0].w || u1.src[0].h != u2.src[0].h || u1.src[0].w < 1 || u1.src[0].h < 1) continue;
            if (u1.dst[0].w != 2 * u1.src[0].w || u1.dst[0].h != 2 * u1.src[0].h) continue;
            if (c.src[0].w != c.p0 || c.src[0].h != c.p1 || c.p0 > u1.dst[0].w || c.p1 > u1.dst[0].h || c.p0 < 1 || c.p1 < 1) continue;
            // the chroma planes must be FINAL planes whose last writer is this colour transform (no later op clamps or reads them differently)
            // (an in-place final clamp of a chroma plane that is larger than the transform's region is folded in as well: the kernel clamps what the
            // colour transform does not write)
            bool later = false;
            std::vector<size_t> clamps;
            for (size_t m = k + 1; m < ops.size(); m++) {
                const bool chroma_clamp = ops[m].kind == OP_CLAMP && same(ops[m].src[0], ops[m].dst[0]) && (same(ops[m].src[0], c.src[1]) || same(ops[m].src[0], c.src[2]));
                if (chroma_clamp) { clamps.push_back(m); continue; }
                for (int d = 0; d < 3; d++) for (int q = 0; q < 3; q++) later = later || same(ops[m].src[d], c.src[q]) || same(ops[m].dst[d], c.src[q]);
            }
            if (later) continue;
            auto overlaps = [](const PlaneRef &a, const PlaneRef &b) {
                return a.buf == b.buf && a.off < b.off + (int64_t)b.w * b.h && b.off < a.off + (int64_t)a.w * a.h;
            };
            const PlaneRef ins[2] = {u1.src[0], u2.src[0]}, outs[3] = {c.src[0], c.src[1], c.src[2]};
            bool alias = false;
            for (const PlaneRef &i : ins) for (const PlaneRef &o : outs) alias = alias || overlaps(i, o);
            for (int a = 0; a < 3; a++) for (int b2 = a + 1; b2 < 3; b2++) alias = alias || overlaps(outs[a], outs[b2]);
            if (alias) continue;
            Op f{};
            f.kind = OP_UPS2_YCBCR;
            f.lo = c.lo; f.hi = c.hi; f.p0 = c.p0; f.p1 = c.p1;
            f.src[0] = c.src[0]; f.src[1] = u1.src[0]; f.src[2] = u2.src[0];
            f.dst[0] = c.src[0]; f.dst[1] = c.src[1]; f.dst[2] = c.src[2];
            f.idct_first = c.idct_first; f.pad = 0;
            for (size_t q = clamps.size(); q-- > 0;) ops.erase(ops.begin() + (long)clamps[q]);
            ops[k - 2] = f;
            ops.erase(ops.begin() + (long)(k - 1), ops.begin() + (long)(k + 1));
            if (getenv("FUIFGPU_VERBOSE")) fprintf(stderr, "fuifgpu: plan %dx%d: chroma upsampling + YCbCr fused into one op (%zu ops)\n", plan.w, plan.h, ops.size());
            return;   // one YCbCr per chain
        }
    }

    // The coefficient slab holds int16 samples; the inverse kernels work on int32 planes.  Most coded samples are Squeeze residuals, each
    // read exactly once by the unsqueeze that consumes it: those kernels take them as int16 straight from the slab (Op::r16).  Every other
    // coded plane an op touches -- the lowest-resolution averages, DCT coefficients, palette / match / permutation planes, anything an
    // earlier op of the schedule has rewritten in place (dequantisation, Approximate, the match transforms) -- goes into Plan::widen and
    // is copied, widened, into the int32 coefficient copy before the schedule runs.
    void mark_int16_residuals() {
        std::vector<std::pair<int64_t, int64_t>> need;
        std::vector<int64_t> dirty;
        auto is_dirty = [&](const PlaneRef &r) { for (int64_t o : dirty) if (o == r.off) return true; return false; };
        auto want = [&](const PlaneRef &r) {
            if (r.buf != BUF_COEF || (int64_t)r.w * r.h <= 0) return;
            for (auto &n : need) if (n.first == r.off) { n.second = std::max<int64_t>(n.second, (int64_t)r.w * r.h); return; }
            need.push_back({r.off, (int64_t)r.w * r.h});
        };
        auto clean_coded = [&](const PlaneRef &r) { return r.buf == BUF_COEF && !is_dirty(r); };
        const char *e16 = getenv("FUIFGPU_INT16_RESIDUALS");   // read per plan like the fusion switches: tests run both forms inside one process
        const bool enabled = !e16 || atoi(e16) != 0;           // 0: widen everything (A/B, tests)
        std::vector<int64_t> made;   // coded planes whose int32 copy a dequantisation WRITES from the int16 samples (nothing to widen for them)
        auto is_made = [&](const PlaneRef &r) { for (int64_t o : made) if (o == r.off) return true; return false; };
        auto want_unless_made = [&](const PlaneRef &r) { if (!(r.buf == BUF_COEF && is_made(r))) want(r); };
        for (Op &op : plan.ops) {
            op.r16 = 0;
            const bool squeeze = op.kind == OP_HSQUEEZE || op.kind == OP_VSQUEEZE;
            const PlaneRef *list = plan.idct_src.data() + op.idct_first;   // the op's side list: iDCT sources, dequantisation / match / permute planes
            const int n_list = op.pad > 0 && (size_t)op.idct_first + (size_t)op.pad <= plan.idct_src.size() ? op.pad : 0;
            if (squeeze && enabled && clean_coded(op.src[1])) { op.r16 = 1; want_unless_made(op.src[0]); }
            else if (op.kind == OP_HSQ2_YCOCG && enabled && clean_coded(op.src[1]) && clean_coded(op.ext[0])) { op.r16 = 1; want_unless_made(op.src[0]); want_unless_made(op.src[2]); }
            else if (op.kind == OP_QUANT && enabled && n_list > 0) {
                // dequantisation of coded planes nobody has touched (the DCT coefficients of a JPEG-transcoded stream): the kernel reads the int16
                // samples and writes sample * q into the int32 copy -- widening and scaling in one pass (quantize.h:32-49)
                bool all_clean = true;
                for (int k = 0; k < n_list; k++) all_clean = all_clean && clean_coded(list[k]) && !is_made(list[k]);
                for (int k = 0; k < n_list && all_clean; k++) for (int m = 0; m < k; m++) all_clean = all_clean && list[m].off != list[k].off;
                if (all_clean) { op.r16 = 1; for (int k = 0; k < n_list; k++) made.push_back(list[k].off); }
            }
            if (!op.r16) { for (int d = 0; d < 3; d++) want_unless_made(op.src[d]); want_unless_made(op.ext[0]); }
            if (!(op.kind == OP_QUANT && op.r16)) for (int k = 0; k < n_list; k++) want_unless_made(list[k]);
            for (int k = 0; k < n_list; k++) if (list[k].buf == BUF_COEF && (op.kind == OP_QUANT || op.kind == OP_MATCH || op.kind == OP_MATCH_APPLY)) dirty.push_back(list[k].off);
            for (int d = 0; d < 3; d++) { want_unless_made(op.dst[d]); if (op.dst[d].buf == BUF_COEF) dirty.push_back(op.dst[d].off); }
            if (op.kind == OP_APPROX && op.src[0].buf == BUF_COEF) dirty.push_back(op.src[0].off);   // quotient * q + remainder in place
        }
        // (a squeeze whose residual is named in some op's side list reads the int32 copy: conservative)
        for (const PlaneRef &r : plan.idct_src) if (!(r.buf == BUF_COEF && is_made(r))) want(r);
        for (Op &op : plan.ops) {
            if (!op.r16) continue;
            auto listed = [&](const PlaneRef &r) { for (const PlaneRef &l : plan.idct_src) if (l.buf == BUF_COEF && l.off == r.off) return true; return false; };
            if (op.kind == OP_QUANT) continue;
            // (want(), not want_unless_made(): a plane "made" by a dequantisation that runs LATER in the schedule than this squeeze would be neither widened
            // nor written yet when the squeeze reads it.  No transform chain produces that order today; a wasted copy is the price of not relying on it -- ADVICE r4)
            if (listed(op.src[1]) || (op.kind == OP_HSQ2_YCOCG && listed(op.ext[0]))) { op.r16 = 0; want(op.src[1]); want(op.ext[0]); }
        }
        plan.widen.clear();
        for (auto &n : need) { plan.widen.push_back(n.first); plan.widen.push_back(n.second); }
        if (getenv("FUIFGPU_VERBOSE")) {
            int64_t samples = 0;
            for (auto &n : need) samples += n.second;
            fprintf(stderr, "fuifgpu: plan %dx%d: %zu coded planes (%lld of %lld coded samples) are widened to int32 before the inverse schedule\n", plan.w, plan.h, need.size(),
                    (long long)samples, (long long)plan.coef_elems);
        }
    }

    // keep: transforms left standing (Image::undo_transforms(keep), image/image.cpp:94-115); the final clamp is only made for keep == 0 (:107)
    bool finalize(int keep) {
        // every plane still referenced by a live channel is a final plane
        int nops_before = (int)ops.size();
        std::vector<int> last_writer(planes.size(), -1), last_kind(planes.size(), 0);
        for (int k = 0; k < nops_before; k++) {
            const ProtoOp &op = ops[k];
            for (int d = 0; d < 3; d++) if (op.dst[d] >= 0) { last_writer[op.dst[d]] = k; last_kind[op.dst[d]] = op.kind; }
            if (op.kind == OP_QUANT || op.kind == OP_MATCH || op.kind == OP_MATCH_APPLY) for (int pl : op.list) { last_writer[pl] = k; last_kind[pl] = op.kind; }
        }
        // final planes that are still coded planes need a copy into OUT
        for (auto &ch : live) {
            if ((int64_t)ch.w * ch.h == 0) continue;
            if (planes[ch.plane].birth < 0) {
                ProtoOp op;
                op.kind = OP_COPY_CLAMP;
                int idx = (int)ops.size();
                op.src[0] = ch.plane;
                op.dst[0] = new_plane(ch.w, ch.h, planes[ch.plane].qsrc, idx);
                touch(ch.plane, idx);
                ops.push_back(op);
                last_writer.push_back(idx); last_kind.push_back(OP_COPY_CLAMP);
                ch.plane = op.dst[0];
            }
        }
        // allocation: final planes -> OUT (bump), everything else born in an op -> TMP (first fit)
        std::vector<bool> is_final(planes.size(), false);
        int64_t out_top = 0;
        for (auto &ch : live) {
            if ((int64_t)ch.w * ch.h == 0) continue;
            PlaneInfo &pi = planes[ch.plane];
            if (is_final[ch.plane]) return fail(FUIFGPU_E_CORRUPT, "two channels share one plane");
            is_final[ch.plane] = true;
            pi.is_final = true;
            pi.buf = BUF_OUT;
            pi.off = out_top;
            out_top += align_up((int64_t)pi.w * pi.h, kPlaneAlign);
        }
        plan.out_elems = out_top;
        Arena arena;
        std::vector<std::vector<int>> dying(ops.size());
        for (size_t p = 0; p < planes.size(); p++)
            if (planes[p].birth >= 0 && !planes[p].is_final && planes[p].death >= 0) dying[planes[p].death].push_back((int)p);
        for (size_t k = 0; k < ops.size(); k++) {
            for (int d = 0; d < 3; d++) {
                int pl = ops[k].dst[d];
                if (pl >= 0 && planes[pl].birth == (int)k && !planes[pl].is_final)
                    planes[pl].off = arena.alloc((int64_t)planes[pl].w * planes[pl].h);
            }
            for (int pl : ops[k].list)   // work planes an op brings along in its side list (the accumulators of a soft match)
                if (pl >= 0 && planes[pl].birth == (int)k && !planes[pl].is_final) planes[pl].off = arena.alloc((int64_t)planes[pl].w * planes[pl].h);
            for (int pl : dying[k]) arena.release(planes[pl].off, (int64_t)planes[pl].w * planes[pl].h);
        }
        plan.tmp_elems = arena.peak;

        // final clamp (image/image.cpp:107-113): fuse into the producing op when it is the last
        // writer, skip when the last writer already clamps to [minval,maxval], else clamp in place
        std::vector<int> clamp_fused(ops.size(), 0);
        for (auto &ch : live) {
            if (keep != 0) break;   // (a copy op without clamp_out is a plain widening copy: transforms.hip launch_op)
            if ((int64_t)ch.w * ch.h == 0) continue;
            int pl = ch.plane;
            int lw = last_writer[pl], lk = last_kind[pl];
            bool range_ok = (lk == OP_YCBCR) || (lk == OP_YCOCG && plan.minval == 0);
            // (the colour transforms clamp what they write -- the p0 x p1 samples of the first channel's geometry.  A chroma plane that is larger
            // than that, block padding of a subsampled JPEG whose size is no multiple of 16, keeps samples they never touch: those need the final
            // clamp of image.cpp:107-113 like any other; no stream at hand leaves those samples out of range, so no fixture would notice its absence)
            if (range_ok && lw >= 0 && ((int64_t)planes[pl].w != (int64_t)ops[lw].p0 || (int64_t)planes[pl].h != (int64_t)ops[lw].p1)) range_ok = false;
            if (range_ok) continue;
            if (lw >= 0 && planes[pl].birth == lw &&
                (lk == OP_HSQUEEZE || lk == OP_VSQUEEZE || lk == OP_IDCT || lk == OP_UPSAMPLE || lk == OP_COPY_CLAMP || lk == OP_PALETTE || lk == OP_PERMUTE)) {
                clamp_fused[lw] = 1;
            } else {
                ProtoOp op;
                op.kind = OP_CLAMP;
                op.src[0] = op.dst[0] = pl;
                ops.push_back(op);
                clamp_fused.push_back(0);
            }
        }

        // resolve to flat ops
        auto ref = [&](int pl) {
            PlaneRef r{};
            if (pl < 0) { r.buf = -1; return r; }
            r.buf = planes[pl].buf; r.w = planes[pl].w; r.h = planes[pl].h; r.qsrc = planes[pl].qsrc; r.off = planes[pl].off;
            return r;
        };
        plan.ops.clear();
        plan.idct_src.clear();
        for (size_t k = 0; k < ops.size(); k++) {
            const ProtoOp &po = ops[k];
            Op op{};
            op.kind = po.kind;
            op.clamp_out = clamp_fused[k];
            op.lo = plan.minval; op.hi = plan.maxval;
            op.p0 = po.p0; op.p1 = po.p1;
            for (int d = 0; d < 3; d++) {
                op.src[d] = ref(po.src[d]); op.dst[d] = ref(po.dst[d]);
                if (po.src_q[d] != -2) op.src[d].qsrc = po.src_q[d];
            }
            op.idct_first = (int)plan.idct_src.size();
            op.pad = (int)po.list.size();
            for (size_t li = 0; li < po.list.size(); li++) {
                PlaneRef r = ref(po.list[li]);
                if (li < po.list_q.size()) r.qsrc = po.list_q[li];
                plan.idct_src.push_back(r);
            }
            plan.ops.push_back(op);
        }
        fuse_chroma_hsqueeze_ycocg();
        fuse_upsample_ycbcr();
        fuse_dequant_into_idct();
        mark_int16_residuals();
        plan.outputs.clear();
        for (auto &ch : live) {
            OutputChannel oc{};
            if ((int64_t)ch.w * ch.h == 0) { oc.plane.buf = BUF_OUT; oc.plane.w = ch.w; oc.plane.h = ch.h; oc.plane.off = 0; }
            else oc.plane = ref(ch.plane);
            oc.hshift = ch.hshift; oc.vshift = ch.vshift; oc.hcshift = ch.hcshift; oc.vcshift = ch.vcshift; oc.component = ch.component;
            plan.outputs.push_back(oc);
        }
        return true;
    }
};

uint64_t fnv1a(uint64_t h, const void *data, size_t n) {
    const uint8_t *p = (const uint8_t *)data;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

}  // namespace

// maniac/chance.cpp:31-65 (state transition table of the 12-bit adaptive bit chance);
// table[2*chance + bit] = next chance.  32.32 fixed point like the reference.
void build_chance_table(uint16_t *t, uint32_t factor, int cut) {
    const int64_t one = 1LL << 32;
    const unsigned size = 4096, max_p = 4096 - cut;
    memset(t, 0, sizeof(uint16_t) * size * 2);
    unsigned last_p8 = 0;
    int64_t p = one / 2;
    for (unsigned i = 0; i < size / 2; i++) {
        unsigned p8 = (unsigned)((size * p + one / 2) >> 32);
        if (p8 <= last_p8) p8 = last_p8 + 1;
        if (last_p8 && last_p8 < size && p8 <= max_p) t[last_p8 * 2 + 1] = (uint16_t)p8;
        p += ((one - p) * factor + one / 2) >> 32;
        last_p8 = p8;
    }
    for (unsigned i = size - max_p; i <= max_p; i++) {
        if (t[i * 2 + 1]) continue;
        p = ((int64_t)i * one + size / 2) / size;
        p += ((one - p) * factor + one / 2) >> 32;
        unsigned p8 = (unsigned)((size * p + one / 2) >> 32);
        if (p8 <= i) p8 = i + 1;
        if (p8 > max_p) p8 = max_p;
        t[i * 2 + 1] = (uint16_t)p8;
    }
    for (unsigned i = 1; i < size; i++) t[i * 2] = (uint16_t)(size - t[(size - i) * 2 + 1]);
}

int parse_and_plan(const uint8_t *blob, size_t n, Plan &plan, int keep) {
    plan = Plan();
    plan.keep = keep;
    ByteReader io{blob, n, 0, false};
    if (n < 4 || (memcmp(blob, "FUIF", 4) && memcmp(blob, "FUAF", 4))) {
        plan.error = FUIFGPU_E_NOT_FUIF;
        plan.message = "not a FUIF stream";
        return plan.error;
    }
    bool multi = !memcmp(blob, "FUAF", 4);
    io.pos = 4;
    plan.nb_channels = io.varint() - '0';
    plan.bit_depth = io.varint() - '&';
    plan.w = io.varint() + 1;
    plan.h = io.varint() + 1;
    if (multi) {
        plan.nb_frames = io.varint() + 2;
        (void)io.varint();
        int numerator = io.varint();
        if (numerator) for (int i = 1; i < plan.nb_frames; i++) (void)io.varint();
        (void)io.varint();
    }
    plan.colormodel = io.varint();
    plan.max_properties = io.varint();
    if (io.eof || plan.nb_channels < 1 || plan.nb_channels > 64 || plan.bit_depth < 1 || plan.bit_depth > 30 || plan.w < 1 ||
        plan.h < 1 || (int64_t)plan.w * plan.h > 0x7fffffffLL || plan.max_properties < 0 ||
        plan.max_properties > 2 * kMaxRefs) {
        plan.error = (plan.max_properties > 2 * kMaxRefs) ? FUIFGPU_E_UNSUPPORTED : FUIFGPU_E_CORRUPT;
        plan.message = (plan.error == FUIFGPU_E_UNSUPPORTED) ? "more reference properties (-E) than the pixel loop's property lanes hold" : "implausible header";
        return plan.error;
    }
    plan.minval = 0;
    plan.maxval = (1 << plan.bit_depth) - 1;
    int rel = 0;
    for (int s = 0; s < 5; s++) { plan.responsive_offsets[s] = io.varint() + rel; rel = plan.responsive_offsets[s]; }
    rel = (int)io.pos;
    for (int s = 0; s < 5; s++) plan.responsive_offsets[s] += rel;

    Builder b(plan);
    for (int c = 0; c < plan.nb_channels; c++) {  // Image(w,h,maxval,nb_channels): image/image.h:117-122
        LiveChannel ch{};
        ch.plane = -1; ch.w = plan.w; ch.h = plan.h; ch.component = c; ch.ctor_data = true;
        b.live.push_back(ch);
    }
    int nb_transforms = io.varint();
    if (nb_transforms < 0 || nb_transforms > 256) { plan.error = FUIFGPU_E_CORRUPT; plan.message = "bad transform count"; return plan.error; }
    for (int i = 0; i < nb_transforms; i++) {
        int v = io.varint();
        if (v < 0) { plan.error = FUIFGPU_E_CORRUPT; plan.message = "truncated transform list"; return plan.error; }
        TransformDesc t;
        t.id = v & 0xf;
        if (has_parameters(t.id)) {
            int np = v >> 4;
            for (int j = 0; j < np; j++) t.params.push_back(io.varint());
        }
        bool ok = true;
        switch (t.id) {
            case TR_YCBCR: case TR_YCOCG: case TR_QUANTIZE: break;
            case TR_SUBSAMPLE: ok = b.meta_subsample(t.params); break;
            case TR_DCT: ok = b.meta_dct(t.params); break;
            case TR_SQUEEZE: ok = b.meta_squeeze(t.params); break;
            case TR_PALETTE: ok = b.meta_palette(t.params); break;
            case TR_APPROXIMATE: ok = b.meta_approximate(t.params); break;
            case TR_2DMATCH: ok = b.meta_match(t.params); break;
            case TR_PERMUTE: ok = b.meta_permute(t.params); break;
            default:
                plan.error = FUIFGPU_E_UNSUPPORTED;
                plan.message = "transform id " + std::to_string(t.id) + " is outside the MI355X hot-path scope";
                return plan.error;
        }
        if (!ok) return plan.error;
        plan.transforms.push_back(t);
    }
    if (io.eof) { plan.error = FUIFGPU_E_CORRUPT; plan.message = "truncated header"; return plan.error; }
    plan.data_start = io.pos;
    if (keep < 0 || keep > (int)plan.transforms.size()) {
        plan.error = FUIFGPU_E_ARG;
        plan.message = "keep is 0 .. the number of transforms (" + std::to_string(plan.transforms.size()) + ")";
        return plan.error;
    }

    // A parameter-less Permute at the END of the list: right after its meta-channel the reference puts the metadata of the
    // channels still to be decoded in coded order (encoding.cpp:576-596,712).  Their geometry is identical (meta_permute
    // checked), so only the component labels of the CODED table become stream data: reported as -1.
    b.permute_is_last = !plan.transforms.empty() && plan.transforms.back().id == TR_PERMUTE && plan.transforms.back().params.empty();
    if (b.permute_is_last)
        for (size_t i = 0; i < b.permute_labels.size() && b.nb_meta + i < b.live.size(); i++) b.live[b.nb_meta + i].component = -1;

    // coded channel table + coefficient slab layout
    int64_t off = 0;
    for (size_t c = 0; c < b.live.size(); c++) {
        LiveChannel &ch = b.live[c];
        ChannelGeom g{};
        g.w = ch.w; g.h = ch.h; g.hshift = ch.hshift; g.vshift = ch.vshift; g.hcshift = ch.hcshift; g.vcshift = ch.vcshift;
        g.component = ch.component;
        g.ctor_data = ch.ctor_data ? 1 : 0;
        g.coef_off = off;
        off += align_up((int64_t)ch.w * ch.h, kPlaneAlign);
        plan.coded.push_back(g);
        PlaneInfo pi;
        pi.w = ch.w; pi.h = ch.h; pi.qsrc = (int)c; pi.buf = BUF_COEF; pi.off = g.coef_off;
        b.planes.push_back(pi);
        ch.plane = (int)c;
    }
    plan.coef_elems = off;

    // inverse schedule: Image::undo_transforms(keep) pops the list from the back until `keep` transforms are left (image/image.cpp:95-106)
    for (int i = (int)plan.transforms.size() - 1; i >= keep; i--) {
        TransformDesc &t = plan.transforms[i];
        bool ok = true;
        switch (t.id) {
            case TR_SQUEEZE: ok = b.inv_squeeze(t.params); break;
            case TR_QUANTIZE:
                ok = b.inv_quantize();
                for (int pl : b.pending_q_clear) b.planes[pl].qsrc = -1;
                b.pending_q_clear.clear();
                break;
            case TR_DCT: ok = b.inv_dct(t.params); break;
            case TR_SUBSAMPLE: ok = b.inv_subsample(t.params); break;
            case TR_YCOCG: ok = b.inv_color(OP_YCOCG); break;
            case TR_YCBCR: ok = b.inv_color(OP_YCBCR); break;
            case TR_PALETTE: ok = b.inv_palette(t.params); break;
            case TR_APPROXIMATE: ok = b.inv_approximate(t.params); break;
            case TR_2DMATCH: ok = b.inv_match(t.params); break;
            case TR_PERMUTE: ok = b.inv_permute(t.params); break;
            default: ok = false; break;
        }
        if (!ok) return plan.error ? plan.error : (plan.error = FUIFGPU_E_CORRUPT);
    }
    if (!b.finalize(keep)) return plan.error;

    uint64_t hsh = 1469598103934665603ull;
    int hdr[8] = {plan.w, plan.h, plan.bit_depth, plan.nb_channels, plan.max_properties, plan.nb_frames, (int)plan.transforms.size(), 0};
    hsh = fnv1a(hsh, hdr, sizeof(hdr));
    for (auto &t : plan.transforms) {
        hsh = fnv1a(hsh, &t.id, sizeof(int));
        if (!t.params.empty()) hsh = fnv1a(hsh, t.params.data(), t.params.size() * sizeof(int));
    }
    if (keep != 0) hsh = fnv1a(hsh, &keep, sizeof(int));   // (a shortened schedule: other ops, other output channels; keep == 0 hashes as it always did)
    plan.signature = hsh;
    return FUIFGPU_OK;
}

}  // namespace fuifgpu
