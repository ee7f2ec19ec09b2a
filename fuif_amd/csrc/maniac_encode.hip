// fuif_amd/csrc/maniac_encode.hip -- the MANIAC pixel loop of the WRITER for gfx950.
//
// The reference encoder (encoding/encoding.cpp:74-207 with maniac/rac_enc.h:28-100, maniac/symbol_enc.h and the write side of
// maniac/compound.h) walks the pixels of a channel group once: properties + prediction, tree walk to a leaf, then the residual
// goes through that leaf's adaptive chances into the range coder.  On the encode side every sample is known in advance, so only
// the last step is serial.  Two kernels per group:
//
//   k_enc_model  one lane per PIXEL: the 2k+13 properties and the prediction (context_predict.h:124-168, 233-289), the walk
//                through the group's context tree (compound.h:142-153) -> per pixel {prediction, leaf}.  No dependency between
//                pixels: this is the part that is serial in the decoder and parallel here.
//   k_enc_rac    one wavefront per group: 64 pixels at a time are staged through LDS (residual, its range, leaf), lane 0 runs
//                the symbol binarisation (symbol.h:154-185, write side), the chance updates (chance.h:77-79) and the 24-bit range
//                coder with its delayed-byte carry handling (rac_enc.h:40-85), and appends the bytes.
//
// The tree itself and the group header are written by the host writer (csrc/writer.cpp) into the same range coder before the
// pixels: the coder's state {range, low, delayed byte, pending 0xFF run} is handed in and handed back.  Output is byte-identical to
// the host writer's (tests/test_zz_gpu_encoder.py), which tests/test_writer.py pins to the reference CLI.
//
// Round 3: first correct path.  A 4K picture's longest group is a chain of 4.1 million symbols on ONE lane, so a single picture
// (maniac_encode_group_gpu: one group per launch pair, synchronous) is slower than on a CPU core; the point of the design is the
// batch: maniac_encode_jobs_gpu runs one wavefront per group over many pictures, as k_maniac_decode does.  Parity of the
// single-group kernels was checked on the MI355X (profiles/r3_gpu_encoder_tests.txt); the job-list kernels share their device code
// and are emulator-verified; nothing was timed in round 3.  The single-group coder keeps leaf chances in global memory (a
// dependent read and a write per binary decision, by lane 0); the batch coder (enc_rac_run_wave) runs the scalar code on the whole
// wavefront and keeps the current leaf in a register with the next one prefetched, as the decoder does.  Its 16 KB chance table in
// LDS limits a CU to 9 such wavefronts: the first thing to look at once it can be timed.
//
//   k_learn_samples_jobs  one lane per SAMPLE of the host's tree learner: the properties and the residual class of every stride-th pixel of
//                every group of a picture whose channels live only on the device (fuifgpu_encode_images_device) -- the same property code as
//                k_enc_model (enc_props_and_guess), so the learner sees what the coder will see.  The batch path's first wall times, with and
//                without the planes crossing PCIe, are in profiles/device_resident_encode.txt.
//   k_learn_samples_cols_jobs / k_learn_root_hist / k_learn_stats / k_learn_shortlist / k_learn_partition (and k_learn_transpose)
//                tree_mode 2: the same samples as columns, which stay on the device, and the integer statistics of the level-wise tree learner
//                (csrc/tree_learn.h) -- one round per tree level for all learning groups of a call; profiles/gpu_tree_learner.txt.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/fuifgpu.h"
#include "maniac_encode.h"

namespace fuifgpu {

namespace {

#define DEV __device__ __forceinline__

constexpr int CH_ZERO = 0, CH_SIGN = 1, CH_EXP = 2, CH_MANT = 16, CH_N = 31;   // symbol.h:97-113: zero, sign, 14 exponent, 15 mantissa chances

DEV int e_iabs(int x) { return x < 0 ? -x : x; }
DEV int e_ilog2(uint32_t l) { return l == 0 ? 0 : 31 - __builtin_clz(l); }
DEV int e_slog(int x) {   // context_predict.h:52-60
    if (x == 0) return 0;
    if (x > 0) return 32 - __builtin_clz((unsigned)x);
    return -(32 - __builtin_clz((unsigned)(-x)));
}
DEV int e_median3(int a, int b, int c) {
    if (a < b) { if (b < c) return b; return a < c ? c : a; }
    if (a < c) return a;
    return b < c ? c : b;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// context model of every pixel, in parallel
namespace {
// the 2k+13 properties of pixel i = (x, y) of a group into p[] (context_predict.h:124-168, 233-289, one pixel); returns its prediction.
// The ONE copy of the property arithmetic on the device: the coder's context model and the learner's samples both come through here.
DEV int enc_props_and_guess(const EncGroup &g, int64_t i, int32_t *p) {
    const int w = g.w;
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    int o = 0;
    for (int k = 0; k < g.nrefs; k++) {   // context_predict.h:233-289, one pixel
        const EncRef rc = g.refs[k];
        int ry = (y << g.vshift) >> rc.vshift; if (ry >= rc.h) ry = rc.h - 1;
        // a palette (hshift -1) coded behind an ordinary meta-channel (the match channel of an animation): the reference's step size is
        // (1 << rc.hshift) >> -1, 0 on its x86 build, and every sample reads the reference row's LAST sample (k_maniac_decode does the same)
        int rx = g.hshift < 0 ? rc.w - 1 : (x << g.hshift) >> rc.hshift; if (rx >= rc.w) rx = rc.w - 1;
        const int v = rc.data[(int64_t)ry * rc.w + rx];
        p[o++] = e_iabs(v); p[o++] = e_slog(v);
    }
    const int32_t *d = g.plane;
    // context_predict.h:126-133
    const int left = x ? d[i - 1] : g.zero;
    const int top = y ? d[i - w] : g.zero;
    const int topleft = (x && y) ? d[i - w - 1] : left;
    const int topright = (x + 1 < w && y) ? d[i - w + 1] : top;
    const int leftleft = x > 1 ? d[i - 2] : left;
    const int toptop = y > 1 ? d[i - 2 * (int64_t)w] : top;
    p[o++] = e_iabs(top); p[o++] = e_iabs(left); p[o++] = e_slog(top); p[o++] = e_slog(left);
    p[o++] = y; p[o++] = x;
    p[o++] = left + top - topleft; p[o++] = topleft + topright - top;
    p[o++] = e_slog(left - topleft); p[o++] = e_slog(topleft - top); p[o++] = e_slog(top - topright);
    p[o++] = e_slog(top - toptop); p[o++] = e_slog(left - leftleft);
    switch (g.predictor) {   // context_predict.h:157-166
        case 0: return g.zero;
        case 1: return (left + top) / 2;
        case 3: return left;
        case 4: return top;
        case 5: return (left + topleft + top + topright) / 4;
        case 6: { const int t = left + top - topleft; return t < g.minval ? g.minval : (t > g.maxval ? g.maxval : t); }
        default: return e_median3((int16_t)(left + top - topleft), left, top);   // :160,165 narrow the gradient to pixel_type (the property above stays an int)
    }
}
DEV void enc_model_pixel(const EncGroup &g, const EncNode *tree, int n_nodes, int64_t i, int32_t *guess_out, int32_t *leaf_out) {
    const int64_t n = (int64_t)g.w * g.h;
    if (i >= n) return;
    int32_t p[kMaxProps];
    const int guess = enc_props_and_guess(g, i, p);
    int pos = 0;
    EncNode nd = tree[0];
    for (int depth = 0; depth < n_nodes && nd.prop >= 0; depth++) {   // compound.h:142-153 (a walk visits every node at most once)
        pos = p[nd.prop & (kMaxProps - 1)] > nd.split ? nd.child : nd.child + 1;
        pos = pos < n_nodes ? pos : 0;
        nd = tree[pos];
    }
    guess_out[i] = guess;
    leaf_out[i] = nd.leaf;
}
}  // namespace

__global__ __launch_bounds__(256) void k_enc_model(EncGroup g, const EncNode *tree, int n_nodes, int32_t *guess_out, int32_t *leaf_out) {
    enc_model_pixel(g, tree, n_nodes, (int64_t)blockIdx.x * 256 + threadIdx.x, guess_out, leaf_out);
}
// the same for a list of groups (of many pictures) in one launch: the blocks of all jobs are numbered through, first_block[k] is
// the first block of job k (first_block[n_jobs] = all blocks), a block finds its job by bisection -- no empty blocks, whatever
// the mix of group sizes (a 4K picture has groups of 40 and of 4 million pixels)
__global__ __launch_bounds__(256) void k_enc_model_jobs(const EncJobDev *jobs, const uint32_t *first_block, int n_jobs) {
    const uint32_t blk = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {                       // the last job whose first block is <= blk
        const int mid = (lo + hi + 1) >> 1;
        if (first_block[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    const EncJobDev &j = jobs[lo];
    enc_model_pixel(j.g, j.tree, j.n_nodes, (int64_t)(blk - first_block[lo]) * 256 + threadIdx.x, j.guess, j.leaf);
}

// what the writer's tree learner looks at (csrc/writer.cpp, Learner): every stride-th pixel of a group, its properties and the zero/exponent
// class of its residual.  One lane per sample, the jobs' blocks numbered through like k_enc_model_jobs'; a lane writes its own row of
// nprops words (rows lie back to back: a wavefront's 64 rows are one contiguous run) and one bucket byte.
__global__ __launch_bounds__(256) void k_learn_samples_jobs(const LearnJobDev *jobs, const uint32_t *first_block, int n_jobs) {
    const uint32_t blk = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {                       // the last job whose first block is <= blk
        const int mid = (lo + hi + 1) >> 1;
        if (first_block[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    const LearnJobDev &j = jobs[lo];
    const int64_t s = (int64_t)(blk - first_block[lo]) * 256 + threadIdx.x;
    if (s >= j.n_samples) return;
    const int64_t i = s * j.stride;         // < w * h: n_samples = ceil(w * h / stride)
    const int d = j.g.plane[i] - enc_props_and_guess(j.g, i, j.props + s * j.nprops);
    j.bucket[s] = (uint8_t)(d == 0 ? 0 : e_ilog2((uint32_t)e_iabs(d)) + 1);
}

// ---------------------------------------------------------------------------------------------
// the serial part: one wavefront, lane 0 codes
namespace {

struct DevRac {   // rac_enc.h:28-100 (RacOutput24): the decoder is three bytes ahead, carries ripple into the delayed byte
    uint32_t range, low;
    int32_t delayed, pending;
    uint8_t *out;
    uint32_t cap, count;
    DEV void emit(int b) { if (count < cap) out[count] = (uint8_t)b; count++; }
    DEV void shift() {
        const uint32_t byte = low >> 16;   // bit 8 = a carry into the bytes already generated
        if (delayed < 0) delayed = (int32_t)byte;
        else if (byte < 0xFF) { emit(delayed); for (; pending; pending--) emit(0xFF); delayed = (int32_t)byte; }
        else if (byte > 0xFF) { emit(delayed + 1); for (; pending; pending--) emit(0x00); delayed = (int32_t)(byte & 0xFF); }
        else pending++;
        low = (low & 0xFFFF) << 8;
        range <<= 8;
    }
    DEV void put12(uint32_t b12, int bit) {   // rac.h:43-52 chance_12bit_chance + rac_enc.h:60-72
        const uint32_t chance = (((range & 0xFFFu) * b12 + 0x800u) >> 12) + ((range >> 12) * b12);
        if (bit) { low += range - chance; range = chance; }
        else range -= chance;
        for (int k = 0; k < 4 && range <= 0x10000u; k++) shift();   // at most three shifts while range >= 1 (rac_enc.h:66-71 loops; bounded here so that no input can hang a wavefront)
    }
};

DEV void dev_coder_write(DevRac &r, uint16_t *ch, int idx, const uint16_t *table, int bit) {
    const uint32_t c = ch[idx];
    r.put12(c, bit);
    ch[idx] = table[c * 2 + bit];   // chance.h:77-79
}

// write side of symbol.h:154-185
DEV void dev_write_symbol(DevRac &r, uint16_t *ch, const uint16_t *table, int min, int max, int value) {
    if (value == 0) { dev_coder_write(r, ch, CH_ZERO, table, 1); return; }
    dev_coder_write(r, ch, CH_ZERO, table, 0);
    const int sign = value > 0;
    if (min < 0 && max > 0) dev_coder_write(r, ch, CH_SIGN, table, sign);
    const int a = e_iabs(value);
    const int e = e_ilog2((uint32_t)a);
    const int amax = sign ? max : -min;
    const int emax = e_ilog2((uint32_t)amax);
    for (int i = 0; i < emax; i++) {
        dev_coder_write(r, ch, CH_EXP + i, table, i == e);
        if (i == e) break;
    }
    int have = 1 << e;
    for (int pos = e; pos > 0;) {
        pos--;
        const int minabs1 = have | (1 << pos);
        if (minabs1 > amax) continue;
        const int bit = (a >> pos) & 1;
        dev_coder_write(r, ch, CH_MANT + pos, table, bit);
        if (bit) have = minabs1;
    }
}

}  // namespace

namespace {
// state[0..3] = RacEncState in / out, state[4] = bytes emitted (out), state[5] = 1 when `out` was too small
DEV void enc_rac_run(const int32_t *plane, const int32_t *guess, const int32_t *leafidx, int64_t n, int minval, int maxval, uint16_t *leaves,
                     const uint16_t *table_g, uint32_t *state, uint8_t *out, uint32_t out_cap) {
    __shared__ uint16_t table[8192];
    __shared__ int32_t s_diff[64], s_min[64], s_max[64], s_leaf[64];
    const int lane = threadIdx.x;
    for (int k = lane; k < 8192; k += 64) table[k] = table_g[k];
    DevRac r;
    r.range = state[0]; r.low = state[1]; r.delayed = (int32_t)state[2]; r.pending = (int32_t)state[3];
    r.out = out; r.cap = out_cap; r.count = 0;
    __syncthreads();
    for (int64_t x0 = 0; x0 < n; x0 += 64) {
        const int nx = (int)(n - x0 < 64 ? n - x0 : 64);
        if (lane < nx) {
            const int gs = guess[x0 + lane];
            s_diff[lane] = plane[x0 + lane] - gs;
            s_min[lane] = minval - gs;
            s_max[lane] = maxval - gs;
            s_leaf[lane] = leafidx[x0 + lane];
        }
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < nx; j++) {
                const int mn = s_min[j], mx = s_max[j];
                if (mn == mx) continue;   // compound.h:228: nothing to code
                dev_write_symbol(r, leaves + (int64_t)s_leaf[j] * CH_N, table, mn, mx, s_diff[j]);   // (s_leaf < n_leaves: k_enc_model only hands out leaf numbers of the tree)
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        state[0] = r.range; state[1] = r.low; state[2] = (uint32_t)r.delayed; state[3] = (uint32_t)r.pending;
        state[4] = r.count; state[5] = r.count > r.cap ? 1u : 0u;
    }
}
}  // namespace

__global__ __launch_bounds__(64) void k_enc_rac(const int32_t *plane, const int32_t *guess, const int32_t *leafidx, int64_t n, int minval, int maxval,
                                                uint16_t *leaves, const uint16_t *table_g, uint32_t *state, uint8_t *out, uint32_t out_cap) {
    enc_rac_run(plane, guess, leafidx, n, minval, maxval, leaves, table_g, state, out, out_cap);
}
// ---- the coder as the batch runs it: the whole wavefront executes the scalar code (uniform control flow, scalars made uniform with
// readfirstlane), so the lanes can hold state: lane i (< 31) keeps chance i of the CURRENT leaf in a register, as k_maniac_decode
// does.  A binary decision reads its chance with v_readlane and updates one lane; memory is touched only when the leaf changes
// (31 lanes store the old one, load the new one: two 62-byte accesses per switch instead of a dependent global read and a write
// per decision) -- and because the encoder knows the NEXT pixel's leaf already, that load is issued one symbol early.
// A lane's own earlier store to the same leaf is seen by its later load (single-thread order), the current leaf is never the
// prefetched one.
namespace {
DEV int e_rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct WaveRac {   // DevRac with uniform state in every lane; only lane 0 stores bytes
    uint32_t range, low;
    int32_t delayed, pending;
    uint8_t *out;
    uint32_t cap, count;
    int lane;
    DEV void emit(int b) { if (lane == 0 && count < cap) out[count] = (uint8_t)b; count++; }
    DEV void shift() {
        const uint32_t byte = low >> 16;
        if (delayed < 0) delayed = (int32_t)byte;
        else if (byte < 0xFF) { emit(delayed); for (; pending; pending--) emit(0xFF); delayed = (int32_t)byte; }
        else if (byte > 0xFF) { emit(delayed + 1); for (; pending; pending--) emit(0x00); delayed = (int32_t)(byte & 0xFF); }
        else pending++;
        low = (low & 0xFFFF) << 8;
        range <<= 8;
    }
    DEV void put12(uint32_t b12, int bit) {
        const uint32_t chance = (((range & 0xFFFu) * b12 + 0x800u) >> 12) + ((range >> 12) * b12);
        if (bit) { low += range - chance; range = chance; }
        else range -= chance;
        for (int k = 0; k < 4 && range <= 0x10000u; k++) shift();
    }
};

DEV void wave_coder_write(WaveRac &r, int &leafv, int idx, const uint16_t *table, int bit) {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane(leafv, idx) & 0xFFFFu;
    r.put12(c, bit);
    const int nc = (int)table[c * 2 + bit];   // chance.h:77-79 (every lane reads the same LDS word)
    if (r.lane == idx) leafv = nc;
}

// write side of symbol.h:154-185, uniform over the wavefront
DEV void wave_write_symbol(WaveRac &r, int &leafv, const uint16_t *table, int min, int max, int value) {
    if (value == 0) { wave_coder_write(r, leafv, CH_ZERO, table, 1); return; }
    wave_coder_write(r, leafv, CH_ZERO, table, 0);
    const int sign = value > 0;
    if (min < 0 && max > 0) wave_coder_write(r, leafv, CH_SIGN, table, sign);
    const int a = e_iabs(value);
    const int e = e_ilog2((uint32_t)a);
    const int amax = sign ? max : -min;
    const int emax = e_ilog2((uint32_t)amax);
    for (int i = 0; i < emax; i++) {
        wave_coder_write(r, leafv, CH_EXP + i, table, i == e);
        if (i == e) break;
    }
    int have = 1 << e;
    for (int pos = e; pos > 0;) {
        pos--;
        const int minabs1 = have | (1 << pos);
        if (minabs1 > amax) continue;
        const int bit = (a >> pos) & 1;
        wave_coder_write(r, leafv, CH_MANT + pos, table, bit);
        if (bit) have = minabs1;
    }
}

DEV void enc_rac_run_wave(const int32_t *plane, const int32_t *guess, const int32_t *leafidx, int64_t n, int minval, int maxval, uint16_t *leaves,
                          const uint16_t *table_g, uint32_t *state, uint8_t *out, uint32_t out_cap) {
    __shared__ uint16_t table[8192];
    __shared__ int32_t s_diff[64], s_min[64], s_max[64], s_leaf[64];
    const int lane = threadIdx.x;
    for (int k = lane; k < 8192; k += 64) table[k] = table_g[k];
    WaveRac r;
    r.range = (uint32_t)e_rfl((int)state[0]); r.low = (uint32_t)e_rfl((int)state[1]); r.delayed = e_rfl((int)state[2]); r.pending = e_rfl((int)state[3]);
    r.out = out; r.cap = out_cap; r.count = 0; r.lane = lane;
    int cur = -1, leafv = 0;         // the current leaf and, in lane i < 31, its chance i
    int pre = -1, prev = 0;          // a prefetched leaf (its number, its chances)
    __syncthreads();
    for (int64_t x0 = 0; x0 < n; x0 += 64) {
        const int nx = (int)(n - x0 < 64 ? n - x0 : 64);
        if (lane < nx) {
            const int gs = guess[x0 + lane];
            s_diff[lane] = plane[x0 + lane] - gs;
            s_min[lane] = minval - gs;
            s_max[lane] = maxval - gs;
            s_leaf[lane] = leafidx[x0 + lane];
        }
        __syncthreads();
        for (int j = 0; j < nx; j++) {
            const int mn = e_rfl(s_min[j]), mx = e_rfl(s_max[j]);
            if (mn == mx) continue;   // compound.h:228: nothing to code
            const int lf = e_rfl(s_leaf[j]);
            if (lf != cur) {
                if (cur >= 0 && lane < CH_N) leaves[(int64_t)cur * CH_N + lane] = (uint16_t)leafv;
                if (lf == pre) leafv = prev;
                else if (lane < CH_N) leafv = leaves[(int64_t)lf * CH_N + lane];
                cur = lf;
                pre = -1;
            }
            // the next pixel's leaf is known already: fetch its chances while this symbol is coded
            if (j + 1 < nx) {
                const int nl = e_rfl(s_leaf[j + 1]);
                if (nl != cur && nl != pre) {
                    if (lane < CH_N) prev = leaves[(int64_t)nl * CH_N + lane];
                    pre = nl;
                }
            }
            wave_write_symbol(r, leafv, table, mn, mx, e_rfl(s_diff[j]));
        }
        __syncthreads();
    }
    if (cur >= 0 && lane < CH_N) leaves[(int64_t)cur * CH_N + lane] = (uint16_t)leafv;
    if (lane == 0) {
        state[0] = r.range; state[1] = r.low; state[2] = (uint32_t)r.delayed; state[3] = (uint32_t)r.pending;
        state[4] = r.count; state[5] = r.count > r.cap ? 1u : 0u;
    }
}
}  // namespace

// one wavefront per job: the groups of a whole batch of pictures code side by side, as k_maniac_decode's tiles decode
__global__ __launch_bounds__(64) void k_enc_rac_jobs(const EncJobDev *jobs, const uint16_t *table_g) {
    const EncJobDev &j = jobs[blockIdx.x];
    enc_rac_run_wave(j.g.plane, j.guess, j.leaf, j.n, j.g.minval, j.g.maxval, j.leaves, table_g, j.state, j.out, j.out_cap);
}

// ---------------------------------------------------------------------------------------------
// One arena: [LearnJobDev x nj][first blocks][every job's property rows][every job's bucket bytes]; the head goes up in one copy, the rows
// and buckets come back in one.
int learn_samples_jobs_gpu(const std::vector<LearnJob> &jobs, LearnSamples &out) {
    out = LearnSamples();
    const size_t nj = jobs.size();
    if (!nj) return FUIFGPU_OK;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t off_first = up(sizeof(LearnJobDev) * nj), head = off_first + up(sizeof(uint32_t) * (nj + 1));
    out.props_off.resize(nj); out.bucket_off.resize(nj);
    size_t words = 0, bytes = 0;
    uint64_t blocks = 0;
    std::vector<uint8_t> host(head, 0);
    LearnJobDev *h_jobs = reinterpret_cast<LearnJobDev *>(host.data());
    uint32_t *first = reinterpret_cast<uint32_t *>(host.data() + off_first);
    for (size_t k = 0; k < nj; k++) {
        const LearnJob &j = jobs[k];
        const int64_t npix = (int64_t)j.g.w * j.g.h;
        if (!j.g.plane || j.g.w < 1 || j.g.h < 1 || j.g.nrefs < 0 || j.g.nrefs > kMaxRefs || j.nprops != 2 * j.g.nrefs + kNonRefProps || j.stride < 1 ||
            j.n_samples != (npix + j.stride - 1) / j.stride)
            return FUIFGPU_E_ARG;
        out.props_off[k] = words; words += (size_t)j.n_samples * (size_t)j.nprops;
        out.bucket_off[k] = bytes; bytes += (size_t)j.n_samples;
        first[k] = (uint32_t)blocks; blocks += ((uint64_t)j.n_samples + 255) / 256;
    }
    first[nj] = (uint32_t)blocks;
    if (blocks > 0x7FFFFFFFull) return FUIFGPU_E_ARG;
    const size_t result = words * sizeof(int32_t) + bytes;
    uint8_t *arena = nullptr;
    if (hipMalloc((void **)&arena, head + result) != hipSuccess) return FUIFGPU_E_HIP;
    for (size_t k = 0; k < nj; k++) {
        LearnJobDev &d = h_jobs[k];
        d.g = jobs[k].g; d.n_samples = jobs[k].n_samples; d.stride = jobs[k].stride; d.nprops = jobs[k].nprops; d.pad = 0;
        d.props = reinterpret_cast<int32_t *>(arena + head) + out.props_off[k];
        d.bucket = arena + head + words * sizeof(int32_t) + out.bucket_off[k];
    }
    int rc = FUIFGPU_OK;
#define ECHK(call) do { if (rc == FUIFGPU_OK && (call) != hipSuccess) rc = FUIFGPU_E_HIP; } while (0)
    ECHK(hipMemcpy(arena, host.data(), head, hipMemcpyHostToDevice));
    if (rc == FUIFGPU_OK) {
        hipLaunchKernelGGL(k_learn_samples_jobs, dim3((unsigned)blocks), dim3(256), 0, nullptr, reinterpret_cast<const LearnJobDev *>(arena),
                           reinterpret_cast<const uint32_t *>(arena + off_first), (int)nj);
        ECHK(hipGetLastError());
    }
    out.raw.resize((result + 3) / 4);
    out.n_words = words;
    ECHK(hipMemcpy(out.raw.data(), arena + head, result, hipMemcpyDeviceToHost));   // synchronises with the null stream's kernels
#undef ECHK
    hipFree(arena);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// The level-wise tree learner's statistics (tree_mode 2; the host side, the record formats and the margin are in csrc/tree_learn.h).
// The device supplies exact integers -- minimum, maximum, order statistics, conditional histograms, the partition -- and a shortlist
// chosen with its own double log2, which is an approximation only: every decision is taken by the host's cost().
//
// Layout: the samples of a learning group are nprops columns of n_samples words; a node is a segment idx[lo, lo + n) of sample numbers
// (level 0: the identity, no array).  A (node, property) scan reads the n sample numbers of the segment (contiguous) and gathers n words
// from ONE column (n_samples * 4 bytes, 240 KB at the default sample of 60 000: a gather inside a cache-resident run, where the row-major
// rows of tree_mode 1 would give 4 useful bytes per row of 4 * nprops).  Per level and group the statistics kernel reads at most
// nprops * passes * 9 bytes per sample of the level's active nodes, passes = 2 + ceil(bits(max - min) / 8) <= 6; nodes of at most 4096
// samples are staged in LDS by the first pass and read from global memory once (9 bytes per sample and property).

// the same sampling as k_learn_samples_jobs, written as columns: lane s writes word s of every column (a wavefront's stores to one
// column are one contiguous run)
__global__ __launch_bounds__(256) void k_learn_samples_cols_jobs(const LearnJobDev *jobs, const uint32_t *first_block, int n_jobs) {
    const uint32_t blk = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {                       // the last job whose first block is <= blk
        const int mid = (lo + hi + 1) >> 1;
        if (first_block[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    const LearnJobDev &j = jobs[lo];
    const int64_t s = (int64_t)(blk - first_block[lo]) * 256 + threadIdx.x;
    if (s >= j.n_samples) return;
    const int64_t i = s * j.stride;         // < w * h: n_samples = ceil(w * h / stride)
    int32_t p[kMaxProps];
    const int d = j.g.plane[i] - enc_props_and_guess(j.g, i, p);
    for (int k = 0; k < j.nprops; k++) j.props[(int64_t)k * j.n_samples + s] = p[k];   // nprops = 2 * nrefs + 13 <= 63 (checked by the host)
    j.bucket[s] = (uint8_t)(d == 0 ? 0 : e_ilog2((uint32_t)e_iabs(d)) + 1);
}

// rows [sample][nprops] -> columns [prop][sample] (fuifgpu_learn_tree on rows that are already in device memory)
__global__ __launch_bounds__(256) void k_learn_transpose(const int32_t *rows, int32_t *cols, int64_t n_samples, int nprops) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples * nprops) return;
    const int64_t p = e / n_samples, s = e - p * n_samples;
    cols[e] = rows[s * nprops + p];
}

namespace {
DEV int learn_bucket(const uint8_t *bucket, int64_t s) { const int b = bucket[s]; return b < kLearnBuckets ? b : kLearnBuckets - 1; }   // (a caller's byte above 16 must not leave the histogram)
}

// one block per job: the histogram of all its samples (the roots; every other node's histogram is known to the host from its parent's split)
__global__ __launch_bounds__(256) void k_learn_root_hist(const LearnTreeJobDev *jobs, int32_t *hist) {
    __shared__ int s_h[kLearnBuckets];
    const LearnTreeJobDev &j = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid < kLearnBuckets) s_h[tid] = 0;
    __syncthreads();
    for (int64_t i = tid; i < j.n_samples; i += 256) atomicAdd(&s_h[learn_bucket(j.bucket, i)], 1);
    __syncthreads();
    if (tid < kLearnBuckets) hist[(int64_t)blockIdx.x * kLearnBuckets + tid] = s_h[tid];
}

// One block per (node, property), the nodes' blocks numbered through (first_block[k] = first block = first record of node k): minimum and
// maximum; the three order statistics k = n * q / 4 by an exact radix selection on (value - minimum) as an unsigned number, 8 bits a pass,
// all three in the same passes; the clamped, de-duplicated candidates in the host learner's order; per candidate the histogram of the
// samples above it.  src: -1 = the segment is the identity (level 0), else the idx buffer the level reads.
constexpr int kLearnStage = 4096;   // samples of a node that fit the block's LDS staging
__global__ __launch_bounds__(256) void k_learn_stats(const LearnTreeJobDev *jobs, const LearnNodeDesc *nodes, const uint32_t *first_block, int n_nodes, int src,
                                                     LearnRec *recs) {
    __shared__ int32_t s_v[kLearnStage];
    __shared__ uint8_t s_b[kLearnStage];
    __shared__ int s_h[4][3][256];          // digit histograms, one copy per wavefront of the block (fewer collisions on a few hot bins)
    __shared__ int s_hg[4][3][kLearnBuckets + 1];
    __shared__ int s_mn, s_mx, s_nc;
    __shared__ uint32_t s_pre[3], s_rank[3];
    __shared__ int32_t s_cand[3];
    const uint32_t blk = blockIdx.x;
    int a = 0, z = n_nodes - 1;
    while (a < z) {                         // the last node whose first block is <= blk
        const int mid = (a + z + 1) >> 1;
        if (first_block[mid] <= blk) a = mid; else z = mid - 1;
    }
    const LearnNodeDesc &nd = nodes[a];
    const LearnTreeJobDev &j = jobs[nd.job];
    const int p = (int)(blk - first_block[a]);
    const int tid = threadIdx.x, wv = tid >> 6;
    const int n = nd.n;
    const int32_t *col = j.cols + (int64_t)p * j.n_samples;
    const int32_t *idx = src < 0 ? nullptr : (src ? j.idx1 : j.idx0) + nd.lo;
    const bool staged = n <= kLearnStage;
    LearnRec &rec = recs[blk];
    if (tid == 0) { s_mn = 0x7FFFFFFF; s_mx = (int)0x80000000; }
    __syncthreads();
    int mn = 0x7FFFFFFF, mx = (int)0x80000000;
    for (int i = tid; i < n; i += 256) {
        const int64_t s = idx ? idx[i] : nd.lo + i;
        const int v = col[s];
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
        if (staged) { s_v[i] = v; s_b[i] = (uint8_t)learn_bucket(j.bucket, s); }
    }
    if (mn <= mx) { atomicMin(&s_mn, mn); atomicMax(&s_mx, mx); }
    __syncthreads();
    mn = s_mn; mx = s_mx;
    if (mn == mx || n < 1) {                // (uniform over the block) a constant property has no candidate
        if (tid == 0) { rec.mn = mn; rec.mx = mx; rec.nc = 0; rec.pad = 0; }
        return;
    }
    const uint32_t span = (uint32_t)mx - (uint32_t)mn;     // exact for any two int32
    const int bits = 32 - __builtin_clz(span);               // span >= 1
    if (tid < 3) { s_pre[tid] = 0; s_rank[tid] = (uint32_t)((uint64_t)n * (uint64_t)(tid + 1) / 4); }
    for (int shift = ((bits + 7) / 8 - 1) * 8; shift >= 0; shift -= 8) {
        for (int k = tid; k < 4 * 3 * 256; k += 256) (&s_h[0][0][0])[k] = 0;
        __syncthreads();
        const bool first = shift + 8 >= bits;                // no digit above this one: every sample takes part
        const int up = first ? 0 : shift + 8;                 // (<= 24)
        const uint32_t pre0 = s_pre[0], pre1 = s_pre[1], pre2 = s_pre[2];
        for (int i = tid; i < n; i += 256) {
            const int v = staged ? s_v[i] : col[idx ? idx[i] : nd.lo + i];
            const uint32_t u = (uint32_t)v - (uint32_t)mn;
            const uint32_t hi = first ? 0u : u >> up;
            const int dg = (int)((u >> shift) & 255u);
            if (hi == pre0) atomicAdd(&s_h[wv][0][dg], 1);
            if (hi == pre1) atomicAdd(&s_h[wv][1][dg], 1);
            if (hi == pre2) atomicAdd(&s_h[wv][2][dg], 1);
        }
        __syncthreads();
        if (tid < 3) {                      // the digit that holds rank s_rank[tid] among the samples under the prefix
            uint32_t rank = s_rank[tid], cum = 0;
            int dg = 0;
            for (; dg < 255; dg++) {
                const uint32_t c = (uint32_t)(s_h[0][tid][dg] + s_h[1][tid][dg] + s_h[2][tid][dg] + s_h[3][tid][dg]);
                if (cum + c > rank) break;
                cum += c;
            }
            s_rank[tid] = rank - cum;
            s_pre[tid] = (s_pre[tid] << 8) | (uint32_t)dg;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int nc = 0;
        for (int q = 0; q < 3; q++) {
            int s = (int)((uint32_t)mn + s_pre[q]);
            if (s >= mx) s = mx - 1;
            if (s < mn) s = mn;
            bool dup = false;
            for (int t = 0; t < nc; t++) dup |= (s_cand[t] == s);
            if (!dup) s_cand[nc++] = s;
        }
        s_nc = nc;
    }
    for (int k = tid; k < 4 * 3 * (kLearnBuckets + 1); k += 256) (&s_hg[0][0][0])[k] = 0;
    __syncthreads();
    const int nc = s_nc;
    const int c0 = s_cand[0], c1 = nc > 1 ? s_cand[1] : 0x7FFFFFFF, c2 = nc > 2 ? s_cand[2] : 0x7FFFFFFF;   // (no value is above INT32_MAX)
    for (int i = tid; i < n; i += 256) {
        int v, b;
        if (staged) { v = s_v[i]; b = s_b[i]; }
        else { const int64_t s = idx ? idx[i] : nd.lo + i; v = col[s]; b = learn_bucket(j.bucket, s); }
        if (v > c0) atomicAdd(&s_hg[wv][0][b], 1);
        if (v > c1) atomicAdd(&s_hg[wv][1][b], 1);
        if (v > c2) atomicAdd(&s_hg[wv][2][b], 1);
    }
    __syncthreads();
    if (tid < 3 * kLearnBuckets) {
        const int t = tid / kLearnBuckets, b = tid - t * kLearnBuckets;
        const int h = s_hg[0][t][b] + s_hg[1][t][b] + s_hg[2][t][b] + s_hg[3][t][b];
        rec.c[t].hg[b] = t < nc ? h : 0;
        if (t < nc) atomicAdd(&s_hg[0][t][kLearnBuckets], h);     // the side's size
    }
    __syncthreads();
    if (tid < 3) { rec.c[tid].s = tid < nc ? s_cand[tid] : 0; rec.c[tid].ng = tid < nc ? s_hg[0][tid][kLearnBuckets] : 0; }
    if (tid == 0) { rec.mn = mn; rec.mx = mx; rec.nc = nc; rec.pad = 0; }
}

namespace {
DEV double learn_cost(const int32_t *hist, int n) {   // Learner::cost with the device's log2: an approximation, used for the shortlist only
    if (n <= 0) return 0.0;
    double c = 0.0;
    for (int b = 0; b < kLearnBuckets; b++) if (hist[b]) c -= hist[b] * log2((double)hist[b] / n);
    return c;
}
}  // namespace

// One wavefront per node: the approximate gain of every valid candidate, then (lane 0, in property / candidate order) the shortlist
__global__ __launch_bounds__(64) void k_learn_shortlist(const LearnNodeDesc *nodes, const uint32_t *first_block, const LearnRec *recs, LearnShort *shorts) {
    __shared__ double s_gain[3 * kMaxProps];
    __shared__ int s_valid[3 * kMaxProps];
    const LearnNodeDesc &nd = nodes[blockIdx.x];
    const uint32_t fb = first_block[blockIdx.x];
    int nprops = (int)(first_block[blockIdx.x + 1] - fb);
    nprops = nprops < kMaxProps ? nprops : kMaxProps;
    const int n = nd.n;
    const double parent = learn_cost(nd.hist, n);
    for (int c = threadIdx.x; c < 3 * nprops; c += 64) {
        const int p = c / 3, t = c - 3 * p;
        const LearnRec &rec = recs[fb + p];
        int valid = 0;
        double gain = 0.0;
        if (t < rec.nc) {
            const LearnCand &cd = rec.c[t];
            if (cd.ng >= nd.min_leaf && n - cd.ng >= nd.min_leaf) {
                int32_t hl[kLearnBuckets];
                for (int b = 0; b < kLearnBuckets; b++) hl[b] = nd.hist[b] - cd.hg[b];
                gain = parent - learn_cost(cd.hg, cd.ng) - learn_cost(hl, n - cd.ng);
                valid = 1;
            }
        }
        s_gain[c] = gain; s_valid[c] = valid;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    LearnShort &sh = shorts[blockIdx.x];
    double best = 0.0;
    bool any = false;
    for (int c = 0; c < 3 * nprops; c++)
        if (s_valid[c] && (!any || s_gain[c] > best)) { best = s_gain[c]; any = true; }
    const double floor_gain = best - (double)n * kLearnMargin;
    int count = 0, overflow = 0;
    for (int c = 0; c < 3 * nprops && any; c++) {
        if (!s_valid[c] || s_gain[c] < floor_gain) continue;
        if (count == kLearnShortCap) { overflow = 1; break; }
        const int p = c / 3, t = c - 3 * p;
        const LearnCand &cd = recs[fb + p].c[t];
        LearnShortEntry &e = sh.e[count++];
        e.prop = p; e.s = cd.s; e.ng = cd.ng;
        for (int b = 0; b < kLearnBuckets; b++) e.hg[b] = cd.hg[b];
    }
    sh.count = count; sh.overflow = overflow;
}

// One block per node that splits: the stable partition of its segment, the ng samples with prop > s first, into the other idx buffer
__global__ __launch_bounds__(256) void k_learn_partition(const LearnTreeJobDev *jobs, const LearnSplitDesc *splits, int src) {
    __shared__ int s_scan[2][256];
    const LearnSplitDesc sp = splits[blockIdx.x];
    const LearnTreeJobDev &j = jobs[sp.job];
    const int32_t *col = j.cols + (int64_t)sp.prop * j.n_samples;
    const int32_t *in = src < 0 ? nullptr : (src ? j.idx1 : j.idx0) + sp.lo;
    int32_t *out = (src == 0 ? j.idx1 : j.idx0) + sp.lo;
    const int tid = threadIdx.x;
    int base_gt = 0, base_le = 0;
    for (int i0 = 0; i0 < sp.n; i0 += 256) {
        const int i = i0 + tid;
        int s = 0, flag = 0;
        if (i < sp.n) { s = in ? in[i] : sp.lo + i; flag = col[s] > sp.s ? 1 : 0; }
        int cur = 0;
        s_scan[0][tid] = flag;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {   // inclusive scan of the 256 flags
            s_scan[cur ^ 1][tid] = s_scan[cur][tid] + (tid >= d ? s_scan[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        const int incl = s_scan[cur][tid], total = s_scan[cur][255];
        if (i < sp.n) {
            const int pos = flag ? base_gt + incl - 1 : sp.ng + base_le + (tid - incl);
            if (pos >= 0 && pos < sp.n) out[pos] = s;   // (ng is the count of the same comparison: always inside)
        }
        const int chunk = sp.n - i0 < 256 ? sp.n - i0 : 256;
        base_gt += total; base_le += chunk - total;
        __syncthreads();
    }
}

namespace {
// the kernels as the provider of a level's statistics (csrc/tree_learn.h); the jobs' device table is the caller's
struct GpuLearnProvider : LearnStatsProvider {
    const LearnTreeJobDev *d_jobs = nullptr;
    std::vector<int> nprops;                 // per job
    int src = -1;                            // the idx buffer the next round reads (-1: the identity)
    uint64_t stat_bytes = 0;
    uint8_t *d_nodes = nullptr, *d_recs = nullptr, *d_shorts = nullptr, *d_splits = nullptr;
    size_t cap_nodes = 0, cap_recs = 0, cap_shorts = 0, cap_splits = 0;
    std::vector<uint32_t> first;

    ~GpuLearnProvider() override { hipFree(d_nodes); hipFree(d_recs); hipFree(d_shorts); hipFree(d_splits); }
    static int grow(uint8_t *&p, size_t &cap, size_t want) {
        if (want <= cap) return FUIFGPU_OK;
        hipFree(p); p = nullptr; cap = 0;
        want += want / 2;
        if (hipMalloc((void **)&p, want) != hipSuccess) return FUIFGPU_E_HIP;
        cap = want;
        return FUIFGPU_OK;
    }
    int root_hists(std::vector<int32_t> &hist) override {
        const size_t nj = nprops.size();
        hist.assign(nj * kLearnBuckets, 0);
        if (!nj) return FUIFGPU_OK;
        int32_t *d = nullptr;
        if (hipMalloc((void **)&d, hist.size() * sizeof(int32_t)) != hipSuccess) return FUIFGPU_E_HIP;
        hipLaunchKernelGGL(k_learn_root_hist, dim3((unsigned)nj), dim3(256), 0, nullptr, d_jobs, d);
        int rc = hipGetLastError() == hipSuccess ? FUIFGPU_OK : FUIFGPU_E_HIP;
        if (rc == FUIFGPU_OK && hipMemcpy(hist.data(), d, hist.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = FUIFGPU_E_HIP;
        stat_bytes += hist.size() * sizeof(int32_t);
        hipFree(d);
        return rc;
    }
    int level(const std::vector<LearnNodeDesc> &nodes, std::vector<LearnShort> &shorts) override {
        const size_t nn = nodes.size();
        shorts.assign(nn, LearnShort());
        if (!nn) return FUIFGPU_OK;
        first.assign(nn + 1, 0);
        uint64_t blocks = 0;
        for (size_t k = 0; k < nn; k++) {
            if (nodes[k].job < 0 || (size_t)nodes[k].job >= nprops.size()) return FUIFGPU_E_ARG;
            first[k] = (uint32_t)blocks; blocks += (uint64_t)nprops[(size_t)nodes[k].job];
        }
        first[nn] = (uint32_t)blocks;
        if (blocks > 0x7FFFFFFFull || nn > 0x7FFFFFFFull) return FUIFGPU_E_ARG;
        const size_t off_first = (sizeof(LearnNodeDesc) * nn + 255) / 256 * 256, head = off_first + sizeof(uint32_t) * (nn + 1);
        int rc = grow(d_nodes, cap_nodes, head);
        if (rc == FUIFGPU_OK) rc = grow(d_recs, cap_recs, sizeof(LearnRec) * (size_t)blocks);
        if (rc == FUIFGPU_OK) rc = grow(d_shorts, cap_shorts, sizeof(LearnShort) * nn);
        if (rc != FUIFGPU_OK) return rc;
        std::vector<uint8_t> host(head, 0);
        memcpy(host.data(), nodes.data(), sizeof(LearnNodeDesc) * nn);
        memcpy(host.data() + off_first, first.data(), sizeof(uint32_t) * (nn + 1));
        if (hipMemcpy(d_nodes, host.data(), head, hipMemcpyHostToDevice) != hipSuccess) return FUIFGPU_E_HIP;
        const LearnNodeDesc *dn = reinterpret_cast<const LearnNodeDesc *>(d_nodes);
        const uint32_t *df = reinterpret_cast<const uint32_t *>(d_nodes + off_first);
        hipLaunchKernelGGL(k_learn_stats, dim3((unsigned)blocks), dim3(256), 0, nullptr, d_jobs, dn, df, (int)nn, src, reinterpret_cast<LearnRec *>(d_recs));
        hipLaunchKernelGGL(k_learn_shortlist, dim3((unsigned)nn), dim3(64), 0, nullptr, dn, df, reinterpret_cast<const LearnRec *>(d_recs),
                           reinterpret_cast<LearnShort *>(d_shorts));
        if (hipGetLastError() != hipSuccess) return FUIFGPU_E_HIP;
        if (hipMemcpy(shorts.data(), d_shorts, sizeof(LearnShort) * nn, hipMemcpyDeviceToHost) != hipSuccess) return FUIFGPU_E_HIP;   // synchronises
        stat_bytes += sizeof(LearnShort) * nn;
        return FUIFGPU_OK;
    }
    int full_slice(size_t node, std::vector<LearnRec> &recs) override {
        if (node + 1 >= first.size()) return FUIFGPU_E_ARG;
        recs.assign((size_t)(first[node + 1] - first[node]), LearnRec());
        if (recs.empty()) return FUIFGPU_OK;
        if (hipMemcpy(recs.data(), d_recs + sizeof(LearnRec) * (size_t)first[node], sizeof(LearnRec) * recs.size(), hipMemcpyDeviceToHost) != hipSuccess) return FUIFGPU_E_HIP;
        stat_bytes += sizeof(LearnRec) * recs.size();
        return FUIFGPU_OK;
    }
    int partition(const std::vector<LearnSplitDesc> &splits) override {
        if (!splits.empty()) {
            const int rc = grow(d_splits, cap_splits, sizeof(LearnSplitDesc) * splits.size());
            if (rc != FUIFGPU_OK) return rc;
            if (hipMemcpy(d_splits, splits.data(), sizeof(LearnSplitDesc) * splits.size(), hipMemcpyHostToDevice) != hipSuccess) return FUIFGPU_E_HIP;
            hipLaunchKernelGGL(k_learn_partition, dim3((unsigned)splits.size()), dim3(256), 0, nullptr, d_jobs, reinterpret_cast<const LearnSplitDesc *>(d_splits), src);
            if (hipGetLastError() != hipSuccess) return FUIFGPU_E_HIP;
        }
        src = src == 0 ? 1 : 0;
        return FUIFGPU_OK;
    }
};

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// jobs[a, b) in one arena: [LearnTreeJobDev][LearnJobDev][first blocks][per job: columns, buckets, idx0, idx1]
int learn_trees_chunk(std::vector<LearnTreeJob> &jobs, size_t a, size_t b, uint64_t *stat_bytes) {
    const size_t nj = b - a;
    const size_t off_sample = up256(sizeof(LearnTreeJobDev) * nj), off_first = off_sample + up256(sizeof(LearnJobDev) * nj);
    const size_t head = off_first + up256(sizeof(uint32_t) * (nj + 1));
    size_t total = head;
    std::vector<size_t> off_cols(nj), off_bucket(nj), off_idx(nj);
    std::vector<uint8_t> host(head, 0);
    uint32_t *first = reinterpret_cast<uint32_t *>(host.data() + off_first);
    uint64_t blocks = 0;
    for (size_t k = 0; k < nj; k++) {
        const LearnJob &j = jobs[a + k].sample;
        const int64_t npix = (int64_t)j.g.w * j.g.h;
        if (!j.g.plane || j.g.w < 1 || j.g.h < 1 || j.g.nrefs < 0 || j.g.nrefs > kMaxRefs || j.nprops != 2 * j.g.nrefs + kNonRefProps || j.stride < 1 ||
            j.n_samples != (npix + j.stride - 1) / j.stride || j.n_samples > 0x7FFFFFFF)
            return FUIFGPU_E_ARG;
        const size_t n = (size_t)j.n_samples;
        off_cols[k] = total; total += up256(n * (size_t)j.nprops * sizeof(int32_t));
        off_bucket[k] = total; total += up256(n);
        off_idx[k] = total; total += 2 * up256(n * sizeof(int32_t));
        first[k] = (uint32_t)blocks; blocks += ((uint64_t)n + 255) / 256;
    }
    first[nj] = (uint32_t)blocks;
    if (blocks > 0x7FFFFFFFull) return FUIFGPU_E_ARG;
    uint8_t *arena = nullptr;
    if (hipMalloc((void **)&arena, total) != hipSuccess) return FUIFGPU_E_HIP;
    LearnTreeJobDev *h_tree = reinterpret_cast<LearnTreeJobDev *>(host.data());
    LearnJobDev *h_sample = reinterpret_cast<LearnJobDev *>(host.data() + off_sample);
    GpuLearnProvider gp;
    std::vector<LevelJob> lj(nj);
    for (size_t k = 0; k < nj; k++) {
        const LearnTreeJob &j = jobs[a + k];
        const size_t n = (size_t)j.sample.n_samples;
        LearnJobDev &d = h_sample[k];
        d.g = j.sample.g; d.n_samples = j.sample.n_samples; d.stride = j.sample.stride; d.nprops = j.sample.nprops; d.pad = 0;
        d.props = reinterpret_cast<int32_t *>(arena + off_cols[k]);
        d.bucket = arena + off_bucket[k];
        LearnTreeJobDev &t = h_tree[k];
        t.cols = d.props; t.bucket = d.bucket;
        t.idx0 = reinterpret_cast<int32_t *>(arena + off_idx[k]);
        t.idx1 = reinterpret_cast<int32_t *>(arena + off_idx[k] + up256(n * sizeof(int32_t)));
        t.n_samples = j.sample.n_samples; t.nprops = j.sample.nprops; t.pad = 0;
        gp.nprops.push_back(j.sample.nprops);
        lj[k].n_samples = j.sample.n_samples; lj[k].nprops = j.sample.nprops; lj[k].prm = j.prm;
    }
    int rc = hipMemcpy(arena, host.data(), head, hipMemcpyHostToDevice) == hipSuccess ? FUIFGPU_OK : FUIFGPU_E_HIP;
    if (rc == FUIFGPU_OK && blocks) {
        hipLaunchKernelGGL(k_learn_samples_cols_jobs, dim3((unsigned)blocks), dim3(256), 0, nullptr, reinterpret_cast<const LearnJobDev *>(arena + off_sample),
                           reinterpret_cast<const uint32_t *>(arena + off_first), (int)nj);
        if (hipGetLastError() != hipSuccess) rc = FUIFGPU_E_HIP;
    }
    if (rc == FUIFGPU_OK) {
        gp.d_jobs = reinterpret_cast<const LearnTreeJobDev *>(arena);
        rc = learn_levelwise(lj, gp);
    }
    if (rc == FUIFGPU_OK) for (size_t k = 0; k < nj; k++) jobs[a + k].nodes.swap(lj[k].nodes);
    if (stat_bytes) *stat_bytes += gp.stat_bytes;
    if (hipDeviceSynchronize() != hipSuccess && rc == FUIFGPU_OK) rc = FUIFGPU_E_HIP;   // nothing of the chunk runs once its arena goes
    hipFree(arena);
    return rc;
}
}  // namespace

int learn_trees_gpu(std::vector<LearnTreeJob> &jobs, uint64_t *stat_bytes_d2h) {
    if (stat_bytes_d2h) *stat_bytes_d2h = 0;
    if (jobs.empty()) return FUIFGPU_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return FUIFGPU_E_HIP;
    const size_t budget = free_b / 4;   // a chunk is a run of consecutive jobs; every tree is learned on its own, so the chunking changes no result
    // samples, buckets, the two idx buffers; the records of a level (at most n / (2 * min_leaf) active nodes of nprops records) on top
    auto bytes_of = [](const LearnTreeJob &j) {
        const size_t n = (size_t)(j.sample.n_samples > 0 ? j.sample.n_samples : 0), np = (size_t)(j.sample.nprops > 0 ? j.sample.nprops : 0);
        const size_t leaf = (size_t)(j.prm.min_leaf > 0 ? j.prm.min_leaf : 1);
        return n * (4 * np + 9) + (n / (2 * leaf) + 1) * (np * sizeof(LearnRec) + sizeof(LearnShort));
    };
    for (size_t a = 0; a < jobs.size();) {
        size_t b = a + 1, sum = bytes_of(jobs[a]);
        while (b < jobs.size() && sum + bytes_of(jobs[b]) <= budget) sum += bytes_of(jobs[b++]);
        const int rc = learn_trees_chunk(jobs, a, b, stat_bytes_d2h);
        if (rc != FUIFGPU_OK) return rc;
        a = b;
    }
    return FUIFGPU_OK;
}

int learn_tree_rows_gpu(const int32_t *rows_device, const uint8_t *bucket_device, int64_t n_samples, int nprops, const LearnParams &prm,
                        std::vector<LearnNode> &nodes) {
    nodes.assign(1, LearnNode());
    if (n_samples < 0 || n_samples > 0x7FFFFFFF || nprops < 1 || nprops >= kMaxProps) return FUIFGPU_E_ARG;
    if (n_samples == 0) return FUIFGPU_OK;
    if (!rows_device || !bucket_device) return FUIFGPU_E_ARG;
    const size_t n = (size_t)n_samples;
    const size_t off_cols = up256(sizeof(LearnTreeJobDev)), off_idx = off_cols + up256(n * (size_t)nprops * sizeof(int32_t));
    const size_t total = off_idx + 2 * up256(n * sizeof(int32_t));
    uint8_t *arena = nullptr;
    if (hipMalloc((void **)&arena, total) != hipSuccess) return FUIFGPU_E_HIP;
    LearnTreeJobDev t;
    t.cols = reinterpret_cast<int32_t *>(arena + off_cols); t.bucket = bucket_device;
    t.idx0 = reinterpret_cast<int32_t *>(arena + off_idx); t.idx1 = reinterpret_cast<int32_t *>(arena + off_idx + up256(n * sizeof(int32_t)));
    t.n_samples = n_samples; t.nprops = nprops; t.pad = 0;
    int rc = hipMemcpy(arena, &t, sizeof(t), hipMemcpyHostToDevice) == hipSuccess ? FUIFGPU_OK : FUIFGPU_E_HIP;
    const uint64_t blocks = ((uint64_t)n * (uint64_t)nprops + 255) / 256;
    if (blocks > 0x7FFFFFFFull) rc = FUIFGPU_E_ARG;
    if (rc == FUIFGPU_OK) {
        hipLaunchKernelGGL(k_learn_transpose, dim3((unsigned)blocks), dim3(256), 0, nullptr, rows_device, reinterpret_cast<int32_t *>(arena + off_cols), n_samples, nprops);
        if (hipGetLastError() != hipSuccess) rc = FUIFGPU_E_HIP;
    }
    if (rc == FUIFGPU_OK) {
        GpuLearnProvider gp;
        gp.d_jobs = reinterpret_cast<const LearnTreeJobDev *>(arena);
        gp.nprops.push_back(nprops);
        std::vector<LevelJob> lj(1);
        lj[0].n_samples = n_samples; lj[0].nprops = nprops; lj[0].prm = prm;
        rc = learn_levelwise(lj, gp);
        if (rc == FUIFGPU_OK) nodes.swap(lj[0].nodes);
    }
    if (hipDeviceSynchronize() != hipSuccess && rc == FUIFGPU_OK) rc = FUIFGPU_E_HIP;
    hipFree(arena);
    return rc;
}

// ---------------------------------------------------------------------------------------------
void EncScratch::release() {
    hipFree(d_guess); hipFree(d_leaf); hipFree(d_bytes); hipFree(d_tree); hipFree(d_leaves); hipFree(d_table); hipFree(d_state);
    *this = EncScratch();
}

int maniac_encode_group_gpu(const EncGroup &g, const EncNode *tree, int n_nodes, int n_leaves, const uint16_t *leaf_init, const uint16_t *pixel_table,
                            RacEncState *state, std::vector<uint8_t> &out, EncScratch &s) {
    if (!g.plane || !tree || n_nodes < 1 || n_leaves < 1 || !leaf_init || !pixel_table || !state || g.w < 1 || g.h < 1 || g.nrefs < 0 || g.nrefs > kMaxRefs)
        return FUIFGPU_E_ARG;
    const size_t n = (size_t)g.w * g.h;
#define ECHK(call) do { if ((call) != hipSuccess) return FUIFGPU_E_HIP; } while (0)
    if (n > s.pixel_cap) {
        hipFree(s.d_guess); hipFree(s.d_leaf); s.d_guess = s.d_leaf = nullptr; s.pixel_cap = 0;
        ECHK(hipMalloc((void **)&s.d_guess, n * 4)); ECHK(hipMalloc((void **)&s.d_leaf, n * 4));
        s.pixel_cap = n;
    }
    // a symbol is at most 1 + 1 + 14 + 14 binary decisions, each well under a byte after renormalisation: 4 bytes per sample is generous
    const size_t bytes_cap = std::min<size_t>(n * 4 + 1024, 0xFFFFFF00u);
    if (bytes_cap > s.bytes_cap) {
        hipFree(s.d_bytes); s.d_bytes = nullptr; s.bytes_cap = 0;
        ECHK(hipMalloc((void **)&s.d_bytes, bytes_cap));
        s.bytes_cap = bytes_cap;
    }
    if ((size_t)n_nodes > s.tree_cap) {
        hipFree(s.d_tree); s.d_tree = nullptr; s.tree_cap = 0;
        ECHK(hipMalloc((void **)&s.d_tree, sizeof(EncNode) * (size_t)n_nodes));
        s.tree_cap = (size_t)n_nodes;
    }
    if ((size_t)n_leaves > s.leaves_cap) {
        hipFree(s.d_leaves); s.d_leaves = nullptr; s.leaves_cap = 0;
        ECHK(hipMalloc((void **)&s.d_leaves, sizeof(uint16_t) * CH_N * (size_t)n_leaves));
        s.leaves_cap = (size_t)n_leaves;
    }
    if (!s.d_table) ECHK(hipMalloc((void **)&s.d_table, sizeof(uint16_t) * 8192));
    if (!s.d_state) ECHK(hipMalloc((void **)&s.d_state, sizeof(uint32_t) * 8));
    std::vector<uint16_t> leaves((size_t)n_leaves * CH_N);
    for (int l = 0; l < n_leaves; l++) memcpy(&leaves[(size_t)l * CH_N], leaf_init, sizeof(uint16_t) * CH_N);
    uint32_t st[8] = {state->range, state->low, (uint32_t)state->delayed, (uint32_t)state->pending, 0, 0, 0, 0};
    ECHK(hipMemcpy(s.d_tree, tree, sizeof(EncNode) * (size_t)n_nodes, hipMemcpyHostToDevice));
    ECHK(hipMemcpy(s.d_leaves, leaves.data(), sizeof(uint16_t) * leaves.size(), hipMemcpyHostToDevice));
    ECHK(hipMemcpy(s.d_table, pixel_table, sizeof(uint16_t) * 8192, hipMemcpyHostToDevice));
    ECHK(hipMemcpy(s.d_state, st, sizeof(st), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_enc_model, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, g, s.d_tree, n_nodes, s.d_guess, s.d_leaf);
    hipLaunchKernelGGL(k_enc_rac, dim3(1), dim3(64), 0, nullptr, g.plane, s.d_guess, s.d_leaf, (int64_t)n, g.minval, g.maxval, s.d_leaves, s.d_table, s.d_state,
                       s.d_bytes, (uint32_t)s.bytes_cap);
    ECHK(hipGetLastError());
    ECHK(hipMemcpy(st, s.d_state, sizeof(st), hipMemcpyDeviceToHost));   // synchronises with the null stream's kernels
    if (st[5]) return FUIFGPU_E_NOMEM;
    const size_t old = out.size();
    out.resize(old + st[4]);
    if (st[4]) ECHK(hipMemcpy(out.data() + old, s.d_bytes, st[4], hipMemcpyDeviceToHost));
    state->range = st[0]; state->low = st[1]; state->delayed = (int32_t)st[2]; state->pending = (int32_t)st[3];
#undef ECHK
    return FUIFGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// the bodies of all jobs, packed back to back (one block per job copies out[0 .. state[4]) to dst + offset[job])
__global__ __launch_bounds__(256) void k_enc_gather(const EncJobDev *jobs, const uint64_t *offset, uint8_t *dst) {
    const EncJobDev &j = jobs[blockIdx.x];
    const uint32_t n = j.state[4] < j.out_cap ? j.state[4] : j.out_cap;
    uint8_t *d = dst + offset[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += 256) d[i] = j.out[i];
}

// A batch: one device arena for all jobs.  Its head -- job table, chance table, every job's tree, leaf chances and coder state --
// is assembled on the host and uploaded in ONE copy; the states come back in one copy, the bodies are packed by k_enc_gather
// and come back in one more (a 1024-picture batch has ~62 000 jobs: per-job copies would cost seconds).
int maniac_encode_jobs_gpu(std::vector<EncJob> &jobs, const uint16_t *pixel_table) {
    if (!pixel_table) return FUIFGPU_E_ARG;
    if (jobs.empty()) return FUIFGPU_OK;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t nj = jobs.size();
    // layout of the head: [EncJobDev x nj][table][states: 32 bytes x nj][per job: tree, leaves]; then per job: guess, leaf, out;
    // then the offsets and the packed bodies
    const size_t off_table = up(sizeof(EncJobDev) * nj), off_states = off_table + up(sizeof(uint16_t) * 8192);
    size_t head = off_states + up(32 * nj);
    std::vector<size_t> off_tree(nj), off_leaves(nj);
    for (size_t k = 0; k < nj; k++) {
        const EncJob &j = jobs[k];
        if (!j.g.plane || j.tree.empty() || j.n_leaves < 1 || j.g.w < 1 || j.g.h < 1 || j.g.nrefs < 0 || j.g.nrefs > kMaxRefs) return FUIFGPU_E_ARG;
        off_tree[k] = head; head += up(sizeof(EncNode) * j.tree.size());
        off_leaves[k] = head; head += up(sizeof(uint16_t) * CH_N * (size_t)j.n_leaves);
    }
    size_t total = head;
    std::vector<size_t> off_guess(nj), off_leaf(nj), off_out(nj);
    std::vector<uint32_t> cap(nj);
    for (size_t k = 0; k < nj; k++) {
        const size_t n = (size_t)jobs[k].g.w * jobs[k].g.h;
        // a symbol is at most 1 + 1 + 14 + 14 binary decisions, each well under a byte after renormalisation: 4 bytes per sample is generous
        cap[k] = (uint32_t)std::min<size_t>(n * 4 + 1024, 0xFFFFFF00u);
        off_guess[k] = total; total += up(n * 4);
        off_leaf[k] = total; total += up(n * 4);
        off_out[k] = total; total += up(cap[k]);
    }
    const size_t off_offsets = total; total += up(sizeof(uint64_t) * nj);
    const size_t off_first = total; total += up(sizeof(uint32_t) * (nj + 1));
    uint8_t *arena = nullptr;
    if (hipMalloc((void **)&arena, total) != hipSuccess) return FUIFGPU_E_HIP;
    int rc = FUIFGPU_OK;
#define ECHK(call) do { if (rc == FUIFGPU_OK && (call) != hipSuccess) rc = FUIFGPU_E_HIP; } while (0)
    std::vector<uint8_t> host(head, 0);
    EncJobDev *h_jobs = reinterpret_cast<EncJobDev *>(host.data());
    memcpy(host.data() + off_table, pixel_table, sizeof(uint16_t) * 8192);
    for (size_t k = 0; k < nj; k++) {
        const EncJob &j = jobs[k];
        EncJobDev &d = h_jobs[k];
        d.g = j.g; d.n = (int64_t)j.g.w * j.g.h; d.n_nodes = (int32_t)j.tree.size(); d.pad = 0; d.pad2 = 0;
        d.tree = reinterpret_cast<const EncNode *>(arena + off_tree[k]);
        d.leaves = reinterpret_cast<uint16_t *>(arena + off_leaves[k]);
        d.state = reinterpret_cast<uint32_t *>(arena + off_states + 32 * k);
        d.guess = reinterpret_cast<int32_t *>(arena + off_guess[k]);
        d.leaf = reinterpret_cast<int32_t *>(arena + off_leaf[k]);
        d.out = arena + off_out[k];
        d.out_cap = cap[k];
        memcpy(host.data() + off_tree[k], j.tree.data(), sizeof(EncNode) * j.tree.size());
        for (int l = 0; l < j.n_leaves; l++) memcpy(host.data() + off_leaves[k] + sizeof(uint16_t) * CH_N * (size_t)l, j.leaf_init, sizeof(uint16_t) * CH_N);
        const uint32_t st[8] = {j.state.range, j.state.low, (uint32_t)j.state.delayed, (uint32_t)j.state.pending, 0, 0, 0, 0};
        memcpy(host.data() + off_states + 32 * k, st, sizeof(st));
    }
    ECHK(hipMemcpy(arena, host.data(), head, hipMemcpyHostToDevice));
    const EncJobDev *d_jobs = reinterpret_cast<const EncJobDev *>(arena);
    const uint16_t *d_table = reinterpret_cast<const uint16_t *>(arena + off_table);
    if (rc == FUIFGPU_OK) {
        std::vector<uint32_t> first(nj + 1);
        uint64_t blocks = 0;
        for (size_t k = 0; k < nj; k++) { first[k] = (uint32_t)blocks; blocks += ((uint64_t)jobs[k].g.w * jobs[k].g.h + 255) / 256; }
        first[nj] = (uint32_t)blocks;
        if (blocks > 0x7FFFFFFFull) rc = FUIFGPU_E_ARG;   // > 5 * 10^11 pixels in one batch: split it
        ECHK(hipMemcpy(arena + off_first, first.data(), sizeof(uint32_t) * (nj + 1), hipMemcpyHostToDevice));
        if (rc == FUIFGPU_OK) {   // the coder reads what the model kernel wrote: it only runs behind it (never on uninitialised guesses)
            hipLaunchKernelGGL(k_enc_model_jobs, dim3((unsigned)blocks), dim3(256), 0, nullptr, d_jobs, reinterpret_cast<const uint32_t *>(arena + off_first), (int)nj);
            hipLaunchKernelGGL(k_enc_rac_jobs, dim3((unsigned)nj), dim3(64), 0, nullptr, d_jobs, d_table);
            ECHK(hipGetLastError());
        }
    }
    std::vector<uint32_t> states(8 * nj);
    ECHK(hipMemcpy(states.data(), arena + off_states, 32 * nj, hipMemcpyDeviceToHost));   // synchronises with the null stream's kernels
    std::vector<uint64_t> offsets(nj);
    uint64_t packed = 0;
    for (size_t k = 0; k < nj && rc == FUIFGPU_OK; k++) {
        if (states[8 * k + 5]) rc = FUIFGPU_E_NOMEM;
        offsets[k] = packed;
        packed += states[8 * k + 4];
    }
    if (rc == FUIFGPU_OK && packed) {
        uint8_t *d_packed = nullptr;
        if (hipMalloc((void **)&d_packed, packed) != hipSuccess) rc = FUIFGPU_E_HIP;
        ECHK(hipMemcpy(arena + off_offsets, offsets.data(), sizeof(uint64_t) * nj, hipMemcpyHostToDevice));
        if (rc == FUIFGPU_OK) {
            hipLaunchKernelGGL(k_enc_gather, dim3((unsigned)nj), dim3(256), 0, nullptr, d_jobs, reinterpret_cast<const uint64_t *>(arena + off_offsets), d_packed);
            ECHK(hipGetLastError());
        }
        std::vector<uint8_t> all(packed);
        ECHK(hipMemcpy(all.data(), d_packed, packed, hipMemcpyDeviceToHost));
        if (rc == FUIFGPU_OK)
            for (size_t k = 0; k < nj; k++) jobs[k].body.assign(all.begin() + offsets[k], all.begin() + offsets[k] + states[8 * k + 4]);
        hipFree(d_packed);
    }
    for (size_t k = 0; k < nj && rc == FUIFGPU_OK; k++)
        jobs[k].state = RacEncState{states[8 * k], states[8 * k + 1], (int32_t)states[8 * k + 2], (int32_t)states[8 * k + 3]};
#undef ECHK
    hipFree(arena);
    return rc;
}

}  // namespace fuifgpu
