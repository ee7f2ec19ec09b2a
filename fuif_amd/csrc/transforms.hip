// fuif_amd/csrc/transforms.hip -- inverse-transform kernels of the FUIF decode path for gfx950.
//
// All of these are integer/FP64 streaming kernels bound by HBM bandwidth; none is GEMM-shaped, so
// no MFMA.  Planes are row-major int32.  One launch processes one schedule op for a whole chunk
// of images: grid.z = image, address = base[buf] + z*stride[buf] + plane offset.
//
//   k_inv_vsqueeze   transform/squeeze.h:173-224   one lane per column, serial down the rows
//   k_inv_hsqueeze_rows  transform/squeeze.h:81-132  one lane per row (the recurrence runs along x), a cache line per step
//   k_inv_ycocg      transform/ycocg.h:49-61       elementwise on three planes (+ clamp)
//   k_inv_ycbcr      transform/ycbcr.h:49-60       float operands, double arithmetic, no FMA
//   k_dequant        transform/quantize.h:32-49    elementwise * Channel::q (per image, per plane)
//
// The reference's samples are pixel_type = int16_t (image/image.h:35).  The planes here are int32 containers of such values: the unsqueeze
// kernels (squeeze_arith.h: unsqueeze_step), k_dequant and the dequantising load of k_idct8x8 store what an assignment to pixel_type keeps
// (narrow16); the other kernels' results fit 16 bits for int16 inputs (clamps, copies, averages) or are outside the reference's defined
// behaviour when they do not (the iDCT's round() into pixel_type, dct.h:289).  k_inv_approx and the soft-match kernels narrow their sums likewise
// (approximate.h:53-55, 2dmatch.h:129,155).
//   k_idct8x8        transform/dct.h:88-107,282-291 FP64, reference summation order, no FMA
//   k_upsample       transform/subsample.h:90-115  "fancy" 2x chroma upsampling
//   k_clamp / k_copy_clamp   image/image.cpp:107-113
//   k_inv_palette    transform/palette.h:57-64     gather through the decoded palette meta-channel
//   k_permute_plane  transform/permute.h:31-54     plane gather by a permutation that is stream data (meta-channel form)
//   k_inv_approx     transform/approximate.h:44-57 quotient * q + remainder, in place
//   k_inv_match_frames  transform/2dmatch.h:147-171  copy / add the co-located sample of an earlier frame
//   k_pack_samples   export/write_pam.h:136-150    interleaved 8/16-bit samples of the final planes (what a PNM/PAM holds)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "fuifgpu_internal.h"
#include "transforms.h"
#include "squeeze_arith.h"

// The reference's x86-64 build has no fused multiply-add: every product and every sum of the FP64 paths (iDCT, YCbCr) is rounded
// on its own.  hipcc fuses a*b+c into v_fma_f64 by default, in the backend, also through __dmul_rn / __dadd_rn (plain operators
// in HIP) and whatever `#pragma clang fp contract(off)` says: this file MUST be compiled with -ffp-contract=off
// (fuif_amd.HIPCC_FLAGS; tests/test_abi_and_plan.py checks the ISA).  Rounds 1-2 shipped contracted code; it passed every
// fixture because a last-bit difference in a double only shows when the value sits within ~1e-13 of a rounding boundary of the
// integer result.

namespace fuifgpu {

namespace {

#define DEV __device__ __forceinline__

DEV int32_t *plane_ptr(const Bases &b, const PlaneRef &p, int z) { return b.base[p.buf] + (int64_t)z * b.stride[p.buf] + p.off; }
// a squeeze residual: TR = int32_t -> like every other plane; TR = coef_t -> the coded plane itself, int16 samples in the coefficient slab (Op::r16)
template <typename TR> DEV const TR *residual_ptr(const Bases &b, const PlaneRef &p, int z);
template <> DEV const int32_t *residual_ptr<int32_t>(const Bases &b, const PlaneRef &p, int z) { return plane_ptr(b, p, z); }
template <> DEV const coef_t *residual_ptr<coef_t>(const Bases &b, const PlaneRef &p, int z) { return b.c16 + (int64_t)z * b.stride[BUF_COEF] + p.off; }
DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

// ---------------------------------------------------------------------------------------------
// vertical unsqueeze: avg (w x h1) + residual (w x h2) -> out (w x (h1+h2)), h1-h2 in {0,1}
constexpr int VS_STEP = 8;
template <typename TR>
__global__ __launch_bounds__(256) void k_inv_vsqueeze(Bases b, PlaneRef pa, PlaneRef pr, PlaneRef po, int clamp, int lo, int hi) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int w = pa.w, h1 = pa.h, h2 = pr.h;
    if (x >= w) return;
    const int32_t *a = plane_ptr(b, pa, blockIdx.z) + x;
    const TR *r = residual_ptr<TR>(b, pr, blockIdx.z) + x;
    int32_t *o = plane_ptr(b, po, blockIdx.z) + x;
    int avg = a[0];
    int prevB = avg;  // first pair uses tendency(avg,avg,next): squeeze.h:186
    int y = 0;
    // VS_STEP row pairs per step, their loads issued together (the recurrence down the column is serial: with one pair per
    // step a lane has a single pair of loads in flight)
    for (; y + VS_STEP < h1 && y + VS_STEP <= h2; y += VS_STEP) {   // avg rows y+1 .. y+VS_STEP all exist
        int nv[VS_STEP], rv[VS_STEP];
#pragma unroll
        for (int k = 0; k < VS_STEP; k++) {
            nv[k] = a[(int64_t)(y + 1 + k) * w];
            rv[k] = r[(int64_t)(y + k) * w];
        }
#pragma unroll
        for (int k = 0; k < VS_STEP; k++) {
            int A, B;
            unsqueeze_step(prevB, avg, nv[k], rv[k], A, B);
            o[(int64_t)(2 * (y + k)) * w] = clamp ? clampi(A, lo, hi) : A;
            o[(int64_t)(2 * (y + k) + 1) * w] = clamp ? clampi(B, lo, hi) : B;
            prevB = B;
            avg = nv[k];
        }
    }
    for (; y < h2; y++) {
        const int next_avg = (y + 1 < h1) ? a[(int64_t)(y + 1) * w] : avg;
        const int res = r[(int64_t)y * w];
        int A, B;
        unsqueeze_step(prevB, avg, next_avg, res, A, B);
        o[(int64_t)(2 * y) * w] = clamp ? clampi(A, lo, hi) : A;
        o[(int64_t)(2 * y + 1) * w] = clamp ? clampi(B, lo, hi) : B;
        prevB = B;
        avg = next_avg;
    }
    if ((h1 + h2) & 1) {  // squeeze.h:217-222
        const int v = a[(int64_t)(h1 - 1) * w];
        o[(int64_t)(2 * (h1 - 1)) * w] = clamp ? clampi(v, lo, hi) : v;
    }
}

// ---------------------------------------------------------------------------------------------
// horizontal unsqueeze: avg (w1 x h) + residual (w2 x h) -> out ((w1+w2) x h), w1-w2 in {0,1}.
// The row recurrence (left = previous B) is serial along x, so lanes own rows: one lane per row, HS_STEP pairs per step.
// A lane walks its own row, so one load instruction touches 64 rows and 64 cache lines; all loads of a step are issued
// before the first use, so every 128-byte line a lane opens is fetched from L2 once and finished from L1 while it is
// still there.  No LDS, no barriers.  Measured on 256 x 4K (profiles/r2_priority_and_balance.txt, r2_transforms.txt): the
// round-1 kernel (64 rows x 32 pairs staged through 33 KB of LDS, 4 wavefronts per CU, three phases between barriers)
// 87.6 ms for the whole inverse schedule; this kernel with 4 pairs per step 68.0 ms (every line re-fetched up to 8
// times); with 32 pairs per step 49.3 ms.
struct __attribute__((packed, aligned(4))) Int4U { int32_t v[4]; };
struct __attribute__((packed, aligned(2))) Short4U { int16_t v[4]; };
// four consecutive residuals (any 4-byte / 2-byte aligned address): one 16-byte or one 8-byte load
DEV Int4U load4(const int32_t *p) { return *reinterpret_cast<const Int4U *>(p); }
DEV Int4U load4(const coef_t *p) {
    const Short4U s = *reinterpret_cast<const Short4U *>(p);
    Int4U v; v.v[0] = s.v[0]; v.v[1] = s.v[1]; v.v[2] = s.v[2]; v.v[3] = s.v[3];
    return v;
}
constexpr int HS_STEP = 32;   // pairs per step = one 128-byte line of each input row, two of the output row
template <typename TR>
__global__ __launch_bounds__(256) void k_inv_hsqueeze_rows(Bases b, PlaneRef pa, PlaneRef pr, PlaneRef po, int clamp, int lo, int hi) {
    const int y = blockIdx.x * 256 + threadIdx.x;
    const int w1 = pa.w, w2 = pr.w, h = pa.h, wo = w1 + w2;
    if (y >= h) return;
    const int32_t *a = plane_ptr(b, pa, blockIdx.z) + (int64_t)y * w1;
    const TR *r = residual_ptr<TR>(b, pr, blockIdx.z) + (int64_t)y * w2;
    int32_t *o = plane_ptr(b, po, blockIdx.z) + (int64_t)y * wo;
    int avg = a[0];
    int left = avg;   // first pair: tendency(avg, avg, next), squeeze.h:89
    int x = 0;
    for (; x + HS_STEP < w1 && x + HS_STEP <= w2; x += HS_STEP) {   // avg[x+1 .. x+HS_STEP] all exist
        Int4U rv[HS_STEP / 4], nv[HS_STEP / 4];
#pragma unroll
        for (int q = 0; q < HS_STEP / 4; q++) {
            rv[q] = load4(r + x + 4 * q);
            nv[q] = *reinterpret_cast<const Int4U *>(a + x + 1 + 4 * q);
        }
#pragma unroll
        for (int q = 0; q < HS_STEP / 4; q++) {
            Int4U o0, o1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int next_avg = nv[q].v[k];
                int A, B;
                unsqueeze_step(left, avg, next_avg, rv[q].v[k], A, B);
                left = B;
                avg = next_avg;
                if (clamp) { A = clampi(A, lo, hi); B = clampi(B, lo, hi); }
                if (k < 2) { o0.v[2 * k] = A; o0.v[2 * k + 1] = B; } else { o1.v[2 * k - 4] = A; o1.v[2 * k - 3] = B; }
            }
            *reinterpret_cast<Int4U *>(o + 2 * (x + 4 * q)) = o0;
            *reinterpret_cast<Int4U *>(o + 2 * (x + 4 * q) + 4) = o1;
        }
    }
    for (; x < w2; x++) {
        const int next_avg = x + 1 < w1 ? a[x + 1] : avg;   // squeeze.h:100
        int A, B;
        unsqueeze_step(left, avg, next_avg, r[x], A, B);
        o[2 * x] = clamp ? clampi(A, lo, hi) : A;
        o[2 * x + 1] = clamp ? clampi(B, lo, hi) : B;
        left = B;
        avg = next_avg;
    }
    if (wo & 1) {  // squeeze.h:129
        const int v = a[w1 - 1];
        o[wo - 1] = clamp ? clampi(v, lo, hi) : v;
    }
}

// The same recurrence with COALESCED global accesses: one wavefront (= one workgroup, so __syncthreads() is wave-local) owns 64
// rows and moves them in tiles of 64 rows x HL_P pairs through its own LDS tile.  Load: 8 lanes fetch the 128 bytes of one
// input row (16 bytes each), 8 rows per instruction; each lane then reads ITS row out of LDS, runs the HL_P pairs, puts the
// 2*HL_P outputs back into LDS (the output tile aliases the input tiles: every lane holds its inputs in registers by then)
// and the tile is written out 16 lanes per 256-byte output row.  Row pitches of 36 / 68 words keep the b128 LDS accesses of
// 16 neighbouring lanes on different banks.
constexpr int HL_P = 32;                   // pairs per tile row: 128-byte input segments, 18 KB of LDS
constexpr int HL_IN_LANES = HL_P / 4;      // lanes that fetch one input row segment (16 bytes each)
constexpr int HL_IN_STEPS = HL_P / 4;      // load instructions per input tile: 64 rows / (64 / HL_IN_LANES) rows per instruction
constexpr int HL_OUT_LANES = HL_P / 2, HL_OUT_STEPS = HL_P / 2;
constexpr int HL_IN_PITCH = HL_P + 4;        // words
constexpr int HL_OUT_PITCH = 2 * HL_P + 4;
template <typename TR>
__global__ __launch_bounds__(64) void k_inv_hsqueeze_tiles(Bases b, PlaneRef pa, PlaneRef pr, PlaneRef po, int clamp, int lo, int hi) {
    __shared__ __attribute__((aligned(16))) int32_t tile[2 * 64 * HL_IN_PITCH];   // HL_P = 32: 18432 bytes; the 64 x 68-word output tile needs 17408
    const int lane = threadIdx.x;
    const int y0 = blockIdx.x * 64;
    const int w1 = pa.w, w2 = pr.w, h = pa.h, wo = w1 + w2;
    const int rows = min(64, h - y0);
    if (rows <= 0) return;
    const int32_t *A = plane_ptr(b, pa, blockIdx.z) + (int64_t)y0 * w1;
    const TR *R = residual_ptr<TR>(b, pr, blockIdx.z) + (int64_t)y0 * w2;
    int32_t *O = plane_ptr(b, po, blockIdx.z) + (int64_t)y0 * wo;
    const bool mine = lane < rows;
    const int32_t *a = A + (int64_t)(mine ? lane : 0) * w1;
    const TR *r = R + (int64_t)(mine ? lane : 0) * w2;
    int32_t *o = O + (int64_t)(mine ? lane : 0) * wo;
    int avg = a[0];
    int left = avg;   // first pair: tendency(avg, avg, next), squeeze.h:89
    int x = 0;
    int32_t *t_res = tile, *t_avg = tile + 64 * HL_IN_PITCH;
    // Software pipeline: the global loads of tile k+1 are issued before tile k is computed and wait in registers (the
    // occupancy is set by the LDS tile, two wavefronts per SIMD; registers are free)
    const int piece8 = lane % HL_IN_LANES, sub8 = lane / HL_IN_LANES;
    Int4U grv[HL_IN_STEPS], gnv[HL_IN_STEPS];
    auto fetch = [&](int xt) {
#pragma unroll
        for (int i = 0; i < HL_IN_STEPS; i++) {
            const int row = min((64 / HL_IN_LANES) * i + sub8, rows - 1);   // rows beyond the plane repeat its last row: no branches around the loads
            grv[i] = load4(R + (int64_t)row * w2 + xt + 4 * piece8);
            gnv[i] = *reinterpret_cast<const Int4U *>(A + (int64_t)row * w1 + xt + 1 + 4 * piece8);
        }
    };
    if (HL_P < w1 && HL_P <= w2) fetch(0);
    for (; x + HL_P < w1 && x + HL_P <= w2; x += HL_P) {   // avg[x+1 .. x+HL_P] all exist
#pragma unroll
        for (int i = 0; i < HL_IN_STEPS; i++) {
            const int row = (64 / HL_IN_LANES) * i + sub8;
            *reinterpret_cast<int4 *>(t_res + row * HL_IN_PITCH + 4 * piece8) = make_int4(grv[i].v[0], grv[i].v[1], grv[i].v[2], grv[i].v[3]);
            *reinterpret_cast<int4 *>(t_avg + row * HL_IN_PITCH + 4 * piece8) = make_int4(gnv[i].v[0], gnv[i].v[1], gnv[i].v[2], gnv[i].v[3]);
        }
        __syncthreads();
        int4 rv[HL_P / 4], nv[HL_P / 4];
#pragma unroll
        for (int q = 0; q < HL_P / 4; q++) {
            rv[q] = *reinterpret_cast<const int4 *>(t_res + lane * HL_IN_PITCH + 4 * q);
            nv[q] = *reinterpret_cast<const int4 *>(t_avg + lane * HL_IN_PITCH + 4 * q);
        }
        __syncthreads();   // every lane has its inputs: the output tile may overwrite them
        if (x + 2 * HL_P < w1 && x + 2 * HL_P <= w2) fetch(x + HL_P);
#pragma unroll
        for (int q = 0; q < HL_P / 4; q++) {
            const int rr[4] = {rv[q].x, rv[q].y, rv[q].z, rv[q].w}, nn[4] = {nv[q].x, nv[q].y, nv[q].z, nv[q].w};
            int ov[8];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int next_avg = nn[k];
                int A2, B2;
                unsqueeze_step(left, avg, next_avg, rr[k], A2, B2);
                left = B2;
                avg = next_avg;
                if (clamp) { A2 = clampi(A2, lo, hi); B2 = clampi(B2, lo, hi); }
                ov[2 * k] = A2; ov[2 * k + 1] = B2;
            }
            *reinterpret_cast<int4 *>(tile + lane * HL_OUT_PITCH + 8 * q) = make_int4(ov[0], ov[1], ov[2], ov[3]);
            *reinterpret_cast<int4 *>(tile + lane * HL_OUT_PITCH + 8 * q + 4) = make_int4(ov[4], ov[5], ov[6], ov[7]);
        }
        __syncthreads();
        {
            const int piece = lane % HL_OUT_LANES, sub = lane / HL_OUT_LANES;
#pragma unroll
            for (int i = 0; i < HL_OUT_STEPS; i++) {
                const int row = (64 / HL_OUT_LANES) * i + sub;
                if (row < rows) {
                    const int4 v = *reinterpret_cast<const int4 *>(tile + row * HL_OUT_PITCH + 4 * piece);
                    Int4U u; u.v[0] = v.x; u.v[1] = v.y; u.v[2] = v.z; u.v[3] = v.w;
                    *reinterpret_cast<Int4U *>(O + (int64_t)row * wo + 2 * x + 4 * piece) = u;
                }
            }
        }
        __syncthreads();   // the next tile's loads overwrite what the stores just read
    }
    if (!mine) return;
    for (; x < w2; x++) {
        const int next_avg = x + 1 < w1 ? a[x + 1] : avg;   // squeeze.h:100
        int A2, B2;
        unsqueeze_step(left, avg, next_avg, r[x], A2, B2);
        o[2 * x] = clamp ? clampi(A2, lo, hi) : A2;
        o[2 * x + 1] = clamp ? clampi(B2, lo, hi) : B2;
        left = B2;
        avg = next_avg;
    }
    if (wo & 1) {  // squeeze.h:129
        const int v = a[w1 - 1];
        o[wo - 1] = clamp ? clampi(v, lo, hi) : v;
    }
}

// OP_HSQ2_YCOCG: the horizontal unsqueeze of Co and of Cg (squeeze.h:81-132) and the inverse YCoCg (ycocg.h:49-61) in one pass.
// Same tiling as k_inv_hsqueeze_tiles with HF_P = 16 pairs per tile row: a lane runs the recurrences of ITS row for both chroma
// planes and leaves the 2 x 32 outputs in LDS; the colour transform then runs in the STORE layout (8 lanes per 128-byte row
// segment), where the Y samples are read straight from global memory and R, G, B are written straight back: the full-size Co
// and Cg planes never exist in memory.
constexpr int HF_P = 16;
constexpr int HF_IN_PITCH = HF_P + 4;
constexpr int HF_OUT_PITCH = 2 * HF_P + 4;
template <typename TR>
__global__ __launch_bounds__(64) void k_inv_hsq2_ycocg(Bases b, PlaneRef pa0, PlaneRef pr0, PlaneRef pa1, PlaneRef pr1, PlaneRef py, PlaneRef pg, PlaneRef pb,
                                                       int maxval) {
    __shared__ __attribute__((aligned(16))) int32_t tile[4 * 64 * HF_IN_PITCH];   // 20480 bytes; the two 64 x 36-word output tiles need 18432
    const int lane = threadIdx.x;
    const int y0 = blockIdx.x * 64;
    const int w1 = pa0.w, w2 = pr0.w, h = pa0.h, wo = w1 + w2;
    const int rows = min(64, h - y0);
    if (rows <= 0) return;
    const int32_t *A[2] = {plane_ptr(b, pa0, blockIdx.z) + (int64_t)y0 * w1, plane_ptr(b, pa1, blockIdx.z) + (int64_t)y0 * w1};
    const TR *R[2] = {residual_ptr<TR>(b, pr0, blockIdx.z) + (int64_t)y0 * w2, residual_ptr<TR>(b, pr1, blockIdx.z) + (int64_t)y0 * w2};
    int32_t *OY = plane_ptr(b, py, blockIdx.z) + (int64_t)y0 * py.w;
    int32_t *OG = plane_ptr(b, pg, blockIdx.z) + (int64_t)y0 * pg.w;
    int32_t *OB = plane_ptr(b, pb, blockIdx.z) + (int64_t)y0 * pb.w;
    const bool mine = lane < rows;
    const int my = mine ? lane : 0;
    int avg[2] = {A[0][(int64_t)my * w1], A[1][(int64_t)my * w1]};
    int left[2] = {avg[0], avg[1]};   // first pair: tendency(avg, avg, next), squeeze.h:89
    auto rgb = [&](int Yv, int Co, int Cg, int &Rr, int &Gg, int &Bb) {   // ycocg.h:49-61
        const int Y = clampi(Yv, 0, maxval);
        Gg = clampi(Y - ((-Cg) >> 1), 0, maxval);
        Bb = clampi(Y + ((1 - Cg) >> 1) - (Co >> 1), 0, maxval);
        Rr = clampi(Co + Bb, 0, maxval);
    };
    int x = 0;
    for (; x + HF_P < w1 && x + HF_P <= w2; x += HF_P) {   // avg[x+1 .. x+HF_P] all exist
        Int4U yv[8];
        {
            // 4 lanes per 64-byte input row segment, 16 rows per instruction; Y: 8 lanes per 128-byte segment, 8 rows per instruction
            const int piece = lane & 3, sub = lane >> 2;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = 16 * i + sub, src = min(row, rows - 1);   // rows beyond the plane repeat its last row: no branches around the loads
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const Int4U rv = load4(R[c] + (int64_t)src * w2 + x + 4 * piece);
                    const Int4U nv = *reinterpret_cast<const Int4U *>(A[c] + (int64_t)src * w1 + x + 1 + 4 * piece);
                    *reinterpret_cast<int4 *>(tile + (2 * c) * 64 * HF_IN_PITCH + row * HF_IN_PITCH + 4 * piece) = make_int4(rv.v[0], rv.v[1], rv.v[2], rv.v[3]);
                    *reinterpret_cast<int4 *>(tile + (2 * c + 1) * 64 * HF_IN_PITCH + row * HF_IN_PITCH + 4 * piece) = make_int4(nv.v[0], nv.v[1], nv.v[2], nv.v[3]);
                }
            }
            const int ypiece = lane & 7, ysub = lane >> 3;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int row = min(8 * i + ysub, rows - 1);
                yv[i] = *reinterpret_cast<const Int4U *>(OY + (int64_t)row * py.w + 2 * x + 4 * ypiece);
            }
        }
        __syncthreads();
        int4 rv[2][HF_P / 4], nv[2][HF_P / 4];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int q = 0; q < HF_P / 4; q++) {
                rv[c][q] = *reinterpret_cast<const int4 *>(tile + (2 * c) * 64 * HF_IN_PITCH + lane * HF_IN_PITCH + 4 * q);
                nv[c][q] = *reinterpret_cast<const int4 *>(tile + (2 * c + 1) * 64 * HF_IN_PITCH + lane * HF_IN_PITCH + 4 * q);
            }
        __syncthreads();   // every lane has its inputs: the output tiles may overwrite them
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int q = 0; q < HF_P / 4; q++) {
                const int rr[4] = {rv[c][q].x, rv[c][q].y, rv[c][q].z, rv[c][q].w}, nn[4] = {nv[c][q].x, nv[c][q].y, nv[c][q].z, nv[c][q].w};
                int ov[8];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int next_avg = nn[k];
                    int A2, B2;
                    unsqueeze_step(left[c], avg[c], next_avg, rr[k], A2, B2);
                    left[c] = B2;
                    avg[c] = next_avg;
                    ov[2 * k] = A2; ov[2 * k + 1] = B2;
                }
                *reinterpret_cast<int4 *>(tile + c * 64 * HF_OUT_PITCH + lane * HF_OUT_PITCH + 8 * q) = make_int4(ov[0], ov[1], ov[2], ov[3]);
                *reinterpret_cast<int4 *>(tile + c * 64 * HF_OUT_PITCH + lane * HF_OUT_PITCH + 8 * q + 4) = make_int4(ov[4], ov[5], ov[6], ov[7]);
            }
        __syncthreads();
        {
            const int piece = lane & 7, sub = lane >> 3;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int row = 8 * i + sub;
                if (row < rows) {
                    const int4 co = *reinterpret_cast<const int4 *>(tile + row * HF_OUT_PITCH + 4 * piece);
                    const int4 cg = *reinterpret_cast<const int4 *>(tile + 64 * HF_OUT_PITCH + row * HF_OUT_PITCH + 4 * piece);
                    const int cov[4] = {co.x, co.y, co.z, co.w}, cgv[4] = {cg.x, cg.y, cg.z, cg.w};
                    Int4U r4, g4, b4;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        int Rr, Gg, Bb;
                        rgb(yv[i].v[k], cov[k], cgv[k], Rr, Gg, Bb);
                        r4.v[k] = Rr; g4.v[k] = Gg; b4.v[k] = Bb;
                    }
                    *reinterpret_cast<Int4U *>(OY + (int64_t)row * py.w + 2 * x + 4 * piece) = r4;
                    *reinterpret_cast<Int4U *>(OG + (int64_t)row * pg.w + 2 * x + 4 * piece) = g4;
                    *reinterpret_cast<Int4U *>(OB + (int64_t)row * pb.w + 2 * x + 4 * piece) = b4;
                }
            }
        }
        __syncthreads();   // the next tile's loads overwrite what the stores just read
    }
    if (!mine) return;
    const int32_t *a0 = A[0] + (int64_t)lane * w1, *a1 = A[1] + (int64_t)lane * w1;
    const TR *r0 = R[0] + (int64_t)lane * w2, *r1 = R[1] + (int64_t)lane * w2;
    int32_t *oy = OY + (int64_t)lane * py.w, *og = OG + (int64_t)lane * pg.w, *ob = OB + (int64_t)lane * pb.w;
    for (; x < w2; x++) {
        int P[2][2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int32_t *a = c ? a1 : a0;
            const TR *r = c ? r1 : r0;
            const int next_avg = x + 1 < w1 ? a[x + 1] : avg[c];   // squeeze.h:100
            unsqueeze_step(left[c], avg[c], next_avg, r[x], P[c][0], P[c][1]);
            left[c] = P[c][1];
            avg[c] = next_avg;
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            int Rr, Gg, Bb;
            rgb(oy[2 * x + k], P[0][k], P[1][k], Rr, Gg, Bb);
            oy[2 * x + k] = Rr; og[2 * x + k] = Gg; ob[2 * x + k] = Bb;
        }
    }
    if (wo & 1) {  // squeeze.h:129
        int Rr, Gg, Bb;
        rgb(oy[wo - 1], a0[w1 - 1], a1[w1 - 1], Rr, Gg, Bb);
        oy[wo - 1] = Rr; og[wo - 1] = Gg; ob[wo - 1] = Bb;
    }
}

// ---------------------------------------------------------------------------------------------
// transform/ycocg.h:49-61, in place on three planes (own row pitches), region w x h
__global__ __launch_bounds__(256) void k_inv_ycocg(Bases b, PlaneRef p0, PlaneRef p1, PlaneRef p2, int w, int h, int maxval) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= w || y >= h) return;
    int32_t *c0 = plane_ptr(b, p0, blockIdx.z) + (int64_t)y * p0.w + x;
    int32_t *c1 = plane_ptr(b, p1, blockIdx.z) + (int64_t)y * p1.w + x;
    int32_t *c2 = plane_ptr(b, p2, blockIdx.z) + (int64_t)y * p2.w + x;
    const int Y = clampi(*c0, 0, maxval);
    const int Co = *c1, Cg = *c2;
    const int G = clampi(Y - ((-Cg) >> 1), 0, maxval);
    const int B = clampi(Y + ((1 - Cg) >> 1) - (Co >> 1), 0, maxval);
    const int R = clampi(Co + B, 0, maxval);
    *c0 = R; *c1 = G; *c2 = B;
}

// transform/ycbcr.h:49-60: `float` operands, double arithmetic left to right, no contraction,
// CLAMP in double, truncating conversion to the integer sample.
__global__ __launch_bounds__(256) void k_inv_ycbcr(Bases b, PlaneRef p0, PlaneRef p1, PlaneRef p2, int w, int h, int minval, int maxval) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= w || y >= h) return;
    int32_t *c0 = plane_ptr(b, p0, blockIdx.z) + (int64_t)y * p0.w + x;
    int32_t *c1 = plane_ptr(b, p1, blockIdx.z) + (int64_t)y * p1.w + x;
    int32_t *c2 = plane_ptr(b, p2, blockIdx.z) + (int64_t)y * p2.w + x;
    const float half = (float)((maxval + 1) / 2);
    const float yy = (float)*c0;
    const float cb = __fsub_rn((float)*c1, half);
    const float cr = __fsub_rn((float)*c2, half);
    const double dy = (double)yy, dcb = (double)cb, dcr = (double)cr;
    double r = __dadd_rn(__dadd_rn(dy, __dmul_rn(1.402, dcr)), 0.5);
    double g = __dadd_rn(__dsub_rn(__dsub_rn(dy, __dmul_rn(0.344136, dcb)), __dmul_rn(0.714136, dcr)), 0.5);
    double bl = __dadd_rn(__dadd_rn(dy, __dmul_rn(1.772, dcb)), 0.5);
    const double mn = (double)minval, mx = (double)maxval;
    r = r < mn ? mn : (r > mx ? mx : r);
    g = g < mn ? mn : (g > mx ? mx : g);
    bl = bl < mn ? mn : (bl > mx ? mx : bl);
    *c0 = (int)r; *c1 = (int)g; *c2 = (int)bl;
}

// ---------------------------------------------------------------------------------------------
// transform/quantize.h:32-49: plane *= q, q = ChannelMeta::q of the plane's source channel.
// grid.y walks the op's plane list.
// TR = coef_t (Op::r16): the planes are coded planes nobody has touched -- read the int16 samples from the coefficient slab and write
// sample * q into the int32 copy (widening and scaling in one pass, also when q == 1); TR = int32_t: in place on the int32 copy.
// quantize.h:41 is `ch.value(y,x) *= q` on a pixel_type &: the product is computed in int and stored as int16 (narrow16), in both forms.
template <typename TR>
__global__ __launch_bounds__(256) void k_dequant(Bases b, const PlaneRef *list, const ChannelMeta *meta, int n_channels, int img_first) {
    const PlaneRef p = list[blockIdx.y];
    const int q = meta[(int64_t)(img_first + blockIdx.z) * n_channels + p.qsrc].q;
    constexpr bool kFrom16 = !std::is_same<TR, int32_t>::value;
    if (q == 1 && !kFrom16) return;
    const int64_t n = (int64_t)p.w * p.h;
    int32_t *d = plane_ptr(b, p, blockIdx.z);
    const TR *s = residual_ptr<TR>(b, p, blockIdx.z);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = narrow16((int)s[i] * q);
}

__global__ __launch_bounds__(256) void k_clamp(Bases b, PlaneRef src, PlaneRef dst, int lo, int hi) {
    const int64_t n = (int64_t)dst.w * dst.h;
    const int32_t *s = plane_ptr(b, src, blockIdx.z);
    int32_t *d = plane_ptr(b, dst, blockIdx.z);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = clampi(s[i], lo, hi);
}

// transform/palette.h:57-64: out(y,x) = palette(component, CLAMP(index(y,x), 0, colours-1)).  The palette is a
// decoded meta-channel (colours x components samples); rows of it stay in L1/L2.
__global__ __launch_bounds__(256) void k_inv_palette(Bases b, PlaneRef pidx, PlaneRef ppal, PlaneRef po, int component, int colours,
                                                     int clamp, int lo, int hi) {
    const int64_t n = (int64_t)po.w * po.h;
    const int32_t *idx = plane_ptr(b, pidx, blockIdx.z);
    const int32_t *pal = plane_ptr(b, ppal, blockIdx.z) + (int64_t)component * ppal.w;
    int32_t *d = plane_ptr(b, po, blockIdx.z);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int v = colours > 0 ? pal[clampi(idx[i], 0, colours - 1)] : 0;   // an empty palette reads Channel::zero (image.h:82)
        d[i] = clamp ? clampi(v, lo, hi) : v;
    }
}

// transform/permute.h:31-54 with the permutation in a meta-channel: output plane i is a copy of candidate plane perm[i],
// perm = the decoded samples of the 1-row meta plane -- per image.  A value that is no channel number (the reference would
// index outside its channel vector) flags the image corrupt and ZERO-FILLS the output plane, so that a flagged image is
// deterministic and shows nothing of an earlier batch's slab.  A value that repeats an earlier one is refused as well:
// stricter than inv_permute (:39-46 copies blindly, twice) but the same verdict as the decode-time metadata permutation
// of encoding.cpp:576-596 / meta_permute (:68-73) and as oracle/fuif_oracle.c gives.
__global__ __launch_bounds__(256) void k_permute_plane(Bases b, PlaneRef pperm, const PlaneRef *cand, int nb, int which, PlaneRef po, int clamp, int lo,
                                                       int hi, int32_t *status, int img_first) {
    const int c = plane_ptr(b, pperm, blockIdx.z)[which];
    bool bad = c < 0 || c >= nb;
    for (int j = 0; j < which && !bad; j++) bad = plane_ptr(b, pperm, blockIdx.z)[j] == c;
    int32_t *d = plane_ptr(b, po, blockIdx.z);
    const int64_t n = (int64_t)po.w * po.h;
    if (bad) {
        if (status && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&status[img_first + blockIdx.z], (int32_t)ST_CORRUPT);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = 0;
        return;
    }
    const int32_t *s = plane_ptr(b, cand[c], blockIdx.z);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = clamp ? clampi(s[i], lo, hi) : s[i];
}

// transform/approximate.h:44-57: ch = ch*q + remainder.  A remainder channel the stream never reached has no
// samples in the reference (`chr.data.size() == 0`, :49,54): then nothing is added and Channel::q keeps its
// value; otherwise Channel::q is taken from the remainder (:50).  `decoded` is per image, so the q hand-over is
// done here on the ChannelMeta the later k_dequant reads.
__global__ __launch_bounds__(256) void k_inv_approx(Bases b, PlaneRef pc, PlaneRef pr, int q, int ctor_data, ChannelMeta *meta, int n_channels,
                                                    int img_first) {
    ChannelMeta *m = meta ? meta + (int64_t)(img_first + blockIdx.z) * n_channels : nullptr;
    const bool reached = m && pr.qsrc >= 0 && m[pr.qsrc].decoded != 0;
    const bool have = reached || ctor_data;
    const int64_t n = (int64_t)pc.w * pc.h;
    int32_t *d = plane_ptr(b, pc, blockIdx.z);
    const int32_t *r = plane_ptr(b, pr, blockIdx.z);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = narrow16(narrow16(d[i] * q) + (have ? r[i] : 0));   // approximate.h:53,55: `*= q`, then `+=`, each on a pixel_type &
    if (have && m && blockIdx.x == 0 && threadIdx.x == 0 && pc.qsrc >= 0 && pr.qsrc >= 0) m[pc.qsrc].q = reached ? m[pr.qsrc].q : 1;
}

// transform/2dmatch.h:147-171, the previous-frame mode (match channel q == 2*fh*fh + (fh&1), :147-149): frames are
// stacked vertically, z = m(y,x) != 0 means "equal to (soft: add) the sample z frames up".  One lane per column,
// serial down the rows (a source may itself be a matched sample of an earlier frame).  Channel::value() only
// checks the linear index (image.h:82-85): a source before the first sample reads Channel::zero.
// The free-offset mode (q == 1) is handled by k_match_init / k_match_jump / k_match_apply below.
__global__ __launch_bounds__(256) void k_inv_match_frames(Bases b, PlaneRef pm, const PlaneRef *list, int n_list, int softmatch, int fh,
                                                          const ChannelMeta *meta, int n_channels, int img_first, int32_t *status) {
    const int z_img = blockIdx.z;
    const int q = (meta && pm.qsrc >= 0) ? meta[(int64_t)(img_first + z_img) * n_channels + pm.qsrc].q : 0;
    if (q != 2 * fh * fh + (fh & 1)) {
        // q == 1 is the free-offset mode (next kernels); anything else the reference refuses (2dmatch.h:172-175)
        if (q != 1 && status && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&status[img_first + z_img], ST_UNSUPPORTED | ST_CORRUPT);
        return;
    }
    const int w = pm.w, h = pm.h;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= w) return;
    const int32_t *m = plane_ptr(b, pm, z_img);
    for (int y = 0; y < h; y++) {
        const int zv = m[(int64_t)y * w + x];
        if (!zv) continue;
        const int64_t src = ((int64_t)y - (int64_t)zv * fh) * w + x;
        const bool inside = src >= 0 && src < (int64_t)w * h;
        for (int k = 0; k < n_list; k++) {
            int32_t *p = plane_ptr(b, list[k], z_img);
            const int sv = inside ? p[src] : 0;
            p[(int64_t)y * w + x] = softmatch ? narrow16(p[(int64_t)y * w + x] + sv) : sv;   // 2dmatch.h:155: `+=` on a pixel_type &
        }
    }
}

// ---- 2D match with free offsets (transform/2dmatch.h:136-146, match channel q == 1) --------------------------
// Reference semantics: in scan order, z = m(y,x) != 0 means value(y,x) = value(y+oy, x+ox) with (ox,oy) = the z-th
// position of a spiral through the already decoded neighbourhood (:33-78) -- the source may itself be a copy.
// Channel::value() only checks the LINEAR index (image.h:82-85), so the source is sample p + oy*w + ox, and a
// source before the first sample reads Channel::zero.  Parallel form: S[p] = p for unmatched samples, else the
// source index; ceil(log2(n)) rounds of S[p] = S[S[p]] make every S[p] a root; one gather finishes the job.
// Soft matches (value += source, :136-140; the CLI never writes them, fuif.cpp:445) take the same route with one accumulator
// per listed plane: value(p) = residual(p) + value(source(p)), so A[p] = residual(p) for a matched sample and 0 for a root,
// every doubling step adds A[S[p]] to A[p] (two copies of the accumulators, read one / write the other), and the gather adds
// the root's sample and keeps the low 16 bits, sign-extended: the reference's `+=` stores a pixel_type at every link.  Forward references (only possible in images narrower than the spiral) are flagged
// FUIFGPU_ST_UNSUPPORTED and the image is left unmatched.
// The list of a soft match is [planes (n), accumulators (n), accumulators (n)]; Op::p1 of a jump / apply op = which copy it reads.
DEV void match_offset(int code, int &xo, int &yo) {   // 2dmatch.h:50-78
    int layer = 0, size = 4;
    while (code > size) { code -= size; layer++; size += 4; }
    if (layer & 1) {
        if (code <= layer) { xo = 1 + layer; yo = -code; }
        else if (code <= 3 + 3 * layer) { xo = 2 + 2 * layer - code; yo = -1 - layer; }
        else { xo = -1 - layer; yo = -4 - 4 * layer + code; }
    } else {
        if (code <= 1 + layer) { xo = -1 - layer; yo = 1 - code; }
        else if (code <= 4 + 3 * layer) { xo = -3 - 2 * layer + code; yo = -1 - layer; }
        else { xo = 1 + layer; yo = -5 - 4 * layer + code; }
    }
}
DEV bool match_free_mode(const PlaneRef &pm, const ChannelMeta *meta, int n_channels, int img) {
    return meta && pm.qsrc >= 0 && meta[(int64_t)img * n_channels + pm.qsrc].q == 1;
}
__global__ __launch_bounds__(256) void k_match_init(Bases b, PlaneRef pm, PlaneRef ps, int softmatch, const PlaneRef *list, int n_list,
                                                    const ChannelMeta *meta, int n_channels, int img_first, int32_t *status) {
    const int img = img_first + blockIdx.z;
    if (!match_free_mode(pm, meta, n_channels, img)) return;
    const int maxz = meta[(int64_t)img * n_channels + pm.qsrc].maxval;
    const int w = pm.w;
    const int64_t n = (int64_t)pm.w * pm.h;
    const int32_t *m = plane_ptr(b, pm, blockIdx.z);
    int32_t *S = plane_ptr(b, ps, blockIdx.z);
    int flag = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int z = m[p];
        int64_t s = p;
        if (z) {
            if (z < 0 || z > maxz) flag |= ST_UNSUPPORTED | ST_CORRUPT;   // offsets_table[z] out of range in the reference
            else {
                int xo, yo;
                match_offset(z, xo, yo);
                const int64_t src = p + (int64_t)yo * w + xo;
                if (src < 0 || src >= n) s = -1;
                else if (src > p) flag |= ST_UNSUPPORTED;                        // would read a sample that is rewritten later
                else s = src;
            }
        }
        S[p] = (int32_t)s;
        if (softmatch)
            for (int k = 0; k < n_list; k++) plane_ptr(b, list[n_list + k], blockIdx.z)[p] = s != p ? plane_ptr(b, list[k], blockIdx.z)[p] : 0;
    }
    if (flag && status) atomicOr(&status[img], flag);
}
__global__ __launch_bounds__(256) void k_match_jump(Bases b, PlaneRef pm, PlaneRef pin, PlaneRef pout, int softmatch, const PlaneRef *list, int n_list,
                                                    int from, const ChannelMeta *meta, int n_channels, int img_first) {
    if (!match_free_mode(pm, meta, n_channels, img_first + blockIdx.z)) return;
    const int64_t n = (int64_t)pin.w * pin.h;
    const int32_t *S = plane_ptr(b, pin, blockIdx.z);
    int32_t *T = plane_ptr(b, pout, blockIdx.z);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int s = S[p];
        T[p] = s >= 0 ? S[s] : s;
        if (softmatch)
            for (int k = 0; k < n_list; k++) {
                const int32_t *a = plane_ptr(b, list[n_list * (1 + from) + k], blockIdx.z);
                // (unsigned: a long chain's sum may pass 2^31; only its low 16 bits are kept in the end)
                plane_ptr(b, list[n_list * (2 - from) + k], blockIdx.z)[p] = (int32_t)((uint32_t)a[p] + (uint32_t)(s >= 0 ? a[s] : 0));
            }
    }
}
__global__ __launch_bounds__(256) void k_match_apply(Bases b, PlaneRef pm, PlaneRef ps, int softmatch, const PlaneRef *list, int n_list, int from,
                                                     const ChannelMeta *meta, int n_channels, int img_first, const int32_t *status) {
    const int img = img_first + blockIdx.z;
    if (!match_free_mode(pm, meta, n_channels, img)) return;
    if (status && (status[img] & ST_UNSUPPORTED)) return;   // flagged by k_match_init: leave the planes alone
    const int64_t n = (int64_t)ps.w * ps.h;
    const int32_t *S = plane_ptr(b, ps, blockIdx.z);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int s = S[p];
        if (s == p) continue;                                // roots are never written: the gather below only reads roots
        for (int k = 0; k < n_list; k++) {
            int32_t *pl = plane_ptr(b, list[k], blockIdx.z);
            const int root = s < 0 ? 0 : pl[s];
            // 2dmatch.h:129: `+=` on a pixel_type & at every link of the chain; narrowing is a ring homomorphism, so narrowing the whole sum once gives the same value
            pl[p] = softmatch ? narrow16((int)((uint32_t)plane_ptr(b, list[n_list * (1 + from) + k], blockIdx.z)[p] + (uint32_t)root)) : root;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// transform/dct.h:60-77 -- the constants exactly as the reference prints them
constexpr double kDCT[64] = {
    0.3535533906, 0.3535533906, 0.3535533906, 0.3535533906, 0.3535533906, 0.3535533906, 0.3535533906, 0.3535533906,
    0.4903926402, 0.4157348062, 0.2777851165, 0.0975451610, -0.0975451610, -0.2777851165, -0.4157348062, -0.4903926402,
    0.4619397663, 0.1913417162, -0.1913417162, -0.4619397663, -0.4619397663, -0.1913417162, 0.1913417162, 0.4619397663,
    0.4157348062, -0.0975451610, -0.4903926402, -0.2777851165, 0.2777851165, 0.4903926402, 0.0975451610, -0.4157348062,
    0.3535533906, -0.3535533906, -0.3535533906, 0.3535533906, 0.3535533906, -0.3535533906, -0.3535533906, 0.3535533906,
    0.2777851165, -0.4903926402, 0.0975451610, 0.4157348062, -0.4157348062, -0.0975451610, 0.4903926402, -0.2777851165,
    0.1913417162, -0.4619397663, 0.4619397663, -0.1913417162, -0.1913417162, 0.4619397663, -0.4619397663, 0.1913417162,
    0.0975451610, -0.2777851165, 0.4157348062, -0.4903926402, 0.4903926402, -0.4157348062, 0.2777851165, -0.0975451610,
};

// One lane per 8x8 block.  Column pass then row pass (dct.h:101-106); every output is
// 0.0 + sum_{u=0..7} k[8u+o]*in[u] accumulated left to right in double with separate mul and add
// (the x86-64 reference build has no FMA), DC gets the float DC offset in float arithmetic
// (dct.h:281,285), result rounded half away from zero (dct.h:289).
//
// The 64 constants are 7 magnitudes with signs, and k*x and (-k)*x are the same product with the other sign, exactly.  So one
// 8-point pass needs 22 multiplications, not 64 (row u of the matrix holds 1, 4, 2, 4, 1, 4, 2, 4 different magnitudes), and
// 56 additions / subtractions in the reference's order: the leading `0.0 +` is dropped -- it only matters for a first product
// of -0.0, which cannot occur (row 0 of the matrix is positive and no input is -0.0: the coefficients are integers and a sum
// that starts from +0.0 never yields -0.0).  Seven constants live in 14 SGPRs (round 2 kept all 64 in SGPRs: 252 spilled
// lanes, two v_readlane per multiplication).
constexpr double kDctMag[7] = {0.3535533906, 0.4903926402, 0.4157348062, 0.2777851165, 0.0975451610, 0.4619397663, 0.1913417162};
// sign * (magnitude index + 1) of kDCT[8u + o]
constexpr signed char kDctCode[64] = {
    1, 1, 1, 1, 1, 1, 1, 1,
    2, 3, 4, 5, -5, -4, -3, -2,
    6, 7, -7, -6, -6, -7, 7, 6,
    3, -5, -2, -4, 4, 2, 5, -3,
    1, -1, -1, 1, 1, -1, -1, 1,
    4, -2, 5, 3, -3, -5, 2, -4,
    7, -6, 6, -7, -7, 6, -6, 7,
    5, -4, 3, -2, 2, -3, 4, -5,
};
constexpr bool dct_code_matches_matrix() {
    for (int i = 0; i < 64; i++) {
        const int c = kDctCode[i];
        const double v = c > 0 ? kDctMag[c - 1] : -kDctMag[-c - 1];
        if (v != kDCT[i]) return false;
    }
    return true;
}
static_assert(dct_code_matches_matrix(), "kDctCode / kDctMag must spell out transform/dct.h:60-77");
DEV void idct_1d(const double (&in)[8], double (&out)[8]) {
    double pr[8][7];
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
        for (int m = 0; m < 7; m++) pr[u][m] = __dmul_rn(kDctMag[m], in[u]);   // the products no output uses are dead code
#pragma unroll
    for (int o = 0; o < 8; o++) {
        double acc = pr[0][0];
#pragma unroll
        for (int u = 1; u < 8; u++) {
            const int c = kDctCode[8 * u + o];
            acc = c > 0 ? __dadd_rn(acc, pr[u][c - 1]) : __dadd_rn(acc, -pr[u][-c - 1]);
        }
        out[o] = acc;
    }
}
// A source plane of kind BUF_COEF16Q (planner peephole fuse_dequant_into_idct) is a coded plane as the entropy kernel stored it: the int16 sample is
// read from the coefficient slab and multiplied by the channel's quantisation constant on the way in (quantize.h:32-49 folded into the load;
// the product narrowed to int16 like the store of quantize.h:41 that it replaces).
// kAc16 (Op::pad2): ALL 63 AC planes are of that kind -- known at compile time, so the 8 loads of a column are issued together as before; only the DC plane
// (entry 0: a product of the unsqueeze chain in a default stream) is tested at run time.  With a per-plane test inside the loop every load waited for
// its own round trip and the kernel's time doubled (23 -> 45 ms per C3 step, profiles/r5_c3_kernel_stats_scalar_q_loads.csv).
template <bool kAc16>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_idct8x8(Bases b, const PlaneRef *list, PlaneRef po, int bw, int bh, int maxval, int clamp, int lo, int hi,
                                                const ChannelMeta *meta, int n_channels, int img_first) {
    const int bx = blockIdx.x * blockDim.x + threadIdx.x;
    const int by = blockIdx.y;
    // The quantisation constants of the 64 source planes, one per lane, parked in LDS: the column loop below reads them with constant offsets
    // (no dependent scalar loads -- plane descriptor, then q -- inside the loop).
    __shared__ int qs[64];
    {
        const PlaneRef pl = list[threadIdx.x];
        qs[threadIdx.x] = (pl.buf == BUF_COEF16Q && meta) ? meta[(int64_t)(img_first + blockIdx.z) * n_channels + pl.qsrc].q : 1;
    }
    __syncthreads();
    if (bx >= bw || by >= bh) return;
    const float dcoff = (float)(((double)maxval + 1.0) * 4.0);
    double tmp[64];   // [output row o][column x] after the column pass
#pragma unroll
    for (int x = 0; x < 8; x++) {
        double col[8], res[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const PlaneRef p = list[u * 8 + x];
            int v;
            if ((u != 0 || x != 0) ? kAc16 : p.buf == BUF_COEF16Q)
                v = narrow16((int)(b.c16 + (int64_t)blockIdx.z * b.stride[BUF_COEF] + p.off)[(int64_t)by * p.w + bx] * qs[u * 8 + x]);
            else
                v = plane_ptr(b, p, blockIdx.z)[(int64_t)by * p.w + bx];
            col[u] = (u == 0 && x == 0) ? (double)__fadd_rn((float)v, dcoff) : (double)v;
        }
        idct_1d(col, res);
#pragma unroll
        for (int o = 0; o < 8; o++) tmp[o * 8 + x] = res[o];
#ifndef FUIF_EMU
        // one column's plane descriptors at a time: with all 64 scalar descriptor loads hoisted to the top the kernel spilled 88 SGPRs; the
        // barrier costs nothing (profiles/r4_idct_variants.txt: 0.554 ms with and without on a 1920 x 2160-block component)
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
    int32_t *o = plane_ptr(b, po, blockIdx.z) + (int64_t)(by * 8) * po.w + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
        double row[8], res[8];
#pragma unroll
        for (int u = 0; u < 8; u++) row[u] = tmp[8 * y + u];
        idct_1d(row, res);
        int outv[8];
#pragma unroll
        for (int oo = 0; oo < 8; oo++) {
            int v = (int)round(res[oo]);
            outv[oo] = clamp ? clampi(v, lo, hi) : v;
        }
        int4 *dst = reinterpret_cast<int4 *>(o + (int64_t)y * po.w);
        dst[0] = make_int4(outv[0], outv[1], outv[2], outv[3]);
        dst[1] = make_int4(outv[4], outv[5], outv[6], outv[7]);
    }
}

// ---------------------------------------------------------------------------------------------
// transform/subsample.h:90-115: horizontal pass (3a+b+1)>>2 / (3a+c+2)>>2 with edge replication,
// then the same vertically on the horizontally upsampled rows.  One lane per output sample.
__global__ __launch_bounds__(256) void k_upsample(Bases b, PlaneRef pi, PlaneRef po, int srh, int srv, int clamp, int lo, int hi) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    const int Y = blockIdx.y;
    const int ow = pi.w, oh = pi.h;
    if (X >= po.w || Y >= po.h) return;
    const int32_t *in = plane_ptr(b, pi, blockIdx.z);
    auto hval = [&](int y, int Xo) -> int {  // value of the horizontally upsampled row y at column Xo
        if (srh == 2) {
            const int x = Xo >> 1;
            const int c = in[(int64_t)y * ow + x];
            if (Xo & 1) return (3 * c + in[(int64_t)y * ow + (x + 1 < ow ? x + 1 : x)] + 2) >> 2;
            return (3 * c + in[(int64_t)y * ow + (x ? x - 1 : 0)] + 1) >> 2;
        }
        return in[(int64_t)y * ow + Xo];
    };
    int v;
    if (srh > 2 || srv > 2) {
        v = in[(int64_t)(Y / srv) * ow + X / srh];   // subsample.h:116-126: plain replication for ratios above 2 (4:1:1)
    } else if (srv == 2) {
        const int y = Y >> 1;
        const int c = hval(y, X);
        if (Y & 1) v = (3 * c + hval(y + 1 < oh ? y + 1 : y, X) + 2) >> 2;
        else v = (3 * c + hval(y ? y - 1 : 0, X) + 1) >> 2;
    } else {
        v = hval(Y, X);
    }
    plane_ptr(b, po, blockIdx.z)[(int64_t)Y * po.w + X] = clamp ? clampi(v, lo, hi) : v;
}

// The 4:2:0 case (both factors 2) with one lane per INPUT sample, which owns the 2x2 outputs above it: 9 loads (its 3x3
// neighbourhood, shared with the neighbouring lanes through L1) for 4 samples instead of 4 loads for 1, a quarter of the
// lanes and blocks, 8-byte stores.  Same arithmetic as k_upsample (subsample.h:90-115).  C3, 1024 x 4K: k_upsample was the
// slowest inverse transform of the JPEG-transcode schedule (61.8 ms per step, 1.4 TB/s; profiles/r2_c3_kernel_stats.csv).
struct __attribute__((packed, aligned(4))) Int2U { int32_t v[2]; };
__global__ __launch_bounds__(256) void k_upsample_2x2(Bases b, PlaneRef pi, PlaneRef po, int clamp, int lo, int hi) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int ow = pi.w, oh = pi.h;
    if (x >= ow || 2 * x >= po.w || 2 * y >= po.h) return;
    const int32_t *in = plane_ptr(b, pi, blockIdx.z);
    const int xm = x ? x - 1 : 0, xp = x + 1 < ow ? x + 1 : x;
    const int ym = y ? y - 1 : 0, yp = y + 1 < oh ? y + 1 : y;
    // the horizontally upsampled row yy at columns 2x (even) and 2x + 1 (odd)
    auto hrow = [&](int yy, int &he, int &ho) {
        const int32_t *r = in + (int64_t)yy * ow;
        const int c = r[x];
        he = (3 * c + r[xm] + 1) >> 2;
        ho = (3 * c + r[xp] + 2) >> 2;
    };
    int me, mo, ce, co, pe, po2;
    hrow(ym, me, mo); hrow(y, ce, co); hrow(yp, pe, po2);
    int v00 = (3 * ce + me + 1) >> 2, v01 = (3 * co + mo + 1) >> 2;     // row 2y: with the row above
    int v10 = (3 * ce + pe + 2) >> 2, v11 = (3 * co + po2 + 2) >> 2;    // row 2y + 1: with the row below
    if (clamp) { v00 = clampi(v00, lo, hi); v01 = clampi(v01, lo, hi); v10 = clampi(v10, lo, hi); v11 = clampi(v11, lo, hi); }
    int32_t *o = plane_ptr(b, po, blockIdx.z) + (int64_t)(2 * y) * po.w + 2 * x;
    const bool two_cols = 2 * x + 1 < po.w, two_rows = 2 * y + 1 < po.h;
    if (two_cols) {
        Int2U a; a.v[0] = v00; a.v[1] = v01;
        *reinterpret_cast<Int2U *>(o) = a;
        if (two_rows) { Int2U c2; c2.v[0] = v10; c2.v[1] = v11; *reinterpret_cast<Int2U *>(o + po.w) = c2; }
    } else {
        o[0] = v00;
        if (two_rows) o[po.w] = v10;
    }
}

// ---------------------------------------------------------------------------------------------
// OP_UPS2_YCBCR: 4:2:0 chroma upsampling (k_upsample_2x2's arithmetic, subsample.h:90-115) + inverse YCbCr (k_inv_ycbcr's arithmetic, ycbcr.h:49-60) in
// one pass.  One lane per chroma INPUT sample owning its 2x2 outputs: 9 + 9 L1-shared chroma loads and two 8-byte loads of Y for 4 pixels, six 8-byte
// stores; the full-size Cb / Cr planes are never written and read back.  Output samples of the chroma planes outside the colour transform's w x h
// region (block padding) get the upsampled value, clamped to [lo, hi] like the final clamp of image.cpp:107-113 leaves them.
__global__ __launch_bounds__(256) void k_ups2_ycbcr(Bases b, PlaneRef py, PlaneRef pcb, PlaneRef pcr, PlaneRef o0, PlaneRef o1, PlaneRef o2, int w, int h, int lo, int hi) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int cw = pcb.w, ch = pcb.h;
    if (x >= cw) return;
    const int32_t *cb_in = plane_ptr(b, pcb, blockIdx.z), *cr_in = plane_ptr(b, pcr, blockIdx.z);
    const int xm = x ? x - 1 : 0, xp = x + 1 < cw ? x + 1 : x;
    const int ym = y ? y - 1 : 0, yp = y + 1 < ch ? y + 1 : y;
    int cbv[4], crv[4];     // [row][column] of the 2x2 outputs
    auto up = [&](const int32_t *in, int (&v)[4]) {
        auto hrow = [&](int yy, int &he, int &ho) {
            const int32_t *r = in + (int64_t)yy * cw;
            const int c = r[x];
            he = (3 * c + r[xm] + 1) >> 2;
            ho = (3 * c + r[xp] + 2) >> 2;
        };
        int me, mo, ce, co, pe, po2;
        hrow(ym, me, mo); hrow(y, ce, co); hrow(yp, pe, po2);
        v[0] = (3 * ce + me + 1) >> 2; v[1] = (3 * co + mo + 1) >> 2;      // row 2y: with the row above
        v[2] = (3 * ce + pe + 2) >> 2; v[3] = (3 * co + po2 + 2) >> 2;     // row 2y + 1: with the row below
    };
    up(cb_in, cbv); up(cr_in, crv);
    const float half = (float)((hi + 1) / 2);
    const double mn = (double)lo, mx = (double)hi;
    int32_t *Yp = plane_ptr(b, py, blockIdx.z), *O0 = plane_ptr(b, o0, blockIdx.z), *O1 = plane_ptr(b, o1, blockIdx.z), *O2 = plane_ptr(b, o2, blockIdx.z);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int Y = 2 * y + r;
        int out0[2], out1[2], out2[2];
        bool in_region[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int X = 2 * x + c;
            in_region[c] = X < w && Y < h;
            const int cb_i = cbv[2 * r + c], cr_i = crv[2 * r + c];
            if (in_region[c]) {
                const float yy = (float)Yp[(int64_t)Y * py.w + X];
                const float cb = __fsub_rn((float)cb_i, half);
                const float cr = __fsub_rn((float)cr_i, half);
                const double dy = (double)yy, dcb = (double)cb, dcr = (double)cr;
                double rr = __dadd_rn(__dadd_rn(dy, __dmul_rn(1.402, dcr)), 0.5);
                double g = __dadd_rn(__dsub_rn(__dsub_rn(dy, __dmul_rn(0.344136, dcb)), __dmul_rn(0.714136, dcr)), 0.5);
                double bl = __dadd_rn(__dadd_rn(dy, __dmul_rn(1.772, dcb)), 0.5);
                rr = rr < mn ? mn : (rr > mx ? mx : rr);
                g = g < mn ? mn : (g > mx ? mx : g);
                bl = bl < mn ? mn : (bl > mx ? mx : bl);
                out0[c] = (int)rr; out1[c] = (int)g; out2[c] = (int)bl;
            } else {
                out0[c] = 0; out1[c] = clampi(cb_i, lo, hi); out2[c] = clampi(cr_i, lo, hi);
            }
        }
        // (the chroma planes are 2cw x 2ch, so both columns and both rows exist there; the Y plane only has the region)
        int32_t *d1 = O1 + (int64_t)Y * o1.w + 2 * x, *d2 = O2 + (int64_t)Y * o2.w + 2 * x;
        Int2U a1; a1.v[0] = out1[0]; a1.v[1] = out1[1];
        Int2U a2; a2.v[0] = out2[0]; a2.v[1] = out2[1];
        *reinterpret_cast<Int2U *>(d1) = a1;
        *reinterpret_cast<Int2U *>(d2) = a2;
        int32_t *d0 = O0 + (int64_t)Y * o0.w + 2 * x;
        if (in_region[0] && in_region[1]) { Int2U a0; a0.v[0] = out0[0]; a0.v[1] = out0[1]; *reinterpret_cast<Int2U *>(d0) = a0; }
        else if (in_region[0]) d0[0] = out0[0];
    }
}

// ---------------------------------------------------------------------------------------------
// Forward YCoCg and Squeeze (the encoder-side subset that is data parallel).  Unlike their inverses
// they have no recurrence -- the residual of a pair reads ORIGINAL neighbours -- so it is one lane per pair.
// transform/ycocg.h:65-95, in place on three contiguous planes of n samples
__global__ __launch_bounds__(256) void k_fwd_ycocg(int32_t *c0, int32_t *c1, int32_t *c2, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int R = c0[i], G = c1[i], B = c2[i];
    c0[i] = (((R + B) >> 1) + G) >> 1;
    c1[i] = R - B;
    c2[i] = G - ((R + B) >> 1);
}
// transform/squeeze.h:135-170: in (w x h) -> avg ((w+1)/2 x h) + residual (w/2 x h)
__global__ __launch_bounds__(256) void k_fwd_hsqueeze(const int32_t *in, int w, int h, int32_t *avg, int32_t *res) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    const int w1 = (w + 1) / 2, w2 = w - w1;
    if (x >= w1 || y >= h) return;
    const int32_t *row = in + (int64_t)y * w;
    if (x >= w2) { avg[(int64_t)y * w1 + x] = row[2 * x]; return; }   // the odd last column is its own average
    const int A = row[2 * x], B = row[2 * x + 1];
    const int a = (A + B + (A > B)) >> 1;
    avg[(int64_t)y * w1 + x] = a;
    int next = a;
    if (x + 1 < w2) { const int C = row[2 * x + 2], D = row[2 * x + 3]; next = (C + D + (C > D)) >> 1; }
    else if (w & 1) next = row[2 * x + 2];
    const int left = x > 0 ? row[2 * x - 1] : a;
    res[(int64_t)y * w2 + x] = (A - B) - smooth_tendency(left, a, next);
}
// transform/squeeze.h:227-263: in (w x h) -> avg (w x (h+1)/2) + residual (w x h/2)
__global__ __launch_bounds__(256) void k_fwd_vsqueeze(const int32_t *in, int w, int h, int32_t *avg, int32_t *res) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    const int h1 = (h + 1) / 2, h2 = h - h1;
    if (x >= w || y >= h1) return;
    if (y >= h2) { avg[(int64_t)y * w + x] = in[(int64_t)(2 * y) * w + x]; return; }   // the odd last row
    const int A = in[(int64_t)(2 * y) * w + x], B = in[(int64_t)(2 * y + 1) * w + x];
    const int a = (A + B + (A > B)) >> 1;
    avg[(int64_t)y * w + x] = a;
    int next = a;
    if (y + 1 < h2) { const int C = in[(int64_t)(2 * y + 2) * w + x], D = in[(int64_t)(2 * y + 3) * w + x]; next = (C + D + (C > D)) >> 1; }
    else if (h & 1) next = in[(int64_t)(2 * y + 2) * w + x];
    const int top = y > 0 ? in[(int64_t)(2 * y - 1) * w + x] : a;
    res[(int64_t)y * w + x] = (A - B) - smooth_tendency(top, a, next);
}
__global__ __launch_bounds__(256) void k_scale(int32_t *d, int64_t n, int q) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = narrow16(d[i] * q);   // quantize.h:41
}
void launch_scale(int32_t *plane, int64_t n, int q, hipStream_t stream) {
    if (n <= 0 || q == 1) return;
    hipLaunchKernelGGL(k_scale, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65535)), dim3(256), 0, stream, plane, n, q);
}
// transform/quantize.h:54-71 fwd_quantize of one plane, in place: every sample divided by the channel's constant, truncating toward
// zero like C.  The range of the quotients (what encoding.cpp:737-739 recomputes before the stream is written) comes out of the same
// pass: every lane keeps its own minimum and maximum over its grid-stride samples, the block folds the 256 pairs through LDS, and
// ONE lane per block touches the two result words.  The division is the compiler's: q is uniform, the pass moves 8 bytes per sample.
// (LDS, __syncthreads, atomicMax and atomicCAS are what the wavefront emulator of the CPU suite offered when this was written; it has
// had atomicMin and __shfl_xor since k_channel_stats below.)
__device__ __forceinline__ void atomic_min_i32(int32_t *p, int32_t v) {
    int32_t seen = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (v < seen) {
        const int32_t was = atomicCAS(p, seen, v);
        if (was == seen) break;
        seen = was;
    }
}
__device__ __forceinline__ void fwd_quantize_plane(int32_t *plane, int64_t n, int q, int32_t *minmax, int block, int n_blocks) {
    __shared__ int32_t s_mn[256], s_mx[256];
    const int t = threadIdx.x;
    if ((int64_t)block * 256 >= n) return;   // the whole block: it has no sample of this plane
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    const int64_t first = (int64_t)block * 256 + t, step = (int64_t)n_blocks * 256;
    // four samples per load and store where the plane starts on a 16-byte boundary (every plane of the writer does); the last n & 3
    // samples, or a plane that does not, go one by one
    const int64_t n4 = (reinterpret_cast<uintptr_t>(plane) & 15) == 0 ? n >> 2 : 0;
    int4 *quads = reinterpret_cast<int4 *>(plane);
    for (int64_t i = first; i < n4; i += step) {
        int4 v = quads[i];
        v.x /= q; v.y /= q; v.z /= q; v.w /= q;
        if (q != 1) quads[i] = v;
        mn = min(min(mn, v.x), min(min(v.y, v.z), v.w)); mx = max(max(mx, v.x), max(max(v.y, v.z), v.w));
    }
    for (int64_t i = 4 * n4 + first; i < n; i += step) {
        const int32_t v = plane[i] / q;
        if (q != 1) plane[i] = v;
        mn = min(mn, v); mx = max(mx, v);
    }
    if (!minmax) return;
    s_mn[t] = mn; s_mx[t] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { s_mn[t] = min(s_mn[t], s_mn[t + s]); s_mx[t] = max(s_mx[t], s_mx[t + s]); }
        __syncthreads();
    }
    if (t == 0) { atomic_min_i32(minmax, s_mn[0]); atomicMax(minmax + 1, s_mx[0]); }
}
// every channel of a picture in one launch: the channels' blocks lie one behind the other in a 1-D grid (QuantChan::first_block, n_blocks),
// so a picture's 60 channels of very different sizes cost no empty blocks; a block finds its channel by bisection (uniform: scalar loads).
// minmax + 2 * slot is the channel's {min, max} pair
__global__ __launch_bounds__(256) void k_fwd_quantize(const QuantChan *table, int n_channels, int32_t *minmax) {
    const int b = blockIdx.x;
    int lo = 0, hi = n_channels - 1;       // the last entry whose first_block <= b (entries without blocks share their successor's)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const QuantChan c = table[lo];
    fwd_quantize_plane(c.plane, c.n, c.q, c.slot >= 0 ? minmax + 2 * (int64_t)c.slot : nullptr, b - c.first_block, c.n_blocks);
}
__global__ __launch_bounds__(256) void k_fwd_quantize_plane(int32_t *plane, int64_t n, int q, int32_t *minmax) {
    fwd_quantize_plane(plane, n, q, minmax, blockIdx.x, gridDim.x);
}
// blocks per plane: 2048 samples (two loads of four per lane) each until the grid is wide enough to fill the device
int fwd_quantize_blocks(int64_t n) { return n <= 0 ? 0 : (int)std::min<int64_t>((n + 2047) / 2048, 1024); }
void launch_fwd_quantize(const QuantChan *dev_table, int n_channels, int total_blocks, int32_t *dev_minmax, hipStream_t stream) {
    if (n_channels <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(k_fwd_quantize, dim3((unsigned)total_blocks), dim3(256), 0, stream, dev_table, n_channels, dev_minmax);
}
void launch_fwd_quantize_plane(int32_t *plane, int64_t n, int q, int32_t *dev_minmax, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_fwd_quantize_plane, dim3((unsigned)fwd_quantize_blocks(n)), dim3(256), 0, stream, plane, n, q, dev_minmax);
}
// {min, max, zero samples} of planes nobody writes: what the writer needs of a transformed channel before it codes it (encoding.cpp:737-739
// and the "predictability" byte of encoding.cpp:113-121) when the channel stays on the device.  One read per sample, nothing stored: up to three
// samples one by one until the address is a multiple of 16, four per load from there, the last ones one by one again.  Every lane folds its
// grid-stride samples, the wavefront folds its 64 lanes with shuffles, and ONE lane per wavefront touches the three result words.
__global__ __launch_bounds__(256) void k_channel_stats(const StatsRec *table, int n_recs, StatsRec one, int32_t *stats) {
    const int b = blockIdx.x;
    int lo = 0;
    if (table) {
        int hi = n_recs - 1;                // the last record whose first_block <= b (records without blocks share their successor's)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
        }
        one = table[lo];
    }
    const int64_t n = one.n;
    const int64_t first = (int64_t)(b - one.first_block) * 256 + threadIdx.x, step = (int64_t)one.n_blocks * 256;
    if (first - threadIdx.x >= n) return;   // the whole block: it has no sample of this plane
    const int32_t *plane = one.plane;
    const int64_t to16 = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(plane) >> 2) & 3)) & 3), head = to16 < n ? to16 : n;
    const int64_t n4 = (n - head) >> 2, ends = n - 4 * n4;   // ends: the samples in front of and behind the quads
    const int4 *quads = reinterpret_cast<const int4 *>(plane + head);
    int32_t mn = INT32_MAX, mx = INT32_MIN, zeros = 0;
    for (int64_t i = first; i < n4; i += step) {
        const int4 v = quads[i];
        mn = min(min(mn, v.x), min(min(v.y, v.z), v.w)); mx = max(max(mx, v.x), max(max(v.y, v.z), v.w));
        zeros += (v.x == 0) + (v.y == 0) + (v.z == 0) + (v.w == 0);
    }
    for (int64_t k = first; k < ends; k += step) {
        const int32_t v = plane[k < head ? k : k + 4 * n4];
        mn = min(mn, v); mx = max(mx, v); zeros += v == 0;
    }
    for (int m = 1; m < 64; m <<= 1) {
        mn = min(mn, __shfl_xor(mn, m)); mx = max(mx, __shfl_xor(mx, m)); zeros += __shfl_xor(zeros, m);
    }
    if ((threadIdx.x & 63) == 0 && mn <= mx) {   // (a wavefront none of whose lanes had a sample keeps mn > mx)
        int32_t *s = stats + 3 * (int64_t)lo;
        atomicMin(s, mn); atomicMax(s + 1, mx); atomicAdd(s + 2, zeros);
    }
}
// blocks per plane: 2048 samples (two loads of four per lane) each until the grid is wide enough to fill the device
int channel_stats_blocks(int64_t n) { return fwd_quantize_blocks(n); }
void launch_channel_stats(const StatsRec *dev_table, int n_recs, StatsRec one, int total_blocks, int32_t *dev_stats, hipStream_t stream) {
    if (total_blocks <= 0) return;
    hipLaunchKernelGGL(k_channel_stats, dim3((unsigned)total_blocks), dim3(256), 0, stream, dev_table, n_recs, one, dev_stats);
}
// import/read_yuv.h:29-63 on the GPU: raw 4:2:0 frames (8-bit samples, or 16-bit little-endian ones; planar, or with the chroma samples
// as one plane of Cb, Cr pairs; rows `pitch` bytes apart) -> tight int32 planes.  Bandwidth bound, 1.5-3 bytes in and 6 out per pixel; no LDS.
// The grid runs over (row segment, plane, frame): a wavefront takes one row segment, a lane one aligned load of 4 samples (4 or 8 bytes)
// or, in a plane of pairs, of 4 pairs (8 or 16 bytes) -- consecutive lanes read consecutive words, a wavefront 256 B to 1 KiB per
// instruction -- and stores them as int32x4, one store per output plane, wherever the destination is on a 16-byte boundary (it is
// for tight frames whose width is a multiple of 4, a hardware decoder's; else four dword stores, still consecutive across the lanes).
// A row starts at base + y * pitch, on any byte (a row of 16-bit samples on an odd byte goes one by one as a whole): the ELEMENTS (samples of a row, Cb and Cr alike) in
// front of the first aligned word and behind the last whole one, at most 3 (7 in a plane of pairs) each, go one by one, byte loads, in
// the first lanes of the row's first segment, as fwd_quantize_plane treats the ends of a plane.  No load touches a byte outside
// [row, row + row bytes): the caller's surface may end with its last row.  In a plane of pairs whose first aligned word starts with a
// Cr sample the odd elements of every word are the Cb samples and the Cr samples belong to the pair before.
template <int BYTES>
__device__ __forceinline__ uint32_t yuv_element(const uint32_t *words, int i) {   // element i of a loaded vector (little-endian)
    return BYTES == 1 ? (words[i >> 2] >> (8 * (i & 3))) & 0xFFu : (words[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
}
template <int BYTES>
__device__ __forceinline__ uint32_t yuv_element_at(const uint8_t *p) {   // one by one: byte loads, any address
    return BYTES == 1 ? p[0] : (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}
// (a compiler vector, one 16-byte store instruction in the IR: written as an int4 struct the aligned form is four member stores, which the
// optimiser merges with the four dword stores of the other branch -- and no dwordx4 store is left, profiles/yuv_forward.txt)
typedef int32_t yuv_quad_t __attribute__((vector_size(16)));
__device__ __forceinline__ void store_quad(int32_t *dst, int a, int b, int c, int d) {
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) { const yuv_quad_t v = {a, b, c, d}; *reinterpret_cast<yuv_quad_t *>(dst) = v; }
    else { dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d; }
}
// one row segment: `n` elements at `row`; PAIRS: element e is component e & 1 of pair e >> 1, which goes to out0 / out1 [e >> 1]; else to out0[e].
// k: the lane's vector among the row's; first_segment: this wavefront also takes the row's ends.  Returns whether a sample exceeded maxval
template <int BYTES, bool PAIRS>
__device__ __forceinline__ bool unpack_row_segment(const uint8_t *row, int64_t n, int32_t *out0, int32_t *out1, int64_t k, bool first_segment, int lane,
                                                   uint32_t maxval) {
    constexpr int E = PAIRS ? 8 : 4, VB = E * BYTES;            // elements and bytes of one vector load
    const int64_t to_aligned = (int64_t)((VB - (reinterpret_cast<uintptr_t>(row) & (VB - 1))) & (VB - 1)) / BYTES;
    const bool split_samples = BYTES == 2 && (reinterpret_cast<uintptr_t>(row) & 1);   // 16-bit samples on odd addresses: no aligned word holds whole ones, the row is all head
    const int64_t head = to_aligned < n && !split_samples ? to_aligned : n, nvec = (n - head) / E, tail = n - head - nvec * E;
    uint32_t over = 0;
    if (k < nvec) {
        const int64_t e0 = head + k * E;
        uint32_t words[VB / 4];
        if constexpr (VB == 4) words[0] = *reinterpret_cast<const uint32_t *>(row + e0 * BYTES);
        else if constexpr (VB == 8) { const uint2 v = *reinterpret_cast<const uint2 *>(row + e0 * BYTES); words[0] = v.x; words[1] = v.y; }
        else {
            const int4 v = *reinterpret_cast<const int4 *>(row + e0 * BYTES);
            words[0] = (uint32_t)v.x; words[1] = (uint32_t)v.y; words[2] = (uint32_t)v.z; words[3] = (uint32_t)v.w;
        }
        uint32_t s[E];
        for (int i = 0; i < E; i++) { s[i] = yuv_element<BYTES>(words, i); over |= s[i] > maxval; }
        if constexpr (!PAIRS) store_quad(out0 + e0, (int)s[0], (int)s[1], (int)s[2], (int)s[3]);
        else {
            // even e0: elements 0, 2, 4, 6 are Cb of pairs e0/2 .. e0/2 + 3 and the odd ones their Cr; odd e0: the odd elements are Cb of pairs
            // (e0+1)/2 .., the even ones Cr of the pairs one before
            const bool swapped = (e0 & 1) != 0;
            store_quad((swapped ? out1 : out0) + (e0 >> 1), (int)s[0], (int)s[2], (int)s[4], (int)s[6]);
            store_quad((swapped ? out0 : out1) + ((e0 + 1) >> 1), (int)s[1], (int)s[3], (int)s[5], (int)s[7]);
        }
    }
    if (first_segment)   // the ends: at most E - 1 elements each (a row of split samples: all of it), one per lane and pass
        for (int64_t i = lane; i < head + tail; i += 64) {
            const int64_t e = i < head ? i : i + nvec * E;
            const uint32_t v = yuv_element_at<BYTES>(row + e * BYTES);
            over |= v > maxval;
            if (!PAIRS) out0[e] = (int32_t)v;
            else ((e & 1) ? out1 : out0)[e >> 1] = (int32_t)v;
        }
    return over != 0;
}
__global__ __launch_bounds__(256) void k_unpack_yuv420(const YuvJob *table, YuvJob one, YuvGeom g, int segs, int32_t *flag) {
    const int job = blockIdx.z / g.nb_frames, f = blockIdx.z - job * g.nb_frames;
    if (table) one = table[job];
    const int p = blockIdx.y;                       // 0: Y; planar: 1 Cb, 2 Cr; nv12: 1 the plane of pairs
    const int pw = p ? g.cw : g.w, ph = p ? g.ch : g.h;
    const int rows4 = blockIdx.x / segs, seg = blockIdx.x - rows4 * segs;
    const int y = rows4 * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // a block: four rows, one wavefront each
    if (y >= ph) return;
    const bool pairs = p && g.nv12;
    const int64_t plane_at = p == 0 ? 0 : g.pitch_y * g.h + (p == 2 ? g.pitch_c * g.ch : 0);
    const uint8_t *row = one.src + f * g.frame_bytes + plane_at + y * (p ? g.pitch_c : g.pitch_y);
    const int64_t plane_samples = (int64_t)pw * ph, at = f * plane_samples + (int64_t)y * pw;
    int32_t *out0 = one.out[p] + at, *out1 = pairs ? one.out[2] + at : nullptr;
    const int64_t k = (int64_t)seg * 64 + lane;
    bool over;
    if (g.bytes == 1) over = pairs ? unpack_row_segment<1, true>(row, 2 * (int64_t)pw, out0, out1, k, seg == 0, lane, (uint32_t)g.maxval)
                                   : unpack_row_segment<1, false>(row, pw, out0, out1, k, seg == 0, lane, (uint32_t)g.maxval);
    else over = pairs ? unpack_row_segment<2, true>(row, 2 * (int64_t)pw, out0, out1, k, seg == 0, lane, (uint32_t)g.maxval)
                      : unpack_row_segment<2, false>(row, pw, out0, out1, k, seg == 0, lane, (uint32_t)g.maxval);
    if (over && flag) atomicOr(flag, 1);   // (rare: a lane that met one)
}
void launch_unpack_yuv420(const YuvJob *dev_table, int n_jobs, YuvJob one, const YuvGeom &g, int32_t *dev_flag, hipStream_t stream) {
    if (n_jobs <= 0 || g.w <= 0 || g.h <= 0 || g.nb_frames <= 0 || g.nb_frames > 65535) return;   // (the callers refuse longer clips)
    // a luma row has at most w / 4 whole vectors, a chroma row or a row of pairs no more; every row has a first segment for its ends
    const int segs = std::max(1, (g.w / 4 + 63) / 64);
    const int64_t frames = (int64_t)n_jobs * g.nb_frames;
    for (int64_t z0 = 0; z0 < frames; z0 += 65535 / g.nb_frames * g.nb_frames) {   // (grid.z holds 65535: whole jobs per launch)
        const int64_t nz = std::min<int64_t>(frames - z0, 65535 / g.nb_frames * g.nb_frames);
        hipLaunchKernelGGL(k_unpack_yuv420, dim3((unsigned)(segs * ((g.h + 3) / 4)), g.nv12 ? 2u : 3u, (unsigned)nz), dim3(256), 0, stream,
                           dev_table ? dev_table + z0 / g.nb_frames : nullptr, one, g, segs, dev_flag);
    }
}
// export/write_yuv.h:29-58 on the GPU, the inverse of k_unpack_yuv420: tight (or block-padded, then cropped) int32 planes -> raw 4:2:0 frames,
// every sample CLAMP(v, 0, maxval) (write_yuv.h:49), one byte each or two little-endian; planar, or the chroma samples as one plane of Cb, Cr
// pairs; rows `pitch` bytes apart.  Bandwidth bound, 6 bytes in and 1.5-3 out per pixel; no LDS.  The same grid and lane mapping as the
// unpacking: a wavefront takes one row segment, a lane reads 4 samples (one int32x4 load wherever the source is on a 16-byte boundary, else
// four dword loads, still consecutive across the lanes) -- in a plane of pairs 4 + 4 -- and writes ONE aligned word of 4 or 8 (pairs: 8 or 16)
// bytes; consecutive lanes write consecutive words.  The ELEMENTS in front of the row's first aligned destination word and behind its last
// whole one, at most 3 (7) each, go one by one as byte stores in the first lanes of the row's first segment; a row of 16-bit samples on an odd
// byte goes that way as a whole.  No store touches a byte outside [row, row + row bytes): pitch padding and whatever follows the last sample
// of the last row stay the caller's.
typedef uint32_t yuv_word2_t __attribute__((vector_size(8)));
typedef uint32_t yuv_word4_t __attribute__((vector_size(16)));
__device__ __forceinline__ void load_quad(const int32_t *src, int32_t *v) {
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) { const yuv_quad_t q = *reinterpret_cast<const yuv_quad_t *>(src); v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3]; }
    else { v[0] = src[0]; v[1] = src[1]; v[2] = src[2]; v[3] = src[3]; }
}
template <int BYTES>
__device__ __forceinline__ void yuv_store_element(uint8_t *p, uint32_t v) {   // one by one: byte stores, any address
    p[0] = (uint8_t)v;
    if (BYTES == 2) p[1] = (uint8_t)(v >> 8);
}
// one row segment: `n` elements to `row`; PAIRS: element e is component e & 1 of pair e >> 1 and comes from in0 / in1 [e >> 1]; else from in0[e].
// k: the lane's word among the row's; first_segment: this wavefront also takes the row's ends
template <int BYTES, bool PAIRS>
__device__ __forceinline__ void pack_row_segment(uint8_t *row, int64_t n, const int32_t *in0, const int32_t *in1, int64_t k, bool first_segment, int lane,
                                                 int maxval) {
    constexpr int E = PAIRS ? 8 : 4, VB = E * BYTES;            // elements and bytes of one word store
    const int64_t to_aligned = (int64_t)((VB - (reinterpret_cast<uintptr_t>(row) & (VB - 1))) & (VB - 1)) / BYTES;
    const bool split_samples = BYTES == 2 && (reinterpret_cast<uintptr_t>(row) & 1);   // 16-bit samples on odd addresses: no aligned word holds whole ones, the row is all head
    const int64_t head = to_aligned < n && !split_samples ? to_aligned : n, nvec = (n - head) / E, tail = n - head - nvec * E;
    if (k < nvec) {
        const int64_t e0 = head + k * E;
        int32_t s[E];
        if constexpr (!PAIRS) load_quad(in0 + e0, s);
        else {
            // even e0: elements 0, 2, 4, 6 are Cb of pairs e0/2 .. e0/2 + 3 and the odd ones their Cr; odd e0: the odd elements are Cb of pairs
            // (e0+1)/2 .., the even ones Cr of the pairs one before
            const bool swapped = (e0 & 1) != 0;
            int32_t a[4], b[4];
            load_quad((swapped ? in1 : in0) + (e0 >> 1), a);
            load_quad((swapped ? in0 : in1) + ((e0 + 1) >> 1), b);
            for (int i = 0; i < 4; i++) { s[2 * i] = a[i]; s[2 * i + 1] = b[i]; }
        }
        uint32_t words[VB / 4];
        for (int i = 0; i < VB / 4; i++) words[i] = 0;
        for (int i = 0; i < E; i++) {
            const uint32_t v = (uint32_t)clampi(s[i], 0, maxval);
            if (BYTES == 1) words[i >> 2] |= v << (8 * (i & 3));
            else words[i >> 1] |= v << (16 * (i & 1));
        }
        uint8_t *dst = row + e0 * BYTES;
        if constexpr (VB == 4) *reinterpret_cast<uint32_t *>(dst) = words[0];
        else if constexpr (VB == 8) { const yuv_word2_t v = {words[0], words[1]}; *reinterpret_cast<yuv_word2_t *>(dst) = v; }
        else { const yuv_word4_t v = {words[0], words[1], words[2], words[3]}; *reinterpret_cast<yuv_word4_t *>(dst) = v; }
    }
    if (first_segment)   // the ends: at most E - 1 elements each (a row of split samples: all of it), one per lane and pass
        for (int64_t i = lane; i < head + tail; i += 64) {
            const int64_t e = i < head ? i : i + nvec * E;
            const int32_t v = !PAIRS ? in0[e] : ((e & 1) ? in1 : in0)[e >> 1];
            yuv_store_element<BYTES>(row + e * BYTES, (uint32_t)clampi(v, 0, maxval));
        }
}
__global__ __launch_bounds__(256) void k_pack_yuv420(YuvPackJob job, YuvGeom g, int segs) {
    const int pic = blockIdx.z / g.nb_frames, f = blockIdx.z - pic * g.nb_frames;
    const int p = blockIdx.y;                       // 0: Y; planar: 1 Cb, 2 Cr; nv12: 1 the plane of pairs
    const int pw = p ? g.cw : g.w, ph = p ? g.ch : g.h;
    const int rows4 = blockIdx.x / segs, seg = blockIdx.x - rows4 * segs;
    const int y = rows4 * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // a block: four rows, one wavefront each
    if (y >= ph) return;
    const bool pairs = p && g.nv12;
    const int64_t plane_at = p == 0 ? 0 : g.pitch_y * g.h + (p == 2 ? g.pitch_c * g.ch : 0);
    uint8_t *row = job.dst + pic * job.dst_stride + f * g.frame_bytes + plane_at + y * (p ? g.pitch_c : g.pitch_y);
    const int64_t src_row = (int64_t)f * ph + y;    // the frames of a clip are stacked in every plane
    const int32_t *in0 = job.plane[p] + pic * job.image_stride + src_row * job.row_pitch[p];
    const int32_t *in1 = pairs ? job.plane[2] + pic * job.image_stride + src_row * job.row_pitch[2] : nullptr;
    const int64_t k = (int64_t)seg * 64 + lane;
    if (g.bytes == 1) {
        if (pairs) pack_row_segment<1, true>(row, 2 * (int64_t)pw, in0, in1, k, seg == 0, lane, g.maxval);
        else pack_row_segment<1, false>(row, pw, in0, in1, k, seg == 0, lane, g.maxval);
    } else {
        if (pairs) pack_row_segment<2, true>(row, 2 * (int64_t)pw, in0, in1, k, seg == 0, lane, g.maxval);
        else pack_row_segment<2, false>(row, pw, in0, in1, k, seg == 0, lane, g.maxval);
    }
}
void launch_pack_yuv420(const YuvPackJob &job, int n_pictures, const YuvGeom &g, hipStream_t stream) {
    if (n_pictures <= 0 || g.w <= 0 || g.h <= 0 || g.nb_frames <= 0 || g.nb_frames > 65535) return;   // (the callers refuse longer clips)
    // a luma row has at most w / 4 whole words, a chroma row or a row of pairs no more; every row has a first segment for its ends
    const int segs = std::max(1, (g.w / 4 + 63) / 64);
    const int64_t frames = (int64_t)n_pictures * g.nb_frames, per_launch = 65535 / g.nb_frames * g.nb_frames;   // (grid.z holds 65535: whole pictures per launch)
    for (int64_t z0 = 0; z0 < frames; z0 += per_launch) {
        const int64_t nz = std::min<int64_t>(frames - z0, per_launch), pic0 = z0 / g.nb_frames;
        YuvPackJob part = job;
        for (int p = 0; p < 3; p++) part.plane[p] += pic0 * job.image_stride;
        part.dst += pic0 * job.dst_stride;
        hipLaunchKernelGGL(k_pack_yuv420, dim3((unsigned)(segs * ((g.h + 3) / 4)), g.nv12 ? 2u : 3u, (unsigned)nz), dim3(256), 0, stream, part, g, segs);
    }
}
// ---------------------------------------------------------------------------------------------
// Forward Palette (transform/palette.h:92-142): which colour tuples occur, then every pixel's colour number.  The reference inserts every
// pixel into a std::set and searches the palette linearly per pixel; here the set is built by all lanes at once and the order of the
// colours (the set's: lexicographic, signed) is made by the host from the few colours found (capi.hip fwd_palette_gpu).
// Every loop below is bounded: the grid-stride loops by n, a probe sequence by the capacity of the table.
//
// Several channels (2..4): the tuple's int16 components packed into 64 bits are the key of an open-addressing table in device memory
// (linear probing, capacity a power of two of at least twice the limit), claimed with a 64-bit compare-and-swap on an empty slot.  Four
// int16 fill the 64 bits, so no key can mean "empty": an empty slot holds 0 and the ONE tuple whose key is 0 is kept apart, in ctl[2].
// The common case -- the colour is in the table already -- is one load; atomics happen once per distinct colour and lane that races for it.
// ctl[0] counts the distinct colours; when it passes the limit ctl[1] is set and every lane stops at its next sample, so a photograph
// costs one insert per lane in flight.  Those inserts can at most fill the table: a probe sequence looks at ctl[1] every 32 slots, and one
// that has seen `capacity` slots ends and reports "too many" (a full table holds more than the limit).  ctl[3]: a sample outside int16.
constexpr int PAL_CTL_COUNT = 0, PAL_CTL_TOO_MANY = 1, PAL_CTL_ZERO_KEY = 2, PAL_CTL_BAD_SAMPLE = 3;
DEV bool palette_key(const PalettePlanes &pp, int64_t i, unsigned long long &key) {
    key = 0;
    bool ok = true;
    for (int c = 0; c < pp.nb; c++) {
        const int32_t v = pp.p[c][i];
        ok &= (uint32_t)(v + 32768) < 65536u;
        key |= (unsigned long long)(uint16_t)v << (16 * c);
    }
    return ok;
}
DEV uint32_t palette_slot(unsigned long long key, int shift) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift); }   // shift = 64 - log2(capacity)
DEV void palette_count_one(uint32_t *ctl, uint32_t limit) {
    if (atomicAdd(ctl + PAL_CTL_COUNT, 1u) + 1u > limit) atomicOr(ctl + PAL_CTL_TOO_MANY, 1u);
}
__global__ __launch_bounds__(256) void k_palette_collect(PalettePlanes pp, int64_t n, unsigned long long *keys, uint32_t cap_mask, int shift, uint32_t limit,
                                                         uint32_t *ctl) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        if (__hip_atomic_load(ctl + PAL_CTL_TOO_MANY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        unsigned long long key;
        if (!palette_key(pp, i, key)) { atomicOr(ctl + PAL_CTL_BAD_SAMPLE, 1u); return; }
        if (key == 0) {
            if (!__hip_atomic_load(ctl + PAL_CTL_ZERO_KEY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) && atomicOr(ctl + PAL_CTL_ZERO_KEY, 1u) == 0)
                palette_count_one(ctl, limit);
            continue;
        }
        uint32_t slot = palette_slot(key, shift) & cap_mask;
        bool placed = false;
        for (uint32_t probe = 0; probe <= cap_mask && !placed; probe++, slot = (slot + 1) & cap_mask) {
            // a photograph: every lane in flight brings a colour of its own and the table fills; long probe sequences look at the verdict
            if ((probe & 31) == 31 && __hip_atomic_load(ctl + PAL_CTL_TOO_MANY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
            unsigned long long cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0) {
                cur = atomicCAS(keys + slot, 0ull, key);
                if (cur == 0) { palette_count_one(ctl, limit); placed = true; }
            }
            placed |= cur == key;
        }
        if (!placed) atomicOr(ctl + PAL_CTL_TOO_MANY, 1u);   // every slot holds another colour
    }
}
// rank[slot]: the colour number of the key in that slot (zero_rank: of the key 0); index may be pp.p[0] -- a lane reads its tuple, then writes
__global__ __launch_bounds__(256) void k_palette_index(PalettePlanes pp, int64_t n, const unsigned long long *keys, const int32_t *rank, uint32_t cap_mask,
                                                       int shift, int32_t zero_rank, int32_t *index) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        unsigned long long key;
        palette_key(pp, i, key);
        int32_t found = zero_rank;
        if (key != 0) {
            found = 0;   // (a key the collect pass has not seen cannot occur; it would end at an empty slot or after `capacity` probes)
            uint32_t slot = palette_slot(key, shift) & cap_mask;
            for (uint32_t probe = 0; probe <= cap_mask; probe++, slot = (slot + 1) & cap_mask) {
                const unsigned long long cur = keys[slot];
                if (cur == key) { found = rank[slot]; break; }
                if (cur == 0) break;
            }
        }
        index[i] = found;
    }
}
// One channel (channel compaction): the limit reaches 0.7 x 65536 there, so the set is a presence bitmap over the int16 range -- 8 KB,
// one per workgroup in LDS (a bit that is already set costs a read), OR-ed into the global one word by word at the end.  The colours are
// its set bits in ascending order and a sample's colour number the count of set bits below its own: prefix[w] = set bits in words < w.
constexpr int PAL_BITMAP_WORDS = 65536 / 32;
__global__ __launch_bounds__(256) void k_palette_collect1(const int32_t *plane, int64_t n, uint32_t *bitmap, uint32_t *ctl) {
    __shared__ uint32_t s_bits[PAL_BITMAP_WORDS];
    for (int k = threadIdx.x; k < PAL_BITMAP_WORDS; k += blockDim.x) s_bits[k] = 0;
    __syncthreads();
    bool bad = false;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t u = (uint32_t)(plane[i] + 32768);
        if (u >= 65536u) { bad = true; continue; }
        const uint32_t m = 1u << (u & 31);
        if (!(s_bits[u >> 5] & m)) atomicOr(&s_bits[u >> 5], m);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PAL_BITMAP_WORDS; k += blockDim.x)
        if (s_bits[k]) atomicOr(bitmap + k, s_bits[k]);
    if (bad) atomicOr(ctl + PAL_CTL_BAD_SAMPLE, 1u);
}
__global__ __launch_bounds__(256) void k_palette_index1(const int32_t *plane, int64_t n, const uint32_t *bitmap, const int32_t *prefix, int32_t *index) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t u = (uint32_t)(plane[i] + 32768) & 0xFFFFu;
        index[i] = prefix[u >> 5] + (int32_t)__popcll((unsigned long long)(bitmap[u >> 5] & ((1u << (u & 31)) - 1u)));
    }
}
// 2048 samples per block until 512 blocks fill the device (each block of the one-channel form ends with up to 2048 atomics)
static unsigned palette_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, 512)); }
void launch_palette_collect(const PalettePlanes &pp, int64_t n, unsigned long long *dev_keys, uint32_t capacity, uint32_t limit, uint32_t *dev_ctl, hipStream_t stream) {
    if (n <= 0) return;
    int log2cap = 0;
    while ((1u << log2cap) < capacity) log2cap++;
    hipLaunchKernelGGL(k_palette_collect, dim3(palette_blocks(n)), dim3(256), 0, stream, pp, n, dev_keys, capacity - 1, 64 - log2cap, limit, dev_ctl);
}
void launch_palette_index(const PalettePlanes &pp, int64_t n, const unsigned long long *dev_keys, const int32_t *dev_rank, uint32_t capacity, int32_t zero_rank,
                          int32_t *index, hipStream_t stream) {
    if (n <= 0) return;
    int log2cap = 0;
    while ((1u << log2cap) < capacity) log2cap++;
    hipLaunchKernelGGL(k_palette_index, dim3(palette_blocks(n)), dim3(256), 0, stream, pp, n, dev_keys, dev_rank, capacity - 1, 64 - log2cap, zero_rank, index);
}
void launch_palette_collect1(const int32_t *plane, int64_t n, uint32_t *dev_bitmap, uint32_t *dev_ctl, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_palette_collect1, dim3(palette_blocks(n)), dim3(256), 0, stream, plane, n, dev_bitmap, dev_ctl);
}
void launch_palette_index1(const int32_t *plane, int64_t n, const uint32_t *dev_bitmap, const int32_t *dev_prefix, int32_t *index, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_palette_index1, dim3(palette_blocks(n)), dim3(256), 0, stream, plane, n, dev_bitmap, dev_prefix, index);
}
// ---------------------------------------------------------------------------------------------
// Forward Matching against the previous frame (transform/2dmatch.h:303-381 with maxdist = -1: what the CLI does for an animation).
// The strip is nb_frames pictures of w x fh one above the other; a sample of row y >= fh "equals" when every plane holds what it holds
// fh rows up.  The reference walks each row with a counter and back-fills (2dmatch.h:314-335): what comes out is m = 1 on every maximal
// horizontal run of equal samples that is at least minmatch long.  Here one wavefront takes one row, 64 samples at a time: the ballot of
// "equals" is the chunk's mask, a lane finds the unequal sample below and above itself in it, `carry` brings the run that ends in front
// of the chunk (saturated at 64: minmatch <= 40) and the mask of the NEXT chunk, taken one iteration ahead, the run that goes on behind
// it -- a run that crosses a whole chunk is long enough whatever follows.  Rows of frame 0 are written 0, so the kernel defines every
// sample of m; a row narrower than minmatch gets zeros.  Every loop runs ceil(w / 64) times for all 64 lanes (the ballots are uniform).
__global__ __launch_bounds__(64) void k_match_frames_runs(MatchPlanes mp, int w, int fh, int minmatch, int64_t pic_stride, int32_t *match) {
    const int y = blockIdx.x, lane = threadIdx.x;
    const int64_t pic = (int64_t)blockIdx.z * pic_stride, row = pic + (int64_t)y * w, up = row - (int64_t)fh * w;
    if (y < fh) {
        for (int x = lane; x < w; x += 64) match[row + x] = 0;
        return;
    }
    auto equal_at = [&](int x) {
        if (x >= w) return false;
        bool eq = true;
        for (int c = 0; c < mp.nb; c++) eq &= mp.p[c][row + x] == mp.p[c][up + x];
        return eq;
    };
    unsigned long long cur = __ballot(equal_at(lane));
    int carry = 0;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const unsigned long long next = __ballot(equal_at(x0 + 64 + lane));
        const unsigned long long differ = ~cur;
        bool long_enough = false;
        if ((cur >> lane) & 1ull) {
            const unsigned long long below = differ & ((1ull << lane) - 1ull);
            const int left = below ? lane - 64 + __builtin_clzll(below) : lane + carry;            // equal samples in front of this one
            const unsigned long long above = lane < 63 ? differ >> (lane + 1) : 0ull;
            const int right = above ? __builtin_ctzll(above) : 63 - lane + (~next ? __builtin_ctzll(~next) : 64);   // ... and behind it
            long_enough = left + 1 + right >= minmatch;
        }
        if (x0 + lane < w) match[row + x0 + lane] = long_enough ? 1 : 0;
        carry = differ ? __builtin_clzll(differ) : 64;
        cur = next;
    }
}
// The three erode sweeps of 2dmatch.h:355-369.  The reference sweeps in place in raster order and flags (negates) a matched sample when
// the sample above or to its left is 0 -- those were visited before it, so 0 there means "never matched", whatever the sweep -- or when
// the sample below or to its right is <= 0 -- not visited yet, so: never matched, or flagged by an EARLIER sweep.  The picture's bottom,
// left and right edges do not count; the row above frame 1 is frame 0's last, all zero.  So sweep k flags what sweep k-1 flagged plus the
// matched samples whose matched lower or right neighbour sweep k-1 flagged, and three sweeps are this depth-3 recursion over the
// match channel AS k_match_frames_runs LEFT IT.  The kernel works in place: it only ever asks "is this sample 0", and a flag turns 1
// into -1, never into 0, so a neighbour that another lane has flagged already answers as it did before.
template <int SWEEPS>
DEV bool match_flagged(const int32_t *m, int w, int h, int x, int y) {   // (x, y) is matched
    const int64_t i = (int64_t)y * w + x;
    if constexpr (SWEEPS == 1) {
        return m[i - w] == 0 || (x > 0 && m[i - 1] == 0) || (y + 1 < h && m[i + w] == 0) || (x + 1 < w && m[i + 1] == 0);
    } else {
        return match_flagged<SWEEPS - 1>(m, w, h, x, y) || (y + 1 < h && m[i + w] != 0 && match_flagged<SWEEPS - 1>(m, w, h, x, y + 1)) ||
               (x + 1 < w && m[i + 1] != 0 && match_flagged<SWEEPS - 1>(m, w, h, x + 1, y));
    }
}
__global__ __launch_bounds__(256) void k_match_frames_erode(int w, int h, int fh, int64_t pic_stride, int32_t *match) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)fh * w || i >= (int64_t)w * h) return;
    int32_t *m = match + (int64_t)blockIdx.z * pic_stride;
    if (m[i] != 0 && match_flagged<3>(m, w, h, (int)(i % w), (int)(i / w))) m[i] = -1;
}
// 2dmatch.h:372-379: a matched sample that kept its mark is 0 in every plane (the decoder copies it from the frame above), a flagged one
// keeps its samples and is an ordinary 1 in the match channel again
__global__ __launch_bounds__(256) void k_match_frames_apply(MatchPlanes mp, int w, int h, int fh, int64_t pic_stride, int32_t *match) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)fh * w || i >= (int64_t)w * h) return;
    const int64_t at = (int64_t)blockIdx.z * pic_stride + i;
    const int32_t v = match[at];
    if (v > 0) for (int c = 0; c < mp.nb; c++) mp.p[c][at] = 0;
    else if (v < 0) match[at] = 1;
}
void launch_fwd_match_frames(const MatchPlanes &mp, int w, int h, int fh, int n_pictures, int64_t pic_stride, int32_t *match, hipStream_t stream) {
    if (w < 1 || h < 1 || n_pictures < 1) return;
    const int minmatch = std::max(5, std::min(40, w / 50));   // 2dmatch.h:312
    const unsigned blocks = (unsigned)(((int64_t)w * h + 255) / 256);
    hipLaunchKernelGGL(k_match_frames_runs, dim3((unsigned)h, 1, (unsigned)n_pictures), dim3(64), 0, stream, mp, w, fh, minmatch, pic_stride, match);
    hipLaunchKernelGGL(k_match_frames_erode, dim3(blocks, 1, (unsigned)n_pictures), dim3(256), 0, stream, w, h, fh, pic_stride, match);
    hipLaunchKernelGGL(k_match_frames_apply, dim3(blocks, 1, (unsigned)n_pictures), dim3(256), 0, stream, mp, w, h, fh, pic_stride, match);
}
void launch_fwd_ycocg(int32_t *c0, int32_t *c1, int32_t *c2, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_fwd_ycocg,dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c0, c1, c2, n);
}
void launch_fwd_squeeze(bool horizontal, const int32_t *in, int w, int h, int32_t *avg, int32_t *res, hipStream_t stream) {
    if (horizontal) hipLaunchKernelGGL(k_fwd_hsqueeze, dim3(((w + 1) / 2 + 255) / 256, h), dim3(256), 0, stream, in, w, h, avg, res);
    else hipLaunchKernelGGL(k_fwd_vsqueeze, dim3((w + 255) / 256, (h + 1) / 2), dim3(256), 0, stream, in, w, h, avg, res);
}

// export/write_pam.h:136-150 (the RGB / gray / +alpha path): for every pixel of the w x h image the first
// `components` channels, CLAMP(v, minval, maxval), one byte per sample or two bytes big-endian.  Planes may be
// wider than the image (DCT-padded): the row pitch is the plane's own width.  A quarter of the bytes of the
// int32 planes (an eighth for 8-bit images) is what a host that only wants the picture has to pull over PCIe.
__global__ __launch_bounds__(256) void k_pack_samples(Bases b, PackedPlanes pp, int w, int h, int lo, int hi, int bytes_per_sample, uint8_t *dst,
                                                      int64_t dst_stride) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= w) return;
    uint8_t *o = dst + (int64_t)blockIdx.z * dst_stride + ((int64_t)y * w + x) * pp.n * bytes_per_sample;
    for (int c = 0; c < pp.n; c++) {
        const int v = clampi(plane_ptr(b, pp.p[c], blockIdx.z)[(int64_t)y * pp.p[c].w + x], lo, hi);
        if (bytes_per_sample == 2) { o[2 * c] = (uint8_t)(v >> 8); o[2 * c + 1] = (uint8_t)(v & 0xFF); }
        else o[c] = (uint8_t)v;
    }
}

void launch_pack(const Bases &b, const PackedPlanes &pp, int w, int h, int lo, int hi, int bytes_per_sample, uint8_t *dst, int64_t dst_stride,
                 int n_images, hipStream_t stream) {
    if (w <= 0 || h <= 0 || n_images <= 0) return;
    hipLaunchKernelGGL(k_pack_samples, dim3((w + 255) / 256, h, n_images), dim3(256), 0, stream, b, pp, w, h, lo, hi, bytes_per_sample, dst, dst_stride);
}

// ---------------------------------------------------------------------------------------------
// Verification aid (no counterpart in the reference): one position-weighted 64-bit sum per image over a slab of int32 planes,
// sum_i v[i] * (i mod 65521 + 1) (two's-complement wrap-around) -- what fuif_amd.dist.plane_checksums computes with torch.  A host
// that decodes step after step (bench.py's overlapped steps, a service that re-decodes) keeps 8 bytes per image and step instead of
// the planes and compares afterwards; streaming, HBM bound (4 bytes per sample).  16-byte loads; blockIdx.y = image.
__global__ __launch_bounds__(256) void k_plane_checksums(const int32_t *planes, int64_t elems, int64_t stride, unsigned long long *sums) {
    const int32_t *src = planes + (int64_t)blockIdx.y * stride;
    unsigned long long acc = 0;
    const int64_t quads = elems / 4;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += step) {
        const int4 v = *reinterpret_cast<const int4 *>(src + 4 * q);
        const unsigned long long w0 = (unsigned long long)((4 * q) % 65521);      // weights w0+1 .. w0+4, each reduced mod 65521
        const long long vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            unsigned long long wk = w0 + (unsigned long long)k;
            if (wk >= 65521ull) wk -= 65521ull;
            acc += (unsigned long long)vs[k] * (wk + 1ull);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = quads * 4; i < elems; i++) acc += (unsigned long long)(long long)src[i] * ((unsigned long long)(i % 65521) + 1ull);
    __shared__ unsigned long long part[256];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(&sums[blockIdx.y], part[0]);
}
void launch_plane_checksums(const int32_t *planes, int64_t elems, int64_t stride, int n_images, unsigned long long *sums, hipStream_t stream) {
    if (n_images <= 0) return;
    (void)hipMemsetAsync(sums, 0, sizeof(unsigned long long) * (size_t)n_images, stream);
    if (elems <= 0) return;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((elems / 4 + 2047) / 2048, 256));
    hipLaunchKernelGGL(k_plane_checksums, dim3((unsigned)blocks, (unsigned)n_images), dim3(256), 0, stream, planes, elems, stride, sums);
}

// ---------------------------------------------------------------------------------------------
static inline dim3 grid1d(int64_t n, int block, int z, int y = 1) {
    int64_t g = (n + block - 1) / block;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return dim3((unsigned)g, (unsigned)y, (unsigned)z);
}

// ---------------------------------------------------------------------------------------------
// int16 coefficient samples -> int32 for the coded planes the inverse kernels want as int32 (Plan::widen: the few planes that are not
// squeeze residuals or freshly dequantised DCT coefficients); streaming, HBM bound (6 bytes per sample).
// one launch for the planes of Plan::widen: blockIdx.y = plane, blockIdx.z = image
__global__ __launch_bounds__(256) void k_widen_planes(const coef_t *src, int32_t *dst, int64_t stride, const int64_t *pairs) {
    const int64_t off = pairs[2 * blockIdx.y], n = pairs[2 * blockIdx.y + 1];
    const coef_t *s = src + (int64_t)blockIdx.z * stride + off;
    int32_t *d = dst + (int64_t)blockIdx.z * stride + off;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) d[i] = s[i];
}
void launch_widen_planes(const coef_t *src, int32_t *dst, int64_t stride, const int64_t *dev_pairs, int n_planes, int64_t max_elems, int n_images, hipStream_t stream) {
    if (n_planes <= 0 || n_images <= 0) return;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((max_elems + 1023) / 1024, 512));
    hipLaunchKernelGGL(k_widen_planes, dim3((unsigned)blocks, (unsigned)n_planes, (unsigned)n_images), dim3(256), 0, stream, src, dst, stride, dev_pairs);
}

void launch_op(const Op &op, const Bases &b, const PlaneRef *dev_list, ChannelMeta *meta, int n_channels, int img_first,
               int n_images, hipStream_t stream, int32_t *status) {
    switch (op.kind) {
        case OP_VSQUEEZE: {
            const int w = op.src[0].w;
            if (w <= 0 || op.dst[0].h <= 0) break;
            if (op.r16) hipLaunchKernelGGL(k_inv_vsqueeze<coef_t>, dim3((w + 255) / 256, 1, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.dst[0], op.clamp_out, op.lo, op.hi);
            else hipLaunchKernelGGL(k_inv_vsqueeze<int32_t>, dim3((w + 255) / 256, 1, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.dst[0], op.clamp_out, op.lo, op.hi);
            break;
        }
        case OP_HSQUEEZE: {
            const int h = op.src[0].h;
            if (h <= 0 || op.dst[0].w <= 0) break;
            static const int tiles = [] { const char *e = getenv("FUIFGPU_HSQUEEZE_TILES"); return e ? atoi(e) : 1; }();   // 0: the lane-per-row kernel for every width (A/B measurements)
            if (tiles && op.src[1].w >= 2 * HL_P) {
                if (op.r16) hipLaunchKernelGGL(k_inv_hsqueeze_tiles<coef_t>, dim3((h + 63) / 64, 1, n_images), dim3(64), 0, stream, b, op.src[0], op.src[1], op.dst[0], op.clamp_out, op.lo, op.hi);
                else hipLaunchKernelGGL(k_inv_hsqueeze_tiles<int32_t>, dim3((h + 63) / 64, 1, n_images), dim3(64), 0, stream, b, op.src[0], op.src[1], op.dst[0], op.clamp_out, op.lo, op.hi);
            } else {
                if (op.r16) hipLaunchKernelGGL(k_inv_hsqueeze_rows<coef_t>, dim3((h + 255) / 256, 1, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.dst[0], op.clamp_out, op.lo, op.hi);
                else hipLaunchKernelGGL(k_inv_hsqueeze_rows<int32_t>, dim3((h + 255) / 256, 1, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.dst[0], op.clamp_out, op.lo, op.hi);
            }
            break;
        }
        case OP_HSQ2_YCOCG: {
            const int h = op.src[0].h;
            if (h <= 0 || op.p0 <= 0) break;
            if (op.r16) hipLaunchKernelGGL(k_inv_hsq2_ycocg<coef_t>, dim3((h + 63) / 64, 1, n_images), dim3(64), 0, stream, b, op.src[0], op.src[1], op.src[2], op.ext[0], op.dst[0], op.dst[1], op.dst[2], op.hi);
            else hipLaunchKernelGGL(k_inv_hsq2_ycocg<int32_t>, dim3((h + 63) / 64, 1, n_images), dim3(64), 0, stream, b, op.src[0], op.src[1], op.src[2], op.ext[0], op.dst[0], op.dst[1], op.dst[2], op.hi);
            break;
        }
        case OP_YCOCG:
            hipLaunchKernelGGL(k_inv_ycocg, dim3((op.p0 + 255) / 256, op.p1, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.src[2],
                               op.p0, op.p1, op.hi);
            break;
        case OP_YCBCR:
            hipLaunchKernelGGL(k_inv_ycbcr, dim3((op.p0 + 255) / 256, op.p1, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.src[2],
                               op.p0, op.p1, op.lo, op.hi);
            break;
        case OP_QUANT: {
            // grid.y = plane of the op's list; 64 grid-striding blocks per plane
            if (op.r16) hipLaunchKernelGGL(k_dequant<coef_t>, dim3(64, op.pad, n_images), dim3(256), 0, stream, b, dev_list + op.idct_first, meta, n_channels, img_first);
            else hipLaunchKernelGGL(k_dequant<int32_t>, dim3(64, op.pad, n_images), dim3(256), 0, stream, b, dev_list + op.idct_first, meta, n_channels, img_first);
            break;
        }
        case OP_IDCT:
            if (op.pad2 && meta) hipLaunchKernelGGL(k_idct8x8<true>, dim3((op.p0 + 63) / 64, op.p1, n_images), dim3(64), 0, stream, b, dev_list + op.idct_first, op.dst[0],
                                                    op.p0, op.p1, op.hi, op.clamp_out, op.lo, op.hi, meta, n_channels, img_first);
            else hipLaunchKernelGGL(k_idct8x8<false>, dim3((op.p0 + 63) / 64, op.p1, n_images), dim3(64), 0, stream, b, dev_list + op.idct_first, op.dst[0],
                                    op.p0, op.p1, op.hi, op.clamp_out, op.lo, op.hi, meta, n_channels, img_first);
            break;
        case OP_UPS2_YCBCR:
            if (op.src[1].w <= 0 || op.src[1].h <= 0) break;
            hipLaunchKernelGGL(k_ups2_ycbcr, dim3((op.src[1].w + 255) / 256, op.src[1].h, n_images), dim3(256), 0, stream, b, op.src[0], op.src[1], op.src[2],
                               op.dst[0], op.dst[1], op.dst[2], op.p0, op.p1, op.lo, op.hi);
            break;
        case OP_UPSAMPLE:
            if (op.p0 == 2 && op.p1 == 2)
                hipLaunchKernelGGL(k_upsample_2x2, dim3((op.src[0].w + 255) / 256, op.src[0].h, n_images), dim3(256), 0, stream, b, op.src[0], op.dst[0],
                                   op.clamp_out, op.lo, op.hi);
            else
                hipLaunchKernelGGL(k_upsample, dim3((op.dst[0].w + 255) / 256, op.dst[0].h, n_images), dim3(256), 0, stream, b, op.src[0], op.dst[0],
                                   op.p0, op.p1, op.clamp_out, op.lo, op.hi);
            break;
        case OP_COPY_CLAMP:
        case OP_CLAMP: {
            // a copy without the fused final clamp (a coded plane that is a final plane of a kept-transform schedule, image.cpp:107): the whole int32 range passes
            const bool plain = op.kind == OP_COPY_CLAMP && !op.clamp_out;
            hipLaunchKernelGGL(k_clamp, grid1d((int64_t)op.dst[0].w * op.dst[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[0], op.dst[0],
                               plain ? INT32_MIN : op.lo, plain ? INT32_MAX : op.hi);
            break;
        }
        case OP_PALETTE:
            if ((int64_t)op.dst[0].w * op.dst[0].h <= 0) break;
            hipLaunchKernelGGL(k_inv_palette, grid1d((int64_t)op.dst[0].w * op.dst[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[0],
                               op.src[1], op.dst[0], op.p0, op.p1, op.clamp_out, op.lo, op.hi);
            break;
        case OP_PERMUTE:
            if ((int64_t)op.dst[0].w * op.dst[0].h <= 0 || op.pad < 1) break;
            hipLaunchKernelGGL(k_permute_plane, grid1d((int64_t)op.dst[0].w * op.dst[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[0],
                               dev_list + op.idct_first, op.pad, op.p0, op.dst[0], op.clamp_out, op.lo, op.hi, status, img_first);
            break;
        case OP_MATCH:
            if (!meta || op.src[0].w <= 0) break;
            hipLaunchKernelGGL(k_inv_match_frames, dim3((op.src[0].w + 255) / 256, 1, n_images), dim3(256), 0, stream, b, op.src[0],
                               dev_list + op.idct_first, op.pad, op.p0, op.p1, meta, n_channels, img_first, status);
            break;
        case OP_MATCH_INIT:
            if (!meta || (int64_t)op.dst[0].w * op.dst[0].h <= 0) break;
            hipLaunchKernelGGL(k_match_init, grid1d((int64_t)op.dst[0].w * op.dst[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[0], op.dst[0],
                               op.p0, dev_list + op.idct_first, op.pad / 3, meta, n_channels, img_first, status);
            break;
        case OP_MATCH_JUMP:
            if (!meta || (int64_t)op.dst[0].w * op.dst[0].h <= 0) break;
            hipLaunchKernelGGL(k_match_jump, grid1d((int64_t)op.dst[0].w * op.dst[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[1], op.src[0],
                               op.dst[0], op.p0, dev_list + op.idct_first, op.pad / 3, op.p1, meta, n_channels, img_first);
            break;
        case OP_MATCH_APPLY:
            if (!meta || (int64_t)op.src[0].w * op.src[0].h <= 0) break;
            hipLaunchKernelGGL(k_match_apply, grid1d((int64_t)op.src[0].w * op.src[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[1], op.src[0],
                               op.p0, dev_list + op.idct_first, op.p0 ? op.pad / 3 : op.pad, op.p1, meta, n_channels, img_first, status);
            break;
        case OP_APPROX:
            if ((!meta && (op.src[0].qsrc >= 0 || op.src[1].qsrc >= 0)) || (int64_t)op.dst[0].w * op.dst[0].h <= 0) break;   // raw planes carry no ChannelMeta
            hipLaunchKernelGGL(k_inv_approx, grid1d((int64_t)op.dst[0].w * op.dst[0].h, 256, n_images), dim3(256), 0, stream, b, op.src[0],
                               op.src[1], op.p0, op.p1, meta, n_channels, img_first);
            break;
        default:
            break;
    }
}

}  // namespace fuifgpu
