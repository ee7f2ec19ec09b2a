// fuif_amd/csrc/transforms.h -- launch interface of the inverse-transform kernels
#pragma once
#include <hip/hip_runtime.h>

#include "fuifgpu_internal.h"

namespace fuifgpu {

// per-launch slab bases: address = base[buf] + z*stride[buf] + plane offset (z = image inside the chunk)
struct Bases {
    int32_t *base[3];
    int64_t stride[3];
    const coef_t *c16;      // the chunk's coefficient slab as the entropy kernel wrote it (int16 samples; same plane offsets and image stride
                            // as base[BUF_COEF]): what the squeeze kernels read their residuals from when Op::r16 is set; may be NULL otherwise
};

void launch_op(const Op &op, const Bases &b, const PlaneRef *dev_list, ChannelMeta *meta, int n_channels, int img_first,
               int n_images, hipStream_t stream, int32_t *status = nullptr);   // status: per-image FUIFGPU_ST_* words (optional)

// coefficient samples as the entropy kernel stores them (int16, fuifgpu_internal.h) -> the int32 planes the inverse kernels work on:
// the planes of Plan::widen ({element offset, elements} pairs, device array) of n_images images: src / dst advance by `stride` elements per image
void launch_widen_planes(const coef_t *src, int32_t *dst, int64_t stride, const int64_t *dev_pairs, int n_planes, int64_t max_elems, int n_images, hipStream_t stream);

// interleaved 8/16-bit samples of up to 5 final planes (export/write_pam.h:136-150)
struct PackedPlanes {
    int32_t n;
    PlaneRef p[5];
};
void launch_pack(const Bases &b, const PackedPlanes &pp, int w, int h, int lo, int hi, int bytes_per_sample, uint8_t *dst, int64_t dst_stride,
                 int n_images, hipStream_t stream);

// per-image position-weighted 64-bit sums of n_images runs of `elems` int32 samples, `stride` samples apart (sums[] is zeroed on the stream first)
void launch_plane_checksums(const int32_t *planes, int64_t elems, int64_t stride, int n_images, unsigned long long *sums, hipStream_t stream);

// forward YCoCg (in place, three contiguous planes of n samples) and forward Squeeze of one plane (transform/ycocg.h:65-95,
// transform/squeeze.h:135-170,227-263): raw device pointers, the writer's optional GPU path
void launch_scale(int32_t *plane, int64_t n, int q, hipStream_t stream);   // transform/quantize.h:32-49 on one plane
void launch_fwd_ycocg(int32_t *c0, int32_t *c1, int32_t *c2, int64_t n, hipStream_t stream);
void launch_fwd_squeeze(bool horizontal, const int32_t *in, int w, int h, int32_t *avg, int32_t *res, hipStream_t stream);
// forward Quantize (transform/quantize.h:54-71) with the range of the quotients: one plane, or every channel of a device table in one launch
// (entry k owns blocks [first_block, first_block + n_blocks) of the grid, n_blocks = fwd_quantize_blocks(n), total_blocks their sum).
// dev_minmax: {min, max} pairs the caller has initialised; NULL (one plane) = no range wanted
int fwd_quantize_blocks(int64_t n_samples);
void launch_fwd_quantize_plane(int32_t *plane, int64_t n, int q, int32_t *dev_minmax, hipStream_t stream);
void launch_fwd_quantize(const QuantChan *dev_table, int n_channels, int total_blocks, int32_t *dev_minmax, hipStream_t stream);
// {min, max, zero samples} of read-only planes, accumulated into caller-initialised triples: every record of a device table in one launch
// (record k owns blocks [first_block, first_block + n_blocks), n_blocks = channel_stats_blocks(n), into dev_stats + 3k), or dev_table == NULL: the one
// record `one` (first_block 0) into dev_stats
int channel_stats_blocks(int64_t n_samples);
void launch_channel_stats(const StatsRec *dev_table, int n_recs, StatsRec one, int total_blocks, int32_t *dev_stats, hipStream_t stream);
// raw YUV 4:2:0 frames -> tight int32 planes (import/read_yuv.h:29-63): every frame of every job of a device table in one launch, or
// dev_table == NULL: the one job `one`.  dev_flag (may be NULL): a word that gets a bit set if a sample exceeds g.maxval
void launch_unpack_yuv420(const YuvJob *dev_table, int n_jobs, YuvJob one, const YuvGeom &g, int32_t *dev_flag, hipStream_t stream);
// int32 Y, Cb, Cr planes -> raw YUV 4:2:0 frames, clamped to [0, g.maxval] (export/write_yuv.h:29-58): the g.nb_frames frames of each of
// n_pictures pictures in one launch; picture k's planes and frames lie k * job.image_stride samples / k * job.dst_stride bytes behind picture 0's
void launch_pack_yuv420(const YuvPackJob &job, int n_pictures, const YuvGeom &g, hipStream_t stream);
// forward Palette (transform/palette.h:92-142).  Several channels: the distinct tuples of nb planes into an open-addressing table of
// `capacity` (a power of two > 2 * limit) zero-initialised 64-bit keys; dev_ctl: four zero-initialised words {distinct colours, too many,
// the all-zero key occurs, a sample outside int16}.  Then every sample's colour number from the table and the ranks of its slots.
// One channel: a zero-initialised presence bitmap of 2048 words over the int16 range, then prefix[w] + the set bits below the sample's own
struct PalettePlanes {
    const int32_t *p[4];
    int32_t nb;
};
void launch_palette_collect(const PalettePlanes &pp, int64_t n, unsigned long long *dev_keys, uint32_t capacity, uint32_t limit, uint32_t *dev_ctl, hipStream_t stream);
void launch_palette_index(const PalettePlanes &pp, int64_t n, const unsigned long long *dev_keys, const int32_t *dev_rank, uint32_t capacity, int32_t zero_rank,
                          int32_t *index, hipStream_t stream);
void launch_palette_collect1(const int32_t *plane, int64_t n, uint32_t *dev_bitmap, uint32_t *dev_ctl, hipStream_t stream);
void launch_palette_index1(const int32_t *plane, int64_t n, const uint32_t *dev_bitmap, const int32_t *dev_prefix, int32_t *index, hipStream_t stream);
// forward Matching against the previous frame (transform/2dmatch.h:303-381 with maxdist = -1) of a strip of frames fh rows high: the
// match channel (w x h, every sample written) from the planes, the erode, then the matched samples of every plane set to zero in place.
// Three launches; picture z of n_pictures has its planes and its match channel z * pic_stride samples behind picture 0's
struct MatchPlanes {
    int32_t *p[8];
    int32_t nb;
};
void launch_fwd_match_frames(const MatchPlanes &mp, int w, int h, int fh, int n_pictures, int64_t pic_stride, int32_t *match, hipStream_t stream);

}  // namespace fuifgpu
