/* include/fuifgpu.h -- C-ABI of libfuifgpu.so: the MI355X (gfx950) FUIF decode path.
 *
 * This is the drop-in boundary for the ONE hot path of cloudinary/fuif: channel-group entropy
 * decode followed by the inverse transform chain.  Each entry point names the reference
 * interface it replaces (paths relative to the reference tree).  Plain pointers and sizes only;
 * no C++ or torch types cross this boundary.  See INTEGRATION.md for the reference-side binding.
 *
 * Threading: a fuifgpu_batch is owned by one host thread at a time.  All device work is enqueued
 * on the hipStream_t passed as `void *stream` (NULL = the default stream).
 */
#ifndef FUIFGPU_H
#define FUIFGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FUIFGPU_ABI_VERSION 3   /* 2: fuifgpu_encode_options starts with struct_size; sibling batches freeze the launch resources.
                                 * 3: every fuifgpu_batch_* call runs on the batch's own device (the caller's is restored on return);
                                 *   the device / peer-copy / checksum / in-flight entry points exist; fuifgpu_batch_create reads FUIFGPU_IN_FLIGHT.
                                 *   A host checks fuifgpu_abi_version() >= the version whose entry points it binds before looking them up. */

/* error codes (0 = success).  The reference reports these conditions as `return false` +
 * e_printf (encoding/encoding.cpp:601-605, 276-279, 697-700). */
#define FUIFGPU_OK 0
#define FUIFGPU_E_NOT_FUIF 1      /* bad magic / short header */
#define FUIFGPU_E_CORRUPT 2       /* header or transform list is inconsistent */
#define FUIFGPU_E_UNSUPPORTED 3   /* feature outside the hot-path scope (`-E k` > 50: more than 25 reference channels per context tree, the CLI default is 12; a data-driven Permute over channels of unequal geometry) */
#define FUIFGPU_E_ARG 4
#define FUIFGPU_E_HIP 5           /* a HIP runtime call failed; see fuifgpu_last_error() */
#define FUIFGPU_E_MISMATCH 6      /* image does not share the batch's plan signature */
#define FUIFGPU_E_NOMEM 7

/* per-image status bits written by the entropy kernel (fuifgpu_batch_status) */
#define FUIFGPU_ST_TRUNCATED 1    /* EOF or preview limit reached: remaining samples are zero-filled
                                     (not an error, encoding/encoding.cpp:209-219) */
#define FUIFGPU_ST_CORRUPT 2      /* the reference would return false */
#define FUIFGPU_ST_UNSUPPORTED 4
#define FUIFGPU_ST_STALLED 8 /* internal error: a group gave up waiting for rows of another group (always with CORRUPT) */

typedef struct fuifgpu_plan fuifgpu_plan;    /* host: parsed header + channel table + inverse schedule */
typedef struct fuifgpu_batch fuifgpu_batch;  /* device: buffers and state for N same-geometry images */

/* replaces the header half of fuif_decode<IO>() (encoding/encoding.cpp:599-702): what
 * `Image(w,h,maxval,nb_channels)` + every Transform::meta_apply() (transform/transform.cpp:66-81)
 * compute, without touching pixel data. */
typedef struct {
    int32_t w, h, bit_depth, maxval, nb_channels, colormodel, max_properties, nb_frames;
    int32_t nb_transforms, nb_coded_channels, nb_output_channels, nb_ops;
    int32_t responsive_offsets[5];
    int32_t data_start;
    int64_t coef_elems, out_elems, tmp_elems; /* elements per image: int16 samples in the coefficient slab (a coded sample is the
                                                 reference's pixel_type, image/image.h:35), int32 in the output and scratch slabs */
    uint64_t signature;
} fuifgpu_image_info;

/* mirrors the geometry fields of `class Channel` (image/image.h:54-91) */
typedef struct {
    int32_t w, h, hshift, vshift, hcshift, vcshift, component, reserved;
    int64_t offset; /* element offset inside the per-image coefficient (coded) or output slab */
} fuifgpu_channel_desc;

const char *fuifgpu_strerror(int code);
const char *fuifgpu_last_error(void);
int fuifgpu_abi_version(void);

/* ---- host side: header parse + planning (no GPU needed) ------------------------------------ */
int fuifgpu_plan_create(const uint8_t *blob, size_t size, fuifgpu_plan **out);
/* A plan whose inverse schedule stops with `keep` transforms left standing: Image::undo_transforms(keep) (image/image.cpp:94-115),
 * what `fuif -d x.fuif out.yuv` runs with keep = 2 (fuif.cpp:229-231).  0 <= keep <= nb_transforms, else FUIFGPU_E_ARG; keep = 0 is
 * fuifgpu_plan_create.  With keep != 0 there is no final clamp (image.cpp:107), the output channels are the channel list the reference
 * has at that point -- remaining meta-channels first, zero-size channels included, every channel with its own size and shifts -- and
 * nb_ops, out_elems, tmp_elems, nb_output_channels describe the shortened schedule; the signature differs from the keep = 0 plan's.  A batch
 * made from such a plan (a sibling: its primary's) plans every uploaded stream with the same keep; fuifgpu_batch_undo_transforms,
 * _undo_transforms_to, _download_out, _out_ptr and fuifgpu_plane_checksums work on it unchanged, fuifgpu_batch_pack_out keeps its rule
 * (a channel smaller than w x h is FUIFGPU_E_ARG).  Both entry points are found by symbol lookup: the ABI version does not change. */
int fuifgpu_plan_create_keep(const uint8_t *blob, size_t size, int keep, fuifgpu_plan **out);
int fuifgpu_plan_keep(const fuifgpu_plan *plan, int *keep);
void fuifgpu_plan_destroy(fuifgpu_plan *plan);
int fuifgpu_plan_info(const fuifgpu_plan *plan, fuifgpu_image_info *info);
int fuifgpu_plan_coded_channel(const fuifgpu_plan *plan, int index, fuifgpu_channel_desc *desc);
int fuifgpu_plan_output_channel(const fuifgpu_plan *plan, int index, fuifgpu_channel_desc *desc);
/* transform list as stored in Image::transform after meta_apply (encoding.cpp:673-693);
 * params_out receives at most cap ints, *nparams the real count */
int fuifgpu_plan_transform(const fuifgpu_plan *plan, int index, int32_t *id, int32_t *params_out, int cap, int32_t *nparams);
/* maniac/chance.cpp:31-65 build_table(), table[2*chance+bit]; host helper used by tests */
void fuifgpu_build_chance_table(uint16_t *table8192, uint32_t alpha, int cut);

/* ---- device side --------------------------------------------------------------------------- */
/* Creates device state for `n_images` streams that all share `plan`'s signature.
 * coef_ext / out_ext: optional caller-owned device slabs of n_images*coef_elems /
 * n_images*out_elems int32 (e.g. a torch tensor's data_ptr); NULL = allocated by the library.
 * tmp_images: number of images whose inverse-transform scratch is resident at once (0 = default). */
int fuifgpu_batch_create(const fuifgpu_plan *plan, int n_images, size_t blob_capacity_bytes,
                         int16_t *coef_ext, int32_t *out_ext, int tmp_images, fuifgpu_batch **out);
void fuifgpu_batch_destroy(fuifgpu_batch *batch);

/* A batch WITHOUT an output slab, for batches whose outputs do not fit next to their coefficients (BASELINE config C4: 256 x
 * 8192x8192x4 -- 137 GB of int16 coefficients, 275 GB of int32 outputs): every image is entropy-decoded in ONE launch, then the
 * inverse transforms run range by range into caller memory (fuifgpu_batch_undo_transforms_to) and the caller consumes each
 * slice before the next.  fuifgpu_batch_undo_transforms, _out_ptr, _download_out and _pack_out are refused on such a batch.
 * The reference has no counterpart: it decodes one image at a time (fuif.cpp:213-233). */
int fuifgpu_batch_create_streaming(const fuifgpu_plan *plan, int n_images, size_t blob_capacity_bytes, int tmp_images, fuifgpu_batch **out);
/* Image::undo_transforms(0) -- undo_transforms(keep) for a plan made with fuifgpu_plan_create_keep, with its smaller out_elems -- for
 * images [first_image, first_image + n_images) of the current decode; their output planes go to
 * out_device (n_images * out_elems int32, device memory; plan output-channel offsets apply inside each image's slice).  Any
 * batch takes it; every image once per decode (a range that repeats an image, or a mix with fuifgpu_batch_undo_transforms, is
 * FUIFGPU_E_ARG).  A range counts as done once the call has queued it; after a failed call (a HIP error) decode again before
 * retrying.  fuifgpu_batch_last_timing's transform_ms is the time of the LAST call's range, not of all ranges of a decode. */
int fuifgpu_batch_undo_transforms_to(fuifgpu_batch *batch, int first_image, int n_images, int32_t *out_device, void *stream);

/* A second set of stream buffers for the SAME slabs, so that the upload of the next batch (host parse + H2D copies, on a copy
 * stream, from another host thread) runs while the previous batch decodes: the sibling owns what fuifgpu_batch_upload writes
 * (stream bytes, tile lists, per-image status / consumed / metadata) and launches with the primary's coefficient and output
 * slabs, decoder scratch, context arenas and transform arena -- ~12 MB per 4K stream instead of a second 45 GB of launch state.
 * Creating the first sibling sizes the primary's decoder scratch and context arenas for the worst case (the device's wavefront
 * capacity, a full batch) and they never move again while a sibling exists, so an upload into one batch on another host thread
 * cannot pull them from under a decode of the other; either batch may be loaded first, with any number of images <= n_images.
 * Rules: decode / undo_transforms of the
 * two on ONE stream (they share the slabs); destroy the sibling first (a sibling that outlives its primary refuses every call).  The pattern, per step k: thread U uploads into batch
 * (k+1)%2 on the copy stream while the caller runs decode + undo_transforms of batch k%2; join; consume; repeat
 * (bench.py's `value_incl_h2d`, tests/test_gpu_synthetic.py).  The reference has no counterpart: it reads one file at a time
 * (encoding/encoding.cpp:745-753). */
int fuifgpu_batch_create_sibling(fuifgpu_batch *primary, size_t blob_capacity_bytes, fuifgpu_batch **out);

/* Stage compressed streams (host pointers) into HBM.  Every blob must parse to the batch's
 * signature.  preview: -1 = full decode, 0..4 = responsive truncation point
 * (fuif_options::preview, encoding/encoding.h:34).  Replaces the IO object handed to
 * fuif_decode<IO>() (fileio.h:33-143). */
int fuifgpu_batch_upload(fuifgpu_batch *batch, const uint8_t *const *blobs, const size_t *sizes,
                         int n_images, int preview, void *stream);

/* replaces the channel loop of fuif_decode (encoding/encoding.cpp:708-717) and
 * fuif_decode_channel (encoding/encoding.cpp:259-429) for every stream of the batch:
 * fills the coefficient slab and the per-channel {minval,maxval,q}. */
int fuifgpu_batch_decode(fuifgpu_batch *batch, void *stream);

/* replaces Image::undo_transforms(0) (image/image.cpp:94-115) for every image of the batch:
 * inverse Squeeze / Quantize / DCT / ChromaSubsample / YCoCg / YCbCr + final clamp into the
 * output slab.  A plan made with fuifgpu_plan_create_keep: undo_transforms(keep), which stops with `keep`
 * transforms left and makes no final clamp. */
int fuifgpu_batch_undo_transforms(fuifgpu_batch *batch, void *stream);
/* (once per decode: the inverse of Approximate rewrites the per-channel metadata, so a second call is refused with FUIFGPU_E_ARG
 * until the batch is decoded again.  The coefficient slab itself is not touched -- the kernels work on a widened copy of a chunk
 * of images -- and fuifgpu_batch_download_coef stays legal after it.) */

int fuifgpu_batch_sync(fuifgpu_batch *batch, void *stream);
/* status[n_images] (FUIFGPU_ST_* bits), bytes_consumed[n_images] (io.ftell() at the end) */
int fuifgpu_batch_status(fuifgpu_batch *batch, int32_t *status, uint32_t *bytes_consumed);
/* {minval,maxval,q,decoded} of every coded channel of one image (Channel::minval/maxval/q) */
int fuifgpu_batch_channel_meta(fuifgpu_batch *batch, int image, int32_t *meta4_per_channel);
int16_t *fuifgpu_batch_coef_ptr(fuifgpu_batch *batch, int image);   /* device pointer: int16 samples (ABI 2; fuifgpu_batch_download_coef hands them out as int32) */
int32_t *fuifgpu_batch_out_ptr(fuifgpu_batch *batch, int image);    /* device pointer */
int fuifgpu_batch_download_coef(fuifgpu_batch *batch, int image, int32_t *host, void *stream);
int fuifgpu_batch_download_out(fuifgpu_batch *batch, int image, int32_t *host, void *stream);
/* ---- packed output: what export/write_pam.h:136-150 puts in a PNM/PAM file ---------------------------------
 * For every pixel of the w x h image the first `components` output channels (0 = all, at most 4), clamped to
 * [0,maxval], 1 byte per sample when maxval < 256 else 2 bytes big-endian, interleaved.  The packing runs on
 * the GPU after fuifgpu_batch_undo_transforms; a host that only wants the picture pulls 1/4 (16-bit) or 1/8
 * (8-bit) of the bytes of the int32 planes over PCIe. */
size_t fuifgpu_plan_packed_bytes(const fuifgpu_plan *plan, int components);                 /* bytes per image */
/* n_images images starting at first_image into a DEVICE buffer of n_images * packed_bytes */
int fuifgpu_batch_pack_out(fuifgpu_batch *batch, int first_image, int n_images, int components, uint8_t *dst_device, void *stream);
/* one image into HOST memory (packs into a temporary device buffer, copies, synchronises the stream) */
int fuifgpu_batch_download_packed(fuifgpu_batch *batch, int image, int components, uint8_t *host, void *stream);

/* Verification aid -- no counterpart in the reference (its tests compare files with `cmp`): sums_device[k] = sum over the
 * elems_per_image int32 samples of image k (image_stride samples apart, a multiple of 4; planes_device 16-byte aligned) of
 * sample * (index mod 65521 + 1), as a wrapping 64-bit integer; asynchronous on `stream`.  A host that decodes step after step into
 * the same planes (bench.py's overlapped steps, fuifgpu_batch_undo_transforms_to slice by slice) keeps 8 bytes per image and step
 * and compares them when the steps are done, instead of holding or downloading the planes of every step. */
int fuifgpu_plane_checksums(const int32_t *planes_device, int64_t elems_per_image, int64_t image_stride, int n_images, uint64_t *sums_device, void *stream);

/* kernel time of the last decode / undo_transforms launch set, measured with hipEvents on the
 * caller's stream (ms); used by bench.py for the roofline */
int fuifgpu_batch_last_timing(fuifgpu_batch *batch, float *decode_ms, float *transform_ms);
/* diagnostic builds (-DFUIF_PROF) only: 8 counters per stream of the last decode, shader cycles
 * {vector phase, property patch, tree walk, leaf switch, symbol decode, per-pixel rest (incl. the row store),
 * 100 MHz ticks of the run segments, shader cycles of the run segments}; all zero in release builds
 * (-DFUIF_PROF_BY_CHANNEL: one row per first channel of a tile, summed over the images, instead of one per stream) */
int fuifgpu_batch_profile(fuifgpu_batch *batch, uint64_t *out8_per_image);
/* diagnostic builds (-DFUIF_STATS or -DFUIF_PROF; FUIFGPU_E_UNSUPPORTED from the release library, whose kernel carries no
 * statistics): the schedule of the last decode launch, 4 words per tile of the work list {image << 32 | first channel,
 * first start, end, ticks some wavefront was running the tile | CU key << 48}, times in 100 MHz s_memrealtime ticks.
 * Logging starts with the first call (which returns *n_tiles = 0); tools/tile_timeline.py turns it into a report. */
int fuifgpu_batch_tile_log(fuifgpu_batch *batch, uint64_t *out4_per_tile, int cap, int *n_tiles);
/* diagnostic: counters of the tile scheduler for the last dense launch {ticks (100 MHz) wavefronts spent without work while
 * tiles were unfinished, tiles picked up (starts + resumptions), suspensions, ticks spent looking for the tile picked up, ticks spent spinning inside tiles (waits a tile could not be
 * suspended for), suspendable tiles that found their context arena full, ticks between picking a tile up and looking for
 * the next one, ticks the wavefronts lived} */
int fuifgpu_batch_sched_stats(fuifgpu_batch *batch, uint64_t *out8);

/* ---- group index (csrc/index.cpp) --------------------------------------
 * A FUIF stream is a chain of channel groups (fuif_decode_channel, encoding/encoding.cpp:259-429),
 * each with its own range coder, whose byte boundaries the encoder knows (encoding.cpp:525-527,542)
 * but does not store.  The index stores them in a trailer BEHIND the stream
 *     <stream> <payload> <u32 LE payload length> "FGIX"
 *     payload = varint 1 ; varint n ; n x { varint channel delta ; varint byte-offset delta }
 * which the reference decoder never reads (it stops after the last group, encoding.cpp:708-717):
 * indexed files still decode with the unmodified reference.  fuifgpu_batch_upload() finds the
 * trailer by itself, ends the stream where the trailer begins and then decodes every group of every image on its own wavefront; streams
 * without one are decoded one wavefront per image.  Ways to get an index: the writer below
 * (emit_index), or decode once and keep fuifgpu_batch_group_index()'s result with the asset. */
/* groups of the trailer of `blob` (n_groups = 0: none / not valid for this stream) */
int fuifgpu_index_parse(const uint8_t *blob, size_t size, int32_t *first_channel, uint32_t *start, int cap, int *n_groups);
/* copy of the stream with a trailer for the given groups (replaces an existing one); free with fuifgpu_free_blob */
int fuifgpu_index_append(const uint8_t *blob, size_t size, const int32_t *first_channel, const uint32_t *start, int n_groups,
                         uint8_t **blob_out, size_t *size_out);
/* after a decode: the groups the entropy kernel went through for one image (any stream, indexed or not) */
int fuifgpu_batch_group_index(fuifgpu_batch *batch, int image, int32_t *first_channel, uint32_t *start, int cap, int *n_groups);
/* enable = 0: ignore trailers from the next upload on (A/B measurements; default 1) */
int fuifgpu_batch_set_group_parallel(fuifgpu_batch *batch, int enable);
/* How many batches the host keeps in flight on this device (default 1); applies from the next upload on.  It only matters for launches with few tiles
 * (streams without group index: one wavefront per picture).  1: such a launch runs with 58 supernodes of every context tree in LDS, one wavefront per
 * SIMD -- the fastest a launch ALONE can be (20.8 s for 1024 x 4K).  2 or more: 20 supernodes, two wavefronts per SIMD -- 6 % slower alone, but the
 * launch of a second batch on a second stream runs beside it: 24.5 s for two such launches instead of 41.6 s (profiles/r5_overlap_timeline_and_wide_variants.txt).
 * The reference decodes one file at a time (fuif.cpp:213-233); no counterpart. */
int fuifgpu_batch_set_in_flight(fuifgpu_batch *batch, int n_batches);

/* ---- several GPUs of one node -----------------------------------------------------------------------------
 * The reference decodes file after file on one core (fuif.cpp:213-233: fuif_decode_file + undo_transforms per file); a batch of
 * independent images shards across the GPUs of a node with no data-path exchange.  Inside ONE process the unit is
 * the calling thread's current device, as in HIP: fuifgpu_set_device() selects it, a batch lives on the device that was current when
 * it was created, and every fuifgpu_batch_* call runs on the batch's own device whatever the calling thread's current device is (it
 * is restored on return) -- so a host runs one thread per device (fuif_decode_files in fuif_amd/boundary does) or one thread over
 * the batches of several devices.  A `stream` handed to a fuifgpu_batch_* call must be a stream OF THE BATCH'S DEVICE (NULL = that
 * device's null stream); the library does not check it, and HIP reports a foreign stream as an invalid handle at the first launch.
 * fuifgpu_dev_* and the single-transform entry points use the calling thread's current device.
 * Several PROCESSES (one per GPU, torch.distributed / RCCL: bench.py, fuif_amd/dist.py) each simply see their own device. */
int fuifgpu_device_count(int *n_devices);
int fuifgpu_set_device(int device);                                   /* FUIFGPU_E_ARG: no such device */
int fuifgpu_get_device(int *device);
int fuifgpu_batch_device(const fuifgpu_batch *batch, int *device);
/* The final gather's building block inside one process: `bytes` from src_device's memory into dst_device's over xGMI (peer access
 * is enabled on first use; without it the runtime stages the copy), asynchronous on `stream` (a stream of the calling thread's
 * current device; NULL = its null stream).  What a host uses to collect the packed pictures (fuifgpu_batch_pack_out) of every
 * GPU's shard on one GPU; the multi-process form of the same gather goes through RCCL (fuif_amd/dist.py gather_packed). */
int fuifgpu_peer_copy(void *dst_device_ptr, int dst_device, const void *src_device_ptr, int src_device, size_t bytes, void *stream);

/* ---- device memory for hosts that are not HIP programs (the boundary layer is plain g++ code) ------------- */
void *fuifgpu_dev_alloc(size_t bytes);                       /* NULL on failure (fuifgpu_last_error) */
void fuifgpu_dev_free(void *device_ptr);
int fuifgpu_dev_mem_info(size_t *free_bytes, size_t *total_bytes);   /* hipMemGetInfo: what a host sizes its batches with */
int fuifgpu_dev_upload(void *dst_device, const void *src_host, size_t bytes);
int fuifgpu_dev_download(void *dst_host, const void *src_device, size_t bytes);   /* waits for the null stream */

/* ---- single-transform entry points on raw device planes (row-major int32) ------------------
 * These are what Transform::apply(image, true) (transform/transform.cpp:48-63) dispatches to in the C++ boundary
 * layer (fuif_amd/boundary/fuif_gpu_boundary.cpp binds Transform::apply for the Squeeze, YCoCg, YCbCr, DCT, Quantize and
 * ChromaSubsample inverses to them: the path of Image::undo_transforms(keep != 0)); tests/test_gpu_transform_exports.py
 * checks each against the oracle.
 * Sample contract: the reference's samples are pixel_type = int16_t (image/image.h:35).  The planes here are int32 containers of
 * such samples: every input sample is an int16 value widened (what the binding copies out of a Channel), and the Squeeze, Quantize,
 * Approximate and soft 2D-match inverses store what the reference's assignment to pixel_type keeps -- the low 16 bits of the int
 * result, sign-extended (squeeze.h:103-107, quantize.h:41, approximate.h:53-55, 2dmatch.h:129,155) -- so every output is again an
 * int16 value widened.  Inputs outside that range are outside the contract. */
/* transform/squeeze.h:81-132 inv_hsqueeze: avg w1 x h + residual w2 x h -> out (w1+w2) x h */
int fuifgpu_inv_hsqueeze(const int32_t *avg, int w1, const int32_t *res, int w2, int h, int32_t *out, int n_planes,
                         int64_t avg_stride, int64_t res_stride, int64_t out_stride, void *stream);
/* transform/squeeze.h:173-224 inv_vsqueeze: avg w x h1 + residual w x h2 -> out w x (h1+h2) */
int fuifgpu_inv_vsqueeze(const int32_t *avg, int h1, const int32_t *res, int h2, int w, int32_t *out, int n_planes,
                         int64_t avg_stride, int64_t res_stride, int64_t out_stride, void *stream);
/* transform/ycocg.h:33-63 inv_YCoCg, in place on three planes with row pitches p0,p1,p2 */
int fuifgpu_inv_ycocg(int32_t *c0, int32_t *c1, int32_t *c2, int w, int h, int p0, int p1, int p2, int maxval, void *stream);
/* transform/ycbcr.h:33-63 inv_YCbCr */
int fuifgpu_inv_ycbcr(int32_t *c0, int32_t *c1, int32_t *c2, int w, int h, int p0, int p1, int p2, int minval, int maxval, void *stream);
/* transform/quantize.h:32-49 inv_quantize of one plane: every sample times the channel's quantisation constant, stored as int16, in place */
int fuifgpu_inv_quantize(int32_t *plane, int64_t n_samples, int q, void *stream);
/* transform/dct.h:88-107 + 282-291: 64 coefficient planes (bw x bh each, src[i] in the
 * reference's own zig-zag position order i=0..63) -> (8bw) x (8bh) samples; DC offset (maxval+1)*4 */
int fuifgpu_idct8x8(const int32_t *const *src64_dev, int bw, int bh, int32_t *out, int maxval, void *stream);
/* transform/subsample.h:90-126 chroma upsampling: the "fancy" filter for srh, srv in {1,2}, plain replication when either is larger (4:1:1) */
int fuifgpu_upsample(const int32_t *in, int w, int h, int srh, int srv, int32_t *out, void *stream);
/* transform/palette.h:57-64 inv_palette, one component per call: out[i] = palette_row[CLAMP(index[i], 0, colours-1)] over w x h samples
 * (palette_row = row `component` of the palette meta-channel; colours == 0 reads Channel::zero, image.h:82). out may not be index. */
int fuifgpu_inv_palette(const int32_t *index, int w, int h, const int32_t *palette_row, int colours, int32_t *out, void *stream);
/* transform/approximate.h:44-57 inv_approximate of one channel, in place: plane[i] = plane[i] * q + remainder[i] (q = parameter + 1), the product
 * and the sum each stored as int16;
 * remainder == NULL = "the remainder channel is not available" (:49,54): nothing is added */
int fuifgpu_inv_approximate(int32_t *plane, const int32_t *remainder, int64_t n_samples, int q, void *stream);
/* transform/2dmatch.h:112-177 inv_match, in place on n_planes (<= 64) w x h planes; match = the match meta-channel, match_q / match_maxval its
 * Channel::q and ::maxval (the mode is data: q == 1 free offsets :136-146, q == 2*fh*fh+(fh&1) previous frames :147-171, anything else
 * FUIFGPU_E_CORRUPT like :172-175). Synchronous. FUIFGPU_E_UNSUPPORTED (planes untouched) for a forward reference (an image narrower than the
 * offset spiral: the one case where the reference's scan order matters). */
int fuifgpu_inv_match(const int32_t *match, int w, int h, int32_t *const *planes, int n_planes, int softmatch, int match_q, int match_maxval,
                      int nb_frames, void *stream);
/* ---- forward transforms of the writer, raw device planes, contiguous rows ----
 * transform/ycocg.h:65-95 fwd_YCoCg, in place on three w x h planes */
int fuifgpu_fwd_ycocg(int32_t *c0, int32_t *c1, int32_t *c2, int w, int h, void *stream);
/* transform/squeeze.h:135-170 fwd_hsqueeze: in w x h -> avg ((w+1)/2) x h + residual (w/2) x h */
int fuifgpu_fwd_hsqueeze(const int32_t *in, int w, int h, int32_t *avg, int32_t *res, void *stream);
/* transform/squeeze.h:227-263 fwd_vsqueeze: in w x h -> avg w x ((h+1)/2) + residual w x (h/2) */
int fuifgpu_fwd_vsqueeze(const int32_t *in, int w, int h, int32_t *avg, int32_t *res, void *stream);
/* transform/quantize.h:54-71 fwd_quantize of one plane, in place: plane[i] = plane[i] / q, truncating toward zero (samples are int16 values
 * widened, as for the other forward entry points).  minmax_device != NULL: the minimum and the maximum of the quotients are accumulated
 * into minmax_device[0] and [1] (device memory, which the caller initialises, e.g. to INT32_MAX / INT32_MIN) -- the ranges
 * encoding/encoding.cpp:737-739 recomputes before a stream is written.  n_samples == 0 touches nothing.  q < 1: FUIFGPU_E_ARG; q == 1 leaves
 * the samples and still gives their range. */
int fuifgpu_fwd_quantize(int32_t *plane, int64_t n_samples, int q, int32_t *minmax_device, void *stream);

/* ---- stream writer (host C++; the input generator) --------------------
 * Writes a lossless FUIF stream the reference decoder accepts, with the format decisions of the
 * reference CLI for photographic PNM input (fuif.cpp:380-455,580-588; encoding/encoding.cpp:455-573).
 * tree_mode 0 = single-leaf MANIAC trees (byte-identical to `fuif -I 0`), 1 = trees learned by the
 * writer's own greedy learner, 2 = learned exactly as 1 with the learner's statistics (minimum, maximum, order statistics,
 * conditional histograms, the partition of the samples) computed by kernels, level by level for all learning groups of the call at
 * once; every floating-point decision stays in the host code of tree_mode 1, so the bytes are those of tree_mode 1 on every entry
 * point and option combination.  The batch entry points, fuifgpu_encode_animations and fuifgpu_encode_yuv420 honour 2 for all
 * channels (host-resident channels go to the device before the trees are learned instead of after; the samples never come to the
 * host); the single-picture entry points take it through the batch writer with one picture.  fuifgpu_encode_channels:
 * FUIFGPU_E_UNSUPPORTED.  No GPU: FUIFGPU_E_HIP (no silent host route).
 * *blob_out is malloc'd; release with fuifgpu_free_blob. */
typedef struct {
    uint32_t struct_size;   /* = sizeof(fuifgpu_encode_options) of the CALLER's header.  The library reads that many bytes and takes
                               every field behind them as 0, so the struct can grow at its end without breaking callers built
                               against an older header (ABI 2: an earlier build appended gpu_entropy to the unversioned struct, and a
                               caller built before that had 4 bytes read past its object).  0 or a size that is not a multiple of
                               4 is FUIFGPU_E_ARG. */
    int32_t ycocg;          /* 1: YCoCg when nch >= 3 (CLI default) */
    int32_t squeeze;        /* 1: default Squeeze (CLI default "responsive") */
    int32_t max_properties; /* CLI default 12 (-E) */
    int32_t tree_mode;      /* 0 none, 1 learned, 2 learned with the statistics on the GPU (same bytes as 1) */
    int32_t max_tree_nodes; /* cap for learned trees (<= 65535) */
    int32_t emit_index;     /* 1: append the group index trailer (see fuifgpu_index_*) */
    int32_t split_bits;     /* learned trees: > 0 = a split must save this many bits (flat); 0 = the default rule, the description
                               length of the extra leaf ((k/2) log2 pixels), which follows the reference encoder's tree sizes */
    int32_t gpu_forward;    /* 1: forward YCoCg and Squeeze run on the GPU (fuifgpu_fwd_*).
                               Same bytes as with 0.  No GPU: FUIFGPU_E_HIP (no silent host route). */
    int32_t gpu_entropy;    /* 1: the MANIAC pixel loop of every compressed channel group runs on the GPU (csrc/maniac_encode.hip: context
                               model of all pixels in parallel, then one wavefront per group for symbol binarisation, chance updates and
                               the range coder, maniac/rac_enc.h:28-100); group headers, tree learning and the tree itself stay host code.
                               Same bytes as with 0.  No GPU: FUIFGPU_E_HIP. */
} fuifgpu_encode_options;
int fuifgpu_encode_image(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                         uint8_t **blob_out, size_t *size_out);
/* A batch of pictures of one size (planes[m]: nch planes of w*h samples): the host prepares every channel group of every picture
 * (header, learned tree, the coder's state behind it), then the MANIAC pixel loops of ALL groups run in one launch pair -- the
 * context model of every pixel in parallel, one wavefront per group for the range coder (csrc/maniac_encode.hip; the way
 * k_maniac_decode runs one wavefront per group of a batch) -- and the host assembles the streams.  blobs_out[m] / sizes_out[m]
 * are what fuifgpu_encode_image writes for picture m, byte for byte (gpu_entropy is implied; opt NULL = CLI defaults).
 * A picture in flight holds its channels on the host and on the device plus 12 bytes of coder scratch per sample (~0.5 GB per 4K
 * RGB picture): the caller sizes its batches to the device (fuifgpu_dev_mem_info) and chunks larger sets.  fuifgpu_encode_images_device
 * holds no host copy of a picture at all (4 + 12 bytes per sample on the device, and on the host one picture's learner samples at a time).
 * Replaces N runs of the reference's `fuif_encode_file` (encoding/encoding.cpp:727-735). */
int fuifgpu_encode_images(const int32_t *const *planes, int n_images, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                          uint8_t **blobs_out, size_t *sizes_out);
/* ---- lossy streams: what `fuif -Q quality[,chroma_quality]` writes for PNM input (fuif.cpp:459-503, the Squeeze branch) ----
 * After YCoCg and Squeeze every channel is divided by a constant that follows from the two qualities, the channel's number of pixel
 * halvings (hcshift + vcshift) and one of two tables (fuif.cpp:70-76): the chroma table for components 1 and 2 whenever opt->ycocg is
 * set (also for pictures of fewer than three channels, like the CLI), the luma table for everything else.  The transform list gets a
 * Quantize entry without parameters; the constants travel in the channel headers (encoding/encoding.cpp:490, transform/quantize.h:54-71).
 * With opt->squeeze == 0 the qualities are first remapped to (400 + x) / 5 (fuif.cpp:461-465: colour quantisation only).
 * With tree_mode 0 the bytes are those of `fuif -I 0 -K 0 -X 0 -Y 0 -Q ...`.  With opt->gpu_forward the division and the ranges of the
 * quotients run on the GPU too (fuifgpu_fwd_quantize's kernel, one launch per picture), and channels that quantise to all zero -- at the
 * usual qualities the two finest chroma layers, fuif.cpp:75 -- are not copied back at all.
 * The DCT route of the CLI (`-J`) is not offered here: see fuif_amd/jpeglike.py for DCT streams. */
typedef struct {
    uint32_t struct_size;   /* = sizeof(fuifgpu_lossy_options) of the CALLER's header, versioned like fuifgpu_encode_options: 0 or a size
                               that is not a multiple of 4 is FUIFGPU_E_ARG; a struct that ends before chroma_quality means "same as quality" */
    float quality;          /* -Q's first number, 0..100; NaN or anything outside is FUIFGPU_E_ARG */
    float chroma_quality;   /* -Q's second number, 0..100, or anything above 100 = same as quality (the CLI's default, 101); NaN or negative
                               is FUIFGPU_E_ARG */
} fuifgpu_lossy_options;
/* fuifgpu_encode_image / fuifgpu_encode_images with the quantisation step.  lossy == NULL, or both qualities >= 100 (fuif.cpp:459), writes
 * exactly the bytes of the lossless call.  Found by symbol lookup: the ABI version does not change. */
int fuifgpu_encode_image_lossy(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                               const fuifgpu_lossy_options *lossy, uint8_t **blob_out, size_t *size_out);
int fuifgpu_encode_images_lossy(const int32_t *const *planes, int n_images, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                                const fuifgpu_lossy_options *lossy, uint8_t **blobs_out, size_t *sizes_out);
/* ---- pictures that already live in device memory (a renderer's output, a torch tensor, a decoded batch's output slab) ----
 * planes_device[m]: nch planes of w*h int32 in DEVICE memory of the calling thread's current device (values in [0, 2^bit_depth-1]);
 * they are read, never written, and stay the caller's.  Same bytes as fuifgpu_encode_images_lossy for the same samples and options;
 * gpu_forward and gpu_entropy are implied.  lossy == NULL: lossless.  Synchronous (null stream), like the other encode calls.
 * The planes are copied device-to-device into working buffers, the forward transforms run there, and the transformed channels stay
 * on the device until the last coded byte: their ranges and zero counts come from one statistics launch, the tree learner's samples
 * from one launch per picture, and only a group that is rolled back to "uncompressed" (encoding.cpp:545-551) comes to the host.
 * Without a HIP device: FUIFGPU_E_HIP (no host route).  A NULL planes_device[m] is FUIFGPU_E_ARG and leaves every blobs_out[m] NULL.
 * Found by symbol lookup, like the three entry points below it: the ABI version does not change. */
int fuifgpu_encode_images_device(const int32_t *const *planes_device, int n_images, int w, int h, int nch, int bit_depth,
                                 const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy,
                                 uint8_t **blobs_out, size_t *sizes_out);
/* one plane's {min, max, number of zero samples} accumulated into stats3_device (device memory the caller presets, e.g.
 * INT32_MAX, INT32_MIN, 0); the plane is only read.  n_samples == 0 touches nothing; n_samples < 0 or > INT32_MAX (the count is an
 * int32), or a NULL pointer with n_samples > 0: FUIFGPU_E_ARG.  Asynchronous on stream */
int fuifgpu_channel_stats(const int32_t *plane_device, int64_t n_samples, int32_t *stats3_device, void *stream);
/* diagnostic: bytes of whole sample planes/channels the LAST encode call of this thread copied host->device and device->host
 * (tables, trees, job records, learner samples, coder state and coded bytes are not planes and are not counted) */
int fuifgpu_encode_plane_traffic(uint64_t *h2d_bytes, uint64_t *d2h_bytes);
/* ---- the writer's tree learner on its own (found by symbol lookup: the ABI version does not change) ----
 * One sample set: n_samples rows of nprops int32 properties, row-major, and one residual class (0..16) per sample.  where: 0 = the
 * recursive host learner of tree_mode 1, 1 = props / bucket are DEVICE pointers (read, never written) and the tree is learned level by
 * level with the kernels of tree_mode 2, 2 = host pointers, level by level with plain C++ statistics (a test aid: the host side of
 * tree_mode 2 without a GPU).  All three write the same node array: nodes_out gets it in the order the host learner numbers it
 * (node 0 the root, prop -1 a leaf, gt / le the children for property > split / <= split), *n_nodes its length (1 = a single leaf).
 * opt NULL: max_nodes 4095, max_depth 14, min_leaf 48, split_bits 0, scale 1.  FUIFGPU_E_ARG: nprops < 1 or > 63, a negative count or
 * one above INT32_MAX, max_nodes < 1, max_depth < 0, min_leaf < 1, a scale that is not a positive finite number, a class above 16
 * (host pointers), or a tree of more than cap nodes. */
typedef struct {
    uint32_t struct_size;   /* = sizeof(fuifgpu_learn_options) */
    int32_t max_nodes, max_depth, min_leaf;
    int32_t split_bits;     /* as fuifgpu_encode_options::split_bits */
    double scale;           /* pixels a sample stands for (the sampling stride) */
} fuifgpu_learn_options;
typedef struct { int32_t prop, split, gt, le; } fuifgpu_learn_node;
int fuifgpu_learn_tree(const int32_t *props, const uint8_t *bucket, int64_t n_samples, int nprops, const fuifgpu_learn_options *opt,
                       int where, fuifgpu_learn_node *nodes_out, int cap, int *n_nodes);
/* diagnostic, per thread, of the LAST encode call: bytes of learner sample rows + classes copied to the host (tree_mode 1 on channels
 * that live on the device), and bytes of level statistics (root histograms, shortlists, record slices) copied to the host (tree_mode 2) */
int fuifgpu_encode_learn_traffic(uint64_t *sample_bytes_d2h, uint64_t *stat_bytes_d2h);
/* ---- Palette and channel compaction: what the CLI tries by default for PNM input that is not a photograph (fuif.cpp:345-350, 374-430;
 * transform/palette.h:92-142) ----
 * In the CLI's order: every channel whose range has 256 values or more and whose samples use fewer than compact_pre_percent of them is
 * replaced by the ranks of the values that occur (only with opt->ycocg, before YCoCg); after YCoCg one palette of at most palette_colors
 * colours over all channels, then -- with more than three channels left -- over all but the last; then every channel that uses fewer
 * than compact_post_percent of its range is compacted.  An attempt that finds too many colours changes nothing and records nothing.
 * Every success records a Palette transform {first channel, last channel, colours found} and puts its palette (colours x channels,
 * hshift -1, colours in lexicographic signed order, component 0 most significant) in front of the channel list; palettes are coded
 * like any channel, with the "left" predictor.  The Squeeze test of fuif.cpp:453 looks at channel 0, i.e. at the newest palette.
 * A quality below 100 with palette_colors > 0 switches all three off (fuif.cpp:345-350; chroma_quality is not looked at).
 * With tree_mode 0 the bytes are those of `fuif -I 0 -K .. -X .. -Y ..`.  With opt->gpu_forward, and always for planes on the device, the
 * colours are collected and the pixels indexed by kernels (fuifgpu_fwd_palette's); the index plane stays on the device like any channel,
 * and a palette's colours are a table, not a plane: fuifgpu_encode_plane_traffic does not count them. */
typedef struct {
    uint32_t struct_size;        /* = sizeof(fuifgpu_palette_options) of the CALLER's header, versioned like fuifgpu_encode_options; fields
                                    the caller's struct ends before are 0 */
    int32_t palette_colors;      /* -K: 0 = off, CLI default 256; below 0 or above 32767 (an index is an int16 sample), or above 0 for
                                    pictures of more than four channels, is FUIFGPU_E_ARG */
    float compact_post_percent;  /* -X: 0 = off, CLI default 70; NaN, negative or above 100 is FUIFGPU_E_ARG */
    float compact_pre_percent;   /* -Y: likewise */
} fuifgpu_palette_options;
/* fuifgpu_encode_image_lossy / fuifgpu_encode_images_lossy / fuifgpu_encode_images_device (planes_on_device != 0) with the three options.
 * palette == NULL or all three 0 writes exactly the bytes of those calls.  Pictures of one batch may end up with different transform
 * chains and channel counts.  Found by symbol lookup: the ABI version does not change. */
int fuifgpu_encode_image_ex(const int32_t *planes, int w, int h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                            const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette, uint8_t **blob_out, size_t *size_out);
int fuifgpu_encode_images_ex(const int32_t *const *planes, int planes_on_device, int n_images, int w, int h, int nch, int bit_depth,
                             const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette,
                             uint8_t **blobs_out, size_t *sizes_out);
/* transform/palette.h:92-142 on raw device planes: the distinct tuples of planes_device[0..nb-1] (nb 1..4, n_samples int32 each, values
 * of int16 range) are collected on the GPU.  More than max_colors of them: *n_colors = -1, nothing else is written.  Otherwise *n_colors
 * is their number, palette_host[c * max_colors + k] component c of colour k (host memory, nb * max_colors words, colours in the
 * reference's order) and index_device[i] the colour of sample i (device memory; it may be planes_device[0] itself).  Synchronous; the
 * kernels run on `stream`.  nb outside 1..4, a negative count, a sample outside the int16 range, or a NULL pointer with work to do:
 * FUIFGPU_E_ARG. */
int fuifgpu_fwd_palette(const int32_t *const *planes_device, int nb, int64_t n_samples, int max_colors, int32_t *index_device,
                        int32_t *palette_host, int *n_colors, void *stream);
/* ---- animations: what `fuif frame-%02d.ppm out.fuif` writes (encoding.cpp:458-473, fuif.cpp:440-448, transform/2dmatch.h:303-381) ----
 * nb_frames pictures of w x frame_h are coded as one strip of w x (nb_frames * frame_h) under the magic "FUAF"; behind h-1 the header
 * carries nb_frames-2, framerate-1, 0 (no per-frame numerators) and 0 loops.  With match_previous the Matching transform runs behind
 * YCoCg and the palettes and in front of Squeeze, over all channels that are left: a meta-channel m of the strip's size goes in FRONT of
 * the channel list (also in front of a palette), m.q = 2*frame_h^2 + (frame_h & 1) (the offset code of "one frame up"), m = 1 on every
 * horizontal run of at least clamp(w/50, 5, 40) samples that equal the sample frame_h rows up in every channel; three erode sweeps unmark
 * the rim of every matched region, and what keeps its mark is stored as 0 in every channel.  m is coded like a palette (predictor
 * "left"); the Squeeze test of fuif.cpp:453 looks at m; Quantize leaves it alone.  The transform is written without parameters.
 * With tree_mode 0 the bytes are those of `fuif -I 0 [-F framerate] [-M 0] ...` on the frames.  With opt->gpu_forward, and always for
 * frames on the device, fuifgpu_fwd_match_frames' kernels do it on the writer's own copies; m stays on the device like any channel.
 * Only the CLI's default (-M -1) and off (-M 0) are offered.  Deeper distances (-M -2, ...) are refused: the reference's back-fill
 * (2dmatch.h:327-329) counts positions, not unmatched samples, so from the second distance on it overwrites samples an earlier distance
 * matched with an offset nobody compared -- a lossless mode that loses pixels. */
typedef struct {
    uint32_t struct_size;    /* = sizeof(fuifgpu_animation_options) of the CALLER's header, versioned like fuifgpu_encode_options; these
                                four fields are its first version: a smaller size, or one that is no multiple of 4, is FUIFGPU_E_ARG */
    int32_t nb_frames;       /* >= 1; 1 writes exactly what fuifgpu_encode_image_ex writes (magic "FUIF", no Matching) */
    int32_t framerate;       /* -F: frames per second, 0 = the CLI's 10; negative is FUIFGPU_E_ARG */
    int32_t match_previous;  /* 1 = -M -1 (what the CLI does for several frames), 0 = -M 0; anything else is FUIFGPU_E_ARG (see above) */
} fuifgpu_animation_options;
/* frames: nb_frames x nch planes of w * frame_h int32, frame after frame (a contiguous (F, C, H, W) array).  anim == NULL: one frame.
 * A strip of more than 2^31-1 samples per channel, or frame_h above 32767 (the offset code is an int), is FUIFGPU_E_ARG.
 * fuifgpu_encode_animations: n clips of one shape in host memory or (on_device != 0) in device memory, through the batch writer like
 * fuifgpu_encode_images_ex; the caller's frames are never written.  Found by symbol lookup: the ABI version does not change. */
int fuifgpu_encode_animation(const int32_t *frames, int w, int frame_h, int nch, int bit_depth, const fuifgpu_encode_options *opt,
                             const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette, const fuifgpu_animation_options *anim,
                             uint8_t **blob_out, size_t *size_out);
int fuifgpu_encode_animations(const int32_t *const *frames, int on_device, int n_clips, int w, int frame_h, int nch, int bit_depth,
                              const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, const fuifgpu_palette_options *palette,
                              const fuifgpu_animation_options *anim, uint8_t **blobs_out, size_t *sizes_out);
/* the transform alone on raw device planes: n_planes (1..8) planes of a w x h strip of nb_frames (>= 2, dividing h) frames; match_dev
 * (w * h int32) gets the match channel, and the planes are modified IN PLACE (matched samples become 0).  Asynchronous on stream */
int fuifgpu_fwd_match_frames(const int32_t *const *planes_dev, int n_planes, int w, int h, int nb_frames, int32_t *match_dev, void *stream);
/* ---- YUV 4:2:0 video frames: what `fuif -y WxH[:b] in.yuv out.fuif` writes (import/read_yuv.h:29-63, fuif.cpp:277-283, 431-435) ----
 * A frame is three planes of raw samples: Y (w x h), then Cb and Cr ((w+1)/2 x (h+1)/2 each), one byte per sample at 8 bits, two bytes
 * little-endian above -- the planar form of a .yuv file, or as a hardware video decoder leaves a frame in device memory: planar (I420) or
 * with the chroma samples interleaved (NV12, P010-like with the value in the LOW bits), often with a row pitch.
 * The stream has three channels of UNEQUAL geometry (chroma: hshift = vshift = 1, hcshift = vcshift = 0) and its transform list starts
 * [YCbCr, ChromaSubsample{0}]: both are only recorded, nothing is computed, the colour transform and the palettes are skipped
 * (image_type == 2).  Default Squeeze runs if the option is on and luma has more than 20 samples (fuif.cpp:453); as the second channel is
 * not luma-sized it has no chroma-first steps (transform/squeeze.h:276), every step covers the three channels, each with its own size.
 * A quality quantises as for PNM input, components 1 and 2 with the chroma table, but with the luma factor times 3.0 and the quality
 * factor over 3.0 (fuif.cpp:432-434) -- fuifgpu_quantization_constant_yuv.  Predictors and everything behind are those of PNM input.
 * nb_frames > 1 writes "FUAF" with the frames stacked per channel (fuif.cpp:309-329) and NO Matching transform: there is no
 * match_previous field, because the reference's previous-frame matcher indexes every channel with luma coordinates
 * (transform/2dmatch.h:321-322) and runs off the end of the chroma planes -- `-M 0` is the only setting of the CLI that works for .yuv
 * clips, and there are no bytes to reproduce for any other.  A clip needs an even h: otherwise the stacked chroma height is not the
 * (H+1)/2 of the strip the decoder expects. */
typedef struct {
    uint32_t struct_size;   /* = sizeof(fuifgpu_yuv_options) of the CALLER's header, versioned like fuifgpu_encode_options: fields the caller's
                               struct ends before are 0 (nb_frames: 1); 0 or a size that is not a multiple of 4 is FUIFGPU_E_ARG */
    int32_t layout;         /* 0 = I420 (Y plane, Cb plane, Cr plane), 1 = NV12 / P0xx (Y plane, then one plane of Cb, Cr pairs); else FUIFGPU_E_ARG */
    int32_t pitch_y;        /* bytes from one luma row to the next, 0 = tight; smaller than a row: FUIFGPU_E_ARG */
    int32_t pitch_c;        /* the same for the chroma planes (NV12: for the interleaved plane) */
    int32_t nb_frames;      /* 1 or more (below 1, or above 65535: FUIFGPU_E_ARG; a struct that ends before the field: 1): frames back to back,
                               each pitch_y * h + pitch_c * ((h+1)/2) * (I420: 2, NV12: 1) bytes; the last row of the last plane may end
                               with its samples */
    int32_t framerate;      /* as in fuifgpu_animation_options */
} fuifgpu_yuv_options;
/* n pictures (or clips) of one shape: frames[m] points at picture m's raw bytes, in host memory or (on_device != 0) in memory of the
 * current device, which is read and never written.  bit_depth 8..14.  yuv NULL = tight I420, one frame.  opt->ycocg is ignored; lossy as
 * for fuifgpu_encode_image_lossy.  A sample above 2^bit_depth - 1 in a 16-bit container is FUIFGPU_E_ARG on every route (the reference
 * would wrap it into its int16 sample).  With tree_mode 0 the bytes are those of
 * `fuif -I 0 -K 0 -X 0 -Y 0 -y WxH[:b] [-Q ..] [-R 0] [-M 0 [-F r]]`.  Host memory with opt->gpu_forward == 0: unpacked by the reference's
 * loops, every picture through the stream writer of fuifgpu_encode_image.  gpu_forward: the RAW frames go to the device (1.5 or 3 bytes
 * per pixel, what fuifgpu_encode_plane_traffic then reports), fuifgpu_unpack_yuv420's kernel unpacks all of them in one launch and the
 * forward Squeeze / Quantize kernels run per channel.  on_device: the same on the caller's memory, and the channels stay on the device
 * until the last coded byte, through the batch writer like fuifgpu_encode_images_device.  An error leaves every blobs_out[m] NULL.
 * Found by symbol lookup, like the two entry points below it: the ABI version does not change. */
int fuifgpu_encode_yuv420(const void *const *frames, int on_device, int n, int w, int h, int bit_depth, const fuifgpu_yuv_options *yuv,
                          const fuifgpu_encode_options *opt, const fuifgpu_lossy_options *lossy, uint8_t **blobs_out, size_t *sizes_out);
/* the unpacking alone on raw device memory: one frame (yuv->nb_frames is not looked at) -> three tight int32 planes, y_out w x h, cb_out
 * and cr_out (w+1)/2 x (h+1)/2.  Asynchronous on stream.  flag_device (may be NULL): one word of device memory that is set to a non-zero
 * value if any sample exceeds 2^bit_depth - 1, and is not written otherwise.  w * h == 0 touches nothing. */
int fuifgpu_unpack_yuv420(const void *frame_device, int w, int h, int bit_depth, const fuifgpu_yuv_options *yuv, int32_t *y_out, int32_t *cb_out,
                          int32_t *cr_out, int32_t *flag_device, void *stream);
/* ---- YUV 4:2:0 frames OUT: what `fuif -d x.fuif out.yuv` writes (fuif.cpp:229-231: undo_transforms(2), then export/write_yuv.h:29-58) ----
 * The plan is made with fuifgpu_plan_create_keep(.., 2, ..): the recorded [YCbCr, ChromaSubsample] pair stays, the decoded Y, Cb, Cr
 * planes are neither upsampled nor colour-transformed, and a kernel (the inverse of fuifgpu_unpack_yuv420's) writes them as raw frame
 * bytes in the layout fuifgpu_yuv_options describes -- every sample CLAMP(v, 0, maxval) (write_yuv.h:49), one byte for maxval < 256, else
 * two little-endian.  Eligible (write_yuv.h:32-33, tightened to 4:2:0): keep == 2, transforms 0 and 1 are YCbCr and ChromaSubsample, exactly
 * three output channels, channels 1 and 2 with hshift == vshift == 1, at most 14 bits.  A plan with another keep is FUIFGPU_E_ARG, a
 * keep = 2 plan of another shape (4:2:2, RGB, a palette ..) FUIFGPU_E_UNSUPPORTED.  The frame is w x h luma and (w+1)/2 x (h+1)/2 chroma
 * samples of the plan's w, h; a plane that is larger (iDCT block padding of JPEG-shaped streams) is cropped, a smaller one is
 * FUIFGPU_E_UNSUPPORTED.  yuv->nb_frames is 1 -- the stacked strip as write_YUV_file writes it: all of Y, all of Cb, all of Cr -- or the
 * stream's nb_frames: the frames back to back as fuifgpu_encode_yuv420 reads them (an odd frame height is then FUIFGPU_E_ARG, as there);
 * anything else is FUIFGPU_E_ARG.  yuv->framerate is not looked at.  No byte outside a row's samples is written: pitch padding stays the
 * caller's.  All found by symbol lookup: the ABI version does not change. */
/* bytes of one image's frame(s) for these options, nb_frames * (pitch_y * fh + pitch_c * ((fh+1)/2) * (I420: 2, NV12: 1)); 0 = this plan
 * cannot be written as 4:2:0 frames (or the options are refused) */
size_t fuifgpu_plan_yuv420_bytes(const fuifgpu_plan *plan, const fuifgpu_yuv_options *yuv);
/* replaces write_YUV_file's loops (write_yuv.h:46-53) for images [first_image, first_image + n_images) of the batch, after
 * fuifgpu_batch_undo_transforms, in ONE launch: image k's frame(s) go to dst_device + k * image_stride_bytes (0 = tight; smaller than
 * fuifgpu_plan_yuv420_bytes: FUIFGPU_E_ARG).  Asynchronous on stream.  Refused on a streaming batch (no output slab: fuifgpu_pack_yuv420
 * on the slices fuifgpu_batch_undo_transforms_to wrote) */
int fuifgpu_batch_pack_yuv420(fuifgpu_batch *batch, int first_image, int n_images, const fuifgpu_yuv_options *yuv, uint8_t *dst_device,
                              int64_t image_stride_bytes, void *stream);
/* one image into HOST memory, fuifgpu_plan_yuv420_bytes bytes (packs into a temporary device buffer whose padding bytes are 0, copies,
 * synchronises the stream): the bytes of the .yuv file of fuif.cpp:229-231 for tight I420 */
int fuifgpu_batch_download_yuv420(fuifgpu_batch *batch, int image, const fuifgpu_yuv_options *yuv, uint8_t *host, void *stream);
/* the packing alone on raw device planes, no batch (write_yuv.h:46-53 for one frame; yuv->nb_frames is not looked at): the inverse of
 * fuifgpu_unpack_yuv420 -- y w x h, cb and cr (w+1)/2 x (h+1)/2, tight int32, bit_depth 8..14.  Asynchronous on stream.  w * h == 0 touches nothing. */
int fuifgpu_pack_yuv420(const int32_t *y, const int32_t *cb, const int32_t *cr, int w, int h, int bit_depth, const fuifgpu_yuv_options *yuv,
                        void *frame_device, void *stream);
/* fuifgpu_quantization_constant for `-y` input: the same tables behind the two factors of fuif.cpp:432-434 */
int fuifgpu_quantization_constant_yuv(float quality, float chroma_quality, int squeeze_option, int chroma_table, int shift);
/* host: the constant fuif.cpp:459-503 gives one channel -- squeeze_option = opt->squeeze (the OPTION, not whether the picture was large
 * enough to be squeezed), chroma_table = 1 for the chroma table, shift = hcshift + vcshift (capped at 15).  1 when both qualities are
 * >= 100.  A negative shift or a quality the entry points above refuse gives -FUIFGPU_E_ARG. */
int fuifgpu_quantization_constant(float quality, float chroma_quality, int squeeze_option, int chroma_table, int shift);
/* channels already in a transform domain (e.g. the quantised DCT coefficient planes import/read_jpeg.h:56-184
 * builds): geometry + q + samples per channel, `transforms` = flat words {id, nparams, params...} of the
 * transforms that produced them; opt->squeeze adds the default Squeeze of the first nb_channels channels */
typedef struct {
    int32_t w, h, hshift, vshift, hcshift, vcshift, component, q;
    const int32_t *data;
} fuifgpu_raw_channel;
int fuifgpu_encode_channels(const fuifgpu_raw_channel *channels, int n_channels, int w, int h, int nb_channels, int bit_depth,
                            const int32_t *transforms, int n_transform_words, const fuifgpu_encode_options *opt,
                            uint8_t **blob_out, size_t *size_out);
void fuifgpu_free_blob(uint8_t *blob);

#ifdef __cplusplus
}
#endif
#endif /* FUIFGPU_H */
