// fuif_amd/csrc/maniac_encode.h -- the writer's MANIAC pixel loop on the GPU ("fixed-tree MANIAC writer",
// maniac/rac_enc.h:28-100, maniac/symbol_enc.h, encoding/encoding.cpp:74-207).  Host interface of maniac_encode.hip.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fuifgpu_internal.h"
#include "tree_learn.h"

namespace fuifgpu {

struct EncRef {            // a reference channel of the group (context_predict.h:233-289), samples on the device
    const int32_t *data;
    int32_t w, h, hshift, vshift;
};
struct EncNode {           // decoder-layout tree node (maniac/compound.h:41-56): prop < 0 = leaf number `leaf`
    int32_t prop, split, child, leaf;
};
struct EncGroup {          // one single-channel group whose samples are all known
    const int32_t *plane;  // device, w x h contiguous
    int32_t w, h, hshift, vshift;
    int32_t minval, maxval, zero, predictor;
    int32_t nrefs;
    EncRef refs[kMaxRefs];
};
struct RacEncState {       // RacOutput24 between two symbols: range, low, the delayed byte (-1 = none yet) and the run of 0xFF behind it
    uint32_t range, low;
    int32_t delayed, pending;
};

// ---- many groups in one launch pair (a batch of pictures) ----------------------------------------------------------------
struct EncJobDev {         // what the kernels see of one job; all pointers are device pointers
    EncGroup g;
    const EncNode *tree;
    int32_t n_nodes, pad;
    int32_t *guess, *leaf; // per pixel, written by k_enc_model_jobs, read by k_enc_rac_jobs
    uint16_t *leaves;      // n_leaves x 31 chances
    uint32_t *state;       // 8 words: RacEncState in / out, bytes emitted, overflow flag
    uint8_t *out;
    uint32_t out_cap, pad2;
    int64_t n;             // pixels
};
struct EncJob {            // host side of one job
    EncGroup g;                        // device pointers of the planes
    std::vector<EncNode> tree;
    int n_leaves = 1;
    uint16_t leaf_init[31];
    RacEncState state;                 // in: behind the tree; out: behind the last symbol
    std::vector<uint8_t> body;         // out: the bytes the coder emitted for the pixels
};
// Runs every job's context model (one launch, blockIdx.y = job) and then every job's coder (one wavefront per job).
int maniac_encode_jobs_gpu(std::vector<EncJob> &jobs, const uint16_t *pixel_table);

// ---- the tree learner's samples of many groups in one launch ----------------------------------------------------------------
struct LearnJobDev {       // what k_learn_samples_jobs sees of one job; all pointers are device pointers
    EncGroup g;
    int64_t n_samples, stride;   // sample s is pixel s * stride (row-major)
    int32_t nprops, pad;         // 2 * g.nrefs + 13
    int32_t *props;              // n_samples rows of nprops properties (k_learn_samples_cols_jobs: nprops columns of n_samples)
    uint8_t *bucket;             // n_samples residual classes: 0 for a zero residual d, else ilog2(|d|) + 1
};
struct LearnJob {          // host side of one job
    EncGroup g;                  // device pointers of the planes
    int64_t n_samples = 0, stride = 1;
    int nprops = 0;
};
struct LearnSamples {      // every job's rows and buckets, as they came back in one copy
    std::vector<int32_t> raw;    // n_words property words, then the bucket bytes
    size_t n_words = 0;
    std::vector<size_t> props_off, bucket_off;   // per job: first word / first byte
    const int32_t *props(size_t job) const { return raw.data() + props_off[job]; }
    const uint8_t *bucket(size_t job) const { return reinterpret_cast<const uint8_t *>(raw.data() + n_words) + bucket_off[job]; }
};
// Computes what the host learner's sampling loop computes (writer.cpp group_tree) for every job, in its order.
int learn_samples_jobs_gpu(const std::vector<LearnJob> &jobs, LearnSamples &out);

// ---- the level-wise tree learner's statistics on the GPU (tree_mode 2; csrc/tree_learn.h has the host side) ---------------------------------
struct LearnTreeJobDev {   // what the learner kernels see of one learning group; all pointers are device pointers
    const int32_t *cols;         // nprops columns of n_samples properties: column-major, so that a (node, property) scan reads one column
    const uint8_t *bucket;       // n_samples residual classes
    int32_t *idx0, *idx1;        // the samples of every node as a segment of sample numbers, ping-pong between the levels
    int64_t n_samples;
    int32_t nprops, pad;
};
struct LearnTreeJob {      // host side: what to sample (as LearnJob), how to learn, the learned tree
    LearnJob sample;
    LearnParams prm;
    std::vector<LearnNode> nodes;
};
// Samples every job on the device (k_learn_samples_cols_jobs) and learns its tree level by level with the statistics kernels, all jobs of a
// chunk in the same rounds; chunks of at most a quarter of the free device memory.  The result does not depend on the chunking.
// *stat_bytes_d2h: bytes of root histograms, shortlists and record slices copied to the host
int learn_trees_gpu(std::vector<LearnTreeJob> &jobs, uint64_t *stat_bytes_d2h);
// The same for one sample set that is already in device memory as row-major rows (fuifgpu_learn_tree, where = 1); the rows are not written
int learn_tree_rows_gpu(const int32_t *rows_device, const uint8_t *bucket_device, int64_t n_samples, int nprops, const LearnParams &prm,
                        std::vector<LearnNode> &nodes);

// grow-only device buffers of one encode call
struct EncScratch {
    int32_t *d_guess = nullptr, *d_leaf = nullptr;
    size_t pixel_cap = 0;
    uint8_t *d_bytes = nullptr;
    size_t bytes_cap = 0;
    EncNode *d_tree = nullptr;
    size_t tree_cap = 0;
    uint16_t *d_leaves = nullptr;
    size_t leaves_cap = 0;
    uint16_t *d_table = nullptr;      // the pixel coder's chance transition table (8192 entries)
    uint32_t *d_state = nullptr;      // RacEncState + byte count + overflow flag
    void release();
    // (release() ends by assigning a fresh EncScratch: one that holds nothing must not call it again)
    ~EncScratch() { if (d_guess || d_leaf || d_bytes || d_tree || d_leaves || d_table || d_state) release(); }
};

// Encodes every sample of the group in row-major order with the given tree (n_nodes >= 1) into the range coder whose state is
// *state (the tree has already gone into it on the host); appends the bytes the coder emits to `out` and leaves the state
// behind the last symbol (the caller flushes).  leaf_init = the 31 chances every leaf starts with (symbol.h:115-138),
// pixel_table = the 2 x 4096 transition table of the pixel coder.  Returns FUIFGPU_OK or FUIFGPU_E_HIP / FUIFGPU_E_NOMEM.
int maniac_encode_group_gpu(const EncGroup &g, const EncNode *tree, int n_nodes, int n_leaves, const uint16_t *leaf_init, const uint16_t *pixel_table,
                            RacEncState *state, std::vector<uint8_t> &out, EncScratch &scratch);

}  // namespace fuifgpu
