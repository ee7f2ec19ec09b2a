// fuif_amd/csrc/tree_learn.h -- the writer's MANIAC tree learner: the recursive host learner (tree_mode 1) and the level-wise learner
// (tree_mode 2) that takes a level's integer statistics from a provider -- the kernels of maniac_encode.hip, or the plain C++ loop below.
// Plain C++ (no HIP): csrc/writer.cpp, csrc/maniac_encode.hip and the stand-alone check tools/learn_tree_check.cpp include it.
//
// Both learners write the same node array.  Every floating-point decision (cost(), the description-length bar, the comparison of gains)
// is taken by the same host expressions in both; a provider supplies exact integers only: per (node, property) the minimum, the maximum,
// the three quartile candidates and per candidate the size and the 17-bin histogram of its "greater" side.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fuifgpu {

struct LearnNode { int prop = -1, split = 0, gt = -1, le = -1; };
constexpr int kLearnBuckets = 17;     // residual classes: 0 for a zero residual d, else ilog2(|d|) + 1 (|d| < 2^16)

// Greedy top-down splits on a pixel sample.  Cost of a sample set = n * H(bucket) where bucket is
// the zero/exponent class of the residual (what the adaptive zero/exp chances have to learn); a
// split is kept when it saves more than `threshold` bits (scaled by the sampling stride).
struct Learner {
    int nprops;
    std::vector<int32_t> props;   // [sample][nprops]
    std::vector<uint8_t> bucket;  // [sample]
    double scale = 1.0;           // pixels represented by one sample
    int max_nodes = 4095, max_depth = 14, min_leaf = 48;
    // leaf_params: the slope of the description-length rule, set so that 4K photographic streams cost the decoder as many
    // tree steps per symbol as the reference encoder's own output for the same images (9.8-9.9 both); a flat 16-bit bar,
    // the rule until round 2, gave 11.1 steps per symbol, trees a third larger and files 0.1 % LARGER (sample-fitted splits)
    double threshold_bits = 0.0, leaf_params = 11.5;
    using LNode = LearnNode;
    std::vector<LNode> nodes;

    static double cost(const int *hist, int n) {
        if (n <= 0) return 0.0;
        double c = 0.0;
        for (int b = 0; b < 17; b++) if (hist[b]) c -= hist[b] * std::log2((double)hist[b] / n);
        return c;
    }
    // what a split has to save: a flat number of bits, or (threshold_bits <= 0) the description length of the extra leaf,
    // (k/2) log2(pixels of the node) for the k chances it has to learn from those pixels
    double bar_of(int n) const { return threshold_bits > 0.0 ? threshold_bits : 0.5 * leaf_params * std::log2((double)n * scale); }
    void build(std::vector<int> &idx, int lo, int hi, int node, int depth) {
        const int n = hi - lo;
        if (n < 2 * min_leaf || depth >= max_depth || (int)nodes.size() + 2 > max_nodes) return;
        int hist[17] = {0};
        for (int i = lo; i < hi; i++) hist[bucket[idx[i]]]++;
        const double parent = cost(hist, n);
        const double bar = bar_of(n);
        if (parent * scale < bar) return;
        double best_gain = 0.0; int best_p = -1, best_s = 0;
        std::vector<int32_t> vals(n);
        for (int p = 0; p < nprops; p++) {
            int mn = 0x7FFFFFFF, mx = (int)0x80000000;
            for (int i = 0; i < n; i++) { int v = props[(size_t)idx[lo + i] * nprops + p]; vals[i] = v; mn = std::min(mn, v); mx = std::max(mx, v); }
            if (mn == mx) continue;
            int cands[3]; int nc = 0;
            for (int qd = 1; qd <= 3; qd++) {
                size_t k = (size_t)n * qd / 4;
                std::nth_element(vals.begin(), vals.begin() + k, vals.end());
                int s = vals[k];
                if (s >= mx) s = mx - 1;
                if (s < mn) s = mn;
                bool dup = false;
                for (int t = 0; t < nc; t++) dup |= (cands[t] == s);
                if (!dup) cands[nc++] = s;
            }
            for (int t = 0; t < nc; t++) {
                const int s = cands[t];
                int hg[17] = {0}; int ng = 0;
                for (int i = lo; i < hi; i++) if (props[(size_t)idx[i] * nprops + p] > s) { hg[bucket[idx[i]]]++; ng++; }
                if (ng < min_leaf || n - ng < min_leaf) continue;
                int hl[17];
                for (int b = 0; b < 17; b++) hl[b] = hist[b] - hg[b];
                double gain = parent - cost(hg, ng) - cost(hl, n - ng);
                if (gain > best_gain) { best_gain = gain; best_p = p; best_s = s; }
            }
        }
        if (best_p < 0 || best_gain * scale < bar) return;
        int mid = (int)(std::partition(idx.begin() + lo, idx.begin() + hi, [&](int i) { return props[(size_t)i * nprops + best_p] > best_s; }) - idx.begin());
        nodes[node].prop = best_p; nodes[node].split = best_s;
        int g = (int)nodes.size(); nodes.push_back(LNode());
        int l = (int)nodes.size(); nodes.push_back(LNode());
        nodes[node].gt = g; nodes[node].le = l;
        build(idx, lo, mid, g, depth + 1);
        build(idx, mid, hi, l, depth + 1);
    }
};

// ---- the level-wise learner ------------------------------------------------------------------------------------------------------------
// Whether and where a node splits depends on its sample set and its depth only -- not on the order of the samples inside it (minimum,
// maximum, order statistics and conditional histograms are functions of the multiset) -- with one exception, the node cap, which follows
// build()'s depth-first order.  So the uncapped tree is built level by level, all nodes of all learning groups of a level in one round of
// a provider, and build()'s walk is replayed over it with the cap at the end: the same tree, numbered the same way.

// what a provider computes per (node, property); POD, read by the kernels as it is
struct LearnCand { int32_t s, ng; int32_t hg[kLearnBuckets]; };      // samples with property > s: their number, their bucket histogram
struct LearnRec { int32_t mn, mx, nc, pad; LearnCand c[3]; };       // nc clamped, de-duplicated candidates in build()'s order (0: constant property)
// per node, the candidates the host has to look at: every valid one (both sides >= min_leaf) whose APPROXIMATE gain -- the provider's own
// double log2 -- is within kLearnMargin * n of the node's best approximate gain, in (property, candidate) order.
constexpr int kLearnShortCap = 8;
struct LearnShortEntry { int32_t prop, s, ng; int32_t hg[kLearnBuckets]; };
struct LearnShort { int32_t count, overflow; LearnShortEntry e[kLearnShortCap]; };   // overflow: more than the cap qualified -- the host reads the node's full records
// The margin, n * 2^-30 for a node of n samples, is derived, not tuned.  A gain is parent - cost(hg) - cost(hl): three sums of at most 17
// terms h * log2(h / n'), each sum at most n * log2(17) < 4.1 n in magnitude.  With a double log2 accurate to 2^-40 relative (the host's
// libm and the device library's log2 are both documented to a few ulp, 2^-52: twelve bits to spare) and the roundings of the quotient, the
// products and the sums (each 2^-53 relative), either side evaluates a gain with an absolute error below 3 * 4.1 n * 2^-39 < n * 2^-35.
// So a candidate whose approximate gain lies more than n * 2^-30 under the best approximate gain lies more than n * (2^-30 - 2^-34) under
// it in the host's arithmetic too and cannot be the host's winner; inside the margin lie the winner and its exact ties (duplicate property
// columns), which the host's own loop resolves in its own order.
constexpr double kLearnMargin = 1.0 / 1073741824.0;   // 2^-30, times n

struct LearnNodeDesc { int32_t job, lo, n, min_leaf; int32_t hist[kLearnBuckets]; int32_t pad[3]; };   // samples idx[lo, lo + n) of `job`, their histogram
struct LearnSplitDesc { int32_t job, lo, n, prop, s, ng; };   // stable partition of idx[lo, lo + n): the ng samples with prop > s first

struct LearnParams {
    int max_nodes = 4095, max_depth = 14, min_leaf = 48;
    double threshold_bits = 0.0, scale = 1.0;
};
struct LevelJob {             // one learning group
    int64_t n_samples = 0;
    int nprops = 0;
    LearnParams prm;
    std::vector<LearnNode> nodes;   // out: what Learner::build leaves in Learner::nodes
};

// "statistics of a level": two providers, the kernels (maniac_encode.hip) and HostLearnProvider below
struct LearnStatsProvider {
    virtual ~LearnStatsProvider() {}
    virtual int root_hists(std::vector<int32_t> &hist) = 0;                                      // n_jobs x 17: the histogram of all samples of every job
    virtual int level(const std::vector<LearnNodeDesc> &nodes, std::vector<LearnShort> &shorts) = 0;   // one round: records (kept by the provider) and shortlists
    virtual int full_slice(size_t node, std::vector<LearnRec> &recs) = 0;                        // the nprops records of node `node` of the last round
    virtual int partition(const std::vector<LearnSplitDesc> &splits) = 0;                        // closes the round
};

// build()'s candidate loop over one property's record
inline void learn_consider(const LearnCand &c, int prop, int n, int min_leaf, const int *hist, double parent, double &best_gain, int &best_p, LearnCand &best) {
    if (c.ng < min_leaf || n - c.ng < min_leaf) return;
    int hl[17];
    for (int b = 0; b < 17; b++) hl[b] = hist[b] - c.hg[b];
    double gain = parent - Learner::cost(c.hg, c.ng) - Learner::cost(hl, n - c.ng);
    if (gain > best_gain) { best_gain = gain; best_p = prop; best = c; }
}

inline int learn_levelwise(std::vector<LevelJob> &jobs, LearnStatsProvider &sp) {
    struct UNode { int prop = -1, split = 0, gt = -1, le = -1; };
    struct Active { int job, unode, lo, n, depth; int hist[17]; double parent, bar; };
    std::vector<std::vector<UNode>> un(jobs.size());
    std::vector<Active> active, next;
    // build()'s early returns that need no statistics, by its own expressions
    auto admit = [&](Active &a) {
        const LearnParams &q = jobs[(size_t)a.job].prm;
        if (a.n < 2 * q.min_leaf || a.depth >= q.max_depth) return false;
        Learner L;
        L.scale = q.scale; L.threshold_bits = q.threshold_bits;
        a.parent = Learner::cost(a.hist, a.n);
        a.bar = L.bar_of(a.n);
        return !(a.parent * q.scale < a.bar);
    };
    std::vector<int32_t> roots;
    int rc = sp.root_hists(roots);
    if (rc) return rc;
    for (size_t j = 0; j < jobs.size(); j++) {
        un[j].assign(1, UNode());
        if (jobs[j].n_samples < 1) continue;
        Active a{(int)j, 0, 0, (int)jobs[j].n_samples, 0, {0}, 0.0, 0.0};
        for (int b = 0; b < 17; b++) a.hist[b] = roots[j * 17 + (size_t)b];
        if (admit(a)) active.push_back(a);
    }
    std::vector<LearnNodeDesc> descs;
    std::vector<LearnShort> shorts;
    std::vector<LearnSplitDesc> splits;
    std::vector<LearnRec> slice;
    while (!active.empty()) {
        descs.resize(active.size());
        for (size_t k = 0; k < active.size(); k++) {
            const Active &a = active[k];
            LearnNodeDesc &d = descs[k];
            d = LearnNodeDesc();
            d.job = a.job; d.lo = a.lo; d.n = a.n; d.min_leaf = jobs[(size_t)a.job].prm.min_leaf;
            for (int b = 0; b < 17; b++) d.hist[b] = a.hist[b];
        }
        if ((rc = sp.level(descs, shorts))) return rc;
        if (shorts.size() != active.size()) return 5;   // (never expected: a provider that answered for another round)
        splits.clear(); next.clear();
        for (size_t k = 0; k < active.size(); k++) {
            const Active &a = active[k];
            const LearnParams &q = jobs[(size_t)a.job].prm;
            double best_gain = 0.0; int best_p = -1; LearnCand best{};
            const LearnShort &sh = shorts[k];
            if (sh.overflow) {
                if ((rc = sp.full_slice(k, slice))) return rc;
                for (size_t p = 0; p < slice.size(); p++)
                    for (int t = 0; t < slice[p].nc && t < 3; t++) learn_consider(slice[p].c[t], (int)p, a.n, q.min_leaf, a.hist, a.parent, best_gain, best_p, best);
            } else {
                for (int e = 0; e < sh.count && e < kLearnShortCap; e++) {
                    LearnCand c;
                    c.s = sh.e[e].s; c.ng = sh.e[e].ng;
                    for (int b = 0; b < 17; b++) c.hg[b] = sh.e[e].hg[b];
                    learn_consider(c, sh.e[e].prop, a.n, q.min_leaf, a.hist, a.parent, best_gain, best_p, best);
                }
            }
            if (best_p < 0 || best_gain * q.scale < a.bar) continue;
            std::vector<UNode> &u = un[(size_t)a.job];
            const int g = (int)u.size();
            u.push_back(UNode()); u.push_back(UNode());
            u[(size_t)a.unode].prop = best_p; u[(size_t)a.unode].split = best.s; u[(size_t)a.unode].gt = g; u[(size_t)a.unode].le = g + 1;
            Active ag{a.job, g, a.lo, best.ng, a.depth + 1, {0}, 0.0, 0.0}, al{a.job, g + 1, a.lo + best.ng, a.n - best.ng, a.depth + 1, {0}, 0.0, 0.0};
            for (int b = 0; b < 17; b++) { ag.hist[b] = best.hg[b]; al.hist[b] = a.hist[b] - best.hg[b]; }
            const bool go_g = admit(ag), go_l = admit(al);
            if (go_g) next.push_back(ag);
            if (go_l) next.push_back(al);
            if (go_g || go_l) splits.push_back(LearnSplitDesc{a.job, a.lo, a.n, best_p, best.s, best.ng});   // (two leaves: nobody reads their order)
        }
        if (next.empty()) break;
        if ((rc = sp.partition(splits))) return rc;
        active.swap(next);
    }
    // build()'s depth-first walk over the uncapped tree, with its node cap
    for (size_t j = 0; j < jobs.size(); j++) {
        struct Walk {
            const std::vector<UNode> &u; std::vector<LearnNode> &nodes; int max_nodes;
            void go(int un_i, int node) {
                const UNode &x = u[(size_t)un_i];
                if (x.prop < 0 || (int)nodes.size() + 2 > max_nodes) return;
                nodes[(size_t)node].prop = x.prop; nodes[(size_t)node].split = x.split;
                const int g = (int)nodes.size(); nodes.push_back(LearnNode());
                const int l = (int)nodes.size(); nodes.push_back(LearnNode());
                nodes[(size_t)node].gt = g; nodes[(size_t)node].le = l;
                go(x.gt, g);
                go(x.le, l);
            }
        };
        jobs[j].nodes.assign(1, LearnNode());
        Walk w{un[j], jobs[j].nodes, jobs[j].prm.max_nodes};
        w.go(0, 0);
    }
    return 0;
}

// ---- the plain C++ provider: fills the same records and shortlists from host rows (CPU tests, the stand-alone sanitizer check; never
// behind an encode call) ------------------------------------------------------------------------------------------------------------------
struct HostLearnProvider : LearnStatsProvider {
    struct Rows { const int32_t *props; const uint8_t *bucket; int64_t n; int nprops; };   // row-major, as Learner::props
    std::vector<Rows> rows;
    std::vector<std::vector<int>> idx;
    std::vector<LearnRec> recs;
    std::vector<size_t> first;     // records of node k of the last round: recs[first[k] .. first[k + 1])
    uint64_t full_fetches = 0;

    void add(const int32_t *props, const uint8_t *bucket, int64_t n, int nprops) {
        rows.push_back(Rows{props, bucket, n, nprops});
        idx.emplace_back((size_t)n);
        for (int64_t i = 0; i < n; i++) idx.back()[(size_t)i] = (int)i;
    }
    int root_hists(std::vector<int32_t> &hist) override {
        hist.assign(rows.size() * 17, 0);
        for (size_t j = 0; j < rows.size(); j++)
            for (int64_t i = 0; i < rows[j].n; i++) hist[j * 17 + rows[j].bucket[i]]++;
        return 0;
    }
    int level(const std::vector<LearnNodeDesc> &nodes, std::vector<LearnShort> &shorts) override {
        first.assign(nodes.size() + 1, 0);
        for (size_t k = 0; k < nodes.size(); k++) first[k + 1] = first[k] + (size_t)rows[(size_t)nodes[k].job].nprops;
        recs.assign(first.back(), LearnRec());
        shorts.assign(nodes.size(), LearnShort());
        std::vector<int32_t> vals;
        std::vector<double> gains;
        for (size_t k = 0; k < nodes.size(); k++) {
            const LearnNodeDesc &nd = nodes[k];
            const Rows &r = rows[(size_t)nd.job];
            const int *ix = idx[(size_t)nd.job].data() + nd.lo;
            const int n = nd.n;
            vals.resize((size_t)n);
            for (int p = 0; p < r.nprops; p++) {
                LearnRec &rec = recs[first[k] + (size_t)p];
                int mn = 0x7FFFFFFF, mx = (int)0x80000000;
                for (int i = 0; i < n; i++) { int v = r.props[(size_t)ix[i] * r.nprops + p]; vals[(size_t)i] = v; mn = std::min(mn, v); mx = std::max(mx, v); }
                rec.mn = mn; rec.mx = mx; rec.nc = 0;
                if (mn == mx) continue;
                for (int qd = 1; qd <= 3; qd++) {
                    size_t kth = (size_t)n * qd / 4;
                    std::nth_element(vals.begin(), vals.begin() + kth, vals.end());
                    int s = vals[kth];
                    if (s >= mx) s = mx - 1;
                    if (s < mn) s = mn;
                    bool dup = false;
                    for (int t = 0; t < rec.nc; t++) dup |= (rec.c[t].s == s);
                    if (!dup) rec.c[rec.nc++].s = s;
                }
                for (int t = 0; t < rec.nc; t++) {
                    LearnCand &c = rec.c[t];
                    for (int i = 0; i < n; i++) if (r.props[(size_t)ix[i] * r.nprops + p] > c.s) { c.hg[r.bucket[ix[i]]]++; c.ng++; }
                }
            }
            // the shortlist, as k_learn_shortlist writes it
            const double parent = Learner::cost(nd.hist, n);
            gains.assign((size_t)r.nprops * 3, 0.0);
            double best = 0.0; bool any = false;
            for (int p = 0; p < r.nprops; p++) {
                const LearnRec &rec = recs[first[k] + (size_t)p];
                for (int t = 0; t < rec.nc; t++) {
                    const LearnCand &c = rec.c[t];
                    if (c.ng < nd.min_leaf || n - c.ng < nd.min_leaf) continue;
                    int hl[17];
                    for (int b = 0; b < 17; b++) hl[b] = nd.hist[b] - c.hg[b];
                    const double g = parent - Learner::cost(c.hg, c.ng) - Learner::cost(hl, n - c.ng);
                    gains[(size_t)p * 3 + (size_t)t] = g;
                    if (!any || g > best) best = g;
                    any = true;
                }
            }
            LearnShort &sh = shorts[k];
            const double floor_gain = best - (double)n * kLearnMargin;
            for (int p = 0; p < r.nprops && any; p++) {
                const LearnRec &rec = recs[first[k] + (size_t)p];
                for (int t = 0; t < rec.nc; t++) {
                    const LearnCand &c = rec.c[t];
                    if (c.ng < nd.min_leaf || n - c.ng < nd.min_leaf || gains[(size_t)p * 3 + (size_t)t] < floor_gain) continue;
                    if (sh.count == kLearnShortCap) { sh.overflow = 1; continue; }
                    LearnShortEntry &e = sh.e[sh.count++];
                    e.prop = p; e.s = c.s; e.ng = c.ng;
                    for (int b = 0; b < 17; b++) e.hg[b] = c.hg[b];
                }
            }
        }
        return 0;
    }
    int full_slice(size_t node, std::vector<LearnRec> &out) override {
        if (node + 1 >= first.size()) return 4;
        full_fetches++;
        out.assign(recs.begin() + (std::ptrdiff_t)first[node], recs.begin() + (std::ptrdiff_t)first[node + 1]);
        return 0;
    }
    int partition(const std::vector<LearnSplitDesc> &splits) override {
        for (const LearnSplitDesc &s : splits) {
            const Rows &r = rows[(size_t)s.job];
            std::vector<int> &ix = idx[(size_t)s.job];
            std::stable_partition(ix.begin() + s.lo, ix.begin() + s.lo + s.n, [&](int i) { return r.props[(size_t)i * r.nprops + s.prop] > s.s; });
        }
        return 0;
    }
};

// one sample set through either host learner (fuifgpu_learn_tree where = 0 / 2, the stand-alone check)
inline void learn_tree_recursive(const int32_t *props, const uint8_t *bucket, int64_t n, int nprops, const LearnParams &q, std::vector<LearnNode> &nodes) {
    Learner L;
    L.nprops = nprops; L.scale = q.scale; L.max_nodes = q.max_nodes; L.max_depth = q.max_depth; L.min_leaf = q.min_leaf; L.threshold_bits = q.threshold_bits;
    L.props.assign(props, props + (size_t)n * (size_t)nprops);
    L.bucket.assign(bucket, bucket + n);
    std::vector<int> idx((size_t)n);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (int)i;
    L.nodes.assign(1, LearnNode());
    L.build(idx, 0, (int)idx.size(), 0, 0);
    nodes = L.nodes;
}
inline int learn_tree_levelwise_host(const int32_t *props, const uint8_t *bucket, int64_t n, int nprops, const LearnParams &q, std::vector<LearnNode> &nodes,
                                     uint64_t *full_fetches = nullptr) {
    HostLearnProvider hp;
    hp.add(props, bucket, n, nprops);
    std::vector<LevelJob> jobs(1);
    jobs[0].n_samples = n; jobs[0].nprops = nprops; jobs[0].prm = q;
    const int rc = learn_levelwise(jobs, hp);
    nodes = jobs[0].nodes;
    if (full_fetches) *full_fetches = hp.full_fetches;
    return rc;
}

}  // namespace fuifgpu
