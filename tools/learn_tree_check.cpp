// tools/learn_tree_check.cpp -- stand-alone check of the level-wise tree learner's host side (csrc/tree_learn.h): seeded sample sets through
// learn_levelwise with the plain C++ statistics provider against the recursive learner, node arrays compared.  No HIP, no library: meant to be
// built with a sanitizer, which then sees the index arithmetic of the rounds, the depth-first replay with the node cap and the slice fetches:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/learn_tree_check.cpp -o /tmp/learn_tree_check && /tmp/learn_tree_check
//
// Prints one summary line and returns 0 when every set agrees.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../fuif_amd/csrc/tree_learn.h"

using namespace fuifgpu;

namespace {
struct Set { std::vector<int32_t> props; std::vector<uint8_t> bucket; int n, nprops; };

Set make_set(uint32_t seed, int n, int nprops, int lo, int hi, int copies) {
    std::mt19937 rng(seed);
    Set s;
    s.n = n; s.nprops = nprops;
    s.props.resize((size_t)n * (size_t)nprops);
    s.bucket.resize((size_t)n);
    std::uniform_int_distribution<int> val(lo, hi), noise(0, 2), which(0, nprops - 1);
    const int a = which(rng), b = which(rng);
    for (int i = 0; i < n; i++) {
        int32_t *row = &s.props[(size_t)i * (size_t)nprops];
        for (int p = 0; p < nprops; p++) row[p] = val(rng);
        for (int p = 1; p < copies && p < nprops; p++) row[p] = row[0];   // identical columns: exact ties, and with ten of them a shortlist overflow
        const int64_t t = ((int64_t)row[copies > 1 ? 0 : a] - lo) * 12 / ((int64_t)hi - lo + 1) + (row[b] > (lo + hi) / 2 ? 3 : 0) + noise(rng);
        s.bucket[(size_t)i] = (uint8_t)(t < 0 ? 0 : (t > 16 ? 16 : t));
    }
    return s;
}

bool equal(const std::vector<LearnNode> &x, const std::vector<LearnNode> &y) {
    if (x.size() != y.size()) return false;
    for (size_t k = 0; k < x.size(); k++)
        if (x[k].prop != y[k].prop || x[k].split != y[k].split || x[k].gt != y[k].gt || x[k].le != y[k].le) return false;
    return true;
}
}  // namespace

int main() {
    int sets = 0, split = 0, capped = 0;
    uint64_t fetches = 0;
    size_t nodes_total = 0;
    std::mt19937 rng(12345);
    for (int k = 0; k < 240; k++) {
        const int n = k < 4 ? k * 32 : 200 + (int)(rng() % 5801);
        const int nprops = 1 + (int)(rng() % 17);
        const bool wide = k % 7 == 3;
        const int copies = k % 11 == 5 ? 10 : (k % 11 == 6 ? 2 : 1);
        const Set s = make_set(1000u + (uint32_t)k, n, nprops, wide ? -(1 << 17) : -40, wide ? (1 << 17) : 40, copies);
        LearnParams q;
        const int leaves[4] = {48, 20, 6, 1};
        q.min_leaf = leaves[rng() % 4];
        q.max_depth = k % 5 == 0 ? 2 : (k % 5 == 1 ? 40 : 14);
        const int caps[5] = {4095, 4095, 7, 15, 8000};
        q.max_nodes = caps[rng() % 5];
        q.threshold_bits = (double)(rng() % 3 == 0 ? 0 : 1 + rng() % 8);
        q.scale = rng() % 2 ? 1.0 : 3.0;
        std::vector<LearnNode> want, got;
        learn_tree_recursive(s.props.data(), s.bucket.data(), s.n, s.nprops, q, want);
        uint64_t f = 0;
        const int rc = learn_tree_levelwise_host(s.props.data(), s.bucket.data(), s.n, s.nprops, q, got, &f);
        if (rc != 0 || !equal(want, got)) {
            std::printf("set %d (n %d, nprops %d, min_leaf %d, depth %d, cap %d): rc %d, %zu nodes against %zu\n", k, n, nprops, q.min_leaf, q.max_depth, q.max_nodes, rc,
                        got.size(), want.size());
            return 1;
        }
        sets++; split += want.size() > 1; fetches += f; nodes_total += want.size();
        capped += (int)want.size() + 2 > q.max_nodes;
    }
    std::printf("learn_tree_check: %d sets agree (%d with a learned tree, %zu nodes, %d at their node cap, %llu full record slices fetched)\n", sets, split, nodes_total,
                capped, (unsigned long long)fetches);
    return (split > sets / 2 && fetches > 0 && capped > 0) ? 0 : 2;
}
