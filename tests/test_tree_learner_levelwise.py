"""CPU: the level-wise tree learner (csrc/tree_learn.h learn_levelwise, what tree_mode 2 runs with the kernels' statistics) against the
recursive host learner of tree_mode 1, through fuifgpu_learn_tree: where=2 takes a level's statistics from the plain C++ provider, which
fills the records and shortlists the kernels fill.  The node arrays must be equal, node for node."""
import ctypes as C

import numpy as np
import pytest

E_ARG = 4


def correlated(seed, n, nprops, lo=-300, hi=300, drivers=2):
    """n samples of nprops properties and residual classes that follow one or two of the properties"""
    rng = np.random.default_rng(seed)
    props = rng.integers(lo, hi + 1, size=(n, nprops)).astype(np.int32)
    a = int(rng.integers(0, nprops))
    b = int(rng.integers(0, nprops))
    t = (props[:, a].astype(np.int64) - lo) * 12 // (hi - lo + 1)
    if drivers > 1:
        t = t + (props[:, b] > (lo + hi) // 2) * 4
    bucket = np.clip(t + rng.integers(0, 3, size=n), 0, 16).astype(np.uint8)
    return props, bucket


def same(gpulib, props, bucket, **kw):
    want = gpulib.learn_tree(props, bucket, where="host", **kw)
    got = gpulib.learn_tree(props, bucket, where="levelwise", **kw)
    assert got.shape == want.shape and np.array_equal(got, want), (kw, want[:8], got[:8])
    return want


@pytest.mark.parametrize("chunk", range(8))
def test_seeded_sample_sets(gpulib, chunk):
    """320 sets of 200..6000 samples with 3..17 properties"""
    split = 0
    for k in range(40):
        seed = 1000 + 40 * chunk + k
        rng = np.random.default_rng(seed)
        n = int(rng.integers(200, 6001))
        nprops = int(rng.integers(3, 18))
        props, bucket = correlated(seed, n, nprops, drivers=1 + seed % 2)
        kw = dict(min_leaf=int(rng.choice([6, 20, 48])), split_bits=int(rng.choice([0, 0, 2, 16])), scale=float(rng.choice([1, 3])))
        split += len(same(gpulib, props, bucket, **kw)) > 1
    assert split >= 30, "hardly any set learned a tree: the cases check nothing"


def test_smallest_node_that_splits(gpulib):
    """min_leaf 48: 95 samples never split (n < 2 * min_leaf), 96 split exactly 48 / 48"""
    for n, nodes in ((95, 1), (96, 3)):
        props = np.zeros((n, 3), np.int32)
        props[:, 1] = np.arange(n) >= n - 48           # two values: the one candidate, 0, has exactly 48 samples above it
        bucket = (np.arange(n) >= n - 48).astype(np.uint8) * 9
        tree = same(gpulib, props, bucket, min_leaf=48, split_bits=1)
        assert len(tree) == nodes
    assert list(tree[0]) == [1, 0, 1, 2]


def test_constant_and_two_valued_properties(gpulib):
    rng = np.random.default_rng(3)
    n = 1500
    props = np.zeros((n, 4), np.int32)
    props[:, 0] = 7                                     # constant: no candidate
    props[:, 1] = rng.integers(0, 2, size=n) * 5 + 10   # two values: every order statistic clamps to mx - 1 or is the minimum
    props[:, 2] = rng.integers(-50, 50, size=n)
    props[:, 3] = 7
    bucket = (props[:, 1] > 10).astype(np.uint8) * 6 + rng.integers(0, 2, size=n).astype(np.uint8)
    tree = same(gpulib, props, bucket, split_bits=1)
    assert tree[0][0] == 1 and tree[0][1] == 10
    props[:, 1] = (np.arange(n) >= n - 60) * 5 + 10     # the upper value only in the last 60: all three quartiles are the minimum
    same(gpulib, props, (props[:, 1] > 10).astype(np.uint8) * 6, split_bits=1)


def test_negative_values_and_the_edges_of_the_range(gpulib):
    rng = np.random.default_rng(4)
    n = 3000
    props = rng.integers(-2 ** 17, 2 ** 17 + 1, size=(n, 5)).astype(np.int32)
    props[:3, 0] = [-2 ** 17, 2 ** 17, 0]
    props[:, 4] = -rng.integers(1, 9, size=n)            # all negative, a narrow range
    bucket = np.clip((props[:, 0] // 2 ** 14) + 8 + (props[:, 4] < -4) * 2, 0, 16).astype(np.uint8)
    assert len(same(gpulib, props, bucket, split_bits=2)) > 3
    wide = props.copy()
    wide[:, 1] = rng.choice([-2 ** 31, 2 ** 31 - 1, -1, 0, 12345], size=n)    # max - min overflows an int32
    same(gpulib, wide, bucket, split_bits=2)


def test_identical_columns_tie_goes_to_the_first(gpulib):
    props, bucket = correlated(5, 2000, 3, drivers=1)
    rng = np.random.default_rng(5)
    drive = rng.integers(-100, 100, size=2000).astype(np.int32)
    props[:, 1] = drive
    props[:, 2] = drive
    props[:, 0] = rng.integers(0, 4, size=2000)
    bucket = np.clip((drive + 100) // 13, 0, 16).astype(np.uint8)
    tree = same(gpulib, props, bucket, split_bits=1)
    assert len(tree) > 1 and 2 not in set(tree[:, 0]), "a tie between equal columns must go to the first"


def test_ten_identical_columns_overflow_the_shortlist(gpulib):
    """30 candidates tie exactly: more than the 8 entries of a shortlist -- the host reads the node's full records"""
    rng = np.random.default_rng(6)
    drive = rng.integers(-100, 100, size=3000).astype(np.int32)
    props = np.repeat(drive[:, None], 10, axis=1)
    bucket = np.clip((drive + 100) // 13, 0, 16).astype(np.uint8)
    tree = same(gpulib, props, bucket, split_bits=1)
    assert len(tree) > 1 and set(tree[:, 0]) <= {-1, 0}


@pytest.mark.parametrize("kw", [dict(max_depth=2), dict(max_depth=0), dict(split_bits=0), dict(split_bits=5), dict(scale=1.0), dict(scale=3.0),
                                dict(min_leaf=1), dict(min_leaf=6, max_depth=40, max_nodes=8000)], ids=str)
def test_limits_and_bars(gpulib, kw):
    props, bucket = correlated(7, 5000, 9)
    tree = same(gpulib, props, bucket, **kw)
    if kw.get("max_depth") == 2:
        assert 1 < len(tree) <= 7
    if kw.get("max_depth") == 0:
        assert len(tree) == 1


@pytest.mark.parametrize("cap", [1, 2, 3, 7, 15, 16])
def test_node_cap_follows_the_depth_first_walk(gpulib, cap):
    props, bucket = correlated(8, 6000, 6)
    full = same(gpulib, props, bucket, min_leaf=20, split_bits=1)
    assert len(full) > 15, "the uncapped tree is no larger than the cap: the case checks nothing"
    tree = same(gpulib, props, bucket, min_leaf=20, split_bits=1, max_nodes=cap)
    assert len(tree) <= cap and len(tree) == (cap if cap % 2 else cap - 1)


def test_empty_and_tiny_sets(gpulib):
    assert len(same(gpulib, np.zeros((0, 3), np.int32), np.zeros(0, np.uint8))) == 1
    assert len(same(gpulib, np.zeros((1, 1), np.int32), np.zeros(1, np.uint8))) == 1


def test_argument_errors(gpulib):
    L = gpulib.lib()
    props, bucket = correlated(9, 400, 3)
    out = np.zeros((1024, 4), np.int32)
    n = C.c_int(0)

    def call(p=props.ctypes.data, b=bucket.ctypes.data, ns=400, k=3, opt=None, where=2, o=out.ctypes.data, cap=64, cnt=C.byref(n)):
        return L.fuifgpu_learn_tree(p, b, ns, k, opt, where, o, cap, cnt)
    for where in (0, 2):
        assert call(where=where) == 0
        assert call(k=0, where=where) == E_ARG
        assert call(ns=-1, where=where) == E_ARG
        assert call(cap=0, where=where) == E_ARG
        assert call(p=None, where=where) == E_ARG
        assert call(o=None, where=where) == E_ARG
        bad = bucket.copy()
        bad[17] = 17
        assert call(b=bad.ctypes.data, where=where) == E_ARG
    assert call(where=3) == E_ARG and call(where=-1) == E_ARG
    tree = gpulib.learn_tree(props, bucket, min_leaf=6, split_bits=1)
    assert len(tree) > 3
    opt = gpulib.LearnOptions(C.sizeof(gpulib.LearnOptions), 4095, 14, 6, 1, 1.0)
    assert call(opt=C.byref(opt), cap=len(tree)) == 0 and n.value == len(tree)
    assert call(opt=C.byref(opt), cap=len(tree) - 1) == E_ARG                 # the tree does not fit
    for field, value in (("min_leaf", 0), ("max_nodes", 0), ("max_depth", -1), ("scale", 0.0), ("scale", float("nan")), ("struct_size", 8)):
        opt = gpulib.LearnOptions(C.sizeof(gpulib.LearnOptions), 4095, 14, 6, 1, 1.0)
        setattr(opt, field, value)
        assert call(opt=C.byref(opt)) == E_ARG, field
    with pytest.raises(gpulib.FuifGpuError) as e:
        gpulib.learn_tree(props, bucket[:-1])
    assert e.value.code == E_ARG
