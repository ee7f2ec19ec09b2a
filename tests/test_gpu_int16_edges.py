"""GPU parity (-m gpu) at the edges of the reference's 16-bit sample type.

The reference stores every sample as pixel_type = int16_t (image/image.h:35) and narrows what its inverse transforms compute
(squeeze.h:92-107,189-213; quantize.h:41).  fuif_amd/edgecases.py writes valid streams whose inverse-transform intermediates leave
16 bits; every other parity test uses streams on which nothing wraps, and compares the kernels with the oracle only.  Here every case
is decoded twice in one batch and compared, coded planes and output planes, with the oracle AND -- where oracle/_ref is built -- with
the real reference decoding the same bytes, as tests/test_gpu_reference_encoded.py does: squeeze residuals as int16 straight from the
coefficient slab and widened first (FUIFGPU_INT16_RESIDUALS), the chroma unsqueeze + YCoCg fused and as three ops
(FUIFGPU_FUSE_YCOCG), the dequantisation folded into the iDCT's loads and as a pass of its own, from int16 and in place on int32
(FUIFGPU_FUSE_DEQUANT x FUIFGPU_INT16_RESIDUALS).  The switches are read when a plan is made.

Geometries (fuif_amd/edgecases.py names what each reaches): 40x24 runs k_inv_hsqueeze_rows and the tail loops; 262x140 runs
k_inv_hsqueeze_tiles over three row tiles, the last partial, with 131 residual columns, and the vertical kernel's VS_STEP loop with a
tail; 70x66 and 134x70 put k_inv_hsq2_ycocg on both sides of its 16-pair tile with a second, partial row tile.  The largest case has
36 680 samples: all of them also run on the wavefront emulator (tests/test_emulated_kernels.py)."""
import numpy as np
import pytest

from fuif_amd import edgecases
from test_gpu_synthetic import gpu_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoded_on_the_cpu(port):
    """name -> (stream, oracle before / after undo_transforms, real reference before / after or None): computed once, shared, never modified"""
    from oracle_py import Ref
    ref = Ref() if Ref.available() else None
    cache = {}

    def get(case):
        if case["name"] not in cache:
            blob = edgecases.build(case)
            d_pre, d_post = port.decode_both(blob)
            assert d_pre.ok and d_post.ok
            r = ref.decode_both(blob) if ref else None
            if r:
                assert r[0].ok and r[1].ok
            cache[case["name"]] = (blob, d_pre, d_post, r)
        return cache[case["name"]]
    return get


def _switches(case):
    if case.get("ycocg"):
        return [dict(FUIFGPU_FUSE_YCOCG=v) for v in ("1", "0")]
    if case.get("dct"):
        return [dict(FUIFGPU_FUSE_DEQUANT=v) for v in ("1", "0")]
    return [dict()]


@pytest.mark.parametrize("int16_residuals", ["1", "0"])
@pytest.mark.parametrize("case", edgecases.CASES, ids=lambda c: c["name"])
def test_streams_at_the_int16_edges_decode_like_the_reference(gpulib, decoded_on_the_cpu, case, int16_residuals, monkeypatch):
    blob, d_pre, d_post, r = decoded_on_the_cpu(case)
    monkeypatch.setenv("FUIFGPU_INT16_RESIDUALS", int16_residuals)
    n_ops = {}
    for sw in _switches(case):
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        n_ops[tuple(sw.values())] = gpulib.Plan(blob).info.nb_ops
        pre, post, st, used = gpu_decode(gpulib, [blob, blob])
        assert not st.any(), (sw, st)
        for what, c_pre, c_post in [("oracle", d_pre, d_post)] + ([("real reference", r[0], r[1])] if r else []):
            for img in range(2):
                assert len(pre[img]) == len(c_pre.channels) and len(post[img]) == len(c_post.channels), (what, sw)
                for i, (g, e) in enumerate(zip(pre[img], c_pre.channels)):
                    if e["size"]:
                        assert np.array_equal(g, e["data"]), "%s %s: coded plane %d of image %d differs from the %s's" % (case["name"], sw, i, img, what)
                for i, (g, e) in enumerate(zip(post[img], c_post.channels)):
                    bad = int((np.asarray(g) != e["data"]).sum())
                    assert bad == 0, "%s %s: output plane %d of image %d differs from the %s's in %d of %d samples" % (case["name"], sw, i, img, what, bad, e["data"].size)
    if case.get("ycocg"):
        # the fused op really ran: OP_HSQ2_YCOCG stands for two horizontal unsqueezes and the colour transform
        assert n_ops[("1",)] == n_ops[("0",)] - 2, n_ops
