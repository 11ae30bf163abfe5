"""GPU parity of K12/K13 (MFMA distance GEMM + exact re-rank) against the oracle: indices and distances bit-exact, in every form the
library ships.  The matrix cores only prune and the canonical re-rank decides, so all three forms owe the brute-force result:

  fused    match_gemm_kernel<false, true> + match_merge_kernel: the default while the matcher's capacity is at most 64 column tiles
           (8192 rows)
  unfused  match_gemm_kernel<false, false> + match_rerank_kernel<4> (rows of up to 1024 columns) / <0> (chunked, ring queue) with
           MATCH_ERR_REL: what the host picks on its own beyond 8192 rows (test_capacity_past_64_column_tiles) and under tuning
           "match_fused" = 0 (every other test here)
  fp8      desc_to_fp8_kernel + match_gemm_kernel<true, false> + the same re-rank kernels with the statistical window and the
           rigorous second pass (spvo_set_match_fp8; bench.py --config 5)

Every L2 test runs in all three through the `form` fixture and asserts, with spvo_match_last_form, that the form it names is the form
that ran.  The inputs and their oracle results live in tests/match_cases.py (tests/test_match_cases_cpu.py checks the inputs themselves:
that fp8_rounding_bias defeats the first pass, that E8 holds on every case); real descriptors through the feature slots are in
tests/test_gpu_pipeline.py::test_fp8_shortlist_matcher.  test_match_golden_fixture and the Hamming matcher run as they always did."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import matching
from tests import match_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(params=mc.FORMS)
def form(request, ctx_vgg, tuning):
    """Puts ctx_vgg's matcher into one of its three forms for the test and back."""
    name = request.param
    if name == "unfused":
        tuning(match_fused=0)
    if name == "fp8":
        ctx_vgg.set_match_fp8(True)
    try:
        yield name
    finally:
        if name == "fp8":
            ctx_vgg.set_match_fp8(False)


def _by_form(argnames, values):
    """form x values in one parametrisation; under the fused form a case keeps the id it had before the other forms were run"""
    rows, ids = [], []
    for f in mc.FORMS:
        for v in values:
            v = v if isinstance(v, tuple) else (v,)
            rows.append((f,) + v)
            ids.append("-".join(str(x) for x in ((f,) if f != "fused" else ()) + v))
    return pytest.mark.parametrize("form," + argnames, rows, indirect=["form"], ids=ids)


def _check(ctx, form, key, selector, cross, swap=False, capacity_tiles=1):
    a, b = mc.case(key)
    if swap:
        a, b = b, a
    if a.shape[1] == 256:
        idx, d = ctx.match(a, b, selector, cross, mc.RATIO)
    else:
        idx, d = ctx.match_l2(a, b, selector, cross, mc.RATIO, dim=a.shape[1])
    if len(a) and len(b):                                                # (an empty side returns without a launch)
        assert ctx.match_last_form() == mc.expected_form(form, len(a), len(b), selector, cross, capacity_tiles), (key, selector, cross)
    ridx, rd = mc.expected(key, selector, cross, swap)
    assert np.array_equal(idx, ridx), (key, form, selector, cross, np.nonzero(idx != ridx)[0][:10])
    if len(b):
        assert np.array_equal(d, rd), (key, form, selector, cross)        # canonical summation order: bit-exact floats


@_by_form("na,nb", mc.SIZES)
def test_match_sizes(ctx_vgg, form, na, nb):
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, ("sizes", na, nb), selector, cross)


def test_match_ties_and_duplicates(ctx_vgg, form):
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, ("ties",), selector, cross)
    # all-zero descriptors: every distance ties at 0
    _check(ctx_vgg, form, ("zeros",), "NN", True)
    _check(ctx_vgg, form, ("zeros",), "KNN", False)


def test_match_golden_fixture(ctx_vgg, golden_dir):
    m = np.load(os.path.join(golden_dir, "oracle_match.npz"))
    idx, d = ctx_vgg.match(m["a"], m["b"], "KNN", False, 0.8)
    assert np.array_equal(idx, m["knn_idx"]) and np.array_equal(d, m["knn_d"])
    idx, _ = ctx_vgg.match(m["a"], m["b"], "NN", True, 0.8)
    assert np.array_equal(idx, m["nn_idx"])


def test_match_unnormalised_large_values(ctx_vgg, form):
    _check(ctx_vgg, form, ("unnormalised",), "KNN", False)
    _check(ctx_vgg, form, ("unnormalised",), "NN", True)


def test_match_near_duplicate_clusters(ctx_vgg, form):
    """Clusters of rows that differ by a few ulps (what an untrained network produces): dozens of train rows sit
    inside the error of the distance GEMM, so the pruning must hand ALL of them to the exact re-rank; ties and
    near-ties resolve under (canonical distance, index) order exactly as the oracle's scan does."""
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, ("near_duplicate_clusters",), selector, cross)
        _check(ctx_vgg, form, ("near_duplicate_clusters",), selector, cross, swap=True)
    _check(ctx_vgg, form, ("near_duplicate_self",), "NN", True)
    _check(ctx_vgg, form, ("near_duplicate_self",), "KNN", False)


def test_match_one_big_cluster_2048(ctx_vgg, form):
    """2048 x 2048 with every row within 1e-6 of one point: every pair is inside the error window, every row is
    re-scored (32 batches per query)."""
    for selector, cross in (("KNN", False), ("NN", True)):
        _check(ctx_vgg, form, ("big_cluster_2048",), selector, cross)


@_by_form("scale", mc.SCALES)
def test_match_scaled_descriptors(ctx_vgg, form, scale):
    """the error window scales with |a|^2 + |b|^2: exactness does not depend on unit norms"""
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, ("scaled", scale), selector, cross)


def test_match_planted_and_one_cluster_700(ctx_vgg, form):
    """300 planted matches and a 200-row cluster at 1e-3 that widens every window (the synthetic half of what
    test_gpu_pipeline.py::test_fp8_shortlist_matcher held; its KNN run and two more selectors)."""
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, ("fp8_synthetic_700",), selector, cross)


def test_fp8_second_pass_is_needed_and_exact(ctx_vgg, form):
    """fp8_rounding_bias (tests/match_cases.py): the e4m3 rounding of the 96 planted pairs is biased, not random, so the statistical
    window of pass 1 drops the true neighbour of all 96 query rows and keeps two distractors (asserted on the model in
    tests/test_match_cases_cpu.py) -- a matcher whose second pass did nothing would return 96 wrong indices here.  (|dt8 - d2| of
    the planted pairs is 0.998 of the rigorous bound E8: the CPU test holds the bound to that; on the device the pairs come back as
    long as dt8 - E8 stays below the distractors' canonical 0.071.)  Both directions, three selectors; the fp32 forms run it as an
    ordinary case."""
    key = ("fp8_rounding_bias",)
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, key, selector, cross)
        _check(ctx_vgg, form, key, selector, cross, swap=True)
    idx, _ = ctx_vgg.match(*mc.case(key), "NN", False, mc.RATIO)
    assert np.array_equal(idx[:mc.BIAS_GROUPS], mc.bias_truth())          # the planted neighbours themselves, not only "what the oracle says"


@pytest.mark.parametrize("form", ["unfused", "fp8"], indirect=True)
@pytest.mark.parametrize("na,nb", mc.CHUNK_EDGES)
def test_match_rerank_chunk_edges(ctx_vgg, form, na, nb):
    """The re-rank kernel's own edges: 1024 | 1025 columns switches match_rerank_kernel<4> (row in registers) to <0> (256-column chunks,
    ring queue) -- with cross-check the sides are swapped and the switch moves to the query count (1025 x 70) --, 1281 leaves a last chunk
    of one column that holds a query's nearest row, and a cluster of 300 near-duplicates overfills one re-score batch across a chunk
    boundary.  (The fused form never runs this kernel.)"""
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, ("chunk_edges", na, nb), selector, cross)


@pytest.mark.parametrize("form", ["fp8"], indirect=True)
@pytest.mark.parametrize("key", mc.OUT_OF_RANGE, ids=lambda k: k[0])
def test_fp8_out_of_range_rows(ctx_vgg, form, key):
    """Rows with 16 |x| beyond e4m3's largest finite value 448: randn * 10, unit rows times 1e4, a single entry of 30 among entries of
    1/16, and SIFT-like 128-d integer rows up to 255 through spvo_match_l2.  The copy has to saturate (a NaN copy drops the row out of
    both passes: index -1, distance inf); |x - x8| then carries the saturation error into E8 and pass 2 re-scores what it must."""
    for selector, cross in mc.SELECTORS:
        _check(ctx_vgg, form, key, selector, cross)


@pytest.mark.parametrize("na,nb", mc.CAPACITY)
def test_capacity_past_64_column_tiles(na, nb):
    """8200 rows on one side: the matcher's capacity becomes 65 column tiles, the merge kernel's lanes no longer cover a row's tiles and
    the host leaves the fused form ON ITS OWN (no switch is set here; spvo_match_last_form must say fused = 0).  The scratch of this
    capacity is about 1.1 GB, which is why the context is this test's own."""
    from spvo import capi
    ctx = capi.Context()
    try:
        for selector, cross in mc.SELECTORS:
            _check(ctx, "fused", ("capacity", na, nb), selector, cross, capacity_tiles=65)
            assert not ctx.match_last_form()["fused"]
    finally:
        ctx.close()


@pytest.mark.parametrize("nbytes", [32, 61, 64])
@pytest.mark.parametrize("selector,cross", [("KNN", False), ("NN", False), ("NN", True)])
def test_hamming_matcher_is_bit_exact(ctx_vgg, nbytes, selector, cross):
    """cv::BFMatcher(NORM_HAMMING) for the classic front end's binary descriptors (ORB 32 bytes, AKAZE 61, BRISK 64) through
    spvo_match_hamming against oracle/matching.py: indices and distances exact, for random bit strings, planted duplicates
    (ties between train rows), near-duplicates one bit apart, and the degenerate sizes."""
    rng = np.random.RandomState(nbytes)
    a = rng.randint(0, 256, (1900, nbytes)).astype(np.uint8)
    b = rng.randint(0, 256, (2000, nbytes)).astype(np.uint8)
    b[100:200] = a[300:400]                                             # exact matches
    b[250:300] = a[300:350]                                             # ... twice: the lower train index has to win
    b[400:500] = a[500:600]
    b[400:500, 0] ^= 1                                                  # one bit apart
    a[700:720] = a[699]                                                 # several queries with the same nearest train row (cross-check)
    for aa, bb in ((a, b), (a[:5], b[:1]), (a[:3], b[:2]), (a[:0], b), (a[:7], b[:0])):
        gi, gd = ctx_vgg.match_hamming(aa, bb, selector, cross)
        ri, rd = matching.bf_match_hamming(aa, bb, selector, cross)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd), (len(aa), len(bb))
    gi, _ = ctx_vgg.match_hamming(a, b, selector, cross)
    if selector == "NN" and not cross:
        assert (gi[300:350] == np.arange(100, 150)).all()              # two identical train rows: the lower index
    if selector == "KNN":
        assert (gi[300:350] == -1).all() and (gi[350:400] == np.arange(150, 200)).all()   # 0 < 0.8 * 0 fails; a single exact partner passes
