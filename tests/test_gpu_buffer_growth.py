"""The buffers that grow on demand, group by group: a context goes through small -> grown -> small again (capacities that depend on
rows and columns separately each grow on their own: a wide crop, a tall one of the same area, a larger one, the first again; row
counts on both sides of each floor or growth rule), and after every step its result equals a fresh context's result for the same
input bit for bit.  What a buffer holds must not depend on how it came to its size -- neither on a re-allocation (freed, sized,
cleared or not as before) nor on the zeros or leftovers of a larger call before.

One table (CASES), one test body.  The solver's growth is pinned by tests/test_gpu_solver_sizes.py.  Two groups have no row because an
existing test takes them through first use, a larger image, a smaller one and the first again and compares with a fresh context, byte
for byte (test_same_bytes_twice_in_one_context_in_a_fresh_one_and_after_another_shape in each): spvo_ctx::brisk_det
(tests/test_gpu_brisk_detect.py) and the detector's buffers of spvo_ctx::akaze (tests/test_gpu_akaze.py).  tests/test_gpu_sift_describe.py
and tests/test_gpu_akaze_mldb.py regrow the image-sized scratch of their entry points on their way, but not the row-sized buffers (the
doubling of the given rows, the floor of 1024 records), so sift_describe and akaze_describe keep their rows."""
import numpy as np
import pytest

from spvo import capi
from tests import akaze_suppress_cases as sc, sift_describe_cases as sdc
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

SHAPES = [(48, 192), (192, 48), (128, 200), (48, 192)]     # wide, tall (the same area), larger, the first again
ROOMY = [(96, 200), (200, 96), (176, 200), (96, 200)]      # the same for ORB, whose 31-pixel border leaves 48 rows no interior


def crop(images, shape, at=(150, 400)):
    return np.ascontiguousarray(images[0][at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]])


def grid(shape, n, border=40):
    """n integer positions on a lattice inside a rows x cols image (they repeat when the lattice is smaller than n)"""
    ys, xs = np.mgrid[border:shape[0] - border:4, border:shape[1] - border:4]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    return np.resize(pts, (n, 2))


def blobs(shape, shift=0):
    """a smooth image of a few Gaussian blobs: a handful of SIFT keypoints, far below any slot capacity here"""
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float32)
    img = np.full(shape, 40, np.float32)
    for i, (cy, cx, s) in enumerate([(20, 24, 3.0), (40, 60, 4.0), (24, 80, 2.5), (44, 20, 3.5), (30, 44, 5.0)]):
        img += (90 + 20 * i) * np.exp(-((y - cy) ** 2 + (x - cx - shift) ** 2) / (2 * s * s))
    return np.clip(img, 0, 255).astype(np.uint8)


def rows_u8(n, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, 32)).astype(np.uint8)


def rows_f32(n, seed):
    d = np.random.RandomState(seed).randn(n, 256).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sift_records(shape, n):
    xy = grid(shape, n, border=12)
    return sdc.records(xy[:, 0], xy[:, 1], 7.0, -1.0, 0)                 # what a FAST + SIFT front end hands over: octave 0, layer 0


def akaze_records(ctx, img, n):
    """n AKAZE records on `img`: the detector's own, repeated (the descriptor drops none)"""
    kp = ctx.akaze_detect(img)["kp"]
    assert len(kp) > 0
    return np.resize(kp, n)


SPVO_ERR_STATE = -4


def slot_steps(fill, rows_of, match, caps):
    """two steps: a pair into slots 0, 1 at caps[0]; then one into slots 2, 3 at caps[1] -- the growth empties every slot (the rows of
    slots 0, 1 are refused with SPVO_ERR_STATE, as at the parent, and as in a fresh context that never filled them), the new pair is
    there and matches as the pair of a fresh context does that made the second call only"""
    def first(ctx):
        return fill(ctx, 0, 1, caps[0]), rows_of(ctx)(0), rows_of(ctx)(1), match(ctx)(0, 1)

    def second(ctx):
        pair = fill(ctx, 2, 3, caps[1])
        for s in (0, 1):
            with pytest.raises(capi.SpvoError) as e:
                rows_of(ctx)(s)
            assert e.value.code == SPVO_ERR_STATE
        return pair, rows_of(ctx)(2), rows_of(ctx)(3), match(ctx)(2, 3)
    return [first, second]


def image_steps(call, shapes=SHAPES):
    return lambda im: [lambda ctx, s=s: call(ctx, crop(im, s)) for s in shapes]


def orb_nfeatures(ctx, img):
    return ctx.orb(img, nfeatures=600 if img.shape == ROOMY[2] else 300)            # the keypoint rows grow with the third image as well


def with_image(call):
    """steps on the 128 x 200 crop, resident behind a FAST call"""
    def steps(im, counts):
        img = crop(im, (128, 200))
        return [lambda ctx, n=n: (ctx.fast(img), call(ctx, img, n))[1] for n in counts]
    return steps


def classic_slots(im):
    l, r = crop(im, (128, 200)), crop(im, (128, 200), at=(150, 396))
    return slot_steps(lambda ctx, a, b, cap: ctx.classic_detect(l, r, a, b, kind="ORB", nfeatures=cap // 2, slot_capacity=cap), lambda ctx: ctx.classic_slot_rows,
                      lambda ctx: ctx.match_hamming_slots, (64, 128))


def sift_slots(im):
    l, r = blobs((64, 96)), blobs((64, 96), shift=3)
    return slot_steps(lambda ctx, a, b, cap: ctx.sift_detect_pair(l, r, a, b, slot_capacity=cap), lambda ctx: ctx.sift_slot_rows, lambda ctx: ctx.match_l2_slots, (64, 128))


# name -> (context options, images -> steps; a step: context -> result)
CASES = {
    # image-sized groups
    "orb": ({}, image_steps(orb_nfeatures, ROOMY)),                                                        # spvo_ctx::orb
    "gftt": ({}, image_steps(lambda ctx, img: ctx.gftt(img))),                                      # spvo_ctx::cls
    "fast": ({}, image_steps(lambda ctx, img: ctx.fast(img))),
    # (spvo_ctx::brisk_det: tests/test_gpu_brisk_detect.py; spvo_ctx::akaze's planes, scratch, tables, lists: tests/test_gpu_akaze.py)
    "sift_detect": ({}, image_steps(lambda ctx, img: ctx.sift_detect(img))),                        # spvo_ctx::sift: image, pyramid, lists
    "sift_describe": ({}, image_steps(lambda ctx, img: ctx.sift_describe(img, sift_records(img.shape, 40)))),   # ... its Gaussian-only pyramid and the given rows
    # row-sized groups: counts on both sides of each floor or rule
    "orb_describe": ({}, lambda im: with_image(lambda ctx, img, n: ctx.orb_describe(None, grid(img.shape, n), shape=img.shape))(im, (8, 600, 8))),
    "orb_describe_octaves": ({}, lambda im: with_image(lambda ctx, img, n: ctx.orb_describe_octaves(None, grid(img.shape, n), np.arange(n) % 2, shape=img.shape))(im, (8, 600, 8))),
    "orb_octaves_link_debug": ({}, lambda im: with_image(
        lambda ctx, img, n: ctx.orb_octaves_link_debug(grid(img.shape, n), np.arange(n) % 2, keep=np.arange(n) % 3 != 0, max_octave=1, shape=img.shape))(im, (8, 600, 8))),
    "brisk_describe": ({}, lambda im: with_image(lambda ctx, img, n: ctx.brisk_describe(None, grid(img.shape, n), 7.0, shape=img.shape, values0=n != 11))(im, (10, 11, 21, 10))),   # doubling
    "akaze_describe": ({}, lambda im: [lambda ctx, n=n: ctx.akaze_describe(None, akaze_records(ctx, crop(im, (128, 200)), n)) for n in (1024, 1025, 1024)]),   # floor 1024
    "akaze_suppress_debug": ({}, lambda im: [lambda ctx, n=n: ctx.akaze_suppress_debug(96, 160, sc.lattice(96, 160, n, 5)) for n in (1024, 1025, 1024)]),
    "sift_link_debug": ({}, lambda im: with_image(
        lambda ctx, img, n: ctx.sift_link_debug(sift_records(img.shape, n), keep=np.arange(n) % 3 != 0, max_octave=1, shape=img.shape))(im, (20, 60, 20))),   # a longer keep list
    "match": (dict(max_keypoints=512), lambda im: [lambda ctx, n=n: ctx.match(rows_f32(n, 1), rows_f32(n, 2), cross_check=True) for n in (100, 1025, 100)]),
    "match_hamming": ({}, lambda im: [lambda ctx, n=n: ctx.match_hamming(rows_u8(n, 1), rows_u8(n, 2), cross_check=True) for n in (100, 1025, 2049, 100)]),   # floor 2048
    # the slots: capacity 64, then 128
    "classic_detect": ({}, classic_slots),                                                          # spvo_ctx::bin
    "sift_detect_pair": ({}, sift_slots),                                                           # spvo_ctx::sift's slots
}


def same(a, b, where=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


@pytest.mark.parametrize("name", list(CASES))
def test_grown_context_equals_a_fresh_one(name, sample_images):
    opts, build = CASES[name]
    steps = build(sample_images)
    grown = make_ctx(**opts)
    try:
        for i, step in enumerate(steps):
            got = step(grown)
            fresh = make_ctx(**opts)
            try:
                want = step(fresh)
            finally:
                fresh.close()
            same(got, want, "%s step %d" % (name, i))
    finally:
        grown.close()
