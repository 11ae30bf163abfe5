"""Cases for the byte-L2 matcher (MatcherType::FLANN on binary descriptors: spvo_match_l2_u8, spvo_match_l2_u8_slots; match.hip.h K12u).

The definition is oracle.matching.bf_match on the rows cast to float32: the EXACT L2 nearest neighbours that cv::FlannBasedMatcher's two
randomized KD-trees approximate.  Squared distances of rows of at most 64 bytes are integers <= 64 * 255^2 = 4 161 600 < 2^24, exact in
float32 in any summation order, so the comparison is index for index and distance for distance AS BITS: no tolerance anywhere.

This module holds the inputs and the integer restatement of the arithmetic the kernel uses (d2 = |a'|^2 + |b'|^2 - 2 a'.b' on
a' = a xor 0x80 read as int8); tests/test_match_u8_cpu.py checks that restatement against the oracle without a GPU."""
import numpy as np

# the kernel's blocking (match.hip.h: U8L2_QT query rows per workgroup = the M of one matrix instruction; U8L2_TT train rows per LDS tile,
# 16 blocks of 16 dealt four to a wave).  The shapes below step over each boundary on each side.
QT, TT = 16, 256
WIDTHS = [1, 31, 32, 33, 61, 64]          # below / at / above the 32-byte pitch, AKAZE's 61, the full 64
SHAPES = [(1, 1), (1, 2), (2, 1), (15, 17), (16, 16), (17, 15), (64, 65), (65, 257), (257, 64)]
TILE_SHAPES = [(QT - 1, TT - 1), (QT, TT), (QT + 1, TT + 1), (TT - 1, QT - 1), (TT, QT), (TT + 1, QT + 1), (2 * QT + 1, 2 * TT + 1), (TT + 1, 63), (TT + 1, 65)]
MODES = [("NN", False), ("KNN", False), ("NN", True)]


def d2_int(a, b):
    """int64 [na, nb]: sum_k (a_k - b_k)^2 on the bytes as numbers"""
    d = a.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]
    return (d * d).sum(-1)


def d2_signed(a, b):
    """the kernel's form: a' = a xor 0x80 read as int8 (= a - 128), d2 = |a'|^2 + |b'|^2 - 2 a'.b', all in int32"""
    sa = (a ^ np.uint8(0x80)).view(np.int8).astype(np.int32)
    sb = (b ^ np.uint8(0x80)).view(np.int8).astype(np.int32)
    na = (sa * sa).sum(1, dtype=np.int32)
    nb = (sb * sb).sum(1, dtype=np.int32)
    return na[:, None] + nb[None, :] - np.int32(2) * (sa @ sb.T).astype(np.int32)


def random_rows(width, na, nb, seed=0):
    rng = np.random.RandomState(1000 * width + 10 * na + nb + seed)
    a = rng.randint(0, 256, (na, width)).astype(np.uint8)
    b = rng.randint(0, 256, (nb, width)).astype(np.uint8)
    # some exact partners and near partners, so that KNN keeps and drops rows and the cross-check has something to decide
    m = min(na, nb) // 2
    if m:
        b[:m] = a[na - m:]
        b[:m:2, 0] ^= 1
    return a, b


def not_hamming(width):
    """query rows of 0x0F; train row 0 differs in ONE 0x80 bit (Hamming 1, d2 = 128^2 = 16384), train row 1 in the 0x01 bit of eight bytes
    (Hamming 8, d2 = 8): L2 picks row 1 at sqrt(8) = 2.828427, Hamming row 0"""
    a = np.full((3, width), 0x0F, np.uint8)
    b = np.full((2, width), 0x0F, np.uint8)
    b[0, width - 1] ^= 0x80
    b[1, :8] ^= 0x01
    return a, b


def full_range():
    """all-0 against all-255 at 64 bytes: d2 = 4 161 600, distance 2040.0 -- as the nearest (train row 0 alone would do; here it is the
    nearest of two equal ones) and as the second nearest (query row 1 has an exact partner in train row 2)"""
    a = np.zeros((2, 64), np.uint8)
    a[1] = 7
    b = np.full((3, 64), 255, np.uint8)
    b[2] = 7
    return a, b


def sign_and_ties():
    """rows of 0x7F against rows of 0x80 (-1 and 0 in the signed domain: d2 = 64), identical train rows at several indices -- the lowest
    index wins, for the nearest and for the second nearest -- and exact copies of a query row: distance 0.  Under cross-check several
    train rows vote for one query: the first of them wins."""
    a = np.full((5, 64), 0x7F, np.uint8)
    a[3] = 0x80
    a[4] = 0x81
    b = np.full((TT + 20, 64), 0x00, np.uint8)
    for i in (5, 9, 40, TT + 3):
        b[i] = 0x80
    for i in (11, 12, TT + 7):
        b[i] = 0x7F
    return a, b


RATIO_BOUNDARY = [(16, 25), (16, 26), (9, 14), (9, 15)]   # (d2_0, d2_1) from a zero query: 4 < 0.8f * 5 is false in float32 (the product rounds to 4), 3 < 0.8f * sqrt(14) = 2.99 is false too


def ratio_boundary(k0, k1, width=32):
    a = np.zeros((1, width), np.uint8)
    b = np.zeros((2, width), np.uint8)
    b[0, :k0] = 1
    b[1, :k1] = 1
    return a, b


def oracle_match(a, b, selector, cross):
    from oracle import matching
    return matching.bf_match(a.astype(np.float32), b.astype(np.float32), selector, cross, 0.8)


def same_bits(got, ref):
    """indices equal and distances equal as bits"""
    return (got[0].dtype == np.int32 and got[1].dtype == np.float32 and np.array_equal(got[0], ref[0])
            and np.array_equal(got[1].view(np.uint32), np.asarray(ref[1], np.float32).view(np.uint32)))
