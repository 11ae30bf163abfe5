"""Rule 11 of tests/akaze_ref.py (the order-dependent suppression between AKAZE candidates) restated over ONE flat candidate list --
level, row, col, response per candidate, levels non-decreasing -- and the hand-made lists that reach the branches no image case reaches:
shared by tests/test_akaze_pair_resident_cpu.py (the restatement against akaze_ref.suppress, and what the lists reach) and
tests/test_gpu_akaze_pair_resident.py (spvo_akaze_suppress_debug against the restatement).  Lists are for shapes only: no image."""
import functools

import numpy as np

from tests import akaze_ref as ak

f32 = np.float32
CAND_DTYPE = np.dtype([("level", np.int32), ("row", np.int32), ("col", np.int32), ("response", np.float32), ("ok", np.int32)])   # spvo_akaze_candidate


def flat_suppress(tables, cand):
    """-> (keep, stats): the indices into `cand` that stay, in output order (rule 11, then the `ok` test), and how often each branch was
    taken.  The arithmetic is akaze_ref.suppress's, float32 with every product and sum rounded separately."""
    n = len(cand)
    ax, ay, asz, aresp = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    alev, aidx, raised = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    st = dict(drops=0, drops_equal=0, same_level=0, from_below=0, below_start=0, several_hits=0, second_loop=0, not_ok=0, max_raised=0)
    began = {}          # level -> the list's length when its first candidate arrived
    m = 0
    for i in range(n):
        lev = int(cand["level"][i])
        began.setdefault(lev, m)
        ratio = f32(2 ** int(tables["octave"][lev]))
        half = f32(f32(0.5) * f32(ratio - f32(1)))
        size = f32(tables["esigma"][lev] * f32(1.5))
        size2 = f32(size * size)
        px, py, resp = f32(f32(cand["col"][i]) * ratio), f32(f32(cand["row"][i]) * ratio), f32(cand["response"][i])
        dx, dy = px - ax[:m], py - ay[:m]
        near = ((alev[:m] == lev) | (alev[:m] == lev - 1)) & (dx * dx + dy * dy <= size2)
        slot = m
        if near.any():
            slot = int(np.argmax(near))
            st["several_hits"] += int(near.sum() > 1)
            st["below_start"] += int(slot < began.get(lev - 1, began[lev]))
            if not resp > aresp[slot]:
                st["drops"] += 1
                st["drops_equal"] += int(resp == aresp[slot])
                continue
            if alev[slot] == lev:
                st["same_level"] += 1
            else:
                st["from_below"] += 1
                raised[slot] += 1
        else:
            m += 1
        ax[slot], ay[slot], asz[slot], aresp[slot], alev[slot], aidx[slot] = f32(px + half), f32(py + half), size, resp, lev, i
    st["max_raised"] = int(raised[:m].max()) if m else 0
    keep = []
    for i in range(m):
        j = np.arange(i + 1, m)
        dx, dy = ax[i] - ax[j], ay[i] - ay[j]
        if ((alev[j] == alev[i] + 1) & (dx * dx + dy * dy <= f32(asz[i] * asz[i])) & (aresp[i] < aresp[j])).any():
            st["second_loop"] += 1
        elif cand["ok"][aidx[i]]:
            keep.append(int(aidx[i]))
        else:
            st["not_ok"] += 1
    return np.array(keep, np.int32), st


def from_levels(cand_per_level):
    """akaze_ref.candidates' per-level records as one flat list"""
    out = np.zeros(sum(len(c["row"]) for c in cand_per_level), CAND_DTYPE)
    at = 0
    for lev, c in enumerate(cand_per_level):
        k = len(c["row"])
        out["level"][at:at + k], out["row"][at:at + k], out["col"][at:at + k] = lev, c["row"], c["col"]
        out["response"][at:at + k], out["ok"][at:at + k] = c["response"], c["ok"]
        at += k
    return out


RESPONSES = np.array([0.0011, 0.0013, 0.0017, 0.0019, 0.0023, 0.0029, 0.0031, 0.0037], f32)


def lattice(rows, cols, n, seed, not_ok=0.0):
    """n candidates spread over the levels of a rows x cols image: positions on a 3-pixel lattice of their octave's plane, responses from
    eight values, level by level and in raster order within a level (several may share a place); not_ok: the share with ok = 0"""
    t = ak.make_tables(rows, cols)
    rng = np.random.RandomState(seed)
    out = np.zeros(n, CAND_DTYPE)
    out["level"] = rng.randint(0, len(t["octave"]), n)
    for i in range(n):
        o = int(t["octave"][out["level"][i]])
        out["row"][i] = 3 * rng.randint(0, max((rows >> o) // 3, 1))
        out["col"][i] = 3 * rng.randint(0, max((cols >> o) // 3, 1))
    out["response"] = RESPONSES[rng.randint(0, len(RESPONSES), n)]
    out["ok"] = rng.random_sample(n) >= not_ok
    return out[np.lexsort((out["col"], out["row"], out["level"]))]


def _list(rows):
    out = np.zeros(len(rows), CAND_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


# name -> (rows, cols, builder)
LISTS = {
    "n0": (96, 160, lambda: lattice(96, 160, 0, 1)),
    "n1": (96, 160, lambda: lattice(96, 160, 1, 2)),
    "n63": (96, 160, lambda: lattice(96, 160, 63, 3)),
    "n64": (96, 160, lambda: lattice(96, 160, 64, 4)),
    "n65": (96, 160, lambda: lattice(96, 160, 65, 5)),
    "300_small": (96, 160, lambda: lattice(96, 160, 300, 6)),
    "3000_small": (96, 160, lambda: lattice(96, 160, 3000, 7)),
    "300_three_octaves": (270, 400, lambda: lattice(270, 400, 300, 8)),
    "3000_three_octaves": (270, 400, lambda: lattice(270, 400, 3000, 9)),
    # more entries than the first loop keeps in LDS (3072): the list's tail is read and written in global memory, scans cross the boundary
    "9000_four_octaves": (320, 640, lambda: lattice(320, 640, 9000, 11)),
    # one place on levels 0 .. 7 with rising responses: ONE slot, replaced seven times, each time from the level below
    "chain": (96, 160, lambda: _list([(lev, 24 >> (lev // 4), 30 >> (lev // 4), 0.001 * (lev + 2), 1) for lev in range(8)])),
    # the second loop fires only through the half-pixel asymmetry between octaves 2 and 3: 320 x 640 has four octaves
    "second_loop_removes": (320, 640, lambda: _list([(11, 22, 24, 0.002, 1), (12, 10, 10, 0.003, 1)])),
    "second_loop_keeps": (320, 640, lambda: _list([(11, 22, 24, 0.003, 1), (12, 10, 10, 0.002, 1)])),
    # a quarter of the candidates failed rule 13: some of them win a replacement, some lose, and the winners are dropped at the end
    "not_ok": (96, 160, lambda: lattice(96, 160, 1500, 10, not_ok=0.25)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rows, cols, tables, candidates, keep, stats) of a hand-made list, the restatement's answer computed once"""
    rows, cols, build = LISTS[name]
    t = ak.make_tables(rows, cols)
    cand = build()
    keep, st = flat_suppress(t, cand)
    return rows, cols, t, cand, keep, st
