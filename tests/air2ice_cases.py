"""Queries and comparisons shared by the batched Brent point-to-point tests
(test_air2ice_batch_cpu.py, test_gpu_air2ice_batch.py).  A query is (Tx height, horizontal
distance, ice height, antenna depth), metres, the arguments of AIRICE_RTF_AIR2ICE."""
import numpy as np

import oracle

FIELDS = 16
STATUS, ITERS, PROBES, LAYERS = 12, 13, 14, 15

# One known row per status class, found on the one-query host route:
# (status, probe steps or None for "any > 0", filled air layers or None, query).
CLASS_ROWS = [
    (0, 0, 4, (63046.65524738756, 35888.55203878302, 3000.0, 232.93002138331286)),
    (0, None, 3, (11904.570671239348, 39514.863273861345, 3000.0, 35.910189045374906)),
    (2, None, None, (36405.1814704372, 176774.14423419876, 36367.26127657653, 0.0)),
    (16, None, None, (3044.7967605382023, 312.26956430451594, 3000.0, 205.19106337821916)),
    (17, None, None, (3003.007088644775, 1860.9263628260198, 3000.0, 10.074738020849377)),
    (34, None, None, (7681.005219126441, 241402.85346866745, 9000.0, 1456.3337800456802)),
    (48, None, None, (6845.888065020705, 175243.7616218542, 24983.320190262515, 0.0)),
    (49, None, None, (158037.5111139781, 86001.61494235201, 3000.0, 201.8577836207742)),
    (None, 152, None, (8081.474211979086, 6858.828864131361, 9000.0, 1960.5958557483068)),
    (0, 0, None, (5000.0, 1000.0, 3000.0, 200.0)),  # the known answer of SURVEY.md §4
]
KAT = CLASS_ROWS[-1][3]


def class_queries():
    return np.array([r[3] for r in CLASS_ROWS])


def draw(which, n, rng):
    """n queries of range A, B (air to air), C (near the ice) or D (sea-level ice)."""
    u = rng.uniform
    if which == "A":
        cols = (u(3100, 99000, n), u(0, 40000, n), np.full(n, 3000.0), u(1, 300, n))
    elif which == "B":
        cols = (u(3200, 99000, n), u(0, 40000, n), u(3000, 3190, n), np.zeros(n))
    elif which == "C":
        cols = (u(3000.5, 3100, n), u(0, 5000, n), np.full(n, 3000.0), u(1, 300, n))
    elif which == "D":
        cols = (u(100, 99000, n), u(0, 40000, n), np.zeros(n), u(1, 300, n))
    else:
        raise ValueError(which)
    return np.stack(cols, axis=1)


def mixed(n, rng, parts=(("A", 1), ("B", 1), ("C", 1), ("D", 1))):
    """n queries of the ranges in the given proportions, range after range."""
    total = sum(w for _, w in parts)
    counts = [n * w // total for _, w in parts]
    counts[0] += n - sum(counts)
    return np.concatenate([draw(k, c, rng) for (k, _), c in zip(parts, counts)])


def nonfinite_queries():
    """The known-answer query with NaN, +inf and -inf in each of its four slots."""
    rows = []
    for slot in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            q = list(KAT)
            q[slot] = bad
            rows.append(q)
    return np.array(rows)


def assert_same_bits(got, ref, what=""):
    """Every value bit for bit; a NaN only has to be a NaN at the same position."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:5])
    diff = (got.view(np.int64) != ref.view(np.int64)) & ~nan
    assert not diff.any(), (what, np.argwhere(diff)[:5], got[diff][:5], ref[diff][:5])


def oracle_rows(om, queries):
    """(n, 16): oracle.rtf_eval(AIRICE_RTF_AIR2ICE) of every query."""
    return np.array([oracle.rtf_eval(om, oracle.RTF_AIR2ICE, q) for q in queries])


def rel_err(got, ref, floor=1e-6):
    """Per-value relative error of (n, k) arrays, 0 where both are NaN, inf where only one is."""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / np.maximum(np.abs(ref), floor)
        err = np.where((got == ref) | (nan_g & nan_r), 0.0, err)  # equal infinities included
    return np.where(nan_g != nan_r, np.inf, np.nan_to_num(err, nan=np.inf))
