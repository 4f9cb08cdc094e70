"""The attenuation spectrum on the GPU (icesol_spectrum_kernel): every frequency list against
icesol_kernel bin by bin over the same solver rows, one launch per call, the layout with a padded
leading dimension, independence of the order of pairs and of frequencies, the bad bins and the
non-finite rows, the class rows against mpmath, and the host wrapper against the device calls
composed by hand.  Pairs, lists and the comparison rule: tests/icespec_cases.py."""
import numpy as np
import pytest

from tests import iceray_cases as rays
from tests import icesol_cases as sol
from tests import icespec_cases as cases

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 3, -777.25
KERNELS = ("icesol_spectrum_kernel", "icesol_kernel", "iceray_kernel")


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _to_device(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(torch.device("cuda:0"))


class Rows:
    """The device tensors of a set of pairs: the columns, iceray_kernel's rows and icesol_kernel's
    output (at 0.1 GHz: the spectrum reads only its type columns)."""

    def __init__(self, solver, q):
        import torch
        self.q = q
        self.cols = [_to_device(q[:, k]) for k in range(3)]
        dev, n = self.cols[0].device, len(q)
        self.rays = torch.empty((rays.FIELDS, n), dtype=torch.float64, device=dev)
        self.sol = torch.empty((sol.FIELDS, n), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream()
        solver.ice_rays_device(*self.cols, self.rays, stream=stream)
        solver.ice_solutions_device(*self.cols, self.rays, self.sol, stream=stream)
        torch.cuda.synchronize()

    def single(self, solver, frequency):
        """icesol_kernel's two attenuation columns at one frequency, (n, 2)."""
        import torch
        out = torch.empty_like(self.sol)
        solver.ice_solutions_device(*self.cols, self.rays, out, frequency=frequency,
                                    stream=torch.cuda.current_stream())
        return out[sol.ATT:sol.ATT + 2].cpu().numpy().T.copy()


def _spectrum(solver, rows, freq, pad=0, a0=1.0):
    """One ice_attenuation_spectrum_device call: ((n, 2, F) values, launches of the three
    kernels); with a pad, ld_f = F + pad and the pad must come back untouched."""
    import torch
    from airiceraytracing_amd import _lib
    n, f = len(rows.q), len(freq)
    fr = _to_device(freq)
    out = torch.full((n, 2, f + pad), SENTINEL, dtype=torch.float64, device=fr.device)
    before = [_lib.launch_count(k) for k in KERNELS]
    solver.ice_attenuation_spectrum_device(rows.cols[0], rows.cols[2], rows.rays, rows.sol, fr,
                                           out, a0=a0, ld_f=f + pad,
                                           stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    launches = [_lib.launch_count(k) - b for k, b in zip(KERNELS, before)]
    o = out.cpu().numpy()
    assert (o[:, :, f:] == SENTINEL).all()
    return o[:, :, :f].copy(), launches


@pytest.fixture(scope="module")
def rows(solver):
    return Rows(solver, cases.pairs())


@pytest.fixture(scope="module")
def single(solver, rows):
    """frequency -> icesol_kernel's attenuation columns over the same rows, once per frequency."""
    cache = {}

    def columns(f):
        if f not in cache:
            cache[f] = rows.single(solver, f)
        return cache[f]
    return columns


def _has(rows):
    """(n, 2): the slot holds a ray; (n): the solver flagged the row non-finite."""
    r = rows.rays.cpu().numpy().T
    types = rows.sol[sol.TYPE:sol.TYPE + 2].cpu().numpy().T.astype(int)
    nonfinite = ~(r[:, rays.STATUS] < 128)
    has = np.zeros(types.shape, dtype=bool)
    for i in np.flatnonzero(~nonfinite):
        for s in range(2):
            has[i, s] = r[i, rays.RANG + types[i, s] - 1] != sol.NO_RAY
    return has, nonfinite


@pytest.mark.parametrize("name", list(cases.frequency_lists()))
def test_against_the_single_frequency_kernel(solver, rows, single, name):
    """Every list, every bin: one launch of icesol_spectrum_kernel and none of the others, the
    column against icesol_kernel's at that frequency (exact 0.0 and NaN on both sides or on
    neither, otherwise 1e-12 max(1, |1 - Att|)), ld_f = F + 3 with the pad untouched; a bad bin is
    NaN where the slot holds a ray and 0.0 where not; a non-finite row is NaN in every bin."""
    freq = cases.frequency_lists()[name]
    att, launches = _spectrum(solver, rows, freq, pad=PAD)
    assert launches == [1, 0, 0], (name, launches)
    has, nonfinite = _has(rows)
    assert nonfinite.sum() == len(rays.nonfinite_queries()) and np.isnan(att[nonfinite]).all()
    assert has.any(axis=0).all() and (~has[~nonfinite]).any()
    worst = 0.0
    for k, f in enumerate(freq):
        if not cases.good(f):
            fin = att[~nonfinite, :, k]
            assert np.isnan(fin[has[~nonfinite]]).all(), (name, k)
            assert (fin[~has[~nonfinite]] == 0.0).all(), (name, k)
            continue
        want = single(f)
        bad = cases.mismatches(att[:, :, k], want)
        assert len(bad) == 0, (name, f, bad[:5], att[bad[0][0], bad[0][1], k], want[tuple(bad[0])])
        with np.errstate(invalid="ignore"):
            d = np.abs(att[:, :, k] - want) / np.maximum(1.0, np.abs(1 - want))
        worst = max(worst, float(np.nanmax(d)))
    print(f"[icespec device] {name}: worst |d| / max(1, |1 - Att|) = {worst:.3e} (bound 1e-12)")


def test_no_pairs_is_no_launch(solver):
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    e = torch.empty(0, dtype=torch.float64, device=dev)
    e2 = torch.empty((rays.FIELDS, 0), dtype=torch.float64, device=dev)
    fr = _to_device(cases.F8)
    with _lib.launched("icesol_spectrum_kernel") as k:
        solver.ice_attenuation_spectrum_device(e, e, e2, e2[:sol.FIELDS], fr, e,
                                               stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    assert k.count == 0


@pytest.mark.parametrize("name", ("F8", "F65", "F257"))
def test_pairs_and_frequencies_are_independent(solver, rows, name):
    """Permuting the pairs permutes the rows bit for bit (the permuted batch also ends in another
    block shape's tail), permuting the frequencies permutes the columns bit for bit, and the
    unpadded layout holds the same bits as the padded one."""
    freq = np.array(cases.frequency_lists()[name])
    att, _ = _spectrum(solver, rows, freq)
    padded, _ = _spectrum(solver, rows, freq, pad=PAD)
    assert rays.same_bits(att, padded)
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(rows.q))
    moved, launches = _spectrum(solver, Rows(solver, rows.q[perm]), freq)
    assert launches == [1, 0, 0] and rays.same_bits(moved, att[perm])
    fperm = rng.permutation(len(freq))
    shuffled, _ = _spectrum(solver, rows, freq[fperm])
    assert rays.same_bits(shuffled, att[:, :, fperm])
    # a batch that ends inside a block: the first 61 pairs alone
    head, _ = _spectrum(solver, Rows(solver, rows.q[:61]), freq)
    assert rays.same_bits(head, att[:61])


def test_a0_scales_the_integral(solver, rows):
    """Att = 1 - |a0 I|: the integral read back from a0 = 1 gives a0 = 0.37.  Both sides round
    1 - x once, the read-back of I from Att loses up to half an ulp of Att and the product rounds
    once more: four roundings of at most 1.2e-16 max(1, |Att|) each, bounded here by 1e-15."""
    one, _ = _spectrum(solver, rows, cases.F8)
    part, _ = _spectrum(solver, rows, cases.F8, a0=0.37)
    has, nonfinite = _has(rows)
    m = has & ~nonfinite[:, None]
    want = 1 - 0.37 * (1 - one[m])
    with np.errstate(invalid="ignore"):
        close = np.abs(part[m] - want) <= 1e-15 * np.maximum(1.0, np.abs(one[m]))
    assert np.all(np.where(np.isnan(want), np.isnan(part[m]), close))
    assert np.isfinite(want).sum() > 8 * 40
    assert (part[~has & ~nonfinite[:, None]] == 0.0).all()


def test_class_rows_against_mpmath(solver):
    """Independent of the solver's formulas: each ray the class rows' slots hold, at the three
    frequencies where the 24-node rule is pinned to mpmath, within the project's bound."""
    q = rays.class_queries()
    rows = Rows(solver, q)
    att, launches = _spectrum(solver, rows, sol.FREQUENCIES)
    assert launches == [1, 0, 0]
    bad, n, worst = cases.mp_failures(q, rows.rays.cpu().numpy().T,
                                      rows.sol[sol.TYPE:sol.TYPE + 2].cpu().numpy().T, att,
                                      sol.FREQUENCIES)
    print(f"[icespec device mpmath] {n} ray x frequency values, worst {worst:.3e} of the bound")
    assert not bad, bad[:5]
    assert n >= 3 * 12


def test_host_wrapper_is_the_device_calls_composed(solver, rows):
    """ice_attenuation_spectrum_host on the 64 pairs, F = 8: each of the three kernels once, and
    the device calls composed by hand bit for bit (the solutions at the first frequency)."""
    import torch
    from airiceraytracing_amd import _lib
    q = rows.q
    before = [_lib.launch_count(k) for k in KERNELS]
    s18, st, att = solver.ice_attenuation_spectrum_host(q[:, 0], q[:, 1], q[:, 2], cases.F8)
    assert [_lib.launch_count(k) - b for k, b in zip(KERNELS, before)] == [1, 1, 1]
    assert s18.shape == (sol.FIELDS, len(q)) and att.shape == (len(q), 2, 8)
    out = torch.empty_like(rows.sol)
    status = torch.empty(len(q), dtype=torch.uint8, device=out.device)
    solver.ice_solutions_device(*rows.cols, rows.rays, out, status, frequency=cases.F8[0],
                                stream=torch.cuda.current_stream())
    by_hand, _ = _spectrum(solver, rows, cases.F8)
    assert rays.same_bits(s18, out.cpu().numpy())
    assert np.array_equal(st, status.cpu().numpy())
    assert rays.same_bits(att, by_hand)
    # bin 0 of the spectrum beside the solutions' own attenuation columns: the same rule
    assert len(cases.mismatches(att[:, :, 0], s18[sol.ATT:sol.ATT + 2].T)) == 0
