"""The attenuation spectrum without a GPU: the n = 1 route of airice_icesol_spectrum_host on the
calling thread and the drop-in's GetAttenuationSpectrum.  Header and exports, the argument checks,
every frequency list against the single-frequency host route bin by bin, the bad bins and the
non-finite rows, the class rows against mpmath, the drop-in bit for bit against the host route and
under another model, and the caller program plain and under ASan + UBSan.
Pairs, lists and the comparison rule: tests/icespec_cases.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import iceray_cases as rays
from tests import icesol_cases as sol
from tests import icespec_cases as cases
from tests.conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "cpp", "icespec_driver")
DRIVER_ASAN = os.path.join(ROOT, "tests", "cpp", "icespec_driver_asan")
KERNELS = ("icesol_spectrum_kernel", "icesol_kernel", "iceray_kernel")
SENTINEL = -777.25


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _host_spectra(solver, q, frequencies, a0=1.0, model=None):
    """airice_icesol_spectrum_host row by row on the calling thread:
    (sol (n, 18), status (n), att (n, 2, F)); nothing may launch."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    n, f = len(q), len(frequencies)
    s18, st, att = np.empty((n, sol.FIELDS)), np.empty(n, dtype=np.int64), np.empty((n, 2, f))
    before = [_lib.launch_count(k) for k in KERNELS]
    with scalar_mode(_lib.SCALAR_HOST):
        for i, (z0, x1, z1) in enumerate(q):
            o, s, a = solver.ice_attenuation_spectrum_host(z0, x1, z1, frequencies, a0=a0,
                                                           model=model)
            s18[i], st[i], att[i] = o[:, 0], s[0], a[0]
    assert [_lib.launch_count(k) for k in KERNELS] == before
    return s18, st, att


@pytest.fixture(scope="module")
def pairs(solver):
    q = cases.pairs()
    ray_rows, _ = rays.host_rows(solver, q)
    for a in (q, ray_rows):
        a.setflags(write=False)
    return q, ray_rows


@pytest.fixture(scope="module")
def single(solver, pairs):
    """frequency -> the (n, 2) attenuation columns of the single-frequency host route, computed
    once per frequency for all the lists."""
    q, _ = pairs
    cache = {}

    def columns(f):
        if f not in cache:
            got, _ = sol.host_solutions(solver, q, frequency=f)
            cache[f] = got[:, sol.ATT:sol.ATT + 2].copy()
        return cache[f]
    return columns


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import AirIceSolver, _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_icesol_spectrum_launch", "airice_icesol_spectrum_host"):
        assert f"int {name}(const double *model3" in header, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert header.count('"icesol_spectrum_kernel"') == 2  # the timer's and the counter's lists
    assert _lib.launch_count("icesol_spectrum_kernel") >= 0
    assert _lib.kernel_time("icesol_spectrum_kernel", reset=False)[1] >= 0
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        assert "int GetAttenuationSpectrum(double RxDepth, double Distance, " in f.read()
    assert callable(AirIceSolver.ice_attenuation_spectrum_device)
    assert callable(AirIceSolver.ice_attenuation_spectrum_host)


def test_argument_checks_need_no_device():
    """Every AIRICE_EINVAL case of both entries, before any device call and with the output
    untouched; n == 0 is a no-op."""
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every launch call below returns first
    counts = [_lib.launch_count(k) for k in KERNELS]

    def launch(**kw):
        a = dict(model=None, z0=p, z1=p, rays=p, ld_rays=8, sol=p, ld_sol=8, n=8, a0=1.0, freq=p,
                 n_freq=4, att=p, ld_f=4, stream=None)
        a.update(kw)
        return L.airice_icesol_spectrum_launch(*a.values()), L.airice_last_error().decode()

    assert launch(n=0, z0=None, z1=None, rays=None, sol=None, freq=None, att=None)[0] == 0
    for name in ("z0", "z1", "rays", "sol", "att"):
        rc, msg = launch(**{name: None})
        assert rc == -1 and f"({name})" in msg, (name, msg)
    rc, msg = launch(freq=None)
    assert rc == -1 and "(freq_ghz)" in msg, msg
    rc, msg = launch(n_freq=0)
    assert rc == -1 and "n_freq" in msg, msg
    for name, kw in (("ld_f", dict(ld_f=3)), ("ld_rays", dict(ld_rays=7)),
                     ("ld_sol", dict(ld_sol=7))):
        rc, msg = launch(**kw)
        assert rc == -1 and f"{name} ({kw[name]})" in msg, (name, msg)
    for bad in (math.nan, math.inf, -math.inf):
        rc, msg = launch(a0=bad)
        assert rc == -1 and "a0" in msg, msg
    bad_models = ((1.78, 0.43, 0.0132), (1.78, -0.43, -0.0132), (1.78, 0.0, 0.0132),
                  (1.78, -0.43, 0.0), (1.78, math.nan, 0.0132))
    for bad in bad_models:
        m = np.array(bad, dtype=np.float64)
        rc, msg = launch(model=_lib.ptr(m))
        assert rc == -1 and "model3" in msg, (bad, msg)

    # the host entry, on real arrays: refused with the outputs as they were
    z0, x1, z1 = (np.array([v]) for v in (-180.0, 100.0, -100.0))
    freq = np.array(cases.F8)
    s18 = np.full((sol.FIELDS, 1), SENTINEL)
    st = np.full(1, 0xAB, dtype=np.uint8)
    att = np.full((1, 2, 8), SENTINEL)

    def host(**kw):
        a = dict(model=None, z0=z0, x1=x1, z1=z1, n=1, a0=1.0, freq=freq, n_freq=8, sol=s18, ld=1,
                 status=st, att=att, ld_f=8)
        a.update(kw)
        args = [_lib.ptr(v) if isinstance(v, np.ndarray) else v for v in a.values()]
        rc = L.airice_icesol_spectrum_host(*args)
        return rc, L.airice_last_error().decode()

    assert host(n=0, z0=None, x1=None, z1=None, freq=None, sol=None, att=None)[0] == 0
    refused = [dict(z0=None), dict(x1=None), dict(z1=None), dict(freq=None), dict(sol=None),
               dict(att=None), dict(n_freq=0), dict(ld_f=7), dict(ld=0), dict(a0=math.nan),
               dict(a0=math.inf)]
    refused += [dict(model=np.array(bad)) for bad in bad_models]
    for kw in refused:
        rc, msg = host(**kw)
        assert rc == -1 and msg, (kw, rc, msg)
        assert (s18 == SENTINEL).all() and (att == SENTINEL).all() and st[0] == 0xAB, kw
    assert host()[0] == 0 and not (att == SENTINEL).any() and st[0] != 0xAB
    assert [_lib.launch_count(k) for k in KERNELS] == counts


@pytest.mark.parametrize("name", list(cases.frequency_lists()))
def test_host_route_against_the_single_frequency_route(solver, pairs, single, name):
    """Every list, every bin: the spectrum's column against ice_solutions_host at that frequency
    (exact 0.0 and NaN on both sides or on neither, otherwise 1e-12 max(1, |1 - Att|)); the
    solutions beside it are those of the list's first frequency bit for bit; the bad bins are NaN
    where the slot holds a ray and 0.0 where it does not; the non-finite rows are NaN throughout."""
    q, ray_rows = pairs
    freq = cases.frequency_lists()[name]
    s18, st, att = _host_spectrum_cached(solver, q, freq)
    nonfinite = (st & sol.NONFINITE) != 0
    assert nonfinite.sum() == len(rays.nonfinite_queries())
    assert np.isnan(att[nonfinite]).all()
    types = s18[:, sol.TYPE:sol.TYPE + 2].astype(int)
    has = np.zeros((len(q), 2), dtype=bool)
    for i in np.flatnonzero(~nonfinite):
        for s in range(2):
            has[i, s] = ray_rows[i, rays.RANG + types[i, s] - 1] != sol.NO_RAY
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
    print(f"[icespec host] {name}: worst |d| / max(1, |1 - Att|) = {worst:.3e} (bound 1e-12)")
    if cases.good(freq[0]):
        first, first_st = sol.host_solutions(solver, q, frequency=freq[0])
        assert rays.same_bits(s18, first) and np.array_equal(st, first_st)
    else:  # the solutions at a bad first bin: the choice stands
        first, _ = sol.host_solutions(solver, q, frequency=0.3)
        assert sol.same_choice(s18, first)


_SPECTRA = {}


def _host_spectrum_cached(solver, q, freq):
    key = tuple(np.asarray(freq, dtype=np.float64).view(np.uint64).tolist())
    if key not in _SPECTRA:
        _SPECTRA[key] = _host_spectra(solver, q, freq)
    return _SPECTRA[key]


def test_class_rows_against_mpmath(solver):
    """Independent of the solver's formulas: each ray the class rows' slots hold, at the three
    frequencies where the 24-node rule is pinned to mpmath, within the project's bound."""
    q = rays.class_queries()
    ray_rows, _ = rays.host_rows(solver, q)
    s18, _, att = _host_spectra(solver, q, sol.FREQUENCIES)
    bad, n, worst = cases.mp_failures(q, ray_rows, s18[:, sol.TYPE:sol.TYPE + 2], att,
                                      sol.FREQUENCIES)
    print(f"[icespec host mpmath] {n} ray x frequency values, worst {worst:.3e} of the bound")
    assert not bad, bad[:5]
    assert n >= 3 * 12


def test_dropin_is_the_host_route_and_follows_the_model(solver):
    """GetAttenuationSpectrum through its mangled name: bit for bit the host route, its argument
    checks, and after SetA / SetB / SetC the other model's spectrum."""
    q = cases.pairs()
    other = (1.75, -0.40, 0.0140)
    _, _, att = _host_spectrum_cached(solver, q, cases.F8)
    _, _, att_other = _host_spectra(solver, q[:12], cases.F8, a0=0.7, model=other)
    for i, (z0, x1, z1) in enumerate(q):
        rc, a0, a1 = cases.dropin_spectrum(z0, x1, z1, cases.F8)
        assert rc == 0 and rays.same_bits(np.stack([a0, a1]), att[i]), i
    for kw in (dict(frequencies=()), dict(a0=math.nan), dict(a0=-math.inf)):
        args = dict(frequencies=cases.F8, a0=1.0)
        args.update(kw)
        rc, a0, a1 = cases.dropin_spectrum(-180.0, 100.0, -100.0, **args)
        assert rc == -1 and (a0 == SENTINEL).all() and (a1 == SENTINEL).all(), kw
    try:
        cases.set_model(other)
        for i, (z0, x1, z1) in enumerate(q[:12]):
            rc, a0, a1 = cases.dropin_spectrum(z0, x1, z1, cases.F8, a0=0.7)
            assert rc == 0 and rays.same_bits(np.stack([a0, a1]), att_other[i]), i
        assert not rays.same_bits(att_other[0], att[0])
        cases.set_model((1.78, 0.43, 0.0132))  # outside B < 0 < C
        assert cases.dropin_spectrum(-180.0, 100.0, -100.0, cases.F8)[0] == -1
    finally:
        cases.set_model((rays.A, rays.B, rays.C))
    rc, a0, a1 = cases.dropin_spectrum(*q[0], cases.F8)
    assert rays.same_bits(np.stack([a0, a1]), att[0])


def test_caller_program_plain_and_under_sanitizers(solver):
    """tests/cpp/icespec_driver as a child program: the drop-in's lines equal the C-ABI's and this
    process's host route bit for bit; the ASan + UBSan build (its own program, nothing preloaded)
    prints the same drop-in lines and reports nothing."""
    lib = subprocess.run([DRIVER], capture_output=True, text=True, check=True)
    assert lib.stderr == "", lib.stderr
    lines = [ln.split() for ln in lib.stdout.splitlines()]
    got = {tag: {(int(ln[1]), int(ln[2])): ln[3:] for ln in lines if ln[0] == tag}
           for tag in "GH"}
    q = rays.class_queries()
    assert len(got["G"]) == len(got["H"]) == 2 * len(q) and got["G"] == got["H"]
    assert ["E", "-1"] in lines
    _, _, att = _host_spectra(solver, q, cases.F8)
    for (i, s), words in got["G"].items():
        mine = [f"{w:016x}" for w in att[i, s].view(np.uint64)]
        assert words == mine, (i, s)
    run = subprocess.run([DRIVER_ASAN], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout.splitlines() == [ln for ln in lib.stdout.splitlines()
                                       if not ln.startswith("H")]
