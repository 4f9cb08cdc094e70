"""The batched Brent point-to-point solve (airice_air2ice_launch / airice_air2ice_host) without a
GPU: the header and exports, one query on the host route bit for bit against
airice_rtf_eval(AIRICE_RTF_AIR2ICE) -- the check that the search's array-free evaluator keeps the
bits of rtf_min_launch -- and against the oracle, non-finite inputs, and the argument checks of
the launch, which return before any device call."""
import ctypes
import os

import numpy as np
import pytest

import oracle
from tests import air2ice_cases as cases
from tests.conftest import ROOT

N_ROWS = 20000


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _host_one(solver, q):
    """airice_air2ice_host with n == 1 on the calling thread: (16 values, status byte)."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    with scalar_mode(_lib.SCALAR_HOST), _lib.launched("air2ice_kernel") as k:
        out, st = solver.air2ice_host(*q)
    assert k.count == 0
    return out[:, 0], int(st[0])


def _rtf_one(solver, q):
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    with scalar_mode(_lib.SCALAR_HOST):
        return solver.rtf_eval(_lib.RTF_AIR2ICE, q)


@pytest.fixture(scope="module")
def rows(solver):
    """(queries, the new host route's values and status bytes, airice_rtf_eval's values): 20,000
    rows, ranges A-D in equal parts after the class rows, computed once."""
    rng = np.random.default_rng(2026)
    cls = cases.class_queries()
    q = np.concatenate([cls, cases.mixed(N_ROWS - len(cls), rng)])
    got = np.empty((len(q), cases.FIELDS))
    st = np.empty(len(q), dtype=np.int64)
    ref = np.empty_like(got)
    for i, row in enumerate(q):
        got[i], st[i] = _host_one(solver, row)
        ref[i] = _rtf_one(solver, row)
    for a in (q, got, st, ref):
        a.setflags(write=False)
    return q, got, st, ref


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_air2ice_launch", "airice_air2ice_host"):
        assert f"int {name}(const airice_medium *m" in header, name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert _lib.launch_count("air2ice_kernel") >= 0  # the counter and the timer exist
    assert _lib.kernel_time("air2ice_kernel", reset=False) == (0.0, 0)


def test_class_rows_are_their_class(solver):
    for status, probes, layers, q in cases.CLASS_ROWS:
        o, st = _host_one(solver, q)
        assert st == int(o[cases.STATUS])
        if status is not None:
            assert st == status, (q, st)
        if probes is not None:
            assert o[cases.PROBES] == probes, (q, o[cases.PROBES])
        elif status == 0:
            assert o[cases.PROBES] > 0, q  # "probe ran"
        if layers is not None:
            assert o[cases.LAYERS] == layers, (q, o[cases.LAYERS])
    o, _ = _host_one(solver, cases.KAT)
    assert abs(o[2] - 154.70167146999108) < 2e-9 * 154.7 and abs(o[10] - 1000.0) < 1e-5


def test_host_route_keeps_the_bits_of_rtf_eval(rows):
    q, got, st, ref = rows
    cases.assert_same_bits(got, ref)
    assert np.array_equal(st, ref[:, cases.STATUS].astype(np.int64))
    # the rows reach every class: clean, probed, UB ends, max-iter, no air layer
    assert (st == 0).sum() > N_ROWS // 2 and (got[:, cases.PROBES] > 0).sum() > 100
    for bit in (1, 2, 16, 32):
        assert (st & bit).any(), bit


def test_host_route_against_the_oracle(rows, oracle_medium):
    q, got, st, _ = rows
    ref = cases.oracle_rows(oracle_medium, q)
    for col in (cases.STATUS, cases.PROBES, cases.LAYERS):
        assert np.array_equal(got[:, col], ref[:, col]), col
    defined = (ref[:, cases.STATUS].astype(np.int64) & 3) == 0  # else reference UB: status only
    err = cases.rel_err(got[defined][:, :12], ref[defined][:, :12])
    worst = float(err.max())
    print(f"[air2ice host vs oracle] {int(defined.sum())} rows compared, max rel {worst:.2e}, "
          f"{int((err > 0).any(axis=1).sum())} rows not bit-equal")
    assert worst <= 1e-9, q[defined][np.argmax(err.max(axis=1))]


def test_nonfinite_inputs_return_and_match_rtf_eval(solver):
    for q in cases.nonfinite_queries():
        o, st = _host_one(solver, q)
        ref = _rtf_one(solver, q)
        cases.assert_same_bits(o, ref, what=tuple(q))
        assert st == int(ref[cases.STATUS])


def test_launch_argument_checks_need_no_device(solver):
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    m = ctypes.byref(solver.medium)
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a device call
    before = _lib.launch_count("air2ice_kernel")
    assert L.airice_air2ice_launch(m, None, None, None, None, 0, None, 0, None, None) == 0
    names = ("m", "txh", "dist", "ice", "depth", "out")
    for i, name in enumerate(names):
        a = [m, p, p, p, p, 8, p, 8, None, None]
        a[i if i < 5 else 6] = None
        assert L.airice_air2ice_launch(*a) == -1, name  # AIRICE_EINVAL
        assert f"({name})" in L.airice_last_error().decode(), (name, L.airice_last_error())
    assert L.airice_air2ice_launch(m, p, p, p, p, 8, p, 7, None, None) == -1
    assert "ld" in L.airice_last_error().decode()
    # the host form checks the same before it allocates or launches
    assert L.airice_air2ice_host(m, None, None, None, None, 0, None, 0, None) == 0
    assert L.airice_air2ice_host(m, p, p, None, p, 8, p, 8, None) == -1
    assert "(ice)" in L.airice_last_error().decode()
    assert L.airice_air2ice_host(m, p, p, p, p, 8, p, 7, None) == -1
    assert _lib.launch_count("air2ice_kernel") == before


def test_air_to_air_host_swaps_and_flips(solver):
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    with scalar_mode(_lib.SCALAR_HOST):
        up, st_up, f_up = solver.air_to_air_host(3100.0, 5000.0, 1000.0)   # Tx below Rx
        down, st_down, f_down = solver.air_to_air_host(5000.0, 3100.0, 1000.0)
        ref = solver.rtf_eval(_lib.RTF_AIR2ICE, (5000.0, 1000.0, 3100.0, 0.0))
    assert f_up.tolist() == [True] and f_down.tolist() == [False]
    assert st_up[0] == st_down[0] == int(ref[cases.STATUS]) == 0
    cases.assert_same_bits(down[:, 0], ref)
    flipped = ref.copy()
    flipped[4] = 180 - ref[4]
    cases.assert_same_bits(up[:, 0], flipped)
    assert abs(ref[3] - 1000.0) < 1e-3
