"""The shared host glue of the *_host entries on the GPU: the batch route leaves the padding of the
caller's columns alone (ld > n), and the three routes of a query -- inside a batch, the one-query
device route through the scalar slot, the one-query host route -- agree: device and batch bit for
bit, host and device within the bound the entry's own tests state.

The table lookup's one-query minimizer fallback is reached through the drop-in's _Table only: the
last test runs the inner-API driver on the device route and counts its launches.

The CoREAS entry has no *_host form either: its one-query routes are the drop-in's
GetHorizontalDistanceToIntersectionPoint, run through the drop-in driver.

(Air2IceRayTracing of the MultiRay variant has its three routes compared in
tests/test_gpu_edges.py::test_single_query_batches, so the route test here starts at the
pythonwrapper variant; the padding test takes both.)"""
import ctypes
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import air2ice_cases, iceray_cases

pytestmark = pytest.mark.gpu

SENTINEL, ST_SENTINEL = -777.25, 0xAB

# three queries per entry (columns in the entry's argument order); query 0 is compared across routes
SOLVE_Q = np.array([(5000.0, 1000.0, -200.0), (20000.0, 5000.0, -300.0), (8000.0, 2500.0, -100.0)])
TRACE_Q = np.array([(-200.0, 3000.0, 5000.0, 1000.0), (-100.0, 3000.0, 20000.0, 5000.0),
                    (-300.0, 3000.0, 8000.0, 2500.0)])  # depth, ice, txh, dist
AIR2ICE_Q = np.array([air2ice_cases.KAT, air2ice_cases.CLASS_ROWS[0][3],
                      air2ice_cases.CLASS_ROWS[1][3]])
ICE_Q = iceray_cases.class_queries()[[0, 2, 4]]


class Entry:
    """One *_host entry: call(q, ld) runs the (n, k) queries into fresh sentinel-filled columns of
    stride ld and returns (out (fields, ld), status (ld) or None)."""

    def __init__(self, name, fields, kernel, queries, rtol, variant=None, focusing=None,
                 status=True):
        self.name, self.fields, self.kernel, self.q, self.rtol = name, fields, kernel, queries, rtol
        self.variant, self.focusing, self.status = variant, focusing, status

    def call(self, q, ld):
        from airiceraytracing_amd import _lib
        L, p = _lib.lib(), _lib.ptr
        n = len(q)
        cols = [np.ascontiguousarray(q[:, k]) for k in range(q.shape[1])]
        out = np.full((self.fields, ld), SENTINEL)
        st = np.full(ld, ST_SENTINEL, dtype=np.uint8) if self.status else None
        if self.name == "solve":
            m = _lib.load_medium(variant=self.variant)
            rc = L.airice_solve_host(ctypes.byref(m), self.variant, 3000.0, *map(p, cols), None, n,
                                     p(out), ld, p(st))
        elif self.name == "air2ice":
            m = _lib.load_medium()
            rc = L.airice_air2ice_host(ctypes.byref(m), *map(p, cols), n, p(out), ld, p(st))
        elif self.name == "iceray":
            rc = L.airice_iceray_host(None, *map(p, cols), n, p(out), ld, p(st))
        elif self.name == "icesol":
            rc = L.airice_icesol_host(None, *map(p, cols), n, 0.9, 0.5, self.focusing, p(out), ld,
                                      p(st))
        else:  # trace: n rows of 10, no stride and no status
            assert ld == n
            m = _lib.load_medium(variant=_lib.VARIANT_PYWRAPPER)
            rows = np.full((n, 10), SENTINEL)
            rc = L.airice_trace_ice_to_air_host(ctypes.byref(m), *map(p, cols), n, p(rows))
            out = np.ascontiguousarray(rows.T)
        assert rc == 0, L.airice_last_error()
        return out, st


def _entries():
    from airiceraytracing_amd import _lib
    return [
        Entry("solve", _lib.SOLVE_FIELDS, "scalar_solve_kernel", SOLVE_Q, 1e-12,
              variant=_lib.VARIANT_MULTIRAY),
        Entry("solve", _lib.PYSOLVE_FIELDS, "scalar_solve_kernel", SOLVE_Q, 1e-12,
              variant=_lib.VARIANT_PYWRAPPER),
        Entry("air2ice", _lib.RTF_AIR2ICE_FIELDS, "air2ice_kernel", AIR2ICE_Q, 1e-9),
        Entry("iceray", _lib.ICERAY_FIELDS, "iceray_kernel", ICE_Q, 1e-9),
        Entry("icesol", _lib.ICESOL_FIELDS, "icesol_kernel", ICE_Q, 1e-9, focusing=0),
        Entry("icesol", _lib.ICESOL_FIELDS, "icesol_kernel", ICE_Q, 1e-9, focusing=1),
        Entry("trace", 10, "scalar_solve_kernel", TRACE_Q, 1e-12, status=False),
    ]


IDS = ["solve-multiray", "solve-pywrapper", "air2ice", "iceray", "icesol", "icesol-focusing",
       "trace"]


@pytest.mark.parametrize("k", range(6), ids=IDS[:6])
def test_batch_route_leaves_the_padding_alone(k):
    """n = 3, ld = 5 into sentinel-filled columns: the three live entries of every column are the
    bits of the same call at ld = n, and entries 3 and 4 still hold the sentinel (airice_solve_host
    used to copy fields * ld doubles back over them)."""
    e = _entries()[k]
    dense, dst = e.call(e.q, 3)
    out, st = e.call(e.q, 5)
    air2ice_cases.assert_same_bits(out[:, :3], dense)
    assert np.array_equal(st[:3], dst)
    assert (out[:, 3:] == SENTINEL).all() and (st[3:] == ST_SENTINEL).all()
    assert not (dense == SENTINEL).any()


@pytest.mark.parametrize("k", range(1, 7), ids=IDS[1:])
def test_the_three_routes_of_a_query_agree(k):
    """Query 0 inside an n = 2 batch, alone on the device (AIRICE_SCALAR_DEVICE: the entry's
    kernel, counted) and alone on the host (AIRICE_SCALAR_HOST: no kernel).  Device and batch: the
    same bits.  Host and device: the status byte and the count columns equal, NaN in the same
    places, the values within the entry's bound (1e-12 for the minimizer entries, as
    tests/test_gpu_edges.py and tests/test_pythonwrapper.py; 1e-9 relative for the Brent and the
    in-ice solves, as tests/test_air2ice_batch_cpu.py, test_gpu_iceray.py, test_gpu_icesol.py)."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    e = _entries()[k]
    pair, pst = e.call(e.q[:2], 2)
    with scalar_mode(_lib.SCALAR_DEVICE), _lib.launched(e.kernel) as kd:
        dev, dst = e.call(e.q[:1], 1)
    with scalar_mode(_lib.SCALAR_HOST), _lib.launched(e.kernel) as kh:
        host, hst = e.call(e.q[:1], 1)
    assert kd.count == 1 and kh.count == 0
    air2ice_cases.assert_same_bits(dev[:, 0], pair[:, 0])
    if e.status:
        assert dst[0] == pst[0] == hst[0]
    d, h = dev[:, 0], host[:, 0]
    assert np.array_equal(np.isnan(d), np.isnan(h))
    fin = ~np.isnan(d)
    if e.rtol == 1e-12:
        worst = float(np.max(np.abs(d[fin] - h[fin]) / (1e-12 + 1e-12 * np.abs(d[fin]))))
        print(f"[{IDS[k]} host vs device] worst {worst:.3e} of atol + rtol |x| at 1e-12")
        np.testing.assert_allclose(h[fin], d[fin], rtol=1e-12, atol=1e-12)
    else:
        counts = {"air2ice": slice(12, 16), "iceray": slice(29, 32), "icesol": slice(0, 0)}[e.name]
        assert np.array_equal(d[counts], h[counts]), (d[counts], h[counts])
        err = air2ice_cases.rel_err(h[fin][None, :], d[fin][None, :])
        print(f"[{IDS[k]} host vs device] worst {float(err.max()):.3e} relative")
        assert err.max() <= e.rtol, (d, h)


def test_table_fallback_runs_on_the_one_query_device_route(tmp_path):
    """The drop-in's GetHorizontalDistanceToIntersectionPoint_Table with AIRICE_SCALAR=device: a
    one-sided query runs its minimizer fallback as one launch of the one-wave kernel through the
    scalar slot.  The inner-API driver (tests/cpp/multiray_inner_driver.cpp) makes exactly one
    other call that launches that kernel, its Air2IceRayTracing solve, so the library's launch
    report must count at least two; and every _Table row -- the fallback rows among them -- has
    the bits of the batched lookup, whose fallback lanes run inside lookup_kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "multiray_inner_driver")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    with open(os.path.join(root, "airiceraytracing_amd", "data", "Atmosphere.dat.gz"), "rb") as f:
        (tmp_path / "Atmosphere.dat").write_bytes(gzip.decompress(f.read()))
    out = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, AIRICE_SCALAR="device", AIRICE_LAUNCH_REPORT="1"))
    assert out.returncode == 0, out.stderr
    report = re.search(r"airice launches:.* scalar_solve_kernel=(\d+)", out.stderr)
    assert report, out.stderr
    assert int(report.group(1)) >= 2, out.stderr
    txt = re.sub(r"-?\b(nan|inf)\b", lambda m: {"nan": "NaN", "-nan": "NaN", "inf": "Infinity",
                                                  "-inf": "-Infinity"}[m.group(0)], out.stdout)
    rows = json.loads(txt)["table_scalar_vs_batch"]
    assert rows and all(row[3] == 1 for row in rows), [row for row in rows if row[3] != 1]


def _run_multiray_driver(tmp_path, scalar):
    """tests/cpp/multiray_driver with the one-query calls on `scalar`: (its JSON, the launches of
    scalar_solve_kernel the library reports at unload)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "multiray_driver")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    with open(os.path.join(root, "airiceraytracing_amd", "data", "Atmosphere.dat.gz"), "rb") as f:
        (tmp_path / "Atmosphere.dat").write_bytes(gzip.decompress(f.read()))
    out = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, AIRICE_SCALAR=scalar, AIRICE_LAUNCH_REPORT="1"))
    assert out.returncode == 0, out.stderr
    report = re.search(r"airice launches:.* scalar_solve_kernel=(\d+)", out.stderr)
    assert report, out.stderr
    txt = re.sub(r"-?\b(nan|inf)\b", lambda m: {"nan": "NaN", "-nan": "NaN", "inf": "Infinity",
                                                  "-inf": "-Infinity"}[m.group(0)], out.stdout)
    return json.loads(txt), int(report.group(1))


def test_the_three_routes_of_the_coreas_entry_agree(tmp_path):
    """GetHorizontalDistanceToIntersectionPoint(5000 m, 1000 m, -200 m, ice 3000 m; cm arguments)
    of the drop-in driver, which prints its 9 values with 17 digits: with AIRICE_SCALAR=device (the
    one-wave kernel through the scalar slot, counted in the library's launch report) the values and
    the returned bool are the bits of query 0 of an n = 2 airice_hdtip_launch batch; with
    AIRICE_SCALAR=host (no such launch) they agree with it within 1e-12, the bound of the other
    minimizer entries (tests/test_gpu_edges.py)."""
    import torch
    from airiceraytracing_amd import AirIceSolver
    dev = torch.device("cuda:0")
    src = torch.tensor([5000e2, 20000e2], dtype=torch.float64, device=dev)
    dist = torch.tensor([1000e2, 5000e2], dtype=torch.float64, device=dev)
    depth = torch.tensor([-200e2, -300e2], dtype=torch.float64, device=dev)
    out = torch.empty((9, 2), dtype=torch.float64, device=dev)
    ok = torch.empty(2, dtype=torch.uint8, device=dev)
    AirIceSolver().hdtip_device(src, dist, depth, 3000e2, out, ok)
    torch.cuda.synchronize()
    batch, batch_ok = out.cpu().numpy()[:, 0], int(ok.cpu().numpy()[0])
    on_device, launches = _run_multiray_driver(tmp_path, "device")
    on_host, host_launches = _run_multiray_driver(tmp_path, "host")
    assert launches >= 1 and host_launches == 0
    air2ice_cases.assert_same_bits(np.array(on_device["hdtip"]), batch)
    assert on_device["hdtip_ok"] == batch_ok == on_host["hdtip_ok"]
    h = np.array(on_host["hdtip"])
    worst = float(np.max(np.abs(h - batch) / (1e-12 + 1e-12 * np.abs(batch))))
    print(f"[hdtip host vs device] worst {worst:.3e} of atol + rtol |x| at 1e-12")
    np.testing.assert_allclose(h, batch, rtol=1e-12, atol=1e-12)
