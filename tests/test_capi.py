"""CPU tests of the drop-in boundary: libairice.so loads, exports every symbol include/airice.h
declares, and its host-side pieces (GDAS ingestion, grid set-up, error codes) agree with the
oracle.  No kernel is launched here (no GPU in this container)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from tests.conftest import ROOT


def header_functions(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?[A-Za-z_][A-Za-z0-9_]*\s*\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*\(",
                       text, flags=re.M)
    return sorted(set(n for n in names if n not in ("if", "while", "for", "return")))


def test_library_exports_every_header_symbol():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    declared = header_functions(os.path.join(ROOT, "include", "airice.h"))
    assert "airice_table_launch" in declared and "Py_TraceIceToAir" in declared
    for name in declared:
        assert hasattr(L, name), name
    assert sorted(declared) == sorted(_lib.EXPORTED_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in nm.splitlines() if " T " in ln)
    assert set(declared) <= exported


def test_library_is_gfx950_code_object():
    from airiceraytracing_amd import _lib
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-n", _lib.LIB_PATH],
                         capture_output=True, text=True)
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in blob or b"amdgcn-amd-amdhsa--gfx950" in blob


def test_host_atmosphere_matches_oracle_bitwise(atmosphere_text, oracle_medium):
    from airiceraytracing_amd import _lib
    m = _lib.Medium()
    _lib.check(_lib.lib().airice_atmosphere_parse(atmosphere_text, len(atmosphere_text), 0,
                                                   ctypes.byref(m)), "parse")
    assert m.max_layers == oracle_medium.max_layers == 4
    assert m.n_points == oracle_medium.n_points
    assert m.N0 == oracle_medium.N0
    for i in range(5):
        assert m.B_air[i] == oracle_medium.B_air[i]
        assert m.C_air[i] == oracle_medium.C_air[i]
        assert m.atmlay_cm[i] == oracle_medium.atmlay[i]
    assert m.pi == 3.1415927
    for z in (0.0, 10.0, 2999.0, 3217.48275, 5000.0, 23141.7538, 80000.0, -150.0):
        assert _lib.lib().airice_nz_air(ctypes.byref(m), z) == oracle.getnz_air(oracle_medium, z)
        assert _lib.lib().airice_nz_ice(ctypes.byref(m), z) == oracle.getnz_ice(oracle_medium, z)


def test_pywrapper_variant_uses_exact_pi(atmosphere_text):
    from airiceraytracing_amd import _lib
    m = _lib.Medium()
    _lib.check(_lib.lib().airice_atmosphere_parse(atmosphere_text, len(atmosphere_text), 1,
                                                   ctypes.byref(m)), "parse")
    assert m.pi == np.pi


@pytest.mark.parametrize("args", [
    (-20000.0, 300000.0, 20.0, 92.0, 180.0, 0.5),
    (-20000.0, 300000.0, 10.0, 90.1, 180.0, 0.1),
    (+5000.0, 300000.0, 7.0, 91.0, 179.0, 0.3),
    (-100.0, 250000.0, 1.0, 90.1, 180.0, 0.01),
])
def test_grid_init_matches_oracle(args):
    from airiceraytracing_amd import make_grid
    g = make_grid(*args)
    og = oracle.grid_init(*args)
    for f in ("start_height", "stop_height", "height_step", "height_steps", "start_angle",
              "stop_angle", "angle_step", "angle_steps", "depth_m", "ice_m", "in_ice",
              "table_rows"):
        assert getattr(g, f) == getattr(og, f), f


@pytest.mark.parametrize("depth_cm,ice_cm,step,rows,kept", [
    (-20000.0, 300000.0, 20.0, 4851, 4851),  # cfg2: every Tx height > 0
    (-20000.0, 0.0, 20.0, 5001, 5000),       # sea-level ice: the Tx = 0 row is skipped
    (+5000.0, 0.0, 10.0, 9996, 9996),        # Rx 50 m in the air above sea-level ice: stop 50 m
    (-100.0, -150000.0, 1000.0, 102, 100),   # ice 1.5 km below sea level: Tx 0 and -1000 skipped
    (-100.0, -100.0, 3.0, 33334, 33334),     # last row kept (unforced Tx 1 m) and forced to -1 m
])
def test_grid_skips_nonpositive_tx_rows(depth_cm, ice_cm, step, rows, kept):
    """MakeRayTracingTable pushes no entries for rows whose Tx height is not > 0 (.cc:2082):
    the table holds the leading table_rows rows while TotalHeightSteps keeps its value."""
    from airiceraytracing_amd import make_grid
    g = make_grid(depth_cm, ice_cm, step, 92.0, 180.0, 0.5)
    og = oracle.grid_init(depth_cm, ice_cm, step, 92.0, 180.0, 0.5)
    assert (g.height_steps, g.table_rows) == (rows, kept)
    assert (og.height_steps, og.table_rows) == (rows, kept)
    assert g.n_rays == og.n_rays == kept * g.angle_steps
    # the oracle's table is the reference's shorter table
    m = oracle.load_atmosphere(os.path.join(ROOT, "airiceraytracing_amd", "data",
                                            "Atmosphere.dat.gz"))
    t = oracle.table_rows(m, og, max(0, rows - 3), rows)
    assert t.shape == (11, max(0, kept - max(0, rows - 3)) * og.angle_steps)


def test_error_codes():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    m = _lib.Medium()
    rc = L.airice_atmosphere_load(b"/nonexistent/Atmosphere.dat", 0, ctypes.byref(m))
    assert rc == -2 and b"cannot open" in L.airice_last_error()
    g = _lib.Grid()
    assert L.airice_grid_init(ctypes.byref(g), -100.0, 300000.0, 0.0, 90.1, 180.0, 0.1) == -1
    # uninitialised medium is rejected before any device work
    assert L.airice_table_launch(ctypes.byref(m), ctypes.byref(g), 0, 1, None, None, 1, None) == -1
    assert L.airice_rays_launch(ctypes.byref(m), None, None, 3000.0, -200.0, 1, 0, None, 0,
                                None) == -1
    # row range outside the grid
    good = _lib.load_medium()
    assert L.airice_grid_init(ctypes.byref(g), -20000.0, 300000.0, 20.0, 92.0, 180.0, 0.5) == 0
    assert L.airice_table_launch(ctypes.byref(good), ctypes.byref(g), 4850, 2, None, None,
                                 10**6, None) == -1
    assert b"outside grid" in L.airice_last_error()
    # unknown variant
    assert L.airice_solve_launch(ctypes.byref(good), 7, 3000.0, None, None, None, None, 0, None,
                                 0, None, None) == -1


def test_one_query_host_calls_reject_null_arguments():
    """The n == 1 host routes (AIRICE_SCALAR_HOST) keep the C-ABI's error contract: a null medium
    or a null input / output pointer is AIRICE_EINVAL, never a dereference."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    L = _lib.lib()
    good = _lib.load_medium()
    one = np.array([5000.0])
    out = np.zeros(_lib.SOLVE_FIELDS)
    st = np.zeros(1, dtype=np.uint8)
    p = _lib.ptr
    with scalar_mode(_lib.SCALAR_HOST):
        assert L.airice_solve_host(None, 0, 3000.0, p(one), p(one), p(one), None, 1, p(out), 1,
                                   p(st)) == -1
        assert b"null" in L.airice_last_error()
        for args in ((None, p(one), p(one)), (p(one), None, p(one)), (p(one), p(one), None)):
            assert L.airice_solve_host(ctypes.byref(good), 0, 3000.0, *args, None, 1, p(out), 1,
                                       p(st)) == -1
        assert L.airice_solve_host(ctypes.byref(good), 0, 3000.0, p(one), p(one), p(one), None, 1,
                                   None, 1, p(st)) == -1
        out10 = np.zeros(10)
        assert L.airice_trace_ice_to_air_host(None, p(one), p(one), p(one), p(one), 1,
                                              p(out10)) == -1
        assert L.airice_trace_ice_to_air_host(ctypes.byref(good), p(one), None, p(one), p(one), 1,
                                              p(out10)) == -1
        assert L.airice_trace_ice_to_air_host(ctypes.byref(good), p(one), p(one), p(one), p(one),
                                              1, None) == -1
        assert L.airice_rtf_eval(None, 3, p(np.array([170.0, 20000.0, 3000.0])), 3, p(out),
                                 out.size) == -1


def test_launch_counters():
    """airice_launch_count: every documented name answers -- 0 on a box without a GPU, where no
    kernel can have run; on a GPU box, where earlier tests of the same process may have launched
    kernels, the count they left, which a reset hands back and takes to 0 --, an unknown one is
    AIRICE_EINVAL."""
    import torch
    from airiceraytracing_amd import _lib
    gpu = torch.cuda.is_available()
    for name in ("table_kernel", "rays_kernel", "scalar_ray_kernel", "roots_kernel",
                 "scalar_solve_kernel", "out_kernel", "lookup_kernel", "rtf_kernel",
                 "single_ray_kernel", "path_kernel"):
        n = _lib.launch_count(name)
        assert n >= 0 if gpu else n == 0, name
        assert _lib.launch_count(name, reset=True) == n, name
        assert _lib.launch_count(name) == 0, name
    cnt = ctypes.c_int64(7)
    assert _lib.lib().airice_launch_count(b"no_such_kernel", ctypes.byref(cnt), 0) == -1
    # the one-query host route launches nothing
    from airiceraytracing_amd.solver import AirIceSolver, scalar_mode
    s = AirIceSolver()
    with scalar_mode(_lib.SCALAR_HOST), _lib.launched("scalar_solve_kernel") as k:
        out, st = s.solve_host(np.array([5000.0]), np.array([1000.0]), np.array([-200.0]), 3000.0)
    assert k.count == 0 and abs(out[10, 0] - 154.70167146999108) < 1e-9 * 155


def test_no_cpu_fallback_when_library_missing(monkeypatch, tmp_path):
    from airiceraytracing_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libairice.so"))
    with pytest.raises(_lib.AirIceLibraryError):
        _lib.lib()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "airiceraytracing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "airice_oracle" not in src, f


# The MultiRayAirIceRefraction.h surface of the reference (its .h:26-204), as demangled
# signatures: every function a caller of the reference can link against, bar the deprecated
# MakeTable / GetInterpolatedValue (.cc:1618-1794).
MULTIRAY_FUNCTIONS = [
    "FindFunctionRoot(gsl_function_struct, double, double, gsl_root_fsolver_type const*, double)",
    "readATMpar()", "readnhFromFile()", "GetB_ice(double)", "GetC_ice(double)",
    "Getnz_ice(double)", "FillInAirRefractiveIndex()", "GetB_air(double)", "GetC_air(double)",
    "Getnz_air(double)", "Refl_S(double, double)", "Trans_S(double, double)",
    "Refl_P(double, double)", "Trans_P(double, double)", "fDnfR(double, void*)",
    "ftimeD(double, void*)", "fpathD(double, void*)",
    "GetRayHorizontalPath(double, double, double, double, int)",
    "GetRayPropagationTime(double, double, double, double, int)",
    "GetRayGeometricPath(double, double, double, double, int)",
    "GetLayerHitPointPar(double, double, double, double, int)", "MakeAtmosphere()",
    "GetAirPropagationPar(double, double, double)",
    "GetIcePropagationPar(double, double, double, double)",
    "MinimizeforLaunchAngle(double, void*)",
    "GetHorizontalDistanceToIntersectionPoint(double, double, double, double, double&, double&, "
    "double&, double&, double&, double&, double&, double&, double&)",
    "oneDLinearInterpolation(double, double, double, double, double)",
    "Extrapolate(int, int, double, int)", "FindExtrapolationLimit(int, double, int)",
    "FindClosestAirTxHeight(double, int&, int&, double&, int&, int&, double&, int)",
    "FindClosestTHD(double, int, int, int&, int&, double&, int)",
    "GetParValues(double, double, double, double, double&, double*, double&, double*)",
    "GetHorizontalDistanceToIntersectionPoint_Table(double, double, double, double, int, double&, "
    "double&, double&, double&, double&, double&, double&, double&, double&)",
    "Air2IceRayTracing(double, double, double, double, double, double*)",
    "GetRayTracingSolutions(double, double, double, double, double*, bool&)",
    "MakeRayTracingTable(double, double, int)",
]
MULTIRAY_DATA = ["nh_data", "lognh_data", "h_data", "GridPositionH", "GridPositionTh",
                 "GridZValue", "GridStartTh", "GridStopTh", "GridStepSizeH_O", "GridStepSizeTh_O",
                 "GridWidthH", "GridWidthTh", "GridPoints", "TotalStepsH_O", "TotalStepsTh_O",
                 "GridStartH", "GridStopH", "ATMLAY", "abc", "C_air", "B_air", "A_ice", "B_ice",
                 "C_ice", "MaxLayers"]
GLOBAL_DATA = ["MaxAirTxHeight", "MinAirTxHeight", "AllTableAllAntData", "AngleStepSize",
               "LoopStartAngle", "LoopStopAngle", "TotalAngleSteps", "HeightStepSize",
               "LoopStartHeight", "LoopStopHeight", "TotalHeightSteps"]


def test_multiray_dropin_exports_the_reference_surface():
    """nm -D of libairice.so holds every function and namespace variable of the reference's
    MultiRayAirIceRefraction.h under its mangled name; the caller-owned AntennaDepths /
    AntennaTableAlreadyMade are weak references (the library loads without them)."""
    from airiceraytracing_amd import _lib
    out = subprocess.run(["nm", "-DC", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    defined, weak = set(), set()
    for ln in out.splitlines():
        parts = ln.split(None, 2)
        if len(parts) == 3 and parts[1] in "TDBR":
            defined.add(parts[2].strip())
        elif len(parts) == 2 and parts[0] == "w":
            weak.add(parts[1].strip())
    ns = "MultiRayAirIceRefraction::"
    missing = [f for f in MULTIRAY_FUNCTIONS if ns + f not in defined]
    assert not missing, missing
    assert any(s.startswith(ns + "flatten(std::vector<std::vector<double") for s in defined)
    assert not [v for v in MULTIRAY_DATA if ns + v not in defined]
    assert not [v for v in GLOBAL_DATA if v not in defined]
    assert {"AntennaDepths", "AntennaTableAlreadyMade"} <= weak


# The exported text symbols of the reference's prebuilt pythonwrapper/libAirIceRayTracing.so
# (nm -D --defined-only, its own std:: template instantiations left out): the AirIceRayTracing::
# namespace of pythonwrapper/AirIceRayTracing.h:23-146, the C++ TraceIceToAir (TraceIceToAir.C:5)
# and the ctypes entry Py_TraceIceToAir (TraceIceToAir.C:75-79).
PYWRAPPER_SYMBOLS = """
Py_TraceIceToAir _Z13TraceIceToAirddddPd
_ZN16AirIceRayTracing10readATMparENSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE
_ZN16AirIceRayTracing14MakeAtmosphereENSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE
_ZN16AirIceRayTracing14readnhFromFileENSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE
_ZN16AirIceRayTracing16FindFunctionRootE19gsl_function_structddPK21gsl_root_fsolver_typedi
_ZN16AirIceRayTracing17Air2IceRayTracingEdddddPd _ZN16AirIceRayTracing19GetLayerHitPointParEddddi
_ZN16AirIceRayTracing19GetRayGeometricPathEddddi _ZN16AirIceRayTracing20GetAirPropagationParEddd
_ZN16AirIceRayTracing20GetIcePropagationParEdddd _ZN16AirIceRayTracing20GetRayHorizontalPathEddddi
_ZN16AirIceRayTracing21GetRayPropagationTimeEddddi
_ZN16AirIceRayTracing21GetRayTracingSolutionEddddRdS0_S0_S0_S0_S0_S0_S0_
_ZN16AirIceRayTracing22MinimizeforLaunchAngleEdPv _ZN16AirIceRayTracing24FillInAirRefractiveIndexEv
_ZN16AirIceRayTracing5fDnfREdPv _ZN16AirIceRayTracing6Refl_PEdd _ZN16AirIceRayTracing6Refl_SEdd
_ZN16AirIceRayTracing6fpathDEdPv _ZN16AirIceRayTracing6ftimeDEdPv _ZN16AirIceRayTracing7Trans_PEdd
_ZN16AirIceRayTracing7Trans_SEdd _ZN16AirIceRayTracing7flattenERKSt6vectorIS0_IdSaIdEESaIS2_EE
_ZN16AirIceRayTracing8GetB_airEd _ZN16AirIceRayTracing8GetB_iceEd _ZN16AirIceRayTracing8GetC_airEd
_ZN16AirIceRayTracing8GetC_iceEd _ZN16AirIceRayTracing9Getnz_airEd _ZN16AirIceRayTracing9Getnz_iceEd
""".split()
PYWRAPPER_DATA = ["nh_data", "lognh_data", "h_data", "ATMLAY", "abc", "C_air", "B_air",
                  "MaxLayers", "UseConstantRefractiveIndex", "A_air", "A_const"]


def test_pywrapper_dropin_exports_the_reference_symbols():
    """Every symbol the reference's libAirIceRayTracing.so exports is defined by libairice.so
    under the same mangled name, so a C++ object built against pythonwrapper/AirIceRayTracing.h
    (or a ctypes user of Py_TraceIceToAir) relinks unchanged; the namespace data is exported too
    (include/AirIceRayTracing.h: one shared copy instead of the reference's header statics)."""
    from airiceraytracing_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3}
    assert len(PYWRAPPER_SYMBOLS) == 30
    missing = [s for s in PYWRAPPER_SYMBOLS if s not in syms]
    assert not missing, missing
    dem = subprocess.run(["nm", "-DC", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    data = {ln.split(None, 2)[2].strip() for ln in dem.splitlines()
            if len(ln.split(None, 2)) == 3 and ln.split(None, 2)[1] in "DB"}
    assert not [v for v in PYWRAPPER_DATA if "AirIceRayTracing::" + v not in data]
    # and the GSL-typed FindFunctionRoot of the two other namespaces
    for ns in ("_ZN24MultiRayAirIceRefraction", "_ZN19RayTracingFunctions"):
        assert ns + "16FindFunctionRootE19gsl_function_structddPK21gsl_root_fsolver_typed" in syms


def test_lookup_pack_rejects_empty_angle_grid():
    """airice_lookup_pack validates the row length before folding row records: a
    zero TotalAngleSteps or an empty table is AIRICE_EINVAL, not a division by zero.  No device
    memory is touched (the pointers are never dereferenced), so this runs on the CPU."""
    import ctypes
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import AirIceSolver
    L = _lib.lib()
    for n, asteps in ((100, 0), (0, 10)):
        t = _lib.LookupTable()
        t.table = 0x10000
        t.ld = max(n, 1)
        t.n_entries = n
        t.loop_stop_height, t.height_step = 3000.0, 10.0
        t.total_height_steps, t.total_angle_steps = 10, asteps
        rc = L.airice_lookup_pack(ctypes.byref(t), ctypes.c_void_p(0x20000), 1 << 20, None)
        assert rc == -1, rc  # AIRICE_EINVAL
        assert b"total_angle_steps" in L.airice_last_error()
        assert L.airice_lookup_pack_floats(n, asteps) == 0
        with pytest.raises(ValueError):
            AirIceSolver.lookup_pack(t)


def test_lookup_pack_checks_capacity():
    """Pack format 2 (library 0.2) changed the packed copy's size: the pack takes the
    buffer's capacity and refuses one sized for another format (format 1's 32-float records are
    larger, but a caller with a smaller buffer -- or a stale AIRICE_LOOKUP_PACK_FLOATS -- must get
    AIRICE_EINVAL, never a write past the end).  No device memory is touched."""
    import ctypes
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    assert b"0.2.0" in L.airice_version() and b"pack format 2" in L.airice_version()
    n, asteps = 858627, 177
    need = L.airice_lookup_pack_floats(n, asteps)
    assert need == _lib.lookup_pack_floats(n, asteps)
    assert need == _lib.lookup_rows_offset(n) + (n // asteps) * 64 + 180 + 4
    t = _lib.LookupTable()
    t.table, t.ld, t.n_entries = 0x10000, n, n
    t.loop_stop_height, t.height_step = 3000.0, 20.0
    t.total_height_steps, t.total_angle_steps = n // asteps, asteps
    rc = L.airice_lookup_pack(ctypes.byref(t), ctypes.c_void_p(0x20000), need - 1, None)
    assert rc == -1, rc
    assert b"pack format 2" in L.airice_last_error()
