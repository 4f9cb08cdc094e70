"""The multi-antenna table lookup without a GPU: airice_table_lookup_launch_multi is declared,
exported and bound; every argument it refuses is refused before any device call (dummy integers
stand for the device pointers: nothing may be dereferenced), and the antenna -> table dedupe of
AirIceSolver.antenna_tables is a pure helper."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("airice_table_lookup_launch_multi", "airice_table_lookup_multi_work_bytes")
FAKE = 0x10000  # a non-null, 16-byte aligned "device pointer"


def test_symbols_declared_exported_and_bound():
    from airiceraytracing_amd import _lib
    header = open(os.path.join(ROOT, "include", "airice.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"#define\s+AIRICE_LOOKUP_MAX_TABLES\s+32\b", header)
    assert _lib.LOOKUP_MAX_TABLES == 32
    assert len(L.airice_table_lookup_launch_multi.argtypes) == 18
    assert '"lookup_multi_kernel"' in header


def test_counter_and_timer_names():
    from airiceraytracing_amd import _lib
    assert _lib.launch_count("lookup_multi_kernel") >= 0
    ms, n = _lib.kernel_time("lookup_multi_kernel", reset=False)
    assert ms >= 0.0 and n >= 0
    cnt = ctypes.c_int64(0)
    assert _lib.lib().airice_launch_count(b"lookup_multi", ctypes.byref(cnt), 0) == -1


def test_work_bytes():
    from airiceraytracing_amd import _lib
    wb = _lib.lib().airice_table_lookup_multi_work_bytes
    assert wb(0, 4) == 0 and wb(33, 4) == 0 and wb(1, -1) == 0
    assert wb(1, 0) > 0 and wb(1, 0) % 16 == 0
    assert wb(32, 100) > wb(32, 4) > wb(3, 4) > 0
    assert wb(3, 5) % 16 == 0


class _Call:
    """A valid 3-table x 4-antenna x 10-source call whose fields a test then breaks."""

    def __init__(self):
        from airiceraytracing_amd import _lib
        self._lib = _lib
        self.medium = _lib.load_medium()
        self.n_tables, self.n_ant, self.n_src = 3, 4, 10
        self.tables = (_lib.LookupTable * 32)()
        for t in self.tables:
            t.table, t.ld, t.n_entries = FAKE, 1000, 1000
            t.loop_stop_height, t.height_step = 2800.0, 250.0
            t.total_height_steps, t.total_angle_steps = 100, 10
            t.entries = None
        self.antenna_table = np.array([0, 1, 0, 2], dtype=np.int32)
        self.depths = np.array([-20000.0, -10000.0, -20000.0, 5000.0])
        self.ld_dist, self.ld = 10, 40
        self.m = ctypes.byref(self.medium)
        self.tab = self.tables
        self.amap = _lib.ptr(self.antenna_table)
        self.dep = _lib.ptr(self.depths)
        self.src = self.dist = self.out = self.ok = self.flags = self.work = FAKE
        self.work_bytes = 1 << 20

    def __call__(self):
        L = self._lib.lib()
        before = _launches()
        rc = self._launch(L)
        assert _launches() == before, "a refused or empty call launched a kernel"
        return rc, L.airice_last_error().decode()

    def _launch(self, L):
        return L.airice_table_lookup_launch_multi(
            self.m, self.tab, self.n_tables, self.amap, self.dep, self.n_ant, self.src, self.dist,
            self.ld_dist, 300000.0, self.n_src, self.out, self.ld, self.ok, self.flags, self.work,
            self.work_bytes, None)


def _launches():
    from airiceraytracing_amd import _lib
    return _lib.launch_count("lookup_multi_kernel") + _lib.launch_count("lookup_kernel")


@pytest.mark.parametrize("field", ["m", "tab", "amap", "dep", "src", "dist", "out", "ok", "flags",
                                   "work"])
def test_null_arguments(field):
    c = _Call()
    setattr(c, field, None)
    rc, msg = c()
    assert rc == -1 and "null" in msg


@pytest.mark.parametrize("n_tables", [0, -1, 33])
def test_table_count_out_of_range(n_tables):
    c = _Call()
    c.n_tables = n_tables
    rc, msg = c()
    assert rc == -1 and "n_tables" in msg and str(n_tables) in msg


@pytest.mark.parametrize("value", [-1, 3])
def test_antenna_table_out_of_range(value):
    c = _Call()
    c.antenna_table[2] = value
    rc, msg = c()
    assert rc == -1 and "antenna_table[2]" in msg


def test_strides_too_short():
    c = _Call()
    c.ld_dist = 9
    rc, msg = c()
    assert rc == -1 and "ld_dist" in msg
    c = _Call()
    c.ld = 39
    rc, msg = c()
    assert rc == -1 and "ld (39)" in msg


@pytest.mark.parametrize("field,value", [("table", None), ("n_entries", 0), ("ld", 999),
                                         ("total_angle_steps", 0), ("total_height_steps", 0),
                                         ("height_step", 0.0), ("height_step", float("nan")),
                                         ("entries", FAKE + 8)])
def test_invalid_table_description_names_the_table(field, value):
    """The conditions of airice_table_lookup_launch, checked per table: table 1 of 3 is broken."""
    from airiceraytracing_amd import _lib
    c = _Call()
    setattr(c.tables[1], field, value)
    rc, msg = c()
    assert rc == -1 and "tables[1]" in msg, msg
    # the single-antenna launch refuses the same description
    rc1 = _lib.lib().airice_table_lookup_launch(c.m, ctypes.byref(c.tables[1]), FAKE, FAKE, FAKE,
                                                300000.0, 10, FAKE, 10, FAKE, FAKE, None)
    assert rc1 == -1
    # a table the call does not read is not checked
    c = _Call()
    setattr(c.tables[3], field, value)
    c.n_ant = 0
    assert c()[0] == 0


def test_workspace_too_small_or_misaligned():
    from airiceraytracing_amd import _lib
    c = _Call()
    need = _lib.lib().airice_table_lookup_multi_work_bytes(3, 4)
    c.work_bytes = need - 1
    rc, msg = c()
    assert rc == -1 and "workspace" in msg and str(need) in msg
    c = _Call()
    c.work = FAKE + 8
    rc, msg = c()
    assert rc == -1 and "workspace" in msg


def test_empty_batches_are_ok_and_launch_nothing():
    c = _Call()
    c.n_ant = 0
    c.ld = 0
    assert c()[0] == 0
    c = _Call()
    c.n_src = 0
    c.ld = c.ld_dist = 0
    c.src = c.dist = c.out = c.ok = c.flags = c.work = None
    assert c()[0] == 0


def test_dedupe_depths():
    from airiceraytracing_amd import dedupe_depths
    distinct, antenna_table = dedupe_depths([-20000, -10000, -20000, 5000])
    assert distinct == [-20000.0, -10000.0, 5000.0]
    assert antenna_table == [0, 1, 0, 2]
    assert dedupe_depths([]) == ([], [])
    # exact equality, as the reference compares AntennaDepths (.cc:1350)
    d, t = dedupe_depths(np.array([-100.0, np.nextafter(-100.0, 0.0), -100.0]))
    assert len(d) == 2 and t == [0, 1, 0]


def test_python_wrapper_checks_shapes():
    """table_lookup_multi_device refuses a distance tensor that is not (n_ant, n_src) before it
    calls the library."""
    import torch
    from airiceraytracing_amd import AirIceSolver
    s = AirIceSolver()
    c = _Call()
    src = torch.zeros(10, dtype=torch.float64)
    with pytest.raises(ValueError):
        s.table_lookup_multi_device(list(c.tables[:3]), [0, 1, 0, 2], c.depths, src,
                                    torch.zeros((3, 10), dtype=torch.float64), 300000.0, None,
                                    None, None)
    with pytest.raises(ValueError):
        s.table_lookup_multi_device(list(c.tables[:3]), [0, 1, 0, 2], c.depths[:3], src,
                                    torch.zeros((4, 10), dtype=torch.float64), 300000.0, None,
                                    None, None)
