"""The argument checks of every *_launch / *_host entry of the C-ABI runtime and the in-ice table
unit, one vocabulary: a null required pointer is AIRICE_EINVAL and named, a nullable one is not
refused, a stride below n is refused with both numbers, n = 0 is AIRICE_OK, an unknown variant is
refused -- all before any HIP call, so no GPU is needed.

No call here may reach a launch or a copy: the device pointers are addresses nothing maps, and
beside the argument under test every call carries a `poison`, an argument that the entry refuses
AFTER its null and stride checks (an uninitialised medium, a stride one short, more items than
one launch holds, a negative frequency, a work buffer one byte short).  A check that went missing
therefore shows as a failed assertion, never as a kernel started on a wild address."""
import ctypes

import numpy as np
import pytest

KERNELS = ("table_kernel", "rays_kernel", "scalar_ray_kernel", "roots_kernel",
           "scalar_solve_kernel", "out_kernel", "lookup_kernel", "rtf_kernel", "single_ray_kernel",
           "path_kernel", "ray_consts_kernel", "ray_paths_kernel", "lookup_multi_kernel",
           "air2ice_kernel", "air_part_kernel", "iceray_kernel", "icesol_kernel",
           "icetab_points_kernel", "icetab_pack_kernel", "icetab_lookup_kernel")
N = 8
HUGE = 1 << 41  # items: more than one launch's 2^31 - 1 blocks of 256


def _fake(k):
    return ctypes.c_void_p(0x100000 * (k + 1))  # 128-byte aligned, never dereferenced


class Ptr:
    """A pointer argument: `name` is what the error message calls it; required or nullable
    (`pair`: the argument that is null together with it); `host`: a real array of this shape."""

    def __init__(self, name, required=True, pair=None, host=None):
        self.name, self.required, self.pair, self.host = name, required, pair, host


def R(name, host=None):
    return Ptr(name, True, host=host)


def Nl(name, pair=None, host=None):
    return Ptr(name, False, pair=pair, host=host)


def _doubles(cols=1):
    return lambda: np.zeros(cols * N)


def _grid():
    from airiceraytracing_amd import _lib
    g = _lib.Grid()
    assert _lib.lib().airice_grid_init(ctypes.byref(g), -20000.0, 300000.0, 20.0, 92.0, 180.0,
                                       0.5) == 0
    return g


def _lookup_table():
    from airiceraytracing_amd import _lib
    t = _lib.LookupTable()
    t.table, t.ld, t.n_entries = 0x100000, 1000, 1000
    t.loop_stop_height, t.height_step = 2800.0, 250.0
    t.total_height_steps, t.total_angle_steps = 100, 10
    return t


def _descs():
    """Three antennas' descriptors as airice_icetab_layout leaves them."""
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    d = np.zeros((3, 8))
    for a, (nx, nz) in enumerate(((4, 5), (7, 9), (5, 13))):
        assert L.airice_icetab_grid(-100.0, 10.0, 5.0, 20.0, nx, nz, -30.0 - a, _lib.ptr(d[a])) == 0
    size = ctypes.c_size_t(0)
    assert L.airice_icetab_layout(_lib.ptr(d), 3, ctypes.byref(size)) == 0
    return d


def _image():
    from airiceraytracing_amd import _lib
    return _lib.aligned_doubles(4096)


def _work_bytes(d):
    from airiceraytracing_amd import _lib
    size = ctypes.c_size_t(0)
    assert _lib.lib().airice_icetab_work_bytes(_lib.ptr(d), 3, ctypes.byref(size)) == 0
    return size.value


# entry -> (arguments in the C order, options).  A plain value is passed as it is; "n" and the
# names in `ld` are the item count and the strides; `poison` overrides arguments so that the call
# is refused after its null and stride checks ("medium": an uninitialised airice_medium).
M = "medium"
ENTRIES = {
    "airice_table_launch": (
        [M, ("g", _grid), ("row_begin", 0), ("row_count", 1), R("d_table"), Nl("d_full"),
         ("ld", 10**6), None], dict(poison=M, ld=["ld"], ld_n=lambda: _grid().angle_steps)),
    "airice_table_host": (
        [M, ("g", _grid), ("row_begin", 0), ("row_count", 1), R("h_table"), Nl("h_full"),
         ("ld", 10**6)], dict(poison=M, ld=["ld"], ld_n=lambda: _grid().angle_steps)),
    "airice_table_launch_multi": (
        [M, R("grids", host=_grid), ("n", 1),
         R("d_tables", host=lambda: (ctypes.c_void_p * 1)(0x100000)),
         R("lds", host=lambda: (ctypes.c_size_t * 1)(10**6)), None], dict(poison=M, n0=True)),
    "airice_rays_launch": (
        [M, R("d_launch"), R("d_txh"), 3000.0, 200.0, 1, ("n", N), R("d_out"), ("ld", N), None],
        dict(poison=M, ld=["ld"], n0=True)),
    "airice_rays_host": (
        [M, R("launch_deg", host=_doubles()), R("txh", host=_doubles()), 3000.0, 200.0, 1,
         ("n", N), R("out", host=_doubles(18)), ("ld", N)], dict(poison=M, ld=["ld"], n0=True)),
    "airice_solve_launch": (
        [M, ("variant", 0), 3000.0, R("d_txh"), R("d_dist"), R("d_depth"), Nl("d_straight_angle"),
         ("n", N), R("d_out"), ("ld", N), Nl("d_status"), None],
        dict(poison=M, ld=["ld"], n0=True, variant=True)),
    "airice_solve_host": (
        [M, ("variant", 0), 3000.0, R("txh", host=_doubles()), R("dist", host=_doubles()),
         R("depth", host=_doubles()), Nl("straight_angle", host=_doubles()), ("n", N),
         R("out", host=_doubles(17)), ("ld", N), Nl("status", host=_doubles())],
        dict(poison=dict(ld=N - 1), ld=["ld"], n0=True, variant=True)),
    "airice_hdtip_launch": (
        [M, R("d_src_cm"), R("d_dist_cm"), R("d_depth_cm"), 300000.0, ("n", N), R("d_out"),
         ("ld", N), R("d_ok"), None], dict(poison=M, ld=["ld"], n0=True)),
    "airice_table_lookup_launch": (
        [M, R("t", host=_lookup_table), R("d_src_cm"), R("d_dist_cm"), R("d_depth_cm"), 300000.0,
         ("n", N), R("d_out"), ("ld", N), R("d_ok"), R("d_flags"), None],
        dict(poison=M, ld=["ld"], n0=True)),
    "airice_table_lookup_launch_multi": (
        [M, R("tables", host=_lookup_table), ("n_tables", 1),
         R("antenna_table", host=lambda: np.zeros(1, dtype=np.int32)),
         R("antenna_depth_cm", host=lambda: np.zeros(1)), ("n_ant", 1), R("d_src_cm"),
         R("d_dist_cm"), ("ld_dist", N), 300000.0, ("n", N), R("d_out"), ("ld", N), R("d_ok"),
         R("d_flags"), R("d_work"), ("work_bytes", 1 << 20), None],
        dict(poison=M, ld=["ld", "ld_dist"], n0=True)),
    "airice_single_ray_launch": (
        [M, 200.0, 135.0, 5000.0, 3000.0, R("d_summary"), Nl("d_x", pair="d_z"),
         Nl("d_z", pair="d_x"), ("cap", 1 << 20), None], dict(poison=M)),
    "airice_single_ray_host": (
        [M, ("depth", 200.0), 135.0, 5000.0, 3000.0, R("summary", host=_doubles()),
         Nl("x", pair="z", host=_doubles()), Nl("z", pair="x", host=_doubles()), ("cap", N)],
        dict(poison=dict(depth=1e300))),  # the plan refuses 2^31 and more samples in the ice
    "airice_ray_paths_launch": (
        [M, 200.0, 3000.0, R("d_launch_deg"), R("txh_m", host=_doubles()), ("n", N),
         R("offsets", host=lambda: np.zeros(N + 1, dtype=np.int64)), R("d_work"),
         ("work_bytes", 1 << 20), R("d_summary"), ("ld", N), Nl("d_x", pair="d_z"),
         Nl("d_z", pair="d_x"), ("cap", 1 << 20), None], dict(poison=M, ld=["ld"], n0=True)),
    "airice_ray_paths_host": (
        [M, 200.0, 3000.0, R("launch_deg", host=_doubles()), R("txh_m", host=_doubles()), ("n", N),
         R("offsets", host=lambda: np.zeros(N + 1, dtype=np.int64)),
         R("summary", host=_doubles(6)), ("ld", N), Nl("x", pair="z", host=_doubles()),
         Nl("z", pair="x", host=_doubles()), ("cap", N)],
        dict(poison=dict(ld=N - 1), ld=["ld"], n0=True)),
    "airice_trace_ice_to_air_launch": (
        [M, R("d_depth"), R("d_ice"), R("d_txh"), R("d_dist"), ("n", N), R("d_out10"), None],
        dict(poison=M, n0=True)),
    "airice_trace_ice_to_air_host": (
        [M, R("depth", host=_doubles()), R("ice", host=_doubles()), R("txh", host=_doubles()),
         R("dist", host=_doubles()), ("n", N), R("out10", host=_doubles(10))],
        dict(poison=M, n0=True)),
    "airice_air2ice_launch": (
        [M, R("txh"), R("dist"), R("ice"), R("depth"), ("n", N), R("out"), ("ld", N),
         Nl("d_status"), None], dict(poison=M, ld=["ld"], n0=True)),
    "airice_air2ice_host": (
        [M, R("txh", host=_doubles()), R("dist", host=_doubles()), R("ice", host=_doubles()),
         R("depth", host=_doubles()), ("n", N), R("out", host=_doubles(16)), ("ld", N),
         Nl("status", host=_doubles())], dict(poison=dict(ld=N - 1), ld=["ld"], n0=True)),
    "airice_iceray_launch": (
        [Nl("model3", host=lambda: np.array((1.78, -0.43, 0.0132))), R("z0"), R("x1"), R("z1"),
         ("n", HUGE), R("out"), ("ld", HUGE), Nl("d_status"), None],
        dict(poison=dict(), ld=["ld"], n0=True)),
    "airice_iceray_host": (
        [Nl("model3", host=lambda: np.array((1.78, -0.43, 0.0132))), R("z0", host=_doubles()),
         R("x1", host=_doubles()), R("z1", host=_doubles()), ("n", N),
         R("out", host=_doubles(32)), ("ld", N), Nl("status", host=_doubles())],
        dict(poison=dict(ld=N - 1), ld=["ld"], n0=True)),
    "airice_icesol_launch": (
        [Nl("model3", host=lambda: np.array((1.78, -0.43, 0.0132))), R("z0"), R("x1"), R("z1"),
         R("rays"), ("ld_rays", N), Nl("d_rays_lower"), ("ld_lower", N), ("n", N), ("a0", 1.0),
         ("frequency_ghz", 0.1), R("out"), ("ld", N), Nl("d_status"), None],
        dict(poison=dict(frequency_ghz=-1.0), ld=["ld", "ld_rays", "ld_lower"], n0=True)),
    "airice_icesol_host": (
        [Nl("model3", host=lambda: np.array((1.78, -0.43, 0.0132))), R("z0", host=_doubles()),
         R("x1", host=_doubles()), R("z1", host=_doubles()), ("n", N), ("a0", 1.0),
         ("frequency_ghz", 0.1), ("focusing", 1), R("out", host=_doubles(18)), ("ld", N),
         Nl("status", host=_doubles())],
        dict(poison=dict(frequency_ghz=-1.0), ld=["ld"], n0=True)),
    "airice_icetab_build_launch": (
        [Nl("model3", host=lambda: np.array((1.78, -0.43, 0.0132))), R("image"),
         R("descs", host=_descs), ("n_ant", 3), ("a0", 1.0), ("frequency_ghz", 0.1), R("work"),
         ("work_bytes", None), None], dict(poison=dict(work_bytes=-1))),
    "airice_icetab_build_host": (
        [Nl("model3", host=lambda: np.array((1.78, -0.43, 0.0132))),
         R("image", host=_image),
         R("descs", host=_descs), ("n_ant", 3), ("a0", 1.0), ("frequency_ghz", 0.1)],
        dict(poison=dict(frequency_ghz=-1.0))),
    "airice_icetab_lookup_launch": (
        [R("image"), ("n_ant", 3), Nl("ant"), R("x"), R("z"), ("n", HUGE), R("out"), ("ld", HUGE),
         Nl("d_status"), None], dict(poison=dict(), ld=["ld"], n0=True)),
}


class _Call:
    def __init__(self, entry):
        from airiceraytracing_amd import _lib
        self._lib = _lib
        self.fn = getattr(_lib.lib(), entry)
        spec, self.opt = ENTRIES[entry]
        self.good = _lib.load_medium()
        self.blank = _lib.Medium()  # max_layers = 0: refused where the launch folds it
        self.keep = []              # the host arrays, alive for the call
        self.names, self.values, self.ptrs, hosts = [], {}, {}, {}
        for k, a in enumerate(spec):
            if a == M:
                name, v = "m", ctypes.byref(self.good)
                self.ptrs[name] = Ptr("m")
            elif isinstance(a, Ptr):
                name, v = a.name, _fake(k)
                if a.host is not None:
                    obj = hosts[name] = a.host()
                    self.keep.append(obj)
                    v = _lib.ptr(obj) if isinstance(obj, np.ndarray) else ctypes.byref(obj) \
                        if isinstance(obj, ctypes.Structure) else obj
                self.ptrs[name] = a
            elif isinstance(a, tuple):
                name, v = a
                if callable(v):
                    obj = v()
                    self.keep.append(obj)
                    v = ctypes.byref(obj)
            else:
                name, v = f"arg{k}", a
            self.names.append(name)
            self.values[name] = v
        if "work_bytes" in self.values and self.values["work_bytes"] is None:
            self.values["work_bytes"] = _work_bytes(hosts["descs"])

    def poison(self):
        p = self.opt["poison"]
        if p == M:
            return dict(m=ctypes.byref(self.blank))
        out = dict(p)
        if out.get("work_bytes") == -1:
            out["work_bytes"] = self.values["work_bytes"] - 1
        return out

    def __call__(self, poisoned=True, **kw):
        a = dict(self.values)
        if poisoned:
            a.update(self.poison())
        a.update(kw)
        before = [self._lib.launch_count(k) for k in KERNELS]
        rc = self.fn(*[a[n] for n in self.names])
        msg = self._lib.lib().airice_last_error().decode()
        assert [self._lib.launch_count(k) for k in KERNELS] == before, "a checked call launched"
        return rc, msg


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_argument_checks(entry):
    c = _Call(entry)
    opt = c.opt
    # each required pointer null in turn: AIRICE_EINVAL, and the message names it
    for name, p in c.ptrs.items():
        if p.required:
            rc, msg = c(**{name: None})
            assert rc == -1 and f"null argument ({name})" in msg, (name, rc, msg)
    # each nullable pointer (with its pair) null: the call goes on to the poison's refusal
    for name, p in c.ptrs.items():
        if not p.required:
            null = {name: None}
            if p.pair:
                null[p.pair] = None
            rc, msg = c(**null)
            assert rc != 0 and "null argument" not in msg, (name, rc, msg)
    # a stride of n - 1: refused with both numbers
    n = opt["ld_n"]() if "ld_n" in opt else c.values.get("n")
    for ld in opt.get("ld", ()):
        rc, msg = c(**{ld: n - 1})
        assert rc == -1 and f"{ld} ({n - 1})" in msg and f"({n})" in msg, (ld, rc, msg)
    # no items: AIRICE_OK whatever the pointers are (the medium is a real one)
    if opt.get("n0"):
        keep = () if entry.startswith("airice_ice") else \
            ("m", "t", "tables", "antenna_table", "antenna_depth_cm", "out")
        nulls = {name: None for name in c.ptrs if name not in keep}
        rc, msg = c(poisoned=False, n=0, **nulls)
        assert rc == 0, (rc, msg)
    # an unknown variant
    if opt.get("variant"):
        rc, msg = c(variant=7)
        assert rc == -1 and "variant 7" in msg, (rc, msg)
