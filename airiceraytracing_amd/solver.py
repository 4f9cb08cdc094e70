"""Batched host API over libairice.so.

Two flavours of every entry point:
  * ``*_device``: inputs/outputs already resident in HBM (torch CUDA tensors or raw
    device pointers), stream-ordered, asynchronous -- the path ``bench.py`` times;
  * ``*_host``: numpy in, numpy out (the library copies, launches, synchronises).

Layouts follow the reference: the table is 11 float columns
(``AllTableAllAntData[ant][col][row]``, MultiRayAirIceRefraction.cc:2101-2111), ray and
solve outputs are the reference ``dummy[]`` slots as double columns.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (Grid, LookupTable, Medium, VARIANT_MULTIRAY, VARIANT_PYWRAPPER, check, lib,
                   ptr)


def make_grid(antenna_depth_cm: float, ice_height_cm: float, height_step: float = 10.0,
              start_angle: float = 90.1, stop_angle: float = 180.0,
              angle_step: float = 0.1) -> Grid:
    """MakeRayTracingTable grid (MultiRayAirIceRefraction.cc:12-21, 2019-2061).  Defaults are
    the reference's globals (10 m x 0.1 deg, 90.1..180 deg, 100 km down to the ice)."""
    g = Grid()
    check(lib().airice_grid_init(ctypes.byref(g), antenna_depth_cm, ice_height_cm, height_step,
                                 start_angle, stop_angle, angle_step), "airice_grid_init")
    return g


class scalar_mode:
    """Where the one-query ray and ray-layer calls run (airice_scalar_mode), for a ``with`` block:
    _lib.SCALAR_HOST (the library's default) or _lib.SCALAR_DEVICE."""

    def __init__(self, mode: int):
        self.mode = mode
        self.prev = None

    def __enter__(self):
        self.prev = lib().airice_scalar_mode(self.mode)
        return self

    def __exit__(self, *exc):
        lib().airice_scalar_mode(self.prev)
        return False


def _stream_handle(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)  # torch.cuda.Stream


def dedupe_depths(depths_cm):
    """The reference's antenna -> table remap (MultiRayAirIceRefraction.cc:1348-1352): antennas at
    exactly the same depth share the table of the first of them.  Returns (the distinct depths in
    first-seen order, antenna_table: each antenna's index into them)."""
    distinct: list[float] = []
    antenna_table: list[int] = []
    for d in (float(x) for x in depths_cm):
        if d not in distinct:
            distinct.append(d)
        antenna_table.append(distinct.index(d))
    return distinct, antenna_table


class AntennaTables:
    """What ``AirIceSolver.antenna_tables`` returns: the distinct antennas' packed device tables
    (``tables``: LookupTable descriptions, ``buffers``: their 11 x n float32 tensors, ``grids``),
    ``antenna_table`` (each antenna's index into them) and ``depths_cm``.  ``firn``: the two-layer
    firn the tables were traced in, or None."""

    def __init__(self, solver, ice_cm, grids, buffers, tables, antenna_table, depths_cm,
                 firn=None):
        self.solver = solver
        self.ice_cm = float(ice_cm)
        self.grids = grids
        self.buffers = buffers
        self.tables = tables
        self.antenna_table = list(antenna_table)
        self.depths_cm = [float(d) for d in depths_cm]
        self.firn = firn

    def lookup(self, src_cm, dist_cm, stream=None):
        """GetHorizontalDistanceToIntersectionPoint_Table of every (antenna, source) pair in one
        launch: ``src_cm`` (n_src) and ``dist_cm`` (n_ant, n_src) float64 device tensors.  Returns
        (out (9, n_ant, n_src) float64, ok (n_ant, n_src) uint8, flags (n_ant, n_src) uint8).
        With a firn the minimizer fallback is not available (it is one-layer): lanes flagged
        LOOKUP_FALLBACK come back as NaN with ok = 0."""
        import torch
        n_ant, n_src = len(self.depths_cm), int(src_cm.numel())
        dev = src_cm.device
        out = torch.empty((9, n_ant, n_src), dtype=torch.float64, device=dev)
        ok = torch.empty((n_ant, n_src), dtype=torch.uint8, device=dev)
        flags = torch.empty((n_ant, n_src), dtype=torch.uint8, device=dev)
        self.solver.table_lookup_multi_device(self.tables, self.antenna_table, self.depths_cm,
                                              src_cm, dist_cm, self.ice_cm, out, ok, flags,
                                              stream=stream)
        if self.firn is not None:
            import contextlib
            ctx = contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)
            with ctx:
                fb = (flags & _lib.LOOKUP_FALLBACK) != 0
                out.masked_fill_(fb.unsqueeze(0), float("nan"))
                ok.masked_fill_(fb, 0)
        return out, ok, flags


class IceTables:
    """The in-ice interpolation tables of some antennas (IceRayTracing::MakeTable): one image of
    float64 on the device -- ``image``, laid out as include/airice.h says -- and its descriptors
    ``descs`` ((n_ant, 8) numpy: x_start, z_start, x_step, z_step, nx, nz, first_record,
    rx_depth).  ``lookup`` is IceRayTracing::GetInterpolatedValue for all 13 parameters of many
    points in one launch."""

    def __init__(self, image, descs):
        self.image = image
        self.descs = descs
        self.n_ant = int(descs.shape[0])
        self._host = None

    def lookup(self, x, z, ant=None, out=None, status=None, ld: int | None = None, stream=None):
        """airice_icetab_lookup_launch on device tensors: ``x``, ``z`` (n float64), ``ant`` (n
        int32, None: antenna 0); parameter c of query i lands at ``out[c, i]`` (13 x ld float64,
        allocated when None), ``status`` (n uint8, optional) takes the _lib.ICETAB_* bits.
        Stream-ordered; returns ``out``."""
        import torch
        n = int(x.numel())
        if out is None:
            out = torch.empty((_lib.ICETAB_PARAMS, n if ld is None else ld), dtype=torch.float64,
                              device=x.device)
        check(lib().airice_icetab_lookup_launch(
            ptr(self.image), self.n_ant, ptr(ant), ptr(x), ptr(z), n, ptr(out),
            int(out.stride(0)) if ld is None else ld, ptr(status), _stream_handle(stream)),
            "airice_icetab_lookup_launch")
        return out

    def host_image(self) -> np.ndarray:
        """The image in host memory (aligned; copied from the device once and kept)."""
        if self._host is None:
            import torch
            torch.cuda.synchronize(self.image.device)
            h = _lib.aligned_doubles(int(self.image.numel()))
            check(lib().airice_memcpy_d2h(ptr(h), ptr(self.image), h.nbytes), "airice_memcpy_d2h")
            self._host = h
        return self._host

    def lookup_host(self, x, z, ant=None):
        """airice_icetab_lookup_host: numpy in, (out (13, n), status (n) uint8) out, on the calling
        thread against ``host_image()``."""
        return icetab_lookup_host(self.host_image(), self.n_ant, x, z, ant)

    def values(self, ant: int) -> np.ndarray:
        """Antenna ``ant``'s table as the reference's 13 columns: a (13, nx, nz) numpy array."""
        return icetab_values(self.host_image(), self.descs, ant)


def icetab_descs(grids) -> tuple[np.ndarray, int]:
    """(n_ant, 8) descriptors with first_record filled (airice_icetab_layout) and the image's
    size in doubles."""
    d = np.array(grids, dtype=np.float64).reshape(-1, _lib.ICETAB_DESC)
    d = np.ascontiguousarray(d)
    size = ctypes.c_size_t(0)
    check(lib().airice_icetab_layout(ptr(d), d.shape[0], ctypes.byref(size)),
          "airice_icetab_layout")
    return d, int(size.value)


def icetab_grid(x_start, z_start, x_step, z_step, nx, nz, rx_depth) -> np.ndarray:
    """airice_icetab_grid: the 8-double descriptor of any grid (first_record 0 until a layout)."""
    d = np.zeros(_lib.ICETAB_DESC, dtype=np.float64)
    check(lib().airice_icetab_grid(float(x_start), float(z_start), float(x_step), float(z_step),
                                   int(nx), int(nz), float(rx_depth), ptr(d)),
          "airice_icetab_grid")
    return d


def icetab_grid_init(shower_hit_distance, shower_depth, rx_depth) -> np.ndarray:
    """airice_icetab_grid_init: MakeTable's own 401 x 201 grid around the shower."""
    d = np.zeros(_lib.ICETAB_DESC, dtype=np.float64)
    check(lib().airice_icetab_grid_init(float(shower_hit_distance), float(shower_depth),
                                        float(rx_depth), ptr(d)), "airice_icetab_grid_init")
    return d


def icetab_image_from_values(descs, values) -> tuple[np.ndarray, np.ndarray]:
    """The host image (aligned) of tables given as the reference's columns: ``values[a]`` is
    (13, nx, nz).  Slots 13..15 of every record are 0.  Returns (image, descs with layout)."""
    d, size = icetab_descs(descs)
    image = _lib.aligned_doubles(size)
    image[:d.size] = d.ravel()
    for a in range(d.shape[0]):
        nx, nz, first = int(d[a, 4]), int(d[a, 5]), int(d[a, 6])
        v = np.asarray(values[a], dtype=np.float64).reshape(_lib.ICETAB_PARAMS, nx * nz)
        rec = image[first * _lib.ICETAB_RECORD:(first + nx * nz) * _lib.ICETAB_RECORD]
        rec.reshape(nx * nz, _lib.ICETAB_RECORD)[:, :_lib.ICETAB_PARAMS] = v.T
    return image, d


def icetab_values(image, descs, ant: int) -> np.ndarray:
    nx, nz, first = int(descs[ant, 4]), int(descs[ant, 5]), int(descs[ant, 6])
    rec = np.asarray(image)[first * _lib.ICETAB_RECORD:(first + nx * nz) * _lib.ICETAB_RECORD]
    rec = rec.reshape(nx * nz, _lib.ICETAB_RECORD)
    return np.ascontiguousarray(rec[:, :_lib.ICETAB_PARAMS].T).reshape(_lib.ICETAB_PARAMS, nx, nz)


def icetab_lookup_host(image, n_ant: int, x, z, ant=None):
    """airice_icetab_lookup_host on a host image (128-byte aligned numpy float64)."""
    arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (x, z)])
    xs, zs = [np.ascontiguousarray(v).ravel() for v in arrs]
    n = xs.size
    a = None
    if ant is not None:
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(ant, dtype=np.int32), xs.shape))
    out = np.empty((_lib.ICETAB_PARAMS, n), dtype=np.float64)
    st = np.empty(n, dtype=np.uint8)
    check(lib().airice_icetab_lookup_host(ptr(image), n_ant, ptr(a), ptr(xs), ptr(zs), n, ptr(out),
                                          max(n, 1), ptr(st)), "airice_icetab_lookup_host")
    return out, st


def icetab_pack_host(sol, status) -> np.ndarray:
    """airice_icetab_pack_host: (18, n) solution columns and n status bytes -> (n, 16) records."""
    sol = np.ascontiguousarray(sol, dtype=np.float64)
    status = np.ascontiguousarray(status, dtype=np.uint8)
    n = sol.shape[1]
    rec = np.empty((n, _lib.ICETAB_RECORD), dtype=np.float64)
    check(lib().airice_icetab_pack_host(ptr(sol), max(n, 1), ptr(status), n, ptr(rec)),
          "airice_icetab_pack_host")
    return rec


class AirIceSolver:
    """One medium (parsed GDAS atmosphere + ice model) and the batched GPU entry points."""

    def __init__(self, atmosphere: str | None = None, variant: int = VARIANT_MULTIRAY):
        self.variant = variant
        self.medium: Medium = _lib.load_medium(atmosphere, variant)

    # ------------------------------------------------------------------ table
    def table_device(self, grid: Grid, table, full=None, row_begin: int = 0,
                     row_count: int | None = None, ld: int | None = None, stream=None,
                     firn=None) -> None:
        """airice_table_launch; with ``firn`` (a ``Firn``) airice_table_launch_firn: the two-layer
        firn, this medium's A_ice with the firn's B and C."""
        if row_count is None:
            row_count = grid.table_rows - row_begin
        n = row_count * grid.angle_steps
        ld = n if ld is None else ld
        if firn is not None:
            check(lib().airice_table_launch_firn(ctypes.byref(self.medium), ctypes.byref(firn),
                                                 ctypes.byref(grid), row_begin, row_count,
                                                 ptr(table), ptr(full), ld,
                                                 _stream_handle(stream)),
                  "airice_table_launch_firn")
            return
        check(lib().airice_table_launch(ctypes.byref(self.medium), ctypes.byref(grid), row_begin,
                                        row_count, ptr(table), ptr(full), ld,
                                        _stream_handle(stream)), "airice_table_launch")

    def tables_device(self, grids, tables, stream=None, firn=None) -> None:
        """Several antennas' whole tables in one launch (airice_table_launch_multi): grids[a] and
        tables[a] (11 x >= grids[a].n_rays float32 device tensors, one per antenna)."""
        n = len(grids)
        garr = (Grid * n)(*grids)
        ptrs = (ctypes.c_void_p * n)(*[ptr(t).value for t in tables])
        lds = (ctypes.c_size_t * n)(*[int(t.shape[-1]) for t in tables])
        if firn is not None:
            check(lib().airice_table_launch_multi_firn(ctypes.byref(self.medium),
                                                       ctypes.byref(firn), garr, n, ptrs, lds,
                                                       _stream_handle(stream)),
                  "airice_table_launch_multi_firn")
            return
        check(lib().airice_table_launch_multi(ctypes.byref(self.medium), garr, n, ptrs, lds,
                                              _stream_handle(stream)),
              "airice_table_launch_multi")

    def table_host(self, grid: Grid, row_begin: int = 0, row_count: int | None = None,
                   full: bool = False, firn=None):
        if row_count is None:
            row_count = grid.table_rows - row_begin
        n = row_count * grid.angle_steps
        table = np.empty((_lib.TABLE_COLUMNS, n), dtype=np.float32)
        fullarr = np.empty((_lib.RAY_FIELDS, n), dtype=np.float64) if full else None
        if firn is not None:
            check(lib().airice_table_host_firn(ctypes.byref(self.medium), ctypes.byref(firn),
                                               ctypes.byref(grid), row_begin, row_count,
                                               ptr(table), ptr(fullarr), n),
                  "airice_table_host_firn")
        else:
            check(lib().airice_table_host(ctypes.byref(self.medium), ctypes.byref(grid),
                                          row_begin, row_count, ptr(table), ptr(fullarr), n),
                  "airice_table_host")
        return (table, fullarr) if full else table

    # ------------------------------------------------------------------ table files
    def save_table(self, path: str, grid: Grid, table) -> None:
        """airice_table_save: one antenna's table (11 x n float32, numpy or a torch tensor on
        any device) with this medium and ``grid`` in the header."""
        if hasattr(table, "detach"):
            table = table.detach().cpu().numpy()
        t = np.asarray(table)
        if t.dtype != np.float32 or t.ndim != 2 or t.shape[0] != _lib.TABLE_COLUMNS:
            raise ValueError(f"save_table: want an ({_lib.TABLE_COLUMNS}, n) float32 table, "
                             f"got {t.dtype} {t.shape}")
        if t.strides[1] != 4:
            t = np.ascontiguousarray(t)
        check(lib().airice_table_save(str(path).encode(), ctypes.byref(self.medium),
                                      ctypes.byref(grid), ptr(t), t.strides[0] // 4, t.shape[1]),
              "airice_table_save")

    @staticmethod
    def table_file_info(path: str) -> _lib.TableFileInfo:
        info = _lib.TableFileInfo()
        check(lib().airice_table_file_read_info(str(path).encode(), ctypes.byref(info)),
              "airice_table_file_read_info")
        return info

    def load_table(self, path: str, check_medium: bool = True):
        """airice_table_load: (grid, 11 x n float32 numpy table), checksum-verified; with
        ``check_medium`` a table traced in another medium is refused."""
        info = self.table_file_info(path)
        n = int(info.n_rays)
        table = np.empty((_lib.TABLE_COLUMNS, n), dtype=np.float32)
        check(lib().airice_table_load(str(path).encode(),
                                      ctypes.byref(self.medium) if check_medium else None,
                                      ptr(table), max(n, 1), ctypes.byref(info)),
              "airice_table_load")
        return info.grid, table

    # ------------------------------------------------------------------ rays
    def rays_device(self, launch_deg, txh, ice_h: float, depth: float, in_ice: bool, out,
                    ld: int | None = None, stream=None, firn=None) -> None:
        n = int(launch_deg.numel())
        if firn is not None:
            check(lib().airice_rays_launch_firn(ctypes.byref(self.medium), ctypes.byref(firn),
                                                ptr(launch_deg), ptr(txh), ice_h, depth,
                                                int(in_ice), n, ptr(out), n if ld is None else ld,
                                                _stream_handle(stream)),
                  "airice_rays_launch_firn")
            return
        check(lib().airice_rays_launch(ctypes.byref(self.medium), ptr(launch_deg), ptr(txh),
                                       ice_h, depth, int(in_ice), n, ptr(out),
                                       n if ld is None else ld, _stream_handle(stream)),
              "airice_rays_launch")

    def rays_host(self, launch_deg, txh, ice_h: float, depth: float, in_ice: bool,
                  firn=None) -> np.ndarray:
        """airice_rays_host: GetRayTracingSolutions for host arrays on the CPU (the one-query
        drop-in's path, same source as the device kernels); (18, n) doubles."""
        a = np.ascontiguousarray(launch_deg, dtype=np.float64).ravel()
        h = np.ascontiguousarray(np.broadcast_to(txh, a.shape), dtype=np.float64).ravel()
        out = np.empty((_lib.RAY_FIELDS, a.size), dtype=np.float64)
        if firn is not None:
            check(lib().airice_rays_host_firn(ctypes.byref(self.medium), ctypes.byref(firn),
                                              ptr(a), ptr(h), ice_h, depth, int(in_ice), a.size,
                                              ptr(out), max(a.size, 1)),
                  "airice_rays_host_firn")
            return out
        check(lib().airice_rays_host(ctypes.byref(self.medium), ptr(a), ptr(h), ice_h, depth,
                                     int(in_ice), a.size, ptr(out), max(a.size, 1)),
              "airice_rays_host")
        return out

    # ------------------------------------------------------------------ minimizer
    def solve_device(self, txh, dist, depth, ice_h: float, out, status=None,
                     straight_angle=None, ld: int | None = None, stream=None,
                     variant: int | None = None) -> None:
        n = int(txh.numel())
        v = self.variant if variant is None else variant
        check(lib().airice_solve_launch(ctypes.byref(self.medium), v, ice_h, ptr(txh), ptr(dist),
                                        ptr(depth), ptr(straight_angle), n, ptr(out),
                                        n if ld is None else ld, ptr(status),
                                        _stream_handle(stream)), "airice_solve_launch")

    def solve_host(self, txh, dist, depth, ice_h: float, straight_angle=None,
                   variant: int | None = None):
        v = self.variant if variant is None else variant
        txh = np.ascontiguousarray(txh, dtype=np.float64)
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        depth = np.ascontiguousarray(depth, dtype=np.float64)
        thr = None if straight_angle is None else np.ascontiguousarray(straight_angle, np.float64)
        n = txh.size
        fields = _lib.PYSOLVE_FIELDS if v == VARIANT_PYWRAPPER else _lib.SOLVE_FIELDS
        out = np.empty((fields, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        check(lib().airice_solve_host(ctypes.byref(self.medium), v, ice_h, ptr(txh), ptr(dist),
                                      ptr(depth), ptr(thr), n, ptr(out), n, ptr(st)),
              "airice_solve_host")
        return out, st

    # ------------------------------------------------------------------ CoREAS entry
    def hdtip_device(self, src_cm, dist_cm, depth_cm, ice_cm: float, out, ok,
                     ld: int | None = None, stream=None) -> None:
        n = int(src_cm.numel())
        check(lib().airice_hdtip_launch(ctypes.byref(self.medium), ptr(src_cm), ptr(dist_cm),
                                        ptr(depth_cm), ice_cm, n, ptr(out),
                                        n if ld is None else ld, ptr(ok),
                                        _stream_handle(stream)), "airice_hdtip_launch")

    # ------------------------------------------------------------------ table lookup
    @staticmethod
    def lookup_table(table, grid: Grid, n_entries: int | None = None,
                     ld: int | None = None) -> LookupTable:
        """Describe an HBM-resident table (11 float columns, column stride ``ld``) for
        ``table_lookup_device``; ``grid`` supplies the globals of the last table made
        (LoopStopHeight, HeightStepSize, TotalHeightSteps, TotalAngleSteps, .cc:1035-1039)."""
        n = grid.n_rays if n_entries is None else n_entries
        t = LookupTable()
        t.table = ptr(table).value
        t.ld = n if ld is None else ld
        t.n_entries = n
        t.loop_stop_height = grid.stop_height
        t.height_step = grid.height_step
        t.total_height_steps = grid.height_steps
        t.total_angle_steps = grid.angle_steps
        return t

    @staticmethod
    def lookup_pack(lt: LookupTable, stream=None):
        """airice_lookup_pack: a packed copy of the table (pack format 2: one 64-byte pair record
        per entry, holding it and the next entry, one 256-byte record per table row and the angle
        vector; torch tensor on the table's device) that ``lt`` then reads; the tensor is kept on
        ``lt``."""
        import torch
        n, asteps = int(lt.n_entries), int(lt.total_angle_steps)
        if n < 1 or asteps < 1:  # as airice_lookup_pack: the row records divide by the row length
            raise ValueError(f"lookup_pack: n_entries ({n}) and total_angle_steps ({asteps}) "
                             "must be >= 1")
        floats = int(lib().airice_lookup_pack_floats(n, asteps))
        packed = torch.empty(floats, dtype=torch.float32,
                             device=torch.device("cuda", torch.cuda.current_device()))
        check(lib().airice_lookup_pack(ctypes.byref(lt), ptr(packed), floats,
                                       _stream_handle(stream)), "airice_lookup_pack")
        lt.entries = ptr(packed).value
        lt._packed = packed
        return packed

    def table_lookup_device(self, lt: LookupTable, src_cm, dist_cm, depth_cm, ice_cm: float,
                            out, ok, flags, ld: int | None = None, stream=None) -> None:
        """Batched GetHorizontalDistanceToIntersectionPoint_Table (.cc:1305-1462): out is the
        9 double columns of ``hdtip_device``; ok the returned bool; flags AIRICE_LOOKUP_*."""
        n = int(src_cm.numel())
        check(lib().airice_table_lookup_launch(ctypes.byref(self.medium), ctypes.byref(lt),
                                               ptr(src_cm), ptr(dist_cm), ptr(depth_cm), ice_cm,
                                               n, ptr(out), n if ld is None else ld, ptr(ok),
                                               ptr(flags), _stream_handle(stream)),
              "airice_table_lookup_launch")

    def table_lookup_multi_device(self, tables, antenna_table, antenna_depth_cm, src_cm, dist_cm,
                                  ice_cm: float, out, ok, flags, ld: int | None = None,
                                  work=None, stream=None):
        """airice_table_lookup_launch_multi: the lookup of n_ant antennas x n_src sources in ONE
        launch.  ``tables``: the distinct LookupTables (at most 32, packed or not);
        ``antenna_table`` / ``antenna_depth_cm``: each antenna's table index and Rx depth (host);
        ``src_cm``: n_src float64 on the device, common to all antennas (sort it once and every
        antenna's lookups run in the faster sorted order); ``dist_cm``: an (n_ant, n_src) device
        tensor whose row stride is passed on.  Query (a, i) lands at ``out[c, a*n_src + i]`` (9
        columns of stride ``ld``, default n_ant*n_src), ``ok`` / ``flags`` at [a*n_src + i]: the
        bits of one ``table_lookup_device`` call per antenna.  ``work``: a device byte tensor of
        airice_table_lookup_multi_work_bytes, allocated here without one.  Stream-ordered; returns
        the workspace, which must outlive the launch."""
        import torch
        n_tab, n_ant, n_src = len(tables), len(antenna_table), int(src_cm.numel())
        if len(antenna_depth_cm) != n_ant:
            raise ValueError(f"table_lookup_multi_device: {n_ant} antenna tables, "
                             f"{len(antenna_depth_cm)} depths")
        if n_ant > 0 and (dist_cm.dim() != 2 or tuple(dist_cm.shape) != (n_ant, n_src)
                          or (n_src > 1 and dist_cm.stride(1) != 1)):
            raise ValueError(f"table_lookup_multi_device: dist_cm must be ({n_ant}, {n_src}) with "
                             f"contiguous rows, got {tuple(dist_cm.shape)}")
        ld_dist = int(dist_cm.stride(0)) if n_ant > 1 else n_src
        tarr = (LookupTable * max(n_tab, 1))(*tables)
        amap = np.ascontiguousarray(antenna_table, dtype=np.int32)
        deps = np.ascontiguousarray(antenna_depth_cm, dtype=np.float64)
        if work is None:
            need = int(lib().airice_table_lookup_multi_work_bytes(n_tab, n_ant))
            work = torch.empty(max(need, 16), dtype=torch.uint8, device=src_cm.device)
        check(lib().airice_table_lookup_launch_multi(
            ctypes.byref(self.medium), tarr, n_tab, ptr(amap), ptr(deps), n_ant, ptr(src_cm),
            ptr(dist_cm), ld_dist, ice_cm, n_src, ptr(out), n_ant * n_src if ld is None else ld,
            ptr(ok), ptr(flags), ptr(work), int(work.numel()), _stream_handle(stream)),
            "airice_table_lookup_launch_multi")
        return work

    def antenna_tables(self, depths_cm, ice_cm: float, height_step: float = 10.0,
                       start_angle: float = 90.1, stop_angle: float = 180.0,
                       angle_step: float = 0.1, stream=None, firn=None) -> AntennaTables:
        """The tables of a set of antennas, ready for ``AntennaTables.lookup``: antennas at the
        same depth share one table (``dedupe_depths``, as the reference); the distinct tables are
        made in one ``tables_device`` launch and packed."""
        import torch
        distinct, antenna_table = dedupe_depths(depths_cm)
        dev = torch.device("cuda", torch.cuda.current_device())
        grids = [make_grid(d, ice_cm, height_step, start_angle, stop_angle, angle_step)
                 for d in distinct]
        buffers = [torch.empty((_lib.TABLE_COLUMNS, g.n_rays), dtype=torch.float32, device=dev)
                   for g in grids]
        self.tables_device(grids, buffers, stream=stream, firn=firn)
        tables = [self.lookup_table(b, g) for b, g in zip(buffers, grids)]
        for t in tables:
            self.lookup_pack(t, stream=stream)
        return AntennaTables(self, ice_cm, grids, buffers, tables, antenna_table, depths_cm,
                             firn=firn)

    # ------------------------------------------------------------------ single ray (cfg1)
    def single_ray_host(self, antenna_depth: float, launch_deg: float, txh: float, ice: float,
                        path: bool = True):
        """SingleRayAirIceRefraction (BASELINE cfg1) on the GPU: the forward trace of one launch
        angle and, with ``path``, the RayPathinAirnIce.txt samples.  Inputs after the CLI's
        clamps; antenna depth positive in ice (SingleRayAirIceRefraction.C:166).  Returns
        (summary[6], x, z): thd_air, L, incident angle on ice, thd_ice, receive angle in ice,
        ice propagation time."""
        info = _lib.SingleRayInfo()
        check(lib().airice_single_ray_plan(ctypes.byref(self.medium), antenna_depth, launch_deg,
                                           txh, ice, ctypes.byref(info)), "airice_single_ray_plan")
        n = int(info.n_air + info.n_ice) if path else 0
        summary = np.empty(_lib.SINGLE_RAY_FIELDS)
        x = np.empty(n)
        z = np.empty(n)
        check(lib().airice_single_ray_host(ctypes.byref(self.medium), antenna_depth, launch_deg,
                                           txh, ice, ptr(summary), ptr(x) if path else None,
                                           ptr(z) if path else None, n),
              "airice_single_ray_host")
        return summary, x, z, info

    # ------------------------------------------------------------------ ray paths, batched
    def _ray_paths_plan(self, txh, ice: float, depth: float):
        h = np.ascontiguousarray(txh, dtype=np.float64).ravel()
        offsets = np.zeros(h.size + 1, dtype=np.int64)
        work = ctypes.c_size_t(0)
        check(lib().airice_ray_paths_plan(ctypes.byref(self.medium), depth, ice, ptr(h), h.size,
                                          ptr(offsets), ctypes.byref(work)),
              "airice_ray_paths_plan")
        return h, offsets, int(work.value)

    def ray_paths_plan(self, txh, ice: float, depth: float) -> np.ndarray:
        """airice_ray_paths_plan (host only): the int64 sample offsets of a batch of rays with Tx
        heights ``txh`` that share ``ice`` and the antenna ``depth`` (positive in ice); ray i owns
        samples [offsets[i], offsets[i+1]).  The counts do not depend on the launch angles."""
        return self._ray_paths_plan(txh, ice, depth)[1]

    def ray_paths_work_bytes(self, txh, ice: float, depth: float) -> int:
        """Bytes of the device workspace ``ray_paths_device`` needs for this batch."""
        return self._ray_paths_plan(txh, ice, depth)[2]

    def ray_paths_device(self, launch_deg, txh, ice: float, depth: float, offsets, summary, x, z,
                         work=None, stream=None, ld: int | None = None):
        """airice_ray_paths_launch: ``launch_deg`` (n float64), ``summary`` (6 x n float64) and
        ``x`` / ``z`` (>= offsets[n] float64 each, or both None for the summaries alone) are
        device tensors; ``txh`` and ``offsets`` (from ``ray_paths_plan``) stay on the host.
        ``work`` is a device byte tensor of ``ray_paths_work_bytes``; without one it is allocated
        here.  Stream-ordered; returns the workspace, which must outlive the launch."""
        import torch
        h = np.ascontiguousarray(txh, dtype=np.float64).ravel()
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = h.size
        if off.size != n + 1 or int(launch_deg.numel()) != n:
            raise ValueError(f"ray_paths_device: {n} Tx heights, {int(launch_deg.numel())} launch "
                             f"angles, {off.size} offsets")
        if (x is None) != (z is None):
            raise ValueError("ray_paths_device: x and z are given together or not at all")
        if work is None:
            work = torch.empty(max(self.ray_paths_work_bytes(h, ice, depth), 16),
                               dtype=torch.uint8, device=summary.device)
        cap = 0 if x is None else min(int(x.numel()), int(z.numel()))
        check(lib().airice_ray_paths_launch(ctypes.byref(self.medium), depth, ice, ptr(launch_deg),
                                            ptr(h), n, ptr(off), ptr(work), int(work.numel()),
                                            ptr(summary), n if ld is None else ld, ptr(x), ptr(z),
                                            cap, _stream_handle(stream)),
              "airice_ray_paths_launch")
        return work

    def ray_paths_host(self, launch_deg, txh, ice: float, depth: float, path: bool = True):
        """airice_ray_paths_host: the paths of n rays (numpy in, numpy out).  Returns
        (summary (6, n), offsets, x, z): the ``single_ray_host`` summary of every ray as columns
        and the concatenated RayPathinAirnIce.txt samples, ray i in [offsets[i], offsets[i+1]);
        x and z are empty without ``path``."""
        a = np.ascontiguousarray(launch_deg, dtype=np.float64).ravel()
        h = np.ascontiguousarray(np.broadcast_to(txh, a.shape), dtype=np.float64).ravel()
        _, offsets, _ = self._ray_paths_plan(h, ice, depth)
        n = a.size
        total = int(offsets[n]) if path else 0
        summary = np.empty((_lib.SINGLE_RAY_FIELDS, n))
        x = np.empty(total)
        z = np.empty(total)
        check(lib().airice_ray_paths_host(ctypes.byref(self.medium), depth, ice, ptr(a), ptr(h), n,
                                          ptr(offsets), ptr(summary), max(n, 1),
                                          ptr(x) if path else None, ptr(z) if path else None,
                                          total), "airice_ray_paths_host")
        return summary, offsets, x, z

    def paths_between(self, txh, dist, depth: float, ice: float, solver: str = "multiray"):
        """The DrawShowerRays composition (DrawShowerRays.C:483-519): solve every (Tx height,
        horizontal distance) pair against one antenna ``depth`` m below the ice surface, then
        sample the path of every solved launch angle in one batch.  ``solver="multiray"`` (the
        default): ``solve_host``, the MultiRayAirIceRefraction bisection (slot 10, LaunchAngleAir);
        ``solver="brent"``: ``air2ice_host``, the GSL-Brent solve of Air2IceRayTracing.C (column 2,
        status from column 12), so the paths are the ones that program draws for each pair.
        Returns (summary, offsets, x, z, status): ``ray_paths_host``'s outputs and the solve's
        AIRICE_SOLVE_* status bytes."""
        h = np.ascontiguousarray(txh, dtype=np.float64).ravel()
        d = np.ascontiguousarray(np.broadcast_to(dist, h.shape), dtype=np.float64).ravel()
        if solver == "brent":
            sol, status = self.air2ice_host(h, d, float(ice), float(depth))
            launch = sol[2]
        elif solver == "multiray":
            sol, status = self.solve_host(h, d, np.full(h.shape, -float(depth)), ice,
                                          variant=VARIANT_MULTIRAY)
            launch = sol[10]
        else:
            raise ValueError(f"paths_between: solver is 'multiray' or 'brent', got {solver!r}")
        return (*self.ray_paths_host(launch, h, ice, float(depth)), status)

    # ------------------------------------------------------------------ Brent solve, batched
    def air2ice_device(self, txh, dist, ice, depth, out, status=None, ld: int | None = None,
                       stream=None) -> None:
        """airice_air2ice_launch: the Air2IceRayTracing.C / AirRayTracing.C point-to-point solve of
        n pairs in one launch.  ``txh``, ``dist``, ``ice``, ``depth`` (n float64 each, m; depth
        positive in ice, 0 for a receiver in the air at height ``ice``), ``out`` (16 x ld float64,
        the AIRICE_RTF_AIR2ICE_FIELDS as columns) and ``status`` (n uint8, optional) are device
        tensors.  ``out[2]`` is the contiguous launch-angle input of ``ray_paths_device``.
        Stream-ordered."""
        n = int(txh.numel())
        check(lib().airice_air2ice_launch(ctypes.byref(self.medium), ptr(txh), ptr(dist), ptr(ice),
                                          ptr(depth), n, ptr(out), n if ld is None else ld,
                                          ptr(status), _stream_handle(stream)),
              "airice_air2ice_launch")

    def air2ice_host(self, txh, dist, ice, depth):
        """airice_air2ice_host: numpy in, numpy out; the four inputs broadcast against each other.
        Returns (out (16, n), status (n) uint8).  One pair runs where scalar_mode() says."""
        arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64)
                                     for a in (txh, dist, ice, depth)])
        t, d, i, p = [np.ascontiguousarray(a).ravel() for a in arrs]
        n = t.size
        out = np.empty((_lib.RTF_AIR2ICE_FIELDS, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        check(lib().airice_air2ice_host(ctypes.byref(self.medium), ptr(t), ptr(d), ptr(i), ptr(p),
                                        n, ptr(out), max(n, 1), ptr(st)), "airice_air2ice_host")
        return out, st

    def air_to_air_host(self, tx_h, rx_h, dist):
        """AirRayTracing.C for n (Tx, Rx) pairs in the air: a Tx below its Rx is swapped with it
        (AirRayTracing.C:38-45) and the pair solved as (max, dist, min, 0) by ``air2ice_host``.
        Returns (out (16, n), status, flipped): column 4, the incident angle on the Rx, is
        reported as 180 - angle where ``flipped`` (AirRayTracing.C:147-157)."""
        t, r, d = [np.ascontiguousarray(a).ravel() for a in np.broadcast_arrays(
            *[np.asarray(a, dtype=np.float64) for a in (tx_h, rx_h, dist)])]
        flipped = t < r
        out, st = self.air2ice_host(np.where(flipped, r, t), d, np.where(flipped, t, r), 0.0)
        out[4] = np.where(flipped, 180 - out[4], out[4])
        return out, st, flipped

    # ------------------------------------------------------------------ in-ice rays, batched
    @staticmethod
    def _ice_model(model):
        """(A, B, C) as the three host doubles the C-ABI reads, or None for the defaults."""
        if model is None:
            return None
        m = np.ascontiguousarray(model, dtype=np.float64).ravel()
        if m.size != 3:
            raise ValueError(f"ice model: (A, B, C), got {m.size} values")
        return m

    def ice_rays_device(self, z0, x1, z1, out, status=None, ld: int | None = None, stream=None,
                        model=None) -> None:
        """airice_iceray_launch: IceRayTracing::IceRayTracing -- the direct, reflected and
        refracted rays between a transmitter at depth ``z0`` and a receiver ``x1`` metres away at
        depth ``z1`` (both negative, in the ice) -- for n pairs in one launch.  ``z0``, ``x1``,
        ``z1`` (n float64 each), ``out`` (32 x ld float64: the _lib.ICERAY_* columns) and
        ``status`` (n uint8, optional: the _lib.ICERAY_D / _R / _RA0 / _RA1 / _NONFINITE bits)
        are device tensors; ``model`` is (A, B, C) of n(z) = A + B exp(-C|z|) on the host, the
        reference's 1.78, -0.43, 0.0132 when None.  Stream-ordered."""
        n = int(z0.numel())
        m = self._ice_model(model)
        check(lib().airice_iceray_launch(ptr(m), ptr(z0), ptr(x1), ptr(z1), n, ptr(out),
                                         n if ld is None else ld, ptr(status),
                                         _stream_handle(stream)), "airice_iceray_launch")

    def ice_rays_host(self, z0, x1, z1, model=None):
        """airice_iceray_host: numpy in, numpy out; the three inputs broadcast against each other.
        Returns (out (32, n), status (n) uint8).  One pair runs where scalar_mode() says (the
        calling thread by default); more are copied to the GPU, solved in one launch and copied
        back."""
        arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (z0, x1, z1)])
        a, b, c = [np.ascontiguousarray(v).ravel() for v in arrs]
        n = a.size
        out = np.empty((_lib.ICERAY_FIELDS, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        m = self._ice_model(model)
        check(lib().airice_iceray_host(ptr(m), ptr(a), ptr(b), ptr(c), n, ptr(out), max(n, 1),
                                       ptr(st)), "airice_iceray_host")
        return out, st

    # ------------------------------------------------------------------ ice-to-air rays, batched
    def ice_to_air_device(self, z0, x1, h, out, status=None, ld: int | None = None, stream=None,
                          model=None) -> None:
        """airice_iceair_launch: IceRayTracing::GetDirectRayPar_Air -- the direct ray from a
        transmitter at depth ``z0`` (<= 0, in the ice) to a receiver ``x1`` metres away and ``h``
        metres above the surface -- for n triples in one launch.  ``z0``, ``x1``, ``h`` (n float64
        each), ``out`` (10 x ld float64: the _lib.ICEAIR_* columns) and ``status`` (n uint8,
        optional: _lib.ICEAIR_ACCEPTED / _NONFINITE) are device tensors; ``model`` as
        ``ice_rays_device``.  Stream-ordered."""
        n = int(z0.numel())
        m = self._ice_model(model)
        check(lib().airice_iceair_launch(ptr(m), ptr(z0), ptr(x1), ptr(h), n, ptr(out),
                                         n if ld is None else ld, ptr(status),
                                         _stream_handle(stream)), "airice_iceair_launch")

    def ice_to_air_host(self, z0, x1, h, model=None):
        """airice_iceair_host: numpy in, numpy out; the three inputs broadcast against each other.
        Returns (out (10, n), status (n) uint8).  One triple runs where scalar_mode() says (the
        calling thread by default); more are copied to the GPU, solved in one launch and copied
        back."""
        arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (z0, x1, h)])
        a, b, c = [np.ascontiguousarray(v).ravel() for v in arrs]
        n = a.size
        out = np.empty((_lib.ICEAIR_FIELDS, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        m = self._ice_model(model)
        check(lib().airice_iceair_host(ptr(m), ptr(a), ptr(b), ptr(c), n, ptr(out), max(n, 1),
                                       ptr(st)), "airice_iceair_host")
        return out, st

    # ------------------------------------------------------------------ first arrivals, batched
    _PAIRINGS = {"elementwise": _lib.PAIRS_ELEMENTWISE, "cross": _lib.PAIRS_CROSS}

    @classmethod
    def _pairing(cls, pairing, n_tx: int, n_rx: int) -> tuple[int, int]:
        """(the AIRICE_PAIRS_* code, the number of pairs) of a first-arrival call."""
        if pairing not in cls._PAIRINGS:
            raise ValueError(f"pairing: 'elementwise' or 'cross', got {pairing!r}")
        if pairing == "elementwise" and n_tx != n_rx:
            raise ValueError(f"elementwise pairing: {n_tx} emitters, {n_rx} antennas")
        return cls._PAIRINGS[pairing], n_tx * n_rx if pairing == "cross" else n_tx

    @staticmethod
    def ice_first_arrivals_work_bytes(n_pairs: int) -> int:
        """airice_icefirst_work_bytes: the device work buffer of ``n_pairs`` pairs."""
        return int(lib().airice_icefirst_work_bytes(n_pairs))

    def ice_first_arrivals_device(self, tx, rx, out, work=None, pairing: str = "elementwise",
                                  status=None, ld: int | None = None, stream=None, model=None):
        """airice_icefirst_launch: IceRayTracing::DirectRayTracer -- the first-arriving ray from
        each emitter to each antenna -- in three launches (geometry, the in-ice solve, the choice).
        ``tx`` (3 x n_tx) and ``rx`` (3 x n_rx) are float64 device tensors of x, y, z rows (z
        negative, in the ice); ``pairing`` is "elementwise" (n_tx == n_rx, pair i) or "cross" (pair
        t * n_rx + r); ``out`` (8 x ld float64: the _lib.ICEFIRST_* columns) and ``status`` (one
        uint8 per pair, optional: the solver's _lib.ICERAY_* bits) are device tensors.  ``work`` is
        a device buffer of ``ice_first_arrivals_work_bytes(pairs)`` bytes; None allocates one with
        torch on ``tx``'s device.  Returns the work buffer, which must stay alive until the
        launches have run.  Stream-ordered."""
        for name, a in (("tx", tx), ("rx", rx)):
            if a.dim() != 2 or a.shape[0] != 3 or (a.shape[1] > 1 and a.stride(1) != 1):
                raise ValueError(f"{name}: a (3, n) tensor with contiguous rows")
        n_tx, n_rx = int(tx.shape[1]), int(rx.shape[1])
        code, pairs = self._pairing(pairing, n_tx, n_rx)
        need = self.ice_first_arrivals_work_bytes(pairs)
        if work is None:
            import torch
            work = torch.empty(max(need, 1), dtype=torch.uint8, device=tx.device)
        m = self._ice_model(model)
        check(lib().airice_icefirst_launch(
            ptr(m), ptr(tx[0]), ptr(tx[1]), ptr(tx[2]), n_tx, ptr(rx[0]), ptr(rx[1]), ptr(rx[2]),
            n_rx, code, ptr(work), int(work.numel() * work.element_size()), ptr(out),
            pairs if ld is None else ld, ptr(status), _stream_handle(stream)),
            "airice_icefirst_launch")
        return work

    def ice_first_arrivals_host(self, tx, rx, pairing: str = "elementwise", model=None):
        """airice_icefirst_host: ``tx`` (3, n_tx) and ``rx`` (3, n_rx) numpy arrays in,
        (out (8, pairs), status (pairs) uint8) out.  One pair runs where scalar_mode() says (the
        calling thread by default); more are copied to the GPU, traced in three launches and
        copied back."""
        t = np.ascontiguousarray(np.asarray(tx, dtype=np.float64).reshape(3, -1))
        r = np.ascontiguousarray(np.asarray(rx, dtype=np.float64).reshape(3, -1))
        code, pairs = self._pairing(pairing, t.shape[1], r.shape[1])
        out = np.empty((_lib.ICEFIRST_FIELDS, pairs), dtype=np.float64)
        st = np.empty(pairs, dtype=np.uint8)
        m = self._ice_model(model)
        check(lib().airice_icefirst_host(ptr(m), ptr(t[0]), ptr(t[1]), ptr(t[2]), t.shape[1],
                                         ptr(r[0]), ptr(r[1]), ptr(r[2]), r.shape[1], code,
                                         ptr(out), max(pairs, 1), ptr(st)),
              "airice_icefirst_host")
        return out, st

    def ice_first_select_device(self, rays, x1, out, status=None, ld: int | None = None,
                                ld_rays: int | None = None, stream=None) -> None:
        """airice_icefirst_select_launch: the first-arrival choice alone, over ``rays`` (32 x
        ld_rays float64, what ``ice_rays_device`` wrote) with ``x1`` (n float64) passed through to
        column 6, in one launch.  ``out`` (8 x ld float64) and ``status`` (n uint8, optional) as
        ``ice_first_arrivals_device``; device tensors.  Stream-ordered."""
        n = int(x1.numel())
        check(lib().airice_icefirst_select_launch(ptr(rays), n if ld_rays is None else ld_rays,
                                                  ptr(x1), n, ptr(out), n if ld is None else ld,
                                                  ptr(status), _stream_handle(stream)),
              "airice_icefirst_select_launch")

    @staticmethod
    def ice_first_select_host(rays, x1):
        """airice_icefirst_select_host: the same choice over host rows ``rays`` (32, n) on the
        calling thread, no GPU.  Returns (out (8, n), status (n) uint8)."""
        r = np.ascontiguousarray(rays, dtype=np.float64)
        x = np.ascontiguousarray(x1, dtype=np.float64).ravel()
        n = x.size
        if r.shape != (_lib.ICERAY_FIELDS, n):
            raise ValueError(f"rays: ({_lib.ICERAY_FIELDS}, {n}), got {r.shape}")
        out = np.empty((_lib.ICEFIRST_FIELDS, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        check(lib().airice_icefirst_select_host(ptr(r), max(n, 1), ptr(x), n, ptr(out), max(n, 1),
                                                ptr(st)), "airice_icefirst_select_host")
        return out, st

    # ------------------------------------------------------------------ in-ice ray paths, batched
    @staticmethod
    def _ice_ray_paths_plan(z0, z1, status, rays: int):
        a, b = [np.ascontiguousarray(v).ravel() for v in np.broadcast_arrays(
            np.asarray(z0, dtype=np.float64), np.asarray(z1, dtype=np.float64))]
        st = None if status is None else np.ascontiguousarray(status, dtype=np.uint8).ravel()
        if st is not None and st.size != a.size:
            raise ValueError(f"ice ray paths: {a.size} pairs, {st.size} status bytes")
        offsets = np.zeros(4 * a.size + 1, dtype=np.int64)
        work = ctypes.c_size_t(0)
        check(lib().airice_icepath_plan(ptr(a), ptr(b), ptr(st), a.size, int(rays), ptr(offsets),
                                        ctypes.byref(work)), "airice_icepath_plan")
        return a, b, st, offsets, int(work.value)

    def ice_ray_paths_plan(self, z0, z1, status=None, rays: int = 15) -> np.ndarray:
        """airice_icepath_plan (host only): the int64 slot offsets of the ray paths of n pairs;
        segment 4 i + r (r = 0 direct, 1 reflected, 2-3 refracted, of pair i) owns slots
        [offsets[4i+r], offsets[4i+r+1]) of x and z.  Exact counts for the direct and reflected
        rays, an upper bound for the refracted ones; 0 for kinds outside ``rays`` (a mask of
        _lib.ICERAY_D / _R / _RA0 / _RA1) and, with ``status`` (the solver's bytes), for rays the
        solver did not accept."""
        return self._ice_ray_paths_plan(z0, z1, status, rays)[3]

    def ice_ray_paths_work_bytes(self, z0, z1, status=None, rays: int = 15) -> int:
        """Bytes of the device workspace ``ice_ray_paths_device`` needs for this batch."""
        return self._ice_ray_paths_plan(z0, z1, status, rays)[4]

    def ice_ray_paths_device(self, z0, x1, z1, rays_out, offsets, count, x, z, z0_host=None,
                             z1_host=None, status=None, rays: int = 15, work=None, stream=None,
                             model=None):
        """airice_icepath_launch: the x(z) samples of every accepted ray of n pairs, over
        ``rays_out``, the (32, ld) tensor ``ice_rays_device`` wrote for the same ``z0``, ``x1``,
        ``z1`` (n float64 device tensors each).  ``count`` (4n int64), ``x`` and ``z``
        (>= offsets[4n] float64 each) are device tensors; ``offsets`` (from
        ``ice_ray_paths_plan``), ``z0_host`` / ``z1_host`` (the depths the plan was made from;
        copied back from the device, which synchronises, when not given) and ``status`` stay on
        the host.  ``work`` is a device byte tensor of ``ice_ray_paths_work_bytes``; without one it
        is allocated here.  Stream-ordered; returns the workspace, which must outlive the launch.
        Slots past a segment's count keep what they held."""
        import torch
        n = int(z0.numel())
        a = z0.detach().cpu().numpy() if z0_host is None else z0_host
        b = z1.detach().cpu().numpy() if z1_host is None else z1_host
        a, b, st, planned, need = self._ice_ray_paths_plan(a, b, status, rays)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if a.size != n or off.size != 4 * n + 1:
            raise ValueError(f"ice_ray_paths_device: {n} pairs, {a.size} host depths, "
                             f"{off.size} offsets")
        if work is None:
            work = torch.empty(max(need, 16), dtype=torch.uint8, device=z0.device)
        m = self._ice_model(model)
        check(lib().airice_icepath_launch(
            ptr(m), ptr(z0), ptr(x1), ptr(z1), ptr(rays_out), int(rays_out.stride(0)), ptr(a),
            ptr(b), ptr(st), n, int(rays), ptr(off), ptr(work), int(work.numel()), ptr(count),
            ptr(x), ptr(z), min(int(x.numel()), int(z.numel())), _stream_handle(stream)),
            "airice_icepath_launch")
        return work

    def ice_ray_paths_host(self, z0, x1, z1, model=None, rays: int = 15):
        """Solver, plan and paths in one call (numpy in, numpy out): ``ice_rays_host``, then the
        paths of every ray it accepted.  Returns (offsets (4n+1), count (4n), x, z): segment
        s = 4 i + r holds its count[s] samples at x / z[offsets[s] : offsets[s] + count[s]], in
        the reference's order (from the upper of the two depths, over the surface or the turning
        depth, down to the lower).  One pair in SCALAR_HOST mode runs on the calling thread
        (airice_icepath_one_host); otherwise the batch is copied to the GPU, sampled in two
        launches and copied back."""
        arrs = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64) for v in (z0, x1, z1)])
        a, b, c = [np.ascontiguousarray(v).ravel() for v in arrs]
        n = a.size
        out, st = self.ice_rays_host(a, b, c, model=model)
        _, _, _, offsets, _ = self._ice_ray_paths_plan(a, c, st, rays)
        total = int(offsets[-1])
        count = np.zeros(4 * n, dtype=np.int64)
        x = np.full(total, np.nan)
        z = np.full(total, np.nan)
        m = self._ice_model(model)
        if n == 1 and lib().airice_scalar_mode(-1) == _lib.SCALAR_HOST:
            for r in range(4):
                cap = int(offsets[r + 1] - offsets[r])
                if cap == 0:
                    continue
                cnt = ctypes.c_int64(0)
                lo = int(offsets[r])
                check(lib().airice_icepath_one_host(
                    ptr(m), 1 << r, a[0], b[0], c[0], out[_lib.ICERAY_LVALUE + r, 0],
                    out[_lib.ICERAY_ZMAX + r - 2, 0] if r >= 2 else 0.0, ptr(x[lo:]), ptr(z[lo:]),
                    cap, ctypes.byref(cnt)), "airice_icepath_one_host")
                count[r] = cnt.value
        elif n > 0:
            check(lib().airice_icepath_host(ptr(m), ptr(a), ptr(b), ptr(c), ptr(out), max(n, 1),
                                            ptr(st), n, int(rays), ptr(offsets), ptr(count),
                                            ptr(x), ptr(z), total), "airice_icepath_host")
        return offsets, count, x, z

    def ice_solutions_device(self, z0, x1, z1, rays, out, status=None, a0: float = 1.0,
                             frequency: float = 0.1, rays_lower=None, ld: int | None = None,
                             stream=None, model=None) -> None:
        """airice_icesol_launch: IceRayTracing::GetRayTracingSolutions -- the two rays a receiver
        sees, in order of arrival, with their ice attenuation -- for n pairs in one launch over
        ``rays``, the (32, ld_rays) tensor ``ice_rays_device`` wrote for the same ``z0``, ``x1``,
        ``z1``.  With ``rays_lower`` (what it wrote for ``z1 - 0.01``) also GetFocusingFactor.
        ``out`` (18 x ld float64: the _lib.ICESOL_* columns) and ``status`` (n uint8, optional:
        the _lib.ICESOL_* bits) are device tensors; ``a0`` and ``frequency`` (GHz) hold for the
        batch; ``model`` as ``ice_rays_device``.  Stream-ordered."""
        n = int(z0.numel())
        m = self._ice_model(model)
        check(lib().airice_icesol_launch(
            ptr(m), ptr(z0), ptr(x1), ptr(z1), ptr(rays), int(rays.stride(0)), ptr(rays_lower),
            0 if rays_lower is None else int(rays_lower.stride(0)), n, float(a0),
            float(frequency), ptr(out), n if ld is None else ld, ptr(status),
            _stream_handle(stream)), "airice_icesol_launch")

    def ice_solutions_host(self, z0, x1, z1, a0: float = 1.0, frequency: float = 0.1,
                           focusing: bool = False, model=None):
        """airice_icesol_host: numpy in, numpy out; the three inputs broadcast against each other.
        Returns (out (18, n), status (n) uint8).  One pair runs where scalar_mode() says (the
        calling thread by default); more are copied to the GPU, solved (iceray_kernel once, twice
        with ``focusing``, then icesol_kernel once) and copied back."""
        arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (z0, x1, z1)])
        a, b, c = [np.ascontiguousarray(v).ravel() for v in arrs]
        n = a.size
        out = np.empty((_lib.ICESOL_FIELDS, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        m = self._ice_model(model)
        check(lib().airice_icesol_host(ptr(m), ptr(a), ptr(b), ptr(c), n, float(a0),
                                       float(frequency), 1 if focusing else 0, ptr(out),
                                       max(n, 1), ptr(st)), "airice_icesol_host")
        return out, st

    def ice_attenuation_spectrum_device(self, z0, z1, rays, sol, freq, out, a0: float = 1.0,
                                        ld_f: int | None = None, stream=None, model=None) -> None:
        """airice_icesol_spectrum_launch: the ice attenuation of each pair's two rays at every
        frequency of ``freq`` (F float64 GHz, a device tensor) in one launch, over ``rays`` (what
        ``ice_rays_device`` wrote) and ``sol`` (what ``ice_solutions_device`` wrote for the same
        pairs at any frequency: only its two ray-type rows are read).  ``out`` is a device tensor
        of 2 n rows of ``ld_f`` (default F) float64: AttRay of pair i, slot s, bin k at
        ``out.view(-1)[(2 i + s) ld_f + k]``, i.e. an (n, 2, F) tensor when ld_f == F.  A bin
        whose frequency is not finite and positive is NaN where the slot holds a ray.
        Stream-ordered."""
        n, f = int(z0.numel()), int(freq.numel())
        m = self._ice_model(model)
        check(lib().airice_icesol_spectrum_launch(
            ptr(m), ptr(z0), ptr(z1), ptr(rays), int(rays.stride(0)), ptr(sol),
            int(sol.stride(0)), n, float(a0), ptr(freq), f, ptr(out), f if ld_f is None else ld_f,
            _stream_handle(stream)), "airice_icesol_spectrum_launch")

    def ice_attenuation_spectrum_host(self, z0, x1, z1, freq, a0: float = 1.0, model=None):
        """airice_icesol_spectrum_host: numpy in, numpy out; the three inputs broadcast against
        each other, ``freq`` is the list of F frequencies (GHz).  Returns (sol (18, n) -- the
        solutions without focusing at freq[0] --, status (n) uint8, att (n, 2, F)).  One pair
        runs where scalar_mode() says (the calling thread by default); more are copied to the
        GPU, solved (iceray_kernel, icesol_kernel and icesol_spectrum_kernel once each) and copied
        back."""
        arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (z0, x1, z1)])
        a, b, c = [np.ascontiguousarray(v).ravel() for v in arrs]
        fr = np.ascontiguousarray(freq, dtype=np.float64).ravel()
        n, f = a.size, fr.size
        sol = np.empty((_lib.ICESOL_FIELDS, n), dtype=np.float64)
        st = np.empty(n, dtype=np.uint8)
        att = np.empty((n, 2, f), dtype=np.float64)
        m = self._ice_model(model)
        check(lib().airice_icesol_spectrum_host(ptr(m), ptr(a), ptr(b), ptr(c), n, float(a0),
                                                ptr(fr), f, ptr(sol), max(n, 1), ptr(st),
                                                ptr(att), f), "airice_icesol_spectrum_host")
        return sol, st, att

    # ------------------------------------------------------------------ in-ice tables
    def ice_tables(self, shower_hit_distance, shower_depth, rx_depths, a0: float = 1.0,
                   frequency: float = 0.1, model=None, grids=None, stream=None) -> IceTables:
        """airice_icetab_build_launch: IceRayTracing::MakeTable for the antennas at depths
        ``rx_depths`` (at most _lib.ICETAB_MAX_BUILD) in four launches -- the grid positions, the
        in-ice solver over every position and its receiver 1 cm lower, the two-ray solutions with
        attenuation and focusing, and the pack into records.  The grid is MakeTable's 401 x 201
        around (``shower_hit_distance``, ``shower_depth``), or ``grids``: one descriptor per
        antenna (``icetab_grid``).  ``a0`` and ``frequency`` (GHz) default to MakeTable's 1 and
        0.1.  Stream-ordered; the work buffer is freed once the stream has used it."""
        import torch
        if grids is None:
            grids = [icetab_grid_init(shower_hit_distance, shower_depth, zr)
                     for zr in np.atleast_1d(np.asarray(rx_depths, dtype=np.float64))]
        descs, size = icetab_descs(grids)
        n_ant = descs.shape[0]
        work = ctypes.c_size_t(0)
        check(lib().airice_icetab_work_bytes(ptr(descs), n_ant, ctypes.byref(work)),
              "airice_icetab_work_bytes")
        dev = torch.device("cuda", torch.cuda.current_device())
        image = torch.empty(size, dtype=torch.float64, device=dev)
        buf = torch.empty((work.value + 7) // 8, dtype=torch.float64, device=dev)
        m = self._ice_model(model)
        check(lib().airice_icetab_build_launch(ptr(m), ptr(image), ptr(descs), n_ant, float(a0),
                                               float(frequency), ptr(buf), buf.numel() * 8,
                                               _stream_handle(stream)),
              "airice_icetab_build_launch")
        if isinstance(stream, torch.cuda.Stream):
            buf.record_stream(stream)
            image.record_stream(stream)
        return IceTables(image, descs)

    def ice_tables_from_values(self, descs, values) -> IceTables:
        """An ``IceTables`` from tables in the reference's column form (saved tables, tests):
        ``descs`` one descriptor per antenna, ``values[a]`` (13, nx, nz).  The image is assembled
        on the host and uploaded with airice_memcpy_h2d."""
        import torch
        image, d = icetab_image_from_values(descs, values)
        dev = torch.device("cuda", torch.cuda.current_device())
        dimage = torch.empty(image.size, dtype=torch.float64, device=dev)
        check(lib().airice_memcpy_h2d(ptr(dimage), ptr(image), image.nbytes), "airice_memcpy_h2d")
        t = IceTables(dimage, d)
        t._host = image
        return t

    # ------------------------------------------------------------------ pythonwrapper
    def trace_ice_to_air_device(self, depth, ice, txh, dist, out10, stream=None) -> None:
        n = int(depth.numel())
        check(lib().airice_trace_ice_to_air_launch(ctypes.byref(self.medium), ptr(depth), ptr(ice),
                                                   ptr(txh), ptr(dist), n, ptr(out10),
                                                   _stream_handle(stream)),
              "airice_trace_ice_to_air_launch")

    def rtf_eval(self, op: int, args) -> np.ndarray:
        """One RayTracingFunctions:: scalar function (AIRICE_RTF_*, include/airice.h) where
        scalar_mode() says -- the host by default, else the GPU -- in the reference's output
        layout."""
        a = np.ascontiguousarray(args, dtype=np.float64)
        n = lib().airice_rtf_outputs(op, int(self.medium.max_layers))
        if n < 0:
            raise ValueError(f"unknown RayTracingFunctions op {op}")
        out = np.zeros(n, dtype=np.float64)
        check(lib().airice_rtf_eval(ctypes.byref(self.medium), op, ptr(a), a.size, ptr(out), n),
              "airice_rtf_eval")
        return out

    def trace_ice_to_air_host(self, depth, ice, txh, dist):
        arrs = [np.ascontiguousarray(np.broadcast_to(a, np.shape(depth)), dtype=np.float64).ravel()
                for a in (depth, ice, txh, dist)]
        n = arrs[0].size
        out = np.empty((n, 10), dtype=np.float64)
        check(lib().airice_trace_ice_to_air_host(ctypes.byref(self.medium), *[ptr(a) for a in arrs],
                                                 n, ptr(out)), "airice_trace_ice_to_air_host")
        return out
