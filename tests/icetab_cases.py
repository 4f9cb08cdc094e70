"""The in-ice interpolation tables restated in plain numpy, one statement of the reference per
line (IceRayTracing.cc:2614-2816), and the synthetic images and queries the CPU and GPU tests
share.  Everything here is float64 scalar arithmetic: no fused operations, IEEE division."""
import numpy as np

from tests.iceray_cases import same_bits  # noqa: F401  (re-exported for the tests)

F = np.float64
DESC, RECORD, PARAMS = 8, 16, 13
CELL, IDW, BAD_ANTENNA = 1, 2, 4
MISSING = F(-1000.0)
# AIRICE_ICESOL_* columns and status bits the pack reads
TIME, PATH, LAUNCH, RECEIVE, IGNORE, INCIDENCE, ATT, FOCUS = 0, 2, 4, 6, 8, 10, 12, 16
FOCUS0, FOCUS1, NONFINITE = 8, 16, 128


def position(start, step, i):
    off = F(step) * F(i)
    return F(start) + off


def grid_init_ref(hit, depth, rx_depth):
    """MakeTable's grid set-up (.cc:2617-2636) with the header's widths and steps."""
    width_x, width_z, step_x, step_z = F(40), F(20), F(0.1), F(0.1)
    nx = int((width_x / step_x) + 1)
    nz = int((width_z / step_z) + 1)
    x_start = F(hit) - (width_x / 2)
    if hit <= width_x / 2:
        x_start = F(0)
    z_start = F(depth) - (width_z / 2)
    z_stop = F(depth) + (width_z / 2)
    if abs(depth) <= 10 or z_stop >= 0:
        z_start = F(-20)
    return np.array([x_start, z_start, step_x, step_z, nx, nz, 0, rx_depth], dtype=F)


def header_doubles(n_ant):
    return (n_ant * DESC + RECORD - 1) // RECORD * RECORD


def layout_ref(descs):
    """first_record of each antenna and the image's size in doubles."""
    d = np.array(descs, dtype=F).reshape(-1, DESC)
    record = header_doubles(len(d)) // RECORD
    for a in range(len(d)):
        d[a, 6] = record
        record += int(d[a, 4]) * int(d[a, 5])
    return d, record * RECORD


def pack_ref(sol, status):
    """One position: the 18 solution values and the status byte -> the 16 slots (.cc:2664-2715)."""
    sol = np.asarray(sol, dtype=F)
    rec = np.zeros(RECORD, dtype=F)
    focusing = [F(1), F(1)]
    if status & FOCUS0:
        focusing[0] = sol[FOCUS]
    if status & FOCUS1:
        focusing[1] = sol[FOCUS + 1]
    if np.isnan(focusing[0]):
        focusing[0] = F(1)
    if np.isnan(focusing[1]):
        focusing[1] = F(1)
    if sol[IGNORE] != 0:
        rec[0:6] = [sol[TIME], sol[PATH], sol[LAUNCH], sol[RECEIVE], sol[ATT], focusing[0]]
    else:
        rec[0:6] = MISSING
    if sol[IGNORE + 1] != 0:
        rec[6:12] = [sol[TIME + 1], sol[PATH + 1], sol[LAUNCH + 1], sol[RECEIVE + 1], sol[ATT + 1],
                     focusing[1]]
        if sol[INCIDENCE + 1] != 100:
            rec[12] = sol[INCIDENCE + 1]
        if sol[INCIDENCE + 1] == 100:
            rec[12] = MISSING
    else:
        rec[6:13] = MISSING
    rec[13] = F(status)
    return rec


def lookup_ref(image, n_ant, ant, xT, zT):
    """GetInterpolatedValue for the 13 parameters of one query (.cc:2736-2816): (values, status)."""
    out = np.full(PARAMS, MISSING, dtype=F)
    if not (0 <= ant < n_ant):
        return out, BAD_ANTENNA
    d = image[ant * DESC:(ant + 1) * DESC]
    x_start, z_start, x_step, z_step = d[0], d[1], d[2], d[3]
    nx, nz, first = int(d[4]), int(d[5]), int(d[6])
    x_stop = position(x_start, x_step, nx - 1)
    z_stop = position(z_start, z_step, nz - 1)
    xT, zT = F(xT), F(zT)
    if not (xT >= x_start and xT <= x_stop and zT >= z_start and zT <= z_stop):
        return out, 0
    x, y = xT, zT
    bx = int(np.floor((xT - x_start) / x_step))
    bz = int(np.floor(np.abs(zT - z_start) / z_step))
    if not (bx + 1 <= nx - 1 and bz + 1 <= nz - 1):
        return out, 0
    x1, y1 = position(x_start, x_step, bx), position(z_start, z_step, bz)
    x2, y2 = position(x_start, x_step, bx + 1), position(z_start, z_step, bz + 1)
    status = CELL

    def record(ix, iz):
        r = first + ix * nz + iz
        return image[r * RECORD:(r + 1) * RECORD]

    r11, r12, r21, r22 = record(bx, bz), record(bx, bz + 1), record(bx + 1, bz), record(bx + 1, bz + 1)
    with np.errstate(all="ignore"):
        for c in range(PARAMS):
            f11, f12, f21, f22 = r11[c], r12[c], r21[c], r22[c]
            if f11 == -1000 or f12 == -1000 or f21 == -1000 or f22 == -1000:
                status |= IDW
                sum1, sum2 = F(0), F(0)
                if f11 != -1000:
                    sum1 = sum1 + (F(1.0) / ((x1 - x) * (x1 - x) + (y1 - y) * (y1 - y))) * f11
                    sum2 = sum2 + (F(1.0) / ((x1 - x) * (x1 - x) + (y1 - y) * (y1 - y)))
                if f12 != -1000:
                    sum1 = sum1 + (F(1.0) / ((x1 - x) * (x1 - x) + (y2 - y) * (y2 - y))) * f12
                    sum2 = sum2 + (F(1.0) / ((x1 - x) * (x1 - x) + (y2 - y) * (y2 - y)))
                if f21 != -1000:
                    sum1 = sum1 + (F(1.0) / ((x2 - x) * (x2 - x) + (y1 - y) * (y1 - y))) * f21
                    sum2 = sum2 + (F(1.0) / ((x2 - x) * (x2 - x) + (y1 - y) * (y1 - y)))
                if f22 != -1000:
                    sum1 = sum1 + (F(1.0) / ((x2 - x) * (x2 - x) + (y2 - y) * (y2 - y))) * f22
                    sum2 = sum2 + (F(1.0) / ((x2 - x) * (x2 - x) + (y2 - y) * (y2 - y)))
                v = sum1 / sum2
                if np.isnan(v):
                    v = MISSING
            else:
                w11 = ((x2 - x) * (y2 - y)) / ((x2 - x1) * (y2 - y1))
                w12 = ((x2 - x) * (y - y1)) / ((x2 - x1) * (y2 - y1))
                w21 = ((x - x1) * (y2 - y)) / ((x2 - x1) * (y2 - y1))
                w22 = ((x - x1) * (y - y1)) / ((x2 - x1) * (y2 - y1))
                v = w11 * f11 + w12 * f12 + w21 * f21 + w22 * f22
            out[c] = v
    return out, status


def lookup_ref_batch(image, n_ant, queries):
    vals = np.empty((len(queries), PARAMS), dtype=F)
    st = np.empty(len(queries), dtype=np.int64)
    for i, (a, x, z) in enumerate(queries):
        vals[i], st[i] = lookup_ref(image, n_ant, int(a), x, z)
    return vals, st


# ---- synthetic tables ----------------------------------------------------------------------------
# (x_start, z_start, x_step, z_step, nx, nz, rx_depth): antenna 0 is hole-free on the reference's
# own steps; antennas 1 and 2 carry the holes; every z_start is negative and antenna 2's grid
# crosses z = 0
GRIDS = ((150.0, -110.0, 0.1, 0.1, 5, 4, -100.0),
         (3.0, -7.5, 0.25, 0.5, 9, 7, -2.0),
         (0.0, -1.4, 0.3, 0.7, 13, 5, -30.0))
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))  # f11, f12, f21, f22 as (dix, diz)


def hole_cells():
    """[(antenna, bx, bz, slots, corner subset)]: each of the 16 subsets of missing corners in
    the slot-0 group on a cell of its own (no two share a corner), then cells whose holes are in
    slots 6..12 only and in slot 12 only."""
    cells = []
    spots = [(1, bx, bz) for bx in (0, 2, 4, 6) for bz in (0, 2, 4)] + \
            [(2, bx, 0) for bx in (0, 2, 4, 6)]
    for subset, (a, bx, bz) in enumerate(spots):
        cells.append((a, bx, bz, range(0, 6), subset))
    cells.append((2, 8, 0, range(6, 13), 0b0110))
    cells.append((2, 10, 0, range(12, 13), 0b1001))
    cells.append((2, 8, 2, range(6, 13), 0b1111))
    return cells


def synthetic_values():
    """values[a]: (13, nx, nz), a different smooth function per slot, with the holes."""
    values = []
    for a, (xs, zs, dx, dz, nx, nz, _) in enumerate(GRIDS):
        x = np.array([position(xs, dx, i) for i in range(nx)])[:, None]
        z = np.array([position(zs, dz, i) for i in range(nz)])[None, :]
        v = np.empty((PARAMS, nx, nz), dtype=F)
        for c in range(PARAMS):
            v[c] = (c + 1.5) * np.sin(0.3 * x + 0.1 * c) + (c + 2.0) * np.cos(0.2 * z - 0.05 * c) \
                + 0.01 * x * z + a
        assert not np.any(v == -1000)
        values.append(v)
    for a, bx, bz, slots, subset in hole_cells():
        for k, (di, dj) in enumerate(CORNERS):
            if subset >> k & 1:
                values[a][list(slots), bx + di, bz + dj] = MISSING
    return values


def synthetic_image():
    """(image as a plain numpy array, descs with layout, values): the layout of include/airice.h
    assembled here, not by the package."""
    values = synthetic_values()
    descs, size = layout_ref([g[:6] + (0.0, g[6]) for g in GRIDS])
    image = np.zeros(size, dtype=F)
    image[:descs.size] = descs.ravel()
    for a, v in enumerate(values):
        nx, nz, first = int(descs[a, 4]), int(descs[a, 5]), int(descs[a, 6])
        rec = image[first * RECORD:(first + nx * nz) * RECORD].reshape(nx * nz, RECORD)
        rec[:, :PARAMS] = v.reshape(PARAMS, nx * nz).T
    return image, descs, values


def edge_queries():
    """(ant, x, z) rows: cell interiors, every node, the stops' edges, just outside each side, NaN
    and infinities, bad antenna indices."""
    q = []
    inf, nan = np.inf, np.nan
    for a, (xs, zs, dx, dz, nx, nz, _) in enumerate(GRIDS):
        xn = [position(xs, dx, i) for i in range(nx)]
        zn = [position(zs, dz, i) for i in range(nz)]
        for ix in range(nx):
            for iz in range(nz):
                q.append((a, xn[ix], zn[iz]))  # every node (upper stops and hole corners included)
                if ix + 1 < nx and iz + 1 < nz:  # the cell's interior, off its centre
                    q.append((a, xn[ix] + F(0.3) * (xn[ix + 1] - xn[ix]),
                              zn[iz] + F(0.6) * (zn[iz + 1] - zn[iz])))
        xm, zm = xn[1] + F(0.5) * (xn[2] - xn[1]), zn[1] + F(0.25) * (zn[2] - zn[1])
        q += [(a, xn[0], zm), (a, xn[-1], zm), (a, xm, zn[0]), (a, xm, zn[-1])]  # on the stops
        q += [(a, np.nextafter(xn[0], -inf), zm), (a, np.nextafter(xn[-1], inf), zm),
              (a, xm, np.nextafter(zn[0], -inf)), (a, xm, np.nextafter(zn[-1], inf)),
              (a, xn[0] - dx, zm), (a, xn[-1] + dx, zm), (a, xm, zn[0] - dz), (a, xm, zn[-1] + dz),
              (a, np.nextafter(xn[-1], -inf), zm), (a, xm, np.nextafter(zn[-1], -inf))]
        q += [(a, nan, zm), (a, xm, nan), (a, nan, nan), (a, inf, zm), (a, -inf, zm), (a, xm, inf),
              (a, xm, -inf)]
    xs, zs = GRIDS[0][0] + 0.05, GRIDS[0][1] + 0.05
    q += [(-1, xs, zs), (3, xs, zs), (2 ** 31 - 1, xs, zs), (-2 ** 31, xs, zs)]
    return np.array(q, dtype=F)


def drawn_queries(n, rng):
    """n queries with the antennas mixed: mostly inside an antenna's grid (a tenth of a width
    over its sides), the edge queries spread among them."""
    q = np.empty((n, 3), dtype=F)
    ant = rng.integers(0, len(GRIDS), n)
    g = np.array([gr[:6] for gr in GRIDS])[ant]
    wx, wz = g[:, 2] * (g[:, 4] - 1), g[:, 3] * (g[:, 5] - 1)
    q[:, 0] = ant
    q[:, 1] = g[:, 0] + wx * rng.uniform(-0.1, 1.1, n)
    q[:, 2] = g[:, 1] + wz * rng.uniform(-0.1, 1.1, n)
    e = edge_queries()
    at = rng.permutation(n)[:min(len(e), n // 2)]
    q[at] = e[rng.permutation(len(e))[:len(at)]]
    return q
