"""Float64 statements of the depth front end, integrate(depth) and the TSDF builders, the case list both test files share, and the
checks that put an implementation's output (the oracle's on the CPU, the kernels' on the GPU) against them.

The float64 functions are written from what each operation means -- a ray length, a weighted mean over a window, a projection, a
signed distance -- not from the oracle's operation order.  A float32 implementation cannot equal them bit for bit; what it may do is
differ where a decision (which pixel, which side of trunc / eta, in front of the camera or not) sits within rounding error of its
boundary.  The constants below say how close that is.  They were measured with tests/test_depth_front_cpu.py::test_print_measured
(oracle against float64 over the whole case list, on a CPU) and each threshold is FOUR times the measured figure: the float32 chain
is a 3-term dot product, one divide and one fused multiply-add (or a 35-step running sum), whose worst case is a small multiple of
its typical case; four leaves room for the GPU's identical arithmetic on the same inputs and nothing more.
test_depth_front_cpu.py::test_recorded_thresholds_match_measurement fails if a figure drifts from what is recorded here.
"""
import numpy as np

from sobfu_amd.synthetic import hash_field

# ---- measured figures (oracle vs float64 over the case list, rounded up to two digits) and the thresholds derived from them ------
# measured: coo 5.007e-05 px, psdf 3.723e-07 m, camz 3.723e-07 m, value 9.555e-06, dists 2.328e-07 (3.9 x 2^-24), bilateral q 9.862e-04 mm,
# builders 2.152e-06
MEASURED_COO = 5.1e-5        # px   largest |coo32 - coo64| over cells that project within a pixel of the image, camz > 0
MEASURED_PSDF = 3.8e-7       # m    largest |psdf32 - psdf64| (finite Dp, same pixel)
MEASURED_CAMZ = 3.8e-7       # m    largest |camz32 - camz64|
MEASURED_VALUE = 9.6e-6      # -    largest |value32 - value64| of integrate(depth) (same pixel, both written)
MEASURED_DISTS_REL = 2.4e-7  # -    largest relative error of compute_dists
MEASURED_BILATERAL_Q = 9.9e-4  # mm largest |q32 - q64| at unpoisoned pixels, inputs <= 8000 mm
MEASURED_PRIM_VALUE = 2.2e-6   # -  largest |value32 - value64| of the five builders
COO_MARGIN = 4 * MEASURED_COO
PSDF_MARGIN = 4 * MEASURED_PSDF
CAMZ_MARGIN = 4 * MEASURED_CAMZ
VALUE_TOL = 4 * MEASURED_VALUE
DISTS_REL_BOUND = 4 * MEASURED_DISTS_REL
BILATERAL_DELTA = 4 * MEASURED_BILATERAL_Q
PRIM_VALUE_TOL = 4 * MEASURED_PRIM_VALUE  # margins on the sdf are this times trunc (value = sdf / trunc)
EXPLAINED_CAP = 0.02  # explained cells <= 2 % of written cells, per case
BAND_CAP = 0.01       # pixels inside the delta band <= 1 % of pixels, per case

F32 = np.float32


# =================================================================================================================================
# float64 references
# =================================================================================================================================
def dists64(depth, intr):
    """ray length in metres of a pixel whose depth (z, mm) is d: d * |((x-cx)/fx, (y-cy)/fy, 1)| / 1000"""
    fx, fy, cx, cy = (np.float64(F32(v)) for v in intr)
    rows, cols = depth.shape
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    return depth.astype(np.float64) * np.sqrt(((x - cx) / fx) ** 2 + ((y - cy) / fy) ** 2 + 1.0) / 1000.0


def _window(rows, cols, ksz):
    """yields (oy, ox, mask, cy, cx): neighbour offsets, where the neighbour lies in the reference's window,
    max(x - ksz/2, 0) <= cx < min(x - ksz/2 + ksz, cols - 1) and the same in y (the last column and row are never neighbours),
    and the neighbour's clipped indices"""
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    for oy in range(-(ksz // 2), ksz - ksz // 2):
        for ox in range(-(ksz // 2), ksz - ksz // 2):
            cy, cx = y + oy, x + ox
            yield oy, ox, (cy >= 0) & (cy < rows - 1) & (cx >= 0) & (cx < cols - 1), np.clip(cy, 0, rows - 1), np.clip(cx, 0, cols - 1)


def bilateral64(depth, ksz, sigma_spatial, sigma_depth):
    """-> (q64, poisoned, starved).  q64: the unrounded weighted mean, weight exp(-(|dp|^2 / (2 ss^2) + dd^2 / (2 sd_mm^2))), NaN where the
    window is empty or every weight is zero.  poisoned: some neighbour differs by so much that dd^2, taken as a 32-bit product, wraps
    negative -- the reference's weight is then exp(+huge), not a bilateral weight at all, and only the oracle says what comes out.
    starved: the weights sum to less than 2^-100 without being zero.  That happens on the last row and column only (a pixel there is not
    in its own window, so no weight is 1) when every neighbour is far away in depth; float32 weights are then subnormal or zero and the
    result is a mean of noise or 0 / 0 = 0: compared with the oracle only, like the poisoned ones, and included in `poisoned`."""
    d = depth.astype(np.int64)
    a_s = 0.5 / (np.float64(F32(sigma_spatial)) ** 2)
    a_d = 0.5 / ((np.float64(F32(sigma_depth)) * 1000.0) ** 2)
    s1, s2 = np.zeros(d.shape), np.zeros(d.shape)
    poisoned = np.zeros(d.shape, bool)
    for oy, ox, m, cy, cx in _window(d.shape[0], d.shape[1], ksz):
        nb = d[cy, cx]
        dd2 = (d - nb) ** 2
        poisoned |= m & (dd2 >= 2 ** 31)  # |dd| <= 65535 so dd^2 < 2^32: wrapped value negative <=> dd^2 >= 2^31
        w = np.where(m, np.exp(-((oy * oy + ox * ox) * a_s + dd2 * a_d)), 0.0)
        s1 += nb * w
        s2 += w
    with np.errstate(invalid="ignore", divide="ignore"):
        q = s1 / s2
    starved = (s2 > 0) & (s2 < 2.0 ** -100)
    return q, poisoned | starved, starved


def bilateral32(depth, ksz, sigma_spatial, sigma_depth):
    """The same mean carried in float32, in the reference's loop order (row-major over the window), exp rounded to float32 from
    float64: the figure |q32 - q64| is measured on this.  (The oracle itself returns only the rounded integer; libm's expf and this
    exp differ in the last place now and then, which is the size of thing delta has to cover anyway.)"""
    d = depth.astype(np.int32)
    sd = F32(sigma_depth) * F32(1000)
    a_s, a_d = F32(0.5) / (F32(sigma_spatial) * F32(sigma_spatial)), F32(0.5) / (sd * sd)
    s1, s2 = np.zeros(d.shape, F32), np.zeros(d.shape, F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for oy, ox, m, cy, cx in _window(d.shape[0], d.shape[1], ksz):
            nb = d[cy, cx]
            dd = (d - nb).astype(np.int64)
            c2 = ((dd * dd) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(F32)
            arg = -(F32(oy * oy + ox * ox) * a_s + c2 * a_d)
            w = np.where(m, np.exp(arg.astype(np.float64)).astype(F32), F32(0))
            s1 = (np.where(m, nb.astype(F32) * w, F32(0)) + s1).astype(F32)
            s2 = (s2 + w).astype(F32)
        return s1 / s2


def _grid(dims):
    X, Y, Z = dims
    return np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")  # k, j, i -- arrays of shape (Z, Y, X)


def integrate64(dists, dims, vs, trunc, eta, R, t, intr):
    """One depth frame into a volume: voxel centre (i + 0.5) vs -> camera point R v + t -> pinhole projection -> floor to a pixel.
    Cells that project outside the image, lie at or behind the camera plane (camz <= 0) or see no measurement (Dp <= 0) are skipped.
    psdf = Dp - camz; value = clamp(psdf / trunc, -1, 1); weight = [psdf > -eta].
    -> dict of (Z, Y, X) arrays: value, weight, written, and the margins that decide a cell's fate: m_px (distance of the projection to
    the nearest pixel boundary -- the image's borders are pixel boundaries too), m_trunc (min |psdf -+ trunc|), m_eta (|psdf + eta|),
    m_camz (|camz|); plus u, v, camz, psdf, px, py for the measurements."""
    vs = np.asarray([F32(v) for v in vs], np.float64)
    R = np.asarray(R, F32).astype(np.float64).reshape(3, 3)
    t = np.asarray(t, F32).astype(np.float64).reshape(3)
    fx, fy, cx, cy = (np.float64(F32(v)) for v in intr)
    trunc, eta = np.float64(F32(trunc)), np.float64(F32(eta))
    rows, cols = dists.shape
    k, j, i = _grid(dims)
    p = np.stack([(i + 0.5) * vs[0], (j + 0.5) * vs[1], (k + 0.5) * vs[2]], -1)
    cam = p @ R.T + t
    camz = cam[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * cam[..., 0] / camz + cx, fy * cam[..., 1] / camz + cy
        inside = (camz > 0) & (u >= 0) & (v >= 0) & (u < cols) & (v < rows)  # NaN compares false
        px = np.where(inside, np.floor(u), 0).astype(np.int64)
        py = np.where(inside, np.floor(v), 0).astype(np.int64)
        Dp = dists[py, px].astype(np.float64)
        written = inside & ~(Dp <= 0)  # a NaN measurement is not <= 0: it is written, as NaN
        psdf = Dp - camz
        value = np.where(psdf >= trunc, 1.0, np.where(psdf <= -trunc, -1.0, psdf / trunc))
        weight = (psdf > -eta).astype(np.float64)
        m_px = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))
        m_px = np.where(np.isfinite(m_px), m_px, np.inf)
        m_trunc = np.minimum(np.abs(psdf - trunc), np.abs(psdf + trunc))
        m_eta = np.abs(psdf + eta)
    big = lambda a: np.where(np.isfinite(a), a, np.inf)  # noqa: E731
    return dict(value=value, weight=weight, written=written, m_px=m_px, m_trunc=big(m_trunc), m_eta=big(m_eta), m_camz=np.abs(camz), u=u, v=v,
                camz=camz, psdf=psdf, px=px, py=py, inside=inside)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum rounds once there and once more to float32 (the
    double rounding can differ from fmaf only on a 2^-29 tie; test_depth_front_cpu.py checks the chain against the oracle bit for bit)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def integrate32_chain(dims, vs, R, t, intr):
    """The float32 chain of the reference (tsdf_volume.cu:70-79): voxel centre x * vs + vs / 2, R v + t through the nested fma of
    kfusion's dot, the camera point as a running sum of R * (0, 0, vs_z) over the planes, projection f * (cam / camz) + c as one fma.
    -> camz, u, v as (Z, Y, X) float32.  Used to measure |coo32 - coo64| / |psdf32 - psdf64| and to search for exact ties."""
    X, Y, Z = dims
    vs = [F32(v) for v in vs]
    R = np.asarray(R, F32).reshape(9)
    t = np.asarray(t, F32).reshape(3)
    fx, fy, cx, cy = (F32(v) for v in intr)
    _, j, i = _grid((X, Y, 1))
    vcx = (i.astype(F32) * vs[0] + vs[0] / F32(2)).astype(F32)
    vcy = (j.astype(F32) * vs[1] + vs[1] / F32(2)).astype(F32)
    vcz = np.full(vcx.shape, vs[2] / F32(2), F32)
    dot = lambda r: _fma32(np.full(vcx.shape, R[r], F32), vcx, _fma32(np.full(vcx.shape, R[r + 1], F32), vcy, (R[r + 2] * vcz).astype(F32)))  # noqa: E731
    camx, camy, camz0 = (dot(0) + t[0]).astype(F32), (dot(3) + t[1]).astype(F32), (dot(6) + t[2]).astype(F32)
    run = [[camx[0]], [camy[0]], [camz0[0]]]
    for c, r in zip(run, (2, 5, 8)):  # one float32 addition of R * (0, 0, vs_z) per plane
        step = F32(R[r] * vs[2])
        for _ in range(Z - 1):
            c.append((c[-1] + step).astype(F32))
    camx, camy, camz = (np.stack(c, 0) for c in run)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = _fma32(np.full(camz.shape, fx, F32), (camx / camz).astype(F32), np.full(camz.shape, cx, F32))
        v = _fma32(np.full(camz.shape, fy, F32), (camy / camz).astype(F32), np.full(camz.shape, cy, F32))
    return camz, u, v


def integrate32(dists, poison, dims, vs, trunc, eta, R, t, intr):
    """integrate(depth) on the float32 chain above -> (volume, psdf32, px, py, written)"""
    camz, u, v = integrate32_chain(dims, vs, R, t, intr)
    rows, cols = dists.shape
    trunc, eta = F32(trunc), F32(eta)
    with np.errstate(invalid="ignore"):
        ok = ~((u < 0) | (v < 0) | (u >= F32(cols)) | (v >= F32(rows))) & (camz > 0) & (u == u) & (v == v)
        px = np.where(ok, np.floor(u), 0).astype(np.int64)
        py = np.where(ok, np.floor(v), 0).astype(np.int64)
        Dp = dists[py, px]
        wr = ok & ~(Dp <= 0)
        psdf = (Dp - camz).astype(F32)
        val = np.where(psdf >= trunc, F32(1), np.where(psdf <= -trunc, F32(-1), (psdf / trunc).astype(F32))).astype(F32)
        w = (psdf > -eta).astype(F32)
    out = poison.copy()
    out[..., 0] = np.where(wr, val, poison[..., 0])
    out[..., 1] = np.where(wr, w, poison[..., 1])
    return out, psdf, px, py, wr


PRIMS = ("sphere", "box", "ellipsoid", "plane", "torus")


def prim64(kind, dims, vs, trunc, eta, params):
    """Signed distances of the five primitives at the voxel centres (i + 0.5) vs.  Box, ellipsoid and torus sit at the reference's
    centre dims / 2 * vs (a float division: 8.5 voxels for 17); sphere and plane are given in volume coordinates.
    -> dict(sdf, value, weight, singular): singular marks cells where the formula itself is 0 / 0 (the ellipsoid's centre)."""
    vs = np.asarray([F32(v) for v in vs], np.float64)
    p = [np.float64(F32(v)) for v in np.atleast_1d(params)]
    trunc, eta = np.float64(F32(trunc)), np.float64(F32(eta))
    k, j, i = _grid(dims)
    x, y, z = (i + 0.5) * vs[0], (j + 0.5) * vs[1], (k + 0.5) * vs[2]
    if kind in ("box", "ellipsoid", "torus"):
        x, y, z = x - dims[0] / 2.0 * vs[0], y - dims[1] / 2.0 * vs[1], z - dims[2] / 2.0 * vs[2]
    weight = np.ones(x.shape)
    singular = np.zeros(x.shape, bool)
    if kind == "sphere":  # params: cx, cy, cz, radius
        sdf = np.sqrt((x - p[0]) ** 2 + (y - p[1]) ** 2 + (z - p[2]) ** 2) - p[3]
        weight = (sdf > -eta).astype(np.float64)
    elif kind == "box":  # half extents
        dx, dy, dz = np.abs(x) - p[0], np.abs(y) - p[1], np.abs(z) - p[2]
        sdf = np.minimum(np.maximum(dx, np.maximum(dy, dz)), 0.0) + np.sqrt(np.maximum(dx, 0) ** 2 + np.maximum(dy, 0) ** 2 + np.maximum(dz, 0) ** 2)
    elif kind == "ellipsoid":  # radii; the first-order distance k0 (k0 - 1) / k1
        k0 = np.sqrt((x / p[0]) ** 2 + (y / p[1]) ** 2 + (z / p[2]) ** 2)
        k1 = np.sqrt((x / p[0] ** 2) ** 2 + (y / p[1] ** 2) ** 2 + (z / p[2] ** 2) ** 2)
        singular = k1 == 0
        with np.errstate(invalid="ignore", divide="ignore"):
            sdf = k0 * (k0 - 1.0) / k1
    elif kind == "plane":  # z of the plane
        sdf = z - p[0]
    elif kind == "torus":  # ring radius, tube radius; the ring lies in the xz plane
        sdf = np.sqrt((np.sqrt(x * x + z * z) - p[0]) ** 2 + y * y) - p[1]
    else:
        raise ValueError(kind)
    with np.errstate(invalid="ignore"):
        value = np.where(sdf >= trunc, 1.0, np.where(sdf <= -trunc, -1.0, sdf / trunc))
    return dict(sdf=sdf, value=value, weight=weight, singular=singular)


# =================================================================================================================================
# checks: an implementation's output against the float64 reference, under the recorded thresholds
# =================================================================================================================================
def poison_volume(dims):
    """What integrate(depth) can never write: values outside [-1, 1], all distinct, and a weight of 7."""
    X, Y, Z = dims
    v = np.empty((Z, Y, X, 2), F32)
    v[..., 0] = (2.0 + np.arange(X * Y * Z, dtype=np.float64) * 2.0 ** -10).astype(F32).reshape(Z, Y, X)
    v[..., 1] = 7.0
    return v


def check_integrate(vol, poison, ref, margins=None):
    """-> (unexplained, explained, written): counts of cells where `vol` (integrated over `poison`) disagrees with integrate64's `ref`
    with no margin under its threshold / with one, and of cells the reference writes.  Disagree: written flag or weight differs, or the
    value is off by more than VALUE_TOL (a NaN value agrees with a NaN value only)."""
    coo_m, psdf_m, camz_m, vtol = margins or (COO_MARGIN, PSDF_MARGIN, CAMZ_MARGIN, VALUE_TOL)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    written = (bits(vol) != bits(poison)).any(-1)
    val, w = vol[..., 0].astype(np.float64), vol[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        vbad = ~((np.abs(val - ref["value"]) <= vtol) | (np.isnan(val) & np.isnan(ref["value"])))
    both = written & ref["written"]
    bad = (written != ref["written"]) | (both & ((w != ref["weight"]) | vbad))
    near = (ref["m_px"] < coo_m) | (ref["m_trunc"] < psdf_m) | (ref["m_eta"] < psdf_m) | (ref["m_camz"] < camz_m)
    return int((bad & ~near).sum()), int((bad & near).sum()), int(ref["written"].sum())


def check_bilateral(out, q64, poisoned, delta=None):
    """-> (wrong, in_band): at unpoisoned pixels `out` must be round-half-even(q64) (0 where q64 is NaN); within delta of a half-integer
    it may be the other neighbour.  wrong counts violations, in_band the unpoisoned pixels inside the band."""
    delta = BILATERAL_DELTA if delta is None else delta
    ok = ~poisoned
    q = np.where(np.isnan(q64), 0.0, q64)
    want = np.rint(q)
    band = ok & (np.abs(q - (np.floor(q) + 0.5)) < delta)
    o = out.astype(np.float64)
    good = (o == want) | (band & ((o == np.floor(q)) | (o == np.floor(q) + 1)))
    return int((ok & ~good).sum()), int(band.sum())


def in_band(q64, poisoned, delta=None):
    delta = BILATERAL_DELTA if delta is None else delta
    q = np.where(np.isnan(q64), 0.0, q64)
    return ~poisoned & (np.abs(q - (np.floor(q) + 0.5)) < delta)


def check_dists(out, depth, intr, bound=None):
    """largest relative error against dists64 (0 where the depth is 0 and the output is exactly 0)"""
    ref = dists64(depth, intr)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(ref == 0, np.where(out == 0, 0.0, np.inf), np.abs(out.astype(np.float64) - ref) / ref)
    return float(rel.max())


def check_prim(vol, ref, trunc, eta, tol=None):
    """-> (bad_values, bad_flags, singular): cells off by more than the tolerance; cells whose weight or clamp side differs although no
    |sdf -+ trunc|, |sdf + eta| is under tol * trunc; cells the formula leaves undefined (not compared)."""
    tol = PRIM_VALUE_TOL if tol is None else tol
    trunc, eta = np.float64(F32(trunc)), np.float64(F32(eta))
    ok = ~ref["singular"]
    val, w = vol[..., 0].astype(np.float64), vol[..., 1].astype(np.float64)
    sdf = ref["sdf"]
    with np.errstate(invalid="ignore"):
        bad_v = ok & ~(np.abs(val - ref["value"]) <= tol)
        near_t = np.minimum(np.abs(sdf - trunc), np.abs(sdf + trunc)) < tol * trunc
        near_e = np.abs(sdf + eta) < tol * trunc
        side = lambda a: np.sign(a) * (np.abs(a) == 1.0)  # noqa: E731
        bad_f = ok & (((w != ref["weight"]) & ~near_e) | ((side(val) != side(ref["value"])) & ~near_t))
    return int(bad_v.sum()), int(bad_f.sum()), int(ref["singular"].sum())


# =================================================================================================================================
# the case list
# =================================================================================================================================
IMAGE_SHAPES = [(1, 1), (1, 64), (3, 5), (4, 63), (5, 65), (9, 130), (70, 33)]  # (rows, cols): across dim3(64, 4) and image_grid


def intrinsics(rows, cols):
    """fx != fy, principal point off centre"""
    f = 60.0 + cols
    return (f, 1.13 * f, 0.43 * cols + 0.7, 0.58 * rows - 0.3)


def depth_image(rows, cols, seed, kind="scene"):
    """uint16 mm.  scene: a slanted wall about 0.9 - 1.5 m away with flat patches, a 350 mm step along a diagonal, millimetre noise
    on a third of the image and a sprinkle of zeros (invalid pixels).  far: the same plus pixels at 40000 / 65535 / 32768 (for the
    unsigned comparisons).  saturated: ordinary depth with a few pixels of 65535 next to it."""
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    h = hash_field((rows, cols), seed, 1.0).astype(np.float64)
    d = 900.0 + 4.0 * x + 7.0 * y
    d = np.where((x // 9 + y // 5) % 3 == 0, 1000.0 + 50.0 * ((x // 9) % 4), d)  # flat patches: the mean of equal depths is that depth
    d = d + np.where(x + 2 * y > 0.8 * (cols + rows), 350.0, 0.0)               # a step of several hundred mm
    d = d + np.where((x + y) % 3 == 0, np.rint(3.0 * h), 0.0)                    # noise
    d = np.where(hash_field((rows, cols), seed + 100, 1.0) > 0.9, 0.0, d)        # holes
    d = d.astype(np.uint16)
    if kind == "far":
        s = hash_field((rows, cols), seed + 200, 1.0)
        d = np.where(s > 0.8, np.uint16(65535), np.where(s > 0.6, np.uint16(40000), np.where(s > 0.5, np.uint16(32768), d))).astype(np.uint16)
    if kind == "saturated":
        d = np.where(hash_field((rows, cols), seed + 300, 1.0) > 0.97, np.uint16(65535), d).astype(np.uint16)
    return d


# (rows, cols, ksz, sigma_spatial, sigma_depth [m], kind).  Saturated case: a pixel of 65535 next to depth d <= 2000 has dd >= 63535, and the
# wrapped square is -(2^32 - dd^2) in [-2.6e8, -131071]; at sigma_depth = 5 mm (1 / (2 sd^2) = 0.02) the exponent's argument is >= 0.02 *
# 131071 - 32 * 0.025 > 2600, far above the 89 where expf is already inf: every such weight is inf and the pixel is 0 by the NaN rule.  The
# band 70 .. 89, where a weight is finite but sum1 overflows alone and (int) rintf(inf) is undefined on the host, needs a wrapped square in
# [-4450, -3500], i.e. dd^2 within 4450 of 2^32 -- impossible, the largest dd^2 is 65535^2 = 2^32 - 131071.  (With a wide sigma_depth it
# would not be: 131071 / (2 sd^2) lands in 70 .. 89 for sd of 27 .. 31 mm.  No case uses a sigma_depth between 10 and 100 mm with 65535 in
# the image.)
BILATERAL_SEED = 1  # of depth_image; chosen (on the float64 reference alone) so that every case below meets BAND_CAP
BILATERAL_CASES = (
    [(r, c, 7, 4.5, 0.005, "scene") for r, c in IMAGE_SHAPES]
    + [(r, c, k, 4.5, 0.005, "scene") for r, c in ((9, 130), (70, 33)) for k in (1, 2, 5, 9)]
    + [(3, 5, 15, 4.5, 0.005, "scene"), (4, 63, 9, 3.0, 0.02, "scene"), (1, 64, 2, 4.5, 0.005, "scene"), (70, 1, 7, 4.5, 0.005, "scene")]
    + [(5, 65, 5, 4.5, 0.005, "saturated"), (9, 130, 7, 4.5, 0.005, "saturated")]
    + [(70, 33, 7, 2.0, 0.05, "scene")]
)

VS0 = F32(1.0 / 128.0)  # a power of two: the z chain of the `inside` pose is exact, camz hits 0.0 on a plane
INTEGRATE_DIMS = [(17, 9, 1), (17, 9, 15), (17, 9, 16), (17, 9, 17), (17, 9, 33), (40, 24, 35), (65, 9, 2)]
POSES = ("identity", "rotated", "inside")
DISTS_SHAPE = (50, 67)


def rot_xy(deg_y, deg_x):
    ay, ax = np.deg2rad(deg_y), np.deg2rad(deg_x)
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    return (Ry @ Rx).astype(F32)


def dists_image(rows, cols, base, specials=True):
    """float32 ray lengths: a wavy surface around `base` metres, with patches of 0, negative, +inf and NaN among the valid pixels"""
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    d = (base * (1.0 + 0.16 * np.sin(0.11 * x) * np.cos(0.13 * y) + 0.002 * x)).astype(F32)
    if specials:
        s = hash_field((rows // 5 + 1, cols // 5 + 1), 77, 1.0)
        s = np.repeat(np.repeat(s, 5, 0), 5, 1)[:rows, :cols]  # 5 x 5 patches
        d = np.where(s > 0.92, F32(0), np.where(s > 0.84, F32(-0.3), np.where(s > 0.76, F32(np.inf), np.where(s > 0.68, F32(np.nan), d)))).astype(F32)
    return d


def integrate_case(dims, pose):
    """-> dict(dists, intr, vs, trunc, eta, R, t).  Anisotropic voxels throughout.
    identity: the volume in front of the camera, wider than the field of view on two sides.
    rotated:  about 25 deg about y composed with 15 deg about x; part of the image sees no voxel, part of the volume is out of view.
    inside:   the camera AT a voxel centre inside the volume, looking along +z (vs_z a power of two, so camz is exactly 0 on that
              voxel's plane: projections there are +-inf and, at the voxel itself, 0 / 0); planes behind it have camz < 0."""
    X, Y, Z = dims
    rows, cols = DISTS_SHAPE
    intr = tuple(F32(v) for v in (80.0, 91.0, 30.3, 27.6))
    if pose == "inside":  # all exact along y: the voxels 1 up / 5 ahead (2 / 10, ...) of the camera project to 89.5 * 0.25 + 27.625 = 50.0 == rows
        intr = tuple(F32(v) for v in (80.0, 89.5, 30.3, 27.625))  # (and no other voxel of these volumes onto a whole pixel row)
    trunc, eta = F32(5) * VS0, F32(2) * VS0
    if pose == "inside":
        vs = (F32(0.8) * VS0, F32(1.25) * VS0, VS0)
        i0, j0, k0 = X // 2, Y // 2, min(Z // 3, Z - 1)
        vc = [(F32(n) * v + v / F32(2)).astype(F32) for n, v in ((i0, vs[0]), (j0, vs[1]))]
        t = np.array([-vc[0], -vc[1], -(F32(k0) + F32(0.5)) * VS0], F32)
        R = np.eye(3, dtype=F32)
        dists = dists_image(rows, cols, 0.09)
    else:
        vs = (VS0, F32(1.25) * VS0, F32(0.8) * VS0)
        ext = np.array([X * float(vs[0]), Y * float(vs[1]), Z * float(vs[2])])
        if pose == "identity":
            R = np.eye(3, dtype=F32)
            t = np.array([-0.5 * ext[0] + 0.013, -0.5 * ext[1] - 0.007, 0.4], F32)
        else:
            R = rot_xy(25.0, 15.0)
            t = (np.array([0.02, -0.01, 0.4 + 0.5 * ext[2]]) - R.astype(np.float64) @ (0.5 * ext)).astype(F32)
        dists = dists_image(rows, cols, 0.4 + 0.5 * ext[2])
    return dict(dists=dists, intr=intr, vs=np.array(vs, F32), trunc=trunc, eta=eta, R=R, t=t)


INTEGRATE_CASES = [(d, p) for d in INTEGRATE_DIMS for p in POSES]

TILE_DIMS = (40, 24, 35)
TILE_BASES = [(0, 0, 0), (17, 0, 0), (0, 9, 16), (17, 9, 17)]


def find_ties(dims, case):
    """Under the identity pose camz is vs_z / 2 + t_z followed by one float32 addition of vs_z per plane.  For each target T in
    (trunc, -trunc, -eta): a plane k and a float32 Dp with fl(Dp - camz_k) == T exactly -> {name: (k, Dp)} (a target may be missing)."""
    camz = integrate32_chain(dims, case["vs"], np.eye(3, dtype=F32), case["t"], case["intr"])[0][:, 0, 0]
    found = {}
    for name, T in (("trunc", case["trunc"]), ("-trunc", -case["trunc"]), ("-eta", -case["eta"])):
        for k in range(1, dims[2]):
            up = dn = F32(camz[k] + F32(T))
            c = [up]
            for _ in range(4):  # a few float32 neighbours of camz_k + T on either side
                up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
                c += [up, dn]
            c = np.array(c, F32)
            hit = c[((c - camz[k]).astype(F32) == F32(T)) & (c > 0)]
            if hit.size and name not in found:
                found[name] = (k, F32(hit[0]))
    return found


BUILDER_DIMS = [(17, 9, 5), (33, 16, 17), (65, 9, 2), (16, 16, 31)]
VSB = F32(0.3 / 33.0)


def builder_case(kind, dims):
    """-> dict(vs, trunc, eta, params): anisotropic voxels (v, 1.25 v, 0.8 v), shapes sized to the volume so every one has cells
    inside, outside and in the unclamped band"""
    vs = np.array([VSB, F32(1.25) * VSB, F32(0.8) * VSB], F32)
    ext = np.array(dims, np.float64) * vs.astype(np.float64)
    m = float(ext.max())
    params = {"sphere": (0.47 * ext[0], 0.55 * ext[1], 0.4 * ext[2], 0.3 * m), "box": (0.3 * ext[0], 0.27 * ext[1], 0.22 * ext[2]),
              "ellipsoid": (0.4 * ext[0], 0.35 * ext[1], 0.3 * ext[2]), "plane": (0.55 * ext[2],), "torus": (0.3 * m, 0.08 * m)}[kind]
    return dict(vs=vs, trunc=F32(3) * VSB, eta=F32(2) * VSB, params=tuple(F32(v) for v in params))


def oracle_prim(oracle, kind, dims, c):
    v = oracle.new_volume(dims)
    p = c["params"]
    if kind == "sphere":
        oracle.init_sphere(v, c["vs"], c["trunc"], c["eta"], p[:3], p[3])
    elif kind == "plane":
        oracle.init_plane(v, c["vs"], c["trunc"], p[0])
    else:
        getattr(oracle, "init_" + kind)(v, c["vs"], c["trunc"], p)
    return v


# ---- pitched images ----------------------------------------------------------------------------------------------------------------
U16_PAD, F32_PAD = 7, 3          # odd element paddings; the float step stays a multiple of 4 bytes
U16_SENTINEL = np.uint16(60001)  # large: a kernel that reads it as depth wraps the bilateral's square / loses the pixel to truncate
F32_SENTINEL = F32(1.0e6)        # large and positive: read as a distance it would clamp the cell to +1


def padded(img, pad, sentinel, guard_rows=0):
    """-> (buffer (rows + guard_rows, cols + pad) filled with the sentinel outside the image, view of the image inside it, step in bytes)"""
    rows, cols = img.shape
    buf = np.full((rows + guard_rows, cols + pad), sentinel, img.dtype)
    buf[:rows, :cols] = img
    return buf, buf[:rows, :cols], buf.strides[0]


def oracle_bilateral(oracle, src, dst, ksz, ss, sd):
    """the oracle on strided views (src uint16, dst uint16 written in place)"""
    import ctypes as C

    oracle.lib().so_bilateral(C.c_void_p(src.ctypes.data), C.c_int(src.strides[0]), C.c_void_p(dst.ctypes.data), C.c_int(dst.strides[0]),
                              C.c_int(src.shape[0]), C.c_int(src.shape[1]), C.c_int(ksz), C.c_float(ss), C.c_float(sd))


def oracle_truncate(oracle, img, max_dist_m):
    import ctypes as C

    oracle.lib().so_truncate_depth(C.c_void_p(img.ctypes.data), C.c_int(img.strides[0]), C.c_int(img.shape[0]), C.c_int(img.shape[1]),
                                   C.c_float(max_dist_m))


def oracle_dists(oracle, depth, dists, intr):
    import ctypes as C

    oracle.lib().so_compute_dists(C.c_void_p(depth.ctypes.data), C.c_int(depth.strides[0]), C.c_void_p(dists.ctypes.data),
                                  C.c_int(dists.strides[0]), C.c_int(depth.shape[0]), C.c_int(depth.shape[1]), *[C.c_float(float(v)) for v in intr])
