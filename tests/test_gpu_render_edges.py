"""The TSDF raycaster and the two shaders (sobfu_amd/csrc/render_kernels.hip) against the numpy restatement tests/render_reference.py,
BIT FOR BIT, on the cases of tests/render_cases.py (tests/test_render_cases_cpu.py proves on the CPU that each reaches the edge it is
named for): points and normals as uint32 of every pixel, misses included, the shaders' images as bytes.  Also pitched outputs with
untouched padding, the shaders on hand-built inputs (saturation, half-way values, NaN, -0, a light at the point), NaN weights through
ops.sample_tsdf, rejected arguments that write nothing, and repeatability."""
import ctypes as C

import numpy as np
import pytest

import mesh_warp_reference as MW
import render_cases as K
import render_reference as RR

pytestmark = pytest.mark.gpu
F = np.float32
LIGHTS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (0.0, 0.0, 5.0))  # the headlight, off-axis, behind the surfaces


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def assert_same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def _raycast(c, vol=None, **kw):
    import torch

    from sobfu_amd import ops

    vol = torch.from_numpy(np.array(c["vol"])).cuda() if vol is None else vol
    return ops.raycast(vol, c["vs"], c["trunc"], c["R"], c["t"], c["intr"], rows=c["rows"], cols=c["cols"], step_factor=c["step_factor"], **kw)


@pytest.mark.parametrize("name", K.CASES)
def test_case_bit_for_bit(name):
    import torch

    from sobfu_amd import ops

    c, ref = K.case(name), K.reference(name)
    p, n = _raycast(c)
    imgs = [ops.render_image(p, n, light=l) for l in LIGHTS]
    col = ops.render_normals(n)
    torch.cuda.synchronize()
    p, n = p.cpu().numpy(), n.cpu().numpy()
    assert_same_bits(n[..., 3], ref["normals"][..., 3], f"{name}: hit flags")
    assert_same_bits(p, ref["points"], f"{name}: points")
    assert_same_bits(n, ref["normals"], f"{name}: normals")
    for l, img in zip(LIGHTS, imgs):
        assert_same_bits(img.cpu().numpy(), RR.render_image(p, n, l), f"{name}: render_image, light {l}")
    assert_same_bits(col.cpu().numpy(), RR.render_normals(n), f"{name}: render_normals")


def _wide(rows, cols, extra, lead, dtype, fill):
    """a (rows, cols + extra, 4) buffer filled with `fill` and its column slice [lead, lead + cols)"""
    import torch

    while ((cols + extra) * 4 * torch.empty(0, dtype=dtype).element_size()) % 64 == 0:  # no row step a multiple of 64 bytes
        extra += 1
    buf = torch.full((rows, cols + extra, 4), fill, dtype=dtype, device="cuda")
    return buf, buf[:, lead:lead + cols]


def _padding_untouched(buf, lead, cols, fill):
    b = buf.cpu().numpy()
    pad = np.concatenate([b[:, :lead].ravel(), b[:, lead + cols:].ravel()])
    return pad.size > 0 and (_bits(pad) == _bits(np.array([fill], b.dtype))[0]).all()


@pytest.mark.parametrize("name", ["size_17x65", "size_7x9", "rotated"])
def test_pitched_outputs(name):
    """raycast and both shaders into column slices of wider, sentinel-filled buffers whose row steps are no multiples of 64 bytes: the
    image part is the contiguous result, the padding keeps its sentinel; called twice into the same buffers"""
    import torch

    from sobfu_amd import ops

    c, ref = K.case(name), K.reference(name)
    rows, cols = c["rows"], c["cols"]
    vol = torch.from_numpy(np.array(c["vol"])).cuda()
    sent = -123.25
    pbuf, pv = _wide(rows, cols, 3, 1, torch.float32, sent)
    nbuf, nv = _wide(rows, cols, 5, 2, torch.float32, sent)
    ibuf, iv = _wide(rows, cols, 7, 3, torch.uint8, 0xA5)
    cbuf, cv = _wide(rows, cols, 9, 5, torch.uint8, 0x5A)
    for t_, size in ((pv, 4), (nv, 4), (iv, 1), (cv, 1)):
        assert (t_.stride(0) * size) % 64 != 0 and t_.stride(0) * size > cols * 4 * size
    for _ in range(2):
        rp, rn = _raycast(c, vol=vol, points=pv, normals=nv)
        assert rp is pv and rn is nv
        assert ops.render_image(pv, nv, light=LIGHTS[1], image=iv) is iv
        assert ops.render_normals(nv, image=cv) is cv
        torch.cuda.synchronize()
        assert_same_bits(pv.cpu().numpy(), ref["points"], "pitched points")
        assert_same_bits(nv.cpu().numpy(), ref["normals"], "pitched normals")
        assert_same_bits(iv.cpu().numpy(), RR.render_image(ref["points"], ref["normals"], LIGHTS[1]), "pitched image")
        assert_same_bits(cv.cpu().numpy(), ref["colours"], "pitched normal colours")
        assert _padding_untouched(pbuf, 1, cols, sent) and _padding_untouched(nbuf, 2, cols, sent)
        assert _padding_untouched(ibuf, 3, cols, 0xA5) and _padding_untouched(cbuf, 5, cols, 0x5A)
    # pitched inputs of the shaders into contiguous outputs
    assert_same_bits(ops.render_image(pv, nv).cpu().numpy(), ref["image"], "image from pitched inputs")
    assert_same_bits(ops.render_normals(nv).cpu().numpy(), ref["colours"], "colours from pitched inputs")


def _half_way(fn, inverse):
    """float32 x with fn(x) exactly k + 0.5 for some integer k in 0 .. 254 (to_byte then adds 0.5 and lands on an integer)"""
    out = []
    for k in range(255):
        x0 = F(inverse(k + 0.5))
        for x in (x0, np.nextafter(x0, F(2)), np.nextafter(x0, F(-2))):
            if fn(F(x)) == F(k + 0.5):
                out.append(F(x))
                break
    return np.array(out, F)


def _shade_value(c):  # render_image of normal (0, 0, -c) at (0, 0, 1) under the headlight: n . l = c
    return F(255) * (F(0.2) + F(0.8) * c)


def _hand_built(rows, cols, light, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (rows, cols, 4)).astype(F)
    p[..., 2] += F(1.5)
    p[..., 3] = 0
    n = rng.standard_normal((rows, cols, 4)).astype(F)
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    n[..., 3] = 1
    flat_p, flat_n = p.reshape(-1, 4), n.reshape(-1, 4)
    specials = []  # (tag, point, normal)
    for s in (3.0, -3.0, 40.0, -40.0):  # non-unit: saturates above 255 and below 0
        specials += [("big", (0.0, 0.0, 1.0, 0.0), (s, -s, -s, 1.0)), ("big", (0.1, 0.2, 1.0, 0.0), (-s, s, s, 1.0))]
    for w in (1.0, 2.0, -0.0, 0.0, np.nan):  # -0.0 and 0 are misses; NaN != 0: a hit
        specials += [("w", (0.1, -0.1, 0.8, 0.0), (0.0, -0.6, -0.8, w))]
    for k in range(3):  # NaN normal components
        v = [0.3, -0.5, -0.8, 1.0]
        v[k] = np.nan
        specials += [("nan", (0.0, 0.1, 1.0, 0.0), tuple(v))]
    specials += [("nan", (np.nan, 0.0, 1.0, 0.0), (0.0, 0.0, -1.0, 1.0)), ("nan", (0.0, 0.0, np.inf, 0.0), (0.0, 0.0, -1.0, 1.0))]
    # the light exactly at the point: ll == 0, 0 / 0 = NaN, fmaxf(0, NaN) = 0: grey 51
    at = tuple(float(F(v)) for v in light) + (0.0,)
    specials += [("at_light", at, (0.0, 0.0, -1.0, 1.0)), ("at_light", at, (0.6, 0.0, 0.8, 2.0))]
    halves_n = _half_way(lambda x: (x * F(0.5) + F(0.5)) * F(255), lambda y: (y / 255 - 0.5) * 2)
    halves_c = _half_way(_shade_value, lambda y: (y / 255 - 0.2) / 0.8)
    halves_c = halves_c[halves_c > 0]  # max(0, n . l) cuts the others off
    assert len(halves_n) >= 40 and len(halves_c) >= 20 and F(0) in halves_n
    halves_n = np.concatenate([[F(0)], halves_n[::len(halves_n) // 40][:40]]).astype(F)  # a spread of them: 3 x 65 pixels hold them all
    halves_c = halves_c[::len(halves_c) // 20][:20]
    for i, x in enumerate(halves_n):
        specials += [("half_n", (0.0, 0.0, 1.0, 0.0), (x, halves_n[(i + 7) % len(halves_n)], halves_n[(i + 13) % len(halves_n)], 1.0))]
    for x in halves_c:
        specials += [("half_c", (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, -x, 1.0))]
    assert len(specials) < rows * cols
    where = rng.permutation(rows * cols)[:len(specials)]
    tags = {}
    for i, (tag, pp, nn) in zip(where, specials):
        flat_p[i], flat_n[i] = pp, nn
        tags.setdefault(tag, []).append(int(i))
    return p, n, tags


@pytest.mark.parametrize("rows,cols", [(3, 65), (5, 130)])
def test_shaders_on_hand_built_inputs(rows, cols):
    import torch

    from sobfu_amd import ops

    for k, light in enumerate(LIGHTS + ((0.25, -0.5, 0.75),)):
        p, n, tags = _hand_built(rows, cols, light, 100 + k)
        want_img, want_col = RR.render_image(p, n, light), RR.render_normals(n)
        # the restatement itself: a light at the point gives grey 51; misses are 0; NaN w is a hit
        assert (want_img.reshape(-1, 4)[tags["at_light"]] == (51, 51, 51, 255)).all()
        assert (want_img[..., 3] == 255).sum() == rows * cols - 2 and (want_col[..., 3] == 0).sum() == 2
        assert set(np.unique(want_col)) >= {0, 255} and set(np.unique(want_img)) >= {0, 51, 255}
        if k == 0:  # the half-way values round up, to k + 1
            g = want_img.reshape(-1, 4)[tags["half_c"], 0].astype(np.float64)
            assert np.array_equal(g, _shade_value(-n.reshape(-1, 4)[tags["half_c"], 2]).astype(np.float64) + 0.5)
        x = n.reshape(-1, 4)[tags["half_n"], 0]
        assert np.array_equal(want_col.reshape(-1, 4)[tags["half_n"], 2].astype(np.float64), ((x * F(0.5) + F(0.5)) * F(255)).astype(np.float64) + 0.5)
        dp, dn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
        img, col = ops.render_image(dp, dn, light=light), ops.render_normals(dn)
        torch.cuda.synchronize()
        assert_same_bits(img.cpu().numpy(), want_img, f"render_image, light {light}")
        assert_same_bits(col.cpu().numpy(), want_col, "render_normals")
        assert_same_bits(dp.cpu().numpy(), p, "the points, unchanged")
        assert_same_bits(dn.cpu().numpy(), n, "the normals, unchanged")


def test_nan_weights_through_sample_tsdf():
    """ops.sample_tsdf shares the raycaster's sampler: a NaN weight among the corners makes the sample invalid (NaN), like a weight of 0"""
    import torch

    from sobfu_amd import ops

    c, ref = K.case("nan_weight"), K.reference("outside")
    vol = np.array(c["vol"])
    planted = np.argwhere(np.isnan(vol[..., 1]))
    assert 1 <= len(planted) <= 3
    R64, t64 = c["R"].astype(np.float64), c["t"].astype(np.float64)
    off = np.array([[0.3, 0.3, -0.3], [-0.4, 0.2, 0.1], [0.0, 0.0, 0.0], [-0.6, -0.7, -0.2]])
    near = [(R64 @ ((np.array([x, y, z]) + o + 0.5) * c["vs"].astype(np.float64)) + t64) for z, y, x in planted for o in off]
    pts = np.concatenate([ref["points"][ref["normals"][..., 3] != 0], np.concatenate([np.array(near), np.zeros((len(near), 1))], 1).astype(F)]).astype(F)
    want = MW.sample_tsdf(vol, c["vs"], c["R"], c["t"], pts)
    one = vol.copy()
    one[..., 1][np.isnan(one[..., 1])] = 1
    differ = np.isnan(want) & ~np.isnan(MW.sample_tsdf(one, c["vs"], c["R"], c["t"], pts))
    assert differ.sum() >= 3 and (~np.isnan(want)).sum() >= 100  # samples that only the NaN weight makes invalid
    got = ops.sample_tsdf(torch.from_numpy(vol).cuda(), c["vs"], c["R"], c["t"], torch.from_numpy(pts).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert_same_bits(got[~np.isnan(want)], want[~np.isnan(want)], "sample_tsdf")


def _strided(base, shape, row_stride, offset=0):
    import torch

    return torch.as_strided(base, shape, (row_stride, shape[2], 1), offset)


def test_bad_arguments_are_rejected_and_write_nothing():
    import torch

    from sobfu_amd import _lib, ops
    from sobfu_amd._lib import HipError

    c = K.case("size_7x9")
    rows, cols = c["rows"], c["cols"]
    vol = torch.from_numpy(np.array(c["vol"])).cuda()
    sent = 7.5
    flat_p = torch.full((rows * cols * 4 + 64,), sent, dtype=torch.float32, device="cuda")
    flat_n = torch.full_like(flat_p, sent)
    flat_i = torch.full((rows * cols * 4 + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    P, N, I = (_strided(f, (rows, cols, 4), cols * 4) for f in (flat_p, flat_n, flat_i))

    def untouched():
        torch.cuda.synchronize()
        return bool((flat_p == sent).all().item() and (flat_n == sent).all().item() and (flat_i == 0x3C).all().item())

    def rejected(fn, code=-1):
        with pytest.raises(HipError) as e:
            fn()
        assert f"(code {code})" in str(e.value), str(e.value)
        assert untouched()

    def cast(vol=vol, points=P, normals=N, **kw):
        a = dict(vs=c["vs"], trunc=c["trunc"], R=c["R"], t=c["t"], intr=c["intr"], rows=rows, cols=cols, step_factor=0.75)
        a.update(kw)
        return ops.raycast(vol, a["vs"], a["trunc"], a["R"], a["t"], a["intr"], rows=a["rows"], cols=a["cols"], step_factor=a["step_factor"],
                           points=points, normals=normals)

    # volumes thinner than 2 voxels on an axis
    for shape in ((1, 4, 4, 2), (4, 1, 4, 2), (4, 4, 1, 2)):
        rejected(lambda: cast(vol=torch.ones(shape, dtype=torch.float32, device="cuda")))
    for kw in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(cols=-3)):
        rejected(lambda: cast(**kw))
    # a row step below cols * 16; a step off its alignment; a pointer off its alignment (a view offset by one element)
    short = _strided(flat_p, (rows, cols, 4), (cols - 1) * 4)
    odd = _strided(flat_p, (rows, cols, 4), cols * 4 + 1)
    off = _strided(flat_p, (rows, cols, 4), cols * 4, 1)
    for bad in (short, odd, off):
        rejected(lambda: cast(points=bad))
        rejected(lambda: cast(normals=bad))
        rejected(lambda: ops.render_image(bad, N, image=I))
        rejected(lambda: ops.render_image(P, bad, image=I))
        rejected(lambda: ops.render_normals(bad, image=I))
    for bad in (_strided(flat_i, (rows, cols, 4), (cols - 1) * 4), _strided(flat_i, (rows, cols, 4), cols * 4 + 1), _strided(flat_i, (rows, cols, 4), cols * 4, 1)):
        rejected(lambda: ops.render_image(P, N, image=bad))
        rejected(lambda: ops.render_normals(N, image=bad))
    # rows or cols < 1 of the shaders (the front end takes them from the tensors: the C ABI directly)
    L = _lib.lib()
    pp, np_, ip = (C.c_void_p(t_.data_ptr()) for t_ in (flat_p, flat_n, flat_i))
    z = C.c_float(0)
    for r_, c_ in ((0, cols), (rows, 0), (-1, cols)):
        assert L.sobfu_hip_render_image(pp, C.c_int(cols * 16), np_, C.c_int(cols * 16), C.c_int(r_), C.c_int(c_), z, z, z, ip, C.c_int(cols * 4), None) == -1
        assert L.sobfu_hip_render_normals(np_, C.c_int(cols * 16), C.c_int(r_), C.c_int(c_), ip, C.c_int(cols * 4), None) == -1
    assert untouched()
    # voxel size, truncation distance, step factor: zero, negative, NaN, Inf
    for bad in (0.0, -0.01, np.nan, np.inf):
        for axis in range(3):
            vs = c["vs"].copy()
            vs[axis] = bad
            rejected(lambda: cast(vs=vs))
        rejected(lambda: cast(trunc=bad))
        rejected(lambda: cast(step_factor=bad))
    fx, fy, cx, cy = c["intr"]
    for intr in ((0.0, fy, cx, cy), (fx, 0.0, cx, cy), (fx, fy, np.nan, cy), (fx, fy, cx, np.nan), (np.inf, fy, cx, cy), (fx, fy, cx, np.inf)):
        rejected(lambda: cast(intr=intr))
    # a non-finite pose, anywhere in R or t (as sobfu_hip_mesh_render rejects it)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(9):
            R = c["R"].copy()
            R.reshape(-1)[k] = bad
            rejected(lambda: cast(R=R))
        for k in range(3):
            t = c["t"].copy()
            t[k] = bad
            rejected(lambda: cast(t=t))
    # a step so small that the bound on the steps of a march reaches 10^6: unsupported
    rejected(lambda: cast(step_factor=1e-7), code=-3)
    ext = np.sqrt((((np.array(K.dims_of(c["vol"])) - 1) * c["vs"].astype(np.float64)) ** 2).sum())
    assert ext / float(F(1e-7) * c["vs"].min()) + 2 >= 1e6
    # and the same buffers take a good call
    cast()
    torch.cuda.synchronize()
    assert_same_bits(P.cpu().numpy(), K.reference("size_7x9")["points"], "points after the rejected calls")
    assert (flat_p[rows * cols * 4:] == sent).all().item()


def test_repeatable_and_the_volume_is_read_only():
    import torch

    for name in ("rotated", "nan_tsdf", "vol_2x2x2"):
        c = K.case(name)
        host = np.array(c["vol"])
        vol = torch.from_numpy(host).cuda()
        p1, n1 = _raycast(c, vol=vol)
        p2, n2 = _raycast(c, vol=vol)
        p3, n3 = _raycast(c, vol=torch.from_numpy(host.copy()).cuda())
        torch.cuda.synchronize()
        for a in (p2, p3):
            assert_same_bits(a.cpu().numpy(), p1.cpu().numpy(), f"{name}: points again")
        for a in (n2, n3):
            assert_same_bits(a.cpu().numpy(), n1.cpu().numpy(), f"{name}: normals again")
        assert_same_bits(vol.cpu().numpy(), host, f"{name}: the volume")
