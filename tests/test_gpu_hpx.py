"""GPU checks of the HEALPix pixel functions (utils.pixelfunc, Runners.regrid_pixels_hpix) against the numpy helper
(hpx_oracle.py) and the refshim restatement of healpix_cxx get_interpol."""
import numpy as np
import pytest

import hpx_oracle as H
from baryonification_amd import utils as U
from baryonification_amd.Runners import regrid_pixels_hpix

pytestmark = pytest.mark.gpu


def _points(nside, n, rng):
    """random points plus both polar caps and phi next to 0 and 2 pi, none within 1e-12 rad of a ring's colatitude"""
    th = np.concatenate([np.arccos(rng.uniform(-1, 1, n)), rng.uniform(0, 0.2 / nside, n // 8), np.pi - rng.uniform(0, 0.2 / nside, n // 8),
                         [0.0, np.pi], np.arccos(rng.uniform(-1, 1, 8))])
    ph = np.concatenate([rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n // 4), [0.3, 1.7],
                         [0.0, 1e-15, 1e-9, 2 * np.pi - 1e-9, np.nextafter(2 * np.pi, 0), 2 * np.pi - 1e-15, 1e-300, 5e-324]])
    rings = H.hp._ring_theta(nside, np.arange(1, 4 * nside))
    d = np.abs(th[:, None] - rings[None, :]).min(1) if nside <= 64 else \
        np.minimum(np.abs(th - rings[np.clip(np.searchsorted(rings, th), 0, rings.size - 1)]),
                   np.abs(th - rings[np.clip(np.searchsorted(rings, th) - 1, 0, rings.size - 1)]))
    keep = d > 1e-12
    return th[keep], ph[keep]


@pytest.mark.parametrize('nside', [1, 2, 3, 4, 64, 1024, 8192])
def test_interp_weights_match_oracle(gpu, nside):
    rng = np.random.default_rng(nside)
    th, ph = _points(nside, 20000, rng)
    pix, w = U.get_interp_weights(nside, th, ph)
    opix, ow = H.get_interp_weights(nside, th, ph)
    assert pix.shape == (4, th.size) and pix.dtype == np.int64 and w.dtype == np.float64
    assert np.array_equal(pix, opix)
    # the colatitude weight divides theta - theta_ring (libm acos / atan2 / cos, 1 ulp apart between the device and numpy) by the
    # ring spacing ~ 1 / nside: 1e-13 up to nside 64, growing with nside beyond (8192: 1.3e-11)
    tol = 1e-13 * max(1.0, nside / 64)
    assert np.abs(w - ow).max() <= tol
    assert np.abs(w.sum(0) - 1).max() < 1e-13
    if nside & (nside - 1) == 0:
        pn, wn = U.get_interp_weights(nside, th, ph, nest=True)
        assert np.array_equal(pn, H.ring2nest(nside, pix)) and np.array_equal(wn, w)
    # phi outside [0, 2 pi) is reduced first (fmod, exact), then the rule applies
    for shift in (4 * np.pi, -2 * np.pi):
        ps = ph[:500] + shift
        red = np.mod(ps, 2 * np.pi)
        ok = red < 2 * np.pi
        pix2, w2 = U.get_interp_weights(nside, th[:500][ok], ps[ok])
        opix2, ow2 = H.get_interp_weights(nside, th[:500][ok], red[ok])
        assert np.array_equal(pix2, opix2) and np.abs(w2 - ow2).max() <= tol


def test_interp_weights_lonlat_scalar_and_docstrings(gpu):
    rng = np.random.default_rng(5)
    lon, lat = rng.uniform(0, 360, 3000), rng.uniform(-90, 90, 3000)
    p1, w1 = U.get_interp_weights(256, lon, lat, lonlat=True)
    p2, w2 = U.get_interp_weights(256, np.pi / 2 - np.radians(lat), np.radians(lon))
    assert np.array_equal(p1, p2) and np.array_equal(w1, w2)
    # >>> hp.get_interp_weights(1, 0) -> ([0, 1, 4, 5], [1., 0., 0., 0.])
    p, w = U.get_interp_weights(1, 0)
    assert p.shape == (4,) and p.tolist() == [0, 1, 4, 5] and np.abs(w - [1, 0, 0, 0]).max() < 1e-15
    # >>> hp.get_interp_weights(1, 0, 0) -> ([1, 2, 3, 0], [0.25, 0.25, 0.25, 0.25]); the same with (0, 90, lonlat=True)
    for args, kw in (((0, 0), {}), ((0, 90), {'lonlat': True})):
        p, w = U.get_interp_weights(1, *args, **kw)
        assert p.tolist() == [1, 2, 3, 0] and np.abs(w - 0.25).max() < 1e-15
    # >>> hp.get_interp_weights(1, [0, np.pi / 2], 0) -> [[1, 4], [2, 5], [3, 11], [0, 8]], [[.25, 1], [.25, 0], [.25, 0], [.25, 0]]
    p, w = U.get_interp_weights(1, [0, np.pi / 2], 0)
    assert p.tolist() == [[1, 4], [2, 5], [3, 11], [0, 8]]
    assert np.abs(w - [[.25, 1], [.25, 0], [.25, 0], [.25, 0]]).max() < 1e-15


@pytest.mark.parametrize('nside,nest', [(1, False), (3, False), (4, False), (4, True), (64, False), (64, True), (2048, True)])
def test_interp_weights_of_pixel_centres(gpu, nside, nest):
    npix = 12 * nside * nside
    ip = np.arange(npix) if npix < 200000 else np.random.default_rng(1).integers(0, npix, 200000)
    pix, w = U.get_interp_weights(nside, ip, nest=nest)
    onpix = (pix == ip[None, :])
    tol = 1e-13 * max(1.0, nside / 64)             # the azimuth weight: phi / (2 pi / nr) rounds at the level of nr ulp
    assert np.abs((w * onpix).sum(0) - 1).max() < tol and np.abs((w * ~onpix).sum(0)).max() < tol
    if not nest:                                   # the same point through the angle path
        th, ph = H.hp.pix2ang(nside, ip)
        p2, w2 = U.get_interp_weights(nside, th, ph)
        assert np.abs((w2 * (p2 == ip[None, :])).sum(0) - 1).max() < 1e-12
    if nside == 1:
        assert pix[:, 0].tolist() == [0, 1, 4, 5]


@pytest.mark.parametrize('nmaps', [1, 3])
@pytest.mark.parametrize('nest', [False, True])
def test_interp_val(gpu, nmaps, nest):
    nside = 512
    rng = np.random.default_rng(nmaps + 10 * nest)
    m = rng.normal(size=(nmaps, 12 * nside * nside)) if nmaps > 1 else rng.normal(size=12 * nside * nside)
    th, ph = _points(nside, 100000, rng)
    v = U.get_interp_val(m, th, ph, nest=nest)
    pix, w = U.get_interp_weights(nside, th, ph, nest=nest)
    ref = (w * m[..., pix]).sum(-2)
    assert v.shape == ref.shape
    assert np.abs(v - ref).max() <= 1e-13 * np.abs(m).max()
    assert np.abs(U.get_interp_val(m.astype(np.float32), th, ph, nest=nest) - (w * m.astype(np.float32)[..., pix]).sum(-2)).max() < 1e-6 * np.abs(m).max()
    assert isinstance(U.get_interp_val(np.ones(12 * 16), 0.4, 0.2), float) or np.ndim(U.get_interp_val(np.ones(12 * 16), 0.4, 0.2)) == 0


def _scale(npix, pix, contrib):
    return np.bincount(np.mod(pix, npix).ravel(), np.abs(contrib).ravel(), minlength=npix).max()


def test_regrid_pixels_hpix_matches_add_at(gpu):
    rng = np.random.default_rng(7)
    npix, N = 12 * 64 * 64, 1000000
    pix = rng.integers(-npix, npix, (N, 4)).astype(np.int32)
    w = rng.uniform(-1, 1, (N, 4))
    vals = rng.normal(size=N)
    h0 = rng.normal(size=npix)
    h = h0.copy()
    out = regrid_pixels_hpix(h, vals, pix, w)
    assert out is h
    ref = h0.copy()
    np.add.at(ref, pix.astype(np.int64).ravel() % npix, (w * vals[:, None]).ravel())
    assert np.abs(h - ref).max() <= 1e-12 * _scale(npix, pix, w * vals[:, None])


def test_regrid_recipe_conserves_the_map(gpu):
    """the reference's own recipe (HealpixRunner.py:333-346): displaced pixel centres -> get_interp_weights(lonlat) -> transpose ->
    regrid_pixels_hpix"""
    nside = 1024
    npix = 12 * nside * nside
    rng = np.random.default_rng(11)
    orig = rng.uniform(0.5, 2.0, npix)
    vec = np.stack(H.hp.pix2vec(nside, np.arange(npix)), axis=1) + rng.normal(scale=3e-4, size=(npix, 3))
    lon, lat = H.hp.vec2ang(vec, lonlat=True)
    c_pix, c_w = U.get_interp_weights(nside, lon, lat, lonlat=True)
    c_pix, c_w = c_pix.T, c_w.T
    new = regrid_pixels_hpix(np.zeros(npix), orig, c_pix, c_w)
    assert np.isclose(new.sum(), orig.sum())
    ref = np.bincount(c_pix.ravel(), (c_w * orig[:, None]).ravel(), minlength=npix)
    assert np.abs(new - ref).max() <= 1e-12 * _scale(npix, c_pix, c_w * orig[:, None])


# ------------------------------------------------------------------------------------------------------------------ ud_grade
ORDERS = [('RING', 'RING'), ('RING', 'NESTED'), ('NEST', 'RING'), ('NESTED', 'NEST')]


@pytest.mark.parametrize('order_in,order_out', ORDERS)
@pytest.mark.parametrize('nside_in,nside_out,power,dtype', [(64, 1, None, None), (128, 32, -2, None), (256, 1024, None, None),
                                                           (32, 64, -2, None), (64, 16, None, np.float32), (16, 16, None, None)])
def test_ud_grade_matches_oracle(gpu, order_in, order_out, nside_in, nside_out, power, dtype):
    rng = np.random.default_rng(nside_in + nside_out)
    m = rng.normal(size=12 * nside_in ** 2)
    out = U.ud_grade(m, nside_out, order_in=order_in, order_out=order_out, power=power, dtype=dtype)
    ref = H.ud_grade(m, nside_out, order_in=order_in, order_out=order_out, power=power, dtype=dtype)
    assert out.dtype == ref.dtype and out.shape == ref.shape
    assert np.array_equal(out, ref)


def test_ud_grade_2d_float32_input_and_order_out_none(gpu):
    rng = np.random.default_rng(3)
    m = rng.normal(size=(3, 12 * 32 ** 2)).astype(np.float32)
    out = U.ud_grade(m, 8, order_in='NEST')
    assert out.dtype == np.float32 and out.shape == (3, 12 * 64)
    assert np.array_equal(out, H.ud_grade(m, 8, order_in='NEST', order_out='NEST'))
    out64 = U.ud_grade(m, 64, dtype=np.float64)
    assert out64.dtype == np.float64 and np.array_equal(out64, H.ud_grade(m, 64, dtype=np.float64))


@pytest.mark.parametrize('pess', [False, True])
@pytest.mark.parametrize('order_in', ['RING', 'NEST'])
def test_ud_grade_bad_children(gpu, pess, order_in):
    nside_in, nside_out = 64, 16
    rng = np.random.default_rng(21)
    m = rng.normal(size=12 * nside_in ** 2)
    bad = rng.random(m.size)
    m[bad < 0.05] = U.UNSEEN
    m[(bad >= 0.05) & (bad < 0.08)] = np.nan
    m[(bad >= 0.08) & (bad < 0.09)] = np.inf
    m[(bad >= 0.09) & (bad < 0.095)] = U.UNSEEN * (1 + 1e-7)               # inside mask_bad's tolerance
    # one output pixel with every child bad
    first = H.children(nside_in, nside_out, [0])[0]
    m[first if order_in == 'NEST' else H.nest2ring(nside_in, first)] = U.UNSEEN
    out = U.ud_grade(m, nside_out, pess=pess, order_in=order_in)
    ref = H.ud_grade(m, nside_out, pess=pess, order_in=order_in)
    assert np.array_equal(out, ref)
    assert np.isfinite(out).all() and (out == U.UNSEEN).any()
    if pess:
        assert (out == U.UNSEEN).mean() > 0.5


def test_ud_grade_2048_to_512_all_orders(gpu):
    nside_in, nside_out = 2048, 512
    rng = np.random.default_rng(2048)
    m_nest = rng.uniform(-1, 3, 12 * nside_in ** 2)
    u, v = H.child_order(nside_in // nside_out)
    perm = H._spread(u) + (H._spread(v) << 1)                     # NEST offsets of the children in the kernel's order
    vals = m_nest.reshape(-1, perm.size)[:, perm]
    ref_nest = H.fixed_order_sum(vals) / perm.size
    ref_ring = ref_nest[H.ring2nest(nside_out, np.arange(12 * nside_out ** 2))]
    m_ring = np.empty_like(m_nest)
    m_ring[H.nest2ring(nside_in, np.arange(m_nest.size))] = m_nest
    for oi, mi in (('RING', m_ring), ('NEST', m_nest)):
        for oo, ref in (('RING', ref_ring), ('NEST', ref_nest)):
            assert np.array_equal(U.ud_grade(mi, nside_out, order_in=oi, order_out=oo), ref), (oi, oo)
    # a pure reorder
    assert np.array_equal(U.ud_grade(m_nest, nside_in, order_in='NEST', order_out='RING'), m_ring)


def test_ud_grade_8192_to_2048_ring_on_device(gpu):
    import torch
    nside_in, nside_out = 8192, 2048
    g = torch.Generator(device='cuda').manual_seed(8192)
    m = torch.rand(12 * nside_in ** 2, dtype=torch.float64, device='cuda', generator=g)
    out = U.ud_grade(m, nside_out)
    assert out.is_cuda and out.dtype == torch.float64 and out.numel() == 12 * nside_out ** 2
    rel = abs(float(out.sum()) * 16 - float(m.sum())) / float(m.sum())
    assert rel <= 1e-12
    q = np.random.default_rng(3).integers(0, out.numel(), 100000)
    P = H.ring2nest(nside_out, q)
    ch = H.nest2ring(nside_in, H.children(nside_in, nside_out, P))
    vals = m[torch.from_numpy(ch.ravel()).cuda()].cpu().numpy().reshape(ch.shape)
    ref = H.fixed_order_sum(vals) / 16
    assert np.array_equal(out[torch.from_numpy(q).cuda()].cpu().numpy(), ref)
    del m, out
    torch.cuda.empty_cache()


def test_anafast_of_a_degraded_4096_map(gpu):
    import torch
    nside_in, nside_out = 4096, 1024
    rng = np.random.default_rng(4096)
    m_nest = rng.normal(size=12 * nside_in ** 2)
    u, v = H.child_order(4)
    perm = H._spread(u) + (H._spread(v) << 1)
    ref = (H.fixed_order_sum(m_nest.reshape(-1, 16)[:, perm]) / 16)[H.ring2nest(nside_out, np.arange(12 * nside_out ** 2))]
    md = torch.from_numpy(m_nest).cuda()
    low = U.ud_grade(md, nside_out, order_in='NEST', order_out='RING')
    del md
    cl = U.anafast(low)
    cl_ref = U.anafast(ref)
    cl = cl.cpu().numpy() if hasattr(cl, 'cpu') else cl
    assert np.abs(cl - cl_ref).max() <= 1e-11 * np.abs(cl_ref).max()
    assert np.array_equal(low.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------------------------ torch
def test_torch_tensors_stay_on_device(gpu):
    import torch
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(9)
    m = rng.normal(size=12 * 64 ** 2)
    mt = torch.from_numpy(m).to(dev)
    lo = U.ud_grade(mt, 16, power=-2)
    assert isinstance(lo, torch.Tensor) and lo.device == dev and np.array_equal(lo.cpu().numpy(), U.ud_grade(m, 16, power=-2))
    th, ph = _points(64, 5000, rng)
    tt, pt = torch.from_numpy(th).to(dev), torch.from_numpy(ph).to(dev)
    p, w = U.get_interp_weights(64, tt, pt)
    pn, wn = U.get_interp_weights(64, th, ph)
    assert p.device == dev and w.device == dev and np.array_equal(p.cpu().numpy(), pn) and np.array_equal(w.cpu().numpy(), wn)
    pi, wi = U.get_interp_weights(64, torch.arange(100, device=dev), nest=True)
    assert pi.device == dev and np.array_equal(pi.cpu().numpy(), U.get_interp_weights(64, np.arange(100), nest=True)[0])
    v = U.get_interp_val(mt, tt, pt)
    assert v.device == dev and np.array_equal(v.cpu().numpy(), U.get_interp_val(m, th, ph))
    h = torch.zeros(12 * 64 ** 2, dtype=torch.float64, device=dev)
    vals = torch.from_numpy(rng.normal(size=th.size)).to(dev)
    r = regrid_pixels_hpix(h, vals, p.T, w.T)
    assert r is h and h.device == dev
    ref = np.bincount(pn.T.ravel(), (wn.T * vals.cpu().numpy()[:, None]).ravel(), minlength=h.numel())
    assert np.abs(h.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
