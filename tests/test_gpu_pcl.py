"""Masked-sky power spectra on the GPU (baryonification_amd/utils/pseudocl.py, csrc/bfgx_pcl.hpp): the mode-coupling matrices against
exact 3j symbols, their sum rule and symmetry at large l, the convention end to end through the transforms, and the workspace's binning,
coupling and decoupling against the numpy restatement of tests/pcl_oracle.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import pcl_oracle as P
import sht_oracle as O
import sht_spin_oracle as OS
from baryonification_amd import _lib, utils as U

pytestmark = pytest.mark.gpu

SHAPES = P.SHAPES
# Per entry, the error bound is TOL times the absolute-sum scale (2l'+1)/(4 pi) sum (2l''+1) |W_l''| |product of symbols|.
# kind 0: at most 100 steps of the two-term recursion, a few roundings each.
# kinds 1 and 2: 16 x the error of pcl_oracle.recursion_matrices (the kernel's recursions in float64 numpy) against the exact matrices on
# these shapes and W, measured on the CPU: P.RECURSION_ERROR = 1.33e-15 for M0+, 2.27e-15 for M++ / M-- (capped at 1e-10).
TOL = {0: 1e-12, 1: min(16 * P.RECURSION_ERROR[1], 1e-10), 2: min(16 * P.RECURSION_ERROR[2], 1e-10)}
KEYS = {0: ('00',), 1: ('0+',), 2: ('++', '--')}


_wl = P.shape_wl


@functools.lru_cache(maxsize=None)
def _exact(lmax, lw):
    rows = P.shape_rows(lmax)
    return rows, P.exact_matrices(_wl(lmax, lw), lmax, rows=rows)


def _matrices(wl, lmax, kind):
    m = U.mode_coupling_matrix(wl, lmax, *{0: (0, 0), 1: (0, 2), 2: (2, 2)}[kind])
    return m if kind == 2 else (m,)


# ---------------------------------------------------------------------------------------------- 1. against the exact oracle
@pytest.mark.parametrize('kind', [0, 1, 2])
@pytest.mark.parametrize('lmax,lw', SHAPES)
def test_matrices_against_exact_3j(gpu, lmax, lw, kind):
    rows, exact = _exact(lmax, lw)
    got = _matrices(_wl(lmax, lw), lmax, kind)
    l = np.arange(lmax + 1)
    outside = np.abs(l[:, None] - l[None, :]) > lw
    if kind:
        outside |= (l[:, None] < 2) | (l[None, :] < 2)
    for key, m in zip(KEYS[kind], got):
        assert m.shape == (lmax + 1, lmax + 1) and m.dtype == np.float64
        assert np.all(m[outside] == 0.0), key
        ref, scale = exact[key]
        err = np.abs(m[rows] - ref)
        worst = (err / np.where(scale > 0, scale, 1.0)).max()
        print("kind %d %s (lmax %d, lw %d): max err / scale = %.3e (tol %.3e)" % (kind, key, lmax, lw, worst, TOL[kind]))
        assert np.all(err <= TOL[kind] * scale), (key, worst)


# ---------------------------------------------------------------------------------------------- 2. large l, no oracle
@functools.lru_cache(maxsize=None)
def _large():
    lmax, lw = 1535, 64
    wl = np.random.default_rng(7).random(lw + 1) + 0.1
    m00 = U.mode_coupling_matrix(wl, lmax)
    mpp, mmm = U.mode_coupling_matrix(wl, lmax, 2, 2)
    return lmax, lw, wl, m00, mpp, mmm


def test_large_l_row_sums(gpu):
    lmax, lw, wl, m00, mpp, mmm = _large()
    S = np.sum((2 * np.arange(lw + 1) + 1) * wl) / (4 * np.pi)
    # ~3100 recursion steps of at most 32 roundings each: 3100 * 32 * 1.1e-16 = 1.1e-11 < 1e-10
    e0 = np.abs(m00[:lmax - lw + 1].sum(axis=1) / S - 1).max()
    e2 = np.abs((mpp + mmm)[2:lmax - lw + 1].sum(axis=1) / S - 1).max()
    print("row sums: M00 %.3e, M++ + M-- %.3e" % (e0, e2))
    assert e0 <= 1e-10 and e2 <= 1e-10


def test_large_l_symmetry_and_band(gpu):
    lmax, lw, wl, m00, mpp, mmm = _large()
    l = np.arange(lmax + 1)
    g = 2.0 * l + 1.0
    outside = np.abs(l[:, None] - l[None, :]) > lw
    for name, m in (('M00', m00), ('M++', mpp), ('M--', mmm)):
        a = g[:, None] * m
        e = np.abs(a - a.T).max() / np.abs(a).max()
        print("symmetry %s: %.3e" % (name, e))
        assert e <= 1e-11, name
        assert np.all(m[outside] == 0.0), name
    assert np.all(mpp[:2] == 0) and np.all(mpp[:, :2] == 0) and np.all(mmm[:2] == 0) and np.all(mmm[:, :2] == 0)


def test_mask_spectrum_beyond_64_kib_of_lds(gpu):
    """lw = 8200 with lmax = 4100 puts 8201 values of W (65 992 B with the 48-entry table) into LDS, past the 64 KiB a kernel gets without
    asking.  Sampled entries against the same recursions in float64 numpy: with W > 0 the scale of an entry is its value, and both sides
    are within 4100 steps x 32 roundings x 1.1e-16 = 1.4e-11 of it, so they agree to 1e-10.  The matrices stay on the device."""
    import torch
    lmax, lw = 4100, 8200
    wl = (np.random.default_rng(8).random(lw + 1) + 0.1) / (1.0 + np.arange(lw + 1.0)) ** 2
    wd = torch.from_numpy(wl).cuda()
    m00 = U.mode_coupling_matrix(wd, lmax)
    mpp, mmm = U.mode_coupling_matrix(wd, lmax, 2, 2)
    pairs = [(0, 0), (2, 2), (4100, 4100), (4100, 0), (3, 4100), (2049, 2051), (4099, 2), (4100, 4037), (1000, 3000)]
    for l, lp in pairs:
        pre = (2 * lp + 1) / (4 * np.pi)
        ref0 = pre * P.recursion_entry(wl, l, lp, 0)
        rp, rm = (pre * x for x in P.recursion_entry(wl, l, lp, 2))
        got = [float(m[l, lp]) for m in (m00, mpp, mmm)]
        print("(%d, %d): M00 %.3e, M++ %.3e, M-- %.3e" % (l, lp, abs(got[0] / ref0 - 1), abs(got[1] - rp) / max(rp, 1e-300), abs(got[2] - rm) / max(rm, 1e-300)))
        assert abs(got[0] - ref0) <= 1e-10 * ref0
        assert abs(got[1] - rp) <= 1e-10 * rp and abs(got[2] - rm) <= 1e-10 * rm
    g = 2.0 * torch.arange(lmax + 1, dtype=torch.float64, device='cuda') + 1.0
    for m in (m00, mpp, mmm):
        a = g[:, None] * m
        assert float((a - a.T).abs().max() / a.abs().max()) <= 1e-11


# ---------------------------------------------------------------------------------------------- 3. constant mask
@pytest.mark.parametrize('lmax', [0, 5, 130])
def test_constant_mask(gpu, lmax):
    c = 0.7
    wl = np.array([4 * np.pi * c * c, 0.0, 0.0])
    eye = np.eye(lmax + 1)
    assert np.abs(U.mode_coupling_matrix(wl, lmax) - c * c * eye).max() <= 1e-14
    mpp, mmm = U.mode_coupling_matrix(wl, lmax, 2, 2)
    eye[:2] = 0
    assert np.abs(mpp - c * c * eye).max() <= 1e-14
    assert np.abs(mmm).max() <= 1e-14
    assert np.abs(U.mode_coupling_matrix(wl, lmax, 0, 2) - c * c * eye).max() <= 1e-14
    assert np.array_equal(U.mode_coupling_matrix(wl, lmax, 2, 0), U.mode_coupling_matrix(wl, lmax, 0, 2))


# ---------------------------------------------------------------------------------------------- 4. one code path
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_host_device_and_python_entries_agree_bit_for_bit(gpu, kind):
    import torch
    lmax, lw = 70, 12
    wl = _wl(lmax, lw)
    n = lmax + 1
    L = _lib.load()
    host = [np.full((n, n), np.nan), np.full((n, n), np.nan)]
    _lib.check(L.bfgx_pcl_coupling(0, lmax, lw, kind, wl.ctypes.data, host[0].ctypes.data, host[1].ctypes.data if kind == 2 else None))
    wd = torch.from_numpy(wl).cuda()
    dev = [torch.full((n, n), float('nan'), dtype=torch.float64, device='cuda') for _ in range(2)]
    _lib.check(L.bfgx_pcl_coupling_device(0, None, lmax, lw, kind, C.c_void_p(wd.data_ptr()), C.c_void_p(dev[0].data_ptr()),
                                          C.c_void_p(dev[1].data_ptr()) if kind == 2 else None))
    torch.cuda.synchronize()
    py = U.mode_coupling_matrix(wd, lmax, *{0: (0, 0), 1: (0, 2), 2: (2, 2)}[kind])
    py = py if kind == 2 else (py,)
    again = _matrices(wl, lmax, kind)
    for i in range(2 if kind == 2 else 1):
        assert py[i].is_cuda and py[i].dtype == torch.float64
        assert host[i].tobytes() == dev[i].cpu().numpy().tobytes() == py[i].cpu().numpy().tobytes() == again[i].tobytes()
    if kind != 2:
        assert np.all(np.isnan(host[1])) and bool(torch.isnan(dev[1]).all())          # m1 is kind 2's alone


# ---------------------------------------------------------------------------------------------- 5. the convention, end to end
L0, LW_MASK = 6, 4


def _unit_modes(lmax):
    """(variance, alm) of the real degrees of freedom of a_{L0 m}: a field of unit power at L0 is their independent sum"""
    out = []
    for m in range(L0 + 1):
        for v in ([1.0] if m == 0 else [1.0, 1.0j]):
            a = np.zeros(O.alm_size(lmax, lmax), dtype=np.complex128)
            a[O.alm_index(lmax, L0, m)] = v
            out.append((1.0 if m == 0 else 0.5, a))
    return out


@functools.lru_cache(maxsize=None)
def _convention(spin):
    """nside, lmax, the mask map, the exact columns L0 of the matrices, the unit-mode maps, and the pseudo-C_l that the numpy transforms
    of tests/sht_oracle.py / tests/sht_spin_oracle.py give for them (summed over the modes)"""
    nside, lmax = (16, 16) if spin == 0 else (32, 12)
    rng = np.random.default_rng(11)
    am = (rng.standard_normal(O.alm_size(LW_MASK, LW_MASK)) + 1j * rng.standard_normal(O.alm_size(LW_MASK, LW_MASK))) * 0.3
    am[:LW_MASK + 1] = am[:LW_MASK + 1].real
    am[0] = 3.0 * np.sqrt(4 * np.pi)
    mask = O.alm2map(am, nside, LW_MASK, LW_MASK)
    wl = O.alm2cl(am, None, LW_MASK, LW_MASK)
    exact = P.exact_matrices(wl, lmax)
    maps, ref = [], 0.0
    for var, a in _unit_modes(lmax):
        if spin == 0:
            m = O.alm2map(a, nside, lmax, lmax)
            pcl = O.alm2cl(O.map2alm(m * mask, nside, lmax, lmax, iter=3), None, lmax, lmax)[None]
        else:
            m = OS.alm2map_spin(np.stack([a, 0 * a]), nside, 2, lmax, lmax)
            eb = OS.map2alm_spin(m * mask, nside, 2, lmax, lmax)
            pcl = np.stack([O.alm2cl(eb[0], None, lmax, lmax), O.alm2cl(eb[1], None, lmax, lmax)])
        maps.append((var, m))
        ref = ref + var * pcl
    cols = [exact['00'][0][:, L0]] if spin == 0 else [exact['++'][0][:, L0], exact['--'][0][:, L0]]
    return nside, lmax, mask, cols, maps, ref


@pytest.mark.parametrize('spin', [0, 2])
def test_convention_end_to_end(gpu, spin):
    nside, lmax, mask, cols, maps, ref = _convention(spin)
    got = 0.0
    for var, m in maps:
        pcl = U.pseudo_cl(m if spin == 0 else (m[0], m[1]), mask1=mask, lmax=lmax)
        got = got + var * (pcl if spin == 0 else pcl[[0, 3]])                          # [00], or EE and BB of [EE, EB, BE, BB]
    for i, col in enumerate(cols):
        oracle_err = np.abs(ref[i] - col).max()
        tol = 4 * oracle_err + 1e-12 * np.abs(col).max()
        err = np.abs(got[i] - col).max()
        print("spin %d spectrum %d: column scale %.3e, numpy-transform error %.3e, GPU error %.3e (tol %.3e)"
              % (spin, i, np.abs(col).max(), oracle_err, err, tol))
        assert err <= tol
    if spin == 2:
        # the tolerance tells a swapped M++ / M-- from a correct one
        assert np.abs(cols[0] - cols[1]).max() > 100 * (4 * np.abs(ref[0] - cols[0]).max())


# ---------------------------------------------------------------------------------------------- 6. the workspace
NSIDE_W, LMAX_W = 8, 23


@functools.lru_cache(maxsize=None)
def _ws_case(spins):
    rng = np.random.default_rng(5)
    npix = 12 * NSIDE_W ** 2
    mask = 0.5 + 0.5 * rng.random(npix)
    mask[: npix // 5] = 0.0
    bins = U.ClBins.linear(2, LMAX_W, 4)
    ws = U.PseudoClWorkspace(mask, spin1=spins[0], spin2=spins[1], bins=bins, lmax=LMAX_W)
    wl = ws.wl
    kind = {(0, 0): 0, (0, 2): 1, (2, 2): 2}[spins]
    mats = {}
    got = _matrices(wl, LMAX_W, kind)
    for key, m in zip(KEYS[kind], got):
        mats[key] = (m, None)
    ref = P.workspace(mats, spins, bins.edges, LMAX_W)
    return mask, bins, ws, ref


def _close(a, b, tol, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    e = np.abs(a - b).max() / np.abs(b).max()
    print("%s: %.3e" % (what, e))
    assert e <= tol, what


@pytest.mark.parametrize('spins', [(0, 0), (0, 2), (2, 2)])
def test_workspace_against_numpy(gpu, spins):
    mask, bins, ws, ref = _ws_case(spins)
    ns, n, nb = ws.ns, LMAX_W + 1, bins.nbins
    assert ns == {(0, 0): 1, (0, 2): 2, (2, 2): 4}[spins] and nb == 5
    assert ws.fsky == pytest.approx(np.mean(mask * mask), rel=1e-14)
    assert np.array_equal(ws.ell, ref['ell'])
    cm = ws.coupling_matrix()
    cm = cm if spins == (2, 2) else (cm,)
    for m, again in zip(cm, _matrices(ws.wl, LMAX_W, ws.kind)):
        assert m.tobytes() == again.tobytes()
    rng = np.random.default_rng(9)
    cl = rng.random((ns, n)) + 0.5
    if spins != (0, 0):
        cl[:, :2] = 0.0
    pcl = ws.couple(cl)
    _close(pcl, ref['couple'](cl), 1e-11, 'couple')
    _close(ws.decouple(pcl), ref['decouple'](pcl), 1e-11, 'decouple')
    _close(ws.bandpower_windows(), ref['windows'], 1e-11, 'windows')
    if spins == (0, 0):
        _close(ws.couple(cl[0]), ref['couple'](cl)[0], 1e-11, 'couple 1-D')
        assert ws.decouple(pcl[0]).shape == (nb,)


@pytest.mark.parametrize('spins', [(0, 0), (0, 2), (2, 2)])
def test_decouple_inverts_couple_on_binned_spectra(gpu, spins):
    mask, bins, ws, ref = _ws_case(spins)
    cb = np.random.default_rng(3).random((ws.ns, bins.nbins)) + 0.5
    cl = bins.unbin_cell(cb, LMAX_W)                                  # constant within bins, zero outside them
    back = ws.decouple(ws.couple(cl))
    e = np.abs(back - cb).max()
    print("decouple(couple(cl)) - cl: %.3e" % e)
    assert e <= 1e-10
    assert np.abs(bins.unbin_cell(back, LMAX_W) - cl).max() <= 1e-10


def test_unit_mask_gives_binned_anafast(gpu):
    """mask = 1 has W_l = 4 pi delta_l0, M = 1 and so bandpowers = binned anafast, up to the quadrature error of the mask's own anafast.
    That error falls as the band limit moves below the pixel scale (numpy transforms of tests/sht_oracle.py, 3 iterations: W_0 / 4 pi - 1
    = -6.9e-5 at nside 8 with l <= 23, the shape of the tests above, -5.9e-11 at nside 32 with l <= 16, -2.3e-13 at nside 64 with
    l <= 16), so the 1e-12 of this check is asked at nside 64, lmax 8, whose mask spectrum runs to l = 16."""
    nside, lmax = 64, 8
    npix = 12 * nside ** 2
    m = np.random.default_rng(21).standard_normal(npix)
    bins = U.ClBins.linear(2, lmax, 2)
    out = U.decoupled_cl(m, mask1=np.ones(npix), bins=bins, lmax=lmax)
    ref = bins.bin_cell(U.anafast(m, lmax=lmax))
    assert sorted(out) == ['cl', 'ell', 'fsky', 'pcl'] and out['fsky'] == pytest.approx(1.0, abs=1e-15)
    assert out['cl'].shape == (1, bins.nbins) and out['pcl'].shape == (1, lmax + 1) and np.array_equal(out['ell'], bins.ell)
    assert bins.nbins == 3
    e = np.abs(out['cl'][0] - ref).max() / np.abs(ref).max()
    print("unit mask: %.3e" % e)
    assert e <= 1e-12


def test_cuda_inputs_give_cuda_outputs_with_the_same_bytes(gpu):
    import torch
    mask, bins, ws, ref = _ws_case((2, 2))
    rng = np.random.default_rng(4)
    npix = 12 * NSIDE_W ** 2
    q, u = rng.standard_normal(npix), rng.standard_normal(npix)
    host = U.decoupled_cl((q, u), mask1=mask, workspace=ws)
    dev = U.decoupled_cl((torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda()), mask1=torch.from_numpy(mask).cuda(), workspace=ws)
    for k in ('ell', 'cl', 'pcl'):
        assert isinstance(host[k], np.ndarray) and dev[k].is_cuda
        assert host[k].tobytes() == dev[k].cpu().numpy().tobytes(), k
    assert host['cl'].shape == (4, bins.nbins) and host['fsky'] == dev['fsky']
    ws_dev = U.PseudoClWorkspace(torch.from_numpy(mask).cuda(), spin1=2, spin2=2, bins=bins, lmax=LMAX_W)
    for a, b in zip(ws.coupling_matrix(), ws_dev.coupling_matrix()):
        assert a.tobytes() == b.tobytes()
    cl = rng.random((4, LMAX_W + 1))
    pd = ws_dev.couple(torch.from_numpy(cl).cuda())
    assert pd.is_cuda and pd.cpu().numpy().tobytes() == ws.couple(cl).tobytes()
    assert ws_dev.decouple(pd).is_cuda
    # a workspace made for other spins is refused
    with pytest.raises(ValueError, match="workspace"):
        U.decoupled_cl(q, mask1=mask, workspace=ws)
