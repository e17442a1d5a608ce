"""Band b of a shell plan holds the rings [1 + b R, 1 + (b + 1) R) (R rings per band: ShellPlan.tile_shape): a contiguous RING pixel range,
the unit of multi-GPU pixel ownership.  plan.bands() and plan.band_apron(b0, b1) against the RING formula written out here, for every band
range of three small shells and three band reaches -- aprons that run past either pole included, which end at pixel 0 and at npix -- and the
band ranges the plan refuses.  Only plans are created: no catalog, no map."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REACH_MAX = 16           # the largest band reach a plan accepts (csrc/bfgx_regrid2.hpp kReachMax)


def _ring_first(nside, ring):
    """first pixel of ring `ring` in RING order (Gorski et al. 2005): 0 before ring 1, npix beyond ring 4 nside - 1"""
    if ring < 1:
        return 0
    if ring >= 4 * nside:
        return 12 * nside * nside
    if ring < nside:
        return 2 * ring * (ring - 1)
    if ring < 3 * nside:
        return 2 * nside * (nside - 1) + (ring - nside) * 4 * nside
    q = 4 * nside - ring
    return 12 * nside * nside - 2 * q * (q + 1)


def _tiny_plan(nside):
    import torch
    from baryonification_amd import engine, synthetic as syn
    z, M, r = np.geomspace(0.1, 0.2, 3), np.geomspace(1e13, 1e14, 3), np.geomspace(1e-2, 10, 8)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], np.zeros((3, 3, 8)), syn.COSMO, 10.0)
    return engine.ShellPlan(model, keep, nside, 16, 0, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('nside', [1, 8, 64])        # 1: the smallest shell a plan accepts (one band that holds both poles)
def test_bands_and_aprons_follow_the_ring_formula(gpu, nside):
    plan = _tiny_plan(nside)
    try:
        npix = 12 * nside * nside
        R, _ = plan.tile_shape()
        nbands = (4 * nside - 1 + R - 1) // R
        first = plan.bands()
        assert first.dtype == np.int64 and first.size == nbands + 1
        assert first.tolist() == [_ring_first(nside, 1 + R * b) for b in range(nbands + 1)]
        assert first[0] == 0 and first[-1] == npix and np.all(np.diff(first) > 0)
        past_north = past_south = 0
        for reach in (1, 2, REACH_MAX):
            plan.set_band_reach(reach)
            for b0 in range(nbands + 1):
                for b1 in range(b0, nbands + 1):
                    want = (_ring_first(nside, 1 + R * b0 - reach), _ring_first(nside, 1 + R * b1 + reach))
                    assert plan.band_apron(b0, b1) == want, (reach, b0, b1)
                    past_north += want[0] == 0 and 1 + R * b0 - reach < 1
                    past_south += want[1] == npix and 1 + R * b1 + reach > 4 * nside - 1
        assert past_north > 0 and past_south > 0          # (aprons past either pole were among them)
        for reach in (0, REACH_MAX + 1):
            with pytest.raises(ValueError, match='band reach must be'):
                plan.set_band_reach(reach)
    finally:
        plan.close()


@pytest.mark.parametrize('nside', [1, 8, 64])
def test_band_ranges_out_of_bounds_are_refused(gpu, nside):
    """band0 > band1, band0 < 0 and band1 > nbands: BFGX_ERR_INVALID (a ValueError) from the apron query and from the entries that take a band
    range, before anything is launched"""
    from baryonification_amd import _lib
    import ctypes as C
    plan = _tiny_plan(nside)
    try:
        nbands = plan.bands().size - 1
        L = _lib.load()
        lo, hi = C.c_int64(0), C.c_int64(0)
        out = C.c_void_p(8)                               # non-NULL, never read: the range is refused first
        for b0, b1 in ((1, 0), (nbands, nbands - 1), (-1, 0), (-1, nbands), (0, nbands + 1), (nbands, nbands + 1)):
            assert L.bfgx_plan_band_apron(plan._h, b0, b1, C.byref(lo), C.byref(hi)) == _lib.ERR_INVALID, (b0, b1)
            assert L.bfgx_last_error().decode() == 'band range out of bounds'
            with pytest.raises(ValueError, match='band range out of bounds'):
                plan.band_apron(b0, b1)
            assert L.bfgx_bands_max_offset2_device(plan._h, b0, b1, out) == _lib.ERR_INVALID, (b0, b1)
            assert L.bfgx_last_error().decode() == 'band range out of bounds'
        assert plan.band_apron(0, nbands) == (0, 12 * nside * nside)
    finally:
        plan.close()
