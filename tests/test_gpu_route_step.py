"""The halo routing of a spatially sharded multi-GPU step and K0's read of the routed blocks, rank by rank on one GPU:
bfgx_disc_rings_device (+ the route margin), bfgx_route_count / _fill / _pack_device, bfgx_route_step_device and
bfgx_plan_set_catalog_blocks against tests/route_oracle.py.  The "ranks" are played one after the other; the collective between them
is a tensor copy: the block source s packed at position (d < s ? d : d - 1) lands in destination d's receive buffer at position
(s < d ? s : s - 1).  Every buffer a kernel writes is a slice of a larger tensor with sentinel words either side, checked afterwards.

Every comparison is exact (integers, sets of halo numbers, whole rows bit for bit) except the three taken from tests/test_gpu_fullsize.py:
2e-6 max|full| for fp32 pix_offsets and 1e-12 max|full| for the fp64 paint (test_band_restricted_pass_with_selected_halos_equals_full_pass),
1e-6 mean(map) for the assembled fp32 map (test_config4_full_size_eight_rank_decomposition_on_one_gpu)."""
import time

import numpy as np
import pytest

import route_oracle as RO

pytestmark = pytest.mark.gpu

EPS = 10.0
BAND_RINGS = 2         # include/bfgx.h: the ring range is the disc's colatitude band widened by 2 rings ...
W_RINGS = 3            # ... and exceeds the rings of the touched pixels by at most 3
GUARD = 64             # sentinel words either side of every buffer a kernel writes
NCOLS = 6


class Ctx:
    pass


@pytest.fixture(scope='module')
def ctx(gpu):
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    from oracle import oracle as O
    c = Ctx()
    c.torch, c.lib, c.engine, c.syn = torch, _lib, engine, syn
    c.dev = torch.device('cuda', 0)
    c.bg = O.Background.from_dict(syn.COSMO)
    c.kcat = syn.make_catalog(20_000)                               # the catalog of the K0 tests; its table serves every plan here
    z, M, r = syn.table_grid(c.kcat, pad=1e-9)
    c.axes = [np.log(1 + z), np.log(M), np.log(r)]
    c.tables = (syn.displacement_table(z, M, r), np.log(syn.paint_table(z, M, r)))
    c.plans, c.truth, c.rings = {}, {}, {}
    yield c
    for p in c.plans.values():
        p.close()


def _plan(c, nside, max_halos=1024, paint=False):
    key = (nside, paint)
    if key not in c.plans:
        model, keep = c.engine.model_from_tables(c.axes, c.tables[1 if paint else 0], c.syn.COSMO, EPS, EPS, log_values=paint)
        c.plans[key] = c.engine.ShellPlan(model, keep, nside, max_halos, 0, c.torch.cuda.current_stream().cuda_stream)
    assert c.plans[key].max_halos >= max_halos
    return c.plans[key]


class Guarded:
    """n elements inside a larger tensor, GUARD sentinel words either side"""
    SENT = {'float64': -7.25e300, 'float32': -7.25e30, 'int32': 0x5A5A5A5A, 'int64': 0x5A5A5A5A5A5A5A5A}

    def __init__(self, c, n, dtype, fill=None):
        self.s = self.SENT[str(dtype).split('.')[-1]]
        self.n = int(n)
        self.whole = c.torch.full((self.n + 2 * GUARD,), self.s, dtype=dtype, device=c.dev)
        self.t = self.whole[GUARD:GUARD + self.n]
        if fill is not None:
            self.t.fill_(fill)

    def ptr(self):
        return self.whole.data_ptr() + GUARD * self.whole.element_size()

    def intact(self):
        return bool((self.whole[:GUARD] == self.s).all().item()) and bool((self.whole[GUARD + self.n:] == self.s).all().item())


def _upload(c, cat, keys=('M', 'z', 'ra', 'dec')):
    cols = {k: c.torch.from_numpy(np.ascontiguousarray(cat[k], dtype=np.float64)).to(c.dev) for k in keys}
    cd = c.lib.make_catalog_dev(cols['M'].numel(), cols['M'].data_ptr(), cols['z'].data_ptr(), cols['ra'].data_ptr(), cols['dec'].data_ptr(),
                                ln1pz_ptr=cols['lnz'].data_ptr() if 'lnz' in cols else 0, lnM_ptr=cols['lnM'].data_ptr() if 'lnM' in cols else 0)
    return cd, cols


def _route_catalog(c, nside):
    """hand-placed rows + random halos with discs from far below a pixel to a few pixels; NSIDE 64: the 20 000 of the route_step tests"""
    nrand = 20_000 if nside == 64 else 3000
    return RO.catalog_with_hand_rows(c.syn.make_catalog(nrand, seed=100 + nside, z_lo=0.02, z_hi=0.3))


def _truth(c, nside):
    """the reference's ring ranges: computed once per NSIDE, shared, never modified"""
    if nside not in c.truth:
        cat, is_random = _route_catalog(c, nside)
        T = RO.true_ring_ranges(nside, cat, EPS, c.bg)
        for v in T.values():
            v.setflags(write=False)
        c.truth[nside] = (cat, is_random, T)
    return c.truth[nside]


def _margins(plan, nside):
    return sorted({0, 1, plan.tile_shape()[0], 4 * nside})


def _gpu_rings(c, nside):
    """disc_rings of the route catalog at every margin of _margins: {margin: int64 [n][2]}, computed once per NSIDE"""
    if nside not in c.rings:
        cat, _, _ = _truth(c, nside)
        plan = _plan(c, nside)
        cd, cols = _upload(c, cat)
        n = cat['M'].size
        out = {}
        try:
            for m in _margins(plan, nside):
                buf = Guarded(c, 2 * n, c.torch.int32)
                plan.set_route_margin(m)
                plan.disc_rings(cd, buf.ptr())
                c.torch.cuda.synchronize()
                assert buf.intact()
                out[m] = buf.t.cpu().numpy().astype(np.int64).reshape(n, 2)
                out[m].setflags(write=False)
        finally:
            plan.set_route_margin(0)
        c.rings[nside] = out
    return c.rings[nside]


# ------------------------------------------------------------------------------------------------------------------ 1. ring ranges

@pytest.mark.parametrize('nside', [1, 2, 16, 64])
def test_disc_rings_cover_every_touched_ring_and_margins_widen_exactly(ctx, nside):
    """Coverage: [first, last] holds every ring the halo can touch (the disc's pixels, the four fallback pixels of a disc with < 4 pixels) --
    would fail for a range narrowed by one ring, a pole disc not clipped to ring 1 / 4 nside - 1, a fallback beyond the last ring left out.
    Invalid rows (M NaN / 0 / < 0 / inf, z <= -1, |dec| > 90, dec NaN) give exactly (1, 0) at every margin -- would fail if the margin
    were applied to an empty range.  A margin m gives the margin-0 range widened by m and clipped, to the integer -- would fail for a
    margin applied twice, on one side only, or before the clip.  Margins outside 0 .. 4 nside are refused."""
    cat, is_random, T = _truth(ctx, nside)
    R = _gpu_rings(ctx, nside)
    v = T['valid']
    nv, ni = len(RO.HAND_VALID), len(RO.HAND_INVALID)
    assert v[:nv].all() and not v[nv:nv + ni].any() and v[is_random].all()
    assert (T['radius'][5:8] >= np.pi).all() and (T['npix_disc'][v] == 0).any() and (T['npix_disc'][v] >= 4).any()
    nl = 4 * nside - 1
    for m, r in R.items():
        first, last = r[:, 0], r[:, 1]
        assert np.array_equal(r[~v], np.tile(RO.EMPTY, ((~v).sum(), 1)))
        assert (first[v] >= 1).all() and (last[v] <= nl).all() and (first[v] <= last[v]).all()
        tf, tl = RO.widen(T['tfirst'], T['tlast'], m, nside)
        assert (first[v] <= tf[v]).all() and (last[v] >= tl[v]).all()
        w0, w1 = RO.widen(R[0][:, 0], R[0][:, 1], m, nside)
        assert np.array_equal(first, w0) and np.array_equal(last, w1)
    assert np.array_equal(R[4 * nside][v], np.tile((1, nl), (v.sum(), 1)))
    plan = _plan(ctx, nside)
    for bad in (-1, 4 * nside + 1):
        with pytest.raises(ValueError):
            plan.set_route_margin(bad)
    buf = Guarded(ctx, 2 * v.size, ctx.torch.int32)                           # (a refused margin changed nothing)
    cd, cols = _upload(ctx, cat)
    plan.disc_rings(cd, buf.ptr())
    assert np.array_equal(buf.t.cpu().numpy().reshape(-1, 2), R[0]) and buf.intact()


def _colatitude_band(nside, T):
    """rings whose colatitude lies in [theta - radius, theta + radius] (first > last: none), from the reference's ring colatitudes"""
    th = RO.ring_colatitudes(nside)
    lo, hi = np.searchsorted(th, T['theta'] - T['radius'], side='left') + 1, np.searchsorted(th, T['theta'] + T['radius'], side='right')
    return lo, hi


@pytest.mark.parametrize('nside', [1, 2, 16, 64])
def test_disc_rings_are_the_colatitude_band_widened_by_two_rings(ctx, nside):
    """What the widening IS: disc_rings_kernel takes ring_above(cos(theta - radius)) - 1 and ring_above(cos(theta + radius)) + 2, i.e. 2
    rings beyond the first and the last ring whose colatitude lies within the disc's colatitude band (query_disc's irmin, irmax), as
    include/bfgx.h states.  With a non-empty band the range is exactly that, clipped; with an empty band (a disc between two rings) it is
    the 4 rings around the gap.  Exact on every valid row but those whose disc edge lies within 1e-9 rad of a ring's colatitude (selected
    by the reference alone, at most 0.1 % of the rows).  Would fail for a widening of 1 or 3 (the kernel used to add a third ring), for
    first / last in swapped roles at the poles, for a margin folded into the base widening."""
    cat, is_random, T = _truth(ctx, nside)
    R = _gpu_rings(ctx, nside)
    v = T['valid'] & (T['radius'] < np.pi)
    near = RO.edge_on_a_ring(nside, T['radius'], T['theta'])
    assert (near & v).sum() <= 1e-3 * v.sum()
    v &= ~near
    lo, hi = _colatitude_band(nside, T)               # an empty band has lo = hi + 1: the rings hi and lo around the disc
    nl = 4 * nside - 1
    for m in (0, 1):
        want_first, want_last = np.maximum(1, lo - BAND_RINGS - m), np.minimum(nl, hi + BAND_RINGS + m)
        assert np.array_equal(R[m][v, 0], want_first[v]) and np.array_equal(R[m][v, 1], want_last[v])


@pytest.mark.parametrize('nside', [1, 2, 16, 64])
def test_disc_rings_exceed_the_touched_rings_by_at_most_the_stated_widening(ctx, nside):
    """Tightness on the random rows: [first, last] exceeds the rings of the disc's pixels (of the four interpolation pixels when the disc is
    empty) by at most W + margin = 3 + margin rings either side: the 2 rings beyond the colatitude band, and one more where the first or
    last ring of the band holds no pixel centre inside the disc (its chord there is shorter than the pixel spacing).  Would fail for a
    margin applied twice or a band widened by 3 -- which the kernel did: 27 of 3000 rows at NSIDE 16 and 1800 of 20 000 at NSIDE 64 then
    exceeded the touched rings by 4."""
    cat, is_random, T = _truth(ctx, nside)
    R = _gpu_rings(ctx, nside)
    for m in (0, 1, _plan(ctx, nside).tile_shape()[0]):
        ex_first, ex_last = T['first'][is_random] - R[m][is_random, 0], R[m][is_random, 1] - T['last'][is_random]
        over = (ex_first > W_RINGS + m) | (ex_last > W_RINGS + m)
        print("NSIDE %d margin %d: %d of %d random rows exceed the touched rings by more than %d; largest excess %d / %d"
              % (nside, m, over.sum(), over.size, W_RINGS + m, ex_first.max(), ex_last.max()))
        assert not over.any()


# ------------------------------------------------------------------------------------------------------------------ 2. count, fill, pack

ROUTE_NSIDE = 64


def _edge_bounds(world):
    """ring bounds over the rings 1 .. 255 with empty ranks leading, in the middle and trailing (where the world has room for them)"""
    top = 4 * ROUTE_NSIDE
    if world == 1:
        return np.array([1, top])
    if world == 2:
        return np.array([1, 100, top])
    if world == 7:
        return np.array([1, 1, 40, 40, 90, 200, top, top])
    b = np.sort(np.random.default_rng(world).integers(1, top + 1, world + 1))
    b[:3], b[-3:] = 1, top
    b[20:23] = b[20]
    return b


def _edge_ranges(n, bounds, seed):
    """n ring ranges: random ones behind prescribed ones -- touching nothing, touching every rank, starting / ending on a bound"""
    top = 4 * ROUTE_NSIDE - 1
    rng = np.random.default_rng(seed)
    first = rng.integers(1, top + 1, n)
    last = np.minimum(first + rng.integers(0, 40, n), top)
    on_bounds = []
    for b in np.unique(bounds):
        on_bounds += [(b, b), (b - 1, b - 1), (b - 1, b), (b, b + 5), (b - 5, b - 1), (b - 5, b), (1, b), (b, top), (1, b - 1)]
    fixed = [(1, top), (100, 99), (1, 0), (top, 1)] + [(max(1, f), min(top, l)) for f, l in on_bounds if l >= 1 and f <= top]
    k = min(n, len(fixed))
    if n > 1:
        first[:k], last[:k] = np.array(fixed[:k]).T
    return first.astype(np.int64), last.astype(np.int64)


def _ids_of(block0):
    """(count, halo numbers) of a block's column 0: the rows in front of the first NaN; everything behind them must be NaN"""
    valid = ~np.isnan(block0)
    m = int(valid.sum())
    assert valid[:m].all()
    return m, block0[:m].astype(np.int64)


def _check_blocks(blocks, host, want, cap, over, prefill=None):
    """blocks [nblk][ncols][cap] (host) against the expected halo numbers per block: each once, whole rows, NaN behind them in column 0,
    nothing written behind them in the other columns; an overflowing block holds `cap` distinct expected halos"""
    for b, w in zip(blocks, want):
        m, ids = _ids_of(b[0])
        assert m == min(w.size, cap) and np.unique(ids).size == m
        if w.size <= cap:
            assert np.array_equal(np.sort(ids), w)
        else:
            assert over and np.isin(ids, w).all()
        assert np.array_equal(b[:, :m].T, host[ids])
        if prefill is not None:
            assert (b[1:, m:] == prefill).all()


@pytest.mark.parametrize('n', [0, 1, 255, 257, 512 * 256 + 1])
@pytest.mark.parametrize('world', [1, 2, 7, 64])
def test_route_count_fill_pack_at_the_edges(ctx, world, n):
    """Prescribed ring ranges against the rule of include/bfgx.h (halo -> rank j iff first <= last, bounds[j] <= last, bounds[j + 1] > first):
    counts, the packed halo numbers per destination (each once, whole rows), fixed-capacity blocks at a capacity that just fits (flag 0)
    and one short (flag 1, the full blocks hold `blockcap` distinct expected halos, the others are complete), NaN behind the packed rows.
    n = 512 * 256 + 1 is the first size at which a workgroup owns more than 256 halos.  Would fail for `<` instead of `<=` on a bound,
    an empty rank not skipped, the last halo of a workgroup's run dropped, rows of different halos mixed, an overflow that writes past
    the block."""
    torch, dev = ctx.torch, ctx.dev
    plan = _plan(ctx, ROUTE_NSIDE)
    bounds = _edge_bounds(world)
    assert bounds.size == world + 1 and (np.diff(bounds) >= 0).all() and (world < 7 or ((np.diff(bounds) == 0).sum() >= 3))
    first, last = _edge_ranges(n, bounds, seed=1000 * world + n % 997)
    want = RO.expected_blocks(first, last, bounds)
    rng = np.random.default_rng(n + world)
    host = rng.normal(size=(n, NCOLS))
    host[:, 0] = np.arange(n)
    cols = [torch.from_numpy(np.ascontiguousarray(host[:, k])).to(dev) for k in range(NCOLS)]
    cptr = [x.data_ptr() for x in cols]
    rings = torch.from_numpy(np.stack([first, last], axis=1).astype(np.int32).reshape(-1)).to(dev)
    counts, cursor = Guarded(ctx, world, torch.int32), Guarded(ctx, world, torch.int32)
    plan.route_count(n, rings.data_ptr(), bounds, counts.ptr())
    cnt = counts.t.cpu().numpy().astype(np.int64)
    assert np.array_equal(cnt, [w.size for w in want]) and counts.intact()
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rows = Guarded(ctx, int(cnt.sum()) * NCOLS, torch.float64, fill=float('nan'))
    plan.route_fill(n, rings.data_ptr(), bounds, start, cptr, cursor.ptr(), rows.ptr())
    got = rows.t.cpu().numpy().reshape(-1, NCOLS)
    assert rows.intact() and cursor.intact() and not np.isnan(got).any()
    for j in range(world):
        blk = got[start[j]:start[j] + cnt[j]]
        ids = blk[:, 0].astype(np.int64)
        assert np.array_equal(np.sort(ids), want[j]) and np.array_equal(blk, host[ids])
    cmax = int(cnt.max())
    for cap, over in ((max(cmax, 1), 0), (cmax - 1, 1)):
        if cap < 1:
            continue
        blocks = Guarded(ctx, world * NCOLS * cap, torch.float64, fill=-7.0)
        ovf = Guarded(ctx, 1, torch.int32, fill=0)
        plan.route_pack(n, rings.data_ptr(), bounds, cap, cptr, cursor.ptr(), blocks.ptr(), ovf.ptr())
        b = blocks.t.cpu().numpy().reshape(world, NCOLS, cap)
        assert int(ovf.t.item()) == over and blocks.intact() and ovf.intact() and cursor.intact()
        _check_blocks(b, host, want, cap, over, prefill=-7.0)


def test_route_entries_refuse_what_they_cannot_pack(ctx):
    """world 0 and 65, 0 and 9 columns, descending bounds, a block capacity of 0: BFGX_ERR_INVALID, nothing written"""
    torch, dev = ctx.torch, ctx.dev
    plan = _plan(ctx, ROUTE_NSIDE)
    n = 10
    rings = torch.ones(2 * n, dtype=torch.int32, device=dev)
    col = torch.zeros(n, dtype=torch.float64, device=dev)
    out, cnt, ovf = Guarded(ctx, 9 * 70 * n, torch.float64), Guarded(ctx, 70, torch.int32), Guarded(ctx, 1, torch.int32)
    cd = ctx.lib.make_catalog_dev(n, col.data_ptr(), col.data_ptr(), col.data_ptr(), col.data_ptr())
    ok_b, one = np.array([1, 100, 256]), [col.data_ptr()]
    for bounds in (np.array([1]), np.arange(1, 67), np.array([1, 100, 99])):             # world 0, world 65, descending
        with pytest.raises(ValueError):
            plan.route_count(n, rings.data_ptr(), bounds, cnt.ptr())
    for bounds, cptr, cap in ((np.array([1]), one, 4), (np.arange(1, 67), one, 4), (np.array([1, 100, 99]), one, 4), (ok_b, [], 4), (ok_b, one * 9, 4),
                              (ok_b, one, 0)):
        if cap:
            with pytest.raises(ValueError):
                plan.route_fill(n, rings.data_ptr(), bounds, np.zeros(max(bounds.size - 1, 1)), cptr, cnt.ptr(), out.ptr())
        with pytest.raises(ValueError):
            plan.route_pack(n, rings.data_ptr(), bounds, cap, cptr, cnt.ptr(), out.ptr(), ovf.ptr())
        with pytest.raises(ValueError):
            plan.route_step(cd, 0, bounds, cap, cptr, cnt.ptr(), out.ptr(), out.ptr(), ovf.ptr())
    for rank in (-1, 2):
        with pytest.raises(ValueError):
            plan.route_step(cd, rank, ok_b, 4, one, cnt.ptr(), out.ptr(), out.ptr(), ovf.ptr())
    ctx.torch.cuda.synchronize()
    for g in (out, cnt, ovf):
        assert g.intact() and bool((g.t == g.s).all().item())


# ------------------------------------------------------------------------------------------------------------------ 3. route_step

def _band_bounds(plan, nside, world):
    from baryonification_amd.utils.Parallelize import band_partition, band_ring_bounds
    first = plan.bands()
    cuts = band_partition(first, world)
    rb = band_ring_bounds(cuts, plan.tile_shape()[0], nside)
    assert rb[0] == 1 and rb[-1] == 4 * nside
    return first, cuts, rb


def _route_step(c, plan, cd, rank, rb, cap, cptr, prefill=-7.0):
    """one route_step call into guarded, prefilled buffers -> (send [world - 1][k][cap], recv [world][k][cap], overflow) on the host"""
    torch, world, k = c.torch, len(rb) - 1, len(cptr)
    send = Guarded(c, (world - 1) * k * cap, torch.float64, fill=prefill)
    recv = Guarded(c, world * k * cap, torch.float64, fill=prefill)
    cursor, ovf = Guarded(c, world, torch.int32), Guarded(c, 1, torch.int32, fill=0)
    plan.route_step(cd, rank, rb, cap, cptr, cursor.ptr(), send.ptr() if world > 1 else 0, recv.ptr(), ovf.ptr())
    torch.cuda.synchronize()
    assert send.intact() and recv.intact() and cursor.intact() and ovf.intact()
    return send, recv, int(ovf.t.item())


@pytest.mark.parametrize('world', [1, 2, 3, 8, 64])
def test_route_step_packs_what_the_rule_and_the_two_call_form_give(ctx, world):
    """route_step for rank 0, a middle rank, the last rank (world 64: also a rank without rings) at a margin of 0 and of one band: the send
    block at position (d < rank ? d : d - 1) holds exactly the halos the rule sends to d from disc_rings' ranges at that margin -- and at
    least those whose touched rings (reference) +- margin reach d's rings --, this rank's own rows sit in the LAST receive block, every
    other receive block has column 0 all NaN, nothing else is written; the sets equal route_pack's on disc_rings' output.  One ring short
    of capacity the flag is raised, the full blocks hold blockcap distinct expected halos.  World 1 takes a NULL send buffer.  Would fail
    for position d instead of d - 1 above the own rank, the margin ignored in the fused pass, the own rows sent, recv column 0 not
    blanked, a ring range that differs between the one-call and the two-call form."""
    torch, dev, nside = ctx.torch, ctx.dev, ROUTE_NSIDE
    plan = _plan(ctx, nside)
    cat, is_random, T = _truth(ctx, nside)
    R = _gpu_rings(ctx, nside)
    n = cat['M'].size
    first_pix, cuts, rb = _band_bounds(plan, nside, world)
    cd, keep = _upload(ctx, cat)
    rng = np.random.default_rng(world)
    host = np.stack([np.arange(n, dtype=np.float64), cat['z'], cat['ra'], cat['dec'], rng.normal(size=n), rng.normal(size=n)], axis=1)
    cols = [torch.from_numpy(np.ascontiguousarray(host[:, k])).to(dev) for k in range(NCOLS)]
    cptr = [x.data_ptr() for x in cols]
    ranks = sorted({0, world // 2, world - 1})
    if world == 64:
        empty = [r for r in range(1, world - 1) if rb[r] == rb[r + 1]]
        assert empty
        ranks.append(empty[len(empty) // 2])
    try:
        for m in (0, plan.tile_shape()[0]):
            want = RO.expected_blocks(R[m][:, 0], R[m][:, 1], rb)
            tf, tl = RO.widen(T['tfirst'], T['tlast'], m, nside)
            for need, w in zip(RO.expected_blocks(tf, tl, rb), want):
                assert np.isin(need, w).all()                                       # (no halo that really reaches a rank is lost)
            assert sum(w.size for w in want) >= T['valid'].sum() and (world == 1 or max(w.size for w in want) < n)
            cap = max(w.size for w in want)
            plan.set_route_margin(m)
            # the two-call form on the same inputs
            rings = Guarded(ctx, 2 * n, torch.int32)
            plan.disc_rings(cd, rings.ptr())
            assert np.array_equal(rings.t.cpu().numpy().reshape(n, 2), R[m]) and rings.intact()
            blocks, cursor, ovf = Guarded(ctx, world * NCOLS * cap, torch.float64, fill=-7.0), Guarded(ctx, world, torch.int32), Guarded(ctx, 1, torch.int32, fill=0)
            plan.route_pack(n, rings.ptr(), rb, cap, cptr, cursor.ptr(), blocks.ptr(), ovf.ptr())
            pack = blocks.t.cpu().numpy().reshape(world, NCOLS, cap)
            assert int(ovf.t.item()) == 0 and blocks.intact()
            pack_ids = [np.sort(_ids_of(b[0])[1]) for b in pack]
            for rank in ranks:
                send, recv, over = _route_step(ctx, plan, cd, rank, rb, cap, cptr)
                assert over == 0
                s = send.t.cpu().numpy().reshape(world - 1, NCOLS, cap)
                r = recv.t.cpu().numpy().reshape(world, NCOLS, cap)
                others = [d for d in range(world) if d != rank]
                assert [RO.block_position(d, rank) for d in others] == list(range(world - 1))
                _check_blocks(s, host, [want[d] for d in others], cap, 0, prefill=-7.0)
                _check_blocks(r[-1:], host, [want[rank]], cap, 0, prefill=-7.0)
                assert np.isnan(r[:-1, 0]).all() and (r[:-1, 1:] == -7.0).all()
                for d in range(world):
                    blk = r[-1] if d == rank else s[RO.block_position(d, rank)]
                    assert np.array_equal(np.sort(_ids_of(blk[0])[1]), pack_ids[d])
            # one row short of the fullest block
            rank = ranks[len(ranks) // 2]
            send, recv, over = _route_step(ctx, plan, cd, rank, rb, cap - 1, cptr)
            assert over == 1
            s = send.t.cpu().numpy().reshape(world - 1, NCOLS, cap - 1)
            r = recv.t.cpu().numpy().reshape(world, NCOLS, cap - 1)
            _check_blocks(s, host, [want[d] for d in range(world) if d != rank], cap - 1, 1, prefill=-7.0)
            _check_blocks(r[-1:], host, [want[rank]], cap - 1, 1, prefill=-7.0)
            assert np.isnan(r[:-1, 0]).all()
    finally:
        plan.set_route_margin(0)


def test_route_step_beyond_its_lds_stash(ctx):
    """route_step launches at most 2048 workgroups and a workgroup keeps the ring ranges of its first 4096 halos in LDS; with
    2048 * 4096 + 2048 halos every workgroup owns 4097 and computes the range of its last one a second time in the packing pass.  The
    halo numbers per block equal disc_rings + route_pack on the same columns (device-side sort), whole rows travel together.  Would fail
    for a stash index off by one, a recomputed range that differs from the first pass's (slots reserved for one destination, rows
    written to another), a 32-bit row offset."""
    torch, dev, nside = ctx.torch, ctx.dev, ROUTE_NSIDE
    plan = _plan(ctx, nside)
    t0 = time.perf_counter()
    n, world, k = 2048 * 4096 + 2048, 2, 3
    gen = torch.Generator(device=dev)
    gen.manual_seed(20250107)
    u = torch.rand((3, n), dtype=torch.float64, device=dev, generator=gen)
    M = torch.pow(10.0, 12.0 + 3.0 * u[0])
    z = 0.02 + 0.28 * u[1]
    dec = torch.rad2deg(torch.asin(2.0 * u[2] - 1.0))
    ident = torch.arange(n, dtype=torch.float64, device=dev)
    del u
    cd = ctx.lib.make_catalog_dev(n, M.data_ptr(), z.data_ptr(), z.data_ptr(), dec.data_ptr())       # (the routing reads M, z, dec)
    cptr = [ident.data_ptr(), z.data_ptr(), dec.data_ptr()]
    rb = np.array([1, 2 * nside, 4 * nside])
    send, recv = Guarded(ctx, (world - 1) * k * n, torch.float64, fill=-7.0), Guarded(ctx, world * k * n, torch.float64, fill=-7.0)
    cursor, ovf = Guarded(ctx, world, torch.int32), Guarded(ctx, 1, torch.int32, fill=0)
    plan.route_step(cd, 0, rb, n, cptr, cursor.ptr(), send.ptr(), recv.ptr(), ovf.ptr())
    rings = Guarded(ctx, 2 * n, torch.int32)
    plan.disc_rings(cd, rings.ptr())
    blocks, cursor2, ovf2 = Guarded(ctx, world * k * n, torch.float64, fill=-7.0), Guarded(ctx, world, torch.int32), Guarded(ctx, 1, torch.int32, fill=0)
    plan.route_pack(n, rings.ptr(), rb, n, cptr, cursor2.ptr(), blocks.ptr(), ovf2.ptr())
    torch.cuda.synchronize()
    for g in (send, recv, cursor, ovf, rings, blocks, cursor2, ovf2):
        assert g.intact()
    assert int(ovf.t.item()) == 0 and int(ovf2.t.item()) == 0
    s, r, b = send.t.view(1, k, n), recv.t.view(world, k, n), blocks.t.view(world, k, n)
    assert bool(torch.isnan(r[0, 0]).all().item())
    total = 0
    for d, blk in ((0, r[1]), (1, s[0])):
        m = int((~torch.isnan(blk[0])).sum().item())
        assert m == int((~torch.isnan(b[d, 0])).sum().item()) and not bool(torch.isnan(blk[0, :m]).any().item())
        ids = blk[0, :m].long()
        assert torch.equal(blk[1, :m], z[ids]) and torch.equal(blk[2, :m], dec[ids])
        assert torch.equal(torch.sort(blk[0, :m]).values, torch.sort(b[d, 0, :m]).values) and bool(torch.isnan(b[d, 0, m:]).all().item())
        assert bool((torch.sort(blk[0, :m]).values.diff() > 0).all().item())
        total += m
    assert n <= total < 1.2 * n
    print("stash case: %.1f s wall" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------------ 4. K0 over the routed blocks

K0_NSIDE = 128
K0_COLS = ('M', 'z', 'ra', 'dec', 'lnz', 'lnM')


def _k0_catalog(c):
    cat = {k: v.copy() for k, v in c.kcat.items()}
    cat['dec'][:8] = [89.95, -89.9, 89.999, -89.7, 60.0, -60.0, 0.01, -0.01]
    cat['M'][:4] *= 30.0                                                    # big discs on the pole caps
    cat['dec'][8:12] = [90.0, -90.0, 90.0, -90.0]                           # on the poles exactly: small discs and big ones
    cat['M'][10:12] = 3e15
    cat['lnz'], cat['lnM'] = c.lib.table_coords(cat['M'], cat['z'])
    assert np.unique(cat['ra']).size == cat['ra'].size                      # ra identifies a row's halo below
    return cat


def _routed_blocks(c, plan, cat, rb, margin):
    """every rank routes its share of the catalog (halo j starts on rank j % world) with route_step; the blocks are copied as the
    all_to_all would -> (recv tensors per rank [world][6][cap], cap, expected halo numbers per rank)"""
    torch, world, n = c.torch, len(rb) - 1, cat['M'].size
    plan.set_route_margin(margin)
    try:
        cd, cols = _upload(c, cat, K0_COLS)
        rings = Guarded(c, 2 * n, torch.int32)
        plan.disc_rings(cd, rings.ptr())
        rg = rings.t.cpu().numpy().astype(np.int64).reshape(n, 2)
        want = RO.expected_blocks(rg[:, 0], rg[:, 1], rb)
        share = [np.arange(s, n, world) for s in range(world)]
        cap = max(int(np.isin(sh, w).sum()) for sh in share for w in want) + 3
        sends, recvs = [], []
        for s in range(world):
            cds, colss = _upload(c, {k: cat[k][share[s]] for k in K0_COLS}, K0_COLS)
            send, recv, over = _route_step(c, plan, cds, s, rb, cap, [colss[k].data_ptr() for k in K0_COLS])
            assert over == 0
            sends.append(send.t.view(world - 1, NCOLS, cap))
            recvs.append((recv, recv.t.view(world, NCOLS, cap)))
        for d in range(world):
            for s in range(world):
                if s != d:
                    recvs[d][1][RO.block_position(s, d)].copy_(sends[s][RO.block_position(d, s)])
        return recvs, cap, want
    finally:
        plan.set_route_margin(0)


def _blocked_catalog(c, recv, world, cap):
    bp, B8 = recv.data_ptr(), cap * 8
    return c.lib.make_catalog_dev(world * cap, bp, bp + B8, bp + 2 * B8, bp + 3 * B8, ln1pz_ptr=bp + 4 * B8, lnM_ptr=bp + 5 * B8)


@pytest.mark.parametrize('world', [3, 8])
def test_k0_reads_the_routed_blocks_as_the_plain_catalog(ctx, world):
    """K0 on what route_step + the collective deliver (set_catalog_blocks(blockcap, 6 blockcap), the descriptor of the benchmark's
    spatial step), for every rank.  (a) Census: the per-row pair counts are 0 on the NaN rows and the halo's plain-catalog count on the
    others; the halos of a rank are exactly the rule's.  (b) offsets_bands (fp32) and paint_bands (fp64) over the rank's bands, output
    prefilled with NaN, equal the full-sphere pass on those pixels.  (d) After set_catalog_blocks(0, 0) the plan reads plain columns
    again.  Would fail for blk_stride dropped from K0's input index, a block received at position s instead of s - 1 above the own
    rank, ln(1+z) / ln M read by plain index, a row of one halo's M with another's position."""
    torch, dev, nside = ctx.torch, ctx.dev, K0_NSIDE
    cat = _k0_catalog(ctx)
    n = cat['M'].size
    plan = _plan(ctx, nside, max_halos=3 * n)
    plan_p = _plan(ctx, nside, max_halos=3 * n, paint=True)
    first, cuts, rb = _band_bounds(plan, nside, world)
    npix = 12 * nside * nside
    cd, cols = _upload(ctx, cat, K0_COLS)
    full = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    plan.offsets(cd, full.data_ptr(), acc_f64=False)
    full_p = torch.zeros(npix, dtype=torch.float64, device=dev)
    plan_p.paint(cd, full_p.data_ptr(), acc_f64=True)
    plain = Guarded(ctx, n, torch.int64)
    tot_plain = plan.count_pairs(cd, True, plain.ptr())
    plain_h = plain.t.cpu().numpy()
    assert plain.intact() and tot_plain == plain_h.sum() and (plain_h > 0).all() and torch.isfinite(full).all().item()
    # the halos on the poles exactly (dec = 90 used to fall outside the sphere by one rounding and was dropped): the reference's pixel counts
    poles = RO.true_ring_ranges(nside, {k: cat[k][8:12] for k in ('M', 'z', 'ra', 'dec')}, EPS, ctx.bg)['npix_disc']
    assert np.array_equal(plain_h[8:12], np.where(poles < 4, 4, poles))
    recvs, cap, want = _routed_blocks(ctx, plan, cat, rb, 0)
    assert world * cap <= plan.max_halos
    order = np.argsort(cat['ra'])
    taken = 0
    try:
        for p in (plan, plan_p):
            p.set_catalog_blocks(cap, NCOLS * cap)
        for rk in range(world):
            g, recv = recvs[rk]
            cdb = _blocked_catalog(ctx, recv, world, cap)
            # (a)
            cnt = Guarded(ctx, world * cap, torch.int64)
            tot = plan.count_pairs(cdb, True, cnt.ptr())
            h, ch = recv.cpu().numpy(), cnt.t.cpu().numpy().reshape(world, cap)
            real = ~np.isnan(h[:, 0])
            ids = order[np.searchsorted(cat['ra'][order], h[:, 2][real])]
            assert cnt.intact() and g.intact() and np.array_equal(cat['ra'][ids], h[:, 2][real])
            assert (ch[~real] == 0).all() and np.array_equal(ch[real], plain_h[ids]) and tot == plain_h[ids].sum()
            assert np.array_equal(np.sort(ids), want[rk])
            for k, name in enumerate(K0_COLS):
                assert np.array_equal(h[:, k][real], cat[name][ids])
            taken += ids.size
            # (b)
            b0, b1 = int(cuts[rk]), int(cuts[rk + 1])
            p0, p1 = int(first[b0]), int(first[b1])
            sl = Guarded(ctx, (p1 - p0) * 3, torch.float32, fill=float('nan'))
            plan.offsets_bands(cdb, b0, b1, sl.ptr(), acc_f64=False)
            slp = Guarded(ctx, p1 - p0, torch.float64, fill=float('nan'))
            plan_p.paint_bands(cdb, b0, b1, slp.ptr(), acc_f64=True)
            torch.cuda.synchronize()
            plan.status()
            plan_p.status()
            assert sl.intact() and slp.intact() and torch.isfinite(sl.t).all().item() and torch.isfinite(slp.t).all().item()
            assert (sl.t - full[p0 * 3:p1 * 3]).abs().max().item() <= 2e-6 * full.abs().max().item()
            assert (slp.t - full_p[p0:p1]).abs().max().item() <= 1e-12 * full_p.abs().max().item()
    finally:
        for p in (plan, plan_p):
            p.set_catalog_blocks(0, 0)
    assert n <= taken <= 1.5 * n
    # (d)
    again = Guarded(ctx, n, torch.int64)
    assert plan.count_pairs(cd, True, again.ptr()) == tot_plain and torch.equal(again.t, plain.t) and again.intact()
    full2 = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    plan.offsets(cd, full2.data_ptr(), acc_f64=False)
    assert (full2 - full).abs().max().item() <= 2e-6 * full.abs().max().item() and full.abs().max().item() > 0


@pytest.mark.parametrize('world', [3, 8])
def test_fused_band_entry_on_routed_blocks_assembles_the_single_gpu_map(ctx, world):
    """(c) With a route margin of one band every rank receives the halos of the bands next to its own; offsets_regrid_bands over
    [b0 - 1, b1 + 1) on the blocked catalog computes its apron rows locally.  The assembled map equals the single-GPU baryonify within
    the stated fp32 tolerance, 1e-6 mean(map); every pixel is stored once; the mass sums agree.  Would fail for the margin ignored in
    route_step (apron rows without their halos), for K0 reading the blocks by plain index."""
    torch, dev, nside = ctx.torch, ctx.dev, K0_NSIDE
    cat = _k0_catalog(ctx)
    n = cat['M'].size
    plan = _plan(ctx, nside, max_halos=3 * n)
    first, cuts, rb = _band_bounds(plan, nside, world)
    nbands, BR, npix = len(first) - 1, plan.tile_shape()[0], 12 * nside * nside
    hmap = ctx.syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    cd, cols = _upload(ctx, cat, K0_COLS)
    full_off = torch.empty(npix * 3, dtype=torch.float32, device=dev)
    full_out = torch.empty(npix, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.baryonify(cd, d_map.data_ptr(), full_off.data_ptr(), full_out.data_ptr(), sums.data_ptr(), acc_f64=False)
    torch.cuda.synchronize()
    plan.status()
    m2 = torch.empty(1, dtype=torch.float32, device=dev)
    plan.max_offset2(full_off.data_ptr(), npix, m2.data_ptr(), acc_f64=False)
    reach = plan.reach_rings(float(m2.item()) ** 0.5)
    assert reach <= BR                                                       # the apron fits into one band
    recvs, cap, want = _routed_blocks(ctx, plan, cat, rb, BR)
    assert world * cap <= plan.max_halos
    new = Guarded(ctx, npix, torch.float64, fill=float('nan'))
    far_acc = torch.zeros(npix, dtype=torch.float64, device=dev)
    s_in, s_out = 0.0, 0.0
    try:
        plan.set_band_reach(reach)
        plan.set_catalog_blocks(cap, NCOLS * cap)
        for rk in range(world):
            g, recv = recvs[rk]
            cdb = _blocked_catalog(ctx, recv, world, cap)
            b0, b1 = int(cuts[rk]), int(cuts[rk + 1])
            B0, B1 = max(b0 - 1, 0), min(b1 + 1, nbands)
            p0, p1 = int(first[b0]), int(first[b1])
            work = Guarded(ctx, (int(first[B1]) - int(first[B0])) * 3, torch.float32, fill=float('nan'))
            rs, foreign = Guarded(ctx, 2, torch.float64, fill=0.0), Guarded(ctx, 1, torch.int64, fill=0)
            plan.offsets_regrid_bands(cdb, B0, B1, work.ptr(), b0, b1, d_map.data_ptr(), new.t[p0:].data_ptr(), rs.ptr(), foreign.ptr(), acc_f64=False)
            torch.cuda.synchronize()
            plan.status()
            assert work.intact() and rs.intact() and foreign.intact() and new.intact() and g.intact()
            fp, fv = plan.far_fetch()
            away = (fp < p0) | (fp >= p1)
            assert int(foreign.t.item()) == int(away.sum())
            if away.any():                                                    # far deposits into another rank's pixels: listed, not applied
                far_acc.index_add_(0, torch.from_numpy(fp[away]).to(dev), torch.from_numpy(fv[away]).to(dev))
            r2 = rs.t.cpu().numpy()
            s_in += r2[0]; s_out += r2[1]
    finally:
        plan.set_catalog_blocks(0, 0)
        plan.set_band_reach(1)
    assert torch.isfinite(new.t).all().item()
    s = sums.cpu().numpy()
    assert np.isclose(s[1], s[0]) and np.isclose(s_in, hmap.sum(), rtol=1e-12) and np.isclose(s_out, s_in) and np.isclose(s_in, s[0], rtol=1e-12)
    diff = (new.t + far_acc - full_out).abs()
    assert diff.max().item() <= 1e-6 * hmap.mean() and (full_out - d_map).abs().max().item() > 0
