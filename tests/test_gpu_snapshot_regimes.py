"""The particle-snapshot kernels (csrc/bfgx_snapshot.hpp, bfgx_snapshot_api.inc) against the brute-force fp64 oracle
(oracle.grid.baryonify_snapshot = bfgo_snapshot_offsets, which knows nothing of cells, lists, pre-filters or queues) in the regimes of
snapshot_regimes.py: coarse cell grids and balls of half the box (periodic cell ranges, the corner cull), a Gpc box with group-size halos
(the 16-byte pre-filter), 61 overlapping cluster balls (the full hit queue, the inline path, lists that are no multiple of 4), particle
counts around the block and chunk sizes, re-wraps in both directions, particles on faces, surfaces and centres, halos outside the box.
test_snapshot_regimes_host.py asserts, on the CPU, that the inputs reach those mechanisms.

Positions: the NaN pattern of the oracle, and |out - ora| <= max(1e-10 scale, 1e-13 L) -- the bound of test_gpu_snapshot.py, with
scale = the largest displacement (min-image of ora - part: a re-wrapped particle does not count as displaced by the box size, which
would loosen the bound a thousandfold).  Census: the kernel's pair count equals the oracle's number of in-ball pairs exactly (the table
is strictly negative and covers every in-ball separation, d = 0 counts on both sides), so one dropped or doubled (halo, particle) pair
shows even where its offset is tiny.  Each test prints err / bound and the census (pytest -s)."""
import numpy as np
import pytest

import snapshot_regimes as SR

pytestmark = pytest.mark.gpu

DEPOSIT_GRID = {3: 33, 2: 100}


class Device(object):
    """a case on the device, as test_snapshot_device_resident_and_errors builds it"""

    def __init__(self, c, redshift=None):
        import torch
        from baryonification_amd import engine
        self.c, self.ndim, self.torch = c, c['ndim'], torch
        self.dev = torch.device('cuda:0')
        self.stream = torch.cuda.current_stream().cuda_stream
        self.redshift = c['redshift'] if redshift is None else redshift
        self.model, self.keep = engine.model_from_tables([np.log(1 + c['tab_z']), np.log(c['tab_M']), np.log(c['tab_r'])], c['tab_values'],
                                                         dict(c['cosmo'], w0=-1.0), c['eps_runner'], c['eps_model'])
        self.p = torch.tensor(np.ascontiguousarray(c['part'].T), device=self.dev)
        self.o = torch.empty_like(self.p)
        self.n = c['part'].shape[0]
        self.cats = []

    def catalog(self, M, hpos):
        from baryonification_amd import _lib
        M, hpos = np.asarray(M, dtype=np.float64), np.asarray(hpos, dtype=np.float64).reshape(-1, 3)
        with np.errstate(all='ignore'):
            lnM = np.log(M.astype(np.float32)).astype(np.float64)
        t = [self.torch.tensor(np.ascontiguousarray(v), dtype=self.torch.float64, device=self.dev) for v in (M, hpos[:, 0], hpos[:, 1], hpos[:, 2], lnM)]
        self.cats.append(t)                                          # (keeps the columns alive)
        return _lib.make_grid_catalog_dev(M.size, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr() if self.ndim == 3 else 0, t[4].data_ptr())

    def plan(self, max_halos):
        from baryonification_amd import engine
        return engine.SnapshotPlan(self.model, self.keep, self.ndim, self.c['L'], self.redshift, max_halos, 0, self.stream)

    def ptrs(self, t):
        return [t[k].data_ptr() for k in range(self.ndim)] + [0] * (3 - self.ndim)

    def displace(self, plan, dcat):
        self.o.fill_(-7.0)
        n_pairs = plan.displace(dcat, self.n, self.ptrs(self.p), self.ptrs(self.o))
        self.torch.cuda.synchronize()
        return self.o.cpu().numpy().T.copy(), n_pairs

    def run(self, M=None, hpos=None):
        """a fresh plan for one catalog (the case's own by default)"""
        M = self.c['M'] if M is None else M
        hpos = self.c['hpos'] if hpos is None else hpos
        plan = self.plan(np.size(M))
        try:
            return self.displace(plan, self.catalog(M, hpos))
        finally:
            plan.close()


def _set_cells(monkeypatch, cells):
    if cells is None:
        monkeypatch.delenv('BFGX_SNAP_CELLS', raising=False)
    else:
        monkeypatch.setenv('BFGX_SNAP_CELLS', str(cells))


def _position_error(c, out, ora):
    """(error, bound, bound with scale = max|ora - part| as test_gpu_snapshot.py writes it)"""
    scale = np.nanmax(np.abs(SR.offsets(c, ora)), initial=0.0)
    literal = np.nanmax(np.abs(ora - c['part']), initial=0.0)
    return (np.nanmax(np.abs(out - ora), initial=0.0), max(1e-10 * scale, 1e-13 * c['L']), max(1e-10 * literal, 1e-13 * c['L']))


def _close(a, b, tol):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b), initial=0.0) <= tol


@pytest.mark.parametrize('name,ndim', [(name, ndim) for name in SR.REGIMES for ndim in (2, 3)])
def test_snapshot_regime_vs_oracle(gpu, monkeypatch, name, ndim):
    """positions and census against the oracle at every cell count of the regime; the outputs of the different cell grids agree to
    1e-13 L and in their census (the grid is only an acceleration structure)"""
    c = SR.case(name, ndim)
    ora, pairs = SR.oracle(name, ndim)
    d = Device(c)
    runs, bad = [], []
    for cells in c['cells']:
        _set_cells(monkeypatch, cells)
        out, n_pairs = d.run()
        err, bound, literal = _position_error(c, out, ora)
        print('%s %dD cells %s: err %.3e / bound %.3e = %.3f (of the bound on max|ora - part|: %.2e); census %d, oracle %d'
              % (name, ndim, cells or 'default', err, bound, err / bound, err / literal, n_pairs, pairs))
        if not np.array_equal(np.isnan(out), np.isnan(ora)):
            bad.append('cells %s: NaN pattern differs at particles %s' % (cells, np.nonzero(np.isnan(out) != np.isnan(ora))[0][:8]))
        if not err <= bound:
            worst = np.argsort(-np.nan_to_num(np.abs(out - ora).max(axis=1)))[:4]
            bad.append('cells %s: err %.3e > bound %.3e, worst particles %s of kind %s' % (cells, err, bound, worst, c['kind'][worst]))
        if name == 'rcut_bites':                                     # (pairs beyond the cut have offset 0: the kernel does not count them)
            if not 0 < n_pairs <= pairs:
                bad.append('cells %s: census %d not in (0, %d]' % (cells, n_pairs, pairs))
        elif n_pairs != pairs:
            bad.append('cells %s: census %d != oracle %d' % (cells, n_pairs, pairs))
        runs.append((cells, out, n_pairs))
    for cells, out, n_pairs in runs[1:]:
        if not _close(out, runs[0][1], 1e-13 * c['L']) or n_pairs != runs[0][2]:
            bad.append('cells %s and %s disagree' % (cells, runs[0][0]))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('ndim', [2, 3])
def test_invalid_halos_change_nothing(gpu, monkeypatch, ndim):
    """halos with M = NaN, 0, < 0, x = NaN and M above the table appended to small_box: same positions (1e-13 L), same census"""
    c = SR.case('small_box', ndim)
    L = c['L']
    d = Device(c)
    for cells in (2, None):
        _set_cells(monkeypatch, cells)
        out, n_pairs = d.run()
        M = np.concatenate([c['M'], [np.nan, 0.0, -1e14, 1e14, c['tab_M'][-1] * 3.0]])
        hpos = np.concatenate([c['hpos'], [[10.0, 10.0, 10.0], [20.0, 20.0, 20.0], [30.0, 30.0, 30.0], [np.nan, 25.0, 25.0], [L / 2, L / 3, L / 4]]])
        if ndim == 2:
            hpos[:, 2] = 0.0
        out2, n_pairs2 = d.run(M, hpos)
        assert n_pairs2 == n_pairs > 0 and _close(out2, out, 1e-13 * L)
        order = np.random.default_rng(7).permutation(M.size)         # the invalid ones in between
        out3, n_pairs3 = d.run(M[order], hpos[order])
        assert n_pairs3 == n_pairs and _close(out3, out, 1e-13 * L)


@pytest.mark.parametrize('ndim', [2, 3])
def test_redshift_outside_the_table(gpu, monkeypatch, ndim):
    """every halo is out of the table: the particles come back bit for bit, nothing is counted"""
    c = SR.case('small_box', ndim)
    _set_cells(monkeypatch, None)
    for z in (0.5, 0.01):
        out, n_pairs = Device(c, redshift=z).run()
        assert n_pairs == 0 and np.array_equal(out, c['part'])


@pytest.mark.parametrize('ndim', [2, 3])
def test_one_plan_different_catalogs(gpu, monkeypatch, ndim):
    """one resident plan fed all halos, the first 5, none, all again: each answer is that of a fresh plan for that catalog (counts,
    cursors, occupancy bitmap and entries are rebuilt per call; nothing stale survives)"""
    c = SR.case('small_box', ndim)
    ora, pairs = SR.oracle('small_box', ndim)
    for cells in (3, None):
        _set_cells(monkeypatch, cells)
        d = Device(c)
        nh = c['M'].size
        fresh = {n: d.run(c['M'][:n], c['hpos'][:n]) for n in (nh, 5, 0)}
        assert fresh[nh][1] == pairs and fresh[0][1] == 0 and np.array_equal(fresh[0][0], c['part']) and 0 < fresh[5][1] < pairs
        plan = d.plan(nh)
        for n in (nh, 5, 0, nh):
            out, n_pairs = d.displace(plan, d.catalog(c['M'][:n], c['hpos'][:n]))
            assert n_pairs == fresh[n][1], (cells, n)
            assert _close(out, fresh[n][0], 1e-13 * c['L']), (cells, n)
        plan.close()


@pytest.mark.parametrize('masses', [False, True])
@pytest.mark.parametrize('name,ndim', [('small_box', 3), ('small_box', 2), ('tails_4097', 3), ('tails_4097', 2)])
def test_fused_deposit_vs_oracle(gpu, monkeypatch, name, ndim, masses):
    """plan.displace_deposit (the KEYS instantiation: the displaced position goes straight into its deposit key) == oracle.grid.make_map
    of the oracle's displaced particles, to 1e-12 max and with the same nonzero cells.  No displaced coordinate lies within 1e-9 L of a
    grid edge (asserted on the CPU), so no rounding decides a cell.  4097 particles: a last deposit chunk of one particle"""
    import torch
    from oracle import grid as G
    c = SR.case(name, ndim)
    ora, pairs = SR.oracle(name, ndim)
    _set_cells(monkeypatch, None)
    n_grid, n = DEPOSIT_GRID[ndim], c['part'].shape[0]
    mass = np.random.default_rng(9).uniform(0.5, 2.0, n) if masses else np.ones(n)
    ref = G.make_map([ora[:, k].copy() for k in range(ndim)], mass, c['L'], n_grid).ravel()
    assert np.isclose(ref.sum(), mass[~np.isnan(ora).any(axis=1)].sum(), rtol=1e-13)
    d = Device(c)
    d_mass = torch.tensor(mass, device=d.dev)
    d_edges = torch.tensor(np.linspace(0, c['L'], n_grid + 1), device=d.dev)
    got = torch.full((n_grid ** ndim,), -1.0, dtype=torch.float64, device=d.dev)
    plan = d.plan(c['M'].size)
    dcat = d.catalog(c['M'], c['hpos'])
    for _ in range(2):                                               # (twice: the deposit's workspaces are reused)
        got.fill_(-1.0)
        n_pairs = plan.displace_deposit(dcat, n, d.ptrs(d.p), d_mass.data_ptr() if masses else 0, n_grid, d_edges.data_ptr(), got.data_ptr())
        torch.cuda.synchronize()
        m = got.cpu().numpy()
        print('%s %dD masses %s: max|map - ref| / max = %.2e, census %d, oracle %d' % (name, ndim, masses, np.abs(m - ref).max() / ref.max(), n_pairs, pairs))
        assert n_pairs == pairs
        assert np.array_equal(m != 0, ref != 0)
        assert np.abs(m - ref).max() <= 1e-12 * ref.max()
    plan.close()


@pytest.mark.parametrize('ndim', [2, 3])
def test_host_entries_see_a_regime(gpu, monkeypatch, ndim):
    """small_box through bfg.Runners.BaryonifySnapshot.process(): the columns entry and the streamed records entry, coarse and default
    cells, to the position bound and with the oracle's census"""
    import baryonification_amd as bfg
    c = SR.case('small_box', ndim)
    ora, pairs = SR.oracle('small_box', ndim)
    part, hpos = c['part'], c['hpos']
    n = part.shape[0]
    HCat = bfg.utils.HaloNDCatalog(x=hpos[:, 0], y=hpos[:, 1], z=hpos[:, 2] if ndim == 3 else None, M=c['M'], redshift=c['redshift'], cosmo=c['cosmo'])
    assert np.array_equal(HCat.cat['x'].astype(np.float64), hpos[:, 0]) and np.array_equal(HCat.cat['M'].astype(np.float64), c['M'])     # float32 values
    Snap = bfg.utils.ParticleSnapshot(x=part[:, 0], y=part[:, 1], z=part[:, 2] if ndim == 3 else None, M=np.ones(n), L=c['L'], redshift=c['redshift'],
                                      cosmo=c['cosmo'])
    model = bfg.Profiles.Baryonification3D(None, None, bfg.utils.Cosmology.from_dict(c['cosmo']), epsilon_max=c['eps_model'])
    model.set_table(c['tab_z'], c['tab_M'], c['tab_r'], c['tab_values'])
    runner = bfg.Runners.BaryonifySnapshot(HCat, Snap, c['eps_runner'], model, verbose=False)
    for cells in (2, None):
        _set_cells(monkeypatch, cells)
        for records in (False, True):
            runner.use_records = records
            new = runner.process()
            out = np.stack([new[k] for k in ('x', 'y', 'z')[:ndim]], axis=1)
            err, bound, literal = _position_error(c, out, ora)
            print('small_box %dD cells %s records %s: err %.3e / bound %.3e = %.3f; census %d, oracle %d'
                  % (ndim, cells or 'default', records, err, bound, err / bound, runner.last_stats['n_pairs'], pairs))
            assert np.array_equal(np.isnan(out), np.isnan(ora)) and err <= bound
            assert runner.last_stats['n_pairs'] == pairs
