"""Shared helpers: golden fixtures -> inputs for the oracle and for the product's runners."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
GOLDEN_CASES = ['c1_baryonify', 'lowz_baryonify', 'rdelta_baryonify', 'massdef_baryonify', 'lowz_paint', 'c1_paint', 'massdef_paint',
                'param1_paint', 'param2_paint', 'param3_paint', 'param4_paint']
COSMO_KEYS = ('Omega_m', 'Omega_b', 'h', 'sigma8', 'n_s', 'w0')


def load_golden(name):
    f = np.load(os.path.join(GOLDEN, name + '.npz'))
    g = {k: f[k] for k in f.files}
    g['kind'] = str(g['kind'])
    g['nside'] = int(g['nside'])
    g['rdelta'] = bool(g['rdelta'])
    g['eps_runner'] = float(g['eps_runner'])
    g['eps_model'] = float(g['eps_model'])
    g['cosmo_runner'] = dict(zip(COSMO_KEYS, g['cosmo_runner'].tolist()))
    g['cosmo_model'] = dict(zip(COSMO_KEYS, g['cosmo_model'].tolist()))
    g['cat'] = {'M': g['cat_M'], 'z': g['cat_z'], 'ra': g['cat_ra'], 'dec': g['cat_dec']}
    g['p_keys'] = [str(k) for k in g['p_keys']] if 'p_keys' in g else []
    g['p_axes'] = {k: g['p_axis_' + k] for k in g['p_keys']}          # per-halo property columns (model.p_keys)
    for k in g['p_keys']:
        g['cat'][k] = g['cat_' + k]
    g['map_in'] = g['map_in'].astype(np.float64)
    for k in ('md_runner', 'md_model'):          # (Delta, rho_type); fixtures older than the mass-definition cases are 200c
        g[k] = (float(g[k][0]), 'critical' if g[k][1] == 0 else 'matter') if k in g else (200.0, 'critical')
    return g


def oracle_run(g):
    from oracle import oracle as O
    axes = [np.log(1 + g['tab_z']), np.log(g['tab_M']), np.log(g['tab_r'])] + [g['p_axes'][k] for k in g['p_keys']]
    bg_r, bg_m = O.Background.from_dict(g['cosmo_runner']), O.Background.from_dict(g['cosmo_model'])
    if g['kind'] == 'baryonify':
        tab = O.Table(axes, g['tab_values'], g['rdelta'], g['eps_model'], p_keys=g['p_keys'])
        return O.baryonify_shell(g['nside'], g['map_in'], g['cat'], tab, g['eps_runner'], bg_r, bg_m, g['md_runner'], g['md_model'])
    with np.errstate(divide='ignore'):
        tab = O.Table(axes, np.log(g['tab_values']), p_keys=g['p_keys'])
    return O.paint_shell(g['nside'], g['cat'], tab, g['eps_runner'], bg_r, md_runner=g['md_runner'])


def product_runner(g, acc_f64=None):
    """Build the product's drop-in objects exactly as a BaryonForge user would."""
    import baryonification_amd as bfg
    cat = g['cat']
    Catalog = bfg.utils.HaloLightConeCatalog(ra=cat['ra'], dec=cat['dec'], M=cat['M'], z=cat['z'], cosmo=g['cosmo_runner'],
                                             **{k: cat[k] for k in g['p_keys']})
    cosmo_model = bfg.utils.Cosmology.from_dict(g['cosmo_model'])
    if g['kind'] == 'baryonify':
        Shell = bfg.utils.LightconeShell(map=g['map_in'], cosmo=g['cosmo_runner'])
        model = bfg.Profiles.Baryonification2D(None, None, cosmo_model, epsilon_max=g['eps_model'], mass_def=bfg.utils.MassDef(*g['md_model']))
        model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'], Rdelta_sampling=g['rdelta'])
        runner = bfg.Runners.BaryonifyShell(Catalog, Shell, g['eps_runner'], model, mass_def=bfg.utils.MassDef(*g['md_runner']), verbose=False)
    else:
        Shell = bfg.utils.LightconeShell(map=np.zeros(12 * g['nside'] ** 2), cosmo=g['cosmo_runner'])
        if g['p_keys']:
            model = bfg.utils.ParamTabulatedProfile(None, cosmo_model)
            model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'], other_params=g['p_axes'])
        else:
            model = bfg.utils.TabulatedProfile(None, cosmo_model)
            model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'])
        runner = bfg.Runners.PaintProfilesShell(Catalog, Shell, g['eps_runner'], model, mass_def=bfg.utils.MassDef(*g['md_runner']), verbose=False)
    runner.acc_f64 = acc_f64
    return runner


# ------------------------------------------------------------------------------------------ regular-grid path
GRID_RUNNER_CASES = ['grid2d_baryonify', 'grid2d_baryonify_ell', 'grid2d_paint', 'grid2d_paint_ell', 'grid3d_baryonify',
                     'grid3d_paint']
# PaintProfilesGrid with a ParamTabulatedProfile (model.p_keys: one or two property axes)
GRID_PARAM_CASES = ['grid2d_param1_paint', 'grid2d_param2_paint', 'grid2d_param1_paint_ell', 'grid3d_param1_paint',
                    'grid3d_param2_paint']


def phases_ok(stats):
    """the three phase times of a one-shot entry's bfgx_stats: present, finite, never negative"""
    return all(np.isfinite(stats[k]) and stats[k] >= 0 for k in ('ms_h2d', 'ms_kernels', 'ms_d2h'))


def load_grid_golden(name):
    f = np.load(os.path.join(GOLDEN, name + '.npz'))
    g = {k: f[k] for k in f.files}
    g['kind'] = str(g['kind'])
    for k in ('ndim', 'npix'):
        if k in g:
            g[k] = int(g[k])
    if g['kind'] in ('baryonify', 'paint'):
        g['rdelta'] = bool(g['rdelta'])
        for k in ('L', 'redshift', 'eps_runner', 'eps_model'):
            g[k] = float(g[k])
        g['cosmo_runner'] = dict(zip(COSMO_KEYS, g['cosmo_runner'].tolist()))
        g['cosmo_model'] = dict(zip(COSMO_KEYS, g['cosmo_model'].tolist()))
        g['cat'] = {'M': g['cat_M'], 'x': g['cat_x'], 'y': g['cat_y'], 'z': g['cat_z']}
        g['rmat'] = g['rmat'] if g['rmat'].size else None
        g['shape'] = (g['npix'],) * g['ndim']
        g['map_in'] = g['map_in'].astype(np.float64)
        g['p_keys'] = [str(k) for k in g['p_keys']] if 'p_keys' in g else []
        g['p_axes'] = {k: g['p_axis_' + k] for k in g['p_keys']}
        for k in g['p_keys']:                  # the float32-rounded property columns, as the catalog holds them
            g['cat'][k] = g['cat_' + k]
    return g


def grid_oracle_run(g):
    from oracle import grid as G
    from oracle import oracle as O
    p_keys = g.get('p_keys', [])               # (callers also pass hand-built dicts without property axes)
    axes = [np.log(1 + g['tab_z']), np.log(g['tab_M']), np.log(g['tab_r'])] + [g['p_axes'][k] for k in p_keys]
    bg = G.grid_background(g['cosmo_runner'])
    if g['kind'] == 'baryonify':
        tab = O.Table(axes, g['tab_values'], g['rdelta'], g['eps_model'], p_keys=p_keys)
        return G.baryonify_grid(g['map_in'], g['bins'], g['cat'], g['redshift'], tab, g['eps_runner'], bg,
                                O.Background.from_dict(g['cosmo_model']), g['rmat'])
    with np.errstate(divide='ignore'):
        tab = O.Table(axes, np.log(g['tab_values']), p_keys=p_keys)
    return G.paint_grid(g['shape'], g['bins'], g['cat'], g['redshift'], tab, g['eps_runner'], bg, g['rmat'])


class _FixedRmat(object):
    """mixin for the *_ell fixtures: they store the shear matrices the reference built (from float32 q_ell / A_ell
    columns that are not kept), so the product runner is handed those instead of re-deriving them"""
    _rmat_fixture = None

    def _rmats(self, what):
        return self._rmat_fixture


def grid_product_runner(g):
    """the product's drop-in objects for a grid fixture, built as a BaryonForge user would"""
    import baryonification_amd as bfg
    cat = g['cat']
    ell = g['rmat'] is not None
    extra = {}
    if ell:         # placeholders: the constructor asserts the columns exist; the matrices come from the fixture
        extra = {'q_ell': np.ones(cat['M'].size), 'A_ell': np.ones((cat['M'].size, 2))}
    p_keys = g.get('p_keys', [])
    extra.update({k: cat[k] for k in p_keys})
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], M=cat['M'], redshift=g['redshift'], cosmo=g['cosmo_runner'],
                                   z=cat['z'] if g['ndim'] == 3 else None, **extra)
    cosmo_model = bfg.utils.Cosmology.from_dict(g['cosmo_model'])
    if g['kind'] == 'baryonify':
        GMap = bfg.utils.GriddedMap(map=g['map_in'].reshape(g['shape']), redshift=g['redshift'], bins=g['bins'], cosmo=g['cosmo_runner'])
        model = bfg.Profiles.Baryonification2D(None, None, cosmo_model, epsilon_max=g['eps_model'])
        model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'], Rdelta_sampling=g['rdelta'])
        base = bfg.Runners.BaryonifyGrid
    else:
        GMap = bfg.utils.GriddedMap(map=np.zeros(g['shape']), redshift=g['redshift'], bins=g['bins'], cosmo=g['cosmo_runner'])
        if p_keys:
            model = bfg.utils.ParamTabulatedProfile(None, cosmo_model)
            model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'], other_params=g['p_axes'])
        else:
            model = bfg.utils.TabulatedProfile(None, cosmo_model)
            model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'])
        base = bfg.Runners.PaintProfilesGrid
    cls = type(base.__name__, (_FixedRmat, base), {}) if ell else base
    runner = cls(HCat, GMap, g['eps_runner'], model, use_ellipticity=ell, verbose=False)
    if ell:
        runner._rmat_fixture = g['rmat']
    return runner


# ------------------------------------------------------------------------------------------ particle snapshots
SNAPSHOT_CASES = ['snap3d_baryonify', 'snap2d_baryonify', 'snap3d_rdelta']


def snapshot_particles(seed, npart, L, halo0):
    """the particle set of the snapshot fixtures (uniform box + a clump at halo 0, incl. separations below the table's
    first radial node); regenerated from the seed so that the fixtures only carry the moved particles"""
    rng = np.random.default_rng(1000 + int(seed))
    part = rng.uniform(0, L, (npart, 3))
    part[:200] = (halo0 + rng.normal(scale=0.05, size=(200, 3))) % L
    part[200:203] = (halo0 + np.array([[1e-5, 0, 0], [0, -2e-4, 0], [3e-4, 3e-4, 3e-4]])) % L
    return part


def load_snapshot_golden(name):
    f = np.load(os.path.join(GOLDEN, name + '.npz'))
    g = {k: f[k] for k in f.files}
    g['ndim'], g['npart'], g['rdelta'] = int(g['ndim']), int(g['npart']), bool(g['rdelta'])
    for k in ('L', 'redshift', 'eps_runner', 'eps_model'):
        g[k] = float(g[k])
    g['cosmo_runner'] = dict(zip(COSMO_KEYS, g['cosmo_runner'].tolist()))
    g['cosmo_model'] = dict(zip(COSMO_KEYS, g['cosmo_model'].tolist()))
    g['cat'] = {'M': g['cat_M'], 'x': g['cat_x'], 'y': g['cat_y'], 'z': g['cat_z']}
    g['part'] = snapshot_particles(int(g['part_seed']), g['npart'], g['L'], g['halo0'])[:, :g['ndim']]
    exp = g['part'].copy()
    exp[g['moved_idx']] = g['moved_pos']
    g['expected'] = exp
    return g


def snapshot_oracle_run(g):
    from oracle import grid as G
    from oracle import oracle as O
    tab = O.Table([np.log(1 + g['tab_z']), np.log(g['tab_M']), np.log(g['tab_r'])], g['tab_values'], g['rdelta'], g['eps_model'])
    out = G.baryonify_snapshot([g['part'][:, d] for d in range(g['ndim'])], g['L'], g['cat'], g['redshift'], tab, g['eps_runner'],
                               G.grid_background(g['cosmo_runner']), O.Background.from_dict(g['cosmo_model']))
    return np.stack(out, axis=1)


def snapshot_product_runner(g):
    import baryonification_amd as bfg
    cat, part, nd = g['cat'], g['part'], g['ndim']
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], z=cat['z'] if nd == 3 else None, M=cat['M'], redshift=g['redshift'],
                                   cosmo=g['cosmo_runner'])
    Snap = bfg.utils.ParticleSnapshot(x=part[:, 0], y=part[:, 1], z=part[:, 2] if nd == 3 else None, M=np.ones(part.shape[0]), L=g['L'],
                                      redshift=g['redshift'], cosmo=g['cosmo_runner'])
    model = bfg.Profiles.Baryonification3D(None, None, bfg.utils.Cosmology.from_dict(g['cosmo_model']), epsilon_max=g['eps_model'])
    model.set_table(g['tab_z'], g['tab_M'], g['tab_r'], g['tab_values'], Rdelta_sampling=g['rdelta'])
    return bfg.Runners.BaryonifySnapshot(HCat, Snap, g['eps_runner'], model, verbose=False)
