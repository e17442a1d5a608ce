"""CPU checks of tests/fft_oracle.py: the long-double DFT agrees with numpy's FFT, numpy's own error against it -- the figure the GPU
bounds in test_gpu_fft.py are built on -- stays where it was measured, the per-column reference of the binned pass adds up to the
full-cube oracle, and the bin-edge shapes of the GPU tests really are shapes where the edge rule decides a bin."""
import numpy as np
import pytest

import fft_oracle as O

SIZES = (8, 16, 32, 64, 128, 256, 512, 1024)
NUMPY_ERR_MAX = 5e-16             # measured 1-D: 1.0e-16 (8), 2.2e-16 (64), 2.4e-16 (512), 2.9e-16 (1024); 2-D: 2.4e-16 (64), 3.1e-16 (256), 3.3e-16 (1024)


@pytest.mark.parametrize('N', SIZES)
def test_dft_ld_vs_numpy_lines(N):
    """one transform, two implementations: a wrong index, sign or wrap in dft_ld shows at full scale, numpy's rounding at 1e-16"""
    e = O.numpy_error(N, 1)
    print("numpy 1-D error vs long double, N = %4d: %.2e" % (N, e))
    assert 0 < e < NUMPY_ERR_MAX


@pytest.mark.parametrize('N', SIZES)
def test_numpy_plane_error_stays_where_the_gpu_bound_assumes_it(N):
    e = O.numpy_error(N)
    print("numpy 2-D error vs long double, N = %4d: %.2e" % (N, e))
    assert 0 < e < NUMPY_ERR_MAX
    assert O.bound(N) <= O.MARGIN * NUMPY_ERR_MAX
    if N > O.LD_WHOLE_PLANES_MAX_N:
        assert e <= 1.25 * O.NUMPY_ERR_RECORDED and O.bound(N) == O.MARGIN * O.NUMPY_ERR_RECORDED


def test_dft_ld_on_exact_inputs():
    """an impulse and a plane wave have spectra known in closed form: dft_ld reproduces them to long-double rounding"""
    for N in (8, 64):
        for (i0, j0) in ((0, 0), (1, 0), (0, 1), (N - 1, N - 1), (N // 2, 3)):
            x = np.zeros((1, N, N))
            x[0, i0, j0] = 1.0
            ref = O.impulse_ref(N, i0, j0)
            assert np.abs(np.abs(ref) - 1).max() < 1e-18
            assert np.abs(O.planes_ref(x, exact=True)[0] - ref).max() < 1e-17
        for (p, q) in ((0, 0), (1, 0), (0, 1), (N // 2, N // 2), (N - 1, 1), (3, N // 2 - 1), (5, N // 2)):
            got = O.planes_ref(O.plane_wave(N, p, q)[None], exact=True)[0]
            ref = O.plane_wave_ref(N, p, q)
            assert sorted(set(ref.ravel())) in ([0.0, 0.5 * N * N], [0.0, N * N], [0.0, 0.5 * N * N, N * N])
            assert ref.sum() in (0.5 * N * N, N * N)            # (the mirror peak lies in the half that is not kept, or both are kept)
            assert np.abs(got - ref).max() < 4e-16 * N * N      # (the fp64 rounding of the cosines themselves, N^2 of them)


@pytest.mark.parametrize('N,nk,blocks', [(16, 7, (1, 2, 3, 10)), (32, 15, (32,)), (32, 15, (3,) * 10 + (2,))])
def test_axis0_pk_ref_over_column_blocks_is_the_full_cube_oracle(N, nk, blocks):
    from oracle import grid as G
    rng = np.random.default_rng(N)
    Map = rng.poisson(4.0, (N, N, N)).astype(np.float64)
    Map[3, 5, 7] += 500.0
    L = 305.0
    k_cen, Pk, k_c = G.power_spectrum(Map, L, nk)
    half = O.planes_ref(Map, exact=False)                       # [a][b][c], the first axis still in real space
    assert sum(blocks) == N
    pk, ks, cnt = np.zeros(nk), np.zeros(nk), np.zeros(nk, dtype=np.int64)
    col0 = 0
    for n in blocks:
        p, k, c = O.axis0_pk_ref(half[:, col0:col0 + n, :], N, col0, L, nk)
        pk += p; ks += k; cnt += c
        col0 += n
    assert np.array_equal(cnt, k_c) and (k_c > 0).all()
    assert np.abs(ks / (k_cen * k_c) - 1).max() <= 1e-13
    assert np.abs(pk / (Pk * k_c) - 1).max() <= 1e-13


# the shapes at which test_gpu_fft.py calls the public entry for the sake of the bin edges: (N, Nk, L)
EDGE_SHAPES = [(64, 31, 305.0), (64, 31, 1.0), (64, 62, 1000 / 3), (32, 5, 305.0)]


@pytest.mark.parametrize('N,nk,L', EDGE_SHAPES)
def test_edge_shapes_exercise_the_edge_rule(N, nk, L):
    differ, on_edge = O.edge_disagreements(N, L, nk)
    print("(%d, %d, %r): reciprocal floor != division floor at %d modes of the half spectrum, %d modes on an edge" % (N, nk, L, differ, on_edge))
    assert differ > 0


@pytest.mark.parametrize('N,nk', [(8, 3), (16, 5), (64, 180), (128, 60)])
def test_the_older_shapes_do_not(N, nk):
    """(why the shapes above were added: at test_gpu_grid.py's parametrisation the two floors never differ)"""
    assert O.edge_disagreements(N, 305.0, nk)[0] == 0


def test_without_the_division_the_counts_would_differ():
    """at (64, 31, 305.0) the reciprocal floor alone puts other numbers of modes into the bins, so the equality of counts that
    test_gpu_fft.py asserts there depends on pk_bin_of's fall-back to the division"""
    from oracle import grid as G
    N, nk, L = 64, 31, 305.0
    true = O.counts_by_rule(N, L, nk, False)
    assert np.array_equal(true, G.power_spectrum(np.zeros((N, N, N)), L, nk)[2])
    assert not np.array_equal(O.counts_by_rule(N, L, nk, True), true)


@pytest.mark.parametrize('N', [8, 16, 64, 256, 512, 1024])
@pytest.mark.parametrize('nk', [254, 2048])
def test_one_hot_modes_reach_the_bins(N, nk):
    modes = O.one_hot_modes(N)
    assert all(0 <= a < N and 0 <= b < N and 0 <= c <= N // 2 for (a, b, c) in modes) and len(set(modes)) >= len(modes) - 2
    bins = [int(O.mode_k_and_bin(N, O.ONE_HOT_L, nk, a, b, c)[1]) for (a, b, c) in modes]
    inside = [m for m, bn in zip(modes, bins) if 0 <= bn < nk]
    assert len(inside) >= 20 and len(inside) <= len(modes) - 8           # both outcomes: a peak in its bin, and no peak anywhere
    assert any(c == 0 for (_, _, c) in inside) and any(0 < c < N // 2 for (_, _, c) in inside)       # weights 1 and 2
    assert len({a for (a, _, _) in inside if a % 2}) >= 3                  # odd rows: an even multiplier in the row permutation drops them
    if N == 1024:
        assert any(c in (508, 509, 510, 511) for (_, _, c) in inside)


@pytest.mark.parametrize('N,nk', [(8, 254), (16, 254), (512, 254), (64, 2048), (256, 2048), (1024, 2048)])
def test_the_nyquist_axis_mode_lands_in_the_last_bin_here(N, nk):
    """k(0, 0, N/2) and the last bin edge are the same number computed two ways; at these shapes rounding leaves the mode inside the
    last bin, where the one-hot test then sees its weight (1: c = N/2 has no mirror image in the other half)"""
    assert (0, 0, N // 2) in O.one_hot_modes(N)
    assert int(O.mode_k_and_bin(N, O.ONE_HOT_L, nk, 0, 0, N // 2)[1]) == nk - 1
