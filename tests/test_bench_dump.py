"""bench.py --dump-outputs: what dump_outputs() writes (no GPU: the same code path on host tensors).  The run itself is in
tests/test_gpu_bench_contract.py::test_dump_outputs_repeatable."""
import os

import numpy as np
import torch

import bench


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    m = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / 'd'), {'map': m, 'sums': torch.tensor([1.5, 2.5], dtype=torch.float64),
                                             'counts': np.array([3, 4], dtype=np.int64)})
    f = _files(tmp_path / 'd')
    assert set(f) == {'map', 'sums', 'counts'} and all(v.dtype == np.float64 for v in f.values())
    assert np.array_equal(f['map'], np.arange(1000.0)) and np.array_equal(f['sums'], [1.5, 2.5]) and np.array_equal(f['counts'], [3.0, 4.0])


def test_large_outputs_are_a_fixed_seeded_sample_under_64_mb(tmp_path):
    n = 12 * 1024 ** 2                                      # the NSIDE 1024 shell of the default bench line
    m = torch.arange(n, dtype=torch.float64) * 0.5
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), {'map': m})
    a, b = _files(tmp_path / 'a'), _files(tmp_path / 'b')
    assert set(a) == {'map_sample', 'map_index'} and a['map_index'].dtype == np.float64
    idx = a['map_index'].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n and idx.size > bench.DUMP_SAMPLE // 2
    assert np.array_equal(a['map_sample'], idx * 0.5)                         # the sample IS the map at those indices
    assert np.array_equal(a['map_index'], b['map_index']) and np.array_equal(a['map_sample'], b['map_sample'])
    assert sum(os.path.getsize(os.path.join(tmp_path / 'a', f)) for f in os.listdir(tmp_path / 'a')) < 64 << 20
    # the same directory reused for a small map: the sampled form of the earlier run does not linger next to the whole one
    bench.dump_outputs(str(tmp_path / 'a'), {'map': m[:10]})
    assert set(_files(tmp_path / 'a')) == {'map'}
