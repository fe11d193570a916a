"""CPU: ``bench.py --dump-outputs`` — the arrays a step returned, named by their place in the output, as float32 /
float64 .npy files inside the size budget; a larger output as a fixed, seeded sample, the same in every run."""
import os

import numpy as np
import torch

import bench


def _step_output():
    g = torch.Generator().manual_seed(0)
    status = torch.zeros(1, dtype=torch.int32)
    frames = [{'color': torch.rand(2, 3, 16, 16, generator=g), 'status': status,
               'radii': torch.arange(40, dtype=torch.int32)} for _ in range(2)]
    return (torch.randn(1, 80, 40, 40, generator=g), torch.randn(1, 80, 40, 40, generator=g, dtype=torch.float64),
            frames, torch.rand(1, 1, 40, 40, generator=g).half())


def _read(d):
    return {f[:-len('.npy')]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 64 * 2 ** 20)
    out = _step_output()
    info = bench.dump_outputs(out, ('lss', 'ht', 'rendered', 'gated'), str(tmp_path))
    got = _read(str(tmp_path))
    # the status tensor every frame shares is written once, under its first name
    assert set(got) == {'lss', 'ht', 'rendered.0.color', 'rendered.0.status', 'rendered.0.radii', 'rendered.1.color',
                        'rendered.1.radii', 'gated'}
    assert got['lss'].dtype == np.float32 and np.array_equal(got['lss'], out[0].numpy())
    assert got['ht'].dtype == np.float64 and np.array_equal(got['ht'], out[1].numpy())
    assert got['rendered.1.color'].dtype == np.float32 and np.array_equal(got['rendered.1.color'], out[2][1]['color'].numpy())
    assert got['rendered.0.radii'].dtype == np.float64 and np.array_equal(got['rendered.0.radii'], np.arange(40))
    assert got['gated'].dtype == np.float32 and np.array_equal(got['gated'], out[3].float().numpy())
    assert all(v['written'] == v['elements'] for v in info.values())


def test_large_outputs_are_a_seeded_sample_within_the_budget(tmp_path, monkeypatch):
    budget = 200_000
    monkeypatch.setattr(bench, 'DUMP_BYTES', budget)
    out = _step_output()
    names = ('lss', 'ht', 'rendered', 'gated')
    a, b = tmp_path / 'a', tmp_path / 'b'
    info = bench.dump_outputs(out, names, str(a))
    bench.dump_outputs(out, names, str(b))
    ga, gb = _read(str(a)), _read(str(b))
    assert sum(v.nbytes for v in ga.values()) <= budget
    assert ga.keys() == gb.keys() and all(np.array_equal(ga[k], gb[k]) for k in ga)
    # the small arrays whole, the two BEV-sized ones sampled: their values are elements of the output
    assert info['rendered.0.radii']['written'] == 40 and info['gated']['written'] == 1600
    for k, t in (('lss', out[0]), ('ht', out[1])):
        assert 0 < info[k]['written'] < t.numel() and ga[k].ndim == 1
        assert np.isin(ga[k], t.numpy().ravel()).all()
