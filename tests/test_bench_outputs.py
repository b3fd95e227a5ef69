"""bench.py --dump-outputs: what the last timed step computed, written as float .npy files of a bounded size and sampled the
same way from run to run (so that two builds can be compared output for output).  CPU only: a stand-in module for the agent."""
import os
import numpy as np
import torch

import bench


class _Agent(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.big = torch.nn.Parameter(torch.arange(300_000, dtype=torch.float32))
        self.small = torch.nn.Parameter(torch.ones(3, 5))
        self.register_buffer('count', torch.tensor(7))             # (an integer buffer: not an output)


def test_step_outputs_sample_is_fixed_bounded_and_float(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE_ELEMS', 10_000)
    ag = _Agent()
    mets = {'model_loss': torch.tensor(1.5), 'actor_ent_scale': 0.25, 'note': 'text'}
    a, b = bench.step_outputs(ag, mets), bench.step_outputs(ag, mets)
    assert sorted(a) == ['metric.actor_ent_scale', 'metric.model_loss', 'param.big', 'param.small']
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert a['metric.model_loss'].dtype == np.float64 and float(a['metric.model_loss']) == 1.5
    big = a['param.big']
    assert big.dtype == np.float32 and 1024 <= big.size <= 10_000
    assert np.all(np.diff(big) > 0)                                 # sorted distinct indices of arange: the values are the indices
    np.testing.assert_array_equal(a['param.small'], np.ones(15, np.float32))
    bench.write_outputs(str(tmp_path / 'out'), a)
    files = sorted(os.listdir(tmp_path / 'out'))
    assert files == sorted(k + '.npy' for k in a)
    np.testing.assert_array_equal(np.load(tmp_path / 'out' / 'param.big.npy'), big)
