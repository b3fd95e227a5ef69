"""The three-way comparison of test_gpu_step_matrix.py for the `act: ELU` configurations: three optimiser steps eagerly, as one eager step
followed by two hipGraph replays (graph.GraphedStep), and as one eager step, a pickle round trip of the whole agent and two more steps on
the copy -- everything that file compares agrees under torch.equal.  B4 x T16 at tiny widths, `slow_target_update=2`, the defaults'
learning rates; its helpers are used as they are, with these four ids added to the table its legs build from:

  elu_v3     : dreamer_v3, ELU in all six blocks (LayerNorm -> ELU; stepwise observe and rollout)
  elu_v2     : dreamer_v2, ELU in all six blocks (norm-free Linear -> ELU)
  elu_v3a    : dreamer_v3, ELU in the actor alone (the rollout leaves the fused node, the world model keeps its fused observe)
  p2e_elu_v2 : Plan2Explore on dreamer_v2 with ELU in all six blocks

Per case the configured activation is live: read from the modules and counted at the nodes of the eager leg."""
import gc

import pytest
import torch

import elu_cases as E
import test_gpu_step_matrix as SM
from test_gpu_elu import count_calls

pytestmark = pytest.mark.gpu

ELU_CASES = {'elu_v3': ('dreamer', 'dreamer_v3', E.BLOCKS), 'elu_v2': ('dreamer', 'dreamer_v2', E.BLOCKS),
             'elu_v3a': ('dreamer', 'dreamer_v3', ('actor',)), 'p2e_elu_v2': ('p2e', 'dreamer_v2', E.BLOCKS)}


def _cases():
    def live(kind, defaults, blocks):
        return lambda ag, m: (E.acts_of(ag) == {k: ('ELU' if k in blocks else 'SiLU') for k in E.BLOCKS}
                              and ag.wm.rssm._norm == ('layer' if defaults == 'dreamer_v3' else 'none')
                              and (kind != 'p2e' or ('disagreement_loss' in m and ag.reward_free)))
    return {cid: (kind, defaults, E.elu_overrides(blocks, {}), None, live(kind, defaults, blocks))
            for cid, (kind, defaults, blocks) in ELU_CASES.items()}


@pytest.mark.parametrize('case', sorted(ELU_CASES))
def test_three_steps_eager_replay_resume(case, monkeypatch):
    from genrl_amd import planes
    from genrl_amd.agent import dreamer_utils as common
    monkeypatch.setattr(SM, '_cases', _cases)
    assert common.planes_route(SM.B * SM.T) and planes.tn_ok(SM.B * SM.T, 32, 32, 32)
    kind, defaults, blocks = ELU_CASES[case]
    batches, obs = SM.make_batches(case)
    cache = {}
    try:
        with monkeypatch.context() as mp:
            calls = count_calls(mp)
            eager = SM.eager_leg(case, batches, obs, cache)
        print(case, calls)
        assert eager['live'], (case, 'the configured activation is not the one that ran')
        assert calls.get(('planes', 'ELU'), 0) > 0 and calls.get('rollout', 0) == 0 and calls.get('tape', 0) == 0, calls
        assert not any(k[0] == 'conv_fp32' for k in calls if isinstance(k, tuple)) and calls.get(('C', 2), 0) > 0, calls
        if len(blocks) == len(E.BLOCKS):
            assert calls.get(('planes', 'SiLU'), 0) == 0 and calls.get(('fp32', 'SiLU'), 0) == 0 and calls.get(('conv_planes', 'SiLU'), 0) == 0, calls
            assert calls.get(('conv_planes', 'ELU'), 0) > 0 and calls.get('observe_seq', 0) == 0 and calls.get(('C', 1), 0) == 0, calls
        else:
            assert calls.get('observe_seq', 0) == SM.STEPS and calls.get(('conv_planes', 'ELU'), 0) == 0 and calls.get(('C', 1), 0) > 0, calls
        SM.check_leg(case, 'eager', eager)
        if kind == 'p2e':
            assert not torch.equal(eager['snap1']['rewnorm']['mag'], eager['snap3']['rewnorm']['mag']), (case, 'StreamNorm.mag did not advance')
        for leg, fn in (('replay', SM.replay_leg), ('resume', SM.resume_leg)):
            out = fn(case, batches, obs, cache)
            SM.check_leg(case, leg, out)
            for i, (x, y) in enumerate(zip(eager['snap1']['groups'], out['snap1']['groups'])):
                SM.same_tensor((case, leg, 'after step 1: group', i), x['flat'], y['flat'])
            SM.compare(case, leg, eager, out)
    finally:
        cache.clear()
        gc.collect()
