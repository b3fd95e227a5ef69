"""The three-way comparison of test_gpu_step_matrix.py for the norm-free conv encoder / decoder: three optimiser steps eagerly,
as one eager step followed by two hipGraph replays (graph.GraphedStep), and as one eager step, a pickle round trip of the whole agent and
two more steps on the copy -- everything that file compares agrees under torch.equal.  B4 x T16 at tiny widths, `slow_target_update=2`, the
defaults' learning rates; its helpers are used as they are, with these ids added to the table its legs build from:

  nf_v2      : dreamer_v2, both conv blocks norm-free
  nf_v2e     : the same + ELU in all six blocks: the DreamerV2 network as published
  nf_v3      : dreamer_v3, both conv blocks norm-free
  nf_v3d_mix : dreamer_v3, the decoder alone norm-free, image + `proprio` (7,) observations
  p2e_nf_v2  : Plan2Explore on dreamer_v2 with both conv blocks norm-free
  genrl_nf   : GenRLAgent with both conv blocks norm-free (eager and resume, as test_gpu_step_matrix.py runs its `genrl`); that file's build
               passes no overrides to GenRLAgent, so this leg builds its own agent

Per case the norm-free route is live: the stacks hold no LayerNorm, genrl_chan_act_{fwd,bwd}_h2u were entered, and no conv layer of a
norm-free stack went through a channel-LayerNorm."""
import gc

import pytest
import torch

import detgen
import convfree_cases as C
import elu_cases as E
import test_gpu_step_matrix as SM
from test_gpu_convfree import CHAN, CHAN_LN, count_entries
from test_gpu_elu import count_calls

pytestmark = pytest.mark.gpu

BOTH = ('encoder', 'decoder')
# id -> (agent kind, defaults, norm-free blocks, ELU blocks, vector observations)
NF_CASES = {'nf_v2': ('dreamer', 'dreamer_v2', BOTH, (), None), 'nf_v2e': ('dreamer', 'dreamer_v2', BOTH, E.BLOCKS, None),
            'nf_v3': ('dreamer', 'dreamer_v3', BOTH, (), None), 'nf_v3d_mix': ('dreamer', 'dreamer_v3', ('decoder',), (), {'proprio': 7}),
            'p2e_nf_v2': ('p2e', 'dreamer_v2', BOTH, (), None), 'genrl_nf': ('genrl', None, BOTH, (), None)}


def _overrides(free, elu, vec_obs):
    from genrl_amd import config
    over = SM._merge(config.vecobs_overrides('mix'), {}) if vec_obs else {}
    over = SM._merge(over, {k: dict(norm='none') for k in free})
    return E.elu_overrides(elu, over)


def _live(kind, free, elu):
    def live(ag, m):
        mods = {'encoder': ag.wm.encoder, 'decoder': ag.wm.heads['decoder']}
        ok = all((not C.norm_params(mod)) == (name in free) for name, mod in mods.items())
        if kind != 'genrl':
            ok = ok and E.acts_of(ag) == {k: ('ELU' if k in elu else 'SiLU') for k in E.BLOCKS}
        return ok and (kind != 'p2e' or ('disagreement_loss' in m and ag.reward_free))
    return live


def _cases():
    return {cid: (kind, defaults, _overrides(free, elu, vec_obs), vec_obs, _live(kind, free, elu))
            for cid, (kind, defaults, free, elu, vec_obs) in NF_CASES.items()}


def _build(case):
    """SM.build, with the overrides handed to GenRLAgent too"""
    from genrl_amd import config
    kind, defaults, over, vec_obs, _ = _cases()[case]
    if kind != 'genrl':
        return _build.orig(case)
    ag = config.make_agent(config.default_cfg(SM.B, SM.T, device='cuda', **SM._merge(config.tiny_overrides(), over, dict(slow_target_update=2))))
    ag.wm.viclip_model = SM._bench().TextStub()
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in ag.state_dict().items()}, SM.SEED)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    return ag


@pytest.mark.parametrize('case', sorted(NF_CASES))
def test_three_steps_eager_replay_resume(case, monkeypatch):
    from genrl_amd import planes
    from genrl_amd.agent import dreamer_utils as common
    kind, defaults, free, elu, vec_obs = NF_CASES[case]
    _build.orig = SM.build
    monkeypatch.setattr(SM, '_cases', _cases)
    monkeypatch.setattr(SM, 'build', _build)
    if kind == 'genrl':
        monkeypatch.setattr(SM, 'step_fn', lambda c: SM._bench().one_step)
    assert common.planes_route(SM.B * SM.T) and planes.tn_ok(SM.B * SM.T, 32, 32, 32)
    batches, obs = SM.make_batches(case)
    cache = {}
    try:
        with monkeypatch.context() as mp:
            calls = count_calls(mp)
            n = count_entries(mp, CHAN + CHAN_LN)
            eager = SM.eager_leg(case, batches, obs, cache)
        print(case, calls, n)
        assert eager['live'], (case, 'the configured stacks are not the ones that ran')
        layers = (4 if 'encoder' in free else 0) + (3 if 'decoder' in free else 0)
        assert n[CHAN[0]] >= layers * SM.STEPS and n[CHAN[1]] >= layers * SM.STEPS, (case, n)
        ln_convs = sum(v for k, v in calls.items() if isinstance(k, tuple) and k[0] in ('conv_fp32', 'conv_planes'))
        if layers == 7:
            assert ln_convs == 0 and n[CHAN_LN[0]] == 0 and n[CHAN_LN[1]] == 0, (case, calls, n)
        else:
            assert ln_convs >= 4 * SM.STEPS, (case, calls)           # the encoder kept its channel-LayerNorms
        SM.check_leg(case, 'eager', eager)
        legs = {'resume': SM.resume_leg}
        if kind != 'genrl':
            legs['replay'] = SM.replay_leg
        for leg in sorted(legs):
            out = legs[leg](case, batches, obs, cache)
            SM.check_leg(case, leg, out)
            for i, (x, y) in enumerate(zip(eager['snap1']['groups'], out['snap1']['groups'])):
                SM.same_tensor((case, leg, 'after step 1: group', i), x['flat'], y['flat'])
            SM.compare(case, leg, eager, out)
    finally:
        cache.clear()
        gc.collect()
