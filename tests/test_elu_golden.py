"""`act: ELU` without a GPU: DreamerAgent and Plan2Explore construct for every case of tests/golden/elu_tiny.npz (generated from the reference
by tests/golden/make_elu_golden.py) with the reference's state_dict contract, every block's activation is read from its module, an
unknown name raises in each of the six blocks (`rssm` included, where it used to be ignored), GenRLAgent refuses a non-SiLU block, agents
built without `act` are what they were, and the ops refuse CPU tensors."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import detgen
import elu_cases as E


def build(kind, defaults, over, B=2, T=18, A=6):
    from genrl_amd import config
    over = dict(config.dreamer_tiny_overrides(), **over)
    if kind == 'p2e':
        return config.make_p2e_agent(config.p2e_cfg(B, T, device='cpu', defaults=defaults, **over), act_dim=A)
    return config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cpu', defaults=defaults, **over), act_dim=A)


@pytest.mark.parametrize('case', sorted(E.CASES))
def test_both_agents_construct_with_the_reference_state_dict(case):
    from genrl_amd import config
    g = E.load()
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, blocks = E.CASES[case]
    over = E.elu_overrides(blocks, config.dreamer_tiny_overrides())
    dr, pe = build('dreamer', defaults, over, B, T, A), build('p2e', defaults, over, B, T, A)
    shapes = E.shapes_of(g, case)
    assert {k: tuple(v.shape) for k, v in dr.state_dict().items()} == shapes
    assert {k: tuple(v.shape) for k, v in pe.state_dict().items() if not k.startswith('disagreement.')} == shapes
    for ag in (dr, pe):
        assert E.acts_of(ag) == {k: ('ELU' if k in blocks else 'SiLU') for k in E.BLOCKS}
        # the nn modules that sit in the Sequentials (get_act) follow: state_dict keys and indices are the reference's
        for name, mod in E.block_modules(ag).items():
            want = nn.ELU if name in blocks else nn.SiLU
            subs = [s for s in mod.modules() if isinstance(s, (nn.ELU, nn.SiLU))]
            assert all(type(s) is want for s in subs), (name, subs)
            assert len(subs) == {'encoder': 4, 'decoder': 3}.get(name, 0), (name, subs)
    dr.load_state_dict(detgen.det_state_dict(shapes, seed))


@pytest.mark.parametrize('defaults', ['dreamer_v3', 'dreamer_v2'])
@pytest.mark.parametrize('block', E.BLOCKS)
def test_an_unknown_activation_raises_in_every_block(block, defaults):
    with pytest.raises(NotImplementedError, match='GELU'):
        build('dreamer', defaults, {block: dict(act='GELU')})
    with pytest.raises(NotImplementedError, match='GELU'):
        build('p2e', defaults, {block: dict(act='GELU')})


def test_modules_refuse_an_unknown_name_on_their_own():
    from genrl_amd.agent import dreamer_utils as common
    with pytest.raises(NotImplementedError, match='Tanh'):
        common.EnsembleRSSM(ensemble=1, stoch=4, discrete=4, deter=32, hidden=32, norm='layer', act='Tanh', action_dim=6, embed_dim=64, device='cpu')
    with pytest.raises(NotImplementedError, match='elu'):
        common.MLP(36, (1,), 2, 32, act='elu', norm='layer', dist='mse')
    rssm = common.EnsembleRSSM(ensemble=1, stoch=4, discrete=4, deter=32, hidden=32, norm='none', act='ELU', action_dim=6, embed_dim=64, device='cpu')
    assert rssm._act == 'ELU' and rssm._img_in[0].bias is None
    assert isinstance(common.get_act('ELU'), nn.ELU) and isinstance(common.get_act('SiLU'), nn.SiLU)


@pytest.mark.parametrize('block', E.BLOCKS + ('connector_rssm',))
def test_genrl_agent_refuses_a_non_silu_block(block):
    from genrl_amd import config
    cfg = config.default_cfg(2, 16, device='cpu', **dict(config.tiny_overrides(), **{block: dict(config.tiny_overrides().get(block, {}), act='ELU')}))
    with pytest.raises(NotImplementedError, match=block):
        config.make_agent(cfg, act_dim=10)
    cfg = config.default_cfg(2, 16, device='cpu', **dict(config.tiny_overrides(), **{block: dict(config.tiny_overrides().get(block, {}), act='SiLU')}))
    config.make_agent(cfg, act_dim=10)               # (naming the default is no refusal)


def test_the_connector_refuses_a_non_silu_act_on_its_own():
    """VideoSSM inherits EnsembleRSSM's `act`; its own layers are SiLU, so it raises where GenRLAgent's check is not in front of it"""
    from genrl_amd.agent import video_utils
    kw = dict(ensemble=1, stoch=4, discrete=4, deter=32, hidden=32, norm='layer', action_dim=512 + 8, embed_dim=64, device='cpu',
              rescale_embeds=True, denoising_ae=True)
    with pytest.raises(NotImplementedError, match='connector_rssm.act'):
        video_utils.VideoSSM(act='ELU', **kw)
    assert video_utils.VideoSSM(act='SiLU', **kw)._act == 'SiLU'


@pytest.mark.parametrize('kind', ['dreamer', 'p2e'])
@pytest.mark.parametrize('defaults', ['dreamer_v3', 'dreamer_v2'])
def test_agents_built_without_act_are_silu_everywhere_with_the_same_fused_flags(defaults, kind):
    ag = build(kind, defaults, {})
    assert E.acts_of(ag) == dict.fromkeys(E.BLOCKS, 'SiLU')
    assert not any(isinstance(s, nn.ELU) for s in ag.modules()) and any(isinstance(s, nn.SiLU) for s in ag.modules())
    head, lat = ag._acting_behavior.actor._out._head, ag.wm.rssm._latent
    assert lat.fused and head.fused == (defaults == 'dreamer_v3')
    assert ag.wm.rssm._norm == ('layer' if defaults == 'dreamer_v3' else 'none')
    g = E.load()
    plain = {k: v for k, v in E.shapes_of(g, 'v3e' if defaults == 'dreamer_v3' else 'v2e').items()}
    assert {k: tuple(v.shape) for k, v in ag.state_dict().items() if not k.startswith('disagreement.')} == plain    # ELU has no parameters


def test_the_one_table_of_codes():
    from genrl_amd import ops
    assert ops.ACTS == {'SiLU': 1, 'ELU': 2}
    assert [ops.act_code(a) for a in ('SiLU', 'ELU', True, False, 0, 1, 2)] == [1, 2, 1, 0, 0, 1, 2]
    for bad in ('GELU', 'elu', 'none', 3, -1):
        with pytest.raises(NotImplementedError):
            ops.act_code(bad)
    for none in (False, 0):              # a dense layer IS its activation: no code 0 there (ops.linear is the layer without one)
        with pytest.raises(NotImplementedError):
            ops.dense_act(torch.zeros(8, 16), None, torch.zeros(32, 16), act=none)
        with pytest.raises(NotImplementedError):
            ops.act_layer_code(none)
    assert ops._ln_code((None, None, 1e-3)) == 1 and ops._ln_code((None, None, 1e-3, 'ELU')) == 2
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'genrl_hip.h')).read()
    for name, code in (('NONE', 0), ('SILU', 1), ('ELU', 2)):
        assert f'#define GENRL_ACT_{name} {code}' in hdr
    from genrl_amd._lib import parse_header
    assert {'genrl_elu_fwd_h2', 'genrl_elu_bwd_h2'} <= set(parse_header())


def test_ops_refuse_cpu_tensors():
    from genrl_amd import ops, ops_planes
    from genrl_amd._lib import GenrlHipError
    x, W, b = torch.zeros(8, 16), torch.zeros(32, 16), torch.zeros(32)
    ga, be = torch.ones(32), torch.zeros(32)
    for act in ('ELU', 'SiLU'):
        with pytest.raises(GenrlHipError):
            ops.ln_act(torch.zeros(8, 32), ga, be, 1e-3, act=act)
        with pytest.raises(GenrlHipError):
            ops.dense_ln_act(x, None, W, b, ga, be, 1e-3, act=act)
        with pytest.raises(GenrlHipError):
            ops.dense_act(x, None, W, act=act)
        with pytest.raises(GenrlHipError):
            ops_planes.dense_ln_act(x, None, W, b, ga, be, 1e-3, act=act)
        with pytest.raises(GenrlHipError):
            ops_planes.dense_act(x, None, W, act=act)
    with pytest.raises(GenrlHipError):
        ops.act_fwd_raw(2, x, x.clone(), 8, 16)
    with pytest.raises(GenrlHipError):
        ops.conv2d_s2(torch.zeros(1, 8, 8, 4), torch.zeros(8, 4, 4, 4), torch.zeros(8), ln=(torch.ones(8), torch.zeros(8), 1e-3, 'ELU'))


def test_fixture_seed_conditions_and_size():
    g = E.load()
    assert float(g['race_margin']) >= 1e-3
    assert g['race_margins'].shape == (157,) and float(g['race_margins'].min()) == float(g['race_margin'])
    tried = g['seeds_tried']                  # the search ran from seed 5: every earlier seed missed the margin, the last one is the seed kept
    assert int(tried[0, 0]) == 5 and int(tried[-1, 0]) == int(g['seed']) and (tried[:-1, 1] < 1e-3).all() and tried[-1, 1] >= 1e-3
    seeds = {int(g[f'{case}.meta'][6]) for case in E.CASES}
    assert seeds == {int(g['seed'])}
    for case in E.CASES:
        mets = E.metrics_of(g, case)
        assert all(np.isfinite(v) for v in mets.values()) and len(mets) > 10
        for ph in ('model', 'actor', 'critic'):
            assert len(E.unpack(g, f'{case}.grad.{ph}')) > 0
        assert set(E.unpack(g, f'{case}.delta')) <= set(E.shapes_of(g, case))
    # the three cases are three computations: ELU in the world model moves the posterior's path, ELU in the actor alone the actions
    assert not np.array_equal(g['v3e.imag_action'], g['v3a.imag_action'])
    assert abs(E.metrics_of(g, 'v3e')['model_loss'] - E.metrics_of(g, 'v3a')['model_loss']) > 1e-3
    assert g['act.eval.action'].shape == g['act.sample.action'].shape == (6,)
    assert os.path.getsize(os.path.join(E.G, 'elu_tiny.npz')) <= os.path.getsize(os.path.join(E.G, 'v2_tiny.npz'))
