"""Norm-free conv encoder / decoder (`encoder.norm: none`, `decoder.norm: none`) without a GPU: DreamerAgent and Plan2Explore
construct for every case of tests/golden/convfree_tiny.npz (generated from the reference by tests/golden/make_convfree_golden.py) with the
reference's state_dict contract, GenRLAgent constructs with the override, any other norm name raises, agents built without the override are
what they were, a plain-torch float32 restatement of the norm-free encoder and decoder reproduces the reference's stored samples, the header
declares the two entries, and the ops refuse CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import detgen
import convfree_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(kind, case=None, over=None, defaults='dreamer_v3', B=2, T=18, A=6):
    from genrl_amd import config
    vec_obs = None
    if case is not None:
        defaults, vec_obs = C.CASES[case][0], C.CASES[case][1]
        over = C.overrides(case, config.dreamer_tiny_overrides())
    else:
        extra, over = over or {}, dict(config.dreamer_tiny_overrides())
        for k, v in extra.items():
            over[k] = dict(over.get(k, {}), **v)
    if kind == 'p2e':
        return config.make_p2e_agent(config.p2e_cfg(B, T, device='cpu', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
    return config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cpu', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)


@pytest.mark.parametrize('case', sorted(C.CASES))
def test_both_agents_construct_with_the_reference_state_dict(case):
    g = C.load()
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    free, elu = C.CASES[case][2], C.CASES[case][3]
    dr, pe = build('dreamer', case), build('p2e', case)
    shapes = C.shapes_of(g, case)
    assert {k: tuple(v.shape) for k, v in dr.state_dict().items()} == shapes
    assert {k: tuple(v.shape) for k, v in pe.state_dict().items() if not k.startswith('disagreement.')} == shapes
    for ag in (dr, pe):
        enc, dec = ag.wm.encoder, ag.wm.heads['decoder']
        for name, mod in (('encoder', enc), ('decoder', dec)):
            assert (not C.norm_params(mod)) == (name in free), (case, name)
            assert mod._norm == ('none' if name in free else 'layer')
            keys = sorted(k for k in mod.state_dict() if k.startswith('_conv_model.'))
            plain = sorted(f'_conv_model.{i}.{p}' for i in (0, 3, 6, 9) for p in ('weight', 'bias'))
            assert (keys == plain) == (name in free), (case, name, keys)
            acts = [type(m) for m in mod._conv_model if isinstance(m, (nn.SiLU, nn.ELU))]
            assert acts == [nn.ELU if name in elu else nn.SiLU] * (4 if name == 'encoder' else 3)
            if name in free and hasattr(mod, '_mlp_model'):
                assert all(m.bias is None for m in mod._mlp_model if isinstance(m, nn.Linear))
        assert {k: m._act for k, m in C.block_modules(ag).items()} == {k: ('ELU' if k in elu else 'SiLU') for k in C.BLOCKS}
    dr.load_state_dict(detgen.det_state_dict(shapes, seed))


def test_genrl_agent_constructs_with_the_override():
    from genrl_amd import config
    assert config.norm_free_convs() == dict(encoder=dict(norm='none'), decoder=dict(norm='none'))
    over = {k: dict(v) for k, v in config.tiny_overrides().items()}
    for k, v in config.norm_free_convs().items():
        over[k].update(v)
    ag = config.make_agent(config.default_cfg(2, 16, device='cpu', **over), act_dim=10)
    assert not C.norm_params(ag.wm.encoder) and not C.norm_params(ag.wm.heads['decoder'])
    plain = config.make_agent(config.default_cfg(2, 16, device='cpu', **config.tiny_overrides()), act_dim=10)
    assert len(C.norm_params(plain.wm.encoder)) == 4 and len(C.norm_params(plain.wm.heads['decoder'])) == 3


@pytest.mark.parametrize('kind', ['dreamer', 'p2e'])
@pytest.mark.parametrize('block', ['encoder', 'decoder'])
def test_any_other_norm_name_raises(block, kind):
    with pytest.raises(NotImplementedError, match='batch'):
        build(kind, over={block: dict(norm='batch')})
    with pytest.raises(NotImplementedError, match='batch'):
        build(kind, over={block: dict(norm='batch')}, defaults='dreamer_v2')


def test_modules_on_their_own():
    from genrl_amd.agent import dreamer_utils as common
    shapes = {'observation': (3, 64, 64)}
    for norm, n in (('none', 0), ('layer', 4)):
        enc = common.Encoder(shapes, cnn_keys='observation', mlp_keys='$^', norm=norm, cnn_depth=4)
        assert len(C.norm_params(enc)) == n and all(enc._conv_model[3 * i].bias is not None for i in range(4))
    dec = common.Decoder(shapes, cnn_keys='observation', mlp_keys='$^', norm='none', cnn_depth=4, cnn_kernels=(5, 5, 6, 6), embed_dim=48)
    assert not C.norm_params(dec) and isinstance(dec._conv_model[10], common.NormLayer)
    for cls in (common.Encoder, common.Decoder):
        with pytest.raises(NotImplementedError, match='instance'):
            cls(shapes, cnn_keys='observation', mlp_keys='$^', norm='instance', cnn_depth=4)


@pytest.mark.parametrize('kind', ['dreamer', 'p2e'])
@pytest.mark.parametrize('defaults', ['dreamer_v3', 'dreamer_v2'])
def test_agents_built_without_the_override_are_unchanged(defaults, kind):
    import elu_cases as E
    ag = build(kind, defaults=defaults)
    assert len(C.norm_params(ag.wm.encoder)) == 4 and len(C.norm_params(ag.wm.heads['decoder'])) == 3
    assert ag.wm.encoder._norm == 'layer' and ag.wm.heads['decoder']._norm == 'layer'
    plain = E.shapes_of(E.load(), 'v3e' if defaults == 'dreamer_v3' else 'v2e')
    assert {k: tuple(v.shape) for k, v in ag.state_dict().items() if not k.startswith('disagreement.')} == plain


# ---------------------------------------------------------------------------------------------- plain-torch restatement
def _act(case):
    return F.elu if 'encoder' in C.CASES[case][3] else F.silu


def restated_embed(sd, frames, act):
    """the norm-free conv encoder (ref :618-621 with NormLayer('none')): frames / 255 - 0.5, four stride-2 convolutions with bias, each
    followed by the activation, flattened NCHW"""
    x = frames.float() / 255.0 - 0.5
    for i in (0, 3, 6, 9):
        x = act(F.conv2d(x, sd[f'wm.encoder._conv_model.{i}.weight'], sd[f'wm.encoder._conv_model.{i}.bias'], stride=2))
    return x.reshape(x.shape[0], -1)


def restated_decoder_mean(sd, feat, act):
    """the norm-free conv decoder (ref :695-699): Linear, then three stride-2 transposed convolutions with bias + activation and a last one alone"""
    p = 'wm.heads.decoder.'
    x = F.linear(feat, sd[p + '_conv_in.0.weight'], sd[p + '_conv_in.0.bias'])
    x = x.reshape(-1, x.shape[-1], 1, 1)
    for i in (0, 3, 6):
        x = act(F.conv_transpose2d(x, sd[f'{p}_conv_model.{i}.weight'], sd[f'{p}_conv_model.{i}.bias'], stride=2))
    return F.conv_transpose2d(x, sd[p + '_conv_model.9.weight'], sd[p + '_conv_model.9.bias'], stride=2)


@pytest.mark.parametrize('case', sorted(C.CASES))
def test_plain_torch_restatement_reproduces_the_stored_samples(case):
    """within 1e-5 relative of the largest stored magnitude, the bound of test_gauss_golden.py"""
    g = C.load()
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    sd = detgen.det_state_dict(C.shapes_of(g, case), seed)
    free = C.CASES[case][2]
    act = _act(case)
    if 'encoder' in free:
        frames = torch.from_numpy(detgen.det_batch(B, T, A=A, seed=seed)['observation'][:, :3])
        want = g[f'{case}.embed']
        got = restated_embed(sd, frames.reshape(-1, 3, 64, 64), act).reshape(want.shape).numpy()
        assert float(np.abs(want).max()) > 1e-3          # (a guard against an all-zero sample, not a bound)
        assert float(np.abs(got - want).max()) <= 1e-5 * float(np.abs(want).max()), case
    assert 'decoder' in free
    feat = torch.from_numpy(g[f'{case}.feat'])
    want = g[f'{case}.recon']
    got = restated_decoder_mean(sd, feat.reshape(-1, feat.shape[-1]), act)[..., ::4, ::4].reshape(want.shape).numpy()
    assert want.shape == (1, 2, 3, 16, 16) and float(np.abs(want).max()) > 0.01
    assert float(np.abs(got - want).max()) <= 1e-5 * float(np.abs(want).max()), case
    # ... and it is the activation that was asked for
    other = F.silu if act is F.elu else F.elu
    wrong = restated_decoder_mean(sd, feat.reshape(-1, feat.shape[-1]), other)[..., ::4, ::4].reshape(want.shape).numpy()
    assert float(np.abs(wrong - want).max()) > 1e-3 * float(np.abs(want).max())


# ---------------------------------------------------------------------------------------------- the C boundary and the ops
def test_the_header_declares_the_entries_and_the_source_defines_them():
    from genrl_amd._lib import parse_header
    decl = parse_header()
    assert {'genrl_chan_act_fwd_h2u', 'genrl_chan_act_bwd_h2u', 'genrl_chan_act_bwd_ws_floats'} <= set(decl)
    assert [n for _, n in decl['genrl_chan_act_fwd_h2u'][1]][-1] == 'stream' and [n for _, n in decl['genrl_chan_act_bwd_h2u'][1]][-1] == 'stream'
    src = open(os.path.join(ROOT, 'genrl_amd', 'csrc', 'rowops.hip')).read()
    for name in ('genrl_chan_act_fwd_h2u', 'genrl_chan_act_bwd_h2u', 'genrl_chan_act_bwd_ws_floats'):
        assert re.search(r'^(int|long) %s\(' % name, src, re.M), name
    for kernel in ('chan_act_fwd_grp_kernel', 'chan_act_bwd_grp_kernel', 'chan_act_fwd_scalar_kernel', 'chan_act_bwd_scalar_kernel'):
        assert re.search(r'__global__[^;{]*\b%s\(' % kernel, src), kernel
    assert 'atomicAdd' not in src[src.index('chan_act_fwd_grp_kernel'):src.index('// out[j] (+)= sum_c part[c][j]')]


def test_ops_refuse_cpu_tensors_and_validate_their_arguments():
    from genrl_amd import ops, ops_conv_planes
    from genrl_amd._lib import GenrlHipError
    x, W, b = torch.zeros(1, 8, 8, 4), torch.zeros(8, 4, 4, 4), torch.zeros(8)
    xt, Wt = torch.zeros(1, 3, 3, 8), torch.zeros(8, 4, 4, 4)
    for act in ('SiLU', 'ELU'):
        with pytest.raises(GenrlHipError):
            ops.conv2d_s2(x, W, b, ln=None, act=act)
        with pytest.raises(GenrlHipError):
            ops.convT2d_s2(xt, Wt, torch.zeros(4), ln=None, act=act)
        with pytest.raises(GenrlHipError):
            ops_conv_planes.conv2d_s2(x, W, b, ln=None, act=act)
        with pytest.raises(GenrlHipError):
            ops_conv_planes.convT2d_s2(xt, Wt, torch.zeros(4), ln=None, act=act)
    with pytest.raises(NotImplementedError, match='GELU'):
        ops.conv2d_s2(x, W, b, ln=None, act='GELU')
    with pytest.raises(NotImplementedError):
        ops_conv_planes.conv2d_s2(x, W, b, ln=None, act=0)
    with pytest.raises(AssertionError):            # a fused channel-LayerNorm names its activation in ln[3]
        ops.conv2d_s2(x, W, b, ln=(torch.ones(8), torch.zeros(8), 1e-3), act='ELU')
    assert ops._nf_code(None, None) == 0 and ops._nf_code(None, 'SiLU') == 1 and ops._nf_code(None, 'ELU') == 2


def test_fixture_seed_conditions_and_size():
    g = C.load()
    assert float(g['race_margin']) >= 1e-3 and float(g['race_margins'].min()) == float(g['race_margin'])
    tried = g['seeds_tried']
    assert int(tried[-1, 0]) == int(g['seed']) and (tried[:-1, 1] < 1e-3).all() and tried[-1, 1] >= 1e-3
    assert {int(g[f'{case}.meta'][6]) for case in C.CASES} == {int(g['seed'])}
    for case in C.CASES:
        mets = C.metrics_of(g, case)
        assert all(np.isfinite(v) for v in mets.values()) and len(mets) > 10
        for ph in ('model', 'actor', 'critic'):
            assert len(C.unpack(g, f'{case}.grad.{ph}')) > 0
        assert set(C.unpack(g, f'{case}.delta')) <= set(C.shapes_of(g, case))
        assert not any('.norm.' in k for k in C.shapes_of(g, case) if '.decoder._conv_model' in k)
    assert any('.norm.' in k for k in C.shapes_of(g, 'v3d') if '.encoder._conv_model' in k)
    # four computations: the activation moves the world model, the norm-free encoder moves the embedding
    assert abs(C.metrics_of(g, 'v2n')['model_loss'] - C.metrics_of(g, 'v2ne')['model_loss']) > 1e-3
    assert g['v3n.embed'].shape != g['v3d.embed'].shape
    assert g['act.eval.action'].shape == g['act.sample.action'].shape == (6,)
    assert os.path.getsize(os.path.join(C.G, 'convfree_tiny.npz')) <= os.path.getsize(os.path.join(C.G, 'v2_tiny.npz'))
