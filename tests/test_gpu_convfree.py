"""Norm-free conv encoder / decoder (`encoder.norm: none`, `decoder.norm: none`) on the MI355X.

Two-layer chains of norm-free layers -- conv + bias + SiLU / ELU, transposed conv likewise -- on the plane route and on the fp32-operand
route against float64 conv2d / conv_transpose2d + activation: outputs rtol 3e-4 / atol 3e-4, every gradient 5e-5 of its largest element
(test_gpu_conv_planes.py's _check), at that file's chain shapes plus one chain that starts from u8 frames.  The weights are scaled so that
both layers' float64 pre-activations have unit spread, and each layer's output maximum is asserted inside [0.5, 8]: the absolute term of
the bound means what it means behind a LayerNorm.  The float64 reference of a shape is computed once and shared by the routes.

DreamerAgent with norm-free conv stacks against the reference's vectors (tests/golden/convfree_tiny.npz) under test_gpu_elu.py's bounds:
latent indices exact, imagined actions and metrics rtol 2e-4 / atol 1e-6 with equal key sets, gradients rtol 1e-3 / atol 1e-5 max|reference| (on the rows the fixture keeps: convfree_cases.grad_rows),
one real optimiser step within 2 lr per element and 5 % in L1 per group, act() in both modes, a finite report().  The route is asserted
live: the norm-free layers went through genrl_chan_act_{fwd,bwd}_h2u and no conv layer of a norm-free stack through a channel-LayerNorm."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detgen
import convfree_cases as C
from test_gpu_elu import count_calls, run_update

pytestmark = pytest.mark.gpu

ACT = {'SiLU': F.silu, 'ELU': F.elu}
CHAN = ('genrl_chan_act_fwd_h2u', 'genrl_chan_act_bwd_h2u')
CHAN_LN = ('genrl_ln_act_fwd_h2u', 'genrl_ln_act_bwd_h2u')          # the channel-LayerNorm's own entries (uniform planes)


def g(s):
    return torch.Generator().manual_seed(s)


def count_entries(monkeypatch, names):
    from genrl_amd._lib import lib
    n = dict.fromkeys(names, 0)
    for name in names:
        orig = getattr(lib(), name)
        monkeypatch.setattr(lib(), name, lambda *a, _o=orig, _n=name: (n.__setitem__(_n, n[_n] + 1), _o(*a))[1])
    return n


# ---------------------------------------------------------------------------------------------- chains against float64
ENC = [(8, 31, 48, 96, 192), (64, 14, 96, 192, 384), (3, 31, 48, 96, 192), (16, 31, 56, 48, 64), 'u8']
DEC = [(64, 1, 1536, 192, 96, 5, 5), (64, 5, 192, 96, 48, 5, 6), (5, 5, 192, 96, 48, 5, 6), (128, 5, 64, 48, 56, 5, 6)]
_refs = {}


def _unit(W, pre):
    """W scaled so that the float64 pre-activation `pre` it produces has unit spread"""
    return (W.double() / pre.std()).float()


def chain_case(kind, shape, act):
    """-> (x, [W1, b1, W2, b2] fp32 leaves' values, float64 output, output weights, float64 gradients of x (None for u8 frames) and the four
    parameters): once per (kind, shape, activation), shared by the routes, never written"""
    key = (kind, shape, act)
    if key in _refs:
        return _refs[key]
    fn = ACT[act]
    if kind == 'enc':
        if shape == 'u8':
            N, Hi, C0, C1, C2 = 4, 64, 3, 48, 96
            x = torch.randint(0, 256, (N, 3, Hi, Hi), generator=g(1), dtype=torch.uint8)
            xin = x.double() / 255.0 - 0.5
        else:
            N, Hi, C0, C1, C2 = shape
            x = torch.randn(N, Hi, Hi, C0, generator=g(1))
            xin = x.double().permute(0, 3, 1, 2)
        W1 = torch.randn(C1, C0, 4, 4, generator=g(2)); W2 = torch.randn(C2, C1, 4, 4, generator=g(4))
        conv = lambda t, W, b: F.conv2d(t, W, b, stride=2)
    else:
        N, Hi, C0, C1, C2, k1, k2 = shape
        x = torch.randn(N, Hi, Hi, C0, generator=g(1))
        xin = x.double().permute(0, 3, 1, 2)
        W1 = torch.randn(C0, C1, k1, k1, generator=g(2)); W2 = torch.randn(C1, C2, k2, k2, generator=g(4))
        conv = lambda t, W, b: F.conv_transpose2d(t, W, b, stride=2)
    b1 = 0.1 * torch.randn(C1, generator=g(3)); b2 = 0.1 * torch.randn(C2, generator=g(5))
    with torch.no_grad():
        W1 = _unit(W1, conv(xin, W1.double(), None))
        y1 = fn(conv(xin, W1.double(), b1.double()))
        W2 = _unit(W2, conv(y1, W2.double(), None))
    leaves = [t.clone().double().requires_grad_(True) for t in (W1, b1, W2, b2)]
    xr = xin.clone().requires_grad_(shape != 'u8')
    y1 = fn(conv(xr, leaves[0], leaves[1]))
    out = fn(conv(y1, leaves[2], leaves[3])).permute(0, 2, 3, 1)
    for name, t in (('inner', y1), ('out', out)):
        assert 0.5 <= float(t.detach().abs().max()) <= 8.0, (key, name, float(t.detach().abs().max()))
    w = torch.randn(out.shape, generator=g(99))
    (out * w.double()).sum().backward()
    gx = None if shape == 'u8' else xr.grad.permute(0, 2, 3, 1)
    _refs[key] = (x, [W1, b1, W2, b2], out.detach(), w, [gx] + [t.grad for t in leaves])
    return _refs[key]


def check_chain(kind, shape, act, route, inner_fp32, monkeypatch):
    from genrl_amd import ops, ops_conv_planes as cp
    monkeypatch.setattr(cp, 'ENABLED', route == 'planes')
    n = count_entries(monkeypatch, CHAN + CHAN_LN + ('genrl_ln_act_fwd', 'genrl_ln_act_bwd'))
    x, params, ref, w, grads = chain_case(kind, shape, act)
    xd = x.cuda() if shape == 'u8' else x.clone().cuda().requires_grad_(True)
    dev = [t.clone().cuda().requires_grad_(True) for t in params]
    xin = xd if shape == 'u8' else xd * 1.0
    on_planes = cp.active(xin)
    assert on_planes == (route == 'planes')
    if on_planes and kind == 'enc' and shape != 'u8':
        xin._planes = cp._uniform_split(xin.detach().reshape(-1, xin.shape[-1]))            # (as a previous layer would have left them)
    mod = cp if on_planes else ops
    layer = mod.conv2d_s2 if kind == 'enc' else mod.convT2d_s2
    y = layer(xin, dev[0], dev[1], ln=None, act=act, fp32_out=inner_fp32)
    if on_planes:
        assert y._lazy is None and (y._planes is not None) == (y.shape[-1] % 4 == 0 and y.numel() // y.shape[-1] >= 64)
        assert y._planes is None or y._planes.uniform
    out = layer(y, dev[2], dev[3], ln=None, act=act)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.float().numpy(), rtol=3e-4, atol=3e-4, err_msg='out')
    (out * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(grads, [xd] + dev)):
        if a is None:
            continue
        scale = max(1e-6, a.abs().max().item())
        err = (b.grad.cpu().double() - a).abs().max().item() / scale
        assert err <= 5e-5, (i, err)
    assert n[CHAN[0]] == 2 and n[CHAN[1]] == 2 and sum(v for k, v in n.items() if k not in CHAN) == 0, n


@pytest.mark.parametrize('inner_fp32', [True, False])
@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('act', ['SiLU', 'ELU'])
@pytest.mark.parametrize('shape', ENC, ids=str)
def test_norm_free_encoder_chain(shape, act, route, inner_fp32, monkeypatch):
    check_chain('enc', shape, act, route, inner_fp32, monkeypatch)


@pytest.mark.parametrize('inner_fp32', [True, False])
@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('act', ['SiLU', 'ELU'])
@pytest.mark.parametrize('shape', DEC, ids=str)
def test_norm_free_decoder_chain(shape, act, route, inner_fp32, monkeypatch):
    check_chain('dec', shape, act, route, inner_fp32, monkeypatch)


def test_bias_gradient_goes_straight_into_the_flat_buffer(monkeypatch):
    """under ops.direct_grads a norm-free layer adds its bias gradient into the parameter's gradient buffer and returns None for it: the
    buffer then holds prior + db, bit for bit the db of the autograd route"""
    from genrl_amd import ops, ops_conv_planes as cp
    x, params, ref, w, grads = chain_case('enc', ENC[0], 'ELU')
    res = {}
    prior = torch.randn(params[1].shape, generator=g(5)).cuda()
    for direct in (False, True):
        monkeypatch.setattr(ops, 'direct_grads', direct)
        W1 = params[0].clone().cuda().requires_grad_(True)
        b1 = torch.nn.Parameter(params[1].clone().cuda())
        b1.grad = prior.clone()
        xin = x.clone().cuda()
        xin._planes = cp._uniform_split(xin.reshape(-1, xin.shape[-1]))
        y = cp.conv2d_s2(xin, W1, b1, ln=None, act='ELU')
        (y * torch.randn(y.shape, generator=g(6)).cuda()).sum().backward()
        torch.cuda.synchronize()
        res[direct] = b1.grad.clone()
    # autograd adds the returned db onto the prior (one rounding); the direct route's `accumulate` does the same addition in the reduction
    assert bool(torch.isfinite(res[True]).all()) and float((res[True] - prior).abs().max()) > 0
    assert torch.equal(res[False], res[True])


# ---------------------------------------------------------------------------------------------- agents against the reference's vectors
def setup(g_, case, lr_zero=True, kind='dreamer'):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g_[f'{case}.meta']]
    defaults, vec_obs, free, elu, _ = C.CASES[case]
    over = C.overrides(case, config.dreamer_tiny_overrides())
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    if kind == 'p2e':
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
        shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
        shapes = C.shapes_of(g_, case)
    for name, mod in (('encoder', ag.wm.encoder), ('decoder', ag.wm.heads['decoder'])):
        assert (not C.norm_params(mod)) == (name in free), (case, name)
    sd = detgen.det_state_dict(shapes, seed)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    batch = {k: v for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    batch.update(C.vec_batch(case, B, T, seed))
    batch = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    sites = lambda: {'rssm.prior': [noise['wm']['prior_q'][t] for t in range(T)], 'rssm.post': [noise['wm']['post_q'][t] for t in range(T)],
                     'imag.act_eps': noise['imag']['act_eps'], 'imag.step_q': noise['imag']['step_q']}
    return ag, sd, batch, sites


def assert_route_live(case, calls, n, route):
    """the norm-free layers ran on the new entries: per update 4 encoder + 3 decoder layers (the decoder's last layer has no activation);
    no conv layer of a norm-free stack met a channel-LayerNorm, on either route's nodes"""
    free = C.CASES[case][2]
    layers = (4 if 'encoder' in free else 0) + (3 if 'decoder' in free else 0)
    assert n[CHAN[0]] >= layers and n[CHAN[1]] >= layers, (case, n)
    ln_convs = sum(v for k, v in calls.items() if isinstance(k, tuple) and k[0] in ('conv_fp32', 'conv_planes'))
    if layers == 7:
        assert ln_convs == 0 and n[CHAN_LN[0]] == 0 and n[CHAN_LN[1]] == 0, (case, calls, n)
    else:
        assert ln_convs >= 4 and not any(k[0] == ('conv_planes' if route == 'fp32' else 'conv_fp32') for k in calls if isinstance(k, tuple)), (case, calls)


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', sorted(C.CASES))
def test_update_vs_reference(case, route, monkeypatch):
    from genrl_amd import ops_conv_planes
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    monkeypatch.setattr(ops_conv_planes, 'ENABLED', route == 'planes')
    calls = count_calls(monkeypatch)
    n = count_entries(monkeypatch, CHAN + CHAN_LN)
    g_ = C.load()
    ag, sd, batch, sites = setup(g_, case)
    mets, cap, grads = run_update(ag, batch, sites)
    print(case, route, calls, n)
    assert_route_live(case, calls, n, route)
    assert (cap['post_idx'] == g_[f'{case}.post_idx']).all() and (cap['imag_idx'] == g_[f'{case}.imag_idx']).all()
    np.testing.assert_allclose(cap['imag_action'], g_[f'{case}.imag_action'], rtol=2e-4, atol=1e-6)
    ref = C.metrics_of(g_, case)
    assert set(mets) == set(ref)
    for key, val in ref.items():
        np.testing.assert_allclose(mets[key], val, rtol=2e-4, atol=1e-6, err_msg=key)
    k = 0
    for ph in ('model', 'actor', 'critic'):
        for name, val in C.unpack(g_, f'{case}.grad.{ph}').items():
            np.testing.assert_allclose(C.grad_rows(grads[ph][name].numpy()).reshape(-1), val, rtol=1e-3, atol=1e-5 * np.abs(val).max(), err_msg=f'{ph}.{name}')
            k += 1
    assert k == sum(len(grads[ph]) for ph in grads) and k > 0
    conv_b = [name for name in grads['model'] if '_conv_model' in name and name.endswith('.bias') and '.norm.' not in name]
    assert len(conv_b) == 8 and all(float(grads['model'][name].abs().max()) > 0.0 for name in conv_b)


@pytest.mark.parametrize('case', sorted(C.CASES))
def test_one_optimizer_step_vs_reference(case):
    """test_gpu_elu.py's rule: a real step at the defaults' learning rates, twice from the same weights: bit-identical; against the
    reference's deltas at most 2 lr per element and 5 % in L1 per group, on the rows the fixture keeps"""
    g_ = C.load()
    after = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g_, case, lr_zero=False)
        run_update(ag, batch, sites)
        after.append({k: v.detach().cpu().clone() for k, v in ag.state_dict().items()})
    assert all(torch.equal(after[0][k], after[1][k]) for k in after[0])
    after = after[0]
    lr = {k: float(g_[f'{case}.opt.{k}'][0]) for k in ('model_opt', 'actor_opt', 'critic_opt')}
    assert {k: float(ag.cfg[k]['lr']) for k in lr} == lr
    delta = C.unpack(g_, f'{case}.delta')
    groups = {'wm': ('wm.', 'model_opt'), 'actor': ('_acting_behavior.actor.', 'actor_opt'), 'critic': ('_acting_behavior.critic.', 'critic_opt')}
    for gname, (prefix, opt) in groups.items():
        num = den = 0.0
        names = [n for n in sd if n.startswith(prefix)]
        assert names and set(names) <= set(delta)
        for n in names:
            moved = (after[n] - sd[n]).double()
            assert float(moved.abs().max()) <= 2.0 * lr[opt], (gname, n, float(moved.abs().max()))
            dp = C.grad_rows(moved.numpy()).reshape(-1); do = delta[n].astype(np.float64) * lr[opt]
            worst = float(np.abs(dp - do).max())
            assert worst <= 2.0 * lr[opt] * 1.05 + 1e-7, (gname, n, worst)
            num += float(np.abs(dp - do).sum()); den += float(np.abs(do).sum())
        print(f'{case} {gname}: L1 of the delta difference {num / den:.3g} of the delta')
        assert den > 0 and num / den <= 0.05, (gname, num / den)


def test_act_in_both_modes_vs_reference():
    from genrl_amd import noise as gnoise
    g_ = C.load()
    ag, sd, batch, sites = setup(g_, 'v2ne')
    B, T, A, S, K, H, seed = [int(x) for x in g_['v2ne.meta']]
    obs = {'observation': batch['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    for mode, ev in (('eval', True), ('sample', False)):
        q = lambda what: detgen.det_noise(f'act.{mode}.{what}', (S, K), 'exp', seed)
        inj = {'rssm.prior': [q('prior_q')], 'rssm.post': [q('post_q')]}
        if not ev:
            inj['actor'] = [detgen.det_noise(f'act.{mode}.act_eps', (1, A), 'normal', seed)]
        with gnoise.inject(inj):
            action, (latent, act_t) = ag.act(obs, None, 0, ev, None)
        assert action.shape == (A,) and action.dtype == np.float32
        assert (latent['stoch'].argmax(-1).cpu().numpy() == g_[f'act.{mode}.latent_idx']).all()
        np.testing.assert_allclose(action, g_[f'act.{mode}.action'], rtol=2e-4, atol=1e-6, err_msg=mode)
        assert torch.equal(act_t[0].cpu(), torch.from_numpy(action))


@pytest.mark.parametrize('kind', ['dreamer', 'p2e'])
def test_report_of_the_published_dreamer_v2_network(kind, monkeypatch):
    from genrl_amd import noise as gnoise
    g_ = C.load()
    B, T = [int(x) for x in g_['v2ne.meta'][:2]]
    ag, sd, batch, sites = setup(g_, 'v2ne', kind=kind)
    n = count_entries(monkeypatch, CHAN + CHAN_LN)
    with gnoise.static(seed=3):
        videos = ag.report(batch)
    torch.cuda.synchronize()
    assert set(videos) == {'openl_observation'}, videos.keys()
    v = videos['openl_observation']
    assert tuple(v.shape) == (B, T, 3, 3 * 64, 64) and bool(torch.isfinite(v).all()) and 0.0 <= float(v.min()) and float(v.max()) <= 1.0
    assert n[CHAN[0]] >= 7 and n[CHAN_LN[0]] == 0, n
