"""The tanh_normal actor head on the MI355X (`actor: {dist: tanh_normal}` on both default sets) against the reference's vectors
(tests/golden/tanh_tiny.npz, made by tests/golden/make_tanh_golden.py), under the bounds test_gpu_v2.py states: latent indices exact, actions
and metrics rtol 2e-4 / atol 1e-6, gradients rtol 1e-3 / atol 1e-5 max|reference| (a gradient of more than 4096 elements is stored on every
fourth index of its first dimension).  Both cases run on the fp32-operand route and with plane operands forced on."""
import os

import numpy as np
import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = {'v3t': ('dreamer_v3', dict(actor=dict(dist='tanh_normal'), actor_ent=3e-4, reward_ema=True)),
         'v2t': ('dreamer_v2', dict(actor=dict(dist='tanh_normal', init_std=1.0)))}
KS = 100
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'tanh_tiny.npz')))
    return _cache['g']


def setup(g, case, lr_zero=True, p2e=False, **more):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, extra = CASES[case]
    over = dict(config.dreamer_tiny_overrides())
    for k, v in dict(extra, **more).items():
        over[k] = dict(over.get(k, {}), **v) if isinstance(v, dict) else v
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    if p2e:
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
        shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
        pre = f'{case}.shape.'
        shapes = {k[len(pre):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith(pre)}
    sd = detgen.det_state_dict(shapes, seed)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    batch = {k: torch.from_numpy(v).cuda() for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    ent_eps = detgen.det_noise('actor.ent_eps', (KS * (H - 1), B * T, A), 'normal', seed)
    sites = lambda: {'rssm.prior': [noise['wm']['prior_q'][t] for t in range(T)], 'rssm.post': [noise['wm']['post_q'][t] for t in range(T)],
                     'imag.act_eps': noise['imag']['act_eps'], 'imag.step_q': noise['imag']['step_q'], 'actor.ent_eps': [ent_eps]}
    return ag, sd, batch, sites


def run_update(ag, batch, sites):
    """-> metrics (floats), captured tensors, gradients per optimiser name"""
    from genrl_amd import noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    grads, cap = {}, {}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    ac = ag._acting_behavior
    orig_wm, orig_tg, orig_al, orig_cl = ag.wm.update, ac.target, ac.actor_loss, ac.critic_loss

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        cap['imag_action'] = seq['action'].detach().cpu().numpy()
        target, mets, baseline = orig_tg(seq)
        cap['imag_target'] = target.detach().cpu().numpy()
        cap['imag_baseline'] = baseline.detach().cpu().numpy()
        return target, mets, baseline

    def al_hook(seq, target, baseline):
        from genrl_amd import ops
        head = ac.actor._out._head
        with torch.no_grad():
            raw = ac._policy_raw(seq)
            mean, std = ops.tanh_normal_mean_std(raw, *head.params())
            cap['raw'], cap['mean'], cap['std'] = raw.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy()
        orig_eg = head.entropy_grad

        def eg_hook(raw_, *a, **k):            # the actor loss's own (single) entropy evaluation
            ent = orig_eg(raw_, *a, **k)
            cap['ent'] = ent.detach()[..., 0].cpu().numpy()
            return ent
        head.entropy_grad = eg_hook
        try:
            return orig_al(seq, target, baseline)
        finally:
            del head.entropy_grad

    def cl_hook(seq, target):
        cap['critic_target_in'] = target.detach().cpu().numpy()
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.actor_loss, ac.critic_loss = wm_hook, tg_hook, al_hook, cl_hook
    try:
        with gnoise.inject(sites()):
            _, mets = ag.update(batch, 0)
    finally:
        common.Optimizer.grad_hook = None
        ag.wm.update, ac.target, ac.actor_loss, ac.critic_loss = orig_wm, orig_tg, orig_al, orig_cl
    torch.cuda.synchronize()
    return {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}, cap, grads


def check_grads(what, got, ref):
    a, b = np.asarray(got), np.asarray(ref)
    if a.size > 4096:
        a = a[::4]
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max(), err_msg=what)


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_update_vs_reference(case, route, monkeypatch):
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    g = load()
    ag, sd, batch, sites = setup(g, case)
    head = ag._acting_behavior.actor._out._head
    assert not head.fused and head.K == KS
    mets, cap, grads = run_update(ag, batch, sites)
    assert (cap['post_idx'] == g[f'{case}.post_idx']).all() and (cap['imag_idx'] == g[f'{case}.imag_idx']).all()
    assert float(np.abs(cap['imag_action'][0]).max()) == 0.0 and float(np.abs(cap['imag_action']).max()) < 1.0
    np.testing.assert_allclose(cap['imag_action'], g[f'{case}.imag_action'], rtol=2e-4, atol=1e-6, err_msg='imagined actions')
    for key in ('raw', 'mean', 'std', 'ent'):
        np.testing.assert_allclose(cap[key], g[f'{case}.{key}'], rtol=2e-4, atol=1e-5, err_msg=key)
    for key in ('imag_target', 'imag_baseline', 'critic_target_in'):
        np.testing.assert_allclose(cap[key], g[f'{case}.{key}'], rtol=2e-4, atol=1e-5, err_msg=key)
    assert set(mets) == set(g[f'{case}.metric_keys'].tolist())
    pre = f'{case}.metrics.'
    for key, val in g.items():
        if key.startswith(pre):
            np.testing.assert_allclose(mets[key[len(pre):]], float(val), rtol=2e-4, atol=1e-6, err_msg=key)
    n = 0
    pre = f'{case}.grad.'
    for key, val in g.items():
        if key.startswith(pre):
            ph, name = key[len(pre):].split('.', 1)
            check_grads(key, grads[ph][name].numpy(), val); n += 1
    assert n == len(grads['actor']) + len(grads['critic']) and n > 0
    for leaf in ('_out', '_std'):
        assert float(grads['actor'][f'_acting_behavior.actor._out.{leaf}.weight'].abs().max()) > 0.0


def test_act_in_both_modes_vs_reference():
    from genrl_amd import noise as gnoise
    g = load()
    ag, sd, batch, sites = setup(g, 'v3t')
    B, T, A, S, K, H, seed = [int(x) for x in g['v3t.meta']]
    obs = {'observation': batch['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    for mode, ev in (('eval', True), ('sample', False)):
        q = lambda what: detgen.det_noise(f'act.{mode}.{what}', (S, K), 'exp', seed)
        eps = detgen.det_noise(f'act.{mode}.act_eps', (KS, 1, A) if ev else (1, A), 'normal', seed)
        with gnoise.inject({'rssm.prior': [q('prior_q')], 'rssm.post': [q('post_q')], 'actor.mean_eps' if ev else 'actor': [eps]}):
            action, (latent, act_t) = ag.act(obs, None, 0, ev, None)
        assert action.shape == (A,) and action.dtype == np.float32 and float(np.abs(action).max()) < 1.0
        assert (latent['stoch'].argmax(-1).cpu().numpy() == g[f'act.{mode}.latent_idx']).all()
        np.testing.assert_allclose(action, g[f'act.{mode}.action'], rtol=2e-4, atol=1e-6, err_msg=mode)
        assert torch.equal(act_t[0].cpu(), torch.from_numpy(action))
    with pytest.raises(NotImplementedError):
        ag._acting_behavior.actor(ag.wm.rssm.get_stoch(latent), latent['deter']).mode()


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_optimizer_step_twice_is_bit_identical(case):
    """a real step (the fixture's learning rates) under noise.static, from the same weights: every parameter and buffer agrees bit for bit,
    and the actor moved by at most two learning rates (Adam's first step is lr sign(g) up to eps)"""
    from genrl_amd import noise as gnoise
    g = load()
    after = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, case, lr_zero=False)
        with gnoise.static(seed=3):
            ag.update(batch, 0)
        torch.cuda.synchronize()
        after.append({k: v.detach().cpu().clone() for k, v in ag.state_dict().items()})
    assert all(torch.equal(after[0][k], after[1][k]) for k in after[0])
    lr = float(ag.cfg.actor_opt['lr'])
    names = [n for n in sd if n.startswith('_acting_behavior.actor.')]
    assert any(n.endswith('_out._std.weight') for n in names)
    for n in names:
        d = (after[0][n] - sd[n]).abs()
        assert 0.0 < float(d.max()) <= 2.0 * lr, (n, float(d.max()), lr)


def test_p2e_update_runs_and_is_reproducible():
    g = load()
    outs = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, 'v2t', p2e=True)
        mets, cap, grads = run_update(ag, batch, sites)
        assert all(np.isfinite(v) for v in mets.values()), mets
        assert {'disagreement_loss', 'actor_loss', 'actor_ent', 'critic_loss'} <= set(mets)
        outs.append((mets, cap, grads))
    (m0, c0, g0), (m1, c1, g1) = outs
    assert m0 == m1                                                              # bit-identical metrics ...
    assert all(np.array_equal(c0[k], c1[k]) for k in c0)
    assert all(torch.equal(g0[ph][n], g1[ph][n]) for ph in g0 for n in g0[ph])      # ... and gradients on the same noise
    assert float(np.abs(c0['imag_action'][1:]).max()) < 1.0


def test_entropy_gradient_reaches_the_std_head():
    """the entropy alone, from the actor's own head product: its gradient reaches `_out._std` (through 1 / std and the samples) and `_out._out`
    (through the samples' Jacobian), which the Normal heads' entropy does not"""
    from genrl_amd.agent import dreamer_utils as common
    g = load()
    ag, sd, batch, sites = setup(g, 'v3t')
    actor = ag._acting_behavior.actor
    H, N = 3, 8
    x = torch.randn(H * N, actor._units, device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    with common.RequiresGrad(actor):
        raw = actor._out.raw(x).reshape(H, N, -1)
        ent = actor._out._head.entropy_grad(raw)
        assert ent.shape == (H, N, 1)
        d_std, d_out = torch.autograd.grad(ent.sum(), [actor._out._std.weight, actor._out._out.weight])
    assert float(d_std.abs().max()) > 0.0 and float(d_out.abs().max()) > 0.0
    assert bool(torch.isfinite(d_std).all()) and bool(torch.isfinite(d_out).all())


@pytest.mark.parametrize('case,actor_ent', [('v3t', 0.0), ('v3t', 3e-4), ('v2t', 0.0), ('v2t', 1e-3)])
def test_exactly_one_entropy_draw_per_update(case, actor_ent, monkeypatch):
    from genrl_amd import noise as gnoise
    g = load()
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    ag, sd, batch, sites = setup(g, case, actor_ent=actor_ent)
    assert float(ag.cfg.actor_ent) == actor_ent
    draws, orig = [], gnoise.draw

    def counting(kind, site, shape, device):
        draws.append((kind, site, tuple(shape)))
        return orig(kind, site, shape, device)
    monkeypatch.setattr(gnoise, 'draw', counting)
    with gnoise.inject(sites()):
        _, mets = ag.update(batch, 0)
    torch.cuda.synchronize()
    mc = [d for d in draws if d[1] in ('actor.ent_eps', 'actor.mean_eps', 'imag.act_mean_eps')]
    assert mc == [('normal', 'actor.ent_eps', (KS * (H - 1), B * T, A))], mc
    assert np.isfinite(float(mets['actor_ent'])) and float(mets['actor_ent_scale']) == pytest.approx(actor_ent)


def test_eval_policy_rollout_draws_its_mean_noise_per_step(monkeypatch):
    """imagine(eval_policy=True) acts on SampleDist.mean: one (K, N, A) draw at imag.act_mean_eps per step and no action noise"""
    from genrl_amd import noise as gnoise
    g = load()
    ag, sd, batch, sites = setup(g, 'v3t')
    A, N, H = int(g['v3t.meta'][2]), 4, 3
    draws, orig = [], gnoise.draw
    monkeypatch.setattr(gnoise, 'draw', lambda kind, site, shape, device: (draws.append((kind, site, tuple(shape))), orig(kind, site, shape, device))[1])
    start = {k: v[:, None] for k, v in ag.wm.rssm.initial(N).items()}
    with torch.no_grad():
        seq = ag.wm.imagine(ag._acting_behavior.actor, start, None, H, eval_policy=True)
    torch.cuda.synchronize()
    assert [d for d in draws if d[1].startswith(('imag.act', 'actor'))] == [('normal', 'imag.act_mean_eps', (KS, N, A))] * H
    assert seq['action'].shape == (H + 1, N, A) and float(seq['action'].abs().max()) < 1.0 and float(seq['action'][1:].abs().max()) > 0.0


def test_a_normal_head_agent_in_the_same_process_keeps_the_smoke_losses():
    """nothing leaks from a tanh_normal agent into a `normal`-head one: smoke()'s three losses are the same numbers before and after a
    tanh_normal update in this process"""
    from test_gpu_gauss import _smoke_losses
    before = _smoke_losses()
    g = load()
    ag, sd, batch, sites = setup(g, 'v3t')
    run_update(ag, batch, sites)
    after = _smoke_losses()
    print('smoke losses:', after)
    assert before == after and all(np.isfinite(v) for v in after.values())
