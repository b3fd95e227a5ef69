"""DreamerAgent and Plan2Explore on the DreamerV2 defaults (config.dreamer_cfg / p2e_cfg with defaults='dreamer_v2') on the MI355X against
the reference's vectors (tests/golden/v2_tiny.npz), under the bounds test_gpu_p2e.py applies to the dreamer_v3 fixture: latent indices
exact, metrics rtol 2e-4 / atol 1e-6, intrinsic reward rtol 2e-4, gradients rtol 1e-3 / atol 1e-5 max|reference|, one real optimiser step
within 2 lr per element and 5 % in L1 per group.  A gradient of more than 4096 elements is stored on every fourth index of its first
dimension (make_v2_golden.py): compared there."""
import os

import numpy as np
import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'v2_tiny.npz')))
    return _cache['g']


def setup(g, kind, lr_zero, **over):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g['meta']]
    over = dict(config.dreamer_tiny_overrides(), **over)
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    if kind == 'p2e':
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults='dreamer_v2', **over), act_dim=A)
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults='dreamer_v2', **over), act_dim=A)
    pre = f'{kind}.shape.'
    shapes = {k[len(pre):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith(pre)}
    sd = detgen.det_state_dict(shapes, seed)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    batch = {k: torch.from_numpy(v).cuda() for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    sites = lambda: {'rssm.prior': [noise['wm']['prior_q'][t] for t in range(T)], 'rssm.post': [noise['wm']['post_q'][t] for t in range(T)],
                     'imag.act_eps': noise['imag']['act_eps'], 'imag.step_q': noise['imag']['step_q']}
    return ag, sd, batch, sites


def run_update(ag, batch, sites):
    """-> metrics (floats), captured tensors, gradients per optimiser name"""
    from genrl_amd import noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    grads, cap = {}, {}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    ac = ag._acting_behavior
    orig_wm, orig_tg = ag.wm.update, ac.target
    orig_ir = getattr(ag, 'compute_intr_reward', None)

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        cap['imag_action'] = seq['action'].detach().cpu().numpy()
        return orig_tg(seq)

    def ir_hook(seq):
        r = orig_ir(seq)
        cap['intr_reward'] = r.detach().cpu().numpy()
        return r
    ag.wm.update, ac.target = wm_hook, tg_hook
    if orig_ir is not None:
        ag.compute_intr_reward = ir_hook
    try:
        with gnoise.inject(sites()):
            _, mets = ag.update(batch, 0)
    finally:
        common.Optimizer.grad_hook = None
        ag.wm.update, ac.target = orig_wm, orig_tg
        if orig_ir is not None:
            ag.compute_intr_reward = orig_ir
    torch.cuda.synchronize()
    return {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}, cap, grads


def check_grads(what, got, ref):
    a, b = np.asarray(got), np.asarray(ref)
    if a.size > 4096:
        a = a[::4]
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max(), err_msg=what)


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('kind', ['dreamer', 'p2e'])
def test_update_vs_reference(kind, route, monkeypatch):
    from genrl_amd import ops, ops_planes
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    calls = {'planes': 0, 'fp32': 0}
    o1, o2 = ops_planes.dense_act, ops.dense_act
    monkeypatch.setattr(ops_planes, 'dense_act', lambda *a, **k: (calls.__setitem__('planes', calls['planes'] + 1), o1(*a, **k))[1])
    monkeypatch.setattr(ops, 'dense_act', lambda *a, **k: (calls.__setitem__('fp32', calls['fp32'] + 1), o2(*a, **k))[1])
    g = load()
    ag, sd, batch, sites = setup(g, kind, True)
    mets, cap, grads = run_update(ag, batch, sites)
    other = 'fp32' if route == 'planes' else 'planes'
    assert calls[route] > 100 and calls[other] == 0, calls          # (every norm-free layer went the route under test)
    assert (cap['post_idx'] == g[f'{kind}.post_idx']).all() and (cap['imag_idx'] == g[f'{kind}.imag_idx']).all()
    ref_a = g[f'{kind}.imag_action']
    np.testing.assert_allclose(cap['imag_action'], ref_a, rtol=2e-4, atol=1e-6)
    assert set(mets) == set(g[f'{kind}.metric_keys'].tolist())
    pre = f'{kind}.metrics.'
    for key, val in g.items():
        if key.startswith(pre):
            np.testing.assert_allclose(mets[key[len(pre):]], float(val), rtol=2e-4, atol=1e-6, err_msg=key)
    n = 0
    pre = f'{kind}.grad.'
    for key, val in g.items():
        if key.startswith(pre):
            ph, name = key[len(pre):].split('.', 1)
            check_grads(key, grads[ph][name].numpy(), val); n += 1
    assert n == sum(len(grads[ph]) for ph in grads if ph != ('model' if kind == 'p2e' else ''))
    if kind == 'p2e':
        r = cap['intr_reward']
        assert r.shape == g['p2e.intr_reward'].shape and float(np.abs(r[0]).max()) == 0.0
        np.testing.assert_allclose(r, g['p2e.intr_reward'], rtol=2e-4, atol=1e-6 * float(np.abs(g['p2e.intr_reward']).max()))


def test_p2e_one_optimizer_step_vs_reference():
    """as test_gpu_p2e.py::test_one_optimizer_step_vs_reference, on the v2 fixture"""
    g = load()
    ag, sd, batch, sites = setup(g, 'p2e', False)
    run_update(ag, batch, sites)
    after = {k: v.detach().cpu() for k, v in ag.state_dict().items()}
    lr = {k: float(g[f'opt.{k}'][0]) for k in ('model_opt', 'actor_opt', 'critic_opt')}
    groups = {'wm': ('wm.', 'model_opt'), 'disagreement': ('disagreement.', 'model_opt'), 'actor': ('_acting_behavior.actor.', 'actor_opt'),
              'critic': ('_acting_behavior.critic.', 'critic_opt')}
    for gname, (prefix, opt) in groups.items():
        num = den = 0.0
        names = [n for n in sd if n.startswith(prefix)]
        assert names
        for n in names:
            dp = (after[n] - sd[n]).double(); do = torch.from_numpy(g[f'delta.{n}'].astype(np.float64)) * lr[opt]
            worst = float((dp - do).abs().max())
            assert worst <= 2.0 * lr[opt] * 1.05 + 1e-7, (gname, n, worst)
            num += float((dp - do).abs().sum()); den += float(do.abs().sum())
        print(f'{gname}: L1 of the delta difference {num / den:.3g} of the delta')
        assert den > 0 and num / den <= 0.05, (gname, num / den)
    for n in after:
        if n.startswith('_acting_behavior._target_critic.'):
            assert torch.equal(after[n], after[n.replace('_target_critic', 'critic')]), n


@pytest.mark.parametrize('kind', ['dreamer', 'p2e'])
def test_act_eval_is_tanh_of_the_head_and_sampling_stays_in_range(kind):
    g = load()
    ag, sd, batch, sites = setup(g, kind, True)
    A = int(g['meta'][2])
    obs = {'observation': batch['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    action, (latent, act_t) = ag.act(obs, None, 0, True, None)
    assert action.shape == (A,) and action.dtype == np.float32
    actor = ag._acting_behavior.actor
    with torch.no_grad():
        x = actor.trunk(ag.wm.rssm.get_stoch(latent), latent['deter'])
        head = x.double() @ actor._out._out.weight.double().t() + actor._out._out.bias.double()
    np.testing.assert_allclose(action, torch.tanh(head)[0].cpu().numpy(), rtol=1e-5, atol=1e-6)
    a2, state = ag.act(obs, None, 1, False, (latent, act_t))
    assert a2.shape == (A,) and float(np.abs(a2).max()) <= 1.0 and not np.allclose(a2, action)
    a3, _ = ag.act(obs, None, 2, True, state)
    assert np.isfinite(a3).all()


def test_entropy_bonus_reaches_the_std_head():
    g = load()
    ag, sd, batch, sites = setup(g, 'dreamer', True)
    assert ag.cfg.actor_ent == 3e-4
    _, _, grads = run_update(ag, batch, sites)
    assert float(grads['actor']['_acting_behavior.actor._out._std.weight'].abs().max()) > 0.0
    # ... and through the entropy term, not only the sampled action: with the actions' gradient path cut (eval_policy rollouts carry none)
    # the reference value is the fixture's, already compared in test_update_vs_reference; here the bonus alone:
    from genrl_amd.agent import dreamer_utils as common
    ac = ag._acting_behavior
    H, N, A = 3, 8, int(g['meta'][2])
    raw = torch.randn(H, N, 2 * A, device='cuda')
    with common.RequiresGrad(ac.actor):
        seq = {'weight': torch.ones(H + 2, N, 1, device='cuda'), 'stoch': torch.zeros(H + 2, N, 4, 4, device='cuda')}
        ac._rollout_actor_raw = raw.requires_grad_(True)
        ac._critic_target = None
        loss, mets = ac.actor_loss(seq, torch.zeros(H + 1, N, 1, device='cuda'), None)
        loss.backward()
    assert float(raw.grad[..., A:].abs().min()) > 0.0 and float(raw.grad[..., :A].abs().max()) == 0.0
    assert 'normed_target_mean' not in mets and 'reward_ema_005' not in mets
