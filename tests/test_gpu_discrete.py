"""Discrete actions on the MI355X (`discrete_actions`: one-hot actor, `actor_grad` dynamics / reinforce) against the reference's vectors
(tests/golden/discrete_tiny.npz, made by tests/golden/make_discrete_golden.py), under the bounds test_gpu_v2.py states: latent indices and
actions exact, metrics rtol 2e-4 / atol 1e-6, gradients rtol 1e-3 / atol 1e-5 max|reference| (a gradient of more than 4096 elements is stored
on every fourth index of its first dimension).  Both cases run on the fp32-operand route and with plane operands forced on."""
import os

import numpy as np
import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = {'v3dyn': ('dreamer_v3', 'dynamics'), 'v2rf': ('dreamer_v2', 'reinforce')}
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'discrete_tiny.npz')))
    return _cache['g']


def setup(g, case, lr_zero=True, p2e=False, **over):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, actor_grad = CASES[case]
    over = dict(config.dreamer_tiny_overrides(), discrete_actions=True, actor_grad=actor_grad, **over)
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
    batch = detgen.det_batch(B, T, A=A, seed=seed)
    batch['action'] = np.eye(A, dtype=np.float32)[g[f'{case}.batch_action_idx'].astype(np.int64)]        # one-hot replayed actions
    batch = {k: torch.from_numpy(v).cuda() for k, v in batch.items() if k != 'clip_video'}
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    act_q = detgen.det_noise('imag.act_q', (H, B * T, A), 'exp', seed)
    sites = lambda: {'rssm.prior': [noise['wm']['prior_q'][t] for t in range(T)], 'rssm.post': [noise['wm']['post_q'][t] for t in range(T)],
                     'imag.act_q': act_q, 'imag.step_q': noise['imag']['step_q']}
    return ag, sd, batch, sites


def run_update(ag, batch, sites):
    """-> metrics (floats), captured tensors, gradients per optimiser name"""
    from genrl_amd import noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    grads, cap = {}, {}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    ac = ag._acting_behavior
    orig_wm, orig_tg, orig_al = ag.wm.update, ac.target, ac.actor_loss

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        cap['imag_action'] = seq['action'].detach().cpu().numpy()
        target, mets, baseline = orig_tg(seq)
        cap['imag_target'] = target.detach().cpu().numpy()
        return target, mets, baseline

    def al_hook(seq, target, baseline):
        from genrl_amd import ops
        with torch.no_grad():
            raw = ac._policy_raw(seq)
            lp, en = ops.onehot_logp_ent(raw, seq['action'][1:-1].detach())
            cap['logits'], cap['logp'], cap['ent'] = raw.cpu().numpy(), lp.cpu().numpy(), en.cpu().numpy()
        return orig_al(seq, target, baseline)
    ag.wm.update, ac.target, ac.actor_loss = wm_hook, tg_hook, al_hook
    try:
        with gnoise.inject(sites()):
            _, mets = ag.update(batch, 0)
    finally:
        common.Optimizer.grad_hook = None
        ag.wm.update, ac.target, ac.actor_loss = orig_wm, orig_tg, orig_al
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
    mets, cap, grads = run_update(ag, batch, sites)
    assert (cap['post_idx'] == g[f'{case}.post_idx']).all() and (cap['imag_idx'] == g[f'{case}.imag_idx']).all()
    assert (cap['imag_action'] == g[f'{case}.imag_action'].astype(np.float32)).all()             # one-hot rows (row 0: zeros), exact
    for key in ('logits', 'logp', 'ent'):
        np.testing.assert_allclose(cap[key], g[f'{case}.{key}'], rtol=2e-4, atol=1e-5, err_msg=key)
    np.testing.assert_allclose(cap['imag_target'], g[f'{case}.imag_target'], rtol=2e-4, atol=1e-5, err_msg='lambda-returns')
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
    assert float(grads['actor']['_acting_behavior.actor._out._out.weight'].abs().max()) > 0.0


def test_act_in_both_modes_vs_reference():
    from genrl_amd import noise as gnoise
    g = load()
    ag, sd, batch, sites = setup(g, 'v3dyn')
    B, T, A, S, K, H, seed = [int(x) for x in g['v3dyn.meta']]
    obs = {'observation': batch['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    for mode, ev in (('eval', True), ('sample', False)):
        n = lambda what, shape: detgen.det_noise(f'act.{mode}.{what}', shape, 'exp', seed)
        with gnoise.inject({'rssm.prior': [n('prior_q', (S, K))], 'rssm.post': [n('post_q', (S, K))], 'actor': [n('act_q', (1, A))]}):
            action, (latent, act_t) = ag.act(obs, None, 0, ev, None)
        assert action.shape == (A,) and action.dtype == np.float32
        assert (latent['stoch'].argmax(-1).cpu().numpy() == g[f'act.{mode}.latent_idx']).all()
        if ev:          # the mixed probabilities
            np.testing.assert_allclose(action, g['act.eval.action'], rtol=2e-4, atol=1e-6)
            assert abs(float(action.sum()) - 1.0) < 1e-5 and float(action.min()) >= 0.01 / A * (1 - 1e-5)
        else:           # a one-hot action, the reference's
            assert (action == g['act.sample.action']).all()
        assert torch.equal(act_t[0].cpu(), torch.from_numpy(action))


def test_p2e_update_runs_and_is_reproducible():
    g = load()
    outs = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, 'v2rf', p2e=True)
        mets, cap, grads = run_update(ag, batch, sites)
        assert all(np.isfinite(v) for v in mets.values()), mets
        assert {'disagreement_loss', 'actor_loss', 'actor_ent', 'critic_loss'} <= set(mets)
        outs.append((mets, cap, grads))
    (m0, c0, g0), (m1, c1, g1) = outs
    assert m0 == m1                                                              # bit-identical metrics ...
    assert all(np.array_equal(c0[k], c1[k]) for k in c0)
    assert all(torch.equal(g0[ph][n], g1[ph][n]) for ph in g0 for n in g0[ph])      # ... and gradients on the same noise
    assert (c0['imag_action'][1:].sum(-1) == 1).all()


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_optimizer_step_moves_the_actor_by_at_most_two_lr(case):
    g = load()
    ag, sd, batch, sites = setup(g, case, lr_zero=False)
    lr = float(ag.cfg.actor_opt['lr'])
    run_update(ag, batch, sites)
    after = {k: v.detach().cpu() for k, v in ag.state_dict().items()}
    names = [n for n in sd if n.startswith('_acting_behavior.actor.')]
    assert names
    for n in names:
        d = (after[n] - sd[n]).abs()
        assert float(d.max()) <= 2.0 * lr, (n, float(d.max()), lr)       # (Adam's first step is lr sign(g) up to eps; weight decay is far below)
        assert float(d.max()) > 0.0, n
