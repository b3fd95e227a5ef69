"""Continuous (Gaussian) latents on the MI355X (`rssm.discrete: False`) against the reference's vectors (tests/golden/gauss_tiny.npz, made by
tests/golden/make_gauss_golden.py) and the plain-torch restatement (tests/gauss_restatement.py), under the bounds test_gpu_v2.py states:
metrics and actions rtol 2e-4 / atol 1e-6, gradients rtol 1e-3 / atol 1e-5 max|reference| (a gradient of more than 4096 elements is stored on
every fourth index of its first dimension).  The latents are real numbers here, not indices: mean / std / stoch and the lambda-returns are
held to rtol 2e-4 with the gradients' form of absolute bound, atol 1e-5 max|reference| (an entry near zero is a sum of O(max) terms).  Both
cases run with plane operands forced on and with the plane path off."""
import os

import numpy as np
import pytest
import torch

import detgen
import gauss_restatement as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = {'v2g': ('dreamer_v2', dict(stoch=6, std_act='softplus'), dict(decoder_inputs='feat')),
         'v3g': ('dreamer_v3', dict(stoch=8, std_act='sigmoid2'), dict())}
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'gauss_tiny.npz')))
    return _cache['g']


def setup(g, case, lr_zero=True, p2e=False, **over):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, rssm, extra = CASES[case]
    over = dict(config.dreamer_tiny_overrides(), **extra, **over)
    over['rssm'] = dict(over['rssm'], discrete=False, **rssm)
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
    n = lambda name, shape: detgen.det_noise(name, shape, 'normal', seed)
    sites = lambda: {'wm.prior_eps': n('wm.prior_eps', (T, B, S)), 'wm.post_eps': n('wm.post_eps', (T, B, S)),
                     'imag.act_eps': n('imag.act_eps', (H, B * T, A)), 'imag.step_eps': n('imag.step_eps', (H, B * T, S))}
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

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        for side in ('post', 'prior'):
            assert set(outputs[side]) == {'mean', 'std', 'stoch', 'deter'}
            for key in ('mean', 'std', 'stoch'):
                cap[f'{side}_{key}'] = outputs[side][key].detach().cpu().numpy()
        cap['kl_value'] = outputs['kl'].detach().cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        for key in ('stoch', 'mean', 'std', 'action'):
            cap[f'imag_{key}'] = seq[key].detach().cpu().numpy()
        target, mets, baseline = orig_tg(seq)
        cap['imag_target'] = target.detach().cpu().numpy()
        return target, mets, baseline
    ag.wm.update, ac.target = wm_hook, tg_hook
    try:
        with gnoise.inject(sites()):
            _, mets = ag.update(batch, 0)
    finally:
        common.Optimizer.grad_hook = None
        ag.wm.update, ac.target = orig_wm, orig_tg
    torch.cuda.synchronize()
    return {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}, cap, grads


def check_grads(what, got, ref):
    a, b = np.asarray(got), np.asarray(ref)
    if a.size > 4096:
        a = a[::4]
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max(), err_msg=what)


def set_route(route, monkeypatch):
    """'planes': plane operands from the first row up; 'fp32': the plane path off (what GENRL_PLANES=0 selects when the package is imported)"""
    from genrl_amd import planes
    if route == 'planes':
        monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0')
    else:
        monkeypatch.setenv('GENRL_PLANES', '0')
        monkeypatch.setattr(planes, 'ENABLED', False)


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_update_vs_reference_and_restatement(case, route, monkeypatch):
    from genrl_amd import ops, ops_planes
    set_route(route, monkeypatch)
    calls = {'planes': 0, 'fp32': 0, 'fused': 0}
    for mod, key in ((ops_planes, 'planes'), (ops, 'fp32')):
        for fn in ('dense_act', 'dense_ln_act'):
            orig = getattr(mod, fn)
            monkeypatch.setattr(mod, fn, lambda *a, _o=orig, _k=key, **k: (calls.__setitem__(_k, calls[_k] + 1), _o(*a, **k))[1])
    for mod, fn in ((ops, 'observe_seq'), (ops, 'rssm_imagine_seq'), (ops, 'imagine_rollout'), (ops_planes, 'imagine_rollout')):
        monkeypatch.setattr(mod, fn, lambda *a, **k: calls.__setitem__('fused', calls['fused'] + 1))
    g = load()
    ag, sd, batch, sites = setup(g, case)
    mets, cap, grads = run_update(ag, batch, sites)
    assert calls['fused'] == 0                  # the sequence entries and the fused rollout are not entered
    assert (calls['planes'] > 0) == (route == 'planes') and (route == 'planes' or calls['fp32'] > 0), calls
    if case == 'v2g':                           # stoch 6: the layers that read the latent first stay on the fp32-operand kernels
        assert calls['fp32'] > 0, calls
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    for key in ('post_mean', 'post_std', 'post_stoch', 'prior_mean', 'prior_std', 'prior_stoch', 'kl_value', 'imag_mean', 'imag_std',
                'imag_stoch', 'imag_target'):
        ref = g[f'{case}.{key}']
        np.testing.assert_allclose(cap[key], ref, rtol=2e-4, atol=1e-5 * np.abs(ref).max(), err_msg=key)
    np.testing.assert_allclose(cap['imag_action'], g[f'{case}.imag_action'], rtol=2e-4, atol=1e-6)
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
    assert n == sum(len(grads[ph]) for ph in grads) and n > 0
    # the restatement on what the GPU itself produced: sample, KL, loss and entropies in float64 from its own mean / std
    balance, free, forward, min_std = [float(x) for x in g[f'{case}.kl_cfg']]
    t = lambda k: torch.from_numpy(cap[k]).double()
    for side in ('post', 'prior'):
        eps = detgen.det_noise(f'wm.{side}_eps', (T, B, S), 'normal', seed).transpose(0, 1).double()
        np.testing.assert_allclose(cap[f'{side}_stoch'], (t(f'{side}_mean') + t(f'{side}_std') * eps).numpy(), rtol=1e-6, atol=1e-6)
        assert float(cap[f'{side}_std'].min()) >= min_std
    loss, value = R.kl_balance({'mean': t('post_mean'), 'std': t('post_std')}, {'mean': t('prior_mean'), 'std': t('prior_std')},
                               bool(forward), balance, free)
    np.testing.assert_allclose(cap['kl_value'], value.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mets['kl_loss'], float(loss), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mets['model_kl'], float(value.mean()), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mets['prior_ent'], float(R.entropy(t('prior_std')).mean()), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mets['post_ent'], float(R.entropy(t('post_std')).mean()), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_optimizer_step_changes_the_weights_reproducibly(case):
    g = load()
    afters = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, case, lr_zero=False)
        run_update(ag, batch, sites)
        afters.append({k: v.detach().cpu() for k, v in ag.state_dict().items()})
    a0, a1 = afters
    assert all(torch.equal(a0[k], a1[k]) for k in a0)                            # a second identical run: bit for bit
    for prefix, opt in (('wm.rssm.', 'model_opt'), ('wm.heads.decoder.', 'model_opt'), ('_acting_behavior.actor.', 'actor_opt'),
                        ('_acting_behavior.critic.', 'critic_opt')):
        lr = float(ag.cfg[opt]['lr'])
        names = [n for n in sd if n.startswith(prefix)]
        assert names
        for n in names:
            d = (a0[n] - sd[n]).abs()
            assert float(d.max()) <= 2.0 * lr * 1.05 + 1e-7, (n, float(d.max()), lr)       # (Adam's first step is lr sign(g) up to eps)
        assert any(float((a0[n] - sd[n]).abs().max()) > 0.0 for n in names), prefix
    for n in ('wm.rssm._obs_dist.weight', 'wm.rssm._ensemble_img_dist.0.weight', 'wm.rssm._img_in.0.weight'):
        assert float((a0[n] - sd[n]).abs().max()) > 0.0, n


def test_act_in_both_modes_vs_reference():
    from genrl_amd import noise as gnoise
    g = load()
    ag, sd, batch, sites = setup(g, 'v3g')
    B, T, A, S, K, H, seed = [int(x) for x in g['v3g.meta']]
    obs = {'observation': batch['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    for mode, ev in (('eval', True), ('sample', False)):
        n = lambda what, shape: detgen.det_noise(f'act.{mode}.{what}', shape, 'normal', seed)
        with gnoise.inject({'rssm.prior': [n('prior_eps', (1, S))], 'rssm.post': [n('post_eps', (1, S))], 'actor': [n('act_eps', (1, A))]}):
            action, (latent, act_t) = ag.act(obs, None, 0, ev, None)
        assert action.shape == (A,) and action.dtype == np.float32 and set(latent) == {'mean', 'std', 'stoch', 'deter'}
        for key in ('mean', 'std', 'stoch'):
            ref = g[f'act.{mode}.{key}']
            np.testing.assert_allclose(latent[key].cpu().numpy(), ref, rtol=2e-4, atol=1e-5 * np.abs(ref).max(), err_msg=f'{mode} {key}')
        np.testing.assert_allclose(action, g[f'act.{mode}.action'], rtol=2e-4, atol=1e-6)
        assert torch.equal(act_t[0].cpu(), torch.from_numpy(action))
    # eval_state_mean: the latent is the posterior's mean (the reference raises there); a second step from that state works
    ag.cfg.eval_state_mean = True
    action, (latent, act_t) = ag.act(obs, None, 0, True, None)
    assert torch.equal(latent['stoch'], latent['mean']) and np.isfinite(action).all()
    np.testing.assert_allclose(latent['mean'].cpu().numpy(), g['act.eval.mean'], rtol=2e-4, atol=1e-5 * np.abs(g['act.eval.mean']).max())
    a2, _ = ag.act(dict(obs, is_first=np.bool_(False)), None, 1, True, (latent, act_t))
    assert np.isfinite(a2).all()


def test_unif_dist_and_a_five_step_imagine_without_gradients():
    """the shapes of the data-free warm-up: a start state drawn from get_unif_dist, then rssm.imagine over five given actions"""
    import math
    from genrl_amd import noise as gnoise
    g = load()
    ag, sd, batch, sites = setup(g, 'v2g')
    rssm = ag.wm.rssm
    Bn, A, S = 4, 6, rssm._stoch
    gen = torch.Generator().manual_seed(1)
    eps0, eps = torch.randn(Bn, S, generator=gen), [torch.randn(Bn, S, generator=gen) for _ in range(5)]
    actions = (torch.rand(Bn, 5, A, generator=gen) * 2 - 1).cuda()
    with torch.no_grad():
        start = dict(rssm.initial(Bn))
        unif = rssm.get_unif_dist(start)
        with gnoise.inject({'rssm.unif': eps0}):
            start['stoch'] = unif.sample()
        assert torch.equal(start['stoch'].cpu(), eps0) and float(unif.mean.abs().max()) == 0.0            # N(0, 1): 0 + 1 eps
        np.testing.assert_allclose(unif.entropy().cpu().numpy(), S * (0.5 + 0.5 * math.log(2 * math.pi)), rtol=1e-6)
        assert torch.equal(unif.mode(), unif.mean) and tuple(rssm.get_dist(start).entropy().shape) == (Bn,)
        with gnoise.inject({'rssm.imagine_eps': torch.stack(eps, 0)}):
            prior = rssm.imagine(actions, start)
        assert {k: tuple(v.shape) for k, v in prior.items()} == {'mean': (Bn, 5, S), 'std': (Bn, 5, S), 'stoch': (Bn, 5, S),
                                                                  'deter': (Bn, 5, rssm._deter)}
        state = start
        with gnoise.inject({'rssm.prior': list(eps)}):          # the same rollout, a step at a time with per-step draws
            for t in range(5):
                state = rssm.img_step(state, actions[:, t])
                assert all(torch.equal(state[k], prior[k][:, t]) for k in prior), t
        with gnoise.inject({'rssm.prior': list(eps)}):          # ... and imagine itself accepts the per-step site
            again = rssm.imagine(actions, start)
        assert all(torch.equal(again[k], prior[k]) for k in prior)
        mean_roll = rssm.imagine(actions, start, sample=False)
        assert torch.equal(mean_roll['stoch'], mean_roll['mean']) and float(mean_roll['std'].min()) >= rssm._min_std
        sd_ = prior['std'].double().cpu()
        np.testing.assert_allclose(rssm.get_dist(prior).entropy().cpu().numpy(), R.entropy(sd_).numpy(), rtol=1e-6)
        video = ag.report({k: v for k, v in batch.items()})      # report / video_pred: observe five steps, imagine the rest
        assert all(bool(torch.isfinite(v).all()) for v in video.values()) and len(video) == 1


def test_p2e_update_runs_and_is_reproducible():
    g = load()
    outs = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, 'v3g', p2e=True)                # stoch 8: a multiple of 4
        assert ag.disagreement.ensemble[0][0].in_features == 8 + 32 + 6
        mets, cap, grads = run_update(ag, batch, sites)
        assert all(np.isfinite(v) for v in mets.values()), mets
        assert {'disagreement_loss', 'actor_loss', 'critic_loss', 'kl_loss', 'prior_ent'} <= set(mets)
        assert float(max(v.abs().max() for v in grads['disagreement'].values())) > 0.0
        outs.append((mets, cap, grads))
    (m0, c0, g0), (m1, c1, g1) = outs
    assert m0 == m1                                                              # bit-identical metrics ...
    assert all(np.array_equal(c0[k], c1[k]) for k in c0)
    assert all(torch.equal(g0[ph][n], g1[ph][n]) for ph in g0 for n in g0[ph])      # ... and gradients on the same noise


@pytest.mark.parametrize('defaults', ['dreamer_v3', 'dreamer_v2'])
def test_the_references_stoch_30_updates_and_both_routes_agree(defaults, monkeypatch):
    """`stoch: 30` (feat 62 wide, `_img_in` input 36, the ensemble's 68: no multiple of 4) through Plan2Explore.update -- world model,
    ensemble, behaviour -- with plane operands forced on and with the plane path off.  There is no reference vector at this width; each route
    is held to the reference within rtol 2e-4 on metrics at the fixture's widths, so the two routes must agree within twice that here."""
    from genrl_amd import config
    B, T, A, S, H, seed = 2, 18, 6, 30, 15, 5
    over = dict(config.dreamer_tiny_overrides(), model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    over['rssm'] = dict(over['rssm'], discrete=False, stoch=S, std_act='sigmoid')
    n = lambda name, shape: detgen.det_noise(name, shape, 'normal', seed)
    sites = lambda: {'wm.prior_eps': n('wm.prior_eps', (T, B, S)), 'wm.post_eps': n('wm.post_eps', (T, B, S)),
                     'imag.act_eps': n('imag.act_eps', (H, B * T, A)), 'imag.step_eps': n('imag.step_eps', (H, B * T, S))}
    batch = {k: torch.from_numpy(v).cuda() for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    res = {}
    for route in ('planes', 'fp32'):
        with monkeypatch.context() as mp:
            set_route(route, mp)
            ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
            assert ag.wm.inp_size == 62 and ag.disagreement.ensemble[0][0].in_features == 68
            sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in ag.state_dict().items()}, seed)
            ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
            res[route] = run_update(ag, batch, sites)
    (m0, c0, g0), (m1, c1, g1) = res['planes'], res['fp32']
    assert set(m0) == set(m1) and all(np.isfinite(v) for v in m0.values())
    for k in m0:
        np.testing.assert_allclose(m0[k], m1[k], rtol=4e-4, atol=2e-6, err_msg=k)
    for k in ('post_mean', 'post_std', 'post_stoch', 'imag_stoch', 'imag_target'):
        assert c0[k].shape[-1] in (S, 1)
        np.testing.assert_allclose(c0[k], c1[k], rtol=4e-4, atol=2e-5 * np.abs(c1[k]).max(), err_msg=k)
    assert float(g0['model']['wm.rssm._img_in.0.weight'].abs().max()) > 0.0 and float(g0['disagreement']['disagreement.ensemble.0.0.weight'].abs().max()) > 0.0


def test_kl_gradient_at_a_lower_free_nats_vs_float64_autograd():
    """in the v2g fixture every KL row lies below the free nats (no KL gradient): the same posterior / prior at free = 0.15, rows on both
    sides of the clamp, through ops.gauss_kl_balance against float64 autograd of the restatement"""
    from genrl_amd import ops
    g = load()
    free, mix = 0.15, 0.2
    t = lambda k: torch.from_numpy(g[f'v2g.{k}'])
    names = ('post_mean', 'post_std', 'prior_mean', 'prior_std')
    dev = [t(k).cuda().requires_grad_(True) for k in names]
    loss, value = ops.gauss_kl_balance(*dev, mix, free)
    (3.0 * loss).backward()
    cpu = [t(k).double().requires_grad_(True) for k in names]
    sg = lambda x: x.detach()
    vl = R.kl(cpu[0], cpu[1], sg(cpu[2]), sg(cpu[3]))[0]
    vr = R.kl(sg(cpu[0]), sg(cpu[1]), cpu[2], cpu[3])[0]
    assert bool((vl < free).any()) and bool((vl > free).any())
    ref = mix * torch.clamp(vl, min=free).mean() + (1 - mix) * torch.clamp(vr, min=free).mean()
    (3.0 * ref).backward()
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-6)
    np.testing.assert_allclose(value.cpu().numpy(), vl.detach().numpy(), rtol=1e-5, atol=1e-7)
    for a, b, name in zip(dev, cpu, names):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=1e-5, atol=1e-6 * float(b.grad.abs().max()), err_msg=name)


def _smoke_losses():
    """the GPU half of smoke(): one tiny GenRLAgent iteration (discrete latents) on fixed weights, batch and noise -> its three losses"""
    import sys
    from genrl_amd import config, noise as gnoise
    from oracle import genrl_oracle as O
    from param_shapes import agent_param_shapes
    from test_gpu_iteration import sites_from
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synth_batch
    B, T, A = 2, 16, 10
    zero = dict(lr=0.0, wd=0.0)
    ag = config.make_agent(config.default_cfg(B, T, device='cuda:0', model_opt=zero, actor_opt=zero, critic_opt=zero, **config.tiny_overrides()),
                           act_dim=A)
    ocfg = O.make_cfg(stoch=4, discrete=4, deter=32, hidden=32, units=32, cnn_depth=4, act_dim=A)
    ag.load_state_dict({k: v.cuda() for k, v in detgen.det_state_dict(agent_param_shapes(ocfg), 0).items()})

    class Clip:
        ignores_text = True

        def get_txt_feat(self, text):
            return torch.nn.functional.normalize(torch.randn(1, 512, generator=torch.Generator().manual_seed(123)), dim=-1)
    ag.wm.viclip_model = Clip()
    batch = {k: torch.from_numpy(v).cuda() for k, v in synth_batch(B, T, A).items()}
    with gnoise.inject(sites_from(detgen.iteration_noise(B, T, 4, 4, A, 16))):
        state, outputs, mets = ag.update_wm(batch, 0)
        _, mets = ag.wm.update_additional_detached_modules(batch, outputs, mets)
        _, mets = ag.update_imag_behavior(state=None, outputs=outputs, metrics=mets, seq_data=batch)
    torch.cuda.synchronize()
    return {k: float(mets[k]) for k in ('model_loss', 'imag_actor_loss', 'imag_critic_loss')}


def test_a_discrete_agent_in_the_same_process_keeps_the_smoke_losses():
    """nothing leaks from a continuous-latent agent into a discrete one: smoke()'s three losses are the same numbers before and after a
    continuous-latent update in this process"""
    before = _smoke_losses()
    g = load()
    ag, sd, batch, sites = setup(g, 'v3g')
    run_update(ag, batch, sites)
    after = _smoke_losses()
    print('smoke losses:', after)
    assert before == after and all(np.isfinite(v) for v in after.values())
