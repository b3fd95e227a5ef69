"""Vector (1-D) observations on the MI355X against the reference's vectors (tests/golden/vecobs_tiny.npz, made by
tests/golden/make_vecobs_golden.py): an image plus a 7-wide `proprio` on the dreamer_v3 defaults (symlog inputs, symlog_mse head) and a 9-wide
state alone on the dreamer_v2 defaults (plain inputs, mse head), each with plane operands forced on and with the plane route out of reach, the
way test_gpu_v2.py forces them.  Bounds are that file's: sampled latent indices exact, metrics rtol 2e-4 / atol 1e-6, `embed` and `likes` rtol
2e-4 (with the same atol 1e-6), gradients rtol 1e-3 / atol 1e-5 max|reference| (a gradient of more than 4096 elements is stored on every
fourth index of its first dimension)."""
import os

import numpy as np
import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MLP = [32, 32]
CASES = {'mix': ('dreamer_v3', 'mix', {'proprio': 7}), 'st': ('dreamer_v2', 'states', {'observation': 9})}
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'vecobs_tiny.npz')))
    return _cache['g']


def vec_batch(case, g):
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    batch = {k: v for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    for key, width in CASES[case][2].items():
        batch[key] = (detgen.det_noise('obs.' + key, (B, T, width), 'normal', seed) * 5).numpy()
    return batch


def setup(g, case, lr_zero=True, p2e=False):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, kind, vec_obs = CASES[case]
    over = dict(config.dreamer_tiny_overrides())
    for k, v in config.vecobs_overrides(kind, mlp_layers=MLP).items():
        over[k] = dict(over[k], **v)
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    if p2e:
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
        shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
        pre = f'{case}.shape.'
        shapes = {k[len(pre):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith(pre)}
    sd = detgen.det_state_dict(shapes, seed)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    batch = {k: torch.from_numpy(v).cuda() for k, v in vec_batch(case, g).items()}
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

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['embed'] = outputs['embed'].detach().cpu().numpy()
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        for key, like in outputs['likes'].items():
            cap[f'like.{key}'] = like.detach().cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        return orig_tg(seq)
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


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_update_vs_reference(case, route, monkeypatch):
    from genrl_amd import ops, ops_planes
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    calls = {'planes': 0, 'fp32': 0, 'symlog_rows': 0, 'vec_like': []}
    for mod, key in ((ops_planes, 'planes'), (ops, 'fp32')):
        for fn in ('dense_act', 'dense_ln_act'):
            orig = getattr(mod, fn)
            monkeypatch.setattr(mod, fn, lambda *a, _o=orig, _k=key, **k: (calls.__setitem__(_k, calls[_k] + 1), _o(*a, **k))[1])
    o_sym, o_like = ops.symlog_rows, ops.vec_like
    monkeypatch.setattr(ops, 'symlog_rows', lambda *a, **k: (calls.__setitem__('symlog_rows', calls['symlog_rows'] + 1), o_sym(*a, **k))[1])
    monkeypatch.setattr(ops, 'vec_like', lambda mode, x, kind, *a, **k: (calls['vec_like'].append(kind), o_like(mode, x, kind, *a, **k))[1])
    g = load()
    ag, sd, batch, sites = setup(g, case)
    mets, cap, grads = run_update(ag, batch, sites)
    # the encoder's first layer (7 or 9 wide) stays on the fp32-operand kernels on either route; everything else follows the route
    assert calls['fp32'] > 0 and (calls['planes'] > 0) == (route == 'planes'), calls
    # one symlog launch for the one key of 'mix', none for the plain contiguous key of 'st'; one log-probability node of the case's kind
    assert calls['symlog_rows'] == (1 if case == 'mix' else 0) and calls['vec_like'] == [1 if case == 'mix' else 0], calls
    assert (cap['post_idx'] == g[f'{case}.post_idx']).all() and (cap['imag_idx'] == g[f'{case}.imag_idx']).all()
    np.testing.assert_allclose(cap['embed'], g[f'{case}.embed'], rtol=2e-4, atol=1e-6, err_msg='embed')
    likes = [k for k in g if k.startswith(f'{case}.like.')]
    assert len(likes) == (3 if case == 'mix' else 2)
    for key in likes:
        np.testing.assert_allclose(cap[key[len(case) + 1:]], g[key], rtol=2e-4, atol=1e-6, err_msg=key)
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
    vec = [k for k in grads['model'] if '_mlp_model' in k or '.dense_' in k]
    assert len(vec) == 18 and all(float(grads['model'][k].abs().max()) > 0.0 for k in vec)          # both MLPs and the head are trained


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
    for prefix, opt in (('wm.encoder._mlp_model.', 'model_opt'), ('wm.heads.decoder._mlp_model.', 'model_opt'),
                        ('wm.heads.decoder.dense_', 'model_opt'), ('wm.rssm.', 'model_opt'), ('_acting_behavior.actor.', 'actor_opt'),
                        ('_acting_behavior.critic.', 'critic_opt')):
        lr = float(ag.cfg[opt]['lr'])
        names = [n for n in sd if n.startswith(prefix)]
        assert names
        for n in names:
            d = (a0[n] - sd[n]).abs()
            assert float(d.max()) <= 2.0 * lr * 1.05 + 1e-7, (n, float(d.max()), lr)       # (Adam's first step is lr sign(g) up to eps)
        assert any(float((a0[n] - sd[n]).abs().max()) > 0.0 for n in names), prefix


def test_act_of_the_states_agent_in_both_modes_vs_reference():
    from genrl_amd import noise as gnoise
    g = load()
    ag, sd, batch, sites = setup(g, 'st')
    B, T, A, S, K, H, seed = [int(x) for x in g['st.meta']]
    obs = {'observation': batch['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    assert obs['observation'].shape == (9,)
    for mode, ev in (('eval', True), ('sample', False)):
        n = lambda what, shape, kind: detgen.det_noise(f'act.{mode}.{what}', shape, kind, seed)
        with gnoise.inject({'rssm.prior': [n('prior_q', (S, K), 'exp')], 'rssm.post': [n('post_q', (S, K), 'exp')],
                            'actor': [n('act_eps', (1, A), 'normal')]}):
            action, (latent, act_t) = ag.act(obs, None, 0, ev, None)
        assert action.shape == (A,) and action.dtype == np.float32
        assert (latent['stoch'].argmax(-1).cpu().numpy() == g[f'act.{mode}.latent_idx']).all()
        np.testing.assert_allclose(action, g[f'act.{mode}.action'], rtol=2e-4, atol=1e-6)
    # a float64 observation, as an environment may emit it, is converted (eval mode again, on the same noise)
    n = lambda what, shape: detgen.det_noise(f'act.eval.{what}', shape, 'exp', seed)
    with gnoise.inject({'rssm.prior': [n('prior_q', (S, K))], 'rssm.post': [n('post_q', (S, K))]}):
        a64, _ = ag.act(dict(obs, observation=obs['observation'].astype(np.float64)), None, 0, True, None)
    np.testing.assert_allclose(a64, g['act.eval.action'], rtol=2e-4, atol=1e-6)


def test_report_of_both_agents():
    g = load()
    ag, sd, batch, sites = setup(g, 'st')
    assert ag.report(dict(batch)) == {}
    ag, sd, batch, sites = setup(g, 'mix')
    video = ag.report(dict(batch))
    assert set(video) == {'openl_observation'} and bool(torch.isfinite(video['openl_observation']).all())


def test_p2e_update_on_the_mixed_case_runs_and_is_reproducible():
    g = load()
    outs = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, 'mix', p2e=True)
        assert ag.disagreement.ensemble[0][2].out_features == 128 + MLP[-1]
        mets, cap, grads = run_update(ag, batch, sites)
        assert all(np.isfinite(v) for v in mets.values()), mets
        assert {'disagreement_loss', 'actor_loss', 'critic_loss', 'kl_loss', 'proprio_loss', 'observation_loss'} <= set(mets)
        assert float(max(v.abs().max() for v in grads['disagreement'].values())) > 0.0
        outs.append((mets, cap, grads))
    (m0, c0, g0), (m1, c1, g1) = outs
    assert m0 == m1                                                              # bit-identical metrics ...
    assert all(np.array_equal(c0[k], c1[k]) for k in c0)
    assert all(torch.equal(g0[ph][n], g1[ph][n]) for ph in g0 for n in g0[ph])      # ... and gradients on the same noise


def test_two_vector_keys_update_and_match_float64_on_the_encoder_side():
    """two keys gathered by two symlog launches into one buffer: the embedding's vector part against the float64 restatement, and a finite
    update with a loss per key"""
    import vecobs_restatement as R
    from genrl_amd import config, noise as gnoise
    B, T, A, seed = 2, 18, 6, 6
    over = dict(config.dreamer_tiny_overrides())
    for k, v in config.vecobs_overrides('mix', key='proprio|touch', mlp_layers=MLP).items():
        over[k] = dict(over[k], **v)
    ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', **over), act_dim=A, vec_obs={'proprio': 7, 'touch': 5})
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in ag.state_dict().items()}, seed)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    batch = {k: v for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    for key, width in (('proprio', 7), ('touch', 5)):
        batch[key] = (detgen.det_noise('obs.' + key, (B, T, width), 'normal', seed) * 5).numpy()
    dev = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    with torch.no_grad():
        embed = ag.wm.encoder(ag.wm.preprocess(dev))
    assert embed.shape == (B, T, 128 + MLP[-1])
    x = R.gather([torch.from_numpy(batch[k]).double() for k in ('proprio', 'touch')], True)
    ref = R.mlp(x, R.layers_of(sd, 'wm.encoder._mlp_model.', len(MLP), torch.float64))
    np.testing.assert_allclose(embed[..., 128:].cpu().numpy(), ref.numpy(), rtol=2e-4, atol=1e-6)
    _, mets = ag.update(dev, 0)
    torch.cuda.synchronize()
    mets = {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}
    assert all(np.isfinite(v) for v in mets.values()) and mets['proprio_loss'] > 0 and mets['touch_loss'] > 0


def test_an_image_only_agent_in_the_same_process_keeps_the_smoke_losses():
    """the new route leaves no process-wide state behind: smoke()'s three losses are the same numbers before and after vector-observation
    updates of both cases in this process"""
    from test_gpu_gauss import _smoke_losses
    before = _smoke_losses()
    g = load()
    for case in sorted(CASES):
        ag, sd, batch, sites = setup(g, case)
        run_update(ag, batch, sites)
    after = _smoke_losses()
    print('smoke losses:', after)
    assert before == after and all(np.isfinite(v) for v in after.values())
