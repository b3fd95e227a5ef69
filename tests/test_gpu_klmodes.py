"""`kl.balance: 0.5`, `kl.free_avg: True` and `clip_rewards: sign | tanh` on the MI355X against the reference's vectors
(tests/golden/klmodes_tiny.npz, made by tests/golden/make_klmodes_golden.py) and float64 autograd of the plain-torch restatement
(tests/klmodes_restatement.py), under the bounds test_gpu_v2.py states: metrics rtol 2e-4 / atol 1e-6, gradients rtol 1e-3 / atol
1e-5 max|reference| (a gradient of more than 4096 elements is stored on every fourth index of its first dimension); the latents' statistics
and the per-row KL rtol 2e-4 with the gradients' form of absolute bound.  The reference's averaged-mode loss has shape [1]: compared after a
squeeze.  Every fixture case runs with plane operands forced on and with the plane path off."""
import gc

import numpy as np
import pytest
import torch

import detgen
import klmodes_cases as C
import klmodes_restatement as R

pytestmark = pytest.mark.gpu


def build(g, case, p2e=False, lr_zero=True, **extra):
    """-> agent with detgen's weights, the device batch, the noise sites of one update_wm"""
    from genrl_amd import config
    kind, (B, T, A, seed), over = C.overrides(g, case, config, lr_zero=lr_zero, **extra)
    S, K = int(g[f'{case}.meta'][3]), int(g[f'{case}.meta'][4])
    if kind == 'genrl':
        ag = config.make_agent(config.default_cfg(B, T, device='cuda', **over), act_dim=A)
    elif p2e:
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', **over), act_dim=A)
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', **over), act_dim=A)
    shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    if not p2e:
        assert shapes == C.shapes_of(g, case)
    ag.load_state_dict({k: v.cuda() for k, v in detgen.det_state_dict(shapes, seed).items()})
    batch = {k: torch.from_numpy(v).cuda() for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if kind == 'genrl' or k != 'clip_video'}
    if K == 0:
        n = lambda name: detgen.det_noise(name, (T, B, S), 'normal', seed)
        sites = lambda: {'wm.prior_eps': n('wm.prior_eps'), 'wm.post_eps': n('wm.post_eps')}
    else:
        noise = detgen.iteration_noise(B, T, S, K, A, ag.cfg.imag_horizon, seed=seed)
        c = noise['conn1']
        sites = lambda: {'wm.prior_q': noise['wm']['prior_q'], 'wm.post_q': noise['wm']['post_q'], 'conn.clip_eps': [c['clip_eps']],
                         'conn.init_q': [c['init_q']], 'conn.ikl_init_q': [c['ikl_init_q']], 'conn.ikl_step_q': [c['ikl_step_q']]}
    return ag, batch, sites


def run_update_wm(ag, batch, sites):
    """-> metrics (floats), captured arrays, the gradients of each optimiser call in order"""
    from genrl_amd import noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    grads, cap = [], {}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.append({names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    orig_pre = ag.wm.preprocess

    def pre_hook(obs):
        out = orig_pre(obs)
        cap['reward'] = out['reward'].detach().cpu().numpy()
        return out
    ag.wm.preprocess = pre_hook
    conn = getattr(ag.wm, 'connector', None)
    if conn is not None:
        orig_ckl = conn.kl_loss

        def ckl_hook(post, prior, **kw):
            loss, value = orig_ckl(post, prior, **kw)
            if 'conn_kl_value' not in cap and torch.is_grad_enabled():
                cap.update(conn_prior_logit=prior['logit'].detach().cpu().numpy(), conn_kl_value=value.detach().cpu().numpy())
            return loss, value
        conn.kl_loss = ckl_hook
    try:
        with gnoise.inject(sites()):
            state, outputs, mets = ag.update_wm(batch, 0)
    finally:
        common.Optimizer.grad_hook = None
        ag.wm.preprocess = orig_pre
        if conn is not None:
            conn.kl_loss = orig_ckl
    torch.cuda.synchronize()
    for side in ('post', 'prior'):
        for key in ag.wm.rssm._latent.stats:
            cap[f'{side}_{key}'] = outputs[side][key].detach().cpu().numpy()
    cap['kl_value'] = outputs['kl'].detach().cpu().numpy()
    return {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}, cap, grads


def check_grads(what, got, ref):
    a, b = np.asarray(got), np.asarray(ref)
    if a.size > 4096:
        a = a[::4]
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max(), err_msg=what)


def count_routes(monkeypatch):
    from genrl_amd import ops, ops_planes
    calls = {'planes': 0, 'fp32': 0}
    for mod, key in ((ops_planes, 'planes'), (ops, 'fp32')):
        for fn in ('dense_act', 'dense_ln_act'):
            orig = getattr(mod, fn)
            monkeypatch.setattr(mod, fn, lambda *a, _o=orig, _k=key, **k: (calls.__setitem__(_k, calls[_k] + 1), _o(*a, **k))[1])
    return calls


def count_modes(monkeypatch):
    """the mode every KL reduction of the op layer ran in"""
    from genrl_amd import ops
    seen = []
    orig = ops._kl_loss_fwd
    monkeypatch.setattr(ops, '_kl_loss_fwd', lambda kl, Rn, mode, mix, free: (seen.append(mode), orig(kl, Rn, mode, mix, free))[1])
    return seen


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', C.CASES)
def test_update_wm_vs_reference(case, route, monkeypatch):
    from genrl_amd import ops
    from test_gpu_gauss import set_route
    set_route(route, monkeypatch)
    calls, modes = count_routes(monkeypatch), count_modes(monkeypatch)
    g = C.load()
    ag, batch, sites = build(g, case)
    mets, cap, grads = run_update_wm(ag, batch, sites)
    assert (calls['planes'] > 0) == (route == 'planes'), calls
    kl = C.kl_of(g, case)
    want = [ops.KL_MODES[R.mode_of(kl['balance'], kl['free_avg'])]]
    if case == 'genrl':
        ck = C.kl_of(g, case, 'conn_kl_cfg')
        want += [ops.KL_MODES[R.mode_of(ck['balance'], ck['free_avg'])]] * 2          # the connector's loss, then its initial-KL metric
    assert modes == want, (modes, want)
    np.testing.assert_allclose(cap['reward'], g[f'{case}.reward'], rtol=1e-6, atol=1e-7, err_msg='clipped reward')
    for key in [k for k in cap if k != 'reward']:
        ref = g[f'{case}.{key}']
        np.testing.assert_allclose(cap[key], ref, rtol=2e-4, atol=1e-5 * np.abs(ref).max(), err_msg=key)
    assert set(g[f'{case}.metric_keys'].tolist()) <= set(mets)
    pre, n = f'{case}.metrics.', 0
    for key, val in g.items():
        if key.startswith(pre):
            print(key, mets[key[len(pre):]], float(np.squeeze(val)))
            np.testing.assert_allclose(mets[key[len(pre):]], float(np.squeeze(val)), rtol=2e-4, atol=1e-6, err_msg=key); n += 1
    assert n == len(g[f'{case}.metric_keys'])
    assert len(grads) == (2 if case == 'genrl' else 1)
    for ph, gd in zip(('model', 'connector'), grads):
        pre, n = f'{case}.grad.{ph}.', 0
        for key, val in g.items():
            if key.startswith(pre):
                check_grads(key, gd[key[len(pre):]].numpy(), val); n += 1
        assert n > 20 or (ph == 'connector' and n > 10), (ph, n)
    # the KL's gradient is in what was compared: the prior head is reached by the KL term alone
    prior_head = float(grads[0]['wm.rssm._ensemble_img_dist.0.weight'].abs().max())
    assert (prior_head == 0.0) if case == 'avg_lo' else (prior_head > 0.0), prior_head


@pytest.mark.parametrize('route', ['planes', 'fp32'])
def test_a_clamped_mean_gives_the_gradients_of_a_zero_kl_scale(route, monkeypatch):
    """averaged free nats with the mean below `free`: the KL term has no gradient at all -- every gradient of the update is bit for bit the
    one of the same agent with `loss_scales.kl = 0`"""
    from test_gpu_gauss import set_route
    set_route(route, monkeypatch)
    g = C.load()
    assert g['avg_lo.kl_value'].mean() < C.kl_of(g, 'avg_lo')['free']
    res = []
    for extra in ({}, dict(loss_scales=dict(kl=0.0))):
        ag, batch, sites = build(g, 'avg_lo', **extra)
        assert ag.cfg.loss_scales.kl == (0.0 if extra else 0.6)
        res.append(run_update_wm(ag, batch, sites))
    (m0, c0, g0), (m1, c1, g1) = res
    assert m0['kl_loss'] == m1['kl_loss'] == pytest.approx(C.kl_of(g, 'avg_lo')['free'], rel=1e-6) and m0['model_loss'] != m1['model_loss']
    assert set(g0[0]) == set(g1[0]) and len(g0[0]) > 30
    for name in g0[0]:
        assert torch.equal(g0[0][name], g1[0][name]), name
    assert any(float(v.abs().max()) > 0 for v in g0[0].values())


def _autograd_case(g, case, tm):
    """the fixture's posterior / prior statistics as float64 CPU leaves and float32 device leaves; tm: the device tensors are (B, T, ..)
    views of time-major storage"""
    cpu, dev = [], []
    for side in ('post', 'prior'):
        st = C.stats_of(g, case, side)
        cpu.append({k: torch.from_numpy(v).double().requires_grad_(True) for k, v in st.items()})
        d = {}
        for k, v in st.items():
            t = torch.from_numpy(v).cuda()
            if tm:
                t = t.transpose(0, 1).contiguous().requires_grad_(True)
                d[k] = (t, t.transpose(0, 1))
            else:
                t = t.requires_grad_(True)
                d[k] = (t, t)
        dev.append(d)
    return cpu, dev


@pytest.mark.parametrize('tm', [False, True], ids=['batch-major', 'time-major view'])
@pytest.mark.parametrize('mode,case,free', [('unbalanced', 'unb_fwd', None), ('unbalanced', 'unb_g', None), ('free_avg', 'avg_hi', None),
                                            ('free_avg', 'avg_g', None), ('free_avg', 'avg_hi', 2.0), ('free_avg', 'avg_g', 3.0)])
def test_ops_in_the_new_modes_vs_float64_autograd(mode, case, free, tm):
    """ops.kl_balance / ops.gauss_kl_balance on the fixture's posteriors and priors; free None: the fixture's own (rows on both sides of the
    clamp in the unbalanced cases, the mean above it in the averaged ones), else a `free` above the mean (no gradient)"""
    from genrl_amd import ops
    g = C.load()
    kl = C.kl_of(g, case)
    free = kl['free'] if free is None else free
    (post, prior), (dpost, dprior) = _autograd_case(g, case, tm)
    ref, value = R.kl_loss(post, prior, kl['forward'], kl['balance'], free, kl['free_avg'])
    assert R.mode_of(kl['balance'], kl['free_avg']) == mode
    (3.0 * ref).backward()
    lhs, rhs = (dprior, dpost) if kl['forward'] else (dpost, dprior)
    mix = kl['balance'] if kl['forward'] else 1 - kl['balance']
    if 'logit' in lhs:
        loss, got = ops.kl_balance(lhs['logit'][1], rhs['logit'][1], mix, free, mode)
    else:
        loss, got = ops.gauss_kl_balance(lhs['mean'][1], lhs['std'][1], rhs['mean'][1], rhs['std'][1], mix, free, mode)
    (3.0 * loss).backward()
    assert loss.dim() == 0 and got.shape == value.shape and not got.requires_grad
    if mode == 'unbalanced':
        assert bool((value < free).any()) and bool((value > free).any())
    np.testing.assert_allclose(float(loss.detach()), float(ref.detach()), rtol=1e-6)
    np.testing.assert_allclose(got.cpu().numpy(), value.numpy(), rtol=1e-5, atol=1e-7)
    clamped = mode == 'free_avg' and float(value.mean()) < free
    for side, c, d in (('post', post, dpost), ('prior', prior, dprior)):
        for k in c:
            leaf = d[k][0]
            a = (leaf.grad.transpose(0, 1) if tm else leaf.grad).cpu().numpy()
            b = c[k].grad.numpy()
            assert leaf.grad.shape == leaf.shape
            if clamped:
                assert float(np.abs(a).max()) == 0.0 and float(np.abs(b).max()) == 0.0, (side, k)
            else:
                assert float(np.abs(b).max()) > 0.0
                np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6 * float(np.abs(b).max()), err_msg=f'{side} {k}')


def test_p2e_update_with_free_avg_is_reproducible():
    from genrl_amd import noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    g = C.load()
    outs = []
    for _ in range(2):
        ag, batch, _ = build(g, 'avg_hi', p2e=True, lr_zero=False)
        assert ag.cfg.kl.free_avg and ag.cfg.clip_rewards == 'tanh'
        grads = {}
        names = {id(q): n for n, q in ag.named_parameters()}
        common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
        try:
            with gnoise.static(seed=3, cache={}):
                _, mets = ag.update(batch, 0)
        finally:
            common.Optimizer.grad_hook = None
        torch.cuda.synchronize()
        mets = {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}
        assert all(np.isfinite(v) for v in mets.values()), mets
        assert {'disagreement_loss', 'actor_loss', 'critic_loss', 'kl_loss'} <= set(mets)
        outs.append((mets, grads, {k: v.detach().cpu() for k, v in ag.state_dict().items()}))
    (m0, g0, s0), (m1, g1, s1) = outs
    assert m0 == m1
    assert all(torch.equal(g0[ph][n], g1[ph][n]) for ph in g0 for n in g0[ph]) and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert float(g0['model']['wm.rssm._ensemble_img_dist.0.weight'].abs().max()) > 0.0


def test_averaged_mode_steps_eager_and_replayed_are_bit_for_bit_equal(monkeypatch):
    """optimiser steps of one averaged-mode DreamerAgent eagerly and as hipGraph replays (graph.GraphedStep): the legs and the comparison
    of test_gpu_step_matrix.py -- metrics of the later steps, every state_dict entry, the optimiser groups -- with this case added to the
    table its legs build from.  The mode is decided on the device (the backward reads the mean the forward wrote), so the capture holds for
    whichever side of `free` a later step's mean falls on."""
    import test_gpu_step_matrix as SM
    from genrl_amd.agent import dreamer_utils as common
    base = SM._cases()
    live = lambda ag, m: ag.cfg.kl.free_avg and ag.cfg.kl.balance != 0.5 and ag.cfg.clip_rewards == 'tanh' and 'kl_loss' in m
    cases = dict(base, avg_v3=('dreamer', 'dreamer_v3', dict(kl=dict(free_avg=True, free=0.3), clip_rewards='tanh'), None, live))
    monkeypatch.setattr(SM, '_cases', lambda: cases)
    modes = count_modes(monkeypatch)
    batches, obs = SM.make_batches('avg_v3')
    cache = {}
    try:
        eager = SM.eager_leg('avg_v3', batches, obs, cache)
        assert eager['live'] and modes and set(modes) == {2}, modes
        SM.check_leg('avg_v3', 'eager', eager)
        out = SM.replay_leg('avg_v3', batches, obs, cache)
        SM.check_leg('avg_v3', 'replay', out)
        SM.compare('avg_v3', 'replay', eager, out)
    finally:
        cache.clear()
        gc.collect()


def test_the_default_configuration_keeps_the_smoke_losses():
    """nothing leaks from a new-mode agent into the default one: smoke()'s three losses are the same numbers before and after a new-mode
    update in this process"""
    from test_gpu_gauss import _smoke_losses
    before = _smoke_losses()
    g = C.load()
    for case in ('unb_fwd', 'avg_g'):
        ag, batch, sites = build(g, case)
        run_update_wm(ag, batch, sites)
    after = _smoke_losses()
    print('smoke losses:', after)
    assert before == after and all(np.isfinite(v) for v in after.values())
