"""`pred_discount: True` on the MI355X: the three ops against float64 autograd of the plain-torch restatement (tests/discount_restatement.py),
and the agents against the reference's vectors (tests/golden/discount_tiny.npz, made by tests/golden/make_discount_golden.py) under the bounds
test_gpu_v2.py states: latent indices exact, metrics rtol 2e-4 / atol 1e-6, gradients rtol 1e-3 / atol 1e-5 max|reference| (a gradient of
more than 4096 elements is stored on every fourth index of its first dimension); the head's raw output, the discounts, the weights and the
lambda-returns rtol 2e-4 / atol 1e-5.  Every fixture case runs with plane operands forced on and with the plane path out of reach."""
import gc

import numpy as np
import pytest
import torch

import detgen
import discount_cases as C
import discount_restatement as R

pytestmark = pytest.mark.gpu


def build(g, case, p2e=False, lr_zero=True, flags=None, **extra):
    """-> agent with detgen's weights, the device batch, the noise sites of one update"""
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, over = C.overrides(case, config.dreamer_tiny_overrides(), lr_zero=lr_zero, **extra)
    if p2e:
        over['grad_heads'] = [h for h in over.get('grad_heads', ['decoder']) if h != 'reward']
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
    shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    if not p2e:
        assert shapes == C.shapes_of(g, case)
    ag.load_state_dict({k: v.cuda() for k, v in detgen.det_state_dict(shapes, seed).items()})
    batch = {k: torch.from_numpy(v).cuda() for k, v in C.batch_of(g, case, detgen, flags).items()}
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    act = ({'imag.act_q': detgen.det_noise('imag.act_q', (H, B * T, A), 'exp', seed)} if f'{case}.batch_action_idx' in g
           else {'imag.act_eps': noise['imag']['act_eps']})
    sites = lambda: dict({'rssm.prior': [noise['wm']['prior_q'][t] for t in range(T)], 'rssm.post': [noise['wm']['post_q'][t] for t in range(T)],
                          'imag.step_q': noise['imag']['step_q']}, **act)
    return ag, batch, sites


def run_update(ag, batch, sites, monkeypatch):
    """-> metrics (floats), captured arrays, gradients per optimiser name"""
    from genrl_amd import noise as gnoise, ops
    from genrl_amd.agent import dreamer_utils as common
    grads, cap, calls = {}, {}, {'like': 0, 'imag': 0, 'lambda': 0, 'scalar': 0}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    ac = ag._acting_behavior
    orig_wm, orig_tg = ag.wm.update, ac.target
    o_like, o_imag, o_lam, o_scalar = ops.binary_like, ops.imag_discount, ops.lambda_return_disc, ops.lambda_return

    def like_hook(x, target):
        calls['like'] += 1
        cap['post_raw'] = x.detach().cpu().numpy()
        out = o_like(x, target)
        cap['like_discount'] = out.detach().cpu().numpy()
        return out

    def imag_hook(x, term, gamma):
        calls['imag'] += 1
        cap['imag_raw'] = x.detach().cpu().numpy()
        assert term is not None and term.dtype == torch.float32 and term.numel() == x.shape[1]
        return o_imag(x, term, gamma)
    monkeypatch.setattr(ops, 'binary_like', like_hook)
    monkeypatch.setattr(ops, 'imag_discount', imag_hook)
    monkeypatch.setattr(ops, 'lambda_return_disc', lambda *a: (calls.__setitem__('lambda', calls['lambda'] + 1), o_lam(*a))[1])
    monkeypatch.setattr(ops, 'lambda_return', lambda *a: (calls.__setitem__('scalar', calls['scalar'] + 1), o_scalar(*a))[1])

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        assert seq.unit_weight is False and seq['discount'].requires_grad and not seq['weight'].requires_grad
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        cap['imag_action'] = seq['action'].detach().cpu().numpy()
        cap['imag_discount'] = seq['discount'].detach().cpu().numpy()
        cap['imag_weight'] = seq['weight'].detach().cpu().numpy()
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
        for name, fn in (('binary_like', o_like), ('imag_discount', o_imag), ('lambda_return_disc', o_lam), ('lambda_return', o_scalar)):
            monkeypatch.setattr(ops, name, fn)
    torch.cuda.synchronize()
    assert calls == {'like': 1, 'imag': 1, 'lambda': 1, 'scalar': 0}, calls
    return {k: float(torch.as_tensor(v).detach()) for k, v in mets.items()}, cap, grads


def count_routes(monkeypatch):
    """how many dense layers went through plane operands and how many through fp32 operands"""
    from genrl_amd import ops, ops_planes
    calls = {'planes': 0, 'fp32': 0}
    for mod, key, fns in ((ops_planes, 'planes', ('dense_act', 'dense_ln_act', 'dense_ln_trunk')), (ops, 'fp32', ('dense_act', 'dense_ln_act'))):
        for fn in fns:
            orig = getattr(mod, fn)
            monkeypatch.setattr(mod, fn, lambda *a, _o=orig, _k=key, **k: (calls.__setitem__(_k, calls[_k] + 1), _o(*a, **k))[1])
    return calls


def check_grads(what, got, ref):
    a, b = np.asarray(got), np.asarray(ref)
    if a.size > 4096:
        a = a[::4]
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max(), err_msg=what)


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', list(C.CASES))
def test_update_vs_reference(case, route, monkeypatch):
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    calls = count_routes(monkeypatch)
    g = C.load()
    ag, batch, sites = build(g, case)
    mets, cap, grads = run_update(ag, batch, sites, monkeypatch)
    assert (calls['planes'] > 0) == (route == 'planes') and (route == 'planes' or calls['fp32'] > 10), calls
    assert (cap['post_idx'] == g[f'{case}.post_idx']).all() and (cap['imag_idx'] == g[f'{case}.imag_idx']).all()
    if f'{case}.batch_action_idx' in g:
        assert (cap['imag_action'] == g[f'{case}.imag_action'].astype(np.float32)).all()
    else:
        np.testing.assert_allclose(cap['imag_action'], g[f'{case}.imag_action'], rtol=2e-4, atol=1e-6)
    for key in ('post_raw', 'like_discount', 'imag_raw', 'imag_discount', 'imag_weight', 'imag_target'):
        ref = g[f'{case}.{key}']
        np.testing.assert_allclose(cap[key].reshape(ref.shape), ref, rtol=2e-4, atol=1e-5, err_msg=key)
    # a terminal start state: exact zeros, as in the reference
    term = g[f'{case}.is_terminal'].reshape(-1)
    assert (cap['imag_discount'][0][term] == 0).all() and (cap['imag_weight'][1:][:, term] == 0).all() and (cap['imag_weight'][0] == 1).all()
    assert set(mets) == set(g[f'{case}.metric_keys'].tolist()) and 'discount_loss' in mets
    pre = f'{case}.metrics.'
    for key, val in g.items():
        if key.startswith(pre):
            print(key, mets[key[len(pre):]], float(val))
            np.testing.assert_allclose(mets[key[len(pre):]], float(val), rtol=2e-4, atol=1e-6, err_msg=key)
    n = {'model': 0, 'actor': 0, 'critic': 0}
    pre = f'{case}.grad.'
    for key, val in g.items():
        if key.startswith(pre):
            ph, name = key[len(pre):].split('.', 1)
            check_grads(key, grads[ph][name].numpy(), val); n[ph] += 1
    assert n['actor'] == len(grads['actor']) and n['critic'] == len(grads['critic']) and n['model'] > 10, n
    assert float(grads['model']['wm.heads.discount._out._out.weight'].abs().max()) > 0.0
    assert float(grads['actor']['_acting_behavior.actor._out._out.weight'].abs().max()) > 0.0


def test_the_discounts_carry_a_gradient_into_the_rollout(monkeypatch):
    """the reference does not detach the head's mean (agent/dreamer.py:275-283): with the head's output layer zeroed the discounts are the
    constant gamma sigmoid(1/2) and pass no gradient; the actor's gradient differs from the one with the fixture's head"""
    g = C.load()
    res = []
    for zero in (False, True):
        ag, batch, sites = build(g, 'v3_ent0')
        if zero:
            with torch.no_grad():
                for p in ag.wm.heads['discount']._out.parameters():
                    p.zero_()
        res.append(run_update(ag, batch, sites, monkeypatch))
    (m0, c0, g0), (m1, c1, g1) = res
    const = 0.99 * float(R.binary_mean(torch.zeros((), dtype=torch.float64)))
    np.testing.assert_allclose(c1['imag_discount'][1:], const, rtol=1e-6)
    name = '_acting_behavior.actor.dense0.weight'
    assert not torch.equal(g0['actor'][name], g1['actor'][name])


def _leaf(x, dev=True):
    return (x.float().cuda() if dev else x.double()).requires_grad_(True)


@pytest.mark.parametrize('lead', [(36,), (2, 18), (257,)])
def test_binary_like_op_vs_float64_autograd(lead):
    from genrl_amd import ops
    g = torch.Generator().manual_seed(len(lead) + lead[0])
    x = torch.randn(*lead, 1, generator=g) * 3
    x.view(-1)[:3] = torch.tensor([80.0, -80.0, 0.0])
    t = (torch.rand(*lead, 1, generator=g) < 0.5).float()
    up = torch.randn(*lead, generator=g)
    xd, x64 = _leaf(x), _leaf(x, False)
    out = ops.binary_like(xd, t.cuda())
    ref = R.binary_like(x64, t.double()).sum(-1)
    assert out.shape == tuple(lead)
    (out * up.cuda()).sum().backward(); (ref * up.double()).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x64.grad.numpy(), rtol=1e-5, atol=1e-6 * float(x64.grad.abs().max()))
    assert xd.grad.shape == xd.shape and bool(torch.isfinite(xd.grad).all())


@pytest.mark.parametrize('flags', ['bool (B, T)', 'float (B, T, 1)', 'none'])
def test_imag_discount_op_vs_float64_autograd(flags):
    from genrl_amd import ops
    g = torch.Generator().manual_seed(3)
    H1, Bn, Tn, gamma = 16, 2, 18, 0.99
    N = Bn * Tn
    x = torch.randn(H1, N, 1, generator=g) * 2
    term = torch.from_numpy(C.is_terminal())
    up = torch.randn(H1, N, 1, generator=g)
    xd, x64 = _leaf(x), _leaf(x, False)
    if flags == 'none':
        given, t64 = None, None
    else:           # what WorldModel.imagine hands in: the flattened flags as float
        src = term if flags.startswith('bool') else term.float()[..., None]
        given, t64 = src.cuda().reshape(-1).float(), term.double().reshape(-1, 1)
    disc, weight = ops.imag_discount(xd, given, gamma)
    d64, w64 = R.imag_discount(x64, t64, gamma)
    assert disc.shape == weight.shape == (H1, N, 1) and disc.requires_grad and not weight.requires_grad
    (disc * up.cuda()).sum().backward(); (d64 * up.double()).sum().backward()
    np.testing.assert_allclose(disc.detach().cpu().numpy(), d64.detach().numpy(), rtol=1e-6)
    np.testing.assert_allclose(weight.cpu().numpy(), w64.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x64.grad.numpy(), rtol=1e-5, atol=1e-6 * float(x64.grad.abs().max()))
    if flags != 'none':
        dead = term.reshape(-1)
        dc, wc = disc.detach().cpu(), weight.cpu()
        assert float(xd.grad[0].abs().max()) == 0.0 and float(dc[0][dead].abs().max()) == 0.0 and float(wc[1:][:, dead].abs().max()) == 0.0


@pytest.mark.parametrize('rows', ['H', 'H + 1'])
@pytest.mark.parametrize('lam', [0.0, 0.95, 1.0])
def test_lambda_return_disc_op_vs_float64_autograd(lam, rows):
    from genrl_amd import ops
    g = torch.Generator().manual_seed(11)
    H, N = 15, 36
    n = H if rows == 'H' else H + 1
    r, v = torch.randn(n, N, 1, generator=g), torch.randn(H + 1, N, 1, generator=g) * 2
    d = torch.rand(n, N, 1, generator=g) * 0.99
    d[:, 0] = 0.0
    up = torch.randn(H, N, 1, generator=g)
    dev, cpu = [_leaf(t) for t in (r, v, d)], [_leaf(t, False) for t in (r, v, d)]
    out = ops.lambda_return_disc(*dev, lam)
    ref = R.lambda_return_disc(*cpu, lam)
    assert out.shape == (H, N, 1)
    (out * up.cuda()).sum().backward(); (ref * up.double()).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    for name, a, b in zip(('reward', 'value', 'disc'), dev, cpu):
        assert a.grad.shape == a.shape
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=1e-5, atol=1e-6 * float(b.grad.abs().max()), err_msg=name)
    if rows == 'H + 1':
        assert float(dev[0].grad[H].abs().max()) == 0.0 and float(dev[2].grad[H].abs().max()) == 0.0
    # equal discounts: the scalar node's bits
    const = torch.full_like(dev[2].detach(), 0.99)
    assert torch.equal(ops.lambda_return_disc(dev[0].detach(), dev[1].detach(), const, lam), ops.lambda_return(dev[0].detach(), dev[1].detach(), 0.99, lam))


def test_p2e_update_with_pred_discount_is_reproducible(monkeypatch):
    from genrl_amd import noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    g = C.load()
    outs = []
    for _ in range(2):
        ag, batch, _ = build(g, 'v3_ent0', p2e=True, lr_zero=False)
        assert ag.cfg.pred_discount and ag.cfg.actor_ent == 0 and 'discount' in ag.wm.heads
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
        assert {'disagreement_loss', 'actor_loss', 'critic_loss', 'discount_loss'} <= set(mets)
        outs.append((mets, grads, {k: v.detach().cpu() for k, v in ag.state_dict().items()}))
    (m0, g0, s0), (m1, g1, s1) = outs
    assert m0 == m1
    assert all(torch.equal(g0[ph][n], g1[ph][n]) for ph in g0 for n in g0[ph]) and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert float(g0['model']['wm.heads.discount._out._out.weight'].abs().max()) > 0.0


def test_terminal_flags_change_the_weights_and_not_the_loss_arithmetic(monkeypatch):
    """an all-zero `is_terminal` batch and the fixture's: the head's raw output is the same bits (the flags are only its target), the
    discount loss is -mean(t z - softplus(z)) of that output against each batch's own 1 - is_terminal, and seq['weight'] differs exactly in
    the terminal columns"""
    g = C.load()
    case = 'v2'
    flags = g[f'{case}.is_terminal']
    res = []
    for f in (np.zeros_like(flags), flags):
        ag, batch, sites = build(g, case, flags=f)
        res.append(run_update(ag, batch, sites, monkeypatch))
    (m0, c0, _), (m1, c1, _) = res
    assert np.array_equal(c0['post_raw'], c1['post_raw']) and np.array_equal(c0['imag_raw'], c1['imag_raw'])
    for m, c, f in ((m0, c0, np.zeros_like(flags)), (m1, c1, flags)):
        want = -R.binary_like(torch.from_numpy(c['post_raw']).double().reshape(f.shape), 1.0 - torch.from_numpy(f).double()).mean()
        # (the kernel's bound on one row is 4 units of 2^-24 of |t z| + softplus(z) <= 1.7, a row's |like| is at least 0.57: below 2e-6 relative)
        np.testing.assert_allclose(m['discount_loss'], float(want), rtol=2e-6)
    assert m0['discount_loss'] != m1['discount_loss']
    term = flags.reshape(-1)
    w0, w1 = c0['imag_weight'], c1['imag_weight']
    assert np.array_equal(w0[:, ~term], w1[:, ~term]) and (w1[1:][:, term] == 0).all() and (w0[1:][:, term] > 0).all()
    assert float(c0['imag_discount'][0].min()) == float(np.float32(0.99))


def test_three_steps_eager_replayed_and_resumed_are_bit_for_bit_equal(monkeypatch):
    """three optimiser steps of a `pred_discount` DreamerAgent eagerly, as hipGraph replays (graph.GraphedStep) and resumed from a pickle: the
    legs and the comparison of test_gpu_step_matrix.py with this case added to the table its legs build from; every batch carries terminal
    flags of its own"""
    import test_gpu_step_matrix as SM
    from genrl_amd import ops
    base = SM._cases()
    live = lambda ag, m: ag.cfg.pred_discount and 'discount' in ag.wm.heads and 'discount_loss' in m and 'reward_ema_005' in m
    cases = dict(base, disc_head=('dreamer', 'dreamer_v3', dict(pred_discount=True, grad_heads=['decoder', 'reward', 'discount']), None, live))
    monkeypatch.setattr(SM, '_cases', lambda: cases)
    seen = []
    o_imag = ops.imag_discount
    monkeypatch.setattr(ops, 'imag_discount', lambda x, term, gamma: (seen.append(term is not None), o_imag(x, term, gamma))[1])
    batches, obs = SM.make_batches('disc_head')
    for i, b in enumerate(batches):
        f = torch.zeros(SM.B, SM.T, dtype=torch.bool)
        f[0, SM.T - 1] = f[1, 3 + i] = f[2, 7] = f[3, i] = True
        b['is_terminal'] = f.cuda()
    cache = {}
    try:
        eager = SM.eager_leg('disc_head', batches, obs, cache)
        assert eager['live'] and seen and all(seen)
        SM.check_leg('disc_head', 'eager', eager)
        for leg, fn in (('replay', SM.replay_leg), ('resume', SM.resume_leg)):
            out = fn('disc_head', batches, obs, cache)
            SM.check_leg('disc_head', leg, out)
            SM.compare('disc_head', leg, eager, out)
    finally:
        cache.clear()
        gc.collect()


def test_the_default_configuration_keeps_the_smoke_losses(monkeypatch):
    """nothing leaks from a `pred_discount` agent into the default one: smoke()'s three losses are the same numbers before and after such an
    update in this process"""
    from test_gpu_gauss import _smoke_losses
    before = _smoke_losses()
    g = C.load()
    ag, batch, sites = build(g, 'v3')
    run_update(ag, batch, sites, monkeypatch)
    after = _smoke_losses()
    print('smoke losses:', after)
    assert before == after and all(np.isfinite(v) for v in after.values())
