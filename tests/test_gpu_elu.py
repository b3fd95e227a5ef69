"""DreamerAgent and Plan2Explore with `act: ELU` blocks on the MI355X against the reference's vectors (tests/golden/elu_tiny.npz), on both
operand routes, under the bounds of test_gpu_v2.py: latent indices exact, imagined actions and metrics rtol 2e-4 / atol 1e-6 with the
metric key set equal, gradients rtol 1e-3 / atol 1e-5 max|reference| (a gradient of more than 4096 elements on every fourth index of its
first dimension), one real optimiser step within 2 lr per element and 5 % in L1 per group.  Route liveness is counted at the nodes: every
ELU layer -- dense and conv -- went through the per-layer node of the route under test with the ELU code and none through the other
route's, the code is read again where it arrives at the C entries, and the entries
that have SiLU built in -- the fused rollout, the policy tape, ops.observe_seq, ops.rssm_imagine_seq -- were not entered by an ELU block."""
import numpy as np
import pytest
import torch

import detgen
import elu_cases as E

pytestmark = pytest.mark.gpu


def setup(g, case, lr_zero=True, kind='dreamer'):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g[f'{case}.meta']]
    defaults, blocks = E.CASES[case]
    over = E.elu_overrides(blocks, config.dreamer_tiny_overrides())
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    if kind == 'p2e':
        ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
        shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    else:
        ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A)
        shapes = E.shapes_of(g, case)
    assert E.acts_of(ag) == {k: ('ELU' if k in blocks else 'SiLU') for k in E.BLOCKS}
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

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        return state, outputs, mets

    def tg_hook(seq):
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        cap['imag_action'] = seq['action'].detach().cpu().numpy()
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


def rows(a):
    """what the fixture keeps of a tensor (make_v2_golden.py::grad_rows), flat"""
    a = np.asarray(a)
    return (a[::4] if a.size > 4096 else a).reshape(-1)


# position of the activation code in the C entries that take one (include/genrl_hip.h), and the stand-alone activation entries
C_ACT_ARG = {'genrl_ln_act_fwd': 11, 'genrl_ln_act_fwd_h2': 11, 'genrl_ln_act_fwd_h2u': 11, 'genrl_ln_act_bwd': 16, 'genrl_ln_act_bwd_h2': 16,
             'genrl_ln_act_bwd_h2u': 16, 'genrl_gemm_h2_ln': 26}
C_ROW_ACT = {'genrl_silu_fwd_h2': 1, 'genrl_silu_bwd_h2': 1, 'genrl_elu_fwd_h2': 2, 'genrl_elu_bwd_h2': 2}


def count_calls(monkeypatch):
    """-> calls: {(route, act): layers that went through a per-layer node of that route with that activation}, {('conv_fp32' | 'conv_planes',
    act): ...} for the conv layers' channel-LayerNorm by the module that ran them, {('C', code): launches} for the activation code handed to
    the C entries from Python (0: a LayerNorm alone), and {name: entries} for the entries that have SiLU built in"""
    from genrl_amd import ops, ops_planes, ops_conv_planes
    from genrl_amd._lib import lib
    calls = {}

    def bump(key):
        calls[key] = calls.get(key, 0) + 1

    def node(mod, name, route):
        orig = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, **k: (bump((route, k.get('act', 'SiLU'))), orig(*a, **k))[1])
    node(ops, 'dense_ln_act', 'fp32'); node(ops, 'dense_act', 'fp32')
    node(ops_planes, 'dense_ln_trunk', 'planes'); node(ops_planes, 'dense_act', 'planes')

    def conv(mod, name, key):
        orig = getattr(mod, name)

        def f(x, W, b, ln=None, **k):
            if ln is not None:
                bump((key, ln[3] if len(ln) > 3 else 'SiLU'))
            return orig(x, W, b, ln=ln, **k)
        monkeypatch.setattr(mod, name, f)
    for mod, key in ((ops, 'conv_fp32'), (ops_conv_planes, 'conv_planes')):
        conv(mod, 'conv2d_s2', key); conv(mod, 'convT2d_s2', key)

    def c_entry(name, code_of):
        orig = getattr(lib(), name)
        monkeypatch.setattr(lib(), name, lambda *a: (bump(('C', code_of(a))), orig(*a))[1])
    for name, pos in C_ACT_ARG.items():
        c_entry(name, lambda a, pos=pos: int(a[pos]))
    for name, code in C_ROW_ACT.items():
        c_entry(name, lambda a, code=code: code)

    def entry(mod, name, key):
        orig = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, **k: (bump(key), orig(*a, **k))[1])
    entry(ops, 'imagine_rollout', 'rollout'); entry(ops_planes, 'imagine_rollout', 'rollout')
    entry(ops, 'observe_seq', 'observe_seq'); entry(ops, 'rssm_imagine_seq', 'rssm_imagine_seq')
    tape_init = ops.ActorTape.__init__
    monkeypatch.setattr(ops.ActorTape, '__init__', lambda self, *a, **k: (bump('tape'), tape_init(self, *a, **k))[1])
    return calls


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', sorted(E.CASES))
def test_update_vs_reference(case, route, monkeypatch):
    from genrl_amd import ops_conv_planes
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    monkeypatch.setattr(ops_conv_planes, 'ENABLED', route == 'planes')       # (the conv layers on the fp32-operand nodes of ops.py, or on planes)
    calls = count_calls(monkeypatch)
    g = E.load()
    ag, sd, batch, sites = setup(g, case)
    mets, cap, grads = run_update(ag, batch, sites)
    other = 'fp32' if route == 'planes' else 'planes'
    print(case, route, calls)
    # route liveness: the ELU layers went through the nodes of the route under test with the ELU code, none through the other route's
    assert calls.get((route, 'ELU'), 0) > (50 if case != 'v3a' else 10) and calls.get((other, 'ELU'), 0) == 0, calls
    assert calls.get('rollout', 0) == 0 and calls.get('tape', 0) == 0, calls
    conv, other_conv = f'conv_{route}', f'conv_{other}'
    assert not any(k[0] == other_conv for k in calls if isinstance(k, tuple)), calls           # (no conv layer on the other route's nodes)
    assert calls.get(('C', 2), 0) > 100, calls                       # the ELU code reached the C entries
    if case == 'v3a':        # the actor alone: the rollout left the fused node, the world model kept its fused observe and its SiLU layers
        assert calls.get('observe_seq', 0) >= 1 and calls.get((route, 'SiLU'), 0) > 0 and calls.get((conv, 'ELU'), 0) == 0, calls
        assert calls.get((conv, 'SiLU'), 0) >= 7 and calls.get(('C', 1), 0) > 0, calls
    else:
        assert calls.get('observe_seq', 0) == 0 and calls.get('rssm_imagine_seq', 0) == 0, calls
        assert calls.get((route, 'SiLU'), 0) == 0 and calls.get((other, 'SiLU'), 0) == 0 and calls.get((conv, 'SiLU'), 0) == 0, calls
        assert calls.get((conv, 'ELU'), 0) >= 7, calls               # 4 encoder + 3 decoder layers with a channel-LayerNorm
        assert calls.get(('C', 1), 0) == 0, calls                    # ... and no LayerNorm or row activation was launched with SiLU's
    assert (cap['post_idx'] == g[f'{case}.post_idx']).all() and (cap['imag_idx'] == g[f'{case}.imag_idx']).all()
    np.testing.assert_allclose(cap['imag_action'], g[f'{case}.imag_action'], rtol=2e-4, atol=1e-6)
    ref = E.metrics_of(g, case)
    assert set(mets) == set(ref)
    for key, val in ref.items():
        np.testing.assert_allclose(mets[key], val, rtol=2e-4, atol=1e-6, err_msg=key)
    n = 0
    for ph in ('model', 'actor', 'critic'):
        for name, val in E.unpack(g, f'{case}.grad.{ph}').items():
            np.testing.assert_allclose(rows(grads[ph][name].numpy()), val, rtol=1e-3, atol=1e-5 * np.abs(val).max(), err_msg=f'{ph}.{name}')
            n += 1
    assert n == sum(len(grads[ph]) for ph in grads) and n > 0


def test_report_and_no_grad_imagine_leave_the_c_scan(monkeypatch):
    """EnsembleRSSM.imagine under no_grad (report, video_pred): an ELU rssm goes step by step, a SiLU rssm keeps ops.rssm_imagine_seq"""
    from genrl_amd import noise as gnoise
    calls = count_calls(monkeypatch)
    g = E.load()
    for case, want in (('v3e', 0), ('v3a', 1)):
        ag, sd, batch, sites = setup(g, case)
        B, T, A = [int(x) for x in g[f'{case}.meta'][:3]]
        calls.clear()
        with torch.no_grad(), gnoise.static(seed=3):
            prior = ag.wm.rssm.imagine(batch['action'][:, :5])
        torch.cuda.synchronize()
        assert calls.get('rssm_imagine_seq', 0) == want and tuple(prior['deter'].shape[:2]) == (B, 5), (case, calls)
        assert bool(torch.isfinite(prior['deter']).all())


@pytest.mark.parametrize('case', ['v3e', 'v2e'])
def test_report_with_elu_blocks(case, monkeypatch):
    """DreamerAgent.report (video_pred: observe five steps, decode, imagine the rest, decode) and Plan2Explore's on an ELU agent: finite frames
    in [0, 1] of the reference's layout, no C scan entered, and the ELU code at the C entries alone"""
    from genrl_amd import noise as gnoise
    g = E.load()
    B, T = [int(x) for x in g[f'{case}.meta'][:2]]
    for kind in ('dreamer', 'p2e'):
        ag, sd, batch, sites = setup(g, case, kind=kind)
        with monkeypatch.context() as mp:
            calls = count_calls(mp)
            with gnoise.static(seed=3):
                videos = ag.report(batch)
        torch.cuda.synchronize()
        assert set(videos) == {'openl_observation'}, videos.keys()
        v = videos['openl_observation']
        assert tuple(v.shape) == (B, T, 3, 3 * 64, 64) and bool(torch.isfinite(v).all()) and 0.0 <= float(v.min()) and float(v.max()) <= 1.0
        assert calls.get('observe_seq', 0) == 0 and calls.get('rssm_imagine_seq', 0) == 0 and calls.get(('C', 1), 0) == 0, (kind, calls)
        assert calls.get(('C', 2), 0) > 0, (kind, calls)


def test_act_in_both_modes_vs_reference():
    """test_gpu_tanh.py's rule: the posterior's latent indices exact, the action rtol 2e-4 / atol 1e-6, the returned state holds the action"""
    from genrl_amd import noise as gnoise
    g = E.load()
    ag, sd, batch, sites = setup(g, 'v3e')
    B, T, A, S, K, H, seed = [int(x) for x in g['v3e.meta']]
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
        assert (latent['stoch'].argmax(-1).cpu().numpy() == g[f'act.{mode}.latent_idx']).all()
        np.testing.assert_allclose(action, g[f'act.{mode}.action'], rtol=2e-4, atol=1e-6, err_msg=mode)
        assert torch.equal(act_t[0].cpu(), torch.from_numpy(action))


def test_plan2explore_with_elu_blocks_twice_is_bit_identical():
    """Plan2Explore on the dreamer_v2 defaults with ELU in all six blocks: two updates from the same weights and noise agree bit for bit in
    every metric and every parameter, and every metric is finite (the ensemble keeps its ReLU)"""
    g = E.load()
    out = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, 'v2e', lr_zero=False, kind='p2e')
        mets, cap, grads = run_update(ag, batch, sites)
        out.append((mets, {k: v.detach().cpu().clone() for k, v in ag.state_dict().items()}))
    assert all(np.isfinite(v) for v in out[0][0].values()) and len(out[0][0]) > 10
    assert out[0][0] == out[1][0]
    assert all(torch.equal(out[0][1][k], out[1][1][k]) for k in out[0][1])
    assert any(not torch.equal(out[0][1][k], sd[k]) for k in sd if k.startswith('disagreement.'))


@pytest.mark.parametrize('case', sorted(E.CASES))
def test_one_optimizer_step_vs_reference(case):
    """a real step at the defaults' learning rates (the fixture's 'opt.*'), twice from the same weights: bit-identical; every parameter
    moved by at most 2 lr (Adam's first step is lr sign(g) up to eps); against the reference's deltas at most 2 lr per element and 5 % in
    L1 per group, the rule of test_gpu_v2.py, on the rows the fixture keeps"""
    g = E.load()
    after = []
    for _ in range(2):
        ag, sd, batch, sites = setup(g, case, lr_zero=False)
        run_update(ag, batch, sites)
        after.append({k: v.detach().cpu().clone() for k, v in ag.state_dict().items()})
    assert all(torch.equal(after[0][k], after[1][k]) for k in after[0])
    after = after[0]
    lr = {k: float(g[f'{case}.opt.{k}'][0]) for k in ('model_opt', 'actor_opt', 'critic_opt')}
    assert {k: float(ag.cfg[k]['lr']) for k in lr} == lr
    delta = E.unpack(g, f'{case}.delta')
    groups = {'wm': ('wm.', 'model_opt'), 'actor': ('_acting_behavior.actor.', 'actor_opt'), 'critic': ('_acting_behavior.critic.', 'critic_opt')}
    for gname, (prefix, opt) in groups.items():
        num = den = 0.0
        names = [n for n in sd if n.startswith(prefix)]
        assert names and set(names) <= set(delta)
        for n in names:
            moved = (after[n] - sd[n]).double()
            assert float(moved.abs().max()) <= 2.0 * lr[opt], (gname, n, float(moved.abs().max()))
            dp = rows(moved.numpy()); do = delta[n].astype(np.float64) * lr[opt]
            worst = float(np.abs(dp - do).max())
            assert worst <= 2.0 * lr[opt] * 1.05 + 1e-7, (gname, n, worst)
            num += float(np.abs(dp - do).sum()); den += float(np.abs(do).sum())
        print(f'{case} {gname}: L1 of the delta difference {num / den:.3g} of the delta')
        assert den > 0 and num / den <= 0.05, (gname, num / den)
    for n in after:
        if n.startswith('_acting_behavior._target_critic.'):
            assert torch.equal(after[n], after[n.replace('_target_critic', 'critic')]), n
