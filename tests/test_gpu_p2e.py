"""Plan2Explore (genrl_amd/agent/plan2explore.py) on the MI355X against the reference's vectors (tests/golden/p2e_tiny.npz) and the
float64 restatement (tests/p2e_restatement.py): one update with the plane routes forced on and forced off, one real optimiser step,
hipGraph replay, the reward_free = False branch against DreamerAgent.update, the ensemble at full width, precision 16."""
import os

import numpy as np
import pytest
import torch

import detgen
import p2e_restatement as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load():
    return dict(np.load(os.path.join(G, 'p2e_tiny.npz')))


def setup(g, lr_zero, agent='p2e', **over):
    from genrl_amd import config
    B, T, A, S, K, H, seed = [int(x) for x in g['meta']]
    over = dict(config.dreamer_tiny_overrides(), **over)
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    cfg = config.p2e_cfg(B, T, device='cuda', **over)
    ag = config.make_p2e_agent(cfg, act_dim=A) if agent == 'p2e' else config.make_dreamer_agent(cfg, act_dim=A)
    shapes = {k[len('shape.'):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith('shape.')}
    sd = detgen.det_state_dict(shapes, seed)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items() if agent == 'p2e' or not k.startswith('disagreement.')})
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
    orig_wm, orig_ir = ag.wm.update, ag.compute_intr_reward

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).cpu().numpy()
        return state, outputs, mets

    def ir_hook(seq):
        r = orig_ir(seq)
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).cpu().numpy()
        cap['intr_reward'] = r.detach().cpu()
        return r
    ag.wm.update, ag.compute_intr_reward = wm_hook, ir_hook
    try:
        with gnoise.inject(sites()):
            _, mets = ag.update(batch, 0)
    finally:
        common.Optimizer.grad_hook = None
        ag.wm.update, ag.compute_intr_reward = orig_wm, orig_ir
    torch.cuda.synchronize()
    assert torch.is_tensor(mets['disagreement_loss']) and mets['disagreement_loss'].is_cuda        # (no host sync: a device scalar)
    return {k: float(v) for k, v in mets.items()}, cap, grads


def reward_bound(what, got, feat, action, sd):
    """intrinsic reward: error against the float64 restatement <= 3 x the float32 restatement's error, floor 1e-6 max|reward|"""
    f, a = torch.as_tensor(feat), torch.as_tensor(action)
    with torch.no_grad():
        r64 = R.intr_reward(f.double(), a.double(), R.members_from(sd, dtype=torch.float64))
        r32 = R.intr_reward(f, a, R.members_from(sd))
    e32 = float((r32.double() - r64).abs().max())
    err = float((got.detach().cpu().double() - r64).abs().max())
    bound = max(3.0 * e32, 1e-6 * float(r64.abs().max()))
    print(f'{what}: |product - float64| {err:.3g}, float32 restatement {e32:.3g}, bound {bound:.3g}')
    assert err <= bound, (what, err, e32, bound)


def ambiguous_units(x, W0, b0):
    """[rows, hidden] mask of the pre-activations the float64 reference puts within rounding of the ReLU's kink.  There the gradient is
    either branch's (a subgradient): an fp32 product lands on either side, and the whole weight-gradient row of that unit -- or input-gradient
    row of that sample -- jumps by a finite amount that no tolerance on rounding covers.  'Within rounding': 8 standard deviations of the
    random-walk model of an fp32 dot product's error, 8 x 2^-24 x sqrt(sum (x w)^2 + b^2); the plane products sit at 0.4-2 x the fp32
    MFMAs' error.  The callers compare every other unit / row under the usual bound, assert that these are a handful, and hold
    each of them to the same bound against the reference with its kink units on either branch (check_either_branch)."""
    x, W0, b0 = x.double(), W0.detach().double(), b0.detach().double()
    pre = x @ W0.t() + b0
    tau = 8.0 * 2.0 ** -24 * torch.sqrt((x * x) @ (W0 * W0).t() + b0 * b0)
    return pre.abs() <= tau


def check_grads(what, got, ref):
    a, b = np.asarray(got), np.asarray(ref)
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max(), err_msg=what)


def check_either_branch(what, got, ref, flips, atol):
    """A gradient row that kink units feed: `flips` holds, per (sample, unit) pair at the kink, the float64 change of the row when that
    pair's ReLU mask is flipped.  The row must hold the usual bound against the reference with SOME choice of branches (the pre-activation
    is within rounding of zero there, so the forward is unchanged and either mask is a valid subgradient)."""
    assert 1 <= len(flips) <= 4, (what, len(flips))
    best = None
    for pick in range(1 << len(flips)):
        alt = ref + sum(f for i, f in enumerate(flips) if pick >> i & 1)
        over = float((np.abs(got - alt) - (atol + 1e-3 * np.abs(alt))).max())
        best = over if best is None else min(best, over)
    print(f'{what}: {len(flips)} kink pair(s), worst excess over the bound on the best branch choice {best:.3g}')
    assert best <= 0.0, (what, best)


@pytest.mark.parametrize('route', ['planes', 'fp32'])
def test_update_vs_reference(route, monkeypatch):
    from genrl_amd import ops_planes
    monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0' if route == 'planes' else '1000000')
    calls = []
    orig = ops_planes._member_fwd
    monkeypatch.setattr(ops_planes, '_member_fwd', lambda inp, *a, **k: (calls.append(inp.on_planes), orig(inp, *a, **k))[1])
    g = load()
    ag, sd, batch, sites = setup(g, True)
    mets, cap, grads = run_update(ag, batch, sites)
    assert len(calls) == 10 and all(c == (route == 'planes') for c in calls), calls       # (5 members, training + reward)
    assert (cap['post_idx'] == g['post_idx']).all() and (cap['imag_idx'] == g['imag_idx']).all()
    n = 0
    for key, val in g.items():
        if key.startswith('metrics.'):
            np.testing.assert_allclose(mets[key[len('metrics.'):]], float(val), rtol=2e-4, atol=1e-6, err_msg=key); n += 1
    assert n >= 27 and 'disagreement_loss' in mets and 'disagreement_grad_norm' in mets
    n = 0
    for key, val in g.items():
        if key.startswith('grad.'):
            _, ph, name = key.split('.', 2)
            if ph in ('disagreement', 'actor'):
                check_grads(key, grads[ph][name].numpy(), val); n += 1
    assert n == 20 + len(grads['actor']) and set(grads['disagreement']) == {k for i in range(5) for k in R.member_names(i)}
    # the intrinsic reward of the update (its own rollout) tracks the reference's, first step zero
    r = cap['intr_reward']
    assert r.shape == g['intr_reward'].shape and float(r[0].abs().max()) == 0.0
    np.testing.assert_allclose(r.numpy(), g['intr_reward'], rtol=2e-4, atol=1e-6 * float(np.abs(g['intr_reward']).max()))
    # ... and on the fixture's own inputs it holds the float64 bound
    seq = {'feat': torch.from_numpy(g['imag_feat']).cuda(), 'action': torch.from_numpy(g['imag_action']).cuda()}
    with torch.no_grad():
        got = ag.compute_intr_reward(seq)
    reward_bound(f'intr_reward[{route}]', got, g['imag_feat'], g['imag_action'], sd)


def test_one_optimizer_step_vs_reference():
    """One step with the real optimiser settings against the reference's, under test_gpu_multistep.py's parameter-delta bounds: every
    element within 2 lr of the reference's change, the L1 of a group's delta difference within 5 % of its delta.  The fixture holds the
    reference's change (after - before) / lr rounded to 1/256 as float16, not the parameters themselves (make_p2e_golden.py), so the
    reference side of both comparisons is itself up to lr / 512 per element off the reference's true step: the 2 lr bound is applied as
    it stands and carries that quantisation inside it (0.1 % of the bound; ~0.1 % in L1 against the 5 %)."""
    g = load()
    ag, sd, batch, sites = setup(g, False)
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
    # the slow critic is no optimiser group: the first update hard-copies the stepped critic into it (agent/dreamer.py:455-462)
    for n in after:
        if n.startswith('_acting_behavior._target_critic.'):
            assert torch.equal(after[n], after[n.replace('_target_critic', 'critic')]), n


def test_graph_replay_is_eager_bit_for_bit():
    from genrl_amd import noise
    from genrl_amd.graph import GraphedStep
    g = load()
    step = lambda ag, batch: ag.update(batch, 0)[1]
    cache, res = {}, []
    for graphed in (False, True):
        ag, sd, batch, _ = setup(g, False)
        mets = []
        grab = lambda m: {k: float(torch.as_tensor(v).detach()) for k, v in m.items()}
        with noise.static(seed=7, cache=cache):
            if graphed:
                gs = GraphedStep(ag, batch, step, warmup=1)          # step 1 = the warm-up (eager), then two replays
                assert len(gs._groups()) == 4
                mets.append(None)
                for _ in range(2):
                    m = gs(); torch.cuda.synchronize(); mets.append(grab(m))
            else:
                for _ in range(3):
                    m = step(ag, batch); torch.cuda.synchronize(); mets.append(grab(m))
        assert all(o._groups[0].step == 3 for o in (ag.wm.model_opt, ag.disagreement_opt, ag._acting_behavior.actor_opt,
                                                    ag._acting_behavior.critic_opt))
        res.append((mets, {k: v.detach().cpu() for k, v in ag.state_dict().items()}))
    (m_e, sd_e), (m_g, sd_g) = res
    for i in (1, 2):
        for k, v in m_e[i].items():
            assert m_g[i][k] == v, (i, k, m_g[i][k], v)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert not torch.equal(sd_e['disagreement.ensemble.0.0.weight'], sd['disagreement.ensemble.0.0.weight'])


def test_reward_free_false_is_dreamer_update():
    from genrl_amd import noise as gnoise
    g = load()
    out = []
    for kind in ('p2e', 'dreamer'):
        ag, sd, batch, sites = setup(g, False, agent=kind)
        if kind == 'p2e':
            ag.reward_free = False
        with gnoise.inject(sites()):
            _, mets = ag.update(batch, 0)
        torch.cuda.synchronize()
        out.append(({k: float(v) for k, v in mets.items()}, {k: v.detach().cpu() for k, v in ag.state_dict().items()}))
    (m_p, sd_p), (m_d, sd_d) = out
    assert set(m_p) == set(m_d) and 'disagreement_loss' not in m_p
    for k, v in m_d.items():
        assert m_p[k] == v, (k, m_p[k], v)
    for k, v in sd_d.items():
        assert torch.equal(sd_p[k], v), k
    for k in sd_p:
        if k.startswith('disagreement.'):
            assert torch.equal(sd_p[k], sd[k]), k                 # the ensemble is untouched


def test_full_width_ensemble_vs_float64(monkeypatch):
    """K = 5, E = 6144, input 1536 + 6: 256 training rows (forward + every gradient) and 512 reward rows (forward + the gradient into the
    rollout) against the float64 restatement on the CPU; the products run on plane operands."""
    from genrl_amd import ops, planes
    from genrl_amd.agent.plan2explore import Disagreement
    ops.set_gemm_precision(ops.F32_MODE)
    assert planes.ENABLED
    torch.set_num_threads(min(16, torch.get_num_threads()))
    Kn, D, A, E = 5, 1536, 6, 6144
    sd = R.det_ensemble_state(Kn, D, A, E, E, seed=9)
    dis = Disagreement(D, A, E, pred_dim=E).cuda()
    dis.load_state_dict({k[len('disagreement.'):]: v.cuda() for k, v in sd.items()})
    from genrl_amd import ops_planes
    count = {'gemm': 0, 'tn': 0}
    narrow = []                   # (m, n, k) of the products on the fp32-operand kernel: only the 6 action columns of d W0 may go there
    og, ot, osg = planes.gemm, planes.gemm_tn, ops_planes.sgemm

    def sgemm_spy(*a, **k):
        narrow.append(tuple(int(v) for v in a[9:12]))
        return osg(*a, **k)
    monkeypatch.setattr(ops_planes, 'sgemm', sgemm_spy)
    monkeypatch.setattr(planes, 'gemm', lambda *a, **k: (count.__setitem__('gemm', count['gemm'] + 1), og(*a, **k))[1])
    monkeypatch.setattr(planes, 'gemm_tn', lambda *a, **k: (count.__setitem__('tn', count['tn'] + 1), ot(*a, **k))[1])
    gen = torch.Generator().manual_seed(3)
    # ---- training: 256 rows
    M = 256
    obs, act, nxt = torch.randn(M, D, generator=gen), torch.rand(M, A, generator=gen) * 2 - 1, torch.randn(M, E, generator=gen) * 0.5
    dis.requires_grad_(True)
    err = dis(obs.cuda(), act.cuda(), nxt.cuda())
    loss = err.mean()
    params = [q for m in dis._members() for q in m]
    grads = torch.autograd.grad(loss, params)
    dis.requires_grad_(False)
    assert count['gemm'] == Kn * 3 and count['tn'] == Kn * 2, count        # (forward x 2 + dgrad; both weight gradients on gemm_tn)
    assert narrow == [(E, A, M)] * Kn, narrow                              # (no product with n or k >= 1536 on fp32 operands)
    m64 = R.members_from(sd, dtype=torch.float64, requires_grad=True)
    l64 = R.forward(obs.double(), act.double(), nxt.double(), m64).mean()
    l64.backward()
    np.testing.assert_allclose(float(loss), float(l64.detach()), rtol=2e-4, atol=1e-6)
    x_t = torch.cat([obs, act], -1)
    x64, t64 = x_t.double(), nxt.double()
    for q, (k, j) in zip(grads, [(k, j) for k in range(Kn) for j in range(4)]):
        got, ref = q.cpu().numpy(), m64[k][j].grad.numpy()
        if j < 2:          # first layer: rows of hidden units at the ReLU's kink in some sample are either branch's (ambiguous_units)
            amb = ambiguous_units(x_t, m64[k][0], m64[k][1])
            kink = amb.any(0).numpy()
            assert kink.sum() <= 16, (k, int(kink.sum()))
            print(f'member {k} {("W0", "b0")[j]}: {int(kink.sum())} of {kink.size} hidden units at the kink')
            atol = 1e-5 * np.abs(ref).max()
            np.testing.assert_allclose(got[~kink], ref[~kink], rtol=1e-3, atol=atol, err_msg=R.member_names(k)[j])
            if kink.any():         # flipping pair (m, u) changes row u of d W0 by +-dh[m, u] x[m], of d b0 by +-dh[m, u]
                with torch.no_grad():
                    W0, b0, W2, b2 = (p.detach() for p in m64[k])
                    pre = x64 @ W0.t() + b0
                    diff = t64 - (torch.relu(pre) @ W2.t() + b2)
                    dout = -diff / diff.norm(dim=-1, keepdim=True) / (M * Kn)
                    for u in np.nonzero(kink)[0]:
                        flips = []
                        for m in torch.nonzero(amb[:, u]).flatten().tolist():
                            dh = float(dout[m] @ W2[:, u]) * (-1.0 if pre[m, u] > 0 else 1.0)
                            flips.append((dh * x64[m]).numpy() if j == 0 else np.float64(dh))
                        check_either_branch(f'{R.member_names(k)[j]}[{u}]', got[u], ref[u], flips, atol)
        else:
            check_grads(R.member_names(k)[j], got, ref)
    del grads, m64
    # ---- reward: 512 rows, gradient into the rollout's features
    H, N = 2, 256
    feat = torch.randn(H + 1, N, D, generator=gen)
    action = torch.rand(H + 1, N, A, generator=gen) * 2 - 1
    w = torch.randn(H + 1, N, 1, generator=gen)
    count['gemm'] = 0
    fd = feat.cuda().requires_grad_(True)
    obs_r, act_r = fd[:-1].reshape(-1, D), action.cuda()[1:].reshape(-1, A)
    r = dis.get_disagreement(obs_r, act_r)
    (r * w[1:].reshape(-1).cuda()).sum().backward()
    assert count['gemm'] == Kn * 4, count
    f64 = feat.double().requires_grad_(True)
    m64 = R.members_from(sd, dtype=torch.float64)
    r64 = R.intr_reward(f64, action.double(), m64)
    (r64 * w.double()).sum().backward()
    with torch.no_grad():
        r32 = R.intr_reward(feat, action, R.members_from(sd))
    e32 = float((r32.double() - r64.detach()).abs().max())
    e = float((r.detach().cpu().double().reshape(H, N, 1) - r64.detach()[1:]).abs().max())
    bound = max(3.0 * e32, 1e-6 * float(r64.abs().max()))
    print(f'full-width reward: |product - float64| {e:.3g}, float32 restatement {e32:.3g}, bound {bound:.3g}')
    assert e <= bound, (e, e32, bound)
    x_r = torch.cat([feat[:-1].reshape(-1, D), action[1:].reshape(-1, A)], -1)
    amb = [ambiguous_units(x_r, m[0], m[1]) for m in m64]
    kink = torch.stack([a.any(1) for a in amb]).any(0).numpy()
    assert kink.sum() <= 32, int(kink.sum())
    print(f'reward: {int(kink.sum())} of {kink.size} rows with a hidden unit at the kink')
    got, ref = fd.grad[:-1].reshape(-1, D).cpu().numpy(), f64.grad[:-1].reshape(-1, D).numpy()
    atol = 1e-5 * np.abs(ref).max()
    np.testing.assert_allclose(got[~kink], ref[~kink], rtol=1e-3, atol=atol, err_msg='d reward / d feat')
    assert narrow == [(E, A, M)] * Kn, narrow                              # (the reward pass put nothing on fp32 operands)
    with torch.no_grad():          # flipping pair (m, member k, unit u) changes d r / d feat[m] by +-dh_k[m, u] W0_k[u, :D]
        for m in np.nonzero(kink)[0]:
            xm = x_r[m].double()
            pre = [xm @ W0.t() + b0 for W0, b0, _, _ in m64]
            p = torch.stack([torch.relu(pre[k]) @ m64[k][2].t() + m64[k][3] for k in range(Kn)])
            dout = float(w[1:].reshape(-1)[m]) * 2.0 * (p - p.mean(0)) / ((Kn - 1) * E)
            flips = []
            for k in range(Kn):
                for u in torch.nonzero(amb[k][m]).flatten().tolist():
                    dh = float(dout[k] @ m64[k][2][:, u]) * (-1.0 if pre[k][u] > 0 else 1.0)
                    flips.append((dh * m64[k][0][u, :D]).numpy())
            check_either_branch(f'd reward / d feat[{m}]', got[m], ref[m], flips, atol)
    assert float(fd.grad[-1].abs().max()) == 0.0


def test_chunked_disagreement_is_the_unchunked_one(monkeypatch):
    """get_disagreement in row chunks (the bounded workspace) gives the same rows and the same gradient as one chunk"""
    from genrl_amd.agent.plan2explore import Disagreement
    sd = R.det_ensemble_state(5, 48, 6, 128, 128, seed=2)
    dis = Disagreement(48, 6, 128, pred_dim=128).cuda()
    dis.load_state_dict({k[len('disagreement.'):]: v.cuda() for k, v in sd.items()})
    gen = torch.Generator().manual_seed(1)
    obs, act = torch.randn(300, 48, generator=gen).cuda(), torch.rand(300, 6, generator=gen).cuda()
    dis.requires_grad_(False)
    out = []
    for chunk in ('4096', '128'):
        monkeypatch.setenv('GENRL_P2E_CHUNK', chunk)
        o = obs.clone().requires_grad_(True)
        r = dis.get_disagreement(o, act)
        r.sum().backward()
        out.append((r.detach(), o.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # a retained graph runs the node's backward again (two consumers of the reward): the same gradient both times
    o = obs.clone().requires_grad_(True)
    r = dis.get_disagreement(o, act)
    g1, = torch.autograd.grad(r.sum(), o, retain_graph=True)
    g2, = torch.autograd.grad(r.sum(), o)
    assert torch.equal(g1, out[0][1]) and torch.equal(g2, g1)
    dis.requires_grad_(True)
    with pytest.raises(Exception):
        dis.get_disagreement(obs, act)                             # frozen members only


def test_precision16_step_runs_and_is_finite():
    from genrl_amd import ops, planes
    g = load()
    saved = planes.ENABLED
    try:
        ag, sd, batch, sites = setup(g, False, precision=16)
        mets, cap, grads = run_update(ag, batch, sites)
        assert all(np.isfinite(v) for v in mets.values()), mets
        assert all(bool(torch.isfinite(v).all()) for v in ag.state_dict().values())
        assert not planes.ENABLED and ops.gemm_precision_is_p16()
    finally:
        ops.set_gemm_precision(ops.F32_MODE)
        planes.ENABLED, planes._amp_saved = saved, None
