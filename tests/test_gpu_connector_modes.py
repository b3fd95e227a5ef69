"""The connector's switches -- `temporal_embeds`, `token_dropout`, `detached_post: False`, `learn_initial: False` -- on the MI355X against
the reference's vectors (tests/golden/connector_tiny.npz, made by tests/golden/make_connector_golden.py) under the bounds of
test_gpu_klmodes.py: metrics rtol 2e-4 / atol 1e-6; per-row KL and logits rtol 2e-4 / atol 1e-5 max|reference|; gradients rtol 1e-3 /
atol 1e-5 max|reference| (a gradient of more than 4096 elements is stored on every fourth index of its first dimension).  Every fixture
case runs with plane operands forced on and with the plane path off; one case at 192 teacher-forced rows (B12 x T16) runs under the default
row threshold against the float64 restatement (tests/connector_restatement.py), so the plane route is taken by the row count."""
import numpy as np
import pytest
import torch

import detgen
import connector_cases as C
import connector_restatement as R
from test_gpu_klmodes import run_update_wm, check_grads, count_routes

pytestmark = pytest.mark.gpu
WORST = {}                 # the largest |error| / bound seen per kind of comparison (printed: the margins the bounds leave)


def near(kind, what, got, ref, rtol, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ratio = float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=what)


def build(B, T, A, seed, over):
    from genrl_amd import config
    ag = config.make_agent(config.default_cfg(B, T, device='cuda', **over), act_dim=A)
    shapes = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    ag.load_state_dict({k: v.cuda() for k, v in detgen.det_state_dict(shapes, seed).items()})
    batch = {k: torch.from_numpy(v).cuda() for k, v in detgen.det_batch(B, T, A=A, seed=seed).items()}
    return ag, batch, shapes


def sites_of(ag, B, T, A, seed, drop_e):
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    noise = detgen.iteration_noise(B, T, S, K, A, ag.cfg.imag_horizon, seed=seed)
    c = noise['conn1']

    def sites():
        s = {'wm.prior_q': noise['wm']['prior_q'], 'wm.post_q': noise['wm']['post_q'], 'conn.clip_eps': [c['clip_eps']],
             'conn.init_q': [c['init_q']], 'conn.ikl_init_q': [c['ikl_init_q']], 'conn.ikl_step_q': [c['ikl_step_q']]}
        if drop_e is not None:
            s['conn.drop'] = [drop_e]
        return s
    return sites, noise


def record_keep(monkeypatch):
    from genrl_amd import ops
    seen, orig = [], ops.tf_inputs
    monkeypatch.setattr(ops, 'tf_inputs', lambda *a: (lambda out: (seen.append(out[1].detach().cpu().numpy()), out)[1])(orig(*a)))
    return seen


def check_update(case_name, sw, mets, cap, grads, ref_metrics, ref_arrays, ref_grads):
    """ref_metrics: name -> float; ref_arrays: 'conn_prior_logit', 'conn_kl_value', 'conn_post_logit'; ref_grads: phase -> name -> array"""
    detached = sw['detached_post']
    assert ('connector_model_loss' in mets) == detached == ('connector_model_grad_norm' in mets), sorted(mets)
    assert set(ref_metrics) <= set(mets)
    for k, v in ref_metrics.items():
        print(case_name, k, mets[k], v)
        near('metrics', k, mets[k], v, 2e-4, 1e-6)
    for got, name in ((cap['conn_prior_logit'], 'conn_prior_logit'), (cap['conn_kl_value'], 'conn_kl_value'), (cap['post_logit'], 'conn_post_logit')):
        ref = ref_arrays[name]
        near('rows', name, got, ref, 2e-4, 1e-5 * np.abs(ref).max())
    assert len(grads) == (2 if detached else 1)
    by_phase = {'model': grads[0], 'connector': grads[-1]}
    for ph, refs in ref_grads.items():
        assert len(refs) > 10, (ph, len(refs))
        for name, ref in refs.items():
            got = by_phase[ph][name].numpy()
            got = got[::4] if got.size > 4096 else got
            if np.abs(ref).max() > 0:
                WORST['grads'] = max(WORST.get('grads', 0.0), float((np.abs(got - ref) / (1e-5 * np.abs(ref).max() + 1e-3 * np.abs(ref))).max()))
            check_grads(f'{ph} {name}', by_phase[ph][name].numpy(), ref)
    if detached:       # the world-model step does not see the connector, and the connector's step nothing else
        assert not any(n.startswith('wm.connector.') for n in grads[0]) and all(n.startswith('wm.connector.') for n in grads[1])
    else:
        assert any(n.startswith('wm.connector.') for n in grads[0]) and any(n.startswith('wm.encoder.') for n in grads[0])


@pytest.mark.parametrize('route', ['planes', 'fp32'])
@pytest.mark.parametrize('case', C.CASES)
def test_update_wm_vs_reference(case, route, monkeypatch):
    from test_gpu_gauss import set_route
    set_route(route, monkeypatch)
    calls, keeps = count_routes(monkeypatch), record_keep(monkeypatch)
    g = C.load()
    from genrl_amd import config
    (B, T, A, seed, nseed), over = C.overrides(g, case, config)
    sw = C.switches_of(g, case)
    ag, batch, shapes = build(B, T, A, seed, over)
    assert shapes == C.shapes_of(g, case)
    sites, _ = sites_of(ag, B, T, A, seed, C.drop_noise(g, case))
    mets, cap, grads = run_update_wm(ag, batch, sites)
    assert (calls['planes'] > 0) == (route == 'planes'), calls
    if sw['token_dropout'] > 0:
        assert len(keeps) == 1 and np.array_equal(keeps[0], g[f'{case}.keep'])
    else:
        assert not keeps                              # (the torch path of the shipped configuration)
    ref_metrics = {k: float(np.squeeze(g[f'{case}.metrics.{k}'])) for k in g[f'{case}.metric_keys'].tolist()}
    ref_grads = {ph: {k[len(f'{case}.grad.{ph}.'):]: v for k, v in g.items() if k.startswith(f'{case}.grad.{ph}.')} for ph in ('model', 'connector')}
    ref_grads = {ph: v for ph, v in ref_grads.items() if v}
    assert set(ref_grads) == ({'connector'} if sw['detached_post'] else {'model', 'connector'})
    check_update(f'{case}/{route}', sw, mets, cap, grads, ref_metrics, {k: g[f'{case}.{k}'] for k in ('conn_prior_logit', 'conn_kl_value', 'conn_post_logit')},
                 ref_grads)
    print('largest error / bound so far:', {k: round(v, 4) for k, v in WORST.items()})


@pytest.mark.parametrize('reset', C.RESETS)
@pytest.mark.parametrize('case', C.IMAGINED)
def test_video_imagine_vs_reference(case, reset):
    from genrl_amd import config, noise as gnoise
    g = C.load()
    (B, T, A, seed, nseed), over = C.overrides(g, case, config)
    ag, batch, _ = build(B, T, A, seed, over)
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    with torch.no_grad(), gnoise.inject({'imag.target_init_q': [detgen.det_noise('vi.init_q', (B * S, K), 'exp', seed)]}):
        out = ag.wm.connector.video_imagine(batch['clip_video'], sample=False, reset_every_n_frames=reset)
    torch.cuda.synchronize()
    for key in ('logit', 'deter'):
        ref = g[f'{case}.vi.{int(reset)}.{key}']
        assert out[key].shape == ref.shape
        near('imagine', f'{key} reset={reset}', out[key].cpu().numpy(), ref, 2e-4, 1e-5 * np.abs(ref).max())
    other = g[f'{case}.vi.{int(not reset)}.deter']          # (the other mode restarts deter, or does not, from the second chunk on)
    assert not np.allclose(out['deter'].cpu().numpy()[:, 8:], other[:, 8:], rtol=2e-4, atol=1e-5 * np.abs(other).max())


def test_192_rows_take_the_plane_route_by_their_count(monkeypatch):
    """all four switches at B12 x T16 under the default row threshold (192), against float64 autograd of the restatement"""
    from genrl_amd import config, ops_planes
    from genrl_amd.agent import dreamer_utils as common
    from oracle import genrl_oracle as O
    monkeypatch.delenv('GENRL_PLANES_MIN_ROWS', raising=False)
    B, T, A, seed, p = 12, 16, 10, 5, 0.25
    assert ops_planes.min_rows() == B * T == 192 and common.planes_route(B * T) and not common.planes_route(B * T - 1)
    calls = count_routes(monkeypatch)
    g = C.load()
    sw = C.switches_of(g, 'all')
    _, over = C.overrides(g, 'all', config)
    ag, batch, shapes = build(B, T, A, seed, over)
    e = detgen.det_noise('conn.drop', (T, B), 'exp', seed)
    u = torch.exp(-e.double())
    assert float((u - p).abs().min()) > 1e-4 and 0 < int((u > p).sum()) < T * B
    sites, noise = sites_of(ag, B, T, A, seed, e)
    mets, cap, grads = run_update_wm(ag, batch, sites)
    assert calls['planes'] > 0, calls
    # the restatement in float64
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        cfg = O.make_cfg(stoch=4, discrete=4, act_dim=A, deter=32, hidden=32, units=32, cnn_depth=4)
        pr = {k: v.double() for k, v in detgen.det_state_dict(shapes, seed).items()}
        names = [k for k in pr if k.startswith(('wm.rssm.', 'wm.encoder.', 'wm.connector.')) and '.aligner.' not in k]
        for k in pr:
            if k.startswith('wm.') and pr[k].is_floating_point():
                pr[k].requires_grad_(True)
        cb = {k: (v.cpu().double() if v.dtype in (torch.float32, torch.uint8) else v.cpu()) for k, v in batch.items()}
        model_loss, outs, wmets = O.wm_loss(pr, cfg, cb, noise['wm'])
        loss, cmets, extra = R.update(pr, cfg, cb['clip_video'], outs['post'], noise['conn1'], sw, R.keep_flags(u, p))
        total = model_loss + loss
        ref = dict(zip(names, torch.autograd.grad(total, [pr[k] for k in names])))
    finally:
        torch.set_default_dtype(prev)
    ref_metrics = {k: float(v.detach()) for k, v in dict(wmets, **cmets, model_loss=total).items()}
    arrays = dict(conn_prior_logit=extra['prior_logit'].detach().numpy(), conn_kl_value=extra['kl_value'].detach().numpy(),
                  conn_post_logit=outs['post']['logit'].detach().numpy())
    sample = lambda x: x[::4] if x.size > 4096 else x
    ref_grads = {'model': {k: sample(v.numpy()) for k, v in ref.items()}}
    check_update('all/192 rows', sw, mets, cap, grads, ref_metrics, arrays, ref_grads)
    print('largest error / bound so far:', {k: round(v, 4) for k, v in WORST.items()})


def test_finetune_mode_releases_an_end_to_end_connector():
    """two real steps of the 'e2e' case, finetune_mode between them: afterwards the connector's weights do not move and own no gradient
    buffer, no connector metric is reported, and the world model's one Adam group goes on from its moments and step count"""
    from genrl_amd import config, noise as gnoise
    g = C.load()
    (B, T, A, seed, nseed), over = C.overrides(g, 'e2e', config, lr_zero=False, model_opt=dict(wd=0.0))
    ag, batch, _ = build(B, T, A, seed, over)
    conn = ag.wm.connector
    with gnoise.static(seed=3, cache={}):
        _, _, m1 = ag.update_wm(batch, 0)
        torch.cuda.synchronize()
        (group,) = ag.wm.model_opt._groups
        held = {id(q) for q in group.params}
        assert all(id(q) in held for q in conn.parameters()) and group.step == 1 and 'connector_kl' in m1
        names = {id(q): n for n, q in ag.wm.named_parameters()}
        moments = {names[id(q)]: group.m[off:off + q.numel()].clone() for q, off in zip(group.params, group.offsets)}
        before = {n: q.detach().clone() for n, q in ag.wm.named_parameters()}
        ag.finetune_mode()
        (group2,) = ag.wm.model_opt._groups
        assert group2 is not group and group2.step == 1 and int(group2.step_dev) == 1
        assert not any(id(q) in {id(x) for x in group2.params} for q in conn.parameters())
        names2 = names
        for q, off in zip(group2.params, group2.offsets):
            assert torch.equal(group2.m[off:off + q.numel()], moments[names2[id(q)]]), names2[id(q)]
            assert torch.equal(q.detach(), before[names2[id(q)]])
        assert all(q.grad is None for q in conn.parameters())
        _, _, m2 = ag.update_wm(batch, 0)
        torch.cuda.synchronize()
    assert not any('connector' in k or 'aligner' in k for k in m2) and group2.step == 2 and len(ag.wm.model_opt._groups) == 1
    after = {n: q.detach() for n, q in ag.wm.named_parameters()}
    assert all(torch.equal(after[n], before[n]) for n in after if n.startswith('connector.'))
    assert not torch.equal(after['encoder._conv_model.0.weight'], before['encoder._conv_model.0.weight'])
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in m2.values())


def test_the_default_configuration_keeps_the_smoke_losses(monkeypatch):
    """nothing leaks from an agent with the switches set into the default one: smoke()'s three losses are the same numbers before and
    after such updates in this process, and the default configuration never reaches the new kernels"""
    from genrl_amd import config, ops
    from genrl_amd._lib import lib
    from test_gpu_gauss import _smoke_losses
    before = _smoke_losses()
    g = C.load()
    for case in ('all', 'drop'):
        (B, T, A, seed, nseed), over = C.overrides(g, case, config)
        ag, batch, _ = build(B, T, A, seed, over)
        sites, _ = sites_of(ag, B, T, A, seed, C.drop_noise(g, case))
        run_update_wm(ag, batch, sites)
    new = []
    monkeypatch.setattr(ops, 'tf_inputs', lambda *a, **k: new.append('tf_inputs'))
    orig = ops.connector_prep
    monkeypatch.setattr(ops, 'connector_prep', lambda *a, temporal=False, **k: (new.append('temporal') if temporal else None, orig(*a, temporal=temporal, **k))[1])
    after = _smoke_losses()
    print('smoke losses:', after)
    assert before == after and all(np.isfinite(v) for v in after.values()) and not new


@pytest.mark.parametrize('case', ['temporal', 'all'])
def test_report_and_reward_target_run_through_the_switches(case):
    """GenRLAgent.report (video_clip_pred and report_text2video) and the cached reward target of update_imag_behavior (_build_target) with
    the switches set: every call reaches get_action with whole sequences, so the slots are one_hot(t % 8) of the position inside the call --
    the target's T + 1 steps start at slot 0 and what is kept of them at slot 1 -- and everything that comes out is finite"""
    from genrl_amd import config, noise as gnoise
    from genrl_amd.tools import genrl_utils as GU
    from test_gpu_infer import FakeClip
    g = C.load()
    (B, T, A, seed, nseed), over = C.overrides(g, case, config, additional_report_fns=['report_text2video'])
    ag, batch, _ = build(B, T, A, seed, over)
    ag.wm.viclip_model = FakeClip()
    conn, nf, E = ag.wm.connector, 8, 512
    calls, orig = [], conn.get_action
    conn.get_action = lambda ve: (lambda a: (calls.append(a), a)[1])(orig(ve))
    labels = GU.DOMAIN2PREDICATES.get('stickman')
    GU.DOMAIN2PREDICATES['stickman'] = ['behaviour 0', 'behaviour 1']
    try:
        with gnoise.static(seed=3, cache={}):
            rep = ag.report(batch, nvid=2)
            lengths = [a.shape[1] for a in calls]
            assert lengths == [nf, T - nf], lengths                   # report_text2video's one chunk, then video_clip_pred's continuation
            state, outputs, mets = ag.update_wm(batch, 0)
            del calls[:]
            _, mets = ag.update_imag_behavior(state=None, outputs=outputs, metrics=mets, seq_data=batch)
            assert len(calls) == 1 and calls[0].shape[0] == B * T and calls[0].shape[2] == E + nf, [a.shape for a in calls]
        torch.cuda.synchronize()
    finally:
        conn.get_action = orig
        if labels is None:
            del GU.DOMAIN2PREDICATES['stickman']
        else:
            GU.DOMAIN2PREDICATES['stickman'] = labels
    slots, steps = calls[0][..., E:].cpu(), calls[0].shape[1]          # (skip_first_target: one step more than the target keeps)
    want = torch.nn.functional.one_hot(torch.arange(steps) % nf, nf).float()
    assert steps > nf + 1 and torch.equal(slots, want.expand(B * T, steps, nf)) and int(slots[0, 1].argmax()) == 1
    assert tuple(ag.unconditional_target['deter'].shape[:2]) == (steps - 1, B * T) and ag.cfg.imag_reward_args.skip_first_target
    assert rep['video_clip_pred'].shape[:2] == (2, T) and rep['text_to_video'].shape[:2] == (2, nf)
    for name in ('video_clip_pred', 'text_to_video', 'openl_observation'):
        assert bool(torch.isfinite(rep[name].float()).all()), name
    assert all(bool(torch.isfinite(torch.as_tensor(v).float()).all()) for v in mets.values()) and any(k.startswith('imag_') for k in mets)
