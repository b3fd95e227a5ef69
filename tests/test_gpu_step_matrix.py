"""Three optimiser steps of EVERY agent configuration, three ways, compared bit for bit: eagerly, as one eager step followed by two
hipGraph replays (graph.GraphedStep), and as one eager step, a pickle round trip of the whole agent, and two more steps on the copy (the
checkpoint / resume path of train.py).  The other GPU test files pin one update of these configurations against the reference at lr = 0 and
take at most one real step; here the weights move (the defaults' learning rates), the slow-critic copy falls between steps
(`slow_target_update=2`), and what is compared is everything a later step depends on: the metrics of steps 2 and 3, every state_dict entry,
the optimiser groups' flat parameters / Adam moments / device step counters, the return EMA, StreamNorm's statistics, the host counters
and the action `act()` returns afterwards (it reads the cached weight operands, which must reflect the last Adam step).

Why the third leg is an independent check: the unpickled agent has fresh Python objects at new device addresses, so every cache keyed by
id(), data_ptr() or a weakref (planes._wcache / _dcache, Optimizer._live_cache) starts empty; whatever the continuing agent carried over
from step 1 in such a cache -- stale or frozen -- the copy rebuilds from the weights themselves.

B = 4, T = 16 at tiny widths: 64-row stages, so under the suite's environment (tests/conftest.py) the plane weight-gradient kernel and the
plane rollout are taken; `v2` and `disc_rf` run a second time with the plane route out of reach.  Every comparison is torch.equal.

StreamNorm.step is a host counter that GraphedStep does not rewind after a capture the way it rewinds the optimiser groups' `step`.
Nothing reads it (dreamer_utils.StreamNorm increments it and `reset` zeroes it; no other use in genrl_amd/), so it is left out of the
comparison: the capture's Python pass counts once, the replays not at all, so it is not the number of steps taken under replay.

Where the two paths meet -- a checkpoint taken WHILE a GraphedStep drives the agent, resumed with eager steps -- is a test of its own
(test_checkpoint_taken_under_replay_resumes_eagerly): the copy carried the driver's `_defer_slow_target` flag along and never copied its
slow critic again, until ActorCritic.__getstate__ left the flag out."""
import gc
import io
import os
import sys

import numpy as np
import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu
B, T, A, SEED = 4, 16, 6, 11
STEPS = 3


def _merge(*overs):
    out = {}
    for over in overs:
        for k, v in over.items():
            out[k] = dict(out.get(k, {}), **v) if isinstance(v, dict) else v
    return out


def _head(ag):
    return ag._acting_behavior.actor._out._head


# id -> (agent kind, defaults, overrides, vector observations, check that the configured route is live (agent, metrics of a step))
def _cases():
    from genrl_amd import config
    from genrl_amd.agent import dreamer_utils as C
    return {
        'v3': ('dreamer', 'dreamer_v3', {}, None,
               lambda ag, m: (ag.wm.grad_heads == ['decoder', 'reward'] and 'reward_loss' in m and ag.cfg.actor_ent == 3e-4
                              and isinstance(_head(ag), C._NormalHead) and not _head(ag).trunc and 'reward_ema_005' in m
                              and not ag.wm.rssm.single_obs_posterior and ag.wm.rssm._norm == 'layer')),
        'v2': ('dreamer', 'dreamer_v2', {}, None,
               lambda ag, m: (ag.wm.rssm._norm == 'none' and ag._acting_behavior.actor._norm == 'none' and _head(ag).trunc
                              and isinstance(ag.wm.heads['reward']._out._head, C._MSEHead) and ag.cfg.image_dist == 'normal_unit_std'
                              and 'reward_ema_005' not in m and ag._acting_behavior.rewnorm._momentum == 1.0)),
        'p2e_v2': ('p2e', 'dreamer_v2', {}, None,
                   lambda ag, m: ('disagreement_loss' in m and ag._acting_behavior.rewnorm._momentum == 0.95
                                  and ag.wm.rssm._norm == 'none' and ag.reward_free)),
        'disc_dyn': ('dreamer', 'dreamer_v3', dict(discrete_actions=True, actor_grad='dynamics'), None,
                     lambda ag, m: isinstance(_head(ag), C._OneHotHead) and ag._acting_behavior.actor_grad == 'dynamics'),
        'disc_rf': ('dreamer', 'dreamer_v2', dict(discrete_actions=True, actor_grad='reinforce'), None,
                    lambda ag, m: (isinstance(_head(ag), C._OneHotHead) and ag._acting_behavior.actor_grad == 'reinforce'
                                   and ag.wm.rssm._norm == 'none')),
        'gauss_v3': ('dreamer', 'dreamer_v3', dict(rssm=dict(discrete=False, stoch=8, std_act='sigmoid2')), None,
                     lambda ag, m: (isinstance(ag.wm.rssm._latent, C._NormalLatent) and ag.wm.rssm._latent.std_act == 'sigmoid2'
                                    and ag.wm.rssm.get_stoch_size() == 8)),
        'gauss_v2': ('dreamer', 'dreamer_v2', dict(rssm=dict(discrete=False, stoch=6, std_act='softplus')), None,
                     lambda ag, m: (isinstance(ag.wm.rssm._latent, C._NormalLatent) and ag.wm.rssm._latent.std_act == 'softplus'
                                    and ag.wm.rssm.get_stoch_size() == 6 and ag.wm.rssm._norm == 'none')),
        'vec_mix': ('dreamer', 'dreamer_v3', config.vecobs_overrides('mix'), {'proprio': 7},
                    lambda ag, m: (ag.wm.encoder.cnn_keys == ['observation'] and ag.wm.encoder.mlp_keys == ['proprio']
                                   and ag.wm.encoder._symlog_inputs and {'proprio_loss', 'observation_loss'} <= set(m))),
        'vec_states': ('dreamer', 'dreamer_v3', config.vecobs_overrides('states'), {'observation': 9},
                       lambda ag, m: (ag.wm.encoder.cnn_keys == [] and ag.wm.encoder.mlp_keys == ['observation']
                                      and ag.wm.heads['decoder'].cnn_keys == [] and not hasattr(ag.wm.encoder, '_conv_model'))),
        'tanh_v3': ('dreamer', 'dreamer_v3', dict(actor=dict(dist='tanh_normal'), actor_ent=3e-4), None,
                    lambda ag, m: isinstance(_head(ag), C._TanhNormalHead) and ag.cfg.actor_ent == 3e-4 and ag.wm.rssm._norm == 'layer'),
        'tanh_v2': ('dreamer', 'dreamer_v2', dict(actor=dict(dist='tanh_normal', init_std=1.0)), None,
                    lambda ag, m: (isinstance(_head(ag), C._TanhNormalHead) and ag._acting_behavior.actor._out._init_std == 1.0
                                   and ag.wm.rssm._norm == 'none')),
        'genrl': ('genrl', None, {}, None,
                  lambda ag, m: (hasattr(ag.wm, 'connector') and ag._imag_behavior is not ag._acting_behavior
                                 and any(k.startswith('connector_') for k in m) and any(k.startswith('imag_') for k in m))),
    }


CASE_IDS = ['v3', 'v2', 'p2e_v2', 'disc_dyn', 'disc_rf', 'gauss_v3', 'gauss_v2', 'vec_mix', 'vec_states', 'tanh_v3', 'tanh_v2', 'genrl']
PARAMS = [(c, 'planes') for c in CASE_IDS] + [('v2', 'fp32'), ('disc_rf', 'fp32')]


def _bench():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    return bench


def build(case):
    """-> a freshly built agent of the case with detgen's weights loaded"""
    from genrl_amd import config
    kind, defaults, over, vec_obs, _ = _cases()[case]
    if kind == 'genrl':
        ag = config.make_agent(config.default_cfg(B, T, device='cuda', **_merge(config.tiny_overrides(), dict(slow_target_update=2))))
        ag.wm.viclip_model = _bench().TextStub()
    else:
        over = _merge(config.dreamer_tiny_overrides(), over, dict(slow_target_update=2))
        if kind == 'p2e':
            ag = config.make_p2e_agent(config.p2e_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
        else:
            ag = config.make_dreamer_agent(config.dreamer_cfg(B, T, device='cuda', defaults=defaults, **over), act_dim=A, vec_obs=vec_obs)
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in ag.state_dict().items()}, SEED)
    ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
    return ag


def make_batches(case):
    """one replay batch per step (the replay leg writes each into the graph's static inputs), and the observation `act` is asked about"""
    kind, defaults, over, vec_obs, _ = _cases()[case]
    act_dim = 10 if kind == 'genrl' else A
    batches = []
    for i in range(STEPS):
        seed = SEED + i
        batch = detgen.det_batch(B, T, A=act_dim, seed=seed)
        if kind != 'genrl':
            batch.pop('clip_video')
        if over.get('discrete_actions'):           # one-hot replayed actions
            batch['action'] = np.eye(act_dim, dtype=np.float32)[batch['action'].argmax(-1)]
        for key, width in (vec_obs or {}).items():
            batch[key] = (detgen.det_noise('obs.' + key, (B, T, width), 'normal', seed) * 5).numpy()
        batches.append({k: torch.from_numpy(v).cuda() for k, v in batch.items()})
    obs = {'observation': batches[0]['observation'][0, 3].cpu().numpy(), 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    for key in (vec_obs or {}):
        obs[key] = batches[0][key][0, 3].cpu().numpy()
    return batches, obs


def step_fn(case):
    if case == 'genrl':
        return _bench().one_step
    return lambda ag, b: ag.update(b, 0)[1]


def behavior(ag):
    from genrl_amd.graph import GraphedStep
    return GraphedStep._behavior(ag)


def groups(ag):
    """every flat optimiser group the iteration steps, reached the way GraphedStep._groups reaches them"""
    ac = behavior(ag)
    opts = [ag.wm.model_opt, ac.actor_opt, ac.critic_opt]
    if getattr(ag, 'disagreement_opt', None) is not None:
        opts.append(ag.disagreement_opt)
    return [g for o in opts for g in o._groups]


def steps_per_iteration(ag):
    """1 for every group but the GenRL connector's, which bench.one_step -- like the reference's train.py -- updates twice per iteration"""
    conn = {id(p) for p in ag.wm.connector.parameters()} if hasattr(ag.wm, 'connector') else set()
    return [2 if id(g.params[0]) in conn else 1 for g in groups(ag)]


def grab(m):
    return {k: torch.as_tensor(v).detach().cpu().clone() for k, v in m.items()}


NORM_STATS = ('mag', 'mean', 'square_mean')


def snapshot(ag):
    """everything a later step depends on, cloned to the host"""
    torch.cuda.synchronize()
    ac = behavior(ag)
    c = lambda t: None if t is None else t.detach().cpu().clone()
    snap = {'state': {k: c(v) for k, v in ag.state_dict().items()},
            'groups': [{k: c(getattr(g, k)) for k in ('flat', 'm', 'v', 'step_dev')} for g in groups(ag)],
            'steps': [g.step for g in groups(ag)], 'updates': ac._updates,
            'rewnorm': {k: c(getattr(ac.rewnorm, k)) for k in NORM_STATS}}
    if ag.cfg.reward_ema:
        snap['ema_vals'] = c(ac.ema_vals)
    return snap


def finish(ag, obs, mets, snap1, cache):
    """the state after the last step and the action `act` returns on it: from the weight operands as the last step (eager, replayed or
    resumed) left them cached, and once more with every cached operand declared stale -- the same weights, so the same action"""
    from genrl_amd import noise, planes
    snap3 = snapshot(ag)
    with noise.static(seed=SEED, cache=cache):
        action, _ = ag.act(obs, None, 0, eval_mode=True, state=None)
        planes.invalidate()
        again, _ = ag.act(obs, None, 0, eval_mode=True, state=None)
    assert np.array_equal(action, again), ('act() read a weight operand that did not reflect the last optimiser step', action, again)
    return dict(mets=mets, snap1=snap1, snap3=snap3, action=np.array(action), per_iter=steps_per_iteration(ag))


def eager_leg(case, batches, obs, cache):
    from genrl_amd import noise
    ag, step = build(case), step_fn(case)
    mets = []
    with noise.static(seed=SEED, cache=cache):
        for i, b in enumerate(batches):
            m = step(ag, b)
            torch.cuda.synchronize()
            mets.append(grab(m))
            if i == 0:
                snap1 = snapshot(ag)
    live = _cases()[case][4](ag, mets[0])
    return dict(finish(ag, obs, mets[1:], snap1, cache), live=live)


def replay_leg(case, batches, obs, cache):
    from genrl_amd import noise
    from genrl_amd.graph import GraphedStep
    ag, step = build(case), step_fn(case)
    mets = []
    with noise.static(seed=SEED, cache=cache):
        gs = GraphedStep(ag, batches[0], step, warmup=1)          # step 1 runs eagerly inside (the warm-up), then the capture
        assert [id(g) for g in gs._groups()] == [id(g) for g in groups(ag)]
        assert gs.items and all(kind == 'graph' for kind, _ in gs.items)
        snap1 = snapshot(ag)
        for b in batches[1:]:
            m = gs(b)
            torch.cuda.synchronize()
            mets.append(grab(m))
    return finish(ag, obs, mets, snap1, cache)


def checkpoint(ag):
    """-> the agent after torch.save / torch.load of the whole object, as train.py checkpoints it: fresh objects at new device addresses"""
    buf = io.BytesIO()
    torch.save(ag, buf)
    buf.seek(0)
    copy = torch.load(buf, weights_only=False)
    assert copy is not ag and groups(copy)[0].flat.data_ptr() != groups(ag)[0].flat.data_ptr()
    return copy


def resume_leg(case, batches, obs, cache):
    from genrl_amd import noise
    ag, step = build(case), step_fn(case)
    mets = []
    with noise.static(seed=SEED, cache=cache):
        m = step(ag, batches[0])
        torch.cuda.synchronize()
        snap1 = snapshot(ag)
        copy = checkpoint(ag)
        del ag, m
        gc.collect()
        for b in batches[1:]:
            m = step(copy, b)
            torch.cuda.synchronize()
            mets.append(grab(m))
    return finish(copy, obs, mets, snap1, cache)


def replay_then_resume_leg(case, batches, obs, cache):
    """step 1 eagerly (the warm-up), step 2 as a replay, then a checkpoint of the agent WHILE a GraphedStep drives it, and step 3 eagerly on
    the copy: the copy belongs to no GraphedStep, so it has to advance its slow critic itself"""
    from genrl_amd import noise
    from genrl_amd.graph import GraphedStep
    ag, step = build(case), step_fn(case)
    mets = []
    with noise.static(seed=SEED, cache=cache):
        gs = GraphedStep(ag, batches[0], step, warmup=1)
        snap1 = snapshot(ag)
        m = gs(batches[1])
        torch.cuda.synchronize()
        mets.append(grab(m))
        copy = checkpoint(ag)
        del ag, gs, m
        gc.collect()
        m = step(copy, batches[2])
        torch.cuda.synchronize()
        mets.append(grab(m))
    return finish(copy, obs, mets, snap1, cache)


def same_tensor(what, a, b):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), (what, float((a.double() - b.double()).abs().max()))


def compare(case, leg, ref, got):
    for i, (a, b) in enumerate(zip(ref['mets'], got['mets'])):
        assert set(a) == set(b), (case, leg, 'step', i + 2, set(a) ^ set(b))
        for k in a:
            assert torch.equal(a[k], b[k]), (case, leg, 'step', i + 2, k, a[k].tolist(), b[k].tolist())
    r, g = ref['snap3'], got['snap3']
    assert set(r['state']) == set(g['state']) and set(r) == set(g)
    for k in r['state']:
        same_tensor((case, leg, k), r['state'][k], g['state'][k])
    assert len(r['groups']) == len(g['groups'])
    for i, (x, y) in enumerate(zip(r['groups'], g['groups'])):
        for k in x:
            same_tensor((case, leg, 'group', i, k), x[k], y[k])
    for k in NORM_STATS:
        same_tensor((case, leg, 'rewnorm', k), r['rewnorm'][k], g['rewnorm'][k])
    if 'ema_vals' in r:
        same_tensor((case, leg, 'ema_vals'), r['ema_vals'], g['ema_vals'])
    assert ref['action'].shape == got['action'].shape and np.array_equal(ref['action'], got['action']), (case, leg, ref['action'], got['action'])


def check_leg(case, leg, out):
    """host counters, and what keeps the comparison from passing vacuously"""
    s1, s3 = out['snap1'], out['snap3']
    assert len(out['mets']) == STEPS - 1
    assert s3['steps'] == [STEPS * n for n in out['per_iter']], (case, leg, s3['steps'])
    assert [int(g['step_dev']) for g in s3['groups']] == s3['steps'], (case, leg)
    assert s3['updates'] == STEPS and s1['updates'] == 1, (case, leg, s3['updates'])
    assert s1['steps'] == out['per_iter'], (case, leg, s1['steps'])
    for i, (x, y) in enumerate(zip(s1['groups'], s3['groups'])):
        assert not torch.equal(x['flat'], y['flat']), (case, leg, 'group', i, 'did not move between step 1 and step 3')
    if case == 'p2e_v2':
        assert not torch.equal(s1['rewnorm']['mag'], s3['rewnorm']['mag']), (case, leg, 'StreamNorm.mag did not advance')
    assert all(bool(torch.isfinite(v).all()) for m in out['mets'] for v in m.values()), (case, leg)
    assert np.isfinite(out['action']).all()


@pytest.mark.parametrize('case,route', PARAMS, ids=[f'{c}-{r}' for c, r in PARAMS])
def test_three_steps_eager_replay_resume(case, route, monkeypatch):
    from genrl_amd import planes
    from genrl_amd.agent import dreamer_utils as common
    if route == 'fp32':
        monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '1000000')
    # the routes the shapes are chosen for: 64-row stages on plane operands, weight gradients on the plane kernel -- or neither
    assert common.planes_route(B * T) == (route == 'planes')
    assert planes.tn_ok(B * T, 32, 32, 32)
    batches, obs = make_batches(case)
    cache = {}                                     # one noise tensor per site, shared by all legs
    try:
        eager = eager_leg(case, batches, obs, cache)
        assert eager['live'], (case, 'the configured route is not the one that ran')
        check_leg(case, 'eager', eager)
        legs = {'resume': resume_leg}
        if case != 'genrl':                        # (its replay is pinned by test_gpu_api.py::test_graph_replay_bit_exact)
            legs['replay'] = replay_leg
        for leg in sorted(legs):
            out = legs[leg](case, batches, obs, cache)
            check_leg(case, leg, out)
            for i, (x, y) in enumerate(zip(eager['snap1']['groups'], out['snap1']['groups'])):
                same_tensor((case, leg, 'after step 1: group', i), x['flat'], y['flat'])
            compare(case, leg, eager, out)
    finally:
        cache.clear()
        gc.collect()


@pytest.mark.parametrize('case', ['v3', 'genrl'])
def test_checkpoint_taken_under_replay_resumes_eagerly(case):
    """train.py saves the whole agent every so often, also while a GraphedStep replays its iteration; a run resumed from
    that file with eager steps must go on exactly as the eager run does -- the slow-critic copy after step 3 included, which under replay is
    the GraphedStep's job and in the resumed run the agent's own again (DreamerAgent's acting behaviour, GenRLAgent's imagination behaviour)"""
    batches, obs = make_batches(case)
    cache = {}
    try:
        eager = eager_leg(case, batches, obs, cache)
        check_leg(case, 'eager', eager)
        out = replay_then_resume_leg(case, batches, obs, cache)
        check_leg(case, 'replay, checkpoint, resume', out)
        compare(case, 'replay, checkpoint, resume', eager, out)
    finally:
        cache.clear()
        gc.collect()
