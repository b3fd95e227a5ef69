"""Three optimiser steps of GenRLAgent with the connector's switches set -- all four, and `detached_post: False` alone -- three ways,
compared bit for bit: eagerly, as one eager step followed by two hipGraph replays (graph.GraphedStep), and resumed from a pickled agent
after the first step.  The legs, the snapshot and the comparison are test_gpu_step_matrix.py's (metrics of the later steps, every
state_dict entry, the optimiser groups' flat parameters / Adam moments / device step counters, the return EMA, the action `act()` returns);
this file adds the two configurations to the table those legs build from.  With the connector trained end to end the world model's
optimiser has ONE group that holds the connector's parameters too, stepped once per iteration, and nothing runs on the `detached` side
stream; the dropout's keep flags come from the noise site 'conn.drop', which `noise.static` fixes like every other site, so a replay
consumes what the eager run consumed."""
import gc

import pytest

import detgen
import test_gpu_step_matrix as SM

pytestmark = pytest.mark.gpu

SWITCHES = {
    'conn_all': dict(connector=dict(temporal_embeds=True, token_dropout=0.25, detached_post=False), connector_rssm=dict(learn_initial=False)),
    'conn_e2e': dict(connector=dict(detached_post=False)),
}


def _live(name):
    def live(ag, m):
        conn, sw = ag.wm.connector, SWITCHES[name]
        return ('connector' in ag.wm.e2e_update_fns and not ag.wm.detached_update_fns and len(ag.wm.model_opt._groups) == 1
                and {id(q) for q in conn.parameters()} <= {id(q) for q in ag.wm.model_opt._groups[0].params}
                and 'connector_kl' in m and 'connector_model_loss' not in m and any(k.startswith('imag_') for k in m)
                and conn.temporal_embeds == sw['connector'].get('temporal_embeds', False)
                and conn.token_dropout == sw['connector'].get('token_dropout', 0)
                and hasattr(conn, 'initial_state_pred') == sw.get('connector_rssm', {}).get('learn_initial', True))
    return live


def add_case(name, monkeypatch):
    """put `name` into the table test_gpu_step_matrix's legs read, built like its 'genrl' case plus the switches"""
    from genrl_amd import config
    cases = dict(SM._cases(), **{name: ('genrl', None, {}, None, _live(name))})
    build, step_fn = SM.build, SM.step_fn

    def build_case(case):
        if case != name:
            return build(case)
        over = SM._merge(config.tiny_overrides(), dict(slow_target_update=2), SWITCHES[name])
        ag = config.make_agent(config.default_cfg(SM.B, SM.T, device='cuda', **over))
        ag.wm.viclip_model = SM._bench().TextStub()
        sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in ag.state_dict().items()}, SM.SEED)
        ag.load_state_dict({k: v.cuda() for k, v in sd.items()})
        return ag
    monkeypatch.setattr(SM, '_cases', lambda: cases)
    monkeypatch.setattr(SM, 'build', build_case)
    monkeypatch.setattr(SM, 'step_fn', lambda case: SM._bench().one_step if case == name else step_fn(case))


@pytest.mark.parametrize('name', sorted(SWITCHES))
def test_three_steps_eager_replay_resume(name, monkeypatch):
    from genrl_amd import ops
    add_case(name, monkeypatch)
    drops, orig = [], ops.tf_inputs
    monkeypatch.setattr(ops, 'tf_inputs', lambda *a: (drops.append(1), orig(*a))[1])
    batches, obs = SM.make_batches(name)
    cache = {}                                     # one noise tensor per site, shared by all legs
    try:
        eager = SM.eager_leg(name, batches, obs, cache)
        assert eager['live'], (name, 'the configured switches are not the ones that ran')
        assert eager['per_iter'] == [1, 1, 1], eager['per_iter']             # one world-model group (connector inside), actor, critic
        assert (len(drops) == SM.STEPS) == (name == 'conn_all') and (not drops) == (name == 'conn_e2e')
        assert ('conn.drop', (SM.T, SM.B)) in cache if name == 'conn_all' else not any(k[0] == 'conn.drop' for k in cache)
        SM.check_leg(name, 'eager', eager)
        for leg, run in (('replay', SM.replay_leg), ('resume', SM.resume_leg)):
            out = run(name, batches, obs, cache)
            SM.check_leg(name, leg, out)
            for i, (x, y) in enumerate(zip(eager['snap1']['groups'], out['snap1']['groups'])):
                SM.same_tensor((name, leg, 'after step 1: group', i), x['flat'], y['flat'])
            SM.compare(name, leg, eager, out)
    finally:
        cache.clear()
        gc.collect()
