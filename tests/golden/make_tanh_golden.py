"""Generate tests/golden/tanh_tiny.npz from the reference's DreamerAgent with `actor: {dist: tanh_normal}`.  Needs a checkout of mazpie/genrl
where ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only the stored file:

    python tests/golden/make_tanh_golden.py

Two DreamerAgent.update cases at tiny widths (detgen.dreamer_tiny_overrides), precision 32, B2 x T18, A = 6, lr = 0, weights from
detgen.det_state_dict, noise replayed through NoiseTape as make_discrete_golden.py does:

  'v3t.*' : conf/defaults/dreamer_v3.yaml + actor {dist: tanh_normal}, actor_ent 3e-4, reward_ema True
  'v2t.*' : conf/defaults/dreamer_v2.yaml + actor {dist: tanh_normal, init_std: 1.0}, that file's reward_ema False

The actor's head is DistLayer 'tanh_normal' (agent/dreamer_utils.py:824-829): SquashedNormal in SampleDist.  All of its noise goes through
Normal.rsample, which ref_harness.inject_noise already replays: the throw-away sample of WorldModel.imagine (agent/dreamer.py:259-260) consumes
imag.act_eps0 first, then every step imag.act_eps[h] and imag.step_q[h], and the actor loss (agent/dreamer.py:421) draws the
(K, H-1, N, A) entropy noise once -- stored under the name actor.ent_eps with its first two axes merged, (K (H-1), N, A).  The tape must be
fully consumed.

Conditions on the seed, asserted below on the CPU: for EVERY categorical race replayed here the two largest ratios p / q differ by at least
1e-3 relative (as make_discrete_golden.py), and every imagined or acted action has |action| < 1 - 1e-5, so that no float32 tanh sits at +-1.
Seeds are tried from FIRST_SEED upwards until both hold; the seed and the margins are stored.

Per case: every metric; posterior / imagined latent indices; the imagined actions; the rollout's raw head outputs at states 0 .. H-2 with the
base Normal's mean and std and the per-row entropy the reference's policy gives on them; the lambda-returns, the baseline and the returns the
critic is trained on; every gradient of the actor and critic groups (grad_rows of make_v2_golden.py); the shape of every state_dict entry.
'act.*': DreamerAgent.act of the v3t agent on one frame, eval mode (SampleDist.mean over a replayed (100, 1, A) draw) and sampling mode, each
from an empty state, with the posterior's latent indices and the head's raw output.  Arrays only; no reference text is stored.  The file must be no larger than
v2_tiny.npz."""
import os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen
import make_v2_golden as mv2
import make_discrete_golden as mdg

torch.set_num_threads(8)
B, T, A = 2, 18, 6
K = 100                 # SampleDist's samples (agent/dreamer_utils.py:29)
FIRST_SEED = 5          # (seeds 5 .. 9 miss the race margin: 2.7e-4, 1.7e-4, 8.0e-5, 6.4e-5, 1.1e-5; seed 10 holds both conditions)
MARGIN, ACTION_MARGIN = 1e-3, 1e-5
CASES = {'v3t': ('dreamer_v3', dict(actor=dict(dist='tanh_normal'), actor_ent=3e-4, reward_ema=True)),
         'v2t': ('dreamer_v2', dict(actor=dict(dist='tanh_normal', init_std=1.0)))}


def make_agent(case, seed):
    defaults, extra = CASES[case]
    over = dict(detgen.dreamer_tiny_overrides())
    for k, v in extra.items():
        over[k] = dict(over.get(k, {}), **v) if isinstance(v, dict) else v
    for k in ('model_opt', 'actor_opt', 'critic_opt'):
        over[k] = dict(lr=0.0, wd=0.0)
    ag = rh.make_ref_dreamer(B, T, A=A, **over) if defaults == 'dreamer_v3' else mv2.make_ref('dreamer', **over)
    ac = ag._acting_behavior
    assert ac.actor._out._dist == 'tanh_normal' and ac.actor_grad == 'dynamics'
    assert bool(ag.cfg.reward_ema) == (case == 'v3t') and ac.actor._out._init_std == extra['actor'].get('init_std', 0.0)
    for d_ in ac._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, seed)
    ag.load_state_dict(det)
    return ag, det


def run(case, seed, action_margins):
    ag, det = make_agent(case, seed)
    m = rh.ref_modules()
    ac = ag._acting_behavior
    S, Kc, H = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete, ag.cfg.imag_horizon
    N = B * T
    noise = detgen.iteration_noise(B, T, S, Kc, A, H, seed=seed)
    ent_eps = detgen.det_noise('actor.ent_eps', (K * (H - 1), N, A), 'normal', seed)
    tape = []
    for t in range(T):
        tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
    tape.append(('normal', noise['imag']['act_eps0']))
    for h in range(H):
        tape.append(('normal', noise['imag']['act_eps'][h])); tape.append(('exp', noise['imag']['step_q'][h]))
    tape.append(('normal', ent_eps.reshape(K, H - 1, N, A)))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n for n, p in ag.named_parameters()}
    grads, phase, cap = {}, ['model'], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_wm, orig_tg, orig_cl = ag.wm.update, ac.target, ac.critic_loss
    orig_ent = m.common.SampleDist.entropy
    heads = {}

    def wm_hook(data, *a, **k):
        state, outputs, mets = orig_wm(data, *a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        target, mets, baseline = orig_tg(seq)
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        cap['imag_action'] = seq['action'].detach().clone()
        cap['imag_target'] = target.detach().clone()
        cap['imag_baseline'] = baseline.detach().clone()
        cap['imag_weight'] = seq['weight'].detach().clone()
        return target, mets, baseline

    def ent_hook(self_):           # the policy of the actor loss: the last evaluation of the two head Linears is its own
        ent = orig_ent(self_)
        base = self_._dist.base_dist
        cap['raw'] = torch.cat([heads['out'], heads['std']], -1)
        cap['mean'], cap['std'], cap['ent'] = base.loc.detach().clone(), base.scale.detach().clone(), ent.detach().clone()
        return ent

    def cl_hook(seq, target):
        phase[0] = 'critic'
        cap['critic_target_in'] = target.detach().clone()
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    hooks = [ac.actor._out._out.register_forward_hook(lambda mod, inp, out: heads.__setitem__('out', out.detach().clone())),
             ac.actor._out._std.register_forward_hook(lambda mod, inp, out: heads.__setitem__('std', out.detach().clone()))]
    batch = detgen.det_batch(B, T, A=A, seed=seed)
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    m.common.SampleDist.entropy = ent_hook
    try:
        with mdg.inject_with_margin(tape):
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
        m.common.SampleDist.entropy = orig_ent
        for h_ in hooks:
            h_.remove()
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    assert cap['raw'].shape == (H - 1, N, 2 * A) and cap['ent'].shape == (H - 1, N)
    action_margins.append(1.0 - float(cap['imag_action'].abs().max()))
    out = {}
    pre = case + '.'
    for k, v in mets.items():
        out[f'{pre}metrics.{k}'] = np.asarray(torch.as_tensor(v).detach().numpy())
    out[f'{pre}metric_keys'] = np.array(sorted(mets))
    for k, v in cap.items():
        out[pre + k] = v.numpy()
    for ph in ('actor', 'critic'):
        for n, gr in grads[ph].items():
            out[f'{pre}grad.{ph}.{n}'] = mv2.grad_rows(gr.numpy())
    for n, v in det.items():
        out[f'{pre}shape.{n}'] = np.array(v.shape, np.int64)
    out[f'{pre}meta'] = np.array([B, T, A, S, Kc, H, seed])
    out[f'{pre}std_cfg'] = np.array([ac.actor._out._min_std, ac.actor._out._init_std, ag.cfg.actor_ent], np.float64)
    return out


def run_act(seed, action_margins):
    ag, det = make_agent('v3t', seed)
    S, Kc = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    batch = detgen.det_batch(B, T, A=A, seed=seed)
    obs = {'observation': batch['observation'][0, 3], 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    out, heads = {}, {}
    head = ag._acting_behavior.actor._out
    head._out.register_forward_hook(lambda mod, inp, o: heads.__setitem__('out', o.detach().clone()))
    head._std.register_forward_hook(lambda mod, inp, o: heads.__setitem__('std', o.detach().clone()))
    for mode, ev in (('eval', True), ('sample', False)):
        tape = [('exp', detgen.det_noise(f'act.{mode}.prior_q', (S, Kc), 'exp', seed)),
                ('exp', detgen.det_noise(f'act.{mode}.post_q', (S, Kc), 'exp', seed)),
                ('normal', detgen.det_noise(f'act.{mode}.act_eps', (K, 1, A) if ev else (1, A), 'normal', seed))]
        tape = rh.NoiseTape('replay', tape)
        with mdg.inject_with_margin(tape), torch.no_grad():
            action, (latent, _) = ag.act(obs, None, 0, ev, None)
        assert tape.pos == len(tape.tape), (mode, tape.pos, len(tape.tape))
        out[f'act.{mode}.action'] = np.asarray(action)
        out[f'act.{mode}.raw'] = torch.cat([heads['out'], heads['std']], -1).numpy()
        out[f'act.{mode}.latent_idx'] = latent['stoch'].argmax(-1).to(torch.int16).numpy()
        action_margins.append(1.0 - float(np.abs(action).max()))
    return out


def attempt(seed):
    del mdg.margins[:]
    action_margins = []
    o = {}
    for case in CASES:
        o.update(run(case, seed, action_margins))
    o.update(run_act(seed, action_margins))
    return o, min(mdg.margins), len(mdg.margins), min(action_margins)


def main():
    seed = FIRST_SEED
    while True:
        o, race, n, act = attempt(seed)
        print('seed', seed, 'smallest relative margin between the two best candidates of a race:', race, 'over', n, 'draws; smallest 1 - |action|:', act)
        if race >= MARGIN and act > ACTION_MARGIN:
            break
        seed += 1
    o['seed'] = np.array(seed)
    o['race_margin'] = np.array(race)
    o['action_margin'] = np.array(act)
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/tanh_tiny.npz'
    np.savez_compressed(path, **o)
    print('tanh_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
