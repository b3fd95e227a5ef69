"""Generate tests/golden/discrete_tiny.npz from the reference's DreamerAgent with `discrete_actions`.  Needs a checkout of mazpie/genrl where
ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only the stored file:

    python tests/golden/make_discrete_golden.py

Two DreamerAgent.update cases at tiny widths (detgen.dreamer_tiny_overrides), precision 32, B2 x T18, A = 6, lr = 0, weights from
detgen.det_state_dict, noise replayed through NoiseTape as make_v2_golden.py does:

  'v3dyn.*' : conf/defaults/dreamer_v3.yaml + discrete_actions + actor_grad dynamics
  'v2rf.*'  : conf/defaults/dreamer_v2.yaml + discrete_actions + actor_grad reinforce

The actor's head is DistLayer 'onehot' (agent/dreamer.py:332-333): its OneHotDist.sample goes through torch.multinomial, replayed as the
exponential race exactly as the latents are (ref_harness.inject_noise); the throw-away sample of WorldModel.imagine (agent/dreamer.py:259-260)
consumes the site imag.act_q0 first, then every step imag.act_q[h] and imag.step_q[h].  The tape must be fully consumed.

Condition on the seed: for EVERY race replayed here (posterior, prior, imagined latents, actions, act()) the two largest ratios p / q differ
by at least 1e-3 relative -- asserted below on the CPU --, so that the float32 summation order of another implementation cannot flip a draw.

Per case: every metric; posterior / imagined latent indices; the imagined one-hot actions; the rollout's logits at states 0 .. H-2 with the
probabilities, log-probabilities of the taken actions and entropies the reference's policy gives on them; the lambda-returns and the baseline;
every gradient of the actor and critic groups (grad_rows of make_v2_golden.py: more than 4096 elements -> every fourth index of the first
dimension); the shape of every state_dict entry.  'act.*': DreamerAgent.act of the v3dyn agent on one frame, eval mode (the mixed
probabilities) and sampling mode (a one-hot action), each from an empty state, with the posterior's latent indices.
Arrays only; no reference text is stored.  The file must be no larger than v2_tiny.npz."""
import os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen
import make_v2_golden as mv2

torch.set_num_threads(8)
B, T, A = 2, 18, 6
SEED = 8                # (seeds 5, 6, 7 miss the margin condition below: 4.6e-4, 1.8e-4, 2.9e-4)
MARGIN = 1e-3
CASES = {'v3dyn': ('dreamer_v3', 'dynamics'), 'v2rf': ('dreamer_v2', 'reinforce')}
margins = []


class inject_with_margin(rh.inject_noise):
    """inject_noise whose one-hot race also records how far apart its two best candidates are"""
    def __enter__(self):
        tape = super().__enter__()
        m = rh.ref_modules()
        F = torch.nn.functional

        def sample(self_, sample_shape=(), seed=None):
            probs = torch.distributions.OneHotCategorical.probs.fget(self_)
            p2 = probs.reshape(-1, probs.shape[-1])
            q = tape.draw('exp', p2.shape, lambda: torch.empty_like(p2).exponential_(1))
            ratio = (p2.detach().double() / q.double())
            top = torch.topk(ratio, 2, -1).values
            margins.append(float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
            idx = torch.argmax(p2.detach() / q, -1)
            assert bool((idx == ratio.argmax(-1)).all())
            s = F.one_hot(idx, probs.shape[-1]).to(probs).reshape(probs.shape)
            return s + (probs - probs.detach())
        m.common.OneHotDist.sample = sample
        return tape


def make_agent(case):
    defaults, actor_grad = CASES[case]
    over = dict(detgen.dreamer_tiny_overrides(), discrete_actions=True, actor_grad=actor_grad)
    for k in ('model_opt', 'actor_opt', 'critic_opt'):
        over[k] = dict(lr=0.0, wd=0.0)
    ag = rh.make_ref_dreamer(B, T, A=A, **over) if defaults == 'dreamer_v3' else mv2.make_ref('dreamer', **over)
    ac = ag._acting_behavior
    assert ac.actor._out._dist == 'onehot' and ac.actor_grad == actor_grad
    for d_ in ac._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, SEED)
    ag.load_state_dict(det)
    return ag, det


def action_noise(H, N):
    return (detgen.det_noise('imag.act_q0', (N, A), 'exp', SEED), detgen.det_noise('imag.act_q', (H, N, A), 'exp', SEED))


def run(case):
    ag, det = make_agent(case)
    ac = ag._acting_behavior
    S, K, H = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete, ag.cfg.imag_horizon
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=SEED)
    q0, qa = action_noise(H, B * T)
    tape = []
    for t in range(T):
        tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
    tape.append(('exp', q0))
    for h in range(H):
        tape.append(('exp', qa[h])); tape.append(('exp', noise['imag']['step_q'][h]))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n for n, p in ag.named_parameters()}
    grads, phase, cap = {}, ['model'], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_wm, orig_tg, orig_cl = ag.wm.update, ac.target, ac.critic_loss

    def wm_hook(data, *a, **k):
        state, outputs, mets = orig_wm(data, *a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        target, mets, baseline = orig_tg(seq)
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        act = seq['action'].detach()
        assert bool(((act == 0) | (act == 1)).all()) and bool((act[1:].sum(-1) == 1).all()) and float(act[0].abs().max()) == 0.0
        cap['imag_action'] = act.to(torch.int8)
        with torch.no_grad():
            got = []
            hook = ac.actor._out._out.register_forward_hook(lambda mod, inp, out: got.append(out.detach().clone()))
            policy = ac.actor(seq['feat'][:-2].detach())
            hook.remove()
            cap['logits'] = got[0]
            cap['probs'] = policy.probs.clone()
            cap['logp'] = policy.log_prob(act[1:-1]).clone()
            cap['ent'] = policy.entropy().clone()
            cap['imag_target'] = target.detach().clone()
            cap['imag_baseline'] = baseline.detach().clone()
            cap['imag_weight'] = seq['weight'].detach().clone()
        return target, mets, baseline

    def cl_hook(seq, target):
        phase[0] = 'critic'
        cap['critic_target_in'] = target.detach().clone()
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    # the replayed actions of a discrete-action environment are one-hot (collect_data.py:204-205)
    g = np.random.Generator(np.random.PCG64([SEED, 77]))
    batch['action'] = np.eye(A, dtype=np.float32)[g.integers(0, A, size=(B, T))]
    cap['batch_action_idx'] = torch.from_numpy(batch['action'].argmax(-1).astype(np.int8))
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with inject_with_margin(tape):
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
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
    out[f'{pre}meta'] = np.array([B, T, A, S, K, H, SEED])
    return out


def run_act():
    ag, det = make_agent('v3dyn')
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    obs = {'observation': batch['observation'][0, 3], 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    out = {}
    for mode, ev in (('eval', True), ('sample', False)):
        tape = [('exp', detgen.det_noise(f'act.{mode}.prior_q', (S, K), 'exp', SEED)),
                ('exp', detgen.det_noise(f'act.{mode}.post_q', (S, K), 'exp', SEED))]
        if not ev:
            tape.append(('exp', detgen.det_noise(f'act.{mode}.act_q', (1, A), 'exp', SEED)))
        tape = rh.NoiseTape('replay', tape)
        with inject_with_margin(tape), torch.no_grad():
            action, (latent, _) = ag.act(obs, None, 0, ev, None)
        assert tape.pos == len(tape.tape), (mode, tape.pos, len(tape.tape))
        out[f'act.{mode}.action'] = np.asarray(action)
        out[f'act.{mode}.latent_idx'] = latent['stoch'].argmax(-1).to(torch.int16).numpy()
    assert set(np.unique(out['act.sample.action'])) == {0.0, 1.0}
    return out


def main():
    o = {}
    for case in CASES:
        o.update(run(case))
    o.update(run_act())
    print('seed', SEED, 'smallest relative margin between the two best candidates of a race:', min(margins), 'over', len(margins), 'draws')
    assert min(margins) >= MARGIN, (SEED, min(margins))
    o['race_margin'] = np.array(min(margins))
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/discrete_tiny.npz'
    np.savez_compressed(path, **o)
    print('discrete_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
