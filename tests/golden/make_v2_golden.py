"""Generate tests/golden/v2_tiny.npz from the reference's DreamerAgent and Plan2Explore on the DreamerV2 defaults.  Needs a checkout of
mazpie/genrl where ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only the
stored file:

    python tests/golden/make_v2_golden.py

conf/defaults/dreamer_v2.yaml + conf/env/dmc_pixels.yaml + agent/dreamer.yaml | agent/plan2explore.yaml at tiny widths
(detgen.dreamer_tiny_overrides), precision 32, B2 x T18, A = 6; weights from detgen.det_state_dict, noise replayed through NoiseTape as
make_p2e_golden.py does.  One RNG site is new: TruncatedNormal.sample (tools/utils.py:114-123) draws through `_standard_normal` in the
namespace of tools/utils.py, patched here to read the tape ('normal'); the throw-away sample of WorldModel.imagine (agent/dreamer.py:260)
consumes imag.act_eps0 first.  The tape must be fully consumed.

  'dreamer.*', lr = 0 : DreamerAgent.update: every metric, posterior / imagined latent indices, the imagined actions, every gradient of the
           model, actor and critic groups, and the inputs / outputs the plain-torch restatement (tests/v2_restatement.py) is checked on:
           the posterior features with the reward head's log-likelihood, one decoded frame with its log-likelihood, the first two imagined
           feature rows, the rollout's rewards, slow-critic values, lambda-returns, critic outputs and the returns the critic is trained on.
  'p2e.*', lr = 0     : Plan2Explore.update: metrics, the (H+1, N, 1) intrinsic reward, the gradients of the disagreement, actor and critic
           groups.
  'delta.*'           : one Plan2Explore.update with the real optimiser settings: (after - before) / lr of the parameter's group, rounded to
           1/256 and stored as float16, exactly as p2e_tiny.npz does (make_p2e_golden.py).
  'dreamer.shape.*' / 'p2e.shape.*' : the shape of every state_dict entry of the two agents; 'dreamer.metric_keys' / 'p2e.metric_keys'.

The file must stay below the size of p2e_tiny.npz, and the two agents' float32 gradients alone (92 348 model + 117 760 disagreement
parameters) would pass it: a gradient of more than 4096 elements is stored on every fourth index of its first dimension (grad_rows: rows
0, 4, 8, ... -- output units of a Linear, input channels of the decoder's first transposed convolution), every other gradient whole.
Arrays only; no reference text is stored."""
import os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen

torch.set_num_threads(8)
B, T, A, SEED = 2, 18, 6, 5


def grad_rows(x):
    """what the fixture keeps of a gradient: all of it up to 4096 elements, else every fourth index of the first dimension"""
    return x if x.size <= 4096 else np.ascontiguousarray(x[::4])


def make_ref(kind, **over):
    m = rh.ref_modules()
    import agent.plan2explore as p2e
    cfg = rh.AD()
    cfg.update(rh._load(f'{rh.REF}/conf/defaults/dreamer_v2.yaml'))
    cfg.update(rh._load(f'{rh.REF}/conf/env/dmc_pixels.yaml'))
    a = rh._load(f'{rh.REF}/agent/{kind}.yaml')
    for k in ('_target_', 'cfg', 'obs_space', 'act_spec'):
        a.pop(k)
    name = a.pop('name')
    cfg.update(a)
    cfg.update(device='cpu', precision=32, batch_size=B, batch_length=T, task='walker_walk')
    for k, v in over.items():
        if isinstance(v, dict) and isinstance(cfg.get(k), dict):
            cfg[k].update(rh._conv(v))
        else:
            cfg[k] = rh._conv(v)
    obs = dict(observation=rh.Spec((3, 64, 64), np.uint8), is_first=rh.Spec((), bool), is_last=rh.Spec((), bool),
               is_terminal=rh.Spec((), bool))
    torch.manual_seed(0)
    cls = p2e.Plan2Explore if kind == 'plan2explore' else m.dreamer.DreamerAgent
    return cls(name=name, cfg=cfg, obs_space=obs, act_spec=rh.Spec((A,), np.float32))


def group_of(name):
    """the optimiser settings a parameter is stepped with (None: a buffer)"""
    if name.startswith(('wm.', 'disagreement.')):
        return 'model_opt'
    if '.actor.' in name:
        return 'actor_opt'
    if '.critic.' in name:
        return 'critic_opt'
    return None


class tape_trunc_normal:
    """TruncatedNormal.sample's `_standard_normal` (the name bound in tools/utils.py) reads the tape"""
    def __init__(self, tape):
        self.tape = tape

    def __enter__(self):
        import tools.utils as tu
        self.tu, self.orig = tu, tu._standard_normal
        tu._standard_normal = lambda shape, dtype=None, device=None: self.tape.draw('normal', tuple(shape), lambda: self.orig(shape, dtype=dtype, device=device))

    def __exit__(self, *a):
        self.tu._standard_normal = self.orig


def run(kind, lr_zero):
    over = dict(detgen.dreamer_tiny_overrides())
    if lr_zero:
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            over[k] = dict(lr=0.0, wd=0.0)
    ag = make_ref(kind, **over)
    ac = ag._acting_behavior
    for d_ in ac._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, SEED)
    ag.load_state_dict(det)
    S, K, H = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete, ag.cfg.imag_horizon
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=SEED)
    tape = []
    for t in range(T):
        tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
    tape.append(('normal', noise['imag']['act_eps0']))
    for h in range(H):
        tape.append(('normal', noise['imag']['act_eps'][h])); tape.append(('exp', noise['imag']['step_q'][h]))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n for n, p in ag.named_parameters()}
    grads, phase, cap = {}, ['model'], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_wm, orig_tg, orig_cl = ag.wm.update, ac.target, ac.critic_loss
    p2e = kind == 'plan2explore'

    def wm_hook(data, *a, **k):
        state, outputs, mets = orig_wm(data, *a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        if not p2e:
            with torch.no_grad():
                cap['post_feat'] = outputs['feat'].detach().clone()
                cap['like_reward'] = outputs['likes']['reward'].detach().clone()
                cap['like_observation'] = outputs['likes']['observation'].detach().clone()
                cap['recon00'] = ag.wm.heads['decoder'](outputs['feat'].detach()[:1, :1])['observation'].mean[0, 0].clone()
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        target, mets, baseline = orig_tg(seq)
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        cap['imag_action'] = seq['action'].detach().clone()
        if not p2e:
            with torch.no_grad():
                cap['imag_feat01'] = seq['feat'].detach()[:2].clone()
                cap['imag_reward'] = seq['reward'].detach().clone()
                cap['imag_value'] = ac._target_critic(seq['feat'].detach()).mean.clone()
                cap['imag_target'] = target.detach().clone()
        return target, mets, baseline

    def cl_hook(seq, target):
        phase[0] = 'critic'
        if not p2e:
            with torch.no_grad():
                cap['critic_out'] = ac.critic(seq['feat'][:-1].detach()).mean.clone()
                # (with `reward_ema: False` the actor loss's `objective += ent_scale * ent` works in place on a view of the returns,
                # agent/dreamer.py:410-423: the critic regresses onto returns that carry the entropy bonus from step 1 on)
                cap['critic_target_in'] = target.detach().clone()
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    if p2e:
        orig_ud, orig_ir = ag.update_disagreement, ag.compute_intr_reward

        def ud_hook(obs, action, next_obs, step):
            phase[0] = 'disagreement'
            return orig_ud(obs, action, next_obs, step)

        def ir_hook(seq):
            r = orig_ir(seq)
            cap['intr_reward'] = r.detach().clone()
            return r
        ag.update_disagreement, ag.compute_intr_reward = ud_hook, ir_hook
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with rh.inject_noise(tape), tape_trunc_normal(tape):
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    out = {}
    pre = 'p2e.' if p2e else 'dreamer.'
    if lr_zero:
        for k, v in mets.items():
            out[f'{pre}metrics.{k}'] = np.asarray(torch.as_tensor(v).detach().numpy())
        out[f'{pre}metric_keys'] = np.array(sorted(mets))
        for k, v in cap.items():
            out[pre + k] = v.numpy()
        for ph in (('disagreement', 'actor', 'critic') if p2e else ('model', 'actor', 'critic')):
            for n, g in grads[ph].items():
                out[f'{pre}grad.{ph}.{n}'] = grad_rows(g.numpy())
        for n, v in det.items():
            out[f'{pre}shape.{n}'] = np.array(v.shape, np.int64)
        out['meta'] = np.array([B, T, A, S, K, H, SEED])
        out['torch_version'] = np.array(torch.__version__)
    else:
        # (deltas in units of the group's learning rate, rounded to 1/256 of it, as float16: see make_p2e_golden.py)
        for n, v in ag.state_dict().items():
            if '._target_critic.' in n:        # (no optimiser group: the first update hard-copies the critic into it; nothing to store)
                continue
            d = (v.detach() - det[n]).double()
            grp = group_of(n)
            out[f'delta.{n}'] = (np.round((d / ag.cfg[grp]['lr']).numpy() * 256) / 256).astype(np.float16) if grp else d.numpy().astype(np.float32)
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            out[f'opt.{k}'] = np.array([ag.cfg[k]['lr'], ag.cfg[k]['eps'], ag.cfg[k]['clip'], ag.cfg[k]['wd']], np.float64)
    return out


def main():
    o = run('dreamer', True)
    o.update(run('plan2explore', True))
    o.update(run('plan2explore', False))
    path = f'{HERE}/v2_tiny.npz'
    np.savez_compressed(path, **o)
    print('v2_tiny.npz', len(o), os.path.getsize(path), 'bytes; p2e_tiny.npz', os.path.getsize(f'{HERE}/p2e_tiny.npz'))


if __name__ == '__main__':
    main()
