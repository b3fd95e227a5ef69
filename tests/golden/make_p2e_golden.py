"""Generate tests/golden/p2e_tiny.npz from the reference's Plan2Explore.  Needs a checkout of mazpie/genrl where ref_harness.REF points
(ref_harness imports it from there and refuses to run without it); the tests read only the stored file:

    python tests/golden/make_p2e_golden.py

Plan2Explore of mazpie/genrl (agent/plan2explore.py) on conf/defaults/dreamer_v3.yaml + conf/env/dmc_pixels.yaml +
agent/plan2explore.yaml at tiny widths (detgen.dreamer_tiny_overrides), B2 x T18, A = 6, imported through ref_harness; weights from
detgen.det_state_dict, noise replayed through NoiseTape as make_golden.run_dreamer does.  Two runs of Plan2Explore.update:
  lr = 0 : every metric, posterior / imagined latent indices, the (H+1, N, 1) intrinsic reward, the inputs of the two disagreement
           calls (feat / action / embed), every gradient of the disagreement, actor and critic groups;
  real optimiser settings : every trained parameter's change after one step, NOT the parameters themselves (146 fp32 tensors would pass
           the size limit of a committed file): 'delta.<name>' = (after - before) / lr of its group, rounded to 1/256 and stored as
           float16, i.e. the step to within lr / 512 per element; the test's bounds carry that rounding (test_gpu_p2e.py).
Inputs and outputs only; no reference text is stored."""
import os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen

torch.set_num_threads(8)
B, T, A, SEED = 2, 18, 6, 5


def make_ref_p2e(**over):
    m = rh.ref_modules()
    import agent.plan2explore as p2e
    cfg = rh.AD()
    cfg.update(rh._load(f'{rh.REF}/conf/defaults/dreamer_v3.yaml'))
    cfg.update(rh._load(f'{rh.REF}/conf/env/dmc_pixels.yaml'))
    a = rh._load(f'{rh.REF}/agent/plan2explore.yaml')
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
    return p2e.Plan2Explore(name=name, cfg=cfg, obs_space=obs, act_spec=rh.Spec((A,), np.float32))


def group_of(name):
    """the optimiser settings a parameter is stepped with (None: a buffer)"""
    if name.startswith(('wm.', 'disagreement.')):
        return 'model_opt'
    if '.actor.' in name:
        return 'actor_opt'
    if '.critic.' in name:
        return 'critic_opt'
    return None


def run(lr_zero):
    over = dict(detgen.dreamer_tiny_overrides())
    if lr_zero:
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            over[k] = dict(lr=0.0, wd=0.0)
    ag = make_ref_p2e(**over)
    for d_ in ag._acting_behavior._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
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
    grads, phase, cap = {}, ['wm'], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_ud, orig_ir, orig_cl, orig_wm = ag.update_disagreement, ag.compute_intr_reward, ag._acting_behavior.critic_loss, ag.wm.update

    def wm_hook(*a, **k):
        state, outputs, mets = orig_wm(*a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        return state, outputs, mets

    def ud_hook(obs, action, next_obs, step):
        phase[0] = 'disagreement'
        cap['train_feat'], cap['train_action'], cap['train_embed'] = obs.detach().clone(), action.detach().clone(), next_obs.detach().clone()
        return orig_ud(obs, action, next_obs, step)

    def ir_hook(seq):
        phase[0] = 'actor'
        r = orig_ir(seq)
        cap['imag_feat'], cap['imag_action'] = seq['feat'].detach().clone(), seq['action'].detach().clone()
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        cap['intr_reward'] = r.detach().clone()
        return r

    def cl_hook(*a, **k):
        phase[0] = 'critic'
        return orig_cl(*a, **k)
    ag.update_disagreement, ag.compute_intr_reward, ag._acting_behavior.critic_loss, ag.wm.update = ud_hook, ir_hook, cl_hook, wm_hook
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with rh.inject_noise(tape):
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    out = {}
    if lr_zero:
        for k, v in mets.items():
            out[f'metrics.{k}'] = np.asarray(torch.as_tensor(v).detach().numpy())
        for k, v in cap.items():
            out[k] = v.numpy()
        for ph in ('disagreement', 'actor', 'critic'):
            for n, g in grads[ph].items():
                out[f'grad.{ph}.{n}'] = g.numpy()
        for n, v in det.items():
            out[f'shape.{n}'] = np.array(v.shape, np.int64)
        out['meta'] = np.array([B, T, A, S, K, H, SEED])
        out['torch_version'] = np.array(torch.__version__)
    else:
        # (deltas in units of the group's learning rate, rounded to 1/256 of it, as float16: Adam's first step is ~lr sign(g), the tests'
        # bounds are 2 lr per element and 5 % in L1 -- a rounding of at most lr / 512 per element, ~0.1 % in L1, is far below both,
        # and the fixture stays within the size limit)
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
    o = run(True)
    o.update(run(False))
    path = f'{HERE}/p2e_tiny.npz'
    np.savez_compressed(path, **o)
    print('p2e_tiny.npz', len(o), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
