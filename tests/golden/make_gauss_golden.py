"""Generate tests/golden/gauss_tiny.npz from the reference's DreamerAgent with continuous (Gaussian) latents, `rssm.discrete: False`.  Needs a
checkout of mazpie/genrl where ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only
the stored file:

    python tests/golden/make_gauss_golden.py

Two DreamerAgent.update cases at tiny widths (detgen.dreamer_tiny_overrides), precision 32, B2 x T18, A = 6, lr = 0, weights from
detgen.det_state_dict, noise replayed through NoiseTape as make_v2_golden.py does:

  'v2g.*' : conf/defaults/dreamer_v2.yaml + rssm.discrete False, stoch 6 (no multiple of 4; the reference's 30 would put the file past its
            size limit: the imagined mean / std / stoch alone are 3 x 16 x 36 x stoch floats), std_act softplus, decoder_inputs feat
  'v3g.*' : conf/defaults/dreamer_v3.yaml + rssm.discrete False, stoch 8, std_act sigmoid2

The latents' Normal.rsample is already read from the tape by ref_harness.inject_noise ('normal').  Order of consumption: per observed step the
prior's noise then the posterior's (wm.prior_eps[t], wm.post_eps[t], each (B, S)); the throw-away action sample of WorldModel.imagine
(imag.act_eps0); then per imagined step the action's noise and the prior's (imag.act_eps[h] (N, A), imag.step_eps[h] (N, S)).  The tape must
be fully consumed.  There is no race among continuous latents, so no condition on the seed.

Per case: every metric; the posterior's and the prior's mean / std / stoch with the raw outputs of `_obs_dist` and `_ensemble_img_dist[0]`
they were made from and the per-row KL; the imagined stoch / mean / std / actions with the raw prior-head outputs of the H imagined steps; the
lambda-returns; every gradient of the model, actor and critic groups (grad_rows of make_v2_golden.py: more than 4096 elements -> every fourth
index of the first dimension); the shape of every state_dict entry.  'act.*': DreamerAgent.act of the v3g agent on one frame from an empty
state, eval mode (the policy's mean) and sampling mode, with the posterior's mean / std / stoch.
Arrays only; no reference text is stored.  The file must be no larger than v2_tiny.npz."""
import contextlib
import os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen
import make_v2_golden as mv2

torch.set_num_threads(8)
B, T, A, SEED = 2, 18, 6, 5
CASES = {'v2g': ('dreamer_v2', dict(stoch=6, std_act='softplus'), dict(decoder_inputs='feat')),
         'v3g': ('dreamer_v3', dict(stoch=8, std_act='sigmoid2'), dict())}


def make_agent(case):
    defaults, rssm, extra = CASES[case]
    over = dict(detgen.dreamer_tiny_overrides(), **extra)
    over['rssm'] = dict(over['rssm'], discrete=False, **rssm)
    for k in ('model_opt', 'actor_opt', 'critic_opt'):
        over[k] = dict(lr=0.0, wd=0.0)
    ag = rh.make_ref_dreamer(B, T, A=A, **over) if defaults == 'dreamer_v3' else mv2.make_ref('dreamer', **over)
    assert not ag.wm.rssm._discrete and ag.wm.rssm._std_act == rssm['std_act'] and ag.wm.rssm._stoch == rssm['stoch']
    for d_ in ag._acting_behavior._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, SEED)
    ag.load_state_dict(det)
    return ag, det


def update_noise(S, H):
    n = lambda name, shape: detgen.det_noise(name, shape, 'normal', SEED)
    N = B * T
    return dict(prior=n('wm.prior_eps', (T, B, S)), post=n('wm.post_eps', (T, B, S)), act0=n('imag.act_eps0', (N, A)),
                act=n('imag.act_eps', (H, N, A)), step=n('imag.step_eps', (H, N, S)))


def run(case):
    ag, det = make_agent(case)
    ac = ag._acting_behavior
    S, H = ag.cfg.rssm.stoch, ag.cfg.imag_horizon
    nz = update_noise(S, H)
    tape = []
    for t in range(T):
        tape.append(('normal', nz['prior'][t])); tape.append(('normal', nz['post'][t]))
    tape.append(('normal', nz['act0']))
    for h in range(H):
        tape.append(('normal', nz['act'][h])); tape.append(('normal', nz['step'][h]))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n for n, p in ag.named_parameters()}
    grads, phase, cap = {}, ['model'], {}
    raws = {'post': [], 'prior': []}
    hooks = [ag.wm.rssm._obs_dist.register_forward_hook(lambda m, i, o: raws['post'].append(o.detach().clone())),
             ag.wm.rssm._ensemble_img_dist[0].register_forward_hook(lambda m, i, o: raws['prior'].append(o.detach().clone()))]
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_wm, orig_tg, orig_cl = ag.wm.update, ac.target, ac.critic_loss

    def wm_hook(data, *a, **k):
        state, outputs, mets = orig_wm(data, *a, **k)
        for side in ('post', 'prior'):
            for key in ('mean', 'std', 'stoch'):
                cap[f'{side}_{key}'] = outputs[side][key].detach().clone()
        cap['kl_value'] = outputs['kl'].detach().clone()
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        target, mets, baseline = orig_tg(seq)
        for key in ('stoch', 'mean', 'std', 'action'):
            cap[f'imag_{key}'] = seq[key].detach().clone()
        cap['imag_target'] = target.detach().clone()
        return target, mets, baseline

    def cl_hook(seq, target):
        phase[0] = 'critic'
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    trunc = mv2.tape_trunc_normal(tape) if CASES[case][0] == 'dreamer_v2' else contextlib.nullcontext()
    try:
        with rh.inject_noise(tape), trunc:
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
        for h_ in hooks:
            h_.remove()
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    assert len(raws['post']) == T and len(raws['prior']) == T + H, (len(raws['post']), len(raws['prior']))
    cap['post_raw'] = torch.stack(raws['post'], 1)                 # (B, T, 2S)
    cap['prior_raw'] = torch.stack(raws['prior'][:T], 1)
    cap['imag_raw'] = torch.stack(raws['prior'][T:], 0)            # (H, N, 2S)
    out = {}
    pre = case + '.'
    for k, v in mets.items():
        out[f'{pre}metrics.{k}'] = np.asarray(torch.as_tensor(v).detach().numpy())
    out[f'{pre}metric_keys'] = np.array(sorted(mets))
    for k, v in cap.items():
        out[pre + k] = v.numpy()
    for ph in ('model', 'actor', 'critic'):
        for n, gr in grads[ph].items():
            out[f'{pre}grad.{ph}.{n}'] = mv2.grad_rows(gr.numpy())
    for n, v in det.items():
        out[f'{pre}shape.{n}'] = np.array(v.shape, np.int64)
    kl = ag.cfg.kl
    out[f'{pre}meta'] = np.array([B, T, A, S, 0, H, SEED])
    out[f'{pre}kl_cfg'] = np.array([float(kl['balance']), float(kl['free']), float(bool(kl['forward'])), float(ag.cfg.rssm.min_std)])
    return out


def run_act():
    ag, det = make_agent('v3g')
    S = ag.cfg.rssm.stoch
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    obs = {'observation': batch['observation'][0, 3], 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    out = {}
    for mode, ev in (('eval', True), ('sample', False)):
        tape = [('normal', detgen.det_noise(f'act.{mode}.prior_eps', (1, S), 'normal', SEED)),
                ('normal', detgen.det_noise(f'act.{mode}.post_eps', (1, S), 'normal', SEED))]
        if not ev:
            tape.append(('normal', detgen.det_noise(f'act.{mode}.act_eps', (1, A), 'normal', SEED)))
        tape = rh.NoiseTape('replay', tape)
        with rh.inject_noise(tape), torch.no_grad():
            action, (latent, _) = ag.act(obs, None, 0, ev, None)
        assert tape.pos == len(tape.tape), (mode, tape.pos, len(tape.tape))
        out[f'act.{mode}.action'] = np.asarray(action)
        for key in ('mean', 'std', 'stoch'):
            out[f'act.{mode}.{key}'] = latent[key].numpy()
    return out


def main():
    o = {}
    for case in CASES:
        o.update(run(case))
    o.update(run_act())
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/gauss_tiny.npz'
    np.savez_compressed(path, **o)
    print('gauss_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
