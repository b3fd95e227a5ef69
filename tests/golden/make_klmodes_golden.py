"""Generate tests/golden/klmodes_tiny.npz from the reference's world-model update in the branches of EnsembleRSSM.kl_loss
(agent/dreamer_utils.py:534-555) that `kl.balance: 0.5` and `kl.free_avg: True` select, and with `clip_rewards: tanh | sign`
(agent/dreamer.py:297-301).  Needs a checkout of mazpie/genrl where ref_harness.REF points (ref_harness imports it from there and refuses to
run without it); the tests read only the stored file:

    python tests/golden/make_klmodes_golden.py

Only `update_wm` runs: the modes reach neither the actor nor the critic.  Weights from detgen.det_state_dict, batch from detgen.det_batch,
noise replayed through NoiseTape (fully consumed), lr = 0, wd = 0, precision 32, seed 5.

DreamerAgent, conf/defaults/dreamer_v3.yaml at detgen.dreamer_tiny_overrides(), B2 x T18, A = 6 (36 KL rows):
  'avg_hi'  : categorical latents, free_avg, free 0.3 (the mean of the rows lies above it), clip_rewards tanh
  'avg_lo'  : categorical latents, free_avg, free 1.0 (the mean lies below: the KL term has no gradient)
  'avg_g'   : Gaussian latents (stoch 8, sigmoid2), free_avg, free 1.0 (mean above)
  'unb_fwd' : categorical latents, balance 0.5, forward True (lhs = prior: pins the side swap); free picked from FREES by the margins
  'unb_g'   : Gaussian latents, balance 0.5, free 1.0, clip_rewards sign
GenRLAgent, conf/defaults/genrl.yaml at detgen.tiny_overrides(), B2 x T16, A = 10 (32 rows):
  'genrl'   : kl.free_avg with connector_kl.balance 0.5 at a non-zero connector_kl.free picked from FREES by the margins; the first
              connector update runs inside update_wm (`connector_kl.free_avg: True` cannot run in the reference: VideoSSM.update adds the
              [1]-shaped loss in place into a 0-d tensor, agent/video_utils.py:195)

Margins asserted here: an unbalanced case has rows on both sides of the clamp and no row within 1e-3 of `free`; an averaged case has its
mean at least 1e-2 away from `free`.

Per case: every metric; the posterior's and the prior's statistics (logit, or mean and std) with the per-row KL ('conn_*': the same of the
connector's KL in the GenRL case); the KL settings; the clipped reward; the gradients of wm.rssm.* and wm.encoder.* (GenRL: and of the
connector but its aligner) sampled by make_v2_golden.grad_rows; the shape of every state_dict entry.
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
SEED = 5
GAUSS = dict(stoch=8, std_act='sigmoid2')
FREES = (0.5, 0.45, 0.4, 0.55, 0.35, 0.3, 0.25, 0.2, 0.15, 0.1)          # tried in this order where a case leaves `free` to the margins
# case: (agent, Gaussian latents, kl, connector_kl, clip_rewards); free None: the first of FREES that passes the margins
CASES = {
    'avg_hi': ('dreamer', False, dict(free_avg=True, free=0.3), None, 'tanh'),
    'avg_lo': ('dreamer', False, dict(free_avg=True, free=1.0), None, 'identity'),
    'avg_g': ('dreamer', True, dict(free_avg=True, free=1.0), None, 'identity'),
    'unb_fwd': ('dreamer', False, dict(balance=0.5, forward=True, free=None), None, 'identity'),
    'unb_g': ('dreamer', True, dict(balance=0.5, free=1.0), None, 'sign'),
    'genrl': ('genrl', False, dict(free_avg=True, free=0.3), dict(balance=0.5, free=None), 'identity'),
}
DIMS = {'dreamer': (2, 18, 6), 'genrl': (2, 16, 10)}


class Margin(AssertionError):
    pass


def check_margins(what, value, cfg):
    """the margins of the docstring on one KL's rows under its settings"""
    v, free = value.detach().double().flatten(), float(cfg['free'])
    if float(cfg['balance']) == 0.5:
        if not (bool((v > free).any()) and bool((v < free).any())):
            raise Margin(f'{what}: free {free} has rows on one side only ({float(v.min()):.4f} .. {float(v.max()):.4f})')
        if float((v - free).abs().min()) < 1e-3:
            raise Margin(f'{what}: a row lies {float((v - free).abs().min()):.2e} from free {free}')
    elif cfg['free_avg']:
        if abs(float(v.mean()) - free) < 1e-2:
            raise Margin(f'{what}: the mean {float(v.mean()):.4f} lies within 1e-2 of free {free}')


def make_agent(case, kl, ckl):
    kind, gauss, _, _, clip = CASES[case]
    B, T, A = DIMS[kind]
    over = dict(detgen.tiny_overrides() if kind == 'genrl' else detgen.dreamer_tiny_overrides())
    if gauss:
        over['rssm'] = dict(over['rssm'], discrete=False, **GAUSS)
    for k in ('model_opt', 'actor_opt', 'critic_opt'):
        over[k] = dict(lr=0.0, wd=0.0)
    over.update(kl=kl, clip_rewards=clip)
    if ckl is not None:
        over.update(connector_kl=ckl, imag_reward_fn='video_text_reward')      # (the imagination behaviour exists, as train.py builds it)
    ag = rh.make_ref_agent(B, T, A=A, **over) if kind == 'genrl' else rh.make_ref_dreamer(B, T, A=A, **over)
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, SEED)
    ag.load_state_dict(det)
    return ag, det


def run(case, kl, ckl):
    kind, gauss = CASES[case][:2]
    B, T, A = DIMS[kind]
    ag, det = make_agent(case, kl, ckl)
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    tape = []
    if gauss:
        n = lambda name: detgen.det_noise(name, (T, B, S), 'normal', SEED)
        pr, po = n('wm.prior_eps'), n('wm.post_eps')
        for t in range(T):
            tape.append(('normal', pr[t])); tape.append(('normal', po[t]))
    else:
        noise = detgen.iteration_noise(B, T, S, K, A, ag.cfg.imag_horizon, seed=SEED)
        for t in range(T):
            tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
        if kind == 'genrl':                              # the first connector update, inside WorldModel.update
            c = noise['conn1']
            tape.append(('randn_like', c['clip_eps'])); tape.append(('exp', c['init_q']))
            for t in range(T):
                tape.append(('exp', c['step_q'][t]))
            tape.append(('exp', c['ikl_init_q'])); tape.append(('exp', c['ikl_step_q']))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n_ for n_, p in ag.named_parameters()}
    grads, cap = [], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads.append({names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None})
        return orig_clip(params, clip, *a, **k)
    orig_pre = ag.wm.preprocess

    def pre_hook(obs):
        out = orig_pre(obs)
        cap['reward'] = out['reward'].detach().clone()
        return out
    ag.wm.preprocess = pre_hook
    if kind == 'genrl':
        conn, orig_ckl = ag.wm.connector, ag.wm.connector.kl_loss

        def ckl_hook(post, prior, **kw):
            loss, value = orig_ckl(post, prior, **kw)
            if 'conn_kl_value' not in cap:               # (the second call is the initial-KL metric)
                cap.update(conn_post_logit=post['logit'].detach().clone(), conn_prior_logit=prior['logit'].detach().clone(),
                           conn_kl_value=value.detach().clone())
            return loss, value
        conn.kl_loss = ckl_hook
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    tb = {k: v for k, v in rh.to_torch(batch).items() if kind == 'genrl' or k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with rh.inject_noise(tape):
            state, outputs, mets = ag.update_wm(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    assert len(grads) == (2 if kind == 'genrl' else 1), len(grads)
    kl_cfg = ag.cfg.kl
    check_margins(f'{case} kl', outputs['kl'], kl_cfg)
    if kind == 'genrl':
        check_margins(f'{case} connector_kl', cap['conn_kl_value'], ag.cfg.connector_kl)
    for side in ('post', 'prior'):
        for key in (('mean', 'std') if gauss else ('logit',)):
            cap[f'{side}_{key}'] = outputs[side][key].detach().clone()
    cap['kl_value'] = outputs['kl'].detach().clone()
    out, pre = {}, case + '.'
    for k, v in mets.items():
        out[f'{pre}metrics.{k}'] = np.asarray(torch.as_tensor(v).detach().numpy())
    out[f'{pre}metric_keys'] = np.array(sorted(mets))
    for k, v in cap.items():
        out[pre + k] = v.numpy()
    for n_, gr in grads[0].items():
        if n_.startswith(('wm.rssm.', 'wm.encoder.')):
            out[f'{pre}grad.model.{n_}'] = mv2.grad_rows(gr.numpy())
    if kind == 'genrl':
        for n_, gr in grads[1].items():
            if '.aligner.' not in n_:
                out[f'{pre}grad.connector.{n_}'] = mv2.grad_rows(gr.numpy())
    for n_, v in det.items():
        out[f'{pre}shape.{n_}'] = np.array(v.shape, np.int64)
    out[f'{pre}meta'] = np.array([B, T, A, S, int(K or 0), SEED])
    cfgs = [kl_cfg] + ([ag.cfg.connector_kl] if kind == 'genrl' else [])
    for name, c in zip(('kl_cfg', 'conn_kl_cfg'), cfgs):          # balance, free, forward, free_avg
        out[pre + name] = np.array([float(c['balance']), float(c['free']), float(bool(c['forward'])), float(bool(c['free_avg']))])
    out[f'{pre}clip_rewards'] = np.array(str(ag.cfg.clip_rewards))
    v = outputs['kl'].detach()
    print(f"{case}: kl rows {float(v.min()):.4f} .. {float(v.max()):.4f} mean {float(v.mean()):.4f}, free {kl_cfg['free']}, "
          f"{int((v > kl_cfg['free']).sum())} of {v.numel()} above; kl_loss {float(mets['kl_loss']):.6f}, reward_loss "
          f"{float(mets.get('reward_loss', float('nan'))):.4f}", flush=True)
    if kind == 'genrl':
        v, f = cap['conn_kl_value'], float(ag.cfg.connector_kl['free'])
        print(f"{case}: connector rows {float(v.min()):.4f} .. {float(v.max()):.4f} mean {float(v.mean()):.4f}, free {f}, "
              f"{int((v > f).sum())} of {v.numel()} above", flush=True)
    return out


def run_picking_free(case):
    """the case with every `free: None` replaced by the first value of FREES that passes the margins"""
    _, _, kl, ckl, _ = CASES[case]
    which = kl if kl.get('free', 0) is None else (ckl if ckl is not None and ckl.get('free', 0) is None else None)
    if which is None:
        return run(case, dict(kl), None if ckl is None else dict(ckl))
    for free in FREES:
        k2, c2 = dict(kl), None if ckl is None else dict(ckl)
        (k2 if which is kl else c2)['free'] = free
        try:
            return run(case, k2, c2)
        except Margin as e:
            print('rejected:', e, flush=True)
    raise AssertionError(f'{case}: no free of {FREES} passes the margins')


def main():
    o = {}
    for case in CASES:
        o.update(run_picking_free(case))
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/klmodes_tiny.npz'
    np.savez_compressed(path, **o)
    print('klmodes_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
