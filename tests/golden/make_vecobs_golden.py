"""Generate tests/golden/vecobs_tiny.npz from the reference's DreamerAgent with vector (1-D) observations.  Needs a checkout of mazpie/genrl
where ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only the stored file:

    python tests/golden/make_vecobs_golden.py

The reference agent is built here from ref_harness's pieces (rh._load, rh.AD, rh.Spec, rh.ref_modules): ref_harness.make_ref_dreamer has the
image-only observation space built in.  Two DreamerAgent.update cases at tiny widths (detgen.dreamer_tiny_overrides, `mlp_layers: [32, 32]` in
encoder and decoder), precision 32, B2 x T18, A = 6, lr = 0, weights from detgen.det_state_dict, noise replayed through NoiseTape as
make_v2_golden.py does (discrete latents: the exponential races of detgen.iteration_noise; the tape must be fully consumed):

  'mix.*' : conf/defaults/dreamer_v3.yaml, the image `observation` + `proprio` (7,); encoder mlp_keys proprio, symlog_inputs True; decoder
            mlp_keys proprio, mlp_dist symlog_mse
  'st.*'  : conf/defaults/dreamer_v2.yaml, `observation` (9,) alone; cnn_keys '$^', mlp_keys observation in both; no symlog, mlp_dist mse

Vector observations are detgen.det_noise('obs.' + key, (B, T, D), 'normal', SEED) * 5: symlog is exercised well away from 0.

Conditions on the seed, asserted below on the CPU.  (1) SymlogDist's `where(distance < tol, 0, distance)` is a discontinuity: in 'mix' no
element has (mode - symlog x)^2 inside [tol / 4, 4 tol].  (2) As in make_discrete_golden.py, for every race replayed here (posterior, prior,
imagined latents, act()) the two largest ratios p / q differ by at least 4e-4 relative, so that the float32 summation order of another
implementation cannot flip a draw: a draw flips only where that margin is below the error of a logit difference, and a tiny-width logit (32
terms of order 1 in fp32, or on fp16-pair planes of 2^-22 relative error) carries about 1e-5.  The 1e-3 of make_discrete_golden.py is out of
reach here: with two cases and act() about 5 000 races are replayed, and no seed in 5 .. 20 has all of them 1e-3 apart (the best, 13, has
9.95e-4).  Seeds are tried from 5 upwards; the first that meets both conditions is used and recorded in `meta` (5 misses (2) with 1.75e-4;
6 meets both).

Per case: every metric; `embed`; the posterior features the decoder reads; the raw output of every vector key's head (`dense_{key}._out`) and the per-(B, T) `likes` of every key; the
posterior's latent indices and logits; the imagined latent indices; every gradient of the model, actor and critic groups (grad_rows of
make_v2_golden.py: more than 4096 elements -> every fourth index of the first dimension); the shape of every state_dict entry.
'act.*': DreamerAgent.act of the 'st' agent on one observation from an empty state, in eval mode and in sampling mode, with the posterior's
latent indices.  Arrays only; no reference text is stored.  The file must be no larger than v2_tiny.npz."""
import contextlib
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
MARGIN, TOL = 4e-4, 1e-8
SEEDS = range(5, 21)
MLP = [32, 32]
CASES = {
    'mix': ('dreamer_v3', {'proprio': 7},
            dict(encoder=dict(mlp_keys='proprio', symlog_inputs=True, mlp_layers=MLP),
                 decoder=dict(mlp_keys='proprio', mlp_dist='symlog_mse', mlp_layers=MLP))),
    'st': ('dreamer_v2', {'observation': 9},
           dict(encoder=dict(cnn_keys='$^', mlp_keys='observation', symlog_inputs=False, mlp_layers=MLP),
                decoder=dict(cnn_keys='$^', mlp_keys='observation', mlp_dist='mse', mlp_layers=MLP))),
}


class SeedRejected(Exception):
    pass


def make_ref(defaults, vec_obs, **over):
    m = rh.ref_modules()
    cfg = rh.AD()
    cfg.update(rh._load(f'{rh.REF}/conf/defaults/{defaults}.yaml'))
    cfg.update(rh._load(f'{rh.REF}/conf/env/dmc_pixels.yaml'))
    a = rh._load(f'{rh.REF}/agent/dreamer.yaml')
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
    for key, width in vec_obs.items():
        obs[key] = rh.Spec((width,), np.float32)
    torch.manual_seed(0)
    return m.dreamer.DreamerAgent(name=name, cfg=cfg, obs_space=obs, act_spec=rh.Spec((A,), np.float32))


def make_agent(case, seed):
    defaults, vec_obs, extra = CASES[case]
    over = dict(detgen.dreamer_tiny_overrides())
    for k, v in extra.items():
        over[k] = dict(over[k], **v)
    for k in ('model_opt', 'actor_opt', 'critic_opt'):
        over[k] = dict(lr=0.0, wd=0.0)
    ag = make_ref(defaults, vec_obs, **over)
    enc, dec = ag.wm.encoder, ag.wm.heads['decoder']
    assert enc.mlp_keys == list(vec_obs) and dec.mlp_keys == list(vec_obs)
    assert (len(enc.cnn_keys), len(dec.cnn_keys)) == ((1, 1) if case == 'mix' else (0, 0))
    for d_ in ag._acting_behavior._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, seed)
    ag.load_state_dict(det)
    return ag, det


def vec_batch(case, seed):
    """detgen.det_batch with the case's vector observations added (a key named 'observation' replaces the frames)"""
    batch = {k: v for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    for key, width in CASES[case][1].items():
        batch[key] = (detgen.det_noise('obs.' + key, (B, T, width), 'normal', seed) * 5).numpy()
    return batch


def run(case, seed):
    ag, det = make_agent(case, seed)
    ac = ag._acting_behavior
    S, K, H = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete, ag.cfg.imag_horizon
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    tape = []
    for t in range(T):
        tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
    tape.append(('normal', noise['imag']['act_eps0']))
    for h in range(H):
        tape.append(('normal', noise['imag']['act_eps'][h])); tape.append(('exp', noise['imag']['step_q'][h]))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n for n, p in ag.named_parameters()}
    grads, phase, cap, raws = {}, ['model'], {}, {}
    dec = ag.wm.heads['decoder']

    def keep_first(key):           # (the update's own call comes first; a forward hook must return None, or its value replaces the output)
        def hook(m, i, o):
            raws.setdefault(key, o.detach().clone())
        return hook
    hooks = [getattr(dec, f'dense_{key}')._out.register_forward_hook(keep_first(key)) for key in dec.mlp_keys]
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_wm, orig_tg, orig_cl = ag.wm.update, ac.target, ac.critic_loss

    def wm_hook(data, *a, **k):
        state, outputs, mets = orig_wm(data, *a, **k)
        cap['embed'] = outputs['embed'].detach().clone()
        cap['feat'] = outputs['feat'].detach().clone()                  # (what the decoder reads: `decoder_inputs: feat`)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        cap['post_logit'] = outputs['post']['logit'].detach().clone()
        for key, like in outputs['likes'].items():
            cap[f'like.{key}'] = like.detach().clone()
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        return orig_tg(seq)

    def cl_hook(seq, target):
        phase[0] = 'critic'
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    batch = vec_batch(case, seed)
    tb = rh.to_torch(batch)
    torch.nn.utils.clip_grad_norm_ = clip_capture
    trunc = mv2.tape_trunc_normal(tape) if CASES[case][0] == 'dreamer_v2' else contextlib.nullcontext()
    try:
        with mdg.inject_with_margin(tape), trunc:
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
        for h_ in hooks:
            h_.remove()
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    assert set(cap) >= {f'like.{k}' for k in dec.mlp_keys + dec.cnn_keys} | {'like.reward'}
    for key in dec.mlp_keys:
        raw = raws[key]
        assert raw.shape == tb[key].shape
        cap[f'vec_raw.{key}'] = raw
        if dec._mlp_dist == 'symlog_mse':        # condition (1): nothing near the tol discontinuity
            x = tb[key]
            d = (raw - torch.sign(x) * torch.log(torch.abs(x) + 1)) ** 2
            near = int(((d >= TOL / 4) & (d <= 4 * TOL)).sum())
            if near:
                raise SeedRejected(f'{case}: {near} element(s) of `{key}` within a factor 4 of tol')
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
    out[f'{pre}meta'] = np.array([B, T, A, S, K, H, seed])
    return out


def run_act(seed):
    ag, det = make_agent('st', seed)
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    batch = vec_batch('st', seed)
    obs = {'observation': batch['observation'][0, 3], 'reward': np.float32(0.0), 'is_first': np.bool_(True),
           'is_last': np.bool_(False), 'is_terminal': np.bool_(False)}
    out = {}
    for mode, ev in (('eval', True), ('sample', False)):
        tape = [('exp', detgen.det_noise(f'act.{mode}.prior_q', (S, K), 'exp', seed)),
                ('exp', detgen.det_noise(f'act.{mode}.post_q', (S, K), 'exp', seed))]
        if not ev:
            tape.append(('normal', detgen.det_noise(f'act.{mode}.act_eps', (1, A), 'normal', seed)))
        tape = rh.NoiseTape('replay', tape)
        with mdg.inject_with_margin(tape), mv2.tape_trunc_normal(tape), torch.no_grad():
            action, (latent, _) = ag.act(obs, None, 0, ev, None)
        assert tape.pos == len(tape.tape), (mode, tape.pos, len(tape.tape))
        out[f'act.{mode}.action'] = np.asarray(action)
        out[f'act.{mode}.latent_idx'] = latent['stoch'].argmax(-1).to(torch.int16).numpy()
    return out


def generate(seed):
    del mdg.margins[:]
    o = {}
    for case in CASES:
        o.update(run(case, seed))
    o.update(run_act(seed))
    margin = min(mdg.margins)
    if margin < MARGIN:
        raise SeedRejected(f'smallest relative margin of a race {margin:.3g} over {len(mdg.margins)} draws')
    o['race_margin'] = np.array(margin)
    return o


def main():
    for seed in SEEDS:
        try:
            o = generate(seed)
            break
        except SeedRejected as e:
            print('seed', seed, 'rejected:', e)
    else:
        raise SystemExit('no seed in %r meets both conditions' % (SEEDS,))
    print('seed', seed, 'race margin', float(o['race_margin']))
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/vecobs_tiny.npz'
    np.savez_compressed(path, **o)
    print('vecobs_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
