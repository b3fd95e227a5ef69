"""Generate tests/golden/convfree_tiny.npz from the reference's DreamerAgent with norm-free conv stacks (`encoder.norm: none`,
`decoder.norm: none`).  Needs a checkout of mazpie/genrl where ref_harness.REF points (ref_harness imports it from there and refuses to run
without it); the tests read only the stored file:

    python tests/golden/make_convfree_golden.py

The reference's Encoder and Decoder build [Conv2d, NormLayer('none'), act] triples for `norm: none` (agent/dreamer_utils.py:587, :669) and
bias-free Linear + act MLP stacks (:597, :679); 'none' is the class default of both.  Four DreamerAgent.update cases (tests/convfree_cases.py)
at tiny widths (detgen.dreamer_tiny_overrides), precision 32, B2 x T18, A = 6, weights from detgen.det_state_dict, noise replayed through
NoiseTape as make_elu_golden.py does, the tape fully consumed:

  'v2n.*'  : conf/defaults/dreamer_v2.yaml + encoder {norm: none} + decoder {norm: none}
  'v2ne.*' : the same + act ELU in rssm, encoder, decoder, reward_head, actor, critic: the DreamerV2 network as published
  'v3n.*'  : conf/defaults/dreamer_v3.yaml + both conv blocks norm-free (every other block keeps its LayerNorm)
  'v3d.*'  : conf/defaults/dreamer_v3.yaml + decoder {norm: none} alone, with the vector observation `proprio` (7,) beside the image
             (make_vecobs_golden.py's 'mix'): the encoder keeps LayerNorm and biases, the decoder's conv stack and its MLP trunk are norm-free
  'act.*'  : DreamerAgent.act of the v2ne agent on one frame, eval mode and sampling mode, each from an empty state, with the posterior's
             latent indices

Asserted here on the CPU: the requested stacks hold no LayerNorm and their conv layers have biases, their MLP stacks are bias-free, the other
conv block holds its LayerNorms; for EVERY categorical race replayed the two largest ratios p / q differ by at least 1e-3 relative
(make_discrete_golden.py), and in 'v3d' no element of the symlog_mse head lies within a factor 4 of its tolerance discontinuity
(make_vecobs_golden.py).  Seeds are tried from FIRST_SEED upwards until both hold; the seed, the margin of every race replayed with it and
the smallest margin of every seed tried are stored.

Per case with lr = 0: every metric and the metric key list; posterior / imagined latent indices; the imagined actions; every gradient of
the model, actor and critic groups (convfree_cases.grad_rows: every fourth index of the first dimension, again while more than 1024
elements remain -- make_v2_golden.py's rule, once above 4096 elements, would pass the size limit with four cases); the shape of every state_dict entry; and the samples the plain-torch
restatement of tests/test_convfree_golden.py is checked on: `embed` of the first three steps, the posterior features of two steps and the
decoder's mean for them on every fourth pixel.  Per case with the defaults' optimiser settings: 'delta' and 'opt.*', as elu_tiny.npz does.
Arrays only; no reference text is stored.  The file must be no larger than v2_tiny.npz."""
import os, sys
import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen
import make_v2_golden as mv2
import make_discrete_golden as mdg
import make_vecobs_golden as mvo
from make_elu_golden import pack
import convfree_cases as C

torch.set_num_threads(8)
B, T, A = 2, 18, 6
FIRST_SEED = 3700       # (about 10 000 races are replayed per seed and roughly one seed in a few thousand keeps all of them 1e-3 apart: a search
#                         over seeds 5 .. 2900 in ranges found none -- the best, 444, reaches 9.7e-4 -- the range from 3700 holds it at 3752 with
#                         1.0e-3; started lower, this loop only takes longer to arrive at the first seed that holds the margin)
MARGIN, TOL = 1e-3, 1e-8
assert (mvo.B, mvo.T, mvo.A) == (B, T, A)


class SeedRejected(Exception):
    pass


def make_agent(case, seed, lr_zero=True):
    defaults, vec_obs, free, elu, _ = C.CASES[case]
    over = C.overrides(case, detgen.dreamer_tiny_overrides())
    if lr_zero:
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            over[k] = dict(lr=0.0, wd=0.0)
    ag = mvo.make_ref(defaults, vec_obs, **over)
    enc, dec = ag.wm.encoder, ag.wm.heads['decoder']
    for name, mod in (('encoder', enc), ('decoder', dec)):
        lns = C.norm_params(mod)
        convs = [m for m in mod._conv_model if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
        assert len(convs) == 4 and all(c.bias is not None for c in convs), (case, name)
        if name in free:
            assert not lns, (case, name, lns)
            assert not vec_obs or all(m.bias is None for m in mod._mlp_model if isinstance(m, nn.Linear)), (case, name)
        else:
            assert len(lns) >= (4 if name == 'encoder' else 3), (case, name, lns)
    for name, mod in C.block_modules(ag).items():
        want = nn.ELU if name in elu else nn.SiLU
        assert type(mod._act) is want, (case, name, mod._act)
    for d_ in ag._acting_behavior._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, seed)
    if 'encoder' in free:
        assert sorted(k for k in det if k.startswith('wm.encoder._conv_model')) == sorted(
            f'wm.encoder._conv_model.{i}.{p}' for i in (0, 3, 6, 9) for p in ('weight', 'bias')), case
    ag.load_state_dict(det)
    return ag, det


def batch_of(case, seed):
    batch = {k: v for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    batch.update(C.vec_batch(case, B, T, seed))
    return batch


def run(case, seed, lr_zero):
    ag, det = make_agent(case, seed, lr_zero)
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

    def keep_first(key):
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
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        with torch.no_grad():
            cap['embed'] = outputs['embed'].detach()[:, :3].clone()
            cap['feat'] = outputs['feat'].detach()[:1, :2].clone()
            cap['recon'] = dec(cap['feat'])['observation'].mean[..., ::4, ::4].clone()
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        cap['imag_action'] = seq['action'].detach().clone()
        return orig_tg(seq)

    def cl_hook(seq, target):
        phase[0] = 'critic'
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    tb = rh.to_torch(batch_of(case, seed))
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with mdg.inject_with_margin(tape), mv2.tape_trunc_normal(tape):
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
        for h_ in hooks:
            h_.remove()
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    for key in dec.mlp_keys:
        if dec._mlp_dist == 'symlog_mse':        # nothing near SymlogDist's tol discontinuity
            x = tb[key]
            d = (raws[key] - torch.sign(x) * torch.log(torch.abs(x) + 1)) ** 2
            near = int(((d >= TOL / 4) & (d <= 4 * TOL)).sum())
            if near:
                raise SeedRejected(f'{case}: {near} element(s) of `{key}` within a factor 4 of tol')
    out = {}
    pre = case + '.'
    if lr_zero:
        keys = sorted(mets)
        out[f'{pre}metric_keys'] = np.array(keys)
        out[f'{pre}metrics'] = np.array([float(torch.as_tensor(mets[k]).detach()) for k in keys], np.float64)
        for k, v in cap.items():
            out[pre + k] = v.numpy()
        for ph in ('model', 'actor', 'critic'):
            out.update(pack(f'{pre}grad.{ph}', {n: C.grad_rows(g.numpy()) for n, g in grads[ph].items()}, np.float32))
        names = list(det)
        out[f'{pre}shape.names'] = np.array(names)
        out[f'{pre}shape.dims'] = np.array([list(det[n].shape) + [0] * (4 - det[n].dim()) for n in names], np.int64)
        out[f'{pre}shape.ndim'] = np.array([det[n].dim() for n in names], np.int64)
        out[f'{pre}meta'] = np.array([B, T, A, S, K, H, seed])
    else:
        deltas = {}
        for n, v in ag.state_dict().items():
            grp = mv2.group_of(n)
            if '._target_critic.' in n or grp is None:
                continue
            d = (v.detach() - det[n]).double()
            deltas[n] = C.grad_rows(np.round((d / ag.cfg[grp]['lr']).numpy() * 256) / 256)
        out.update(pack(f'{pre}delta', deltas, np.float16))
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            out[f'{pre}opt.{k}'] = np.array([ag.cfg[k]['lr'], ag.cfg[k]['eps'], ag.cfg[k]['clip'], ag.cfg[k]['wd']], np.float64)
    return out


def run_act(seed):
    ag, det = make_agent('v2ne', seed)
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    batch = detgen.det_batch(B, T, A=A, seed=seed)
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


def attempt(seed):
    del mdg.margins[:]
    o = {}
    for case in C.CASES:
        o.update(run(case, seed, True))
    o.update(run_act(seed))
    return o, list(mdg.margins)


def main():
    seed, tried = FIRST_SEED, []
    while True:
        try:
            o, margins = attempt(seed)
            race = min(margins)
        except SeedRejected as e:
            print('seed', seed, 'rejected:', e, flush=True)
            race, margins = 0.0, []
        print('seed', seed, 'smallest relative margin between the two best candidates of a race:', race, 'over', len(margins), 'draws', flush=True)
        tried.append((seed, race))
        if race >= MARGIN:
            break
        seed += 1
    for case in C.CASES:
        o.update(run(case, seed, False))
    o['seed'] = np.array(seed)
    o['race_margin'] = np.array(race)
    o['race_margins'] = np.array(margins, np.float64)          # every replayed race of the seed kept, in replay order (the cases, then act)
    o['seeds_tried'] = np.array(tried, np.float64)             # (seed, its smallest margin; 0: rejected by the tol condition) from FIRST_SEED up
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/convfree_tiny.npz'
    np.savez_compressed(path, **o)
    print('convfree_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
