"""Generate tests/golden/elu_tiny.npz from the reference's DreamerAgent with `act: ELU` blocks.  Needs a checkout of mazpie/genrl where
ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only the stored file:

    python tests/golden/make_elu_golden.py

`# act: elu` is the marked alternative on every block of conf/defaults/*.yaml and conf/env/dmc_pixels.yaml; the reference's Encoder, Decoder,
MLP and EnsembleRSSM pass it to get_act (agent/dreamer_utils.py:862-868), where 'ELU' is torch.nn.ELU (alpha 1).  Three DreamerAgent.update
cases at tiny widths (detgen.dreamer_tiny_overrides), precision 32, B2 x T18, A = 6, weights from detgen.det_state_dict, noise replayed
through NoiseTape as make_v2_golden.py does, the tape fully consumed:

  'v3e.*' : conf/defaults/dreamer_v3.yaml + act ELU in rssm, encoder, decoder, reward_head, actor, critic
  'v2e.*' : conf/defaults/dreamer_v2.yaml + the same six: norm-free Linear -> ELU in the RSSM and the heads, channel-LayerNorm -> ELU in the convs
  'v3a.*' : conf/defaults/dreamer_v3.yaml + actor {act: ELU} alone: the blocks are independent of each other
  'act.*' : DreamerAgent.act of the v3e agent on one frame, eval mode (the head's mean: no action noise) and sampling mode (Normal.sample
            of the policy, routed through the tape), each from an empty state, with the posterior's latent indices

Asserted here on the CPU: every block asked for holds nn.ELU and every other block nn.SiLU, in the `_act` of the module and in its
nn.Sequentials; and for EVERY categorical race replayed the two largest ratios p / q differ by at least 1e-3 relative
(make_discrete_golden.py).  Seeds are tried from FIRST_SEED upwards until that holds; the seed, the margin of every race replayed with it
and the smallest margin of every seed tried are stored.

Per case with lr = 0: every metric and the metric key list; posterior / imagined latent indices; the imagined actions; every gradient of
the model, actor and critic groups (grad_rows of make_v2_golden.py: every fourth index of the first dimension above 4096 elements); the
shape of every state_dict entry.  Per case with the defaults' optimiser settings: 'delta' = (after - before) / lr of the parameter's
group, rounded to 1/256 and stored as float16 on the same grad_rows, and 'opt.*', as v2_tiny.npz does.  Gradients, deltas and shapes are
packed per group (pack below): names, element counts and the values end to end.  Arrays only; no reference text is stored.  The file must
be no larger than v2_tiny.npz."""
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
from elu_cases import BLOCKS, CASES, block_modules

torch.set_num_threads(8)
B, T, A = 2, 18, 6
FIRST_SEED = 5          # (seeds 5 .. 34 miss the race margin over the 157 replayed draws: between 2.2e-6 and 6.4e-4; seed 35 holds it with 1.16e-3)
MARGIN = 1e-3


def make_agent(case, seed, lr_zero=True):
    defaults, elu = CASES[case]
    over = dict(detgen.dreamer_tiny_overrides())
    for k in elu:
        over[k] = dict(over.get(k, {}), act='ELU')
    if lr_zero:
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            over[k] = dict(lr=0.0, wd=0.0)
    ag = rh.make_ref_dreamer(B, T, A=A, **over) if defaults == 'dreamer_v3' else mv2.make_ref('dreamer', **over)
    n_elu = n_silu = 0
    for name, mod in block_modules(ag).items():
        want = nn.ELU if name in elu else nn.SiLU
        assert type(mod._act) is want, (case, name, mod._act)
        for sub in mod.modules():
            assert not isinstance(sub, (nn.ELU, nn.SiLU)) or type(sub) is want, (case, name, sub)
    for sub in ag.modules():
        n_elu += isinstance(sub, nn.ELU); n_silu += isinstance(sub, nn.SiLU)
    assert (n_silu == 0) == (len(elu) == len(BLOCKS)) and n_elu > 0, (case, n_elu, n_silu)
    ac = ag._acting_behavior
    for d_ in ac._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, seed)
    ag.load_state_dict(det)
    return ag, det


class normal_sample_on_tape:
    """Normal.sample (what Independent(Normal).sample of the 'normal' actor head calls in DreamerAgent.act) draws through Normal.rsample,
    which ref_harness.inject_noise replays"""
    def __enter__(self):
        self.orig = torch.distributions.Normal.sample

        def sample(self_, sample_shape=torch.Size()):
            with torch.no_grad():
                return torch.distributions.Normal.rsample(self_, sample_shape)
        torch.distributions.Normal.sample = sample

    def __exit__(self, *a):
        torch.distributions.Normal.sample = self.orig


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
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        cap['imag_action'] = seq['action'].detach().clone()
        return orig_tg(seq)

    def cl_hook(seq, target):
        phase[0] = 'critic'
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    batch = detgen.det_batch(B, T, A=A, seed=seed)
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with mdg.inject_with_margin(tape), mv2.tape_trunc_normal(tape):
            _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    out = {}
    pre = case + '.'
    if lr_zero:
        keys = sorted(mets)
        out[f'{pre}metric_keys'] = np.array(keys)
        out[f'{pre}metrics'] = np.array([float(torch.as_tensor(mets[k]).detach()) for k in keys], np.float64)
        for k, v in cap.items():
            out[pre + k] = v.numpy()
        for ph in ('model', 'actor', 'critic'):
            out.update(pack(f'{pre}grad.{ph}', {n: mv2.grad_rows(g.numpy()) for n, g in grads[ph].items()}, np.float32))
        names = list(det)
        out[f'{pre}shape.names'] = np.array(names)
        out[f'{pre}shape.dims'] = np.array([list(det[n].shape) + [0] * (4 - det[n].dim()) for n in names], np.int64)
        out[f'{pre}shape.ndim'] = np.array([det[n].dim() for n in names], np.int64)
        out[f'{pre}meta'] = np.array([B, T, A, S, K, H, seed])
    else:
        deltas = {}
        for n, v in ag.state_dict().items():
            grp = mv2.group_of(n)
            if '._target_critic.' in n or grp is None:   # (no optimiser group: the slow critic is hard-copied by the first update; buffers)
                continue
            d = (v.detach() - det[n]).double()
            deltas[n] = mv2.grad_rows(np.round((d / ag.cfg[grp]['lr']).numpy() * 256) / 256)
        out.update(pack(f'{pre}delta', deltas, np.float16))
        for k in ('model_opt', 'actor_opt', 'critic_opt'):
            out[f'{pre}opt.{k}'] = np.array([ag.cfg[k]['lr'], ag.cfg[k]['eps'], ag.cfg[k]['clip'], ag.cfg[k]['wd']], np.float64)
    return out


def pack(prefix, arrays, dtype):
    """{name: array} as three entries -- names, element counts, the values end to end -- (one zip member per tensor costs more than most
    of them hold); tests/elu_cases.py::unpack undoes it"""
    names = list(arrays)
    return {f'{prefix}.names': np.array(names), f'{prefix}.sizes': np.array([arrays[n].size for n in names], np.int64),
            f'{prefix}.data': np.concatenate([np.asarray(arrays[n], dtype).reshape(-1) for n in names])}


def run_act(seed):
    ag, det = make_agent('v3e', seed)
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
        with mdg.inject_with_margin(tape), normal_sample_on_tape(), torch.no_grad():
            action, (latent, _) = ag.act(obs, None, 0, ev, None)
        assert tape.pos == len(tape.tape), (mode, tape.pos, len(tape.tape))
        out[f'act.{mode}.action'] = np.asarray(action)
        out[f'act.{mode}.latent_idx'] = latent['stoch'].argmax(-1).to(torch.int16).numpy()
    return out


def attempt(seed):
    del mdg.margins[:]
    o = {}
    for case in CASES:
        o.update(run(case, seed, True))
    o.update(run_act(seed))
    return o, list(mdg.margins)


def main():
    seed, tried = FIRST_SEED, []
    while True:
        o, margins = attempt(seed)
        race = min(margins)
        print('seed', seed, 'smallest relative margin between the two best candidates of a race:', race, 'over', len(margins), 'draws', flush=True)
        tried.append((seed, race))
        if race >= MARGIN:
            break
        seed += 1
    for case in CASES:
        o.update(run(case, seed, False))
    o['seed'] = np.array(seed)
    o['race_margin'] = np.array(race)
    o['race_margins'] = np.array(margins, np.float64)          # every replayed race of the seed kept, in replay order (v3e, v2e, v3a, act)
    o['seeds_tried'] = np.array(tried, np.float64)             # (seed, its smallest margin) from FIRST_SEED up to the seed kept
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/elu_tiny.npz'
    np.savez_compressed(path, **o)
    print('elu_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
