"""Generate tests/golden/discount_tiny.npz from the reference's DreamerAgent with `pred_discount: True`: the discount head of
WorldModel.__init__ (agent/dreamer.py:147-148), its loss (:229-243) and the learned discounts and weights of WorldModel.imagine (:274-286)
in the behaviour update.  Needs a checkout of mazpie/genrl where ref_harness.REF points (ref_harness imports it from there and refuses to run
without it); the tests read only the stored file:

    python tests/golden/make_discount_golden.py

DreamerAgent.update at tiny widths (detgen.dreamer_tiny_overrides plus `discount_head.units: 32`), precision 32, B2 x T18, A = 6, lr = 0,
wd = 0, weights from detgen.det_state_dict, noise replayed through NoiseTape (fully consumed) as make_v2_golden.py and
make_discrete_golden.py do.  Each case has a seed of its own (stored in its `meta`): the first of SEEDS with which every race replayed in
the case keeps the margin of make_discrete_golden.py (1e-3 relative between its two best candidates).  The cases are the table of
tests/discount_cases.py:

  'v3'             : conf/defaults/dreamer_v3.yaml (reward_ema), grad_heads [decoder, reward, discount]
  'v3_ent0'        : the same defaults with actor_ent 0 and the head outside grad_heads (its input is stop-gradiented)
  'v2'             : conf/defaults/dreamer_v2.yaml (no EMA, actor_ent 3e-4)
  'disc_reinforce' : dreamer_v3.yaml + discrete_actions + actor_grad reinforce

The world-model half is the reference as it stands.  The behaviour half cannot run there unaided: agent/dreamer.py:275 calls
`.mean()` on a distribution whose `mean` is a property, `1.0 - flatten(is_terminal)` (:279) raises on a bool tensor and the `cat` of :280
needs the flags shaped (B, T, 1).  So the batch carries `is_terminal` as float (B, T, 1), and wm.heads['discount'] is wrapped -- here, in
MeanCallable below -- so that the object it returns answers `.mean()` with the wrapped distribution's `.mean`.  Nothing else is replaced:
the reference's own code runs everything after that call.

Terminal flags (discount_cases.TERMINALS): 6 of the 36 start states, inside both windows and at both windows' last step; asserted below.

Per case: every metric; the flags; the discount head's raw output over the posterior (B, T, 1) with its log-likelihood, and over the H+1
rollout states; seq['discount'], seq['weight'], the normalised rewards, the slow critic's values and the lambda-returns; the returns the
critic regresses onto; the gradients of the actor, the critic, wm.heads.discount.* and wm.rssm.* sampled by make_v2_golden.grad_rows; the
shape of every state_dict entry.
Arrays only; no reference text is stored.  The file must be no larger than v2_tiny.npz."""
import os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen
import discount_cases as C
import make_v2_golden as mv2
import make_discrete_golden as mdg

torch.set_num_threads(8)
B, T, A = C.B, C.T, C.A
SEEDS = range(1, 65)          # tried in this order, per case: the first whose races all keep the margin is the case's seed


class MeanCallable(torch.nn.Module):
    """wm.heads['discount'] whose distribution answers `.mean()` (agent/dreamer.py:275) with the property `.mean` of the reference's own
    distribution; every other attribute is that distribution's"""
    class Dist:
        def __init__(self, dist):
            self._dist = dist

        def mean(self):
            return self._dist.mean

        def __getattr__(self, name):
            return getattr(self._dist, name)

    def __init__(self, head):
        super().__init__()
        self.head = head

    def forward(self, x):
        return MeanCallable.Dist(self.head(x))


def make_agent(case, seed):
    defaults, over = C.overrides(case, detgen.dreamer_tiny_overrides())
    ag = rh.make_ref_dreamer(B, T, A=A, **over) if defaults == 'dreamer_v3' else mv2.make_ref('dreamer', **over)
    ac = ag._acting_behavior
    assert ag.cfg.pred_discount and 'discount' in ag.wm.heads and ag.wm.heads['discount']._out._dist == 'binary'
    for d_ in ac._target_critic.parameters():       # un-alias the slow critic (agent/dreamer.py:361-362)
        d_.data = d_.data.clone()
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, seed)
    ag.load_state_dict(det)
    return ag, det


def run(case, seed):
    ag, det = make_agent(case, seed)
    ac = ag._acting_behavior
    S, K, H = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete, ag.cfg.imag_horizon
    discrete = bool(ag.cfg.get('discrete_actions', False))
    trunc = ac.actor._out._dist == 'trunc_normal'
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    tape = []
    for t in range(T):
        tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
    if discrete:
        q0, qa = (detgen.det_noise(name, shape, 'exp', seed) for name, shape in (('imag.act_q0', (B * T, A)), ('imag.act_q', (H, B * T, A))))
        tape.append(('exp', q0))
    else:
        tape.append(('normal', noise['imag']['act_eps0']))
    for h in range(H):
        tape.append(('exp', qa[h]) if discrete else ('normal', noise['imag']['act_eps'][h]))
        tape.append(('exp', noise['imag']['step_q'][h]))
    tape = rh.NoiseTape('replay', tape)
    names = {id(p): n for n, p in ag.named_parameters()}
    grads, phase, cap = {}, ['model'], {}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads[phase[0]] = {names[id(p)]: p.grad.detach().clone() for p in params if p.grad is not None}
        return orig_clip(params, clip, *a, **k)
    orig_wm, orig_tg, orig_cl = ag.wm.update, ac.target, ac.critic_loss
    head = ag.wm.heads['discount']
    raws = []
    hook = head._out._out.register_forward_hook(lambda mod, inp, out: raws.append(out.detach().clone()))
    ag.wm.heads['discount'] = MeanCallable(head)            # (after `names`: the parameters keep the reference's names)

    def wm_hook(data, *a, **k):
        state, outputs, mets = orig_wm(data, *a, **k)
        cap['post_idx'] = outputs['post']['stoch'].detach().argmax(-1).to(torch.int16)
        cap['like_discount'] = outputs['likes']['discount'].detach().clone()
        return state, outputs, mets

    def tg_hook(seq):
        phase[0] = 'actor'
        target, mets, baseline = orig_tg(seq)
        cap['imag_idx'] = seq['stoch'].detach().argmax(-1).to(torch.int16)
        act = seq['action'].detach()
        cap['imag_action'] = act.to(torch.int8) if discrete else act.clone()
        with torch.no_grad():
            cap['imag_discount'] = seq['discount'].detach().clone()
            cap['imag_weight'] = seq['weight'].detach().clone()
            cap['imag_reward'] = seq['reward'].detach().clone()
            cap['imag_value'] = ac._target_critic(seq['feat'].detach()).mean.clone()
            cap['imag_target'] = target.detach().clone()
        return target, mets, baseline

    def cl_hook(seq, target):
        phase[0] = 'critic'
        cap['critic_target_in'] = target.detach().clone()
        return orig_cl(seq, target)
    ag.wm.update, ac.target, ac.critic_loss = wm_hook, tg_hook, cl_hook
    batch = detgen.det_batch(B, T, A=A, seed=seed)
    if discrete:         # the replayed actions of a discrete-action environment are one-hot (collect_data.py:204-205)
        g = np.random.Generator(np.random.PCG64([seed, 77]))
        batch['action'] = np.eye(A, dtype=np.float32)[g.integers(0, A, size=(B, T))]
        cap['batch_action_idx'] = torch.from_numpy(batch['action'].argmax(-1).astype(np.int8))
    flags = C.is_terminal()
    C.check_terminals(flags)
    cap['is_terminal'] = torch.from_numpy(flags)
    tb = {k: v for k, v in rh.to_torch(batch).items() if k != 'clip_video'}
    tb['is_terminal'] = torch.from_numpy(flags.astype(np.float32))[..., None]          # float (B, T, 1): see the docstring
    torch.nn.utils.clip_grad_norm_ = clip_capture
    try:
        with mdg.inject_with_margin(tape):
            if trunc:
                with mv2.tape_trunc_normal(tape):
                    _, mets = ag.update(tb, 0)
            else:
                _, mets = ag.update(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
        hook.remove()
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    # the head ran twice: over the posterior in WorldModel.loss, over the rollout's H+1 states in WorldModel.imagine
    assert len(raws) == 2 and raws[0].shape == (B, T, 1) and raws[1].shape == (H + 1, B * T, 1), [r.shape for r in raws]
    cap['post_raw'], cap['imag_raw'] = raws
    w, d = cap['imag_weight'], cap['imag_discount']
    term = torch.from_numpy(flags.reshape(-1))
    assert float(d[0][term].abs().max()) == 0.0 and float(w[1:][:, term].abs().max()) == 0.0 and float(w[0].min()) == 1.0
    assert 'discount_loss' in mets
    out, pre = {}, case + '.'
    for k, v in mets.items():
        out[f'{pre}metrics.{k}'] = np.asarray(torch.as_tensor(v).detach().numpy())
    out[f'{pre}metric_keys'] = np.array(sorted(mets))
    for k, v in cap.items():
        out[pre + k] = v.numpy()
    n_rssm = 0
    for n, gr in grads['model'].items():
        if n.startswith(('wm.heads.discount.', 'wm.rssm.')):
            out[f'{pre}grad.model.{n}'] = mv2.grad_rows(gr.numpy())
            n_rssm += n.startswith('wm.rssm.')
    assert n_rssm > 5
    for ph in ('actor', 'critic'):
        for n, gr in grads[ph].items():
            out[f'{pre}grad.{ph}.{n}'] = mv2.grad_rows(gr.numpy())
    for n, v in det.items():
        out[f'{pre}shape.{n}'] = np.array(v.shape, np.int64)
    out[f'{pre}meta'] = np.array([B, T, A, S, K, H, seed])
    out[f'{pre}hyper'] = np.array([ag.cfg.discount, ag.cfg.discount_lambda, ag.cfg.loss_scales['discount'], ag.cfg.actor_ent,
                                   float(bool(ag.cfg.reward_ema))], np.float64)
    gd = grads['model']['wm.heads.discount._out._out.weight']
    print(f"{case}: discount_loss {float(mets['discount_loss']):.6f}, actor_loss {float(mets['actor_loss']):.6f}, critic_loss "
          f"{float(mets['critic_loss']):.6f}; weight {float(w.min()):.4f} .. {float(w.max()):.4f}; |d head| max {float(gd.abs().max()):.3e}; "
          f"grad_heads {list(ag.cfg.grad_heads)}, actor_ent {ag.cfg.actor_ent}, reward_ema {ag.cfg.reward_ema}", flush=True)
    return out


def main():
    o, worst = {}, []
    for case in C.CASES:
        for seed in SEEDS:
            del mdg.margins[:]
            out = run(case, seed)
            print(case, 'seed', seed, 'smallest relative margin between the two best candidates of a race:', min(mdg.margins), 'over',
                  len(mdg.margins), 'draws', flush=True)
            if min(mdg.margins) >= mdg.MARGIN:
                break
        else:
            raise AssertionError(f'{case}: no seed of {SEEDS} keeps the margin {mdg.MARGIN}')
        o.update(out)
        worst.append(min(mdg.margins))
    o['race_margin'] = np.array(min(worst))
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/discount_tiny.npz'
    np.savez_compressed(path, **o)
    print('discount_tiny.npz', len(o), os.path.getsize(path), 'bytes; v2_tiny.npz', os.path.getsize(f'{HERE}/v2_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/v2_tiny.npz')


if __name__ == '__main__':
    main()
