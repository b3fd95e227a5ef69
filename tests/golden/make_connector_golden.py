"""Generate tests/golden/connector_tiny.npz from the reference's VideoSSM (agent/video_utils.py:64-240) with its four switches off their
shipped values: `connector.temporal_embeds: True` (get_action, :114-125), `connector.token_dropout: p` (:178-179),
`connector.detached_post: False` (:160-163, agent/genrl.py:46) and `connector_rssm.learn_initial: False` (:87-112).  Needs a checkout of
mazpie/genrl where ref_harness.REF points (ref_harness imports it from there and refuses to run without it); the tests read only the
stored file:

    python tests/golden/make_connector_golden.py

GenRLAgent, conf/defaults/genrl.yaml at detgen.tiny_overrides(), B2 x T16, A = 10, lr = wd = 0, precision 32, weights from
detgen.det_state_dict and the batch from detgen.det_batch at seed 5; noise replayed through NoiseTape (fully consumed).
The reference's modules are evaluated with float64 as torch's default dtype on these float32 weights, batch and noise (`precision: 32`
stays: no autocast), and the results are stored as float32.  In float32 the reference's own rounding of the end-to-end cases' world-model
gradients -- a backward pass through a loss of 2600 -- is 2e-6 of the largest element, above the 1e-5 / 1e-6 bound the CPU test holds the
float64 restatement to.  The reference builds its distributions on `logit.float()`, so its sampled latents are cast back to the default
dtype (`wide_samples`); the KL, the entropies and the twohot likelihood are still float32 arithmetic inside.
One `update_wm`, which includes the first connector update:
  'temporal' : temporal_embeds
  'drop'     : token_dropout 0.25
  'noinit'   : learn_initial False (no initial_state_pred: ten state_dict entries fewer, no draw for an initial state)
  'e2e'      : detached_post False (one backward, one optimiser call over the world model and the connector)
  'all'      : all four
The reference draws the dropout's flags with torch.rand(B), which is no NoiseTape kind: for the duration of a run torch.rand is swapped for
a function that hands out the rows of a stored (T, B) tensor of uniforms, and restored afterwards.  The uniforms come from the first seed of
NOISE_SEEDS under which every one of them lies at least 1e-3 from p, and step 0 and some later step each have a kept and a dropped row.
In 'e2e' the sampled wm.encoder gradients must differ from those of the same run with detached_post True by more than the GPU tests'
gradient tolerance (rtol 1e-3, atol 1e-5 max|reference|): else the case would pin nothing.

Per case: every metric; the connector KL's posterior and prior logits and its per-row value; the uniforms and the keep flags (dropout
cases); the gradients sampled by make_v2_golden.grad_rows -- the connector's but its aligner's for every case, wm.rssm.* and wm.encoder.*
for 'e2e' and 'all'; the name and shape of every state_dict entry (`shape_names`, `shape_dims` padded with -1); for 'temporal', 'noinit'
and 'all' the logit and deter of one video_imagine(sample=False) call on the batch's clip embeddings per value of reset_every_n_frames (its initial-state draw: detgen noise
'vi.init_q').  Arrays only; no reference text is stored.  The file must be no larger than klmodes_tiny.npz."""
import os, sys, zlib
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh
import detgen
import make_v2_golden as mv2

torch.set_num_threads(8)
SEED = 5
B, T, A = 2, 16, 10
P = 0.25
NOISE_SEEDS = (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)        # tried in this order for the dropout's uniforms
# case: temporal_embeds, token_dropout, detached_post, learn_initial
CASES = {
    'temporal': (True, 0.0, True, True),
    'drop': (False, P, True, True),
    'noinit': (False, 0.0, True, False),
    'e2e': (False, 0.0, False, True),
    'all': (True, P, False, False),
}
IMAGINED = ('temporal', 'noinit', 'all')


class Margin(AssertionError):
    pass


def uniforms(nseed):
    g = np.random.Generator(np.random.PCG64([zlib.crc32(b'noise:conn.drop'), nseed]))
    return g.random((T, B)).astype(np.float32)


def check_uniforms(u, p):
    keep = u > p
    if float(np.abs(u - p).min()) < 1e-3:
        raise Margin(f'a uniform lies {float(np.abs(u - p).min()):.2e} from p')
    mixed = [bool(keep[t].any() and not keep[t].all()) for t in range(T)]
    if not (mixed[0] and any(mixed[1:])):
        raise Margin(f'steps with a kept and a dropped row: {[t for t in range(T) if mixed[t]]}')


def pick_noise_seed():
    for nseed in NOISE_SEEDS:
        try:
            check_uniforms(uniforms(nseed), P)
            return nseed
        except Margin as e:
            print(f'noise seed {nseed} rejected:', e, flush=True)
    raise AssertionError(f'no noise seed of {NOISE_SEEDS} passes the margins')


class wide_samples:
    """Inside rh.inject_noise: the sampled one-hot latents come out in torch's default dtype.  The reference builds its distributions on
    `logit.float()` (agent/dreamer_utils.py:415, :836), so under a float64 default its samples are float32 and its float64 layers refuse
    them; the values (0 / 1 plus the straight-through term) and the gradient path are unchanged by the cast."""
    def __enter__(self):
        m = rh.ref_modules()
        self._inner = inner = m.common.OneHotDist.sample
        m.common.OneHotDist.sample = lambda self_, *a, **k: inner(self_, *a, **k).to(torch.get_default_dtype())

    def __exit__(self, *a):
        rh.ref_modules().common.OneHotDist.sample = self._inner


class RandRows:
    """stands in for torch.rand during a run: call t returns row t of the stored uniforms"""
    def __init__(self, u):
        self.u, self.pos = torch.from_numpy(u), 0

    def __call__(self, *size, **kw):
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        assert size == (self.u.shape[1],), size
        self.pos += 1
        return self.u[self.pos - 1].clone()


def f32(t):
    return t.numpy().astype(np.float32)


def make_agent(switches):
    temporal, p, detached, learn = switches
    over = dict(detgen.tiny_overrides())
    for k in ('model_opt', 'actor_opt', 'critic_opt'):
        over[k] = dict(lr=0.0, wd=0.0)
    over['connector_rssm'] = dict(over['connector_rssm'], learn_initial=learn)
    over['connector'] = dict(temporal_embeds=temporal, token_dropout=p, detached_post=detached)
    over['imag_reward_fn'] = 'video_text_reward'           # (the imagination behaviour exists, as train.py builds it)
    ag = rh.make_ref_agent(B, T, A=A, **over)
    det = detgen.det_state_dict({k: v.shape for k, v in ag.state_dict().items()}, SEED)
    ag.load_state_dict(det)
    return ag, det


def run(case, switches, nseed):
    """-> the stored arrays of one update_wm (and the video_imagine calls) under `switches`"""
    temporal, p, detached, learn = switches
    ag, det = make_agent(switches)
    S, K = ag.cfg.rssm.stoch, ag.cfg.rssm.discrete
    noise = detgen.iteration_noise(B, T, S, K, A, ag.cfg.imag_horizon, seed=SEED)
    tape, c = [], noise['conn1']
    for t in range(T):
        tape.append(('exp', noise['wm']['prior_q'][t])); tape.append(('exp', noise['wm']['post_q'][t]))
    tape.append(('randn_like', c['clip_eps']))
    if learn:
        tape.append(('exp', c['init_q']))
    for t in range(T):
        tape.append(('exp', c['step_q'][t]))
    if learn:
        tape.append(('exp', c['ikl_init_q']))
    tape.append(('exp', c['ikl_step_q']))
    tape = rh.NoiseTape('replay', tape)
    names = {id(q): n_ for n_, q in ag.named_parameters()}
    grads, cap = [], {}
    orig_clip, orig_rand = torch.nn.utils.clip_grad_norm_, torch.rand

    def clip_capture(params, clip, *a, **k):
        params = list(params)
        grads.append({names[id(q)]: q.grad.detach().clone() for q in params if q.grad is not None})
        return orig_clip(params, clip, *a, **k)
    conn, orig_ckl = ag.wm.connector, ag.wm.connector.kl_loss

    def ckl_hook(post, prior, **kw):
        loss, value = orig_ckl(post, prior, **kw)
        if 'conn_kl_value' not in cap:               # (the second call is the initial-KL metric)
            cap.update(conn_post_logit=post['logit'].detach().clone(), conn_prior_logit=prior['logit'].detach().clone(),
                       conn_kl_value=value.detach().clone())
        return loss, value
    conn.kl_loss = ckl_hook
    batch = detgen.det_batch(B, T, A=A, seed=SEED)
    tb = {k: v.double() if v.is_floating_point() else v for k, v in rh.to_torch(batch).items()}
    rows = RandRows(uniforms(nseed)) if p > 0 else None
    torch.nn.utils.clip_grad_norm_ = clip_capture
    if rows is not None:
        torch.rand = rows
    try:
        with rh.inject_noise(tape), wide_samples():
            state, outputs, mets = ag.update_wm(tb, 0)
    finally:
        torch.nn.utils.clip_grad_norm_, torch.rand = orig_clip, orig_rand
        conn.kl_loss = orig_ckl
    assert tape.pos == len(tape.tape), (tape.pos, len(tape.tape))
    assert rows is None or rows.pos == T, rows.pos
    assert len(grads) == (2 if detached else 1), len(grads)
    out, pre = {}, case + '.'
    for k, v in mets.items():
        out[f'{pre}metrics.{k}'] = f32(torch.as_tensor(v).detach())
    out[f'{pre}metric_keys'] = np.array(sorted(mets))
    for k, v in cap.items():
        out[pre + k] = f32(v)
    if rows is not None:
        out[f'{pre}drop_u'] = rows.u.numpy()
        out[f'{pre}keep'] = (rows.u.numpy() > p).astype(np.float32)
    for n_, gr in grads[-1].items():
        if n_.startswith('wm.connector.') and '.aligner.' not in n_:
            out[f'{pre}grad.connector.{n_}'] = mv2.grad_rows(f32(gr))
    if not detached:
        for n_, gr in grads[0].items():
            if n_.startswith(('wm.rssm.', 'wm.encoder.')):
                out[f'{pre}grad.model.{n_}'] = mv2.grad_rows(f32(gr))
    out[f'{pre}shape_names'] = np.array(list(det))               # (two arrays per case: an entry per tensor would outweigh the data)
    out[f'{pre}shape_dims'] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in det.values()], np.int64)
    out[f'{pre}meta'] = np.array([B, T, A, S, int(K), SEED, nseed])
    out[f'{pre}switches'] = np.array([float(temporal), float(p), float(detached), float(learn)])
    if case in IMAGINED:
        emb = tb['clip_video']
        for reset in (True, False):
            vt = rh.NoiseTape('replay', [('exp', detgen.det_noise('vi.init_q', (B * S, K), 'exp', SEED))] if learn else [])
            with rh.inject_noise(vt), wide_samples(), torch.no_grad():
                vi = conn.video_imagine(emb, sample=False, reset_every_n_frames=reset)
            assert vt.pos == len(vt.tape)
            for key in ('logit', 'deter'):
                out[f'{pre}vi.{int(reset)}.{key}'] = f32(vi[key].detach())
    v = cap['conn_kl_value']
    print(f"{case}: connector rows {float(v.min()):.4f} .. {float(v.max()):.4f}, connector_kl {float(mets['connector_kl']):.6f}, "
          f"model_loss {float(mets['model_loss']):.4f}, {sorted(k for k in mets if 'connector' in k)}", flush=True)
    return out, grads


def main():
    torch.set_default_dtype(torch.float64)
    nseed = pick_noise_seed()
    o = {}
    for case, switches in CASES.items():
        o.update(run(case, switches, nseed)[0])
    temporal, p, _, learn = CASES['e2e']
    _, grads = run('e2e with detached_post', (temporal, p, True, learn), nseed)          # (its arrays are not stored)
    det = {n_: mv2.grad_rows(f32(gr)) for n_, gr in grads[0].items() if n_.startswith('wm.encoder.')}
    moved = 0
    for n_, ref in det.items():
        got = o[f'e2e.grad.model.{n_}']
        moved += bool((np.abs(got - ref) > 1e-3 * np.abs(ref) + 1e-5 * np.abs(ref).max()).any())
    print(f'e2e: {moved} of {len(det)} wm.encoder gradients differ from the detached run by more than the gradient tolerance', flush=True)
    assert moved == len(det) and moved > 0, (moved, len(det))
    o['torch_version'] = np.array(torch.__version__)
    path = f'{HERE}/connector_tiny.npz'
    np.savez_compressed(path, **o)
    print('connector_tiny.npz', len(o), os.path.getsize(path), 'bytes; klmodes_tiny.npz', os.path.getsize(f'{HERE}/klmodes_tiny.npz'))
    assert os.path.getsize(path) <= os.path.getsize(f'{HERE}/klmodes_tiny.npz')


if __name__ == '__main__':
    main()
