"""Plain-torch restatement of the connector (VideoSSM) with its four switches -- `temporal_embeds`, `token_dropout`, `detached_post` and
`learn_initial` -- written from their semantics on the layer functions of oracle/genrl_oracle.py, for any floating dtype:
test_connector_golden.py checks it in float64 against the reference's vectors (tests/golden/connector_tiny.npz), the GPU tests use it as
the reference where the fixture has no case (autograd supplies its gradients).

  actions    [embedding * sqrt(E) | n_frames slots]; the slots are zeros, or one_hot(t % n_frames) with t the position inside the tensor
             that is handed in (so the length-1 sequences of the initial-KL metric always get slot 0)
  initial    the zero state, or deter_0 = MLP(first action) with stoch_0 sampled from its prior
  update     teacher-forced prior pass: at every step t (0 included) the previous stoch -- the initial state's at t = 0, the world
             model's posterior of t-1 after -- times keep[t, b] (one flag per row and step; deter is not masked), then dense, GRU, prior
             head; loss = aligner cosine distance + loss_scale * KL(posterior, prior); the posterior is a constant of that loss unless
             detached_post is False.  The initial-KL metric re-initialises at every chunk but the first and is never masked.
  imagine    open loop from initial(first action) in mode, over all T steps or restarting deter at every chunk of n_frames
"""
import math

import torch
import torch.nn.functional as F

from oracle import genrl_oracle as O
import klmodes_restatement as KR

CONNECTOR_KL = dict(free=0.0, forward=True, balance=0.8, free_avg=False)         # agent/genrl.yaml, unchanged by the cases
PRE = 'wm.connector.'


def actions(cfg, embed, temporal):
    """embed (B, T, E) -> (B, T, E + n_frames)"""
    B, T = embed.shape[:2]
    slots = embed.new_zeros(B, T, cfg.n_frames)
    if temporal:
        t = torch.arange(T)
        slots[:, t, t % cfg.n_frames] = 1.0
    return torch.cat([embed * math.sqrt(cfg.clip_dim), slots], -1)


def initial(p, cfg, action0, q, learn):
    if learn:
        return O.connector_initial(p, cfg, action0, q, PRE)
    R = action0.shape[0]
    return dict(stoch=action0.new_zeros(R, cfg.stoch, cfg.discrete), deter=action0.new_zeros(R, cfg.deter),
                logit=action0.new_zeros(R, cfg.stoch, cfg.discrete))


def keep_flags(u, p):
    """the reference's `rand > p` on stored uniforms (T, B) -> 0/1 floats"""
    return (u > p).to(u.dtype)


def update(p, cfg, clip_video, wm_post, noise, sw, keep=None, kl=CONNECTOR_KL, lafite=0.5, loss_scale=1.0):
    """-> loss, metrics, dict(prior_logit (B,T,S,K), kl_value (B,T)).  wm_post: 'stoch' and 'logit' (B,T,S,K), attached or not;
    noise: 'clip_eps' (B,T,E), 'init_q', 'ikl_init_q', 'ikl_step_q' (read with learn_initial only, but for ikl_step_q); keep (T,B)"""
    nf = cfg.n_frames
    B, T = clip_video.shape[:2]
    G = T // nf
    clean = clip_video[:, nf - 1::nf].reshape(B, G, 1, -1).repeat(1, 1, nf, 1).reshape(B, T, -1)
    noisy = F.normalize((1 - lafite) * clean + lafite * F.normalize(noise['clip_eps'].to(clean.dtype), dim=-1), dim=-1)
    restored = F.normalize(O.aligner(p, noisy, f'{PRE}aligner.'), dim=-1)
    cosine_distance = 1 - F.cosine_similarity(restored, clean, dim=-1).mean()
    act = actions(cfg, clean, sw['temporal_embeds'])
    post = wm_post if not sw['detached_post'] else {k: v.detach() for k, v in wm_post.items()}
    state = initial(p, cfg, act[:, 0], noise.get('init_q'), sw['learn_initial'])
    stoch, deter, logits = state['stoch'], state['deter'], []
    for t in range(T):
        if t > 0:
            stoch = post['stoch'][:, t - 1]
        if sw['token_dropout'] > 0:
            stoch = stoch * keep[t].to(stoch.dtype)[:, None, None]
        step = O.img_step(p, cfg, PRE, stoch, deter, act[:, t], None)            # (the step's own sample feeds nothing)
        deter = step['deter']
        logits.append(step['logit'])
    prior_logit = torch.stack(logits, 1)
    kl_loss, kl_value = KR.kl_loss({'logit': post['logit']}, {'logit': prior_logit}, **kl)
    loss = cosine_distance + loss_scale * kl_loss
    metrics = dict(aligner_cosine_distance=cosine_distance, connector_kl=kl_value.mean())
    with torch.no_grad():
        heads = lambda v: v.reshape(B, G, nf, *v.shape[2:])[:, 1:, 0].reshape(B * (G - 1), *v.shape[2:])
        a = actions(cfg, heads(clean).unsqueeze(1), sw['temporal_embeds'])[:, 0]
        state = initial(p, cfg, a, noise.get('ikl_init_q'), sw['learn_initial'])
        step = O.img_step(p, cfg, PRE, state['stoch'], state['deter'], a, noise['ikl_step_q'])
        metrics['connector_initial_kl'] = KR.kl_loss({'logit': heads(post['logit']).detach()}, {'logit': step['logit']}, **kl)[1].mean()
    return loss, metrics, dict(prior_logit=prior_logit, kl_value=kl_value)


def video_imagine(p, cfg, embed, sw, init_q, reset, dreamer_init=None):
    """VideoSSM.video_imagine(sample=False, denoise=False) -> dict of (B, T, ..): 'stoch', 'deter', 'logit'"""
    B, T = embed.shape[:2]
    act = actions(cfg, embed, sw['temporal_embeds'])
    state = initial(p, cfg, act[:, 0], init_q, sw['learn_initial'])
    if dreamer_init is not None:
        state['stoch'] = dreamer_init['stoch']
    outs = []
    for t in range(T):
        if reset and t > 0 and t % cfg.n_frames == 0:                # deter restarts at every chunk; stoch carries over
            state = dict(state, deter=torch.zeros_like(state['deter']))
        state = O.img_step(p, cfg, PRE, state['stoch'], state['deter'], act[:, t], None)
        outs.append(state)
    return {k: torch.stack([d[k] for d in outs], 1) for k in outs[0]}
