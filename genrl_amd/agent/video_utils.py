"""The connector of the GenRL hot path: a state-space model driven by video-language embeddings
(VideoSSM) plus the embedding denoiser in front of it (UNetDenoiser).

API and parameter names follow mazpie/genrl `agent/video_utils.py` (SURVEY.md §8a row a15/a18 and the
weight contract), so published checkpoints load; the computation is organised for the HIP ops:
everything that does not depend on the recurrence is evaluated for all T steps at once and only the
GRU recurrence itself runs as a scan (`ops.gru_seq`).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dreamer_utils as common
from .. import noise, ops


def _unit(x):
    return F.normalize(x, dim=-1)


class ResidualLinear(nn.Module):
    """y = act(norm(W x + b)) + proj(x)   (agent/video_utils.py:8-25; `prenorm` is never set)."""
    def __init__(self, in_channels, out_channels, norm='layer', act='SiLU', prenorm=False):
        super().__init__()
        assert not prenorm
        self.layer = nn.Linear(in_channels, out_channels)
        self.norm_layer = common.NormLayer(norm, out_channels)
        self.act = common.get_act(act)
        self.res_proj = nn.Linear(in_channels, out_channels) if in_channels != out_channels else nn.Identity()
        self._fused = norm != 'none'                    # Linear + LayerNorm + SiLU as one node
        assert self._fused != isinstance(self.act, nn.Identity)

    def forward(self, x):
        if self._fused:
            y = common._dense_ln_silu(x, self.layer, self.norm_layer)
        else:
            y = ops.linear(x, self.layer.weight, self.layer.bias)
        skip = x if isinstance(self.res_proj, nn.Identity) else ops.linear(x, self.res_proj.weight, self.res_proj.bias)
        return y + skip


class UNetDenoiser(nn.Module):
    """n_layers down (last one narrows to mid_channels), n_layers mid, n_layers up with skip
    concatenation, first up-layer linear (agent/video_utils.py:27-61)."""
    def __init__(self, in_channels, mid_channels, n_layers, norm='layer', act='SiLU'):
        super().__init__()
        widths = [in_channels] * (n_layers - 1) + [mid_channels]
        block = lambda i, o: ResidualLinear(i, o, norm=norm, act=act)
        self.down = nn.ModuleList(block(in_channels, w) for w in widths)
        self.mid = nn.ModuleList(block(mid_channels, mid_channels) for _ in range(n_layers))
        ups = [ResidualLinear(2 * mid_channels, in_channels, norm='none', act='Identity')]
        ups += [block(2 * in_channels, in_channels) for _ in range(n_layers - 1)]
        self.up = nn.ModuleList(ups)

    def forward(self, x):
        skips = []
        for f in self.down:
            x = f(x)
            skips.append(x)
        for f in self.mid:
            x = f(x)
        for f in self.up:
            x = f(torch.cat([x, skips.pop()], dim=-1))
        return x


class VideoSSM(common.EnsembleRSSM):
    def __init__(self, *args, connector_kl={}, temporal_embeds=False, detached_post=True, n_frames=8,
                 token_dropout=0., loss_scale=1, clip_add_noise=0, clip_lafite_noise=0, rescale_embeds=False,
                 denoising_ae=False, learn_initial=True, **kwargs):
        super().__init__(*args, **kwargs)
        if self._act != 'SiLU':          # (the aligner, the action MLP and the teacher-forced prior below are SiLU layers)
            raise NotImplementedError(f"the connector runs SiLU layers: `connector_rssm.act` is {self._act!r} (DESIGN 5n)")
        if connector_kl.get('free_avg', False):
            # the reference's connector raises on it: its free_avg loss has shape [1] and VideoSSM.update adds it in place into a 0-d
            # tensor (agent/video_utils.py:195), so there is nothing to compare against
            raise NotImplementedError('`connector_kl.free_avg: True` is refused: the reference\'s connector raises on it (DESIGN 5o)')
        if not 0 <= token_dropout < 1:
            raise ValueError(f'`connector.token_dropout` is a probability below 1, not {token_dropout!r}')
        hidden, deter, norm, act_dim = kwargs['hidden'], kwargs['deter'], kwargs['norm'], kwargs['action_dim']
        self.n_frames = n_frames
        self.viclip_emb_dim = act_dim - n_frames
        self.clip_const = math.sqrt(self.viclip_emb_dim)
        self.connector_kl, self.loss_scale = connector_kl, loss_scale
        self.clip_add_noise, self.clip_lafite_noise = clip_add_noise, clip_lafite_noise
        self.temporal_embeds, self.token_dropout, self.detached_post = temporal_embeds, token_dropout, detached_post
        self.rescale_embeds, self.denoising_ae, self.learn_initial = rescale_embeds, denoising_ae, learn_initial
        if denoising_ae:
            self.aligner = UNetDenoiser(self.viclip_emb_dim, self.viclip_emb_dim // 2, n_layers=2, norm='layer', act='SiLU')
        if learn_initial:                                          # (:88-95; without it initial() is the zero state)
            mlp = [nn.Linear(act_dim, hidden), common.NormLayer(norm, hidden), common.get_act('SiLU'),
                   nn.Linear(hidden, hidden), common.NormLayer(norm, hidden), common.get_act('SiLU'),
                   nn.Linear(hidden, deter)]
            self.initial_state_pred = nn.Sequential(*mlp)          # learned deter_0 from the first "action"
        del self._obs_out, self._obs_dist                      # a connector has no observation posterior

    # ------------------------------------------------------------------ pieces
    def get_action(self, video_embed):
        """The SSM's 'action' = [clip embedding (optionally x sqrt(E)) | n_frames slots]  (:114-125).  The slots are zeros, or with
        `temporal_embeds` one_hot(t % n_frames), t the position along dimension 1 of what was handed in."""
        if self.rescale_embeds:
            video_embed = video_embed * self.clip_const
        if self.temporal_embeds:
            # (device arithmetic only: an indexed assignment copies its scalar from the host, which a hipGraph capture refuses)
            B, T = video_embed.shape[:2]
            t = torch.arange(T, device=video_embed.device)[:, None] % self.n_frames
            slots = (t == torch.arange(self.n_frames, device=video_embed.device)[None]).to(video_embed.dtype)
            return torch.cat([video_embed, slots[None].expand(B, T, self.n_frames)], dim=-1)
        pad = video_embed.new_zeros(*video_embed.shape[:-1], self.n_frames)
        return torch.cat([video_embed, pad], dim=-1)

    def _initial_deter(self, action0):
        fc = self.initial_state_pred
        h = common._dense_ln_silu(action0, fc[0], fc[1])
        h = common._dense_ln_silu(h, fc[3], fc[4])
        return ops.linear(h, fc[6].weight, fc[6].bias)

    def initial(self, batch_size, init_embed=None, ignore_learned=False, site='conn.init_q'):
        """Zero state, or (learned) deter_0 = MLP(first action) with stoch_0 sampled from its prior (:100-112)."""
        state = super().initial(batch_size)
        if ignore_learned or not self.learn_initial:
            return state
        assert init_embed is not None
        if init_embed.shape[-1] == self.viclip_emb_dim:        # bare embedding: append the frame slots
            init_embed = torch.cat([init_embed, init_embed.new_zeros(*init_embed.shape[:-1], 8)], -1)
        state['deter'] = self._initial_deter(init_embed)
        stoch, stats = self.get_stoch_stats_from_deter_state(state, site=site)
        state['stoch'] = stoch
        state.update(stats)
        return state

    def _noisy(self, clean):
        """Training-time corruption of the (unit) embeddings: additive and/or 'lafite' mixing noise."""
        e, dev = clean, clean.device
        if self.clip_add_noise > 0:
            e = _unit(e + self.clip_add_noise * noise.draw('normal', 'conn.add_eps', e.shape, dev))
        if self.clip_lafite_noise > 0:
            lam = self.clip_lafite_noise
            e = _unit((1 - lam) * e + lam * _unit(noise.draw('normal', 'conn.clip_eps', e.shape, dev)))
        return e

    def _prior_under_teacher_forcing(self, actions_tm, post_stoch, B, T):
        """Prior logits (B,T,S,K) of the connector when stoch_{t-1} is the world model's posterior
        (stoch_{-1}: the learned initial state).  actions_tm: (T,B,A)."""
        S, K = self._stoch, self._discrete
        first = self.initial(B, init_embed=actions_tm[0])
        if self.token_dropout > 0:
            # stoch_{t-1} times one keep flag per row and step, step 0 included (:178-179): `rand > p` on u = exp(-e), e ~ Exp(1)
            e = noise.draw('exp', 'conn.drop', (T, B), actions_tm.device)
            shifted, _ = ops.tf_inputs(first['stoch'].reshape(B, S * K), post_stoch.reshape(B, T, S * K), e, float(self.token_dropout))
        else:
            shifted = torch.cat([first['stoch'].reshape(1, B, S * K), post_stoch.reshape(B, T, S * K).transpose(0, 1)[:-1]], 0)
        x = common._dense_ln_silu(shifted.reshape(T * B, S * K), self._img_in[0], self._img_in[1],
                                  actions_tm.reshape(T * B, -1))
        deter = ops.gru_seq(x.reshape(T, B, -1), None, first['deter'], self._cell._layer.weight,
                            self._cell._norm.weight, self._cell._norm.bias)
        return self._prior_logits(deter.reshape(T * B, -1)).reshape(T, B, S, K).transpose(0, 1)

    def _initial_kl(self, embeds, post, B, T):
        """Metric: KL at the first step of every chunk but the first when the state is re-initialised
        from that chunk's embedding (:197-205).  No gradient."""
        nf, G = self.n_frames, T // self.n_frames
        heads = lambda v: v.reshape(B, G, nf, *v.shape[2:])[:, 1:, 0].reshape(B * (G - 1), *v.shape[2:])
        a = self.get_action(heads(embeds).unsqueeze(1))[:, 0]         # (length-1 sequences: frame slot 0, :198-201)
        state = self.initial(B * (G - 1), init_embed=a, site='conn.ikl_init_q')
        prior = self.img_step(state, a, site='conn.ikl_step_q')
        return ops.wmean(self.kl_loss({'logit': heads(post['logit'])}, prior, **self.connector_kl)[1], None, 1.0)    # (kl_loss reads the logits only)

    # ------------------------------------------------------------------ training step (:127-207)
    def update(self, video_embed, wm_post):
        nf, dev = self.n_frames, self.device
        B, T = video_embed.shape[:2]
        # one embedding per aligned nf-frame chunk (its last frame's), held over the chunk
        metrics, loss = {}, None
        fused = (self.clip_add_noise == 0 and self.clip_lafite_noise > 0 and self.denoising_ae and video_embed.is_cuda
                 and self.rescale_embeds)
        if fused:
            # chunk embeddings, lafite noise and the SSM's time-major 'actions' in one launch; the aligner's cosine loss
            # (normalize + cosine_similarity + mean) as one node
            eps = noise.draw('normal', 'conn.clip_eps', video_embed.shape, dev)
            clean, embeds, actions_tm = ops.connector_prep(video_embed.to(dev), eps, nf, float(self.clip_lafite_noise),
                                                           float(self.clip_const), temporal=self.temporal_embeds)
            cosine_distance = ops.cosine_distance(self.aligner(embeds), clean)
            metrics['aligner_cosine_distance'] = cosine_distance
            loss = cosine_distance
            embeds = clean
        else:
            # one embedding per aligned nf-frame chunk (its last frame's), held over the chunk
            clean = video_embed[:, nf - 1::nf].to(dev).reshape(B, T // nf, 1, -1).repeat(1, 1, nf, 1).reshape(B, T, -1)
            embeds = self._noisy(clean)
            if self.denoising_ae:
                assert (self.clip_lafite_noise + self.clip_add_noise) > 0, 'Nothing to denoise'
                restored = _unit(self.aligner(embeds))
                cosine_distance = 1 - F.cosine_similarity(restored, clean, dim=-1).mean()
                metrics['aligner_cosine_distance'] = cosine_distance
                loss = cosine_distance
                embeds = clean                                   # the SSM itself consumes the clean embedding
            actions_tm = self.get_action(embeds).transpose(0, 1).contiguous()
        # (detached_post False: the connector trains end to end with the world model, the KL's posterior side and the teacher-forced
        # stoch stay attached, :160-163)
        held = (lambda v: v.detach()) if self.detached_post else (lambda v: v)
        post = {k: held(v.reshape(B, T, *v.shape[2:])) for k, v in wm_post.items()}
        prior_logit = self._prior_under_teacher_forcing(actions_tm, post['stoch'], B, T)
        kl_loss, kl_value = self.kl_loss(post, {'logit': prior_logit}, **self.connector_kl)
        metrics['connector_kl'] = ops.wmean(kl_value.detach(), None, 1.0)
        kl_term = kl_loss if self.loss_scale == 1 else self.loss_scale * kl_loss
        loss = kl_term if loss is None else loss + kl_term
        with torch.no_grad():
            metrics['connector_initial_kl'] = self._initial_kl(embeds, post, B, T)
        return loss, metrics

    # ------------------------------------------------------------------ open-loop generation (:209-240)
    def video_imagine(self, video_embed, dreamer_init=None, sample=True, reset_every_n_frames=True, denoise=False):
        B, T = video_embed.shape[:2]
        if denoise and self.denoising_ae:
            video_embed = _unit(self.aligner(video_embed))
        actions = self.get_action(video_embed)
        state = self.initial(batch_size=B, init_embed=actions[:, 0], site='imag.target_init_q')
        if dreamer_init is not None:
            state[self.cell_input] = dreamer_init[self.cell_input]
        if not reset_every_n_frames:
            return self.imagine(actions, state, sample=sample)
        pieces = []
        for chunk in torch.chunk(actions, T // self.n_frames, dim=1):    # deter restarts at every chunk
            pieces.append(self.imagine(chunk, state, sample=sample))
            state = self.initial(batch_size=B, ignore_learned=True)
            state[self.cell_input] = pieces[-1][self.cell_input][:, -1]
        return {k: torch.cat([p[k] for p in pieces], dim=1) for k in pieces[0]}
