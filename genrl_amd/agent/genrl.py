"""GenRLAgent for the MI355X-native hot path.

Drop-in for the class `train.py` instantiates through `agent.genrl.GenRLAgent` (same constructor
keywords, attributes, method names and metric keys — SURVEY.md §8b): a DreamerAgent whose world
model carries a video-language *connector* (VideoSSM) that is trained next to it, and whose
imagination behaviour is rewarded by a language/video target instead of the environment.
Reference locations are cited per member; the bodies are organised around the batched HIP ops.
"""
import re
import torch

from .dreamer import DreamerAgent, ActorCritic, stop_gradient, env_reward
from . import dreamer_utils as common
from . import video_utils
from .. import streams
from ..tools.genrl_utils import *          # reward functions are resolved by NAME from this namespace


N_FRAMES = 8                                # frames summarised by one InternVideo2 clip embedding
DEFAULT_EMBED_DIM = 512


def connector_update_fn(self, module_name, data, outputs, metrics):
    """`update_fn` registered with WorldModel.add_module_to_update (agent/genrl.py:7-25): trains the
    connector on the batch's clip embeddings against the world model's (detached) posterior."""
    if not getattr(self.cfg, 'viclip_encode', False):
        raise NotImplementedError('on-the-fly InternVideo2 embedding is host-side preprocessing; provide '
                                  "data['clip_video'] (viclip_encode=True), as process_dataset.py does")
    return getattr(self, module_name).update(data['clip_video'], outputs['post'])


def _chunk_embeddings(clip, n_frames, first, B, T):
    """One embedding per aligned n_frames chunk (taken at the chunk's last frame, starting at
    index `first`), held for the whole chunk: (B, T, E)."""
    picked = clip[:B, first::n_frames]
    return picked.reshape(B, T // n_frames, 1, -1).expand(-1, -1, n_frames, -1).reshape(B, T, -1)


class GenRLAgent(DreamerAgent):
    def __init__(self, **kwargs):  # agent/genrl.py:28-49
        cfg = kwargs['cfg']
        if not cfg.rssm.get('discrete', False) or not cfg.connector_rssm.get('discrete', False):
            raise NotImplementedError('GenRLAgent needs discrete latents (`rssm.discrete`, `connector_rssm.discrete`): its connector '
                                      'teacher-forces one-hot latents; continuous latents are built for DreamerAgent and Plan2Explore')
        if cfg.get('pred_discount', False):
            raise NotImplementedError('GenRLAgent is built without the discount head (conf/env/dmc_pixels.yaml:6): `pred_discount: True` '
                                      'is built for DreamerAgent and Plan2Explore')
        for part in ('encoder', 'decoder'):
            vec = [k for k, v in kwargs['obs_space'].items() if len(v.shape) == 1 and re.match(cfg[part].get('mlp_keys', r'.*'), k)]
            if vec:
                raise NotImplementedError(f'GenRLAgent is built on one image key: `{part}.mlp_keys` selects {vec}; vector observations '
                                          'are built for DreamerAgent and Plan2Explore')
        for block in ('rssm', 'encoder', 'decoder', 'reward_head', 'actor', 'critic', 'connector_rssm'):
            if cfg[block].get('act', 'SiLU') != 'SiLU':
                raise NotImplementedError(f"GenRLAgent runs SiLU blocks: `{block}.act` is {cfg[block]['act']!r}; its connector, the batched "
                                          "observe and the fused rollout have SiLU built in.  `act: ELU` is built for DreamerAgent and "
                                          "Plan2Explore")
        super().__init__(**kwargs)
        self.n_frames = N_FRAMES
        assert self.cfg.batch_length % self.n_frames == 0, 'Fix batch length param'
        clip_spec = self.obs_space['clip_video'] if 'clip_video' in self.obs_space else None
        self.viclip_emb_dim = clip_spec.shape[0] if clip_spec is not None else DEFAULT_EMBED_DIM
        self._attach_connector()
        if getattr(self.cfg, 'imag_reward_fn', None) is not None:
            self.instantiate_imag_behavior()

    def _attach_connector(self):
        cfg = self.cfg
        opts = dict(cfg.connector)
        opts.update(cfg.connector_rssm)
        opts.update(connector_kl=cfg.connector_kl, n_frames=self.n_frames, cell_input='stoch', device=self.device,
                    action_dim=self.viclip_emb_dim + self.n_frames,      # embedding + per-frame slots
                    clip_add_noise=cfg.clip_add_noise, clip_lafite_noise=cfg.clip_lafite_noise)
        connector = video_utils.VideoSSM(**opts).to(self.device)
        connector.requires_grad_(False)
        self.wm.add_module_to_update('connector', connector, connector_update_fn, detached=cfg.connector.detached_post)

    def instantiate_imag_behavior(self):  # agent/genrl.py:51-54
        behavior = ActorCritic(self.cfg, self.act_spec, self.wm.inp_size, name='imag').to(self.device)
        behavior.requires_grad_(False)
        behavior.rewnorm = common.StreamNorm(**self.cfg.imag_reward_norm, device=self.device)
        self._imag_behavior = behavior

    def finetune_mode(self):  # agent/genrl.py:56-60
        if self.wm.e2e_update_fns:          # (a connector that trained end to end sat in the world model's Adam group: it leaves it)
            self.wm.model_opt.release([p for k in self.wm.e2e_update_fns for p in getattr(self.wm, k).parameters()])
        self.wm.detached_update_fns, self.wm.e2e_update_fns = {}, {}
        self.wm.grad_heads.append('reward')
        self._acting_behavior = self._imag_behavior

    # ------------------------------------------------------------------ reporting (agent/genrl.py:64-106)
    def report(self, data, key='observation', nvid=8):
        """Adds 'video_clip_pred': ground truth | reconstruction of the first chunk followed by the
        connector's open-loop video prediction from the later chunks' embeddings | error."""
        assert getattr(self.cfg, 'viclip_encode', False)
        wm, nf = self.wm, self.wm.connector.n_frames
        with torch.no_grad():
            out = super().report(data)
            rows, horizon = data['observation'][:nvid, nf:].shape[:2]
            decode = lambda states: wm.heads['decoder'](wm.decoder_input_fn(states))[key].mean
            # context: posterior over the first chunk
            embed = wm.encoder(wm.preprocess(data))
            context, _ = wm.rssm.observe(embed[:nvid, :nf], data['action'][:nvid, :nf], data['is_first'][:nvid, :nf])
            last = {name: value[:, -1] for name, value in context.items()}
            # continuation: connector rollout driven by the remaining chunks' clip embeddings
            clips = _chunk_embeddings(data['clip_video'].to(self.device), nf, 2 * nf - 1, rows, horizon)
            dreamed = wm.connector.video_imagine(clips, last, reset_every_n_frames=False)
            frames = torch.cat([decode(context)[:nvid, :nf] + 0.5, decode(dreamed) + 0.5], 1).clamp(0, 1)
            truth = data[key][:nvid].float() / 255
            out['video_clip_pred'] = torch.cat([truth, frames, (frames - truth + 1) / 2], 3)
        return out

    # ------------------------------------------------------------------ imagination (agent/genrl.py:108-124)
    def update_imag_behavior(self, state=None, outputs=None, metrics={}, seq_data=None):
        self._apply_precision()
        name = getattr(self.cfg, 'imag_reward_fn', None)
        if name is None:
            # (pre-training: no behaviour update follows the connector updates that cfg.overlap_detached put on the side
            # stream; they must be ordered before the caller reuses or frees the batch / posterior they read)
            streams.join()
            return outputs['post'], metrics
        post, is_terminal = self._posterior_for(outputs, seq_data)
        start = {k: stop_gradient(v) for k, v in post.items()}
        reward = globals()[name]                                    # e.g. video_text_reward
        extra = self.cfg.imag_reward_args
        metrics.update(self._imag_behavior.update(self.wm, start, is_terminal, lambda seq: reward(self, seq, **extra)))
        streams.join()          # side-stream connector updates (cfg.overlap_detached) are ordered from here on
        return start, metrics
