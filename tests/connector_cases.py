"""The cases of tests/golden/connector_tiny.npz as the CPU and the GPU tests read them: the switches of each case come from the arrays the
generator stored (`switches`, `meta`), never from a second table."""
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('temporal', 'drop', 'noinit', 'e2e', 'all')
IMAGINED = ('temporal', 'noinit', 'all')              # the cases that store video_imagine outputs
RESETS = (True, False)                                # ... one call per value of reset_every_n_frames
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'connector_tiny.npz')))
    return _cache['g']


def switches_of(g, case):
    temporal, p, detached, learn = [float(x) for x in g[f'{case}.switches']]
    return dict(temporal_embeds=bool(temporal), token_dropout=p, detached_post=bool(detached), learn_initial=bool(learn))


def meta_of(g, case):
    """-> B, T, A, S, K, seed, noise seed"""
    return tuple(int(x) for x in g[f'{case}.meta'])


def shapes_of(g, case):
    return {str(n): tuple(int(x) for x in d if x >= 0) for n, d in zip(g[f'{case}.shape_names'], g[f'{case}.shape_dims'])}


def overrides(g, case, config, lr_zero=True, **extra):
    """-> (B, T, A, seed, noise seed), the configuration overrides of the case"""
    B, T, A, S, K, seed, nseed = meta_of(g, case)
    sw = switches_of(g, case)
    over = dict(config.tiny_overrides())
    over['connector_rssm'] = dict(over['connector_rssm'], learn_initial=sw['learn_initial'])
    over['connector'] = dict(temporal_embeds=sw['temporal_embeds'], token_dropout=sw['token_dropout'], detached_post=sw['detached_post'])
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    over.update(extra)
    return (B, T, A, seed, nseed), over


def drop_noise(g, case):
    """the Exp(1) tensor of the site 'conn.drop' whose flags are the stored uniforms' (u = exp(-e)), or None without dropout"""
    import torch
    if f'{case}.drop_u' not in g:
        return None
    return torch.from_numpy((-np.log(g[f'{case}.drop_u'].astype(np.float64))).astype(np.float32))
