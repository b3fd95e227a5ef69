"""The cases of tests/golden/klmodes_tiny.npz as the CPU and the GPU tests read them: the settings of each case come from the arrays the
generator stored (kl_cfg, conn_kl_cfg, clip_rewards, meta), never from a second table."""
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('avg_hi', 'avg_lo', 'avg_g', 'unb_fwd', 'unb_g', 'genrl')
GAUSS = dict(stoch=8, std_act='sigmoid2')
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'klmodes_tiny.npz')))
    return _cache['g']


def kl_of(g, case, name='kl_cfg'):
    balance, free, forward, free_avg = [float(x) for x in g[f'{case}.{name}']]
    return dict(balance=balance, free=free, forward=bool(forward), free_avg=bool(free_avg))


def shapes_of(g, case):
    pre = f'{case}.shape.'
    return {k[len(pre):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith(pre)}


def stats_of(g, case, side, pre=''):
    """the stored statistics of one side ('post' / 'prior'; pre 'conn_': of the connector's KL) as a dict of arrays"""
    keys = ('mean', 'std') if f'{case}.{pre}{side}_mean' in g else ('logit',)
    return {k: g[f'{case}.{pre}{side}_{k}'] for k in keys}


def overrides(g, case, config, lr_zero=True, **extra):
    """-> agent kind ('dreamer' | 'genrl'), (B, T, A, seed), the configuration overrides of the case"""
    B, T, A, S, K, seed = [int(x) for x in g[f'{case}.meta']]
    kind = 'genrl' if f'{case}.conn_kl_cfg' in g else 'dreamer'
    over = dict(config.tiny_overrides() if kind == 'genrl' else config.dreamer_tiny_overrides())
    if K == 0:
        over['rssm'] = dict(over['rssm'], discrete=False, **GAUSS)
        assert S == GAUSS['stoch']
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    over.update(kl=kl_of(g, case), clip_rewards=str(g[f'{case}.clip_rewards']))
    if kind == 'genrl':
        over['connector_kl'] = kl_of(g, case, 'conn_kl_cfg')
    over.update(extra)
    return kind, (B, T, A, seed), over
