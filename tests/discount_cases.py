"""The cases of tests/golden/discount_tiny.npz (`pred_discount: True`) as the generator, the CPU and the GPU tests read them: one table of
settings, the terminal flags of the batch, and the loaders of what the generator stored."""
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
B, T, A = 2, 18, 6
# case: (defaults, overrides on top of the tiny widths and `pred_discount: True`)
CASES = {
    'v3': ('dreamer_v3', dict(grad_heads=['decoder', 'reward', 'discount'])),                    # reward_ema, the head trained end to end
    'v3_ent0': ('dreamer_v3', dict(actor_ent=0)),                                               # the one-launch actor objective, weighted
    'v2': ('dreamer_v2', dict()),                                                               # no EMA, entropy bonus
    'disc_reinforce': ('dreamer_v3', dict(discrete_actions=True, actor_grad='reinforce')),       # one-hot head, REINFORCE
}
# (window, step) of the terminal flags: inside windows and at both windows' last step -- 6 of the 36 start states
TERMINALS = ((0, 5), (0, 11), (0, T - 1), (1, 2), (1, 8), (1, T - 1))
_cache = {}


def load():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(os.path.join(G, 'discount_tiny.npz')))
    return _cache['g']


def is_terminal(flags=TERMINALS):
    """(B, T) bool"""
    t = np.zeros((B, T), bool)
    for b, s in flags:
        t[b, s] = True
    return t


def check_terminals(t):
    """what the fixture asks of the flags: between 4 and half of the start states, one inside a window, one at a window's last step"""
    n = int(t.sum())
    assert 4 <= n <= t.size // 2, n
    assert bool(t[:, 1:-1].any()) and bool(t[:, -1].any())


def tiny(base):
    """tiny overrides with the discount head's width: `dreamer_tiny_overrides()` of genrl_amd.config has it, the copy in detgen.py gets it
    here"""
    over = dict(base)
    over.setdefault('discount_head', dict(units=32))
    return over


def overrides(case, base, lr_zero=True, **extra):
    """-> defaults, the configuration overrides of the case on top of `base` (a dict of tiny overrides)"""
    defaults, more = CASES[case]
    over = dict(tiny(base), pred_discount=True, **more)
    if lr_zero:
        over.update(model_opt=dict(lr=0.0, wd=0.0), actor_opt=dict(lr=0.0, wd=0.0), critic_opt=dict(lr=0.0, wd=0.0))
    over.update(extra)
    return defaults, over


def shapes_of(g, case):
    pre = f'{case}.shape.'
    return {k[len(pre):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith(pre)}


def batch_of(g, case, detgen, flags=None):
    """the numpy batch of a case: detgen.det_batch with the fixture's terminal flags (flags: another (B, T) bool array) and, in the
    discrete-action case, its one-hot replayed actions"""
    batch = detgen.det_batch(B, T, A=A, seed=int(g[f'{case}.meta'][6]))
    batch['is_terminal'] = g[f'{case}.is_terminal'].astype(bool) if flags is None else flags
    if f'{case}.batch_action_idx' in g:
        batch['action'] = np.eye(A, dtype=np.float32)[g[f'{case}.batch_action_idx'].astype(np.int64)]
    batch.pop('clip_video')
    return batch
