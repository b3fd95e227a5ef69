"""Plain-torch restatement of EnsembleRSSM.kl_loss in its three modes -- balanced, unbalanced (`balance: 0.5`) and averaged free nats
(`free_avg: True`) -- for categorical and Gaussian latents, and of `clip_rewards`.  Written from the formulas, for any floating dtype:
test_klmodes_golden.py checks it against the reference's vectors (tests/golden/klmodes_tiny.npz); the GPU tests use it in float64 as the
reference (autograd supplies its gradients) and in float32 as the yardstick of the kernels' error.

The reduction on its own -- per-row KL -> loss and mean (loss_from_rows), scalar gradient -> the per-row upstream gradients of the two KL
sides (loss_bwd) -- is what the kernel pair genrl_kl_loss_{fwd,bwd} computes; it is written out here with torch.maximum's tie rule (half the
gradient where the two arguments are equal)."""
import torch

import gauss_restatement as GR
from discrete_restatement import probs

MODES = {'balanced': 0, 'unbalanced': 1, 'free_avg': 2}


def mode_of(balance, free_avg):
    """the branch the reference takes: `balance == 0.5` is tested first, on the Python float; free_avg is not read there"""
    return 'unbalanced' if balance == 0.5 else ('free_avg' if free_avg else 'balanced')


def cat_kl(lp, lq):
    """KL(Independent(OneHotDist(lp), 1) || Independent(OneHotDist(lq), 1)): logits (..., S, K) with the 1 % uniform mix -> (...)"""
    p, q = probs(lp), probs(lq)
    return (p * (torch.log(p) - torch.log(q))).sum(-1).sum(-1)


def row_kl(lhs, rhs):
    """per-row KL(lhs || rhs) of two dicts of statistics: 'logit', or 'mean' and 'std'"""
    if 'logit' in lhs:
        return cat_kl(lhs['logit'], rhs['logit'])
    return GR.kl(lhs['mean'], lhs['std'], rhs['mean'], rhs['std'])[0]


def kl_loss(post, prior, forward, balance, free, free_avg):
    """-> 0-d loss, per-row value KL(lhs || rhs); differentiable into both dicts the way the reference's is"""
    sg = lambda d: {k: v.detach() for k, v in d.items()}
    lhs, rhs = (prior, post) if forward else (post, prior)
    mix = balance if forward else 1 - balance
    mode = mode_of(balance, free_avg)
    clamp = lambda v: torch.maximum(v, v.new_tensor(free))          # (torch.maximum: half the gradient at a tie; torch.clamp gives all of it)
    if mode == 'unbalanced':
        value = row_kl(lhs, rhs)
        return clamp(value).mean(), value.detach()
    vl, vr = row_kl(lhs, sg(rhs)), row_kl(sg(lhs), rhs)
    if mode == 'free_avg':
        return mix * clamp(vl.mean()) + (1 - mix) * clamp(vr.mean()), vl.detach()
    return mix * clamp(vl).mean() + (1 - mix) * clamp(vr).mean(), vl.detach()


def loss_from_rows(kl, mode, mix, free):
    """per-row KL (R,) -> loss, mean(kl)"""
    mean = kl.mean()
    if mode == 'free_avg':
        c = torch.clamp(mean, min=free)
        return mix * c + (1 - mix) * c, mean
    m = torch.clamp(kl, min=free).mean()
    return (m if mode == 'unbalanced' else mix * m + (1 - mix) * m), mean


def loss_bwd(kl, gloss, mode, mix, free):
    """-> gp, gq (R,): the gradient of gloss * loss with respect to the left side's and the right side's per-row KL"""
    gm = gloss / kl.numel()
    v = kl.mean().expand_as(kl) if mode == 'free_avg' else kl
    g = torch.where(v > free, gm, torch.where(v == free, 0.5 * gm, torch.zeros_like(gm))) * torch.ones_like(kl)
    if mode == 'unbalanced':
        return g, g.clone()
    return mix * g, (1 - mix) * g


def clip_reward(reward, name):
    if name == 'identity':
        return reward
    return {'sign': torch.sign, 'tanh': torch.tanh}[name](reward)
