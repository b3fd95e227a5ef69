"""Plain-torch restatement of the continuous-latent arithmetic (`rssm.discrete: False`): the sufficient-statistics head with its
reparameterised sample, the Normal-Normal KL under Independent(., 1), the entropies and the balanced free-nats loss, each with its gradient
written out.  Written from the formulas, for any floating dtype: test_gauss_golden.py checks it against the reference's vectors, and
test_gpu_gauss_kernels.py uses it in float64 as the reference and in float32 as the yardstick of the kernels' error."""
import math

import torch

STD_ACTS = ('softplus', 'sigmoid', 'sigmoid2')


def act(x, std_act):
    """the std activation before `+ min_std`; softplus is torch's (threshold 20)"""
    if std_act == 'softplus':
        return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20))))
    if std_act == 'sigmoid':
        return torch.sigmoid(x)
    assert std_act == 'sigmoid2', std_act
    return 2 * torch.sigmoid(x / 2)


def dact(x, std_act):
    if std_act == 'softplus':
        return torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))
    # sigmoid'(y) = e / (1 + e)^2 with e = exp(-|y|): s (1 - s) loses the tail to the rounding of s towards 1, in float64 too from |y| = 37
    e = torch.exp(-(x if std_act == 'sigmoid' else x / 2).abs())
    return e / (1 + e) ** 2


def head(raw, eps, std_act, min_std):
    """raw (..., 2S) = [mean | std_raw] -> mean, std, stoch = mean + std eps (eps None: stoch = mean)"""
    S = raw.shape[-1] // 2
    mean, std = raw[..., :S], act(raw[..., S:], std_act) + min_std
    return mean, std, (mean + std * eps if eps is not None else mean)


def head_bwd(dstoch, dmean, dstd, raw, eps, std_act):
    """-> d raw (..., 2S) and the magnitude of the terms each element is summed from; an absent gradient is zero"""
    S = raw.shape[-1] // 2
    z = torch.zeros_like(raw[..., :S])
    gs, gm, gd = (z if t is None else t for t in (dstoch, dmean, dstd))
    e = z if eps is None else eps
    d = dact(raw[..., S:], std_act)
    draw = torch.cat([gs + gm, (gs * e + gd) * d], -1)
    scale = torch.cat([gs.abs() + gm.abs(), ((gs * e).abs() + gd.abs()) * d], -1)
    return draw, scale


def kl(ml, sl, mr, sr):
    """KL(N(ml, sl) || N(mr, sr)) summed over the last dimension (torch's kl_normal_normal under Independent(., 1)) and the sum of
    the magnitudes of its four terms"""
    v = (sl / sr) ** 2
    t = ((ml - mr) / sr) ** 2
    return (0.5 * (v + t - 1 - torch.log(v))).sum(-1), (0.5 * (v + t + 1 + torch.log(v).abs())).sum(-1)


def kl_bwd(ml, sl, mr, sr, gp, gq):
    """-> (d mean_l, d std_l, d mean_r, d std_r) with gp / gq the per-row upstream gradients of the left / right side, and the magnitudes
    of the terms each is summed from"""
    gp, gq = gp[..., None], gq[..., None]
    d = ml - mr
    grads = (gp * d / sr ** 2, gp * (sl / sr ** 2 - 1 / sl), -gq * d / sr ** 2, gq * (1 / sr - (sl ** 2 + d ** 2) / sr ** 3))
    scales = ((gp * d / sr ** 2).abs(), gp.abs() * (sl / sr ** 2 + 1 / sl), (gq * d / sr ** 2).abs(),
              gq.abs() * (1 / sr + (sl ** 2 + d ** 2) / sr ** 3))
    return grads, scales


def entropy(std):
    return (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).sum(-1)


def kl_balance(post, prior, forward, balance, free):
    """EnsembleRSSM.kl_loss (balance != 0.5, free_avg False) on dicts of mean / std -> loss, per-row value.  Both KLs have the same value:
    they differ in which side is detached"""
    lhs, rhs = (prior, post) if forward else (post, prior)
    mix = balance if forward else 1 - balance
    value, _ = kl(lhs['mean'], lhs['std'], rhs['mean'], rhs['std'])
    clamped = torch.clamp(value, min=free).mean()
    return mix * clamped + (1 - mix) * clamped, value
