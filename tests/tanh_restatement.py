"""Plain-torch restatement of the squashed-Gaussian actor head (DistLayer 'tanh_normal': SquashedNormal in SampleDist) in whatever dtype its
inputs have: the yardstick of test_tanh_golden.py (float32, against the reference's vectors) and of test_gpu_tanh_kernels.py (float64 as the
truth, float32 as the error a careful implementation makes).  The backward forms are the analytic ones and return, beside each gradient, the
magnitude of the terms it is summed from."""
import math

import torch

K = 100                       # SampleDist's samples
F = torch.nn.functional


def head(raw, min_std, init_std):
    """raw (..., 2A) = [out | std_raw] -> mean = 5 tanh(out / 5), std = softplus(std_raw + init_std) + min_std"""
    A = raw.shape[-1] // 2
    return 5.0 * torch.tanh(raw[..., :A] / 5.0), F.softplus(raw[..., A:] + init_std) + min_std


def sample(raw, eps, min_std, init_std):
    """-> action = tanh(x), x = mean + std eps, mean, std"""
    mean, std = head(raw, min_std, init_std)
    x = mean + std * eps
    return torch.tanh(x), x, mean, std


def ladj(x):
    """log |d tanh(x) / dx| in the form that never overflows"""
    return 2.0 * (math.log(2.0) - x - F.softplus(-2.0 * x))


def log_prob(x, mean, std):
    """the squashed Gaussian's log-density of tanh(x), summed over the action dimensions"""
    return (-(x - mean) ** 2 / (2.0 * std ** 2) - torch.log(std) - 0.5 * math.log(2.0 * math.pi) - ladj(x)).sum(-1)


def mc_mean(raw, eps, min_std, init_std):
    """eps (K, ..., A) -> the mean of the K samples"""
    return sample(raw, eps, min_std, init_std)[0].mean(0)


def entropy(raw, eps, min_std, init_std):
    """eps (K, ..., A) -> -mean_k log_prob(sample_k), (...,)"""
    _, x, mean, std = sample(raw, eps, min_std, init_std)
    return -log_prob(x, mean, std).mean(0)


def tanh_scale(raw, eps, min_std, init_std):
    """the magnitude a float32 tanh(x) is uncertain on: its own, and (1 - tanh^2) times the magnitude of the two terms x = mean + std eps is
    summed from (where they cancel the rounding error follows the terms, not what is left of them)"""
    action, x, mean, std = sample(raw, eps, min_std, init_std)
    return action.abs() + (1.0 - action ** 2) * (mean.abs() + (std * eps).abs())


def entropy_scale(raw, eps, min_std, init_std):
    """the magnitude of the terms an entropy is summed from: per sample and dimension eps^2 / 2, |log std|, log(2 pi) / 2 and the three terms
    of ladj (x counted as the magnitude of ITS two terms), averaged over the samples and summed over the dimensions"""
    _, x, mean, std = sample(raw, eps, min_std, init_std)
    t = (0.5 * eps ** 2 + torch.log(std).abs() + 0.5 * math.log(2.0 * math.pi)
         + 2.0 * (math.log(2.0) + mean.abs() + (std * eps).abs() + F.softplus(-2.0 * x)))
    return t.mean(0).sum(-1)


def _jacobians(raw, init_std):
    """d mean / d out = 1 - tanh^2(out / 5), d std / d std_raw = sigmoid(std_raw + init_std), and the magnitude 1 + tanh^2 of the first one's
    two terms"""
    A = raw.shape[-1] // 2
    th2 = torch.tanh(raw[..., :A] / 5.0) ** 2
    return 1.0 - th2, torch.sigmoid(raw[..., A:] + init_std), 1.0 + th2


def sample_bwd(g, raw, eps, min_std, init_std):
    """d raw of sum(g * action), and the magnitude each element is uncertain on: 1 - action^2 carries 2 |action| times tanh's"""
    action = sample(raw, eps, min_std, init_std)[0]
    jm, js, sjm = _jacobians(raw, init_std)
    dx = g * (1.0 - action ** 2)
    sx = g.abs() * ((1.0 - action ** 2) + 2.0 * action.abs() * tanh_scale(raw, eps, min_std, init_std))
    return torch.cat([dx * jm, dx * eps * js], -1), torch.cat([sx * sjm, sx * eps.abs() * js], -1)


def entropy_bwd(g, raw, eps, min_std, init_std):
    """d raw of sum(g * entropy) (g (...,)), and the magnitude of the terms each element is summed from"""
    action, x, mean, std = sample(raw, eps, min_std, init_std)
    ts = tanh_scale(raw, eps, min_std, init_std)
    dmean, dstd = (-2.0 * action).mean(0), 1.0 / std + (-2.0 * action * eps).mean(0)
    smean, sstd = (2.0 * ts).mean(0), 1.0 / std + (2.0 * ts * eps.abs()).mean(0)
    jm, js, sjm = _jacobians(raw, init_std)
    gg = g[..., None]
    return torch.cat([gg * dmean * jm, gg * dstd * js], -1), torch.cat([gg.abs() * smean * sjm, gg.abs() * sstd * js], -1)


def actor_loss(target, ent, ent_scale, offset_scale=None):
    """agent/dreamer.py:392-429 with actor_grad 'dynamics' and unit weights: target (H, N), ent (H-1, N); offset_scale: the return EMA's
    (offset, scale) or None -> loss, normed target"""
    normed = target if offset_scale is None else (target - offset_scale[0]) / offset_scale[1]
    return -(normed[1:] + ent_scale * ent).mean(), normed
