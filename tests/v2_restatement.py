"""Plain-torch restatement of the arithmetic the DreamerV2 defaults add (conf/defaults/dreamer_v2.yaml of mazpie/genrl), written from the
formulas: a norm-free layer (Linear without bias, then SiLU), the truncated-normal actor head, the squared-error log-likelihood of the
one-wide heads, the unit-variance image likelihood and the un-normalised actor objective.  Any dtype (the tests run it in float32 against
the fixture and in float64 as the yardstick of the kernels)."""
import math

import torch

CLAMP = 1e-6


def dense_silu(x, W, x2=None):
    """SiLU([x, x2] W^T)"""
    if x2 is not None:
        x = torch.cat([x, x2], -1)
    pre = x @ W.t()
    return pre * torch.sigmoid(pre)


def silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def mlp(sd, prefix, x, layers=4):
    """a norm-free MLP trunk and its output layer(s): -> out (, raw std of a normal-family head)"""
    dt = x.dtype
    for i in range(layers):
        x = dense_silu(x, sd[f'{prefix}.dense{i}.weight'].to(dt))
    out = x @ sd[f'{prefix}._out._out.weight'].to(dt).t() + sd[f'{prefix}._out._out.bias'].to(dt)
    if f'{prefix}._out._std.weight' in sd:
        return out, x @ sd[f'{prefix}._out._std.weight'].to(dt).t() + sd[f'{prefix}._out._std.bias'].to(dt)
    return out


def trunc_normal(out, raw_std, eps, min_std=0.1, init_std=0.0):
    """-> action (clamped in value, identity in gradient), mean, std, unclamped x"""
    mean = torch.tanh(out)
    std = 2 * torch.sigmoid((raw_std + init_std) / 2) + min_std
    x = mean + eps * std
    clamped = torch.clamp(x, -1 + CLAMP, 1 - CLAMP)
    return x - x.detach() + clamped.detach(), mean, std, x


def normal_entropy(std):
    return (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).sum(-1)


def mse_log_prob(out, x):
    return -((out - x) ** 2).sum(-1)


def unit_std_log_prob(mean, x):
    """Independent(Normal(mean, 1), 3).log_prob(x) per frame"""
    D = mean.shape[-1] * mean.shape[-2] * mean.shape[-3]
    return -0.5 * ((mean - x) ** 2).sum((-3, -2, -1)) - 0.5 * D * math.log(2 * math.pi)


def lambda_return(reward, value, disc, lam):
    """reward, value (H+1, N, 1): returns of steps 0..H-1, bootstrapped with value[H]"""
    H = reward.shape[0] - 1
    last = value[H]
    outs = []
    for t in range(H - 1, -1, -1):
        last = reward[t] + disc * ((1 - lam) * value[t + 1] + lam * last)
        outs.append(last)
    return torch.stack(outs[::-1], 0)


def actor_loss(target, ent, ent_scale):
    """`reward_ema: False`: the raw lambda-return (+ entropy bonus), unit weights"""
    return -(target[1:] + ent_scale * ent).mean()
