"""Plain-torch restatement of the vector-observation arithmetic: the symlog gather of the encoder's MLP inputs, the Linear + LayerNorm + SiLU
stack of the encoder's and the decoder's `_mlp_model`, the two vector log-probabilities (MSEDist on a D-wide head; SymlogDist 'mse' / 'sum'
with its `tol`) with their gradients written out, and the decoder's vector branch.  Written from the formulas, for any floating dtype:
test_vecobs_golden.py checks it against the reference's vectors, and test_gpu_vecobs_kernels.py uses it in float64 as the reference and in
float32 as the yardstick of the kernels' error."""
import torch

KINDS = {'mse': 0, 'symlog_mse': 1}


def symlog(x):
    """sign(x) log(|x| + 1); |x| + 1 is rounded in x's dtype before the logarithm (no log1p)"""
    return torch.sign(x) * torch.log(torch.abs(x) + 1)


def symexp(x):
    return torch.sign(x) * (torch.exp(torch.abs(x)) - 1)


def gather(xs, use_symlog):
    """the first MLP layer's input: the keys side by side, symlog'ed or as they are"""
    x = torch.cat(list(xs), -1)
    return symlog(x) if use_symlog else x


def mlp(x, layers):
    """layers: (W, b, gamma, beta, eps) per layer -> SiLU(LayerNorm(x W^T + b)) layer by layer"""
    for W, b, gamma, beta, eps in layers:
        x = torch.nn.functional.silu(torch.nn.functional.layer_norm(x @ W.t() + b, (W.shape[0],), gamma, beta, eps))
    return x


def layers_of(sd, prefix, n, dtype=torch.float32, eps=1e-5):
    """the n layers of the `_mlp_model` at `prefix` in a state_dict (entries 3 i: Linear, 3 i + 1: NormLayer)"""
    t = lambda k: sd[prefix + k].to(dtype)
    return [(t(f'{3 * i}.weight'), t(f'{3 * i}.bias'), t(f'{3 * i + 1}._layer.weight'), t(f'{3 * i + 1}._layer.bias'), eps) for i in range(n)]


def target_of(x, kind):
    """what the head regresses (t) and the magnitude T of the scales: kind 0 t = x, T = |x|; kind 1 t = symlog(x), T = max(|t|, 1) -- the
    rounding of |x| + 1 is an absolute 2^-24 in the logarithm"""
    if kind == 0:
        return x, x.abs()
    t = symlog(x)
    return t, t.abs().clamp_min(1.0)


def like(mode, x, kind, tol=1e-8):
    """-> log_prob (mode.shape[:-1]) and the sum of the magnitudes its terms are made of, sum_d (|mode| + T)^2"""
    t, T = target_of(x, kind)
    d = (mode - t) ** 2
    if kind == 1:
        d = torch.where(d < tol, torch.zeros_like(d), d)
    return -d.sum(-1), ((mode.abs() + T) ** 2).sum(-1)


def like_bwd(mode, x, g, kind, tol=1e-8):
    """-> d like / d mode scaled by g (mode.shape[:-1]), and the magnitude 2 (|mode| + T) |g| of its terms; kind 1: exactly 0 where the
    squared difference is below tol (what torch.where gives the reference)"""
    t, T = target_of(x, kind)
    diff = mode - t
    dm = -2 * diff * g[..., None]
    if kind == 1:
        dm = torch.where(diff ** 2 < tol, torch.zeros_like(dm), dm)
    return dm, 2 * (mode.abs() + T) * g.abs()[..., None]


def decoder_vec(feat, layers, heads):
    """the decoder's vector branch: the trunk once, then one Linear per key; heads: {key: (W, b)} -> {key: raw output}"""
    x = mlp(feat, layers)
    return {key: x @ W.t() + b for key, (W, b) in heads.items()}
