"""MI355X-native building blocks behind the reference's `agent/dreamer_utils.py` API.

Class names, constructor signatures, sub-module and parameter names follow the reference
(mazpie/genrl agent/dreamer_utils.py; weight contract in SURVEY.md §8a) so that `state_dict()`s and
pickled agents are interchangeable; every forward/backward runs in the hand-written HIP kernels
of libgenrl_hip.so (genrl_amd/ops.py).  nn.Module containers (nn.Linear, nn.Conv2d, nn.LayerNorm)
are used only as *parameter holders*: their torch forward is never called on the hot path.

What the GenRL path and the dreamer_v3 / dreamer_v2 defaults configure is implemented (norm 'layer'/'none', act SiLU / ELU, discrete or
continuous latents, GRU cell, dists mse / twohot / normal / trunc_normal / tanh_normal / onehot / symlog_mse / binary, image_dist mse / normal_unit_std, vector
observation keys beside or instead of one image key); other reference options raise.
"""
import contextlib
import re

import numpy as np
import torch
import torch.nn as nn

import os
from .. import noise, ops, ops_conv_planes, ops_planes, streams
from .. import planes as pl          # (module; `planes=` below are operand handles)


class Module(nn.Module):
    """nn.Module whose load_state_dict also drops the cached weight planes (genrl_amd/planes.py)"""
    def load_state_dict(self, *args, **kwargs):
        pl.invalidate()
        return super().load_state_dict(*args, **kwargs)


def symlog(x):  # ref :13-14
    return torch.sign(x) * torch.log(torch.abs(x) + 1.0)


def symexp(x):  # ref :16-17
    return torch.sign(x) * (torch.exp(torch.abs(x)) - 1.0)


# ----------------------------------------------------------------------------- distributions

class MSEDist:
    """ref :62-83.  `log_prob` accepts the raw uint8 frames (preprocess fused into the kernel)."""
    def __init__(self, mode, agg='sum'):
        assert agg == 'sum'
        self._mode = mode

    @property
    def mean(self):
        return self._mode

    def mode(self):
        return self._mode

    def log_prob(self, value):
        assert self._mode.shape == value.shape, (self._mode.shape, value.shape)
        if value.dtype != torch.uint8:           # already-preprocessed floats: undo (x+0.5)*255 exactly
            value = torch.round((value + 0.5) * 255.0).to(torch.uint8)
        lead = self._mode.shape[:-3]
        like = ops.mse_like(self._mode.reshape((-1,) + tuple(self._mode.shape[-3:])),
                            value.reshape((-1,) + tuple(value.shape[-3:])))
        return like.reshape(lead)


class NormalUnitStdDist(MSEDist):
    """Independent(Normal(mode, 1.0), 3) of the decoder with `image_dist: normal_unit_std` (ref :704): per frame
    log_prob = -1/2 sum (mode - x)^2 - 1/2 D log 2 pi = MSEDist's log_prob (the same kernel) halved, minus a constant."""
    def log_prob(self, value):
        D = int(np.prod(self._mode.shape[-3:]))
        return super().log_prob(value) * 0.5 - 0.5 * D * float(np.log(2.0 * np.pi))


class MSEHeadDist:
    """MSEDist on an MLP head (ref :62-83 through DistLayer 'mse', :808-809; the one-wide reward / critic heads of
    conf/defaults/dreamer_v2.yaml): log_prob(x) = -(out - x)^2 summed over the event dimension, mean = out."""
    def __init__(self, mode):
        self._mode = mode

    @property
    def mean(self):
        return self._mode

    def mode(self):
        return self._mode

    def log_prob(self, value):
        assert self._mode.shape == value.shape, (self._mode.shape, value.shape)
        if self._mode.shape[-1] == 1:
            return ops.sqerr_like(self._mode, value)
        return ops.vec_like(self._mode, value.float(), ops.VEC_LIKE_KINDS['mse'])       # (a decoder's vector key)


class BinaryDist:
    """DistLayer 'binary' (ref :820-823) on a one-wide head: Independent(BernoulliDist(sigmoid(x)), 1), whose first positional parameter is
    `logits` (ref :199-201) -- so the distribution is Bernoulli(logits = z) with z = sigmoid(x).  Restated as the reference computes it:
    log_prob(t) = t z - softplus(z), mean = sigmoid(z) in (0.5, 0.731), so the mode is 1."""
    def __init__(self, raw):
        assert raw.shape[-1] == 1, raw.shape
        self._raw = raw

    @property
    def mean(self):
        return torch.sigmoid(torch.sigmoid(self._raw))

    def mode(self):
        p = self.mean             # (torch's Bernoulli.mode: probs >= 0.5, NaN at the tie, which a z below 2^-24 rounds the mean to)
        return torch.where(p == 0.5, torch.full_like(p, float('nan')), (p >= 0.5).to(p.dtype))

    def log_prob(self, value):
        assert self._raw.numel() == value.numel(), (self._raw.shape, value.shape)
        return ops.binary_like(self._raw, value.float())


class SymlogDist:
    """ref :85-118 with dist 'mse', agg 'sum' over one event dimension (DistLayer 'symlog_mse', :839-840): the head regresses symlog(x);
    squared differences below `tol` count as 0, in value and in gradient.  mean() / mode() are methods, as the reference has them."""
    def __init__(self, mode, dims=1, dist='mse', agg='sum', tol=1e-8):
        assert dims == 1 and dist == 'mse' and agg == 'sum', (dims, dist, agg)
        self._mode, self._tol = mode, tol
        self.batch_shape, self.event_shape = mode.shape[:-1], mode.shape[-1:]

    def mode(self):
        return symexp(self._mode)

    def mean(self):
        return symexp(self._mode)

    def log_prob(self, value):
        assert self._mode.shape == value.shape, (self._mode.shape, value.shape)
        return ops.vec_like(self._mode, value.float(), ops.VEC_LIKE_KINDS['symlog_mse'], self._tol)


class TwoHotDist:
    """ref :120-171 (255 symlog buckets in [-20, 20])."""
    def __init__(self, logits, low=-20.0, high=20.0):
        assert logits.shape[-1] == 255
        assert low == -20.0 and high == 20.0
        self.logits = logits

    @property
    def mean(self):
        return ops.twohot_mean(self.logits)

    @property
    def mode(self):
        return self.mean

    def log_prob(self, x):
        return ops.twohot_logprob(self.logits, x)


class OneHotDist:
    """ref :177-197 wrapped in Independent(.,1) (ref :413-415): unimix categorical latents.  independent=False: the bare OneHotDist of
    DistLayer 'onehot' (ref :835-836), the policy of a discrete-action actor -- one categorical per row, with log_prob; `site` names the
    noise site its draws come from."""
    def __init__(self, logits, site='onehot', independent=True):
        self.logits_raw = logits
        self.site = site
        self.independent = independent

    def sample(self, sample_shape=()):
        lg = self.logits_raw
        K = lg.shape[-1]
        q = noise.draw('exp', self.site, (lg.numel() // K, K), lg.device)
        return ops.onehot_sample(lg, q)

    def mode(self):
        return ops.onehot_mode(self.logits_raw)

    @property
    def probs(self):
        """Class probabilities after the 1 % uniform mix (what OneHotCategorical(probs=...) holds, ref :179-183)."""
        K = self.logits_raw.shape[-1]
        return ops.UNIMIX * torch.softmax(self.logits_raw.float(), -1) + (1.0 - ops.UNIMIX) / K

    @property
    def mean(self):          # OneHotCategorical.mean; train.py:297 stores it as the start 'logit' of data-free rollouts
        if not self.independent:        # (the action DreamerAgent.act returns in eval mode, agent/dreamer.py:54-59)
            return ops.onehot_probs(self.logits_raw)
        return self.probs

    def log_prob(self, action):
        assert not self.independent, 'log_prob is implemented for the policy head only'
        return ops.onehot_logp_ent(self.logits_raw, action)[0]

    def entropy(self):
        if not self.independent:
            return ops.onehot_logp_ent(self.logits_raw, None)[1]
        return ops.cat_entropy(self.logits_raw)


def kl_divergence(p, q):
    return ops.cat_kl(p.logits_raw, q.logits_raw)


class LatentNormalDist:
    """Independent(Normal(mean, std), 1) of EnsembleRSSM.get_dist with `discrete: False` (ref :416-419), in the mould of OneHotDist: `sample`
    is the reparameterised one (the reference binds it to rsample) and draws its noise at `site`.  (The training path does not come through
    here: its samples are made from the head's raw output by ops.gauss_head, in the kernel that computes mean and std.)"""
    def __init__(self, mean, std, site='normal'):
        self._mean, self.std, self.site = mean, std, site

    def sample(self, sample_shape=()):
        eps = noise.draw('normal', self.site, tuple(self._mean.shape), self._mean.device)
        return torch.addcmul(self._mean, self.std, eps)

    rsample = sample

    @property
    def mean(self):
        return self._mean

    def mode(self):
        return self._mean

    def entropy(self):
        return ops.gauss_entropy(self.std)


class NormalDist:
    """Independent(Normal(tanh(out), std), 1) of DistLayer 'normal' (ref :814-819) or, by its head (HEADS below), 'trunc_normal':
    Independent(TruncatedNormal(tanh(out), std), 1) (ref :830-834, tools/utils.py:102-123), whose sample is clamped to [-1 + 1e-6, 1 - 1e-6]
    in value with the identity as its gradient and whose mean and entropy are the untruncated Normal's (pyd.Normal's, as the reference's)."""
    def __init__(self, raw, head, site='actor'):
        self.raw, self.head, self.site = raw, head, site

    def sample(self):
        A = self.raw.shape[-1] // 2
        eps = noise.draw('normal', self.site, tuple(self.raw.shape[:-1]) + (A,), self.raw.device)
        return self.head.sample(self.raw, eps)

    rsample = sample

    @property
    def mean(self):
        return self.head.mean(self.raw)

    def entropy(self):
        return (0.5 + 0.5 * np.log(2 * np.pi) + torch.log(self.head.mean_std(self.raw)[1])).sum(-1)


TruncNormalDist = NormalDist


class TanhNormalDist(NormalDist):
    """SampleDist(Independent(SquashedNormal(mean, std), 1)) of DistLayer 'tanh_normal' (ref :824-829, :28-60; tools/utils.py:126-170), from
    the head's raw output: `sample` is the reparameterised tanh(mean + std eps); `mean` and `entropy()` are Monte-Carlo estimates over the
    head's K samples, drawn at sites of their own on every call, as the reference redraws them."""
    @property
    def mean(self):
        return self.head.mean(self.raw, site=f'{self.site}.mean_eps')

    def entropy(self):
        return self.head.entropy_grad(self.raw, site=f'{self.site}.ent_eps')[..., 0]

    def mode(self):          # (the reference's raises too: SquashedNormal has no `expand`, ref :45-47; nothing calls it)
        raise NotImplementedError('mode() of a tanh_normal head')


# ----------------------------------------------------------------------------- policy / output heads

class _Head:
    """What the code around a DistLayer asks about its `dist`: one subclass per kind, listed in HEADS.  A policy head (`noise` set) also
    has sample(raw, noise), mean(raw) and the entropy from raw in the forms its callers use: entropy_grad (differentiable, (..., 1): what the
    actor objective adds), entropy_mean (the metric, from entropy_grad's if given) and the kernels behind the distribution object's."""
    has_std = False          # a second Linear `_std` beside `_out`: raw = [out | std_raw], twice as wide
    planes_linear = False    # the head product may read the operand planes the trunk left (DistLayer.raw)
    fused = False            # the policy tape and the fused rollout have this head built in (WorldModel.imagine)
    reinforce = False        # actor_grad 'reinforce' is implemented on it
    noise = None             # (kind, site) of a rollout's action noise

    def __init__(self, layer):
        self.layer = layer

    def weights(self):          # (weight, bias) of the head as ONE product: `_out` and `_std` stacked
        L = self.layer
        if not self.has_std:
            return L._out.weight, L._out.bias
        return torch.cat([L._out.weight, L._std.weight], 0), torch.cat([L._out.bias, L._std.bias], 0)

    def entropy_mean(self, raw, ent=None):
        if ent is None:         # a metric only: no backward through it
            with torch.no_grad():
                ent = self.entropy_grad(raw)
        return self.reduce(ent.detach())

    reduce = staticmethod(torch.mean)


class _TwoHotHead(_Head):
    planes_linear, dist = True, TwoHotDist


class _MSEHead(_Head):
    def dist(self, raw):
        return MSEHeadDist(raw.reshape(list(raw.shape[:-1]) + list(self.layer._shape)))


class _SymlogMSEHead(_Head):
    def dist(self, raw):
        assert len(self.layer._shape) == 1, 'symlog_mse is built for vector keys'
        return SymlogDist(raw)


class _NormalHead(_Head):
    """'normal': std = (max_std - min_std) sigmoid(raw_std + 2) + min_std, ops.actor_*.  trunc ('trunc_normal'): std = 2 sigmoid((raw_std +
    init_std) / 2) + min_std (ref :832), ops.trunc_normal_*; the entropy is the untruncated Normal's and has no one-launch metric kernel."""
    has_std, noise = True, ('normal', 'imag.act_eps')

    def __init__(self, layer, trunc=False):
        self.layer, self.trunc, self.fused = layer, trunc, not trunc

    def params(self):
        return self.layer._min_std, self.layer._init_std if self.trunc else self.layer._max_std

    def sample(self, raw, eps):
        return (ops.trunc_normal_sample if self.trunc else ops.actor_sample)(raw, eps, *self.params())

    def mean_std(self, raw):         # (kernels, no gradient: NormalDist's mean and entropy)
        return (ops.trunc_normal_mean_std if self.trunc else ops.actor_mean_std)(raw, *self.params())

    def mean(self, raw):
        return self.mean_std(raw)[0]

    def entropy_grad(self, raw):
        (mn, p), raw_std = self.params(), raw[..., raw.shape[-1] // 2:]
        std = 2.0 * torch.sigmoid((raw_std + p) / 2.0) + mn if self.trunc else (p - mn) * torch.sigmoid(raw_std + 2.0) + mn
        return (0.5 + 0.5 * np.log(2 * np.pi) + torch.log(std)).sum(-1)[..., None]

    def entropy_mean(self, raw, ent=None):
        if ent is None and not self.trunc:
            return ops.normal_entropy_mean(raw, *self.params())       # (one launch)
        return super().entropy_mean(raw, ent)

    def dist(self, raw):
        return NormalDist(raw, self)


class _TanhNormalHead(_Head):
    """'tanh_normal': the squashed Gaussian tanh(N(5 tanh(out / 5), softplus(raw_std + init_std) + min_std)) (ref :824-829), ops.tanh_normal_*.
    Its mean and entropy are SampleDist's estimates over K samples (ref :28-60): each call draws its own (K, ..., A) noise, as K times
    the leading dimensions by (rows, A) -- the reference's (K, ..., rows, A) memory, batch rows in dimension 1 (noise._ROWS_DIM1)."""
    has_std, noise = True, ('normal', 'imag.act_eps')
    K = 100                  # SampleDist's `samples` (ref :29)

    def params(self):
        return self.layer._min_std, self.layer._init_std

    def mc_eps(self, raw, site):
        lead, A = tuple(raw.shape[:-1]), raw.shape[-1] // 2
        eps = noise.draw('normal', site, (self.K * int(np.prod(lead[:-1])), lead[-1], A), raw.device)
        return eps.reshape((self.K,) + lead + (A,))

    def sample(self, raw, eps):
        return ops.tanh_normal_sample(raw, eps, *self.params())

    def mean(self, raw, site='imag.act_mean_eps'):          # (random: what act(eval_mode=True) and imagine(eval_policy=True) use)
        return ops.tanh_normal_mc_mean(raw, self.mc_eps(raw, site), *self.params())

    def entropy_grad(self, raw, site='actor.ent_eps'):
        return ops.tanh_normal_entropy(raw, self.mc_eps(raw, site), *self.params())[..., None]

    def dist(self, raw):
        return TanhNormalDist(raw, self)


class _OneHotHead(_Head):
    """`discrete_actions`: the logits of a unimix categorical; its draws are exponential-race noise from a site of their own"""
    planes_linear, reinforce, noise = True, True, ('exp', 'imag.act_q')
    reduce = staticmethod(lambda ent: ops.wmean(ent, None, 1.0))

    def sample(self, raw, q):
        return ops.onehot_sample(raw, q)

    def mean(self, raw):             # the mixed probabilities (OneHotDist.mean, ref :266)
        return ops.onehot_probs(raw)

    def entropy_grad(self, raw):
        return ops.onehot_logp_ent(raw, None)[1][..., None]

    def dist(self, raw):
        return OneHotDist(raw.float(), site='actor', independent=False)


class _BinaryHead(_Head):
    """'binary': the discount head of `pred_discount: True` (BinaryDist), one-wide"""
    def __init__(self, layer):
        if int(np.prod(layer._shape)) != 1:
            raise NotImplementedError(f'a binary head of shape {tuple(layer._shape)}: the discount head is one-wide')
        self.layer = layer

    def dist(self, raw):
        return BinaryDist(raw)


HEADS = {'mse': _MSEHead, 'twohot': _TwoHotHead, 'normal': _NormalHead, 'trunc_normal': lambda layer: _NormalHead(layer, trunc=True),
         'tanh_normal': _TanhNormalHead, 'onehot': _OneHotHead, 'symlog_mse': _SymlogMSEHead, 'binary': _BinaryHead}


# ----------------------------------------------------------------------------- scans (API parity)

def lambda_return(reward, value, pcont, bootstrap, lambda_, axis):
    """ref :228-253 (axis 0, constant pcont).  reward/value (H,N,1); bootstrap (N,1)."""
    assert axis == 0
    disc = float(pcont) if isinstance(pcont, (int, float)) else float(pcont.flatten()[0])
    v = torch.cat([value, bootstrap[None]], 0)
    return ops.lambda_return(reward, v, disc, lambda_)


def static_scan(fn, inputs, start, reverse=False, unpack=False):
    """ref :255-300 (generic python scan; the hot loops do not use it)."""
    last, outs = start, None
    for i in range(inputs[0].shape[0]):
        last = fn(last, *[x[i] for x in inputs]) if unpack else fn(last, tuple(x[i] for x in inputs))
        items = [last] if isinstance(last, dict) else list(last)
        if outs is None:
            outs = [{k: [v] for k, v in it.items()} if isinstance(it, dict) else [it] for it in items]
        else:
            for o, it in zip(outs, items):
                if isinstance(it, dict):
                    for k, v in it.items():
                        o[k].append(v)
                else:
                    o.append(it)
    return [{k: torch.stack(v, 0) for k, v in o.items()} if isinstance(o, dict) else torch.stack(o, 0) for o in outs]


# ----------------------------------------------------------------------------- layers

def get_act(name):
    if name == 'none':
        return nn.Identity()
    if hasattr(nn, name):
        return getattr(nn, name)()
    raise NotImplementedError(name)


_consts = {}


def _const(shape, value, dev, dtype=torch.float32):
    """A constant tensor that is never written (initial RSSM states are replaced, not updated in place; a backward pass's seed): cached,
    so that a training step does not spend a fill launch on it and a replayed graph finds it at the address it captured."""
    key = (tuple(shape), float(value), str(dev), dtype)
    if key not in _consts:
        _consts[key] = torch.full(tuple(shape), float(value), device=dev, dtype=dtype)
    return _consts[key]


def planes_route(rows, switch=None, widths=(), cuda=True):
    """Whether a product over `rows` rows takes the plane-operand kernels (ops_planes): planes enabled, on the GPU, from
    ops_planes.min_rows() rows up, every width in `widths` a multiple of 4, and the environment switch `switch` (read per call) not '0'."""
    return bool(pl.ENABLED and cuda and rows >= ops_planes.min_rows() and all(w % 4 == 0 for w in widths)
                and (switch is None or os.environ.get(switch, '1') != '0'))


class NormLayer(Module):  # ref :844-859
    def __init__(self, name, dim=None):
        super().__init__()
        if name == 'none':
            self._layer = None
        elif name == 'layer':
            assert dim is not None
            self._layer = nn.LayerNorm(dim)
        else:
            raise NotImplementedError(name)

    def forward(self, features):
        if self._layer is None:
            return features
        return ops.ln_act(features, self._layer.weight, self._layer.bias, self._layer.eps, act=False)


class ImgChLayerNorm(nn.Module):  # ref :1031-1040 (parameter holder; applied on NHWC rows)
    def __init__(self, ch, eps=1e-03):
        super().__init__()
        self.norm = torch.nn.LayerNorm(ch, eps=eps)

    def forward(self, x):  # x NCHW, API parity only (hot path works on NHWC)
        y = ops.ln_act(x.permute(0, 2, 3, 1).contiguous(), self.norm.weight, self.norm.bias, self.norm.eps, act=False)
        return y.permute(0, 3, 1, 2)


def _block_act(act):
    """a block's `act:` -> the name its layers run with: 'SiLU' or 'ELU' (ops.ACTS); any other name raises NotImplementedError(name)"""
    ops.act_code(str(act))
    return str(act)


def _dense_ln_silu(x, lin, norm, x2=None, planes=None, act='SiLU'):
    """Linear (+ second concatenated input) + LayerNorm + the block's activation (act: 'SiLU' / 'ELU') with the reference's layer
    objects.  planes: h2 planes of
    the inputs (genrl_amd/planes.py) when the caller has them.  NormLayer('none') (conf/defaults/dreamer_v2.yaml): Linear without
    bias + activation (dense_act), under the same row threshold and switch.  A first input whose width is no multiple of 4 (continuous latents
    with the reference's `stoch: 30`) stays on the fp32-operand kernels, whose scalar-load form takes any width and row spacing."""
    use_planes = planes_route(x.numel() // x.shape[-1], 'GENRL_PLANES_MLP', (lin.weight.shape[0], x.shape[-1]), x.is_cuda)
    if norm._layer is None:
        assert lin.bias is None, 'a norm-free layer has no bias (ref :339-346, :734)'
        if use_planes:
            return ops_planes.dense_act(x, x2, lin.weight, planes=planes, act=act)
        return ops.dense_act(x, x2, lin.weight, act=act)
    if use_planes:          # (-0.75 ms/step at c2 with the BK-64 128x128 tile)
        return ops_planes.dense_ln_act(x, x2, lin.weight, lin.bias, norm._layer.weight, norm._layer.bias, norm._layer.eps,
                                   planes=planes, act=act)
    return ops.dense_ln_act(x, x2, lin.weight, lin.bias, norm._layer.weight, norm._layer.bias, norm._layer.eps, act=act)


class GRUCell(Module):  # ref :750-785
    def __init__(self, inp_size, size, norm=False, act='Tanh', update_bias=-1, device='cuda', **kwargs):
        super().__init__()
        assert norm and act == 'Tanh' and update_bias == -1, 'only the GenRL configuration is implemented'
        self._inp_size, self._size = inp_size, size
        self._update_bias = update_bias
        self.device = device
        self._layer = nn.Linear(inp_size + size, 3 * size, bias=False, **kwargs)
        self._norm = nn.LayerNorm(3 * size)

    def get_initial_state(self, inputs=None, batch_size=None, dtype=None):
        return _const((batch_size, self._size), 0.0, self.device)

    @property
    def state_size(self):
        return self._size

    def forward(self, inputs, deter_state):
        out = ops.gru_step(inputs, deter_state[0], self._layer.weight, self._norm.weight, self._norm.bias)
        return out, [out]


class DistLayer(Module):  # ref :787-841
    def __init__(self, in_dim, shape, dist='mse', min_std=0.1, max_std=1.0, init_std=0.0, bias=True):
        super().__init__()
        self._in_dim = in_dim
        self._shape = shape if type(shape) in [list, tuple] else [shape]
        self._dist, self._min_std, self._init_std, self._max_std = dist, min_std, init_std, max_std
        self._out = nn.Linear(in_dim, int(np.prod(shape)), bias=bias)
        if dist not in HEADS:
            raise NotImplementedError(dist)
        self._head = HEADS[dist](self)
        if self._head.has_std:
            self._std = nn.Linear(in_dim, int(np.prod(shape)))

    def raw(self, inputs):
        h = getattr(inputs, '_planes', None)          # the trunk's last layer left its output's operand planes (ops_planes)
        if h is not None and self._head.planes_linear and planes_route(inputs.numel() // inputs.shape[-1], 'GENRL_PLANES_LINEAR'):
            return ops_planes.linear(inputs, self._out.weight, self._out.bias, h)
        out = ops.linear(inputs, self._out.weight, self._out.bias)
        if self._head.has_std:
            std = ops.linear(inputs, self._std.weight, self._std.bias)
            return torch.cat([out, std], -1)
        return out

    def forward(self, inputs):
        return self._head.dist(self.raw(inputs))


class MLP(Module):  # ref :718-747
    def __init__(self, in_shape, shape, layers, units, act='SiLU', norm='none', **out):
        super().__init__()
        self._act = _block_act(act)
        self._in_shape = in_shape
        if out['dist'] == 'twohot':
            shape = 255
        self._shape = (shape,) if isinstance(shape, int) else shape
        self._layers, self._units, self._norm = layers, units, norm
        last_units = in_shape
        for index in range(self._layers):
            self.add_module(f'dense{index}', nn.Linear(last_units, units, bias=norm != 'none'))
            self.add_module(f'norm{index}', NormLayer(norm, units))
            last_units = units
        self._out = DistLayer(units, shape, **out)

    def trunk(self, features, features2=None, planes=None):
        """features2: optional second input concatenated after `features` (feat = [stoch, deter])
        consumed without materialising the concatenation.  planes: h2 planes of the inputs, if the caller has them."""
        x = features.reshape([-1, features.shape[-1]])
        x2 = features2.reshape([-1, features2.shape[-1]]) if features2 is not None else None
        if (self._layers > 1 and self._norm != 'none'
                and planes_route(x.shape[0], 'GENRL_PLANES_MLP', (self._units, x.shape[-1]), x.is_cuda)):
            # every layer on plane operands: the whole chain as one node, which writes no fp32 copy of a hidden activation that only the
            # next layer's plane product reads (ops_planes._TrunkPlanes) -- layer by layer the same launches as the loop below
            layers = [(getattr(self, f'dense{i}').weight, getattr(self, f'dense{i}').bias, getattr(self, f'norm{i}')._layer.weight,
                       getattr(self, f'norm{i}')._layer.bias, getattr(self, f'norm{i}')._layer.eps) for i in range(self._layers)]
            x = ops_planes.dense_ln_trunk(x, x2, layers, planes=planes, act=self._act)
        else:
            for index in range(self._layers):
                x = _dense_ln_silu(x, getattr(self, f'dense{index}'), getattr(self, f'norm{index}'), x2, planes=planes, act=self._act)
                x2 = planes = None
        out = x.reshape(list(features.shape[:-1]) + [x.shape[-1]])
        h = getattr(x, '_planes', None)        # (reshape returns a new tensor object: carry the operand planes of the rows along)
        if h is not None:
            out._planes = h
        return out

    def forward(self, features, features2=None, planes=None):
        return self._out(self.trunk(features, features2, planes))


# ----------------------------------------------------------------------------- encoder / decoder

def _conv_norm(norm, depth):
    """the norm module of a conv layer (ref :587, :669): ImgChLayerNorm for 'layer', NormLayer('none') for 'none' (no parameters: the layer is
    conv + bias + act); any other name raises NotImplementedError(name), as the reference's NormLayer does"""
    if norm == 'layer':
        return ImgChLayerNorm(depth)
    if norm != 'none':
        raise NotImplementedError(norm)
    return NormLayer('none', depth)


def _conv_ln(norm_mod, act):
    """the keywords a conv layer's node takes for its norm module: the fused channel-LayerNorm, or the activation alone"""
    if isinstance(norm_mod, ImgChLayerNorm):
        return dict(ln=(norm_mod.norm.weight, norm_mod.norm.bias, norm_mod.norm.eps, act))
    return dict(ln=None, act=act)


def _conv_sizes(size, kernels, transposed=False):
    out = []
    for k in kernels:
        size = 2 * (size - 1) + k if transposed else (size - k) // 2 + 1
        out.append(size)
    return out


def _mlp_stack(in_dim, widths, norm, act):
    """the `_mlp_model` of the reference's Encoder / Decoder (ref :590-602, :672-682): Linear, NormLayer, act per width"""
    layers, prev = [], in_dim
    for width in widths:
        layers += [nn.Linear(prev, width, bias=norm != 'none'), NormLayer(norm, width), get_act(act)]
        prev = width
    return nn.Sequential(*layers)


def _run_mlp_stack(model, x, act):
    for i in range(0, len(model), 3):
        x = _dense_ln_silu(x, model[i], model[i + 1], act=act)
    return x


class Encoder(Module):  # ref :558-628
    def __init__(self, shapes, cnn_keys=r'.*', mlp_keys=r'.*', act='SiLU', norm='none',
                 cnn_depth=48, cnn_kernels=(4, 4, 4, 4), mlp_layers=[400, 400, 400, 400], symlog_inputs=False):
        super().__init__()
        self.shapes = shapes
        self.cnn_keys = [k for k, v in shapes.items() if re.match(cnn_keys, k) and len(v) == 3]
        self.mlp_keys = [k for k, v in shapes.items() if re.match(mlp_keys, k) and len(v) == 1]
        self._act = _block_act(act)
        if norm not in ('layer', 'none'):
            raise NotImplementedError(norm)
        self._norm = norm
        assert self.cnn_keys or self.mlp_keys, 'no observation key selected'
        self._cnn_depth, self._cnn_kernels = cnn_depth, cnn_kernels
        self._mlp_layers, self._symlog_inputs = list(mlp_layers), symlog_inputs
        if self.cnn_keys:
            layers = []
            for i, kernel in enumerate(self._cnn_kernels):
                prev_depth = 3 if i == 0 else 2 ** (i - 1) * self._cnn_depth
                depth = 2 ** i * self._cnn_depth
                layers += [nn.Conv2d(prev_depth, depth, kernel, stride=2), _conv_norm(norm, depth), get_act(act)]
            self._conv_model = nn.Sequential(*layers)
        if self.mlp_keys:           # ref :590-602; the first layer reads the keys side by side, in `shapes` order
            assert self._mlp_layers, 'vector keys need at least one MLP layer'
            self._mlp_model = _mlp_stack(sum(shapes[k][0] for k in self.mlp_keys), self._mlp_layers, norm, act)

    def forward(self, data):
        out = None
        if self.cnn_keys:
            key = self.cnn_keys[0]
            x = data[key]
            shape = self.shapes[key]
            batch_dims = x.shape[:-len(shape)]
            x = x.reshape((-1,) + tuple(x.shape)[len(batch_dims):])
            out = self._cnn(x)
            out = out.reshape(tuple(batch_dims) + tuple(out.shape[1:]))
        if not self.mlp_keys:
            return out
        vec = self._mlp(data)
        return vec if out is None else torch.cat([out, vec], -1)        # [cnn | mlp], ref :610-616

    def _mlp(self, data):
        """ref :623-628: the vector keys side by side (symlog'ed with `symlog_inputs`), one launch per key into the first layer's input
        buffer and no concatenation; a single contiguous fp32 key without symlog is read where it lies"""
        xs = [data[k] for k in self.mlp_keys]
        lead = xs[0].shape[:-1]
        xs = [(x if x.dtype == torch.float32 else x.float()).reshape(-1, x.shape[-1]) for x in xs]
        if len(xs) == 1 and not self._symlog_inputs and xs[0].is_contiguous():
            x = xs[0]
        else:
            x = torch.empty(xs[0].shape[0], sum(v.shape[1] for v in xs), device=xs[0].device)
            col = 0
            for v in xs:
                ops.symlog_rows(v, out=x, col=col, symlog=self._symlog_inputs)
                col += v.shape[1]
        x = _run_mlp_stack(self._mlp_model, x, self._act)
        return x.reshape(tuple(lead) + (x.shape[-1],))

    def _cnn(self, x):
        """x: uint8 NCHW frames (x/255-0.5 fused into the first layer's patch gather) or float NCHW."""
        if x.dtype != torch.uint8:
            x = x.permute(0, 2, 3, 1).contiguous()
        conv2d = ops_conv_planes.conv2d_s2 if ops_conv_planes.active(x) else ops.conv2d_s2     # (products on h2 planes where they fit)
        last = len(self._cnn_kernels) - 1
        for i in range(last + 1):
            conv, ln = self._conv_model[3 * i], self._conv_model[3 * i + 1]
            # (an inner layer's fp32 activation has no reader when the next layer gathers from its planes forward AND backward: decided by
            # the next layer's own predicates, ops_conv_planes.consumer_reads_planes_only -- not by position)
            nxt = True if i == last else ('conv', self._cnn_kernels[i + 1])
            x = conv2d(x, conv.weight, conv.bias, fp32_out=nxt, planes_out=i != last, **_conv_ln(ln, self._act))
        n, h, w, c = x.shape
        return ops.transpose_last2(x.reshape(n, h * w, c)).reshape(n, c * h * w)    # NCHW flatten, ref :621


class Decoder(Module):  # ref :631-715
    def __init__(self, shapes, cnn_keys=r'.*', mlp_keys=r'.*', act='SiLU', norm='none',
                 cnn_depth=48, cnn_kernels=(4, 4, 4, 4), mlp_layers=[400, 400, 400, 400], embed_dim=1024,
                 mlp_dist='mse', image_dist='mse'):
        super().__init__()
        self._embed_dim, self._shapes = embed_dim, shapes
        self.cnn_keys = [k for k, v in shapes.items() if re.match(cnn_keys, k) and len(v) == 3]
        self.mlp_keys = [k for k, v in shapes.items() if re.match(mlp_keys, k) and len(v) == 1]
        self._act = _block_act(act)
        if norm not in ('layer', 'none'):
            raise NotImplementedError(norm)
        self._norm = norm
        assert image_dist in ('mse', 'normal_unit_std')
        self._image_dist = image_dist
        assert len(self.cnn_keys) <= 1 and (self.cnn_keys or self.mlp_keys), 'one image key at most, and at least one key'
        self._cnn_depth, self._cnn_kernels = cnn_depth, cnn_kernels
        self.channels = {k: self._shapes[k][0] for k in self.cnn_keys}
        if self.cnn_keys:
            self._conv_in = nn.Sequential(nn.Linear(embed_dim, 32 * self._cnn_depth))
            layers, n = [], len(self._cnn_kernels)
            for i, kernel in enumerate(self._cnn_kernels):
                prev_depth = 32 * self._cnn_depth if i == 0 else 2 ** (n - (i - 1) - 2) * self._cnn_depth
                depth = 2 ** (n - i - 2) * self._cnn_depth
                last = i == n - 1
                if last:
                    depth = sum(self.channels.values())
                layers += [nn.ConvTranspose2d(prev_depth, depth, kernel, stride=2),
                           NormLayer('none', depth) if last else _conv_norm(norm, depth),
                           nn.Identity() if last else get_act(act)]
            self._conv_model = nn.Sequential(*layers)
        if self.mlp_keys:           # ref :672-684: one trunk on the features, one DistLayer per vector key
            assert len(mlp_layers) > 0, 'vector keys need at least one MLP layer'
            self._mlp_model = _mlp_stack(embed_dim, list(mlp_layers), norm, act)
            for key in self.mlp_keys:
                self.add_module(f'dense_{key}', DistLayer(mlp_layers[-1], shapes[key], dist=mlp_dist))

    def forward(self, features):
        if not self.mlp_keys:
            return self._cnn(features)
        outputs = self._cnn(features) if self.cnn_keys else {}
        outputs.update(self._mlp(features))
        return outputs

    def _mlp(self, features):
        """ref :708-715: the trunk runs once and every vector key's head reads it"""
        x = _run_mlp_stack(self._mlp_model, features.reshape(-1, features.shape[-1]), self._act)
        x = x.reshape(tuple(features.shape[:-1]) + (x.shape[-1],))
        return {key: getattr(self, f'dense_{key}')(x) for key in self.mlp_keys}

    def _cnn(self, features):
        lead = features.shape[:-1]
        x = ops.linear(features.reshape(-1, features.shape[-1]), self._conv_in[0].weight, self._conv_in[0].bias)
        x = x.reshape(-1, 1, 1, 32 * self._cnn_depth)             # NHWC with 1x1 pixels
        n = len(self._cnn_kernels)
        convT2d = ops_conv_planes.convT2d_s2 if ops_conv_planes.active(x) else ops.convT2d_s2
        for i in range(n):
            conv = self._conv_model[3 * i]
            if i != n - 1:
                ln = self._conv_model[3 * i + 1]
                # (the 3-channel last layer reads fp32 values, no planes; an inner layer's fp32 output is skipped when the next layer's own
                # predicates say it reads planes only)
                nconv = self._conv_model[3 * (i + 1)]
                nxt = True if i == n - 2 else ('convT', nconv.out_channels, self._cnn_kernels[i + 1])
                x = convT2d(x, conv.weight, conv.bias, fp32_out=nxt, planes_out=i != n - 2, **_conv_ln(ln, self._act))
            else:
                x = ops.convT2d_s2(x, conv.weight, conv.bias, out_nchw=True)     # frames leave in the reference's NCHW
        image_dist = NormalUnitStdDist if self._image_dist == 'normal_unit_std' else MSEDist          # ref :704
        return {key: image_dist(x.reshape(tuple(lead) + tuple(x.shape[1:]))) for key in self.channels}


# ----------------------------------------------------------------------------- RSSM

_tm = lambda x: x.transpose(0, 1).contiguous()          # (B, T, ..) -> (T, B, ..)
_bm = lambda x: x.transpose(0, 1)                       # ... and back, as a view


class _Latent:
    """What EnsembleRSSM asks about its latent kind: _CatLatent or _NormalLatent, chosen once; a new kind is added as a third class.
    fused: the batched observe, the C scans (ops.observe_seq, ops.rssm_imagine_seq) and the fused rollout exist for it.
    scan_draw: a step-by-step scan draws its noise once and a step consumes its slice (False: a draw per step at the step's own site)."""
    def zero_state(self, rows, dev):          # ref :355-359 (read-only constants, built once per shape)
        return dict.fromkeys(self.stats + ('stoch',), _const((rows,) + self.shape, 0.0, dev))


class _CatLatent(_Latent):
    """`discrete: K`: S categorical latents of K classes with a 1 % uniform mix, one-hot samples; a head puts out their S x K logits"""
    noise_kind, noise_suffix, stats, fused, scan_draw = 'exp', 'q', ('logit',), True, False

    def __init__(self, stoch, discrete):
        self.shape = (stoch, discrete)
        self.head_width = self.stoch_size = stoch * discrete

    def flat(self, stoch):
        return stoch.reshape(list(stoch.shape[:-2]) + [self.stoch_size])

    def noise_shape(self, lead):
        return (int(np.prod(lead)) * self.shape[0], self.shape[1])

    def head(self, raw, q, sample):           # a head's raw output -> stoch, stats; sample False: the mode
        logit = raw.reshape(list(raw.shape[:-1]) + list(self.shape))
        return (ops.onehot_sample(logit, q) if sample else ops.onehot_mode(logit)), {'logit': logit}

    def dist(self, state):
        return OneHotDist(state['logit'].float())

    def unif_dist(self, state):
        return OneHotDist(torch.ones_like(state['logit']), site='rssm.unif')

    def kl(self, lhs, rhs, mix, free, mode='balanced'):   # mix max(KL(l || sg r), free).mean() + (1 - mix) max(KL(sg l || r), free).mean() as one node
        return ops.kl_balance(lhs['logit'], rhs['logit'], mix, free, mode)


class _NormalLatent(_Latent):
    """`discrete: False` (ref :333-335): S Normal latents, reparameterised samples; a head puts out [mean | std_raw]"""
    noise_kind, noise_suffix, stats, fused, scan_draw = 'normal', 'eps', ('mean', 'std'), False, True

    def __init__(self, stoch, std_act, min_std):
        self.shape, self.std_act, self.min_std = (stoch,), std_act, min_std
        self.head_width, self.stoch_size = 2 * stoch, stoch

    def flat(self, stoch):
        return stoch

    def noise_shape(self, lead):
        return tuple(lead) + self.shape

    def head(self, raw, eps, sample):
        """_suff_stats_layer + get_dist(stats).sample() (ref :513-521, :416-419).  sample False: stoch = mean -- what the reference's
        prior falls back to (ref :483-486); its posterior calls `dist.mode()` without that guard (ref :456) and raises, see DESIGN 5g."""
        mean, std, stoch = ops.gauss_head(raw, eps if sample else None, self.std_act, self.min_std)
        return stoch, {'mean': mean, 'std': std}

    def dist(self, state):
        return LatentNormalDist(state['mean'].float(), state['std'].float())

    def unif_dist(self, state):               # N(0, 1), ref :427-429
        return LatentNormalDist(torch.zeros_like(state['mean']), torch.ones_like(state['std']), site='rssm.unif')

    def kl(self, lhs, rhs, mix, free, mode='balanced'):   # the same node on Normal latents (torch's kl_normal_normal under Independent(., 1))
        return ops.gauss_kl_balance(lhs['mean'], lhs['std'], rhs['mean'], rhs['std'], mix, free, mode)


class EnsembleRSSM(Module):  # ref :302-555
    def __init__(self, ensemble=5, stoch=30, deter=200, hidden=200, discrete=False, act='SiLU', norm='none',
                 std_act='softplus', min_std=0.1, action_dim=None, embed_dim=1536, device='cuda',
                 single_obs_posterior=False, cell_input='stoch', cell_type='gru'):
        super().__init__()
        assert action_dim is not None
        assert ensemble == 1 and cell_type == 'gru' and cell_input == 'stoch' and norm in ('layer', 'none'), \
            'ensemble 1, GRU, norm layer / none'
        assert discrete or std_act in ops.STD_ACTS, std_act      # (read by continuous latents only, ref :515-519)
        # the activation of _img_in, _ensemble_img_out and _obs_out (ref :339-351).  The batched observe, the C scans and the fused rollout
        # have SiLU built in: an ELU block goes step by step through the per-layer nodes, as the norm-free layers do
        self._act = _block_act(act)
        self.device = device
        self._embed_dim, self._action_dim, self._ensemble = embed_dim, action_dim, ensemble
        self._stoch, self._deter, self._hidden, self._discrete = stoch, deter, hidden, discrete
        self._norm, self._cell_type, self.cell_input = norm, cell_type, cell_input
        self._std_act, self._min_std = std_act, min_std
        self.single_obs_posterior = single_obs_posterior
        self._latent = _CatLatent(stoch, discrete) if self._discrete else _NormalLatent(stoch, std_act, min_std)
        self._cell = GRUCell(self._hidden, self._deter, norm=True, device=self.device)
        self._ensemble_img_dist = nn.ModuleList([nn.Linear(hidden, self._latent.head_width) for _ in range(ensemble)])
        self._obs_dist = nn.Linear(hidden, self._latent.head_width)
        bias = norm != 'none'              # (a norm-free layer has no bias, ref :339-346; the GRU cell keeps its LayerNorm, ref :322)
        self._img_in = nn.Sequential(nn.Linear(self.get_stoch_size() + action_dim, hidden, bias=bias), NormLayer(norm, hidden))
        self._ensemble_img_out = nn.ModuleList(
            [nn.Sequential(nn.Linear(deter, hidden, bias=bias), NormLayer(norm, hidden)) for _ in range(ensemble)])
        in_obs = embed_dim if single_obs_posterior else deter + embed_dim
        self._obs_out = nn.Sequential(nn.Linear(in_obs, hidden, bias=bias), NormLayer(norm, hidden))

    # ---- shapes / helpers
    def initial(self, batch_size):
        return dict(self._latent.zero_state(batch_size, self.device), deter=self._cell.get_initial_state(None, batch_size))

    def get_stoch_size(self):
        return self._latent.stoch_size

    def get_deter_size(self):
        return self._cell.state_size

    def get_feat_size(self):
        return self.get_deter_size() + self.get_stoch_size()

    def get_stoch(self, state):
        return self._latent.flat(state['stoch'])

    def get_deter(self, state):
        return state['deter']

    def get_feat(self, state):
        return torch.cat([self.get_stoch(state), self.get_deter(state)], -1)

    def get_dist(self, state, ensemble=False):
        assert not ensemble
        return self._latent.dist(state)

    def get_unif_dist(self, state):
        return self._latent.unif_dist(state)

    def _scan_noise(self, site, step_site, T, B, dev):
        """The latent noise of a T-step scan over B rows, one draw at `site` + '_q' / '_eps'.  Tests that replay the reference's per-step
        draws inject them under the step site's name (one tensor per obs_step call, `rssm.post` / `rssm.prior`): stacked in call order."""
        lat, inj = self._latent, noise._injected
        site, shape = f'{site}_{lat.noise_suffix}', lat.noise_shape((B,))
        if inj is not None and site not in inj and step_site in inj:
            return torch.stack([noise.draw(lat.noise_kind, step_site, shape, dev) for _ in range(T)], 0)
        return noise.draw(lat.noise_kind, site, (T,) + shape, dev)

    # ---- single steps (API parity; acting / data-free paths)
    def _prior_raw(self, deter):
        x = _dense_ln_silu(deter, self._ensemble_img_out[0][0], self._ensemble_img_out[0][1], act=self._act)
        return ops.linear(x, self._ensemble_img_dist[0].weight, self._ensemble_img_dist[0].bias)

    def _prior_logits(self, deter):
        lg = self._prior_raw(deter)
        return lg.reshape(list(lg.shape[:-1]) + [self._stoch, self._discrete])

    def _post_raw(self, embed, deter=None):
        if self.single_obs_posterior:
            x = _dense_ln_silu(embed, self._obs_out[0], self._obs_out[1], act=self._act)
        else:
            x = _dense_ln_silu(deter, self._obs_out[0], self._obs_out[1], embed, act=self._act)
        return ops.linear(x, self._obs_dist.weight, self._obs_dist.bias)

    def _post_logits(self, embed, deter=None):
        lg = self._post_raw(embed, deter)
        return lg.reshape(list(lg.shape[:-1]) + [self._stoch, self._discrete])

    def _sample_head(self, raw, sample, site, eps=None):     # eps: this step's slice of a scan's noise, else (when sampling) drawn at `site`
        lat = self._latent
        if sample and eps is None:
            eps = noise.draw(lat.noise_kind, site, lat.noise_shape(raw.shape[:-1]), raw.device)
        return lat.head(raw, eps, sample)

    def get_stoch_stats_from_deter_state(self, temp_state, sample=True, site='rssm.prior', eps=None):
        return self._sample_head(self._prior_raw(temp_state['deter']), bool(sample), site, eps)

    def img_step(self, prev_state, prev_action, sample=True, site='rssm.prior', eps=None):
        """dense, GRU step, prior head, sample.  eps: the step's noise where a scan or a rollout drew it for all steps at once"""
        x = _dense_ln_silu(self.get_stoch(prev_state), self._img_in[0], self._img_in[1], prev_action, act=self._act)
        deter = ops.gru_step(x, prev_state['deter'], self._cell._layer.weight, self._cell._norm.weight,
                             self._cell._norm.bias)
        stoch, stats = self.get_stoch_stats_from_deter_state({'deter': deter}, sample, site, eps)
        return {'stoch': stoch, 'deter': deter, **stats}

    def get_post_stoch(self, embed, prior, should_sample=True, eps=None):
        return self._sample_head(self._post_raw(embed, prior['deter']), bool(should_sample), 'rssm.post', eps)

    def obs_step(self, prev_state, prev_action, embed, is_first, should_sample=True, eps=None):
        """eps: (prior, posterior) noise of this step when a scan drew it for all steps at once"""
        m = 1.0 - is_first.float()
        prev_state = {k: torch.einsum('b,b...->b...', m, v) for k, v in prev_state.items()}
        prev_action = torch.einsum('b,b...->b...', m, prev_action)
        e_prior, e_post = eps or (None, None)
        prior = self.img_step(prev_state, prev_action, should_sample, eps=e_prior)
        stoch, stats = self.get_post_stoch(embed, prior, should_sample, e_post)
        return {'stoch': stoch, 'deter': prior['deter'], **stats}, prior

    # ---- sequences
    def observe(self, embed, action, is_first, state=None):
        """ref :362-371.  With single_obs_posterior the posterior, `_img_in`, the x-half of the GRU
        projection and the prior head are batched over all T steps; only h_{t-1} W_h + LN + gates is
        sequential (ops.gru_seq).  Without it, falls back to the step-by-step form."""
        B, T = action.shape[:2]
        if not self._latent.fused or self._act != 'SiLU':          # (the batched form and the scan have SiLU built in)
            return self._observe_stepwise(embed, action, is_first, state)
        if not self.single_obs_posterior:
            # (the scan's C launch loop has the LayerNorm launches of `norm: layer` built in: norm-free layers go step by step)
            if self._norm == 'none' or os.environ.get('GENRL_OBSERVE_SEQ', '1') == '0':
                return self._observe_stepwise(embed, action, is_first, state)
            return self._observe_scan(embed, action, is_first, state)
        S, K = self._stoch, self._discrete
        dev = embed.device
        emb, act, first = _tm(embed), _tm(action), _tm(is_first)
        mask = (1.0 - first.float()).contiguous()                              # (T,B)
        plog = self._post_logits(emb.reshape(T * B, -1)).reshape(T, B, S, K)
        pst = ops.onehot_sample(plog, noise.draw('exp', 'wm.post_q', (T, B * S, K), dev))
        st0 = state if state is not None else self.initial(B)
        q_prior = noise.draw('exp', 'wm.prior_q', (T, B * S, K), dev)
        # Everything below only feeds the KL term (with `decoder_inputs: stoch` the decoder and the
        # reward head need the posterior alone): when `fork_prior` is set it is enqueued on a side
        # stream, so this latency-bound T-step chain runs beside the conv-heavy decoder work; autograd
        # replays each branch's backward on its own stream.  The caller joins before using `prior`.
        ctx = streams.fork('scan') if getattr(self, 'fork_prior', False) else contextlib.nullcontext()
        with ctx:
            prev = torch.cat([st0['stoch'].reshape(1, B, S * K), pst.reshape(T, B, S * K)[:-1]], 0)
            mrow = mask.reshape(T * B, 1)
            x = _dense_ln_silu((prev.reshape(T * B, S * K) * mrow), self._img_in[0], self._img_in[1],
                               act.reshape(T * B, -1) * mrow)
            deter = ops.gru_seq(x.reshape(T, B, -1), mask, st0['deter'], self._cell._layer.weight,
                                self._cell._norm.weight, self._cell._norm.bias)
            qlog = self._prior_logits(deter.reshape(T * B, -1)).reshape(T, B, S, K)
            qst = ops.onehot_sample(qlog, q_prior)
        post = {'stoch': _bm(pst), 'deter': _bm(deter), 'logit': _bm(plog)}
        prior = {'stoch': _bm(qst), 'deter': _bm(deter), 'logit': _bm(qlog)}
        return post, prior

    def _observe_scan(self, embed, action, is_first, state=None):
        """ref :362-371 with the posterior on [deter, embed] (`single_obs_posterior: false`, conf/defaults/dreamer_v3.yaml:5): the
        sampled latent is inside the recurrence.  ONE autograd node (ops.observe_seq): the action half of `_img_in` and the embed half
        of `_obs_out` are batched over T, the remaining chain is eight launches per step each way from C (csrc/seq.hip); the prior head
        does not feed the recurrence and runs on all T * B rows afterwards."""
        B, T = action.shape[:2]
        S, K = self._stoch, self._discrete
        dev = embed.device
        emb, act, first = _tm(embed), _tm(action), _tm(is_first)
        mask = (1.0 - first.float()).contiguous()                              # (T,B)
        st0 = state if state is not None else self.initial(B)
        q_post = self._scan_noise('wm.post', 'rssm.post', T, B, dev)
        q_prior = self._scan_noise('wm.prior', 'rssm.prior', T, B, dev)
        lin_i, ln_i = self._img_in[0], self._img_in[1]._layer
        lin_o, ln_o = self._obs_out[0], self._obs_out[1]._layer
        deter, plog, pst = ops.observe_seq(
            emb, act, mask, st0['stoch'].reshape(B, S * K), st0['deter'], q_post,
            lin_i.weight, lin_i.bias, ln_i.weight, ln_i.bias, self._cell._layer.weight, self._cell._norm.weight, self._cell._norm.bias,
            lin_o.weight, lin_o.bias, ln_o.weight, ln_o.bias, self._obs_dist.weight, self._obs_dist.bias, ln_i.eps, ln_o.eps)
        qlog = self._prior_logits(deter.reshape(T * B, -1)).reshape(T, B, S, K)
        qst = ops.onehot_sample(qlog, q_prior)
        post = {'stoch': _bm(pst.reshape(T, B, S, K)), 'deter': _bm(deter), 'logit': _bm(plog.reshape(T, B, S, K))}
        prior = {'stoch': _bm(qst), 'deter': _bm(deter), 'logit': _bm(qlog)}
        return post, prior

    def _observe_stepwise(self, embed, action, is_first, state=None):
        B, T = action.shape[:2]
        state = state if state is not None else self.initial(B)
        posts, priors = [], []
        e_prior = e_post = [None] * T
        if self._latent.scan_draw:
            e_prior = self._scan_noise('wm.prior', 'rssm.prior', T, B, embed.device)
            e_post = self._scan_noise('wm.post', 'rssm.post', T, B, embed.device)
        for t in range(T):
            post, prior = self.obs_step(state, action[:, t], embed[:, t], is_first[:, t], eps=(e_prior[t], e_post[t]))
            posts.append(post); priors.append(prior); state = post
        st = lambda L: {k: torch.stack([d[k] for d in L], 1) for k in L[0]}
        return st(posts), st(priors)

    def imagine(self, action, state=None, sample=True):
        """ref :373-381: prior rollout for given actions (B,T,A)."""
        B, T = action.shape[:2]
        state = state if state is not None else self.initial(B)
        if (self._latent.fused and not torch.is_grad_enabled() and action.is_cuda and self._norm != 'none' and self._act == 'SiLU'
                and os.environ.get('GENRL_OBSERVE_SEQ', '1') != '0'):
            # forward only (the data-free block's warm-up rollouts, report, video_imagine all run under no_grad): the action half of
            # `_img_in` batched over T, the eight launches per step of the remaining chain from ONE host call (csrc/seq.hip)
            S, K = self._stoch, self._discrete
            lin_i, ln_i = self._img_in[0], self._img_in[1]._layer
            lin_o, ln_o = self._ensemble_img_out[0][0], self._ensemble_img_out[0][1]._layer
            q = self._scan_noise('rssm.imagine', 'rssm.prior', T, B, action.device) if sample else None
            deter, logit, stoch = ops.rssm_imagine_seq(
                action.transpose(0, 1), state['stoch'].reshape(B, S * K), state['deter'], q, S, K,
                lin_i.weight, lin_i.bias, ln_i.weight, ln_i.bias, self._cell._layer.weight, self._cell._norm.weight,
                self._cell._norm.bias, lin_o.weight, lin_o.bias, ln_o.weight, ln_o.bias, self._ensemble_img_dist[0].weight,
                self._ensemble_img_dist[0].bias, ln_i.eps, ln_o.eps)
            return {'stoch': _bm(stoch.reshape(T, B, S, K)), 'deter': _bm(deter), 'logit': _bm(logit.reshape(T, B, S, K))}
        eps = self._scan_noise('rssm.imagine', 'rssm.prior', T, B, action.device) if sample and self._latent.scan_draw else [None] * T
        outs = []
        for t in range(T):
            state = self.img_step(state, action[:, t], sample, eps=eps[t])
            outs.append(state)
        return {k: torch.stack([d[k] for d in outs], 1) for k in outs[0]}

    # ---- losses
    def kl_loss(self, post, prior, forward, balance, free, free_avg):
        """ref :534-555.  The reference tests `balance == 0.5` first, on the Python float, and reads neither mix nor free_avg in that
        branch; the loss of its free_avg branch has shape [1], here it stays 0-d."""
        lhs, rhs = (prior, post) if forward else (post, prior)
        mix = balance if forward else (1 - balance)
        mode = 'unbalanced' if balance == 0.5 else ('free_avg' if free_avg else 'balanced')
        return self._latent.kl(lhs, rhs, mix, free, mode)


# ----------------------------------------------------------------------------- optimiser

class FlatGroup:
    """Parameters of one optimiser group re-homed into one flat fp32 buffer (params and grads are
    views), so clip-norm + decay + Adam is one pass and DP needs one all-reduce per group."""
    ALIGN = 64          # floats: every parameter starts on a 256-byte boundary (the vector-load GEMMs need 16)
    NORM_SLOTS = 8

    def __init__(self, params):
        self.params = [p for p in params]
        dev = self.params[0].device
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.n = n
        self.flat = torch.zeros(n, device=dev)              # (the gaps stay zero: zero gradient, zero Adam moments)
        self.grad = torch.zeros(n, device=dev)
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.step = 0
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)   # device-side Adam step (graph replay)
        for p, off in zip(self.params, self.offsets):
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)
            p.grad = self.grad[off:off + k].view(p.shape)
        # gradient-norm metric slots, used round-robin: the 0-d tensor an optimiser call hands out stays valid for the next
        # NORM_SLOTS - 1 steps of this group (a caller that aggregates metrics over a few steps reads what it was given)
        self.norm = torch.zeros(self.NORM_SLOTS, device=dev)
        self.norm_i = 0

    def norm_slot(self):
        k = self.norm_i
        self.norm_i = (k + 1) % self.NORM_SLOTS
        return self.norm[k:k + 1]

    def owns(self, params):
        return len(params) == len(self.params) and all(a is b for a, b in zip(params, self.params))

    def rebind(self):
        """re-attach .grad views (zero_grad(set_to_none) or external code may have dropped them)"""
        for p, off in zip(self.params, self.offsets):
            g = self.grad[off:off + p.numel()].view(p.shape)
            if p.grad is None:
                p.grad = g
            elif p.grad.data_ptr() != g.data_ptr():
                g.copy_(p.grad); p.grad = g


class Optimizer:
    """ref :871-932: backward -> clip by global norm -> p *= (1-wd) for *every* handed parameter
    -> Adam -> zero_grad, as HIP kernels over flat buffers and without host syncs (metrics are
    0-d device tensors).  `grad_reduce` is the DP hook (one all-reduce per group)."""
    grad_reduce = None      # set by genrl_amd.dp: callable(flat_grad) -> divisor
    grad_reduce_async = None   # set by genrl_amd.dp: callable(flat_grad) -> (wait(), world): the reduction runs beside later work
    overlap_under_dp = False   # set by genrl_amd.dp for RCCL: collectives are stream-ordered, the connector's side stream may stay on
    grad_hook = None        # test hook: callable(opt_name, params) after backward, before the step
    reduce_hook = None      # test hook: callable(opt_name, group, gscale) after the DP reduction, before clip / Adam

    def __init__(self, name, parameters, lr, eps=1e-4, clip=None, wd=None, opt='adam', wd_pattern=r'.*', use_amp=False):
        assert 0 <= wd < 1
        assert not clip or 1 <= clip
        assert opt == 'adam' and wd_pattern == r'.*'
        self._use_amp = use_amp   # precision 16 = bf16 MFMA operands (ops.set_gemm_precision): no GradScaler, nothing to do here
        self._name, self._clip, self._wd, self._lr, self._eps = name, clip, wd, lr, eps
        self._params = list(parameters)
        self._groups = []
        self._live_cache = {}
        self._pending = []
        self._once = True

    def _group_for(self, params):
        for g in self._groups:
            if g.owns(params):
                return g
        # a parameter can only live in one flat buffer: groups must be disjoint
        ids = {id(p) for p in params}
        for g in self._groups:
            assert not ids & {id(p) for p in g.params}, 'overlapping optimiser groups'
        g = FlatGroup(params)
        self._groups.append(g)
        return g

    def __call__(self, loss, params, decay_only=(), defer=False, flush_pending=True):
        """defer=True (data parallel only): the gradient all-reduce is STARTED here and the clip / Adam pass is left
        pending until flush() -- or this optimiser's next call, after that call's backward (flush_pending=False: not by
        that call -- it runs on a side stream and the pending step belongs to the main one): the reduction then runs
        beside whatever the caller enqueues in between (the connector update behind the world-model reduction, the
        critic update behind the actor's).  The returned grad-norm metric is a device scalar in one of the group's
        NORM_SLOTS round-robin slots, written when the step completes (stream order makes that invisible to a reader on
        the same stream): it keeps its value for the next NORM_SLOTS - 1 steps of the group; read (or clone) it before."""
        params = [p for p in params]
        assert len(loss.shape) == 0 or (len(loss.shape) == 1 and loss.shape[0] == 1), (self._name, loss.shape)
        metrics = {}
        if self._once:
            count = sum(p.numel() for p in params if p.requires_grad)
            print(f'Found {count} {self._name} parameters.')
            self._once = False
        metrics[f'{self._name}_loss'] = loss.detach()
        # parameters that get a gradient from this loss form the Adam group; the others handed in
        # only receive weight decay (connector weights during the world-model step).
        key = tuple(id(p) for p in params)
        if key not in self._live_cache:                 # graph topology is static across iterations
            self._live_cache[key] = [p for p in params if p.requires_grad and _in_graph(loss, p)]
        live = self._live_cache[key]
        group = self._group_for(live)
        group.rebind()
        ops.direct_grads = True        # weight-gradient kernels accumulate straight into the flat gradient buffers
        ops.defer_begin()              # ... and the LayerNorm backward passes leave their parameter-gradient partials unreduced
        try:
            loss.backward(gradient=_const(loss.shape, 1.0, loss.device, loss.dtype))       # (a cached seed: torch would fill a fresh ones tensor per call)
        except BaseException:
            ops.direct_grads = False
            ops.defer_abort()          # a failed backward pass: its partial sets (possibly never written) are NOT summed into the gradients
            raise
        ops.direct_grads = False
        ops.defer_flush()              # one launch sums them all (the backward pass's streams have been joined by autograd)
        if Optimizer.grad_hook is not None:
            Optimizer.grad_hook(self._name, live)
        if flush_pending:
            self.flush()               # an earlier deferred step: its reduction had this backward to hide behind
        gscale, wait = 1.0, None
        if Optimizer.grad_reduce is not None:
            if defer and Optimizer.grad_reduce_async is not None:
                wait, world = Optimizer.grad_reduce_async(group.grad)
                gscale = 1.0 / world
            else:
                gscale = 1.0 / Optimizer.grad_reduce(group.grad)
        # weight decay of the handed-in parameters that are not live (disjoint from the Adam group: order-free)
        if self._wd:
            live_ids = {id(p) for p in live}
            for p in params:
                if id(p) not in live_ids:
                    other = self._flat_owner(p)
                    if other is None:
                        ops.scale_(p.data, 1.0 - self._wd) if p.data.is_contiguous() else p.data.mul_(1.0 - self._wd)
            for g in self._decay_groups(params, live_ids):
                ops.scale_(g.flat, 1.0 - self._wd)
            pl.invalidate([p for p in params if id(p) not in live_ids])     # (their cached weight planes are stale)
        slot = group.norm_slot()
        metrics[f'{self._name}_grad_norm'] = slot[0]
        pend = (group, gscale, wait, slot)
        if wait is not None:
            self._pending.append(pend)
        else:
            self._finish(pend)
        return metrics

    def _finish(self, pend):
        group, gscale, wait, slot = pend
        if wait is not None:
            wait()
        if Optimizer.reduce_hook is not None:
            Optimizer.reduce_hook(self._name, group, gscale)
        ops.grad_norm(group.grad, slot, gscale, step_inc=group.step_dev)     # (also: device step count += 1)
        group.step += 1
        pl.invalidate(group.params)         # (these weights change below: their cached weight planes are stale)
        ops.adam_step(group.flat, group.grad, group.m, group.v, slot, gscale, float(self._clip or 0.0),
                      self._lr, self._eps, float(self._wd or 0.0), group.step, step_dev=group.step_dev, zero_grad=True)
        # (the gradient buffer was cleared by the Adam pass)

    def flush(self):
        """complete the deferred steps (no-op otherwise)"""
        while self._pending:
            self._finish(self._pending.pop(0))

    def release(self, params):
        """Stop stepping `params` (GenRLAgent.finetune_mode after a connector trained end to end, `connector.detached_post: False`: its
        weights leave the world model's loss).  A group that holds some of them is rebuilt over its other parameters, which keep their
        Adam moments and step count; the released ones keep their values in storage of their own, without a gradient buffer, and are
        only decayed from then on, like every parameter that is handed in without being live."""
        self.flush()
        ids = {id(p) for p in params}
        for i, g in enumerate(self._groups):
            if not ids & {id(p) for p in g.params}:
                continue
            pl.invalidate(g.params)
            old = {id(p): off for p, off in zip(g.params, g.offsets)}
            for p in g.params:
                if id(p) in ids:
                    p.data, p.grad = p.data.clone(), None
            new = FlatGroup([p for p in g.params if id(p) not in ids])
            for p, off in zip(new.params, new.offsets):
                k, o = p.numel(), old[id(p)]
                new.m[off:off + k].copy_(g.m[o:o + k]); new.v[off:off + k].copy_(g.v[o:o + k])
            new.step = g.step
            new.step_dev.copy_(g.step_dev)
            self._groups[i] = new
        self._live_cache.clear()

    def _flat_owner(self, p):
        for g in self._groups:
            for q in g.params:
                if q is p:
                    return g
        return None

    def _decay_groups(self, params, live_ids):
        """flat groups all of whose parameters were handed in without being live"""
        ids = {id(p) for p in params} - live_ids
        return [g for g in self._groups if g.params and all(id(q) in ids for q in g.params)]


def _in_graph(loss, p):
    """True if parameter p is reachable from loss in the autograd graph."""
    cache = getattr(loss, '_genrl_leafs', None)
    if cache is None:
        cache, seen, stack = set(), set(), [loss.grad_fn]
        while stack:
            fn = stack.pop()
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            if hasattr(fn, 'variable'):
                cache.add(id(fn.variable))
            stack.extend(f for f, _ in fn.next_functions)
        try:
            loss._genrl_leafs = cache
        except Exception:
            pass
    return id(p) in cache


# ----------------------------------------------------------------------------- misc (ref :934-1029)

class StreamNorm:
    def __init__(self, shape=(), momentum=0.99, scale=1.0, eps=1e-8, device='cuda'):
        self.device, self._shape, self._momentum, self._scale, self._eps = device, tuple(shape), momentum, scale, eps
        self.mag = self.mean = self.square_mean = None
        self.step = 0

    def reset(self):
        self.step, self.mag, self.mean, self.square_mean = 0, None, None, None

    def __call__(self, inputs):
        """All seven reductions of the reference (:956-1001) from ONE pass over the inputs (ops.moments):
        [mean, std, mean |x|, mean x^2]."""
        metrics = {}
        scalar = self._shape == () and inputs.is_cuda
        mom = ops.moments(inputs) if scalar else None
        self.update(inputs, mom)
        metrics['mean'] = mom[0] if scalar else inputs.mean()
        metrics['std'] = mom[1] if scalar else inputs.std()
        outputs = self.transform(inputs)
        if self._momentum == 1 and scalar:                 # identity transform: the normed statistics are the same numbers
            metrics['normed_mean'], metrics['normed_std'] = mom[0], mom[1]
        else:
            metrics['normed_mean'] = outputs.mean()
            metrics['normed_std'] = outputs.std()
        return outputs, metrics

    def update(self, inputs, mom=None):
        self.step += 1
        if self._momentum == 1 and self.mag is not None:
            return                                  # ema(old, new) = 1 * old + 0 * new: the statistics never move again
        # in place once the state exists: under hipGraph replay the state tensors keep their capture-time addresses, so the EMA
        # advances across replays (a rebinding `old = m * old + (1 - m) * new` froze `old` at its warm-up value)
        def ema(old, new):
            if old is None:
                return new.detach().clone()
            return old.mul_(self._momentum).add_(new.detach(), alpha=1 - self._momentum)
        if mom is not None:        # scalar statistics from the one-pass kernel: the same EMA (ref :972-984), first call = copy
            self.mag, self.mean, self.square_mean = ema(self.mag, mom[2]), ema(self.mean, mom[0]), ema(self.square_mean, mom[3])
            return
        batch = inputs.detach().reshape((-1,) + self._shape)
        self.mag = ema(self.mag, torch.abs(batch).mean(0))
        self.mean = ema(self.mean, torch.mean(batch))
        self.square_mean = ema(self.square_mean, torch.mean(batch * batch))

    def transform(self, inputs):
        if self._momentum == 1:
            return inputs
        values = inputs.reshape((-1,) + self._shape) / (self.mag[None] + self._eps) * self._scale
        return values.reshape(inputs.shape)


class RequiresGrad:
    def __init__(self, model):
        self._model = model

    def __enter__(self):
        self._model.requires_grad_(requires_grad=True)

    def __exit__(self, *args):
        self._model.requires_grad_(requires_grad=False)


class RewardEMA:
    """ref :1014-1029.  `all_gather` is the DP hook so the quantiles see the global batch."""
    all_gather = None

    def __init__(self, device, alpha=1e-2):
        self.device, self.alpha = device, alpha
        self.range = torch.tensor([0.05, 0.95]).to(device)

    def __call__(self, x, ema_vals):
        """-> (offset, scale); also leaves self.last = tensor [offset, scale, q05, q95] (device)."""
        flat_x = torch.flatten(x.detach())
        if RewardEMA.all_gather is not None:
            flat_x = RewardEMA.all_gather(flat_x)
        if flat_x.is_cuda and ema_vals.is_contiguous():
            # radix-select quantiles + EMA + clip in one kernel (stats.hip) instead of sort + ~10 elementwise launches
            self.last = ops.quantile_ema(flat_x, ema_vals, self.alpha, 0.05, 0.95)
            return self.last[0], self.last[1]
        x_quantile = torch.quantile(input=flat_x, q=self.range)
        ema_vals[:] = self.alpha * x_quantile + (1 - self.alpha) * ema_vals
        scale = torch.clip(ema_vals[1] - ema_vals[0], min=1.0)
        self.last = None
        return ema_vals[0].detach(), scale.detach()
