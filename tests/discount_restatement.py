"""Plain-torch restatement of the learned discount of `pred_discount: True` in the dtype of its inputs: float64 is the reference of
the kernel and op tests, float32 the yardstick their bounds come from.  It restates what the reference computes, not what it should have been:
DistLayer 'binary' hands sigmoid(x) to BernoulliDist's first parameter, `logits` (agent/dreamer_utils.py:820-823, :199-201), so the
distribution is Bernoulli(logits = z) with z = sigmoid(x) and its mean is sigmoid(sigmoid(x)).

Each backward returns (gradient, scale): the scale is the magnitude of the terms an element is summed from, what a rounding error of the
element is proportional to (the convention of tests/gauss_restatement.py)."""
import torch
import torch.nn.functional as F


def binary_like(x, t):
    """Independent(Bernoulli(logits = sigmoid(x)), 1).log_prob(t) on a one-wide event, elementwise: t z - softplus(z)"""
    z = torch.sigmoid(x)
    return t * z - F.softplus(z)


def binary_like_scale(x, t):
    z = torch.sigmoid(x)
    return (t * z).abs() + F.softplus(z)


def binary_mean(x):
    return torch.sigmoid(torch.sigmoid(x))


def binary_like_bwd(x, t, g):
    """d like / dx = g (t - sigmoid(z)) z (1 - z); 1 - z as sigmoid(-x): no cancellation at either end"""
    z, omz = torch.sigmoid(x), torch.sigmoid(-x)
    p = torch.sigmoid(z)
    return g * (t - p) * (z * omz), g.abs() * (t.abs() + p) * (z * omz)


def imag_probs(x, term):
    """p [H1, N]: the head's mean at the H1 rollout states, row 0 replaced by 1 - term where term [N] is given (agent/dreamer.py:274-280)"""
    p = binary_mean(x)
    if term is not None:
        p = torch.cat([(1.0 - term)[None], p[1:]], 0)
    return p


def imag_discount(x, term, gamma):
    """-> disc = gamma p, weight = cumprod(cat(1, p[:-1])) multiplied in time order (agent/dreamer.py:283-286)"""
    p = imag_probs(x, term)
    w = [torch.ones_like(p[0])]
    for t in range(1, p.shape[0]):
        w.append(w[-1] * p[t - 1])
    return gamma * p, torch.stack(w, 0)


def imag_discount_bwd(x, gdisc, term_given, gamma):
    z, omz = torch.sigmoid(x), torch.sigmoid(-x)
    p, omp = torch.sigmoid(z), torch.sigmoid(-z)
    d = gdisc * gamma * (p * omp) * (z * omz)
    if term_given:
        d = torch.cat([torch.zeros_like(d[:1]), d[1:]], 0)
    return d, d.abs()


def lambda_return_disc(reward, value, disc, lam):
    """lambda_return with a tensor pcont (agent/dreamer_utils.py:228-253): reward, disc [H(+1), N] (a row H is not read), value [H+1, N]
    -> [H, N]: R_t = r_t + d_t ((1 - lam) v_{t+1} + lam R_{t+1}), R_H = v_H"""
    H = value.shape[0] - 1
    agg, out = value[H], []
    for t in range(H - 1, -1, -1):
        inp = reward[t] + disc[t] * value[t + 1] * (1.0 - lam)
        agg = inp + disc[t] * lam * agg
        out.append(agg)
    return torch.stack(out[::-1], 0)


def lambda_return_disc_scale(reward, value, disc, lam):
    r, v, d = reward.abs(), value.abs(), disc.abs()
    H = value.shape[0] - 1
    agg, out = v[H], []
    for t in range(H - 1, -1, -1):
        agg = r[t] + d[t] * v[t + 1] * abs(1.0 - lam) + d[t] * abs(lam) * agg
        out.append(agg)
    return torch.stack(out[::-1], 0)


def lambda_return_disc_bwd(gret, value, disc, ret, lam, rows):
    """-> (dreward, dvalue, ddisc), their scales; rows: H or H + 1 rows in dreward and ddisc (row H zero).  `ret` is the forward's output."""
    H = value.shape[0] - 1
    z = torch.zeros_like(value[0])
    a, A = z, z
    dr, dv, dd, sr, sv, sd = [], [z], [], [], [z], []
    for t in range(H):
        dprev = disc[t - 1] if t > 0 else z
        a = gret[t] + dprev * lam * a
        A = gret[t].abs() + dprev.abs() * abs(lam) * A
        rn = value[H] if t == H - 1 else ret[t + 1]
        dr.append(a); sr.append(A)
        dd.append(a * ((1.0 - lam) * value[t + 1] + lam * rn))
        sd.append(A * (abs(1.0 - lam) * value[t + 1].abs() + abs(lam) * rn.abs()))
        last = t == H - 1
        dv.append(disc[t] * a if last else disc[t] * (1.0 - lam) * a)
        sv.append(disc[t].abs() * A if last else disc[t].abs() * abs(1.0 - lam) * A)
    if rows == H + 1:
        dr.append(z); dd.append(z); sr.append(z); sd.append(z)
    st = lambda xs: torch.stack(xs, 0)
    return (st(dr), st(dv), st(dd)), (st(sr), st(sv), st(sd))
