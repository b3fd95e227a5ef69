"""The loss, sampling and optimiser kernels of csrc/dist.hip and csrc/optim.hip against float64 references computed on the host
from the same fp32 inputs.

The references are the oracle's own functions (oracle/genrl_oracle.py) run on float64 copies of the inputs, with gradients taken
by autograd, so that the semantics are checked along with the rounding.  Scalar parameters (unimix, discount, lambda, mix, free
nats) are the fp32 values the kernels receive.  The exception is the two-hot head: its reference is a short float64 restatement
on the kernel's fp32 bucket table (a float64 linspace differs from it by ~1e-6, which moves the two-hot weights by more than the
bound).

The shapes sit on both sides of every boundary in the code: the lane-group width W = 4 / 8 / 16 / 32 / 64 that dispatch_w picks
from K (and K = 65, refused), cat_kl_fwd's loop over the latents in steps of 256 / W, the two plane paths of onehot_bwd_h2, every
register-slice width of align_index_kernel, the 4-rows-per-workgroup kernels with a ragged last workgroup, the 256-thread loops
of the KL balance and the MSE likelihood, and the grid-stride loop of the gradient norm past 1024 workgroups.  Misaligned views
take the scalar paths of the gradient norm and Adam.

Bounds are per element: |kernel - float64| <= K * 2^-24 * S, where S is a float64 magnitude of the element's terms.  Each K
sits about ten times above the largest ratio measured on an MI355X (RATIOS records them per run).  Outputs are prefilled with
NaN, and every output buffer has padding columns and a guard row that must come back bit-identical.  Discrete outputs (samples,
modes, alignment indices) must be exactly the float64 choice wherever that choice has a clear margin."""
import math
from types import SimpleNamespace
from unittest import mock

import pytest
import torch

from f64check import PAD, checker, in_buf, out_buf, untouched
from oracle import genrl_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]

EINVAL = 1
UNIMIX = 0.99

# K per checked quantity (see the module docstring)
K = {
    'cat.probs': 200, 'cat.dlogits': 64, 'cat.kl': 32, 'cat.ent': 20, 'cat.dkl': 128,
    'twohot.logp': 100, 'twohot.mean': 32, 'twohot.dlogits': 48,
    'klbal.loss': 200, 'klbal.grad': 10,
    'lambda.ret': 20, 'lambda.grad': 18,
    'mse.like': 16, 'mse.dmean': 10,
    'maxcos.r': 40, 'maxcos.dv': 44,
    'gnorm': 12, 'adam.p': 12, 'adam.m': 24, 'adam.v': 22, 'scale': 10,
}
RATIOS = {}             # largest |kernel - float64| / (2^-24 S) seen per quantity (the margin each K leaves)
within = checker(K, RATIOS)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(x):
    """the fp32 value a float argument reaches the kernel as"""
    return float(torch.tensor(x, dtype=torch.float32))


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    return lib()


def vec_out(n, dtype=torch.float32):
    fill = PAD if dtype == torch.float32 else -7
    buf = torch.full((n + 4,), fill, dtype=dtype, device='cuda')
    buf[:n] = float('nan') if dtype == torch.float32 else -9
    return buf, buf[:n]


def vec_untouched(what, buf, n):
    fill = PAD if buf.dtype == torch.float32 else -7
    assert (buf[n:] == fill).all(), f'{what}: a kernel wrote past its output'


# ====================================================================================== categorical latents
KS = [1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]


def cat_inputs(G, K, seed):
    """logits of spread 2 with per-group offsets, q in [0.05, 1.05); group 0: all logits and q equal; group 1 (K >= 3): two equal
    maxima at classes 1 and K - 1 with equal q there (exact ties: the first index wins)"""
    g = gen(seed)
    lg = torch.randn(G, K, generator=g) * 2 + 3 * torch.randn(G, 1, generator=g)
    q = torch.rand(G, K, generator=g) + 0.05
    lg[0] = 0.5; q[0] = 0.7
    if K >= 3 and G > 1:
        lg[1] = torch.rand(K, generator=g) - 2
        lg[1, 1] = lg[1, K - 1] = 4.0
        q[1, 1] = q[1, K - 1] = 0.3
    return lg, q


def probs64(lg):
    return O.unimix_probs(lg.double(), UNIMIX)


def check_choice(what, sample, score, ties=()):
    """sample: the kernel's one-hot [G, K]; score: the float64 scores.  Where the best and second-best scores differ by more than
    1e-5 relative the class is the float64 argmax, elsewhere one of the near-tied classes; rows in `ties` (exact ties planted in
    the fp32 inputs) must give their first tied index."""
    s = sample.detach().cpu()
    G, K = s.shape
    assert ((s == 0) | (s == 1)).all() and (s.sum(1) == 1).all(), f'{what}: not one-hot'
    got = s.argmax(1)
    top = score.max(1).values
    best = score.argmax(1)
    if K > 1:
        second = score.scatter(1, best[:, None], -math.inf).max(1).values
        clear = top - second > 1e-5 * top.abs()
        bad = clear & (got != best)
        assert not bad.any(), f'{what}: {int(bad.sum())} groups off the float64 argmax, first {int(bad.nonzero()[0])}'
        near = score.gather(1, got[:, None])[:, 0] >= top - 1e-5 * top.abs()
        assert near.all(), f'{what}: a class outside the near-tied set'
    for row, first in ties:
        assert int(got[row]) == first, (what, row, int(got[row]), first)


def cat_ties(G, K):
    return [(0, 0)] + ([(1, 1)] if K >= 3 and G > 1 else [])


def cat_bwd_scale(p, pn, g):
    """float64 magnitude of p (a (g - <g, pn>) / s - <., p>) per element"""
    return 2 * p * (g.abs() + (g.abs() * pn).sum(-1, keepdim=True)) + 1e-30


@pytest.mark.parametrize('K', KS)
def test_onehot_sample_and_mode(L, K):
    """genrl_onehot_fwd at every W: the sample (argmax pn / q) and the mode (argmax pn) against the float64 choice, the unimix
    probabilities against float64; G * W is not a multiple of 256 (a partial last workgroup)"""
    G = 1001
    lg, q = cat_inputs(G, K, K)
    ld, qd = lg.cuda(), q.cuda()
    pn = probs64(lg)
    for noise in (True, False):
        sb, sample = vec_out(G * K)
        pb, probs = vec_out(G * K)
        assert L.genrl_onehot_fwd(ld.data_ptr(), qd.data_ptr() if noise else None, sample.data_ptr(), probs.data_ptr(), G, K, UNIMIX,
                                  stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('sample', sb, G * K); vec_untouched('probs', pb, G * K)
        score = pn / q.double() if noise else pn
        check_choice('sample' if noise else 'mode', sample.view(G, K), score, cat_ties(G, K))
        within('cat.probs', probs.view(G, K), pn, pn)
        ref = O.onehot_sample(lg.double(), q.double(), UNIMIX) if noise else O.onehot_mode(lg.double(), UNIMIX)
        agree = ref.argmax(1) == sample.view(G, K).cpu().argmax(1)
        assert agree.float().mean() > 0.99          # (the oracle's sample / mode: the same choice outside near ties)
    # probs may be absent
    sb, sample = vec_out(G * K)
    assert L.genrl_onehot_fwd(ld.data_ptr(), qd.data_ptr(), sample.data_ptr(), None, G, K, UNIMIX, stream()) == 0
    torch.cuda.synchronize()
    check_choice('sample', sample.view(G, K), pn / q.double(), cat_ties(G, K))


def onehot_grad_ref(lg, q, up):
    """float64 autograd of the oracle's straight-through sample at upstream `up`"""
    l64 = lg.double().requires_grad_()
    O.onehot_sample(l64, q.double(), UNIMIX).backward(up)
    return l64.grad


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('acc', [0, 1])
def test_onehot_straight_through_backward(L, K, acc):
    """genrl_onehot_bwd at every W, with and without accumulate, against float64 autograd of the oracle's sample"""
    G = 1001
    lg, q = cat_inputs(G, K, 10 + K)
    gs = torch.randn(G, K, generator=gen(K))
    prior = torch.randn(G, K, generator=gen(K + 1))
    ld, gd = lg.cuda(), gs.cuda()
    db, dl = vec_out(G * K)
    if acc:
        dl.copy_(prior.view(-1))
    assert L.genrl_onehot_bwd(ld.data_ptr(), gd.data_ptr(), dl.data_ptr(), G, K, UNIMIX, acc, stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('dlogits', db, G * K)
    ref = onehot_grad_ref(lg, q, gs.double())
    pn = probs64(lg); p = torch.softmax(lg.double(), -1)
    sc = cat_bwd_scale(p, pn, gs.double())
    if acc:
        ref, sc = ref + prior.double(), sc + prior.double().abs()
    within('cat.dlogits', dl.view(G, K), ref, sc)


CAT_KL_CASES = [(K, 7) for K in KS] + [(3, 63), (4, 64), (4, 65), (4, 200), (33, 3), (64, 4), (64, 5)]


def cat_kl_scale(lp, lq):
    pp, pq = probs64(lp), probs64(lq)
    a, b = O.probs_to_logits(pp).abs(), O.probs_to_logits(pq).abs()
    return (pp * (a + b + 1)).sum(-1).sum(-1), (pp * (a + 1)).sum(-1).sum(-1), (pq * (b + 1)).sum(-1).sum(-1)


@pytest.mark.parametrize('K,S', CAT_KL_CASES)
def test_cat_kl_forward(L, K, S):
    """genrl_cat_kl_fwd: KL(P || Q) summed over S latents, with and without the two entropies, against the oracle's cat_kl /
    cat_entropy; S on both sides of the loop step 256 / W"""
    R = 37
    g = gen(K * 1000 + S)
    lp = torch.randn(R, S, K, generator=g) * 2; lq = torch.randn(R, S, K, generator=g) * 2
    lq[3] = lp[3]                                          # P == Q: KL 0
    lpd, lqd = lp.cuda(), lq.cuda()
    klr = O.cat_kl(lp.double(), lq.double(), UNIMIX)
    epr, eqr = O.cat_entropy(lp.double(), UNIMIX), O.cat_entropy(lq.double(), UNIMIX)
    skl, sep, seq_ = cat_kl_scale(lp, lq)
    for ent in (True, False):
        kb, kl = vec_out(R); eb, ep = vec_out(R); qb, eq = vec_out(R)
        assert L.genrl_cat_kl_fwd(lpd.data_ptr(), lqd.data_ptr(), kl.data_ptr(), ep.data_ptr() if ent else None,
                                  eq.data_ptr() if ent else None, R, S, K, UNIMIX, stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('kl', kb, R); vec_untouched('ent_p', eb, R); vec_untouched('ent_q', qb, R)
        within('cat.kl', kl, klr, skl)
        assert float(kl[3]) == 0.0
        if ent:
            within('cat.ent[p]', ep, epr, sep)
            within('cat.ent[q]', eq, eqr, seq_)
        else:
            assert ep.isnan().all() and eq.isnan().all()


@pytest.mark.parametrize('K,S', CAT_KL_CASES)
def test_cat_kl_backward(L, K, S):
    """genrl_cat_kl_bwd with dlp only, dlq only and both, against float64 autograd of sum_r gp[r] KL_r (dlp) and gq[r] KL_r (dlq)"""
    R = 37
    g = gen(K * 100 + S)
    lp = torch.randn(R, S, K, generator=g) * 2; lq = torch.randn(R, S, K, generator=g) * 2
    gp = torch.randn(R, generator=g); gq = torch.randn(R, generator=g)
    lpd, lqd, gpd, gqd = lp.cuda(), lq.cuda(), gp.cuda(), gq.cuda()
    a, b = lp.double().requires_grad_(), lq.double().requires_grad_()
    (O.cat_kl(a, b.detach(), UNIMIX) * gp.double()).sum().backward()
    (O.cat_kl(a.detach(), b, UNIMIX) * gq.double()).sum().backward()
    pp, pq = probs64(lp), probs64(lq)
    sp, sq = torch.softmax(lp.double(), -1), torch.softmax(lq.double(), -1)
    up = O.probs_to_logits(pp).abs() + O.probs_to_logits(pq).abs() + 1
    sdp = cat_bwd_scale(sp, pp, up) * gp.double().abs()[:, None, None]
    sdq = cat_bwd_scale(sq, pq, pp / pq) * gq.double().abs()[:, None, None]
    N = R * S * K
    for want_p, want_q in ((True, False), (False, True), (True, True)):
        pb, dlp = vec_out(N); qb, dlq = vec_out(N)
        assert L.genrl_cat_kl_bwd(lpd.data_ptr(), lqd.data_ptr(), gpd.data_ptr(), gqd.data_ptr(), dlp.data_ptr() if want_p else None,
                                  dlq.data_ptr() if want_q else None, R, S, K, UNIMIX, stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('dlp', pb, N); vec_untouched('dlq', qb, N)
        if want_p:
            within('cat.dkl[dlp]', dlp.view(R, S, K), a.grad, sdp)
        else:
            assert dlp.isnan().all()
        if want_q:
            within('cat.dkl[dlq]', dlq.view(R, S, K), b.grad, sdq)
        else:
            assert dlq.isnan().all()


def test_categorical_kernels_refuse_65_classes(L):
    """K = 65: every dispatch_w entry point returns GENRL_EINVAL and writes nothing"""
    G, K = 8, 65
    x = torch.zeros(G * K, device='cuda'); gr = torch.ones(G, device='cuda')
    outs = [torch.full((G * K,), float('nan'), device='cuda') for _ in range(4)]
    assert L.genrl_onehot_fwd(x.data_ptr(), None, outs[0].data_ptr(), outs[1].data_ptr(), G, K, UNIMIX, stream()) == EINVAL
    assert L.genrl_onehot_bwd(x.data_ptr(), x.data_ptr(), outs[2].data_ptr(), G, K, UNIMIX, 0, stream()) == EINVAL
    assert L.genrl_cat_kl_fwd(x.data_ptr(), x.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 2, 4, K, UNIMIX,
                              stream()) == EINVAL
    assert L.genrl_cat_kl_bwd(x.data_ptr(), x.data_ptr(), gr.data_ptr(), gr.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), 2, 4, K,
                              UNIMIX, stream()) == EINVAL
    torch.cuda.synchronize()
    assert all(o.isnan().all() for o in outs)


# (S, K): rowlen S * K; W == K with rowlen 64 / 1024 -> one workgroup per plane row; else the genrl_split_h2 pass
H2_CASES = [(16, 4, 'row'), (2, 32, 'row'), (32, 32, 'row'), (16, 64, 'row'), (4, 4, 'split'), (8, 5, 'split'), (64, 32, 'split')]


@pytest.mark.parametrize('S,K,path', H2_CASES)
@pytest.mark.parametrize('acc', [0, 1])
def test_onehot_plane_outputs(L, S, K, path, acc):
    """genrl_onehot_fwd_h2 / genrl_onehot_bwd_h2: the fp32 outputs against float64, the planes equal to genrl_split_h2 of the
    kernel's own fp32 output; the forward planes hold 0 / 1 at scale 2^14 (inv 2^-14)"""
    from genrl_amd import planes
    R = 70
    rowlen, G = S * K, 70 * S
    lg, q = cat_inputs(G, K, S * K + acc)
    ld, qd = lg.cuda(), q.cuda()
    sb, sample = vec_out(G * K)
    P = planes.Planes(R, rowlen, 'cuda')
    assert L.genrl_onehot_fwd_h2(ld.data_ptr(), qd.data_ptr(), sample.data_ptr(), None, G, K, UNIMIX, P.ptr(), rowlen, P.ld, P.plane,
                                 P.inv_ptr(), stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('sample', sb, G * K)
    check_choice('sample[h2]', sample.view(G, K), probs64(lg) / q.double(), cat_ties(G, K))
    assert (P.inv == 2.0 ** -14).all()
    ref = planes.split(sample.view(R, rowlen))
    assert torch.equal(P.inv, ref.inv) and torch.equal(P.t[:, :, :rowlen], ref.t[:, :, :rowlen])
    assert torch.equal(P.float(), sample.view(R, rowlen))
    gs = torch.randn(G, K, generator=gen(S + K))
    prior = torch.randn(G, K, generator=gen(S + K + 1)) * 3
    gd = gs.cuda()
    db, dl = vec_out(G * K)
    if acc:
        dl.copy_(prior.view(-1))
    Pd = planes.Planes(R, rowlen, 'cuda')
    assert L.genrl_onehot_bwd_h2(ld.data_ptr(), gd.data_ptr(), dl.data_ptr(), G, K, UNIMIX, acc, Pd.ptr(), rowlen, Pd.ld, Pd.plane,
                                 Pd.inv_ptr(), stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('dlogits', db, G * K)
    gref = onehot_grad_ref(lg, q, gs.double())
    sc = cat_bwd_scale(torch.softmax(lg.double(), -1), probs64(lg), gs.double())
    if acc:
        gref, sc = gref + prior.double(), sc + prior.double().abs()
    within('cat.dlogits[h2]', dl.view(G, K), gref, sc, key='cat.dlogits')
    ref = planes.split(dl.view(R, rowlen))
    assert torch.equal(Pd.inv, ref.inv) and torch.equal(Pd.t[:, :, :rowlen], ref.t[:, :, :rowlen])


@pytest.mark.parametrize('with_gsample', [False, True])
def test_onehot_masked_forms(L, with_gsample):
    """genrl_onehot_fwd_masked / genrl_onehot_bwd_masked (the scan's forms): sample2 = scale[row] * sample, idx2 = the class or -1
    where the scale is 0, and the backward of upstream = gsample + scale[row] * g2 against float64; scale rows 0, 1 and 0.37"""
    rows, S, K = 33, 8, 32
    G = rows * S
    lg, q = cat_inputs(G, K, 77)
    scale = torch.tensor([0.0, 1.0, 0.37] * 11)
    ld, qd, scd = lg.cuda(), q.cuda(), scale.cuda()
    sb, sample = vec_out(G * K); s2b, sample2 = vec_out(G * K)
    ib, idx2 = vec_out(G, torch.int32)
    assert L.genrl_onehot_fwd_masked(ld.data_ptr(), qd.data_ptr(), sample.data_ptr(), sample2.data_ptr(), idx2.data_ptr(), scd.data_ptr(),
                                     S, G, K, UNIMIX, stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('sample', sb, G * K); vec_untouched('sample2', s2b, G * K); vec_untouched('idx2', ib, G)
    s = sample.view(G, K).cpu()
    check_choice('sample[masked]', s, probs64(lg) / q.double(), cat_ties(G, K))
    rs = scale.repeat_interleave(S)
    assert torch.equal(sample2.view(G, K).cpu(), s * rs[:, None])
    assert torch.equal(idx2.cpu(), torch.where(rs != 0, s.argmax(1), -1).int())
    g = gen(78)
    gs = torch.randn(G, K, generator=g); g2 = torch.randn(G, K, generator=g)
    gsd, g2d = gs.cuda(), g2.cuda()
    for acc in (0, 1):
        db, dl = vec_out(G * K)
        prior = torch.randn(G, K, generator=g)
        if acc:
            dl.copy_(prior.view(-1))
        assert L.genrl_onehot_bwd_masked(ld.data_ptr(), gsd.data_ptr() if with_gsample else None, g2d.data_ptr(), scd.data_ptr(), S,
                                         dl.data_ptr(), G, K, UNIMIX, acc, stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('dlogits', db, G * K)
        up = rs.double()[:, None] * g2.double() + (gs.double() if with_gsample else 0)
        sup = rs.double()[:, None] * g2.double().abs() + (gs.double().abs() if with_gsample else 0)
        gref = onehot_grad_ref(lg, q, up)
        sc = cat_bwd_scale(torch.softmax(lg.double(), -1), probs64(lg), sup)
        if acc:
            gref, sc = gref + prior.double(), sc + prior.double().abs()
        within('cat.dlogits[masked]', dl.view(G, K), gref, sc, key='cat.dlogits')


# ====================================================================================== two-hot symlog head
def twohot_x(R, b32, seed):
    """0, +-1e-7, values whose fp32 symlog sits on a bucket, beyond symexp(+-20), +-3e38, then spread values"""
    special = [0.0, 1e-7, -1e-7, 3e38, -3e38, 1e9, -1e9, 4.9e8, -4.9e8]
    b = b32.double()
    special += [float(O.symexp(b[j])) for j in (0, 1, 60, 126, 127, 128, 200, 253, 254)]
    x = torch.tensor(special, dtype=torch.float32)
    rest = O.symexp(torch.randn(max(R - len(x), 0), generator=gen(seed)) * 6).float()
    return torch.cat([x, rest])[:R]


def twohot_ref(logits, x, b):
    """float64 TwoHotDist.log_prob target (agent/dreamer_utils.py:147-171) on the bucket table b -> (log_prob, target, |symlog x|)"""
    xs = O.symlog(x)
    below = ((b <= xs[:, None]).sum(-1) - 1).clamp(0, 254)
    above = (255 - (b > xs[:, None]).sum(-1)).clamp(0, 254)
    eq = below == above
    db = torch.where(eq, 1.0, (b[below] - xs).abs()); da = torch.where(eq, 1.0, (b[above] - xs).abs())
    wb, wa = da / (db + da), db / (db + da)
    t = torch.zeros(len(x), 255, dtype=torch.float64)
    t.scatter_add_(1, below[:, None], wb[:, None]); t.scatter_add_(1, above[:, None], wa[:, None])
    logp = logits - torch.logsumexp(logits, -1, keepdim=True)
    return (t * logp).sum(-1), t, below, above, xs.abs()


TWOHOT_CASES = [(1, 255, 256), (3, 256, 255), (4, 300, 260), (5, 255, 260), (4097, 256, 256), (4097, 300, 255), (100003, 256, 260)]


@pytest.mark.parametrize('R,ld,ldd', TWOHOT_CASES)
def test_twohot_heads(L, R, ld, ldd):
    """genrl_twohot_fwd / genrl_twohot_bwd, mode 0 (log_prob of x) and 1 (mean = symexp(E bucket)), against float64 on the kernel's
    fp32 bucket table; logits lines ld apart (NaN padding), dlogits lines ldd apart: column 255 a defined zero when ldd > 255,
    the columns past it untouched"""
    from genrl_amd import ops
    bd = ops.twohot_buckets('cuda')
    b = bd.cpu().double()
    delta = float((b[1:] - b[:-1]).min())
    g = gen(R + ld + ldd)
    lg = torch.randn(R, 255, generator=g) * 2
    if R > 8:
        lg[7] = -30.0; lg[7, 250] = 10.0                   # peaked on a large bucket: mean ~ symexp(19)
    x = twohot_x(R, bd.cpu(), R)
    gout = torch.randn(R, generator=g)
    lgd = in_buf(lg, ld)
    xd, god = x.cuda(), gout.cuda()
    l64 = lg.double()
    logp, t, below, above, axs = twohot_ref(l64, x.double(), b)
    m = l64.max(-1, keepdim=True).values
    p = torch.softmax(l64, -1)
    lse = torch.logsumexp(l64, -1)
    lb, la = l64.gather(1, below[:, None])[:, 0], l64.gather(1, above[:, None])[:, 0]
    move = (axs + 1) / delta                               # the weights' sensitivity to the rounding of the fp32 symlog
    s_logp = (lb - lse).abs() + (la - lse).abs() + lse.abs() + m[:, 0].abs() + (la - lb).abs() * move
    mu = (p * b).sum(-1)
    A = (p * b.abs()).sum(-1)
    mean = O.symexp(mu)
    s_mean = torch.exp(mu.abs()) * (A + mu.abs() + 1)
    cols = torch.arange(255)
    win = ((cols[None, :] >= below[:, None] - 1) & (cols[None, :] <= above[:, None] + 1)).double()
    for mode in (0, 1):
        ob, out = vec_out(R)
        assert L.genrl_twohot_fwd(lgd.data_ptr(), ld, xd.data_ptr(), bd.data_ptr(), out.data_ptr(), R, mode, stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('out', ob, R)
        if mode == 0:
            within('twohot.logp', out, logp, s_logp)
        else:
            within('twohot.mean', out, mean, s_mean)
        cw = 256 if ldd > 255 else 255
        db_, dl = out_buf(R, cw, ldd)
        assert L.genrl_twohot_bwd(lgd.data_ptr(), ld, xd.data_ptr(), bd.data_ptr(), god.data_ptr(), dl.data_ptr(), ldd, R, mode,
                                  stream()) == 0
        torch.cuda.synchronize()
        untouched('dlogits', db_, dl)
        if ldd > 255:
            assert (dl[:, 255] == 0).all()
        ga = gout.double()[:, None]
        if mode == 0:
            ref = ga * (t - p)
            sc = ga.abs() * (p * (1 + (l64 - m).abs()) + t + win * move[:, None])
        else:
            ref = ga * torch.exp(mu.abs())[:, None] * p * (b - mu[:, None])
            bm = (b - mu[:, None]).abs()
            sc = ga.abs() * torch.exp(mu.abs())[:, None] * p * ((1 + (l64 - m).abs()) * bm + b.abs() + mu.abs()[:, None]
                                                                 + A[:, None] * (bm + 1))
        within('twohot.dlogits', dl[:, :255], ref, sc)
    # the oracle's own two-hot log_prob / mean (float64 linspace buckets) agree with the restatement to its bucket offsets
    xs = x.double()[:64]
    assert torch.allclose(O.twohot_logprob(l64[:64], xs[:, None]), logp[:64], rtol=1e-4, atol=1e-4)


# ====================================================================================== balanced free-nats KL loss
def kl_value_stand_in(lhs, rhs):
    """cat_kl replaced by the per-row KL values themselves (gradient 1 into whichever side is not detached): kl_loss then gives
    d loss / d KL of each side at the kernel's own fp32 KL"""
    return lhs.detach() + (lhs - lhs.detach()) + (rhs - rhs.detach())


@pytest.mark.parametrize('R', [1, 255, 256, 257, 70000])
@pytest.mark.parametrize('mix', [0.15, 0.8])
def test_kl_balance(L, R, mix):
    """genrl_cat_kl_fwd -> genrl_kl_balance_fwd / _bwd against the oracle's kl_loss: the per-row KL against float64 from the
    logits; the loss and the two sides' per-row gradients at the kernel's KL, with free = the KL of a block of identical rows (an
    exact tie: torch.maximum gives half the gradient there) and free = 0 with rows of P == Q (KL exactly 0, also a tie)"""
    S, Kc = 4, 8
    g = gen(R + int(mix * 100))
    lp = torch.randn(R, S, Kc, generator=g) * 2; lq = torch.randn(R, S, Kc, generator=g) * 2
    tie = torch.arange(R) % 5 == 1
    same = ((torch.arange(R) % 7 == 3) | (torch.arange(R) == R - 1)) & ~tie
    lp[tie] = lp[min(1, R - 1)].clone(); lq[tie] = lq[min(1, R - 1)].clone()
    lq[same] = lp[same]
    kb, kl = vec_out(R)
    lpd, lqd = lp.cuda(), lq.cuda()
    assert L.genrl_cat_kl_fwd(lpd.data_ptr(), lqd.data_ptr(), kl.data_ptr(), None, None, R, S, Kc, UNIMIX, stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('kl', kb, R)
    post64, prior64 = lp.double(), lq.double()
    _, value = O.kl_loss(post64, prior64, False, 1 - f32(mix), 0.0)
    within('cat.kl[rows]', kl, value, cat_kl_scale(lp, lq)[0], key='cat.kl')
    k32 = kl.cpu()
    assert (k32[same] == 0).all()
    frees = [0.0]
    if tie.any():
        frees.append(float(k32[tie][0]))
        assert (k32[tie] == frees[1]).all()
    gloss = torch.tensor([1.7])
    gld = gloss.cuda()
    for free in frees:
        lb, loss = vec_out(1)
        assert L.genrl_kl_balance_fwd(kl.data_ptr(), R, mix, free, loss.data_ptr(), stream()) == 0
        pb, gp = vec_out(R); qb, gq = vec_out(R)
        assert L.genrl_kl_balance_bwd(kl.data_ptr(), gld.data_ptr(), R, mix, free, gp.data_ptr(), gq.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('loss', lb, 1); vec_untouched('gp', pb, R); vec_untouched('gq', qb, R)
        a = k32.double().requires_grad_(); c = k32.double().requires_grad_()
        with mock.patch.object(O, 'cat_kl', kl_value_stand_in):
            ref, _ = O.kl_loss(a, c, False, 1 - f32(mix), free)
        ref.backward(gloss.double()[0])
        mx = torch.maximum(k32.double(), torch.tensor(free, dtype=torch.float64))
        within('klbal.loss', loss, ref.detach().reshape(1), mx.abs().mean().reshape(1))
        within('klbal.grad[gp]', gp, a.grad, a.grad.abs() + 1e-300, key='klbal.grad')
        within('klbal.grad[gq]', gq, c.grad, c.grad.abs() + 1e-300, key='klbal.grad')
        at_tie, above = k32 == free, k32 > free
        assert at_tie.any()
        gpc = gp.cpu()
        if above.any():
            assert (gpc[at_tie] * 2 == gpc[above][0]).all()          # half the gradient at a tie
        assert (gpc[k32 < free] == 0).all()


# ====================================================================================== lambda-return scan
def lam_scales(absr, absv, H, disc, lam):
    """float64 magnitudes of the forward recursion's terms and their propagation (rounding at step k carried by (disc lam)^(k-t))"""
    Sagg = absv[H]
    E = torch.zeros_like(absv[0])
    S = torch.zeros_like(absr)
    for t in range(H - 1, -1, -1):
        Sagg = absr[t] + disc * absv[t + 1] * (1 - lam) + disc * lam * Sagg
        E = Sagg + disc * lam * E
        S[t] = E
    return S


@pytest.mark.parametrize('H', [1, 2, 15, 16, 64])
@pytest.mark.parametrize('N', [1, 255, 256, 257, 65537])
def test_lambda_return(L, H, N):
    """genrl_lambda_return_fwd / _bwd against the oracle's lambda_return and its float64 autograd, for lambda 0 / 0.95 / 1 and
    discount 0.99 / 1; zero_tail 1: the reward gradient's row H is zero, 0: untouched"""
    g = gen(H * 100000 + N)
    reward = torch.randn(H, N, generator=g); value = torch.randn(H + 1, N, generator=g) * 3
    gret = torch.randn(H, N, generator=g)
    rd, vd, gd = reward.cuda(), value.cuda(), gret.cuda()
    combos = [(lam, disc) for lam in (0.0, 0.95, 1.0) for disc in (0.99, 1.0)]
    for c, (lam, disc) in enumerate(combos):
        lam32, disc32 = f32(lam), f32(disc)
        r64 = reward.double().requires_grad_(); v64 = value.double().requires_grad_()
        ret = O.lambda_return(r64, v64[:H], torch.full((H, N), disc32, dtype=torch.float64), v64[H], lam32)
        ret.backward(gret.double())
        ob, out = out_buf(H, N, N)
        assert L.genrl_lambda_return_fwd(rd.data_ptr(), vd.data_ptr(), out.data_ptr(), H, N, disc, lam, stream()) == 0
        zt = c % 2
        rb, dr = out_buf(H + 1, N, N)
        vb, dv = out_buf(H + 1, N, N)
        assert L.genrl_lambda_return_bwd(gd.data_ptr(), dr.data_ptr(), dv.data_ptr(), H, N, disc, lam, zt, stream()) == 0
        torch.cuda.synchronize()
        untouched('ret', ob, out); untouched('dvalue', vb, dv)
        untouched('dreward', rb, dr)
        assert (dr[H] == 0).all() if zt else dr[H].isnan().all()
        within('lambda.ret', out, ret.detach(), lam_scales(reward.double().abs(), value.double().abs(), H, disc32, lam32))
        # backward: a_t = gret_t + disc lam a_{t-1}; magnitudes and their propagation as in the forward
        ga = gret.double().abs()
        Sa = torch.zeros_like(ga); Ea = torch.zeros(N, dtype=torch.float64); acc = torch.zeros(N, dtype=torch.float64)
        for t in range(H):
            acc = ga[t] + disc32 * lam32 * acc
            Ea = acc + disc32 * lam32 * Ea
            Sa[t] = Ea
        within('lambda.grad[dreward]', dr[:H], r64.grad, Sa, key='lambda.grad')
        sv = torch.cat([torch.zeros(1, N, dtype=torch.float64), disc32 * Sa], 0)
        within('lambda.grad[dvalue]', dv, v64.grad, sv + 1e-300, key='lambda.grad')
        assert (dv[0] == 0).all()


# ====================================================================================== MSE image likelihood
@pytest.mark.parametrize('E', [1, 255, 256, 257, 12288])
@pytest.mark.parametrize('frames', [1, 7, 300])
def test_mse_likelihood(L, E, frames):
    """genrl_mse_fwd / _bwd: like = -sum (mean - (obs / 255 - 0.5))^2 per frame and its gradient, against float64 with the oracle's
    preprocess_obs; observations include 0 and 255"""
    g = gen(E * 1000 + frames)
    obs = torch.randint(0, 256, (frames, E), generator=g, dtype=torch.uint8)
    obs.view(-1)[::3] = 0; obs.view(-1)[1::5] = 255
    mean = torch.rand(frames, E, generator=g) - 0.5 + 0.1 * torch.randn(frames, E, generator=g)
    glike = torch.randn(frames, generator=g)
    md, od, gd = mean.cuda(), obs.cuda(), glike.cuda()
    lb, like = vec_out(frames)
    assert L.genrl_mse_fwd(md.data_ptr(), od.data_ptr(), like.data_ptr(), frames, E, stream()) == 0
    db, dm = out_buf(frames, E, E)
    assert L.genrl_mse_bwd(md.data_ptr(), od.data_ptr(), gd.data_ptr(), dm.data_ptr(), frames, E, stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('like', lb, frames); untouched('dmean', db, dm)
    m64 = mean.double().requires_grad_()
    target = O.preprocess_obs(obs.double())
    ref = -((m64 - target) ** 2).sum(-1)
    ref.backward(glike.double())
    d = (mean.double() - target).abs()
    t = mean.double().abs() + target.abs() + 0.5
    within('mse.like', like, ref.detach(), (d * (d + t)).sum(-1))
    within('mse.dmean', dm, m64.grad, 2 * glike.double().abs()[:, None] * (d + t))


# ====================================================================================== max-cosine reward
def maxcos_inputs(R, E, urow, seed):
    """u: Ru target rows of spread norms; v row r by r % 4: 0.5 x a random row (|u| > |v|), 2 x (|v| > |u|), u[urow[r]] (a tie),
    -u[urow[r]] (norms bitwise equal, u != v)"""
    g = gen(seed)
    Ru = max(R // 2, 1) if urow else R
    u = torch.randn(Ru, E, generator=g) * torch.exp(torch.randn(Ru, 1, generator=g))
    idx = torch.randint(0, Ru, (R,), generator=g) if urow else torch.arange(R)
    if urow and R > 2:
        idx[1] = idx[2]                                   # repeats
    ur = u[idx]
    rnd = torch.randn(R, E, generator=g)
    rnd = rnd / rnd.norm(dim=1, keepdim=True) * ur.norm(dim=1, keepdim=True)
    kind = torch.arange(R) % 4
    v = torch.where((kind == 0)[:, None], 0.5 * rnd, torch.where((kind == 1)[:, None], 2 * rnd, torch.where((kind == 2)[:, None], ur, -ur)))
    return u, idx, v


@pytest.mark.parametrize('E', [1, 48, 63, 64, 65, 1024, 1025])
@pytest.mark.parametrize('R', [1, 3, 4, 5, 9001])
@pytest.mark.parametrize('urow', [False, True])
def test_maxcos(L, E, R, urow):
    """genrl_maxcos_fwd / _bwd: sum (u / mn)(v / mn), mn = max(|u|, |v|), and its gradient in v, against the oracle's
    max_cosine_similarity and float64 autograd (torch.max splits the gradient evenly at a tie), u rows picked by urow"""
    u, idx, v = maxcos_inputs(R, E, urow, E * 10 + R)
    ud, vd = u.cuda(), v.cuda()
    ird = idx.cuda() if urow else None
    gout = torch.randn(R, generator=gen(R + E))
    gd = gout.cuda()
    ob, out = vec_out(R)
    assert L.genrl_maxcos_fwd(ud.data_ptr(), vd.data_ptr(), ird.data_ptr() if urow else None, out.data_ptr(), R, E, stream()) == 0
    db, dv = out_buf(R, E, E)
    assert L.genrl_maxcos_bwd(ud.data_ptr(), vd.data_ptr(), ird.data_ptr() if urow else None, gd.data_ptr(), dv.data_ptr(), R, E,
                              stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('out', ob, R); untouched('dv', db, dv)
    u64 = u.double()[idx]
    v64 = v.double().requires_grad_()
    ref = O.max_cosine_similarity(u64, v64)
    ref.backward(gout.double())
    nu, nv = u64.norm(dim=1), v.double().norm(dim=1)
    mx2 = torch.maximum(nu, nv) ** 2
    uv = (u64.abs() * v.double().abs()).sum(1)
    within('maxcos.r', out, ref.detach(), uv / mx2)
    sc = gout.double().abs()[:, None] * (u64.abs() / mx2[:, None] + 2 * uv[:, None] * v.double().abs() / (nv ** 4)[:, None])
    within('maxcos.dv', dv, v64.grad, sc)


# ====================================================================================== reward alignment
ALIGN_E = [24, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049, 3000]
ALIGN_TNF = [(32, 1, 1), (32, 4, 300), (32, 8, 1), (9, 8, 300), (2, 1, 1)]


def identity_conv_in(p, stoch):
    return stoch.reshape(list(stoch.shape[:-2]) + [-1])


@pytest.mark.parametrize('E', ALIGN_E)
@pytest.mark.parametrize('T,nf,N', ALIGN_TNF)
def test_align_index(L, E, T, nf, N):
    """genrl_align_index at every register-slice width (EPT 2 / 4 / 6 / 8 and the re-reading path past E = 2048): each column
    has its best window planted (agent rows t*..t*+nf-1 = the nf target rows); the flattened target row index must equal the
    oracle's video_text_reward alignment (its conv_in projection replaced by the identity) exactly, and the rewards the product
    computes from it (genrl_maxcos_fwd with urow) must match the oracle's"""
    g = gen(E * 100 + T * 10 + nf)
    ct = torch.randn(T, N, E, generator=g)
    ca = torch.randn(T, N, E, generator=g) * torch.exp(0.3 * torch.randn(T, N, 1, generator=g))
    best = torch.randint(0, T - nf, (N,), generator=g)
    for n in range(N):
        ca[int(best[n]):int(best[n]) + nf, n] = ct[:nf, n]
    ctd, cad = ct.cuda(), ca.cuda()
    ub, urow = vec_out(T * N, torch.int64)
    assert L.genrl_align_index(ctd.data_ptr(), cad.data_ptr(), urow.data_ptr(), T, N, E, nf, stream()) == 0
    torch.cuda.synchronize()
    vec_untouched('urow', ub, T * N)
    cfg = SimpleNamespace(n_frames=nf)
    with mock.patch.object(O, 'conv_in', identity_conv_in):
        reward, ts_idx = O.video_text_reward(None, cfg, ca.double()[..., None], ct.double()[..., None])
        # the margin the planted windows leave (the test's precondition)
        scores = torch.stack([O.max_cosine_similarity(ct.double()[:nf], ca.double()[t:t + nf]).mean(0) for t in range(T - nf)], 0)
    top2 = scores.topk(min(2, T - nf), 0).values
    assert torch.equal(scores.argmax(0), best)
    if T - nf > 1:
        assert (top2[0] - top2[1] > 0.05).all()
    want = ts_idx * N + torch.arange(N)[None, :]
    assert torch.equal(urow.view(T, N).cpu(), want)
    rb, r = vec_out(T * N)
    assert L.genrl_maxcos_fwd(ctd.data_ptr(), cad.data_ptr(), urow.data_ptr(), r.data_ptr(), T * N, E, stream()) == 0
    torch.cuda.synchronize()
    u64 = ct.double().reshape(T * N, E)[want.reshape(-1)]
    v64 = ca.double().reshape(T * N, E)
    mx2 = torch.maximum(u64.norm(dim=1), v64.norm(dim=1)) ** 2
    within('maxcos.r[aligned]', r, reward.reshape(-1), (u64.abs() * v64.abs()).sum(1) / mx2, key='maxcos.r')


def test_align_index_refusals(L):
    """T = 33, nf = 9 and nf = T are refused (GENRL_EINVAL) and write nothing"""
    E, N = 64, 2
    x = torch.zeros(40 * N * E, device='cuda')
    for T, nf in ((33, 4), (16, 9), (8, 8)):
        ub, urow = vec_out(40 * N, torch.int64)
        assert L.genrl_align_index(x.data_ptr(), x.data_ptr(), urow.data_ptr(), T, N, E, nf, stream()) == EINVAL
        torch.cuda.synchronize()
        assert (urow == -9).all()


# ====================================================================================== optimiser
NS = [0, 1, 3, 5, 1024, 1025, 8388607, 8388608, 8388609, 33554435]


def flat_buf(src, off):
    """src (CPU fp32 [n]) at `off` floats into a device buffer whose other floats hold PAD"""
    n = src.numel()
    buf = torch.full((n + 8,), PAD, device='cuda')
    view = buf[off:off + n]
    view.copy_(src)
    return buf, view


def flat_untouched(what, buf, view):
    off = view.storage_offset() - buf.storage_offset()
    n = view.numel()
    assert (buf[:off] == PAD).all() and (buf[off + n:] == PAD).all(), f'{what}: a kernel wrote outside its range'


def big_randn(n, seed, scale=1.0):
    return torch.randn(n, generator=gen(seed)) * scale


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_grad_norm(L, n, off):
    """genrl_grad_norm = scale * ||g||_2 against the oracle's global_grad_norm (float64) at views 0..3 floats past 16-byte alignment
    (the scalar path), with n past 1024 workgroups (the grid-stride loop); step_inc goes up by exactly one per call"""
    g = big_randn(n, n + off) * torch.exp(torch.randn(1, generator=gen(n)))
    buf, gv = flat_buf(g, off)
    ws = torch.full((L.genrl_sqnorm_ws_floats(n),), float('nan'), device='cuda')
    step = torch.tensor([41], dtype=torch.int32, device='cuda')
    ref = float(O.global_grad_norm([g.double()]))
    for k, scale in enumerate((1.0, 0.25)):
        ob, out = vec_out(1)
        assert L.genrl_grad_norm(gv.data_ptr(), n, out.data_ptr(), ws.data_ptr(), scale, step.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        vec_untouched('norm', ob, 1)
        within('gnorm', out, torch.tensor([ref * scale], dtype=torch.float64), torch.tensor([ref * scale], dtype=torch.float64))
        assert int(step) == 42 + k
    flat_untouched('g', buf, gv)
    assert torch.equal(gv.cpu(), g)


ADAM_LR, ADAM_EPS = 1e-3, 1e-8
# the betas reach the kernel as fp32: 1 - 0.999f differs from 0.001 by 1.3e-5 relative, 1 - 0.9f from 0.1 by 2.4e-7; the float64
# reference (the oracle, betas 0.9 / 0.999) differs from the kernel's exact arithmetic by that much on the terms those feed
DB1 = abs((1 - f32(0.9)) - 0.1) / 0.1 / 2.0 ** -24
DB2 = abs((1 - f32(0.999)) - 0.001) / 0.001 / 2.0 ** -24


def adam_layouts(n):
    """(offset of p, g, m, v) in floats: aligned, and rotations that put every offset 0..3 on every buffer"""
    rots = [tuple((o + k) % 4 for k in range(4)) for o in range(4)]
    return [(0, 0, 0, 0)] + (rots if n <= 1 << 16 else rots[1:2])


def adam_cases():
    return [(n, lay) for n in NS for lay in adam_layouts(n)]


# (clip relative to the norm: None = off (clip 0), 0.5 = engaged, 10 = not engaged; gscale; wd; step; step on the device; zero_grad)
ADAM_STEPS = [(0.5, 1.0, 0.0, 1, False, True), (10.0, 0.5, 1e-2, 2, True, False), (None, 0.5, 1e-2, 1000, True, True)]


@pytest.mark.parametrize('n,layout', adam_cases())
def test_adam_step(L, n, layout):
    """genrl_grad_norm -> genrl_adam_step over three steps (clip engaged / not engaged / off, gscale 1 / 0.5, wd 0 / 1e-2, steps
    1, 2 and 1000, the step count on the host and on the device), each step against the oracle's optimizer_step from the kernel's
    own fp32 state; zero_grad leaves g exactly 0 inside the range; nothing outside the ranges is written; genrl_scale"""
    gg = gen(n + 17 * sum(layout))
    p0 = torch.randn(n, generator=gg)
    bufs = {k: flat_buf(t, o) for k, t, o in zip('pgmv', (p0, torch.zeros(n), torch.zeros(n), torch.zeros(n)), layout)}
    pv, gv, mv, vv = (bufs[k][1] for k in 'pgmv')
    ws = torch.empty(1024, device='cuda')
    norm = torch.empty(1, device='cuda')
    counter = torch.tensor([0], dtype=torch.int32, device='cuda')
    for clip_rel, gscale, wd, step, on_dev, zero_grad in ADAM_STEPS:
        g = torch.randn(n, generator=gg) * 0.3
        gv.copy_(g)
        if step == 1000:
            counter.fill_(999)
        p, m, v = pv.cpu(), mv.cpu(), vv.cpu()              # the kernel's own state before this step
        assert L.genrl_grad_norm(gv.data_ptr(), n, norm.data_ptr(), ws.data_ptr(), gscale, counter.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert int(counter) == step
        ref_norm = float(O.global_grad_norm([g.double() * gscale])) if n else 0.0
        clip = 0.0 if clip_rel is None else f32(clip_rel * ref_norm)
        assert L.genrl_adam_step(pv.data_ptr(), gv.data_ptr(), mv.data_ptr(), vv.data_ptr(), n, norm.data_ptr(), gscale, clip, ADAM_LR,
                                 0.9, 0.999, ADAM_EPS, wd, 0 if on_dev else step, counter.data_ptr() if on_dev else None, int(zero_grad),
                                 stream()) == 0
        torch.cuda.synchronize()
        for k in 'pgmv':
            flat_untouched(k, *bufs[k])
        if n == 0:
            continue
        params = {'w': p.double()}
        state = {'w': (step - 1, m.double(), v.double())}
        O.optimizer_step(params, {'w': g.double() * gscale}, state, f32(ADAM_LR), f32(ADAM_EPS), math.inf if clip == 0.0 else clip, f32(wd))
        _, mr, vr = state['w']
        # magnitudes: coef from the fp32 norm, the update's terms, the betas' fp32 rounding (DB1, DB2)
        gc = (g.double() * gscale).abs() * (1.0 if clip == 0.0 else min(clip / (ref_norm + 1e-6), 1.0))
        sm = 0.9 * m.double().abs() + 0.1 * gc * (1 + DB1)
        sv = 0.999 * v.double() + 0.001 * gc * gc * (1 + DB2)
        bc1 = 1 - 0.9 ** step
        upd = (ADAM_LR / bc1) * sm / (vr.sqrt() / math.sqrt(1 - 0.999 ** step) + ADAM_EPS)
        within('adam.m', mv, mr, sm + 1e-300)
        within('adam.v', vv, vr, sv + 1e-300)
        within('adam.p', pv, params['w'], (1 - wd) * p.double().abs() + upd * (4 + DB1 + DB2))
        if zero_grad:
            assert (gv == 0).all()
        else:
            assert torch.equal(gv.cpu(), g)
    s = f32(0.37)
    before = pv.cpu()
    assert L.genrl_scale(pv.data_ptr(), n, s, stream()) == 0
    torch.cuda.synchronize()
    flat_untouched('p', *bufs['p'])
    within('scale', pv, before.double() * s, (before.double() * s).abs())


@pytest.mark.parametrize('n', [5, 1025, 8388609])
def test_adam_device_step_equals_host_step(L, n):
    """the step count read from the device (graph replay) gives bit-identical parameters and moments to the same step given on
    the host, at steps 1, 2 and 1000"""
    gg = gen(n)
    p0, g = torch.randn(n, generator=gg), torch.randn(n, generator=gg)
    norm = torch.tensor([float(g.norm())], device='cuda')
    for step in (1, 2, 1000):
        outs = []
        for on_dev in (False, True):
            p, gd, m, v = p0.cuda(), g.cuda(), torch.full((n,), 1e-3, device='cuda'), torch.full((n,), 1e-4, device='cuda')
            counter = torch.tensor([step], dtype=torch.int32, device='cuda')
            assert L.genrl_adam_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, norm.data_ptr(), 1.0, 1.0, ADAM_LR, 0.9,
                                     0.999, ADAM_EPS, 1e-2, 0 if on_dev else step, counter.data_ptr() if on_dev else None, 0,
                                     stream()) == 0
            torch.cuda.synchronize()
            outs.append((p, m, v))
        for a, b in zip(*outs):
            assert torch.equal(a, b), step
