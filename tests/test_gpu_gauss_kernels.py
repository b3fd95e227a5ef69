"""The continuous-latent kernels (csrc/gaussian.hip) through their C entry points, under the convention of test_gpu_discrete_kernels.py:
error against float64, bounded per case by 2x the error the float32 CPU restatement (tests/gauss_restatement.py, plain torch) makes against
float64 on the same inputs, with a floor of 4 units of 2^-24 x scale.  The factor 2 covers a different evaluation order; the yardstick is the
restatement, never the kernel.  Outputs are NaN-prefilled inside PAD-filled buffers with a guard row (and padding columns where the output is
pitched): nothing may be written outside.

Scales.  mean is a copy: exact.  std: its elementwise magnitude.  stoch = mean + std eps: the elementwise magnitude |mean| + |std eps| of its
two terms (where they cancel the rounding error follows the terms, not what is left of them -- the rule the KL row states below).  A KL row:
the sum over S of the magnitudes of its four terms, 0.5 (v + t + 1 + |log v|).  Entropies: max(|result|, 1) per row.  Gradients: the magnitude
of the terms each element is summed from (gauss_restatement.head_bwd / kl_bwd return them).

Shapes: R in {1, 5, 257} (one row, a few, more than one workgroup of KL groups), S in {1, 3, 30, 32, 33, 64, 200} (below a lane group, the
reference's 30 whose std half is 8-byte aligned only, a whole group, one past, a whole wave, several strides), plus S past one sweep of the
head's workgroup; raw / draw pitches 2S, 2S + 4 (16-byte accesses stay possible) and 2S + 3 (they do not), and a pointer that is only 4-byte
aligned.  Input kinds: moderate, wide (raw x 8: softplus crosses its threshold 20, the sigmoids saturate), strongly negative raw (std collapses
to min_std), equal distributions and means 10 apart at min_std for the KL."""
import math

import pytest
import torch

import gauss_restatement as R
from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

RS, SS = [1, 5, 257], [1, 3, 30, 32, 33, 64, 200]
ACTS = {'softplus': 0, 'sigmoid': 1, 'sigmoid2': 2}
MIN_STD = 0.1
K = {}
RATIOS = {}
within = checker(K, RATIOS)
FLOOR, FACTOR = 4.0, 2.0


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\ngauss kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


def vec_out(n):
    buf = torch.full((n + 4,), PAD, device='cuda')
    buf[:n] = float('nan')
    return buf, buf[:n]


def vec_untouched(what, buf, n):
    assert torch.equal(buf[n:], torch.full_like(buf[n:], PAD)), f'{what}: wrote past its output'


def bounded(what, got, ref64, rest32, scale):
    key = what.split('[')[0]
    live = scale > 0
    rest = float(((rest32.double() - ref64).abs()[live] / (U * scale[live])).max()) if bool(live.any()) else 0.0
    K[key] = max(FACTOR * rest, FLOOR)
    print(f'{what}: restatement ratio {rest:.3g}, bound {K[key]:.3g}', end='; ')
    within(what, got, ref64, scale)
    print(f'worst kernel ratio so far {RATIOS[key]:.3g}')


def ptr(t):
    return t.data_ptr() if t is not None else None


def pitch_of(S, pitch):
    return 2 * S + {'tight': 0, 'pad4': 4, 'pad3': 3}[pitch]


def make_raw(Rn, S, kind, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(Rn, 2 * S, generator=g)
    if kind == 'wide':
        raw = raw * 8
    elif kind == 'negative':
        raw[:, S:] = raw[:, S:] - 30.0
    rn = lambda: torch.randn(Rn, S, generator=g)
    return raw, rn(), rn(), rn(), rn()         # raw, eps, dstoch, dmean, dstd


def run_head(L, Rn, S, pitch, act, kind, off=0):
    from genrl_amd._lib import check
    raw, eps, gs, gm, gd = make_raw(Rn, S, kind, 11 + Rn + 1000 * S)
    code = ACTS[act]
    ld = pitch_of(S, pitch)
    rawd = in_buf(raw, ld, off)
    epsd, gsd, gmd, gdd = eps.cuda(), gs.cuda(), gm.cuda(), gd.cuda()
    tag = f'[{Rn}x{S},{pitch},{act},{kind},off{off}]'
    keep = {}
    for has_eps in (True, False):
        m64, s64, z64 = R.head(raw.double(), eps.double() if has_eps else None, act, MIN_STD)
        m32, s32, z32 = R.head(raw, eps if has_eps else None, act, MIN_STD)
        bufs = [out_buf(Rn, S, S) for _ in range(3)]
        check(L.genrl_gauss_head_fwd(rawd.data_ptr(), ld, ptr(epsd) if has_eps else None, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(),
                                     bufs[2][1].data_ptr(), Rn, S, code, MIN_STD, stream()), 'gauss_head_fwd')
        for (b, v), name in zip(bufs, ('mean', 'std', 'stoch')):
            untouched(name + tag, b, v)
        mean, std, stoch = (v for _, v in bufs)
        assert torch.equal(mean.cpu(), raw[:, :S]), 'mean is a copy'
        bounded('std.fwd' + tag, std, s64, s32, s64.abs())
        if has_eps:
            bounded('stoch.fwd' + tag, stoch, z64, z32, m64.abs() + (s64 * eps.double()).abs())
        else:
            assert torch.equal(stoch, mean), 'mean form: stoch = mean'
        assert float(std.min()) >= MIN_STD
        keep[has_eps] = (std.clone(), stoch.clone())
    # every output alone (the others NULL)
    for i, name in enumerate(('mean', 'std', 'stoch')):
        b, v = out_buf(Rn, S, S)
        args = [None, None, None]
        args[i] = v.data_ptr()
        check(L.genrl_gauss_head_fwd(rawd.data_ptr(), ld, epsd.data_ptr(), *args, Rn, S, code, MIN_STD, stream()), 'gauss_head_fwd')
        untouched(name + ' alone' + tag, b, v)
        assert torch.equal(v, (raw[:, :S].cuda(), *keep[True])[i]), name + ' alone'
    # backward: every combination of upstream gradients (at least one), with and without eps; then accumulation
    lddr = pitch_of(S, pitch)
    for has_eps in (True, False):
        for mask in range(1, 8):
            a = [t if mask >> i & 1 else None for i, t in enumerate((gs, gm, gd))]
            ad = [t if mask >> i & 1 else None for i, t in enumerate((gsd, gmd, gdd))]
            d64, scale = R.head_bwd(*[None if t is None else t.double() for t in a], raw.double(), eps.double() if has_eps else None, act)
            d32, _ = R.head_bwd(*a, raw, eps if has_eps else None, act)
            dbuf, d = out_buf(Rn, 2 * S, lddr, off)
            check(L.genrl_gauss_head_bwd(ptr(ad[0]), ptr(ad[1]), ptr(ad[2]), rawd.data_ptr(), ld, ptr(epsd) if has_eps else None,
                                         d.data_ptr(), lddr, Rn, S, code, 0, stream()), 'gauss_head_bwd')
            untouched('draw' + tag, dbuf, d)
            bounded(f'draw.{"eps" if has_eps else "mean"}' + tag, d, d64, d32, scale)
    base = torch.randn(Rn, 2 * S, generator=torch.Generator().manual_seed(3))
    dbuf, d = out_buf(Rn, 2 * S, lddr, off)
    d.copy_(base)
    check(L.genrl_gauss_head_bwd(gsd.data_ptr(), gmd.data_ptr(), gdd.data_ptr(), rawd.data_ptr(), ld, epsd.data_ptr(), d.data_ptr(), lddr,
                                 Rn, S, code, 1, stream()), 'gauss_head_bwd')
    untouched('draw (accumulate)' + tag, dbuf, d)
    d64, scale = R.head_bwd(gs.double(), gm.double(), gd.double(), raw.double(), eps.double(), act)
    d32, _ = R.head_bwd(gs, gm, gd, raw, eps, act)
    bounded('draw.acc' + tag, d, base.double() + d64, base + d32, base.double().abs() + scale)


@pytest.mark.parametrize('pitch', ['tight', 'pad4', 'pad3'])
@pytest.mark.parametrize('S', SS)
@pytest.mark.parametrize('Rn', RS)
def test_head_vs_float64(L, Rn, S, pitch):
    for i, act in enumerate(ACTS):
        for kind in ('moderate', 'wide', 'negative'):
            run_head(L, Rn, S, pitch, act, kind)


@pytest.mark.parametrize('S', [32, 1028, 1030])
def test_head_unaligned_pointer_and_more_than_one_sweep(L, S):
    """a raw / draw pointer that is only 4-byte aligned takes the scalar path whatever S is; S past 4 x 256 (16-byte accesses) or 256 (scalar)
    needs more than one sweep of the workgroup"""
    for off in (0, 1):
        run_head(L, 5, S, 'tight', 'softplus', 'wide', off)


def test_head_limits(L):
    """wide inputs cross softplus's threshold 20 on both sides of it; strongly negative raw leaves std = min_std up to rounding"""
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0, 19.5, 20.0, 20.5, 90.0]])
    outs = [out_buf(1, 4, 4) for _ in range(3)]
    assert L.genrl_gauss_head_fwd(x.cuda().data_ptr(), 8, None, *[v.data_ptr() for _, v in outs], 1, 4, 0, MIN_STD, stream()) == 0
    ref = R.head(x.double(), None, 'softplus', MIN_STD)[1]
    assert float(((outs[1][1].cpu().double() - ref).abs() / ref).max()) <= 4 * U
    for act, code in ACTS.items():
        x = torch.cat([torch.zeros(3, 5), torch.full((3, 5), -40.0)], 1)
        outs = [out_buf(3, 5, 5) for _ in range(3)]
        assert L.genrl_gauss_head_fwd(x.cuda().data_ptr(), 10, None, *[v.data_ptr() for _, v in outs], 3, 5, code, MIN_STD, stream()) == 0
        assert float((outs[1][1] - MIN_STD).abs().max()) <= 2 * U * MIN_STD + 1e-16, act


def test_head_rejects_unsupported_arguments(L):
    x = torch.zeros(4, 16, device='cuda')
    e = torch.zeros(4, 8, device='cuda')
    bufs = [out_buf(4, 8, 8) for _ in range(3)]
    o = [v.data_ptr() for _, v in bufs]
    dbuf, d = out_buf(4, 16, 16)
    st = stream()
    assert L.genrl_gauss_head_fwd(x.data_ptr(), 16, e.data_ptr(), *o, 4, 0, 0, MIN_STD, st) == 1           # S < 1
    assert L.genrl_gauss_head_fwd(x.data_ptr(), 15, e.data_ptr(), *o, 4, 8, 0, MIN_STD, st) == 1           # pitch below 2S
    assert L.genrl_gauss_head_fwd(x.data_ptr(), 16, e.data_ptr(), *o, 4, 8, 3, MIN_STD, st) == 1           # unknown std_act
    assert L.genrl_gauss_head_fwd(x.data_ptr(), 16, e.data_ptr(), None, None, None, 4, 8, 0, MIN_STD, st) == 1   # no output
    assert L.genrl_gauss_head_fwd(None, 16, e.data_ptr(), *o, 4, 8, 0, MIN_STD, st) == 1
    assert L.genrl_gauss_head_bwd(None, None, None, x.data_ptr(), 16, e.data_ptr(), d.data_ptr(), 16, 4, 8, 0, 0, st) == 1
    assert L.genrl_gauss_head_bwd(e.data_ptr(), None, None, x.data_ptr(), 16, e.data_ptr(), d.data_ptr(), 15, 4, 8, 0, 0, st) == 1
    assert L.genrl_gauss_head_bwd(e.data_ptr(), None, None, x.data_ptr(), 16, e.data_ptr(), d.data_ptr(), 16, 4, 8, -1, 0, st) == 1
    assert L.genrl_gauss_head_bwd(e.data_ptr(), None, None, x.data_ptr(), 16, e.data_ptr(), None, 16, 4, 8, 0, 0, st) == 1
    assert L.genrl_gauss_head_fwd(x.data_ptr(), 16, e.data_ptr(), *o, 0, 8, 0, MIN_STD, st) == 0            # no rows: nothing to do
    torch.cuda.synchronize()
    for b, v in bufs + [(dbuf, d)]:
        assert bool(torch.isnan(v).all())
        untouched('rejected call', b, v)


# ---------------------------------------------------------------------------------------------------------------- KL

def make_kl(Rn, S, kind, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(Rn, S, generator=g)
    sp = torch.nn.functional.softplus
    if kind == 'wide':
        ml, mr, sl, sr = 8 * rn(), 8 * rn(), MIN_STD + sp(8 * rn()), MIN_STD + sp(8 * rn())
    elif kind == 'negative':
        ml, mr, sl, sr = rn(), rn(), MIN_STD + sp(rn() - 30), MIN_STD + sp(rn() - 30)
    elif kind == 'apart':
        ml = rn()
        mr, sl, sr = ml + 10.0, torch.full((Rn, S), MIN_STD), torch.full((Rn, S), MIN_STD)
    else:
        ml, mr, sl, sr = rn(), rn(), MIN_STD + sp(rn()), MIN_STD + sp(rn())
        if kind == 'equal':
            mr, sr = ml.clone(), sl.clone()
    return ml, sl, mr, sr, torch.randn(Rn, generator=g), torch.randn(Rn, generator=g)


def run_kl(L, Rn, S, kind):
    from genrl_amd._lib import check
    ml, sl, mr, sr, gp, gq = make_kl(Rn, S, kind, 23 + Rn + 1000 * S)
    D = [t.double() for t in (ml, sl, mr, sr)]
    dev = [t.cuda() for t in (ml, sl, mr, sr)]
    p = [t.data_ptr() for t in dev]
    tag = f'[{Rn}x{S},{kind}]'
    kl64, scale = R.kl(*D)
    kl32, _ = R.kl(ml, sl, mr, sr)
    el64, er64, el32, er32 = R.entropy(D[1]), R.entropy(D[3]), R.entropy(sl), R.entropy(sr)
    one = lambda r: r.abs().clamp_min(1.0)
    first = None
    for want in ((1, 1, 1), (1, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        outs = [vec_out(Rn) for _ in range(3)]
        o = [v.data_ptr() if w else None for (_, v), w in zip(outs, want)]
        means = (p[0], p[2]) if want[0] else (None, None)          # (without kl the means are not read)
        check(L.genrl_gauss_kl_fwd(means[0], p[1] if (want[0] or want[1]) else None, means[1], p[3] if (want[0] or want[2]) else None, *o,
                                   Rn, S, stream()), 'gauss_kl_fwd')
        for (b, v), w, name in zip(outs, want, ('kl', 'ent_l', 'ent_r')):
            vec_untouched(name + tag, b, Rn)
            if not w:
                assert bool(torch.isnan(v).all()), name + ' was not asked for'
        if want[0]:
            bounded('kl.fwd' + tag, outs[0][1], kl64, kl32, scale)
        if want[1]:
            bounded('ent.fwd' + tag, outs[1][1], el64, el32, one(el64))
        if want[2]:
            bounded('ent.fwd' + tag, outs[2][1], er64, er32, one(er64))
        if want == (1, 1, 1):
            if first is None:
                first = [v.clone() for _, v in outs]
            else:               # the same call again: bit-identical
                assert all(torch.equal(a, v) for a, (_, v) in zip(first, outs)), 'repeat run differs'
    if kind == 'equal':         # the float64 value, 0, on the term scale
        assert float(kl64.abs().max()) == 0.0 and bool((first[0].cpu().double().abs() <= K['kl.fwd'] * U * scale).all())
    g64, gscale = R.kl_bwd(*D, gp.double(), gq.double())
    g32, _ = R.kl_bwd(ml, sl, mr, sr, gp, gq)
    gpd, gqd = gp.cuda(), gq.cuda()
    names = ('dmean_l', 'dstd_l', 'dmean_r', 'dstd_r')
    prev = None
    for mask in (15, 3, 12, 1, 2, 4, 8, 5, 10, 15):
        outs = [out_buf(Rn, S, S) for _ in range(4)]
        o = [v.data_ptr() if mask >> i & 1 else None for i, (_, v) in enumerate(outs)]
        check(L.genrl_gauss_kl_bwd(*p, gpd.data_ptr() if mask & 3 else None, gqd.data_ptr() if mask & 12 else None, *o, Rn, S, stream()),
              'gauss_kl_bwd')
        for i, (b, v) in enumerate(outs):
            untouched(names[i] + tag, b, v)
            if mask >> i & 1:
                bounded(f'{names[i]}.bwd' + tag, v, g64[i].expand_as(D[0]), g32[i].expand_as(ml), gscale[i].expand_as(D[0]))
            else:
                assert bool(torch.isnan(v).all())
        if mask == 15:
            if prev is None:
                prev = [v.clone() for _, v in outs]
            else:
                assert all(torch.equal(a, v) for a, (_, v) in zip(prev, outs)), 'repeat run differs'


@pytest.mark.parametrize('S', SS)
@pytest.mark.parametrize('Rn', RS)
def test_kl_vs_float64(L, Rn, S):
    for kind in ('moderate', 'wide', 'negative', 'equal', 'apart'):
        run_kl(L, Rn, S, kind)


def test_kl_largest_supported_width_and_means_apart(L):
    run_kl(L, 5, 1024, 'moderate')
    run_kl(L, 3, 1000, 'apart')
    # means 10 apart at std 0.1: t = 10^4 per latent, v = 1
    ml, sl, mr, sr, _, _ = make_kl(3, 1000, 'apart', 23 + 3 + 1000 * 1000)
    want = R.kl(ml.double(), sl.double(), mr.double(), sr.double())[0]
    assert float((want / (1000 * 0.5 * 1e4) - 1).abs().max()) < 1e-5


def test_kl_rejects_unsupported_arguments(L):
    x = torch.ones(4, 8, device='cuda')
    g = torch.ones(4, device='cuda')
    bk, k = vec_out(4)
    bufs = [out_buf(4, 8, 8) for _ in range(4)]
    o = [v.data_ptr() for _, v in bufs]
    p, st = x.data_ptr(), stream()
    assert L.genrl_gauss_kl_fwd(p, p, p, p, k.data_ptr(), None, None, 4, 0, st) == 1
    assert L.genrl_gauss_kl_fwd(p, p, p, p, None, None, None, 4, 8, st) == 1
    assert L.genrl_gauss_kl_fwd(None, p, p, p, k.data_ptr(), None, None, 4, 8, st) == 1
    assert L.genrl_gauss_kl_fwd(None, None, None, p, None, k.data_ptr(), None, 4, 8, st) == 1      # ent_l without std_l
    assert L.genrl_gauss_kl_bwd(p, p, p, p, g.data_ptr(), g.data_ptr(), None, None, None, None, 4, 8, st) == 1
    assert L.genrl_gauss_kl_bwd(p, p, p, p, None, g.data_ptr(), *o, 4, 8, st) == 1                 # a left output without gp
    assert L.genrl_gauss_kl_bwd(p, p, p, None, g.data_ptr(), g.data_ptr(), *o, 4, 8, st) == 1
    assert L.genrl_gauss_kl_bwd(p, p, p, p, g.data_ptr(), g.data_ptr(), *o, 4, 0, st) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(k).all())
    vec_untouched('kl', bk, 4)
    for b, v in bufs:
        assert bool(torch.isnan(v).all())
        untouched('rejected call', b, v)


# ---------------------------------------------------------------------------------------------------------------- op layer

def test_ops_gradients_match_float64_autograd():
    """ops.gauss_head and ops.gauss_kl_balance end to end (head -> KL with rows on both sides of the free nats -> loss) against float64
    autograd of the restatement; raw arrives as a column slice of a padded buffer, the states as (B, T, S) views of time-major storage"""
    from genrl_amd import ops
    T_, B_, S = 7, 3, 30
    g = torch.Generator().manual_seed(5)
    raws = [torch.randn(T_, B_, 2 * S, generator=g) for _ in range(2)]
    epss = [torch.randn(T_, B_, S, generator=g) for _ in range(2)]
    mix, free = 0.8, 130.0

    def run(dtype, dev):
        leaves, stats = [], []
        for raw, eps in zip(raws, epss):
            x = raw.to(dtype=dtype, device=dev)
            if dev == 'cuda':           # a column slice of rows padded to 64 floats
                pad = torch.zeros(T_, B_, 64, device=dev)
                pad[..., :2 * S] = x
                x = pad
            x.requires_grad_(True)
            leaves.append(x)
            v = x[..., :2 * S]
            if dev == 'cuda':
                mean, std, stoch = ops.gauss_head(v, eps.cuda(), 'softplus', MIN_STD)
            else:
                mean, std, stoch = R.head(v, eps.to(dtype), 'softplus', MIN_STD)
            stats.append({k: t.transpose(0, 1) for k, t in dict(mean=mean, std=std, stoch=stoch).items()})       # (B, T, S) views
        post, prior = stats
        if dev == 'cuda':
            loss, value = ops.gauss_kl_balance(post['mean'], post['std'], prior['mean'], prior['std'], 1 - mix, free)
            ent = ops.gauss_entropy(post['std'])
        else:
            sg = lambda d: {k: t.detach() for k, t in d.items()}
            vl = R.kl(post['mean'], post['std'], sg(prior)['mean'], sg(prior)['std'])[0]
            vr = R.kl(sg(post)['mean'], sg(post)['std'], prior['mean'], prior['std'])[0]
            loss = (1 - mix) * torch.clamp(vl, min=free).mean() + mix * torch.clamp(vr, min=free).mean()
            value, ent = vl.detach(), R.entropy(post['std'].detach())
        total = loss + 0.01 * (post['stoch'] * post['stoch']).sum() + 0.02 * prior['stoch'].sum()
        total.backward()
        return loss.detach(), value, ent, [x.grad[..., :2 * S] for x in leaves]
    l64, v64, e64, g64 = run(torch.float64, 'cpu')
    l, v, e, gr = run(torch.float32, 'cuda')
    assert v.shape == (B_, T_) and e.shape == (B_, T_)
    assert bool((v64 < free).any()) and bool((v64 > free).any())
    close = lambda a, b, what: torch.testing.assert_close(a.cpu().double(), b, rtol=2e-5, atol=2e-6, msg=lambda m: what + ': ' + m)
    close(l, l64, 'loss'); close(v, v64, 'per-row KL'); close(e, e64, 'entropy')
    for a, b, what in zip(gr, g64, ('d raw (posterior)', 'd raw (prior)')):
        close(a, b, what)
