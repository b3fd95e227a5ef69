"""The squashed-Gaussian head kernels (csrc/heads.hip) through their C entry points, under the convention of test_gpu_gauss_kernels.py:
error against float64, bounded per case by 2x the error the float32 CPU restatement (tests/tanh_restatement.py, plain torch) makes against
float64 on the same inputs, with a floor of 4 units of 2^-24 x scale.  The factor 2 covers a different evaluation order; the yardstick is the
restatement, never the kernel.  Outputs are NaN-prefilled inside PAD-filled buffers with a guard row (and padding columns where the output is
pitched): nothing may be written outside.

Scales (tanh_restatement.py states them next to the formulas).  mean, std: their elementwise magnitude.  A tanh(x), x = mean + std eps: its
own magnitude plus (1 - tanh^2) (|mean| + |std eps|): where the two terms of x cancel, the rounding error follows the terms, not what is
left of them; the Monte-Carlo mean takes the mean of that over the samples.  An entropy: the mean over the samples, summed over the action
dimensions, of the magnitudes of its terms eps^2 / 2, |log std|, log(2 pi) / 2, 2 log 2, 2 (|mean| + |std eps|), 2 softplus(-2x).  Gradients:
the magnitude of the terms each element is summed from, with 1 - tanh^2 counted as 1 + tanh^2.

Shapes: R in {1, 3, 37, 300} (one row, a few, an odd count, more than one workgroup at every group width) x A in {1, 2, 5, 6, 17, 64} (below
the smallest group, inside it, the reference's 6, one past a group of 16, a whole wave) x K in {1, 3, 100} (one sample, less than one unrolled
sweep, SampleDist's own).  Input kinds: moderate, and wide (raw x 6: the softplus crosses its threshold 20, 5 tanh(out / 5) saturates, x
reaches past -10 where softplus(-2x) is the identity)."""
import pytest
import torch

import tanh_restatement as R
from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

RS, AS, KS = [1, 3, 37, 300], [1, 2, 5, 6, 17, 64], [1, 3, 100]
MIN_STD, INIT_STD = 0.1, 1.0
BOUND = {}
RATIOS, REST = {}, {}
within = checker(BOUND, RATIOS)
FLOOR, FACTOR = 4.0, 2.0


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\ntanh_normal kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})
    print('the float32 restatement on the same inputs:', {k: round(v, 3) for k, v in sorted(REST.items())})


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
    REST[key] = max(REST.get(key, 0.0), rest)
    BOUND[key] = max(FACTOR * rest, FLOOR)
    print(f'{what}: restatement ratio {rest:.3g}, bound {BOUND[key]:.3g}', end='; ')
    within(what, got, ref64, scale)
    print(f'worst kernel ratio so far {RATIOS[key]:.3g}')


def make(Rn, A, Kn, kind, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(Rn, 2 * A, generator=g) * (6.0 if kind == 'wide' else 1.0)
    return raw, torch.randn(Rn, A, generator=g), torch.randn(Kn, Rn, A, generator=g), torch.randn(Rn, A, generator=g), torch.randn(Rn, generator=g)


P = (MIN_STD, INIT_STD)
D = lambda *ts: [t.double() for t in ts]


def run_head(L, Rn, A, kind):
    from genrl_amd._lib import check
    raw, eps, _, g, _ = make(Rn, A, 1, kind, 7 + Rn + 1000 * A)
    rawd, epsd = raw.cuda(), eps.cuda()
    tag = f'[{Rn}x{A},{kind}]'
    a64, _, m64, s64 = R.sample(*D(raw, eps), *P)
    a32, _, m32, s32 = R.sample(raw, eps, *P)
    keep = None
    for ld in (A, A + 3):                  # action rows tight and padded
        (ab, a), (mb, m), (sb, s) = out_buf(Rn, A, ld), out_buf(Rn, A, A), out_buf(Rn, A, A)
        check(L.genrl_tanh_normal_head_fwd(rawd.data_ptr(), epsd.data_ptr(), a.data_ptr(), m.data_ptr(), s.data_ptr(), Rn, A, *P,
                                           0 if ld == A else ld, stream()), 'tanh_normal_head_fwd')
        for name, b, v in (('action', ab, a), ('mean', mb, m), ('std', sb, s)):
            untouched(name + tag, b, v)
        bounded('head.mean' + tag, m, m64, m32, m64.abs())
        bounded('head.std' + tag, s, s64, s32, s64.abs())
        bounded('head.action' + tag, a, a64, a32, R.tanh_scale(*D(raw, eps), *P))
        assert float(s.min()) >= MIN_STD and float(a.abs().max()) <= 1.0 and float(m.abs().max()) <= 5.0
        if keep is None:
            keep = [v.clone() for v in (a, m, s)]
        else:
            assert all(torch.equal(k_, v) for k_, v in zip(keep, (a, m, s))), 'the action pitch changed a value'
    for i, name in enumerate(('action', 'mean', 'std')):          # every output alone (the others NULL)
        b, v = out_buf(Rn, A, A)
        args = [None, None, None]
        args[i] = v.data_ptr()
        check(L.genrl_tanh_normal_head_fwd(rawd.data_ptr(), epsd.data_ptr(), *args, Rn, A, *P, 0, stream()), 'tanh_normal_head_fwd')
        untouched(name + ' alone' + tag, b, v)
        assert torch.equal(v, keep[i]), name + ' alone'
    # the mean form: eps NULL, action = tanh(mean)
    b, v = out_buf(Rn, A, A)
    check(L.genrl_tanh_normal_head_fwd(rawd.data_ptr(), None, v.data_ptr(), None, None, Rn, A, *P, 0, stream()), 'tanh_normal_head_fwd')
    untouched('mean form' + tag, b, v)
    zero = torch.zeros_like(eps)
    bounded('head.action' + tag, v, R.sample(*D(raw, zero), *P)[0], R.sample(raw, zero, *P)[0], R.tanh_scale(*D(raw, zero), *P))
    # backward, daction tight and padded
    d64, scale = R.sample_bwd(*D(g, raw, eps), *P)
    d32, _ = R.sample_bwd(g, raw, eps, *P)
    first = None
    for ld in (A, A + 3):
        gd = in_buf(g, ld)
        db, d = out_buf(Rn, 2 * A, 2 * A)
        check(L.genrl_tanh_normal_head_bwd(gd.data_ptr(), rawd.data_ptr(), epsd.data_ptr(), d.data_ptr(), Rn, A, *P, 0 if ld == A else ld,
                                           stream()), 'tanh_normal_head_bwd')
        untouched('draw' + tag, db, d)
        bounded('head.draw' + tag, d, d64, d32, scale)
        first = d.clone() if first is None else first
        assert torch.equal(first, d), 'the daction pitch changed a value'


def run_mc(L, Rn, A, Kn, kind):
    from genrl_amd._lib import check
    raw, _, eps, _, g = make(Rn, A, Kn, kind, 13 + Rn + 1000 * A + 7 * Kn)
    rawd, epsd, gd = raw.cuda(), eps.cuda(), g.cuda()
    tag = f'[{Rn}x{A}x{Kn},{kind}]'
    e64, e32 = R.entropy(*D(raw, eps), *P), R.entropy(raw, eps, *P)
    m64, m32 = R.mc_mean(*D(raw, eps), *P), R.mc_mean(raw, eps, *P)
    escale, mscale = R.entropy_scale(*D(raw, eps), *P), R.tanh_scale(*D(raw, eps), *P).mean(0)
    keep = None
    for want in ((1, 1), (1, 0), (0, 1), (1, 1)):
        (eb, e), (mb, m) = vec_out(Rn), out_buf(Rn, A, A)
        check(L.genrl_tanh_normal_mc_fwd(rawd.data_ptr(), epsd.data_ptr(), e.data_ptr() if want[0] else None, m.data_ptr() if want[1] else None,
                                         Rn, A, Kn, *P, stream()), 'tanh_normal_mc_fwd')
        vec_untouched('ent' + tag, eb, Rn); untouched('mean_action' + tag, mb, m)
        if want[0]:
            bounded('mc.ent' + tag, e, e64, e32, escale)
        else:
            assert bool(torch.isnan(e).all()), 'ent was not asked for'
        if want[1]:
            bounded('mc.mean' + tag, m, m64, m32, mscale)
            assert float(m.abs().max()) <= 1.0
        else:
            assert bool(torch.isnan(m).all()), 'mean_action was not asked for'
        if want == (1, 1):
            if keep is None:
                keep = (e.clone(), m.clone())
            else:               # the same call again: bit-identical
                assert torch.equal(keep[0], e) and torch.equal(keep[1], m), 'repeat run differs'
        elif want[0]:
            assert torch.equal(keep[0], e), 'ent alone differs'
        else:
            assert torch.equal(keep[1], m), 'mean_action alone differs'
    d64, scale = R.entropy_bwd(*D(g, raw, eps), *P)
    d32, _ = R.entropy_bwd(g, raw, eps, *P)
    first = None
    for _ in range(2):
        db, d = out_buf(Rn, 2 * A, 2 * A)
        check(L.genrl_tanh_normal_ent_bwd(gd.data_ptr(), rawd.data_ptr(), epsd.data_ptr(), d.data_ptr(), Rn, A, Kn, *P, 0, stream()),
              'tanh_normal_ent_bwd')
        untouched('draw' + tag, db, d)
        bounded('mc.draw' + tag, d, d64, d32, scale)
        first = d.clone() if first is None else first
        assert torch.equal(first, d), 'repeat run differs'
    base = torch.randn(Rn, 2 * A, generator=torch.Generator().manual_seed(3))
    db, d = out_buf(Rn, 2 * A, 2 * A)
    d.copy_(base)
    check(L.genrl_tanh_normal_ent_bwd(gd.data_ptr(), rawd.data_ptr(), epsd.data_ptr(), d.data_ptr(), Rn, A, Kn, *P, 1, stream()),
          'tanh_normal_ent_bwd')
    untouched('draw (accumulate)' + tag, db, d)
    bounded('mc.draw_acc' + tag, d, base.double() + d64, base + d32, base.double().abs() + scale)


@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('Rn', RS)
def test_head_vs_float64(L, Rn, A):
    for kind in ('moderate', 'wide'):
        run_head(L, Rn, A, kind)


@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('Rn', RS)
def test_mc_vs_float64(L, Rn, A):
    for Kn in KS:
        for kind in ('moderate', 'wide'):
            run_mc(L, Rn, A, Kn, kind)


def test_limit_inputs_stay_finite(L):
    """out = +-50 (5 tanh saturates), std_raw = 25 (above the softplus threshold) or -30 (std collapses to min_std), eps = +-6: x reaches
    +-190, far past -10 where softplus(-2x) takes its identity branch.  Every output of the four kernels is finite."""
    from genrl_amd._lib import check
    A, Kn = 4, 3
    rows = [[o] * A + [s] * A for o in (50.0, -50.0) for s in (25.0, -30.0)]
    raw = torch.tensor(rows)
    Rn = raw.shape[0]
    for sign in (6.0, -6.0):
        eps = torch.full((Kn, Rn, A), sign)
        eps[1] = -sign
        rawd, epsd = raw.cuda(), eps.cuda()
        one = torch.ones(Rn, A, device='cuda')
        (ab, a), (mb, m), (sb, s), (db, d) = out_buf(Rn, A, A), out_buf(Rn, A, A), out_buf(Rn, A, A), out_buf(Rn, 2 * A, 2 * A)
        check(L.genrl_tanh_normal_head_fwd(rawd.data_ptr(), epsd.data_ptr(), a.data_ptr(), m.data_ptr(), s.data_ptr(), Rn, A, MIN_STD, 0.0, 0,
                                           stream()), 'tanh_normal_head_fwd')
        check(L.genrl_tanh_normal_head_bwd(one.data_ptr(), rawd.data_ptr(), epsd.data_ptr(), d.data_ptr(), Rn, A, MIN_STD, 0.0, 0, stream()),
              'tanh_normal_head_bwd')
        (eb, e), (qb, q), (gb, gr) = vec_out(Rn), out_buf(Rn, A, A), out_buf(Rn, 2 * A, 2 * A)
        check(L.genrl_tanh_normal_mc_fwd(rawd.data_ptr(), epsd.data_ptr(), e.data_ptr(), q.data_ptr(), Rn, A, Kn, MIN_STD, 0.0, stream()),
              'tanh_normal_mc_fwd')
        check(L.genrl_tanh_normal_ent_bwd(one.data_ptr(), rawd.data_ptr(), epsd.data_ptr(), gr.data_ptr(), Rn, A, Kn, MIN_STD, 0.0, 0,
                                          stream()), 'tanh_normal_ent_bwd')
        for name, v in (('action', a), ('mean', m), ('std', s), ('draw', d), ('ent', e), ('mean_action', q), ('d ent', gr)):
            assert bool(torch.isfinite(v).all()), (name, sign, v)
        x = R.sample(raw.double(), eps.double(), MIN_STD, 0.0)[1]
        assert float(x.min()) < -10.0 and float(x.max()) > 10.0
        collapsed = raw[:, A] == -30.0
        assert float((s[collapsed.cuda()] - MIN_STD).abs().max()) <= 2 * U * MIN_STD + 1e-16       # std == min_std to 2 ulps
        assert float((s[~collapsed.cuda()].cpu() - (25.0 + MIN_STD)).abs().max()) <= 2 * U * 25.1    # the identity branch


def test_rejected_arguments_leave_the_buffers_untouched(L):
    A, Rn, Kn = 6, 4, 3
    raw, eps = torch.zeros(Rn, 2 * A, device='cuda'), torch.zeros(Kn, Rn, A, device='cuda')
    g = torch.ones(Rn, A, device='cuda')
    (ab, a), (mb, m), (sb, s), (db, d) = out_buf(Rn, A, A), out_buf(Rn, A, A), out_buf(Rn, A, A), out_buf(Rn, 2 * A, 2 * A)
    (eb, e) = vec_out(Rn)
    r, p, st = raw.data_ptr(), eps.data_ptr(), stream()
    o = (a.data_ptr(), m.data_ptr(), s.data_ptr())
    for bad_a in (0, 65, -1):
        assert L.genrl_tanh_normal_head_fwd(r, p, *o, Rn, bad_a, *P, 0, st) == 1
        assert L.genrl_tanh_normal_head_bwd(g.data_ptr(), r, p, d.data_ptr(), Rn, bad_a, *P, 0, st) == 1
        assert L.genrl_tanh_normal_mc_fwd(r, p, e.data_ptr(), m.data_ptr(), Rn, bad_a, Kn, *P, st) == 1
        assert L.genrl_tanh_normal_ent_bwd(g.data_ptr(), r, p, d.data_ptr(), Rn, bad_a, Kn, *P, 0, st) == 1
    assert L.genrl_tanh_normal_head_fwd(r, p, None, None, None, Rn, A, *P, 0, st) == 1             # no output
    assert L.genrl_tanh_normal_head_fwd(None, p, *o, Rn, A, *P, 0, st) == 1
    assert L.genrl_tanh_normal_head_fwd(r, p, *o, Rn, A, *P, A - 1, st) == 1                       # action pitch below A
    assert L.genrl_tanh_normal_head_bwd(g.data_ptr(), r, None, d.data_ptr(), Rn, A, *P, 0, st) == 1
    assert L.genrl_tanh_normal_head_bwd(g.data_ptr(), r, p, None, Rn, A, *P, 0, st) == 1
    for bad_k in (0, -1):
        assert L.genrl_tanh_normal_mc_fwd(r, p, e.data_ptr(), m.data_ptr(), Rn, A, bad_k, *P, st) == 1
        assert L.genrl_tanh_normal_ent_bwd(g.data_ptr(), r, p, d.data_ptr(), Rn, A, bad_k, *P, 0, st) == 1
    assert L.genrl_tanh_normal_mc_fwd(r, p, None, None, Rn, A, Kn, *P, st) == 1                    # both outputs NULL
    assert L.genrl_tanh_normal_mc_fwd(r, None, e.data_ptr(), m.data_ptr(), Rn, A, Kn, *P, st) == 1
    assert L.genrl_tanh_normal_ent_bwd(None, r, p, d.data_ptr(), Rn, A, Kn, *P, 0, st) == 1
    assert L.genrl_tanh_normal_ent_bwd(g.data_ptr(), r, p, None, Rn, A, Kn, *P, 1, st) == 1
    assert L.genrl_tanh_normal_mc_fwd(r, p, e.data_ptr(), m.data_ptr(), 0, A, Kn, *P, st) == 0     # no rows: nothing to do
    assert L.genrl_tanh_normal_head_fwd(r, p, *o, 0, A, *P, 0, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(e).all())
    vec_untouched('ent', eb, Rn)
    for b, v in ((ab, a), (mb, m), (sb, s), (db, d)):
        assert bool(torch.isnan(v).all())
        untouched('rejected call', b, v)


def test_ops_gradients_match_float64_autograd():
    """ops.tanh_normal_sample, ops.tanh_normal_entropy and ops.tanh_normal_mc_mean on (H, N, 2A) raw against float64 autograd of the
    restated formulas: the loss sends gradient through a sample and through the entropy at once"""
    from genrl_amd import ops
    H, N, A = 3, 5, 6
    g = torch.Generator().manual_seed(5)
    raw0 = torch.randn(H, N, 2 * A, generator=g) * 2
    eps, mc = torch.randn(H, N, A, generator=g), torch.randn(R.K, H, N, A, generator=g)
    w, we = torch.randn(H, N, A, generator=g), torch.randn(H, N, generator=g)

    def run(dtype, dev):
        raw = raw0.to(dtype=dtype, device=dev).requires_grad_(True)
        c = lambda t: t.to(dtype=dtype, device=dev)
        if dev == 'cuda':
            action, ent = ops.tanh_normal_sample(raw, c(eps), *P), ops.tanh_normal_entropy(raw, c(mc), *P)
            mean = ops.tanh_normal_mc_mean(raw, c(mc), *P)
            assert not mean.requires_grad
        else:
            action, ent, mean = R.sample(raw, c(eps), *P)[0], R.entropy(raw, c(mc), *P), R.mc_mean(raw, c(mc), *P).detach()
        ((action * c(w)).sum() + (ent * c(we)).sum()).backward()
        return action.detach(), ent.detach(), mean, raw.grad
    ref = run(torch.float64, 'cpu')
    got = run(torch.float32, 'cuda')
    assert got[0].shape == (H, N, A) and got[1].shape == (H, N) and got[2].shape == (H, N, A) and got[3].shape == (H, N, 2 * A)
    for a, b, what in zip(got, ref, ('action', 'entropy', 'Monte-Carlo mean', 'd raw')):
        torch.testing.assert_close(a.cpu().double(), b, rtol=2e-5, atol=2e-6, msg=lambda m_, what=what: what + ': ' + m_)
    # the entropy alone: its gradient reaches both halves of raw
    raw = raw0.cuda().requires_grad_(True)
    ops.tanh_normal_entropy(raw, mc.cuda(), *P).sum().backward()
    assert float(raw.grad[..., :A].abs().min()) > 0.0 and float(raw.grad[..., A:].abs().min()) > 0.0
    from genrl_amd._lib import GenrlHipError
    with pytest.raises(GenrlHipError):
        ops.tanh_normal_entropy(raw0, mc, *P)               # no CPU fallback
