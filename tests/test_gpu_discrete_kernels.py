"""The discrete-action kernels (csrc/discrete.hip) through their C entry points, under the convention of test_gpu_ensemble_kernels.py:
error against float64, bounded per case by 2x the error the float32 CPU restatement (tests/discrete_restatement.py, plain torch, autograd
for the backward) makes against float64 on the same inputs, with a floor of 4 units of 2^-24 x scale.  The factor 2 covers the different
summation order; the yardstick is the restatement, never the kernel.  Outputs are NaN-prefilled inside PAD-filled buffers with a guard row.

Scales.  logp and ent are functions of probabilities that carry a relative rounding error of a few 2^-24: log p then carries that as an
ABSOLUTE error whatever |log p| is (log 0.995 = -0.005 is no more accurate than log 0.5), so their scale is max(|result|, 1).  A row of
dlogits: the magnitude of the terms it is summed from (grad_scale).  The objective's loss: the mean of |terms| (a mean of terms of both signs
is no more accurate than the terms); its statistics: the mean magnitude of the normalised returns; its gradients: elementwise magnitude, with
the magnitude of the two numbers whose difference the advantage is for dlogp."""
import math

import pytest
import torch

import discrete_restatement as R
from f64check import PAD, U, checker, out_buf, untouched

pytestmark = pytest.mark.gpu

KS, GS = [2, 3, 6, 18, 33, 64], [1, 5, 257]
K = {}
RATIOS = {}
within = checker(K, RATIOS)
FLOOR, FACTOR = 4.0, 2.0
MIX = R.UNIMIX


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\ndiscrete kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


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


def logp_ent_restatement(logits, action, glogp, gent, dtype):
    lg = logits.to(dtype).clone().requires_grad_(True)
    logp, ent = R.logp_ent(lg, action.to(dtype), MIX)
    out = {}
    for name, terms in (('both', (logp * glogp.to(dtype)).sum() + (ent * gent.to(dtype)).sum()), ('logp', (logp * glogp.to(dtype)).sum()),
                        ('ent', (ent * gent.to(dtype)).sum())):
        out[name] = torch.autograd.grad(terms, lg, retain_graph=True)[0]
    return logp.detach(), ent.detach(), out


def grad_scale(logits, glogp, gent):
    """[G, 1]: the magnitude of the terms a row of dlogits is summed from.  d logp / d logit_k is a difference of two numbers of at most 1
    (the taken class against the probabilities); d ent / d logit_k = -p_k (log p_k + ent) up to the mix, a difference of p_k |log p_k| and
    p_k ent that cancels entirely where the logits are equal.  Rounding errors follow the terms, not what is left of them."""
    p = R.probs(logits.double(), MIX)
    ent = -(p * p.log()).sum(-1, keepdim=True)
    scale = torch.zeros(logits.shape[0], 1, dtype=torch.float64)
    if glogp is not None:
        scale = scale + glogp.double().abs()[:, None]
    if gent is not None:
        scale = scale + gent.double().abs()[:, None] * (p * (p.log().abs() + ent)).amax(-1, keepdim=True)
    return scale


def make_case(G, Kn, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'equal':
        logits = torch.full((G, Kn), 0.7)
    elif kind == 'gap':
        logits = torch.randn(G, Kn, generator=g)
        logits[:, 0] += 100.0
    else:
        logits = torch.randn(G, Kn, generator=g) * float(kind)
    action = torch.eye(Kn)[torch.randint(0, Kn, (G,), generator=g)]
    if kind == 'gap':
        action[0] = torch.eye(Kn)[1]                   # a taken action of the smallest probability
    glogp, gent = torch.randn(G, generator=g), torch.randn(G, generator=g)
    return logits, action, glogp, gent


def run_logp_ent(L, G, Kn, kind):
    from genrl_amd._lib import check
    logits, action, glogp, gent = make_case(G, Kn, kind, 17 + G + 100 * Kn)
    lp64, en64, d64 = logp_ent_restatement(logits, action, glogp, gent, torch.float64)
    lp32, en32, d32 = logp_ent_restatement(logits, action, glogp, gent, torch.float32)
    lgd, acd, gld, ged = logits.cuda(), action.cuda(), glogp.cuda(), gent.cuda()
    tag = f'[{G}x{Kn},{kind}]'
    one = lambda r: r.abs().clamp_min(1.0)
    # forward: each output alone (the other NULL), then both
    for want_lp, want_en in ((True, False), (False, True), (True, True)):
        lbuf, lp = vec_out(G); ebuf, en = vec_out(G)
        check(L.genrl_onehot_logp_ent_fwd(lgd.data_ptr(), acd.data_ptr() if want_lp else None, lp.data_ptr() if want_lp else None,
                                          en.data_ptr() if want_en else None, G, Kn, MIX, stream()), 'logp_ent_fwd')
        if want_lp:
            bounded('logp.fwd' + tag, lp, lp64, lp32, one(lp64))
        else:
            assert bool(torch.isnan(lp).all())
        if want_en:
            bounded('ent.fwd' + tag, en, en64, en32, one(en64))
        else:
            assert bool(torch.isnan(en).all())
        vec_untouched('logp', lbuf, G); vec_untouched('ent', ebuf, G)
    # backward: both upstream gradients, each alone, and accumulation
    for name, (use_lp, use_en) in (('both', (True, True)), ('logp', (True, False)), ('ent', (False, True))):
        dbuf, d = out_buf(G, Kn, Kn)
        check(L.genrl_onehot_logp_ent_bwd(lgd.data_ptr(), acd.data_ptr() if use_lp else None, gld.data_ptr() if use_lp else None,
                                          ged.data_ptr() if use_en else None, d.data_ptr(), G, Kn, MIX, 0, stream()), 'logp_ent_bwd')
        untouched('dlogits', dbuf, d)
        scale = grad_scale(logits, glogp if use_lp else None, gent if use_en else None).expand_as(d64[name])
        bounded(f'dlogits.{name}' + tag, d, d64[name], d32[name], scale)
    base = torch.randn(G, Kn, generator=torch.Generator().manual_seed(3))
    dbuf, d = out_buf(G, Kn, Kn)
    d.copy_(base)
    check(L.genrl_onehot_logp_ent_bwd(lgd.data_ptr(), acd.data_ptr(), gld.data_ptr(), ged.data_ptr(), d.data_ptr(), G, Kn, MIX, 1,
                                      stream()), 'logp_ent_bwd')
    untouched('dlogits (accumulate)', dbuf, d)
    ref = base.double() + d64['both']
    scale = base.double().abs() + grad_scale(logits, glogp, gent)
    bounded('dlogits.acc' + tag, d, ref, base + d32['both'], scale)
    return logits, lp, en, lp64, en64


@pytest.mark.parametrize('spread', [1, 30])
@pytest.mark.parametrize('Kn', KS)
@pytest.mark.parametrize('G', GS)
def test_logp_ent_vs_float64(L, G, Kn, spread):
    run_logp_ent(L, G, Kn, spread)


def test_logp_ent_equal_logits(L):
    """all logits equal: the entropy is log K (within the case's own bound), the gradient of the entropy vanishes"""
    for Kn in (3, 64):
        logits, lp, en, lp64, en64 = run_logp_ent(L, 5, Kn, 'equal')
        bound = K['ent.fwd'] * U * max(math.log(Kn), 1.0)
        assert float((en.double().cpu() - math.log(Kn)).abs().max()) <= bound and float((en64 - math.log(Kn)).abs().max()) <= bound


def test_logp_ent_wide_gap(L):
    """one logit 100 above the rest: the other classes sit on the floor unimix / K of the mix; everything finite"""
    from genrl_amd._lib import check
    for Kn in (6, 33):
        logits, lp, en, lp64, en64 = run_logp_ent(L, 5, Kn, 'gap')
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(en).all())
        p_min = float(R.probs(logits.double(), MIX).min())
        assert abs(p_min - MIX / Kn) <= 1e-12
        assert abs(float(lp[0]) - math.log(MIX / Kn)) <= K['logp.fwd'] * U * abs(math.log(MIX / Kn))     # (row 0 took such a class)
        d = torch.full((5, Kn), float('nan'), device='cuda')
        ac = torch.eye(Kn)[[1] * 5].cuda()
        g1 = torch.ones(5, device='cuda')
        check(L.genrl_onehot_logp_ent_bwd(logits.cuda().data_ptr(), ac.data_ptr(), g1.data_ptr(), g1.data_ptr(), d.data_ptr(), 5, Kn, MIX,
                                          0, stream()), 'logp_ent_bwd')
        assert bool(torch.isfinite(d).all())


def test_logp_ent_rejects_unsupported_widths(L):
    for Kn in (1, 65):
        x = torch.zeros(4, Kn, device='cuda')
        lbuf, lp = vec_out(4); ebuf, en = vec_out(4)
        assert L.genrl_onehot_logp_ent_fwd(x.data_ptr(), x.data_ptr(), lp.data_ptr(), en.data_ptr(), 4, Kn, MIX, stream()) == 1
        dbuf, d = out_buf(4, Kn, Kn)
        assert L.genrl_onehot_logp_ent_bwd(x.data_ptr(), x.data_ptr(), lp.data_ptr(), en.data_ptr(), d.data_ptr(), 4, Kn, MIX, 0, stream()) == 1
        torch.cuda.synchronize()
        assert bool(torch.isnan(lp).all()) and bool(torch.isnan(en).all()) and bool(torch.isnan(d).all())
        vec_untouched('logp', lbuf, 4); vec_untouched('ent', ebuf, 4); untouched('dlogits', dbuf, d)


def reinforce_restatement(t, b, lp, en, w, os_, ent_scale, dtype):
    c = lambda x: None if x is None else x.to(dtype)
    t, b, lp, en = [c(x).clone().requires_grad_(True) for x in (t, b, lp, en)]
    loss, (mean, std) = R.reinforce_objective(t, b, lp, en, c(w), c(os_), ent_scale)
    gs = torch.autograd.grad(loss * 1.7, (t, b, lp, en), allow_unused=True)
    gs = [torch.zeros_like(x) if g is None else g for g, x in zip(gs, (t, b, lp, en))]
    return loss.detach(), mean.detach(), std.detach(), gs


@pytest.mark.parametrize('ent_scale', [0.0, 3e-4])
@pytest.mark.parametrize('use_os', [False, True])
@pytest.mark.parametrize('use_w', [False, True])
@pytest.mark.parametrize('N', [1, 5, 1000])
@pytest.mark.parametrize('H', [2, 3, 16])
def test_reinforce_obj_vs_float64(L, H, N, use_w, use_os, ent_scale):
    from genrl_amd._lib import check
    g = torch.Generator().manual_seed(H * 1000 + N)
    t, b = torch.randn(H, N, generator=g) * 3 + 1, torch.randn(H, N, generator=g) * 3 + 1
    lp, en = -torch.rand(H - 1, N, generator=g) * 5, torch.rand(H - 1, N, generator=g) * 2
    w = torch.rand(H - 1, N, generator=g) if use_w else None
    os_ = torch.tensor([-0.3, 2.5]) if use_os else None
    r64 = reinforce_restatement(t, b, lp, en, w, os_, ent_scale, torch.float64)
    r32 = reinforce_restatement(t, b, lp, en, w, os_, ent_scale, torch.float32)
    td, bd, lpd, end = t.cuda(), b.cuda(), lp.cuda(), en.cuda()
    wd = w.cuda() if use_w else None
    osd = os_.cuda() if use_os else None
    ptr = lambda x: None if x is None else x.data_ptr()
    gd = torch.tensor([1.7], device='cuda')
    tag = f'[{H}x{N},w{int(use_w)},os{int(use_os)},e{ent_scale}]'
    runs = []
    for _ in range(2):
        lbuf, loss = vec_out(1); sbuf, st = vec_out(2)
        check(L.genrl_reinforce_obj_fwd(td.data_ptr(), bd.data_ptr(), lpd.data_ptr(), end.data_ptr(), ptr(wd), ptr(osd), ent_scale, H, N,
                                        loss.data_ptr(), st.data_ptr(), stream()), 'reinforce_obj_fwd')
        outs = []
        for rows in (H - 1, H, H, H - 1):
            outs.append(out_buf(rows, N, N))
        check(L.genrl_reinforce_obj_bwd(gd.data_ptr(), td.data_ptr(), bd.data_ptr(), lpd.data_ptr(), ptr(wd), ptr(osd), ent_scale, H, N,
                                        outs[0][1].data_ptr(), outs[1][1].data_ptr(), outs[2][1].data_ptr(), outs[3][1].data_ptr(), stream()),
              'reinforce_obj_bwd')
        runs.append((loss.clone(), st.clone(), [o[1].clone() for o in outs]))
    vec_untouched('loss', lbuf, 1); vec_untouched('stats', sbuf, 2)
    for name, (buf, view) in zip(('dlogp', 'dtarget', 'dbaseline', 'dent'), outs):
        untouched(name, buf, view)
    # two runs are bit-identical
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, c) for a, c in zip(runs[0][2], runs[1][2]))
    assert torch.equal(runs[0][1], runs[1][1]) or not use_os
    # the loss: a mean of terms of both signs -> scale = the mean magnitude of its terms
    nt = lambda x: R.normed(x.double(), None if os_ is None else os_.double())
    terms = (lp.double() * (nt(t)[1:] - nt(b)[1:])).abs() + ent_scale * en.double().abs()
    terms = terms * (w.double() if use_w else 1.0)
    bounded('reinforce.loss' + tag, loss, r64[0].reshape(1), r32[0].reshape(1), terms.mean().reshape(1).clamp_min(1e-30))
    if use_os:
        n64 = nt(t)
        bounded('reinforce.mean' + tag, st[:1], r64[1].reshape(1), r32[1].reshape(1), n64.abs().mean().reshape(1))
        if H * N > 1:
            bounded('reinforce.std' + tag, st[1:], r64[2].reshape(1), r32[2].reshape(1), n64.abs().mean().reshape(1))
    else:
        assert bool(torch.isnan(st).all())           # without the return EMA the statistics are not written
    dt64, db64, dl64, de64 = r64[3]
    dt32, db32, dl32, de32 = r32[3]
    dlogp, dtarget, dbaseline, dent = runs[0][2]
    for name, got, r6, r3 in (('dlogp', dlogp, dl64, dl32), ('dtarget', dtarget, dt64, dt32), ('dbaseline', dbaseline, db64, db32),
                              ('dent', dent, de64, de32)):
        # (dlogp = coefficient x advantage, and the advantage is a difference that may cancel: its scale is that of the two numbers)
        coef = 1.7 * (w.double() if use_w else torch.ones(H - 1, N, dtype=torch.float64)) / ((H - 1) * N)
        scale = coef * (nt(t)[1:].abs() + nt(b)[1:].abs()) if name == 'dlogp' else r6.abs()
        bounded(f'reinforce.{name}' + tag, got, r6, r3, scale)
    # row 0 of the returns and the baseline is unused: exactly zero
    assert float(dtarget[0].abs().max()) == 0.0 and float(dbaseline[0].abs().max()) == 0.0


def test_reinforce_obj_null_outputs_and_bad_shapes(L):
    from genrl_amd._lib import check
    H, N = 3, 5
    t = torch.randn(H, N, device='cuda'); lp = -torch.rand(H - 1, N, device='cuda')
    g = torch.ones(1, device='cuda')
    buf, dl = out_buf(H - 1, N, N)
    check(L.genrl_reinforce_obj_bwd(g.data_ptr(), t.data_ptr(), t.data_ptr(), lp.data_ptr(), None, None, 0.0, H, N, dl.data_ptr(), None, None,
                                    None, stream()), 'reinforce_obj_bwd')
    untouched('dlogp', buf, dl)
    assert float(dl.abs().max()) == 0.0                # target == baseline: no advantage
    lbuf, loss = vec_out(1)
    assert L.genrl_reinforce_obj_fwd(t.data_ptr(), t.data_ptr(), lp.data_ptr(), lp.data_ptr(), None, None, 0.0, 1, N, loss.data_ptr(), None,
                                     stream()) == 1        # H < 2
    assert L.genrl_reinforce_obj_fwd(t.data_ptr(), t.data_ptr(), lp.data_ptr(), None, None, None, 3e-4, H, N, loss.data_ptr(), None,
                                     stream()) == 1        # an entropy scale without entropies
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all())


def test_op_layer_functions_match_the_restatement():
    """ops.onehot_logp_ent / ops.onehot_probs / ops.reinforce_objective as autograd nodes"""
    from genrl_amd import ops
    g = torch.Generator().manual_seed(5)
    H, N, A = 4, 9, 6
    logits = torch.randn(H - 1, N, A, generator=g) * 2
    action = torch.eye(A)[torch.randint(0, A, (H - 1, N), generator=g)]
    t, b = torch.randn(H, N, 1, generator=g), torch.randn(H, N, 1, generator=g)
    os_ = torch.tensor([0.2, 1.5, 0.0, 0.0])

    def run(dev, dtype):
        lg = logits.to(dev, dtype).requires_grad_(True); tt = t.to(dev, dtype).requires_grad_(True); bb = b.to(dev, dtype).requires_grad_(True)
        if dev == 'cuda':
            lp, en = ops.onehot_logp_ent(lg, action.cuda())
            loss, st = ops.reinforce_objective(tt, bb, lp, en, None, os_.cuda(), 3e-4)
            probs = ops.onehot_probs(lg.detach())
        else:
            lp, en = R.logp_ent(lg, action.to(dtype))
            loss, st = R.reinforce_objective(tt[..., 0], bb[..., 0], lp, en, None, os_.to(dtype), 3e-4)
            probs = R.probs(lg.detach())
        loss.backward()
        return [x.detach().cpu().double() for x in (lp, en, loss, st[0], st[1], probs, lg.grad, tt.grad, bb.grad)]
    got, ref = run('cuda', torch.float32), run('cpu', torch.float64)
    for a, c in zip(got, ref):
        assert a.shape == c.shape or a.numel() == c.numel()
        assert torch.allclose(a.reshape(c.shape), c, rtol=1e-5, atol=1e-6 * float(c.abs().max()))
    en_only = ops.onehot_logp_ent(logits.cuda(), None)[1]
    assert torch.allclose(en_only.cpu().double(), ref[1], rtol=1e-5)
    with pytest.raises(Exception):
        ops.onehot_logp_ent(logits, action)            # no CPU fallback
