"""genrl_kl_loss_fwd / genrl_kl_loss_bwd (csrc/dist.hip) through their C entry points in the three modes (GENRL_KL_*), under the convention of
test_gpu_gauss_kernels.py: error against float64, bounded per case by 2x the error the float32 CPU restatement
(klmodes_restatement.loss_from_rows / loss_bwd, plain torch) makes against float64 on the same inputs, with a floor of 4 units of
2^-24 x scale.  The yardstick is the restatement, never the kernel.  Outputs are NaN-prefilled inside PAD-filled buffers: nothing may be
written outside, and a rejected call writes nothing at all.

The float64 reference reads what the kernel reads: the float32 rows, and `free`, `mix` and the upstream gradient as the float32 the C
boundary rounds them to (which side of the clamp a row lies on is decided by that `free`, exactly, on both sides).  Scales: loss -- the mean of the magnitudes it is summed from,
mean(max(|kl|, |free|)) (averaged mode: max(mean|kl|, |free|)); mean -- mean|kl|; gp / gq -- their own elementwise magnitude (a product of
two or three factors); an exact zero must be an exact zero.

Shapes: R in {1, 36, 255, 256, 257, 1000}: one wave's worth, one full workgroup, the 256 boundary from both sides, several strides of the
one-workgroup sum and several workgroups of the backward.  mix in {0.2, 0.85}; free 0, inside the rows' range (0.45: the mean lies above;
0.95: below) and above every row."""
import numpy as np
import pytest
import torch

import klmodes_restatement as R
from f64check import PAD, U, checker

pytestmark = pytest.mark.gpu

RS = [1, 36, 255, 256, 257, 1000]
FREES = [0.0, 0.45, 0.95, 2.0]
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
    print('\nkl_loss kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


def vec_out(n):
    buf = torch.full((n + 4,), PAD, device='cuda')
    buf[:n] = float('nan')
    return buf, buf[:n]


def vec_untouched(what, buf, n):
    assert torch.equal(buf[n:], torch.full_like(buf[n:], PAD)), f'{what}: wrote past its output'


def bounded(what, got, ref64, rest32, scale):
    key = what.split('[')[0]
    ref64, rest32, scale = (torch.as_tensor(t).reshape(got.shape) for t in (ref64, rest32, scale))
    live = scale > 0
    rest = float(((rest32.double() - ref64).abs()[live] / (U * scale[live])).max()) if bool(live.any()) else 0.0
    K[key] = max(FACTOR * rest, FLOOR)
    within(what, got, ref64, scale)
    print(f'{what}: restatement ratio {rest:.3g}, bound {K[key]:.3g}, worst kernel ratio so far {RATIOS[key]:.3g}')


def f32(x):
    return float(np.float32(x))


def rows(Rn, seed=0):
    """float32 per-row KLs in (0.2, 1.2): uniform, so the mean lies near 0.7 for R > 1"""
    return 0.2 + torch.rand(Rn, generator=torch.Generator().manual_seed(100 + Rn + seed))


def run(L, kl, mode, mix, free, gloss=1.7, tag=''):
    """one forward and one backward of the pair on `kl` (float32, CPU) against float64 -> loss, mean, gp, gq (device tensors)"""
    from genrl_amd._lib import check
    Rn, code = kl.numel(), R.MODES[mode]
    free, mix, gloss = f32(free), f32(mix), f32(gloss)
    kd, gl = kl.cuda(), torch.tensor([gloss], device='cuda')
    (lb, loss), (mb, mean), (pb, gp), (qb, gq) = vec_out(1), vec_out(1), vec_out(Rn), vec_out(Rn)
    check(L.genrl_kl_loss_fwd(kd.data_ptr(), Rn, code, mix, free, loss.data_ptr(), mean.data_ptr(), stream()), 'kl_loss_fwd')
    check(L.genrl_kl_loss_bwd(kd.data_ptr(), mean.data_ptr(), gl.data_ptr(), Rn, code, mix, free, gp.data_ptr(), gq.data_ptr(), stream()),
          'kl_loss_bwd')
    for what, b, n in (('loss', lb, 1), ('mean', mb, 1), ('gp', pb, Rn), ('gq', qb, Rn)):
        vec_untouched(what + tag, b, n)
    k64 = kl.double()
    l64, m64 = R.loss_from_rows(k64, mode, mix, free)
    # which side of the clamp the float32 mean lies on decides the averaged mode: the cases keep the mean away from `free` (or exactly on it)
    if mode == 'free_avg':
        assert float(m64) == free or abs(float(m64) - free) > 1e-4 * max(1.0, free), (tag, float(m64), free)
    l32, m32 = R.loss_from_rows(kl, mode, mix, free)
    lscale = torch.maximum(k64.abs().mean(), torch.tensor(abs(free), dtype=torch.float64)) if mode == 'free_avg' \
        else torch.maximum(k64.abs(), torch.tensor(abs(free), dtype=torch.float64)).mean()
    bounded(f'loss.{mode}' + tag, loss, l64, l32, lscale)
    bounded('mean' + tag, mean, m64, m32, k64.abs().mean())
    g64 = R.loss_bwd(k64, torch.tensor(gloss, dtype=torch.float64), mode, mix, free)
    g32 = R.loss_bwd(kl, torch.tensor(gloss), mode, mix, free)
    for name, got, a, b in (('gp', gp, g64[0], g32[0]), ('gq', gq, g64[1], g32[1])):
        assert not bool(torch.isnan(got).any()), f'{name}{tag}: an element was not written'
        assert torch.equal(got.cpu() == 0, a == 0), f'{name}{tag}: the exact zeros differ'
        bounded(f'{name}.{mode}' + tag, got, a, b, a.abs())
    return loss, mean, gp, gq


@pytest.mark.parametrize('mode', sorted(R.MODES))
@pytest.mark.parametrize('Rn', RS)
def test_pair_vs_float64(L, Rn, mode):
    for mix in (0.2, 0.85):
        for free in FREES:
            kl = rows(Rn)
            if mode == 'free_avg' and Rn == 1 and abs(float(kl[0]) - f32(free)) < 1e-2:
                kl = kl + 0.05
            tag = f'[{Rn},{mode},mix{mix},free{free}]'
            loss, mean, gp, gq = run(L, kl, mode, mix, free, tag=tag)
            above = kl > f32(free)
            if free == 2.0:                                   # above every row: the loss is the clamp's floor, no gradient anywhere
                assert float(gp.abs().max()) == 0.0 and float(gq.abs().max()) == 0.0
                assert abs(float(loss) - 2.0) <= 4 * U * 2.0
            elif free == 0.0:
                assert bool((gp > 0).all()) and bool((gq > 0).all())
            elif mode != 'free_avg' and Rn > 1:                # rows on both sides of the clamp
                assert bool(above.any()) and not bool(above.all())
                assert torch.equal(gp.cpu() > 0, above) and torch.equal(gq.cpu() > 0, above)
            if mode == 'unbalanced':
                assert torch.equal(gp, gq)
            if mode == 'free_avg' and Rn > 1:                  # every row the same gradient: all of it or none
                assert float(gp.max()) == float(gp.min()) and float(gq.max()) == float(gq.min())
                assert (float(gp[0]) > 0) == (float(kl.double().mean()) > f32(free))
    # the same call again: bit-identical
    again = run(L, rows(Rn), mode, 0.85, 0.45, tag=f'[{Rn},{mode},again]')
    once = run(L, rows(Rn), mode, 0.85, 0.45, tag=f'[{Rn},{mode},again]')
    assert all(torch.equal(a, b) for a, b in zip(again, once))


def test_unbalanced_tie_gets_half_the_gradient(L):
    kl = rows(36)
    free = float(kl[7])
    assert int((kl == free).sum()) == 1
    loss, mean, gp, gq = run(L, kl, 'unbalanced', 0.2, free, gloss=2.0, tag='[tie]')
    full = float(gp[kl.argmax()])
    assert full > 0 and float(gp[7]) == 0.5 * full and float(gq[7]) == 0.5 * full
    _, _, bp, bq = run(L, kl, 'balanced', 0.2, free, gloss=2.0, tag='[tie]')
    assert float(bp[7]) == 0.5 * float(bp[kl.argmax()]) and float(bq[7]) == 0.5 * float(bq[kl.argmax()])


@pytest.mark.parametrize('mix', [0.2, 0.85])
def test_averaged_tie_is_on_the_mean(L, mix):
    """256 rows of 0.5, free 0.5: the sum 128 and the mean 0.5 are exact in float32, so this is a tie: every row gets half of
    mix gloss / R and half of (1 - mix) gloss / R"""
    kl = torch.full((256,), 0.5)
    loss, mean, gp, gq = run(L, kl, 'free_avg', mix, 0.5, gloss=2.0, tag='[avg tie]')
    assert float(mean) == 0.5
    above = run(L, kl, 'free_avg', mix, 0.25, gloss=2.0, tag='[avg above]')
    assert torch.equal(gp, 0.5 * above[2]) and torch.equal(gq, 0.5 * above[3]) and float(gp.min()) > 0 and float(gq.min()) > 0
    gm = torch.tensor(2.0) / 256
    assert torch.equal(above[2].cpu(), (torch.tensor(mix) * gm).expand(256)) and torch.equal(above[3].cpu(), ((1.0 - torch.tensor(mix)) * gm).expand(256))


@pytest.mark.parametrize('Rn', RS)
def test_clamped_mean_yields_exact_zeros(L, Rn):
    kl = rows(Rn)
    free = float(kl.max()) - 1e-3 if Rn > 1 else float(kl.max()) + 0.1          # rows above `free`, the mean below it
    assert float(kl.double().mean()) < f32(free) - 1e-3
    loss, mean, gp, gq = run(L, kl, 'free_avg', 0.85, free, tag=f'[{Rn},clamped mean]')
    assert torch.equal(gp, torch.zeros_like(gp)) and torch.equal(gq, torch.zeros_like(gq))
    assert float(loss) == pytest.approx(f32(free), rel=4 * U)


@pytest.mark.parametrize('Rn', RS)
def test_mode_0_equals_the_balanced_pair_bit_for_bit(L, Rn):
    kl = rows(Rn, seed=3)
    kd, gl = kl.cuda(), torch.tensor([1.3], device='cuda')
    for mix in (0.2, 0.85):
        for free in (0.0, 0.45, float(kl[0]), 2.0):
            old = [torch.full((n,), float('nan'), device='cuda') for n in (1, Rn, Rn)]
            new = [torch.full((n,), float('nan'), device='cuda') for n in (1, Rn, Rn)]
            assert L.genrl_kl_balance_fwd(kd.data_ptr(), Rn, mix, free, old[0].data_ptr(), stream()) == 0
            assert L.genrl_kl_balance_bwd(kd.data_ptr(), gl.data_ptr(), Rn, mix, free, old[1].data_ptr(), old[2].data_ptr(), stream()) == 0
            for mean in (None, torch.zeros(1, device='cuda')):          # mean is optional outside the averaged mode
                mp = None if mean is None else mean.data_ptr()
                assert L.genrl_kl_loss_fwd(kd.data_ptr(), Rn, 0, mix, free, new[0].data_ptr(), mp, stream()) == 0
                assert L.genrl_kl_loss_bwd(kd.data_ptr(), mp, gl.data_ptr(), Rn, 0, mix, free, new[1].data_ptr(), new[2].data_ptr(), stream()) == 0
                assert all(torch.equal(a, b) for a, b in zip(old, new)), (Rn, mix, free)


def test_rejections_write_nothing(L):
    kd, gl = rows(36).cuda(), torch.ones(1, device='cuda')
    (lb, loss), (mb, mean), (pb, gp), (qb, gq) = vec_out(1), vec_out(1), vec_out(36), vec_out(36)
    k, g, lo, me, p, q, st = kd.data_ptr(), gl.data_ptr(), loss.data_ptr(), mean.data_ptr(), gp.data_ptr(), gq.data_ptr(), stream()
    for mode in (3, -1, 7):                                                                      # unknown modes
        assert L.genrl_kl_loss_fwd(k, 36, mode, 0.8, 0.5, lo, me, st) == 1
        assert L.genrl_kl_loss_bwd(k, me, g, 36, mode, 0.8, 0.5, p, q, st) == 1
    for Rn in (0, -4):
        assert L.genrl_kl_loss_fwd(k, Rn, 0, 0.8, 0.5, lo, me, st) == 1
        assert L.genrl_kl_loss_bwd(k, me, g, Rn, 0, 0.8, 0.5, p, q, st) == 1
    assert L.genrl_kl_loss_fwd(None, 36, 0, 0.8, 0.5, lo, me, st) == 1
    assert L.genrl_kl_loss_fwd(k, 36, 1, 0.8, 0.5, None, me, st) == 1
    assert L.genrl_kl_loss_fwd(k, 36, 2, 0.8, 0.5, lo, None, st) == 1                             # the averaged mode needs `mean`
    assert L.genrl_kl_loss_bwd(k, None, g, 36, 2, 0.8, 0.5, p, q, st) == 1
    assert L.genrl_kl_loss_bwd(None, me, g, 36, 1, 0.8, 0.5, p, q, st) == 1                       # the per-row modes need `kl`
    assert L.genrl_kl_loss_bwd(k, me, None, 36, 0, 0.8, 0.5, p, q, st) == 1
    assert L.genrl_kl_loss_bwd(k, me, g, 36, 0, 0.8, 0.5, None, q, st) == 1
    assert L.genrl_kl_loss_bwd(k, me, g, 36, 0, 0.8, 0.5, p, None, st) == 1
    torch.cuda.synchronize()
    for what, b, v in (('loss', lb, loss), ('mean', mb, mean), ('gp', pb, gp), ('gq', qb, gq)):
        assert bool(torch.isnan(v).all()), what
        vec_untouched(what, b, v.numel())
