"""The kernels of the learned discount (csrc/discount.hip) through their C entry points, under the convention of test_gpu_gauss_kernels.py:
error against float64, bounded per case by 2x the error the float32 CPU restatement (tests/discount_restatement.py, plain torch) makes against
float64 on the same inputs, with a floor of 4 units of 2^-24 x scale.  The factor 2 covers a different evaluation order; the yardstick is the
restatement, never the kernel.  Outputs are NaN-prefilled inside PAD-filled buffers with a guard row: every element must be written and
nothing outside.

Scales: the magnitude of the terms an element is summed from.  like: |t z| + softplus(z).  Its gradient: |g| (|t| + sigmoid(z)) z (1 - z).
disc and weight: their own magnitude (products).  d x of the discounts: its own magnitude.  A lambda-return: the same recurrence on the
magnitudes of reward, value and discount; its gradients: the recurrence a_t on magnitudes, times the magnitudes of what multiplies it
(discount_restatement.lambda_return_disc_bwd returns them).

Shapes: rows / columns 1, 36 (the fixture's), 255, 256, 257 (the 256-thread workgroup's edge) and 1000 (several workgroups); H1 in {2, 3, 16}
and H in {1, 2, 15}: the time loops run once, twice and many times.  gamma and lam cross the C boundary as floats: the float64 reference
and the restatement take the float32 values of 0.99 and 0.95, the kernels' actual inputs (1 - 0.95f is 4 units of 2^-24 away from 0.05)."""
import numpy as np
import pytest
import torch

import discount_restatement as R
from f64check import PAD, U, checker, out_buf, untouched

pytestmark = pytest.mark.gpu

K, RATIOS, REST = {}, {}, {}
within = checker(K, RATIOS)
FLOOR, FACTOR = 4.0, 2.0
NS = [1, 255, 256, 257, 1000]
GAMMA, LAMS = float(np.float32(0.99)), (0.0, float(np.float32(0.95)), 1.0)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\ndiscount kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})
    print('the float32 restatement on the same inputs:', {k: round(v, 3) for k, v in sorted(REST.items())})


def bounded(what, got, ref64, rest32, scale):
    key = what.split('[')[0]
    live = scale > 0
    rest = float(((rest32.double() - ref64).abs()[live] / (U * scale[live])).max()) if bool(live.any()) else 0.0
    REST[key] = max(REST.get(key, 0.0), rest)
    K[key] = max(FACTOR * rest, FLOOR)
    print(f'{what}: restatement ratio {rest:.3g}, bound {K[key]:.3g}', end='; ')
    within(what, got, ref64, scale)
    print(f'worst kernel ratio so far {RATIOS[key]:.3g}')


def mat_out(rows, cols):
    return out_buf(rows, cols, cols)


def ok(code, what):
    from genrl_amd._lib import check
    check(code, what)


@pytest.mark.parametrize('Rn', [1, 36, 255, 256, 257, 1000])
def test_binary_like_vs_float64(L, Rn):
    g = torch.Generator().manual_seed(100 + Rn)
    for special in (None, 80.0, -80.0, 0.0):
        for tv in (0.0, 1.0, 0.5, 'mixed'):
            x = torch.randn(Rn, generator=g) * 4
            if special is not None:
                x[::7] = special
            t = torch.tensor([0.0, 1.0, 0.5])[torch.arange(Rn) % 3] if tv == 'mixed' else torch.full((Rn,), tv)
            gl = torch.randn(Rn, generator=g)
            gl = gl + 0.5 * torch.sign(gl)          # (|g| >= 0.5: a gradient at x = -80, ~1e-35 |g|, stays a normal float32)
            tag = f'[{Rn},x{special},t{tv}]'
            xd, td, gd = x.cuda(), t.cuda(), gl.cuda()
            buf, like = mat_out(1, Rn)
            ok(L.genrl_binary_like_fwd(xd.data_ptr(), td.data_ptr(), like.data_ptr(), Rn, stream()), 'binary_like_fwd')
            untouched('like' + tag, buf, like)
            bounded('like.fwd' + tag, like[0], R.binary_like(x.double(), t.double()), R.binary_like(x, t),
                    R.binary_like_scale(x.double(), t.double()))
            buf, dx = mat_out(1, Rn)
            ok(L.genrl_binary_like_bwd(xd.data_ptr(), td.data_ptr(), gd.data_ptr(), dx.data_ptr(), Rn, stream()), 'binary_like_bwd')
            untouched('dx' + tag, buf, dx)
            d64, scale = R.binary_like_bwd(x.double(), t.double(), gl.double())
            bounded('like.bwd' + tag, dx[0], d64, R.binary_like_bwd(x, t, gl)[0], scale)
            assert bool(torch.isfinite(like).all()) and bool(torch.isfinite(dx).all())
            if special in (80.0, -80.0) and tv != 0.5:          # the gradient does not vanish to zero at either end
                assert float(dx[0, 0].abs()) > 0.0


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('H1', [2, 3, 16])
def test_imag_discount_vs_float64(L, H1, N):
    g = torch.Generator().manual_seed(7 * H1 + N)
    gamma = GAMMA
    x = torch.randn(H1, N, generator=g) * 3
    x[0, 0], x[-1, 0], x[1, -1] = 80.0, -80.0, 0.0
    gd = torch.randn(H1, N, generator=g)
    gd = gd + 0.5 * torch.sign(gd)              # (|g| >= 0.5: a gradient at |x| = 80, ~4e-36 |g|, stays a normal float32)
    flags = (torch.rand(N, generator=g) < 0.3).float()
    flags[0] = 1.0                       # a column that is terminal at the start
    if N > 1:
        flags[1] = 0.0
    xd, gdd = x.cuda(), gd.cuda()
    for term in (None, flags):
        tag = f'[{H1}x{N},{"term" if term is not None else "no term"}]'
        td = term.cuda() if term is not None else None
        d64, w64 = R.imag_discount(x.double(), None if term is None else term.double(), gamma)
        d32, w32 = R.imag_discount(x, term, gamma)
        (bd, disc), (bw, weight) = mat_out(H1, N), mat_out(H1, N)
        ok(L.genrl_imag_discount_fwd(xd.data_ptr(), td.data_ptr() if td is not None else None, H1, N, gamma, disc.data_ptr(),
                                     weight.data_ptr(), stream()), 'imag_discount_fwd')
        untouched('disc' + tag, bd, disc); untouched('weight' + tag, bw, weight)
        bounded('disc.fwd' + tag, disc, d64, d32, d64.abs())
        bounded('weight.fwd' + tag, weight, w64, w32, w64.abs())
        assert torch.equal(weight[0], torch.ones(N, device='cuda'))
        bx, dx = mat_out(H1, N)
        ok(L.genrl_imag_discount_bwd(xd.data_ptr(), gdd.data_ptr(), int(term is not None), H1, N, gamma, dx.data_ptr(), stream()),
           'imag_discount_bwd')
        untouched('dx' + tag, bx, dx)
        dx64, scale = R.imag_discount_bwd(x.double(), gd.double(), term is not None, gamma)
        bounded('disc.bwd' + tag, dx, dx64, R.imag_discount_bwd(x, gd, term is not None, gamma)[0], scale)
        assert bool(torch.isfinite(dx).all())
        if term is not None:
            dead = term.bool().cuda()
            assert float(disc[0][dead].abs().max()) == 0.0 and float(weight[1:][:, dead].abs().max()) == 0.0
            assert torch.equal(disc[0][~dead], torch.full_like(disc[0][~dead], gamma))
            assert float(dx[0].abs().max()) == 0.0
        else:
            assert float(dx[0].abs().min()) > 0.0 and float(weight.min()) > 0.0


def lambda_inputs(H, N, rows, seed):
    g = torch.Generator().manual_seed(seed)
    reward = torch.randn(rows, N, generator=g)
    value = torch.randn(H + 1, N, generator=g) * 2
    disc = torch.rand(rows, N, generator=g) * 0.99
    disc[:, 0] = 0.0                    # a column of zero discounts
    gret = torch.randn(H, N, generator=g)
    if rows == H + 1:                   # the unread row: whatever it holds
        reward[H], disc[H] = float('nan'), float('nan')
    return reward, value, disc, gret


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('H', [1, 2, 15])
def test_lambda_return_disc_vs_float64(L, H, N):
    for lam in LAMS:
        for rows in (H, H + 1):
            reward, value, disc, gret = lambda_inputs(H, N, rows, 31 * H + N + rows)
            tag = f'[{H}x{N},lam{lam:.2f},{rows} rows]'
            rd, vd, dd, gd = reward.cuda(), value.cuda(), disc.cuda(), gret.cuda()
            r_, d_ = reward[:H], disc[:H]
            buf, ret = mat_out(H, N)
            ok(L.genrl_lambda_return_disc_fwd(rd.data_ptr(), vd.data_ptr(), dd.data_ptr(), ret.data_ptr(), H, N, lam, stream()),
               'lambda_return_disc_fwd')
            untouched('ret' + tag, buf, ret)
            bounded('lambda.fwd' + tag, ret, R.lambda_return_disc(r_.double(), value.double(), d_.double(), lam),
                    R.lambda_return_disc(r_, value, d_, lam), R.lambda_return_disc_scale(r_.double(), value.double(), d_.double(), lam))
            assert torch.equal(ret[:, 0].cpu(), reward[:H, 0]), 'zero discounts: the return is the reward'
            (br, dr), (bv, dv), (bd, ddisc) = mat_out(rows, N), mat_out(H + 1, N), mat_out(rows, N)
            retc = ret.contiguous()
            ok(L.genrl_lambda_return_disc_bwd(gd.data_ptr(), vd.data_ptr(), dd.data_ptr(), retc.data_ptr(), dr.data_ptr(), dv.data_ptr(),
                                              ddisc.data_ptr(), H, N, lam, int(rows == H + 1), stream()), 'lambda_return_disc_bwd')
            for name, b, v in (('dreward', br, dr), ('dvalue', bv, dv), ('ddisc', bd, ddisc)):
                untouched(name + tag, b, v)
            ret_in = retc.cpu()               # (the backward reads the forward's fp32 output: so do both restatements)
            g64, s64 = R.lambda_return_disc_bwd(gret.double(), value.double(), d_.double(), ret_in.double(), lam, rows)
            g32, _ = R.lambda_return_disc_bwd(gret, value, d_, ret_in, lam, rows)
            for name, got, a, b, s in zip(('dreward', 'dvalue', 'ddisc'), (dr, dv, ddisc), g64, g32, s64):
                bounded(f'lambda.{name}' + tag, got, a, b, s)
            assert float(dv[0].abs().max()) == 0.0
            if rows == H + 1:
                assert float(dr[H].abs().max()) == 0.0 and float(ddisc[H].abs().max()) == 0.0


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('H', [1, 2, 15])
def test_equal_discounts_give_the_scalar_kernels_bits(L, H, N):
    for lam in LAMS:
        for rows in (H, H + 1):
            reward, value, _, gret = lambda_inputs(H, N, rows, 5 * H + N)
            reward = torch.nan_to_num(reward, nan=0.25)
            gamma = GAMMA
            rd, vd, gd = reward.cuda(), value.cuda(), gret.cuda()
            dd = torch.full((rows, N), gamma, device='cuda')
            ret_s, ret_d = torch.empty(H, N, device='cuda'), torch.empty(H, N, device='cuda')
            ok(L.genrl_lambda_return_fwd(rd.data_ptr(), vd.data_ptr(), ret_s.data_ptr(), H, N, gamma, lam, stream()), 'lambda_return_fwd')
            ok(L.genrl_lambda_return_disc_fwd(rd.data_ptr(), vd.data_ptr(), dd.data_ptr(), ret_d.data_ptr(), H, N, lam, stream()),
               'lambda_return_disc_fwd')
            assert torch.equal(ret_s, ret_d), (H, N, lam, rows)
            e = lambda r: torch.empty(r, N, device='cuda')
            dr_s, dv_s, dr_d, dv_d, ddisc = e(rows), e(H + 1), e(rows), e(H + 1), e(rows)
            tail = int(rows == H + 1)
            ok(L.genrl_lambda_return_bwd(gd.data_ptr(), dr_s.data_ptr(), dv_s.data_ptr(), H, N, gamma, lam, tail, stream()), 'lambda_return_bwd')
            ok(L.genrl_lambda_return_disc_bwd(gd.data_ptr(), vd.data_ptr(), dd.data_ptr(), ret_d.data_ptr(), dr_d.data_ptr(), dv_d.data_ptr(),
                                              ddisc.data_ptr(), H, N, lam, tail, stream()), 'lambda_return_disc_bwd')
            assert torch.equal(dr_s, dr_d) and torch.equal(dv_s, dv_d), (H, N, lam, rows)


def test_rejections_write_nothing(L):
    N, H = 36, 3
    x = torch.randn(H + 1, N, device='cuda')
    outs = [mat_out(H + 1, N) for _ in range(3)]
    p = lambda i: outs[i][1].data_ptr()
    s = stream()
    calls = [
        L.genrl_binary_like_fwd(x.data_ptr(), x.data_ptr(), p(0), 0, s),
        L.genrl_binary_like_fwd(None, x.data_ptr(), p(0), N, s),
        L.genrl_binary_like_fwd(x.data_ptr(), None, p(0), N, s),
        L.genrl_binary_like_fwd(x.data_ptr(), x.data_ptr(), None, N, s),
        L.genrl_binary_like_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), p(0), -1, s),
        L.genrl_binary_like_bwd(x.data_ptr(), x.data_ptr(), None, p(0), N, s),
        L.genrl_binary_like_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, N, s),
        L.genrl_imag_discount_fwd(x.data_ptr(), None, 0, N, 0.99, p(0), p(1), s),
        L.genrl_imag_discount_fwd(x.data_ptr(), None, H + 1, 0, 0.99, p(0), p(1), s),
        L.genrl_imag_discount_fwd(None, None, H + 1, N, 0.99, p(0), p(1), s),
        L.genrl_imag_discount_fwd(x.data_ptr(), None, H + 1, N, 0.99, None, p(1), s),
        L.genrl_imag_discount_fwd(x.data_ptr(), None, H + 1, N, 0.99, p(0), None, s),
        L.genrl_imag_discount_bwd(x.data_ptr(), x.data_ptr(), 1, 0, N, 0.99, p(0), s),
        L.genrl_imag_discount_bwd(x.data_ptr(), x.data_ptr(), 1, H + 1, -5, 0.99, p(0), s),
        L.genrl_imag_discount_bwd(x.data_ptr(), None, 1, H + 1, N, 0.99, p(0), s),
        L.genrl_imag_discount_bwd(x.data_ptr(), x.data_ptr(), 1, H + 1, N, 0.99, None, s),
        L.genrl_lambda_return_disc_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), p(0), 0, N, 0.95, s),
        L.genrl_lambda_return_disc_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), p(0), H, 0, 0.95, s),
        L.genrl_lambda_return_disc_fwd(x.data_ptr(), x.data_ptr(), None, p(0), H, N, 0.95, s),
        L.genrl_lambda_return_disc_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, H, N, 0.95, s),
        L.genrl_lambda_return_disc_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), p(0), p(1), p(2), 0, N, 0.95, 1, s),
        L.genrl_lambda_return_disc_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), p(0), p(1), p(2), H, 0, 0.95, 1, s),
        L.genrl_lambda_return_disc_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, p(0), p(1), p(2), H, N, 0.95, 1, s),
        L.genrl_lambda_return_disc_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), p(0), p(1), None, H, N, 0.95, 1, s),
        L.genrl_lambda_return_disc_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, p(1), p(2), H, N, 0.95, 1, s),
    ]
    assert calls == [1] * len(calls), calls
    torch.cuda.synchronize()
    for buf, view in outs:
        untouched('rejected call', buf, view)
        assert bool(torch.isnan(view).all()), 'a rejected call wrote into its output'
