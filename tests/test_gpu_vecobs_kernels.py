"""The vector-observation kernels (csrc/vecobs.hip) through their C entry points, under the convention of test_gpu_gauss_kernels.py: error
against float64, bounded per case by 2x the error the float32 CPU restatement (tests/vecobs_restatement.py, plain torch) makes against float64
on the same inputs, with a floor of 4 units of 2^-24 x scale.  The factor 2 covers a different evaluation order; the yardstick is the
restatement, never the kernel.  Outputs are NaN-prefilled inside PAD-filled buffers with a guard row and padding columns: nothing may be
written outside.

Scales.  symlog: max(|symlog x|, 1) -- the rounding of |x| + 1 is an absolute 2^-24 in the logarithm.  A `like` row: sum_d (|mode| + T)^2 with
T = |x| (kind 0) or max(|symlog x|, 1) (kind 1).  dmode: 2 (|mode| + T) |g|.  (vecobs_restatement.like / like_bwd return them.)

Shapes: R in {1, 5, 257} (one row, a few, more than one workgroup of lane groups), D in {1, 3, 7, 9, 24, 32, 33, 64, 200} (below a lane
group, the fixture's odd widths, a whole group and one past it, a whole wave, several strides); pitches D, D + 4 (16-byte accesses stay
possible) and D + 3 (they do not); a base that is only 4-byte aligned; for symlog_rows a destination that is a column slice starting at a
column that is no multiple of 4.  Input kinds: moderate; wide (x * 1e4 with +-3e38, 0, -0 and 1e-9 among it; where float32 itself overflows --
(mode - 3e38)^2 -- the restatement's own error, and with it the bound, is infinite and the kernel must merely not produce NaN: kind 0 runs the
same inputs with 3e18 in place of 3e38 as well, where the bound is finite); mode equal to the target computed in float32 (like and gradient
exactly 0); for kind 1 a two-sided tol case with |mode - t| <= 5e-5 or >= 2e-4 and nothing
between, whose sides are asserted on the CPU in float32 and float64 before the kernel is looked at."""
import pytest
import torch

import vecobs_restatement as R
from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

RS, DS = [1, 5, 257], [1, 3, 7, 9, 24, 32, 33, 64, 200]
PITCH = {'tight': 0, 'pad4': 4, 'pad3': 3}
TOL = 1e-8
K = {}
RATIOS, REST = {}, {}
within = checker(K, RATIOS)
FLOOR, FACTOR = 4.0, 2.0
SPECIALS = [3e38, -3e38, 0.0, -0.0, 1e-9, -1e-9]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    fin = lambda d: {k: round(v, 3) for k, v in sorted(d.items())}
    print('\nvecobs kernels, largest |kernel - float64| / (2^-24 scale):', fin(RATIOS))
    print('vecobs kernels, largest |float32 restatement - float64| / (2^-24 scale):', fin(REST))


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
    K[key] = max(FACTOR * rest, FLOOR)
    print(f'{what}: restatement ratio {rest:.3g}, bound {K[key]:.3g}', end='; ')
    assert not bool(torch.isnan(got).any()), what + ': NaN'
    within(what, got, ref64, scale)
    print(f'worst kernel ratio so far {RATIOS[key]:.3g}')


def make_x(Rn, D, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Rn, D, generator=g) * 5
    if kind == 'wide':
        x = x * 1e4
        flat = x.view(-1)
        for i in range(0, flat.numel(), 3):                 # every third element: one of the special values, in rotation
            flat[i] = SPECIALS[(i // 3 + Rn + D) % len(SPECIALS)]
    return x, g


# ---------------------------------------------------------------------------------------------------------------- symlog_rows

def run_symlog(L, Rn, D, pitch, kind, off=0, col=0):
    from genrl_amd._lib import check
    x, _ = make_x(Rn, D, kind, 7 + Rn + 1000 * D)
    ldx, ldy = D + PITCH[pitch], D + PITCH[pitch] + col
    xd = in_buf(x, ldx, off)
    tag = f'[{Rn}x{D},{pitch},{kind},off{off},col{col}]'
    y64, y32 = R.symlog(x.double()), R.symlog(x)
    for flag in (1, 0):
        buf, y = out_buf(Rn, D, ldy, off + col)         # (a view that starts `col` floats into its line: a column slice of a wider buffer)
        check(L.genrl_symlog_rows(xd.data_ptr(), ldx, y.data_ptr(), ldy, Rn, D, flag, stream()), 'symlog_rows')
        untouched('symlog' + tag, buf, y)
        if flag:
            bounded(f'symlog.{kind}' + tag, y, y64, y32, y64.abs().clamp_min(1.0))
            nz = y.cpu() != 0
            assert torch.equal(torch.signbit(y.cpu())[nz], torch.signbit(x)[nz])          # the sign follows x
        else:
            assert torch.equal(y.cpu(), x), 'symlog 0 is a copy'


@pytest.mark.parametrize('pitch', sorted(PITCH))
@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('Rn', RS)
def test_symlog_rows_vs_float64(L, Rn, D, pitch):
    for kind in ('moderate', 'wide'):
        run_symlog(L, Rn, D, pitch, kind)


@pytest.mark.parametrize('D', [7, 24, 32])
def test_symlog_rows_unaligned_base_and_column_slice(L, D):
    """a base that is only 4-byte aligned takes the scalar path whatever D is; so does a destination slice that starts at column 5 of a wider
    buffer, while one that starts at column 4 of a buffer with a pitch of a multiple of 4 keeps the 16-byte accesses"""
    for off, col in ((1, 0), (0, 5), (0, 4), (3, 1)):
        run_symlog(L, 5, D, 'tight', 'wide', off, col)
        run_symlog(L, 257, D, 'pad4', 'moderate', off, col)


def test_symlog_rows_keeps_nan_and_signed_zero(L):
    x = torch.tensor([[float('nan'), 0.0, -0.0, 1.0, -1.0, float('inf'), float('-inf')]])
    buf, y = out_buf(1, 7, 7)
    assert L.genrl_symlog_rows(x.cuda().data_ptr(), 7, y.data_ptr(), 7, 1, 7, 1, stream()) == 0
    y = y.cpu()[0]
    assert bool(torch.isnan(y[0])) and float(y[1]) == 0.0 and not bool(torch.signbit(y[1])) and float(y[2]) == 0.0 and bool(torch.signbit(y[2]))
    assert abs(float(y[3]) - 0.6931471805599453) <= 2 * U and float(y[4]) == -float(y[3])
    assert float(y[5]) == float('inf') and float(y[6]) == float('-inf')


# ---------------------------------------------------------------------------------------------------------------- vec_like

def make_like(Rn, D, kind, inp, seed):
    """-> mode, x, g (CPU fp32) and, for the tol case, the mask of the elements on the small side"""
    x, g = make_x(Rn, D, 'wide' if inp.startswith('wide') else 'moderate', seed)
    if inp == 'wide18':         # the wide inputs with +-3e38 brought down to +-3e18: their squares stay inside float32 and the bound finite
        x = torch.where(x.abs() > 1e38, torch.sign(x) * 3e18, x)
    mode = torch.randn(Rn, D, generator=g)
    small = None
    if inp == 'equal':
        mode = x.clone() if kind == 0 else R.symlog(x)
    elif inp == 'tol':
        small = torch.rand(Rn, D, generator=g) < 0.5
        mag = torch.where(small, torch.rand(Rn, D, generator=g) * 4e-5, 2.5e-4 + torch.rand(Rn, D, generator=g) * 1e-2)
        sign = torch.where(torch.rand(Rn, D, generator=g) < 0.5, -1.0, 1.0)
        mode = R.symlog(x) + sign * mag
    return mode, x, torch.randn(Rn, generator=g), small


def run_like(L, Rn, D, pitch, kind, inp, off=0):
    from genrl_amd._lib import check
    mode, x, g, small = make_like(Rn, D, kind, inp, 31 + Rn + 1000 * D + kind)
    ld = D + PITCH[pitch]
    md, xd, gd = in_buf(mode, ld, off), in_buf(x, ld + 1, off), g.cuda()          # (mode and x at pitches of their own)
    tag = f'[{Rn}x{D},{pitch},{inp},off{off}]'
    if inp == 'tol':            # the sides of tol, on the CPU in both precisions, before the kernel is looked at
        for dt in (torch.float32, torch.float64):
            d = (mode.to(dt) - R.symlog(x.to(dt))) ** 2
            assert bool((d[small] < TOL / 2).all()) and bool((d[~small] > 2 * TOL).all()), dt
    l64, scale = R.like(mode.double(), x.double(), kind, TOL)
    l32, _ = R.like(mode, x, kind, TOL)
    first = None
    for _ in range(2):
        buf, like = vec_out(Rn)
        check(L.genrl_vec_like_fwd(md.data_ptr(), ld, xd.data_ptr(), ld + 1, like.data_ptr(), Rn, D, kind, TOL, stream()), 'vec_like_fwd')
        vec_untouched('like' + tag, buf, Rn)
        bounded(f'like{kind}.{inp}' + tag, like, l64, l32, scale)
        if first is None:
            first = like.clone()
        else:
            assert torch.equal(first, like), 'repeat run differs'
    d64, dscale = R.like_bwd(mode.double(), x.double(), g.double(), kind, TOL)
    d32, _ = R.like_bwd(mode, x, g, kind, TOL)
    lddm = ld + 2
    dbuf, dm = out_buf(Rn, D, lddm, off)
    check(L.genrl_vec_like_bwd(md.data_ptr(), ld, xd.data_ptr(), ld + 1, gd.data_ptr(), dm.data_ptr(), lddm, Rn, D, kind, TOL, 0, stream()),
          'vec_like_bwd')
    untouched('dmode' + tag, dbuf, dm)
    bounded(f'dmode{kind}.{inp}' + tag, dm, d64, d32, dscale)
    if inp == 'equal':
        assert float(first.abs().max()) == 0.0 and float(dm.abs().max()) == 0.0, 'mode == target: like and gradient are exactly 0'
    if inp == 'tol':
        assert float(dm.cpu()[small].abs().max() if bool(small.any()) else 0.0) == 0.0, 'below tol: the gradient is exactly 0'
        assert bool((dm.cpu()[~small] != 0).all()) or not bool((g != 0).all())
    if inp in ('moderate', 'tol'):          # accumulation into a prefilled dmode
        base = torch.randn(Rn, D, generator=torch.Generator().manual_seed(3))
        dbuf, dm = out_buf(Rn, D, lddm, off)
        dm.copy_(base)
        check(L.genrl_vec_like_bwd(md.data_ptr(), ld, xd.data_ptr(), ld + 1, gd.data_ptr(), dm.data_ptr(), lddm, Rn, D, kind, TOL, 1, stream()),
              'vec_like_bwd')
        untouched('dmode (accumulate)' + tag, dbuf, dm)
        bounded(f'dmode{kind}.acc' + tag, dm, base.double() + d64, base + d32, base.double().abs() + dscale)
        if inp == 'tol' and bool(small.any()):
            assert torch.equal(dm.cpu()[small], base[small])


@pytest.mark.parametrize('pitch', sorted(PITCH))
@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('Rn', RS)
def test_vec_like_vs_float64(L, Rn, D, pitch):
    for kind in (0, 1):
        for inp in ('moderate', 'wide', 'equal') + (('tol',) if kind == 1 else ('wide18',)):
            run_like(L, Rn, D, pitch, kind, inp)


@pytest.mark.parametrize('D', [7, 32])
def test_vec_like_unaligned_base(L, D):
    for kind in (0, 1):
        run_like(L, 5, D, 'tight', kind, 'moderate', off=1)
        run_like(L, 257, D, 'pad3', kind, 'wide', off=3)


def test_rejected_arguments_and_empty_calls_write_nothing(L):
    """D < 1, a pitch below D, a missing pointer, an unknown kind or a bad tol return 1 before any launch; R == 0 returns 0 without one"""
    x = torch.ones(4, 8, device='cuda')
    g = torch.ones(4, device='cuda')
    ybuf, y = out_buf(4, 8, 8)
    dbuf, d = out_buf(4, 8, 8)
    lbuf, like = vec_out(4)
    p, st = x.data_ptr(), stream()
    assert L.genrl_symlog_rows(p, 8, y.data_ptr(), 8, 4, 0, 1, st) == 1
    assert L.genrl_symlog_rows(p, 7, y.data_ptr(), 8, 4, 8, 1, st) == 1
    assert L.genrl_symlog_rows(p, 8, y.data_ptr(), 7, 4, 8, 1, st) == 1
    assert L.genrl_symlog_rows(None, 8, y.data_ptr(), 8, 4, 8, 1, st) == 1
    assert L.genrl_symlog_rows(p, 8, None, 8, 4, 8, 1, st) == 1
    assert L.genrl_symlog_rows(p, 8, y.data_ptr(), 8, -1, 8, 1, st) == 1
    assert L.genrl_symlog_rows(p, 8, y.data_ptr(), 8, 0, 8, 1, st) == 0
    assert L.genrl_vec_like_fwd(p, 8, p, 8, like.data_ptr(), 4, 0, 0, TOL, st) == 1
    assert L.genrl_vec_like_fwd(p, 7, p, 8, like.data_ptr(), 4, 8, 0, TOL, st) == 1
    assert L.genrl_vec_like_fwd(p, 8, p, 7, like.data_ptr(), 4, 8, 0, TOL, st) == 1
    assert L.genrl_vec_like_fwd(p, 8, p, 8, like.data_ptr(), 4, 8, 2, TOL, st) == 1
    assert L.genrl_vec_like_fwd(p, 8, p, 8, like.data_ptr(), 4, 8, 1, -1.0, st) == 1
    assert L.genrl_vec_like_fwd(p, 8, p, 8, like.data_ptr(), 4, 8, 1, float('nan'), st) == 1
    assert L.genrl_vec_like_fwd(None, 8, p, 8, like.data_ptr(), 4, 8, 0, TOL, st) == 1
    assert L.genrl_vec_like_fwd(p, 8, p, 8, None, 4, 8, 0, TOL, st) == 1
    assert L.genrl_vec_like_fwd(p, 8, p, 8, like.data_ptr(), 0, 8, 0, TOL, st) == 0
    assert L.genrl_vec_like_bwd(p, 8, p, 8, g.data_ptr(), d.data_ptr(), 8, 4, 0, 0, TOL, 0, st) == 1
    assert L.genrl_vec_like_bwd(p, 8, p, 8, g.data_ptr(), d.data_ptr(), 7, 4, 8, 0, TOL, 0, st) == 1
    assert L.genrl_vec_like_bwd(p, 8, p, 8, None, d.data_ptr(), 8, 4, 8, 0, TOL, 0, st) == 1
    assert L.genrl_vec_like_bwd(p, 8, p, 8, g.data_ptr(), None, 8, 4, 8, 0, TOL, 0, st) == 1
    assert L.genrl_vec_like_bwd(p, 8, p, 8, g.data_ptr(), d.data_ptr(), 8, 4, 8, -1, TOL, 0, st) == 1
    assert L.genrl_vec_like_bwd(p, 8, p, 8, g.data_ptr(), d.data_ptr(), 8, 0, 8, 1, TOL, 1, st) == 0
    torch.cuda.synchronize()
    for b, v in ((ybuf, y), (dbuf, d)):
        assert bool(torch.isnan(v).all())
        untouched('rejected call', b, v)
    assert bool(torch.isnan(like).all())
    vec_untouched('like', lbuf, 4)


# ---------------------------------------------------------------------------------------------------------------- op layer

def test_ops_against_float64_autograd():
    """ops.symlog_rows gathering two keys into one buffer, and ops.vec_like of both kinds with mode a column slice of a padded buffer,
    against float64 autograd of the restatement"""
    from genrl_amd import ops
    B_, T_ = 3, 5
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(B_, T_, 7, generator=g) * 50, torch.randn(B_, T_, 5, generator=g) * 50
    buf = torch.full((B_ * T_, 12), float('nan'), device='cuda')
    assert ops.symlog_rows(a.cuda(), out=buf, col=0) is buf and ops.symlog_rows(b.cuda(), out=buf, col=7) is buf
    ref = R.gather([a.double(), b.double()], True).reshape(B_ * T_, 12)
    torch.testing.assert_close(buf.cpu().double(), ref, rtol=0, atol=4 * U * float(ref.abs().max()))
    torch.testing.assert_close(ops.symlog_rows(a.cuda()).cpu().double(), R.symlog(a.double()), rtol=0, atol=4 * U * float(ref.abs().max()))
    assert torch.equal(ops.symlog_rows(a.cuda(), symlog=False).cpu(), a)
    for kind in (0, 1):
        mode = torch.randn(B_, T_, 9, generator=g)
        x = torch.randn(B_, T_, 9, generator=g) * 5
        w = torch.randn(B_, T_, generator=g)
        pad = torch.zeros(B_, T_, 12, device='cuda')
        pad[..., :9] = mode
        pad.requires_grad_(True)
        like = ops.vec_like(pad[..., :9], x.cuda(), kind)
        assert like.shape == (B_, T_)
        (like * w.cuda()).sum().backward()
        m64 = mode.double().requires_grad_(True)
        l64 = R.like(m64, x.double(), kind)[0]
        (l64 * w.double()).sum().backward()
        torch.testing.assert_close(like.detach().cpu().double(), l64.detach(), rtol=2e-6, atol=1e-6)
        torch.testing.assert_close(pad.grad[..., :9].cpu().double(), m64.grad, rtol=2e-6, atol=1e-6)
        assert float(pad.grad[..., 9:].abs().max()) == 0.0
