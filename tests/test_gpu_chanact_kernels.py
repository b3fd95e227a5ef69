"""genrl_chan_act_fwd_h2u / genrl_chan_act_bwd_h2u (csrc/rowops.hip): the activation of a norm-free conv layer over its pixel rows, with
the bias gradient and the uniform planes of its output, for SiLU and ELU against float64.

Bound, per quantity and case (test_gpu_elu_kernels.py's convention): |kernel - float64| <= max(2 r, 4) 2^-24 scale per element, where r is
the worst ratio the float32 plain-torch CPU restatement (F.silu / F.elu, autograd for the backward, its own `sum(0)` for db) reaches against
float64 on the same inputs; r < 64 is asserted.  Scales are that file's with the LayerNorm terms reduced to |z| itself: |z| + |y| for the
forward; |dy| elu'(z) (1 + |z| where z <= 0) resp. |dy| s (1 + |z| (1 - s)) with s = sigmoid(z) for the backward; for db the sum of the rows'
scales.  2^-126 is added to every scale (a result below fp32's smallest normal number may flush: SiLU at z = -95).

Inputs: rows of spread 10^(-2 .. 1) with column 0 positive and column 1 negative, so both signs are in every row; the last columns of every
row hold the special values 0, -0, +-1e-6, +-1e-4, +-1e-3, +-95 -- all ten where the row has twelve columns or more, N - 2 of them rotating
with the row where it is narrower (N = 4, 6, 8).  Shapes: the smallest that select each arm and each loop edge -- lane groups of 16 / 32 /
64 lanes (N = 4, 64 | 68, 128 | 132, 256), two to four float4 per lane (N = 260, 384, 772, 1024), the scalar arm (N = 6, N = 1028, a row
spacing that is no multiple of 4, a base pointer one float off); M = 1, 63, 64, 70 (no multiple of the 4 / 8 / 16 rows of a workgroup), and
M = 32776 at N = 8 / 4100 at N = 384: past 2048 (forward) and 1024 (backward) workgroups, so that the row loop runs again."""
import pytest
import torch
import torch.nn.functional as F

from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

SILU, ELU, EINVAL = 1, 2, 1
ACTS = {'SiLU': SILU, 'ELU': ELU}
K, RATIOS, REST = {}, {}, {}
within = checker(K, RATIOS)
TINY = 2.0 ** -126 / U
SPECIAL = [0.0, -0.0, 1e-6, -1e-6, 1e-4, -1e-4, 1e-3, -1e-3, 95.0, -95.0]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\nchan_act kernels, worst |restatement - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(REST.items())})
    print('chan_act kernels, worst |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


def bounded(what, got, ref64, rest32, scale):
    key = what.split('[')[0]
    with torch.no_grad():
        r = float(((rest32.double() - ref64).abs() / (U * scale).clamp_min(1e-300)).max())
    REST[key] = max(REST.get(key, 0.0), r)
    assert r < 64.0, (what, r)
    K[key] = max(2.0 * r, 4.0)
    print(f'{what}: restatement {r:.3g}', end='; ')
    within(what, got, ref64, scale)
    print(f'kernel worst so far {RATIOS[key]:.3g}')


def inputs(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 3.0 - 2.0)
    x[:, 0] = x[:, 0].abs() + 1e-3
    x[:, 1] = -x[:, 1].abs() - 1e-3
    sp = torch.tensor(SPECIAL)
    n = min(len(SPECIAL), N - 2)
    idx = (torch.arange(M)[:, None] * n + torch.arange(n)[None, :]) % len(SPECIAL)
    x[:, N - n:] = sp[idx]
    dy = torch.randn(M, N, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 2.0 - 1.0)
    return x, dy


def reference(x, dy, act, dtype):
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    y = F.silu(xr) if act == SILU else F.elu(xr)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, xr.grad.sum(0)


def scales(x, dy, act):
    z, dy = x.double(), dy.double()
    if act == SILU:
        s = torch.sigmoid(z)
        y = z * s
        sdx = dy.abs() * s * (1 + z.abs() * (1 - s)) + TINY
    else:
        y = F.elu(z)
        d = torch.where(z > 0, torch.ones_like(z), torch.exp(z))
        sdx = dy.abs() * d * (1 + torch.where(z > 0, torch.zeros_like(z), z.abs())) + TINY
    return dict(y=z.abs() + y.abs() + TINY, dx=sdx, db=sdx.sum(0))


CASES = ([(M, N, 'pad') for N in (4, 64, 68, 128, 132, 256, 384, 6) for M in (1, 63, 64, 70)]
         + [(70, N, 'pad') for N in (260, 772, 1024, 1028)] + [(70, 64, 'ld_odd'), (70, 128, 'off1'), (32776, 8, 'pad'), (4100, 384, 'pad')])
_refs = {}


def case(M, N, act):
    """inputs, float64 reference, float32 restatement and scales of a shape: computed once, shared, never written"""
    if (M, N, act) not in _refs:
        x, dy = inputs(M, N, 3 * M + N)
        _refs[(M, N, act)] = ((x, dy), reference(x, dy, act, torch.float64), reference(x, dy, act, torch.float32), scales(x, dy, act))
    return _refs[(M, N, act)]


def layout(name, N):
    """-> (ld of x, ld of dy, ld of the outputs, offset in floats)"""
    if name == 'ld_odd':
        return N + 3, N + 5, N + 7, 0
    if name == 'off1':
        return N + 4, N + 8, N + 12, 1
    return N + 4, N + 8, N + 12, 0


def fwd(L, x, M, N, act, lay='pad', P=None, amax=None):
    lx, _, lo, off = layout(lay, N)
    xd = in_buf(x, lx, off)
    ybuf, y = out_buf(M, N, lo, off)
    pl = (P.ptr(), P.ld, P.plane, P.inv_ptr(), amax.data_ptr()) if P is not None else (None, 0, 0, None, None)
    assert L.genrl_chan_act_fwd_h2u(xd.data_ptr(), lx, y.data_ptr(), lo, M, N, act, *pl, stream()) == 0
    torch.cuda.synchronize()
    untouched('chan_act y', ybuf, y)
    return y


def bwd(L, x, dy, M, N, act, lay='pad', P=None, amax=None, db=None, accumulate=0, want_db=True):
    lx, ly, lo, off = layout(lay, N)
    xd, dyd = in_buf(x, lx, off), in_buf(dy, ly, off)
    dbuf, dx = out_buf(M, N, lo, off)
    nws = L.genrl_chan_act_bwd_ws_floats(M, N)
    ws = torch.full((nws + 8,), PAD, device='cuda')
    if want_db:
        bbuf = torch.full((N + 8,), PAD, device='cuda')
        dbv = bbuf[4:4 + N]
        dbv.copy_(db) if db is not None else dbv.fill_(float('nan'))
    pl = (P.ptr(), P.ld, P.plane, P.inv_ptr(), amax.data_ptr()) if P is not None else (None, 0, 0, None, None)
    assert L.genrl_chan_act_bwd_h2u(dyd.data_ptr(), ly, xd.data_ptr(), lx, dx.data_ptr(), lo, dbv.data_ptr() if want_db else None,
                                    ws.data_ptr() if want_db else None, accumulate, M, N, act, *pl, stream()) == 0
    torch.cuda.synchronize()
    untouched('chan_act dx', dbuf, dx)
    assert bool((ws[nws:] == PAD).all()), 'the workspace was overrun'
    if not want_db:
        assert bool((ws == PAD).all())
        return dx, None
    untouched('chan_act db', bbuf, dbv)
    return dx, dbv


@pytest.mark.parametrize('act', sorted(ACTS))
@pytest.mark.parametrize('M,N,lay', CASES)
def test_forward_and_backward_vs_float64(L, M, N, lay, act):
    code = ACTS[act]
    (x, dy), r64, r32, sc = case(M, N, code)
    tag = f'[{M}x{N} {lay}]'
    y = fwd(L, x, M, N, code, lay)
    assert not bool(torch.isnan(y).any())
    bounded(f'{act}.y' + tag, y, r64[0], r32[0], sc['y'])
    dx, db = bwd(L, x, dy, M, N, code, lay)
    assert not bool(torch.isnan(dx).any() | torch.isnan(db).any())
    bounded(f'{act}.dx' + tag, dx, r64[1], r32[1], sc['dx'])
    bounded(f'{act}.db' + tag, db, r64[2], r32[2], sc['db'])
    # two calls: the same bits; without db: the same dx and an untouched workspace
    y2 = fwd(L, x, M, N, code, lay)
    dx2, db2 = bwd(L, x, dy, M, N, code, lay)
    dx3, _ = bwd(L, x, dy, M, N, code, lay, want_db=False)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(db, db2) and torch.equal(dx, dx3)
    # accumulate adds exactly onto a prefilled db
    prior = torch.randn(N, generator=torch.Generator().manual_seed(7)).cuda()
    _, db4 = bwd(L, x, dy, M, N, code, lay, db=prior, accumulate=1)
    assert torch.equal(db4, prior + db)


@pytest.mark.parametrize('act', sorted(ACTS))
def test_special_values(L, act):
    """z = +-0, |z| = 1e-6 .. 1e-3, z = +-95 follow siluf_ / eluf_ of common.h: expm1 semantics, no overflow; a NaN stays a NaN and makes no other"""
    code = ACTS[act]
    z = torch.tensor([SPECIAL + [float('nan'), 0.5]] * 3)
    M, N = z.shape
    y = fwd(L, z, M, N, code).cpu()
    dx, db = bwd(L, z, torch.full_like(z, 3.0), M, N, code)
    dx, db = dx.cpu(), db.cpu()
    z64 = z[:, :10].double()
    if code == ELU:
        want, dwant = torch.where(z64 > 0, z64, torch.expm1(z64)), torch.where(z64 > 0, torch.ones_like(z64), torch.exp(z64))
    else:
        s = torch.sigmoid(z64)
        want, dwant = z64 * s, s * (1 + z64 * (1 - s))
    assert ((y[:, :10].double() - want).abs() <= 6 * U * want.abs() + 2.0 ** -126).all(), y[0]
    assert ((dx[:, :10].double() - 3 * dwant).abs() <= 6 * U * 3 * dwant.abs() + 2.0 ** -126).all(), dx[0]
    assert y[0, 0] == 0 and y[0, 1] == 0 and float(dx[0, 0]) == float(dx[0, 1]) == (3.0 if code == ELU else 1.5)
    assert bool(torch.isfinite(y[:, :10]).all() & torch.isfinite(dx[:, :10]).all())
    assert int(torch.isnan(y).sum()) == 3 and bool(torch.isnan(y[:, 10]).all()) and int(torch.isnan(dx).sum()) == 3
    assert int(torch.isnan(db).sum()) == 1 and bool(torch.isnan(db[10]))


@pytest.mark.parametrize('act', sorted(ACTS))
@pytest.mark.parametrize('M,N', [(1, 4), (64, 64), (70, 68), (63, 132), (300, 256), (70, 384), (70, 1024), (32776, 8)])
def test_uniform_planes_are_the_split_of_the_stored_output(L, M, N, act):
    from genrl_amd import planes, ops_conv_planes as cp
    code = ACTS[act]
    x, dy = inputs(M, N, 3 * M + N)
    for which in ('y', 'dx'):
        P = planes.Planes(M, N, 'cuda', zero=False)
        P.t.fill_(0x3c00)                   # (fp16 1.0 everywhere: the padding columns must be WRITTEN as zeros)
        amax = torch.full((2048 + 4,), PAD, device='cuda')
        if which == 'y':
            out, plain = fwd(L, x, M, N, code, P=P, amax=amax), fwd(L, x, M, N, code)
        else:
            (out, db), (plain, db0) = bwd(L, x, dy, M, N, code, P=P, amax=amax), bwd(L, x, dy, M, N, code)
            assert torch.equal(db, db0)
        assert torch.equal(out, plain) and bool((amax[2048:] == PAD).all())
        oc = out.contiguous()
        ref = cp._uniform_split(oc)
        assert torch.equal(P.inv, ref.inv) and torch.equal(P.t, ref.t)
        assert (P.t[:, :, N:] == 0).all() and (P.inv == P.inv[0]).all()
        m = float(oc.abs().max())
        assert float(P.inv[0]) * 2 ** 14 <= m < float(P.inv[0]) * 2 ** 15
        err = (P.float() - oc).abs()
        assert (err <= 2.0 ** -21 * m).all() and (err <= 2.0 ** -22 * oc.abs() + 2.0 ** -37 * m).all()


def test_refusals_leave_every_output_untouched(L):
    """an unknown activation code (0 included), planes on the scalar arm, planes without inv / amax_ws or narrower than the row, a row spacing
    below N, db without a workspace: status 1 before any launch; M <= 0: status 0 and no launch"""
    from genrl_amd import planes
    M, N = 64, 64
    x = torch.randn(M, N, device='cuda'); dy = torch.randn(M, N, device='cuda')
    y = torch.full((M, N), PAD, device='cuda'); dx = torch.full((M, N), PAD, device='cuda'); db = torch.full((N,), PAD, device='cuda')
    ws = torch.full((L.genrl_chan_act_bwd_ws_floats(M, N),), PAD, device='cuda'); amax = torch.full((2048,), PAD, device='cuda')
    P = planes.Planes(M, N, 'cuda')
    t0, i0 = P.t.clone(), P.inv.clone()
    pl = (P.ptr(), P.ld, P.plane, P.inv_ptr(), amax.data_ptr())
    none = (None, 0, 0, None, None)
    s = stream()
    f = lambda *, ldx=N, ldy=N, m=M, n=N, act=SILU, p=none, xp=x.data_ptr(): L.genrl_chan_act_fwd_h2u(xp, ldx, y.data_ptr(), ldy, m, n, act, *p, s)
    b = lambda *, lddy=N, ldx=N, lddx=N, m=M, n=N, act=SILU, p=none, dbp=db.data_ptr(), wsp=ws.data_ptr(), xp=x.data_ptr(): \
        L.genrl_chan_act_bwd_h2u(dy.data_ptr(), lddy, xp, ldx, dx.data_ptr(), lddx, dbp, wsp, 0, m, n, act, *p, s)
    for code in (0, 3, -1):
        assert f(act=code) == EINVAL and f(act=code, p=pl) == EINVAL and b(act=code) == EINVAL and b(act=code, p=pl) == EINVAL
        assert f(act=code, m=0) == EINVAL and b(act=code, m=0) == EINVAL
    for m in (0, -5):
        assert f(m=m, p=pl) == 0 and b(m=m, p=pl) == 0
    # planes on the scalar arm: N % 4, a row spacing that is no multiple of 4, a base pointer one float off
    assert f(n=62, p=pl) == EINVAL and b(n=62, p=pl) == EINVAL
    assert f(n=60, ldx=62, p=pl) == EINVAL and b(n=60, lddx=62, p=pl) == EINVAL
    assert f(n=60, xp=x.data_ptr() + 4, p=pl) == EINVAL and b(n=60, xp=x.data_ptr() + 4, p=pl) == EINVAL
    assert f(n=1028, ldx=1028, ldy=1028, m=2, p=pl) == EINVAL
    # incomplete plane arguments
    assert f(p=(P.ptr(), P.ld, P.plane, None, amax.data_ptr())) == EINVAL and f(p=(P.ptr(), P.ld, P.plane, P.inv_ptr(), None)) == EINVAL
    assert f(p=(P.ptr(), 32, P.plane, P.inv_ptr(), amax.data_ptr())) == EINVAL and f(p=(P.ptr(), 66, P.plane, P.inv_ptr(), amax.data_ptr())) == EINVAL
    assert b(p=(P.ptr(), P.ld, P.plane, None, amax.data_ptr())) == EINVAL and b(p=(P.ptr(), P.ld, P.plane, P.inv_ptr(), None)) == EINVAL
    # shapes
    assert f(n=0) == EINVAL and f(ldx=60) == EINVAL and f(ldy=60) == EINVAL and b(n=0) == EINVAL and b(lddy=60) == EINVAL and b(lddx=60) == EINVAL
    assert b(wsp=None) == EINVAL
    torch.cuda.synchronize()
    for t in (y, dx, db, ws, amax):
        assert bool((t == PAD).all())
    assert torch.equal(P.t, t0) and torch.equal(P.inv, i0)
