"""The row kernels of the Plan2Explore ensemble (csrc/ensemble.hip, the ReLU of csrc/rowact.hip) through their C entry points, with padded row pitches.

ReLU forward / backward: bit-identical to torch, planes bit-identical to planes.split of the fp32 output.
l2err and ens_var, forward and backward: error against float64, bounded per case by 2x the error the float32 CPU restatement of the
same formula (plain torch, autograd for the backward) makes against float64 on the same inputs, with a floor of 4 units of 2^-24 x
scale (scale: the magnitude of the row's result).  The factor 2 covers the different summation order; the yardstick is the
restatement, never the kernel.  The measured ratios (in units of 2^-24 x scale) are recorded in RATIOS and printed.
Outputs are NaN-prefilled inside PAD-filled buffers with a guard row: a kernel that skips an element or writes outside fails."""
import pytest
import torch

from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

MS, NS, KS = [1, 37, 192, 1000], [128, 1540, 6144, 12288], [2, 5]
K = {}                  # bound per quantity, set per case from the restatement's own error (see the module docstring)
RATIOS = {}
within = checker(K, RATIOS)
FLOOR, FACTOR = 4.0, 2.0


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\nensemble kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


def rows(M, N, seed, spread=True):
    """rows whose magnitudes span 1e-3 .. 1e3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g)
    if spread:
        x = x * torch.pow(10.0, torch.rand(M, 1, generator=g) * 5.0 - 2.5)
    return x.clamp(-1e3, 1e3)


def vec_out(n):
    buf = torch.full((n + 4,), PAD, device='cuda')
    buf[:n] = float('nan')
    return buf, buf[:n]


def bounded(what, got, ref64, rest32, scale):
    """|got - ref64| <= max(FACTOR x the restatement's worst ratio, FLOOR) x 2^-24 scale, elementwise"""
    key = what.split('[')[0]
    live = scale > 0                       # (an element of scale 0 -- an exactly-zero result -- must come out exactly: `within` below)
    rest = float(((rest32.double() - ref64).abs()[live] / (U * scale[live])).max()) if bool(live.any()) else 0.0
    K[key] = max(FACTOR * rest, FLOOR)
    print(f'{what}: restatement ratio {rest:.3g}, bound {K[key]:.3g}', end='; ')
    within(what, got, ref64, scale)
    print(f'worst kernel ratio so far {RATIOS[key]:.3g}')


def planes_equal_split(P, y):
    from genrl_amd import planes
    Q = planes.split(y.contiguous())
    assert torch.equal(P.t, Q.t) and torch.equal(P.inv, Q.inv)


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('M', MS)
def test_relu_bit_identical_and_planes(L, M, N):
    from genrl_amd import planes
    from genrl_amd._lib import check
    x = rows(M, N, 1 + M + N)
    x[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    dy = rows(M, N, 2 + M + N)
    xd, dyd = in_buf(x, N + 4), in_buf(dy, N + 8)
    ybuf, y = out_buf(M, N, N + 12)
    P = planes.Planes(M, N, 'cuda')
    check(L.genrl_relu_fwd_h2(xd.data_ptr(), N + 4, y.data_ptr(), N + 12, M, N, P.ptr(), P.ld, P.plane, P.inv_ptr(), stream()), 'relu_fwd')
    xt = x.cuda().requires_grad_(True)
    yt = torch.relu(xt)
    assert torch.equal(y, yt.detach())
    untouched('relu y', ybuf, y)
    planes_equal_split(P, y)
    dbuf, dx = out_buf(M, N, N + 4)
    Pd = planes.Planes(M, N, 'cuda')
    check(L.genrl_relu_bwd_h2(dyd.data_ptr(), N + 8, y.data_ptr(), N + 12, dx.data_ptr(), N + 4, M, N, Pd.ptr(), Pd.ld, Pd.plane,
                              Pd.inv_ptr(), stream()), 'relu_bwd')
    yt.backward(dy.cuda())
    assert torch.equal(dx, xt.grad)
    untouched('relu dx', dbuf, dx)
    planes_equal_split(Pd, dx)
    # without planes, in place
    z = x.cuda().contiguous()
    check(L.genrl_relu_fwd_h2(z.data_ptr(), N, z.data_ptr(), N, M, N, None, 0, 0, None, stream()), 'relu_fwd')
    assert torch.equal(z, yt.detach())


def test_relu_rejects_bad_shapes(L):
    x = torch.zeros(4, 8, device='cuda')
    assert L.genrl_relu_fwd_h2(x.data_ptr(), 8, x.data_ptr(), 8, 4, 6, None, 0, 0, None, stream()) == 1        # N % 4
    assert L.genrl_relu_fwd_h2(x.data_ptr(), 6, x.data_ptr(), 8, 4, 8, None, 0, 0, None, stream()) == 1        # pitch
    assert L.genrl_ens_var_fwd(x.data_ptr(), 32, 8, 9, x.data_ptr(), 1, 8, stream()) == 1                      # K > 8
    assert L.genrl_ens_var_fwd(x.data_ptr(), 32, 8, 1, x.data_ptr(), 1, 8, stream()) == 1                      # K < 2


def l2_restatement(t, p, g, dtype):
    t, p, g = t.to(dtype), p.to(dtype).clone().requires_grad_(True), g.to(dtype)
    err = torch.norm(t - p, dim=-1, p=2)
    err.backward(g)
    return err.detach(), p.grad


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('M', MS)
def test_l2err_vs_float64(L, M, N):
    from genrl_amd import planes
    from genrl_amd._lib import check
    t, p = rows(M, N, 3 + M + N), rows(M, N, 4 + M + N)
    if M > 2:
        p[2] = t[2]                                    # a row with p == t: err 0, dp 0, no NaN
    g = rows(M, 1, 5 + M + N, spread=False)[:, 0]
    e64, d64 = l2_restatement(t, p, g, torch.float64)
    e32, d32 = l2_restatement(t, p, g, torch.float32)
    td, pd = in_buf(t, N + 4), in_buf(p, N + 8)
    ebuf, err = vec_out(M)
    check(L.genrl_l2err_fwd(td.data_ptr(), N + 4, pd.data_ptr(), N + 8, err.data_ptr(), M, N, stream()), 'l2err_fwd')
    bounded(f'l2err.fwd[{M}x{N}]', err, e64, e32, e64.abs())
    assert torch.equal(ebuf[M:], torch.full_like(ebuf[M:], PAD))
    dbuf, dp = out_buf(M, N, N + 4)
    P = planes.Planes(M, N, 'cuda')
    gd = g.cuda()
    check(L.genrl_l2err_bwd(gd.data_ptr(), err.data_ptr(), td.data_ptr(), N + 4, pd.data_ptr(), N + 8, dp.data_ptr(), N + 4, M, N,
                            P.ptr(), P.ld, P.plane, P.inv_ptr(), stream()), 'l2err_bwd')
    untouched('l2err dp', dbuf, dp)
    scale = d64.abs().amax(1, keepdim=True).expand_as(d64)
    bounded(f'l2err.bwd[{M}x{N}]', dp, d64, d32, scale)
    planes_equal_split(P, dp)
    if M > 2:
        assert float(err[2]) == 0.0 and float(dp[2].abs().max()) == 0.0 and float(d64[2].abs().max()) == 0.0


def var_restatement(p, g, dtype):
    p, g = p.to(dtype).clone().requires_grad_(True), g.to(dtype)
    r = torch.var(p, dim=0).mean(dim=-1)
    r.backward(g)
    return r.detach(), p.grad


@pytest.mark.parametrize('Kn', KS)
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('M', MS)
def test_ens_var_vs_float64(L, M, N, Kn):
    from genrl_amd import planes
    from genrl_amd._lib import check
    base = rows(M, N, 6 + M + N)
    p = base[None] + torch.stack([rows(M, N, 7 + M + N + k) for k in range(Kn)]) * 0.3
    if M > 2:
        p[:, 2] = base[2]                              # identical members: variance exactly 0 and zero gradient
    p = p.clamp(-1e3, 1e3)
    g = rows(M, 1, 8 + M + N, spread=False)[:, 0]
    r64, d64 = var_restatement(p, g, torch.float64)
    r32, d32 = var_restatement(p, g, torch.float32)
    ld = N + 4
    member = (M + 1) * ld                              # members apart by a guard row
    pbuf = torch.full((Kn * member + 4,), float('nan'), device='cuda')
    pv = pbuf[:Kn * member].view(Kn, M + 1, ld)[:, :M, :N]
    pv.copy_(p)
    rbuf, r = vec_out(M)
    check(L.genrl_ens_var_fwd(pbuf.data_ptr(), member, ld, Kn, r.data_ptr(), M, N, stream()), 'ens_var_fwd')
    bounded(f'ens_var.fwd[{M}x{N}x{Kn}]', r, r64, r32, r64.abs())
    assert torch.equal(rbuf[M:], torch.full_like(rbuf[M:], PAD))
    dbuf = torch.full((Kn * member + 4,), PAD, device='cuda')
    dv = dbuf[:Kn * member].view(Kn, M + 1, ld)[:, :M, :N]
    dv.fill_(float('nan'))
    P = planes.Planes(Kn * M, N, 'cuda')
    gd = g.cuda()
    check(L.genrl_ens_var_bwd(gd.data_ptr(), pbuf.data_ptr(), member, ld, Kn, dbuf.data_ptr(), member, ld, M, N,
                              P.ptr(), M * P.ld, P.ld, P.plane, P.inv_ptr(), M, stream()), 'ens_var_bwd')
    dp = dv.clone()
    dv.fill_(PAD)
    assert torch.equal(dbuf, torch.full_like(dbuf, PAD)), 'ens_var_bwd wrote outside its output'
    scale = d64.abs().amax(2, keepdim=True).expand_as(d64)
    bounded(f'ens_var.bwd[{M}x{N}x{Kn}]', dp, d64, d32, scale)
    planes_equal_split(P, dp.reshape(Kn * M, N))
    # planes only (dp NULL) gives the same planes; g NULL means g = 1
    P2 = planes.Planes(Kn * M, N, 'cuda')
    check(L.genrl_ens_var_bwd(gd.data_ptr(), pbuf.data_ptr(), member, ld, Kn, None, 0, 0, M, N,
                              P2.ptr(), M * P2.ld, P2.ld, P2.plane, P2.inv_ptr(), M, stream()), 'ens_var_bwd')
    assert torch.equal(P.t, P2.t) and torch.equal(P.inv, P2.inv)
    if M > 2:
        assert float(r[2]) == 0.0 and float(dp[:, 2].abs().max()) == 0.0


def test_op_layer_functions_match_torch():
    """ops.relu / ops.l2err / ops.ens_var as autograd nodes (contiguous operands)"""
    from genrl_amd import ops
    x = rows(50, 256, 11).cuda().requires_grad_(True)
    t = rows(50, 256, 12).cuda()
    y = ops.relu(x)
    e = ops.l2err(t, y)
    e.sum().backward()
    x2 = x.detach().clone().requires_grad_(True)
    torch.norm(t - torch.relu(x2), dim=-1).sum().backward()
    assert torch.equal(y.detach(), torch.relu(x2).detach())
    assert torch.allclose(x.grad, x2.grad, rtol=1e-5, atol=1e-7)
    # the variance against float64 (torch's own float32 variance loses the deviations of members a few ulps apart: no yardstick)
    pc = rows(15, 256, 14, spread=False).reshape(5, 3, 256)
    p = pc.cuda().requires_grad_(True)
    r = ops.ens_var(p)
    r.sum().backward()
    p2 = pc.double().requires_grad_(True)
    r2 = torch.var(p2, 0).mean(-1)
    r2.sum().backward()
    assert torch.allclose(r.detach().cpu().double(), r2.detach(), rtol=1e-5)
    assert torch.allclose(p.grad.cpu().double(), p2.grad, rtol=1e-5, atol=1e-6 * float(p2.grad.abs().max()))
    with pytest.raises(Exception):
        ops.relu(torch.zeros(4, 8))                    # no CPU fallback
