"""The kernels of the DreamerV2 defaults (csrc/rowact.hip, heads.hip, vecobs.hip) and the dense_act nodes built on them, against float64.

SiLU pair and truncated-normal head: |kernel - float64| <= max(2 x the worst ratio of the float32 CPU restatement of the same formula
(tests/v2_restatement.py, autograd for the backward), FLOOR) x 2^-24 x scale per element, the bound of test_gpu_ensemble_kernels.py.  scale
is the float64 magnitude of the terms the element is made of; FLOOR counts the roundings of the formula in fp32: expf within 1 ulp and tanhf
within 2 ulp (the device library's documented accuracy), half an ulp per following operation -- 4 for y = x / (1 + e^-x) (1 + 3 x 0.5), 8 for
the chains with two such factors (silu', tanh + sigmoid x eps).  A result below fp32's smallest normal number may flush: 2^-126 is added to
the allowed error (x = -100 gives -0 where float64 has -3.7e-42).  Planes must equal planes.split of the stored fp32 output bit for bit.
dense_act: the bounds of test_gpu_plane_variants.py / test_gpu_gemm_variants.py for the product of the route, K 2^-24 sum |a| |b| (+ the h2
floor) with K = 150 (the largest of the plane tile families) / 100 (the largest fp32-operand family that M <= 200 rows can reach), carried
through the SiLU and the chain rule in float64 (see dense_bounds)."""
import pytest
import torch

import v2_restatement as R
from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

K, RATIOS = {}, {}
within = checker(K, RATIOS)
FACTOR = 2.0
TINY = 2.0 ** -126 / U           # (scale units: U x TINY = the smallest normal fp32 number)
SPECIAL = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\nv2 kernels, largest |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


def bounded(what, got, ref64, rest32, scale, floor):
    key = what.split('[')[0]
    rest = float(((rest32.double() - ref64).abs() / (U * scale)).max())
    K[key] = max(FACTOR * rest, floor)
    within(what, got, ref64, scale)


def planes_equal_split(P, y):
    from genrl_amd import planes
    Q = planes.split(y.contiguous())
    assert torch.equal(P.t, Q.t) and torch.equal(P.inv, Q.inv)


def silu_inputs(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 3.0 - 2.0)
    x.view(-1)[:len(SPECIAL)] = torch.tensor(SPECIAL)[:M * N]
    dy = torch.randn(M, N, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 4.0 - 2.0)
    return x, dy


@pytest.mark.parametrize('N', [4, 36, 1028, 12288])
@pytest.mark.parametrize('M', [1, 3, 2049])
def test_silu_pair_vs_float64_and_planes(L, M, N):
    from genrl_amd import planes
    from genrl_amd._lib import check
    x, dy = silu_inputs(M, N, 1 + M + N)
    x64, dy64 = x.double(), dy.double()
    sg = torch.sigmoid(x64)
    y64, d64 = x64 * sg, dy64 * R.silu_grad(x64)
    xr = x.clone().requires_grad_(True)
    y32 = torch.nn.functional.silu(xr)
    y32.backward(dy)
    xd, dyd = in_buf(x, N + 4), in_buf(dy, N + 8)
    ybuf, y = out_buf(M, N, N + 12)
    P = planes.Planes(M, N, 'cuda')
    check(L.genrl_silu_fwd_h2(xd.data_ptr(), N + 4, y.data_ptr(), N + 12, M, N, P.ptr(), P.ld, P.plane, P.inv_ptr(), stream()), 'silu_fwd')
    untouched('silu y', ybuf, y)
    assert not bool(torch.isnan(y).any())
    bounded(f'silu.fwd[{M}x{N}]', y, y64, y32.detach(), y64.abs() + TINY, 4.0)
    planes_equal_split(P, y)
    dbuf, dx = out_buf(M, N, N + 4)
    Pd = planes.Planes(M, N, 'cuda')
    check(L.genrl_silu_bwd_h2(dyd.data_ptr(), N + 8, xd.data_ptr(), N + 4, dx.data_ptr(), N + 4, M, N, Pd.ptr(), Pd.ld, Pd.plane,
                              Pd.inv_ptr(), stream()), 'silu_bwd')
    untouched('silu dx', dbuf, dx)
    assert not bool(torch.isnan(dx).any())
    bounded(f'silu.bwd[{M}x{N}]', dx, d64, xr.grad, dy64.abs() * sg * (1 + x64.abs() * (1 - sg)) + TINY, 8.0)
    planes_equal_split(Pd, dx)
    # the special inputs: no NaN, x = -100 gives -0 or a tiny negative, +-0 gives 0
    flat = y.reshape(-1)[:min(len(SPECIAL), M * N)].cpu()
    if M * N >= len(SPECIAL):
        assert float(flat[7]) <= 0.0 and float(flat[7]) > -1e-37 and float(flat[6]) == 100.0 and float(flat[0]) == 0.0 and float(flat[1]) == 0.0
    # in place, without planes: the same bits
    z = x.cuda().contiguous()
    check(L.genrl_silu_fwd_h2(z.data_ptr(), N, z.data_ptr(), N, M, N, None, 0, 0, None, stream()), 'silu_fwd')
    assert torch.equal(z, y)
    gz = dy.cuda().contiguous()
    check(L.genrl_silu_bwd_h2(gz.data_ptr(), N, x.cuda().contiguous().data_ptr(), N, gz.data_ptr(), N, M, N, None, 0, 0, None, stream()), 'silu_bwd')
    assert torch.equal(gz, dx)


def test_silu_nan_stays_nan_and_bad_shapes_are_refused(L):
    x = torch.zeros(4, 8, device='cuda')
    x[1, 2] = float('nan')
    y = torch.empty_like(x)
    assert L.genrl_silu_fwd_h2(x.data_ptr(), 8, y.data_ptr(), 8, 4, 8, None, 0, 0, None, stream()) == 0
    assert bool(torch.isnan(y[1, 2])) and int(torch.isnan(y).sum()) == 1
    assert L.genrl_silu_fwd_h2(x.data_ptr(), 8, y.data_ptr(), 8, 4, 6, None, 0, 0, None, stream()) == 1        # N % 4
    assert L.genrl_silu_fwd_h2(x.data_ptr(), 6, y.data_ptr(), 8, 4, 8, None, 0, 0, None, stream()) == 1        # pitch
    assert L.genrl_silu_bwd_h2(x.data_ptr(), 8, x.data_ptr(), 8, y.data_ptr(), 4, 4, 8, None, 0, 0, None, stream()) == 1
    with pytest.raises(Exception):
        from genrl_amd import ops
        ops.dense_act(torch.zeros(4, 8), None, torch.zeros(8, 8))                # no CPU fallback


@pytest.mark.parametrize('A', [1, 6, 7])
@pytest.mark.parametrize('rows', [1, 65, 4099])
def test_trunc_normal_head_vs_float64(L, rows, A):
    from genrl_amd import ops
    g = torch.Generator().manual_seed(10 * rows + A)
    raw = torch.randn(rows, 2 * A, generator=g) * 1.5
    eps = torch.randn(rows, A, generator=g) * 1.5            # (std ~ 1.1: about a fifth of the elements leaves [-1, 1] on each side)
    if rows == 1 and A == 1:
        raw, eps = torch.tensor([[0.3, 0.2]]), torch.tensor([[2.0]])
    dact = torch.randn(rows, A, generator=g)
    MIN, INIT = 0.1, 0.0

    def restate(dtype):
        r = raw.to(dtype).clone().requires_grad_(True)
        a, mean, std, x = R.trunc_normal(r[:, :A], r[:, A:], eps.to(dtype), MIN, INIT)
        (a * dact.to(dtype)).sum().backward()
        return a.detach(), mean.detach(), std.detach(), x.detach(), r.grad
    a64, m64, s64, x64, g64 = restate(torch.float64)
    a32, m32, s32, _, g32 = restate(torch.float32)
    lo, hi = float((x64 < -1).double().mean()), float((x64 > 1).double().mean())
    if rows > 1:
        assert lo >= 0.1 and hi >= 0.1, (lo, hi)            # the clamp branch is taken on both sides, on the float64 reference itself
    else:
        assert lo + hi > 0
    rd, ed = raw.cuda().requires_grad_(True), eps.cuda()
    act = ops.trunc_normal_sample(rd, ed, MIN, INIT)
    mean, std = ops.trunc_normal_mean_std(rd, MIN, INIT)
    (act * dact.cuda()).sum().backward()
    r64, e64 = raw.double(), eps.double()
    bounded(f'tn.mean[{rows}x{A}]', mean, m64, m32, r64[:, :A].abs() + m64.abs(), 4.0)
    bounded(f'tn.std[{rows}x{A}]', std, s64, s32, r64[:, A:].abs() + s64, 4.0)
    bounded(f'tn.action[{rows}x{A}]', act, a64, a32, m64.abs() + e64.abs() * s64, 8.0)
    assert float(act.detach().abs().max()) <= float(torch.tensor(1 - 1e-6, dtype=torch.float32))
    # the gradient on clamped elements is the unclamped formula's (the float64 reference is the straight-through expression itself)
    sgm = torch.sigmoid((r64[:, A:] + INIT) / 2)
    formula = torch.cat([dact.double() * (1 - m64 ** 2), dact.double() * e64 * sgm * (1 - sgm)], 1)
    assert torch.allclose(formula, g64, rtol=1e-9, atol=1e-12)            # (two float64 evaluations of one expression)
    scale = torch.cat([dact.double().abs() * (1 + m64 ** 2), (dact.double() * e64).abs() * sgm * (1 + sgm)], 1) + TINY
    bounded(f'tn.draw[{rows}x{A}]', rd.grad, g64, g32, scale, 8.0)
    clamped = ((x64 < -1) | (x64 > 1))
    assert bool((rd.grad.cpu()[:, :A][clamped] != 0).any()) or not bool(clamped.any())


def dense_bounds(x, x2, W, dy, Kc, on_planes):
    """float64 reference of y = SiLU([x, x2] W^T) and its gradients for upstream dy, with per-element error bounds: a product's own
    Kc 2^-24 sum |a| |b| (+ the h2 floor of test_gpu_plane_variants.py, 2^-36 (inv_a sum |b| + inv_b sum |a|) with inv <= 2^-14 max|row|),
    the SiLU kernels' 8 x 2^-24 on their own terms, and each operand's error carried through the next product in absolute value
    (|silu'| <= 1.1, |silu''| <= 0.5)."""
    xa = (torch.cat([x, x2], -1) if x2 is not None else x).double()
    Wd, dyd = W.double(), dy.double()

    def prod_err(a, b, ea=None):            # error bound of a @ b^T computed on operands a (error ea), b exact
        e = Kc * U * (a.abs() @ b.abs().t())
        if on_planes:
            e = e + 2.0 ** -50 * (a.abs().amax(1, keepdim=True) * b.abs().sum(1)[None] + a.abs().sum(1, keepdim=True) * b.abs().amax(1)[None])
        return e + (ea @ b.abs().t() if ea is not None else 0)
    pre = xa @ Wd.t()
    e_pre = prod_err(xa, Wd)
    sg = torch.sigmoid(pre)
    y = pre * sg
    e_y = 1.1 * e_pre + 4 * U * y.abs() + U * TINY
    ds = R.silu_grad(pre)
    dpre = dyd * ds
    e_dpre = dyd.abs() * 0.5 * e_pre + 8 * U * dyd.abs() * sg * (1 + pre.abs() * (1 - sg)) + U * TINY
    dx = dpre @ Wd
    e_dx = prod_err(dpre, Wd.t(), e_dpre)
    dW = dpre.t() @ xa
    e_dW = prod_err(dpre.t(), xa.t(), e_dpre.t())
    return (y, e_y), (dx, e_dx), (dW, e_dW)


def close_to(what, got, ref, err):
    got = got.detach().cpu().double()
    bad = ~((got - ref).abs() <= err)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} out of bound; worst error / bound {float(((got - ref).abs() / err.clamp_min(1e-300)).max()):.3g}'
    return float(((got - ref).abs() / err.clamp_min(1e-300)).max())


@pytest.mark.parametrize('second', [False, True])
@pytest.mark.parametrize('N', [32, 512])
@pytest.mark.parametrize('Kd', [48, 1030])
@pytest.mark.parametrize('rows', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('route', ['planes', 'fp32'])
def test_dense_act_vs_float64(route, rows, Kd, N, second):
    from genrl_amd import ops, ops_planes, planes
    ops.set_gemm_precision(ops.F32_MODE)
    g = torch.Generator().manual_seed(rows + Kd + N + second)
    K2 = 6 if second else 0
    K1 = Kd - K2
    x = torch.randn(rows, K1, generator=g)
    x2 = (torch.rand(rows, K2, generator=g) * 2 - 1) if second else None
    W = torch.randn(N, Kd, generator=g) / Kd ** 0.5
    dy = torch.randn(rows, N, generator=g)
    on_planes = route == 'planes'
    (y64, e_y), (dx64, e_dx), (dW64, e_dW) = dense_bounds(x, x2, W, dy, 150.0 if on_planes else 100.0, on_planes)
    xd = x.cuda().requires_grad_(True)
    x2d = x2.cuda().requires_grad_(True) if second else None
    Wp = torch.nn.Parameter(W.cuda())
    calls = []
    og = planes.gemm
    planes.gemm = lambda *a, **k: (calls.append(1), og(*a, **k))[1]
    try:
        y = ops_planes.dense_act(xd, x2d, Wp) if on_planes else ops.dense_act(xd, x2d, Wp)
        y.backward(dy.cuda())
    finally:
        planes.gemm = og
    assert len(calls) == ((3 if second else 2) if on_planes else 0), calls
    if on_planes:
        planes_equal_split(y._planes[0], y.detach())
    r = [close_to('y', y, y64, e_y), close_to('dx1', xd.grad, dx64[:, :K1], e_dx[:, :K1]), close_to('dW', Wp.grad, dW64, e_dW)]
    if second:
        r.append(close_to('dx2', x2d.grad, dx64[:, K1:], e_dx[:, K1:]))
    RATIOS[f'dense_act.{route}'] = max(RATIOS.get(f'dense_act.{route}', 0.0), max(r))


def test_sqerr_head_vs_float64():
    from genrl_amd import ops
    g = torch.Generator().manual_seed(4)
    out, x, w = torch.randn(17, 301, 1, generator=g), torch.randn(17, 301, 1, generator=g), torch.randn(17, 301, generator=g)
    od = out.cuda().requires_grad_(True)
    like = ops.sqerr_like(od, x.cuda())
    (like * w.cuda()).sum().backward()
    o64 = out.double().requires_grad_(True)
    l64 = R.mse_log_prob(o64, x.double())
    (l64 * w.double()).sum().backward()
    assert like.shape == (17, 301)
    K['sqerr'] = 4.0        # (a subtraction, a product, a negation / scaling: at most 2 ulp of the terms)
    within('sqerr[like]', like, l64.detach(), (out.double().abs() + x.double().abs()).squeeze(-1) ** 2, key='sqerr')
    within('sqerr[grad]', od.grad, o64.grad, 2 * (out.double().abs() + x.double().abs()) * w.double().abs()[..., None], key='sqerr')
