"""`act = 2` (ELU, torch.nn.ELU with alpha 1) in the C entries that take an activation code -- genrl_ln_act_{fwd,bwd}, _h2, _h2u and
genrl_gemm_h2_ln -- and the stand-alone pair genrl_elu_{fwd,bwd}_h2 (csrc/rowact.hip), against float64.

Bound, per quantity and case (the convention of test_gpu_ensemble_kernels.py): |kernel - float64| <= max(2 r, 4) 2^-24 scale per element,
where r is the worst ratio the float32 plain-torch CPU restatement of the same function (F.elu(F.layer_norm(...)), autograd for the
backward) reaches against float64 on the same inputs, and scale is the float64 magnitude of the terms the element is made of: for a
LayerNorm output |gamma| (|x^| + rstd mean|x|) + |beta| (the terms of z) + |y|; for the backward |dy| elu'(z) (1 + the terms of z where
z <= 0: exp(z) carries z's rounding) through the same sums as the values; column sums: the sum of the rows' scales.  The yardstick is the
restatement, never the kernel, and the inputs are mild enough that the restatement itself stays below 64 on every quantity (asserted).

Inputs: rows of spread e^(0.5 n) around small means, row 1 constant (zero variance); gamma ~ 1, beta ~ 0.3, so that the normalised
pre-activation z = gamma x^ + beta has both signs in every row; the last eleven columns have gamma = 0 and beta = the special values, so
that EVERY row holds z = 0 exactly, |z| = 1e-6, 1e-4, 1e-3 in both signs (expm1, not exp - 1), z = -95 and z = +95, and -0.0.
The shapes are the smallest at which each instantiation of csrc/rowops.hip is selected (test_gpu_row_kernel_variants.py's boundaries)."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_row_kernel_variants as RK
from f64check import PAD, U, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

ELU, EINVAL = 2, 1
EPS = 1e-3
K, RATIOS, REST = {}, {}, {}
within = checker(K, RATIOS)
TINY = 2.0 ** -126 / U           # (scale units: U x TINY = the smallest normal fp32 number)
SPECIAL_Z = [0.0, -0.0, 1e-6, -1e-6, 1e-4, -1e-4, 1e-3, -1e-3, -95.0, 95.0, -2e-5]
stream = RK.stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    yield lib()
    print('\nELU kernels, worst |restatement - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(REST.items())})
    print('ELU kernels, worst |kernel - float64| / (2^-24 scale):', {k: round(v, 3) for k, v in sorted(RATIOS.items())})


def bounded(what, got, ref64, rest32, scale):
    """max(2 r, 4) with r the restatement's own worst ratio on this case; r < 64 (mild inputs)"""
    key = what.split('[')[0]
    with torch.no_grad():
        r = float(((rest32.double() - ref64).abs() / (U * scale).clamp_min(1e-300)).max())
    REST[key] = max(REST.get(key, 0.0), r)
    assert r < 64.0, (what, r)
    K[key] = max(2.0 * r, 4.0)
    print(f'{what}: restatement {r:.3g}', end='; ')
    within(what, got, ref64, scale)
    print(f'kernel worst so far {RATIOS[key]:.3g}')


def ln_inputs(M, N, seed):
    g = RK.gen(seed)
    x = torch.randn(M, N, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g)) + 0.3 * torch.randn(M, 1, generator=g)
    if M >= 3:
        x[1] = 3.7
    gamma = 1 + 0.3 * torch.randn(N, generator=g)
    beta = 0.3 * torch.randn(N, generator=g)
    n = len(SPECIAL_Z)
    gamma[N - n:] = 0.0
    beta[N - n:] = torch.tensor(SPECIAL_Z)
    dy = torch.randn(M, N, generator=g)
    return x, gamma, beta, dy


def reference(x, gamma, beta, dy, dtype):
    """y = elu(layer_norm(x) gamma + beta) and its gradients by autograd in `dtype`; -> y, mean, rstd, dx, dgamma, dbeta, colsum(dx)"""
    xr, gr, br = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))          # (fresh leaves: the inputs are shared)
    y = F.elu(F.layer_norm(xr, (x.shape[1],), gr, br, EPS))
    y.backward(dy.to(dtype))
    mean = xr.detach().mean(1)
    rstd = 1.0 / torch.sqrt(((xr.detach() - mean[:, None]) ** 2).mean(1) + EPS)
    return y.detach(), mean, rstd, xr.grad, gr.grad, br.grad, xr.grad.sum(0)


def scales(x, gamma, beta, dy):
    x = x.double(); ga = gamma.double(); be = beta.double(); dy = dy.double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)
    xh = (x - mean) * rstd
    mabs = x.abs().mean(1, keepdim=True)
    z = xh * ga + be
    sz = ga.abs() * (xh.abs() + rstd * mabs) + be.abs()
    sy = sz + F.elu(z).abs()
    d = torch.where(z > 0, torch.ones_like(z), torch.exp(z))
    sdz = dy.abs() * d * (1 + torch.where(z > 0, torch.zeros_like(z), sz)) + TINY
    t = sdz * ga.abs()
    sdx = rstd * (t + t.mean(1, keepdim=True) + xh.abs() * (t * xh.abs()).mean(1, keepdim=True)) + TINY
    return dict(y=sy, mean=mabs[:, 0], rstd=rstd[:, 0], dx=sdx, dgamma=(sdz * (xh.abs() + 1)).sum(0), dbeta=sdz.sum(0), dcolsum=sdx.sum(0))


# (M, N, layout): narrow lane groups GL 16 / 32 / 64, wave NV 2..4 on both sides of a workgroup's 64 rows, block NV 2..4, the generic path
# (M < 64 at N <= 256, N % 4 != 0, N > 4096), lines that are no multiple of 4 floats apart, base pointers one float off, and one backward
# with more than one row per workgroup
CASES = ([(100, N, 'pad') for N in (64, 68, 132, 256)] + [(M, N, 'pad') for N in (260, 512, 772, 1024) for M in (63, 64)]
         + [(63, N, 'pad') for N in (1028, 2048, 3076, 4096)] + [(40, 200, 'pad'), (300, 255, 'pad'), (70, 6000, 'pad')]
         + [(300, 512, 'ld_odd'), (300, 128, 'off1'), (2100, 512, 'pad')])
_refs = {}


def case(M, N):
    """inputs, float64 reference, float32 restatement and scales of a shape: computed once, shared, never written"""
    if (M, N) not in _refs:
        inp = ln_inputs(M, N, 3 * M + N)
        _refs[(M, N)] = (inp, reference(*inp, torch.float64), reference(*inp, torch.float32), scales(*inp))
    return _refs[(M, N)]


@pytest.mark.parametrize('M,N,layout', CASES)
def test_layernorm_elu_forward_and_backward_vs_float64(L, M, N, layout):
    (x, gamma, beta, dy), r64, r32, sc = case(M, N)
    tag = f'[{M}x{N} {layout}]'
    y, mean, rstd = RK._ln_fwd(L, x, gamma, beta, M, N, EPS, ELU, layout)
    assert not bool(torch.isnan(y).any())
    bounded('elu_ln.y' + tag, y, r64[0], r32[0], sc['y'])
    bounded('elu_ln.mean' + tag, mean, r64[1], r32[1], sc['mean'])
    bounded('elu_ln.rstd' + tag, rstd, r64[2], r32[2], sc['rstd'])
    # the special columns: z = beta exactly in every row
    n = len(SPECIAL_Z)
    ys = y[:, N - n:].cpu()
    want = torch.tensor([0.0, 0.0, 1e-6, -1e-6, 1e-4, -1e-4, 1e-3, -1e-3, -1.0, 95.0, -2e-5], dtype=torch.float64)
    want = torch.where(want < 0, torch.expm1(torch.tensor(SPECIAL_Z, dtype=torch.float32).double()), want)
    assert ((ys.double() - want).abs() <= 6 * U * want.abs()).all(), ys[0]          # (expm1f: 1 ulp; exp(z) - 1 would miss by 1e-2 at 1e-6)
    # backward at the float64 statistics rounded to fp32 (the kernel's inputs)
    dx, (dg, db, dc) = RK._ln_bwd_call(L, dy, x, gamma, beta, r64[1].float(), r64[2].float(), M, N, ELU, layout)
    assert not bool(torch.isnan(dx).any())
    bounded('elu_ln.dx' + tag, dx, r64[3], r32[3], sc['dx'])
    bounded('elu_ln.dgamma' + tag, dg, r64[4], r32[4], sc['dgamma'])
    bounded('elu_ln.dbeta' + tag, db, r64[5], r32[5], sc['dbeta'])
    bounded('elu_ln.dcolsum' + tag, dc, r64[6], r32[6], sc['dcolsum'])


def test_layernorm_elu_deferred_parameter_reduction_is_bit_identical(L):
    """accumulate_params & 4 on the wave kernel: the partial rows summed later by genrl_reduce_params_batch give the immediate form's bits"""
    M, N = 2100, 512
    (x, gamma, beta, dy), r64, _, _ = case(M, N)
    mean, rstd = r64[1].float(), r64[2].float()
    prior = [torch.randn(N, generator=RK.gen(k)).cuda() for k in range(3)]
    dx0, imm = RK._ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, ELU, 'pad', acc=1, prior=prior)
    dx1, dfr = RK._ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, ELU, 'pad', acc=1, prior=prior, defer=True)
    assert torch.equal(dx0, dx1) and all(torch.equal(a, b) for a, b in zip(imm, dfr))
    dxs, _ = RK._ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, 1, 'pad', acc=1, prior=prior)
    assert not torch.equal(dx0, dxs)                # (... and it is not SiLU's)


@pytest.mark.parametrize('M,N', [(300, 68), (300, 260), (63, 4096), (300, 255)])
def test_layernorm_elu_h2_planes_equal_the_split_of_the_fp32_output(L, M, N):
    from genrl_amd import planes
    x, gamma, beta, dy = ln_inputs(M, N, 5 * M + N)
    P = planes.Planes(M, N, 'cuda')
    y, mean, rstd = RK._ln_fwd(L, x, gamma, beta, M, N, EPS, ELU, 'pad', planes=P)
    y0, mean0, rstd0 = RK._ln_fwd(L, x, gamma, beta, M, N, EPS, ELU, 'pad')
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    ref = planes.split(y.contiguous())
    assert torch.equal(P.inv, ref.inv) and torch.equal(P.t[:, :, :N], ref.t[:, :, :N])
    xd, dyd, gd, bd = x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda()
    dx0 = torch.full((M, N), float('nan'), device='cuda'); dx1 = dx0.clone()
    Pd = planes.Planes(M, N, 'cuda')
    assert L.genrl_ln_act_bwd(dyd.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              dx0.data_ptr(), N, None, None, None, None, M, N, ELU, 0, stream()) == 0
    assert L.genrl_ln_act_bwd_h2(dyd.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 dx1.data_ptr(), N, None, None, None, None, M, N, ELU, 0, Pd.ptr(), Pd.ld, Pd.plane, Pd.inv_ptr(),
                                 stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1) and not bool(torch.isnan(dx1).any())
    ref = planes.split(dx1)
    assert torch.equal(Pd.inv, ref.inv) and torch.equal(Pd.t[:, :, :N], ref.t[:, :, :N])


@pytest.mark.parametrize('M,N', [(64, 64), (300, 256)])
def test_layernorm_elu_uniform_planes(L, M, N):
    """genrl_ln_act_{fwd,bwd}_h2u with act = 2 under test_layernorm_uniform_planes's rule: |ELU(z)| <= |z|, the bound holds as for SiLU"""
    from genrl_amd import planes
    x, gamma, beta, dy = ln_inputs(M, N, 7 * M + N)
    P = planes.Planes(M, N, 'cuda')
    P.uniform = True
    y, mean, rstd = RK._ln_fwd(L, x, gamma, beta, M, N, EPS, ELU, 'pad', planes=P)
    y0, _, _ = RK._ln_fwd(L, x, gamma, beta, M, N, EPS, ELU, 'pad')
    assert torch.equal(y, y0)
    bound = float(gamma.abs().max()) * N ** 0.5 + float(beta.abs().max())
    assert (P.inv == P.inv[0]).all() and (P.t[:, :, N:] == 0).all()
    assert float(P.inv[0]) * 2 ** 14 <= bound < float(P.inv[0]) * 2 ** 15
    yc = y.contiguous()
    assert float(yc.abs().max()) <= bound
    assert ((P.float() - yc).abs() <= 2.0 ** -21 * bound).all()
    assert ((P.float() - yc).abs() <= 2.0 ** -22 * yc.abs() + 2.0 ** -37 * bound).all()
    dyd, xd, gd, bd = dy.cuda(), x.cuda(), gamma.cuda(), beta.cuda()
    dx0 = torch.full((M, N), float('nan'), device='cuda'); dx1 = dx0.clone()
    assert L.genrl_ln_act_bwd(dyd.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              dx0.data_ptr(), N, None, None, None, None, M, N, ELU, 0, stream()) == 0
    Pd = planes.Planes(M, N, 'cuda')
    amax = torch.empty(2048, device='cuda')
    assert L.genrl_ln_act_bwd_h2u(dyd.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                  dx1.data_ptr(), N, None, None, None, None, M, N, ELU, 0, Pd.ptr(), Pd.ld, Pd.plane, Pd.inv_ptr(),
                                  amax.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    m = float(dx1.abs().max())
    assert (Pd.inv == Pd.inv[0]).all() and float(Pd.inv[0]) * 2 ** 14 <= m < float(Pd.inv[0]) * 2 ** 15
    assert ((Pd.float() - dx1).abs() <= 2.0 ** -22 * dx1.abs() + 2.0 ** -37 * m).all()


# ---------------------------------------------------------------------------------------------- genrl_elu_{fwd,bwd}_h2
def elu_inputs(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 3.0 - 2.0)
    sp = torch.tensor([0.0, -0.0, 1e-6, -1e-6, 1e-3, -1e-3, 100.0, -100.0])
    x.view(-1)[:len(sp)] = sp[:M * N]
    dy = torch.randn(M, N, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 4.0 - 2.0)
    return x, dy


@pytest.mark.parametrize('N', [4, 36, 1028, 12288])
@pytest.mark.parametrize('M', [1, 3, 2049])
def test_elu_pair_vs_float64_and_planes(L, M, N):
    """the shapes and checks test_gpu_v2_kernels.py applies to genrl_silu_*_h2"""
    from genrl_amd import planes
    from genrl_amd._lib import check
    x, dy = elu_inputs(M, N, 1 + M + N)
    x64, dy64 = x.double(), dy.double()
    d64 = torch.where(x64 > 0, torch.ones_like(x64), torch.exp(x64))
    y64, g64 = F.elu(x64), dy64 * d64
    xr = x.clone().requires_grad_(True)
    y32 = F.elu(xr)
    y32.backward(dy)
    xd, dyd = in_buf(x, N + 4), in_buf(dy, N + 8)
    ybuf, y = out_buf(M, N, N + 12)
    P = planes.Planes(M, N, 'cuda')
    check(L.genrl_elu_fwd_h2(xd.data_ptr(), N + 4, y.data_ptr(), N + 12, M, N, P.ptr(), P.ld, P.plane, P.inv_ptr(), stream()), 'elu_fwd')
    untouched('elu y', ybuf, y)
    assert not bool(torch.isnan(y).any())
    bounded(f'elu.fwd[{M}x{N}]', y, y64, y32.detach(), y64.abs() + TINY)
    Q = planes.split(y.contiguous())
    assert torch.equal(P.t, Q.t) and torch.equal(P.inv, Q.inv)
    dbuf, dx = out_buf(M, N, N + 4)
    Pd = planes.Planes(M, N, 'cuda')
    check(L.genrl_elu_bwd_h2(dyd.data_ptr(), N + 8, xd.data_ptr(), N + 4, dx.data_ptr(), N + 4, M, N, Pd.ptr(), Pd.ld, Pd.plane,
                             Pd.inv_ptr(), stream()), 'elu_bwd')
    untouched('elu dx', dbuf, dx)
    assert not bool(torch.isnan(dx).any())
    bounded(f'elu.bwd[{M}x{N}]', dx, g64, xr.grad, dy64.abs() * d64 * (1 + torch.where(x64 > 0, torch.zeros_like(x64), x64.abs())) + TINY)
    Q = planes.split(dx.contiguous())
    assert torch.equal(Pd.t, Q.t) and torch.equal(Pd.inv, Q.inv)
    # both aliasings, without planes: the same bits
    z = x.cuda().contiguous()
    check(L.genrl_elu_fwd_h2(z.data_ptr(), N, z.data_ptr(), N, M, N, None, 0, 0, None, stream()), 'elu_fwd')
    assert torch.equal(z, y)
    gz = dy.cuda().contiguous()
    check(L.genrl_elu_bwd_h2(gz.data_ptr(), N, x.cuda().contiguous().data_ptr(), N, gz.data_ptr(), N, M, N, None, 0, 0, None, stream()), 'elu_bwd')
    assert torch.equal(gz, dx)


def test_elu_special_values_and_refusals(L):
    """+-0, +-1e-30, +-100 and NaN: y = -1 and dy/dx = 0 at -100, y = 100 at +100, 1 at both zeros, NaN stays NaN and nothing else becomes one"""
    from genrl_amd import planes
    sp = [0.0, -0.0, 1e-30, -1e-30, 100.0, -100.0, float('nan'), 0.5]
    x = torch.tensor([sp, sp[::-1]], device='cuda')
    g = torch.full_like(x, 3.0)
    y = torch.full_like(x, PAD); dx = torch.full_like(x, PAD)
    P = planes.Planes(2, 8, 'cuda')
    assert L.genrl_elu_fwd_h2(x.data_ptr(), 8, y.data_ptr(), 8, 2, 8, P.ptr(), P.ld, P.plane, P.inv_ptr(), stream()) == 0
    assert L.genrl_elu_bwd_h2(g.data_ptr(), 8, x.data_ptr(), 8, dx.data_ptr(), 8, 2, 8, None, 0, 0, None, stream()) == 0
    y0, d0 = y[0].cpu(), dx[0].cpu()
    assert y0[:6].tolist() == [0.0, 0.0, float(torch.tensor(1e-30)), float(torch.tensor(-1e-30)), 100.0, -1.0] and float(y0[7]) == 0.5
    assert d0[:5].tolist() == [3.0, 3.0, 3.0, 3.0, 3.0] and 0.0 <= float(d0[5]) < 1e-37 and float(d0[7]) == 3.0
    assert bool(torch.isnan(y0[6])) and bool(torch.isnan(d0[6])) and int(torch.isnan(y).sum()) == 2 and int(torch.isnan(dx).sum()) == 2
    assert torch.equal(y[1].flip(0)[[0, 1, 2, 3, 4, 5, 7]], y[0][[0, 1, 2, 3, 4, 5, 7]])
    # the contract of genrl_silu_*_h2: N % 4, pitches
    assert L.genrl_elu_fwd_h2(x.data_ptr(), 8, y.data_ptr(), 8, 2, 6, None, 0, 0, None, stream()) == EINVAL
    assert L.genrl_elu_fwd_h2(x.data_ptr(), 6, y.data_ptr(), 8, 2, 8, None, 0, 0, None, stream()) == EINVAL
    assert L.genrl_elu_bwd_h2(x.data_ptr(), 8, x.data_ptr(), 8, y.data_ptr(), 4, 2, 8, None, 0, 0, None, stream()) == EINVAL


# ---------------------------------------------------------------------------------------------- genrl_gemm_h2_ln, act = 2
@pytest.mark.parametrize('M,N,K0', [(64, 64, 64), (200, 64, 128), (64, 1024, 64), (200, 1024, 128)])
def test_fused_product_layernorm_elu_vs_the_two_launches_and_float64(L, M, N, K0):
    """one 64-row block and a ragged last block, one column tile and sixteen.  The product is the two-launch form's bit for bit; `y`, `mean`
    and `rstd` of the one-launch form -- and of the two launches (genrl_gemm_h2 + genrl_ln_act_fwd_h2, act = 2) -- are within the file's
    bound of float64 on the same C, with the float32 restatement as the yardstick; the last eleven columns carry the special values of z
    (gamma = 0, beta = z), so the epilogue's ELU arm meets |z| = 1e-6 and z = -95 in every row; the planes hold the fp32 output"""
    import test_gpu_gemm_ln as GL
    from genrl_amd import planes, ops_planes
    assert L_ok(M, N)
    (a0, b0, _, _), bias, gamma, beta = GL._case(M, N, K0, 0, seed=M + N)
    n = len(SPECIAL_Z)
    gamma[N - n:] = 0.0
    beta[N - n:] = torch.tensor(SPECIAL_Z, device='cuda')
    C_ref = torch.empty(M, N, device='cuda'); y_ref = torch.empty(M, N, device='cuda')
    m_ref = torch.empty(M, device='cuda'); r_ref = torch.empty(M, device='cuda')
    p_ref = planes.Planes(M, N, 'cuda')
    planes.gemm(a0, b0, C_ref, N, bias, M, N)
    ops_planes._ln_fwd(C_ref.data_ptr(), gamma, beta, y_ref.data_ptr(), m_ref.data_ptr(), r_ref.data_ptr(), M, N, EPS, p_ref, 0, ELU)
    C = torch.full((M, N), float('nan'), device='cuda'); y = torch.full((M, N), float('nan'), device='cuda')
    mean = torch.full((M,), float('nan'), device='cuda'); rstd = torch.full((M,), float('nan'), device='cuda')
    out_p = planes.Planes(M, N, 'cuda')
    planes.gemm_ln(a0, b0, C, bias, M, N, gamma, beta, EPS, out_p, 0, y=y, mean=mean, rstd=rstd, act=ELU)
    torch.cuda.synchronize()
    planes.check_ln_failure()
    assert torch.equal(C, C_ref)
    assert not bool(torch.isnan(y).any() | torch.isnan(mean).any() | torch.isnan(rstd).any())
    inp = (C.cpu(), gamma.cpu(), beta.cpu(), torch.zeros(M, N))
    r64, r32, sc = reference(*inp, torch.float64), reference(*inp, torch.float32), scales(*inp)
    tag = f'[{M}x{N}]'
    for name, form in (('gemm_ln', (y, mean, rstd)), ('gemm+ln', (y_ref, m_ref, r_ref))):
        bounded(f'elu_{name}.y' + tag, form[0], r64[0], r32[0], sc['y'])
        bounded(f'elu_{name}.mean' + tag, form[1], r64[1], r32[1], sc['mean'])
        bounded(f'elu_{name}.rstd' + tag, form[2], r64[2], r32[2], sc['rstd'])
    z = torch.tensor(SPECIAL_Z, dtype=torch.float32).double()
    want = torch.where(z > 0, z, torch.expm1(z))
    assert ((y[:, N - n:].cpu().double() - want).abs() <= 6 * U * want.abs()).all(), y[0, N - n:]
    sil = F.silu(F.layer_norm(C.double(), (N,), gamma.double(), beta.double(), EPS))
    assert (y.double() - sil).abs().max().item() > 0.1              # (... and it is not SiLU)
    bound = (gamma.abs().max() * N ** .5 + beta.abs().max()).item()
    assert (out_p.inv == out_p.inv[0]).all() and 2 ** 14 <= bound / out_p.inv[0].item() < 65504
    err = (out_p.float().double() - y.double()).abs()
    assert (err <= 2.0 ** -21 * y.double().abs() + 2.0 ** -36 * bound).all(), err.max().item()
    planes.check_ln_failure()


def L_ok(M, N):
    from genrl_amd import planes
    from genrl_amd._lib import lib
    return lib().genrl_gemm_h2_ln_ok(M, N) == 1 and planes.gemm_ln_ok(M, N)


# ---------------------------------------------------------------------------------------------- an unknown code
def test_act_3_is_refused_before_any_launch_by_every_entry_that_takes_a_code(L):
    from genrl_amd import planes
    M, N = 64, 64
    x = torch.randn(M, N, device='cuda'); dy = torch.randn(M, N, device='cuda')
    gamma = torch.ones(N, device='cuda'); beta = torch.zeros(N, device='cuda')
    mean = torch.zeros(M, device='cuda'); rstd = torch.ones(M, device='cuda')
    outs = [torch.full((M, N), PAD, device='cuda') for _ in range(2)] + [torch.full((M,), PAD, device='cuda') for _ in range(2)] + \
           [torch.full((N,), PAD, device='cuda') for _ in range(3)]
    y, dx, mo, ro, dg, db, dc = outs
    ws = torch.full((max(L.genrl_ln_ws_floats(M, N), 1),), PAD, device='cuda')
    amax = torch.full((2048,), PAD, device='cuda')
    P = planes.Planes(M, N, 'cuda')
    t0, i0 = P.t.clone(), P.inv.clone()
    pl = (P.ptr(), P.ld, P.plane, P.inv_ptr())
    fa = (x.data_ptr(), N, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), N, mo.data_ptr(), ro.data_ptr(), M, N, EPS, 3)
    ba = (dy.data_ptr(), N, x.data_ptr(), N, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), N,
          dg.data_ptr(), db.data_ptr(), dc.data_ptr(), ws.data_ptr(), M, N, 3, 0)
    assert L.genrl_ln_act_fwd(*fa, stream()) == EINVAL
    assert L.genrl_ln_act_fwd_h2(*fa, *pl, stream()) == EINVAL
    assert L.genrl_ln_act_fwd_h2u(*fa, *pl, stream()) == EINVAL
    assert L.genrl_ln_act_bwd(*ba, stream()) == EINVAL
    assert L.genrl_ln_act_bwd_h2(*ba, *pl, stream()) == EINVAL
    assert L.genrl_ln_act_bwd_h2u(*ba, *pl, amax.data_ptr(), stream()) == EINVAL
    assert L.genrl_ln_act_fwd(*fa[:-1], -1, stream()) == EINVAL
    a0, b0 = planes.split(x), planes.split(torch.randn(N, N, device='cuda'))
    C = torch.full((M, N), PAD, device='cuda')
    sync, part = planes._ln_workspace(x.device)
    assert L.genrl_gemm_h2_ln(a0.ptr(0), a0.ld, a0.plane, a0.inv_ptr(0), b0.ptr(0), b0.ld, b0.plane, b0.inv_ptr(0), a0.ld,
                              None, 0, 0, None, None, 0, 0, None, 0, C.data_ptr(), N, None, M, N, gamma.data_ptr(), beta.data_ptr(), EPS, 3,
                              y.data_ptr(), N, mo.data_ptr(), ro.data_ptr(), *pl, (part.data_ptr() + 15) // 16 * 16, sync.data_ptr(),
                              stream()) == EINVAL
    torch.cuda.synchronize()
    for t in outs + [ws, amax, C]:
        assert bool((t == PAD).all())
    assert torch.equal(P.t, t0) and torch.equal(P.inv, i0)
    planes.check_ln_failure()
