"""Every template instantiation the row-kernel dispatchers of csrc/rowops.hip (and the connector / aligner kernels of
csrc/stats.hip) can select, against float64 references computed on the host from the same fp32 inputs.

Each dispatcher picks its kernel from N / D / A / M and the operands' alignment; the shapes here sit on both sides of every
boundary (narrow lane groups GL 16 / 32 / 64, wave kernels NV 2..4, block kernels NV 2..4, the generic path, the GRU's DV 1..4,
the fused actor head's MAXO 12 / 20 / 32 / 64 forward and 6 / 10 / 16 / 32 backward, the gather LayerNorm's NV 1..4) and past
the grid caps, so that the grid-stride loops and the per-workgroup partial rows cover more than one row each.

Bounds are per element: |kernel - float64| <= K * 2^-24 * S, where S is a float64 magnitude of the terms the element is made of
(|gamma| |x^| + |beta| plus the row's mean |x| rstd for a LayerNorm output, sum |y| |W| + |b| for a product, the sum of the
per-row scales for a reduction over rows).  Each K sits about ten times above the largest ratio the kernels reach (measured on
an MI355X): a subtly wrong kernel (variance over N - 1, a dropped slice, a dropped partial row, a lane off by one) fails by
orders of magnitude.  Outputs are prefilled with NaN, so an element a kernel never writes fails; every buffer has padding
columns and a guard row, which must come back bit-identical."""
import pytest
import torch
import torch.nn.functional as F

from f64check import PAD, checker, in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

EINVAL = 1

# K per checked quantity (see the module docstring)
K = {
    'ln.y': 96, 'ln.mean': 100, 'ln.rstd': 32,
    'ln.dx': 24, 'ln.dparam': 16, 'ln.dcolsum': 20,
    'gru.h': 4, 'gru.dpre': 3, 'gru.dh': 8, 'gru.dparam': 0.2,       # (the GRU scales are loose sums: K < 1)
    'head.raw': 8, 'head.action': 16, 'head.draw': 10, 'head.mean_std': 20,
    'gather.xpre': 48,
    'conn.noisy': 24, 'cos.loss': 2, 'cos.dx': 64,
}
RATIOS = {}             # largest |kernel - float64| / (2^-24 S) seen per quantity (the margin each K leaves)
within = checker(K, RATIOS)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    return lib()


def vec_out(n):
    buf = torch.full((n + 4,), PAD, device='cuda')
    buf[:n] = float('nan')
    return buf, buf[:n]


# ====================================================================================== LayerNorm (+SiLU)
def ln_inputs(M, N, seed):
    """rows of spread e^(0.5 n) around small means; row 1 constant (variance 0), the last row's mean 10^3 x its spread"""
    g = gen(seed)
    x = torch.randn(M, N, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g)) + 0.3 * torch.randn(M, 1, generator=g)
    if M >= 3:
        x[1] = 3.7
        x[-1] = 1000.0 + torch.randn(N, generator=g)
    gamma = 1 + 0.3 * torch.randn(N, generator=g)
    beta = 0.3 * torch.randn(N, generator=g)
    return x, gamma, beta


def ln_fwd_ref(x, gamma, beta, eps, act):
    x = x.double(); ga = gamma.double(); be = beta.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    z = xh * ga + be
    y = F.silu(z) if act else z
    mabs = x.abs().mean(1, keepdim=True)
    sz = ga.abs() * (xh.abs() + rstd * mabs) + be.abs()
    sy = 1.1 * sz + y.abs() if act else sz
    return y, mean[:, 0], rstd[:, 0], sy, mabs[:, 0]


def ln_bwd_ref(dy, x, gamma, beta, mean, rstd, act):
    """float64 backward of y = act(LN(x) gamma + beta) at the given (fp32) statistics; -> dx, its scale, and per-column
    (dgamma, dbeta, dcolsum) with their scales"""
    dy = dy.double(); x = x.double(); ga = gamma.double(); be = beta.double()
    mean = mean.double()[:, None]; rstd = rstd.double()[:, None]
    xh = (x - mean) * rstd
    if act:
        z = xh * ga + be
        s = torch.sigmoid(z)
        dz = dy * s * (1 + z * (1 - s))
        sdz = dy.abs() * (1.1 + 0.5 * (xh.abs() * ga.abs() + be.abs()))
    else:
        dz, sdz = dy, dy.abs()
    e = dz * ga
    t = sdz * ga.abs()
    m1 = e.mean(1, keepdim=True); m2 = (e * xh).mean(1, keepdim=True)
    dx = rstd * (e - m1 - xh * m2)
    sdx = rstd * (t + t.mean(1, keepdim=True) + xh.abs() * (t * xh.abs()).mean(1, keepdim=True))
    sums = ((dz * xh).sum(0), dz.sum(0), dx.sum(0))
    scales = ((sdz * (xh.abs() + 1)).sum(0), sdz.sum(0), sdx.sum(0))
    return dx, sdx, sums, scales


# (M, N, act, layout): layout 'pad' = every operand in lines of N + 4 (or the next multiple of 4) floats;
# 'ld_odd' = x / y / dy / dx lines not a multiple of 4 floats apart; 'off1' = base pointers one float past 16-byte alignment
def _ln_cases():
    cases = []
    narrow = {64: 40000, 68: 17000, 128: 300, 132: 9000, 256: 9000}      # rows past the forward's / backward's narrow grid caps
    for N, big in narrow.items():
        cases += [(64, N, 1, 'pad'), (100, N, 0, 'pad'), (big, N, int(N % 8 == 0), "pad")]
    for N in (260, 512, 516, 768, 772, 1024):                             # wave per row; > 8192 rows: the forward's grid stride
        cases += [(1, N, 1, 'pad'), (63, N, 0, 'pad'), (64, N, 1, 'pad'), (8200 if N in (260, 772, 1024) else 2100, N, int(N % 8 == 4), "pad")]
    for N in (1028, 2048, 2052, 3072, 3076, 4096):                        # block per row; > 2048 rows, > 512 backward workgroups
        cases += [(1, N, 0, 'pad'), (63, N, 1, 'pad'), (2100, N, int(N % 8 == 0), "pad")]
    cases += [(40, 200, 1, 'pad'), (1, 64, 0, 'pad'),                   # generic: M < 64 with N <= 256
              (300, 255, 1, 'pad'), (300, 1030, 0, 'pad'), (300, 4100, 1, 'pad'), (70, 6000, 0, 'pad'),    # N % 4 != 0, N > 4096
              (300, 512, 1, 'ld_odd'), (300, 128, 0, 'ld_odd'), (300, 2048, 1, 'ld_odd'),
              (300, 512, 0, 'off1'), (300, 128, 1, 'off1'), (2100, 3072, 0, 'off1')]
    return cases


LN_CASES = _ln_cases()


def _layout(N, layout):
    if layout == 'ld_odd':
        return N + 3, 0
    if layout == 'off1':
        return (N + 7) // 4 * 4, 1
    return (N + 7) // 4 * 4, 0


def _ln_fwd(L, x, gamma, beta, M, N, eps, act, layout, planes=None):
    ld, off = _layout(N, layout)
    xd = in_buf(x, ld, off)
    yb, y = out_buf(M, N, ld + 4 if layout == 'pad' else ld, off)
    mb, mean = vec_out(M)
    rb, rstd = vec_out(M)
    gd, bd = gamma.cuda(), beta.cuda()
    if planes is None:
        rc = L.genrl_ln_act_fwd(xd.data_ptr(), xd.stride(0), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), y.stride(0), mean.data_ptr(),
                                rstd.data_ptr(), M, N, eps, act, stream())
    else:
        fn = L.genrl_ln_act_fwd_h2u if planes.uniform else L.genrl_ln_act_fwd_h2
        rc = fn(xd.data_ptr(), xd.stride(0), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(),
                M, N, eps, act, planes.ptr(), planes.ld, planes.plane, planes.inv_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    untouched('y', yb, y); untouched('mean', mb, mean); untouched('rstd', rb, rstd)
    return y, mean, rstd


@pytest.mark.parametrize('M,N,act,layout', LN_CASES)
def test_layernorm_forward(L, M, N, act, layout):
    x, gamma, beta = ln_inputs(M, N, M + N)
    eps = 1e-3
    y, mean, rstd = _ln_fwd(L, x, gamma, beta, M, N, eps, act, layout)
    yr, mr, rr, sy, mabs = ln_fwd_ref(x, gamma, beta, eps, act)
    within('ln.y', y, yr, sy)
    within('ln.mean', mean, mr, mabs)
    within('ln.rstd', rstd, rr, rr)


def _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, layout, with_params=True, np_=3, acc=0, prior=None, defer=False):
    from genrl_amd import ops
    ld, off = _layout(N, layout)
    xd, dyd = in_buf(x, ld, off), in_buf(dy, ld, off)
    dxb, dx = out_buf(M, N, ld + 4 if layout == 'pad' else ld, off)
    gd, bd, md, rd = gamma.cuda(), beta.cuda(), mean.cuda(), rstd.cuda()
    outs = [vec_out(N) for _ in range(3)]
    if prior is not None:
        for (_, o), p in zip(outs, prior):
            o.copy_(p)
    ws = torch.empty(L.genrl_ln_ws_floats(M, N), device='cuda')
    flag = acc
    if defer:
        ops.DEFER_REDUCTIONS, prev = True, ops.DEFER_REDUCTIONS
        ops.defer_begin()
        flag |= ops.defer_reduce(M, N, ws, outs[0][1], outs[1][1], outs[2][1] if np_ == 3 else None)
        assert flag & 4
    try:
        rc = L.genrl_ln_act_bwd(dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0), gd.data_ptr(), bd.data_ptr(), md.data_ptr(),
                                rd.data_ptr(), dx.data_ptr(), dx.stride(0), outs[0][1].data_ptr() if with_params else None,
                                outs[1][1].data_ptr() if with_params else None, outs[2][1].data_ptr() if with_params and np_ == 3 else None,
                                ws.data_ptr(), M, N, act, flag, stream())
        assert rc == 0
        if defer:
            ops.defer_flush()
    finally:
        if defer:
            ops.DEFER_REDUCTIONS = prev
    torch.cuda.synchronize()
    untouched('dx', dxb, dx)
    for k, (b, o) in enumerate(outs):
        if with_params and (k < 2 or np_ == 3):
            untouched('param grad', b, o)
    return dx, [o for _, o in outs]


@pytest.mark.parametrize('M,N,act,layout', LN_CASES)
def test_layernorm_backward(L, M, N, act, layout):
    """dx, dgamma, dbeta and the column sums of dx; the statistics are the float64 ones rounded to fp32 (the kernel's inputs)"""
    x, gamma, beta = ln_inputs(M, N, M + N)
    _, mean, rstd, _, _ = ln_fwd_ref(x, gamma, beta, 1e-3, act)
    mean, rstd = mean.float(), rstd.float()
    dy = torch.randn(M, N, generator=gen(M * 7 + N))
    dx, (dg, db, dc) = _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, layout)
    dxr, sdx, sums, scales = ln_bwd_ref(dy, x, gamma, beta, mean, rstd, act)
    within('ln.dx', dx, dxr, sdx)
    within('ln.dparam[dgamma]', dg, sums[0], scales[0])
    within('ln.dparam[dbeta]', db, sums[1], scales[1])
    within('ln.dcolsum', dc, sums[2], scales[2])


# one shape per backward kernel family (narrow GL 16 / 64, wave, block): np = 2 and 3, accumulate (bit 1), deferral (bit 4)
FLAG_CASES = [(20000, 64, 1), (9000, 256, 0), (2100, 512, 1), (8200, 1024, 0), (2100, 2052, 1), (600, 4096, 0)]


@pytest.mark.parametrize('M,N,act', FLAG_CASES)
def test_layernorm_backward_flags(L, M, N, act):
    from genrl_amd._lib import lib
    x, gamma, beta = ln_inputs(M, N, 5 * M + N)
    _, mean, rstd, _, _ = ln_fwd_ref(x, gamma, beta, 1e-3, act)
    mean, rstd = mean.float(), rstd.float()
    dy = torch.randn(M, N, generator=gen(M + 3 * N))
    dxr, sdx, sums, scales = ln_bwd_ref(dy, x, gamma, beta, mean, rstd, act)
    prior = [torch.randn(N, generator=gen(k)).cuda() * float(sums[k].abs().mean()) for k in range(3)]
    assert lib().genrl_ln_bwd_parts(M, N) > 0
    for np_ in (2, 3):
        dx, (dg, db, dc) = _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, 'pad', np_=np_, acc=1, prior=prior)
        within('ln.dx', dx, dxr, sdx)
        for k, o in enumerate((dg, db, dc)[:np_]):
            within(f'ln.dparam[acc {k}]', o, sums[k] + prior[k].cpu().double(), scales[k] + prior[k].cpu().double().abs(),
                   key='ln.dcolsum' if k == 2 else 'ln.dparam')
        if np_ == 2:
            assert torch.equal(dc, prior[2])                              # no column sums asked for: untouched
        # deferral: the same partial rows summed later by genrl_reduce_params_batch -- bit-identical to the immediate form
        for acc in (1,):                # (genrl_reduce_params_batch adds: the deferred form is the accumulating one)
            dx0, imm = _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, 'pad', np_=np_, acc=acc, prior=prior)
            dx1, dfr = _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, 'pad', np_=np_, acc=acc, prior=prior, defer=True)
            assert torch.equal(dx0, dx1)
            for a, b in list(zip(imm, dfr))[:np_]:
                assert torch.equal(a, b)
    # dx only (no parameter gradients)
    dx, outs = _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, 'pad', with_params=False)
    within('ln.dx', dx, dxr, sdx)
    assert all(o.isnan().all() for o in outs)


def test_layernorm_backward_generic_two_level_reduction(L):
    """the generic backward at 70 000 rows x 255: 1094 chunk partials, more than one reduce_chunks2m launch sums, take the
    two-level reduce_chunksA -> reduce_chunks2 path (and reduce_cols' for the column sums); float64 reference in row blocks"""
    M, N, act = 70000, 255, 1
    x, gamma, beta = ln_inputs(M, N, 11)
    mean = torch.empty(M); rstd = torch.empty(M)
    for r0 in range(0, M, 8192):
        _, m, r, _, _ = ln_fwd_ref(x[r0:r0 + 8192], gamma, beta, 1e-3, act)
        mean[r0:r0 + 8192], rstd[r0:r0 + 8192] = m.float(), r.float()
    dy = torch.randn(M, N, generator=gen(12))
    prior = [torch.randn(N, generator=gen(13 + k)).cuda() for k in range(3)]
    dx, outs = _ln_bwd_call(L, dy, x, gamma, beta, mean, rstd, M, N, act, 'pad', acc=1, prior=prior)
    sums = [prior[k].cpu().double() for k in range(3)]
    scales = [prior[k].cpu().double().abs() for k in range(3)]
    dx = dx.cpu()
    for r0 in range(0, M, 8192):
        sl = slice(r0, r0 + 8192)
        dxr, sdx, s, sc = ln_bwd_ref(dy[sl], x[sl], gamma, beta, mean[sl], rstd[sl], act)
        within('ln.dx', dx[sl], dxr, sdx)
        for k in range(3):
            sums[k] = sums[k] + s[k]; scales[k] = scales[k] + sc[k]
    for k in range(3):
        within(f'ln.dparam[{k}]', outs[k], sums[k], scales[k], key='ln.dcolsum' if k == 2 else 'ln.dparam')


PLANE_CASES = [(300, 68, 1), (9000, 256, 0), (300, 260, 1), (8200, 1024, 0), (2100, 2052, 1), (63, 4096, 0), (300, 255, 1), (70, 4100, 0)]


@pytest.mark.parametrize('M,N,act', PLANE_CASES)
def test_layernorm_plane_outputs_equal_the_split_of_the_fp32_output(L, M, N, act):
    """genrl_ln_act_{fwd,bwd}_h2: the planes the kernels write themselves (wave / block) and the ones split after the fp32 pass
    (narrow, generic) are bit-identical to planes.split of the fp32 output they return; the fp32 output is the plain call's"""
    from genrl_amd import planes
    x, gamma, beta = ln_inputs(M, N, 3 * M + N)
    P = planes.Planes(M, N, 'cuda')
    y, mean, rstd = _ln_fwd(L, x, gamma, beta, M, N, 1e-3, act, 'pad', planes=P)
    y0, mean0, rstd0 = _ln_fwd(L, x, gamma, beta, M, N, 1e-3, act, 'pad')
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    ref = planes.split(y.contiguous())
    assert torch.equal(P.inv, ref.inv) and torch.equal(P.t[:, :, :N], ref.t[:, :, :N])
    dy = torch.randn(M, N, generator=gen(M + 5 * N))
    xd, dyd = x.cuda(), dy.cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    dx0 = torch.full((M, N), float('nan'), device='cuda'); dx1 = dx0.clone()
    Pd = planes.Planes(M, N, 'cuda')
    assert L.genrl_ln_act_bwd(dyd.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              dx0.data_ptr(), N, None, None, None, None, M, N, act, 0, stream()) == 0
    assert L.genrl_ln_act_bwd_h2(dyd.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 dx1.data_ptr(), N, None, None, None, None, M, N, act, 0, Pd.ptr(), Pd.ld, Pd.plane, Pd.inv_ptr(),
                                 stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    ref = planes.split(dx1)
    assert torch.equal(Pd.inv, ref.inv) and torch.equal(Pd.t[:, :, :N], ref.t[:, :, :N])


@pytest.mark.parametrize('M,N,act', [(64, 64, 1), (17000, 68, 0), (9000, 132, 1), (300, 256, 0)])
def test_layernorm_uniform_planes(L, M, N, act):
    """genrl_ln_act_{fwd,bwd}_h2u (the narrow kernels only): one scale for the tensor; the planes reproduce the fp32 output within
    the uniform split's bound; the fp32 outputs are the plain calls'"""
    from genrl_amd import planes
    x, gamma, beta = ln_inputs(M, N, 7 * M + N)
    P = planes.Planes(M, N, 'cuda')
    P.uniform = True
    y, mean, rstd = _ln_fwd(L, x, gamma, beta, M, N, 1e-3, act, 'pad', planes=P)
    y0, _, _ = _ln_fwd(L, x, gamma, beta, M, N, 1e-3, act, 'pad')
    assert torch.equal(y, y0)
    bound = float(gamma.abs().max()) * N ** 0.5 + float(beta.abs().max())
    assert (P.inv == P.inv[0]).all() and (P.t[:, :, N:] == 0).all()
    assert float(P.inv[0]) * 2 ** 14 <= bound < float(P.inv[0]) * 2 ** 15
    yc = y.contiguous()
    assert ((P.float() - yc).abs() <= 2.0 ** -21 * bound).all()
    assert ((P.float() - yc).abs() <= 2.0 ** -22 * yc.abs() + 2.0 ** -37 * bound).all()
    dy = torch.randn(M, N, generator=gen(M + 9 * N)).cuda()
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    dx0 = torch.full((M, N), float('nan'), device='cuda'); dx1 = dx0.clone()
    assert L.genrl_ln_act_bwd(dy.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              dx0.data_ptr(), N, None, None, None, None, M, N, act, 0, stream()) == 0
    Pd = planes.Planes(M, N, 'cuda')
    amax = torch.empty(2048, device='cuda')
    assert L.genrl_ln_act_bwd_h2u(dy.data_ptr(), N, xd.data_ptr(), N, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                  dx1.data_ptr(), N, None, None, None, None, M, N, act, 0, Pd.ptr(), Pd.ld, Pd.plane, Pd.inv_ptr(),
                                  amax.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    m = float(dx1.abs().max())
    assert (Pd.inv == Pd.inv[0]).all() and float(Pd.inv[0]) * 2 ** 14 <= m < float(Pd.inv[0]) * 2 ** 15
    assert ((Pd.float() - dx1).abs() <= 2.0 ** -22 * dx1.abs() + 2.0 ** -37 * m).all()


# ====================================================================================== GRU gates
def gru_inputs(R, D, seed):
    g = gen(seed)
    pre = torch.randn(R, 3 * D, generator=g) * 1.5 + 0.2 * torch.randn(R, 1, generator=g)
    h = torch.randn(R, D, generator=g)
    gamma = 1 + 0.2 * torch.randn(3 * D, generator=g)
    beta = 0.2 * torch.randn(3 * D, generator=g)
    return pre, h, gamma, beta


def gru_ref(pre, h, gamma, beta, eps, mean=None, rstd=None):
    """-> float64 autograd leaves and (h', its scale, mean, rstd, S_z sum per gate element, pc, xh) -- at the given statistics
    when mean / rstd are passed (the backward's inputs), else at float64 ones"""
    p = pre.double().requires_grad_(); hh = h.double().requires_grad_()
    ga = gamma.double().requires_grad_(); be = beta.double().requires_grad_()
    D = h.shape[1]
    if mean is None:
        m = p.mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(((p - m) ** 2).mean(1, keepdim=True) + eps)
    else:
        m = p.mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(((p - m) ** 2).mean(1, keepdim=True) + eps)
        # the kernel's backward assumes its inputs are the statistics of `pre`: differentiate through them, evaluate at the given values
        m = m + (mean.double()[:, None] - m.detach()); rs = rs + (rstd.double()[:, None] - rs.detach())
    xh = (p - m) * rs
    z = xh * ga + be
    pr, pc, pu = z[:, :D], z[:, D:2 * D], z[:, 2 * D:]
    r = torch.sigmoid(pr); c = torch.tanh(r * pc); u = torch.sigmoid(pu - 1.0)
    out = u * c + (1 - u) * hh
    with torch.no_grad():
        mabs = p.abs().mean(1, keepdim=True)
        sz = ga.abs() * (xh.abs() + rs * mabs) + be.abs()
        szs = sz[:, :D] + sz[:, D:2 * D] + sz[:, 2 * D:]
        sout = (1 + pc.abs() + hh.abs()) * szs + c.abs() + hh.abs()
    return (p, hh, ga, be), out, sout, m.detach()[:, 0], rs.detach()[:, 0], szs, pc.detach(), xh.detach(), u.detach()


GRU_CASES = [(2100, 1024), (63, 1028), (1, 2048), (600, 3072), (2100, 4096), (7, 12)]


@pytest.mark.parametrize('R,D', GRU_CASES)
@pytest.mark.parametrize('second', ['none', 'hout2', 'hout2_scaled'])
def test_gru_gates_forward(L, R, D, second):
    """genrl_gru_gates_fwd_ld2 at DV 1..4, > 2048 rows (the grid stride), padded ldh / ldo / ldo2, the second output with and without
    a per-row scale"""
    pre, h, gamma, beta = gru_inputs(R, D, R + D)
    eps = 1e-3
    pd = pre.cuda(); hd = in_buf(h, D + 4)
    gd, bd = gamma.cuda(), beta.cuda()
    hb, ho = out_buf(R, D, D + 8)
    h2b, h2 = out_buf(R, D, D + 12)
    mb, mean = vec_out(R); rb, rstd = vec_out(R)
    scale = (torch.rand(R, generator=gen(R)) < 0.7).float() * 1.5
    sd = scale.cuda()
    rc = L.genrl_gru_gates_fwd_ld2(pd.data_ptr(), hd.data_ptr(), hd.stride(0), gd.data_ptr(), bd.data_ptr(), ho.data_ptr(), ho.stride(0),
                                   h2.data_ptr() if second != 'none' else None, h2.stride(0),
                                   sd.data_ptr() if second == 'hout2_scaled' else None, mean.data_ptr(), rstd.data_ptr(), R, D, eps, stream())
    assert rc == 0
    torch.cuda.synchronize()
    untouched('hout', hb, ho); untouched('hout2', h2b, h2); untouched('mean', mb, mean); untouched('rstd', rb, rstd)
    _, out, sout, mr, rr, _, _, _, _ = gru_ref(pre, h, gamma, beta, eps)
    out = out.detach()
    within('gru.h', ho, out, sout)
    within('ln.mean[gru]', mean, mr, pre.double().abs().mean(1), key='ln.mean')
    within('ln.rstd[gru]', rstd, rr, rr, key='ln.rstd')
    if second == 'none':
        assert h2.isnan().all()
    elif second == 'hout2':
        assert torch.equal(h2, ho)
    else:
        assert torch.equal(h2, ho * sd[:, None])


@pytest.mark.parametrize('R,D', [(2100, 1024), (63, 1028), (520, 2048), (600, 3072), (520, 4096), (7, 12)])
def test_gru_gates_backward_scan_order(L, R, D):
    """genrl_gru_gates_bwd over T = 3 steps with the scan's bit sequence 4, 2|4, 2 (partials piled up in the workspace, one reduction
    at the end) against the float64 sum of the steps' parameter gradients; dpre / dh of every step; dhout2 with a per-row scale
    and two K-split slabs; padded lddo / ldh / lddh"""
    T, eps = 3, 1e-3
    gd_prior = torch.randn(3 * D, generator=gen(1)).cuda()
    dg = torch.full((3 * D,), float('nan'), device='cuda'); db = dg.clone()
    ws = torch.empty(L.genrl_gru_ws_floats(R, D), device='cuda')
    sum_g = torch.zeros(3 * D, dtype=torch.float64); sum_b = sum_g.clone(); sc_g = sum_g.clone(); sc_b = sum_g.clone()
    flags = [4] + [2 | 4] * (T - 2) + [2]
    for t, flag in enumerate(flags):
        pre, h, gamma, beta = gru_inputs(R, D, 100 * t + R + D)
        _, _, _, mr, rr, _, _, _, _ = gru_ref(pre, h, gamma, beta, eps)
        mean, rstd = mr.float(), rr.float()
        g = gen(7 * t + D)
        dhout = torch.randn(R, D, generator=g); dhout2 = torch.randn(R, D, generator=g)
        slabs = torch.randn(2, R, D, generator=g) * 0.5
        scale = (torch.rand(R, generator=g) < 0.7).float() * 1.5
        pd, hd = pre.cuda(), in_buf(h, D + 4)
        dod = in_buf(dhout, D + 8)
        d2d, sld, scd = dhout2.cuda(), slabs.cuda(), scale.cuda()
        gmd, btd, md, rd = gamma.cuda(), beta.cuda(), mean.cuda(), rstd.cuda()
        dpb, dpre = out_buf(R, 3 * D, 3 * D)
        dhb, dh = out_buf(R, D, D + 4)
        rc = L.genrl_gru_gates_bwd(dod.data_ptr(), dod.stride(0), d2d.data_ptr(), scd.data_ptr(), pd.data_ptr(), hd.data_ptr(), hd.stride(0),
                                   gmd.data_ptr(), btd.data_ptr(), md.data_ptr(), rd.data_ptr(), dpre.data_ptr(), dh.data_ptr(), dh.stride(0),
                                   dg.data_ptr(), db.data_ptr(), ws.data_ptr(), R, D, flag, sld.data_ptr(), 2, R * D, stream())
        assert rc == 0
        torch.cuda.synchronize()
        untouched('dpre', dpb, dpre); untouched('dh', dhb, dh)
        leaves, out, _, _, rs, szs, pc, xh, u = gru_ref(pre, h, gamma, beta, eps, mean, rstd)
        go = dhout.double() + (dhout2.double() + slabs.double().sum(0)) * scale.double()[:, None]
        out.backward(go)
        sgo = dhout.double().abs() + (dhout2.double().abs() + slabs.double().abs().sum(0)) * scale.double()[:, None]
        sdz = sgo * (1 + pc.abs()) * (1 + szs)
        sdz3 = torch.cat([sdz] * 3, 1)
        tg = sdz3 * gamma.double().abs()
        sdp = rs[:, None] * (tg + tg.mean(1, keepdim=True) + xh.abs() * (tg * xh.abs()).mean(1, keepdim=True))
        within('gru.dpre', dpre, leaves[0].grad, sdp)
        within('gru.dh', dh, leaves[1].grad, sgo * (1 + szs))
        sum_g += leaves[2].grad; sum_b += leaves[3].grad
        sc_g += (sdz3 * (xh.abs() + 1)).sum(0); sc_b += sdz3.sum(0)
        if flag & 4:
            assert dg.isnan().all() and db.isnan().all()                 # deferred: the parameter gradients untouched
    within('gru.dparam[dgamma]', dg, sum_g, sc_g)
    within('gru.dparam[dbeta]', db, sum_b, sc_b)
    # accumulate into existing parameter gradients (bit 1), one step
    dg.copy_(gd_prior); db.copy_(gd_prior)
    rc = L.genrl_gru_gates_bwd(dod.data_ptr(), dod.stride(0), d2d.data_ptr(), scd.data_ptr(), pd.data_ptr(), hd.data_ptr(), hd.stride(0),
                               gmd.data_ptr(), btd.data_ptr(), md.data_ptr(), rd.data_ptr(), dpre.data_ptr(), dh.data_ptr(), dh.stride(0),
                               dg.data_ptr(), db.data_ptr(), ws.data_ptr(), R, D, 1, sld.data_ptr(), 2, R * D, stream())
    assert rc == 0
    torch.cuda.synchronize()
    pr = gd_prior.cpu().double()
    within('gru.dparam[acc dgamma]', dg, pr + leaves[2].grad, pr.abs() + (sdz3 * (xh.abs() + 1)).sum(0), key='gru.dparam')
    within('gru.dparam[acc dbeta]', db, pr + leaves[3].grad, pr.abs() + sdz3.sum(0), key='gru.dparam')


def test_gru_gates_refuses_what_it_cannot_run(L):
    R, D = 4, 4100
    pre, h = torch.zeros(R, 3 * D, device='cuda'), torch.zeros(R, D, device='cuda')
    gb = torch.zeros(3 * D, device='cuda')
    ho = torch.full((R, D), float('nan'), device='cuda'); m = torch.empty(R, device='cuda'); r = torch.empty(R, device='cuda')
    assert L.genrl_gru_gates_fwd(pre.data_ptr(), h.data_ptr(), D, gb.data_ptr(), gb.data_ptr(), ho.data_ptr(), D, None, None, m.data_ptr(),
                                 r.data_ptr(), R, D, 1e-3, stream()) == EINVAL
    assert L.genrl_gru_gates_fwd(pre.data_ptr(), h.data_ptr(), 1026, gb.data_ptr(), gb.data_ptr(), ho.data_ptr(), 1024, None, None, m.data_ptr(),
                                 r.data_ptr(), R, 1024, 1e-3, stream()) == EINVAL
    torch.cuda.synchronize()
    assert ho.isnan().all()


# ====================================================================================== actor head
MIN_STD, MAX_STD = 0.1, 1.0


def head_ref(raw, eps):
    """float64: action = tanh(raw_o) + ((max - min) sigmoid(raw_s + 2) + min) eps; -> (action, mean, std) as autograd results"""
    A = raw.shape[1] // 2
    mean = torch.tanh(raw[:, :A])
    std = (MAX_STD - MIN_STD) * torch.sigmoid(raw[:, A:] + 2.0) + MIN_STD
    return mean + std * eps if eps is not None else mean, mean, std


def head_scale(sraw_o, sraw_s, eps, mean, std):
    e = eps.abs() if eps is not None else 0.0
    return sraw_o + 0.25 * (MAX_STD - MIN_STD) * e * sraw_s + mean.abs() + std * e + std


@pytest.mark.parametrize('U', [512, 1024, 2048])
@pytest.mark.parametrize('A', [1, 6, 7, 10, 11, 12, 16, 17, 32])
def test_actor_head_linear_forward(L, A, U):
    """genrl_actor_head_linear_fwd at every MAXO (2A <= 12 / 20 / 32 / 64; U = 2048 runs the k loop twice): raw against float64
    y W^T + b, action against the float64 head, the planes equal to split(action), with and without noise"""
    from genrl_amd import planes
    R = 130
    g = gen(A * 100 + U)
    y = torch.randn(R, U, generator=g); W = torch.randn(2 * A, U, generator=g) / U ** 0.5; b = 0.5 * torch.randn(2 * A, generator=g)
    eps = torch.randn(R, A, generator=g)
    yd = in_buf(y, U + 4); Wd, bd, ed = W.cuda(), b.cuda(), eps.cuda()
    AP = (A + 3) // 4 * 4
    rawr = y.double() @ W.double().t() + b.double()
    sraw = y.double().abs() @ W.double().abs().t() + b.double().abs()
    for noise in (True, False):
        rb, raw = out_buf(R, 2 * A, 2 * A)
        ab, act = out_buf(R, A, AP + 4)
        P = planes.Planes(R, A, 'cuda')
        rc = L.genrl_actor_head_linear_fwd(yd.data_ptr(), yd.stride(0), Wd.data_ptr(), bd.data_ptr(), ed.data_ptr() if noise else None,
                                           raw.data_ptr(), act.data_ptr(), R, U, A, MIN_STD, MAX_STD, act.stride(0), P.ptr(), P.ld, P.plane,
                                           P.inv_ptr(), stream())
        assert rc == 0
        torch.cuda.synchronize()
        untouched('raw', rb, raw); untouched('action', ab, act)
        within('head.raw', raw, rawr, sraw)
        e = eps.double() if noise else None
        ar, mr, sr = head_ref(rawr, e)
        within('head.action', act, ar, head_scale(sraw[:, :A], sraw[:, A:], e, mr, sr))
        ref = planes.split(act.contiguous())
        assert torch.equal(P.inv, ref.inv) and torch.equal(P.t[:, :, :A], ref.t[:, :, :A]) and (P.t[:, :, A:] == 0).all()


@pytest.mark.parametrize('up', [True, False])
@pytest.mark.parametrize('A', [1, 6, 7, 10, 11, 12, 16, 17, 32])
def test_actor_head_linear_backward(L, A, up):
    """genrl_actor_head_linear_bwd at every MAXO (A <= 6 / 10 / 16 / 32) against float64 autograd of the head formula at
    d action = dx WaT^T (+ the upstream gradient)"""
    R = 130
    Ud = 2048 if A in (12, 32) else 1024
    g = gen(A * 10 + up)
    dx = torch.randn(R, Ud, generator=g); WaT = torch.randn(A, Ud, generator=g) / Ud ** 0.5
    raw = torch.randn(R, 2 * A, generator=g); eps = torch.randn(R, A, generator=g)
    AP = (A + 3) // 4 * 4
    dup = torch.randn(R, A, generator=g)
    dxd = in_buf(dx, Ud + 4); Wd, rd, ed = WaT.cuda(), raw.cuda(), eps.cuda()
    dud = in_buf(dup, AP + 4)
    db_, draw = out_buf(R, 2 * A, 2 * A)
    rc = L.genrl_actor_head_linear_bwd(dxd.data_ptr(), dxd.stride(0), Wd.data_ptr(), dud.data_ptr() if up else None, dud.stride(0),
                                       rd.data_ptr(), ed.data_ptr(), draw.data_ptr(), R, Ud, A, MIN_STD, MAX_STD, stream())
    assert rc == 0
    torch.cuda.synchronize()
    untouched('draw', db_, draw)
    gref = dx.double() @ WaT.double().t() + (dup.double() if up else 0)
    sg = dx.double().abs() @ WaT.double().abs().t() + (dup.double().abs() if up else 0)
    r64 = raw.double().requires_grad_()
    act, _, _ = head_ref(r64, eps.double())
    act.backward(gref)
    s = sg + gref.abs()
    within('head.draw', draw, r64.grad, torch.cat([s, s * eps.double().abs() * 0.25 * (MAX_STD - MIN_STD)], 1))


def test_actor_head_linear_refusals(L):
    """A > 32 and U % 4 != 0 are refused (GENRL_EINVAL) before anything is launched"""
    R = 8
    for A, U in ((33, 1024), (6, 1026), (0, 1024)):
        y = torch.zeros(R, 1028, device='cuda'); W = torch.zeros(2 * max(A, 1), 1028, device='cuda')
        raw = torch.full((R, 2 * max(A, 1)), float('nan'), device='cuda'); act = torch.full((R, 36), float('nan'), device='cuda')
        eps = torch.zeros(R, max(A, 1), device='cuda')
        assert L.genrl_actor_head_linear_fwd(y.data_ptr(), 1028, W.data_ptr(), None, eps.data_ptr(), raw.data_ptr(), act.data_ptr(), R, U, A,
                                             MIN_STD, MAX_STD, 36, None, 0, 0, None, stream()) == EINVAL
        assert L.genrl_actor_head_linear_bwd(y.data_ptr(), 1028, W.data_ptr(), None, 36, raw.data_ptr(), eps.data_ptr(), act.data_ptr(), R, U, A,
                                             MIN_STD, MAX_STD, stream()) == EINVAL
        torch.cuda.synchronize()
        assert raw.isnan().all() and act.isnan().all()


@pytest.mark.parametrize('A', [1, 6, 12, 17, 32])
def test_actor_head_fwd_flat_and_row_kernels(L, A):
    """genrl_actor_head_fwd (flat kernel: action with ld_action > A, mean, std) and genrl_actor_head_fwd_h2 (row kernel + planes),
    ops.actor_mean_std (no noise, no action) against the float64 head"""
    from genrl_amd import ops, planes
    R = 300
    g = gen(A)
    raw = torch.randn(R, 2 * A, generator=g) * 2; eps = torch.randn(R, A, generator=g)
    rd, ed = raw.cuda(), eps.cuda()
    r64 = raw.double()
    ar, mr, sr = head_ref(r64, eps.double())
    sa = head_scale(r64[:, :A].abs(), r64[:, A:].abs(), eps.double(), mr, sr)
    lda = (A + 3) // 4 * 4 + 4
    for rows in (False, True):
        ab, act = out_buf(R, A, lda)
        mb, mean = out_buf(R, A, A); sb, std = out_buf(R, A, A)
        if rows:
            P = planes.Planes(R, A, 'cuda')
            rc = L.genrl_actor_head_fwd_h2(rd.data_ptr(), ed.data_ptr(), act.data_ptr(), mean.data_ptr(), std.data_ptr(), R, A, MIN_STD, MAX_STD,
                                           lda, P.ptr(), P.ld, P.plane, P.inv_ptr(), stream())
        else:
            rc = L.genrl_actor_head_fwd(rd.data_ptr(), ed.data_ptr(), act.data_ptr(), mean.data_ptr(), std.data_ptr(), R, A, MIN_STD, MAX_STD,
                                        lda, stream())
        assert rc == 0
        torch.cuda.synchronize()
        untouched('action', ab, act); untouched('mean', mb, mean); untouched('std', sb, std)
        within('head.action', act, ar, sa)
        within('head.mean_std[mean]', mean, mr, r64[:, :A].abs() + mr.abs(), key='head.mean_std')
        within('head.mean_std[std]', std, sr, r64[:, A:].abs() + sr, key='head.mean_std')
        if rows:
            ref = planes.split(act.contiguous())
            assert torch.equal(P.inv, ref.inv) and torch.equal(P.t[:, :, :A], ref.t[:, :, :A])
    m2, s2 = ops.actor_mean_std(rd.reshape(10, 30, 2 * A))
    within('head.mean_std[ops mean]', m2.reshape(R, A), mr, r64[:, :A].abs() + mr.abs(), key='head.mean_std')
    within('head.mean_std[ops std]', s2.reshape(R, A), sr, r64[:, A:].abs() + sr, key='head.mean_std')


# ====================================================================================== one-hot gather + LayerNorm
@pytest.mark.parametrize('N', [256, 260, 768, 1024, 12])
def test_onehot_gather_layernorm(L, N):
    """genrl_onehot_gather_ln_fwd at NV 1..4: xpre += the S gathered rows of wT (idx -1: nothing; one row all -1), then
    SiLU(LayerNorm); padded ldw / ldx / ldy"""
    M, S, K = 70, 32, 32
    g = gen(N)
    idx = torch.randint(0, K, (M, S), generator=g, dtype=torch.int32)
    idx[torch.rand(M, S, generator=g) < 0.2] = -1
    idx[3] = -1
    wT = torch.randn(S * K, N, generator=g) * 0.3
    xpre = torch.randn(M, N, generator=g) + 0.5
    gamma = 1 + 0.3 * torch.randn(N, generator=g); beta = 0.3 * torch.randn(N, generator=g)
    wd = in_buf(wT, N + 4)
    xb = torch.full(((M + 1) * (N + 8) + 4,), PAD, device='cuda')
    xd = xb[:M * (N + 8)].view(M, N + 8)[:, :N]
    xd.copy_(xpre)
    yb, y = out_buf(M, N, N + 12)
    mb, mean = vec_out(M); rb, rstd = vec_out(M)
    gd, bd, idd = gamma.cuda(), beta.cuda(), idx.cuda()
    rc = L.genrl_onehot_gather_ln_fwd(idd.data_ptr(), S, K, wd.data_ptr(), wd.stride(0), xd.data_ptr(), xd.stride(0), gd.data_ptr(),
                                      bd.data_ptr(), y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(), M, N, 1e-3, stream())
    assert rc == 0
    torch.cuda.synchronize()
    untouched('xpre', xb, xd); untouched('y', yb, y); untouched('mean', mb, mean); untouched('rstd', rb, rstd)
    sel = torch.zeros(M, N, dtype=torch.float64); ssel = sel.clone()
    for s in range(S):
        on = idx[:, s] >= 0
        rows = wT.double()[s * K + idx[:, s].clamp_min(0).long()]
        sel += torch.where(on[:, None], rows, 0.0); ssel += torch.where(on[:, None], rows.abs(), 0.0)
    xr = xpre.double() + sel
    within('gather.xpre', xd, xr, xpre.double().abs() + ssel)
    assert torch.equal(xd[3].cpu(), xpre[3])
    # the LayerNorm of the fp32 sum the kernel wrote back (its input)
    yr, mr, rr, sy, mabs = ln_fwd_ref(xd.cpu(), gamma, beta, 1e-3, 1)
    within('ln.y[gather]', y, yr, sy, key='ln.y')
    within('ln.mean[gather]', mean, mr, mabs, key='ln.mean')
    within('ln.rstd[gather]', rstd, rr, rr, key='ln.rstd')


# ====================================================================================== connector inputs, aligner loss
@pytest.mark.parametrize('nf', [1, 4, 8])
def test_connector_prep(L, nf):
    """clean = the last frame of each nf-frame chunk, noisy = normalize((1 - lam) clean + lam normalize(eps)) against float64
    F.normalize (one all-zero eps row: the 1e-12 clamp), the time-major action block [clean * cscale | 0 x nf]"""
    B, T, E, lam, cscale = 32, 32, 512, 0.3, 2.5
    g = gen(nf)
    video = torch.randn(B, T, E, generator=g); eps = torch.randn(B, T, E, generator=g)
    eps[2, 5] = 0
    vd, ed = video.cuda(), eps.cuda()
    cb, clean = out_buf(B * T, E, E); nb, noisy = out_buf(B * T, E, E)
    ab, act = out_buf(T * B, E + nf, E + nf)
    assert L.genrl_connector_prep(vd.data_ptr(), ed.data_ptr(), clean.data_ptr(), noisy.data_ptr(), act.data_ptr(), B, T, E, nf, lam, cscale,
                                  stream()) == 0
    torch.cuda.synchronize()
    untouched('clean', cb, clean); untouched('noisy', nb, noisy); untouched('act', ab, act)
    src = torch.arange(T) // nf * nf + nf - 1
    cr = video[:, src]
    assert torch.equal(clean.cpu().view(B, T, E), cr)
    a = act.cpu().view(T, B, E + nf)
    assert torch.equal(a[..., :E], (cr.double() * cscale).float().transpose(0, 1))
    assert (a[..., E:] == 0).all()
    m = (1 - lam) * cr.double() + lam * F.normalize(eps.double(), dim=-1)
    nr = F.normalize(m, dim=-1)
    sn = ((1 - lam) * cr.double().abs() + lam * F.normalize(eps.double(), dim=-1).abs()) / m.norm(dim=-1, keepdim=True) + nr.abs()
    within('conn.noisy', noisy.view(B, T, E), nr, sn)
    # ops wrapper: the same launch
    c2, n2, a2 = __import__('genrl_amd.ops', fromlist=['ops']).connector_prep(vd, ed, nf, lam, cscale)
    assert torch.equal(c2, clean.view(B, T, E)) and torch.equal(n2, noisy.view(B, T, E)) and torch.equal(a2, act.view(T, B, E + nf))


def test_connector_prep_refuses_partial_chunks(L):
    B, T, E = 2, 30, 64
    v = torch.zeros(B, T, E, device='cuda')
    out = torch.full((B * T * (E + 4),), float('nan'), device='cuda')
    assert L.genrl_connector_prep(v.data_ptr(), v.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), B, T, E, 4, 0.3, 1.0, stream()) == EINVAL
    torch.cuda.synchronize()
    assert out.isnan().all()


@pytest.mark.parametrize('R,E', [(64, 512), (33, 1000)])
def test_cosine_distance(L, R, E):
    """ops.cosine_distance forward and gradient against float64 1 - cosine_similarity(normalize(x), c).mean(), with one all-zero x row
    and one all-zero c row compared against what float64 torch does there"""
    from genrl_amd import ops
    g = gen(R + E)
    x = torch.randn(R, E, generator=g) * torch.exp(torch.randn(R, 1, generator=g)); c = torch.randn(R, E, generator=g)
    x[5] = 0
    c[9] = 0
    xd = x.cuda().requires_grad_()
    loss = ops.cosine_distance(xd, c.cuda())
    loss.backward(torch.tensor(1.5, device='cuda'))
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_()
    ref = 1 - F.cosine_similarity(F.normalize(x64, dim=-1), c.double(), dim=-1).mean()
    (1.5 * ref).backward()
    within('cos.loss', loss.detach().reshape(1), ref.detach().reshape(1), torch.full((1,), 2.0, dtype=torch.float64))
    # scale: sum of |terms| of -(g / R) (c^ / max(|r|, 1e-8) - cos r / |r|^2) / max(|x|, 1e-12)
    with torch.no_grad():
        xx, cc = x.double(), c.double()
        nx = xx.norm(dim=-1, keepdim=True).clamp_min(1e-12); rn = xx.norm(dim=-1, keepdim=True) / nx
        ch = cc / cc.norm(dim=-1, keepdim=True).clamp_min(1e-8)
        cos_abs = ((xx / nx).abs() * ch.abs()).sum(-1, keepdim=True) / rn.clamp_min(1e-8)      # (|cos| as a sum of |terms|)
        s = 1.5 / R * (ch.abs() / rn.clamp_min(1e-8) + torch.where(rn >= 1e-8, cos_abs * (xx / nx).abs() / rn.clamp_min(1e-8) ** 2, 0.0)) / nx
    within('cos.dx', xd.grad, x64.grad, s)
