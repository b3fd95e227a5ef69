"""The flat forward and backward kernels that the three continuous actor heads share (csrc/heads.hip: head_fwd_kernel<Head>,
head_bwd_kernel<Head>; the heads themselves in csrc/actor_heads.h), through the C entry points of each head.  The kernels are the one place
where the heads' indexing lives -- element i -> row r, column a; raw[r, a] and raw[r, A + a]; action rows ld_action apart -- so every head is
run with tight and padded action rows, with noise and without (eps NULL: the mode), at one element, and at 65 x 7 = 455 elements (a second
256-thread workgroup, a partial one).

Nothing here states a formula or a tolerance of its own.  Each head is compared with the float64 restatement of its own kernel test, under
that test's bound, scales and inputs: test_gpu_row_kernel_variants.py for the Normal head (head_ref, head_scale and the K of 'head.*'),
test_gpu_v2_kernels.py for the truncated-normal head (v2_restatement.trunc_normal; 2 x the float32 restatement's own error with that test's
floors), test_gpu_tanh_kernels.py for the squashed head (tanh_restatement.sample / sample_bwd).  The Normal head's gradient has no flat test
there; it takes the bound of the linear-fused backward at a product of one term, d action = g x 1 (so the magnitude of the product's terms
is |g|).  The arithmetic has no tail to exclude: every element is compared.  The action buffer is NaN inside PAD-filled padding columns and
a guard row, all of which must come back bit for bit."""
import pytest
import torch

import test_gpu_row_kernel_variants as NV
import test_gpu_tanh_kernels as TH
import test_gpu_v2_kernels as V2
from f64check import in_buf, out_buf, untouched

pytestmark = pytest.mark.gpu

HEADS = ['normal', 'trunc_normal', 'tanh_normal']
TN = (0.1, 0.0)            # min_std, init_std of test_gpu_v2_kernels.py's truncated-normal cases


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    return lib()


def inputs(head, Rn, A):
    """raw, eps, daction as the head's own test draws them"""
    g = torch.Generator().manual_seed(1000 * HEADS.index(head) + 10 * Rn + A)
    width = {'normal': 2.0, 'trunc_normal': 1.5, 'tanh_normal': 1.0}[head]
    raw = torch.randn(Rn, 2 * A, generator=g) * width
    eps = torch.randn(Rn, A, generator=g) * (1.5 if head == 'trunc_normal' else 1.0)
    return raw, eps, torch.randn(Rn, A, generator=g)


def trunc_restate(raw, eps, dact, dtype):
    A = eps.shape[1]
    r = raw.to(dtype).clone().requires_grad_(True)
    a, mean, std, _ = V2.R.trunc_normal(r[:, :A], r[:, A:], eps.to(dtype), *TN)
    (a * dact.to(dtype)).sum().backward()
    return a.detach(), mean.detach(), std.detach(), r.grad


def check_forward(head, tag, raw, e, act, mean, std):
    """e: the noise, zeros for the mode (every restatement's x = mean + std e is then the mean itself)"""
    A = e.shape[1]
    r64, e64 = raw.double(), e.double()
    if head == 'normal':
        ar, mr, sr = NV.head_ref(r64, e64)
        NV.within('head.action' + tag, act, ar, NV.head_scale(r64[:, :A].abs(), r64[:, A:].abs(), e64, mr, sr))
        NV.within('head.mean_std[mean]' + tag, mean, mr, r64[:, :A].abs() + mr.abs(), key='head.mean_std')
        NV.within('head.mean_std[std]' + tag, std, sr, r64[:, A:].abs() + sr, key='head.mean_std')
    elif head == 'trunc_normal':
        a64, m64, s64, _ = trunc_restate(raw, e, torch.ones_like(e), torch.float64)
        a32, m32, s32, _ = trunc_restate(raw, e, torch.ones_like(e), torch.float32)
        V2.bounded('tn.mean' + tag, mean, m64, m32, r64[:, :A].abs() + m64.abs(), 4.0)
        V2.bounded('tn.std' + tag, std, s64, s32, r64[:, A:].abs() + s64, 4.0)
        V2.bounded('tn.action' + tag, act, a64, a32, m64.abs() + e64.abs() * s64, 8.0)
    else:
        a64, _, m64, s64 = TH.R.sample(r64, e64, *TH.P)
        a32, _, m32, s32 = TH.R.sample(raw, e, *TH.P)
        TH.bounded('head.mean' + tag, mean, m64, m32, m64.abs())
        TH.bounded('head.std' + tag, std, s64, s32, s64.abs())
        TH.bounded('head.action' + tag, act, a64, a32, TH.R.tanh_scale(r64, e64, *TH.P))


@pytest.mark.parametrize('noise', [True, False])
@pytest.mark.parametrize('pad', [0, 5])
@pytest.mark.parametrize('A', [1, 7])
@pytest.mark.parametrize('Rn', [1, 65])
@pytest.mark.parametrize('head', HEADS)
def test_flat_forward(L, head, Rn, A, pad, noise):
    from genrl_amd._lib import check
    raw, eps, _ = inputs(head, Rn, A)
    rd, ed = raw.cuda(), eps.cuda()
    ld = A + pad
    (ab, act), (mb, mean), (sb, std) = out_buf(Rn, A, ld), out_buf(Rn, A, A), out_buf(Rn, A, A)
    fwd = {'normal': (L.genrl_actor_head_fwd, (NV.MIN_STD, NV.MAX_STD)), 'trunc_normal': (L.genrl_trunc_normal_head_fwd, TN),
           'tanh_normal': (L.genrl_tanh_normal_head_fwd, TH.P)}[head]
    check(fwd[0](rd.data_ptr(), ed.data_ptr() if noise else None, act.data_ptr(), mean.data_ptr(), std.data_ptr(), Rn, A, *fwd[1], ld,
                 stream()), head + ' forward')
    torch.cuda.synchronize()
    untouched('action', ab, act); untouched('mean', mb, mean); untouched('std', sb, std)
    check_forward(head, f'[{Rn}x{A},ld {ld},{"eps" if noise else "mode"}]', raw, eps if noise else torch.zeros_like(eps), act, mean, std)


@pytest.mark.parametrize('pad', [0, 5])
@pytest.mark.parametrize('A', [1, 7])
@pytest.mark.parametrize('Rn', [1, 65])
@pytest.mark.parametrize('head', HEADS)
def test_flat_backward(L, head, Rn, A, pad):
    from genrl_amd._lib import check
    raw, eps, dact = inputs(head, Rn, A)
    rd, ed = raw.cuda(), eps.cuda()
    ld = A + pad
    gd = in_buf(dact, ld)
    db, draw = out_buf(Rn, 2 * A, 2 * A)
    if head == 'normal':
        rc = L.genrl_actor_head_bwd(gd.data_ptr(), rd.data_ptr(), ed.data_ptr(), draw.data_ptr(), Rn, A, NV.MIN_STD, NV.MAX_STD, ld, stream())
    elif head == 'trunc_normal':
        rc = L.genrl_trunc_normal_head_bwd(gd.data_ptr(), rd.data_ptr(), ed.data_ptr(), draw.data_ptr(), Rn, A, TN[1], ld, stream())
    else:
        rc = L.genrl_tanh_normal_head_bwd(gd.data_ptr(), rd.data_ptr(), ed.data_ptr(), draw.data_ptr(), Rn, A, *TH.P, ld, stream())
    check(rc, head + ' backward')
    torch.cuda.synchronize()
    untouched('draw', db, draw)
    tag = f'[{Rn}x{A},ld {ld}]'
    r64, e64, g64 = raw.double(), eps.double(), dact.double()
    if head == 'normal':
        r = r64.clone().requires_grad_()
        NV.head_ref(r, e64)[0].backward(g64)
        s = g64.abs() + g64.abs()            # test_actor_head_linear_backward's s = (sum |dx| |WaT|) + |d action| at d action = g x 1
        NV.within('head.draw' + tag, draw, r.grad, torch.cat([s, s * e64.abs() * 0.25 * (NV.MAX_STD - NV.MIN_STD)], 1))
    elif head == 'trunc_normal':
        _, m64, _, d64 = trunc_restate(raw, eps, dact, torch.float64)
        d32 = trunc_restate(raw, eps, dact, torch.float32)[3]
        sgm = torch.sigmoid((r64[:, A:] + TN[1]) / 2)
        scale = torch.cat([g64.abs() * (1 + m64 ** 2), (g64 * e64).abs() * sgm * (1 + sgm)], 1) + V2.TINY
        V2.bounded('tn.draw' + tag, draw, d64, d32, scale, 8.0)
    else:
        d64, scale = TH.R.sample_bwd(g64, r64, e64, *TH.P)
        TH.bounded('head.draw' + tag, draw, d64, TH.R.sample_bwd(dact, raw, eps, *TH.P)[0], scale)
