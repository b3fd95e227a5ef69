"""The kernels behind the connector's switches against float64 torch: genrl_connector_prep_slots (the fused input kernel with the
frame-slot columns chosen) and genrl_tf_inputs_{fwd,bwd} (the teacher-forced input under token dropout).  The slot columns and everything
tf_inputs writes are copied or zeroed values: compared with `==`.  The other outputs of the prep kernel are held to the bounds
test_gpu_row_kernel_variants.py::test_connector_prep uses (its `within`, its K)."""
import pytest
import torch
import torch.nn.functional as F

from f64check import out_buf, untouched
from test_gpu_row_kernel_variants import within, gen, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    return lib()


@pytest.mark.parametrize('nf', [4, 8])
@pytest.mark.parametrize('E', [40, 256, 300, 512])
def test_connector_prep_slots(L, E, nf):
    """temporal off: bit for bit the old entry's three outputs; on: the slot columns are one_hot(t % nf), exactly 0 / 1, and clean, noisy
    and the embedding columns of the actions do not move"""
    from genrl_amd import ops
    B, T, lam, cscale = 3, 16, 0.3, 2.5
    g = gen(E + nf)
    video = torch.randn(B, T, E, generator=g); eps = torch.randn(B, T, E, generator=g)
    eps[2, 5] = 0
    vd, ed = video.cuda(), eps.cuda()
    outs = {}
    for name, call in (('old', lambda *a: L.genrl_connector_prep(*a, stream())), ('off', lambda *a: L.genrl_connector_prep_slots(*a, 0, stream())),
                       ('on', lambda *a: L.genrl_connector_prep_slots(*a, 1, stream()))):
        cb, clean = out_buf(B * T, E, E); nb, noisy = out_buf(B * T, E, E)
        ab, act = out_buf(T * B, E + nf, E + nf)
        assert call(vd.data_ptr(), ed.data_ptr(), clean.data_ptr(), noisy.data_ptr(), act.data_ptr(), B, T, E, nf, lam, cscale) == 0
        torch.cuda.synchronize()
        untouched('clean', cb, clean); untouched('noisy', nb, noisy); untouched('act', ab, act)
        outs[name] = (clean.cpu().view(B, T, E), noisy.cpu().view(B, T, E), act.cpu().view(T, B, E + nf))
    for a, b in zip(outs['old'], outs['off']):
        assert torch.equal(a, b)
    assert torch.equal(outs['on'][0], outs['old'][0]) and torch.equal(outs['on'][1], outs['old'][1])
    assert torch.equal(outs['on'][2][..., :E], outs['old'][2][..., :E])
    slots = outs['on'][2][..., E:]
    assert ((slots == 0) | (slots == 1)).all() and (outs['old'][2][..., E:] == 0).all()
    assert torch.equal(slots, F.one_hot(torch.arange(T) % nf, nf).float()[:, None].expand(T, B, nf))
    # the remaining outputs against float64, as test_connector_prep states them
    src = torch.arange(T) // nf * nf + nf - 1
    cr = video[:, src]
    clean, noisy, act = outs['on']
    assert torch.equal(clean, cr) and torch.equal(act[..., :E], (cr.double() * cscale).float().transpose(0, 1))
    m = (1 - lam) * cr.double() + lam * F.normalize(eps.double(), dim=-1)
    nr = F.normalize(m, dim=-1)
    sn = ((1 - lam) * cr.double().abs() + lam * F.normalize(eps.double(), dim=-1).abs()) / m.norm(dim=-1, keepdim=True) + nr.abs()
    within('conn.noisy', noisy, nr, sn)
    # the ops wrapper: the keyword selects the launch, its default is the old entry
    for kw, want in (({}, 'old'), (dict(temporal=False), 'old'), (dict(temporal=True), 'on')):
        got = ops.connector_prep(vd, ed, nf, lam, cscale, **kw)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, outs[want]))


def tf_reference(first, post, keep):
    """float64 torch: x (T, B, W) from first (B, W), post (B, T, W), keep (T, B)"""
    shifted = torch.cat([first[None], post.transpose(0, 1)[:-1]], 0)
    return shifted * keep[..., None]


@pytest.mark.parametrize('W', [16, 20, 1024])
def test_tf_inputs_forward_and_backward(L, W):
    """every T in {1, 2, 16} and B in {1, 5}; thresholds that keep every row, drop every row, and mix; dpost asked for and NULL; bases
    that are 16-byte aligned (float4 rows) and one float off (scalar rows).  Exact: values are copied or zeroed."""
    for T in (1, 2, 16):
        for B in (1, 5):
            g = gen(W * 100 + T * 10 + B)
            first, post = torch.randn(B, W, generator=g), torch.randn(B, T, W, generator=g)
            e = torch.empty(T, B).exponential_(1.0, generator=g)
            grad = torch.randn(T, B, W, generator=g)
            srt = e.flatten().sort().values
            middle = float((srt[T * B // 2 - 1] + srt[T * B // 2]) / 2) if T * B > 1 else 1e30          # between the two middle draws
            for what, thresh in (('all kept', 1e30), ('all dropped', 0.0), ('mixed', middle)):
                keep = (e < thresh).double()
                if what == 'mixed' and T * B > 1:
                    assert 0 < keep.sum() < T * B
                f64 = first.double().requires_grad_(); p64 = post.double().requires_grad_()
                ref = tf_reference(f64, p64, keep)
                ref.backward(grad.double())
                for off in (0, 1):
                    xb, x = out_buf(T * B, W, W, off); kb, kp = out_buf(1, T * B, T * B)
                    fd = torch.empty(B * W + 4, device='cuda')[off:off + B * W].copy_(first.reshape(-1))
                    pd = torch.empty(B * T * W + 4, device='cuda')[off:off + B * T * W].copy_(post.reshape(-1))
                    ed = e.cuda()
                    assert L.genrl_tf_inputs_fwd(fd.data_ptr(), pd.data_ptr(), ed.data_ptr(), thresh, B, T, W, x.data_ptr(), kp.data_ptr(),
                                                 stream()) == 0
                    torch.cuda.synchronize()
                    untouched('x', xb, x); untouched('keep', kb, kp)
                    assert torch.equal(kp.cpu().view(T, B).double(), keep), what
                    assert torch.equal(x.cpu().view(T, B, W).double(), ref.detach()), (what, T, B, off)
                    gd = torch.empty(T * B * W + 4, device='cuda')[off:off + T * B * W].copy_(grad.reshape(-1))
                    keepd = kp.reshape(-1).contiguous()
                    for want_dpost in (True, False):
                        fb, df = out_buf(B, W, W, off); pb, dp = out_buf(B * T, W, W, off)
                        assert L.genrl_tf_inputs_bwd(gd.data_ptr(), keepd.data_ptr(), B, T, W, df.data_ptr(),
                                                     dp.data_ptr() if want_dpost else None, stream()) == 0
                        torch.cuda.synchronize()
                        untouched('dfirst', fb, df)
                        assert torch.equal(df.cpu().double(), f64.grad), (what, T, B, off)
                        if want_dpost:
                            untouched('dpost', pb, dp)
                            assert torch.equal(dp.cpu().view(B, T, W).double(), p64.grad), (what, T, B, off)
                            assert (dp.cpu().view(B, T, W)[:, T - 1] == 0).all()
                        else:
                            untouched('dpost', pb, dp)
                            assert dp.isnan().all()


@pytest.mark.parametrize('post_grad', [True, False])
def test_tf_inputs_autograd_node(post_grad):
    """ops.tf_inputs(first, post, e, p): keep = e < -log p (u = exp(-e) > p), x and the gradients of float64 torch; post's gradient is
    computed only when post asks for one"""
    from genrl_amd import ops
    B, T, W, p = 5, 16, 20, 0.25
    g = gen(7)
    first, post = torch.randn(B, W, generator=g), torch.randn(B, T, W, generator=g)
    e = torch.empty(T, B).exponential_(1.0, generator=g)
    grad = torch.randn(T, B, W, generator=g)
    keep = (torch.exp(-e.double()) > p).double()
    assert 0 < keep.sum() < T * B and (torch.exp(-e.double()) - p).abs().min() > 1e-4
    fd, pd = first.cuda().requires_grad_(), post.cuda().requires_grad_(post_grad)
    x, kp = ops.tf_inputs(fd, pd, e.cuda(), p)
    assert x.shape == (T, B, W) and kp.shape == (T, B) and not kp.requires_grad
    x.backward(grad.cuda())
    torch.cuda.synchronize()
    f64, p64 = first.double().requires_grad_(), post.double().requires_grad_()
    ref = tf_reference(f64, p64, keep)
    ref.backward(grad.double())
    assert torch.equal(kp.cpu().double(), keep) and torch.equal(x.detach().cpu().double(), ref.detach())
    assert torch.equal(fd.grad.cpu().double(), f64.grad)
    assert (pd.grad is None) if not post_grad else torch.equal(pd.grad.cpu().double(), p64.grad)


def test_tf_inputs_refuses_bad_arguments(L):
    out = torch.full((64,), float('nan'), device='cuda')
    z = torch.zeros(64, device='cuda')
    for B, T, W in ((0, 2, 4), (2, 0, 4), (2, 2, 0)):
        assert L.genrl_tf_inputs_fwd(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1.0, B, T, W, out.data_ptr(), out.data_ptr(), stream()) == 1
        assert L.genrl_tf_inputs_bwd(z.data_ptr(), z.data_ptr(), B, T, W, out.data_ptr(), None, stream()) == 1
    assert L.genrl_tf_inputs_fwd(None, z.data_ptr(), z.data_ptr(), 1.0, 2, 2, 4, out.data_ptr(), out.data_ptr(), stream()) == 1
    assert L.genrl_tf_inputs_bwd(z.data_ptr(), z.data_ptr(), 2, 2, 4, None, None, stream()) == 1
    torch.cuda.synchronize()
    assert out.isnan().all()
    with pytest.raises(AssertionError):
        __import__('genrl_amd.ops', fromlist=['ops']).tf_inputs(z[:8].view(2, 4), z[:16].view(2, 2, 4), z[:4].view(2, 2), 0.0)
