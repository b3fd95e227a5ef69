"""The imagination update without the fp32 copies nobody reads, and with fewer dependent launches on the rollout's backward chain:
genrl_gru_gates_bwd_h2 / genrl_onehot_bwd_h2 with a NULL fp32 output (planes only), genrl_gemm_h2_pair (two products on one A operand
in one launch), the rollout backward through them (C launch loop and Python twin), the policy tape and the MLP trunk without fp32 hidden
activations.  Nothing here may change a bit: every comparison is torch.equal / a digest of the raw bytes."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lean_imag_rollout.json')
EINVAL = 1


@pytest.fixture(scope='module')
def env():
    from genrl_amd import planes, ops
    from genrl_amd._lib import lib, check
    return planes, ops, lib(), check


def _st():
    return torch.cuda.current_stream().cuda_stream


def _planes_equal(P, Q):
    return torch.equal(P.t, Q.t) and torch.equal(P.inv, Q.inv)


@pytest.mark.parametrize('R', [1, 5, 64])
@pytest.mark.parametrize('D', [256, 1024])
def test_gru_gates_bwd_without_fp32_dpre(env, R, D):
    planes, ops, L, check = env
    g = torch.Generator(device='cuda').manual_seed(100 * D + R)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
    pre, h, dout, d2 = rn(R, 3 * D), rn(R, D), rn(R, D), rn(R, D)
    gam, bet = rn(3 * D), rn(3 * D)
    mean, rstd = pre.mean(1).contiguous(), (pre.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    ws = torch.empty(L.genrl_gru_ws_floats(R, D), device='cuda')

    def run(with_dpre):
        dp = torch.full((R, 3 * D), float('nan'), device='cuda') if with_dpre else None
        dh = torch.empty(R, D, device='cuda')
        dg, db = torch.zeros(3 * D, device='cuda'), torch.zeros(3 * D, device='cuda')
        P = planes.Planes(R, 3 * D, 'cuda')
        check(L.genrl_gru_gates_bwd_h2(dout.data_ptr(), D, d2.data_ptr(), None, pre.data_ptr(), h.data_ptr(), D, gam.data_ptr(),
                                       bet.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dp.data_ptr() if with_dpre else None,
                                       dh.data_ptr(), D, dg.data_ptr(), db.data_ptr(), ws.data_ptr(), R, D, 0, None, 0, 0,
                                       P.ptr(), P.ld, P.plane, P.inv_ptr(), _st()), 'gru_gates_bwd_h2')
        return dp, dh, dg, db, P
    dp, dh0, dg0, db0, P0 = run(True)
    _, dh1, dg1, db1, P1 = run(False)
    assert torch.isfinite(dp).all()
    assert _planes_equal(P0, P1)
    assert torch.equal(dh0, dh1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)
    # no fp32 copy AND no planes: nothing would be written
    dh = torch.empty(R, D, device='cuda')
    rc = L.genrl_gru_gates_bwd_h2(dout.data_ptr(), D, None, None, pre.data_ptr(), h.data_ptr(), D, gam.data_ptr(), bet.data_ptr(),
                                  mean.data_ptr(), rstd.data_ptr(), None, dh.data_ptr(), D, None, None, None, R, D, 0, None, 0, 0,
                                  None, 0, 0, None, _st())
    assert rc == EINVAL
    rc = L.genrl_gru_gates_bwd(dout.data_ptr(), D, None, None, pre.data_ptr(), h.data_ptr(), D, gam.data_ptr(), bet.data_ptr(),
                               mean.data_ptr(), rstd.data_ptr(), None, dh.data_ptr(), D, None, None, None, R, D, 0, None, 0, 0, _st())
    assert rc == EINVAL


@pytest.mark.parametrize('rows', [1, 3, 64])
def test_onehot_bwd_without_fp32_dlogits(env, rows):
    planes, ops, L, check = env
    S, K = 32, 32
    SK = S * K
    g = torch.Generator(device='cuda').manual_seed(rows)
    lg = torch.randn(rows, SK, device='cuda', generator=g)
    gs = torch.randn(rows, SK, device='cuda', generator=g)

    def run(with_d):
        d = torch.full((rows, SK), float('nan'), device='cuda') if with_d else None
        P = planes.Planes(rows, SK, 'cuda')
        check(L.genrl_onehot_bwd_h2(lg.data_ptr(), gs.data_ptr(), d.data_ptr() if with_d else None, rows * S, K, 0.99, 0, P.ptr(), SK,
                                    P.ld, P.plane, P.inv_ptr(), _st()), 'onehot_bwd_h2')
        return d, P
    d0, P0 = run(True)
    _, P1 = run(False)
    assert torch.isfinite(d0).all() and _planes_equal(P0, P1)
    # accumulate reads the fp32 copy: NULL is refused; so is a plane row the kernel cannot write itself (second-pass split of dlogits)
    P = planes.Planes(rows, SK, 'cuda')
    assert L.genrl_onehot_bwd_h2(lg.data_ptr(), gs.data_ptr(), None, rows * S, K, 0.99, 1, P.ptr(), SK, P.ld, P.plane, P.inv_ptr(),
                                 _st()) == EINVAL
    P32 = planes.Planes(rows * 32, 32, 'cuda')
    assert L.genrl_onehot_bwd_h2(lg.data_ptr(), gs.data_ptr(), None, rows * S, K, 0.99, 0, P32.ptr(), 32, P32.ld, P32.plane,
                                 P32.inv_ptr(), _st()) == EINVAL
    assert L.genrl_onehot_bwd(lg.data_ptr(), gs.data_ptr(), None, rows * S, K, 0.99, 0, _st()) == EINVAL


@pytest.mark.parametrize('K', [64, 192])
@pytest.mark.parametrize('N0,N1', [(64, 64), (128, 64), (64, 200)])
@pytest.mark.parametrize('M', [1, 63, 64, 65, 192])
def test_gemm_h2_pair_is_two_gemm_h2(env, M, N0, N1, K):
    planes, ops, L, check = env
    g = torch.Generator(device='cuda').manual_seed(M * 1000 + N0 + N1 + K)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
    A = planes.split(rn(M, K) * torch.exp2(torch.randint(-6, 7, (M, 1), device='cuda', generator=g).float()))
    B0, B1 = planes.split(rn(N0, K) * 0.1), planes.split(rn(N1, K) * 3.0)
    G = 4                                               # guard columns behind each C's rows
    ld0, ld1 = N0 + G, (N1 + 3) // 4 * 4 + G
    fill0, fill1 = rn(M, ld0), rn(M, ld1)
    for acc0 in (0, 1):
        for acc1 in (0, 1):
            r0, r1, p0, p1 = fill0.clone(), fill1.clone(), fill0.clone(), fill1.clone()
            planes.gemm(A, B0, r0, ld0, None, M, N0, accumulate=bool(acc0))
            planes.gemm(A, B1, r1, ld1, None, M, N1, accumulate=bool(acc1))
            check(L.genrl_gemm_h2_pair(A.ptr(), A.ld, A.plane, A.inv_ptr(), A.ld,
                                       B0.ptr(), B0.ld, B0.plane, B0.inv_ptr(), p0.data_ptr(), ld0, N0, acc0,
                                       B1.ptr(), B1.ld, B1.plane, B1.inv_ptr(), p1.data_ptr(), ld1, N1, acc1, M, _st()), 'gemm_h2_pair')
            assert torch.equal(p0, r0) and torch.equal(p1, r1), (acc0, acc1)
            assert torch.equal(p0[:, N0:], fill0[:, N0:]) and torch.equal(p1[:, N1:], fill1[:, N1:])      # guards untouched
            assert not torch.equal(p0[:, :N0], fill0[:, :N0]) and not torch.equal(p1[:, :N1], fill1[:, :N1])


def test_gemm_h2_pair_refuses_a_ragged_first_product(env):
    planes, ops, L, check = env
    M, K = 64, 64
    A, B0, B1 = planes.Planes(M, K, 'cuda'), planes.Planes(96, K, 'cuda'), planes.Planes(64, K, 'cuda')
    C0, C1 = torch.zeros(M, 96, device='cuda'), torch.zeros(M, 64, device='cuda')
    rc = L.genrl_gemm_h2_pair(A.ptr(), A.ld, A.plane, A.inv_ptr(), A.ld, B0.ptr(), B0.ld, B0.plane, B0.inv_ptr(), C0.data_ptr(), 96, 96, 0,
                              B1.ptr(), B1.ld, B1.plane, B1.inv_ptr(), C1.data_ptr(), 64, 64, 0, M, _st())
    assert rc == EINVAL
    assert (C0 == 0).all() and (C1 == 0).all()


@pytest.mark.parametrize('N0,N1', [(1024, 512), (64, 448)])
def test_gemm_h2_pair_xcd_aware_order(env, N0, N1):
    """grids that take the XCD-aware tile order (8 row panels): 16 + 8 column tiles -- both products' tiles dealt to each of the 4 XCD
    columns -- and 1 + 7, which do not divide by 4: the products' tiles stay in launch order"""
    planes, ops, L, check = env
    g = torch.Generator(device='cuda').manual_seed(11)
    M, K = 512, 128
    A = planes.split(torch.randn(M, K, device='cuda', generator=g))
    B0, B1 = planes.split(torch.randn(N0, K, device='cuda', generator=g)), planes.split(torch.randn(N1, K, device='cuda', generator=g))
    r0, r1 = torch.randn(M, N0, device='cuda', generator=g), torch.randn(M, N1, device='cuda', generator=g)
    p0, p1 = r0.clone(), r1.clone()
    planes.gemm(A, B0, r0, N0, None, M, N0, accumulate=True)
    planes.gemm(A, B1, r1, N1, None, M, N1)
    planes.gemm_pair(A, B0, p0, N0, N0, True, B1, p1, N1, N1, False, M)
    assert torch.equal(p0, r0) and torch.equal(p1, r1)


# ---- the rollout's backward as a whole
def rollout_case(A, with_dlogit, with_daction, seq_c, U=256, hold=None):
    """-> {name: gradient} of one plane rollout (H = 3, N = 64, U = D, S K = 256) and its backward; every random input from fixed seeds.
    Uses only what the rollout's callers use, so that it also runs on the revision before this file to record the golden digests."""
    from genrl_amd import ops, ops_planes
    H, N, S, K = 3, 64, 8, 32
    D, SK = U, S * K
    g = torch.Generator(device='cuda').manual_seed(7 + A)
    rn = lambda *s, sc=1.0: (torch.randn(*s, device='cuda', generator=g) * sc)
    # (nn.Parameters, as in the product: their weight planes live in the planes cache -- the C loop is handed pointers, not handles)
    par = lambda *s, sc=1.0, off=0.0: torch.nn.Parameter(off + rn(*s, sc=sc))
    w = lambda o, i: torch.nn.Parameter(rn(o, i, sc=i ** -0.5), requires_grad=False)
    layers = [(par(U, SK + D, sc=(SK + D) ** -0.5), par(U, sc=0.1), par(U, sc=0.1, off=1.0), par(U, sc=0.1), 1e-3),
              (par(U, U, sc=U ** -0.5), par(U, sc=0.1), par(U, sc=0.1, off=1.0), par(U, sc=0.1), 1e-3)]
    head_w, head_b = par(2 * A, U, sc=U ** -0.5), par(2 * A, sc=0.1)
    seq_was = ops.SEQ_C
    ops.SEQ_C = seq_c
    try:
        tape = ops_planes.ActorTapePlanes(H, N, layers, head_w, head_b, 'cuda')
        spec = ops.RolloutSpec(tape, w(U, SK + A), rn(U, sc=0.1), 1.0 + rn(U, sc=0.1), rn(U, sc=0.1), 1e-3,
                               w(3 * D, U + D), 1.0 + rn(3 * D, sc=0.1), rn(3 * D, sc=0.1),
                               w(U, D), rn(U, sc=0.1), 1.0 + rn(U, sc=0.1), rn(U, sc=0.1), 1e-3, w(SK, U), rn(SK, sc=0.1), S, K, 0.1, 1.0)
        idx = torch.randint(0, K, (N, S), device='cuda', generator=g)
        stoch0 = torch.nn.functional.one_hot(idx, K).float()
        deter0, logit0 = torch.tanh(rn(N, D)), rn(N, S, K)
        eps = rn(H, N, A)
        q = torch.rand(H, N, S, K, device='cuda', generator=g) * 0.9 + 0.05
        st, de, lg, ac, raw = ops_planes.imagine_rollout(stoch0, deter0, logit0, eps, q, spec)
        loss = (st * rn(*st.shape)).sum() + (de * rn(*de.shape)).sum() + (raw * rn(*raw.shape)).sum()
        wl, wa = rn(*lg.shape), rn(*ac.shape)
        if with_dlogit:
            loss = loss + (lg * wl).sum()
        if with_daction:
            loss = loss + (ac * wa).sum()
        loss.backward()
    finally:
        ops.SEQ_C = seq_was
    if hold is not None:
        hold.append(tape)
    out = {'head_w': head_w.grad, 'head_b': head_b.grad, 'd_raw': tape.d_raw}
    for l, lay in enumerate(layers):
        for n, t in zip(('W', 'b', 'gamma', 'beta'), lay[:4]):
            out[f'l{l}.{n}'] = t.grad
    return out


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def case_key(A, with_dlogit, with_daction, U=256):
    return f'A{A}.dlogit{int(with_dlogit)}.daction{int(with_daction)}.U{U}'


ROLLOUT_CASES = [(A, dl, da, 256) for A in (1, 10) for dl in (False, True) for da in (False, True)] + [(10, False, False, 320)]


@pytest.mark.parametrize('A,with_dlogit,with_daction,U', ROLLOUT_CASES)
def test_rollout_backward_c_loop_python_twin_and_parent_values(A, with_dlogit, with_daction, U):
    """the C launch loop (genrl_imagine_seq_bwd) and its Python twin return the same bits, and both the bits the revision before the lean
    stores / the pair product / the single head backward returned (tests/golden/lean_imag_rollout.json: SHA-256 of each gradient's bytes,
    recorded once on that revision with this file's rollout_case)"""
    hold = []
    gc = rollout_case(A, with_dlogit, with_daction, True, U, hold)
    gp = rollout_case(A, with_dlogit, with_daction, False, U)
    assert set(gc) == set(gp)
    for n in gc:
        assert gc[n] is not None and torch.isfinite(gc[n]).all(), n
        assert torch.equal(gc[n], gp[n]), n
    if U > 256:           # (the hidden layer's fp32 copy has no reader left: its weight gradient takes the planes)
        assert hold[0].y[0] is None and hold[0].y[-1] is not None
    else:
        assert all(y is not None for y in hold[0].y)
    want = json.load(open(GOLDEN))[case_key(A, with_dlogit, with_daction, U)]
    assert set(want) == set(gc)
    for n in gc:
        assert digest(gc[n]) == want[n], n


# ---- the MLP trunk as one node
def _trunk_params(K_in, widths, frozen):
    g = torch.Generator(device='cuda').manual_seed(5)
    rn = lambda *s, sc=1.0: torch.randn(*s, device='cuda', generator=g) * sc
    layers, k = [], K_in
    for n in widths:
        lay = [rn(n, k, sc=k ** -0.5), rn(n, sc=0.1), 1.0 + rn(n, sc=0.1), rn(n, sc=0.1)]
        layers.append(tuple(t.requires_grad_(not frozen) for t in lay) + (1e-3,))
        k = n
    return layers


def _trunk_run(one_node, two_inputs, with_planes, frozen):
    """-> (output, hidden fp32 copies kept by the node | None, gradients) of a 3-layer Dense -> LayerNorm -> SiLU trunk over 128 rows"""
    from genrl_amd import ops_planes, planes
    M, widths = 128, (512, 320, 512)
    K1, K2 = (192, 128) if two_inputs else (320, 0)
    g = torch.Generator(device='cuda').manual_seed(6)
    x1 = torch.randn(M, K1, device='cuda', generator=g).requires_grad_(True)
    x2 = torch.randn(M, K2, device='cuda', generator=g).requires_grad_(True) if two_inputs else None
    wgt = torch.randn(M, widths[-1], device='cuda', generator=g)
    layers = _trunk_params(K1 + K2, widths, frozen)
    hp = None
    if with_planes:
        hp = ((planes.split(x1.detach()), 0),) + (((planes.split(x2.detach()), 0),) if two_inputs else ())
    if one_node:
        y = ops_planes.dense_ln_trunk(x1, x2, layers, planes=hp)
        hidden = y.grad_fn.hidden_y
    else:
        y, a2, h = x1, x2, hp
        for W, b, ga, be, eps in layers:
            y = ops_planes.dense_ln_act(y, a2, W, b, ga, be, eps, planes=h)
            a2 = h = None
        hidden = None
    assert y._planes[0].cols == widths[-1]
    yp = y._planes[0]
    (y * wgt).sum().backward()
    grads = {'x1': x1.grad, 'x2': x2.grad if two_inputs else None}
    for l, lay in enumerate(layers):
        for n, t in zip(('W', 'b', 'gamma', 'beta'), lay[:4]):
            grads[f'l{l}.{n}'] = t.grad
    return y.detach(), yp, hidden, grads


@pytest.fixture(scope='module')
def trunk_book():
    """tests/golden/lean_imag_trunk.json: the digests of the PER-LAYER chain's output, planes and gradients on the revision where that chain
    and the one-node trunk were two separate implementations (they share their products since: the recorded values keep the comparison
    below anchored to an independent one)"""
    from test_gpu_dense_nodes import Book
    b = Book('lean_imag_trunk.json')
    yield b
    b.save()


def _check_parent_trunk(book, key, one_node, chain):
    for y, p, g in (one_node, chain):             # (recording keeps the last: the per-layer chain's)
        book.check(key, {'y': digest(y), 'planes.t': digest(p.t), 'planes.inv': digest(p.inv),
                         **{n: (digest(t) if t is not None else None) for n, t in g.items()}})


@pytest.mark.parametrize('frozen', [False, True])
@pytest.mark.parametrize('with_planes', [False, True])
@pytest.mark.parametrize('two_inputs', [False, True])
def test_trunk_node_is_the_per_layer_chain_without_fp32_hidden_activations(trunk_book, two_inputs, with_planes, frozen):
    """(the suite runs with GENRL_TN_MIN_ROWS=64: at 128 rows every weight gradient takes the plane kernel)"""
    y1, p1, hidden, g1 = _trunk_run(True, two_inputs, with_planes, frozen)
    y0, p0, _, g0 = _trunk_run(False, two_inputs, with_planes, frozen)
    assert torch.equal(y1, y0) and _planes_equal(p1, p0)
    assert hidden == [None, None]            # no (M, width) fp32 hidden activation exists: the last layer's output is the node's result
    assert set(g1) == set(g0)
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None), n
        if g0[n] is not None:
            assert torch.equal(g1[n], g0[n]), n
    assert g1['x1'] is not None and (frozen or g1['l0.W'] is not None)
    _check_parent_trunk(trunk_book, f'two{int(two_inputs)}.planes{int(with_planes)}.frozen{int(frozen)}', (y1, p1, g1), (y0, p0, g0))


@pytest.mark.parametrize('frozen', [False, True])
def test_trunk_node_below_the_plane_weight_gradient_threshold(monkeypatch, trunk_book, frozen):
    """below planes.tn_min_rows() the weight gradients read the fp32 hidden activations: the node keeps them -- unless the weights are
    frozen (a slow critic), where nobody reads them at any row count"""
    monkeypatch.setenv('GENRL_TN_MIN_ROWS', '256')
    y1, p1, hidden, g1 = _trunk_run(True, True, True, frozen)
    y0, p0, _, g0 = _trunk_run(False, True, True, frozen)
    assert torch.equal(y1, y0) and _planes_equal(p1, p0)
    if frozen:
        assert hidden == [None, None]
    else:
        assert [tuple(h.shape) for h in hidden] == [(128, 512), (128, 320)]
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None), n
        if g0[n] is not None:
            assert torch.equal(g1[n], g0[n]), n
    _check_parent_trunk(trunk_book, f'tn256.frozen{int(frozen)}', (y1, p1, g1), (y0, p0, g0))
