"""The direct convolution kernels of csrc/conv.hip where their loops repeat, and its patch movers bit for bit.

The six MFMA kernels at the 3-channel ends of the networks run under a grid cap and walk the rest of their work in a loop; the
other kernel tests (test_gpu_conv_planes.py) stop at one trip per wave.  Here they are called through the C ABI (no dependence on
ops.CONVT_DIRECT* / CONV1_DIRECT or the environment) at shapes that make the loops repeat; test_case_table restates the launch
arithmetic in Python, needs no GPU and asserts that every shape still reaches what it is there for (move a cap -> move the shapes):

  convT forward (convt_small_co_fwd_kernel, cap 1280 workgroups = 5120 waves)
    400x7x33 Co 3 NCHW   10800 blocks: 3 trips (PAR 0, 1, 0: both register sets, the `more` prefetch of the next block twice), sbx 2
                         and row step 5 (both carries of the index walk), a 3-position last block per row, Wo = 70: scalar stores
    400x7x34 Co 3 NCHW   the same walk, Wo = 72: the 16-byte stores
    400x7x34 Co 4 NHWC   the same walk, all 16 MFMA columns, the NHWC epilogue
    180x7x66, 180x7x67   8100 blocks: 2 trips (the loop leaves through its inner break), bpr 5
    4x30x30, 5x30x30 NHWC Co 3   one trip: a failure here is the block, not the loop
  convT dgrad (convt_small_co_dgrad_kernel, cap 768 workgroups = 3072 waves)
    180x7x66             6300 blocks: 3 trips, sbx 2, row step 5, the cur <- nxt hand-over twice
    180x7x67             the same walk with a 3-pixel last block per row
    4x30x30              one trip
  convT wgrad, staged (convt_small_co_wgrad_lds_kernel, Wo % 4 == 0; 2048 waves, 512 partials)
    180x7x66             6300 chunks, per 4: store_chunk after load_chunk three times per wave, shares that cross image rows and
                         images, 118 idle workgroups that must write a zero partial into a NaN-filled workspace
    4x30x30              per 1
  convT wgrad, unstaged (convt_small_co_wgrad_kernel)
    180x7x67             21420 groups of 4 pixels, per 11 (odd: the a0/a1 alternation ends on a0), a 3-pixel last group per row, 100
                         idle waves, 25 idle workgroups
    3x13x9               per 1
  conv1 forward (conv1_u8_fwd_kernel, cap 1024 workgroups = 4096 waves)
    460x14x68            Ho 6, Wo 33: 8280 blocks, 3 trips, sbx 1, row step 3, a 1-pixel last block per row
    8x64x64              one trip
  conv1 wgrad (conv1_u8_wgrad_kernel, 2048 waves, 512 partials)
    460x14x68            8280 chunks, per 5, shares across rows and images, 98 idle workgroups
    8x64x64              per 1

Every case runs on two kinds of input.  EXACT: x, W, b, dy are integers in [-3, 3], frames have pixels in {0, 255} ((float)p / 255 -
0.5 is exactly -+0.5), so every partial sum is a multiple of 0.5 far below 2^24, every summation order gives the same fp32 value
and the kernel must equal the float64 reference under torch.equal: a block computed from the wrong row, a group counted twice or
skipped at a share boundary, a stale register set or an unwritten partial all fail it.  RANDOM: randn / randint(0, 256), per
element |kernel - float64| <= K 2^-24 S, S = the float64 sum of |term| (with |bias|), K = the number of fp32 additions on the
longest path into the element -- derived, worst-case, loose on purpose, not to be tightened from the measurements:

  kernel                   K                      largest ratio |kernel - float64| / (2^-24 S) measured on an MI355X
  convT forward            433                    6.14
  convT dgrad              112                    5.67
  conv1 forward            49                     5.44
  convT wgrad, staged      pixels summed + 516    0.45 at 3600 pixels (K 4116), 0.249 at 83160 (K 83676)
  convT wgrad, unstaged    pixels summed + 516    1.14 at 351 pixels (K 867), 0.216 at 84420 (K 84936)
  conv1 wgrad              pixels summed + 516    0.363 at 7688 pixels (K 8204), 0.176 at 91080 (K 91596)

(516 covers the sum of the workgroup's four waves and of the 512 partials.)  A wave that drops one chunk of 16
pixels out of 91080 stays inside the random bound: the exact inputs do the sharp work, the random ones guard the arithmetic on
general values.  RATIOS records the ratios per run and test_ratio_summary prints them (pytest -s).

Outputs live between guard floats (f64check.PAD) in NaN-filled regions, the wgrad workspace is NaN-filled, dx and dWp are asked
for together and each alone (bit-identical: the kernels are deterministic), and the documented refusals return GENRL_EINVAL and
write nothing.

The movers (genrl_im2col_s2 in its three modes, the u8 fast and generic kernels against each other; genrl_col2im_s2 on every
path and clamp of rp; genrl_transpose_last2 with accumulate; genrl_gather_windows on its 16-byte and byte paths with wrapping
windows) are pure data movement or exact small-integer sums: torch.equal against F.unfold / F.fold / an indexed copy."""
import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f64check import PAD, checker

gpu = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]


def on_gpu(fn):
    for m in gpu:
        fn = m(fn)
    return fn


EINVAL = 1
CI, KT, KC = 48, 6, 4                    # convT: input channels, kernel; conv1: kernel
G = 64                                   # guard floats in front of and behind every output region (keeps 16-byte alignment)
NAN = float('nan')

# K per checked quantity (module docstring); the wgrad entries are added per shape: pixels summed + 516
K = {'convt.fwd': 433, 'convt.dx': 112, 'conv1.fwd': 49}
RATIOS = {}
within = checker(K, RATIOS)

# ---------------------------------------------------------------------------------------------- the case table
# convT: (N, Hi, Wi, Co, nchw, backward too)
CONVT = {
    'loop3-scalar-tail': (400, 7, 33, 3, True, False),
    'loop3-vec-stores': (400, 7, 34, 3, True, False),
    'loop3-co4-nhwc': (400, 7, 34, 4, False, False),
    'loop-staged': (180, 7, 66, 3, True, True),
    'loop-unstaged': (180, 7, 67, 3, True, True),
    'single-staged': (4, 30, 30, 3, True, True),
    'single-unstaged': (3, 13, 9, 3, True, True),
    'single-nhwc': (5, 30, 30, 3, False, False),
}
CONVT_FWD_LOOP3 = ('loop3-scalar-tail', 'loop3-vec-stores', 'loop3-co4-nhwc')
CONVT_BWD = [c for c, v in CONVT.items() if v[5]]
CONVT_BWD_LOOP = ('loop-staged', 'loop-unstaged')
# conv1: (N, Hi, Wi)
CONV1 = {'loop': (460, 14, 68), 'single': (8, 64, 64)}
KINDS = ('exact', 'random')


def cdiv(a, b):
    return -(-a // b)


def capped_walk(nblk, bpr, rows, cap):
    """launch arithmetic of the three capped kernels: one block per wave and trip, 4 waves per workgroup"""
    grid = min(cdiv(nblk, 4), cap)
    step = 4 * grid
    return dict(nblk=nblk, bpr=bpr, rows=rows, grid=grid, step=step, trips=cdiv(nblk, step), sbx=step % bpr, srow=(step // bpr) % rows,
                simg=(step // bpr) // rows)


def convt_fwd_plan(N, Hi, Wi):
    Hq, Wq = Hi + 2, Wi + 2
    bpr = cdiv(Wq, 16)
    return dict(capped_walk(N * Hq * bpr, bpr, Hq, 1280), last_valid=Wq - 16 * (bpr - 1), Ho=2 * Hq, Wo=2 * Wq)


def convt_dgrad_plan(N, Hi, Wi):
    bpr = cdiv(Wi, 16)
    return dict(capped_walk(N * Hi * bpr, bpr, Hi, 768), last_valid=Wi - 16 * (bpr - 1))


def conv1_fwd_plan(N, Hi, Wi):
    Ho, Wo = (Hi - KC) // 2 + 1, (Wi - KC) // 2 + 1
    bpr = cdiv(Wo, 16)
    return dict(capped_walk(N * Ho * bpr, bpr, Ho, 1024), last_valid=Wo - 16 * (bpr - 1), Ho=Ho, Wo=Wo)


def share_plan(n, upr, rows, unit):
    """the wgrads: 512 workgroups of 4 waves, each wave a contiguous share of `per` units (upr units per image row)"""
    nw = 4 * 512
    per = cdiv(n, nw)
    busy = cdiv(n, per)
    starts = np.arange(busy) * per
    ends = np.minimum(starts + per, n) - 1
    return dict(n=n, upr=upr, per=per, busy_waves=busy, idle_waves=nw - busy, idle_wgs=512 - cdiv(busy, 4), last_valid=unit,
                cross_row=bool((starts // upr != ends // upr).any()), cross_img=bool((starts // (upr * rows) != ends // (upr * rows)).any()))


def convt_wgrad_plan(N, Hi, Wi):
    Wo = 2 * (Wi - 1) + KT
    staged = Wo % 4 == 0                     # (and 16-byte aligned x, dy: the tests' buffers are)
    unit = 16 if staged else 4
    upr = cdiv(Wi, unit)
    return dict(share_plan(N * Hi * upr, upr, Hi, Wi - unit * (upr - 1)), staged=staged, unit=unit)


def conv1_wgrad_plan(N, Hi, Wi):
    Ho, Wo = (Hi - KC) // 2 + 1, (Wi - KC) // 2 + 1
    bpr = cdiv(Wo, 16)
    return dict(share_plan(N * Ho * bpr, bpr, Ho, Wo - 16 * (bpr - 1)), unit=16)


def simulate_walk(p):
    """the kernels' incremental (bx, row, img) walk for every wave against the plain decode of blk -> carries fired (bx, row)"""
    blk = np.arange(p['step'], dtype=np.int64)
    bx, row, img = blk % p['bpr'], (blk // p['bpr']) % p['rows'], (blk // p['bpr']) // p['rows']
    fired = [0, 0]
    while True:
        live = blk < p['nblk']
        if not live.any():
            return fired
        assert (bx[live] == blk[live] % p['bpr']).all() and (row[live] == (blk[live] // p['bpr']) % p['rows']).all()
        assert (img[live] == (blk[live] // p['bpr']) // p['rows']).all()
        nxt = live & (blk + p['step'] < p['nblk'])             # (the walk matters only where a next block exists)
        bx, row, img = bx + p['sbx'], row + p['srow'], img + p['simg']
        c = bx >= p['bpr']; bx[c] -= p['bpr']; row[c] += 1; fired[0] += int((c & nxt).sum())
        c = row >= p['rows']; row[c] -= p['rows']; img[c] += 1; fired[1] += int((c & nxt).sum())
        assert (bx < p['bpr']).all() and (row < p['rows']).all()   # one subtraction per carry is enough
        blk = blk + p['step']


def test_case_table():
    """the launch arithmetic of the six kernels restated (caps 1280 / 768 / 1024 workgroups, 512 partials, bpr, gpr, nblk, per, the
    stride decomposition): every looped case makes >= 3 trips (per >= 3), fires both carries, ends its rows on a partly valid block
    and leaves workgroups idle in the wgrads; every single case makes one trip.  If a cap moves, move the shapes with it."""
    def looped(p):
        assert p['trips'] >= 3 and p['sbx'] != 0 and p['srow'] != 0, p
        assert 0 < p['last_valid'] < 16, p
        fired = simulate_walk(p)
        assert fired[0] > 0 and fired[1] > 0, (p, fired)

    def shared(p):
        assert p['per'] >= 3 and p['idle_wgs'] >= 1 and p['cross_row'] and p['cross_img'], p
        assert 0 < p['last_valid'] < p['unit'], p

    for c in CONVT_FWD_LOOP3:
        N, Hi, Wi, Co, nchw, _ = CONVT[c]
        p = convt_fwd_plan(N, Hi, Wi)
        looped(p)
        assert (p['nblk'], p['step'], p['bpr'], p['sbx'], p['srow']) == (10800, 5120, 3, 2, 5), p
    assert convt_fwd_plan(400, 7, 33)['Wo'] == 70 and convt_fwd_plan(400, 7, 34)['Wo'] % 4 == 0       # scalar tail / 16-byte stores
    assert CONVT['loop3-co4-nhwc'][3:5] == (4, False)
    for c in CONVT_BWD_LOOP:
        N, Hi, Wi = CONVT[c][:3]
        p = convt_fwd_plan(N, Hi, Wi)
        assert (p['nblk'], p['bpr'], p['trips']) == (8100, 5, 2) and 0 < p['last_valid'] < 16, p
        simulate_walk(p)
        p = convt_dgrad_plan(N, Hi, Wi)
        assert (p['nblk'], p['step'], p['bpr'], p['sbx'], p['srow']) == (6300, 3072, 5, 2, 5), p
        looped(p)
        assert p['last_valid'] == (3 if c == 'loop-unstaged' else 2)
        w = convt_wgrad_plan(N, Hi, Wi)
        shared(w)
    w = convt_wgrad_plan(*CONVT['loop-staged'][:3])
    assert w['staged'] and (w['n'], w['per'], w['idle_wgs']) == (6300, 4, 118), w
    w = convt_wgrad_plan(*CONVT['loop-unstaged'][:3])
    assert not w['staged'] and (w['upr'], w['n'], w['per']) == (17, 21420, 11) and w['per'] % 2 == 1 and w['idle_waves'] > 0, w
    p = conv1_fwd_plan(*CONV1['loop'])
    looped(p)
    assert (p['Ho'], p['Wo'], p['bpr'], p['last_valid'], p['nblk'], p['step'], p['sbx'], p['srow']) == (6, 33, 3, 1, 8280, 4096, 1, 3), p
    w = conv1_wgrad_plan(*CONV1['loop'])
    shared(w)
    assert (w['n'], w['per']) == (8280, 5), w
    # the single-trip cases: one block per wave, one unit per wave
    for c in ('single-staged', 'single-unstaged', 'single-nhwc'):
        N, Hi, Wi = CONVT[c][:3]
        assert convt_fwd_plan(N, Hi, Wi)['trips'] == 1
        if CONVT[c][5]:
            assert convt_dgrad_plan(N, Hi, Wi)['trips'] == 1 and convt_wgrad_plan(N, Hi, Wi)['per'] == 1
    assert convt_wgrad_plan(*CONVT['single-staged'][:3])['staged'] and not convt_wgrad_plan(*CONVT['single-unstaged'][:3])['staged']
    assert conv1_fwd_plan(*CONV1['single'])['trips'] == 1 and conv1_wgrad_plan(*CONV1['single'])['per'] == 1
    # the kernels' int block counters and the exactness argument: every exact-input sum stays far below 2^24
    for N, Hi, Wi, Co, _, _ in CONVT.values():
        assert N * Hi * Wi * 9 < 2 ** 24
    for N, Hi, Wi in CONV1.values():
        assert N * (Hi // 2) * (Wi // 2) * 3 < 2 ** 24


# ---------------------------------------------------------------------------------------------- helpers of the GPU tests
def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    return lib()


def guarded(n, fill=NAN):
    """-> (buf, out): a region of n floats holding `fill` between G guard floats of PAD on either side"""
    buf = torch.full((n + 2 * G,), PAD, device='cuda')
    out = buf[G:G + n]
    out.fill_(fill)
    return buf, out


def guards_ok(what, buf):
    n = buf.numel() - 2 * G
    assert bool((buf[:G] == PAD).all()) and bool((buf[G + n:] == PAD).all()), f'{what}: a kernel wrote outside its output'


def all_nan(t):
    return bool(torch.isnan(t).all())


def draw(kind, shape, seed):
    if kind == 'exact':
        return torch.randint(-3, 4, shape, generator=gen(seed)).float()
    return torch.randn(shape, generator=gen(seed))


def settle(what, kind, got, ref, scale, key):
    """exact inputs: bit for bit the float64 result; random inputs: within K 2^-24 S per element"""
    assert bool(torch.isfinite(got).all()), f'{what}: output not finite (a part left unwritten?)'
    if kind == 'exact':
        r32 = ref.float()
        assert torch.equal(r32.double(), ref), f'{what}: the exact reference is not an fp32 value'
        g = got.detach().cpu()
        if not torch.equal(g, r32):
            bad = (g != r32).nonzero()
            raise AssertionError(f'{what}: {bad.shape[0]} of {g.numel()} elements differ from the exact result, first at '
                                 f'{tuple(int(v) for v in bad[0])}: got {float(g[tuple(bad[0])])!r}, exact {float(r32[tuple(bad[0])])!r}')
    else:
        within(what, got, ref, scale, key=key)


# ---------------------------------------------------------------------------------------------- transposed convolution
@functools.lru_cache(None)
def convt_data(case, kind):
    """inputs (fp32, CPU) and float64 references of a convT case: forward and its |term| sums; with backward, dx / dWp and theirs"""
    N, Hi, Wi, Co, nchw, bwd = CONVT[case]
    seed = 100 * list(CONVT).index(case) + 7 * KINDS.index(kind)
    x = draw(kind, (N, Hi, Wi, CI), seed + 1)
    W = draw(kind, (CI, Co, KT, KT), seed + 2)
    b = draw(kind, (Co,), seed + 3)
    d = dict(x=x, Wp=W.permute(0, 2, 3, 1).contiguous(), b=b)             # Wp: (ci, kh, kw, co)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(bwd)
    W64 = W.double().requires_grad_(bwd)
    y = F.conv_transpose2d(x64, W64, b.double(), stride=2)
    lay = (lambda t: t) if nchw else (lambda t: t.permute(0, 2, 3, 1))
    d['y'] = lay(y.detach()).contiguous()
    if kind == 'random' or bwd:
        xa, Wa = x64.detach().abs().requires_grad_(bwd), W64.detach().abs().requires_grad_(bwd)
        ya = F.conv_transpose2d(xa, Wa, b.double().abs(), stride=2)
        d['y_scale'] = lay(ya.detach()).contiguous()
    if bwd:
        dy = draw(kind, tuple(y.shape), seed + 4)
        d['dy'] = dy
        y.backward(dy.double())
        ya.backward(dy.double().abs())
        to_wp = lambda t: t.permute(0, 2, 3, 1).reshape(CI, KT * KT * Co).contiguous()
        d['dx'], d['dx_scale'] = x64.grad.permute(0, 2, 3, 1).contiguous(), xa.grad.permute(0, 2, 3, 1).contiguous()
        d['dWp'], d['dWp_scale'] = to_wp(W64.grad), to_wp(Wa.grad)
    return d


def convt_fwd(L, xd, Wpd, bd, case, Ci=CI, k=KT, Co=None):
    N, Hi, Wi, Co0, nchw, _ = CONVT[case]
    Ho, Wo = 2 * (Hi - 1) + KT, 2 * (Wi - 1) + KT
    buf, o = guarded(N * Co0 * Ho * Wo)
    rc = L.genrl_convt_small_co_fwd(xd.data_ptr(), Wpd.data_ptr(), bd.data_ptr(), o.data_ptr(), N, Hi, Wi, Ci, Co or Co0, k, int(nchw), stream())
    torch.cuda.synchronize()
    shape = (N, Co0, Ho, Wo) if nchw else (N, Ho, Wo, Co0)
    return rc, buf, o.view(shape)


@on_gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', list(CONVT))
def test_convt_forward(L, case, kind):
    """genrl_convt_small_co_fwd at every case of the table: the trips of the block loop on alternating register sets, both carries,
    the scalar / 16-byte / NHWC epilogues"""
    d = convt_data(case, kind)
    xd, Wpd, bd = d['x'].cuda(), d['Wp'].cuda(), d['b'].cuda()
    rc, buf, y = convt_fwd(L, xd, Wpd, bd, case)
    assert rc == 0
    guards_ok(case, buf)
    settle(f'convt.fwd[{case}]', kind, y, d['y'], d.get('y_scale'), 'convt.fwd')
    rc, _, y2 = convt_fwd(L, xd, Wpd, bd, case)
    assert rc == 0 and torch.equal(y2, y), 'two runs differ'


def convt_bwd(L, xd, Wpd, dyd, case, want_dx=True, want_dw=True, ws=True, Ci=CI, k=KT, Co=None):
    N, Hi, Wi, Co0 = CONVT[case][:4]
    bx, dx = guarded(N * Hi * Wi * CI)
    bw, dw = guarded(CI * KT * KT * Co0)
    wsd = torch.full((L.genrl_convt_small_co_bwd_ws_floats(CI, Co0),), NAN, device='cuda') if ws else None
    rc = L.genrl_convt_small_co_bwd(xd.data_ptr(), Wpd.data_ptr(), dyd.data_ptr(), dx.data_ptr() if want_dx else None,
                                    dw.data_ptr() if want_dw else None, wsd.data_ptr() if ws else None, N, Hi, Wi, Ci, Co or Co0, k, stream())
    torch.cuda.synchronize()
    guards_ok(case + ' dx', bx); guards_ok(case + ' dWp', bw)
    return rc, dx.view(N, Hi, Wi, CI), dw.view(CI, KT * KT * Co0)


@on_gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CONVT_BWD)
def test_convt_backward(L, case, kind):
    """genrl_convt_small_co_bwd: dgrad's block loop with its prefetch hand-over; the staged (Wo % 4 == 0) and unstaged wgrads with shares
    of several chunks / groups, idle workgroups over a NaN-filled workspace; dx and dWp together and each alone, bit-identical"""
    N, Hi, Wi, Co = CONVT[case][:4]
    d = convt_data(case, kind)
    xd, Wpd, dyd = d['x'].cuda(), d['Wp'].cuda(), d['dy'].cuda()
    rc, dx, dw = convt_bwd(L, xd, Wpd, dyd, case)
    assert rc == 0
    wkey = f'convt.dW.{"staged" if convt_wgrad_plan(N, Hi, Wi)["staged"] else "unstaged"}@{N * Hi * Wi}px'
    K[wkey] = N * Hi * Wi + 516
    settle(f'convt.dx[{case}]', kind, dx, d['dx'], d['dx_scale'], 'convt.dx')
    settle(f'convt.dWp[{case}]', kind, dw, d['dWp'], d['dWp_scale'], wkey)
    rc, dx1, dw1 = convt_bwd(L, xd, Wpd, dyd, case, want_dw=False, ws=False)
    assert rc == 0 and torch.equal(dx1, dx) and all_nan(dw1), 'dx alone'
    rc, dx2, dw2 = convt_bwd(L, xd, Wpd, dyd, case, want_dx=False)
    assert rc == 0 and torch.equal(dw2, dw) and all_nan(dx2), 'dWp alone'


@on_gpu
def test_convt_refusals(L):
    """Ci != 48, k != 6 (forward and backward), Co = 4 (backward), dWp without ws: GENRL_EINVAL and nothing written"""
    case = 'single-staged'
    d = convt_data(case, 'exact')
    xd, Wpd, bd, dyd = d['x'].cuda(), d['Wp'].cuda(), d['b'].cuda(), d['dy'].cuda()
    for kw in (dict(Ci=32), dict(k=4), dict(k=5), dict(Co=5)):
        rc, buf, y = convt_fwd(L, xd, Wpd, bd, case, **kw)
        assert rc == EINVAL and all_nan(y), kw
        guards_ok(str(kw), buf)
    for kw in (dict(Ci=32), dict(k=4), dict(Co=4), dict(ws=False), dict(ws=False, want_dx=False)):
        rc, dx, dw = convt_bwd(L, xd, Wpd, dyd, case, **kw)
        assert rc == EINVAL and all_nan(dx) and all_nan(dw), kw


# ---------------------------------------------------------------------------------------------- first encoder layer from u8 frames
# the kernels' pixel arithmetic (float)p / 255.0f - 0.5f in IEEE fp32 (numpy: correctly rounded division, no reciprocal)
LUT = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255) - np.float32(0.5))


def preprocess32(u8):
    return LUT[u8.long()]


@functools.lru_cache(None)
def conv1_data(case, kind):
    N, Hi, Wi = CONV1[case]
    seed = 5000 + 100 * list(CONV1).index(case) + 7 * KINDS.index(kind)
    Ho, Wo = (Hi - KC) // 2 + 1, (Wi - KC) // 2 + 1
    if kind == 'exact':
        u8 = (torch.randint(0, 2, (N, 3, Hi, Wi), generator=gen(seed)) * 255).to(torch.uint8)
        xin = u8.double() / 255 - 0.5
    else:
        u8 = torch.randint(0, 256, (N, 3, Hi, Wi), generator=gen(seed), dtype=torch.uint8)
        xin = preprocess32(u8).double()
    W = draw(kind, (48, 3, KC, KC), seed + 1)
    b = draw(kind, (48,), seed + 2)
    dy = draw(kind, (N, Ho, Wo, 48), seed + 3)
    W64 = W.double().requires_grad_()
    y = F.conv2d(xin, W64, b.double(), stride=2)
    y.backward(dy.double().permute(0, 3, 1, 2))
    Wa = W.double().abs().requires_grad_()
    ya = F.conv2d(xin.abs(), Wa, b.double().abs(), stride=2)
    ya.backward(dy.double().abs().permute(0, 3, 1, 2))
    to_wp = lambda t: t.detach().permute(0, 2, 3, 1).reshape(48, 48).contiguous()             # (co, kh, kw, c)
    return dict(u8=u8, Wp=to_wp(W).contiguous(), b=b, dy=dy, y=y.detach().permute(0, 2, 3, 1).contiguous(),
                y_scale=ya.detach().permute(0, 2, 3, 1).contiguous(), dWp=to_wp(W64.grad), dWp_scale=to_wp(Wa.grad))


def conv1_fwd(L, ud, Wpd, bd, shape, Wi=None, Co=48, k=KC):
    N, Hi, Wi0 = shape
    Ho, Wo = (Hi - KC) // 2 + 1, (Wi0 - KC) // 2 + 1
    buf, y = guarded(N * Ho * Wo * 48)
    rc = L.genrl_conv1_u8_fwd(ud.data_ptr(), Wpd.data_ptr(), bd.data_ptr(), y.data_ptr(), N, Hi, Wi or Wi0, Co, k, stream())
    torch.cuda.synchronize()
    guards_ok('conv1 y', buf)
    return rc, y.view(N, Ho, Wo, 48)


def conv1_wgrad(L, ud, dyd, shape, Wi=None, Co=48, k=KC, ws=True):
    N, Hi, Wi0 = shape
    buf, dw = guarded(48 * 48)
    wsd = torch.full((L.genrl_conv1_u8_wgrad_ws_floats(48),), NAN, device='cuda') if ws else None
    rc = L.genrl_conv1_u8_wgrad(ud.data_ptr(), dyd.data_ptr(), dw.data_ptr(), wsd.data_ptr() if ws else None, N, Hi, Wi or Wi0, Co, k, stream())
    torch.cuda.synchronize()
    guards_ok('conv1 dWp', buf)
    return rc, dw.view(48, 48)


@on_gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', list(CONV1))
def test_conv1_forward(L, case, kind):
    """genrl_conv1_u8_fwd: three trips of the block loop with both carries and a 1-pixel last block per row, against one trip"""
    d = conv1_data(case, kind)
    ud, Wpd, bd = d['u8'].cuda(), d['Wp'].cuda(), d['b'].cuda()
    rc, y = conv1_fwd(L, ud, Wpd, bd, CONV1[case])
    assert rc == 0
    settle(f'conv1.fwd[{case}]', kind, y, d['y'], d['y_scale'], 'conv1.fwd')
    rc, y2 = conv1_fwd(L, ud, Wpd, bd, CONV1[case])
    assert rc == 0 and torch.equal(y2, y), 'two runs differ'


@on_gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', list(CONV1))
def test_conv1_wgrad(L, case, kind):
    """genrl_conv1_u8_wgrad: shares of five chunks across rows and images, idle workgroups over a NaN-filled workspace"""
    N, Hi, Wi = CONV1[case]
    d = conv1_data(case, kind)
    ud, dyd = d['u8'].cuda(), d['dy'].cuda()
    rc, dw = conv1_wgrad(L, ud, dyd, CONV1[case])
    assert rc == 0
    p = conv1_fwd_plan(N, Hi, Wi)
    wkey = f'conv1.dW@{N * p["Ho"] * p["Wo"]}px'
    K[wkey] = N * p['Ho'] * p['Wo'] + 516
    settle(f'conv1.dWp[{case}]', kind, dw, d['dWp'], d['dWp_scale'], wkey)
    rc, dw2 = conv1_wgrad(L, ud, dyd, CONV1[case])
    assert rc == 0 and torch.equal(dw2, dw), 'two runs differ'


@on_gpu
def test_conv1_refusals(L):
    """odd Wi, Co != 48, dWp without ws: GENRL_EINVAL and nothing written"""
    d = conv1_data('single', 'exact')
    ud, Wpd, bd, dyd = d['u8'].cuda(), d['Wp'].cuda(), d['b'].cuda(), d['dy'].cuda()
    for kw in (dict(Wi=63), dict(Co=32), dict(Co=64)):
        rc, y = conv1_fwd(L, ud, Wpd, bd, CONV1['single'], **kw)
        assert rc == EINVAL and all_nan(y), kw
    for kw in (dict(Wi=63), dict(Co=32), dict(ws=False)):
        rc, dw = conv1_wgrad(L, ud, dyd, CONV1['single'], **kw)
        assert rc == EINVAL and all_nan(dw), kw


# ---------------------------------------------------------------------------------------------- the movers, bit for bit
def im2col_ref(x_nchw, k):
    """cols[(n, a, b), (kh, kw, c)] = x[n, c, 2 a + kh, 2 b + kw]"""
    N, C, Hi, Wi = x_nchw.shape
    Ho, Wo = (Hi - k) // 2 + 1, (Wi - k) // 2 + 1
    cols = F.unfold(x_nchw, k, stride=2).view(N, C, k, k, Ho, Wo)
    return cols.permute(0, 4, 5, 2, 3, 1).reshape(N * Ho * Wo, k * k * C).contiguous()


def im2col(L, ind, shape, k, mode, ptr=None):
    N, C, Hi, Wi = shape
    M = N * ((Hi - k) // 2 + 1) * ((Wi - k) // 2 + 1)
    buf, cols = guarded(M * k * k * C)
    rc = L.genrl_im2col_s2(ptr or ind.data_ptr(), cols.data_ptr(), N, Hi, Wi, C, k, mode, stream())
    torch.cuda.synchronize()
    guards_ok(f'im2col {shape} k {k} mode {mode}', buf)
    return rc, cols.view(M, k * k * C)


@on_gpu
@pytest.mark.parametrize('N,Hi,Wi,C,k,modes', [(3, 9, 11, 8, 4, (0, 1)), (2, 13, 10, 96, 4, (0, 1)), (2, 9, 8, 5, 5, (0, 1)), (1, 6, 6, 4, 6, (0, 1)),
                                               (2, 5, 5, 7, 1, (0, 1)), (2, 18, 22, 3, 6, (1,))])
def test_im2col_fp32(L, N, Hi, Wi, C, k, modes):
    """genrl_im2col_s2 modes 0 (NHWC) and 1 (NCHW, reached by no other test) on the same values: 36 patch rows = a ragged second
    workgroup; K = 1536: the offset-table fill and the 64-lane copy loops repeat; k = 5, 6, 1; the decoder's own 3-channel use"""
    x = torch.randn(N, C, Hi, Wi, generator=gen(N * Hi + C))
    ref = im2col_ref(x, k)
    for mode in modes:
        src = (x.permute(0, 2, 3, 1) if mode == 0 else x).contiguous().cuda()
        rc, cols = im2col(L, src, (N, C, Hi, Wi), k, mode)
        assert rc == 0 and torch.equal(cols.cpu(), ref), mode


@on_gpu
def test_im2col_u8(L):
    """mode 2: the C3 / k4 fast kernel, the generic kernel (odd width, C = 4; reached by no other test), and the two against each other
    on an even-width case (the generic one through a frame pointer one byte into a larger buffer: it fails the fast path's alignment
    test and is valid for byte loads)"""
    for N, C, Hi, Wi in [(3, 3, 10, 12), (2, 3, 64, 64), (3, 3, 11, 13), (2, 4, 10, 12)]:
        u8 = torch.randint(0, 256, (N, C, Hi, Wi), generator=gen(Hi * Wi + C), dtype=torch.uint8)
        ref = im2col_ref(preprocess32(u8), 4)
        rc, cols = im2col(L, u8.cuda(), (N, C, Hi, Wi), 4, 2)
        assert rc == 0 and torch.equal(cols.cpu(), ref), (N, C, Hi, Wi)
    shape = (3, 3, 10, 12)
    u8 = torch.randint(0, 256, shape, generator=gen(77), dtype=torch.uint8)
    big = torch.zeros(u8.numel() + 64, dtype=torch.uint8, device='cuda')
    big[1:1 + u8.numel()] = u8.reshape(-1).cuda()
    assert big.data_ptr() % 2 == 0
    rc0, fast = im2col(L, u8.cuda(), shape, 4, 2)
    rc1, generic = im2col(L, big, shape, 4, 2, ptr=big.data_ptr() + 1)
    assert rc0 == 0 and rc1 == 0 and torch.equal(fast, generic) and torch.equal(fast.cpu(), im2col_ref(preprocess32(u8), 4))


@on_gpu
def test_im2col_refuses_k7(L):
    x = torch.randn(1, 4, 9, 9, generator=gen(1)).cuda()
    for mode in (0, 1):
        rc, cols = im2col(L, x, (1, 4, 9, 9), 7, mode)
        assert rc == EINVAL and all_nan(cols)


@on_gpu
@pytest.mark.parametrize('N,Ha,Wa,C,k,nchw,bias,over', [
    (2, 13, 9, 3, 6, True, True, False),        # rp = 342, 1320 pixels: a ragged last workgroup
    (2, 13, 9, 1, 6, True, True, False),        # rp clamped to 512
    (2, 13, 9, 1, 6, False, True, False),
    (2, 5, 4, 192, 6, False, True, False),      # 16-byte lanes, rp clamped to 32
    (3, 6, 5, 48, 6, False, True, False),
    (3, 6, 5, 48, 6, False, False, False),
    (2, 7, 5, 6, 6, False, True, False),        # C % 4 != 0: the scalar path
    (2, 6, 7, 8, 5, False, True, False),
    (2, 6, 7, 3, 5, True, True, False),
    (2, 14, 14, 8, 4, False, False, True),      # the gradient of a 31-wide input: last row / column = exact zeros, written
    (2, 14, 14, 3, 4, True, False, True),
])
def test_col2im(L, N, Ha, Wa, C, k, nchw, bias, over):
    """genrl_col2im_s2 on integer cols (sums of <= 9 terms + bias are exact in any order) against F.fold in float64"""
    cols = torch.randint(-3, 4, (N * Ha * Wa, k * k * C), generator=gen(Ha * Wa + C + k)).float()
    b = torch.randint(-3, 4, (C,), generator=gen(C)).float()
    Ho, Wo = 2 * (Ha - 1) + k + int(over), 2 * (Wa - 1) + k + int(over)
    ref = F.fold(cols.double().view(N, Ha * Wa, k, k, C).permute(0, 4, 2, 3, 1).reshape(N, C * k * k, Ha * Wa), (Ho, Wo), k, stride=2)
    if bias:
        ref = ref + b.double().view(1, C, 1, 1)
    if over:
        assert bool((ref[:, :, -1, :] == 0).all()) and bool((ref[:, :, :, -1] == 0).all())
    if not nchw:
        ref = ref.permute(0, 2, 3, 1)
    cd, bd = cols.cuda(), b.cuda()
    buf, out = guarded(N * Ho * Wo * C)
    rc = L.genrl_col2im_s2(cd.data_ptr(), bd.data_ptr() if bias else None, out.data_ptr(), N, Ha, Wa, C, k, Ho if over else 0, Wo if over else 0,
                           int(nchw), stream())
    torch.cuda.synchronize()
    guards_ok('col2im', buf)
    assert rc == 0 and torch.equal(out.cpu().view(ref.shape), ref.float().contiguous())


@on_gpu
def test_col2im_refuses_k7(L):
    cols = torch.zeros(4 * 4, 49 * 4, device='cuda')
    buf, out = guarded(19 * 19 * 4)
    assert L.genrl_col2im_s2(cols.data_ptr(), None, out.data_ptr(), 1, 4, 4, 4, 7, 0, 0, 0, stream()) == EINVAL
    torch.cuda.synchronize()
    assert all_nan(out)
    guards_ok('col2im k 7', buf)


@on_gpu
@pytest.mark.parametrize('acc', [0, 1])
def test_transpose_last2(L, acc):
    """out[b, c, p] (+)= in[b, p, c]; B P C = 1221: several workgroups, a partial last one"""
    B, P, C = 3, 37, 11
    x = torch.randint(-9, 10, (B, P, C), generator=gen(1)).float()
    prior = torch.randint(-9, 10, (B, C, P), generator=gen(2)).float()
    buf, out = guarded(B * P * C)
    if acc:
        out.copy_(prior.reshape(-1))
    xd = x.cuda()
    assert L.genrl_transpose_last2(xd.data_ptr(), out.data_ptr(), B, P, C, acc, stream()) == 0
    torch.cuda.synchronize()
    guards_ok('transpose', buf)
    ref = x.transpose(1, 2) + (prior if acc else 0)
    assert torch.equal(out.cpu().view(B, C, P), ref.contiguous())


@on_gpu
@pytest.mark.parametrize('row_bytes,dst_off', [(12288, 0), (4, 0), (36, 0), (64, 1)])
def test_gather_windows(L, row_bytes, dst_off):
    """genrl_gather_windows on a ring of 7 rows, windows of 5 from rows 0, 4 and 6 (two wrap): three trips of the 16-byte loop; rows
    that are no multiple of 16 bytes and a destination one byte into its buffer take the byte path"""
    ring, T, starts = 7, 5, [0, 4, 6]
    src = torch.randint(0, 256, (ring, row_bytes), generator=gen(row_bytes), dtype=torch.uint8)
    n = len(starts) * T * row_bytes
    guard = 32
    buf = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device='cuda')
    lo = 16 + dst_off
    buf[lo:lo + n] = 0x5A
    sd, st = src.cuda(), torch.tensor(starts, dtype=torch.int64, device='cuda')
    assert (buf.data_ptr() + lo) % 16 == dst_off
    assert L.genrl_gather_windows(sd.data_ptr(), row_bytes, ring, st.data_ptr(), len(starts), T, buf.data_ptr() + lo, stream()) == 0
    torch.cuda.synchronize()
    idx = (torch.tensor(starts)[:, None] + torch.arange(T)[None, :]) % ring
    got = buf.cpu()
    assert torch.equal(got[lo:lo + n].view(len(starts), T, row_bytes), src[idx])
    assert bool((got[:lo] == 0xA5).all()) and bool((got[lo + n:] == 0xA5).all()), 'wrote outside the destination'


@on_gpu
def test_ratio_summary():
    """prints the largest |kernel - float64| / (2^-24 S) per kernel next to its K (run with -s); the last test of the module"""
    print('\ndirect conv kernels, worst ratio (K):', json.dumps({k: f'{v:.3g} ({K[k]})' for k, v in sorted(RATIOS.items())}))
    for k, v in RATIOS.items():
        assert v <= K[k]
