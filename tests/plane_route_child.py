"""Route table and child-process runner of test_gpu_plane_variants.py (not a test module).

`python plane_route_child.py GROUP OUT.json` runs the cases of one group in a fresh process whose environment the parent set
(GENRL_GEMM_LOG and, per group, GENRL_PLANES_HL / GENRL_HL_WIDE / GENRL_PLANES_2PER: gemm_planes.hip reads each of them once per
process).  Per call it records the largest (|kernel - float64| - floor) / (2^-24 scale), whether
anything outside the output changed, the launch-log families, genrl_planes_last_route and the return code; the parent asserts.

Operands (`h2_exact`) are exactly representable in h2: a = (h + l 2^-11) / s with fp16 h (row maximum in [2^14, 2^15)) and fp16 l
below half an ulp of h at 2^11, so that genrl_split_h2 recovers h and l.  Signs: h of A follows alpha[m] gamma[k], l of A
alpha'[m] delta[k], h of B beta[n] delta[k], l of B beta'[n] gamma[k]: every h*l and every l*h product of one output element
has one sign (a dropped or mis-paired cross term adds up over K to ~2^-13 of the scale), while the h*h and l*l products carry
gamma[k] delta[k], random over k.  `plain` operands are random fp32 with row magnitudes over 2^+-20, zero rows and rows with
one element 2^12 above the rest."""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from f64check import PAD, U, out_buf, untouched_ok as outside_ok  # noqa: E402

EINVAL = 1
SWITCHES = ('GENRL_GEMM_LOG', 'GENRL_PLANES_HL', 'GENRL_HL_WIDE', 'GENRL_PLANES_2PER')
ROUTE_BITS = {'64/ns3': 0x1, '64/ns2': 0x2, '64/sample': 0x4, '64/ln': 0x8, '128/plain': 0x10, '128/hl': 0x20, '128/hlw': 0x40,
              'conv/plain': 0x80, 'conv/hl': 0x100, 'conv/hlw': 0x200, 'conv/tall96': 0x400, 'subpixel/hl': 0x800,
              'subpixel/hlw': 0x1000, 'x3/64': 0x2000, 'x3/128': 0x4000, 'tn': 0x8000, 'tn/conv': 0x10000}
IMG_INV = 2.0 ** -14      # inverse scale of the uniform-scale images
FLOOR_H2 = 2.0 ** -36        # absolute representation loss of a scaled element (the l plane's fp16 subnormal half ulp x 2^-11)


def route_names(word):
    bits = word & 0xFFFFFFFF
    return sorted(k for k, b in ROUTE_BITS.items() if bits & b), word >> 32


# ----------------------------------------------------------------------------------------------------------- the route table
def g(cid, M, N, K, route, K1=0, fam=None, bias=True, acc=True, pad=(0, 0, 0), r0=(0, 0, 0), c_off=0, force=0, kind='exact',
      zero=None, seg_exp=0):
    """one genrl_gemm_h2 product: K (K1) true lengths of segment 0 (1), k rounded up to 64; pad: extra plane columns of A, B (
    multiples of 64) and extra C columns; r0: a_row0 / a1_row0 / b_row0 (rows skipped in front of the operands); zero: rows made 0
    ('a1' / 'a0' / 'b1': rows 0, 5, M-1 / columns 3, N-1); seg_exp: segment 1's row magnitudes 2^seg_exp of segment 0's"""
    return dict(id=cid, op='h2', M=M, N=N, K=K, K1=K1, route=route, fam=fam, bias=bias, acc=acc, pad=pad, r0=r0, c_off=c_off,
                force=force, kind=kind, zero=zero, seg_exp=seg_exp)


BIG = ['h2/128']
ROUTES = {
    'h2': [
        g('64.ns3.small.ragged', 100, 70, 100, ['64/ns3'], fam=['h2/64'], pad=(64, 0, 3), c_off=1),
        g('64.ns3.two-seg.offsets', 300, 200, 128, ['64/ns3'], K1=96, fam=['h2/64'], r0=(3, 5, 7), pad=(0, 64, 2)),
        g('64.ns3.no-bias.no-acc', 257, 129, 200, ['64/ns3'], fam=['h2/64'], bias=False, acc=False),
        g('64.ns3.plain-operands', 520, 300, 700, ['64/ns3'], K1=300, fam=['h2/64'], kind='plain'),
        g('64.ns3.ntile256', 1024, 1024, 512, ['64/ns3'], fam=['h2/64']),
        g('64.ns2.ntile257', 16448, 64, 256, ['64/ns2'], fam=['h2/64']),
        g('64.ns2.K1536', 1280, 1280, 1024, ['64/ns2'], K1=512, fam=['h2/64']),
        g('64.ns3.K1600', 1280, 1280, 1024, ['64/ns3'], K1=576, fam=['h2/64']),
        g('64.t64-2047', 131008, 64, 64, ['64/ns2'], fam=['h2/64'], bias=False),
        g('128.t64-2048', 131072, 64, 64, ['128/hl'], fam=BIG, bias=False),
        g('128.two-seg', 8192, 1024, 256, ['128/hl'], K1=128, fam=BIG * 2, r0=(2, 0, 1), pad=(64, 64, 4)),
        g('128.rowsplit.17408x1024', 17408, 1024, 1024, ['128/hl', '64/ns3'], fam=['h2/128', 'h2/64'], acc=False),
        g('128.no-split.M%128', 17400, 1024, 1024, ['128/hl'], fam=BIG, acc=False),
        g('128.no-split.r>128', 34944, 1024, 128, ['128/hl'], fam=BIG, acc=False),
        g('128.no-split.r%tn', 7680, 1152, 256, ['128/hl'], fam=BIG, acc=False),
        g('128.force2.N192', 1000, 192, 256, ['128/hlw'], fam=BIG, force=2),
        g('128.force2.N200', 1000, 200, 256, ['128/hl'], fam=BIG, force=2),
        g('128.force2.N320', 1000, 320, 192, ['128/hl'], fam=BIG, force=2, c_off=2),
        g('128.force2.N576', 700, 576, 128, ['128/hlw'], fam=BIG, force=2, pad=(0, 0, 4)),
        g('128.force2.N190.ragged', 777, 190, 300, ['128/hlw'], K1=64, fam=BIG * 2, force=2),
        g('128.force1.big', 65536, 128, 64, ['64/ns2'], fam=['h2/64'], force=1, bias=False),
    ],
    'seg': [
        g('seg.64.a1-2^40', 300, 200, 256, ['64/ns3'], K1=128, fam=['h2/64'], seg_exp=40),
        g('seg.64.a1-2^-40', 300, 200, 256, ['64/ns3'], K1=128, fam=['h2/64'], seg_exp=-40),
        g('seg.64.zero-a1-rows', 300, 200, 256, ['64/ns3'], K1=128, fam=['h2/64'], zero='a1'),
        g('seg.64.zero-a0-rows', 300, 200, 256, ['64/ns3'], K1=128, fam=['h2/64'], zero='a0'),
        g('seg.64.zero-b1-rows', 300, 200, 256, ['64/ns3'], K1=128, fam=['h2/64'], zero='b1'),
        g('seg.64.zero-a1-b1', 1280, 1280, 512, ['64/ns2'], K1=512, fam=['h2/64'], zero='a1b1'),
        g('seg.128.zero-a1-rows', 8192, 1024, 256, ['128/hl'], K1=128, fam=BIG * 2, zero='a1'),
    ],
}
for _m in ('hl0', 'wide0', 'wide2'):
    ROUTES[_m] = [
        g(f'{_m}.128.N1024', 8192, 1024, 256, ['128/plain' if _m == 'hl0' else '128/hl'], K1=64, fam=BIG * 2),
        g(f'{_m}.128.N192', 1000, 192, 256, [{'hl0': '128/plain', 'wide0': '128/hl', 'wide2': '128/hlw'}[_m]], fam=BIG, force=2),
        g(f'{_m}.128.N384', 1000, 384, 256, [{'hl0': '128/plain', 'wide0': '128/hl', 'wide2': '128/hlw'}[_m]], fam=BIG, force=2,
          pad=(0, 0, 1)),
        g(f'{_m}.128.N190.ragged', 777, 190, 300, [{'hl0': '128/plain', 'wide0': '128/hl', 'wide2': '128/hlw'}[_m]], fam=BIG,
          force=2),
    ]
ROUTES['2per0'] = [g('2per0.ntile400', 1280, 1280, 512, ['64/ns3'], fam=['h2/64'], K1=64)]
ROUTES['2per1'] = [g('2per1.ntile20', 300, 200, 512, ['64/ns2'], fam=['h2/64'], K1=64),
                   g('2per1.ntile256.K2048', 1024, 1024, 2048, ['64/ns2'], fam=['h2/64'])]
GROUP_ENV = {'hl0': {'GENRL_PLANES_HL': '0'}, 'wide0': {'GENRL_HL_WIDE': '0'}, 'wide2': {'GENRL_HL_WIDE': '2'},
             '2per0': {'GENRL_PLANES_2PER': '0'}, '2per1': {'GENRL_PLANES_2PER': '1'}}

# stride-2 convolutions: (id, Nimg, H, W, Cc, k, N, ld_img extra, route [, env group])
CONV = [
    ('conv.tall96.K1024', 2, 21, 21, 64, 4, 96, 0, 'conv/tall96'),
    ('conv.hl.K896.N96', 2, 21, 21, 56, 4, 96, 8, 'conv/hl'),
    ('conv.hl.N104', 2, 21, 21, 64, 4, 104, 0, 'conv/hl'),
    ('conv.tall96.N48.odd', 3, 19, 23, 72, 4, 48, 0, 'conv/tall96'),
    ('conv.hlw.N192.K%64', 2, 17, 18, 48, 3, 192, 16, 'conv/hlw'),
    ('conv.hl.N256', 1, 34, 34, 48, 4, 256, 0, 'conv/hl'),
]
# sub-pixel: (id, Nimg, Hi, Wi, Cc, T, Co, Ho, Wo, bias, zero tap)
SUBPIXEL = [
    ('subpixel.hlw.Co48', 2, 8, 9, 64, 2, 48, 16, 18, True, False),
    ('subpixel.hl.Co96.nobias', 1, 7, 10, 48, 2, 96, 14, 19, False, False),
    ('subpixel.hlw.k5-as-6', 2, 6, 6, 48, 3, 48, 15, 15, True, True),
    ('subpixel.hl.Ho>2Hq', 1, 5, 6, 48, 2, 96, 14, 13, True, False),
]
# TN: (id, NI, NJ, M, acc, ldc extra, a_row0, b_row0)
TN = [
    ('tn.one-split.M64', 100, 70, 64, False, 3, 0, 0),
    ('tn.one-split', 256, 256, 512, True, 0, 64, 0),
    ('tn.splits.short-last', 130, 200, 64 * 107, True, 4, 0, 64),
    ('tn.splits.ragged', 96, 1000, 64 * 300, False, 0, 0, 0),
    ('tn.one-split.NJ%4', 200, 99, 256, True, 1, 0, 0),
]
TN_CONV = [('tnconv.small', 48, 2, 18, 18, 48, 4), ('tnconv.larger', 96, 4, 34, 30, 48, 4)]
GROUPS = list(ROUTES) + ['x3', 'sample', 'ln', 'conv', 'conv_hl0', 'tn', 'split', 'refuse']


def tn_plan(NI, NJ, M):
    """(nsplit, stages per split) as gemm_planes_tn.hip's tn_plan"""
    tiles, stages = -(-NI // 128) * -(-NJ // 128), M // 64
    smax = min(max(stages // 8, 1), 64)
    best, bc = 1, -1
    for s in range(1, smax + 1):
        cost = -(-(tiles * s) // 256) * (-(-stages // s) + 8)
        if bc < 0 or cost < bc:
            bc, best = cost, s
    sps = -(-stages // best)
    return -(-stages // sps), sps


# ----------------------------------------------------------------------------------------------------------- operands
def _sg(gen, n):
    return torch.where(torch.rand(n, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)


def h2_exact(rows, K, gen, sh, sl, rexp=10, rowexp=None):
    """fp32 [rows, K] exactly representable in h2, signs sh / sl ([rows, K] +-1) of h / l"""
    e = torch.randint(2, 15, (rows, K), generator=gen).double()
    e[:, 0] = 14                                                   # the row maximum: h in [2^14, 2^15)
    h = torch.randint(1024, 2048, (rows, K), generator=gen).double() * torch.exp2(e - 10)
    lo = torch.randint(1024, 2048, (rows, K), generator=gen).double() * torch.exp2(e - 12)    # l / 2^11 < 2^(e-12): below half an ulp of h
    if rowexp is None:
        rowexp = torch.randint(-rexp, rexp + 1, (rows, 1), generator=gen).double()
    x = (sh * h + sl * lo * 2.0 ** -11) * torch.exp2(rowexp - 14)
    x32 = x.float()
    assert torch.equal(x32.double(), x)
    return x32


def exact_pair(M, N, K, gen, rexp=10, rowexp_a=None):
    al, al2, be, be2 = _sg(gen, M)[:, None], _sg(gen, M)[:, None], _sg(gen, N)[:, None], _sg(gen, N)[:, None]
    ga, de = _sg(gen, K)[None, :], _sg(gen, K)[None, :]
    A = h2_exact(M, K, gen, al * ga, al2 * de, rexp, rowexp_a)
    B = h2_exact(N, K, gen, be * de, be2 * ga, rexp)
    return A, B


def plain(rows, K, gen):
    x = torch.randn(rows, K, generator=gen) * torch.exp2(torch.randint(-20, 21, (rows, 1), generator=gen).float())
    x[::7] = 0.0
    spike = torch.arange(3, max(rows, 3), 11)
    x[spike, torch.randint(0, K, (len(spike),), generator=gen)] *= 4096.0
    return x


# ----------------------------------------------------------------------------------------------------------- device helpers
def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def split_dev(L, X, ld):
    """genrl_split_h2 of X (CPU fp32 [R, Cn]) -> (planes int16 [2 R ld], inv [R]) on the device"""
    R, Cn = X.shape
    x = X.cuda().contiguous()
    pl = torch.full((2 * R * ld + 64,), -1, dtype=torch.int16, device='cuda')
    inv = torch.empty(R + 4, device='cuda')
    rc = L.genrl_split_h2(x.data_ptr(), Cn, R, Cn, pl.data_ptr(), ld, R * ld, inv.data_ptr(), 0, stream())
    assert rc == 0, rc
    return pl, inv


def ratio_of(got, ref, scale, floor, Kc=None):
    """-> (worst |got - ref| / (2^-24 scale) over elements outside the floor, worst over all of err / (2^-24 scale + floor)) as
    the parent's bound reads: err <= Kc 2^-24 scale + floor  <=>  (err - floor) / (2^-24 scale) <= Kc"""
    got = got.double()
    err = (got - ref).abs()
    r = (err - floor).clamp_min(0) / (U * scale).clamp_min(1e-300)
    r = torch.nan_to_num(r, nan=float('inf'))
    return float(r.max()) if r.numel() else 0.0


class Log:
    def __init__(self):
        self.pos = 0

    def take(self):
        p = os.environ['GENRL_GEMM_LOG']
        if not os.path.exists(p):
            return []
        with open(p) as f:
            f.seek(self.pos)
            txt = f.read()
            self.pos = f.tell()
        return [ln.split()[0] for ln in txt.splitlines() if ln.strip()]


# ----------------------------------------------------------------------------------------------------------- genrl_gemm_h2
def _operands(c, gen):
    M, N, K, K1 = c['M'], c['N'], c['K'], c['K1']
    if c['kind'] == 'plain':
        A0, B0 = plain(M, K, gen), plain(N, K, gen)
        A1, B1 = (plain(M, K1, gen), plain(N, K1, gen)) if K1 else (None, None)
    else:
        A0, B0 = exact_pair(M, N, K, gen)
        A1 = B1 = None
        if K1:
            rexp = torch.randint(-10, 11, (M, 1), generator=gen).double()
            A1, B1 = exact_pair(M, N, K1, gen, rowexp_a=rexp + c['seg_exp'])
    z = c['zero'] or ''
    rows = [r for r in (0, 5, M - 1) if r < M]
    if 'a1' in z:
        A1[rows] = 0.0
    if 'a0' in z:
        A0[rows] = 0.0
    if 'b1' in z:
        B1[[3, N - 1]] = 0.0
    return A0, B0, A1, B1


def run_h2_case(c, L, log):
    gen = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    M, N = c['M'], c['N']
    A0, B0, A1, B1 = _operands(c, gen)
    ar0, a1r0, br0 = c['r0']
    pa, pb, pc = c['pad']

    def seg(A, B, arow0, brow0):
        k = -(-A.shape[1] // 64) * 64
        lda, ldb = k + pa, k + pb
        Af = torch.cat([torch.randn(arow0, A.shape[1], generator=gen), A]) if arow0 else A
        Bf = torch.cat([torch.randn(brow0, B.shape[1], generator=gen), B]) if brow0 else B
        ap, ai = split_dev(L, Af, lda)
        bp, bi = split_dev(L, Bf, ldb)
        Ra, Rb = Af.shape[0], Bf.shape[0]
        return dict(a=ap.data_ptr() + 2 * arow0 * lda, lda=lda, ap=Ra * lda, ai=ai.data_ptr() + 4 * arow0,
                    b=bp.data_ptr() + 2 * brow0 * ldb, ldb=ldb, bp=Rb * ldb, bi=bi.data_ptr() + 4 * brow0, k=k,
                    keep=(ap, ai, bp, bi), ainv=ai[arow0:arow0 + M].double(), binv=bi[brow0:brow0 + N].double())
    s0 = seg(A0, B0, ar0, br0)
    s1 = seg(A1, B1, a1r0, br0) if A1 is not None else None
    Ad = [A0.cuda().double()] + ([A1.cuda().double()] if s1 else [])
    Bd = [B0.cuda().double()] + ([B1.cuda().double()] if s1 else [])
    ref = sum(a @ b.T for a, b in zip(Ad, Bd))
    scale = sum(a.abs() @ b.abs().T for a, b in zip(Ad, Bd))
    floor = 0.0
    for a, b, s in zip(Ad, Bd, [s0] + ([s1] if s1 else [])):
        floor = floor + FLOOR_H2 * (s['ainv'][:, None] * b.abs().sum(1)[None, :] + a.abs().sum(1)[:, None] * s['binv'][None, :])
    bias = (torch.randn(N, generator=gen) * 2.0 ** torch.randint(-4, 5, (N,), generator=gen)).cuda()
    C0 = (torch.randn(M, N, generator=gen).cuda().double() * ref.abs().clamp_min(1e-30) * 0.5).float()
    ldc = N + pc
    prev = L.genrl_planes_force_tile(c['force'])
    out = []
    try:
        for acc in ([False, True] if c['acc'] else [False]):
            reps = []
            for rep in range(2):
                cbuf, cv = out_buf(M, N, ldc, c['c_off'])
                if acc:
                    cv.copy_(C0)
                b_ = bias if c['bias'] else None
                x = s1 or dict(a=None, lda=0, ap=0, ai=None, b=None, ldb=0, bp=0, bi=None, k=0)
                rc = L.genrl_gemm_h2(s0['a'], s0['lda'], s0['ap'], s0['ai'], s0['b'], s0['ldb'], s0['bp'], s0['bi'], s0['k'],
                                     x['a'], x['lda'], x['ap'], x['ai'], x['b'], x['ldb'], x['bp'], x['bi'], x['k'],
                                     cv.data_ptr(), ldc, P(b_), M, N, int(acc), stream())
                route = int(L.genrl_planes_last_route())
                torch.cuda.synchronize()
                reps.append((rc, route, log.take(), cbuf, cv))
            (rc, route, fams, cbuf, cv), (_, _, _, cbuf2, cv2) = reps
            r_ref = ref + ((bias.double()[None, :] if b_ is not None else 0.0) + (C0.double() if acc else 0.0))
            r_sc = scale + ((bias.double().abs()[None, :] if b_ is not None else 0.0) + (C0.double().abs() if acc else 0.0))
            out.append(dict(call='acc' if acc else 'plain', rc=rc, route=route_names(route), fams=fams,
                            ratio=ratio_of(cv, r_ref, r_sc, floor), finite=bool(torch.isfinite(cv).all()),
                            untouched=outside_ok(cbuf, cv), repro=bool(torch.equal(cv, cv2))))
    finally:
        L.genrl_planes_force_tile(prev)
    return out


# ----------------------------------------------------------------------------------------------------------- uniform planes
def host_split(X, inv=None):
    """h2 split of X (CPU fp32 [R, C]) as the kernels do it: one power-of-two scale per row (inv given: that scale everywhere) ->
    (h, l fp16 as int16 bits, inv fp32 [R])"""
    x = X.numpy().astype(np.float32)
    if inv is None:
        amax = np.abs(x).max(1).astype(np.float32)
        E = ((amax.view(np.uint32) >> 23) & 255).astype(np.int64)
        es = np.where(amax == 0, 250, np.clip(268 - E, 4, 249))
        inv = ((254 - es) << 23).astype(np.uint32).view(np.float32)
    inv = np.broadcast_to(np.asarray(inv, np.float32).reshape(-1), (x.shape[0],)).copy()
    sc = (((254 - ((inv.view(np.uint32) >> 23) & 255)) << 23).astype(np.uint32)).view(np.float32)
    xs = (x * sc[:, None]).astype(np.float32)
    h = xs.astype(np.float16)
    lo = ((xs - h.astype(np.float32)) * np.float32(2048.0)).astype(np.float32).astype(np.float16)
    return torch.from_numpy(h.view(np.int16).copy()), torch.from_numpy(lo.view(np.int16).copy()), torch.from_numpy(inv)


def planes_dev(h, lo, ld, extra_rows=0):
    """[2][R][ld] int16 planes on the device from host h, l ([R, C]), zero padded"""
    R, C = h.shape
    pl = torch.zeros(2, R + extra_rows, ld, dtype=torch.int16)
    pl[0, :R, :C] = h
    pl[1, :R, :C] = lo
    return pl.reshape(-1).cuda(), (R + extra_rows) * ld


def h2_value(h, lo, inv):
    """float64 value of host planes"""
    hv = torch.from_numpy(h.numpy().view(np.float16).astype(np.float64))
    lv = torch.from_numpy(lo.numpy().view(np.float16).astype(np.float64))
    return (hv + lv / 2048.0) * inv.double()[:, None]


def uniform_image(rows, C, gen):
    """NHWC image rows x C of exact h2 values whose rows all reach [1, 2): one scale (inverse 2^-14) for the whole tensor"""
    return h2_exact(rows, C, gen, _sg(gen, rows * C).reshape(rows, C), _sg(gen, rows * C).reshape(rows, C), rowexp=torch.zeros(rows, 1))


def patches(img, n, H, W, C, k, s):
    oh, ow = (H - k) // s + 1, (W - k) // s + 1
    v = img.reshape(-1).as_strided((n, oh, ow, k, k, C), (H * W * C, s * W * C, s * C, W * C, C, 1))
    return v.reshape(n * oh * ow, k * k * C)


def run_conv(cid, n, H, W, Cc, k, N, ldx, route, L, log):
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    img = uniform_image(n * H * W, Cc, gen)
    Ko = k * k * Cc
    b_ld = -(-Ko // 64) * 64
    Wt = plain(N, Ko, gen) if 'odd' in cid else exact_pair(N, 8, Ko, gen)[0]
    amax = float(img.abs().max())
    hi, li, iv = host_split(img)
    inv_u = float(iv.max())
    hi, li, iv = host_split(img, inv_u)
    ld_img = Cc + ldx
    ipl, iplane = planes_dev(hi, li, ld_img)
    iinv = torch.full((n * H * W,), inv_u, device='cuda')
    bpl, binv = split_dev(L, Wt, b_ld)
    ho, wo = (H - k) // 2 + 1, (W - k) // 2 + 1
    M = n * ho * wo
    A64 = patches(h2_value(hi, li, iv).cuda(), n, H, W, Cc, k, 2)
    B64 = Wt.cuda().double()
    ref, scale = A64 @ B64.T, A64.abs() @ B64.abs().T
    floor = FLOOR_H2 * (inv_u * B64.abs().sum(1)[None, :] + A64.abs().sum(1)[:, None] * binv[:N].double()[None, :])
    bias = torch.randn(N, generator=gen).cuda()
    C0 = torch.randn(M, N, generator=gen).cuda() * 4.0
    out = []
    for acc in (False, True):
        reps = []
        for rep in range(2):
            cbuf, cv = out_buf(M, N, N + 4)
            if acc:
                cv.copy_(C0)
            rc = L.genrl_gemm_h2_conv(ipl.data_ptr(), ld_img, iplane, iinv.data_ptr(), n, H, W, Cc, k, bpl.data_ptr(), b_ld, N * b_ld,
                                      binv.data_ptr(), cv.data_ptr(), N + 4, P(bias) if acc else None, N, int(acc), stream())
            route_w = int(L.genrl_planes_last_route())
            torch.cuda.synchronize()
            reps.append((rc, route_w, log.take(), cbuf, cv))
        (rc, route_w, fams, cbuf, cv), (_, _, _, _, cv2) = reps
        r_ref = ref + ((bias.double()[None, :] + C0.double()) if acc else 0.0)
        r_sc = scale + ((bias.double().abs()[None, :] + C0.double().abs()) if acc else 0.0)
        out.append(dict(call='acc' if acc else 'plain', rc=rc, route=route_names(route_w), fams=fams, want=[route],
                        ratio=ratio_of(cv, r_ref, r_sc, floor), finite=bool(torch.isfinite(cv).all()),
                        untouched=outside_ok(cbuf, cv), repro=bool(torch.equal(cv, cv2))))
    return out


def run_subpixel(cid, n, Hi, Wi, Cc, T, Co, Ho, Wo, with_bias, zero_tap, L, log):
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    pad = T - 1
    Hp, Wp = Hi + 2 * pad, Wi + 2 * pad
    Hq, Wq = Hp - T + 1, Wp - T + 1
    img = torch.zeros(n, Hp, Wp, Cc)
    img[:, pad:pad + Hi, pad:pad + Wi] = uniform_image(n * Hi * Wi, Cc, gen).reshape(n, Hi, Wi, Cc)
    img = img.reshape(-1, Cc)
    hi, li, iv = host_split(img, IMG_INV)
    ipl, iplane = planes_dev(hi, li, Cc)
    iinv = torch.full((n * Hp * Wp,), IMG_INV, device='cuda')
    K = T * T * Cc
    b_ld = -(-K // 64) * 64
    N = 4 * Co
    Wt = exact_pair(N, 8, K, gen)[0].reshape(2, 2, Co, T, T, Cc)
    if zero_tap:                                   # k = 2T - 1: tap index 2T - 1 (a = 1, u = 0 / b = 1, v = 0) does not exist
        Wt[1, :, :, 0] = 0.0
        Wt[:, 1, :, :, 0] = 0.0
    Wt = Wt.reshape(N, K)
    bpl, binv = split_dev(L, Wt, b_ld)
    bias = torch.randn(N, generator=gen).cuda() if with_bias else None
    A64 = patches(h2_value(hi, li, iv).cuda(), n, Hp, Wp, Cc, T, 1)
    B64 = Wt.cuda().double()
    R, S = A64 @ B64.T, A64.abs() @ B64.abs().T
    F = FLOOR_H2 * (IMG_INV * B64.abs().sum(1)[None, :] + A64.abs().sum(1)[:, None] * binv[:N].double()[None, :])
    if bias is not None:
        R, S = R + bias.double()[None, :], S + bias.double().abs()[None, :]
    ref = torch.full((n, 2 * Hq, 2 * Wq, Co), float('nan'), dtype=torch.float64, device='cuda')
    scale, floor = torch.ones_like(ref), torch.zeros_like(ref)
    for t, src in ((ref, R), (scale, S), (floor, F)):
        v = src.reshape(n, Hq, Wq, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * Hq, 2 * Wq, Co)
        t[:] = v
    hh, ww = min(Ho, 2 * Hq), min(Wo, 2 * Wq)
    reps = []
    for rep in range(2):
        buf = torch.full((n * Ho * Wo * Co + 64,), PAD, device='cuda')
        outv = buf[:n * Ho * Wo * Co].view(n, Ho, Wo, Co)
        outv[:, :hh, :ww].fill_(float('nan'))
        rc = L.genrl_gemm_h2_subpixel(ipl.data_ptr(), Cc, iplane, iinv.data_ptr(), n, Hp, Wp, Cc, T, bpl.data_ptr(), b_ld, N * b_ld,
                                      binv.data_ptr(), outv.data_ptr(), Ho, Wo, Co, P(bias), stream())
        route_w = int(L.genrl_planes_last_route())
        torch.cuda.synchronize()
        reps.append((rc, route_w, log.take(), buf, outv))
    (rc, route_w, fams, buf, outv), (_, _, _, buf2, _) = reps
    got = outv[:, :hh, :ww]
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:n * Ho * Wo * Co].view(n, Ho, Wo, Co)[:, :hh, :ww] = False
    return [dict(call='plain', rc=rc, route=route_names(route_w), fams=fams, want=['subpixel/hlw' if -(-N // 192) * 192 < -(-N // 128) * 128 else 'subpixel/hl'],
                 ratio=ratio_of(got, ref[:, :hh, :ww], scale[:, :hh, :ww], floor[:, :hh, :ww]), finite=bool(torch.isfinite(got).all()),
                 untouched=bool((buf[mask] == PAD).all()), repro=bool(torch.equal(buf, buf2)),
                 nothing=bool((buf[mask] == PAD).all()) and bool(torch.isnan(got).all()))]


# ----------------------------------------------------------------------------------------------------------- TN
def tn_operands(M, NI, NJ, gen):
    """A [M, NI], B [M, NJ]: h2-exact per row m, cross terms of one output element of one sign; rows 7, 8 of A and B zero, rows
    from 64 on spread over 2^+-30 (some of them vanish in their split by design)"""
    ga, de = _sg(gen, M)[:, None], _sg(gen, M)[:, None]
    rexp_a = torch.randint(-10, 11, (M, 1), generator=gen).double()
    rexp_b = torch.randint(-10, 11, (M, 1), generator=gen).double()
    if M > 128:
        rexp_a[64::5] += 30.0
        rexp_b[100::9] -= 30.0
    A = h2_exact(M, NI, gen, ga * _sg(gen, NI)[None, :], de * _sg(gen, NI)[None, :], rowexp=rexp_a)
    B = h2_exact(M, NJ, gen, de * _sg(gen, NJ)[None, :], ga * _sg(gen, NJ)[None, :], rowexp=rexp_b)
    A[7:9] = 0.0
    B[8:10] = 0.0
    return A, B


def tn_floor(A64, B64, ia, ib, M, sps):
    """per element: 2^-24 sum_m cref(split of m) |a'(m, i)| (the fp16 rounding of b' f below fp16's normal range, at most 2^-25 per
    plane value) + the whole contribution of rows whose factor f < 2^-24 (those vanish: gemm_planes_tn.hip header)"""
    e = torch.log2(ia.double()) + torch.log2(ib.double())
    f = torch.empty_like(e)
    cref = torch.empty_like(e)
    for s0 in range(0, M, sps * 64):
        sl = slice(s0, min(M, s0 + sps * 64))
        emax = e[sl].max()
        f[sl] = torch.exp2(e[sl] - emax)
        cref[sl] = torch.exp2(emax)
    ap = A64.abs() / ia.double()[:, None]
    fl = 2.0 ** -24 * (cref[:, None] * ap).sum(0)[:, None]
    gone = (f < 2.0 ** -24).double()[:, None]
    return fl + (A64.abs() * gone).T @ B64.abs()


def run_tn(cid, NI, NJ, M, acc, pc, ar0, br0, L, log):
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    A, B = tn_operands(M, NI, NJ, gen)
    a_ld, b_ld = -(-NI // 64) * 64, -(-NJ // 64) * 64
    Af = torch.cat([torch.randn(ar0, NI, generator=gen), A]) if ar0 else A
    Bf = torch.cat([torch.randn(br0, NJ, generator=gen), B]) if br0 else B
    apl, ai = split_dev(L, Af, a_ld)
    bpl, bi = split_dev(L, Bf, b_ld)
    ia, ib = ai[ar0:ar0 + M].clone(), bi[br0:br0 + M].clone()       # (16-byte aligned copies)
    nsplit, sps = tn_plan(NI, NJ, M)
    wsb = int(L.genrl_gemm_h2_tn_ws_bytes(NI, NJ, M))
    ws = torch.full(((wsb + 4095) // 4,), float('nan'), device='cuda')
    A64, B64 = A.cuda().double(), B.cuda().double()
    ref, scale = A64.T @ B64, A64.abs().T @ B64.abs()
    floor = tn_floor(A64, B64, ia, ib, M, sps)
    ldc = NJ + pc
    C0 = torch.randn(NI, NJ, generator=gen).cuda()
    reps = []
    for rep in range(2):
        cbuf, cv = out_buf(NI, NJ, ldc)
        if acc:
            cv.copy_(C0)
        rc = L.genrl_gemm_h2_tn(apl.data_ptr() + 2 * ar0 * a_ld, a_ld, Af.shape[0] * a_ld, ia.data_ptr(),
                                bpl.data_ptr() + 2 * br0 * b_ld, b_ld, Bf.shape[0] * b_ld, ib.data_ptr(), cv.data_ptr(), ldc, NI, NJ, M,
                                int(acc), ws.data_ptr(), wsb, stream())
        route_w = int(L.genrl_planes_last_route())
        torch.cuda.synchronize()
        reps.append((rc, route_w, log.take(), cbuf, cv))
    (rc, route_w, fams, cbuf, cv), (_, _, _, _, cv2) = reps
    r_ref, r_sc = (ref + C0.double(), scale + C0.double().abs()) if acc else (ref, scale)
    return [dict(call='acc' if acc else 'plain', rc=rc, route=route_names(route_w), fams=fams, want=['tn'], splits=nsplit,
                 ratio=ratio_of(cv, r_ref, r_sc, floor), finite=bool(torch.isfinite(cv).all()), untouched=outside_ok(cbuf, cv),
                 repro=bool(torch.equal(cv, cv2)))]


def run_tn_conv(cid, NI, n, H, W, Cc, k, L, log):
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    ho, wo = (H - k) // 2 + 1, (W - k) // 2 + 1
    M = n * ho * wo
    assert M % 64 == 0, (cid, M)
    NJ = k * k * Cc
    img = uniform_image(n * H * W, Cc, gen)
    hi, li, iv = host_split(img, IMG_INV)
    ipl, iplane = planes_dev(hi, li, Cc)
    iinv = torch.full((max(M, n * H * W) + 64,), IMG_INV, device='cuda')
    A = tn_operands(M, NI, 8, gen)[0]
    a_ld = -(-NI // 64) * 64
    apl, ai = split_dev(L, A, a_ld)
    m = torch.arange(M)
    nn_, oy, ox = m // (ho * wo), (m // wo) % ho, m % wo
    ro = ((nn_ * H + 2 * oy) * W + 2 * ox) * Cc * 2
    rowoff = torch.cat([ro, ro[-1:].repeat(256)]).to(torch.int32).cuda()
    Pm = patches(h2_value(hi, li, iv).cuda(), n, H, W, Cc, k, 2)
    A64 = A.cuda().double()
    ref, scale = A64.T @ Pm, A64.abs().T @ Pm.abs()
    nsplit, sps = tn_plan(NI, NJ, M)
    floor = tn_floor(A64, Pm, ai[:M], iinv[:M], M, sps)
    wsb = int(L.genrl_gemm_h2_tn_ws_bytes(NI, NJ, M))
    ws = torch.full(((wsb + 4095) // 4,), float('nan'), device='cuda')
    reps = []
    for rep in range(2):
        cbuf, cv = out_buf(NI, NJ, NJ)
        rc = L.genrl_gemm_h2_tn_conv(apl.data_ptr(), a_ld, M * a_ld, ai.data_ptr(), ipl.data_ptr(), Cc, iplane, iinv.data_ptr(),
                                     rowoff.data_ptr(), W, Cc, k, cv.data_ptr(), NJ, NI, M, 0, ws.data_ptr(), wsb, stream())
        route_w = int(L.genrl_planes_last_route())
        torch.cuda.synchronize()
        reps.append((rc, route_w, log.take(), cbuf, cv))
    (rc, route_w, fams, cbuf, cv), (_, _, _, _, cv2) = reps
    return [dict(call='plain', rc=rc, route=route_names(route_w), fams=fams, want=['tn/conv'], splits=nsplit,
                 ratio=ratio_of(cv, ref, scale, floor), finite=bool(torch.isfinite(cv).all()), untouched=outside_ok(cbuf, cv),
                 repro=bool(torch.equal(cv, cv2)))]


# ----------------------------------------------------------------------------------------------------------- x3
def run_x3(L, log):
    out = {}
    for cid, M, N, K, K1, force, want in (('x3.64.two-seg', 300, 200, 128, 64, 0, 'x3/64'), ('x3.128.two-seg', 1000, 300, 192, 128, 2, 'x3/128'),
                                           ('x3.128.auto', 8192, 1024, 64, 0, 0, 'x3/128')):
        gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
        segs = [(plain(M, K, gen), plain(N, K, gen))] + ([(plain(M, K1, gen), plain(N, K1, gen))] if K1 else [])
        pls = []
        for A, B in segs:
            k = A.shape[1]
            pa = torch.zeros(3 * M * k + 64, dtype=torch.int16, device='cuda')
            pb = torch.zeros(3 * N * k + 64, dtype=torch.int16, device='cuda')
            for X, pl, R in ((A, pa, M), (B, pb, N)):
                x = X.cuda()
                assert L.genrl_split_x3(x.data_ptr(), k, R, k, pl.data_ptr(), k, R * k, 0, stream()) == 0
            pls.append((pa, pb, k))
        ref = sum(A.cuda().double() @ B.cuda().double().T for A, B in segs)
        scale = sum(A.cuda().double().abs() @ B.cuda().double().abs().T for A, B in segs)
        bias = torch.randn(N, generator=gen).cuda()
        C0 = torch.randn(M, N, generator=gen).cuda()
        prev = L.genrl_planes_force_tile(force)
        res = []
        for acc in (False, True):
            reps = []
            for rep in range(2):
                cbuf, cv = out_buf(M, N, N + 2)
                if acc:
                    cv.copy_(C0)
                (a0, b0, k0), (a1, b1, k1_) = pls[0], (pls[1] if K1 else (None, None, 0))
                rc = L.genrl_gemm_x3(a0.data_ptr(), k0, M * k0, b0.data_ptr(), k0, N * k0, k0, P(a1), k1_, M * k1_, P(b1), k1_, N * k1_,
                                     k1_, cv.data_ptr(), N + 2, P(bias) if acc else None, M, N, int(acc), stream())
                route_w = int(L.genrl_planes_last_route())
                torch.cuda.synchronize()
                reps.append((rc, route_w, log.take(), cbuf, cv))
            (rc, route_w, fams, cbuf, cv), (_, _, _, _, cv2) = reps
            r_ref = ref + ((bias.double()[None, :] + C0.double()) if acc else 0.0)
            r_sc = scale + ((bias.double().abs()[None, :] + C0.double().abs()) if acc else 0.0)
            res.append(dict(call='acc' if acc else 'plain', rc=rc, route=route_names(route_w), fams=fams, want=[want],
                            ratio=ratio_of(cv, r_ref, r_sc, 0.0), finite=bool(torch.isfinite(cv).all()), untouched=outside_ok(cbuf, cv),
                            repro=bool(torch.equal(cv, cv2))))
        L.genrl_planes_force_tile(prev)
        out[cid] = res
    return out


# ----------------------------------------------------------------------------------------------------------- split kernels
def check_split(X, pl, inv, ld, transpose):
    """-> list of failures of the documented representation and of the exact float64 recomputation"""
    R_, C_ = X.shape
    Xs = X.T.contiguous() if transpose else X
    R, C = Xs.shape
    bad = []
    h, lo, iv = host_split(Xs)
    inv = inv[:R].cpu()
    if not torch.equal(inv, iv):
        bad.append(f'inv differs from float64 recomputation at {int((inv != iv).nonzero()[0])}')
    e = torch.log2(inv.double())
    if not torch.equal(e, e.round()):
        bad.append('inv not a power of two')
    p = pl[:2 * R * ld].view(2, R, ld).cpu()
    if not torch.equal(p[0, :, :C], h) or not torch.equal(p[1, :, :C], lo):
        d = ((p[0, :, :C] != h) | (p[1, :, :C] != lo)).nonzero()[0]
        bad.append(f'planes differ from float64 recomputation at {tuple(int(v) for v in d)}')
    if ld > C and (p[:, :, C:] != 0).any():
        bad.append('padding not zero')
    x64 = Xs.double()
    amax = x64.abs().max(1).values
    nz = amax > 0
    s = 1.0 / inv.double()
    top = amax * s
    big = amax >= 2.0 ** -108           # (s is capped at 2^122 below that: the row maximum x s stays under 2^14)
    if not ((top[big] >= 2 ** 14) & (top[big] < 2 ** 15)).all():
        bad.append('row maximum x s outside [2^14, 2^15)')
    if not (inv[nz & ~big] == 2.0 ** -122).all():
        bad.append('nonzero row below 2^-108 without inv = 2^-122')
    if not (inv[~nz] == 2.0 ** -123).all():
        bad.append('zero row without inv = 2^-123')
    if (p[:, ~nz, :] != 0).any():
        bad.append('zero row with nonzero planes')
    val = h2_value(p[0, :, :C], p[1, :, :C], torch.ones(R))
    xs = x64 * s[:, None]
    near = x64.abs() >= amax[:, None] * 2.0 ** -28
    if ((xs - val).abs() > 2.0 ** -22 * xs.abs())[near & big[:, None]].any():
        bad.append('|a s - h - l / 2^11| > 2^-22 |a s| within 2^-28 of the row maximum')
    return bad


def split_inputs(gen, R, C):
    """plain rows, row 2 zero, column 1 zero, row 4 nonzero below 2^-108 (inverse scale 2^-122, not the zero row's 2^-123)"""
    X = plain(R, C, gen)
    X[2, :] = 0.0
    X[:, 1] = 0.0
    if R > 4:
        X[4] = torch.randn(C, generator=gen) * 2.0 ** -118
    return X


def run_split(L, log):
    out = {}
    for cid, R, C, ld, tr in (('split.rows', 70, 100, 128, 0), ('split.rows.wide', 5, 1000, 1024, 0), ('split.t', 100, 70, 128, 1),
                              ('split.t.tall', 1000, 33, 1024, 1)):
        gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
        X = split_inputs(gen, R, C)
        Ro = C if tr else R
        x = X.cuda()
        pl = torch.full((2 * Ro * ld + 64,), 0x5A5A, dtype=torch.int16, device='cuda')
        inv = torch.full((Ro + 4,), float('nan'), device='cuda')
        rc = L.genrl_split_h2(x.data_ptr(), C, R, C, pl.data_ptr(), ld, Ro * ld, inv.data_ptr(), tr, stream())
        torch.cuda.synchronize()
        bad = check_split(X, pl, inv, ld, tr) if rc == 0 else []
        if (pl[2 * Ro * ld:] != 0x5A5A).any():
            bad.append('wrote past the planes')
        out[cid] = dict(rc=rc, bad=bad)
    # batch: 70 entries, 35 row and 35 transposed ones interleaved: each pass takes two chunks (32 + 3 entries)
    from genrl_amd._lib import struct
    Desc = struct('genrl_split_desc')
    gen = torch.Generator().manual_seed(77)
    ents = []
    descs = (Desc * 70)()
    for i in range(70):
        R, C = int(torch.randint(1, 150, (1,), generator=gen)), int(torch.randint(1, 150, (1,), generator=gen))
        tr = i % 2
        Ro, Co = (C, R) if tr else (R, C)
        ld = -(-Co // 64) * 64 + (64 if i % 7 == 0 else 0)
        X = split_inputs(gen, R, C) if R > 2 and C > 1 else plain(R, C, gen)
        x = X.cuda()
        pl = torch.full((2 * Ro * ld + 64,), 0x5A5A, dtype=torch.int16, device='cuda')
        inv = torch.full((Ro + 4,), float('nan'), device='cuda')
        descs[i] = Desc(x.data_ptr(), C, R, C, pl.data_ptr(), ld, Ro * ld, inv.data_ptr(), tr)
        ents.append((X, x, pl, inv, ld, tr, Ro))
    rc = L.genrl_split_h2_batch(descs, 70, stream())
    torch.cuda.synchronize()
    bad = []
    for i, (X, x, pl, inv, ld, tr, Ro) in enumerate(ents):
        bad += [f'entry {i}: {b}' for b in check_split(X, pl, inv, ld, tr)]
        if (pl[2 * Ro * ld:] != 0x5A5A).any():
            bad.append(f'entry {i}: wrote past the planes')
    out['split.batch70'] = dict(rc=rc, bad=bad)
    # x3: three bf16 planes, exact: h + m + l = x for every element (normal range)
    for cid, R, C, ld, tr in (('x3split.rows', 70, 100, 128, 0), ('x3split.t', 100, 70, 104, 1)):
        gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
        X = torch.randn(R, C, generator=gen) * torch.exp2(torch.randint(-20, 21, (R, 1), generator=gen).float())
        Ro, Co = (C, R) if tr else (R, C)
        x = X.cuda()
        pl = torch.full((3 * Ro * ld + 64,), 0x5A5A, dtype=torch.int16, device='cuda')
        rc = L.genrl_split_x3(x.data_ptr(), C, R, C, pl.data_ptr(), ld, Ro * ld, tr, stream())
        torch.cuda.synchronize()
        p = pl[:3 * Ro * ld].view(3, Ro, ld).cpu().to(torch.int32) & 0xFFFF
        v = sum(((p[i] << 16).to(torch.int32).view(torch.float32)).double() for i in range(3))
        Xo = (X.T if tr else X).double()
        bad = []
        if not torch.equal(v[:, :Co], Xo):
            bad.append('h + m + l != x')
        if ld > Co and (p[:, :, Co:] != 0).any():
            bad.append('padding not zero')
        if (pl[3 * Ro * ld:] != 0x5A5A).any():
            bad.append('wrote past the planes')
        out[cid] = dict(rc=rc, bad=bad)
    return out


# ----------------------------------------------------------------------------------------------------------- sample / LayerNorm epilogues
# genrl_gemm_h2_ln: (id, M, N, K, K1, zero rows, segment-1 exponent offset); N % 64 == 0 and every workgroup resident (genrl_gemm_h2_ln_ok)
LN = [
    ('ln.one-seg.M60.N1024', 60, 1024, 192, 0, None, 0),
    ('ln.two-seg.N512', 1000, 512, 256, 128, None, 0),
    ('ln.a1-2^30', 700, 256, 256, 128, None, 30),         # (2^40: the fp32 variance of the C rows would overflow)
    ('ln.a1-2^-40', 700, 256, 256, 128, None, -40),
    ('ln.zero-a1-rows', 700, 256, 256, 128, 'a1', 0),
    ('ln.zero-b1-rows', 700, 256, 256, 128, 'b1', 0),
]
# genrl_gemm_h2_sample: (id, M, N, K)
SAMPLE = [('sample.1000x1024', 1000, 1024, 1024), ('sample.ragged.300x64', 300, 64, 200)]


def _h2_case_operands(cid, M, N, K, K1, zero, seg_exp, L):
    c = g(cid, M, N, K, [], K1=K1, zero=zero, seg_exp=seg_exp)
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    A0, B0, A1, B1 = _operands(c, gen)
    segs = []
    for A, B in ((A0, B0), (A1, B1)) if K1 else ((A0, B0),):
        k = -(-A.shape[1] // 64) * 64
        ap, ai = split_dev(L, A, k)
        bp, bi = split_dev(L, B, k)
        segs.append(dict(a=ap, ai=ai, b=bp, bi=bi, k=k, A=A.cuda().double(), B=B.cuda().double()))
    ref = sum(x['A'] @ x['B'].T for x in segs)
    scale = sum(x['A'].abs() @ x['B'].abs().T for x in segs)
    floor = sum(FLOOR_H2 * (x['ai'][:M].double()[:, None] * x['B'].abs().sum(1)[None, :] + x['A'].abs().sum(1)[:, None] *
                            x['bi'][:N].double()[None, :]) for x in segs)
    return gen, segs, ref, scale, floor


def _seg_args(segs, M, N):
    out = []
    for i in range(2):
        if i < len(segs):
            x = segs[i]
            out += [x['a'].data_ptr(), x['k'], M * x['k'], x['ai'].data_ptr(), x['b'].data_ptr(), x['k'], N * x['k'], x['bi'].data_ptr(), x['k']]
        else:
            out += [None, 0, 0, None, None, 0, 0, None, 0]
    return out


def run_ln(cid, M, N, K, K1, zero, seg_exp, L, log):
    """C = A0 B0^T (+ A1 B1^T) + bias per element against float64; y = SiLU(LayerNorm(C) gamma + beta) and mean against the float64
    LayerNorm of the kernel's own C"""
    assert L.genrl_gemm_h2_ln_ok(M, N) == 1, (cid, M, N)
    gen, segs, ref, scale, floor = _h2_case_operands(cid, M, N, K, K1, zero, seg_exp, L)
    bias = torch.randn(N, generator=gen).cuda()
    gamma = (1.0 + 0.2 * torch.randn(N, generator=gen)).cuda()
    beta = (0.1 * torch.randn(N, generator=gen)).cuda()
    part = torch.zeros(int(L.genrl_gemm_h2_ln_part_floats(M, N)) + 64, device='cuda')
    sync = torch.zeros(int(L.genrl_gemm_h2_ln_sync_words()) + 4, dtype=torch.int32, device='cuda')
    reps = []
    for rep in range(2):
        cbuf, cv = out_buf(M, N, N)
        ybuf, yv = out_buf(M, N, N)
        mean = torch.full((M,), float('nan'), device='cuda')
        rstd = torch.full((M,), float('nan'), device='cuda')
        rc = L.genrl_gemm_h2_ln(*_seg_args(segs, M, N), cv.data_ptr(), N, bias.data_ptr(), M, N, gamma.data_ptr(), beta.data_ptr(),
                                1e-5, 1, yv.data_ptr(), N, mean.data_ptr(), rstd.data_ptr(), None, 0, 0, None, part.data_ptr(),
                                sync.data_ptr(), stream())
        route_w = int(L.genrl_planes_last_route())
        torch.cuda.synchronize()
        reps.append((rc, route_w, log.take(), cbuf, cv, ybuf, yv, mean))
    (rc, route_w, fams, cbuf, cv, ybuf, yv, mean), (_, _, _, _, cv2, _, yv2, _) = reps
    c64 = cv.double()
    mu = c64.mean(1, keepdim=True)
    z = (c64 - mu) / torch.sqrt(((c64 - mu) ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    y64 = z * torch.sigmoid(z)
    y_err = float(((yv.double() - y64).abs() / (1.0 + y64.abs())).max())
    m_err = float(((mean.double() - mu[:, 0]).abs() / (c64.abs().mean(1) + 1e-30)).max())
    return [dict(call='plain', rc=rc, route=route_names(route_w), fams=fams, want=['64/ln'],
                 ratio=ratio_of(cv, ref + bias.double()[None, :], scale + bias.double().abs()[None, :], floor),
                 finite=bool(torch.isfinite(cv).all()) and bool(torch.isfinite(yv).all()) and int(sync[0]) == 0,
                 untouched=outside_ok(cbuf, cv) and outside_ok(ybuf, yv), repro=bool(torch.equal(cv, cv2) and torch.equal(yv, yv2)),
                 y_err=y_err, mean_err=m_err)]


def run_sample(cid, M, N, K, L, log):
    """C = A B^T + bias per element against float64; the one-hot sample = argmax_k (0.99 softmax + 0.01 / 32)_k / q_k of the kernel's
    own C per 32-class latent (a tie of the two best within 2^-20 may go either way)"""
    gen, segs, ref, scale, floor = _h2_case_operands(cid, M, N, K, 0, None, 0, L)
    bias = torch.randn(N, generator=gen).cuda()
    q = (-torch.log(torch.rand(M, N, generator=gen).clamp_min(1e-12))).cuda()
    reps = []
    for rep in range(2):
        cbuf, cv = out_buf(M, N, N)
        sbuf, sv = out_buf(M, N, N)
        rc = L.genrl_gemm_h2_sample(*_seg_args(segs, M, N)[:9], cv.data_ptr(), N, bias.data_ptr(), M, N, q.data_ptr(), N, 0.99,
                                    sv.data_ptr(), N, None, 0, 0, None, stream())
        route_w = int(L.genrl_planes_last_route())
        torch.cuda.synchronize()
        reps.append((rc, route_w, log.take(), cbuf, cv, sbuf, sv))
    (rc, route_w, fams, cbuf, cv, sbuf, sv), (_, _, _, _, cv2, _, sv2) = reps
    lg = cv.double().reshape(M, N // 32, 32)
    p = 0.99 * torch.softmax(lg, -1) + 0.01 / 32
    sc = p / q.double().reshape(M, N // 32, 32)
    top2 = sc.topk(2, -1).values
    onehot = sv.double().reshape(M, N // 32, 32)
    ok_shape = bool(((onehot == 0) | (onehot == 1)).all()) and bool((onehot.sum(-1) == 1).all())
    chosen = (onehot * sc).sum(-1)
    tie = (top2[..., 0] - top2[..., 1]) <= 2.0 ** -20 * top2[..., 0]
    agree = ok_shape and bool(((chosen == top2[..., 0]) | (tie & (chosen >= top2[..., 1]))).all())
    return [dict(call='plain', rc=rc, route=route_names(route_w), fams=fams, want=['64/sample'],
                 ratio=ratio_of(cv, ref + bias.double()[None, :], scale + bias.double().abs()[None, :], floor),
                 finite=bool(torch.isfinite(cv).all()), untouched=outside_ok(cbuf, cv) and outside_ok(sbuf, sv),
                 repro=bool(torch.equal(cv, cv2) and torch.equal(sv, sv2)), sample_ok=agree)]


# ----------------------------------------------------------------------------------------------------------- refusals
def run_refusals(L, log):
    s = stream()
    pl = torch.zeros(2 * 256 * 256 + 64, dtype=torch.int16, device='cuda')
    inv = torch.full((1024,), 2.0 ** -14, device='cuda')
    p, iv = pl.data_ptr(), inv.data_ptr()
    h2 = lambda c, k0=64, lda=64, k1=0, ld1=64: L.genrl_gemm_h2(p, lda, 64 * 64, iv, p, 64, 64 * 64, iv, k0, p if k1 else None, ld1, 64 * 64,
                                                               iv if k1 else None, p if k1 else None, ld1, 64 * 64, iv if k1 else None, k1,
                                                               c, 64, None, 64, 64, 0, s)
    conv = lambda c, Cc=48, b_ld=768, ld_img=48: L.genrl_gemm_h2_conv(p, ld_img, 1000, iv, 1, 10, 10, Cc, 4, p, b_ld, 64 * b_ld, iv, c, 64,
                                                                      None, 64, 0, s)
    sub = lambda c, Co=48, off=0: L.genrl_gemm_h2_subpixel(p, 48, 1000, iv, 1, 5, 5, 48, 2, p, 192, 4 * Co * 192, iv, c + off, 8, 8, Co,
                                                           None, s)
    ws = torch.zeros(1 << 20, device='cuda')
    wsb = int(L.genrl_gemm_h2_tn_ws_bytes(64, 64, 128))
    tn = lambda c, M=128, wb=wsb, woff=0, ioff=0: L.genrl_gemm_h2_tn(p, 64, 128 * 64, iv + ioff, p, 64, 128 * 64, iv, c, 64, 64, 64, M, 0,
                                                                    ws.data_ptr() + woff, wb, s)
    calls = {                          # (the base arguments of each entry point: accepted, they write C)
        'h2.base': lambda c: h2(c),
        'conv.base': lambda c: conv(c),
        'subpixel.base': lambda c: sub(c),
        'tn.base': lambda c: tn(c),
        'h2.k0%64': lambda c: h2(c, k0=96),
        'h2.k1%64': lambda c: h2(c, k1=32),
        'h2.lda%8': lambda c: h2(c, lda=68),
        'h2.ld1%8': lambda c: h2(c, k1=64, ld1=66),
        'conv.Cc<48': lambda c: conv(c, Cc=40, b_ld=640, ld_img=40),
        'conv.Cc%8': lambda c: conv(c, Cc=52, b_ld=832, ld_img=52),
        'conv.b_ld-short': lambda c: conv(c, b_ld=704),
        'conv.b_ld-long': lambda c: conv(c, b_ld=832),
        'subpixel.Co%4': lambda c: sub(c, Co=50),
        'subpixel.unaligned-out': lambda c: sub(c, off=4),
        'tn.M%64': lambda c: tn(c, M=96),
        'tn.ws-short': lambda c: tn(c, wb=wsb - 4),
        'tn.ws-unaligned': lambda c: tn(c, woff=128),
        'tn.scales-unaligned': lambda c: tn(c, ioff=4),
    }
    out = {}
    for cid, fn in calls.items():
        buf = torch.full((64 * 64 * 8 + 64,), PAD, device='cuda')
        rc = int(fn(buf.data_ptr()))
        route_w = int(L.genrl_planes_last_route())
        torch.cuda.synchronize()
        out[cid] = dict(rc=rc, want=0 if cid.endswith('.base') else EINVAL, route=route_names(route_w),
                        untouched=bool((buf == PAD).all()), fams=log.take())
    return out


def run_group(group, L, log):
    if group in ROUTES:
        return {c['id']: run_h2_case(c, L, log) for c in ROUTES[group]}
    if group == 'conv':
        res = {c[0]: run_conv(*c, L, log) for c in CONV}
        res.update({c[0]: run_subpixel(*c, L, log) for c in SUBPIXEL})
        return res
    if group == 'conv_hl0':
        res = {c[0] + '.hl0': run_conv(c[0] + '.hl0', *c[1:8], 'conv/plain', L, log) for c in CONV[:3]}
        # the sub-pixel epilogue lives in the half-stage kernel: refused without it
        res['subpixel.hl0-refused'] = run_subpixel(*SUBPIXEL[0], L, log)
        return res
    if group == 'tn':
        res = {c[0]: run_tn(*c, L, log) for c in TN}
        res.update({c[0]: run_tn_conv(*c, L, log) for c in TN_CONV})
        return res
    if group == 'x3':
        return run_x3(L, log)
    if group == 'ln':
        return {c[0]: run_ln(*c, L, log) for c in LN}
    if group == 'sample':
        return {c[0]: run_sample(*c, L, log) for c in SAMPLE}
    if group == 'split':
        return run_split(L, log)
    if group == 'refuse':
        return run_refusals(L, log)
    raise KeyError(group)


def main(group, path):
    from genrl_amd._lib import lib
    L = lib()
    res = run_group(group, L, Log())
    with open(path, 'w') as f:
        json.dump(res, f)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
