"""The rectangular h2 tiles of csrc/gemm_planes.hip -- 64 x 192 (genrl_planes_force_tile 3, four plane-alternating half stages) and 128 x 64 (4, three
stages of 64 k; also genrl_gemm_h2_pair's) -- and the route that gives them the 1024-row GRU products of the imagination rollout.

A rectangular tile issues, per output element, the MFMA sequence of the 64 x 64 tile: every result here must be torch.equal to the forced
64 x 64 one.  Against float64 the bound is test_gpu_plane_variants.py's for the 64 x 64 family (|C - ref| <= Kc 2^-24 scale + floor, Kc =
K['64'], operands and floor as plane_route_child.py builds them).  Shapes: the smallest that reach every path -- one ragged tile; several
tiles with a ragged last row and column tile; K = 64 x 9 (every slot of the four- and of the three-stage ring and every fragment set wraps
twice); two segments with the boundary on a stage (K1 = 64) and far from the ring's period (K1 = 576), segment 1 at 2^+-40 of segment 0
and all-zero rows of a0 / a1 / b1 in the first AND the later 64-row / 64-column groups of a tile (rows 70, 199 of 128-row tiles, columns
70, 150 of 192-column tiles: the fold's zero-row rule runs once per group); bias, accumulation, row offsets, c_off, padded ldc.
The route's edges run at the rollout's own sizes (a few GFLOP each)."""
import json
import os
import subprocess
import sys
import tempfile
import zlib

import pytest
import torch

import plane_route_child as R
from f64check import out_buf, untouched_ok

pytestmark = pytest.mark.gpu

EINVAL = 1
KC = 150                  # test_gpu_plane_variants.K['64']
BIT = {'64/ns3': 0x1, '64/ns2': 0x2, '64x192': 0x20000, '128x64': 0x40000}
TILES = {3: '64x192', 4: '128x64'}


@pytest.fixture(scope='module')
def L():
    from genrl_amd._lib import lib
    return lib()


def names(word):
    return sorted(k for k, b in BIT.items() if (word & 0xFFFFFFFF) & b) + ([hex(word & ~sum(BIT.values()) & 0xFFFFFFFF)]
                                                                           if word & ~sum(BIT.values()) & 0xFFFFFFFF else [])


class forced:
    def __init__(self, L, t):
        self.L, self.t = L, t

    def __enter__(self):
        self.prev = self.L.genrl_planes_force_tile(self.t)

    def __exit__(self, *a):
        self.L.genrl_planes_force_tile(self.prev)


# (id, M, N, K, K1, dict(bias, r0 = (a_row0, a1_row0, b_row0), pad = (A, B, C), c_off, seg_exp, zero))
CASES = [
    ('one-tile.ragged', 70, 100, 64, 0, dict(c_off=1, pad=(64, 0, 3))),
    ('tiles.130x200.K128', 130, 200, 128, 0, dict(bias=False)),
    ('tiles.257x385.K192', 257, 385, 192, 0, dict(r0=(3, 0, 7), pad=(0, 64, 2))),
    ('ring-wrap.K576', 130, 200, 576, 0, dict(c_off=2)),
    ('seg.K1-64', 200, 200, 128, 64, dict(r0=(2, 5, 1))),
    ('seg.K1-576', 130, 200, 64, 576, dict(bias=False)),
    ('seg.a1-2^40', 200, 200, 128, 64, dict(seg_exp=40)),
    ('seg.a1-2^-40', 200, 200, 128, 64, dict(seg_exp=-40)),
    ('seg.zero-a1', 200, 200, 128, 64, dict(zero='a1')),
    ('seg.zero-a0', 200, 200, 128, 64, dict(zero='a0')),
    ('seg.zero-b1', 200, 200, 128, 64, dict(zero='b1')),
    ('seg.zero-a1-b1.K1-576', 200, 200, 64, 576, dict(zero='a1b1', pad=(0, 0, 4))),
]


def operands(cid, M, N, K, K1, o):
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    A0, B0 = R.exact_pair(M, N, K, gen)
    A1 = B1 = None
    if K1:
        rexp = torch.randint(-10, 11, (M, 1), generator=gen).double()
        A1, B1 = R.exact_pair(M, N, K1, gen, rowexp_a=rexp + o.get('seg_exp', 0))
    z = o.get('zero') or ''
    rows, cols = [r for r in (0, 5, 70, M - 1) if r < M], [c for c in (3, 70, 150, N - 1) if c < N]
    if 'a1' in z:
        A1[rows] = 0.0
    if 'a0' in z:
        A0[rows] = 0.0
    if 'b1' in z:
        B1[cols] = 0.0
    return gen, A0, B0, A1, B1


@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_forced_tiles_match_the_64x64_tile_and_float64(L, cid):
    _, M, N, K, K1, o = next(c for c in CASES if c[0] == cid)
    gen, A0, B0, A1, B1 = operands(cid, M, N, K, K1, o)
    ar0, a1r0, br0 = o.get('r0', (0, 0, 0))
    pa, pb, pc = o.get('pad', (0, 0, 0))
    c_off = o.get('c_off', 0)

    def seg(A, B, arow0, brow0):
        k = -(-A.shape[1] // 64) * 64
        lda, ldb = k + pa, k + pb
        Af = torch.cat([torch.randn(arow0, A.shape[1], generator=gen), A]) if arow0 else A
        Bf = torch.cat([torch.randn(brow0, B.shape[1], generator=gen), B]) if brow0 else B
        ap, ai = R.split_dev(L, Af, lda)
        bp, bi = R.split_dev(L, Bf, ldb)
        return dict(a=ap.data_ptr() + 2 * arow0 * lda, lda=lda, ap=Af.shape[0] * lda, ai=ai.data_ptr() + 4 * arow0,
                    b=bp.data_ptr() + 2 * brow0 * ldb, ldb=ldb, bp=Bf.shape[0] * ldb, bi=bi.data_ptr() + 4 * brow0, k=k,
                    keep=(ap, ai, bp, bi), ainv=ai[arow0:arow0 + M].double(), binv=bi[brow0:brow0 + N].double())
    s0 = seg(A0, B0, ar0, br0)
    s1 = seg(A1, B1, a1r0, br0) if A1 is not None else None
    x = s1 or dict(a=None, lda=0, ap=0, ai=None, b=None, ldb=0, bp=0, bi=None, k=0)
    Ad = [A0.cuda().double()] + ([A1.cuda().double()] if s1 else [])
    Bd = [B0.cuda().double()] + ([B1.cuda().double()] if s1 else [])
    ref = sum(a @ b.T for a, b in zip(Ad, Bd))
    scale = sum(a.abs() @ b.abs().T for a, b in zip(Ad, Bd))
    floor = 0.0
    for a, b, s in zip(Ad, Bd, [s0] + ([s1] if s1 else [])):
        floor = floor + R.FLOOR_H2 * (s['ainv'][:, None] * b.abs().sum(1)[None, :] + a.abs().sum(1)[:, None] * s['binv'][None, :])
    bias = (torch.randn(N, generator=gen) * 2.0 ** torch.randint(-4, 5, (N,), generator=gen)).cuda() if o.get('bias', True) else None
    C0 = (torch.randn(M, N, generator=gen).cuda().double() * ref.abs().clamp_min(1e-30) * 0.5).float()
    ldc = N + pc
    for acc in (False, True):
        got = {}
        for tile in (1, 3, 4):
            with forced(L, tile):
                cbuf, cv = out_buf(M, N, ldc, c_off)
                if acc:
                    cv.copy_(C0)
                rc = L.genrl_gemm_h2(s0['a'], s0['lda'], s0['ap'], s0['ai'], s0['b'], s0['ldb'], s0['bp'], s0['bi'], s0['k'],
                                     x['a'], x['lda'], x['ap'], x['ai'], x['b'], x['ldb'], x['bp'], x['bi'], x['k'],
                                     cv.data_ptr(), ldc, R.P(bias), M, N, int(acc), R.stream())
                route = names(int(L.genrl_planes_last_route()))
            torch.cuda.synchronize()
            what = f'{cid} tile {tile} acc {acc}'
            assert rc == 0, (what, rc)
            assert route == [TILES[tile]] if tile != 1 else route[0].startswith('64/'), (what, route)
            assert bool(torch.isfinite(cv).all()), f'{what}: C holds Inf or NaN'
            assert untouched_ok(cbuf, cv), f'{what}: a kernel wrote outside its output'
            got[tile] = cv
        r_ref = ref + ((bias.double()[None, :] if bias is not None else 0.0) + (C0.double() if acc else 0.0))
        r_sc = scale + ((bias.double().abs()[None, :] if bias is not None else 0.0) + (C0.double().abs() if acc else 0.0))
        for tile in (3, 4):
            ratio = R.ratio_of(got[tile], r_ref, r_sc, floor)
            print(f'{cid} {TILES[tile]} acc {acc}: worst (|C - ref| - floor) = {ratio:.3g} x 2^-24 scale (64x64: '
                  f'{R.ratio_of(got[1], r_ref, r_sc, floor):.3g})')
            assert ratio <= KC, f'{cid} {TILES[tile]} acc {acc}: {ratio:.3g} x 2^-24 scale, bound {KC}'
            assert torch.equal(got[tile], got[1]), (f'{cid} {TILES[tile]} acc {acc}: differs from the 64x64 tile in '
                                                    f'{int((got[tile] != got[1]).sum())} elements')


# ---- the pair of products on the 128 x 64 tile
def _pair(L, planes, A, B0, B1, C0, ld0, N0, acc0, C1, ld1, N1, acc1, M):
    rc = L.genrl_gemm_h2_pair(A.ptr(), A.ld, A.plane, A.inv_ptr(), A.ld, B0.ptr(), B0.ld, B0.plane, B0.inv_ptr(), C0.data_ptr(), ld0, N0, acc0,
                              B1.ptr(), B1.ld, B1.plane, B1.inv_ptr(), C1.data_ptr(), ld1, N1, acc1, M, R.stream())
    return rc, names(int(L.genrl_planes_last_route()))


@pytest.mark.parametrize('M,N0,N1,K', [(130, 128, 128, 192), (130, 128, 100, 192), (257, 64, 200, 448)])
def test_pair_on_the_128x64_tile_is_two_gemm_h2(L, M, N0, N1, K):
    from genrl_amd import planes
    g = torch.Generator(device='cuda').manual_seed(M * 1000 + N0 + N1 + K)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
    A = planes.split(rn(M, K) * torch.exp2(torch.randint(-6, 7, (M, 1), device='cuda', generator=g).float()))
    B0, B1 = planes.split(rn(N0, K) * 0.1), planes.split(rn(N1, K) * 3.0)
    G = 4                                               # guard columns behind each C's rows
    ld0, ld1 = N0 + G, (N1 + 3) // 4 * 4 + G
    fill0, fill1 = rn(M, ld0), rn(M, ld1)
    for acc0, acc1 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        r0, r1, p0, p1 = fill0.clone(), fill1.clone(), fill0.clone(), fill1.clone()
        with forced(L, 1):
            planes.gemm(A, B0, r0, ld0, None, M, N0, accumulate=bool(acc0))
            planes.gemm(A, B1, r1, ld1, None, M, N1, accumulate=bool(acc1))
        with forced(L, 4):
            rc, route = _pair(L, planes, A, B0, B1, p0, ld0, N0, acc0, p1, ld1, N1, acc1, M)
        assert rc == 0 and route == ['128x64'], (rc, route)
        assert torch.equal(p0, r0) and torch.equal(p1, r1), (acc0, acc1)
        assert torch.equal(p0[:, N0:], fill0[:, N0:]) and torch.equal(p1[:, N1:], fill1[:, N1:])      # guards untouched
        assert not torch.equal(p0[:, :N0], fill0[:, :N0]) and not torch.equal(p1[:, :N1], fill1[:, :N1])


@pytest.mark.parametrize('force', [0, 4])
def test_pair_is_still_refused_where_it_was(L, force):
    """a first product that is no multiple of 64 columns wide; products genrl_gemm_h2 runs on the two-stage ring (400 tiles, k <= 1536)"""
    from genrl_amd import planes
    for M, N0, N1, K in ((64, 96, 64, 64), (1280, 1280, 1280, 64)):
        A, B0, B1 = planes.Planes(M, K, 'cuda'), planes.Planes(N0, K, 'cuda'), planes.Planes(N1, K, 'cuda')
        for P in (A, B0, B1):
            P.t.zero_(); P.inv.fill_(1.0)
        C0, C1 = torch.zeros(M, N0, device='cuda'), torch.zeros(M, N1, device='cuda')
        C0.fill_(7.0); C1.fill_(7.0)
        with forced(L, force):
            rc, route = _pair(L, planes, A, B0, B1, C0, N0, N0, 0, C1, N1, N1, 0, M)
        torch.cuda.synchronize()
        assert rc == EINVAL and route == [], (M, N0, N1, rc, route)
        assert bool((C0 == 7.0).all()) and bool((C1 == 7.0).all())


# ---- the route at its edges (auto), every result equal to the forced 64 x 64 one
EDGES = [       # (id, M, N, K, route)
    ('1024x3072.K1600', 1024, 3072, 1600, '64x192'),
    ('1024x3072.K1536', 1024, 3072, 1536, '64/ns2'),
    ('960x3072.240-tiles', 960, 3072, 1600, '64x192'),
    ('896x3072.224-tiles', 896, 3072, 1600, '64/ns3'),
]
PAIR_EDGES = [('pair.1024', 1024, '128x64'), ('pair.896', 896, '64/ns3')]


def _edge_operands(M, N, K, seed):
    from genrl_amd import planes
    g = torch.Generator(device='cuda').manual_seed(seed)
    A = planes.split(torch.randn(M, K, device='cuda', generator=g) * torch.exp2(torch.randint(-6, 7, (M, 1), device='cuda', generator=g).float()))
    B = planes.split(torch.randn(N, K, device='cuda', generator=g) * 0.05)
    return planes, A, B


def run_edge(L, M, N, K):
    planes, A, B = _edge_operands(M, N, K, M + N + K)
    out = {}
    for tile in (0, 1):
        C = torch.full((M, N), float('nan'), device='cuda')
        with forced(L, tile):
            planes.gemm(A, B, C, N, None, M, N)
            out[tile] = (C, names(int(L.genrl_planes_last_route())))
    torch.cuda.synchronize()
    return out[0][1], bool(torch.equal(out[0][0], out[1][0])) and bool(torch.isfinite(out[0][0]).all())


def run_pair_edge(L, M):
    planes, A, B0 = _edge_operands(M, 1024, 3072, M)
    B1 = planes.split(torch.randn(1024, 3072, device='cuda', generator=torch.Generator(device='cuda').manual_seed(M + 1)) * 0.02)
    C0 = torch.randn(M, 1024, device='cuda', generator=torch.Generator(device='cuda').manual_seed(M + 2))
    r0, r1, p1 = C0.clone(), torch.full((M, 1024), float('nan'), device='cuda'), torch.full((M, 1024), float('nan'), device='cuda')
    with forced(L, 1):
        planes.gemm(A, B0, r0, 1024, None, M, 1024, accumulate=True)
        planes.gemm(A, B1, r1, 1024, None, M, 1024)
    rc, route = _pair(L, planes, A, B0, B1, C0, 1024, 1024, 1, p1, 1024, 1024, 0, M)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return route, bool(torch.equal(C0, r0)) and bool(torch.equal(p1, r1)) and bool(torch.isfinite(p1).all())


@pytest.mark.parametrize('cid', [e[0] for e in EDGES])
def test_route_edges(L, cid):
    _, M, N, K, want = next(e for e in EDGES if e[0] == cid)
    route, same = run_edge(L, M, N, K)
    assert route == [want], (cid, route)
    assert same, f'{cid}: the routed result differs from the forced 64x64 one'


@pytest.mark.parametrize('cid', [e[0] for e in PAIR_EDGES])
def test_pair_route_edges(L, cid):
    _, M, want = next(e for e in PAIR_EDGES if e[0] == cid)
    route, same = run_pair_edge(L, M)
    assert route == [want], (cid, route)
    assert same, f'{cid}: the pair differs from its two 64x64 launches'


def test_switch_off_keeps_the_64x64_routes():
    """GENRL_PLANES_RECT=0 (read once per process: a child): the products the route takes run where they ran before it"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'out.json')
        env = dict(os.environ, GENRL_PLANES_RECT='0')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, f'exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}'
        with open(out) as f:
            res = json.load(f)
    assert res['1024x3072.K1600'] == [['64/ns3'], True], res
    assert res['pair.1024'] == [['64/ns3'], True], res


if __name__ == '__main__':
    from genrl_amd._lib import lib
    _L = lib()
    _res = {'1024x3072.K1600': run_edge(_L, 1024, 3072, 1600), 'pair.1024': run_pair_edge(_L, 1024)}
    with open(sys.argv[1], 'w') as _f:
        json.dump(_res, _f)
