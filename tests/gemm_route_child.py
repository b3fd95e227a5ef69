"""Route table and child-process runner of test_gpu_gemm_variants.py (not a test module).

`python gemm_route_child.py GROUP OUT.json` runs the cases of one group of ROUTES in a fresh process whose environment the parent
set (GENRL_GEMM_LOG, GENRL_GEMM_TRACE and, per group, GENRL_SKINNY_MAX_M / GENRL_GEMM_FORCE: gemm.hip reads each of them once per
process).  Per case, mode and call it records the largest |kernel - float64| / (2^-24 scale), whether anything outside the output
changed, the launch-log families and fallback-trace lines the call produced, genrl_sgemm_ws_floats and genrl_sgemm_last_pipe.  The
parent asserts on them.

Operands (`operand`) are exact sums x = h + m + l of three bf16-sized terms (8, 8 and 6 significant bits at 2^0, 2^-9 and 2^-18
relative), so the bf16x3 split recovers h, m, l exactly.  The main terms h carry random signs in one operand, so the products
cancel like those of random data and the fp32 accumulation error stays small.  The signs of h in the other operand and of l in
the first follow one rank-1 pattern alpha[row] * gamma[k] (and those of m another one): every h*l cross product (l*h in half the
cases) and every m*m product of one output element then has the same sign, and a dropped or mis-paired low term adds up over K
to ~2^-18 of the scale instead of cancelling.  m takes the opposite sign of h in about half the elements, where rounding to bf16
goes away from zero (a truncation would differ).  Row magnitudes spread over 2^-10 .. 2^10."""
import json
import zlib
import os
import sys
from unittest import mock

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from f64check import U, in_buf, out_buf, untouched  # noqa: E402

MODES = (0, 2, 3, 1)                 # genrl_set_gemm_precision: 0 fp32 MFMA, 2 bf16x3 on the 128 tile, 3 bf16x3 everywhere, 1 bf16
MODE_NAME = {0: 'f32', 1: 'bf16', 2: 'bf16x3-big', 3: 'bf16x3'}
FAMILY = {'skinny': 'f32/skinny', 'tall': 'f32/tall', 'rr64': 'f32/tile64', 'cfg64': 'f32/tile64', 'mid': 'f32/tile64',
          'rr128': 'f32/tile128', 'rect': 'f32/tile128', 'cfg128': 'f32/tile128', 'parts': 'f32/skinny'}
FALLBACK = ('cfg64', 'mid', 'cfg128')


def case(cid, lay, M, N, K, kind, off=(0, 0, 0), pad=(0, 0, 0), kind1=None, split=False, fam=None, fb=None, note=''):
    """one product: layout (A, B each k- or row-contiguous), offsets and line padding (floats) of A, B, C, the route `kind` it must
    take, in mode 1 (bf16 operands bypass the skinny and tall kernels) `kind1`, whether split-K is planned"""
    return dict(id=cid, lay=lay, M=M, N=N, K=K, kind=kind, off=off, pad=pad, kind1=kind1 or kind, split=split, fam=fam, fb=fb,
                note=note)


def conv(cid, which, n, H, W, C, k, other, kind, kind3=None, split=False, note=''):
    """implicit-conv product: which = 1 -> patches (n*oh*ow x k*k*C) times weights (other x k*k*C); which = 2 -> dy^T (other
    channels x pixels) times patches; kind3: the route in mode 3 (the 96-wide tiles stay out of it)"""
    oh, ow = (H - k) // 2 + 1, (W - k) // 2 + 1
    P, KK = n * oh * ow, k * k * C
    M, N, K = (P, other, KK) if which == 1 else (other, KK, P)
    return dict(id=cid, which=which, img=(n, H, W, C, k), M=M, N=N, K=K, kind=kind, kind3=kind3 or kind, kind1=kind, split=split,
                note=note)


# ----------------------------------------------------------------------------------------------------------- the route table
# kind: skinny = skinny_kernel<MB, B_KC> (MB 1: M <= 16, 2: M <= 32 and the 33..128-row "skinny_mid" row groups, 4: only under
# GENRL_SKINNY_MAX_M); tall = sgemm_tall_kernel<NB, KC, B_KC>; rr64 / rr128 = sgemm_rr_kernel<2 / 4, A_KC, B_KC, 0, KX, .., BF>
# (KX: K and the split length whole BK steps); rect = the 96-wide gathered tiles <4, .., G, false, 4, 3> / <4, .., 3, 4>;
# cfg64 / mid / cfg128 = the fallback sgemm_kernel<64,64,64,4,2> / <64,64,16,1,2> / <128,128,16,1,1>.
ROUTES = {
    'skinny': [
        case('skinny.MB1.kk.ragged-K', 'kk', 1, 200, 333, 'skinny', kind1='cfg64', pad=(3, 3, 0)),   # (launch_rr: M >= 4)
        case('skinny.MB1.kr.M16.odd-ldb', 'kr', 16, 1000, 1034, 'skinny', kind1='cfg64', pad=(2, 3, 0)),
        case('skinny.MB2.kk.M17.padded', 'kk', 17, 255, 96, 'skinny', kind1='rr64', pad=(4, 4, 1)),
        case('skinny.MB2.kr.M32.N130', 'kr', 32, 130, 520, 'skinny', kind1='cfg64'),
        case('skinny.mid.kk.M33', 'kk', 33, 1024, 1024, 'skinny', kind1='rr64'),
        case('skinny.mid.kr.M128', 'kr', 128, 1024, 1024, 'skinny', kind1='rr64'),
        case('skinny.mid.kk.64x1536x1024', 'kk', 64, 1536, 1024, 'skinny', kind1='rr64'),
        case('skinny.mid.kr.64x1024x1536', 'kr', 64, 1024, 1536, 'skinny', kind1='rr64'),
        case('skinny.unaligned-A', 'kk', 20, 77, 101, 'skinny', off=(1, 0, 0), kind1='cfg64', fb=True),
        case('skinny.kr.unaligned-B-C', 'kr', 5, 64, 64, 'skinny', off=(0, 1, 3), kind1='cfg64'),
        # just past the skinny limits: tiles, split-K planned
        case('skinny-edge.M129', 'kk', 129, 1024, 1024, 'rr64', split=True),
        case('skinny-edge.M65.N1536', 'kk', 65, 1536, 1024, 'rr64', split=True),
        case('skinny-edge.M64.N1536.K1536', 'kr', 64, 1536, 1536, 'rr64', split=True),
        case('skinny-edge.N1025', 'kk', 100, 1025, 1024, 'rr64', split=True),
        case('skinny-edge.K1025', 'kk', 100, 1024, 1025, 'rr64', split=True, pad=(3, 3, 0)),
        case('skinny-edge.rk.M16', 'rk', 16, 300, 64, 'rr64'),
    ],
    'tall': [
        case('tall.3x3.kk', 'kk', 16384, 48, 48, 'tall', kind1='rr64'),
        case('tall.7x3.kr.N49', 'kr', 16384, 49, 48, 'tall', kind1='cfg64', pad=(0, 0, 3)),
        case('tall.7x3.kk.N112', 'kk', 16400, 112, 48, 'tall', kind1='rr64'),
        case('tall.3x7.kk.K112', 'kk', 16384, 48, 112, 'tall', kind1='rr64'),
        case('tall.3x7.kr.K100', 'kr', 16390, 40, 100, 'tall', kind1='rr64', pad=(4, 0, 4)),
        case('tall.7x6.kr.N113', 'kr', 16384, 113, 48, 'tall', kind1='cfg64', pad=(0, 0, 3)),
        case('tall.7x6.kr.N200.slabs2', 'kr', 20000, 200, 96, 'tall', kind1='rr64'),
        case('tall.7x6.kr.N240.slabs3', 'kr', 16384, 240, 96, 'tall', kind1='rr64'),
        case('tall-edge.kk.N113', 'kk', 16384, 113, 48, 'rr64'),
        case('tall-edge.K116', 'kk', 16384, 48, 116, 'rr64'),
        case('tall-edge.M16383', 'kk', 16383, 48, 48, 'rr64'),
        case('tall-edge.K50', 'kk', 16384, 48, 50, 'rr64', pad=(2, 2, 0)),
        case('tall-edge.kr.N100.K100', 'kr', 16384, 100, 100, 'rr64'),
        case('tall-edge.unaligned-C', 'kk', 16384, 48, 48, 'rr64', off=(0, 0, 1)),
    ],
    'tile': [
        case('rr64.kk.KX', 'kk', 300, 200, 256, 'rr64'),
        case('rr64.kk.K250', 'kk', 300, 200, 250, 'rr64', pad=(2, 2, 0)),
        case('rr64.kr.KX', 'kr', 257, 130, 128, 'rr64', pad=(0, 2, 0)),
        case('rr64.rk.K96', 'rk', 130, 257, 96, 'rr64', pad=(2, 0, 0)),
        case('rr64.rr.padded255', 'rr', 255, 255, 200, 'rr64', pad=(1, 1, 1)),
        case('rr64.kk.odd-ldc', 'kk', 1024, 255, 512, 'rr64', pad=(0, 0, 2)),
        case('rr64.kk.c_off1', 'kk', 200, 100, 64, 'rr64', off=(0, 0, 1)),
        case('rr64.kr.c_off3', 'kr', 200, 100, 100, 'rr64', off=(0, 0, 3)),
        case('rr64.rk.4x4x4', 'rk', 4, 4, 4, 'rr64'),
        case('rr64.kk.511-big-tiles', 'kk', 65408, 128, 96, 'rr64'),
        case('rr128.kk.512-tiles.KX', 'kk', 65536, 128, 96, 'rr128'),
        case('rr128.kr.K40', 'kr', 2048, 4096, 40, 'rr128'),
        case('rr128.rk.KX', 'rk', 4096, 2048, 64, 'rr128'),
        case('rr128.rr.ragged', 'rr', 4100, 2050, 36, 'rr128', pad=(0, 2, 2)),
        case('rr128.kk.c_off2', 'kk', 2048, 4096, 40, 'rr128', off=(0, 0, 2)),
        case('tail-split.17408x1024x1024', 'kk', 17408, 1024, 1024, 'rr128', fam=('f32/tile128', 'f32/tile64')),
    ],
    'split': [
        case('split.small.kk.KX', 'kk', 256, 256, 4096, 'rr64', split=True),
        case('split.small.kr.K5000', 'kr', 200, 136, 5000, 'rr64', split=True),
        case('split.small.rk.N70', 'rk', 130, 70, 1034, 'rr64', split=True, pad=(2, 2, 2)),
        case('split.big.kk.KX', 'kk', 96, 1728, 20000, 'rr128', split=True),
        case('split.big.rr.ragged', 'rr', 100, 1700, 20010, 'rr128', split=True),
    ],
    'fallback': [
        case('cfg128.kk.unaligned-A', 'kk', 2048, 4096, 40, 'cfg128', off=(1, 0, 0)),
        case('cfg128.kk.odd-lda', 'kk', 2048, 4096, 40, 'cfg128', pad=(1, 0, 0)),
        case('cfg128.rr.unaligned-B.ragged', 'rr', 4100, 2050, 36, 'cfg128', off=(0, 2, 0)),
        case('cfg128.kr.split', 'kr', 96, 1728, 20000, 'cfg128', off=(0, 1, 0), split=True),
        case('mid.kk.512-tiles', 'kk', 512, 4096, 40, 'mid', off=(1, 0, 0)),
        case('mid-edge.kk.511-tiles', 'kk', 448, 4672, 40, 'cfg64', off=(1, 0, 0)),
        case('cfg64.kr.unaligned-B', 'kr', 300, 200, 100, 'cfg64', off=(0, 1, 0)),
        case('cfg64.rk.unpadded-M37', 'rk', 37, 53, 29, 'cfg64'),
        case('cfg64.rr.odd-ld', 'rr', 130, 70, 50, 'cfg64', pad=(1, 3, 1)),
        case('cfg64.kk.split', 'kk', 200, 136, 5000, 'cfg64', off=(3, 0, 1), split=True),
    ],
    'conv': [
        conv('conv1.rect.N96', 1, 4, 258, 258, 4, 4, 96, 'rect', kind3='rr128'),
        conv('conv1.rect.N192', 1, 4, 258, 258, 4, 4, 192, 'rect', kind3='rr128'),
        conv('conv1.rect.N92', 1, 4, 258, 258, 4, 4, 92, 'rect', kind3='rr128'),
        conv('conv1.square.N128', 1, 4, 258, 258, 4, 4, 128, 'rr128', note='96-wide rule rejects N = 128'),
        conv('conv1.tile64.N48', 1, 2, 34, 34, 8, 4, 48, 'rr64'),
        conv('conv1.tile64.C6', 1, 2, 34, 34, 6, 4, 48, 'rr64', note='C % 4 != 0 with every gathered vector 16-byte aligned'),
        conv('conv2.rect.M96', 2, 1, 18, 18, 4096, 4, 96, 'rect', kind3='rr128'),
        conv('conv2.rect.M192', 2, 1, 18, 18, 2048, 4, 192, 'rect', kind3='rr128'),
        conv('conv2.rect.M92.split', 2, 8, 102, 102, 108, 4, 92, 'rect', kind3='rr128', split=True),
        conv('conv2.square.M128', 2, 1, 18, 18, 4096, 4, 128, 'rr128', note='96-wide rule rejects M = 128'),
        conv('conv2.tile64.M48', 2, 2, 34, 34, 8, 4, 48, 'rr64'),
    ],
    # environment switches (one child each)
    'skinny256': [
        case('skinny4.kk.256x2048', 'kk', 256, 2048, 300, 'skinny', kind1='rr64', note='skinny_kernel<4, true>'),
        case('skinny4.kr.100x4096', 'kr', 100, 4096, 64, 'skinny', kind1='rr64', note='skinny_kernel<4, false>'),
        case('skinny4.g32.kk.200x1024', 'kk', 200, 1024, 200, 'skinny', kind1='rr64', note='skinny_kernel<2, true>, 7 row groups'),
        case('skinny4-edge.M257', 'kk', 257, 1024, 1024, 'rr64', split=True),
    ],
    'force_s': [
        case('force-s7.rr64.kk', 'kk', 300, 200, 1000, 'rr64', split=True),
        case('force-s7.cfg64.kr', 'kr', 300, 200, 1000, 'cfg64', off=(0, 1, 0), split=True),
    ],
    'force_b': [
        case('force-b10.rr128.kk.empty-split', 'kk', 200, 300, 1100, 'rr128', split=True, note='split 9 starts at k = 1152'),
        case('force-b10.rr128.kr.KX.empty-splits', 'kr', 200, 300, 1024, 'rr128', split=True, note='splits 8, 9 start at 1024, 1152'),
        case('force-b10.cfg128.kk', 'kk', 200, 300, 1100, 'cfg128', off=(1, 0, 0), split=True),
    ],
    'force_m': [
        case('force-m3.mid.kk', 'kk', 300, 200, 600, 'mid', off=(1, 0, 0), split=True),
        case('force-m3.rr64.kk', 'kk', 300, 200, 600, 'rr64', split=True),
    ],
}
GROUP_ENV = {'skinny256': {'GENRL_SKINNY_MAX_M': '256'}, 'force_s': {'GENRL_GEMM_FORCE': 's,7'},
             'force_b': {'GENRL_GEMM_FORCE': 'b,10'}, 'force_m': {'GENRL_GEMM_FORCE': 'm,3'}}
GROUPS = list(ROUTES) + ['parts', 'refuse']
SWITCHES = ('GENRL_GEMM_LOG', 'GENRL_GEMM_TRACE', 'GENRL_SKINNY_MAX_M', 'GENRL_GEMM_FORCE', 'GENRL_GEMM_MODE')

# genrl_sgemm_skinny_parts: (nparts, M, N, K, B layout, part_stride extra floats, A offset)
PARTS = [(1, 1, 100, 1000, 'kc', 0, 0), (2, 16, 64, 520, 'rc', 37, 0), (7, 17, 130, 1034, 'kc', 4, 0), (64, 32, 100, 1000, 'rc', 5, 0),
         (7, 1, 33, 96, 'rc', 1, 0), (64, 16, 48, 2000, 'kc', 0, 0), (2, 32, 1024, 64, 'kc', 100, 1), (1, 17, 17, 5, 'rc', 3, 0)]


def expect(c, mode, group):
    """-> (route kind, log families, fallback trace expected, split expected, pipe) of case c in `mode`"""
    kind = c['kind1'] if mode == 1 else (c.get('kind3', c['kind']) if mode == 3 else c['kind'])
    fam = tuple(c['fam']) if c.get('fam') else (FAMILY[kind],)
    fb = kind in FALLBACK or bool(c.get('fb'))
    pipe = {'rr64': (0, 1, 0, 3), 'rr128': (0, 1, 3, 3), 'rect': (0, 1, 0, 3)}.get(kind, (0, 0, 0, 0))[mode]
    split = c['split']
    if mode == 1 and c['kind'] in ('skinny', 'tall'):
        split = c['M'] <= 128 and c['K'] >= 1024      # the tiles plan split-K for these few-row products with long K
    return kind, fam, fb, split, pipe


def key_of(kind, pipe, mode, split, group):
    """K table key: route family . arithmetic"""
    fam = {'rr64': 'tile', 'rr128': 'tile', 'rect': 'tile', 'cfg64': 'fallback', 'mid': 'fallback', 'cfg128': 'fallback'}.get(kind, kind)
    if group == 'conv':
        fam = 'conv'
    if split and fam in ('tile', 'fallback'):
        fam = 'split'
    arith = 'bf16' if mode == 1 else ('x3' if pipe == 3 else 'f32')
    return f'{fam}.{arith}'


# ----------------------------------------------------------------------------------------------------------- operands
def _signs(g, n):
    return torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)


def operand(rows, K, g, pat, rank1, rexp=10):
    """fp32 [rows, K] = h + m + l exactly (see the module docstring); pat = (gamma, gamma_m): the shared k sign patterns.  rank1
    'h': the signs of h follow alpha[row] * gamma[k] and those of l are random; 'l': the other way round; None: all random."""
    e = torch.randint(-2, 3, (rows, K), generator=g).double() + torch.randint(-rexp, rexp + 1, (rows, 1), generator=g).double()
    h = torch.randint(129, 256, (rows, K), generator=g).double() * torch.exp2(e - 7)
    m = torch.randint(129, 256, (rows, K), generator=g).double() * torch.exp2(e - 16)
    lo = torch.randint(33, 64, (rows, K), generator=g).double() * torch.exp2(e - 23)
    r1 = _signs(g, rows)[:, None] * pat[0][None, :K] if rank1 else None
    rnd = torch.where(torch.rand(rows, K, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    sh, sl = (r1, rnd) if rank1 == 'h' else ((rnd, r1) if rank1 == 'l' else (rnd, -rnd))
    sm = _signs(g, rows)[:, None] * pat[1][None, :K] if rank1 else -rnd
    x = sh * h + sl * lo + sm * m
    x32 = x.float()
    assert torch.equal(x32.double(), x)
    return x32


def bf16_rne(x):
    """fp32 -> nearest-even bf16 -> fp32, as the kernels round (finite inputs)"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000)
    return r.to(torch.int64).where(r < 2 ** 31, r - 2 ** 32).to(torch.int32).view(torch.float32)


def place(src, ld, off):
    """src (CPU fp32 [rows, cols]) in a NaN-padded device buffer at `off`; -> the whole buffer (the view's base)"""
    return in_buf(src, ld, off)._base


# ----------------------------------------------------------------------------------------------------------- the child
class Probe:
    """launch-log lines and fallback-trace lines produced since the last call"""

    def __init__(self):
        self.trace_path = os.environ['GENRL_TRACE_FILE']
        fd = os.open(self.trace_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(fd, 2)                                            # C stderr -> file (unbuffered fprintf)
        os.close(fd)
        self.tpos = 0
        self.lpos = 0

    def take(self):
        lines = []
        if os.path.exists(os.environ['GENRL_GEMM_LOG']):
            with open(os.environ['GENRL_GEMM_LOG']) as f:
                f.seek(self.lpos)
                txt = f.read()
                self.lpos = f.tell()
            lines = [ln.split()[0] for ln in txt.splitlines() if ln.strip()]
        with open(self.trace_path) as f:
            f.seek(self.tpos)
            txt = f.read()
            self.tpos = f.tell()
        trace = [ln for ln in txt.splitlines() if ln.startswith('[genrl gemm fallback]')]
        return lines, trace


def ratio_of(got, ref, scale):
    err = (got.detach().cpu().double() - ref).abs()
    r = err / (U * scale).clamp_min(1e-300)
    return float(torch.nan_to_num(r, nan=float('inf')).max()) if r.numel() else 0.0


def nan_empty_patch():
    """ops.sgemm* allocate the split-K workspace with torch.empty: hand them NaN-filled memory, so that a split that writes
    nothing (or a reduce that reads past the written slices) shows"""
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_floating_point():
            t.fill_(float('nan'))
        return t
    return mock.patch.object(torch, 'empty', nan_empty)


def run_sgemm_case(c, group, ops, L, probe):
    g = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    M, N, K, lay = c['M'], c['N'], c['K'], c['lay']
    pat = (_signs(g, K), _signs(g, K))
    ra, rb = ('h', 'l') if zlib.crc32(c['id'].encode()) & 1 else ('l', 'h')
    A, B = operand(M, K, g, pat, ra), operand(N, K, g, pat, rb)
    bias = torch.randn(N, generator=g) * 2.0 ** torch.randint(-4, 5, (N,), generator=g)
    a_off, b_off, c_off = c['off']
    pa, pb, pc = c['pad']
    a_kc, b_kc = lay[0] == 'k', lay[1] == 'k'
    lda = (K if a_kc else M) + pa
    ldb = (K if b_kc else N) + pb
    ldc = N + pc
    a = place(A if a_kc else A.T.contiguous(), lda, a_off)
    b = place(B if b_kc else B.T.contiguous(), ldb, b_off)
    a_rs, a_ks = (lda, 1) if a_kc else (1, lda)
    b_rs, b_ks = (ldb, 1) if b_kc else (1, ldb)
    refs = {}
    out = {}
    for mode in MODES:
        Ar, Br = (bf16_rne(A), bf16_rne(B)) if mode == 1 else (A, B)
        arith = 1 if mode == 1 else 0
        if arith not in refs:
            A64, B64 = Ar.double(), Br.double()
            refs[arith] = (A64 @ B64.T, A64.abs() @ B64.abs().T)
        ref, scale = refs[arith]
        C0 = torch.randn(M, N, generator=g) * ref.abs().float().clamp_min(1e-30) * 0.5
        prev = ops.set_gemm_precision(MODE_NAME[mode])
        try:
            res = []
            for acc in (False, True):
                cbuf, cview = out_buf(M, N, ldc, c_off)
                if acc:
                    cview.copy_(C0)
                with nan_empty_patch():
                    ops.sgemm(a, a_rs, a_ks, b, b_rs, b_ks, cbuf, ldc, bias.cuda() if acc else None, M, N, K,
                              accumulate=acc, a_off=a_off, b_off=b_off, c_off=c_off)
                pipe = int(L.genrl_sgemm_last_pipe())
                torch.cuda.synchronize()
                r_ref = ref + (bias.double()[None, :] + C0.double() if acc else 0.0)
                r_sc = scale + (bias.double().abs()[None, :] + C0.double().abs() if acc else 0.0)
                res.append(record(cview, r_ref, r_sc, cbuf, probe, pipe, int(L.genrl_sgemm_ws_floats(M, N, K))))
                del cbuf, cview
        finally:
            ops.set_gemm_precision(prev)
        out[mode] = res
    return out


def record(cview, ref, scale, cbuf, probe, pipe, ws):
    fams, trace = probe.take()
    try:
        untouched('C', cbuf, cview)
        tmsg = ''
    except AssertionError as e:
        tmsg = str(e)
    return dict(ratio=ratio_of(cview, ref, scale), untouched=tmsg, fams=fams, trace=trace, pipe=pipe, ws=ws)


def patches64(img64, n, H, W, C, k):
    oh, ow = (H - k) // 2 + 1, (W - k) // 2 + 1
    v = img64.as_strided((n, oh, ow, k, k, C), (H * W * C, 2 * W * C, 2 * C, W * C, C, 1))
    return v.reshape(n * oh * ow, k * k * C)        # columns in (kh, kw, c) order


def run_conv_case(c, group, ops, L, probe):
    g = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    n, H, W, C, k = c['img']
    M, N, K, which = c['M'], c['N'], c['K'], c['which']
    pix = n * ((H - k) // 2 + 1) * ((W - k) // 2 + 1)
    KK = k * k * C
    img = operand(n * H * W, C, g, None, None, rexp=3)
    other = N if which == 1 else M
    Wt = operand(other, KK if which == 1 else pix, g, None, None)
    ximg = in_buf(img, C)                                    # NHWC image, NaN past its end
    if which == 1:
        args = (ximg, KK, 1, in_buf(Wt, KK), KK, 1)          # patches [pixels][K] times weights [Co][K]
    else:
        args = (in_buf(Wt.T.contiguous(), M), 1, M, ximg, 1, KK)     # dy [pixels][Co] (row-contiguous A) times patches

    def conv_ref(im, w):
        P, Wd = patches64(im.double().reshape(-1), n, H, W, C, k), w.double()
        if which == 1:
            return P @ Wd.T, P.abs() @ Wd.abs().T
        return Wd @ P, Wd.abs() @ P.abs()                   # C[co, kk] = sum_p dy[p, co] patches[p, kk]
    bias = torch.randn(N, generator=g)
    refs = {}
    out = {}
    for mode in MODES:
        arith = 1 if mode == 1 else 0
        if arith not in refs:
            refs[arith] = conv_ref(bf16_rne(img), bf16_rne(Wt)) if mode == 1 else conv_ref(img, Wt)
        ref, scale = refs[arith]
        C0 = torch.randn(M, N, generator=g) * ref.abs().float().clamp_min(1e-30) * 0.5
        prev = ops.set_gemm_precision(MODE_NAME[mode])
        try:
            res = []
            for acc in (False, True):
                cbuf, cview = out_buf(M, N, N)
                if acc:
                    cview.copy_(C0)
                with nan_empty_patch():
                    ops.sgemm_conv(*args, cview, N, bias.cuda() if acc else None, M, N, K, which, (H, W, C, k), accumulate=acc)
                pipe = int(L.genrl_sgemm_last_pipe())
                torch.cuda.synchronize()
                r_ref = ref + (bias.double()[None, :] + C0.double() if acc else 0.0)
                r_sc = scale + (bias.double().abs()[None, :] + C0.double().abs() if acc else 0.0)
                res.append(record(cview, r_ref, r_sc, cbuf, probe, pipe, int(L.genrl_sgemm_ws_floats(M, N, K))))
        finally:
            ops.set_gemm_precision(prev)
        out[mode] = res
    return out


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_parts(L, probe):
    out = {}
    for (nparts, M, N, K, blay, extra, aoff) in PARTS:
        cid = f'parts.n{nparts}.M{M}.N{N}.K{K}.{blay}' + (f'.a_off{aoff}' if aoff else '')
        g = torch.Generator().manual_seed(nparts * 1000 + M * 10 + N)
        pat = (_signs(g, K), _signs(g, K))
        A, B = operand(M, K, g, pat, 'h'), operand(N, K, g, pat, 'l')
        a = in_buf(A, K, aoff)
        if blay == 'kc':
            b, b_rs, b_ks = in_buf(B, K), K, 1
        else:
            b, b_rs, b_ks = in_buf(B.T.contiguous(), N), 1, N
        ldp = N + 3
        stride = M * ldp + extra
        buf = torch.full((nparts * stride + ldp + 4,), -1.2345678e33, device='cuda')
        views = [buf[s * stride:s * stride + M * ldp].view(M, ldp)[:, :N] for s in range(nparts)]
        for v in views:
            v.fill_(float('nan'))
        rc = int(L.genrl_sgemm_skinny_parts(a.data_ptr(), K, b.data_ptr(), b_rs, b_ks, buf.data_ptr(), ldp, stride, M, N, K, nparts,
                                            stream()))
        torch.cuda.synchronize()
        fams, trace = probe.take()
        total = sum(v.detach().cpu().double() for v in views)
        A64, B64 = A.double(), B.double()
        mask = torch.ones_like(buf, dtype=torch.bool)
        for v in views:
            off = v.storage_offset()
            idx = off + torch.arange(M, device='cuda')[:, None] * ldp + torch.arange(N, device='cuda')[None, :]
            mask[idx.reshape(-1)] = False
        rest = buf[mask]
        ok = bool(torch.equal(rest, torch.full_like(rest, -1.2345678e33)))
        out[cid] = dict(rc=rc, ratio=ratio_of(total, A64 @ B64.T, A64.abs() @ B64.abs().T), untouched='' if ok else 'wrote between parts',
                        fams=fams, trace=trace, pipe=int(L.genrl_sgemm_last_pipe()))
    return out


def run_refusals(L, probe):
    """every call must return its code and write nothing"""
    EINVAL = 1
    out = {}
    A = torch.randn(64 * 64 + 8, device='cuda')
    img = torch.randn(2 * 18 * 18 * 8 + 8, device='cuda')
    wt = torch.randn(64 * 128 + 8, device='cuda')
    s = stream()
    sg = lambda a, a_rs, a_ks, b, b_rs, b_ks, c, M, N, K: int(L.genrl_sgemm(a, a_rs, a_ks, b, b_rs, b_ks, c, 64, None, M, N, K, 0, None, 0, s))
    sc = lambda a, a_rs, a_ks, b, b_rs, b_ks, c, M, N, K, which, H, W, C, k: int(L.genrl_sgemm_conv(
        a, a_rs, a_ks, b, b_rs, b_ks, c, 64, None, M, N, K, 0, None, 0, which, H, W, C, k, s))
    ap, ip, wp = A.data_ptr(), img.data_ptr(), wt.data_ptr()
    # sgemm_conv which = 1: 2 images 18 x 18 x 8, k = 4 -> 128 pixels x 128; which = 2 likewise
    calls = {
        'sgemm.K0': (EINVAL, lambda c: sg(ap, 64, 1, ap, 64, 1, c, 16, 16, 0)),
        'sgemm.K-1': (EINVAL, lambda c: sg(ap, 64, 1, ap, 64, 1, c, 16, 16, -1)),
        'sgemm.A-no-unit-stride': (EINVAL, lambda c: sg(ap, 64, 2, ap, 64, 1, c, 16, 16, 16)),
        'sgemm.B-no-unit-stride': (EINVAL, lambda c: sg(ap, 64, 1, ap, 3, 64, c, 16, 16, 16)),
        'sgemm.M0': (0, lambda c: sg(ap, 64, 1, ap, 64, 1, c, 0, 16, 16)),
        'sgemm.N0': (0, lambda c: sg(ap, 64, 1, ap, 64, 1, c, 16, 0, 16)),
        'sgemm.M-3': (0, lambda c: sg(ap, 64, 1, ap, 64, 1, c, -3, 16, 16)),
        'conv1.img_c-5': (EINVAL, lambda c: sc(ip, 80, 1, wp, 80, 1, c, 128, 64, 80, 1, 18, 18, 5, 4)),
        'conv1.img_c-3': (EINVAL, lambda c: sc(ip, 48, 1, wp, 48, 1, c, 128, 64, 48, 1, 18, 18, 3, 4)),
        'conv2.img_c-3': (EINVAL, lambda c: sc(wp, 1, 64, ip, 1, 48, c, 64, 48, 128, 2, 18, 18, 3, 4)),
        'conv1.unaligned-image': (EINVAL, lambda c: sc(ip + 4, 128, 1, wp, 128, 1, c, 128, 64, 128, 1, 18, 18, 8, 4)),
        'conv2.unaligned-image': (EINVAL, lambda c: sc(wp, 1, 64, ip + 8, 1, 128, c, 64, 128, 128, 2, 18, 18, 8, 4)),
        'conv1.unaligned-weights': (EINVAL, lambda c: sc(ip, 128, 1, wp + 4, 128, 1, c, 128, 64, 128, 1, 18, 18, 8, 4)),
        'conv1.kk-mismatch': (EINVAL, lambda c: sc(ip, 128, 1, wp, 128, 1, c, 128, 64, 124, 1, 18, 18, 8, 4)),
        'conv1.pixels-not-whole-images': (EINVAL, lambda c: sc(ip, 128, 1, wp, 128, 1, c, 100, 64, 128, 1, 18, 18, 8, 4)),
        'conv2.kk-mismatch': (EINVAL, lambda c: sc(wp, 1, 64, ip, 1, 128, c, 64, 132, 128, 2, 18, 18, 8, 4)),
        'conv2.pixels-not-whole-images': (EINVAL, lambda c: sc(wp, 1, 64, ip, 1, 128, c, 64, 128, 120, 2, 18, 18, 8, 4)),
        'conv.which3': (EINVAL, lambda c: sc(ip, 128, 1, wp, 128, 1, c, 128, 64, 128, 3, 18, 18, 8, 4)),
        'conv.k-larger-than-image': (EINVAL, lambda c: sc(ip, 128, 1, wp, 128, 1, c, 128, 64, 128, 1, 3, 18, 8, 4)),
        'parts.nparts0': (EINVAL, lambda c: int(L.genrl_sgemm_skinny_parts(ap, 64, ap, 64, 1, c, 64, 64 * 16, 16, 16, 64, 0, s))),
        'parts.nparts65': (EINVAL, lambda c: int(L.genrl_sgemm_skinny_parts(ap, 64, ap, 64, 1, c, 64, 64, 1, 16, 64, 65, s))),
        'parts.M33': (EINVAL, lambda c: int(L.genrl_sgemm_skinny_parts(ap, 64, ap, 64, 1, c, 64, 64 * 33, 33, 16, 64, 2, s))),
        'parts.K0': (EINVAL, lambda c: int(L.genrl_sgemm_skinny_parts(ap, 64, ap, 64, 1, c, 64, 64 * 16, 16, 16, 0, 2, s))),
        'parts.B-no-unit-stride': (EINVAL, lambda c: int(L.genrl_sgemm_skinny_parts(ap, 64, ap, 64, 2, c, 64, 64 * 16, 16, 16, 16, 2, s))),
    }
    for cid, (want, fn) in calls.items():
        buf = torch.full((64 * 200 + 4,), -1.2345678e33, device='cuda')
        rc = fn(buf.data_ptr())
        torch.cuda.synchronize()
        fams, trace = probe.take()
        ok = bool((buf == -1.2345678e33).all())
        out[cid] = dict(rc=rc, want=want, untouched='' if ok else 'wrote to C', fams=fams, trace=trace)
    return out


def main(group, path):
    from genrl_amd import ops
    from genrl_amd._lib import lib
    L = lib()
    probe = Probe()
    res = {}
    if group == 'parts':
        res = run_parts(L, probe)
    elif group == 'refuse':
        res = run_refusals(L, probe)
    else:
        for c in ROUTES[group]:
            run = run_conv_case if 'which' in c else run_sgemm_case
            res[c['id']] = {str(m): v for m, v in run(c, group, ops, L, probe).items()}
    with open(path, 'w') as f:
        json.dump(res, f)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
