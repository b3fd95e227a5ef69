"""The autograd nodes of the dense layer on [x1, x2] -- ops.dense_ln_act / dense_act / gru_step on fp32 operands, ops_planes.dense_ln_act /
dense_ln_trunk / dense_act on plane operands -- pinned bit for bit, and GEMM launch for GEMM launch, against the revision BEFORE their
products were defined once (tests/golden/dense_nodes.json: SHA-256 of the output's, its planes' and every gradient's bytes, and the
(M, N, K, tag) of every GEMM launch of one forward + backward in launch order, recorded once on that revision with this file).  The shapes
are the smallest that reach every branch of the shared code under the suite's GENRL_PLANES_MIN_ROWS=0 / GENRL_TN_MIN_ROWS=64."""
import hashlib
import json
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def digest(t):
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class Book:
    """the entries of tests/golden/<name>: check(key, got) asserts that `got` (a dict of digests / lists) is the stored entry.
    GENRL_RECORD_GOLDEN=<directory> (on the revision whose values are the reference, never on the code under test): check() stores
    instead and save() writes <directory>/<name>"""
    def __init__(self, name):
        self.name, self.rec_dir = name, os.environ.get('GENRL_RECORD_GOLDEN')
        self.data = {} if self.rec_dir else json.load(open(os.path.join(GOLDEN_DIR, name)))

    def check(self, key, got):
        got = json.loads(json.dumps(got))             # (tuples become lists, as in the stored entry)
        if self.rec_dir:
            self.data[key] = got
            return
        want = self.data[key]
        assert set(got) == set(want), key
        for n in got:
            assert got[n] == want[n], (key, n, got[n], want[n])

    def save(self):
        if self.rec_dir:
            with open(os.path.join(self.rec_dir, self.name), 'w') as f:
                f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(self.data.items())) + '\n}\n')


@pytest.fixture(scope='module')
def book():
    b = Book('dense_nodes.json')
    yield b
    b.save()


MODES = ['all', 'frozen', 'x1_nograd', 'optimizer']       # which leaves want a gradient; 'optimizer': all, through Optimizer.__call__


def run_case(node, M, N, K1, K2, have, mode, key):
    """one forward + backward of `node` over M rows: x1 (M, K1), x2 (M, K2) or None, width N.  have: 'both' | 'first' | 'none' of the
    inputs come with the caller's planes (plane nodes).  -> the entry of the golden file"""
    from genrl_amd import ops, ops_planes, planes
    g = torch.Generator(device='cuda').manual_seed(zlib.crc32(key.encode()))
    rn = lambda *s, sc=1.0, off=0.0: off + torch.randn(*s, device='cuda', generator=g) * sc
    par = lambda *s, **kw: torch.nn.Parameter(rn(*s, **kw), requires_grad=mode != 'frozen')
    x1 = rn(M, K1).requires_grad_(mode != 'x1_nograd')
    x2 = rn(M, K2).requires_grad_(True) if K2 else None
    dense = lambda n, k: (par(n, k, sc=k ** -0.5), par(n, sc=0.1), par(n, sc=0.1, off=1.0), par(n, sc=0.1))
    names = ('W', 'b', 'gamma', 'beta')
    if node == 'f32.gru_step':
        assert K2 == N
        W, gamma, beta = par(3 * N, K1 + K2, sc=(K1 + K2) ** -0.5), par(3 * N, sc=0.1, off=1.0), par(3 * N, sc=0.1)
        params = {'W': W, 'gamma': gamma, 'beta': beta}
        fn = lambda: ops.gru_step(x1, x2, W, gamma, beta)
    elif node.endswith('dense_ln_trunk'):
        layers = [dense(N, K1 + K2), dense(N, N)]
        params = {f'l{l}.{n}': t for l, lay in enumerate(layers) for n, t in zip(names, lay)}
    else:
        lay = dense(N, K1 + K2)
        params = dict(zip(names, lay)) if 'ln' in node else {'W': lay[0]}
    hp = None
    if node.startswith('planes.') and have != 'none':
        hp = ((planes.split(x1.detach()), 0), (planes.split(x2.detach()), 0) if (K2 and have == 'both') else None)
    if node == 'f32.dense_ln_act':
        fn = lambda: ops.dense_ln_act(x1, x2, *lay, 1e-3)
    elif node == 'f32.dense_act':
        fn = lambda: ops.dense_act(x1, x2, lay[0])
    elif node == 'planes.dense_ln_act':
        fn = lambda: ops_planes.dense_ln_act(x1, x2, *lay, 1e-3, planes=hp)
    elif node == 'planes.dense_ln_trunk':
        fn = lambda: ops_planes.dense_ln_trunk(x1, x2, [l + (1e-3,) for l in layers], planes=hp)
    elif node == 'planes.dense_act':
        fn = lambda: ops_planes.dense_act(x1, x2, lay[0], planes=hp)
    got = {}
    prof = []
    ops.gemm_profile = planes.gemm_profile = prof         # (ONE list: the launches of both operand kinds in their common order)
    try:
        y = fn()
        wgt = rn(*y.shape)
        loss = (y * wgt).sum()
        if mode == 'optimizer':
            from genrl_amd.agent.dreamer_utils import Optimizer
            plist = list(params.values())
            met = Optimizer('dense', plist, lr=1e-2, eps=1e-4, clip=100.0, wd=1e-2)(loss, plist)
            got['grad_norm'] = digest(met['dense_grad_norm'])
        else:
            loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.gemm_profile = planes.gemm_profile = None
    got['gemms'] = [[m, n, k, tag] for m, n, k, _, _, tag in prof]
    got['y'] = digest(y)
    yp = getattr(y, '_planes', None)
    if node.startswith('planes.'):
        assert yp is not None and yp[1] == 0 and (yp[0].rows, yp[0].cols) == (M, N)
        got['y.planes.t'], got['y.planes.inv'] = digest(yp[0].t), digest(yp[0].inv)
    got['d.x1'] = digest(x1.grad)
    if x2 is not None:
        got['d.x2'] = digest(x2.grad)
    for n, p in params.items():
        # (the Adam pass clears the flat gradient buffer: after the step the parameters carry the gradients' bits)
        got[('p.' if mode == 'optimizer' else 'd.') + n] = digest(p.data if mode == 'optimizer' else p.grad)
    return got


def _check_which_gradients(got, mode, x1_grad):
    """what holds whatever the golden file says: a gradient exists exactly where one was asked for"""
    assert got['y'] is not None and got['gemms']
    assert (got['d.x1'] is not None) == x1_grad
    for n, v in got.items():
        if n.startswith('d.') and n != 'd.x1':
            assert (v is not None) == (mode != 'frozen' or n == 'd.x2'), n
        if n.startswith('p.'):
            assert v is not None


# fp32 operands: one input; two; K % 4 != 0 above 32 rows (ops._aligned_block's compact copy) and at 32 (no copy)
F32_SHAPES = [(64, 64, 0), (64, 64, 32), (64, 64, 10), (32, 64, 10)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('M,K1,K2', F32_SHAPES)
@pytest.mark.parametrize('node', ['f32.dense_ln_act', 'f32.dense_act'])
def test_fp32_dense_nodes_keep_the_parent_bits_and_launches(book, node, M, K1, K2, mode):
    key = f'{node}.M{M}.N128.K{K1}+{K2}.{mode}'
    got = run_case(node, M, 128, K1, K2, 'none', mode, key)
    _check_which_gradients(got, mode, mode != 'x1_nograd')
    book.check(key, got)


@pytest.mark.parametrize('mode', MODES)
def test_fp32_gru_step_keeps_the_parent_bits_and_launches(book, mode):
    key = f'f32.gru_step.R64.I64.D64.{mode}'
    got = run_case('f32.gru_step', 64, 64, 64, 64, 'none', mode, key)
    _check_which_gradients(got, mode, mode != 'x1_nograd')
    book.check(key, got)


# plane operands.  M: 128 = weight gradient on genrl_gemm_h2_tn, 32 = below GENRL_TN_MIN_ROWS (fp32-operand weight gradient, fp32 dpre
# kept).  N: 256 = the LayerNorm backward writes fp32; 320 = fused product + LayerNorm, planes-only backward; 328 = N % 64 != 0, unfused
# product, planes-only backward.  Inputs: caller planes on both, on none, on the first alone (where the LayerNorm nodes drop both handles
# and the norm-free node splits the second)
PLANE_INPUTS = [(192, 128, 'both'), (192, 128, 'none'), (192, 128, 'first'), (320, 0, 'both'), (320, 0, 'none')]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('K1,K2,have', PLANE_INPUTS)
@pytest.mark.parametrize('N', [256, 320, 328])
@pytest.mark.parametrize('M', [128, 32])
@pytest.mark.parametrize('node', ['planes.dense_ln_act', 'planes.dense_ln_trunk', 'planes.dense_act'])
def test_plane_dense_nodes_keep_the_parent_bits_and_launches(book, node, M, N, K1, K2, have, mode):
    assert os.environ.get('GENRL_PLANES_MIN_ROWS') == '0' and os.environ.get('GENRL_TN_MIN_ROWS') == '64'      # (tests/conftest.py)
    key = f'{node}.M{M}.N{N}.K{K1}+{K2}.{have}.{mode}'
    got = run_case(node, M, N, K1, K2, have, mode, key)
    _check_which_gradients(got, mode, mode != 'x1_nograd')
    book.check(key, got)
