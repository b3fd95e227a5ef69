"""Every route of the fp32-operand GEMM engine (csrc/gemm.hip: genrl_sgemm, genrl_sgemm_conv, genrl_sgemm_skinny_parts) against
float64 products computed on the host from the same fp32 operands.

The route table (gemm_route_child.ROUTES) holds one or more products per kernel instantiation that sgemm_impl, launch_rr,
launch_cfg and genrl_sgemm_skinny_parts can select, with shapes on both sides of each dispatch boundary: the skinny limits (M = 32 /
33, 64 / 65, 128 / 129; N and K = 1024 / 1025), the tall kernel (M = 16383 / 16384, K = 112 / 116, K % 4, each (NB, KC) at its N
and K edges, one to three column slabs), K % BK on and off (the KX loaders), 511 / 512 tiles for the 128 tile and the 256-thread
fallback, split-K from both cost loops, the row split of 17408 x 1024 x 1024, ragged M and N, unpadded or odd line pitches and
operand / output offsets of 1..3 floats (the fallback kernels and the unaligned-C epilogue), the implicit-conv operand at 64, 128
and 96-wide tiles, and the plans forced by GENRL_GEMM_FORCE (an empty last split included) and GENRL_SKINNY_MAX_M.

Each group of the table runs in a fresh child process (gemm_route_child.py) with GENRL_GEMM_LOG and GENRL_GEMM_TRACE set, and,
for the switch groups, GENRL_SKINNY_MAX_M or GENRL_GEMM_FORCE: gemm.hip reads them once per process.  Every product runs in
precision modes 0, 2, 3 and 1, once into a NaN-filled output and once with bias and accumulation onto a finite C0.  Here the
parent checks, per call:
  - the route: the launch-log families of the call, the fallback trace line (present exactly for the fallback kernels and the
    unaligned skinny loads), genrl_sgemm_ws_floats > 0 exactly for planned split-K, genrl_sgemm_last_pipe;
  - the values: |C - ref| <= Kc 2^-24 (|A| @ |B|^T + |bias| + |C0|) per element, ref the float64 product (in mode 1 the float64
    product of the operands rounded to bf16, nearest even); Kc per route family and arithmetic, about ten times the worst ratio
    measured on an MI355X (RATIOS holds this run's);
  - nothing outside C changed: padding columns, the guard row, the floats before a C offset.
Refusals (K <= 0, no unit stride, conv operands the gather cannot take) must write nothing; M or N <= 0 is a successful no-op.

After a child dies on a signal or hits its time limit, no further child is started: their tests skip with that reason."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import gemm_route_child as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]

EINVAL = 1
CHILD_TIMEOUT = 600

# Kc per route family . arithmetic (f32: fp32 MFMA, x3: fp32 split into three bf16 terms, bf16: precision 16 against the
# float64 product of the rounded operands), about ten times the worst ratio measured on an MI355X.  The tall kernel's is the
# largest: it starts its accumulators at the bias, so every MFMA rounds relative to it.
K = {
    'skinny.f32': 30, 'tall.f32': 250, 'tile.f32': 100, 'tile.x3': 64, 'tile.bf16': 32,
    'split.f32': 36, 'split.x3': 20, 'split.bf16': 20, 'fallback.f32': 90, 'fallback.bf16': 44,
    'conv.f32': 120, 'conv.x3': 100, 'conv.bf16': 40, 'parts.f32': 18,
}
RATIOS = {}
SEEN = []                # (case, mode, route kind, families, pipe) for the printed summary
_RESULTS = {}
_DEAD = []


def child(group):
    """results of `group`, from one child process per group and module run"""
    if group in _RESULTS:
        if isinstance(_RESULTS[group], str):
            raise AssertionError(_RESULTS[group])
        return _RESULTS[group]
    if _DEAD:
        pytest.skip(f'no more GPU children after {_DEAD[0]}')
    with tempfile.TemporaryDirectory() as d:
        env = {k: v for k, v in os.environ.items() if k not in R.SWITCHES}
        env.update(R.GROUP_ENV.get(group, {}), GENRL_GEMM_LOG=os.path.join(d, 'log'), GENRL_GEMM_TRACE='1',
                   GENRL_TRACE_FILE=os.path.join(d, 'trace'))
        out = os.path.join(d, 'out.json')
        try:
            r = subprocess.run([sys.executable, R.__file__, group, out], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            _DEAD.append(f'group {group} timed out ({CHILD_TIMEOUT} s)')
            raise AssertionError(_DEAD[-1])
        if r.returncode < 0:
            _DEAD.append(f'group {group} died on signal {-r.returncode}')
            raise AssertionError(f'{_DEAD[-1]}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}')
        trace = open(os.path.join(d, 'trace')).read() if os.path.exists(os.path.join(d, 'trace')) else ''
        if r.returncode != 0:
            _RESULTS[group] = f'group {group}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}\n{trace[-4000:]}'
            raise AssertionError(_RESULTS[group])
        with open(out) as f:
            _RESULTS[group] = json.load(f)
    return _RESULTS[group]


def check_calls(cid, c, group, res):
    for mode in R.MODES:
        kind, fam, fb, split, pipe = R.expect(c, mode, group)
        key = R.key_of(kind, pipe, mode, split, group)
        for call, r in zip(('plain', 'bias+acc'), res[str(mode)]):
            what = f'{cid} mode {mode} ({R.MODE_NAME[mode]}) {call}'
            SEEN.append((cid, mode, call, kind, tuple(r['fams']), r['pipe'], key, r['ratio']))
            assert tuple(r['fams']) == fam, f'{what}: launch log {r["fams"]}, expected {fam} (route {kind})'
            assert bool(r['trace']) == fb, f'{what}: fallback trace {r["trace"]}, expected {"one" if fb else "none"}'
            if kind != 'skinny':      # (for the skinny kernel, which takes none, the size is the tiles' upper bound)
                assert (r['ws'] > 0) == split, f'{what}: genrl_sgemm_ws_floats = {r["ws"]}, split-K {"expected" if split else "not expected"}'
            assert r['pipe'] == pipe, f'{what}: genrl_sgemm_last_pipe = {r["pipe"]}, expected {pipe}'
            assert not r['untouched'], f'{what}: {r["untouched"]}'
            RATIOS[key] = max(RATIOS.get(key, 0.0), r['ratio'])
            assert r['ratio'] <= K[key], f'{what}: worst |C - ref| = {r["ratio"]:.3g} x 2^-24 scale, bound {K[key]} ({key})'


def _ids(group):
    return [c['id'] for c in R.ROUTES[group]]


def _case(group, cid):
    return next(c for c in R.ROUTES[group] if c['id'] == cid)


@pytest.fixture(scope='module', autouse=True)
def summary():
    yield
    if SEEN:
        print('\nfp32 GEMM routes (case / mode / call: expected route, launch log, pipe, K key, worst ratio):')
        for cid, mode, call, kind, fams, pipe, key, ratio in SEEN:
            print(f'  {cid:44s} {mode} {call:8s} {kind:7s} {"+".join(fams):24s} pipe {pipe}  {key:14s} {ratio:.3g}')
        print('worst ratio per K key:', json.dumps({k: round(v, 3) for k, v in sorted(RATIOS.items())}))


@pytest.mark.parametrize('cid', _ids('skinny'))
def test_skinny_routes(cid):
    check_calls(cid, _case('skinny', cid), 'skinny', child('skinny')[cid])


@pytest.mark.parametrize('cid', _ids('tall'))
def test_tall_routes(cid):
    check_calls(cid, _case('tall', cid), 'tall', child('tall')[cid])


@pytest.mark.parametrize('cid', _ids('tile'))
def test_tile_routes(cid):
    check_calls(cid, _case('tile', cid), 'tile', child('tile')[cid])


@pytest.mark.parametrize('cid', _ids('split'))
def test_split_k_routes(cid):
    check_calls(cid, _case('split', cid), 'split', child('split')[cid])


@pytest.mark.parametrize('cid', _ids('fallback'))
def test_fallback_routes(cid):
    check_calls(cid, _case('fallback', cid), 'fallback', child('fallback')[cid])


@pytest.mark.parametrize('cid', _ids('conv'))
def test_implicit_conv_routes(cid):
    check_calls(cid, _case('conv', cid), 'conv', child('conv')[cid])


@pytest.mark.parametrize('group,cid', [(g, c['id']) for g in R.GROUP_ENV for c in R.ROUTES[g]])
def test_switch_routes(group, cid):
    """GENRL_SKINNY_MAX_M=256 (skinny_kernel<4, *>), GENRL_GEMM_FORCE=s,7 / b,10 (empty last splits) / m,3 (the 256-thread
    fallback with split-K)"""
    check_calls(cid, _case(group, cid), group, child(group)[cid])


def test_skinny_parts():
    """genrl_sgemm_skinny_parts: nparts 1..64, M 1..32, both B layouts, part_stride beyond M * ldp; the parts sum to the float64
    product and nothing between them is written"""
    res = child('parts')
    assert len(res) == len(R.PARTS)
    for cid, r in res.items():
        assert r['rc'] == 0, (cid, r['rc'])
        assert r['fams'] == ['f32/skinny'] and not r['trace'], (cid, r['fams'], r['trace'])
        assert r['pipe'] == 0, (cid, r['pipe'])
        assert not r['untouched'], (cid, r['untouched'])
        RATIOS['parts.f32'] = max(RATIOS.get('parts.f32', 0.0), r['ratio'])
        SEEN.append((cid, 0, 'parts', 'skinny', tuple(r['fams']), r['pipe'], 'parts.f32', r['ratio']))
        assert r['ratio'] <= K['parts.f32'], f'{cid}: worst ratio {r["ratio"]:.3g}, bound {K["parts.f32"]}'


def test_refusals_write_nothing():
    res = child('refuse')
    for cid, r in res.items():
        assert r['rc'] == r['want'], f'{cid}: returned {r["rc"]}, expected {r["want"]}'
        assert not r['untouched'], f'{cid}: {r["untouched"]}'
