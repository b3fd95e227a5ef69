"""Every route of the plane GEMM engine (csrc/gemm_planes.hip: genrl_gemm_h2, _conv, _subpixel, genrl_gemm_x3, the split kernels;
csrc/gemm_planes_tn.hip: genrl_gemm_h2_tn, _tn_conv) against float64 products of the fp32 values the caller split.

The route table (plane_route_child.ROUTES, CONV, SUBPIXEL, TN, TN_CONV) puts shapes on both sides of each dispatch predicate: the
64 / 128 tile at t64 = 2047 / 2048 and under genrl_planes_force_tile, the two-per-CU ring at 256 / 257 tiles and K = 1536 / 1600
(and forced by GENRL_PLANES_2PER=0 / 1), the row split of 17408 x 1024 and its near misses (M % 128, r > 128, r % tn), use_wide
at N = 190, 192, 200, 320, 384, 576 under GENRL_HL_WIDE = 1 / 0 / 2, GENRL_PLANES_HL=0, two segments on both tiles, bias and
accumulation, ldc padding, c_off, row offsets of both operands, ragged M and N; the tall 256 x 96 conv tile at K = 1024 / 896 and
N = 96 / 104, K not a multiple of 64, odd images, ld_img > Cc; the sub-pixel form at 192 / 384 columns, a zero tap, images that
drop and leave unreached output positions; TN at one split and at splits from tn_splits with a short last one, NJ % 4 != 0;
genrl_gemm_h2_ln and genrl_gemm_h2_sample (their pre-activation per element, the epilogue outputs against float64 of the kernel's
own C), segment-1 scales 2^+-40 (2^30 on _ln) away and all-zero rows of A1 / B1 on both; and an imagination from RSSM.initial.
Each group runs in a fresh child process (GENRL_GEMM_LOG set, plus its switch: gemm_planes.hip reads them once per process).

Per call the parent checks the route (genrl_planes_last_route: the instantiations and, for TN, the split count; the launch-log
families), that the result is finite and bit-identical across two runs, that nothing outside the output changed, and
  |C - ref| <= Kc 2^-24 (sum_k |a| |b| + |bias| + |C0|) + floor      per element, Kc per route family (K below).
floor (derived from the representation, per element):
  - h2 operands: a scaled element a s = h + l / 2^11 keeps 2^-22 |a s| for elements within 2^-28 of its row maximum; below that
    the fp16 l plane runs into its subnormals, an absolute loss of at most 2^-25 / 2^11 = 2^-36 in scaled units, i.e. 2^-36
    inv[row] in the element.  Summed over k: floor = 2^-36 (inv_a[m] sum_k |b[n, k]| + inv_b[n] sum_k |a[m, k]|) per segment.
  - TN: the B fragments are multiplied by f[m] = inv_a[m] inv_b[m] / cref in fp16; values that fall below fp16's normal range
    lose at most 2^-25 per plane value (2^-24 sum_m cref |a'(m, i)| over both planes), and rows with f < 2^-24 vanish by design
    (gemm_planes_tn.hip header): their whole contribution sum_m |A(m, i)| |B(m, j)| joins the floor.
Refusals must return GENRL_EINVAL, report no route and write nothing.  The split kernels are compared bit for bit with a float64
recomputation and against the documented representation.

Worst ratios measured on an MI355X and the Kc set from them are next to K."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import plane_route_child as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]

EINVAL = 1
CHILD_TIMEOUT = 600
# Kc per route family, about ten times the worst ratio measured on an MI355X (64x64 tiles 14.6, 128x128 / 128x192 7.6, stride-2
# conv 16.9, sub-pixel 4.0, TN 12.4, x3 15.9)
K = {'64': 150, '128': 80, 'conv': 170, 'subpixel': 40, 'tn': 125, 'x3': 160}
RATIOS = {}
_RESULTS = {}
_DEAD = []


def child(group, env_group=None):
    key = group if env_group is None else f'{group}@{env_group}'
    if key in _RESULTS:
        if isinstance(_RESULTS[key], str):
            raise AssertionError(_RESULTS[key])
        return _RESULTS[key]
    if _DEAD:
        pytest.skip(f'no more GPU children after {_DEAD[0]}')
    with tempfile.TemporaryDirectory() as d:
        env = {k: v for k, v in os.environ.items() if k not in R.SWITCHES}
        env.update(R.GROUP_ENV.get(env_group or group, {}), GENRL_GEMM_LOG=os.path.join(d, 'log'))
        out = os.path.join(d, 'out.json')
        try:
            r = subprocess.run([sys.executable, R.__file__, group, out], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            _DEAD.append(f'group {group} timed out ({CHILD_TIMEOUT} s)')
            raise AssertionError(_DEAD[-1])
        if r.returncode < 0:
            _DEAD.append(f'group {group} died on signal {-r.returncode}')
            raise AssertionError(f'{_DEAD[-1]}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}')
        if r.returncode != 0:
            _RESULTS[key] = f'group {group}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}'
            raise AssertionError(_RESULTS[key])
        with open(out) as f:
            _RESULTS[key] = json.load(f)
    return _RESULTS[key]


def family(routes):
    r = routes[0]
    return 'subpixel' if r.startswith('subpixel') else ('conv' if r.startswith('conv') else ('tn' if r.startswith('tn') else
                                                                                           ('x3' if r.startswith('x3') else r.split('/')[0])))


def check(cid, calls, want, fams=None, splits=None):
    for r in calls:
        what = f'{cid} ({r["call"]})'
        assert r['rc'] == 0, f'{what}: returned {r["rc"]}'
        routes, nsplit = r['route']
        assert routes == sorted(want), f'{what}: genrl_planes_last_route {routes}, expected {sorted(want)}'
        if splits is not None:
            assert nsplit == splits, f'{what}: {nsplit} splits, expected {splits}'
        if fams is not None:
            assert r['fams'] == fams, f'{what}: launch log {r["fams"]}, expected {fams}'
        assert r['finite'], f'{what}: C holds Inf or NaN'
        assert r['untouched'], f'{what}: a kernel wrote outside its output'
        assert r['repro'], f'{what}: two runs differ'
        key = family(want)
        RATIOS[key] = max(RATIOS.get(key, 0.0), r['ratio'])
        assert r['ratio'] <= K[key], f'{what}: worst (|C - ref| - floor) = {r["ratio"]:.3g} x 2^-24 scale, bound {K[key]} ({key})'


@pytest.fixture(scope='module', autouse=True)
def summary():
    yield
    if RATIOS:
        print('\nplane GEMM routes, worst ratio per family:', json.dumps({k: round(v, 3) for k, v in sorted(RATIOS.items())}))


@pytest.mark.parametrize('group,cid', [(g, c['id']) for g in R.ROUTES for c in R.ROUTES[g]])
def test_gemm_h2_routes(group, cid):
    c = next(c for c in R.ROUTES[group] if c['id'] == cid)
    check(cid, child(group)[cid], c['route'], c['fam'])


@pytest.mark.parametrize('cid', [c[0] for c in R.CONV + R.SUBPIXEL])
def test_conv_routes(cid):
    r = child('conv')[cid]
    check(cid, r, r[0]['want'])


def test_conv_routes_without_half_stages():
    """GENRL_PLANES_HL=0: the two-whole-stages conv instantiation; the sub-pixel form is refused (its epilogue needs the other)"""
    res = child('conv_hl0', 'hl0')
    for cid, r in res.items():
        if cid == 'subpixel.hl0-refused':
            assert r[0]['rc'] == EINVAL and r[0]['nothing'], (cid, r[0]['rc'], 'wrote' if not r[0]['nothing'] else '')
        else:
            check(cid, r, ['conv/plain'])


@pytest.mark.parametrize('cid', [c[0] for c in R.TN + R.TN_CONV])
def test_tn_routes(cid):
    r = child('tn')[cid]
    check(cid, r, r[0]['want'], splits=r[0]['splits'])
    if cid == 'tn.splits.short-last':
        assert r[0]['splits'] == 12, r[0]['splits']       # 107 stages in splits of 9: the last one has 8


@pytest.mark.parametrize('cid', [c[0] for c in R.LN])
def test_gemm_h2_ln(cid):
    """the pre-activation C per element (two segments with 2^+-40 scale offsets and zero rows of A1 / B1 included); y and mean finite
    and within 2^-16 of the float64 LayerNorm + SiLU of the kernel's own C; the exchange's failure word stays 0"""
    r = child('ln')[cid]
    check(cid, r, ['64/ln'], ['h2/64ln'])
    assert r[0]['y_err'] <= 2.0 ** -16 and r[0]['mean_err'] <= 2.0 ** -16, (cid, r[0]['y_err'], r[0]['mean_err'])


@pytest.mark.parametrize('cid', [c[0] for c in R.SAMPLE])
def test_gemm_h2_sample(cid):
    """the logits C per element; the one-hot sample is the exponential-race argmax of the kernel's own C"""
    r = child('sample')[cid]
    check(cid, r, ['64/sample'], ['h2/64'])
    assert r[0]['sample_ok'], f'{cid}: the sample is not the argmax of the kernel\'s own logits'


def test_x3_routes():
    for cid, r in child('x3').items():
        check(cid, r, r[0]['want'])


def test_split_kernels():
    for cid, r in child('split').items():
        assert r['rc'] == 0, (cid, r['rc'])
        assert not r['bad'], f'{cid}: {r["bad"][:5]}'


def test_refusals_write_nothing():
    """every refusal returns GENRL_EINVAL, launches nothing and writes nothing; the base arguments it varies are accepted"""
    res = child('refuse')
    for cid, r in res.items():
        if r['want'] == 0:
            assert r['rc'] == 0 and r['route'][0] and not r['untouched'], f'{cid}: base call returned {r["rc"]}, route {r["route"]}'
            continue
        assert r['rc'] == EINVAL, f'{cid}: returned {r["rc"]}, expected GENRL_EINVAL'
        assert r['untouched'], f'{cid}: wrote to C'
        assert r['route'][0] == [] and r['fams'] == [], f'{cid}: launched {r["route"]} {r["fams"]}'


@pytest.mark.parametrize('tiny', [True, False])
def test_rollout_from_the_initial_state(tiny, monkeypatch):
    """the imagination from RSSM.initial (zero stoch, zero deter: the GRU cell's initial state) on the plane path: its first
    products [x, deter] W_g^T and [stoch, action] W_in^T have all-zero segment-1 rows.  Every metric and every actor / critic
    gradient must be finite and agree with the fp32-operand path on the same weights and noise (the plane products' rounding and
    the few categorical samples it may flip stay well inside the tolerance)"""
    import math
    import detgen
    from param_shapes import agent_param_shapes
    from oracle import genrl_oracle as O
    from genrl_amd import config, noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    from test_gpu_iteration import FakeClip
    BS, BL, A, H, seed = 4, 16, 10, 15, 5
    S, Kc = (4, 4) if tiny else (32, 32)
    wid = dict(deter=32, hidden=32, units=32, cnn_depth=4) if tiny else {}
    ocfg = O.make_cfg(stoch=S, discrete=Kc, act_dim=A, horizon=H, **wid)
    p = detgen.det_state_dict(agent_param_shapes(ocfg), seed)
    nz = detgen.iteration_noise(BS, BL, S, Kc, A, H, seed=seed)['imag']

    def run(planes):
        if planes:
            monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '0')
        else:
            monkeypatch.delenv('GENRL_PLANES_MIN_ROWS', raising=False)      # (64 rows: below the default's 192, the fp32 operands)
        zero = dict(lr=0.0, wd=0.0)
        cfg = config.default_cfg(BS, BL, device='cuda', imag_horizon=H, model_opt=zero, actor_opt=zero, critic_opt=zero,
                                 **(config.tiny_overrides() if tiny else {}))
        ag = config.make_agent(cfg, act_dim=A)
        ag.load_state_dict({k: v.cuda() for k, v in p.items()})
        ag.wm.viclip_model = FakeClip()
        init = ag.wm.rssm.initial(BS * BL)
        post = {k: v.reshape(BS, BL, *v.shape[1:]).clone() for k, v in init.items()}
        assert all(float(v.abs().max()) == 0.0 for v in post.values())
        grads = {}
        names = {id(q): n for n, q in ag.named_parameters()}
        common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone() for q in params})
        try:
            with gnoise.inject({'imag.act_eps': nz['act_eps'], 'imag.step_q': nz['step_q'], 'imag.target_init_q': nz['target_init_q']}):
                outputs = dict(post=post, is_terminal=torch.zeros(BS, BL, device='cuda'))
                _, mets = ag.update_imag_behavior(state=None, outputs=outputs, metrics={}, seq_data=None)
        finally:
            common.Optimizer.grad_hook = None
        return {k: float(v) for k, v in mets.items()}, grads
    m1, g1 = run(True)
    m0, g0 = run(False)
    bad = {k: v for k, v in m1.items() if not math.isfinite(v)}
    assert not bad, f'plane path from the initial state: non-finite metrics {bad}'
    for ph in g1:
        for n, gr in g1[ph].items():
            assert bool(torch.isfinite(gr).all()), f'plane path from the initial state: non-finite gradient {ph} {n}'
    far = {k: (m1[k], m0[k]) for k in m0 if abs(m1[k] - m0[k]) > 2e-2 * abs(m0[k]) + 1e-3}
    assert not far, f'plane path vs fp32 operands from the initial state: {far}'
