"""Full-WIDTH parity cases for the BASELINE configs that the reference-recorded goldens only pin at tiny widths
(tests/test_gpu_iteration.py: c3_dreamer_tiny, c4_tiny; tests/test_gpu_datafree.py: c5_datafree_tiny): the same
iterations at the configs' real layer widths, on batches the CPU oracle finishes in seconds, against the oracle on the
same weights / batch / noise -- every metric and the per-phase gradient norms within north_star's 1e-3 relative.
(c1 and c2 at full size: test_gpu_iteration.py.)  Plus the operand edge cases of the split-operand GEMMs."""
import os
import numpy as np
import pytest
import torch

import detgen
from param_shapes import agent_param_shapes
from oracle import genrl_oracle as O
from oracle.iteration import run_iteration, run_dreamer_iteration, _leafs, _grads, group_names
from test_gpu_iteration import run_product, FakeClip

pytestmark = pytest.mark.gpu


def _phase_norm(gs):
    return np.sqrt(sum(float((t.double() ** 2).sum()) for t in gs.values()))


def _check_metrics(mets, om, min_checked):
    n = 0
    for k, v in mets.items():
        if k in om and np.isfinite(om[k]):
            np.testing.assert_allclose(v, om[k], rtol=1e-3, atol=1e-5, err_msg=k)
            n += 1
    assert n >= min_checked, (n, sorted(set(mets) & set(om)))


@pytest.mark.parametrize('B,T', [(8, 16), (32, 32)])
def test_c4_kitchen_128px_full_width_vs_oracle(B, T):
    """configs[3]: 128x128 frames, five-layer encoder / decoder at cnn_depth 48 (48..768 channels, E = 3072), A = 9,
    default 1024-wide RSSM / heads; B8 x T16 and the config's FULL size B32 x T32 (the CPU oracle needs ~15 s for that one)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    over = dict(encoder=dict(cnn_kernels=[4, 4, 4, 4, 4]), decoder=dict(cnn_kernels=[5, 5, 5, 6, 6]))
    oc = dict(img=128, enc_kernels=(4, 4, 4, 4, 4), dec_kernels=(5, 5, 5, 6, 6))
    meta = {'meta': (B, T, 9, 32, 32, 16, 4), 'img': 128}
    g, ocfg, p, batch, noise, ag, outputs, mets_wm, mets, grads = run_product(meta, True, over, oc)
    assert outputs['embed'].shape[-1] == 3072
    res = run_iteration(p, ocfg, batch, noise, FakeClip().get_txt_feat(''), apply_updates=False)
    _check_metrics({**mets_wm, **mets}, {k: float(v) for k, v in res['metrics'].items()}, 20)
    post_idx = res['outs']['post']['stoch'].argmax(-1).numpy()
    assert (outputs['post']['stoch'].argmax(-1).cpu().numpy() != post_idx).mean() < 2e-3
    for ph in ('wm', 'conn2', 'actor', 'critic'):
        np.testing.assert_allclose(_phase_norm(grads[ph]), _phase_norm(res['grads'][ph]), rtol=1e-3, err_msg=ph)


@pytest.mark.parametrize('T', [48, 50])
def test_c3_dreamer_v3_512_units_vs_oracle(T):
    """configs[2] at its widths: DreamerAgent with dreamer_v3.yaml (deter = hidden = units = 512, posterior from
    [deter, embed], decoder on feat, trained reward head, env_reward, actor entropy 3e-4, horizon 15), walker A = 6,
    T = 48 and the config's own T = 50 (no multiple of 8: not a GenRL length); B8 = the per-GPU batch of its DP-8 layout."""
    from genrl_amd import config, noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B, A, S, K, H, seed = 8, 6, 32, 32, 15, 6
    zero = dict(lr=0.0, wd=0.0)
    cfg = config.dreamer_cfg(B, T, device='cuda', model_opt=zero, actor_opt=zero, critic_opt=zero)
    ag = config.make_dreamer_agent(cfg, act_dim=A)
    ocfg = O.make_cfg(stoch=S, discrete=K, act_dim=A, horizon=H, deter=512, hidden=512, units=512,
                      single_obs_posterior=False, decoder_inputs='feat', reward_grad=True, actor_ent=3e-4)
    p = detgen.det_state_dict(agent_param_shapes(ocfg, dreamer=True), seed)
    assert {k: tuple(v.shape) for k, v in ag.state_dict().items()} == {k: tuple(v.shape) for k, v in p.items()}
    ag.load_state_dict({k: v.cuda() for k, v in p.items()})
    bc = {k: torch.from_numpy(v) for k, v in detgen.det_batch(B, T, A=A, seed=seed).items() if k != 'clip_video'}
    batch = {k: v.cuda() for k, v in bc.items()}
    noise = detgen.iteration_noise(B, T, S, K, A, H, seed=seed)
    sites = {'rssm.prior': [noise['wm']['prior_q'][t] for t in range(T)],
             'rssm.post': [noise['wm']['post_q'][t] for t in range(T)],
             'imag.act_eps': noise['imag']['act_eps'], 'imag.step_q': noise['imag']['step_q']}
    grads = {}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(
        {'model': 'wm', 'actor': 'actor', 'critic': 'critic'}[opt], {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    try:
        with gnoise.inject(sites):
            state, outputs, mets = ag.update_wm(batch, 0)
            mets_wm = {k: float(v) for k, v in mets.items()}
            _, mets = ag.update_acting_behavior(state, outputs, {}, batch)
    finally:
        common.Optimizer.grad_hook = None
    mets = {k: float(v) for k, v in mets.items()}
    res = run_dreamer_iteration(p, ocfg, bc, noise)
    _check_metrics({**mets_wm, **mets}, {k: float(v) for k, v in res['metrics'].items()}, 15)
    post_idx = res['outs']['post']['stoch'].argmax(-1).numpy()
    assert (outputs['post']['stoch'].argmax(-1).cpu().numpy() != post_idx).mean() < 2e-3
    for ph in ('wm', 'actor', 'critic'):
        np.testing.assert_allclose(_phase_norm(grads[ph]), _phase_norm(res['grads'][ph]), rtol=1e-3, err_msg=ph)


@pytest.mark.parametrize('operands', ['default_planes_from_256_rows', 'exact_fp32_switch'])
def test_c5_datafree_256_rows_horizon_15_vs_oracle(operands, monkeypatch):
    """configs[4]'s update: update_imag_behavior on 256 imagined start rows (batch_size 16 x batch_length 16) with
    horizon 15 at full width -- the pure RSSM.imagine / lambda-return / actor-critic stress.  (The data-free block's
    own call sequence -- uniform latents, connector starts, warm-up rollouts -- is pinned to the reference's recorded
    outputs in test_gpu_datafree.py.)  Runs under the PRODUCT's operand policy (round 6: plane operands from 192 rows:
    sampled latents may differ on near-ties, at the rate the c3 / c4 full-size cases accept) and with the explicit switch
    back to fp32 operands at this size (GENRL_PLANES_MIN_ROWS=320: every sampled latent exact)."""
    _c5_case(operands, 10, monkeypatch)


@pytest.mark.parametrize('operands', ['default_planes_from_256_rows', 'exact_fp32_switch'])
@pytest.mark.parametrize('A', [12, 32])
def test_c5_datafree_action_width_vs_oracle(A, operands, monkeypatch):
    """The c5 case above at action widths the goldens never run: A = 12 (the quadruped tasks; the action rows of
    roundup4(A) columns have no padding column, and the fused actor head takes its MAXO = 32 forward / MAXO = 16 backward
    instantiations) and A = 32 (the largest width the fused head accepts: MAXO = 64 / 32)."""
    _c5_case(operands, A, monkeypatch)


def _c5_case(operands, A, monkeypatch):
    from genrl_amd import config, noise as gnoise
    from genrl_amd.agent import dreamer_utils as common
    from genrl_amd import ops_planes
    if operands == 'exact_fp32_switch':
        monkeypatch.setenv('GENRL_PLANES_MIN_ROWS', '320')
    else:
        monkeypatch.delenv('GENRL_PLANES_MIN_ROWS', raising=False)    # the product's default threshold (192 rows)
        assert ops_planes.min_rows() == 192
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    BS, BL, S, K, H, seed = 16, 16, 32, 32, 15, 8
    zero = dict(lr=0.0, wd=0.0)
    cfg = config.default_cfg(BS, BL, device='cuda', imag_horizon=H, model_opt=zero, actor_opt=zero, critic_opt=zero)
    ag = config.make_agent(cfg, act_dim=A)
    ocfg = O.make_cfg(stoch=S, discrete=K, act_dim=A, horizon=H)
    p = detgen.det_state_dict(agent_param_shapes(ocfg), seed)
    ag.load_state_dict({k: v.cuda() for k, v in p.items()})
    ag.wm.viclip_model = FakeClip()
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, K, (BS, BL, S), generator=g)
    post = dict(stoch=torch.nn.functional.one_hot(idx, K).float(), deter=torch.tanh(torch.randn(BS, BL, 1024, generator=g)),
                logit=torch.randn(BS, BL, S, K, generator=g))
    noise = detgen.iteration_noise(BS, BL, S, K, A, H, seed=seed)['imag']
    grads = {}
    names = {id(q): n for n, q in ag.named_parameters()}
    common.Optimizer.grad_hook = lambda opt, params: grads.__setitem__(opt, {names[id(q)]: q.grad.detach().clone().cpu() for q in params})
    try:
        with gnoise.inject({'imag.act_eps': noise['act_eps'], 'imag.step_q': noise['step_q'],
                            'imag.target_init_q': noise['target_init_q']}):
            outputs = dict(post={k: v.cuda() for k, v in post.items()}, is_terminal=torch.zeros(BS, BL, device='cuda'))
            _, mets = ag.update_imag_behavior(state=None, outputs=outputs, metrics={}, seq_data=None)
    finally:
        common.Optimizer.grad_hook = None
    mets = {k: float(v) for k, v in mets.items()}
    # the oracle's imagination phase (oracle/iteration.py, third block)
    gn = group_names(p)
    q = _leafs(p, gn['actor'] + gn['critic'])
    seq = O.imagine(q, ocfg, post, noise)
    with torch.no_grad():
        target = O.video_imagine_target(p, ocfg, FakeClip().get_txt_feat(''), BS * BL, H + 1, noise['target_init_q'])
    reward, _ = O.video_text_reward(q, ocfg, seq['stoch'], target['stoch'])
    al, cl, lam_t, om, _ = O.actor_critic_losses(q, ocfg, seq, reward, torch.zeros(2))
    ga, gc = _grads(al, q, gn['actor']), _grads(cl, q, gn['critic'])
    om = {f'imag_{k}': (float(v) if torch.is_tensor(v) else v) for k, v in
          dict(actor_loss=al, critic_loss=cl, **O.stream_norm_metrics(reward.detach()), **om).items()}
    # sampled target latents at full width: exact on the fp32-operand kernels; with plane operands (the default from 192 rows) one of
    # the 8192 samples falls on the other side of a near-tie -- the same < 2e-3 rule as the c3 / c4 cases above
    mism = (ag.unconditional_target['stoch'].argmax(-1).cpu() != target['stoch'].argmax(-1)).float().mean().item()
    if operands == 'exact_fp32_switch':
        # (GENRL_GEMM_MODE=3, the experimental split on every tile, also moves one near-tie: <= 2 of 8192 there)
        assert mism == 0 or (os.environ.get('GENRL_GEMM_MODE') == '3' and mism <= 3e-4), mism
    else:
        assert mism < 2e-3, mism
    _check_metrics(mets, om, 12)
    np.testing.assert_allclose(_phase_norm(grads['actor']), _phase_norm(ga), rtol=1e-3)
    np.testing.assert_allclose(_phase_norm(grads['critic']), _phase_norm(gc), rtol=1e-3)


def test_split_operand_gemm_edge_values():
    """The split-operand products (h2 planes: gemm_planes_kernel, and the in-register bf16 split sgemm_rr<BF=3>) against fp32
    MFMAs (GENRL_GEMM_MODE=0 arithmetic) on operand values at the edges: an Inf operand gives NaN where the fp32 MFMA gives
    Inf (the residual of the split is Inf - Inf; documented in DESIGN.md) and stays confined to the affected outputs;
    magnitudes down to 1e-30 keep fp32-sized error; below ~1e-33 the low terms of the unscaled bf16 split flush and that
    product degrades gracefully (relative error <= 2^-8 of those tiny terms, absolute error far below fp32's normal range),
    while the row-scaled h2 planes keep full accuracy."""
    from genrl_amd import ops, planes
    g = torch.Generator(device='cuda').manual_seed(1)
    M = N = K = 256
    A = torch.randn(M, K, device='cuda', generator=g); B = torch.randn(N, K, device='cuda', generator=g)

    def products(A, B):
        out = {}
        for mode in ('f32', 'bf16x3'):
            prev = ops.set_gemm_precision(mode)
            try:
                C = torch.empty(M, N, device='cuda')
                ops.sgemm(A, K, 1, B, K, 1, C, N, None, M, N, K)
                out[mode] = C
            finally:
                ops.set_gemm_precision(prev)
        C = torch.empty(M, N, device='cuda')
        planes.gemm(planes.split(A), planes.split(B), C, N, None, M, N)
        out['h2'] = C
        return out
    # tiny magnitudes that every term of the split still resolves
    o = products(A * 1e-30, B * 1e+10)
    ref = (A.double() * 1e-30) @ (B.double() * 1e10).t()
    for k in ('bf16x3', 'h2'):
        assert ((o[k].double() - ref).abs().max() / ref.abs().mean()).item() < 2e-5, k
    # magnitudes where the low terms underflow: still a usable product (error bounded by the dropped bits)
    o = products(A * 1e-36, B)
    ref = (A.double() * 1e-36) @ B.double().t()
    for k in ('bf16x3', 'h2'):
        assert ((o[k].double() - ref).abs().max() / ref.abs().mean()).item() < (2e-2 if k == 'bf16x3' else 2e-5), k
        assert torch.isfinite(o[k]).all()
    # one infinite operand element
    Ai = A.clone(); Ai[3, 7] = float('inf')
    o = products(Ai, B)
    assert torch.isinf(o['f32'][3]).all() and torch.isfinite(o['f32'][torch.arange(M) != 3]).all()
    for k in ('bf16x3', 'h2'):
        assert not torch.isfinite(o[k][3]).any(), k                       # NaN (or Inf) across the affected row ...
        assert torch.isfinite(o[k][torch.arange(M) != 3]).all(), k        # ... and nowhere else
