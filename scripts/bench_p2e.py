"""Plan2Explore's ensemble at c3 size on one MI355X: the HIP path against torch-ROCm eager (vendor BLAS, fp32) in one process.

    python scripts/bench_p2e.py [--reps 7] [--warmup 2] [--hip-only]

Two pieces, each timed with device events around work that ends in a synchronise, HIP and torch legs interleaved per repeat:
  train  : Disagreement.forward on B64 x (T50 - 1) = 3136 rows + the backward to all 236 M parameters (no optimiser step in either leg)
  reward : get_disagreement on H15 x 3200 = 48 000 imagined rows + the backward into the rollout's features (ensemble frozen)
Widths: feat 1536, action 6, hidden = embed = 6144, 5 members.  FLOPs are counted from the shapes (2 m n k per product: forward, dgrad
and weight-gradient products; the row kernels are not counted); TF/s = those FLOPs / the median time.  Peak memory: the allocator's high
water mark over one call of the leg, weights and cached weight planes included; "work GB" is that mark less what was allocated when the
call began (the call's own workspace).  Prints a table and one JSON line.  Needs the GPU: there is no CPU leg."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, D, A, E = 5, 1536, 6, 6144
B, T, HOR = 64, 50, 15


def flops(rows, train):
    fwd = 2 * rows * ((D + A) * E + E * E) * K
    if train:       # dgrad into the hidden layer + both weight gradients
        return fwd + 2 * rows * (E * E + E * E + (D + A) * E) * K
    return fwd + 2 * rows * (E * E + E * D) * K          # dgrad into the hidden layer and into the features


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return e0.elapsed_time(e1), peak, peak - held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--hip-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_p2e.py measures on the GPU only'
    from genrl_amd import ops
    from genrl_amd.agent.plan2explore import Disagreement
    ops.set_gemm_precision(ops.F32_MODE)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    dis = Disagreement(D, A, E, pred_dim=E).cuda()
    params = list(dis.parameters())
    n_train, n_rew = B * (T - 1), HOR * B * T
    g = torch.Generator(device='cuda').manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
    obs_t, act_t, nxt_t = rnd(n_train, D), rnd(n_train, A).tanh(), rnd(n_train, E) * 0.5
    obs_r, act_r = rnd(n_rew, D), rnd(n_rew, A).tanh()

    def hip_train():
        dis.requires_grad_(True)
        torch.autograd.grad(dis(obs_t, act_t, nxt_t).mean(), params)
        dis.requires_grad_(False)

    def hip_reward():
        o = obs_r.detach().requires_grad_(True)
        dis.get_disagreement(o, act_r).sum().backward()

    def member(x, m):
        return torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, m[0].weight, m[0].bias)), m[2].weight, m[2].bias)

    def torch_train():
        dis.requires_grad_(True)
        x = torch.cat([obs_t, act_t], -1)
        err = torch.cat([torch.norm(nxt_t - member(x, m), dim=-1, p=2, keepdim=True) for m in dis.ensemble], 1)
        torch.autograd.grad(err.mean(), params)
        dis.requires_grad_(False)

    def torch_reward():
        o = obs_r.detach().requires_grad_(True)
        x = torch.cat([o, act_r], -1)
        torch.var(torch.stack([member(x, m) for m in dis.ensemble], 0), dim=0).mean(-1).sum().backward()

    legs = [('train/hip', hip_train, n_train, True), ('reward/hip', hip_reward, n_rew, False)]
    if not args.hip_only:
        legs = [legs[0], ('train/torch', torch_train, n_train, True), legs[1], ('reward/torch', torch_reward, n_rew, False)]
    times, peak, work = {n: [] for n, *_ in legs}, {}, {}
    for rep in range(args.warmup + args.reps):
        for name, fn, rows, train in legs:               # interleaved: every repeat runs every leg once
            ms, mem, own = timed(fn)
            if rep >= args.warmup:
                times[name].append(ms)
                peak[name], work[name] = max(peak.get(name, 0), mem), max(work.get(name, 0), own)
    out = {}
    print(f'{"leg":14s} {"rows":>6s} {"median ms":>10s} {"min":>8s} {"max":>8s} {"TF/s":>7s} {"peak GB":>8s} {"work GB":>8s}')
    for name, fn, rows, train in legs:
        med = statistics.median(times[name])
        tf = flops(rows, train) / (med * 1e-3) / 1e12
        out[name] = dict(rows=rows, median_ms=round(med, 3), min_ms=round(min(times[name]), 3), max_ms=round(max(times[name]), 3),
                         tflops=round(tf, 1), peak_gb=round(peak[name] / 1e9, 2), work_gb=round(work[name] / 1e9, 2), tflop=round(flops(rows, train) / 1e12, 2))
        print(f'{name:14s} {rows:6d} {med:10.2f} {min(times[name]):8.2f} {max(times[name]):8.2f} {tf:7.1f} {peak[name] / 1e9:8.2f} {work[name] / 1e9:8.2f}')
    print(json.dumps(dict(bench='p2e', reps=args.reps, K=K, D=D, A=A, E=E, legs=out)))


if __name__ == '__main__':
    main()
