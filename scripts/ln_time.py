"""LayerNorm(+SiLU) fwd / bwd kernel time at the model's shapes: python scripts/ln_time.py"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from genrl_amd._lib import lib, check
L = lib(); dev = 'cuda'
st = torch.cuda.current_stream().cuda_stream
def timeit(fn, n=200):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
out = []
for M in (128, 1024, 16384):
    N = 1024
    x = torch.randn(M, N, device=dev); dy = torch.randn(M, N, device=dev); y = torch.empty_like(x); dx = torch.empty_like(x)
    g = torch.randn(N, device=dev); b = torch.randn(N, device=dev); mean = torch.empty(M, device=dev); rstd = torch.empty(M, device=dev)
    ws = torch.empty(L.genrl_ln_ws_floats(M, N), device=dev); gb = torch.empty(3, N, device=dev)
    f = timeit(lambda: check(L.genrl_ln_act_fwd(x.data_ptr(), N, g.data_ptr(), b.data_ptr(), y.data_ptr(), N, mean.data_ptr(), rstd.data_ptr(), M, N, 1e-5, 1, st), 'f'))
    bw = timeit(lambda: check(L.genrl_ln_act_bwd(dy.data_ptr(), N, x.data_ptr(), N, g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), N, gb[0].data_ptr(), gb[1].data_ptr(), gb[2].data_ptr(), ws.data_ptr(), M, N, 1, 0, st), 'b'))
    bn = timeit(lambda: check(L.genrl_ln_act_bwd(dy.data_ptr(), N, x.data_ptr(), N, g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), N, None, None, None, None, M, N, 1, 0, st), 'b'))
    from genrl_amd import planes as _pl
    P = _pl.Planes(M, N, dev)
    fp = timeit(lambda: check(L.genrl_ln_act_fwd_h2(x.data_ptr(), N, g.data_ptr(), b.data_ptr(), y.data_ptr(), N, mean.data_ptr(), rstd.data_ptr(), M, N, 1e-5, 1, P.ptr(), P.ld, P.plane, P.inv_ptr(), st), 'fp'))
    out.append(f'M={M}: fwd {f:.1f} fwd+planes {fp:.1f} bwd+params {bw:.1f} bwd {bn:.1f} us')
print(' | '.join(out))
