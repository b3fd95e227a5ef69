"""Helpers of the float64 kernel tests (test_gpu_row_kernel_variants.py, test_gpu_dist_optim_variants.py, test_gpu_plane_variants.py, test_gpu_conv_loops.py): per-element bounds
against a float64 reference, NaN-prefilled output buffers with padding columns and a guard row, and the check that a kernel
wrote nothing outside its output."""
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff
PAD = -1.2345678e33     # what the padding columns and guard rows of output buffers hold


def checker(K, RATIOS):
    """-> within(what, got, ref, scale, key=None): |got - ref| <= K[key] 2^-24 scale elementwise (got: any device / dtype; ref,
    scale: float64 CPU); key defaults to `what` up to its first '['.  The largest ratio |got - ref| / (2^-24 scale) seen per
    key is recorded in RATIOS."""
    def within(what, got, ref, scale, key=None):
        key = key or what.split('[')[0]
        got = got.detach().cpu().double()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        err = (got - ref).abs()
        ratio = err / (U * scale).clamp_min(1e-300)
        worst = float(torch.nan_to_num(ratio, nan=math.inf).max()) if ratio.numel() else 0.0
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
        bad = ~(err <= K[key] * U * scale)
        if bad.any():
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements out of bound (K = {K[key]}, worst ratio {worst:.3g}); '
                                 f'first at {i}: got {float(got[i])!r}, float64 {float(ref[i])!r}, scale {float(scale[i])!r}')
    return within


def out_buf(rows, cols, ld, off=0):
    """NaN-filled output [rows, cols] inside a buffer of rows + 1 lines of ld floats starting `off` floats in; the rest holds PAD"""
    buf = torch.full(((rows + 1) * ld + off + 4,), PAD, device='cuda')
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.fill_(float('nan'))
    return buf, view


def in_buf(src, ld, off=0):
    """src (CPU fp32 [rows, cols]) copied into a device buffer of lines ld floats apart, `off` floats in; padding = NaN"""
    rows, cols = src.shape
    buf = torch.full(((rows + 1) * ld + off + 4,), float('nan'), device='cuda')
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(src)
    return view


def untouched(what, buf, view):
    """every float of buf outside `view` still holds PAD"""
    assert untouched_ok(buf, view), f'{what}: a kernel wrote outside its output'


def untouched_ok(buf, view):
    """-> whether every float of buf outside `view` still holds PAD"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    off = view.storage_offset() - buf.storage_offset()
    rows, cols = view.shape if view.dim() == 2 else (1, view.numel())
    ld = view.stride(0) if view.dim() == 2 else cols
    idx = off + torch.arange(rows, device='cuda')[:, None] * ld + torch.arange(cols, device='cuda')[None, :]
    mask[idx.reshape(-1)] = False
    rest = buf[mask]
    return bool(torch.equal(rest, torch.full_like(rest, PAD)))
