"""The imagination rollout (WorldModel.imagine, agent/dreamer.py:254-287) on pre-split ("h2 plane") GEMM operands.

Same autograd node structure as ops._Rollout / ops.ActorTape (one node for the H-step loop, the policy's backward batched
over all H*N rows), but every activation that feeds a GEMM is written by its producing row kernel as two fp16 planes of
the row-scaled value plus the row's inverse scale (genrl_*_h2 entry points) next to its fp32 copy, the frozen world-model /
policy weights are split once per optimiser step (planes.weight), and the products run in genrl_gemm_h2: fp32-accurate
arithmetic on the fp16 matrix cores (three MFMAs per block and k-step) with a pure DMA + MFMA K loop.  Two-input layers ([stoch, action] -> img_in, [x, deter] -> GRU, [stoch, deter] -> policy) are ONE
launch with two operand segments.  Weight gradients stay on the fp32-operand kernels (ops.sgemm)."""
import os

import torch
from torch.autograd import Function

from ._lib import lib, check, struct as _cstruct
from . import planes
from . import planes as pl          # (module alias: `planes=` parameters below are operand handles)
from . import ops
from .ops import _p, _f32, _ln_param_targets, _wgrad_target, _bias_grad, sgemm, fill, UNIMIX

_stream = ops._stream


def _ln_fwd(pre_ptr, gamma, beta, y_ptr, mean_ptr, rstd_ptr, M, N, eps, P, row0, act=1):
    check(lib().genrl_ln_act_fwd_h2(pre_ptr, N, _p(gamma), _p(beta), y_ptr, N, mean_ptr, rstd_ptr, M, N, eps, act,
                                    P.ptr(row0), P.ld, P.plane, P.inv_ptr(row0), _stream()), 'ln_act_fwd_h2')


def _ln_bwd(dy_ptr, pre_ptr, gamma, beta, mean_ptr, rstd_ptr, dpre_ptr, M, N, P, row0, g0=None, g1=None, g2=None, ws=None,
            acc_p=0, act=1):
    check(lib().genrl_ln_act_bwd_h2(dy_ptr, N, pre_ptr, N, _p(gamma), _p(beta), mean_ptr, rstd_ptr, dpre_ptr, N, _p(g0),
                                    _p(g1), _p(g2), _p(ws), M, N, act, acc_p, P.ptr(row0), P.ld, P.plane, P.inv_ptr(row0),
                                    _stream()), 'ln_act_bwd_h2')


class ActorTapePlanes(ops.ActorTape):
    """ops.ActorTape with plane copies of the hidden activations (time-major rows h*N + n) and plane-operand products for the
    forward and the batched dgrad; the weight gradients read the fp32 copies."""
    def __init__(self, H, N, layers, head_w, head_b, dev):
        super().__init__(H, N, layers, head_w, head_b, dev)
        self.yp = [planes.Planes(H * N, l[0].shape[0], dev) for l in layers]

    def _keeps_y(self, l):
        """The last layer's output is the head's input.  A hidden layer's fp32 copy has ONE reader -- the next layer's weight gradient, and only
        where that product stays on the fp32-operand kernel (_backward: `not tn`): with it on planes the LayerNorm writes planes only (self.y[l]
        is None), where its kernel can (the fused product + LayerNorm always can; the row kernel from 257 to 4096 columns)."""
        if l == len(self.layers) - 1:
            return True
        U, Un = self.layers[l][0].shape[0], self.layers[l + 1][0].shape[0]
        return not (planes.tn_ok(self.H * self.N, Un, U, U) and 256 < U <= 4096 and U % 4 == 0)

    def _forward(self, *args, **kwargs):
        # (the step-by-step form reads every layer's fp32 output and fills no planes: this tape is driven by imagine_rollout alone)
        raise ops.GenrlHipError('ActorTapePlanes runs inside ops_planes.imagine_rollout only; the step-by-step rollout takes ops.ActorTape')

    def _forward_planes(self, t, sp_, dp_, out):
        """layer 0 input = rows t*N.. of the rollout's stoch / deter planes (sp_, dp_)"""
        N = self.N
        Ap, row0 = None, t * N
        for l, (W, b, gamma, beta, eps) in enumerate(self.layers):
            U, K = W.shape
            pre, y = self.pre[l], self.y[l]
            off = t * N * U
            fuse = planes.gemm_ln_ok(N, U, pre.device)
            if l == 0:
                K1 = sp_.cols
                if fuse:
                    planes.gemm_ln(sp_, planes.weight(W, c0=0, c1=K1), pre, b, N, U, gamma, beta, eps, self.yp[l], row0, y=y, mean=self.mean[l],
                                   rstd=self.rstd[l], a_row0=row0, A1=dp_, B1=planes.weight(W, c0=K1), a1_row0=row0, c_off=off, y_off=off, m_off=t * N)
                else:
                    planes.gemm(sp_, planes.weight(W, c0=0, c1=K1), pre, U, b, N, U, a_row0=row0, A1=dp_, B1=planes.weight(W, c0=K1),
                                a1_row0=row0, c_off=off)
            elif fuse:
                planes.gemm_ln(Ap, planes.weight(W), pre, b, N, U, gamma, beta, eps, self.yp[l], row0, y=y, mean=self.mean[l], rstd=self.rstd[l],
                               a_row0=row0, c_off=off, y_off=off, m_off=t * N)
            else:
                planes.gemm(Ap, planes.weight(W), pre, U, b, N, U, a_row0=row0, c_off=off)
            if not fuse:
                _ln_fwd(pre.data_ptr() + 4 * off, gamma, beta, (y.data_ptr() + 4 * off) if y is not None else None, self.mean[l].data_ptr() + 4 * t * N,
                        self.rstd[l].data_ptr() + 4 * t * N, N, U, eps, self.yp[l], row0)
            Ap = self.yp[l]
        if out is None:               # the caller runs the output layer fused with the Normal head (ActorTape.head_fused)
            return None
        A2, Kx = self.head_w.shape
        sgemm(self.y[-1], Kx, 1, self.head_w, Kx, 1, out, A2, self.head_b, N, A2, Kx, a_off=t * N * Kx)
        return out

    def _backward(self):
        assert self.inputs is not None, 'ActorTape.inputs (time-major rollout states) not set'
        H, N = self.H, self.N
        M = H * N
        dev = self.d_raw.device
        A2, U = self.head_w.shape
        d = self.d_raw.reshape(M, A2)
        x_last = self.y[-1]
        dWh, dbh = self.head_param_grads(d, x_last)
        dy = torch.empty(M, U, device=dev)
        sgemm(d, A2, 1, self.head_w, 1, U, dy, U, None, M, U, A2)
        grads = [None] * len(self.layers)
        dpre_p = None
        for l in range(len(self.layers) - 1, -1, -1):
            W, b, gamma, beta, eps = self.layers[l]
            U, K = W.shape
            # weight gradients: on the same planes through the transposing kernel (genrl_gemm_h2_tn) from TN_MIN_ROWS rows up
            tn = planes.tn_ok(M, U, K, K)
            if l == 0:
                sp_ = getattr(self, 'state_planes', None)
                tn = tn and sp_ is not None and self.inputs[0].shape[-1] % 4 == 0
            # the fp32 copy of the pre-activation gradient has one reader, the fp32-operand weight-gradient kernel: with that product on
            # planes the LayerNorm backward writes planes only (as _TrunkPlanes.backward), where its kernel writes planes itself
            planes_only = tn and 256 < U <= 4096 and U % 4 == 0
            dpre = None if planes_only else torch.empty(M, U, device=dev)
            if dpre_p is None or dpre_p.cols != U:
                dpre_p = planes.Planes(M, U, dev)
            g0, g1, g2, ws, acc_p, direct = _ln_param_targets(M, U, gamma, beta, b, dev, bias_optional=True)
            _ln_bwd(_p(dy), _p(self.pre[l]), gamma, beta, _p(self.mean[l]), _p(self.rstd[l]), _p(dpre), M, U, dpre_p, 0,
                    g0, g1, g2, ws, acc_p)
            tw, acc, dW = _wgrad_target(W)
            if l > 0:
                x = self.y[l - 1]
                if tn:
                    planes.gemm_tn(dpre_p, self.yp[l - 1], tw, K, U, K, M, accumulate=acc)
                else:
                    # (_keeps_y decided at construction with the same tn_ok: the two can part only if the switches changed in between)
                    assert x is not None, 'the fp32 input of a weight gradient on the fp32-operand kernel was not kept (tn_ok changed since the tape was built)'
                    sgemm(dpre, 1, U, x, 1, K, tw, K, None, U, K, M, accumulate=acc)
                dy = torch.empty(M, K, device=dev)
                planes.gemm(dpre_p, planes.weight(W, transpose=True), dy, K, None, M, K)
            else:
                x1, x2 = self.inputs
                K1, K2 = x1.shape[-1], x2.shape[-1]
                assert x1.is_contiguous() and x2.is_contiguous() and x1.shape[0] >= H and K1 + K2 == K
                if tn:
                    planes.gemm_tn(dpre_p, sp_[0], tw, K, U, K1, M, accumulate=acc)
                    planes.gemm_tn(dpre_p, sp_[1], tw, K, U, K2, M, accumulate=acc, c_off=K1)
                else:
                    sgemm(dpre, 1, U, x1, 1, K1, tw, K, None, U, K1, M, accumulate=acc)
                    sgemm(dpre, 1, U, x2, 1, K2, tw, K, None, U, K2, M, c_off=K1, accumulate=acc)
            grads[l] = (dW, None if (direct or b is None) else g2, None if direct else g0,
                        None if direct else g1)
        return dWh, dbh, grads


class _RolloutPlanes(Function):
    """ops._Rollout on plane operands.  Returns time-major stoch (H+1,N,S,K), deter (H+1,N,D), logit (H+1,N,S,K),
    action (H+1,N,A), raw (H,N,2A)."""
    @staticmethod
    def forward(ctx, stoch0, deter0, logit0, eps, q, spec, head_w, head_b, *actor_params):
        ctx.set_materialize_grads(False)
        sp, tape = spec, spec.tape
        dev = deter0.device
        dims, bufs, eps, q = ops._rollout_buffers(stoch0, deter0, logit0, eps, q, sp, tape)
        H, N, S, K, D, A, U, AP = dims
        stoch, deter, logit, action, raws, x_pre, g_pre, o_pre, st = bufs
        SK = S * K
        f = lambda *shape: torch.empty(*shape, device=dev)
        # planes of every GEMM operand, rows h*N + n
        stoch_p, deter_p = planes.Planes((H + 1) * N, SK, dev), planes.Planes((H + 1) * N, D, dev)
        act_p = planes.Planes((H + 1) * N, A, dev)                 # (zero padded to 64 columns; row block 0 unused)
        x_p, o_p = planes.Planes(N, U, dev), planes.Planes(N, U, dev)      # consumed within the step: one row block
        planes.split(stoch[0], out=stoch_p); planes.split(deter[0], out=deter_p)
        # (x and o -- the img_in / img_out activations -- are consumed within the step as PLANES only: no fp32 copy is written where the
        # LayerNorm kernel can do without, 5.9 -> 5.4 us per launch at 1 024 rows)
        planes_only = 256 < U <= 4096 and U % 4 == 0
        x, o = (None, None) if planes_only else (f(N, U), f(N, U))
        w_in_s, w_in_a = planes.weight(sp.in_w, c0=0, c1=SK), planes.weight(sp.in_w, c0=SK, c1=SK + A)
        w_g_x, w_g_h = planes.weight(sp.gru_w, c0=0, c1=U), planes.weight(sp.gru_w, c0=U)
        w_out, w_dist = planes.weight(sp.out_w), planes.weight(sp.dist_w)
        pt = lambda t, off: t.data_ptr() + 4 * off
        L = lib()
        seq_c = ops.SEQ_C and planes.gemm_profile is None and len(tape.layers) <= ops._max_layers('genrl_rollout')
        # Dense -> LayerNorm -> SiLU as ONE launch where the shape allows (genrl_gemm_h2_ln: policy layers, img_in, img_out: 10 launches per step)
        fuse_any = planes.ln_fused_here(dev)                 # (per layer: genrl_gemm_h2_ln_ok(N, width), in C and in the Python twin alike)
        fuse_ln = fuse_any and planes.gemm_ln_ok(N, U, dev)
        if seq_c:
            # the H-step launch loop in C (csrc/seq.hip: genrl_imagine_seq_fwd -- the loop below, launch for launch, from one host call)
            common, layers = ops._rollout_fields(sp, tape, dims, bufs, x=x, o=o, eps=eps, q=q)
            a = fill(_cstruct('genrl_rollout')(), **common, stoch_p=stoch_p, deter_p=deter_p, act_p=act_p, x_p=x_p, o_p=o_p, w_in_s=w_in_s,
                     w_in_a=w_in_a, w_g_x=w_g_x, w_g_h=w_g_h, w_out=w_out, w_dist=w_dist)
            for l, fields in enumerate(layers):
                W_ = tape.layers[l][0]
                if l == 0:                # layer 0: the stoch / deter column blocks of its weight
                    fill(a, pw0s=planes.weight(W_, c0=0, c1=SK), pw0d=planes.weight(W_, c0=SK))
                else:
                    fill(a, at=l, pw=planes.weight(W_))
                fill(a, at=l, pyp=tape.yp[l], **fields)
            if fuse_any:
                sync_, part_ = planes._ln_workspace(dev)
                fill(a, ln_part=(part_.data_ptr() + 15) // 16 * 16, ln_sync=sync_.data_ptr())
            check(L.genrl_imagine_seq_fwd(a, _stream()), 'imagine_seq_fwd')
        for h in (() if seq_c else range(H)):
            r0, r1 = h * N, (h + 1) * N
            tape._forward_planes(h, stoch_p, deter_p, None)
            tape.head_fused(h, pt(eps, h * N * A), pt(raws, h * N * 2 * A), pt(action, r1 * AP), AP, sp.min_std, sp.max_std, act_p, r1)
            # img_in: [stoch_h | action_{h+1}] -> hidden, LN + SiLU
            if fuse_ln:
                planes.gemm_ln(stoch_p, w_in_s, x_pre, sp.in_b, N, U, sp.in_g, sp.in_be, sp.in_eps, x_p, 0, y=x, mean=st['xm'], rstd=st['xr'],
                               a_row0=r0, A1=act_p, B1=w_in_a, a1_row0=r1, c_off=h * N * U, m_off=r0)
            else:
                planes.gemm(stoch_p, w_in_s, x_pre, U, sp.in_b, N, U, a_row0=r0, A1=act_p, B1=w_in_a, a1_row0=r1, c_off=h * N * U)
                _ln_fwd(pt(x_pre, h * N * U), sp.in_g, sp.in_be, _p(x), pt(st['xm'], r0), pt(st['xr'], r0), N, U, sp.in_eps, x_p, 0)
            # GRU: [x | deter_h] W_g^T -> LN + gates -> deter_{h+1}
            planes.gemm(x_p, w_g_x, g_pre, 3 * D, None, N, 3 * D, A1=deter_p, B1=w_g_h, a1_row0=r0, c_off=h * N * 3 * D)
            check(L.genrl_gru_gates_fwd_h2(pt(g_pre, h * N * 3 * D), pt(deter, r0 * D), D, _p(sp.gru_g), _p(sp.gru_be),
                                           pt(deter, r1 * D), D, None, None, pt(st['gm'], r0), pt(st['gr'], r0), N, D, 1e-5,
                                           deter_p.ptr(r1), deter_p.ld, deter_p.plane, deter_p.inv_ptr(r1), _stream()),
                  'gru_gates_fwd_h2')
            # prior head: img_out (+LN+SiLU), dist, sample
            if fuse_ln:
                planes.gemm_ln(deter_p, w_out, o_pre, sp.out_b, N, U, sp.out_g, sp.out_be, sp.out_eps, o_p, 0, y=o, mean=st['om'], rstd=st['or'],
                               a_row0=r1, c_off=h * N * U, m_off=r0)
            else:
                planes.gemm(deter_p, w_out, o_pre, U, sp.out_b, N, U, a_row0=r1, c_off=h * N * U)
                _ln_fwd(pt(o_pre, h * N * U), sp.out_g, sp.out_be, _p(o), pt(st['om'], r0), pt(st['or'], r0), N, U, sp.out_eps, o_p, 0)
            if K == 32 and sp.dist_b is not None:
                # prior logits AND their sample in one launch: softmax -> unimix -> exponential race in the product's epilogue
                planes.gemm_sample(o_p, w_dist, logit, SK, sp.dist_b, N, SK, q, SK, UNIMIX, stoch, SK, stoch_p, c_off=r1 * SK,
                                   q_off=h * N * SK, s_off=r1 * SK, sp_row0=r1)
            else:
                planes.gemm(o_p, w_dist, logit, SK, sp.dist_b, N, SK, c_off=r1 * SK)
                check(L.genrl_onehot_fwd_h2(pt(logit, r1 * SK), pt(q, h * N * SK), pt(stoch, r1 * SK), None, N * S, K, UNIMIX,
                                            stoch_p.ptr(r1), SK, stoch_p.ld, stoch_p.plane, stoch_p.inv_ptr(r1), _stream()),
                      'onehot_fwd_h2')
        tape.state_planes = (stoch_p, deter_p)        # rows h*N + n: the heads evaluated on the rollout take them as operands
        return ops._rollout_outputs(ctx, sp, dims, bufs, eps)

    @staticmethod
    def backward(ctx, d_stoch, d_deter, d_logit, d_action, d_raws):
        sp, tape = ctx.sp, ctx.sp.tape
        stoch, deter, logit, raws, eps, x_pre, g_pre, o_pre, st = ctx.bufs
        H, N, S, K, D, A, U, AP = ctx.dims
        SK = S * K
        dev = deter.device
        f = lambda *shape: torch.empty(*shape, device=dev)
        ds, dd, dl_in, dact_all, dha, dhb = ops._rollout_upstream(ctx.dims, dev, d_stoch, d_deter, d_logit, d_action)
        # (d o_pre is consumed as planes only: the LayerNorm backward writes no fp32 copy of it where its kernel can do without)
        no_dx = 256 < U <= 4096 and U % 4 == 0
        # (d g_pre has plane readers only -- the two GRU dgrads -- and so has d logits unless an upstream logit gradient is accumulated into
        # its fp32 copy: neither is written in fp32 where the kernel writes the planes itself, csrc/dist.hip onehot_bwd_impl)
        no_dlg = dl_in is None and lib().genrl_onehot_bwd_planes_only_ok(K, SK) == 1
        dlg, do, do_pre, dx = (None if no_dlg else f(N, SK)), f(N, U), (None if no_dx else f(N, U)), f(N, U)
        # d x_pre of EVERY step: the head's backward, which nothing in the loop waits for, then runs once over all H N rows behind it
        dx_pre = f(H, N, U)
        dlg_p, dop_p, dg_p, dxp_p = planes.Planes(N, SK, dev), planes.Planes(N, U, dev), planes.Planes(N, 3 * D, dev), planes.Planes(N, U, dev)
        cur, nxt = dha, None
        # transposed weight planes: rows = the product's output columns
        wt_dist, wt_out = planes.weight(sp.dist_w, True), planes.weight(sp.out_w, True)
        wt_g_x, wt_g_h = planes.weight(sp.gru_w, True, 0, U), planes.weight(sp.gru_w, True, U)
        wt_in_s = planes.weight(sp.in_w, True, 0, SK)
        waT = sp.in_w.detach()[:, SK:SK + A].t().contiguous()            # (A, U): the action columns, for the fused head backward
        pt = lambda t, off: t.data_ptr() + 4 * off
        L = lib()
        seq_c = ops.SEQ_C and planes.gemm_profile is None
        if seq_c:
            # the dgrad chain's launch loop in C (csrc/seq.hip: genrl_imagine_seq_bwd -- the loop below, launch for launch)
            # (its forward fields are a subset of the rollout's; dg_pre and dx_pre stay NULL: planes only, and the slab per step instead)
            common, _ = ops._rollout_fields(sp, tape, ctx.dims, (None, deter, logit, None, raws, x_pre, g_pre, o_pre, st), eps=eps)
            a = _cstruct('genrl_rollout_bwd')()
            fill(a, **{n_: common[n_] for n_, _t in a._fields_ if n_ in common},
                 ds=ds, dd=dd, dl_in=dl_in, dact_all=dact_all, d_raw=tape.d_raw, dlg=dlg, dov=do, do_pre=do_pre, dx=dx, dx_pre_all=dx_pre,
                 dha=dha, dhb=dhb, waT=waT, dlg_p=dlg_p, dop_p=dop_p, dg_p=dg_p, dxp_p=dxp_p, wt_dist=wt_dist, wt_out=wt_out, wt_g_x=wt_g_x,
                 wt_g_h=wt_g_h, wt_in_s=wt_in_s)
            check(L.genrl_imagine_seq_bwd(a, _stream()), 'imagine_seq_bwd')
        for h in (() if seq_c else range(H - 1, -1, -1)):
            r0, r1 = h * N, (h + 1) * N
            if dl_in is not None:
                dlg.copy_(dl_in[h + 1])
            check(L.genrl_onehot_bwd_h2(pt(logit, r1 * SK), pt(ds, r1 * SK), _p(dlg), N * S, K, UNIMIX, int(dl_in is not None),
                                        dlg_p.ptr(), SK, dlg_p.ld, dlg_p.plane, dlg_p.inv_ptr(), _stream()), 'onehot_bwd_h2')
            planes.gemm(dlg_p, wt_dist, do, U, None, N, U)
            _ln_bwd(_p(do), pt(o_pre, h * N * U), sp.out_g, sp.out_be, pt(st['om'], r0), pt(st['or'], r0), _p(do_pre), N, U,
                    dop_p, 0)
            planes.gemm(dop_p, wt_out, dd, D, None, N, D, accumulate=True, c_off=r1 * D)
            # GRU: upstream = dd[h+1] (+ recurrent part from step h+1's GRU, held in `nxt`)
            check(L.genrl_gru_gates_bwd_h2(pt(dd, r1 * D), D, nxt.data_ptr() if nxt is not None else None, None,
                                           pt(g_pre, h * N * 3 * D), pt(deter, r0 * D), D, _p(sp.gru_g), _p(sp.gru_be),
                                           pt(st['gm'], r0), pt(st['gr'], r0), None, _p(cur), D, None, None, None, N, D,
                                           0, None, 0, 0, dg_p.ptr(), dg_p.ld, dg_p.plane, dg_p.inv_ptr(), _stream()),
                  'gru_gates_bwd_h2')
            # the two GRU dgrads share their A operand: one launch (d h accumulates into `cur`, d x overwrites)
            planes.gemm_pair(dg_p, wt_g_h, cur, D, D, True, wt_g_x, dx, U, U, False, N)
            _ln_bwd(_p(dx), pt(x_pre, h * N * U), sp.in_g, sp.in_be, pt(st['xm'], r0), pt(st['xr'], r0), pt(dx_pre, h * N * U), N, U,
                    dxp_p, 0)
            planes.gemm(dxp_p, wt_in_s, ds, SK, None, N, SK, accumulate=True, c_off=r0 * SK)
            nxt, cur = cur, (dhb if cur is dha else dha)
        if not seq_c:
            # d action_{h+1} = dx_pre W_a (+ upstream) and the head's backward -> d raw_h, all H steps in one launch (rows h N + n)
            check(L.genrl_actor_head_linear_bwd(_p(dx_pre), U, _p(waT), pt(dact_all, N * AP) if dact_all is not None else None, AP,
                                                _p(raws), _p(eps), _p(tape.d_raw), H * N, U, A, sp.min_std, sp.max_std, _stream()),
                  'actor_head_linear_bwd')
        return ops._rollout_param_grads(tape, d_raws)


# ---- the dense layer on [x1, x2] with plane operands: its three products, defined once for the nodes below (on fp32 operands: ops._dense2_*)

def _dense_fwd(M, in1, in2, W, b, pre, need_w, ln=None, act=1):
    """pre (M, N) = [x1, x2] W^T (+ b) and, with ln = (gamma, beta, eps, out_p, y, mean, rstd), y / out_p = act(LayerNorm(pre)) (y None: planes
    only; act: the GENRL_ACT_* code, 1 SiLU / 2 ELU).  in1 / in2: (fp32 rows, Planes | None, first row) of the inputs; fp32 rows of in2 None: one input.  The product runs on planes when
    every input comes with them -- with the LayerNorm and the activation in ONE launch where planes.gemm_ln_ok holds (row statistics exchanged inside one
    XCD's L2: genrl_gemm_h2_ln) -- else on the fp32 rows (ops._dense2_fwd).
    -> the inputs' ((P1, r1), (P2, r2)) for the node to keep, where the weight gradient (need_w: somebody wants it) will really take them
    (genrl_gemm_h2_tn); else None: the fp16 copies would live from forward to backward for nothing"""
    (a, Pa, ra), (c, Pb, rb) = in1, in2
    N, K = W.shape
    two = c is not None
    K1 = a.shape[1] if two else K
    on_planes = Pa is not None and (not two or Pb is not None)
    fused = on_planes and ln is not None and planes.gemm_ln_ok(M, N, pre.device)
    if on_planes:
        # (two inputs: ONE launch with two operand segments, the column blocks of W)
        w1 = planes.weight(W, c0=0, c1=K1)
        seg = dict(a_row0=ra, A1=Pb, B1=planes.weight(W, c0=K1), a1_row0=rb) if two else dict(a_row0=ra)
        if fused:
            gamma, beta, eps, out_p, y, mean, rstd = ln
            planes.gemm_ln(Pa, w1, pre, b, M, N, gamma, beta, eps, out_p, 0, y=y, mean=mean, rstd=rstd, act=act, **seg)
        else:
            planes.gemm(Pa, w1, pre, N, b, M, N, **seg)
    else:
        ops._dense2_fwd(a, c, W, b, pre)
    if ln is not None and not fused:
        gamma, beta, eps, out_p, y, mean, rstd = ln
        _ln_fwd(_p(pre), gamma, beta, _p(y), _p(mean), _p(rstd), M, N, eps, out_p, 0, act)
    keep = on_planes and need_w and planes.tn_ok(M, N, K1, K) and (not two or (K - K1) % 4 == 0) and ra % 4 == 0 and rb % 4 == 0
    return ((Pa, ra), (Pb, rb)) if keep else None


def _dense_dgrad(dpre_p, W, K1, need1, need2):
    """-> (d1, d2) = dpre W[:, :K1] (M, K1), dpre W[:, K1:] (M, K - K1) from the planes of dpre and the transposed weight planes; None where
    not needed"""
    M, K2 = dpre_p.rows, W.shape[1] - K1
    d1 = d2 = None
    if need1:
        d1 = torch.empty(M, K1, device=W.device)
        planes.gemm(dpre_p, planes.weight(W, True, 0, K1), d1, K1, None, M, K1)
    if need2:
        d2 = torch.empty(M, K2, device=W.device)
        planes.gemm(dpre_p, planes.weight(W, True, K1), d2, K2, None, M, K2)
    return d1, d2


def _dense_wgrad(dpre_p, dpre, ip, a, c, W):
    """dW = dpre^T [x1, x2], written or added where _wgrad_target says: genrl_gemm_h2_tn on the planes of dpre and the input planes the node
    kept (ip: what _dense_fwd returned), else -- ip None -- the fp32-operand kernels on dpre and the inputs' fp32 rows (ops._dense2_wgrad).
    c None: one input.  -> what the node returns to autograd for W"""
    if ip is None:
        return ops._dense2_wgrad(dpre, a, c, W)
    (N, K), M, K1 = W.shape, dpre_p.rows, ip[0][0].cols
    tgt, acc, dW = _wgrad_target(W)
    planes.gemm_tn(dpre_p, ip[0][0], tgt, K, N, K1, M, accumulate=acc, b_row0=ip[0][1])
    if c is not None:
        planes.gemm_tn(dpre_p, ip[1][0], tgt, K, N, K - K1, M, accumulate=acc, b_row0=ip[1][1], c_off=K1)
    return dW


class _LinearPlanes(Function):
    """ops._Linear (y = x W^T + b) with the forward and dgrad products on plane operands: P = (Planes of x, first row) when
    the caller has them (a rollout's states), else x is split here; the dgrad splits dy.  Weight / bias gradients: fp32-operand
    kernels (ops.sgemm / colsum), as everywhere."""
    @staticmethod
    def forward(ctx, x, W, b, P, r0):
        x2 = _f32(x).reshape(-1, x.shape[-1]).contiguous()
        M, K = x2.shape
        N = W.shape[0]
        if P is None:
            P, r0 = planes.split(x2), 0
        Np = (N + 3) // 4 * 4            # (255-bin two-hot heads: rows padded to 256 floats, the caller gets a column slice)
        y = torch.empty(M, Np, device=x.device)
        planes.gemm(P, planes.weight(W), y, Np, b, M, N, a_row0=r0)
        ctx.save_for_backward(x2, W)
        ctx.bias = b
        ctx.xshape = x.shape
        ctx.in_planes = (P, r0) if (ctx.needs_input_grad[1] and planes.tn_ok(M, N, K, K) and r0 % 4 == 0) else None
        return (y if Np == N else y[:, :N]).view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, W = ctx.saved_tensors
        M, K = x2.shape
        N = W.shape[0]
        b = ctx.bias
        dy2, ldy = ops._rows_ld(dy.reshape(M, N))        # (a gradient arriving in padded rows is read in place)
        dx = dW = db = None
        tn = ctx.needs_input_grad[1] and ctx.in_planes is not None and planes.tn_ok(M, N, K, K)
        dyp = planes.split(dy2) if (ctx.needs_input_grad[0] or tn) else None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=dy.device)
            planes.gemm(dyp, planes.weight(W, transpose=True), dx, K, None, M, K)
            dx = dx.reshape(ctx.xshape)
        if ctx.needs_input_grad[1]:
            tgt, acc, dW = _wgrad_target(W)
            if tn:
                planes.gemm_tn(dyp, ctx.in_planes[0], tgt, K, N, K, M, accumulate=acc, b_row0=ctx.in_planes[1])
            else:
                sgemm(dy2, 1, ldy, x2, 1, K, tgt, K, None, N, K, M, accumulate=acc)
        if b is not None and ctx.needs_input_grad[2]:
            db = _bias_grad(b, dy2, ldy)
        return dx, dW, db, None, None


def linear(x, W, b=None, planes_of_x=None):
    """planes_of_x = (Planes handle, first row) of x's rows, if the caller has them"""
    P, r0 = planes_of_x if planes_of_x is not None else (None, 0)
    M = x.numel() // x.shape[-1]
    if P is not None and (P.cols != x.shape[-1] or r0 + M > P.rows):
        P, r0 = None, 0
    return _LinearPlanes.apply(x, W, b, P, r0)


# rows from which products run on plane operands.  Round 5 (profiles/r05_minrows_ab.txt, whole step, one box): at 384 / 400 rows the plane
# rollout's 16 + 10 launches per step beat the fp32-operand rollout's 20 + 14 by 15 % / 7 % (17.0 -> 14.5 ms at 12 sequences of c2,
# 13.9 -> 12.9 at the 8 x 50 per-rank batch of c3 under DP-8), at 256 rows by 8-12 % (c5 9.4 -> 8.5 ms, c2 at 8 sequences 13.6 -> 12.5).
# Round 6 takes the measured win (round-5 verdict item 2; profiles/r06_minrows_ab.txt, one box: c5 9.5 -> 8.5 ms, c2 at 8 sequences = 256 rows
# 13.1 -> 12.2, at 6 sequences = 192 rows 12.1 -> 11.4; at 4 sequences = 128 rows the fp32-operand kernels still win, 10.0 against 10.5): plane
# operands from 192 rows.  With them one of the 8 192 sampled latents of the 256-row full-width c5 case falls on the other side of a near-tie
# -- the flip rate (1.2e-4) the suite accepts for c3 / c4 (< 2e-3) -- and GENRL_PLANES_MIN_ROWS=320 (or any larger value) is the explicit
# switch back to the exact-fp32 operands at that size (tests/test_gpu_fullsize.py runs the c5 case both ways).
MIN_ROWS_PLANES = 192


def min_rows():
    """rows from which the plane-operand path is used (GENRL_PLANES_MIN_ROWS overrides: the parity tests run it at tiny sizes)"""
    import os
    return int(os.environ.get('GENRL_PLANES_MIN_ROWS', MIN_ROWS_PLANES))


def _input_handles(x1, x2, planes_, both_or_none):
    """(P1, r1), (P2, r2) of dense_ln_act's / dense_act's inputs: the caller's ((P1, row0), (P2, row0) | None), else the inputs' own `_planes`
    attribute (a previous layer's output); dropped where they do not cover the rows.  A second input that comes without: both_or_none (the
    LayerNorm layers, whose product then runs on the fp32 rows) drops the first input's too; the norm-free layer keeps them and splits the second"""
    M = x1.numel() // x1.shape[-1]
    if planes_ is None:
        h1 = getattr(x1, '_planes', None)
        h2 = getattr(x2, '_planes', None) if x2 is not None else None
    else:
        h1, h2 = planes_[0], (planes_[1] if len(planes_) > 1 else None)
    if h1 is not None and (h1[0].cols != x1.shape[-1] or h1[1] + M > h1[0].rows):
        h1 = None
    if x2 is not None and h2 is not None and (h2[0].cols != x2.shape[-1] or h2[1] + M > h2[0].rows):
        h2 = None
    if both_or_none and x2 is not None and h2 is None:
        h1 = None
    return (h1 if h1 is not None else (None, 0)), (h2 if h2 is not None else (None, 0))


def dense_ln_act(x1, x2, W, b, gamma, beta, eps=1e-5, planes=None, act='SiLU'):
    """y = act(LayerNorm([x1, x2] W^T + b)), act 'SiLU' / 'ELU'  (ops.dense_ln_act, agent/dreamer_utils.py:739-747) on plane operands: a trunk of one layer.
    -> y with y._planes = (planes of y, 0) for the next layer.  planes = ((P1, row0), (P2, row0) | None) of the inputs when the caller has them
    (rollout states); otherwise the inputs' own `_planes` attribute (a previous layer's output) is used."""
    return dense_ln_trunk(x1, x2, [(W, b, gamma, beta, eps)], planes=planes, act=act)


class _TrunkPlanes(Function):
    """A chain of layers y = act(LayerNorm([x1, x2] W^T + b)), one activation (SiLU or ELU, by its code) for the chain (ops._DenseLNAct; an MLP trunk: agent/dreamer_utils.py:739-747) with plane
    operands as ONE autograd node, the way ActorTapePlanes treats the policy.  Per layer: the forward product runs on planes when the inputs
    come with them, the output's planes are written by the LayerNorm kernel, the backward's dgrad products use the planes its LayerNorm
    backward emits and the transposed weight planes, the weight gradient the kept input planes or the fp32-operand kernels (_dense_fwd /
    _dense_dgrad / _dense_wgrad).  The same launches in the same order, forward and backward, as a chain of one-layer nodes -- bit-identical
    outputs and gradients, the same accumulation order into the flat gradient buffers -- but a hidden layer's output is consumed inside the
    node, as planes, so its fp32 copy is written only where somebody reads it: the NEXT layer's weight gradient while it stays on the fp32-operand
    kernel (below planes.tn_min_rows() rows), or a LayerNorm kernel that cannot write planes without it.  No tensor with undefined contents
    leaves the node: the caller gets the last layer's fp32 output alone.  params: (W, b, gamma, beta) per layer; out_ps: the output planes
    per layer; P1 / P2 (+ first rows): the planes of layer 0's inputs, or None."""
    @staticmethod
    def forward(ctx, x1, x2, P1, r1, P2, r2, eps, act, out_ps, *params):
        ctx.act = act
        a = _f32(x1).reshape(-1, x1.shape[-1]).contiguous()
        c = _f32(x2).reshape(-1, x2.shape[-1]).contiguous() if x2 is not None else None
        M, K1 = a.shape
        K2 = c.shape[1] if c is not None else 0
        L = len(out_ps)
        dev = a.device
        needs_w = [ctx.needs_input_grad[9 + 4 * l] for l in range(L)]
        pres, means, rstds, ys, in_planes = [], [], [], [], []
        for l in range(L):
            W, b, gamma, beta = params[4 * l:4 * l + 4]
            N, K = W.shape
            if l == 0:
                assert K == K1 + K2
                in1, in2 = (a, P1, r1), (c, P2, r2)
            else:
                in1, in2 = (None, out_ps[l - 1], 0), (None, None, 0)
            # the fp32 copy of this layer's output: the node's result (last layer), else see the class comment
            keep_y = l == L - 1 or not (256 < N <= 4096 and N % 4 == 0
                                        and (not needs_w[l + 1] or planes.tn_ok(M, params[4 * (l + 1)].shape[0], N, N)))
            pre = torch.empty(M, N, device=dev)
            y = torch.empty(M, N, device=dev) if keep_y else None
            mean = torch.empty(M, device=dev); rstd = torch.empty(M, device=dev)
            in_planes.append(_dense_fwd(M, in1, in2, W, b, pre, needs_w[l], (gamma, beta, eps[l], out_ps[l], y, mean, rstd), ctx.act))
            pres.append(pre); means.append(mean); rstds.append(rstd); ys.append(y)
        ctx.save_for_backward(a, c if c is not None else a.new_empty(0), *params[0::4], *params[2::4], *params[3::4])
        ctx.biases = list(params[1::4])
        ctx.has2, ctx.L = c is not None, L
        ctx.pres, ctx.means, ctx.rstds, ctx.in_planes = pres, means, rstds, in_planes
        ctx.hidden_y = ys[:-1]                  # fp32 copies of the hidden activations that have a reader (None: planes only)
        ctx.shapes = (x1.shape, x2.shape if x2 is not None else None)
        return ys[-1].reshape(*x1.shape[:-1], ys[-1].shape[1])

    @staticmethod
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        L = ctx.L
        a, c = saved[0], saved[1]
        Ws, gammas, betas = saved[2:2 + L], saved[2 + L:2 + 2 * L], saved[2 + 2 * L:2 + 3 * L]
        ng = ctx.needs_input_grad
        M, K1_0 = a.shape
        dev = dy.device
        out = [None] * (9 + 4 * L)
        dyl = dy.reshape(M, Ws[-1].shape[0]).contiguous()
        for l in range(L - 1, -1, -1):
            W, gamma, beta, b = Ws[l], gammas[l], betas[l], ctx.biases[l]
            N, K = W.shape
            has2 = l == 0 and ctx.has2
            K1 = K1_0 if l == 0 else K
            K2 = K - K1
            need_w, need_b, need_g = ng[9 + 4 * l], ng[10 + 4 * l], ng[11 + 4 * l]
            # (what the per-layer chain's node sees as its input's requires_grad: anything upstream of this layer that wants a gradient)
            need_x1 = ng[0] if l == 0 else (ng[0] or ng[1] or any(ng[9:9 + 4 * l]))
            ip = ctx.in_planes[l]
            use_tn = ip is not None and planes.tn_ok(M, N, K1, K) and (not has2 or K2 % 4 == 0)
            planes_only = 256 < N <= 4096 and N % 4 == 0          # (the LayerNorm kernels that write planes themselves)
            dpre = torch.empty(M, N, device=dev) if ((need_w and not use_tn) or not planes_only) else None
            dpre_p = planes.Planes(M, N, dev)
            need_p = need_w or need_b or need_g
            g0, g1, g2, ws, acc_p, direct = _ln_param_targets(M, N, gamma, beta, b, dev, need=need_p)
            _ln_bwd(_p(dyl), _p(ctx.pres[l]), gamma, beta, _p(ctx.means[l]), _p(ctx.rstds[l]), _p(dpre), M, N, dpre_p, 0, g0, g1, g2, ws, acc_p,
                    ctx.act)
            d1, d2 = _dense_dgrad(dpre_p, W, K1, need_x1, has2 and ng[1])
            dW = None
            if need_w:
                xin = a if l == 0 else ctx.hidden_y[l - 1]
                assert use_tn or xin is not None, 'the fp32 input of a weight gradient on the fp32-operand kernel was not kept'
                dW = _dense_wgrad(dpre_p, dpre, ip if use_tn else None, xin, c if has2 else None, W)
            if need_p and not direct:
                out[9 + 4 * l:13 + 4 * l] = [dW, (g2 if b is not None else None), g0, g1]
            else:
                out[9 + 4 * l] = dW
            if l == 0:
                out[0], out[1] = ops._as(d1, ctx.shapes[0]), ops._as(d2, ctx.shapes[1])
            dyl = d1
            if dyl is None:          # (nothing upstream wants a gradient: the per-layer chain stops here too)
                break
        return tuple(out)


def dense_ln_trunk(x1, x2, layers, planes=None, act='SiLU'):
    """layers: [(W, b, gamma, beta, eps), ...] of a Dense -> LayerNorm -> act ('SiLU' / 'ELU') chain whose first layer reads [x1, x2] (x2 may be None).
    -> the last layer's output, with its `_planes` for the head's product; the same values and gradients as dense_ln_act layer by layer
    (see _TrunkPlanes); `planes` as dense_ln_act's"""
    M = x1.numel() // x1.shape[-1]
    (P1, r1), (P2, r2) = _input_handles(x1, x2, planes, True)
    out_ps = [pl.Planes(M, l[0].shape[0], x1.device) for l in layers]
    flat = [q for l in layers for q in l[:4]]
    y = _TrunkPlanes.apply(x1, x2, P1, r1, P2, r2, [float(l[4]) for l in layers], ops.act_layer_code(act), out_ps, *flat)
    y._planes = (out_ps[-1], 0)
    return y


class _DenseActPlanes(Function):
    """ops._DenseAct (y = act([x1, x2] W^T), act SiLU or ELU by its code: a norm-free layer of conf/defaults/dreamer_v2.yaml) with plane operands: the product
    runs on the inputs' planes (P1 / P2 with their first rows: a previous layer's output or a rollout's states; inputs that come without
    are split here), genrl_silu_fwd_h2 / genrl_elu_fwd_h2 writes the output's planes (out_p) for the next product, the backward's _bwd_h2 emits
    the planes of the pre-activation gradient for the dgrad products (transposed weight planes) and, where planes.tn_ok holds, for the
    weight gradient through genrl_gemm_h2_tn; below that the weight gradient stays on the fp32-operand kernels."""
    @staticmethod
    def forward(ctx, x1, x2, W, P1, r1, P2, r2, out_p, act=1):
        a = _f32(x1).reshape(-1, x1.shape[-1]).contiguous()
        c = _f32(x2).reshape(-1, x2.shape[-1]).contiguous() if x2 is not None else None
        M, K1 = a.shape
        K2 = c.shape[1] if c is not None else 0
        N, K = W.shape
        assert K == K1 + K2
        if P1 is None:
            P1, r1 = planes.split(a.detach()), 0
        if c is not None and P2 is None:
            P2, r2 = planes.split(c.detach()), 0
        pre = torch.empty(M, N, device=a.device)
        ctx.in_planes = _dense_fwd(M, (a, P1, r1), (c, P2, r2), W, None, pre, ctx.needs_input_grad[2])
        y = torch.empty_like(pre)
        ops.act_fwd_raw(act, pre, y, M, N, out_p)
        ctx.act = act
        ctx.save_for_backward(a, c if c is not None else a.new_empty(0), W, pre)
        ctx.has2 = c is not None
        ctx.shapes = (x1.shape, x2.shape if x2 is not None else None)
        return y.reshape(*x1.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        a, c, W, pre = ctx.saved_tensors
        M, K1 = a.shape
        N = W.shape[0]
        dpre = torch.empty_like(pre)
        dpre_p = planes.Planes(M, N, dy.device)
        ops.act_bwd_raw(ctx.act, _f32(dy).reshape(M, N).contiguous(), pre, dpre, M, N, dpre_p)
        d1, d2 = _dense_dgrad(dpre_p, W, K1, ctx.needs_input_grad[0], ctx.has2 and ctx.needs_input_grad[1])
        dW = _dense_wgrad(dpre_p, dpre, ctx.in_planes, a, c if ctx.has2 else None, W) if ctx.needs_input_grad[2] else None
        return ops._as(d1, ctx.shapes[0]), ops._as(d2, ctx.shapes[1]), dW, None, None, None, None, None, None


def dense_act(x1, x2, W, planes=None, act='SiLU'):
    """-> y = act([x1, x2] W^T), act 'SiLU' / 'ELU', with y._planes = (planes of y, 0) for the next layer; `planes` as dense_ln_act's"""
    M = x1.numel() // x1.shape[-1]
    (P1, r1), (P2, r2) = _input_handles(x1, x2, planes, False)
    out_p = pl.Planes(M, W.shape[0], x1.device)
    y = _DenseActPlanes.apply(x1, x2, W, P1, r1, P2, r2, out_p, ops.act_layer_code(act))
    y._planes = (out_p, 0)
    return y


def imagine_rollout(stoch0, deter0, logit0, eps, q, spec):
    tape = spec.tape
    flat = [qq for l in tape.layers for qq in l[:4]]
    return _RolloutPlanes.apply(stoch0, deter0, logit0, eps, q, spec, tape.head_w, tape.head_b, *flat)


# ---- the Plan2Explore ensemble (agent/plan2explore.py:8-41): members of Linear([obs, action]) -> ReLU -> Linear
def _member_route(M, D=0):
    """plane operands for the member products?  (as everywhere: from min_rows() rows up while the plane path is on -- a precision-16
    agent has switched it off, and the fp32-operand kernels then round to bf16 themselves; an observation width D that is no multiple of 4
    -- continuous latents with `stoch: 30` -- stays on the fp32-operand kernels, whose scalar-load form takes any width)"""
    return pl.ENABLED and M >= min_rows() and D % 4 == 0


class EnsembleInputs:
    """[obs, action] rows of an ensemble call, prepared ONCE for all members: contiguous fp32 rows and, on the plane route, their planes
    (the action block is a second operand segment, zero padded to 64 columns: no concatenated copy)"""
    def __init__(self, obs, action, on_planes=None):
        self.obs = _f32(obs).reshape(-1, obs.shape[-1]).contiguous()
        self.act = _f32(action.detach()).reshape(-1, action.shape[-1]).contiguous()
        ops._on_gpu(self.obs, self.act)
        self.M, self.D = self.obs.shape
        self.A = self.act.shape[1]
        assert self.act.shape[0] == self.M
        self.on_planes = _member_route(self.M, self.D) if on_planes is None else on_planes
        self.Po = pl.split(self.obs.detach()) if self.on_planes else None
        self.Pa = pl.split(self.act) if self.on_planes else None


def _member_fwd(inp, W0, b0, W2, b2, out=None):
    """-> h = relu([obs, act] W0^T + b0) (M x H), its planes (plane route), out = h W2^T + b2 (M x E; into `out` if given)"""
    M, D, A = inp.M, inp.D, inp.A
    H, E = W0.shape[0], W2.shape[0]
    dev = inp.obs.device
    h = torch.empty(M, H, device=dev)
    out = out if out is not None else torch.empty(M, E, device=dev)
    if inp.on_planes:
        Ph = pl.Planes(M, H, dev)
        pl.gemm(inp.Po, pl.weight(W0, c0=0, c1=D), h, H, b0, M, H, A1=inp.Pa, B1=pl.weight(W0, c0=D))
        ops.relu_fwd_raw(h, h, M, H, Ph)
        pl.gemm(Ph, pl.weight(W2), out, E, b2, M, E)
        return h, Ph, out
    w1, ld1 = ops._aligned_block(W0, D, M)
    sgemm(inp.obs, D, 1, w1, ld1, 1, h, H, b0, M, H, D)
    sgemm(inp.act, A, 1, W0, D + A, 1, h, H, None, M, H, A, accumulate=True, b_off=D)
    ops.relu_fwd_raw(h, h, M, H)
    sgemm(h, H, 1, W2, H, 1, out, E, b2, M, E, H)
    return h, None, out


def _member_dgrad(inp, W0, W2, dp, dPp, p_row0, h, dobs=None, accumulate=False, c_off=0):
    """dh = dp W2 -> ReLU backward (in `dh`, + planes on the plane route) -> optionally dobs (+)= dpre W0[:, :D].  dPp: planes of dp from row
    p_row0 (plane route; dp may then be None).  -> dpre, its planes"""
    M, D = inp.M, inp.D
    H, E = W0.shape[0], W2.shape[0]
    dev = h.device
    dh = torch.empty(M, H, device=dev)
    if inp.on_planes:
        Ppre = pl.Planes(M, H, dev)
        pl.gemm(dPp, pl.weight(W2, transpose=True), dh, H, None, M, H, a_row0=p_row0)
        ops.relu_bwd_raw(dh, h, dh, M, H, Ppre)
        if dobs is not None:
            pl.gemm(Ppre, pl.weight(W0, True, 0, D), dobs, D, None, M, D, accumulate=accumulate, c_off=c_off)
        return dh, Ppre
    sgemm(dp, E, 1, W2, 1, H, dh, H, None, M, H, E)
    ops.relu_bwd_raw(dh, h, dh, M, H)
    if dobs is not None:
        w1, ld1 = ops._aligned_block(W0, D, M)
        sgemm(dh, H, 1, w1, 1, ld1, dobs, D, None, M, D, H, accumulate=accumulate, c_off=c_off)
    return dh, None


class _MemberMLP(Function):
    """One ensemble member on [obs, action]: out = relu([obs, act] W0^T + b0) W2^T + b2, or -- with `target` -- its prediction error
    ||target - out||_2 per row in the same node (agent/plan2explore.py:24-29), so that the error's backward hands the planes of d out
    straight to the dgrad and weight-gradient products.  Products: plane operands (genrl_gemm_h2, weight gradients genrl_gemm_h2_tn where
    planes.tn_ok holds) or the fp32-operand kernels, per EnsembleInputs.on_planes."""
    @staticmethod
    def forward(ctx, obs, W0, b0, W2, b2, inp, target):
        h, Ph, out = _member_fwd(inp, W0, b0, W2, b2)
        M, E = out.shape
        ctx.inp, ctx.Ph, ctx.params = inp, Ph, (W0, b0, W2, b2)
        if target is None:
            ctx.save_for_backward(h)
            ctx.err = False
            return out.reshape(*obs.shape[:-1], E)
        t = _f32(target.detach()).reshape(M, E).contiguous()
        err = torch.empty(M, device=out.device)
        check(lib().genrl_l2err_fwd(_p(t), E, _p(out), E, _p(err), M, E, _stream()), 'l2err_fwd')
        ctx.save_for_backward(h, t, out, err)
        ctx.err = True
        return err

    @staticmethod
    def backward(ctx, g):
        inp, Ph = ctx.inp, ctx.Ph
        W0, b0, W2, b2 = ctx.params
        M, D, A = inp.M, inp.D, inp.A
        H, E = W0.shape[0], W2.shape[0]
        dev = g.device
        on_planes = inp.on_planes
        if ctx.err:
            h, t, out, err = ctx.saved_tensors
            dp = torch.empty(M, E, device=dev)
            dPp = pl.Planes(M, E, dev) if on_planes else None
            ops.l2err_bwd_raw(_f32(g).reshape(M).contiguous(), err, t, out, dp, M, E, dPp)
        else:
            h, = ctx.saved_tensors
            dp = _f32(g).reshape(M, E).contiguous()
            dPp = pl.split(dp) if on_planes else None
        dW0 = db0 = dW2 = db2 = dobs = None
        if ctx.needs_input_grad[3]:
            tgt, acc, dW2 = _wgrad_target(W2)
            if on_planes and pl.tn_ok(M, E, H, H):
                pl.gemm_tn(dPp, Ph, tgt, H, E, H, M, accumulate=acc)
            else:
                sgemm(dp, 1, E, h, 1, H, tgt, H, None, E, H, M, accumulate=acc)
        if ctx.needs_input_grad[4]:
            db2 = _bias_grad(b2, dp)
        if ctx.needs_input_grad[0]:
            dobs = torch.empty(M, D, device=dev)
        dpre, Ppre = _member_dgrad(inp, W0, W2, dp, dPp, 0, h, dobs)
        if ctx.needs_input_grad[1]:
            tgt, acc, dW0 = _wgrad_target(W0)
            K0 = D + A
            if on_planes and pl.tn_ok(M, H, D, K0):
                pl.gemm_tn(Ppre, inp.Po, tgt, K0, H, D, M, accumulate=acc)
            elif on_planes and pl.tn_ok(M, H, D, D):
                # W0's rows are D + A floats apart -- 1542 at full width: not the 16-byte rows the split-K reduce stores -- so the
                # product lands in a compact (H, D) block and a strided copy adds it into place
                tmp = torch.empty(H, D, device=dev)
                pl.gemm_tn(Ppre, inp.Po, tmp, D, H, D, M)
                ops.copy2d(tmp, D, tgt, K0, H, D, accumulate=acc)
            else:
                sgemm(dpre, 1, H, inp.obs, 1, D, tgt, K0, None, H, D, M, accumulate=acc)
            sgemm(dpre, 1, H, inp.act, 1, A, tgt, K0, None, H, A, M, accumulate=acc, c_off=D)
        if ctx.needs_input_grad[2]:
            db0 = _bias_grad(b0, dpre)
        return (dobs.reshape(-1, D) if dobs is not None else None), dW0, db0, dW2, db2, None, None


def member_mlp(inp, W0, b0, W2, b2, target=None):
    """inp: EnsembleInputs.  -> prediction (M x E), or with `target` the row-wise L2 prediction error (M)"""
    return _MemberMLP.apply(inp.obs, W0, b0, W2, b2, inp, target)


def disagreement_chunk_rows():
    """rows of get_disagreement processed at a time (GENRL_P2E_CHUNK overrides): bounds its workspace, see _Disagreement"""
    return int(os.environ.get('GENRL_P2E_CHUNK', 4096))


class _Disagreement(Function):
    """r[m] = mean_e var_k member_k([obs, act])[m, e] (agent/plan2explore.py:33-41) for FROZEN members, in row chunks.

    r[m] depends on row m of obs alone, so d loss / d obs[m] = g[m] J[m] with J[m] = d r[m] / d obs[m]: the forward computes r AND J chunk by
    chunk (members' forward, variance, its backward with g = 1 emitting the planes of every d pred_k, the two dgrad products per member) and
    drops every activation at the chunk's end; the backward is one row scaling.  Nothing of size rows x 6144 outlives a chunk: at most
    (3 K + 2) blocks of C x max(E, H) floats are live for C chunk rows whatever the row count (K predictions, K hidden activations, the
    planes of K d pred, one d hidden + planes: 1.7 GB at K = 5, C = 4096, 6144 wide), plus J (rows x obs width).  The members' weights get no gradient here: the reference evaluates the reward with the ensemble frozen."""
    @staticmethod
    def forward(ctx, obs, act, K, *params):
        if any(ctx.needs_input_grad[3:]):
            raise ops.GenrlHipError('get_disagreement differentiates through frozen members only (train them through Disagreement.forward)')
        obs2 = _f32(obs).reshape(-1, obs.shape[-1]).contiguous()
        act2 = _f32(act).reshape(-1, act.shape[-1]).contiguous()
        M, D = obs2.shape
        dev = obs2.device
        need_j = ctx.needs_input_grad[0]
        r = torch.empty(M, device=dev)
        J = torch.empty(M, D, device=dev) if need_j else None
        on_planes = _member_route(M, D)
        C = disagreement_chunk_rows()
        E = params[2].shape[0]
        for c0 in range(0, M, C):
            c1 = min(M, c0 + C)
            n = c1 - c0
            inp = EnsembleInputs(obs2[c0:c1], act2[c0:c1], on_planes)
            preds = torch.empty(K, n, E, device=dev)
            hs = []
            for k in range(K):
                hs.append(_member_fwd(inp, *params[4 * k:4 * k + 4], out=preds[k])[0])
            ops.ens_var_fwd_raw(preds, r[c0:c1], K, n, E)
            if not need_j:
                continue
            dPp = pl.Planes(K * n, E, dev) if on_planes else None
            dp = None if on_planes else torch.empty(K, n, E, device=dev)
            ops.ens_var_bwd_raw(None, preds, dp, K, n, E, dPp)
            for k in range(K):
                W0, _, W2, _ = params[4 * k:4 * k + 4]
                _member_dgrad(inp, W0, W2, dp[k] if dp is not None else None, dPp, k * n, hs[k], J, accumulate=k > 0, c_off=c0 * D)
        if need_j:
            ctx.save_for_backward(J)          # (saved, not an attribute: a retained graph may run this backward again)
        ctx.oshape = obs.shape
        return r

    @staticmethod
    def backward(ctx, g):
        J, = ctx.saved_tensors
        return (J * g.reshape(-1, 1)).reshape(ctx.oshape), None, None, *([None] * (len(ctx.needs_input_grad) - 3))


def get_disagreement(obs, action, members):
    """members: [(W0, b0, W2, b2), ...] -> (rows,) disagreement; differentiable w.r.t. obs"""
    flat = [q for m in members for q in m]
    return _Disagreement.apply(obs, action.detach(), len(members), *flat)
