"""Plain-torch restatement of the discrete-action arithmetic (`discrete_actions`, `actor_grad: reinforce`): the one-hot head of the actor
(DistLayer 'onehot' -> OneHotDist: softmax, 1 % uniform mix, torch's renormalisation, log-probability, entropy) and the two actor objectives.
Written from the formulas, for any floating dtype: test_discrete_golden.py checks it against the reference's vectors, and
test_gpu_discrete_kernels.py uses it in float64 as the reference and in float32 as the yardstick of the kernels' error."""
import torch

UNIMIX = 0.01                                   # weight of the uniform part
EPS32 = 1.1920928955078125e-07                  # torch.finfo(float32).eps: the clamp of probs_to_logits in the precision the head runs in


def probs(logits, unimix=UNIMIX):
    K = logits.shape[-1]
    u = (1.0 - unimix) * torch.softmax(logits, -1) + unimix / K
    return u / u.sum(-1, keepdim=True)


def logp_ent(logits, action, unimix=UNIMIX):
    """-> log_prob(action) (action: one-hot rows), entropy()"""
    p = probs(logits, unimix)
    lg = torch.log(p.clamp(EPS32, 1.0 - EPS32))
    return (action * lg).sum(-1), -(p * lg).sum(-1)


def normed(x, offset_scale):
    return x if offset_scale is None else (x - offset_scale[0]) / offset_scale[1]


def reinforce_objective(target, baseline, logp, ent, weight, offset_scale, ent_scale):
    """target, baseline [H, N]; logp, ent, weight [H-1, N] (weight None: 1) -> loss, (mean, std of the normalised target)"""
    nt, nb = normed(target, offset_scale), normed(baseline, offset_scale)
    objective = logp * (nt[1:] - nb[1:]) + ent_scale * ent
    w = 1.0 if weight is None else weight
    return -(w * objective).mean(), (nt.mean(), nt.std())


def dynamics_objective(target, ent, weight, offset_scale, ent_scale):
    nt = normed(target, offset_scale)
    w = 1.0 if weight is None else weight
    return -(w * (nt[1:] + ent_scale * ent)).mean(), (nt.mean(), nt.std())
