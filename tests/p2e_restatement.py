"""Plain-torch restatement of the Plan2Explore ensemble (mazpie/genrl agent/plan2explore.py), our own code: the yardstick of the
ensemble tests, in float32 or float64 (the dtype of what it is given).

  member:            Linear(obs_dim + action_dim, hidden) -> ReLU -> Linear(hidden, pred_dim)          (ref :12-16)
  forward:           errors[m, k] = || next_obs[m] - member_k(cat[obs, action])[m] ||_2                 (ref :18-31)
  get_disagreement:  var over the members (unbiased), mean over the features                            (ref :33-41)
  loss:              errors.mean()                                                                      (ref :63-65)
  intrinsic reward:  rows of feat[:-1] / action[1:], a zero first step                                  (ref :73-84)"""
import torch

import detgen


def member(x, W0, b0, W2, b2):
    return torch.relu(x @ W0.t() + b0) @ W2.t() + b2


def forward(obs, action, next_obs, members):
    x = torch.cat([obs, action], -1)
    return torch.cat([torch.norm(next_obs - member(x, *m), dim=-1, p=2, keepdim=True) for m in members], 1)


def get_disagreement(obs, action, members):
    x = torch.cat([obs, action], -1)
    return torch.var(torch.stack([member(x, *m) for m in members], 0), dim=0).mean(-1)


def intr_reward(feat, action, members):
    """feat (H+1, N, D), action (H+1, N, A) -> (H+1, N, 1)"""
    obs, act = feat[:-1], action[1:]
    r = get_disagreement(obs.reshape(-1, obs.shape[-1]), act.reshape(-1, act.shape[-1]), members)
    return torch.cat([torch.zeros_like(r[:feat.shape[1]]).reshape(1, -1, 1), r.reshape(obs.shape[0], -1, 1)], 0)


def member_names(k, prefix='disagreement.'):
    return [f'{prefix}ensemble.{k}.{i}.{w}' for i in (0, 2) for w in ('weight', 'bias')]


def members_from(sd, K=5, dtype=torch.float32, prefix='disagreement.', requires_grad=False):
    """[(W0, b0, W2, b2)] * K from a state dict"""
    conv = lambda t: torch.as_tensor(t).detach().cpu().to(dtype).clone().requires_grad_(requires_grad)
    return [tuple(conv(sd[n]) for n in member_names(k, prefix)) for k in range(K)]


def det_ensemble_state(K, obs_dim, action_dim, hidden, pred_dim, seed):
    """deterministic weights under the agent's state_dict names (detgen.det_param: uniform +-1/sqrt(fan_in))"""
    shapes = {}
    for k in range(K):
        n = member_names(k)
        shapes[n[0]], shapes[n[1]], shapes[n[2]], shapes[n[3]] = (hidden, obs_dim + action_dim), (hidden,), (pred_dim, hidden), (pred_dim,)
    return detgen.det_state_dict(shapes, seed)
