"""MI355X-native `agent/plan2explore.py`: Disagreement and Plan2Explore with the reference's API (mazpie/genrl
agent/plan2explore.py) on top of the HIP kernels.  Same constructor signatures, attribute / method / metric names and
state_dict keys (`disagreement.ensemble.{k}.{0,2}.{weight,bias}`); the ensemble's products and row kernels are
genrl_amd/ops_planes.py's member_mlp / get_disagreement (csrc/ensemble.hip).  Supported on the dreamer_v3 and dreamer_v2 defaults."""
import torch
import torch.nn as nn

from . import dreamer_utils as common
from .dreamer import DreamerAgent, env_reward, stop_gradient
from .. import ops, ops_planes


class Disagreement(common.Module):  # ref :8-41
    def __init__(self, obs_dim, action_dim, hidden_dim, n_models=5, pred_dim=None):
        super().__init__()
        if pred_dim is None:
            pred_dim = obs_dim
        # (parameter holders, as everywhere: their torch forward is never called)
        self.ensemble = nn.ModuleList([
            nn.Sequential(nn.Linear(obs_dim + action_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, pred_dim))
            for _ in range(n_models)
        ])

    def _members(self):
        return [(m[0].weight, m[0].bias, m[2].weight, m[2].bias) for m in self.ensemble]

    def forward(self, obs, action, next_obs):  # ref :18-31 -> (rows, n_models) prediction errors
        assert obs.shape[0] == next_obs.shape[0]
        assert obs.shape[0] == action.shape[0]
        inp = ops_planes.EnsembleInputs(obs, action)         # (the inputs' planes, once for all members)
        return torch.stack([ops_planes.member_mlp(inp, *m, target=next_obs) for m in self._members()], dim=1)

    def get_disagreement(self, obs, action):  # ref :33-41 -> (rows,)
        assert obs.shape[0] == action.shape[0]
        return ops_planes.get_disagreement(obs, action, self._members())


class Plan2Explore(DreamerAgent):  # ref :44-108
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        in_dim = self.wm.inp_size
        pred_dim = self.wm.embed_dim
        self.hidden_dim = pred_dim
        self.reward_free = True

        self.disagreement = Disagreement(in_dim, self.act_dim, self.hidden_dim, pred_dim=pred_dim).to(self.device)

        # optimizers
        self.disagreement_opt = common.Optimizer('disagreement', self.disagreement.parameters(), **self.cfg.model_opt,
                                                 use_amp=self._use_amp)
        self.disagreement.train()
        self.requires_grad_(requires_grad=False)

    def update_disagreement(self, obs, action, next_obs, step):  # ref :60-71
        metrics = dict()
        error = self.disagreement(obs, action, next_obs)
        loss = ops.wmean(error, None, 1.0)
        metrics.update(self.disagreement_opt(loss, self.disagreement.parameters()))
        metrics['disagreement_loss'] = loss.detach()          # (a device scalar, like every metric here: no host sync)
        return metrics

    def compute_intr_reward(self, seq):  # ref :73-84
        obs, action = seq['feat'][:-1], stop_gradient(seq['action'][1:])
        lead = list(action.shape[:-1])
        reward = self.disagreement.get_disagreement(obs.reshape(-1, obs.shape[-1]), action.reshape(-1, action.shape[-1]))
        reward = reward.reshape(lead + [1])
        # intr_rew[0] = 0, intr_rew[1:] = reward
        return torch.cat([torch.zeros([1] + lead[1:] + [1], device=reward.device), reward], 0)

    def update(self, data, step):  # ref :86-108
        B, T, _ = data['action'].shape
        state, outputs, metrics = self.update_wm(data, step)
        start = {k: stop_gradient(v) for k, v in outputs['post'].items()}
        if self.reward_free:
            T = T - 1
            inp = stop_gradient(outputs['feat'][:, :-1]).reshape(B * T, -1)
            action = data['action'][:, 1:].reshape(B * T, -1)
            out = stop_gradient(outputs['embed'][:, 1:]).reshape(B * T, -1)
            with common.RequiresGrad(self.disagreement):
                metrics.update(self.update_disagreement(inp, action, out, step))
            metrics.update(self._acting_behavior.update(self.wm, start, data['is_terminal'], reward_fn=self.compute_intr_reward))
        else:
            metrics.update(self._acting_behavior.update(self.wm, start, data['is_terminal'], lambda seq: env_reward(self, seq)))
        return state, metrics
