"""Drop-in ``CustomMAEnv`` (custom/ma_customenv.py of the reference) backed by the HIP env.

Same constructor, attributes and reset()/step() dict API as the reference
(custom/ma_customenv.py:71-334), so ``util.create_custom_ma_env``, ``MADDPGAgent.train`` and
``customeval.py`` run unchanged with ``marl-responsible-nav_amd`` first on ``sys.path``.
Each call runs one env (E = 1) through libgridenv's kernels on the current HIP device; use
``marlnav.VecGridEnv`` for batched throughput.

Differences, all deliberate and documented in DESIGN.md:
* RNG: spawns and the scripted policy use a counter-based Philox stream keyed by ``seed``
  instead of numpy's PCG64 / global MT19937 / unseeded ``random`` (ma_customenv.py:97,441,
  custom_agent.py:31).  The step semantics given the same draws are bit-exact (tests/).
* ``render()`` is out of scope (pygame UI).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from marlnav.scenario import CompiledScenario, builtin
from marlnav.vec_env import VecGridEnv

N_DISCRETE_ACTIONS = 9

try:  # gymnasium is not a dependency; mirror its two space types when absent
    from gymnasium.spaces import Box, Discrete  # type: ignore
except Exception:  # pragma: no cover - exercised when gymnasium is missing
    class Discrete:
        def __init__(self, n):
            self.n = int(n)

        def __repr__(self):
            return f"Discrete({self.n})"

    class Box:
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

        def __repr__(self):
            return f"Box({self.low}, {self.high}, {self.shape}, {self.dtype})"


class CustomMAEnv:
    metadata = {"name": "custom_ma_env_hip"}

    def __init__(self, render=False, fear=True, seed=None, scenario: str | CompiledScenario = "level3",
                 device=None, feal=False, fear_full=False):
        """feal (not in the reference's signature; needs fear=True): step()'s info dict also carries
        info["feal"], Responsibility.FeAL of the step for every world agent (a length-N list).
        fear_full (likewise): info["fear_matrix"], Responsibility.FeAR of the step with every world agent
        as actor and every agent listed (an N x N list of lists: actor i -> agent j)."""
        if render:
            raise NotImplementedError("render() is out of scope of the HIP build (pygame UI)")
        sc = builtin(scenario) if isinstance(scenario, str) else scenario
        self.scenario = sc
        if seed is None:  # the reference seeds default_rng(None) from OS entropy
            seed = int.from_bytes(os.urandom(8), "little")
        self.seed = int(seed)
        self.possible_agents = [f"agent_{r}" for r in range(sc.K)]           # :88
        self.agents = self.possible_agents[:]                                  # :89
        self.action_space = Discrete(N_DISCRETE_ACTIONS)                       # :90 (instance attr)
        self._observation_spaces = {a: Box(low=-1.0, high=16.0, shape=(sc.H, sc.W), dtype=np.float64)
                                    for a in self.possible_agents}
        self.rendering = False
        self.fear = fear
        if feal and not fear:
            raise ValueError("CustomMAEnv(feal=True) needs fear=True (FeAL is computed from the FeAR step's record)")
        self.feal = bool(feal)
        if fear_full and not fear:
            raise ValueError("CustomMAEnv(fear_full=True) needs fear=True (the matrix is computed from the FeAR "
                             "step's record)")
        self.fear_full = bool(fear_full)
        self._env = VecGridEnv(sc, num_envs=1, fear=fear, fear_weight=0.0, max_steps=0, auto_reset=False,
                               seed=self.seed, device=device, debug=True, feal=self.feal,
                               fear_full=self.fear_full)
        self._initialized = False
        self.Action4Agents = []
        self.MdR4Agents = []
        self.num_moves = 0

    # PettingZoo ParallelEnv surface -------------------------------------------------------
    @property
    def num_agents(self):
        return len(self.agents)

    @property
    def max_num_agents(self):
        return len(self.possible_agents)

    def observation_space(self, agent):                                        # :115-116
        return self._observation_spaces[agent]

    def render(self):
        raise NotImplementedError("render() is out of scope of the HIP build (pygame UI)")

    def close(self):                                                           # :161-167
        pass

    @property
    def AgentLocations(self):
        """World.AgentLocations as (row, col) tuples."""
        pos = self._env.positions()[0].cpu().numpy()
        return [self.scenario.rc(c) for c in pos]

    def _masks(self, mask_row):
        out = {}
        for k, a in enumerate(self.agents):
            m = int(mask_row[k]) & 0x1FF
            out[a] = {"action_mask": np.array([(m >> b) & 1 for b in range(9)], dtype=np.int8)}
        return out

    def _obs_dict(self, obs):
        o = obs[:, 0].cpu().numpy().astype(np.float64)
        return {a: o[k] for k, a in enumerate(self.agents)}

    def reset(self, seed=None, options=None):                                  # :169-215
        obs, mask = self._env.reset()
        torch.cuda.synchronize(self._env.device)
        self._initialized = True
        self.agents = self.possible_agents[:]
        self.rewards = {a: 0 for a in self.agents}
        self._cumulative_rewards = {a: 0 for a in self.agents}
        self.terminations = {a: False for a in self.agents}
        self.truncation = {a: False for a in self.agents}
        self.num_moves = 0
        self.observations = self._obs_dict(obs)
        info = {"fear": 0.0}
        info.update(self._masks(mask[0].cpu().numpy()))
        return self.observations, info

    def step(self, actions):                                                   # :217-334
        if not actions:
            return {}, {}, {}, {}, {}
        if not self._initialized:
            raise RuntimeError("step() before reset()")
        acts = [int(a) for a in actions]
        if len(acts) != self.scenario.K or any(not 0 <= a < N_DISCRETE_ACTIONS for a in acts):
            raise ValueError(f"need {self.scenario.K} actions in 0..8, got {actions!r}")
        r = self._env.step(torch.tensor([acts], dtype=torch.int32))
        torch.cuda.synchronize(self._env.device)
        self.num_moves += 1
        act = r.actions[0].cpu().tolist()
        mdr = r.mdr[0].cpu().tolist()
        self.Action4Agents = [(i, a) for i, a in enumerate(act)]
        self.MdR4Agents = [[i, m] for i, m in enumerate(mdr)]
        reward = r.reward[0].cpu().numpy()
        fear = r.fear[0].cpu().numpy()
        term = r.term[0].cpu().numpy()
        trunc = r.trunc[0].cpu().numpy()
        self.rewards = {a: int(reward[k]) for k, a in enumerate(self.agents)}
        self.terminations = {a: bool(term[k]) for k, a in enumerate(self.agents)}
        self.truncation = {a: bool(trunc[k]) for k, a in enumerate(self.agents)}
        self.observations = self._obs_dict(r.obs)
        info = {"fear": {a: np.float64(fear[k]) for k, a in enumerate(self.agents)},
                "agent_crashes": int(r.crashes[0].item()),
                "apples_caught": int(r.apples[0].item())}
        if self.feal:
            info["feal"] = r.feal[0].cpu().tolist()
        if self.fear_full:
            info["fear_matrix"] = r.resp_full[0].cpu().tolist()
        info.update(self._masks(r.mask[0].cpu().numpy()))
        return self.observations, self.rewards, self.terminations, self.truncation, info


def manhattan_dist(loc_1, loc_2):                                              # :511-512
    return sum(abs(a - b) for a, b in zip(loc_1, loc_2))
