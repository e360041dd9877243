"""Test doubles that speak the REFERENCE's env protocol (an SB3 vec env:
``reset() -> np [N, D]``, ``step(np actions) -> (obs, reward, done, infos)``
with ``infos`` a list of one dict of numpy values per env --
mprl/rl/sampler/temporal_correlated_sampler.py:226-303,
mprl/rl/sampler/black_box_sampler.py:200-230,
mprl/util/util_mp.py:144-185), for tests/test_vec_adapter_*.py.

* ``OracleVecEnv``: pure numpy / CPU; the episode physics are the CPU
  restatement oracle/env_oracle.py (test infrastructure), one dict per env;
* ``ReplayVecEnv``: replays a GPU ``Synthetic*Env`` through the protocol
  (device -> per-env numpy dicts), so that the adapter path can be compared BIT
  FOR BIT with the direct path on the same physics;
* ``ScriptedVecEnv`` + ``StubPolicy`` / ``StubCritic``: closed-form float64
  content in which every reset, episode, env and step is distinguishable, for
  the multi-episode fixture (tests/golden/make_multi_episode.py,
  tests/test_multi_episode_gpu.py).
"""
import types

import numpy as np
import torch

from oracle import env_oracle as E


class _Space:
    def __init__(self, shape):
        self.shape = tuple(shape)


class _Spec:
    def __init__(self, T):
        self.max_episode_steps = T


def _metric_sequence(value, T):
    """A task metric as the reference's envs log it: one value per step, the
    LAST is what the sampler keeps."""
    seq = np.zeros(T, dtype=np.float64)
    seq[-1] = value
    return seq


class OracleVecEnv:
    """N point-mass envs of one family, stepped on the host (float64 numpy in,
    as MuJoCo hands out)."""

    def __init__(self, task, num_envs, dof, d_task, T, dt, seed=0):
        self.task, self.num_envs, self.dof = task, num_envs, dof
        self.d_task, self.T, self.dt = d_task, T, dt
        self.rng = np.random.default_rng(seed)
        D = d_task + 1 + 2 * dof
        self.observation_space = _Space((D,))
        self.action_space = _Space((2 * dof,))
        self._inner = types.SimpleNamespace(dt=dt, spec=_Spec(T))
        self.envs = [self._inner]
        self._obs0 = None

    def reset(self):
        N, dof = self.num_envs, self.dof
        goal = torch.from_numpy(self.rng.uniform(-1, 1, (N, dof)))
        pos = torch.from_numpy(0.1 * self.rng.uniform(-1, 1, (N, dof)))
        self._obs0 = E.reset_obs(self.task, self.d_task, goal, pos,
                                 torch.zeros_like(pos))
        return self._obs0.numpy().copy()

    def step(self, actions):
        assert isinstance(actions, np.ndarray) and \
            actions.shape == (self.num_envs, self.T, 2 * self.dof)
        a = torch.from_numpy(np.asarray(actions, dtype=np.float64))
        states, rewards, flags, metrics = E.rollout(
            self.task, a, self._obs0, self.dof, self.d_task, self.dt)
        T = self.T
        term = np.zeros(T, dtype=bool)
        trunc = np.zeros(T, dtype=bool)
        trunc[-1] = True
        infos = []
        for n in range(self.num_envs):
            d = {"step_states": states[n, 1:].numpy().copy(),
                 "step_rewards": rewards[n].numpy().copy(),
                 "step_terminations": term.copy(),
                 "step_truncations": trunc.copy(),
                 "segment_length": T,
                 "success": _metric_sequence(float(metrics[n, 0]), T),
                 "final_distance": _metric_sequence(float(metrics[n, 1]), T),
                 "not_for_the_sampler": "text"}
            if self.task in ("table_tennis", "hopper"):
                d["hit_ball"] = flags[n].numpy().copy()
                d["has_left_floor"] = flags[n].numpy().copy()
            infos.append(d)
        reward = rewards.sum(-1).numpy()
        done = np.ones(self.num_envs, dtype=bool)
        return self.reset(), reward, done, infos

    def env_method(self, name, *a, **k):
        return [None] * self.num_envs

    def get_attr(self, name):
        return [getattr(self._inner, name)] * self.num_envs

    def close(self):
        pass


class ReplayVecEnv:
    """A GPU synthetic env behind the reference protocol (numpy out, list of
    dicts); ``black_box``: the ``trajectory_length`` protocol."""

    def __init__(self, synthetic, black_box=False):
        self.syn, self.black_box = synthetic, black_box
        self.num_envs = synthetic.num_env
        self.observation_space = synthetic.observation_space
        self.action_space = synthetic.action_space
        self.envs = [types.SimpleNamespace(dt=synthetic.dt,
                                           spec=synthetic.spec)]
        self.steps_seen = 0

    def reset(self):
        return self.syn.reset().cpu().numpy()

    def step(self, actions):
        assert isinstance(actions, np.ndarray)
        self.steps_seen += 1
        a = torch.from_numpy(actions).to(self.syn.device)
        nxt, rew, done, inf = self.syn.step(a)
        host = {k: v.cpu().numpy() for k, v in inf.items()
                if torch.is_tensor(v) and k not in ("step_states_full",
                                                    "obs_moment_partials")}
        T = self.syn.num_times
        infos = []
        for n in range(self.num_envs):
            d = {}
            for k, v in host.items():
                if k in ("success", "final_distance"):
                    d[k] = _metric_sequence(v[n], T).astype(v.dtype)
                elif k in ("segment_length", "trajectory_length"):
                    d[k] = int(v[n])
                else:
                    d[k] = v[n]
            infos.append(d)
        return nxt.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), infos

    def env_method(self, name, *a, **k):
        return [None] * self.num_envs

    def get_attr(self, name):
        return [getattr(self.envs[0], name)] * self.num_envs

    def close(self):
        pass


# ---------------------------------------------------------------------------
# Scripted env + closed-form stub policy / critic: every reset, episode, env
# and step is distinguishable, nothing is random.  Shared by the generator
# tests/golden/make_multi_episode.py (which drives the REFERENCE's samplers
# with them) and tests/test_multi_episode_gpu.py (this repository's samplers),
# so both sides see the same objects.
# ---------------------------------------------------------------------------
def _event_step(n, e, T):
    """Step at which env n's event fires in episode e: a different one per
    env and episode, step 0 and "never" (T) among them."""
    return (0, T, 2, T - 1, 4)[(n + 2 * e) % 5]


class ScriptedVecEnv:
    """The reference protocol with closed-form float64 content.

    * ``reset()`` number r hands out ``obs[n, j] = sin(0.7 r + 1.3 n + 0.37 j)
      + 0.1 r`` (the time column: ``0.05 r + 0.01 n``), and every ``step``
      ends with such a reset, as an SB3 vec env's does;
    * episode e's step states / rewards are functions of the actions, of e and
      of the observation the episode started from; ``segment_length`` /
      ``trajectory_length`` vary with n and e, a termination sits at the last
      valid step; ``hit_ball`` / ``has_left_floor`` fire at ``_event_step``;
    * the task metrics are per-step sequences whose last element differs from
      the others.
    ``black_box``: actions are [N, K] parameter vectors, the observation has no
    [time | pos | vel] tail."""

    METRICS = ("success", "final_distance")

    def __init__(self, num_envs, dof, d_task, T, dt, black_box=False):
        self.num_envs, self.dof, self.d_task = num_envs, dof, d_task
        self.T, self.dt, self.black_box = T, dt, black_box
        self.D = d_task if black_box else d_task + 1 + 2 * dof
        self.observation_space = _Space((self.D,))
        self.action_space = _Space((2 * dof,))
        self._inner = types.SimpleNamespace(dt=dt, spec=_Spec(T))
        self.envs = [self._inner]
        self.resets = self.episodes = 0
        self._obs0 = None

    def reset(self):
        r = self.resets
        self.resets += 1
        n = np.arange(self.num_envs, dtype=np.float64)[:, None]
        j = np.arange(self.D, dtype=np.float64)[None, :]
        obs = np.sin(0.7 * r + 1.3 * n + 0.37 * j) + 0.1 * r
        if not self.black_box:
            obs[:, self.d_task] = 0.05 * r + 0.01 * n[:, 0]
        self._obs0 = obs
        return obs.copy()

    def step(self, actions):
        assert isinstance(actions, np.ndarray) and \
            actions.dtype == np.float64 and actions.shape[0] == self.num_envs
        e = self.episodes
        self.episodes += 1
        N, T = self.num_envs, self.T
        n = np.arange(N)
        t = np.arange(T)
        length = T - (n + 2 * e) % 3
        infos = []
        if self.black_box:
            reward = -0.1 * np.square(actions).sum(-1) + e \
                + 0.3 * self._obs0[:, 0]
        else:
            assert actions.shape == (N, T, 2 * self.dof)
            j = np.arange(self.D)
            states = np.cos(0.3 * j + 0.11 * e) * actions[..., j % (2 * self.dof)] \
                + 0.01 * t[None, :, None] + 0.5 * e \
                + 0.1 * self._obs0[:, None, :]
            rewards = -0.01 * np.square(actions).sum(-1) + 0.1 * e \
                + 0.001 * t[None] * (n[:, None] + 1) + 0.2 * self._obs0[:, :1]
            reward = rewards.sum(-1) + 0.5
        for i in range(N):
            d = {key: 0.25 * t + i + 10 * e + 100 * k
                 for k, key in enumerate(self.METRICS)}
            d["not_for_the_sampler"] = "text"
            if self.black_box:
                d["trajectory_length"] = int(length[i])
            else:
                d["step_states"] = states[i].copy()
                d["step_rewards"] = rewards[i].copy()
                d["step_terminations"] = (t == length[i] - 1) & (length[i] < T)
                d["step_truncations"] = t == T - 1
                d["segment_length"] = int(length[i])
                event = t >= _event_step(i, e, T)
                d["hit_ball"], d["has_left_floor"] = event, event.copy()
            infos.append(d)
        done = np.ones(N, dtype=bool)
        return self.reset(), reward, done, infos

    def env_method(self, name, *a, **k):
        return [None] * self.num_envs

    def get_attr(self, name):
        return [getattr(self._inner, name)] * self.num_envs

    def close(self):
        pass


def _table(rows, cols, phase, like):
    """A fixed [rows, cols] matrix of the dtype / device of `like`."""
    i = torch.arange(rows, dtype=like.dtype, device=like.device)[:, None]
    j = torch.arange(cols, dtype=like.dtype, device=like.device)[None, :]
    return torch.sin(phase + 0.9 * i + 0.53 * j) / (rows ** 0.5)


class StubPolicy:
    """A policy that is a closed-form function of its inputs (torch ops only,
    any device).  The "noise" of ``sample`` is a function of the call count,
    so every episode gets its own.  ``contextual``: the Cholesky factor depends
    on the observation; otherwise one matrix for all rows, handed out through
    ``expand(base [K, K], N)`` (default: a plain stride-0 expand)."""

    def __init__(self, num_dof, num_basis, contextual=False, expand=None):
        self.num_dof, self.num_basis = num_dof, num_basis
        self.dim_out = num_dof * num_basis
        self.contextual = contextual
        self.expand = expand or (lambda base, N: base.expand(N, -1, -1))
        self.calls = 0

    def policy(self, obs):
        K = self.dim_out
        mean = torch.tanh(obs @ _table(obs.shape[-1], K, 0.2, obs))
        base = torch.tril(_table(K, K, 1.1, obs)) * 0.3 + \
            torch.eye(K, dtype=obs.dtype, device=obs.device)
        if self.contextual:
            L = base[None] * (1 + 0.1 * torch.tanh(obs[:, :1, None]))
        else:
            L = self.expand(base, obs.shape[0])
        return mean, L

    def sample(self, require_grad, params_mean, params_L, times=None,
               init_time=None, init_pos=None, init_vel=None, use_mean=False):
        K = self.dim_out
        self.calls += 1
        noise = torch.sin(0.9 * torch.arange(
            K, dtype=params_mean.dtype, device=params_mean.device)
            + 1.7 * self.calls)
        params = params_mean if use_mean else \
            params_mean + torch.einsum("nij,j->ni", params_L, noise)
        if times is None:                           # black box: the parameters
            return params
        w = params.reshape(-1, self.num_dof, self.num_basis)
        k = torch.arange(1, self.num_basis + 1, dtype=times.dtype,
                         device=times.device)
        phase = times[..., None] * k                # [N, T, nb]
        pos = init_pos[:, None] + torch.einsum("ndk,ntk->ntd", w,
                                               torch.sin(phase))
        vel = init_vel[:, None] + torch.einsum("ndk,ntk->ntd", w,
                                               torch.cos(phase)) \
            + 0.1 * init_time[:, None, None]
        return torch.cat([pos, vel], -1)

    def log_prob(self, actions, params_mean, params_L, times=None,
                 init_time=None, init_pos=None, init_vel=None,
                 pred_pairs=None):
        logdet = torch.diagonal(params_L, dim1=-2, dim2=-1).abs().log().sum(-1)
        if pred_pairs is None:                      # black box: [N]
            return -0.5 * torch.square(actions - params_mean).sum(-1) - logdet
        a, b = actions[:, pred_pairs[:, 0]], actions[:, pred_pairs[:, 1]]
        return -0.01 * torch.square(a - 0.5 * b).sum(-1) - logdet[:, None] \
            + 0.01 * (times[:, pred_pairs[:, 1]] - init_time[:, None]) \
            + 0.1 * init_pos.sum(-1, keepdim=True) \
            - 0.2 * init_vel.sum(-1, keepdim=True)


class StubCritic:
    """V(x) = tanh(x . w) with a fixed w (torch ops only, any device)."""

    def critic(self, x):
        return torch.tanh(x @ _table(x.shape[-1], 1, 0.4, x))


# The multi-episode cases of tests/golden/multi_episode.npz: sampler kind, env
# id (the id alone selects the MDP-reward re-shaping), sizes, episodes per env,
# observation normalisation, covariance head of the stub policy, pair
# selection and the runs made one after the other on ONE sampler
# ("train" / "eval": an evaluation run is deterministic).
MULTI_EPISODE_CASES = {
    "tc_norm_table_tennis": dict(
        kind="tc", env_id="TableTennis4D-v0", N=4, N_test=3, T=7, dof=2,
        nb=2, d_task=3, E=3, E_test=2, norm=True, contextual=True,
        pairs=dict(num_select=3, fixed_interval=True),
        runs=("train", "train", "eval")),
    "tc_norm_hopper": dict(
        kind="tc", env_id="HopperJumpSparse-v0", N=5, N_test=2, T=6, dof=2,
        nb=2, d_task=3, E=3, E_test=1, norm=True, contextual=False,
        pairs=dict(num_select=4, fixed_interval=False), runs=("train",)),
    "tc_raw_plain": dict(
        kind="tc", env_id="BoxPushingDense-v0", N=3, N_test=2, T=7, dof=3,
        nb=2, d_task=4, E=3, E_test=2, norm=False, contextual=False,
        pairs=dict(num_select=3, fixed_interval=True), runs=("train",)),
    "bb_train": dict(
        kind="bb", env_id="BoxPushingDense-v0", N=4, N_test=2, T=9, dof=2,
        nb=3, d_task=7, E=3, E_test=2, norm=False, contextual=False,
        pairs=None, runs=("train",)),
}


def scripted_env_fn(case):
    """``vec_env_fn`` of a case: one fresh ScriptedVecEnv per call."""
    c = MULTI_EPISODE_CASES[case]

    def fn(env_id, num_env, seed, render, mp_args, **kwargs):
        return ScriptedVecEnv(num_env, c["dof"], c["d_task"], c["T"], 0.02,
                              black_box=c["kind"] == "bb")
    return fn


def sampler_kwargs(case, device):
    """Constructor arguments both the reference's samplers and this
    repository's take."""
    c = MULTI_EPISODE_CASES[case]
    kw = dict(env_id=c["env_id"], num_env_train=c["N"],
              num_env_test=c["N_test"], episodes_per_train_env=c["E"],
              episodes_per_test_env=c["E_test"], dtype="torch.float64",
              device=device, seed=0,
              task_specified_metrics=list(ScriptedVecEnv.METRICS))
    if c["kind"] == "tc":
        kw.update(norm_step_obs=c["norm"], time_pairs_config=dict(c["pairs"]))
    return kw


def run_case(case, sampler, expand=None):
    """The runs of a case on `sampler`; per run the result dict, the step
    count, the pairs, the observation statistics and one draw from torch's
    global generator taken right after (pins its position)."""
    c = MULTI_EPISODE_CASES[case]
    policy = StubPolicy(c["dof"], c["nb"], c["contextual"], expand)
    critic = StubCritic()
    torch.manual_seed(1234)
    out = []
    for kind in c["runs"]:
        res, steps = sampler.run(training=kind == "train", policy=policy,
                                 critic=critic, deterministic=kind == "eval")
        rec = dict(res)
        rec["num_steps"] = torch.as_tensor(int(steps))
        rec["generator_next"] = torch.randint(0, 1 << 30, size=[])
        if c["kind"] == "tc":
            # (copies: a sampler may update its statistics in place)
            rec["pred_pairs"] = sampler.pred_pairs.clone()
            if sampler.obs_rms is not None:
                rec["obs_rms_mean"] = sampler.obs_rms.mean.clone()
                rec["obs_rms_var"] = sampler.obs_rms.var.clone()
                rec["obs_rms_count"] = torch.as_tensor(
                    float(sampler.obs_rms.count), dtype=torch.float64)
        out.append(rec)
    return out
